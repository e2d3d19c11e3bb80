"""Floating-rate notes (cavour/trades/credit/frn.py:56-560).

Construction, schedule and the host measures follow the reference method by method.  The curve Greeks
(VALUE / DELTA / GAMMA) go through the valuation engine (`Engine._compute_frn`: a float leg plus fixed flows on the
GPU); the discount margins, prices, durations and dv01s of many FRNs at once go through `FRNBook.measures`
(market/position/frn_book.py, the adr_frn_measures kernels).  The scalar methods here are the specification both are
tested against.

Reference quirks kept on purpose (each is named again where it happens):

* times: `value` reads both curves' own nodes through ``DiscountCurve.df(dt, self._dc_type)`` - year fractions in
  the FRN's day count from each curve's value date, not ACT/ACT as for bonds;
* forward: ``(D_idx(start) / D_idx(end) - 1)`` divided by the INDEX curve's ``_dc_type`` year fraction of the
  period; the coupon then multiplies the rate by the FRN's own year fraction;
* first fixing: `value` applies ``first_fixing_rate`` to the first coupon paid after settlement; the engine applies
  it to coupon 0 of the whole schedule (for a seasoned FRN that coupon is in the past and masked, so there the
  override has no effect);
* cap and floor: applied in `value` and `accrued_interest`; the engine ignores them;
* accrued interest: at ``first_fixing_rate + margin``, or at the margin alone without a first fixing;
* discount margin: discounts by ``exp(-dm * yf(settlement, payment))`` in the FRN's day count on top of
  ``D(payment) / D(settlement)``; the principal sits at the adjusted maturity date (not the lagged last payment);
* solver: `brentq` on [-0.10, 0.20] with ``xtol=1e-8``; failing that scipy's `newton` from ``dm_guess``
  (``tol=1e-8``, ``maxiter=50``); failing both, `LibError`;
* `modified_duration` is the central +-1bp DM difference of dirty prices over the base price; `dv01` is
  ``|PV(dm + 1bp) - PV(dm)|``;
* a seasoned FRN without a first fixing raises in `value` (``index_curve.df(start)`` sees a negative time,
  ``interpolator.interpolate``); the engine prices it, because its interpolation extrapolates flat.
"""
from __future__ import annotations

import numpy as np
from scipy.optimize import brentq, newton

from ...utils.calendar import BusDayAdjustTypes, Calendar, CalendarTypes, DateGenRuleTypes
from ...utils.currency import CurrencyTypes
from ...utils.date import Date
from ...utils.day_count import DayCount, DayCountTypes
from ...utils.error import LibError
from ...utils.frequency import FrequencyTypes
from ...utils.global_types import CurveTypes, InstrumentTypes
from ...utils.helpers import check_argument_types, label_to_string
from ...utils.schedule import Schedule

DM_BRACKET = (-0.10, 0.20)
DM_XTOL = 1e-8
NEWTON_TOL, NEWTON_MAXITER = 1e-8, 50
BUMP = 0.0001


class FRN:
    def __init__(self,
                 issue_dt: Date,
                 maturity_dt_or_tenor: (Date, str),
                 quoted_margin: float,
                 freq_type: FrequencyTypes,
                 dc_type: DayCountTypes,
                 currency: CurrencyTypes,
                 floating_index: CurveTypes,
                 face_value: float = 100.0,
                 payment_lag: int = 0,
                 cap_rate: (float, type(None)) = None,
                 floor_rate: (float, type(None)) = None,
                 first_fixing_rate: (float, type(None)) = None,
                 cal_type: CalendarTypes = CalendarTypes.WEEKEND,
                 bd_type: BusDayAdjustTypes = BusDayAdjustTypes.FOLLOWING,
                 dg_type: DateGenRuleTypes = DateGenRuleTypes.BACKWARD,
                 end_of_month: bool = False):
        """FRN paying the ``floating_index`` forward plus ``quoted_margin`` (decimal) on the face (frn.py:81-175).
        The maturity is business-day adjusted; ``first_fixing_rate`` is the known fixing of a seasoned note."""
        check_argument_types(self.__init__, locals())
        self._issue_dt = issue_dt
        self._quoted_margin = quoted_margin
        self._freq_type = freq_type
        self._dc_type = dc_type
        self._currency = currency
        self._floating_index = floating_index
        self._face_value = face_value
        self._payment_lag = payment_lag
        self._cap_rate = cap_rate
        self._floor_rate = floor_rate
        self._first_fixing_rate = first_fixing_rate
        self._cal_type = cal_type
        self._bd_type = bd_type
        self._dg_type = dg_type
        self._end_of_month = end_of_month
        maturity = (maturity_dt_or_tenor if isinstance(maturity_dt_or_tenor, Date)
                    else issue_dt.add_tenor(maturity_dt_or_tenor))
        self._maturity_dt = Calendar(cal_type).adjust(maturity, bd_type)
        if issue_dt >= self._maturity_dt:
            raise LibError("Issue date must be before maturity date")
        # filled by `value`
        self._rates, self._coupon_payments, self._payment_dfs, self._payment_pvs = [], [], [], []
        self.derivative_type = InstrumentTypes.FRN
        self._generate_payment_schedule()

    def _generate_payment_schedule(self):
        """Accrual periods of the adjusted schedule; payments ``payment_lag`` business days after the accrual end;
        year fractions in the FRN's day count (frn.py:179-231)."""
        dts = Schedule(effective_dt=self._issue_dt, termination_dt=self._maturity_dt, freq_type=self._freq_type,
                       cal_type=self._cal_type, bd_type=self._bd_type, dg_type=self._dg_type,
                       end_of_month=self._end_of_month)._adjusted_dts
        if len(dts) < 2:
            raise LibError("Schedule must have at least two dates")
        counter = DayCount(self._dc_type)
        calendar = Calendar(self._cal_type)
        self._payment_dts, self._start_accrued_dts, self._end_accrued_dts = [], [], []
        self._year_fracs, self._accrued_days = [], []
        prev = dts[0]
        for nxt in dts[1:]:
            self._start_accrued_dts.append(prev)
            self._end_accrued_dts.append(nxt)
            self._payment_dts.append(nxt if self._payment_lag == 0 else calendar.add_business_days(nxt, self._payment_lag))
            frac, days, _ = counter.year_frac(prev, nxt)
            self._year_fracs.append(frac)
            self._accrued_days.append(days)
            prev = nxt

    def position(self, model):
        from ...market.position.position import Position
        return Position(self, model)

    # ------------------------------------------------------------------------------------------ prices
    def _coupon_rate(self, rate):
        """The margin, then the cap, then the floor."""
        rate = rate + self._quoted_margin
        if self._cap_rate is not None:
            rate = min(rate, self._cap_rate)
        if self._floor_rate is not None:
            rate = max(rate, self._floor_rate)
        return rate

    def value(self, value_dt: Date, discount_curve, index_curve=None, discount_margin: float = 0.0,
              settlement_dt: Date = None):
        """PV of the coupons paid after settlement and of the face at the adjusted maturity, discounted relative to
        ``df(settlement)`` with the discount margin over the FRN's year fraction from settlement (frn.py:235-361)."""
        if discount_curve is None:
            raise LibError("Discount curve is required")
        if index_curve is None:
            index_curve = discount_curve
        if settlement_dt is None:
            settlement_dt = value_dt
        self._rates, self._coupon_payments, self._payment_dfs, self._payment_pvs = [], [], [], []
        df_settle = discount_curve.df(settlement_dt, self._dc_type)
        counter = DayCount(self._dc_type)
        index_counter = DayCount(index_curve._dc_type)
        first_payment = True
        pv = 0.0
        for i, pay_dt in enumerate(self._payment_dts):
            if pay_dt > settlement_dt:
                start, end = self._start_accrued_dts[i], self._end_accrued_dts[i]
                if first_payment and self._first_fixing_rate is not None:
                    # the known fixing replaces the forward of the first coupon paid after settlement
                    fwd = self._first_fixing_rate
                    first_payment = False
                else:
                    index_frac = index_counter.year_frac(start, end)[0]
                    # raises for a start before the index curve's value date (a seasoned FRN without a fixing)
                    df_start = index_curve.df(start, self._dc_type)
                    df_end = index_curve.df(end, self._dc_type)
                    fwd = (df_start / df_end - 1.0) / index_frac
                rate = self._coupon_rate(fwd)
                coupon = rate * self._year_fracs[i] * self._face_value
                dm_frac = counter.year_frac(settlement_dt, pay_dt)[0]
                df_pay = discount_curve.df(pay_dt, self._dc_type) / df_settle
                if discount_margin != 0.0:
                    df_pay *= np.exp(-discount_margin * dm_frac)
                payment_pv = coupon * df_pay
                pv += payment_pv
                self._rates.append(rate)
                self._coupon_payments.append(coupon)
                self._payment_dfs.append(df_pay)
                self._payment_pvs.append(payment_pv)
            else:
                self._rates.append(0.0)
                self._coupon_payments.append(0.0)
                self._payment_dfs.append(0.0)
                self._payment_pvs.append(0.0)
        if self._maturity_dt > settlement_dt:
            # the face at the ADJUSTED maturity date, not at the (lagged) last payment date
            dm_frac = counter.year_frac(settlement_dt, self._maturity_dt)[0]
            df_mat = discount_curve.df(self._maturity_dt, self._dc_type) / df_settle
            if discount_margin != 0.0:
                df_mat *= np.exp(-discount_margin * dm_frac)
            principal_pv = self._face_value * df_mat
            pv += principal_pv
            if self._payment_pvs:
                self._payment_pvs[-1] += principal_pv
        return pv

    def dirty_price(self, value_dt: Date, discount_curve, index_curve=None, discount_margin: float = 0.0,
                    settlement_dt: Date = None):
        """Per 100 face (frn.py:365-390)."""
        pv = self.value(value_dt, discount_curve, index_curve, discount_margin, settlement_dt)
        return 100.0 * pv / self._face_value

    def accrued_interest(self, settlement_dt: Date):
        """Per 100 face: the period of the first coupon paid after settlement, from its start to settlement, at
        ``first_fixing_rate + margin`` (the margin alone without a fixing), capped and floored (frn.py:394-446)."""
        counter = DayCount(self._dc_type)
        for i, pay_dt in enumerate(self._payment_dts):
            if pay_dt > settlement_dt:
                start = self._start_accrued_dts[i]
                if settlement_dt >= start:
                    frac = counter.year_frac(start, settlement_dt)[0]
                    rate = (self._first_fixing_rate + self._quoted_margin if self._first_fixing_rate is not None
                            else self._quoted_margin)
                    if self._cap_rate is not None:
                        rate = min(rate, self._cap_rate)
                    if self._floor_rate is not None:
                        rate = max(rate, self._floor_rate)
                    accrued = rate * frac * self._face_value
                    return 100.0 * accrued / self._face_value
        return 0.0

    def clean_price(self, value_dt: Date, discount_curve, index_curve=None, discount_margin: float = 0.0,
                    settlement_dt: Date = None):
        """Dirty price minus accrued interest, per 100 face (frn.py:450-478)."""
        if settlement_dt is None:
            settlement_dt = value_dt
        dirty = self.dirty_price(value_dt, discount_curve, index_curve, discount_margin, settlement_dt)
        return dirty - self.accrued_interest(settlement_dt)

    # ------------------------------------------------------------------------------------------ discount margin
    def discount_margin(self, settlement_dt: Date, discount_curve, index_curve, clean_price: float,
                        dm_guess: float = 0.0):
        """The DM whose dirty price equals ``clean_price`` plus accrued: brentq on the fixed bracket, scipy's newton
        (a secant without a derivative) from ``dm_guess`` when that fails, `LibError` when both fail
        (frn.py:482-527)."""
        target_dirty = clean_price + self.accrued_interest(settlement_dt)

        def price_error(dm):
            return self.dirty_price(settlement_dt, discount_curve, index_curve, dm, settlement_dt) - target_dirty
        try:
            return brentq(price_error, DM_BRACKET[0], DM_BRACKET[1], xtol=DM_XTOL)
        except Exception:
            try:
                return newton(price_error, dm_guess, tol=NEWTON_TOL, maxiter=NEWTON_MAXITER)
            except Exception:
                raise LibError(f"Failed to converge on discount margin for price {clean_price}")

    # ------------------------------------------------------------------------------------------ risk
    def modified_duration(self, value_dt: Date, discount_curve, index_curve=None, discount_margin: float = 0.0,
                          settlement_dt: Date = None):
        """-(P(dm + 1bp) - P(dm - 1bp)) / (2 bp P(dm)) on dirty prices - a shift of the DM, not of the curve
        (frn.py:531-575)."""
        if settlement_dt is None:
            settlement_dt = value_dt
        p0 = self.dirty_price(value_dt, discount_curve, index_curve, discount_margin, settlement_dt)
        p_up = self.dirty_price(value_dt, discount_curve, index_curve, discount_margin + BUMP, settlement_dt)
        p_down = self.dirty_price(value_dt, discount_curve, index_curve, discount_margin - BUMP, settlement_dt)
        return -(p_up - p_down) / (2 * BUMP * p0)

    def dv01(self, value_dt: Date, discount_curve, index_curve=None, discount_margin: float = 0.0,
             settlement_dt: Date = None):
        """|PV(dm + 1bp) - PV(dm)| in currency (frn.py:579-614)."""
        if settlement_dt is None:
            settlement_dt = value_dt
        pv = self.value(value_dt, discount_curve, index_curve, discount_margin, settlement_dt)
        pv_bumped = self.value(value_dt, discount_curve, index_curve, discount_margin + BUMP, settlement_dt)
        return abs(pv_bumped - pv)

    # ------------------------------------------------------------------------------------------ printing
    def print_payments(self):
        """The schedule without valuations (frn.py:636-668)."""
        print("=" * 80)
        print("FRN PAYMENT SCHEDULE")
        print("=" * 80)
        print(f"Issue Date:        {self._issue_dt}")
        print(f"Maturity Date:     {self._maturity_dt}")
        print(f"Quoted Margin:     {self._quoted_margin * 10000:.2f} bp")
        print(f"Frequency:         {self._freq_type}")
        print(f"Day Count:         {self._dc_type}")
        print(f"Face Value:        {self._face_value:.2f}")
        print(f"Currency:          {self._currency}")
        print(f"Floating Index:    {self._floating_index}")
        if self._cap_rate is not None:
            print(f"Cap Rate:          {self._cap_rate * 100:.4f}%")
        if self._floor_rate is not None:
            print(f"Floor Rate:        {self._floor_rate * 100:.4f}%")
        print("=" * 80)
        print(f"\n{'Num':<5} {'Pay Date':<12} {'Start':<12} {'End':<12} {'Days':<6} {'Year Frac':<10}")
        print("-" * 80)
        for i in range(len(self._payment_dts)):
            print(f"{i + 1:<5} {str(self._payment_dts[i]):<12} {str(self._start_accrued_dts[i]):<12} "
                  f"{str(self._end_accrued_dts[i]):<12} {self._accrued_days[i]:<6} {self._year_fracs[i]:<10.6f}")

    def print_valuation(self):
        """The last valuation, coupon by coupon (frn.py:672-703)."""
        if not self._rates:
            print("No valuation available. Call value() first.")
            return
        print("=" * 80)
        print("FRN VALUATION")
        print("=" * 80)
        print(f"\n{'Num':<5} {'Pay Date':<12} {'Rate %':<10} {'Payment':<15} {'DF':<10} {'PV':<15}")
        print("-" * 80)
        for i in range(len(self._payment_dts)):
            print(f"{i + 1:<5} {str(self._payment_dts[i]):<12} {self._rates[i] * 100:<10.4f} "
                  f"{self._coupon_payments[i]:<15.2f} {self._payment_dfs[i]:<10.6f} {self._payment_pvs[i]:<15.2f}")
        print("-" * 80)
        print(f"{'Total PV:':<50} {sum(self._payment_pvs):<15.2f}")
        print("=" * 80)

    def __repr__(self):
        s = label_to_string("OBJECT TYPE", type(self).__name__)
        s += label_to_string("ISSUE DATE", self._issue_dt)
        s += label_to_string("MATURITY DATE", self._maturity_dt)
        s += label_to_string("QUOTED MARGIN (BP)", self._quoted_margin * 10000)
        s += label_to_string("FREQUENCY", self._freq_type)
        s += label_to_string("DAY COUNT", self._dc_type)
        s += label_to_string("CURRENCY", self._currency)
        s += label_to_string("FLOATING INDEX", self._floating_index)
        s += label_to_string("FACE VALUE", self._face_value)
        if self._cap_rate is not None:
            s += label_to_string("CAP RATE (%)", self._cap_rate * 100)
        if self._floor_rate is not None:
            s += label_to_string("FLOOR RATE (%)", self._floor_rate * 100)
        return s
