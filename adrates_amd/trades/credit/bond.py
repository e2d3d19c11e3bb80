"""Fixed-coupon, zero-coupon and amortizing bonds (cavour/trades/credit/bond.py:60-1118).

Construction, schedule and the host measures follow the reference method by method.  The curve Greeks
(VALUE / DELTA / GAMMA) go through the valuation engine (`Engine._compute_bond`, a fixed-flows-only batch on
the GPU); the spread and yield measures of many bonds at once go through `BondBook.measures`
(market/position/bond_book.py, the adr_bond_measures kernels).  The scalar methods here are the specification
both are tested against.

Reference quirks kept on purpose (each is named again where it happens):

* spread and yield times are calendar days over 365.25 from SETTLEMENT; curve times are ACT/ACT ISDA from the
  curve's value date (`DiscountCurve.df`);
* `value` discounts relative to ``df(settlement)`` and always takes its amortizing branch, because
  ``_principal_payments`` exists for every bond;
* `yield_to_maturity`, `duration` and `convexity` price the coupons plus the FULL face at the UNADJUSTED
  maturity date, so they ignore amortization;
* ``duration(..., 'modified')`` returns the Macaulay number;
* `dv01` and `cs01` are the same central difference in the z-spread;
* the solvers try `brentq` on a fixed bracket and fall back to scipy's `newton` from a fixed start.
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
from ...utils.global_types import InstrumentTypes
from ...utils.helpers import check_argument_types, label_to_string
from ...utils.schedule import Schedule

SPREAD_DAYS_IN_YEAR = 365.25     # bond.py: (payment_dt - settlement_dt) / 365.25 for every spread and yield time
Z_BRACKET, Z_START = (-0.1, 0.5), 0.01
YTM_BRACKET, YTM_START = (-0.5, 0.5), 0.05
BUMP = 0.0001


class Bond:
    def __init__(self,
                 issue_dt: Date,
                 maturity_dt_or_tenor: (Date, str),
                 coupon: float,
                 freq_type: FrequencyTypes,
                 dc_type: DayCountTypes,
                 currency: CurrencyTypes,
                 face_value: float = 100.0,
                 payment_lag: int = 0,
                 amortization_schedule: (list, type(None)) = None,
                 cal_type: CalendarTypes = CalendarTypes.WEEKEND,
                 bd_type: BusDayAdjustTypes = BusDayAdjustTypes.FOLLOWING,
                 dg_type: DateGenRuleTypes = DateGenRuleTypes.BACKWARD,
                 end_of_month: bool = False):
        """Bond paying ``coupon`` (decimal, per year) on the outstanding principal (bond.py:80-160).
        ``amortization_schedule``: the outstanding principal after each coupon period (None: bullet)."""
        check_argument_types(self.__init__, locals())
        self.derivative_type = InstrumentTypes.BOND
        self._maturity_dt = (maturity_dt_or_tenor if isinstance(maturity_dt_or_tenor, Date)
                             else issue_dt.add_tenor(maturity_dt_or_tenor))
        if issue_dt >= self._maturity_dt:
            raise LibError("Issue date must be before maturity date")
        self._issue_dt = issue_dt
        self._coupon = coupon
        self._freq_type = freq_type
        self._dc_type = dc_type
        self._currency = currency
        self._face_value = face_value
        self._payment_lag = payment_lag
        self._cal_type = cal_type
        self._bd_type = bd_type
        self._dg_type = dg_type
        self._end_of_month = end_of_month
        self._amortization_schedule = amortization_schedule
        self._is_zero_coupon = coupon == 0.0 or freq_type == FrequencyTypes.ZERO
        if self._is_zero_coupon:
            # one flow: the face at the UNADJUSTED maturity date, no payment lag
            self._payment_dts = [self._maturity_dt]
            self._year_fracs = [0.0]
            self._coupon_payments = [0.0]
            self._accrual_start_dts = [issue_dt]
            self._accrual_end_dts = [self._maturity_dt]
            self._num_coupons = 0
            self._principal_schedule = [self._face_value, 0.0]
            self._principal_payments = [self._face_value]
        else:
            self._generate_coupon_schedule()

    def _generate_coupon_schedule(self):
        """Coupon periods of the adjusted schedule; coupons accrue on the principal outstanding at the period's start
        (bond.py:162-247)."""
        calendar = Calendar(self._cal_type)
        dts = Schedule(effective_dt=self._issue_dt, termination_dt=self._maturity_dt, freq_type=self._freq_type,
                       cal_type=self._cal_type, bd_type=self._bd_type, dg_type=self._dg_type,
                       end_of_month=self._end_of_month)._adjusted_dts
        periods = len(dts) - 1
        if self._amortization_schedule is not None:
            if len(self._amortization_schedule) != periods:
                raise LibError(f"Amortization schedule length ({len(self._amortization_schedule)}) "
                               f"must match number of payment periods ({periods})")
            self._principal_schedule = [self._face_value] + list(self._amortization_schedule)
        else:
            self._principal_schedule = [self._face_value] * periods + [0.0]
        counter = DayCount(self._dc_type)
        self._accrual_start_dts, self._accrual_end_dts, self._payment_dts = [], [], []
        self._year_fracs, self._coupon_payments, self._principal_payments = [], [], []
        start = self._issue_dt
        for i, end in enumerate(dts[1:]):
            frac = counter.year_frac(start, end)[0]
            self._accrual_start_dts.append(start)
            self._accrual_end_dts.append(end)
            self._payment_dts.append(calendar.add_business_days(end, self._payment_lag))
            self._year_fracs.append(frac)
            self._coupon_payments.append(frac * self._coupon * self._principal_schedule[i])
            self._principal_payments.append(self._principal_schedule[i] - self._principal_schedule[i + 1])
            start = end
        self._num_coupons = len(self._payment_dts)

    def position(self, model):
        from ...market.position.position import Position
        return Position(self, model)

    # ------------------------------------------------------------------------------------------ prices
    @staticmethod
    def _spread_time(dt, settlement_dt):
        return (dt - settlement_dt) / SPREAD_DAYS_IN_YEAR

    def value(self, value_dt: Date, discount_curve, z_spread: float = 0.0, settlement_dt: Date = None):
        """PV of the flows paid after settlement, discounted relative to ``df(settlement)`` with the z-spread applied
        over the spread time (bond.py:262-370).  Coupons first, then the principal repayments: the reference's
        amortizing branch, which every bond takes since ``_principal_payments`` always exists.  A principal <= 0 is
        not paid."""
        if settlement_dt is None:
            settlement_dt = value_dt
        df_settle = discount_curve.df(settlement_dt)
        self._payment_dfs, self._coupon_pvs, self._principal_pvs = [], [], []

        def rel_df(dt):
            df = discount_curve.df(dt)
            if z_spread != 0.0:
                df = df * np.exp(-z_spread * self._spread_time(dt, settlement_dt))
            return df / df_settle

        pv = 0.0
        for i, dt in enumerate(self._payment_dts):
            if dt > settlement_dt:
                rel = rel_df(dt)
                cpv = self._coupon_payments[i] * rel
                pv += cpv
                self._payment_dfs.append(rel)
                self._coupon_pvs.append(cpv)
            else:
                self._payment_dfs.append(0.0)
                self._coupon_pvs.append(0.0)
        for i, dt in enumerate(self._payment_dts):
            if dt > settlement_dt and self._principal_payments[i] > 0:
                ppv = self._principal_payments[i] * rel_df(dt)
                pv += ppv
                self._principal_pvs.append(ppv)
            else:
                self._principal_pvs.append(0.0)
        return pv

    def accrued_interest(self, settlement_dt: Date):
        """Coupon accrued on the FACE from the start of the period paid next (bond.py:372-405)."""
        if self._is_zero_coupon:
            return 0.0
        last = self._issue_dt
        for i, dt in enumerate(self._payment_dts):
            if dt <= settlement_dt:
                last = self._accrual_end_dts[i]
            else:
                last = self._accrual_start_dts[i]
                break
        return DayCount(self._dc_type).year_frac(last, settlement_dt)[0] * self._coupon * self._face_value

    def _accrued_per_100(self, settlement_dt):
        return (self.accrued_interest(settlement_dt) / self._face_value) * 100.0

    def dirty_price(self, value_dt: Date, discount_curve, z_spread: float = 0.0, settlement_dt: Date = None):
        if settlement_dt is None:
            settlement_dt = value_dt
        return (self.value(value_dt, discount_curve, z_spread, settlement_dt) / self._face_value) * 100.0

    def clean_price(self, value_dt: Date, discount_curve, z_spread: float = 0.0, settlement_dt: Date = None):
        if settlement_dt is None:
            settlement_dt = value_dt
        return self.dirty_price(value_dt, discount_curve, z_spread, settlement_dt) - self._accrued_per_100(settlement_dt)

    # ------------------------------------------------------------------------------------------ yields and spreads
    def _target_pv(self, settlement_dt, clean_price):
        return ((clean_price + self._accrued_per_100(settlement_dt)) / 100.0) * self._face_value

    def _yield_flows(self, settlement_dt):
        """(spread times, amounts) the yield measures price: coupons paid after settlement plus the FULL face at the
        UNADJUSTED maturity date - amortization is ignored (bond.py:488-503, 648-750)."""
        taus, amts = [], []
        for i, dt in enumerate(self._payment_dts):
            if dt > settlement_dt:
                taus.append(self._spread_time(dt, settlement_dt))
                amts.append(self._coupon_payments[i])
        if self._maturity_dt > settlement_dt:
            taus.append(self._spread_time(self._maturity_dt, settlement_dt))
            amts.append(self._face_value)
        return taus, amts

    @staticmethod
    def _solve(fn, bracket, start):
        """brentq on the bracket; scipy's newton (a secant without a derivative) from ``start`` when the bracket has
        no sign change (bond.py:506-511, 562-567)."""
        try:
            return brentq(fn, bracket[0], bracket[1], maxiter=100)
        except Exception:
            return newton(fn, start, maxiter=100)

    def yield_to_maturity(self, settlement_dt: Date, clean_price: float):
        """Continuously compounded yield on the spread times (bond.py:450-511)."""
        target = self._target_pv(settlement_dt, clean_price)
        taus, amts = self._yield_flows(settlement_dt)

        def diff(y):
            pv = 0.0
            for t, a in zip(taus, amts):
                pv += a * np.exp(-y * t)
            return pv - target
        return self._solve(diff, YTM_BRACKET, YTM_START)

    def current_yield(self):
        """The coupon rate itself, 0 for a zero-coupon bond (bond.py:515-530)."""
        return 0.0 if self._is_zero_coupon else self._coupon

    def z_spread(self, settlement_dt: Date, discount_curve, clean_price: float):
        """Parallel spread over the curve that reprices the clean price (bond.py:532-569)."""
        target = self._target_pv(settlement_dt, clean_price)
        return self._solve(lambda z: self.value(settlement_dt, discount_curve, z, settlement_dt) - target,
                           Z_BRACKET, Z_START)

    def g_spread(self, settlement_dt: Date, govt_curve, clean_price: float):
        """Yield minus the government curve's zero rate at maturity in the bond's own conventions (bond.py:571-604)."""
        return (self.yield_to_maturity(settlement_dt, clean_price) -
                govt_curve.zero_rate(self._maturity_dt, freq_type=self._freq_type, dc_type=self._dc_type))

    def i_spread(self, settlement_dt: Date, discount_curve, clean_price: float):
        """Yield minus the swap curve's zero rate at maturity (bond.py:606-634)."""
        return (self.yield_to_maturity(settlement_dt, clean_price) -
                discount_curve.zero_rate(self._maturity_dt, freq_type=self._freq_type, dc_type=self._dc_type))

    # ------------------------------------------------------------------------------------------ risk
    def _yield_moments(self, settlement_dt, discount_curve, z_spread):
        clean = self.clean_price(settlement_dt, discount_curve, z_spread, settlement_dt)
        ytm = self.yield_to_maturity(settlement_dt, clean)
        taus, amts = self._yield_flows(settlement_dt)
        total = weighted = weighted2 = 0.0
        for t, a in zip(taus, amts):
            pv = a * np.exp(-ytm * t)
            total += pv
            weighted += pv * t
            weighted2 += pv * t ** 2
        return total, weighted, weighted2

    def duration(self, settlement_dt: Date, discount_curve, duration_type: str = 'modified', z_spread: float = 0.0):
        """Macaulay duration at the yield of the price at ``z_spread`` (bond.py:648-703).  'modified' returns the
        Macaulay number too: the reference treats the two as equal under continuous compounding."""
        total, weighted, _ = self._yield_moments(settlement_dt, discount_curve, z_spread)
        kind = duration_type.lower()
        if kind in ('macaulay', 'modified'):
            return weighted / total
        raise ValueError(f"Unknown duration type: {duration_type}")

    def convexity(self, settlement_dt: Date, discount_curve, z_spread: float = 0.0):
        """Sum of PV t^2 over PV at the yield (bond.py:705-750)."""
        total, _, weighted2 = self._yield_moments(settlement_dt, discount_curve, z_spread)
        return weighted2 / total

    def dv01(self, settlement_dt: Date, discount_curve, z_spread: float = 0.0):
        """(PV(z - 1bp) - PV(z + 1bp)) / 2 - a shift of the z-spread, not of the curve (bond.py:752-783)."""
        down = self.value(settlement_dt, discount_curve, z_spread - BUMP, settlement_dt)
        up = self.value(settlement_dt, discount_curve, z_spread + BUMP, settlement_dt)
        return (down - up) / 2.0

    def cs01(self, settlement_dt, discount_curve, z_spread: float = 0.0):
        """The same number as `dv01` (bond.py:834-875)."""
        return self.dv01(settlement_dt, discount_curve, z_spread)

    def key_rate_durations(self, model):
        """-delta / PV * 1e4 per curve tenor, from the engine's curve delta (bond.py:785-832)."""
        from ...market.position.engine import Engine
        from ...utils.global_types import RequestTypes
        res = Engine(model).compute(self, [RequestTypes.VALUE, RequestTypes.DELTA])
        price = res.value.amount
        return {tenor: (-float(d) / price * 10000.0 if price != 0 else 0.0)
                for tenor, d in zip(res.risk.tenors, res.risk.risk_ladder)}

    # ------------------------------------------------------------------------------------------ schedules
    @staticmethod
    def generate_equal_principal_schedule(face_value: float, num_periods: int):
        """Outstanding principal after each of ``num_periods`` equal repayments (bond.py:1028-1058)."""
        if num_periods <= 0:
            raise LibError("Number of periods must be positive")
        step = face_value / num_periods
        return [max(0.0, face_value - i * step) for i in range(1, num_periods + 1)]

    @staticmethod
    def generate_annuity_schedule(face_value: float, num_periods: int, coupon_rate: float, freq_type: FrequencyTypes):
        """Outstanding principal of a constant-payment annuity at the periodic rate coupon / periods per year
        (bond.py:1060-1114; frequencies other than annual, semi-annual, quarterly and monthly count as annual)."""
        if num_periods <= 0:
            raise LibError("Number of periods must be positive")
        per_year = {FrequencyTypes.ANNUAL: 1, FrequencyTypes.SEMI_ANNUAL: 2, FrequencyTypes.QUARTERLY: 4,
                    FrequencyTypes.MONTHLY: 12}.get(freq_type, 1)
        r = coupon_rate / per_year
        if r == 0:
            return Bond.generate_equal_principal_schedule(face_value, num_periods)
        factor = (1 + r) ** num_periods
        payment = face_value * (r * factor) / (factor - 1)
        out, balance = [], face_value
        for _ in range(num_periods):
            balance -= payment - balance * r
            out.append(max(0.0, balance))
        return out

    def __repr__(self):
        s = label_to_string("OBJECT TYPE", type(self).__name__)
        s += label_to_string("ISSUE DATE", self._issue_dt)
        s += label_to_string("MATURITY DATE", self._maturity_dt)
        s += label_to_string("COUPON", f"{self._coupon * 100:.4f}%")
        s += label_to_string("FREQUENCY", self._freq_type)
        s += label_to_string("DAY COUNT", self._dc_type)
        s += label_to_string("CURRENCY", self._currency)
        s += label_to_string("FACE VALUE", self._face_value)
        if self._is_zero_coupon:
            s += label_to_string("TYPE", "ZERO COUPON BOND")
        else:
            s += label_to_string("NUMBER OF COUPONS", self._num_coupons)
        return s
