"""Year-on-year inflation leg: ``N * alpha_i * (I(te_i - lag) / I(te_i - 12M - lag) - 1 + spread)`` per period.

Restates cavour/trades/rates/swap_yoy_inflation_leg.py: the constructor :75-185, `generate_payment_schedule` :189-260
and `value` :264-367.

Quirks kept on purpose:
- the YoY start is ``end.add_months(-12)`` whatever the frequency, so the periods of a monthly or quarterly leg
  overlap; both reference dates are lagged by the index;
- a payment on or before the value date is skipped and its slots hold 0.0;
- discounting uses ``df(dt, leg dc_type)``.  The valuation results live in ``_dfs`` / ``_pvs``, not in the
  ``_payment_dfs`` / ``_payment_pvs`` that the engine's cash-flow table looks for, so the engine reports no YoY items
  (market/position/inflation_engine.py).
"""
from __future__ import annotations

from ...market.indices.inflation_index import InflationIndex
from ...utils.calendar import BusDayAdjustTypes, Calendar, CalendarTypes, DateGenRuleTypes
from ...utils.date import Date
from ...utils.day_count import DayCount, DayCountTypes
from ...utils.error import LibError
from ...utils.frequency import FrequencyTypes
from ...utils.global_types import InstrumentTypes, SwapTypes
from ...utils.global_vars import ONE_MILLION
from ...utils.helpers import check_argument_types
from ...utils.schedule import Schedule


class SwapYoYInflationLeg:
    def __init__(self,
                 effective_dt: Date,
                 end_dt: (Date, str),
                 leg_type: SwapTypes,
                 inflation_index: InflationIndex,
                 freq_type: FrequencyTypes,
                 dc_type: DayCountTypes,
                 notional: float = ONE_MILLION,
                 spread: float = 0.0,
                 payment_lag: int = 0,
                 cal_type: CalendarTypes = CalendarTypes.WEEKEND,
                 bd_type: BusDayAdjustTypes = BusDayAdjustTypes.FOLLOWING,
                 dg_type: DateGenRuleTypes = DateGenRuleTypes.BACKWARD,
                 end_of_month: bool = False):
        check_argument_types(self.__init__, locals())
        self.instrument_type = InstrumentTypes.SWAP_YOY_INFLATION_LEG
        self._termination_dt = end_dt if isinstance(end_dt, Date) else effective_dt.add_tenor(end_dt)
        self._maturity_dt = Calendar(cal_type).adjust(self._termination_dt, bd_type)
        if effective_dt > self._maturity_dt:
            raise LibError("Start date after maturity date")
        self._effective_dt = effective_dt
        self._end_dt = end_dt
        self._leg_type = leg_type
        self._inflation_index = inflation_index
        self._freq_type = freq_type
        self._dc_type = dc_type
        self._notional = notional
        self._spread = spread
        self._payment_lag = payment_lag
        self._cal_type = cal_type
        self._bd_type = bd_type
        self._dg_type = dg_type
        self._end_of_month = end_of_month
        self._start_cpis, self._end_cpis, self._yoy_rates = [], [], []
        self._payments, self._dfs, self._pvs = [], [], []
        self.generate_payment_schedule()

    def generate_payment_schedule(self):
        dts = Schedule(self._effective_dt, self._termination_dt, self._freq_type, self._cal_type, self._bd_type,
                       self._dg_type, end_of_month=self._end_of_month)._adjusted_dts
        if len(dts) < 2:
            raise LibError("Schedule has none or only one date")
        calendar = Calendar(self._cal_type)
        counter = DayCount(self._dc_type)
        self._start_accrued_dts, self._end_accrued_dts, self._payment_dts = [], [], []
        self._year_fracs, self._accrued_days, self._yoy_start_dts, self._yoy_end_dts = [], [], [], []
        for i in range(1, len(dts)):
            start_dt, end_dt = dts[i - 1], dts[i]
            year_frac, num_days, _ = counter.year_frac(start_dt, end_dt, None, None)
            payment_dt = end_dt if self._payment_lag == 0 else calendar.add_business_days(end_dt, self._payment_lag)
            self._start_accrued_dts.append(start_dt)
            self._end_accrued_dts.append(end_dt)
            self._payment_dts.append(payment_dt)
            self._year_fracs.append(year_frac)
            self._accrued_days.append(num_days)
            self._yoy_start_dts.append(end_dt.add_months(-12))
            self._yoy_end_dts.append(end_dt)

    def value(self, value_dt: Date, discount_curve, inflation_curve=None) -> float:
        if inflation_curve is not None:
            self._inflation_index.set_inflation_curve(inflation_curve)
        self._start_cpis, self._end_cpis, self._yoy_rates = [], [], []
        self._payments, self._dfs, self._pvs = [], [], []
        leg_pv = 0.0
        for i, payment_dt in enumerate(self._payment_dts):
            if payment_dt <= value_dt:
                for slot in (self._start_cpis, self._end_cpis, self._yoy_rates, self._payments, self._dfs, self._pvs):
                    slot.append(0.0)
                continue
            start_cpi = self._inflation_index.get_index(self._yoy_start_dts[i], apply_lag=True)
            end_cpi = self._inflation_index.get_index(self._yoy_end_dts[i], apply_lag=True)
            if start_cpi <= 0.0:
                raise LibError(f"Start CPI must be positive, got {start_cpi}")
            yoy_rate = (end_cpi / start_cpi) - 1.0
            payment = self._notional * self._year_fracs[i] * (yoy_rate + self._spread)
            df = discount_curve.df(payment_dt, self._dc_type) / discount_curve.df(value_dt, self._dc_type)
            pv = payment * df
            self._start_cpis.append(start_cpi)
            self._end_cpis.append(end_cpi)
            self._yoy_rates.append(yoy_rate)
            self._payments.append(payment)
            self._dfs.append(df)
            self._pvs.append(pv)
            leg_pv += pv
        if self._leg_type == SwapTypes.PAY:
            leg_pv *= -1.0
        return leg_pv
