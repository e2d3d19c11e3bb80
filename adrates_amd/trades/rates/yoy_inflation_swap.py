"""Year-on-year inflation swap: a fixed leg against a YoY inflation leg on one schedule.

Restates cavour/trades/rates/yoy_inflation_swap.py: the constructor :80-201, `value` :205-243, `breakeven_rate`
:247-318 and `pv01` :322-352.

Quirks kept on purpose:
- there is no ``position()`` method; price it with ``Position(swap, model)``.  ``derivative_type`` is
  YOY_INFLATION_SWAP, which the engine prices (market/position/inflation_engine.py);
- the fixed leg's floating index is a placeholder chosen by currency (USD_OIS_SOFR for any other currency);
- `breakeven_rate` and `pv01` discount with ``df(dt, ACT_365F)`` although both legs use ``dc_type``.
"""
from __future__ import annotations

from ...market.indices.inflation_index import InflationIndex
from ...utils.calendar import BusDayAdjustTypes, Calendar, CalendarTypes, DateGenRuleTypes
from ...utils.currency import CurrencyTypes
from ...utils.date import Date
from ...utils.day_count import DayCountTypes
from ...utils.error import LibError
from ...utils.frequency import FrequencyTypes
from ...utils.global_types import CurveTypes, InstrumentTypes, SwapTypes
from ...utils.global_vars import ONE_MILLION
from ...utils.helpers import check_argument_types
from .swap_fixed_leg import SwapFixedLeg
from .swap_yoy_inflation_leg import SwapYoYInflationLeg

_FIXED_INDEX = {CurrencyTypes.GBP: CurveTypes.GBP_OIS_SONIA, CurrencyTypes.USD: CurveTypes.USD_OIS_SOFR,
                CurrencyTypes.EUR: CurveTypes.EUR_OIS_ESTR}


class YoYInflationSwap:
    def __init__(self,
                 effective_dt: Date,
                 term_dt_or_tenor: (Date, str),
                 fixed_leg_type: SwapTypes,
                 fixed_rate: float,
                 inflation_index: InflationIndex,
                 freq_type: FrequencyTypes,
                 notional: float = ONE_MILLION,
                 inflation_spread: float = 0.0,
                 dc_type: DayCountTypes = DayCountTypes.ACT_365F,
                 payment_lag: int = 0,
                 cal_type: CalendarTypes = CalendarTypes.WEEKEND,
                 bd_type: BusDayAdjustTypes = BusDayAdjustTypes.FOLLOWING,
                 dg_type: DateGenRuleTypes = DateGenRuleTypes.BACKWARD,
                 end_of_month: bool = False):
        check_argument_types(self.__init__, locals())
        self.instrument_type = InstrumentTypes.YOY_INFLATION_SWAP
        self.derivative_type = InstrumentTypes.YOY_INFLATION_SWAP
        self._termination_dt = (term_dt_or_tenor if isinstance(term_dt_or_tenor, Date)
                                else effective_dt.add_tenor(term_dt_or_tenor))
        self._maturity_dt = Calendar(cal_type).adjust(self._termination_dt, bd_type)
        if effective_dt > self._maturity_dt:
            raise LibError("Start date after maturity date")
        self._effective_dt = effective_dt
        self._fixed_leg_type = fixed_leg_type
        self._fixed_rate = fixed_rate
        self._inflation_index = inflation_index
        self._freq_type = freq_type
        self._notional = notional
        self._inflation_spread = inflation_spread
        self._dc_type = dc_type
        self._payment_lag = payment_lag
        self._cal_type = cal_type
        self._bd_type = bd_type
        self._dg_type = dg_type
        self._end_of_month = end_of_month
        inflation_leg_type = SwapTypes.RECEIVE if fixed_leg_type == SwapTypes.PAY else SwapTypes.PAY
        currency = inflation_index._currency
        self._fixed_leg = SwapFixedLeg(
            effective_dt=effective_dt, end_dt=self._termination_dt, leg_type=fixed_leg_type, coupon=fixed_rate,
            freq_type=freq_type, dc_type=dc_type, floating_index=_FIXED_INDEX.get(currency, CurveTypes.USD_OIS_SOFR),
            currency=currency, notional=notional, payment_lag=payment_lag, cal_type=cal_type, bd_type=bd_type,
            dg_type=dg_type, end_of_month=end_of_month)
        self._inflation_leg = SwapYoYInflationLeg(
            effective_dt=effective_dt, end_dt=self._termination_dt, leg_type=inflation_leg_type,
            inflation_index=inflation_index, freq_type=freq_type, dc_type=dc_type, notional=notional,
            spread=inflation_spread, payment_lag=payment_lag, cal_type=cal_type, bd_type=bd_type, dg_type=dg_type,
            end_of_month=end_of_month)
        self._fixed_pv = None
        self._inflation_pv = None

    def value(self, value_dt: Date, discount_curve, inflation_curve=None) -> float:
        self._fixed_pv = self._fixed_leg.value(value_dt, discount_curve)
        self._inflation_pv = self._inflation_leg.value(value_dt, discount_curve, inflation_curve)
        return self._fixed_pv + self._inflation_pv

    def _annuity(self, value_dt, discount_curve):
        annuity = 0.0
        for i, payment_dt in enumerate(self._fixed_leg._payment_dts):
            if payment_dt <= value_dt:
                continue
            df = (discount_curve.df(payment_dt, DayCountTypes.ACT_365F) /
                  discount_curve.df(value_dt, DayCountTypes.ACT_365F))
            annuity += self._fixed_leg._year_fracs[i] * df
        return annuity

    def breakeven_rate(self, value_dt: Date, discount_curve, inflation_curve=None) -> float:
        inflation_pv = self._inflation_leg.value(value_dt, discount_curve, inflation_curve)
        annuity = self._annuity(value_dt, discount_curve)
        if annuity <= 0:
            raise LibError("Annuity must be positive for breakeven calculation")
        if self._fixed_leg_type == SwapTypes.PAY:
            return inflation_pv / (self._notional * annuity)
        return -inflation_pv / (self._notional * annuity)

    def pv01(self, value_dt: Date, discount_curve) -> float:
        return abs(self._notional * self._annuity(value_dt, discount_curve) * 0.0001)
