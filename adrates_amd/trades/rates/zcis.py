"""Zero-coupon inflation swap: ``N * ((1 + r) ** T - 1)`` against ``N * (I(T - lag) / I(base - lag) - 1)`` at maturity.

Restates cavour/trades/rates/zcis.py: the constructor :70-174, `value` :178-235, `breakeven_inflation_rate` :239-282
and `pv01` :286-315.

Quirks kept on purpose:
- a ZCIS has an ``instrument_type`` but no ``derivative_type``, so the valuation engine cannot price it
  (`Engine.compute` fails on the missing attribute, as in the reference); its measures are these host methods;
- T is the swap day count's year fraction from the effective date to the ADJUSTED maturity; the fixed payment is
  discounted with ``df(dt, ACT_365F)``;
- `breakeven_inflation_rate` annualises the projected index return over that T; `pv01` is the derivative of the
  fixed payment's PV with respect to r, for 1bp, always positive.
"""
from __future__ import annotations

from ...market.indices.inflation_index import InflationIndex
from ...utils.calendar import BusDayAdjustTypes, Calendar, CalendarTypes
from ...utils.date import Date
from ...utils.day_count import DayCount, DayCountTypes
from ...utils.error import LibError
from ...utils.global_types import InstrumentTypes, SwapTypes
from ...utils.global_vars import ONE_MILLION
from ...utils.helpers import check_argument_types
from .swap_inflation_leg import SwapInflationLeg


class ZeroCouponInflationSwap:
    def __init__(self,
                 effective_dt: Date,
                 term_dt_or_tenor: (Date, str),
                 fixed_leg_type: SwapTypes,
                 fixed_rate: float,
                 inflation_index: InflationIndex,
                 notional: float = ONE_MILLION,
                 payment_lag: int = 0,
                 dc_type: DayCountTypes = DayCountTypes.ACT_365F,
                 cal_type: CalendarTypes = CalendarTypes.WEEKEND,
                 bd_type: BusDayAdjustTypes = BusDayAdjustTypes.FOLLOWING):
        check_argument_types(self.__init__, locals())
        self.instrument_type = InstrumentTypes.ZCIS
        self._termination_dt = (term_dt_or_tenor if isinstance(term_dt_or_tenor, Date)
                                else effective_dt.add_tenor(term_dt_or_tenor))
        calendar = Calendar(cal_type)
        self._maturity_dt = calendar.adjust(self._termination_dt, bd_type)
        if effective_dt > self._maturity_dt:
            raise LibError("Start date after maturity date")
        self._effective_dt = effective_dt
        self._fixed_leg_type = fixed_leg_type
        self._fixed_rate = fixed_rate
        self._inflation_index = inflation_index
        self._notional = notional
        self._payment_lag = payment_lag
        self._dc_type = dc_type
        self._cal_type = cal_type
        self._bd_type = bd_type
        self._payment_dt = (self._maturity_dt if payment_lag == 0
                            else calendar.add_business_days(self._maturity_dt, payment_lag))
        self._inflation_leg = SwapInflationLeg(
            effective_dt=effective_dt, end_dt=self._termination_dt,
            leg_type=SwapTypes.RECEIVE if fixed_leg_type == SwapTypes.PAY else SwapTypes.PAY,
            inflation_index=inflation_index, notional=notional, payment_lag=payment_lag, cal_type=cal_type,
            bd_type=bd_type)
        self._fixed_return = None
        self._fixed_payment = None
        self._fixed_pv = None
        self._inflation_pv = None
        self._payment_df = None

    def _year_frac(self):
        return DayCount(self._dc_type).year_frac(self._effective_dt, self._maturity_dt)[0]

    def _df(self, value_dt, discount_curve):
        if self._payment_dt > value_dt:
            return (discount_curve.df(self._payment_dt, DayCountTypes.ACT_365F) /
                    discount_curve.df(value_dt, DayCountTypes.ACT_365F))
        return 0.0

    def value(self, value_dt: Date, discount_curve, inflation_curve=None) -> float:
        year_frac = self._year_frac()
        self._fixed_return = ((1.0 + self._fixed_rate) ** year_frac) - 1.0
        self._fixed_payment = self._notional * self._fixed_return
        self._payment_df = self._df(value_dt, discount_curve)
        self._fixed_pv = self._fixed_payment * self._payment_df if self._payment_dt > value_dt else 0.0
        if self._fixed_leg_type == SwapTypes.PAY:
            self._fixed_pv *= -1.0
        self._inflation_pv = self._inflation_leg.value(value_dt, discount_curve, inflation_curve)
        return self._fixed_pv + self._inflation_pv

    def breakeven_inflation_rate(self, value_dt: Date, discount_curve, inflation_curve=None) -> float:
        self._inflation_leg.value(value_dt, discount_curve, inflation_curve)
        inflation_return = self._inflation_leg._inflation_return
        year_frac = self._year_frac()
        if year_frac <= 0:
            raise LibError("Year fraction must be positive")
        if inflation_return <= -1.0:
            raise LibError(f"Inflation return too negative: {inflation_return}")
        return ((1.0 + inflation_return) ** (1.0 / year_frac)) - 1.0

    def pv01(self, value_dt: Date, discount_curve) -> float:
        year_frac = self._year_frac()
        df = self._df(value_dt, discount_curve)
        dpv_dr = self._notional * year_frac * ((1.0 + self._fixed_rate) ** (year_frac - 1.0)) * df
        return abs(dpv_dr) * 0.0001
