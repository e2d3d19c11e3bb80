"""Inflation leg of a zero-coupon inflation swap: one payment ``N * (I(T - lag) / I(base - lag) - 1)`` at maturity.

Restates cavour/trades/rates/swap_inflation_leg.py: the constructor :70-165 and `value` :169-247.

Quirks kept on purpose: the base index is read at the EFFECTIVE date (lagged), so a seasoned leg's base is a fixing;
the payment is discounted with ``df(dt, ACT_365F)``, whatever the curve's day count; and a payment on or before the
value date is worth 0, but its amount is still computed (so `value` raises when the index cannot be read).
"""
from __future__ import annotations

from ...market.indices.inflation_index import InflationIndex
from ...utils.calendar import BusDayAdjustTypes, Calendar, CalendarTypes
from ...utils.date import Date
from ...utils.day_count import DayCountTypes
from ...utils.error import LibError
from ...utils.global_types import InstrumentTypes, SwapTypes
from ...utils.global_vars import ONE_MILLION
from ...utils.helpers import check_argument_types


class SwapInflationLeg:
    def __init__(self,
                 effective_dt: Date,
                 end_dt: (Date, str),
                 leg_type: SwapTypes,
                 inflation_index: InflationIndex,
                 notional: float = ONE_MILLION,
                 payment_lag: int = 0,
                 cal_type: CalendarTypes = CalendarTypes.WEEKEND,
                 bd_type: BusDayAdjustTypes = BusDayAdjustTypes.FOLLOWING):
        check_argument_types(self.__init__, locals())
        self.instrument_type = InstrumentTypes.SWAP_INFLATION_LEG
        self._termination_dt = end_dt if isinstance(end_dt, Date) else effective_dt.add_tenor(end_dt)
        calendar = Calendar(cal_type)
        self._maturity_dt = calendar.adjust(self._termination_dt, bd_type)
        if effective_dt > self._maturity_dt:
            raise LibError("Start date after maturity date")
        self._effective_dt = effective_dt
        self._leg_type = leg_type
        self._inflation_index = inflation_index
        self._notional = notional
        self._payment_lag = payment_lag
        self._cal_type = cal_type
        self._bd_type = bd_type
        self._payment_dt = (self._maturity_dt if payment_lag == 0
                            else calendar.add_business_days(self._maturity_dt, payment_lag))
        self._base_cpi_ref_dt = effective_dt
        self._final_cpi_ref_dt = self._maturity_dt
        self._base_index = None
        self._final_index = None
        self._inflation_return = None
        self._payment_amount = None
        self._payment_df = None
        self._payment_pv = None

    def value(self, value_dt: Date, discount_curve, inflation_curve=None) -> float:
        if inflation_curve is not None:
            self._inflation_index.set_inflation_curve(inflation_curve)
        self._base_index = self._inflation_index.get_index(self._base_cpi_ref_dt, apply_lag=True)
        self._final_index = self._inflation_index.get_index(self._final_cpi_ref_dt, apply_lag=True)
        if self._base_index <= 0.0:
            raise LibError(f"Base index must be positive, got {self._base_index}")
        self._inflation_return = (self._final_index / self._base_index) - 1.0
        self._payment_amount = self._notional * self._inflation_return
        if self._payment_dt > value_dt:
            df_value = discount_curve.df(value_dt, DayCountTypes.ACT_365F)
            df_payment = discount_curve.df(self._payment_dt, DayCountTypes.ACT_365F)
            self._payment_df = df_payment / df_value
            self._payment_pv = self._payment_amount * self._payment_df
            leg_pv = self._payment_pv
        else:
            self._payment_df = 0.0
            self._payment_pv = 0.0
            leg_pv = 0.0
        if self._leg_type == SwapTypes.PAY:
            leg_pv *= -1.0
        return leg_pv
