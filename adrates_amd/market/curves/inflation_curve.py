"""Inflation curve from zero-coupon inflation swap quotes: cumulative index factors for forward CPI projection.

Restates cavour/market/curves/inflation_curve.py: the constructor and its checks :94-156, `_prepare_curve_builder_inputs`
:160-199, `_build_curve` :203-251, `_check_refits` (tolerance ZCIS_TOL = 1e-10) :319-367, `forward_index` :371-403 and
`inflation_rate` :407-441.

Quirks kept on purpose:
- there is no bootstrap.  The nodes are ``(0, 1)`` and ``(T_k, (1 + b_k) ** T_k)`` with ``b_k`` each ZCIS's fixed
  rate and ``T_k`` the curve day count's year fraction from that ZCIS's EFFECTIVE date to its maturity - not from
  the curve's value date.  The ``discount_curve`` argument is stored and never used;
- LINEAR and COMPOUND both map to LINEAR_ZERO_RATES, FLAT to FLAT_FWD_RATES;
- the host methods (`forward_index`, `inflation_rate`, so every trade's `value`) read the nodes through
  ``DiscountCurve._df`` (interpolator._point).  The valuation engine reads the same nodes through
  InterpolatorAd.simple_interpolate instead; the two differ before ``T_1`` under LINEAR_ZERO_RATES (the engine
  interpolates from a zero rate of 0 at t = 0, `_point` holds the first node's rate flat), beyond the last node
  (the engine clamps, which under FLAT_FWD_RATES means no inflation at all; `_point` extrapolates the last slope)
  and before the value date (the engine's factor is 1; `forward_index` raises).
"""
from __future__ import annotations

import numpy as np

from ...utils.currency import CurrencyTypes
from ...utils.date import Date
from ...utils.day_count import DayCount, DayCountTypes
from ...utils.error import LibError
from ...utils.global_types import InflationIndexTypes, InflationInterpTypes, InterpTypes
from .discount_curve import DiscountCurve

ZCIS_TOL = 1e-10

INFLATION_INTERP = {
    InflationInterpTypes.LINEAR: InterpTypes.LINEAR_ZERO_RATES,
    InflationInterpTypes.COMPOUND: InterpTypes.LINEAR_ZERO_RATES,
    InflationInterpTypes.FLAT: InterpTypes.FLAT_FWD_RATES,
}


class InflationCurve(DiscountCurve):
    def __init__(self,
                 value_dt: Date,
                 zcis_instruments: list,
                 base_cpi: float,
                 currency: CurrencyTypes,
                 index_type: InflationIndexTypes,
                 discount_curve: DiscountCurve = None,
                 interp_type: InflationInterpTypes = InflationInterpTypes.LINEAR,
                 dc_type: DayCountTypes = DayCountTypes.ACT_365F,
                 check_refit: bool = False):
        if base_cpi <= 0.0:
            raise LibError("Base CPI must be positive")
        if len(zcis_instruments) < 2:
            raise LibError("Need at least 2 ZCIS instruments to build a curve")
        self._value_dt = value_dt
        self._used_swaps = zcis_instruments
        self._base_cpi = base_cpi
        self._currency = currency
        self._index_type = index_type
        self._discount_curve = discount_curve
        self._interp_type_infl = interp_type
        self._dc_type = dc_type
        self._check_refit = check_refit
        self._build_curve(self._prepare_curve_builder_inputs())
        if self._check_refit:
            self._check_refits(ZCIS_TOL)

    def _prepare_curve_builder_inputs(self):
        """The ZCIS fixed rates; sets ``swap_times`` (effective -> maturity) and the display ``tenors``."""
        counter = DayCount(self._dc_type)
        rates, self.swap_times, self.tenors = [], [], []
        for zcis in self._used_swaps:
            rates.append(zcis._fixed_rate)
            yf = counter.year_frac(zcis._effective_dt, zcis._maturity_dt)[0]
            self.swap_times.append(yf)
            self.tenors.append(f"{int(round(yf))}Y" if abs(yf - round(yf)) < 0.1 else f"{yf:.2f}Y")
        return rates

    def _build_curve(self, breakeven_rates):
        self._interp_type = INFLATION_INTERP.get(self._interp_type_infl, InterpTypes.LINEAR_ZERO_RATES)
        times, factors = [0.0], [1.0]
        for t_mat, rate in zip(self.swap_times, breakeven_rates):
            times.append(t_mat)
            factors.append((1.0 + rate) ** t_mat)
        self._times = np.array(times, dtype=np.float64)
        self._dfs = np.array(factors, dtype=np.float64)
        if not all(self._times[i] < self._times[i + 1] for i in range(len(self._times) - 1)):
            raise LibError("Pillar times must be strictly increasing")

    def _check_refits(self, zcis_tol):
        counter = DayCount(self._dc_type)
        for zcis in self._used_swaps:
            yf = counter.year_frac(zcis._effective_dt, zcis._maturity_dt)[0]
            factor = self._df(yf)
            implied = factor ** (1.0 / yf) - 1.0 if yf > 0 else 0.0
            diff = abs(implied - zcis._fixed_rate)
            if diff > zcis_tol:
                raise LibError(f"ZCIS with maturity {zcis._maturity_dt} not repriced. "
                               f"Difference is {diff * 10000:.4f} bps")

    def forward_index(self, target_date: Date) -> float:
        """``base_cpi`` times the curve's factor at the curve-day-count time from the value date."""
        if target_date < self._value_dt:
            raise LibError(f"Cannot project CPI before value date. Target: {target_date}, Value: {self._value_dt}")
        yf = DayCount(self._dc_type).year_frac(self._value_dt, target_date)[0]
        return self._base_cpi * self._df(yf)

    def inflation_rate(self, start_dt: Date, end_dt: Date) -> float:
        """Annualised rate r with ``(1 + r) ** yf = I(end) / I(start)``."""
        if end_dt <= start_dt:
            raise LibError("End date must be after start date")
        cpi_start = self.forward_index(start_dt)
        cpi_end = self.forward_index(end_dt)
        yf = DayCount(self._dc_type).year_frac(start_dt, end_dt)[0]
        if yf <= 0:
            raise LibError("Year fraction must be positive")
        return (cpi_end / cpi_start) ** (1.0 / yf) - 1.0
