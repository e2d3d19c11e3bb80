"""CPI / RPI / HICP index: fixings, publication lag, intra-month interpolation and forward projection.

Restates cavour/market/indices/inflation_index.py: the constructor and its checks :75-153, the seasonality checks
and adjustment :157-213, `add_fixing` :217-233, `set_inflation_curve` :237-248, `get_index` :252-297,
`inflation_ratio` :301-333, `_apply_lag` :337-352, `_get_historical_index` :356-412, `_interpolate` (FLAT / LINEAR /
COMPOUND) :416-470 and `get_all_fixings` :474-484.

Quirks kept on purpose:
- the base fixing is stored as an ordinary fixing, so the fixing range always starts at ``base_date``;
- a date strictly inside the fixing range is interpolated between its bracketing fixings (not only intra-month), and
  a date outside the range goes to the curve's ``forward_index`` (then raises when no curve is set);
- seasonality multiplies the fixings as well as the curve's projections, by the LAGGED date's month;
- LINEAR and COMPOUND measure elapsed time in ACT/365F year fractions, whatever the index.
"""
from __future__ import annotations

from typing import Dict, Optional

from ...utils.currency import CurrencyTypes
from ...utils.date import Date
from ...utils.day_count import DayCount, DayCountTypes
from ...utils.error import LibError
from ...utils.global_types import InflationIndexTypes, InflationInterpTypes
from ...utils.helpers import check_argument_types


class InflationIndex:
    def __init__(self,
                 index_type: InflationIndexTypes,
                 base_date: Date,
                 base_index: float,
                 currency: CurrencyTypes,
                 lag_months: int = 3,
                 interp_type: InflationInterpTypes = InflationInterpTypes.LINEAR,
                 seasonality_factors: Optional[Dict[int, float]] = None):
        check_argument_types(self.__init__, locals())
        if base_index <= 0.0:
            raise LibError("Base index must be positive")
        if lag_months < 0:
            raise LibError("Lag months must be non-negative")
        if seasonality_factors is not None:
            self._validate_seasonality_factors(seasonality_factors)
        self._index_type = index_type
        self._base_date = base_date
        self._base_index = base_index
        self._currency = currency
        self._lag_months = lag_months
        self._interp_type = interp_type
        self._seasonality_factors = seasonality_factors or {}
        self._use_seasonality = len(self._seasonality_factors) > 0
        # {excel serial: (Date, value)} - Date is not hashable
        self._fixings: Dict[float, tuple] = {base_date._excel_dt: (base_date, base_index)}
        self._inflation_curve = None

    def _validate_seasonality_factors(self, factors: Dict[int, float]):
        if set(factors.keys()) != set(range(1, 13)):
            raise LibError(f"Seasonality factors must include all months 1-12. Got: {sorted(factors.keys())}")
        for month, factor in factors.items():
            if factor <= 0:
                raise LibError(f"Seasonality factors must be positive. Month {month} has factor {factor}")
        avg_factor = sum(factors.values()) / 12.0
        if abs(avg_factor - 1.0) > 0.01:
            raise LibError(f"Seasonality factors should average to 1.0 (within 1% tolerance). "
                           f"Got average: {avg_factor:.6f}")

    def _apply_seasonality(self, date: Date, cpi_value: float) -> float:
        if not self._use_seasonality:
            return cpi_value
        return cpi_value * self._seasonality_factors.get(date._m, 1.0)

    def add_fixing(self, fixing_date: Date, index_value: float):
        if index_value <= 0.0:
            raise LibError(f"Index value must be positive, got {index_value}")
        self._fixings[fixing_date._excel_dt] = (fixing_date, index_value)

    def set_inflation_curve(self, inflation_curve):
        self._inflation_curve = inflation_curve

    def get_index(self, ref_date: Date, apply_lag: bool = True) -> float:
        """The index at ``ref_date`` shifted back by the lag: a fixing (or an interpolation between two), else the
        curve's projection; seasonality applied last."""
        lookup_date = self._apply_lag(ref_date) if apply_lag else ref_date
        index_value = self._get_historical_index(lookup_date)
        if index_value is not None:
            return self._apply_seasonality(lookup_date, index_value)
        if self._inflation_curve is not None:
            return self._apply_seasonality(lookup_date, self._inflation_curve.forward_index(lookup_date))
        raise LibError(f"No fixing available for {lookup_date} and no inflation curve set. "
                       f"Add fixings via add_fixing() or set curve via set_inflation_curve().")

    def inflation_ratio(self, start_dt: Date, end_dt: Date, apply_lag: bool = True) -> float:
        index_start = self.get_index(start_dt, apply_lag=apply_lag)
        index_end = self.get_index(end_dt, apply_lag=apply_lag)
        if index_start <= 0.0:
            raise LibError(f"Start index must be positive, got {index_start}")
        return index_end / index_start

    def _apply_lag(self, ref_date: Date) -> Date:
        return ref_date.add_months(-self._lag_months)

    def _get_historical_index(self, lookup_date: Date) -> Optional[float]:
        if not self._fixings:
            return None
        keys = sorted(self._fixings.keys())
        dates = [self._fixings[k][0] for k in keys]
        if lookup_date < dates[0] or lookup_date > dates[-1]:
            return None
        if lookup_date._excel_dt in self._fixings:
            return self._fixings[lookup_date._excel_dt][1]
        for i in range(len(dates) - 1):
            if dates[i] <= lookup_date <= dates[i + 1]:
                return self._interpolate(lookup_date, dates[i], dates[i + 1], self._fixings[keys[i]][1],
                                         self._fixings[keys[i + 1]][1])
        return None

    def _interpolate(self, target_date: Date, lower_date: Date, upper_date: Date, lower_value: float,
                     upper_value: float) -> float:
        if self._interp_type == InflationInterpTypes.FLAT:
            return lower_value
        if self._interp_type in (InflationInterpTypes.LINEAR, InflationInterpTypes.COMPOUND):
            counter = DayCount(DayCountTypes.ACT_365F)
            total = counter.year_frac(lower_date, upper_date)[0]
            elapsed = counter.year_frac(lower_date, target_date)[0]
            if total == 0:
                return lower_value
            weight = elapsed / total
            if self._interp_type == InflationInterpTypes.LINEAR:
                return lower_value + weight * (upper_value - lower_value)
            return lower_value * ((upper_value / lower_value) ** weight)
        raise LibError(f"Unknown interpolation type: {self._interp_type}")

    def get_all_fixings(self) -> list:
        """``[(Date, value), ...]`` in insertion order, the base fixing first."""
        return [(date, value) for date, value in self._fixings.values()]
