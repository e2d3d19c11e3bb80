"""A book of year-on-year inflation swaps of one currency and one index: PV and both curves' ladders and gammas.

`YoYBook.compute` is the engine's VALUE / DELTA / GAMMA (market/position/inflation_engine.py) for every swap at once:
one launch of adr_yoy_risk (csrc/yoy_risk.hip) for the inflation side and one discount-side batch through the OIS
route, whose fixed flows carry the amounts that launch projected.
"""
from __future__ import annotations

from typing import Iterable

import numpy as np

from ... import _native
from ...trades.rates.yoy_inflation_swap import YoYInflationSwap
from ...utils.error import LibError
from ...utils.global_types import RequestTypes
from .engine import Engine
from .inflation_engine import price_yoy, yoy_curves


def tile_yoy_book(book: dict, reps: int) -> dict:
    """``reps`` copies of a compiled coupon book (`compile_yoy_coupons` output), one after another - a large book from a
    few distinct swaps, for benchmarks and scale tests."""
    off = np.asarray(book["cpn_off"], dtype=np.int64)
    counts = np.tile(off[1:] - off[:-1], reps)
    out = {"cpn_off": np.concatenate(([0], np.cumsum(counts))).astype(np.int64)}
    for k in _native.YOY_FIELDS:
        out[k] = np.tile(np.asarray(book[k], dtype=np.float64), reps)
    return out


class YoYBook:
    """YoY swaps of ONE currency and ONE index, on ``model``'s OIS curve for that currency and its inflation curve."""

    def __init__(self, swaps: Iterable[YoYInflationSwap], model):
        self.swaps = list(swaps)
        if not self.swaps:
            raise LibError("YoYBook needs at least one swap")
        for s in self.swaps:
            if not isinstance(s, YoYInflationSwap):
                raise LibError(f"YoYBook takes YoYInflationSwap objects, not {type(s).__name__}")
        keys = {(s._inflation_index._currency, s._inflation_index._index_type) for s in self.swaps}
        if len(keys) != 1:
            raise LibError("YoYBook holds swaps of one currency and one index; make one book per pair")
        self.model = model
        idx = self.swaps[0]._inflation_index
        self.currency = idx._currency
        self.curve, self.inflation_curve, self.curve_type, self.inflation_curve_type = yoy_curves(
            model, idx._currency, idx._index_type.name)
        self._engine = Engine(model)

    def __len__(self):
        return len(self.swaps)

    def compute(self, request_list, per_trade=True, aggregate=False) -> dict:
        """Per swap (``pv``, ``delta`` [n, P_d], ``gamma``, ``infl_delta`` [n, P_i], ``infl_gamma``, ``infl_pv``: the
        inflation leg alone) and / or for the book (``agg_pv``, ``agg_delta``, ``agg_gamma``, ``agg_infl_*``), plus the
        projected ``amount`` of every YoY coupon, ``tenors`` and ``infl_tenors``."""
        reqs = set(request_list)
        if not reqs & {RequestTypes.VALUE, RequestTypes.DELTA, RequestTypes.GAMMA}:
            raise LibError("YoYBook.compute needs VALUE, DELTA or GAMMA")
        out = price_yoy(self._engine, self.curve, self.inflation_curve, self.swaps, reqs, per_trade=per_trade,
                        aggregate=aggregate)
        out["curve_type"], out["inflation_curve_type"], out["currency"] = (self.curve_type, self.inflation_curve_type,
                                                                           self.currency)
        return out
