"""A book of floating-rate notes of one currency and one index: batched discount margins and curve Greeks.

`FRNBook.measures` is `FRN.discount_margin`, `dirty_price`, `clean_price`, `value`, `modified_duration` and `dv01`
for every FRN at once, in one launch of the adr_frn_measures kernel (csrc/frn_measures.hip) on the discount and index
curves' OWN node sets - the nodes `DiscountCurve.df` reads.  `FRNBook.compute` is the engine's VALUE / DELTA / GAMMA
for every FRN in one batch (VALUE only when the index curve is not the discount curve).

The per-coupon and per-FRN arrays are compiled on the host (see include/adrates.h, adr_frn_measures): for each coupon
paid after settlement its discount-curve payment time and index-curve accrual times (year fractions in the FRN's day
count from each curve's value date, as ``DiscountCurve.df(dt, frn._dc_type)``), the index curve's and the FRN's year
fractions of the period, the DM time from settlement and whether the first fixing replaces its forward - the first
coupon paid after settlement, as in `FRN.value`; per FRN the settlement and maturity times, the terms and the accrued
interest per 100.
"""
from __future__ import annotations

from typing import Iterable

import numpy as np

from ... import _native
from ...trades.credit.frn import FRN
from ...utils.day_count import DayCount
from ...utils.error import LibError
from ...utils.global_types import InterpTypes, RequestTypes
from ...utils.helpers import times_from_dates
from .engine import Engine, bond_curve_type, price_frns

_NODE_INTERP = (InterpTypes.FLAT_FWD_RATES, InterpTypes.LINEAR_FWD_RATES, InterpTypes.LINEAR_ZERO_RATES)


def compile_frn_measures(frns, disc_curve, index_curve, settlement_dt) -> dict:
    """Inputs of adr_frn_measures for ``frns`` settling on ``settlement_dt``: ``cpn_off`` and the fields of
    `_native.FRN_FLOW_FIELDS` / `_native.FRN_FIELDS` except the quote and the solver's start."""
    index_counter = DayCount(index_curve._dc_type)
    off = [0]
    cols = {k: [] for k in _native.FRN_FLOW_FIELDS + _native.FRN_FIELDS}
    for f in frns:
        dc = f._dc_type
        counter = DayCount(dc)
        disc_time = lambda dt: times_from_dates(dt, disc_curve._value_dt, dc)
        index_time = lambda dt: times_from_dates(dt, index_curve._value_dt, dc)
        first = f._first_fixing_rate is not None
        for i, pay_dt in enumerate(f._payment_dts):
            if pay_dt > settlement_dt:                  # coupons on or before settlement are not paid
                start, end = f._start_accrued_dts[i], f._end_accrued_dts[i]
                cols["cpn_T"].append(disc_time(pay_dt))
                cols["cpn_ts"].append(index_time(start))
                cols["cpn_te"].append(index_time(end))
                cols["cpn_ialpha"].append(index_counter.year_frac(start, end)[0])
                cols["cpn_alpha"].append(float(f._year_fracs[i]))
                cols["cpn_tau"].append(counter.year_frac(settlement_dt, pay_dt)[0])
                cols["cpn_fix"].append(1.0 if first else 0.0)
                first = False
        off.append(len(cols["cpn_T"]))
        paid = f._maturity_dt > settlement_dt
        cols["frn_Ts"].append(disc_time(settlement_dt))
        cols["frn_TM"].append(disc_time(f._maturity_dt) if paid else np.nan)
        cols["frn_tauM"].append(counter.year_frac(settlement_dt, f._maturity_dt)[0] if paid else 0.0)
        cols["frn_face"].append(float(f._face_value))
        cols["frn_margin"].append(float(f._quoted_margin))
        cols["frn_cap"].append(np.inf if f._cap_rate is None else float(f._cap_rate))
        cols["frn_floor"].append(-np.inf if f._floor_rate is None else float(f._floor_rate))
        cols["frn_ffr"].append(0.0 if f._first_fixing_rate is None else float(f._first_fixing_rate))
        cols["frn_acc100"].append(f.accrued_interest(settlement_dt))
    out = {"cpn_off": np.array(off, dtype=np.int64)}
    for k, v in cols.items():
        if v or k in _native.FRN_FLOW_FIELDS:
            out[k] = np.array(v, dtype=np.float64)
    return out


def tile_frn_measures(book: dict, reps: int) -> dict:
    """``reps`` copies of a compiled book (`compile_frn_measures` output, with or without quotes), one after another -
    a large book from a few distinct FRNs, for benchmarks and scale tests."""
    off = np.asarray(book["cpn_off"], dtype=np.int64)
    counts = np.tile(off[1:] - off[:-1], reps)
    out = {"cpn_off": np.concatenate(([0], np.cumsum(counts))).astype(np.int64)}
    for k in _native.FRN_FLOW_FIELDS + _native.FRN_FIELDS:
        if k in book:
            out[k] = np.tile(np.asarray(book[k], dtype=np.float64), reps)
    return out


class FRNBook:
    """FRNs of ONE currency and ONE floating index, discounted on ``model``'s OIS curve for that currency."""

    def __init__(self, frns: Iterable[FRN], model, settlement_dt=None):
        self.frns = list(frns)
        if not self.frns:
            raise LibError("FRNBook needs at least one FRN")
        for f in self.frns:
            if not isinstance(f, FRN):
                raise LibError(f"FRNBook takes FRN objects, not {type(f).__name__}")
        if len({f._currency for f in self.frns}) != 1 or len({f._floating_index for f in self.frns}) != 1:
            raise LibError("FRNBook holds FRNs of one currency and one index; make one book per pair")
        self.model = model
        self.curve_type = bond_curve_type(self.frns[0])
        self.index_type = self.frns[0]._floating_index
        self.currency = self.frns[0]._currency
        self.curve = getattr(model.curves, self.curve_type.name)
        self.index_curve = getattr(model.curves, self.index_type.name)
        for c in (self.curve, self.index_curve):
            if c._interp_type not in _NODE_INTERP:
                raise LibError("Invalid interpolation scheme.")
        self.settlement_dt = self.curve._value_dt if settlement_dt is None else settlement_dt
        self._arrays = None
        self._engine = Engine(model)

    def __len__(self):
        return len(self.frns)

    @property
    def arrays(self) -> dict:
        """The compiled per-coupon / per-FRN inputs (without quotes); built once."""
        if self._arrays is None:
            self._arrays = compile_frn_measures(self.frns, self.curve, self.index_curve, self.settlement_dt)
        return self._arrays

    @staticmethod
    def _nodes(curve):
        return (curve._interp_type.value, np.asarray(curve._times, dtype=np.float64),
                np.asarray(curve._dfs, dtype=np.float64))

    def inputs(self, clean_prices=None, dms=None, dm_guess=0.0):
        """``(discount nodes, index nodes, book arrays with frn_quote and frn_guess, quote_is_dm)`` for
        adr_frn_measures; each nodes entry is ``(interp method, node times, node dfs)``."""
        if (clean_prices is None) == (dms is None):
            raise LibError("give exactly one of clean_prices and dms")
        quote = clean_prices if dms is None else dms
        n = len(self.frns)
        book = dict(self.arrays)
        book["frn_quote"] = np.broadcast_to(np.asarray(quote, dtype=np.float64), (n,)).copy()
        book["frn_guess"] = np.broadcast_to(np.asarray(dm_guess, dtype=np.float64), (n,)).copy()
        return self._nodes(self.curve), self._nodes(self.index_curve), book, dms is not None

    def measures(self, clean_prices=None, dms=None, dm_guess=0.0, ctx=None) -> dict:
        """Per-FRN arrays ``dm``, ``dirty``, ``clean`` (per 100), ``pv`` (currency), ``mod_duration``, ``dv01`` and
        ``status`` in one launch.  With ``clean_prices`` (per 100 face) the DM is solved (``dm_guess``: the fallback's
        start); with ``dms`` it is given.  status 0: solved inside the bracket; 1: by the fallback; 2: no root (NaN
        where `FRN.discount_margin` raises); 3: not priceable (NaN where `FRN.value` raises)."""
        disc, index, book, is_dm = self.inputs(clean_prices, dms, dm_guess)
        return _native.frn_measures(ctx or _native.default_context(), disc, index, book, is_dm)

    def compute(self, request_list, per_trade=True, aggregate=False) -> dict:
        """VALUE / DELTA / GAMMA of every FRN (``pv``, ``delta``, ``gamma``) and / or of the book (``agg_pv``,
        ``agg_delta``, ``agg_gamma``) in one batch, as `_native.price` returns them, plus ``tenors``.  A book whose
        index curve is not its discount curve has VALUE only."""
        reqs = set(request_list)
        if not reqs & {RequestTypes.VALUE, RequestTypes.DELTA, RequestTypes.GAMMA}:
            raise LibError("FRNBook.compute needs VALUE, DELTA or GAMMA")
        single = self.index_type == self.curve_type
        if not single and reqs & {RequestTypes.DELTA, RequestTypes.GAMMA}:
            raise LibError("Dual-curve FRN delta/gamma not yet implemented. "
                           "Use same curve for discounting and projection.")
        out = price_frns(self._engine, self.curve, self.frns, reqs, per_trade=per_trade, aggregate=aggregate,
                         index_model=None if single else self.index_curve)
        out["curve_type"], out["currency"] = self.curve_type, self.currency
        return out

    def revalue(self, grid, dms, buckets=None, spread_shocks=None, per_trade=False) -> dict:
        """The book's PV at the discount margins ``dms`` (one per FRN, e.g. ``measures(...)["dm"]``) under every
        scenario of ``grid``, a `ScenarioGrid` of this book's curve, paired with ``spread_shocks``:
        `ScenarioGrid.revalue_credit` (single-curve FRNs only)."""
        return grid.revalue_credit(self.frns, dms, buckets=buckets, spread_shocks=spread_shocks, per_trade=per_trade)
