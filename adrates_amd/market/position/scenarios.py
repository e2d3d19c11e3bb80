"""Scenario batches: many shocked versions of one curve, bootstrapped and priced on the GPU.

The reference shocks a curve by building a whole new `Model` per shock
(`Model.scenario`, cavour/models/models.py:507-557) and re-running the JAX scan,
`jacrev` and `hessian` for each (cavour/market/position/engine.py:2246-2412);
its finite-difference helpers do that twice per bumped tenor
(tests/test_ois_request_types.py:137-207).  A shock moves the par rates only -
schedules, hence the knot grid, stay - so here all shocked curves of a grid are
bootstrapped together by the device builder (csrc/curve_build.hip,
adr_curve_set_build) and every scenario is priced with the ordinary kernels.

Shocks use `Model.scenario`'s convention: a float shifts every quote, a dict
``{tenor: shift}`` only the named ones; shifts are in the quotes' units (percent).

Full revaluation - the P&L vector behind historical-simulation VaR, expected
shortfall and stress tests - does not loop over the scenarios: `ScenarioGrid.revalue`
/ `pnl` and `revalue_on_curves` price the book under all curves in one launch of
csrc/scenario_pv.hip (adr_scenario_pv), which reads the trades once and takes
discount factors only (no Jacobians).

Credit books - bonds at their z-spreads, FRNs at their discount margins - are
revalued under joint (curve, spread) scenarios by `ScenarioGrid.revalue_credit` /
`pnl_credit` and `revalue_credit_on_curves` in one launch of
csrc/credit_scenario_pv.hip (adr_credit_scenario_pv): a spread per trade, a spread
shock per scenario and credit bucket.

Sub-books - desks, counterparties, margin accounts - get their P&L vectors from the SAME single launch:
`ScenarioGrid.revalue_sub_books` / `pnl_sub_books` (and the credit forms) take one key per trade and return one row
per distinct key, each with the bits the whole-book call gives on that sub-book alone; `tail_measures` and
`ScenarioGrid.sub_book_var_es` turn the rows into VaR and expected shortfall on the device (csrc/subbook.hip).
YoY books have the same through `revalue_yoy_on_curves_sub_books` and `YoYBook.revalue_sub_books`.

Delta-gamma P&L: `ScenarioGrid.pnl_delta_gamma` / `pnl_delta_gamma_sub_books` put the grid's shocks, in basis points,
through the desks' delta and gamma ladders instead of revaluing (market/position/ladder_pnl.py, adr_ladder_pnl);
`explain_sub_books` sets that beside `pnl_sub_books` - the unexplained P&L per desk and scenario - and
`sub_book_delta_gamma_var_es` chains ladders, P&L and tail kernel on the device.

Credit desks have the same three: `pnl_credit_delta_gamma_sub_books` (ladders at the spreads plus CS01, spread gamma and the
rate x spread cross gamma per bucket, adr_credit_subbook_ladders), `explain_credit_sub_books` beside `pnl_credit_sub_books`
and `sub_book_credit_delta_gamma_var_es`.

Firm-wide: `combine_sub_book_rows` adds the per-desk rows of the rates, credit and inflation launches by label and
`allocate_tail` splits the firm's VaR and expected shortfall among the desks (adr_scenario_tail_alloc, csrc/subbook.hip).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Union

import numpy as np

from ... import _native
from ...trades.credit.bond import SPREAD_DAYS_IN_YEAR
from ...trades.compiler import (TradeBatch, compile_bonds, compile_frns, compile_ois, compile_yoy_coupons,
                                compile_yoy_fixed_legs)
from ...utils.error import LibError
from ...utils.global_types import CurveTypes, InstrumentTypes, InterpTypes, RequestTypes
from ...utils.helpers import to_tenor
from .engine import BOND_CURVES, _SUPPORTED_INTERP, frn_is_single_curve
from .inflation_engine import inflation_inputs
from .ladder_pnl import (credit_delta_gamma_sub_books, credit_shock_matrix_bp, delta_gamma_sub_books, first_ratio_trade,
                         shock_matrix_bp)
from ..curves.curve_tables import build_engine_curve

Shock = Union[float, Dict[str, float]]


def shocked_quotes(base_px: Sequence[float], tenors: Sequence[str], shock: Shock) -> List[float]:
    """The quote list `Model.scenario` would build the shocked curve from (models.py:539-546)."""
    if isinstance(shock, dict):
        return [base_px[i] + shock.get(t, 0.0) for i, t in enumerate(tenors)]
    return [px + shock for px in base_px]


def _interp_value(method) -> int:
    """An `InterpTypes` member or its value as the value of a scheme the kernels take."""
    method = int(getattr(method, "value", method))
    if method not in _SUPPORTED_INTERP:
        raise LibError("Invalid interpolation scheme.")
    return method


def _disc_infl_methods(disc_method, infl_method):
    """The same for a YoY pair: the discount curve's scheme and the inflation curve's, which has two to choose from."""
    dm, im = int(getattr(disc_method, "value", disc_method)), int(getattr(infl_method, "value", infl_method))
    if dm not in _SUPPORTED_INTERP or im not in (InterpTypes.LINEAR_ZERO_RATES.value, InterpTypes.FLAT_FWD_RATES.value):
        raise LibError("Invalid interpolation scheme.")
    return dm, im


def _first_appearance(keys):
    """``(labels, index)``: the distinct ``keys`` in order of first appearance, and the number of each."""
    index = {}
    for k in keys:
        if k not in index:
            index[k] = len(index)
    return list(index), index


def _concat_batches(batches: Sequence[TradeBatch]) -> TradeBatch:
    """One batch holding the trades of ``batches`` in order."""
    batches = [b for b in batches if b.n_trades]
    if len(batches) == 1:
        return batches[0]
    cat = lambda name: np.concatenate([np.asarray(getattr(b, name), dtype=np.float64) for b in batches])
    offs = lambda name: np.concatenate([[0]] + [np.asarray(getattr(b, name)[1:]) + base for b, base in zip(
        batches, np.cumsum([0] + [int(getattr(b, name)[-1]) for b in batches[:-1]]))]).astype(np.int64)
    weight = None
    if any(b.flt_weight is not None for b in batches):
        weight = np.concatenate([np.ones(b.flt_tp.shape[0]) if b.flt_weight is None else b.flt_weight for b in batches])
    return TradeBatch(offs("fix_off"), offs("flt_off"), cat("fix_tp"), cat("fix_pay"), cat("flt_tp"), cat("flt_ts"),
                      cat("flt_te"), cat("flt_alpha"), cat("notional"), cat("spread"), cat("fix_sign"), cat("flt_sign"),
                      weight)


def compile_book(trades, value_dt, curve_type: CurveTypes):
    """``(batch, pv_const [n] or None, order)`` for a revaluation on ``curve_type``'s curve.

    ``trades`` is a compiled `TradeBatch` (taken as it is) or a list of `OIS`, `Bond` and single-curve `FRN` objects
    that all discount and project on that curve.  A mixed list becomes ONE batch, grouped OIS, bonds, FRNs: trade
    ``order[j]`` of the list is trade ``j`` of the batch.  ``pv_const`` holds what does not depend on the curve (an
    FRN coupon paid at the value time, `compile_frns`).  A dual-curve FRN, a cross-currency trade or a trade of
    another currency raises `LibError` naming it."""
    if isinstance(trades, TradeBatch):
        if trades.n_trades < 1:
            raise LibError("the batch holds no trade")
        return trades, None, None
    trades = list(trades)
    if not trades:
        raise LibError("no trades to revalue")
    currency = next((c for c, t in BOND_CURVES.items() if t == curve_type), None)
    kinds = {InstrumentTypes.OIS_SWAP: [], InstrumentTypes.BOND: [], InstrumentTypes.FRN: []}
    for i, t in enumerate(trades):
        kind = getattr(t, "derivative_type", None)
        if kind == InstrumentTypes.XCCY_SWAP:
            raise LibError(f"trade {i} ({type(t).__name__}) is a cross-currency trade: two curves per scenario are "
                           "outside the scenario revaluation")
        if kind not in kinds:
            raise LibError(f"trade {i} ({type(t).__name__}) is not an OIS, a Bond or an FRN")
        if kind == InstrumentTypes.FRN and not frn_is_single_curve(t):
            raise LibError(f"trade {i} is a dual-curve FRN (index {t._floating_index.name}): its forwards need a second "
                           "curve per scenario")
        ccy = getattr(t, "_currency", None)
        if ccy != currency or (kind != InstrumentTypes.BOND and t._floating_index != curve_type):
            raise LibError(f"trade {i} ({type(t).__name__}, {getattr(ccy, 'name', ccy)}) is not on the grid's curve "
                           f"{curve_type.name}")
        kinds[kind].append(i)
    pick = lambda idx: [trades[i] for i in idx]
    pieces, order, const = [], [], []
    for kind, compiler in ((InstrumentTypes.OIS_SWAP, compile_ois), (InstrumentTypes.BOND, compile_bonds),
                           (InstrumentTypes.FRN, compile_frns)):
        idx = kinds[kind]
        if not idx:
            continue
        piece = compiler(pick(idx), value_dt)
        if kind == InstrumentTypes.FRN:
            piece, c = piece
            const.append(c)
        else:
            const.append(np.zeros(len(idx)))
        pieces.append(piece)
        order += idx
    const = np.concatenate(const)
    return _concat_batches(pieces), (const if np.any(const != 0.0) else None), np.asarray(order, dtype=np.int64)


def _finish(out, const, order, per_trade, sub_off=None):
    """Add the curve-independent amounts - to the book, or with ``sub_off`` per sub-book in batch order - and put per-trade
    rows back into the caller's order."""
    if const is not None and sub_off is None:
        out["book_pv"] = out["book_pv"] + float(np.sum(const))
    elif const is not None:
        add = np.array([float(np.sum(const[lo:hi])) if np.any(const[lo:hi] != 0.0) else 0.0
                        for lo, hi in zip(sub_off[:-1], sub_off[1:])])
        live = add != 0.0
        out["sub_pv"][live] = out["sub_pv"][live] + add[live, None]
    if per_trade:
        pv = out["pv"] if const is None else out["pv"] + const[None, :]
        if order is not None and not np.array_equal(order, np.arange(order.size)):
            back = np.empty_like(pv)
            back[:, order] = pv
            pv = back
        out["pv"] = pv
    return out


def revalue_on_curves(method, times, dfs, trades, value_dt, per_trade=False, ctx=None, host=False, curve_type=None):
    """PVs of a book under caller-supplied scenario curves: no `ScenarioGrid`, no bootstrap.

    ``method``: an `InterpTypes` member or its value; ``times [K]``: the knot grid shared by all curves (first knot
    t = 0); ``dfs [S, K]``: one row of positive discount factors per scenario - historical curves, stress curves, the
    rows of a `ScenarioGrid`.  ``trades``: see `compile_book` (objects are checked against ``curve_type``, default the
    GBP OIS curve; a `TradeBatch` is taken as it is).  Returns ``{"book_pv": [S]}`` and, with ``per_trade``,
    ``"pv": [S, n]``.  ``host=True`` runs the CPU twin of the kernel (same arithmetic and summation order; no GPU)."""
    method = _interp_value(method)
    book = compile_book(trades, value_dt, curve_type or CurveTypes.GBP_OIS_SONIA)
    return _revalue(_Curves.on_arrays(method, times, dfs, ctx, host), per_trade, book)


@dataclass
class CreditBook:
    """`compile_credit_book`'s result: `compile_book`'s ``batch``, ``pv_const`` and ``order`` plus, in BATCH order, the
    spread times per fixed flow / float coupon, the spread ``z`` and the bucket index per trade, and the bucket labels."""
    batch: TradeBatch
    pv_const: Optional[np.ndarray]
    order: np.ndarray
    fix_tau: np.ndarray
    flt_tau: np.ndarray
    z: np.ndarray
    bucket: np.ndarray
    labels: list


def compile_credit_book(trades, value_dt, curve_type: CurveTypes, spreads, buckets=None) -> CreditBook:
    """A mixed list of `OIS`, `Bond` and single-curve `FRN` objects as ONE batch (`compile_book`: the same lists, the
    same refusals, the same ``order``) with what adr_credit_scenario_pv needs besides it.

    ``spreads``: one per trade of the list (or one number for all) - the z-spread of a bond, the discount margin of an
    FRN, as `BondBook.measures` / `FRNBook.measures` return them; an OIS has none: anything but 0 is refused.
    Spread times: a bond flow's ``(payment_dt - value_dt) / SPREAD_DAYS_IN_YEAR`` (the time of `Bond.z_spread` with
    settlement at the value date), an FRN flow's year fraction from the value date in the FRN's day count (the DM
    time with settlement at the value date), 0 for an OIS.  An FRN coupon paid at the value time (``pv_const``) has
    spread time 0 and stays as it is.

    ``buckets``: one hashable label or None (not shocked) per trade - an issuer, a rating, a sector.  The labels are
    numbered 0 .. G - 1 in order of first appearance and returned as ``labels``; more than 32 raise `LibError`."""
    if isinstance(trades, TradeBatch):
        raise LibError("a compiled TradeBatch carries no dates: the spread times need the Bond and FRN objects")
    trades = list(trades)
    batch, const, order = compile_book(trades, value_dt, curve_type)
    n = len(trades)
    try:
        spreads = np.broadcast_to(np.asarray(spreads, dtype=np.float64), (n,))
    except ValueError:
        raise LibError(f"spreads needs one entry per trade ({n})") from None
    if not np.all(np.isfinite(spreads)):
        raise LibError("spreads must be finite")
    if buckets is None:
        buckets = [None] * n
    buckets = list(buckets)
    if len(buckets) != n:
        raise LibError(f"buckets needs one entry per trade ({n}), not {len(buckets)}")
    def bucketed():                     # the labels to number; an OIS among them is refused where it stands
        for i, lab in enumerate(buckets):
            if lab is None:
                continue
            if trades[i].derivative_type == InstrumentTypes.OIS_SWAP:
                raise LibError(f"trade {i} is an OIS: it carries no credit spread, so its bucket must be None")
            yield lab
    labels, index = _first_appearance(bucketed())
    if len(labels) > _native.CREDIT_MAX_BUCKETS:
        raise LibError(f"{len(labels)} distinct buckets: at most {_native.CREDIT_MAX_BUCKETS} fit one launch")
    fix_tau = np.zeros(batch.fix_tp.shape[0])
    flt_tau = np.zeros(batch.flt_tp.shape[0])
    for j, i in enumerate(order):
        t = trades[i]
        f0, f1 = int(batch.fix_off[j]), int(batch.fix_off[j + 1])
        l0, l1 = int(batch.flt_off[j]), int(batch.flt_off[j + 1])
        if t.derivative_type == InstrumentTypes.OIS_SWAP:
            if spreads[i] != 0.0:
                raise LibError(f"trade {i} is an OIS: it carries no credit spread, so its spread must be 0")
        elif t.derivative_type == InstrumentTypes.BOND:
            tau = [(dt - value_dt) / SPREAD_DAYS_IN_YEAR for dt in t._payment_dts]
            if len(tau) != f1 - f0:
                raise LibError(f"trade {i}: {len(tau)} payment dates for {f1 - f0} compiled flows")
            fix_tau[f0:f1] = tau
        else:
            # compile_frns' times ARE year fractions from the value date in the FRN's day count
            fix_tau[f0:f1] = batch.fix_tp[f0:f1]
            flt_tau[l0:l1] = batch.flt_tp[l0:l1]
    z = np.array([spreads[i] for i in order], dtype=np.float64)
    bucket = np.array([-1 if buckets[i] is None else index[buckets[i]] for i in order], dtype=np.int32)
    return CreditBook(batch, const, order, fix_tau, flt_tau, z, bucket, labels)


def shocked_spreads(labels, shock: Shock) -> np.ndarray:
    """``[G]``: one scenario's spread shocks in DECIMALS from a shock in BASIS POINTS - a float shifts every bucket, a
    dict ``{label: shift}`` the named ones; ``labels`` as `compile_credit_book` returns them."""
    labels = list(labels)
    if isinstance(shock, dict):
        unknown = [k for k in shock if k not in labels]
        if unknown:
            raise LibError(f"no bucket named {unknown} (buckets: {labels})")
        return np.array([shock.get(lab, 0.0) for lab in labels], dtype=np.float64) * 1e-4
    return np.full(len(labels), float(shock) * 1e-4)


def _spread_rows(spread_shocks, G):
    """``spread_shocks`` as [rows, G] decimals, or None where there is nothing to shock."""
    if spread_shocks is None:
        return None if G == 0 else np.zeros((1, G))
    dz = np.atleast_2d(np.asarray(spread_shocks, dtype=np.float64))
    if dz.ndim != 2 or dz.shape[1] != G:
        raise LibError(f"spread_shocks must have shape [n_scenarios, {G}] or [{G}] (one column per bucket), not "
                       f"{list(np.shape(spread_shocks))}")
    return None if G == 0 else dz


def _grid_spread_rows(dz, S, G, with_base):
    """`_spread_rows`' result checked against a grid of ``S`` scenarios; ``with_base`` appends the base pair's row."""
    if dz is not None and dz.shape[0] not in (1, S):
        raise LibError(f"{dz.shape[0]} spread-shock rows for a grid of {S} scenarios: one shared row or one per scenario")
    if with_base and dz is not None:            # the base pair: the unshocked curve with a zero spread shock
        dz = np.vstack([np.broadcast_to(dz, (S, G)), np.zeros((1, G))])
    return dz


def revalue_credit_on_curves(method, times, dfs, spread_shocks, trades, spreads, buckets, value_dt, per_trade=False,
                             ctx=None, host=False, curve_type=None):
    """PVs of a credit book under caller-supplied scenario PAIRS, in one launch of csrc/credit_scenario_pv.hip.

    ``times [K]`` and ``dfs [S, K]`` as `revalue_on_curves` takes them; ``spread_shocks [S, G]`` in decimals, one column
    per bucket label (`shocked_spreads` makes a row).  A single row, ``dfs [K]`` or ``spread_shocks [G]``, is shared
    by all scenarios; ``spread_shocks=None`` shocks no spread.  ``trades``, ``spreads`` and ``buckets``: see
    `compile_credit_book`.  Returns ``{"book_pv": [S], "labels": [...]}`` and, with ``per_trade``, ``"pv": [S, n]`` in
    the list's order.  ``host=True`` runs the CPU twin of the kernel (same arithmetic and summation order; no GPU)."""
    method = _interp_value(method)
    book = compile_credit_book(trades, value_dt, curve_type or CurveTypes.GBP_OIS_SONIA, spreads, buckets)
    dz = _spread_rows(spread_shocks, len(book.labels))
    return _revalue(_Curves.on_arrays(method, times, dfs, ctx, host), per_trade, book, dz)


def _gather_offsets(off, perm):
    """``(offsets of the rows perm of a CSR array, gather index of their entries)``."""
    off = np.asarray(off, dtype=np.int64)
    length = (off[1:] - off[:-1])[perm]
    new_off = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    idx = np.repeat(off[:-1][perm] - new_off[:-1], length) + np.arange(int(new_off[-1]), dtype=np.int64)
    return new_off, idx


def _permute_batch(batch: TradeBatch, perm: np.ndarray):
    """``(batch with trade j = trade perm[j] of ``batch``, fixed-flow gather index, float-coupon gather index)``."""
    fix_off, fi = _gather_offsets(batch.fix_off, perm)
    flt_off, li = _gather_offsets(batch.flt_off, perm)
    f = lambda name, idx: np.asarray(getattr(batch, name), dtype=np.float64)[idx]
    weight = None if batch.flt_weight is None else np.asarray(batch.flt_weight, dtype=np.float64)[li]
    return TradeBatch(fix_off, flt_off, f("fix_tp", fi), f("fix_pay", fi), f("flt_tp", li), f("flt_ts", li), f("flt_te", li),
                      f("flt_alpha", li), f("notional", perm), f("spread", perm), f("fix_sign", perm), f("flt_sign", perm),
                      weight), fi, li


@dataclass
class SubBooks:
    """`split_sub_books`' result: the batch with every sub-book's trades consecutive, ``pv_const`` and ``order`` to match
    (`compile_book`), the labels in order of first appearance, ``sub_off [B + 1]`` (sub-book ``b`` is the trades
    ``sub_off[b] .. sub_off[b + 1]`` of the batch) and, where the batch was re-ordered, the gather indices of its trades,
    fixed flows and float coupons (None: left as it was)."""
    batch: TradeBatch
    pv_const: Optional[np.ndarray]
    order: Optional[np.ndarray]
    labels: list
    sub_off: np.ndarray
    perm: Optional[np.ndarray] = None
    fix_idx: Optional[np.ndarray] = None
    flt_idx: Optional[np.ndarray] = None


def split_sub_books(batch: TradeBatch, pv_const, order, keys) -> SubBooks:
    """Cut a compiled book (`compile_book`'s triple) into sub-books by ``keys``, one hashable value per trade of the
    CALLER's input, labelled in order of first appearance.

    From an object list (``order`` given) the batch is stably sorted by label after `compile_book`'s own grouping, so a
    sub-book's trades keep the order `compile_book` gives that sub-book alone.  A `TradeBatch` (``order`` None) is taken
    as it is and must already hold each label's trades consecutively: `LibError` names the first label that reappears."""
    keys = list(keys)
    n = batch.n_trades
    if len(keys) != n:
        raise LibError(f"keys needs one entry per trade ({n}), not {len(keys)}")
    labels, index = _first_appearance(keys)
    if order is None:
        code = np.array([index[k] for k in keys], dtype=np.int64)
        back = np.nonzero(code[1:] < code[:-1])[0]
        # labels are numbered by first appearance, so a consecutive layout is a non-decreasing one
        if back.size:
            j = int(back[0]) + 1
            raise LibError(f"the batch does not hold the trades of sub-book {keys[j]!r} consecutively: it reappears at trade "
                           f"{j}; sort the batch by key, or pass the trade objects")
        perm = None
    else:
        code = np.array([index[keys[i]] for i in order], dtype=np.int64)
        perm = np.argsort(code, kind="stable")
        code = code[perm]
        if np.array_equal(perm, np.arange(n)):
            perm = None
    sub_off = np.searchsorted(code, np.arange(len(labels) + 1), side="left").astype(np.int64)
    if perm is None:
        return SubBooks(batch, pv_const, order, labels, sub_off)
    batch, fi, li = _permute_batch(batch, perm)
    return SubBooks(batch, None if pv_const is None else pv_const[perm], order[perm], labels, sub_off, perm, fi, li)


@dataclass
class _Curves:
    """Where the discount rows of a revaluation come from, as the `_native` scenario entries take them: host arrays priced
    on the device (``suffix`` "", ``head`` the scheme, ``times`` and ``dfs``), the same on the host twin ("_host", no
    context) or a `CurveSet` read in place ("_set", ``head`` the set)."""
    suffix: str
    head: tuple
    ctx: Optional[_native.Context] = None          # None on the device: the default context, made when the call is

    @classmethod
    def on_arrays(cls, method, times, dfs, ctx, host):
        return cls("_host" if host else "", (method, times, dfs), ctx)

    def call(self, entry, batch, dz, per_trade_data, sub_off, per_trade):
        """The entry ``entry`` of this kind; the optional groups are sequences, empty where the entry has none."""
        fn = getattr(_native, entry + self.suffix)
        if self.suffix == "_host":
            return fn(*self.head, *dz, batch, *per_trade_data, *sub_off, per_trade=per_trade)
        ctx = self.ctx or _native.default_context()
        with _native.DeviceTrades(ctx, batch) as dev:
            return fn(ctx, *self.head, *dz, dev, *per_trade_data, *sub_off, per_trade=per_trade)


def _revalue(curves: _Curves, per_trade, book, dz=None, *keys):
    """One revaluation of a compiled book, in one launch: ``book`` is `compile_book`'s triple (``dz`` stays None) or a
    `CreditBook` (``dz`` holds its spread-shock rows, `_spread_rows`), cut into sub-books where ``keys`` is given
    (`split_sub_books`)."""
    credit = isinstance(book, CreditBook)
    batch, const, order = (book.batch, book.pv_const, book.order) if credit else book
    data = [book.z, book.bucket, book.fix_tau, book.flt_tau] if credit else []
    sub_off = ()
    if keys:
        sb = split_sub_books(batch, const, order, *keys)
        batch, const, order, sub_off = sb.batch, sb.pv_const, sb.order, (sb.sub_off,)
        if credit and sb.perm is not None:          # the re-ordered batch's order
            data = [book.z[sb.perm], book.bucket[sb.perm], book.fix_tau[sb.fix_idx], book.flt_tau[sb.flt_idx]]
    entry = ("credit_scenario_subbook_pv" if keys else "credit_scenario_pv") if credit else \
        ("scenario_subbook_pv" if keys else "scenario_pv")
    out = curves.call(entry, batch, [dz] if credit else [], data, sub_off, per_trade)
    if credit:
        out["buckets" if keys else "labels"] = book.labels
    if keys:
        out["labels"] = sb.labels
    return _finish(out, const, order, per_trade, *sub_off)


def revalue_on_curves_sub_books(method, times, dfs, trades, keys, value_dt, per_trade=False, ctx=None, host=False,
                                curve_type=None):
    """`revalue_on_curves` per sub-book, in ONE launch: ``keys`` holds one hashable value per trade (a desk, a
    counterparty, an account).  Returns ``{"labels": [...], "sub_pv": [B, S]}`` - the labels in order of first appearance,
    row ``b`` the PV vector of sub-book ``labels[b]``, bit for bit what `revalue_on_curves` gives on that sub-book alone
    - and, with ``per_trade``, ``"pv": [S, n]`` in the caller's order.  A `TradeBatch` must hold each label's trades
    consecutively (`split_sub_books`)."""
    method = _interp_value(method)
    book = compile_book(trades, value_dt, curve_type or CurveTypes.GBP_OIS_SONIA)
    return _revalue(_Curves.on_arrays(method, times, dfs, ctx, host), per_trade, book, None, keys)


def revalue_credit_on_curves_sub_books(method, times, dfs, spread_shocks, trades, spreads, buckets, keys, value_dt,
                                       per_trade=False, ctx=None, host=False, curve_type=None):
    """`revalue_credit_on_curves` per sub-book, in ONE launch (``keys``: see `revalue_on_curves_sub_books`; a sub-book
    may cut across credit buckets).  Returns ``{"labels": [...], "sub_pv": [B, S], "buckets": [...]}`` - ``buckets`` the
    credit-bucket labels, one column of ``spread_shocks`` each - and, with ``per_trade``, ``"pv": [S, n]``."""
    method = _interp_value(method)
    book = compile_credit_book(trades, value_dt, curve_type or CurveTypes.GBP_OIS_SONIA, spreads, buckets)
    dz = _spread_rows(spread_shocks, len(book.labels))
    return _revalue(_Curves.on_arrays(method, times, dfs, ctx, host), per_trade, book, dz, keys)


def shocked_breakevens(curve, shock: Shock) -> np.ndarray:
    """``[P]``: an inflation curve's breakeven rates under a shock in BASIS POINTS - a float shifts every pillar, a dict
    ``{tenor: shift}`` the named ones, tenors as ``to_tenor(curve.swap_times)`` labels them.  An inflation curve has no
    bootstrap (its nodes are ``(T_k, (1 + b_k) ** T_k)``), so the shocked rates ARE the shocked curve."""
    _, T, b = inflation_inputs(curve)
    if isinstance(shock, dict):
        tenors = to_tenor(list(T))
        unknown = sorted(set(shock) - set(tenors))
        if unknown:
            raise LibError(f"no pillar named {unknown} on the inflation curve (pillars: {tenors})")
        return b + np.array([shock.get(t, 0.0) for t in tenors], dtype=np.float64) * 1e-4
    return b + float(shock) * 1e-4


def yoy_book_arrays(swaps_or_book, value_dt):
    """``(fixed, coupons)`` for adr_yoy_scenario_pv: from a list of `YoYInflationSwap` (compiled against ``value_dt``)
    or from a ready pair ``((fix_off, fix_tp, fix_pay) or None, coupon dict or None)``, which is taken as it is."""
    if isinstance(swaps_or_book, tuple) and len(swaps_or_book) == 2 and not hasattr(swaps_or_book[0], "derivative_type"):
        return swaps_or_book
    swaps = list(swaps_or_book)
    if not swaps:
        raise LibError("no swaps to revalue")
    return compile_yoy_fixed_legs(swaps, value_dt), compile_yoy_coupons(swaps, value_dt)


def revalue_yoy_on_curves(disc_method, times, dfs, infl_method, T, b, swaps_or_book, value_dt, per_trade=False, ctx=None,
                          host=False):
    """PVs of a YoY inflation swap book under caller-supplied scenario PAIRS, in one launch of csrc/yoy_scenario_pv.hip.

    ``disc_method`` / ``infl_method``: `InterpTypes` members or their values; ``times [K]`` and ``dfs [S, K]`` the
    discount scenarios as `revalue_on_curves` takes them, ``T [P]`` and ``b [S, P]`` the inflation pillars and the
    breakeven rates per scenario (`shocked_breakevens`, or a history of curves).  A single row, ``dfs [K]`` or
    ``b [P]``, means that curve is not shocked and is shared by all scenarios.  ``swaps_or_book``: `YoYInflationSwap`
    objects or compiled arrays (`yoy_book_arrays`).  Returns ``{"book_pv": [S]}`` and, with ``per_trade``,
    ``"pv": [S, n]``.  ``host=True`` runs the CPU twin of the kernel (same arithmetic and summation order; no GPU)."""
    dm, im = _disc_infl_methods(disc_method, infl_method)
    fixed, coupons = yoy_book_arrays(swaps_or_book, value_dt)
    if host:
        return _native.yoy_scenario_pv_host(dm, times, dfs, im, T, b, fixed, coupons, per_trade=per_trade)
    return _native.yoy_scenario_pv(ctx or _native.default_context(), dm, times, dfs, im, T, b, fixed, coupons,
                                   per_trade=per_trade)


@dataclass
class YoYSubBooks:
    """`split_yoy_sub_books`' result: the compiled arrays with every sub-book's swaps consecutive, the labels in order of
    first appearance, ``sub_off [B + 1]`` and ``perm`` (swap ``j`` of the arrays is swap ``perm[j]`` of the caller's; None:
    left as it was)."""
    fixed: Optional[tuple]
    coupons: Optional[dict]
    labels: list
    sub_off: np.ndarray
    perm: Optional[np.ndarray] = None


def split_yoy_sub_books(fixed, coupons, keys) -> YoYSubBooks:
    """Cut a compiled YoY book (`yoy_book_arrays`' pair) into sub-books by ``keys``, one hashable value per swap,
    labelled in order of first appearance.  The swaps are stably sorted by label, so a sub-book's swaps keep the order
    they have in the caller's list - the order the whole-book call gives that sub-book alone."""
    keys = list(keys)
    if fixed is None and coupons is None:
        raise LibError("neither fixed legs nor YoY coupons")
    n = (np.asarray(fixed[0]) if fixed is not None else np.asarray(coupons["cpn_off"])).size - 1
    if len(keys) != n:
        raise LibError(f"keys needs one entry per swap ({n}), not {len(keys)}")
    labels, index = _first_appearance(keys)
    code = np.array([index[k] for k in keys], dtype=np.int64)
    perm = np.argsort(code, kind="stable")
    sub_off = np.searchsorted(code[perm], np.arange(len(labels) + 1), side="left").astype(np.int64)
    if np.array_equal(perm, np.arange(n)):
        return YoYSubBooks(fixed, coupons, labels, sub_off)
    if fixed is not None:
        off, idx = _gather_offsets(fixed[0], perm)
        fixed = (off, np.asarray(fixed[1], dtype=np.float64)[idx], np.asarray(fixed[2], dtype=np.float64)[idx])
    if coupons is not None:
        off, idx = _gather_offsets(coupons["cpn_off"], perm)
        coupons = dict({k: np.asarray(coupons[k], dtype=np.float64)[idx] for k in _native.YOY_FIELDS}, cpn_off=off)
    return YoYSubBooks(fixed, coupons, labels, sub_off, perm)


def _finish_yoy_sub_books(out, sb: YoYSubBooks, per_trade):
    """The labels, and the per-swap rows back in the caller's order."""
    out["labels"] = sb.labels
    if per_trade and sb.perm is not None:
        back = np.empty_like(out["pv"])
        back[:, sb.perm] = out["pv"]
        out["pv"] = back
    return out


def revalue_yoy_on_curves_sub_books(disc_method, times, dfs, infl_method, T, b, swaps_or_book, keys, value_dt, per_trade=False,
                                    ctx=None, host=False):
    """`revalue_yoy_on_curves` per sub-book, in ONE launch: ``keys`` holds one hashable value per swap (a desk, a
    counterparty, an account).  Returns ``{"labels": [...], "sub_pv": [B, S]}`` - the labels in order of first appearance,
    row ``b`` the PV vector of sub-book ``labels[b]``, bit for bit what `revalue_yoy_on_curves` gives on that sub-book
    alone - and, with ``per_trade``, ``"pv": [S, n]`` in the caller's order."""
    dm, im = _disc_infl_methods(disc_method, infl_method)
    sb = split_yoy_sub_books(*yoy_book_arrays(swaps_or_book, value_dt), keys)
    if host:
        out = _native.yoy_scenario_subbook_pv_host(dm, times, dfs, im, T, b, sb.fixed, sb.coupons, sb.sub_off, per_trade=per_trade)
    else:
        out = _native.yoy_scenario_subbook_pv(ctx or _native.default_context(), dm, times, dfs, im, T, b, sb.fixed, sb.coupons,
                                              sb.sub_off, per_trade=per_trade)
    return _finish_yoy_sub_books(out, sb, per_trade)


def _tail(pnl, level):
    pnl = np.sort(np.asarray(pnl, dtype=np.float64).reshape(-1))
    if pnl.size == 0 or not 0.0 < level < 1.0:
        raise ValueError("a P&L vector and a confidence level inside (0, 1) are needed")
    # (1 - level) * S in floating point can land a hair above an integer (0.05 * 20 != 1 exactly)
    k = int(np.ceil(round((1.0 - level) * pnl.size, 9)))
    return pnl[:max(1, k)]


def historical_var(pnl, level: float = 0.99) -> float:
    """Historical-simulation value at risk: minus the ``k``-th smallest P&L, ``k = ceil((1 - level) * S)`` (at least
    1) - no interpolation between order statistics.  A loss is a positive VaR."""
    return float(-_tail(pnl, level)[-1])


def expected_shortfall(pnl, level: float = 0.99) -> float:
    """Minus the mean of the ``ceil((1 - level) * S)`` smallest P&Ls - the tail `historical_var` ends at, that
    scenario included."""
    return float(-np.mean(_tail(pnl, level)))


def tail_count(level: float, n_pnl: int) -> int:
    """``k`` of `historical_var` / `expected_shortfall` for ``n_pnl`` P&L values: ``ceil((1 - level) * n_pnl)``, at least 1."""
    if n_pnl < 1 or not 0.0 < level < 1.0:
        raise ValueError("a P&L vector and a confidence level inside (0, 1) are needed")
    return max(1, int(np.ceil(round((1.0 - level) * n_pnl, 9))))


def _tail_args(rows, base_col, level, min_rows):
    """``(rows [B, S_tot] as float64, the P&L values per row, their tail count)`` after the check `tail_measures` and
    `allocate_tail` share."""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    if rows.ndim != 2 or rows.shape[0] < min_rows or not -1 <= base_col < rows.shape[1]:
        raise LibError(f"rows must have shape [n_rows, n_columns] and base_col be -1 or a column, not {list(rows.shape)}, {base_col}")
    m = rows.shape[1] - (1 if base_col >= 0 else 0)
    return rows, m, tail_count(level, m)


def tail_measures(rows, level: float = 0.99, base_col: int = -1, host: bool = False, ctx=None):
    """``(var [B], es [B])``: `historical_var` and `expected_shortfall` of every row of ``rows [B, S]`` in one kernel
    (adr_scenario_tail; ``host=True``: its CPU twin, the same bits).  ``base_col >= 0``: the P&L of a row is every OTHER
    column minus that column (the base curve priced as one more scenario); -1: the rows already are P&L.  ``es`` adds the
    tail in ascending order, so it agrees with `expected_shortfall` (NumPy's pairwise mean) to rounding, not bit for
    bit; ``var`` is the same order statistic.  A row holding a NaN gives NaN.  Rows wider than
    ``_native.SCENARIO_TAIL_MAX`` P&L values do not fit the kernel's LDS and are done by NumPy per row."""
    rows, m, k = _tail_args(rows, base_col, level, 0)
    if m > _native.SCENARIO_TAIL_MAX:
        pnl = rows if base_col < 0 else np.delete(rows, base_col, axis=1) - rows[:, base_col:base_col + 1]
        out = np.array([[historical_var(r, level), expected_shortfall(r, level)] if not np.any(np.isnan(r)) else [np.nan, np.nan]
                        for r in pnl]).reshape(-1, 2)
        return out[:, 0].copy(), out[:, 1].copy()
    if host:
        return _native.scenario_tail_host(rows, k, base_col)
    return _native.scenario_tail(ctx or _native.default_context(), rows, k, base_col)


def _allocate_tail_numpy(rows, k, base_col):
    """adr_scenario_tail_alloc's rule in NumPy, sum for sum: the same bits as the kernel and its host twin."""
    pnl = rows if base_col < 0 else np.delete(rows, base_col, axis=1) - rows[:, base_col:base_col + 1]
    B, m = pnl.shape
    slots = np.zeros((64, m))
    for r in range(B):                                  # row r to slot r % 64, in row order from 0.0
        slots[r % 64] = slots[r % 64] + pnl[r]
    h = 32
    while h >= 1:
        slots[:h] = slots[:h] + slots[h:2 * h]
        h //= 2
    tot = slots[0]
    if np.any(np.isnan(tot)):
        return {"var": np.nan, "es": np.nan, "comp_var": np.full(B, np.nan), "comp_es": np.full(B, np.nan)}
    bits = tot.view(np.int64)
    key = bits ^ ((bits >> 63) & np.int64(0x7FFFFFFFFFFFFFFF))       # the tail kernel's total order: -0.0 before +0.0
    order = np.lexsort((np.arange(m), key))[:k]
    es, comp = 0.0, np.zeros(B)
    for e in order:
        es = es + tot[e]
        comp = comp + pnl[:, e]
    return {"var": float(-tot[order[-1]]), "es": float(-es / float(k)), "comp_var": -pnl[:, order[-1]],
            "comp_es": -comp / float(k)}


def allocate_tail(rows, level: float = 0.99, base_col: int = -1, host: bool = False, ctx=None):
    """The firm's tail and how much of it every row carries - the Euler allocation of VaR and expected shortfall to the
    desks, in one chain of kernels (adr_scenario_tail_alloc; ``host=True``: its CPU twin, the same bits).

    ``rows [B, S]``: one row per desk, as `pnl_sub_books` or `combine_sub_book_rows` give them; ``base_col`` as in
    `tail_measures`.  With ``k = tail_count(level, S)`` and the scenarios ordered by the FIRM's P&L (the column sums in a
    fixed order; ties go to the earlier scenario), ``var`` and ``es`` are the firm's `historical_var` and expected
    shortfall, ``comp_var [B]`` every row's loss in the firm's ``k``-th worst scenario and ``comp_es [B]`` its mean loss
    over the firm's ``k`` worst: ``comp_es`` sums to ``es`` and ``comp_var`` to ``var`` up to rounding.  A NaN anywhere
    gives NaN everywhere.  Rows wider than ``_native.SCENARIO_ALLOC_MAX`` P&L values do not fit the kernel's LDS and are
    done by NumPy under the same rule."""
    rows, m, k = _tail_args(rows, base_col, level, 1)
    rows = np.ascontiguousarray(rows)
    if m > _native.SCENARIO_ALLOC_MAX:
        return _allocate_tail_numpy(rows, k, base_col)
    if host:
        return _native.scenario_tail_alloc_host(rows, k, base_col)
    return _native.scenario_tail_alloc(ctx or _native.default_context(), rows, k, base_col)


def combine_sub_book_rows(parts):
    """One row per label across several sub-book results: ``parts`` is a list of ``(labels, rows [B_i, S])`` - the
    ``labels`` and ``sub_pv`` (or P&L rows) of the rates, credit and YoY sub-book calls on the same scenarios.  Returns
    ``{"labels": [...], "rows": [B, S]}`` with the labels in order of first appearance across the parts; a label's row is
    its first part's row with the later parts' rows added in list order, so a label found in one part only keeps that
    part's bits."""
    checked, width = [], None
    for i, (labs, rows) in enumerate(parts):
        rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
        labs = list(labs)
        if rows.ndim != 2 or rows.shape[0] != len(labs):
            raise LibError(f"part {i}: {len(labs)} labels for rows of shape {list(rows.shape)}")
        if width is None:
            width = rows.shape[1]
        if rows.shape[1] != width:
            raise LibError(f"part {i} has {rows.shape[1]} columns, the parts before it {width}: the scenarios must be the same")
        if len(set(labs)) != len(labs):
            raise LibError(f"part {i} names a label twice")
        checked += zip(labs, rows)
    if not checked:
        raise LibError("no parts to combine")
    labels, index = _first_appearance(lab for lab, _ in checked)
    out = [None] * len(labels)
    for lab, row in checked:
        j = index[lab]
        out[j] = row.copy() if out[j] is None else out[j] + row
    return {"labels": labels, "rows": np.stack(out)}


class ScenarioGrid:
    """``len(shocks)`` shocked versions of ``model.curves[curve_name]`` resident on the GPU."""

    def __init__(self, model, curve_name: str, shocks: Iterable[Shock], with_gamma: bool = True, ctx=None):
        if curve_name not in model._curve_params_dict:
            raise ValueError(f"No stored parameters found for curve '{curve_name}'")
        params = model._curve_params_dict[curve_name]
        self.model, self.curve_name = model, curve_name
        self.curve = getattr(model.curves, curve_name)
        method = _interp_value(self.curve._interp_type)
        self.shocks = list(shocks)
        # OISCurve stores quote / 100 as the swap's fixed coupon (models.py build_curve); same division here
        self.rates = np.array([[px / 100.0 for px in shocked_quotes(params["px_list"], params["tenor_list"], s)]
                               for s in self.shocks], dtype=np.float64).reshape(len(self.shocks), -1)
        base = build_engine_curve(self.curve.swap_rates, self.curve.swap_times, self.curve.year_fracs,
                                  with_hessian=with_gamma)
        self._ctx = ctx or _native.default_context()
        self._plan = _native.CurvePlan(self._ctx, method, base)
        self._set = self._plan.build(self.rates)
        self.base = base

    def __len__(self):
        return len(self.shocks)

    def device_curve(self, i: int):
        return self._set[i]

    def download(self, i: int):
        """Scenario ``i``'s ``dfs, jac, hess`` - the reference's cache dict for the shocked curve."""
        return self._set.download(i)

    def price(self, derivatives, reqs=(RequestTypes.VALUE,), aggregate: bool = False):
        """Price the trades under every scenario.

        Returns a dict of arrays with a leading scenario axis: ``pv [S, n]``, ``delta [S, n, P]``,
        ``gamma [S, n, P, P]`` (per request), or ``agg_*`` sums over the trades when ``aggregate``."""
        reqs = set(reqs)
        batch = compile_ois(list(derivatives), self.curve._value_dt)
        outs = []
        with _native.DeviceTrades(self._ctx, batch) as trades:
            for i in range(len(self)):
                outs.append(_native.price(self._ctx, self._set[i], trades,
                                          want_value=RequestTypes.VALUE in reqs,
                                          want_delta=RequestTypes.DELTA in reqs,
                                          want_gamma=RequestTypes.GAMMA in reqs,
                                          per_trade=not aggregate, aggregate=aggregate))
        keys = outs[0].keys() if outs else ()
        return {k: np.stack([np.asarray(o[k]) for o in outs]) for k in keys}

    def _dfs(self):
        """The scenarios' discount factors [S, K] on the host (downloaded once)."""
        if getattr(self, "_dfs_host", None) is None:
            self._dfs_host = np.stack([self._set.download(i)[0] for i in range(len(self))])
        return self._dfs_host

    def _with_base(self):
        """``(times, dfs [S + 1, K])``: the scenarios' rows with the base curve (the host builder's) appended as one more."""
        return self.base.times, np.vstack([self._dfs(), self.base.dfs[None, :]])

    def _curves(self, with_base) -> _Curves:
        """The set read in place, or with ``with_base`` the host rows of `_with_base`."""
        if with_base:
            return _Curves("", (self.curve._interp_type.value, *self._with_base()), self._ctx)
        return _Curves("_set", (self._set,), self._ctx)

    def _book(self, trades):
        return compile_book(trades, self.curve._value_dt, CurveTypes[self.curve_name])

    def _credit_book(self, trades, spreads, buckets, spread_shocks, with_base):
        """``(credit book, spread-shock rows)`` for the grid's scenarios, with ``with_base`` those of the base pair too."""
        book = compile_credit_book(trades, self.curve._value_dt, CurveTypes[self.curve_name], spreads, buckets)
        return book, _grid_spread_rows(_spread_rows(spread_shocks, len(book.labels)), len(self), len(book.labels), with_base)

    def revalue(self, trades, per_trade: bool = False):
        """The book's PV under every scenario, in ONE launch on the grid's own discount factors (`price` makes a
        launch per scenario and needs OIS): ``{"book_pv": [S]}`` and, with ``per_trade``, ``"pv": [S, n]``.

        ``trades``: a list of `OIS`, `Bond` and single-curve `FRN` objects of the grid's curve (a mixed list is one
        batch) or a compiled `TradeBatch`; see `compile_book` for what is refused.  Only discount factors are read, so
        ``ScenarioGrid(..., with_gamma=False)`` is the cheaper grid to feed it (the builder still makes Jacobians)."""
        return _revalue(self._curves(False), per_trade, self._book(trades))

    def pnl(self, trades) -> np.ndarray:
        """``[S]``: the book's PV under each scenario minus its PV on the unshocked curve.  The base curve
        (``self.base.dfs``, the host builder's) is priced by the same launch as one more scenario row, so the
        difference carries no noise between kernels: a zero shock whose curve has the base curve's bits gives 0."""
        book = _revalue(self._curves(True), False, self._book(trades))["book_pv"]
        return book[:-1] - book[-1]

    def revalue_credit(self, trades, spreads, buckets=None, spread_shocks=None, per_trade: bool = False):
        """`revalue` for a credit book: bonds discounted at their z-spreads, FRNs at their discount margins, and
        scenario ``s`` pairs the grid's curve ``s`` with the spread shocks ``spread_shocks[s]``.

        ``spreads`` and ``buckets``: one per trade, see `compile_credit_book`.  ``spread_shocks``: ``[S, G]`` decimals,
        one column per bucket in order of first appearance (`shocked_spreads` makes a row from basis points), one
        shared row ``[G]``, or None (curve shocks only).  The grid's curves are read where the device builder left
        them.  Returns ``{"book_pv": [S], "labels": [...]}`` and, with ``per_trade``, ``"pv": [S, n]``."""
        return _revalue(self._curves(False), per_trade, *self._credit_book(trades, spreads, buckets, spread_shocks, False))

    def pnl_credit(self, trades, spreads, buckets=None, spread_shocks=None) -> np.ndarray:
        """``[S]``: the credit book's PV under each (curve, spread shock) pair minus its PV on the unshocked curve with
        unshocked spreads.  As in `pnl`, the base pair is one more row of the same launch: a zero curve shock with a
        zero spread shock gives exactly 0."""
        book = _revalue(self._curves(True), False,
                        *self._credit_book(trades, spreads, buckets, spread_shocks, True))["book_pv"]
        return book[:-1] - book[-1]

    def revalue_sub_books(self, trades, keys, per_trade: bool = False):
        """`revalue` per sub-book, in the SAME single launch: ``keys`` holds one hashable value per trade (a desk, a
        counterparty, a margin account).  Returns ``{"labels": [...], "sub_pv": [B, S]}``: the labels in order of first
        appearance, row ``b`` the PV vector of sub-book ``labels[b]`` - bit for bit `revalue`'s ``book_pv`` on that
        sub-book alone, ready for `historical_var` - and, with ``per_trade``, ``"pv": [S, n]`` in the caller's order.
        A `TradeBatch` must hold each label's trades consecutively (`split_sub_books`)."""
        return _revalue(self._curves(False), per_trade, self._book(trades), None, keys)

    def pnl_sub_books(self, trades, keys) -> np.ndarray:
        """``[B, S]``: `pnl` per sub-book (rows in the order of `revalue_sub_books`' labels), the base curve priced by
        the same launch as one more scenario: a zero shock gives exactly 0 in every sub-book."""
        sub = _revalue(self._curves(True), False, self._book(trades), None, keys)["sub_pv"]
        return sub[:, :-1] - sub[:, -1:]

    def sub_book_var_es(self, trades, keys, level: float = 0.99):
        """``{"labels": [...], "var": [B], "es": [B]}`` straight from the trades: the sub-book launch and the tail kernel
        in one chain, so the ``[B, S]`` P&L matrix never leaves the device.  The P&L is `pnl_sub_books`' (scenario minus
        base curve; what does not depend on the curve cancels and is not added), ``var`` and ``es`` are `tail_measures`'."""
        sb = split_sub_books(*self._book(trades), keys)
        S = len(self)
        if S > _native.SCENARIO_TAIL_MAX:
            raise LibError(f"{S} scenarios: at most {_native.SCENARIO_TAIL_MAX} fit the tail kernel; use pnl_sub_books and "
                           "tail_measures")
        with _native.DeviceTrades(self._ctx, sb.batch) as dev:
            var, es = _native.scenario_subbook_var_es(self._ctx, self.curve._interp_type.value, *self._with_base(), dev,
                                                      sb.sub_off, tail_count(level, S), base_col=S)
        return {"labels": sb.labels, "var": var, "es": es}

    def revalue_credit_sub_books(self, trades, spreads, keys, buckets=None, spread_shocks=None, per_trade: bool = False):
        """`revalue_credit` per sub-book in one launch; ``keys`` as in `revalue_sub_books` (a sub-book may cut across
        credit buckets).  Returns ``{"labels": [...], "sub_pv": [B, S], "buckets": [...]}`` - ``buckets`` the credit-bucket
        labels, one column of ``spread_shocks`` each - and, with ``per_trade``, ``"pv": [S, n]``."""
        return _revalue(self._curves(False), per_trade,
                        *self._credit_book(trades, spreads, buckets, spread_shocks, False), keys)

    def pnl_credit_sub_books(self, trades, spreads, keys, buckets=None, spread_shocks=None) -> np.ndarray:
        """``[B, S]``: `pnl_credit` per sub-book, the base pair priced by the same launch as one more row."""
        sub = _revalue(self._curves(True), False,
                       *self._credit_book(trades, spreads, buckets, spread_shocks, True), keys)["sub_pv"]
        return sub[:, :-1] - sub[:, -1:]

    # ---------------------------------------------------------------------------------------------- delta-gamma P&L
    def shocks_bp(self) -> np.ndarray:
        """``[S, P]``: the grid's shocks as moves of the par quotes in basis points (quotes are in percent: 100 bp per
        unit), from the shocks themselves - what `ladder_pnl` takes beside the curve's ladders."""
        return shock_matrix_bp(self.model._curve_params_dict[self.curve_name]["tenor_list"], self.shocks, 100.0)

    def _engine(self):
        from .engine import Engine
        if getattr(self, "_ladder_engine", None) is None:
            self._ladder_engine = Engine(self.model)
        return self._ladder_engine

    def pnl_delta_gamma_sub_books(self, trades, keys, parts: bool = False) -> dict:
        """`pnl_sub_books` without the revaluation: every desk's ladders on the base curve (`price_sub_books`, one launch)
        times the grid's shocks (`ladder_pnl`, one kernel).  Returns `delta_gamma_sub_books`' dict: ``{"labels", "pnl"
        [B, S], "pv", "delta", "gamma", "tenors"}`` plus ``"delta_pnl"`` and ``"gamma_pnl"`` with ``parts``; the labels and
        rows are in `pnl_sub_books`' order."""
        return delta_gamma_sub_books(self._engine(), self.curve, trades, keys, self.shocks_bp(), parts=parts,
                                     curve_type=CurveTypes[self.curve_name])

    def pnl_delta_gamma(self, trades) -> np.ndarray:
        """``[S]``: the book's delta-gamma P&L under the grid's shocks - `pnl` to second order in the shocks, from one
        ladder launch instead of a revaluation (the sub-book form with one key, its row)."""
        trades = trades if isinstance(trades, TradeBatch) else list(trades)
        n = trades.n_trades if isinstance(trades, TradeBatch) else len(trades)
        return self.pnl_delta_gamma_sub_books(trades, [0] * n)["pnl"][0]

    def explain_sub_books(self, trades, keys) -> dict:
        """P&L explain per desk and scenario: ``{"labels", "full", "delta_pnl", "gamma_pnl", "unexplained"}``, all
        ``[B, S]`` - ``full`` is `pnl_sub_books`' full revaluation, the parts are `pnl_delta_gamma_sub_books`', and
        ``unexplained = full - (delta_pnl + gamma_pnl)``: third order in the shocks where the ladders describe the book."""
        trades = trades if isinstance(trades, TradeBatch) else list(trades)
        keys = list(keys)
        sub = _revalue(self._curves(True), False, self._book(trades), None, keys)         # `pnl_sub_books`, with its labels
        full = sub["sub_pv"][:, :-1] - sub["sub_pv"][:, -1:]
        dg = self.pnl_delta_gamma_sub_books(trades, keys, parts=True)
        assert dg["labels"] == sub["labels"] and full.shape == dg["pnl"].shape, "the two routes order the desks differently"
        return {"labels": sub["labels"], "full": full, "delta_pnl": dg["delta_pnl"], "gamma_pnl": dg["gamma_pnl"],
                "unexplained": full - (dg["delta_pnl"] + dg["gamma_pnl"])}

    def _ladder_curve(self):
        """The base curve with its Jacobian and Hessian on the grid's context, uploaded once."""
        if getattr(self, "_base_dev", None) is None:
            base = self.base                # a grid built with with_gamma=False has no Hessian: the host builder makes one
            if base.hess is None:
                base = build_engine_curve(self.curve.swap_rates, self.curve.swap_times, self.curve.year_fracs)
            self._base_dev = _native.DeviceCurve(self._ctx, self.curve._interp_type.value, base.times, base.dfs, base.jac, base.hess)
        return self._base_dev

    def sub_book_delta_gamma_var_es(self, trades, keys, level: float = 0.99) -> dict:
        """``{"labels": [...], "var": [B], "es": [B]}`` of the delta-gamma P&L straight from the trades: the ladder launch
        (adr_subbook_ladders_dev), the P&L kernel (adr_ladder_pnl_dev) and the tail kernel (adr_scenario_tail_dev) in one
        chain on one stream, so neither the ladders nor the ``[B, S]`` matrix leave the device.  ``var`` and ``es`` are
        `tail_measures`' of `pnl_delta_gamma_sub_books`' ``pnl``, bit for bit.  A book holding a trade with a ratio node
        (a payment lag, a per-coupon notional) is refused: the chain has no pricer for it.  The buffers are torch tensors;
        where torch brings a HIP runtime of its own, import torch before the first call into this library, as the tools do."""
        import torch
        sb = split_sub_books(*self._book(trades), keys)
        S = len(self)
        if S > _native.SCENARIO_TAIL_MAX:
            raise LibError(f"{S} scenarios: at most {_native.SCENARIO_TAIL_MAX} fit the tail kernel; use "
                           "pnl_delta_gamma_sub_books and tail_measures")
        bad = first_ratio_trade(sb, _native.ratio_flags_host(sb.batch))
        if bad >= 0:
            raise LibError(f"trade {bad} has a ratio node (a payment lag or a per-coupon notional): the device chain has no "
                           "pricer for it; use pnl_delta_gamma_sub_books and tail_measures", status=_native.ADR_ERR_UNSUPPORTED)
        ctx, curve = self._ctx, self._ladder_curve()
        B, P, n = len(sb.labels), curve.n_pillars, sb.batch.n_trades
        dev = torch.device("cuda", ctx.device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
        plan, shocks = up(_native.scenario_subbook_plan(n, sb.sub_off)), up(self.shocks_bp())
        ladders, work, pnl, var_es = new(B, 1 + P + P * P), new(_native.subbook_ladders_work(curve, n, B)[0]), new(B, S), new(2, B)
        torch.cuda.synchronize(dev)
        with _native.DeviceTrades(ctx, sb.batch) as dev_trades:
            _native.subbook_ladders_dev(ctx, curve, dev_trades, B, plan.data_ptr(), _native.REQ_VALUE | _native.REQ_DELTA |
                                        _native.REQ_GAMMA, ladders.data_ptr(), work.data_ptr())
            _native.ladder_pnl_dev(ctx, B, P, ladders.data_ptr(), S, shocks.data_ptr(), pnl.data_ptr())
            _native.scenario_tail_dev(ctx, B, S, pnl.data_ptr(), tail_count(level, S), var_es[0].data_ptr(),
                                      var_es[1].data_ptr(), base_col=-1)
            ctx.sync()
        out = var_es.cpu().numpy()
        return {"labels": sb.labels, "var": out[0].copy(), "es": out[1].copy()}

    # --------------------------------------------------------------------------------------- credit delta-gamma P&L
    def pnl_credit_delta_gamma_sub_books(self, trades, spreads, keys, buckets=None, spread_shocks=None, parts: bool = False) -> dict:
        """`pnl_credit_sub_books` without the revaluation: every desk's ladders at its spreads with CS01, spread gamma and
        cross gamma per bucket (`price_credit_sub_books`, one launch chain) times the grid's joint shocks (`ladder_pnl`, one
        kernel).  ``spread_shocks`` as `pnl_credit_sub_books` takes them.  Returns `credit_delta_gamma_sub_books`' dict;
        the labels and rows are in `pnl_credit_sub_books`' order.  A trade with a ratio node is refused."""
        trades = list(trades)
        dz = None
        if spread_shocks is not None:
            dz = np.atleast_2d(np.asarray(spread_shocks, dtype=np.float64))
            if dz.shape[0] not in (1, len(self)):
                raise LibError(f"{dz.shape[0]} spread-shock rows for a grid of {len(self)} scenarios: one shared row or one per "
                               "scenario")
            dz = None if dz.shape[1] == 0 else dz
        return credit_delta_gamma_sub_books(self._engine(), self.curve, trades, spreads, keys, buckets, self.shocks_bp(), dz,
                                            parts=parts, curve_type=CurveTypes[self.curve_name])

    def pnl_credit_delta_gamma(self, trades, spreads, buckets=None, spread_shocks=None) -> np.ndarray:
        """``[S]``: the credit book's delta-gamma P&L under the grid's joint shocks - `pnl_credit` to second order (the
        sub-book form with one key, its row)."""
        trades = list(trades)
        return self.pnl_credit_delta_gamma_sub_books(trades, spreads, [0] * len(trades), buckets, spread_shocks)["pnl"][0]

    def explain_credit_sub_books(self, trades, spreads, keys, buckets=None, spread_shocks=None) -> dict:
        """P&L explain per credit desk and scenario: ``{"labels", "full", "delta_pnl", "gamma_pnl", "unexplained"}``, all
        ``[B, S]`` - ``full`` is `pnl_credit_sub_books`' full revaluation under the joint shocks, the parts are
        `pnl_credit_delta_gamma_sub_books`' (``delta_pnl`` holds the CS01 term, ``gamma_pnl`` the spread and cross gammas),
        and ``unexplained = full - (delta_pnl + gamma_pnl)``: third order in the shocks."""
        trades, keys = list(trades), list(keys)
        sub = _revalue(self._curves(True), False, *self._credit_book(trades, spreads, buckets, spread_shocks, True), keys)
        full = sub["sub_pv"][:, :-1] - sub["sub_pv"][:, -1:]
        dg = self.pnl_credit_delta_gamma_sub_books(trades, spreads, keys, buckets, spread_shocks, parts=True)
        assert dg["labels"] == sub["labels"] and dg["buckets"] == sub["buckets"] and full.shape == dg["pnl"].shape, \
            "the two routes order the desks differently"
        return {"labels": sub["labels"], "full": full, "delta_pnl": dg["delta_pnl"], "gamma_pnl": dg["gamma_pnl"],
                "unexplained": full - (dg["delta_pnl"] + dg["gamma_pnl"])}

    def sub_book_credit_delta_gamma_var_es(self, trades, spreads, keys, buckets=None, spread_shocks=None, level: float = 0.99) -> dict:
        """``{"labels": [...], "var": [B], "es": [B]}`` of the credit delta-gamma P&L straight from the trades: the ladder
        chain (adr_credit_subbook_ladders_dev), the P&L kernel (adr_ladder_pnl_dev on the augmented rows) and the tail kernel
        (adr_scenario_tail_dev) on one stream, so neither the ladders nor the ``[B, S]`` matrix leave the device.  ``var`` and
        ``es`` are `tail_measures`' of `pnl_credit_delta_gamma_sub_books`' ``pnl``, bit for bit.  A trade with a ratio node is
        refused.  The buffers are torch tensors; where torch brings a HIP runtime of its own, import torch before the first
        call into this library, as the tools do."""
        import torch
        from .sub_book_ladders import credit_cell_book
        S = len(self)
        if S > _native.SCENARIO_TAIL_MAX:
            raise LibError(f"{S} scenarios: at most {_native.SCENARIO_TAIL_MAX} fit the tail kernel; use "
                           "pnl_credit_delta_gamma_sub_books and tail_measures")
        cb = credit_cell_book(list(trades), self.curve._value_dt, CurveTypes[self.curve_name], spreads, keys, buckets)
        G = len(cb.buckets)
        dz = _grid_spread_rows(_spread_rows(spread_shocks, G), S, G, False)
        ctx, curve = self._ctx, self._ladder_curve()
        B, P, n = len(cb.labels), curve.n_pillars, cb.batch.n_trades
        Q = P + G
        if Q > _native.LADDER_PNL_MAX_PILLARS:
            raise LibError(f"{P} pillars and {G} buckets: at most {_native.LADDER_PNL_MAX_PILLARS} columns fit the P&L kernel")
        cell_off, desk_cell_off, cell_bucket = _native.credit_subbook_cells(cb.bucket, cb.sub_off)
        C = cell_bucket.size
        dev = torch.device("cuda", ctx.device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
        bufs = {"z": up(cb.z), "bucket": up(cb.bucket), "fix_tau": up(cb.fix_tau), "flt_tau": up(cb.flt_tau),
                "cell_plan": up(_native.scenario_subbook_plan(n, cell_off)), "desk_cell_off": up(desk_cell_off),
                "cell_bucket": up(cell_bucket)}
        shocks = up(credit_shock_matrix_bp(self.shocks_bp(), dz))
        ladders, work = new(B, 1 + Q + Q * Q), new(_native.credit_subbook_ladders_work(curve, n, B, C)[0])
        pnl, var_es = new(B, S), new(2, B)
        torch.cuda.synchronize(dev)
        with _native.DeviceTrades(ctx, cb.batch) as dev_trades:
            _native.credit_subbook_ladders_dev(ctx, curve, dev_trades, cb.fix_tau.size, cb.flt_tau.size, G, B, C,
                                               {k: v.data_ptr() if v.numel() else 0 for k, v in bufs.items()},
                                               _native.REQ_VALUE | _native.REQ_DELTA | _native.REQ_GAMMA, ladders.data_ptr(),
                                               work.data_ptr())
            _native.ladder_pnl_dev(ctx, B, Q, ladders.data_ptr(), S, shocks.data_ptr(), pnl.data_ptr())
            _native.scenario_tail_dev(ctx, B, S, pnl.data_ptr(), tail_count(level, S), var_es[0].data_ptr(),
                                      var_es[1].data_ptr(), base_col=-1)
            ctx.sync()
        out = var_es.cpu().numpy()
        return {"labels": cb.labels, "var": out[0].copy(), "es": out[1].copy()}

    def close(self):
        if getattr(self, "_base_dev", None) is not None:
            self._base_dev.close()
            self._base_dev = None
        self._set.close()
        self._plan.close()


def bump_ladder(tenors: Sequence[str], bump_bp: float = 1.0) -> List[Shock]:
    """Shocks for central finite differences: base, then +/- ``bump_bp`` on each tenor in turn
    (tests/test_ois_request_types.py:171-207 does these one `Model.scenario` at a time)."""
    h = bump_bp * 0.01            # quotes are in percent: 1 bp = 0.01
    shocks: List[Shock] = [0.0]
    for t in tenors:
        shocks.append({t: h})
        shocks.append({t: -h})
    return shocks


def finite_difference_delta(grid_values: np.ndarray, bump_bp: float = 1.0) -> np.ndarray:
    """Per-tenor central differences from values priced on a `bump_ladder` grid: [n, P] per 1 bp."""
    up, down = grid_values[1::2], grid_values[2::2]
    return ((up - down) / (2.0 * bump_bp)).T
