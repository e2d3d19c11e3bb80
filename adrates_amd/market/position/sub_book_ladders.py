"""Per-desk PV, delta and gamma ladders of a book from one launch (adr_subbook_ladders): `price_sub_books`.

The book is compiled, sorted by key and cut exactly as the scenario sub-books are (`scenarios.compile_book`,
`split_sub_books`), and every desk's row is the projection of that desk's own knot-space sums.  A desk's row has
exactly the bits of the same call on that desk's trades alone.

Trades with ratio nodes (a payment lag, a per-coupon notional) are outside the launch.  They are taken out before the
upload by `has_ratio_node`, priced per desk by ``price_batch`` (OIS) or ``price_frns`` (FRNs) with ``per_trade=False,
aggregate=True`` and added to the desk's row in float64: such desks are outside the bit contract.  The host route (``host=True``) has no pricer for them
and refuses such a book.

Credit desks: `price_credit_sub_books` prices bonds at their z-spreads and FRNs at their discount margins and returns, beside
the curve ladders AT THE SPREADS, every desk's CS01 and spread gamma per credit bucket and the rate x spread cross gamma
(adr_credit_subbook_ladders).  It has no route for ratio nodes and refuses such a trade.

Inflation desks: `price_yoy_sub_books` returns every desk's row on ``Q = P_d + P_i`` columns - the discount pillars, then the
inflation curve's: the discount ladders, the breakeven ladders and the discount x breakeven cross gamma of a YoY book
(adr_yoy_subbook_ladders), which no other route has.
"""
from dataclasses import dataclass

import numpy as np

from ... import _native
from ...trades.compiler import TradeBatch
from ...utils.error import LibError
from ...utils.global_types import CurveTypes, InstrumentTypes, RequestTypes
from ...utils.helpers import to_tenor
from ..curves.curve_tables import build_engine_curve
from .engine import Engine, price_batch, price_frns
from .scenarios import (_permute_batch, compile_book, compile_credit_book, split_sub_books, split_yoy_sub_books,
                        yoy_book_arrays)


def has_ratio_node(batch: TradeBatch) -> np.ndarray:
    """``[n]`` bool: the trade has a float coupon that accrues and is not paid on its accrual end, or a per-coupon
    notional other than 1 (the library's own rule, route::flag_lagged, which the upload applies)."""
    return _native.ratio_flags_host(batch)


def _curve_type_of(engine, ir_model):
    """The `CurveTypes` under which ``engine``'s model holds ``ir_model``."""
    for ct in CurveTypes:
        if getattr(engine.model.curves, ct.name, None) is ir_model:
            return ct
    raise LibError("ir_model is not a curve of the engine's model: pass curve_type")


def _host_curve(ir_model):
    host = build_engine_curve(ir_model.swap_rates, ir_model.swap_times, ir_model.year_fracs)
    return host, to_tenor(list(ir_model.swap_times))


def price_sub_books(engine: Engine, ir_model, trades, keys, reqs, host=False, curve_type=None):
    """``{"labels", "pv" [B], "delta" [B, P], "gamma" [B, P, P], "tenors"}`` of the sub-books of ``trades`` by ``keys``
    (one hashable key per trade; labels in order of first appearance).

    ``trades``: a mixed list of OIS, bonds and single-curve FRNs on ``ir_model``'s curve, or a compiled `TradeBatch`
    without ratio nodes that holds each key's trades consecutively (`split_sub_books`).  What ``reqs`` does not ask
    for is zeros.  ``host``: the CPU twin (adr_subbook_ladders_host), no GPU needed.  ``curve_type``: the curve the
    trades are checked against (`compile_book`), default the one under which the engine's model holds ``ir_model``."""
    reqs = set(reqs)
    want_gamma = RequestTypes.GAMMA in reqs
    want_delta = want_gamma or RequestTypes.DELTA in reqs
    trades, keys = trades if isinstance(trades, TradeBatch) else list(trades), list(keys)
    batch, const, order = compile_book(trades, ir_model._value_dt, curve_type or _curve_type_of(engine, ir_model))
    sb = split_sub_books(batch, const, order, keys)
    B, off = len(sb.labels), sb.sub_off
    ratio = has_ratio_node(sb.batch)
    plain = sb.batch
    plain_off = off
    if ratio.any():
        if host or sb.order is None:
            j = int(np.nonzero(ratio)[0][0])
            raise LibError(f"trade {j if sb.order is None else int(sb.order[j])} has a ratio node (a payment lag or a "
                           "per-coupon notional): " + ("the host route of price_sub_books has no pricer for it" if host else
                                                       "a compiled TradeBatch carries no objects to price it from"))
        keep = np.nonzero(~ratio)[0]
        plain_off = np.concatenate([[0], np.cumsum(~ratio)])[off].astype(np.int64)
        plain = _permute_batch(sb.batch, keep)[0] if keep.size else None
    method = ir_model._interp_type.value
    if host:
        curve, tenors = _host_curve(ir_model)
        out = _native.subbook_ladders_host(method, curve.times, curve.dfs, curve.jac, curve.hess if want_gamma else None,
                                           plain, plain_off, want_delta, want_gamma)
    else:
        cur = engine._device_curve(ir_model)
        tenors = cur["tenors"]
        P = cur["dev"].n_pillars
        if plain is None:
            out = {"pv": np.zeros(B), "delta": np.zeros((B, P)), "gamma": np.zeros((B, P, P))}
        else:
            with _native.DeviceTrades(cur["ctx"], plain) as dev_trades:
                out = _native.subbook_ladders(cur["ctx"], cur["dev"], dev_trades, plain_off, want_delta, want_gamma)
        for b in range(B):                   # the desks that hold trades with ratio nodes: one aggregate launch per kind
            idx = [int(sb.order[j]) for j in range(off[b], off[b + 1]) if ratio[j]]
            for pricer, kind in ((price_batch, InstrumentTypes.OIS_SWAP), (price_frns, InstrumentTypes.FRN)):
                mine = [trades[i] for i in idx if trades[i].derivative_type == kind]
                if not mine:
                    continue
                res = pricer(engine, ir_model, mine, reqs | {RequestTypes.VALUE}, per_trade=False, aggregate=True)
                out["pv"][b] += res["agg_pv"]
                if want_delta:
                    out["delta"][b] += res["agg_delta"]
                if want_gamma:
                    out["gamma"][b] += res["agg_gamma"]
    if sb.pv_const is not None:              # the FRN compiler's curve-independent amounts, per desk; price_frns has added
        const = np.where(ratio, 0.0, sb.pv_const)      # those of the trades it priced
        for b in range(B):
            c = const[off[b]:off[b + 1]]
            if np.any(c != 0.0):
                out["pv"][b] += float(np.sum(c))
    out["labels"] = sb.labels
    out["tenors"] = tenors
    return out


@dataclass
class CreditCells:
    """`credit_cell_book`'s result: the batch ordered by (desk, bucket) - within a desk the unbucketed trades first, then
    the buckets ascending, a stable sort of `split_sub_books`' order - with the per-trade and per-flow spread arrays to
    match, ``pv_const`` (or None), ``order`` (trade ``j`` of the batch is trade ``order[j]`` of the caller's list), the desk
    labels, ``sub_off [B + 1]`` and the bucket labels."""
    batch: TradeBatch
    pv_const: object
    order: np.ndarray
    labels: list
    sub_off: np.ndarray
    z: np.ndarray
    bucket: np.ndarray
    fix_tau: np.ndarray
    flt_tau: np.ndarray
    buckets: list


def credit_cell_book(trades, value_dt, curve_type, spreads, keys, buckets=None) -> CreditCells:
    """`compile_credit_book`, `split_sub_books` and the (desk, bucket) ordering adr_credit_subbook_ladders asks for.  A trade
    with a ratio node is refused by its index in the caller's list."""
    book = compile_credit_book(trades, value_dt, curve_type, spreads, buckets)
    sb = split_sub_books(book.batch, book.pv_const, book.order, list(keys))
    z, bucket, fix_tau, flt_tau = book.z, book.bucket, book.fix_tau, book.flt_tau
    if sb.perm is not None:
        z, bucket, fix_tau, flt_tau = z[sb.perm], bucket[sb.perm], fix_tau[sb.fix_idx], flt_tau[sb.flt_idx]
    batch, const, order = sb.batch, sb.pv_const, sb.order
    desk = np.repeat(np.arange(len(sb.labels), dtype=np.int64), np.diff(sb.sub_off))
    perm = np.lexsort((bucket, desk))                    # stable; the desks stay where they are
    if not np.array_equal(perm, np.arange(perm.size)):
        batch, fi, li = _permute_batch(batch, perm)
        z, bucket, fix_tau, flt_tau = z[perm], bucket[perm], fix_tau[fi], flt_tau[li]
        const, order = (None if const is None else const[perm]), order[perm]
    ratio = np.nonzero(has_ratio_node(batch))[0]
    if ratio.size:
        raise LibError(f"trade {int(order[ratio[0]])} has a ratio node (a payment lag or a per-coupon notional): the credit "
                       "sub-book ladders take trades whose float coupons are paid on their accrual end; "
                       "pnl_credit_sub_books revalues such a book", status=_native.ADR_ERR_UNSUPPORTED)
    return CreditCells(batch, const, order, sb.labels, sb.sub_off, z, bucket, fix_tau, flt_tau, book.labels)


def price_credit_sub_books(engine: Engine, ir_model, trades, spreads, keys, buckets, reqs, host=False, curve_type=None):
    """The desks' ladders at their spreads and their spread Greeks, from one launch chain (adr_credit_subbook_ladders).

    ``trades``: a list of `OIS`, `Bond` and single-curve `FRN` objects on ``ir_model``'s curve; ``spreads`` and ``buckets``
    one per trade as `compile_credit_book` takes them (``buckets=None``: no bucket anywhere); ``keys`` one hashable desk key
    per trade.  Returns ``{"labels", "buckets", "tenors", "pv" [B], "delta" [B, P], "gamma" [B, P, P], "cs01" [B, G],
    "spread_gamma" [B, G], "cross_gamma" [B, G, P], "ladders" [B, 1 + Q + Q Q]}``: ``delta`` per bp of a par quote and
    ``gamma`` per bp squared, both at the spreads; ``cs01`` per bp of the bucket's spread, ``spread_gamma`` and
    ``cross_gamma`` per bp squared; ``ladders`` the augmented rows (Q = P + G) that `ladder_pnl` takes beside
    `credit_shock_matrix_bp`'s rows.  What ``reqs`` does not ask for is zeros.  ``host``: the CPU twin, no GPU needed.  A
    trade with a ratio node is refused by its index in ``trades``."""
    reqs = set(reqs)
    want_gamma = RequestTypes.GAMMA in reqs
    want_delta = want_gamma or RequestTypes.DELTA in reqs
    cb = credit_cell_book(list(trades), ir_model._value_dt, curve_type or _curve_type_of(engine, ir_model), spreads, keys, buckets)
    G = len(cb.buckets)
    method = ir_model._interp_type.value
    if host:
        curve, tenors = _host_curve(ir_model)
        out = _native.credit_subbook_ladders_host(method, curve.times, curve.dfs, curve.jac, curve.hess if want_gamma else None,
                                                  cb.batch, cb.z, cb.bucket, cb.fix_tau, cb.flt_tau, G, cb.sub_off, want_delta,
                                                  want_gamma)
    else:
        cur = engine._device_curve(ir_model)
        tenors = cur["tenors"]
        with _native.DeviceTrades(cur["ctx"], cb.batch) as dev_trades:
            out = _native.credit_subbook_ladders(cur["ctx"], cur["dev"], dev_trades, cb.z, cb.bucket, cb.fix_tau, cb.flt_tau, G,
                                                 cb.sub_off, want_delta, want_gamma)
    if cb.pv_const is not None:              # the FRN compiler's curve-independent amounts (spread time 0), per desk
        for b in range(len(cb.labels)):
            c = cb.pv_const[cb.sub_off[b]:cb.sub_off[b + 1]]
            if np.any(c != 0.0):
                out["pv"][b] += float(np.sum(c))
                out["ladders"][b, 0] = out["pv"][b]
    out["labels"], out["buckets"], out["tenors"] = cb.labels, cb.buckets, tenors
    return out


def price_yoy_sub_books(engine: Engine, disc_curve, infl_curve, swaps_or_book, keys, reqs, host=False):
    """The inflation desks' augmented ladders from one launch chain (adr_yoy_subbook_ladders).

    ``swaps_or_book``: `YoYInflationSwap` objects or compiled arrays (`yoy_book_arrays`) on ``disc_curve`` and ``infl_curve``;
    ``keys`` one hashable desk key per swap.  Returns ``{"labels", "pv" [B], "delta" [B, Q], "gamma" [B, Q, Q], "tenors",
    "infl_tenors", "ladders" [B, 1 + Q + Q Q]}`` on ``Q = P_d + P_i`` columns, the discount pillars (``tenors``) first and then
    the inflation curve's (``infl_tenors``): ``delta`` per bp of a par quote or of a breakeven rate, ``gamma`` per bp squared
    with the discount block, the breakeven block and, in ``gamma[:, :P_d, P_d:]`` and its transpose, the cross block;
    ``ladders`` the same rows as `ladder_pnl` takes them beside `yoy_shock_matrix_bp`'s.  What ``reqs`` does not ask for is
    zeros.  ``host``: the CPU twin, no GPU needed."""
    from .inflation_engine import inflation_inputs
    reqs = set(reqs)
    want_gamma = RequestTypes.GAMMA in reqs
    want_delta = want_gamma or RequestTypes.DELTA in reqs
    sb = split_yoy_sub_books(*yoy_book_arrays(swaps_or_book, engine.model.value_dt), list(keys))
    im, T, b = inflation_inputs(infl_curve)
    method = disc_curve._interp_type.value
    if host:
        curve, tenors = _host_curve(disc_curve)
        out = _native.yoy_subbook_ladders_host(method, curve.times, curve.dfs, curve.jac, curve.hess if want_gamma else None, im,
                                               T, b, sb.fixed, sb.coupons, sb.sub_off, want_delta, want_gamma)
    else:
        cur = engine._device_curve(disc_curve)
        tenors = cur["tenors"]
        out = _native.yoy_subbook_ladders(cur["ctx"], cur["dev"], im, T, b, sb.fixed, sb.coupons, sb.sub_off, want_delta,
                                          want_gamma)
    rows = out["ladders"]
    Q = len(tenors) + T.size
    return {"labels": sb.labels, "pv": out["pv"], "delta": rows[:, 1:1 + Q].copy(), "gamma": rows[:, 1 + Q:].reshape(-1, Q, Q).copy(),
            "tenors": tenors, "infl_tenors": to_tenor(list(infl_curve.swap_times)), "ladders": rows}
