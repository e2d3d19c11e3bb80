"""Delta-gamma P&L from ladders: what a desk's delta ladder and gamma matrix say it makes under a scenario set, without
a revaluation (adr_ladder_pnl, csrc/ladder_pnl.hip).

    pnl[b][s] = delta_b . x_s + 1/2 x_s' Gamma_b x_s

``delta [B, P]`` is per basis point and ``gamma [B, P, P]`` per basis point squared, as every pricing route of this
package returns them; ``x_s`` is scenario ``s``'s move of the ``P`` quotes in basis points (`shock_matrix_bp`).  The call
is generic over the curve: the discount ladders of `price_sub_books` take the par-quote shocks of a `ScenarioGrid`, the
inflation ladders of `YoYBook.compute` the breakeven shocks.

`delta_gamma_sub_books` joins `price_sub_books` and `ladder_pnl`: every desk's intraday P&L vector from one ladder launch
and one P&L launch.  The gap to full revaluation - the unexplained P&L per desk and scenario - is
`ScenarioGrid.explain_sub_books`.

Inflation desks take it too: `price_yoy_sub_books`' rows on the discount and the inflation pillars beside
`yoy_shock_matrix_bp`'s joint rows.

Credit desks take the same kernel: `price_credit_sub_books`' augmented rows hold, beside the curve ladders at the spreads,
CS01, spread gamma and the rate x spread cross gamma per bucket in the layout of a ladder over ``P + G`` "pillars", so
`credit_delta_gamma_sub_books` is `ladder_pnl` on those rows and `credit_shock_matrix_bp`'s joint shocks.
"""
from __future__ import annotations

from typing import Iterable, Sequence

import numpy as np

from ... import _native
from ...utils.error import LibError
from ...utils.global_types import RequestTypes

_PARTS = ("pnl", "delta_pnl", "gamma_pnl")


def ladder_rows(delta, gamma=None) -> np.ndarray:
    """``[B, 1 + P + P P]``: ``delta [B, P]`` and ``gamma [B, P, P]`` (None: zeros) in the layout adr_subbook_ladders
    writes, with a zero PV slot (adr_ladder_pnl does not read it)."""
    delta = np.asarray(delta, dtype=np.float64)
    if delta.ndim != 2 or delta.shape[1] < 1:
        raise LibError(f"delta must have shape [n_desks, n_pillars], not {list(delta.shape)}")
    B, P = delta.shape
    rows = np.zeros((B, 1 + P + P * P))
    rows[:, 1:1 + P] = delta
    if gamma is not None:
        gamma = np.asarray(gamma, dtype=np.float64)
        if gamma.shape != (B, P, P):
            raise LibError(f"gamma must have shape [{B}, {P}, {P}] to match delta, not {list(gamma.shape)}")
        rows[:, 1 + P:] = gamma.reshape(B, P * P)
    return rows


def ladder_pnl(delta, gamma, shocks_bp, parts=False, host=False, ctx=None):
    """``[B, S]``: the delta-gamma P&L of ``B`` ladders under ``S`` scenarios, in one kernel.

    ``delta [B, P]`` per bp; ``gamma [B, P, P]`` per bp squared, used as given (no symmetry is assumed), or None: the
    delta P&L alone, and gamma is not read; ``shocks_bp [S, P]`` (`shock_matrix_bp`, `ScenarioGrid.shocks_bp`).  With
    ``parts`` a dict ``{"pnl", "delta_pnl", "gamma_pnl"}`` whose parts add up to ``pnl`` bit for bit.  ``host=True`` runs
    the CPU twin: the same fused multiply-adds in the same order, hence the same bits; no GPU needed."""
    shocks_bp = np.atleast_2d(np.asarray(shocks_bp, dtype=np.float64))
    rows = ladder_rows(delta, gamma)
    if shocks_bp.ndim != 2 or shocks_bp.shape[0] < 1 or shocks_bp.shape[1] != np.shape(delta)[1]:
        raise LibError(f"shocks_bp must have shape [n_scenarios, {np.shape(delta)[1]}] (one column per pillar of the ladder), "
                       f"not {list(shocks_bp.shape)}")
    if gamma is None:
        want = (False, True, False)
    else:
        want = (True, True, True) if parts else (True, False, False)
    if host:
        out = _native.ladder_pnl_host(rows, shocks_bp, want)
    else:
        out = _native.ladder_pnl(ctx or _native.default_context(), rows, shocks_bp, want)
    if gamma is None:
        out = {"pnl": out["delta_pnl"], "delta_pnl": out["delta_pnl"], "gamma_pnl": np.zeros_like(out["delta_pnl"])}
    return {k: out[k] for k in _PARTS} if parts else out["pnl"]


def shock_matrix_bp(tenors: Sequence[str], shocks: Iterable, bp_per_unit: float) -> np.ndarray:
    """``[S, P]``: the shocks of a scenario set as moves of the ``P`` quotes in basis points, built from the shocks
    themselves (not from differences of shocked quotes, which would carry their rounding).

    ``shocks``: `Model.scenario`'s convention - a float moves every tenor, a dict ``{tenor: move}`` the named ones (a
    name that is no tenor of the curve moves nothing, as in `shocked_quotes`); ``bp_per_unit``: basis points per unit of
    the shocks (100 for par quotes in percent, 1 for shocks given in basis points)."""
    tenors = list(tenors)
    rows = [[float(s.get(t, 0.0)) * bp_per_unit for t in tenors] if isinstance(s, dict) else [float(s) * bp_per_unit] * len(tenors)
            for s in shocks]
    return np.array(rows, dtype=np.float64).reshape(len(rows), len(tenors))


def first_ratio_trade(sub_books, batch_flags) -> int:
    """The caller's number of the first trade of a split book (`split_sub_books`) that has a ratio node, or -1."""
    hit = np.nonzero(batch_flags)[0]
    if not hit.size:
        return -1
    j = int(hit[0])
    return j if sub_books.order is None else int(sub_books.order[j])


def delta_gamma_sub_books(engine, ir_model, trades, keys, shocks_bp, parts=False, host=False, curve_type=None):
    """Every desk's delta-gamma P&L vector: `price_sub_books` (one ladder launch) and then `ladder_pnl` (one kernel).

    ``trades`` and ``keys`` as `price_sub_books` takes them (trades with ratio nodes follow its rule: priced per desk
    beside the launch on the device, refused on the host route); ``shocks_bp [S, P]`` on ``ir_model``'s pillars.
    Returns ``{"labels", "pnl" [B, S], "pv" [B], "delta" [B, P], "gamma" [B, P, P], "tenors"}`` and with ``parts`` also
    ``"delta_pnl"`` and ``"gamma_pnl"``.  ``host=True`` runs both steps on their CPU twins; no GPU needed."""
    from .sub_book_ladders import price_sub_books
    reqs = {RequestTypes.VALUE, RequestTypes.DELTA, RequestTypes.GAMMA}
    out = price_sub_books(engine, ir_model, trades, keys, reqs, host=host, curve_type=curve_type)
    ctx = None if host else engine._device_curve(ir_model)["ctx"]
    pnl = ladder_pnl(out["delta"], out["gamma"], shocks_bp, parts=parts, host=host, ctx=ctx)
    out.update(pnl if parts else {"pnl": pnl})
    return out


def credit_shock_matrix_bp(shocks_bp, spread_shocks) -> np.ndarray:
    """``[S, P + G]``: joint shock rows for the augmented ladders of `price_credit_sub_books` - the curve shocks
    ``shocks_bp [S, P]`` in basis points as they are, then the spread shocks ``spread_shocks [S, G]`` in DECIMALS (as
    `pnl_credit_sub_books` takes them) times 1e4.  Either side may be one row, shared by all scenarios; ``spread_shocks=None``
    with no bucket."""
    x = np.atleast_2d(np.asarray(shocks_bp, dtype=np.float64))
    y = np.zeros((1, 0)) if spread_shocks is None else np.atleast_2d(np.asarray(spread_shocks, dtype=np.float64))
    if x.ndim != 2 or y.ndim != 2:
        raise LibError(f"shocks_bp [S, P] and spread_shocks [S, G] are needed, not {list(x.shape)} and {list(y.shape)}")
    S = max(x.shape[0], y.shape[0])
    if x.shape[0] not in (1, S) or y.shape[0] not in (1, S):
        raise LibError(f"{x.shape[0]} curve-shock rows and {y.shape[0]} spread-shock rows: each must be one shared row or one "
                       "row per scenario")
    return np.ascontiguousarray(np.hstack([np.broadcast_to(x, (S, x.shape[1])), np.broadcast_to(y, (S, y.shape[1])) * 1e4]))


def yoy_shock_matrix_bp(shocks_bp, breakevens=None, b0=None, infl_shocks_bp=None) -> np.ndarray:
    """``[S, P_d + P_i]``: joint shock rows for the augmented ladders of `price_yoy_sub_books` - the discount curve's shocks
    ``shocks_bp [S, P_d]`` in basis points as they are, then the breakeven moves in basis points: ``(breakevens - b0) * 1e4``
    from breakeven rows ``[S, P_i]`` and the base rates ``b0 [P_i]``, or ``infl_shocks_bp [S, P_i]`` as they are (moves built
    from the shocks themselves carry no rounding of a difference).  Either side may be one row, shared by all scenarios."""
    if (breakevens is None) == (infl_shocks_bp is None):
        raise LibError("give breakevens (with b0) or infl_shocks_bp")
    x = np.atleast_2d(np.asarray(shocks_bp, dtype=np.float64))
    if infl_shocks_bp is not None:
        y = np.atleast_2d(np.asarray(infl_shocks_bp, dtype=np.float64))
    else:
        if b0 is None:
            raise LibError("breakeven rows need the base rates b0")
        y = (np.atleast_2d(np.asarray(breakevens, dtype=np.float64)) - np.asarray(b0, dtype=np.float64).reshape(1, -1)) * 1e4
    if x.ndim != 2 or y.ndim != 2:
        raise LibError(f"shocks_bp [S, P_d] and breakeven rows [S, P_i] are needed, not {list(x.shape)} and {list(y.shape)}")
    S = max(x.shape[0], y.shape[0])
    if x.shape[0] not in (1, S) or y.shape[0] not in (1, S):
        raise LibError(f"{x.shape[0]} curve-shock rows and {y.shape[0]} breakeven rows: each must be one shared row or one row per "
                       "scenario")
    return np.ascontiguousarray(np.hstack([np.broadcast_to(x, (S, x.shape[1])), np.broadcast_to(y, (S, y.shape[1]))]))


def augmented_ladder_pnl(ladders, shocks, parts=False, host=False, ctx=None):
    """`ladder_pnl` on ready rows ``ladders [B, 1 + Q + Q Q]`` and ``shocks [S, Q]``: ``[B, S]``, or with ``parts`` the
    dict of `ladder_pnl`."""
    want = (True, True, True) if parts else (True, False, False)
    if host:
        out = _native.ladder_pnl_host(ladders, shocks, want)
    else:
        out = _native.ladder_pnl(ctx or _native.default_context(), ladders, shocks, want)
    return {k: out[k] for k in _PARTS} if parts else out["pnl"]


def credit_delta_gamma_sub_books(engine, ir_model, trades, spreads, keys, buckets, shocks_bp, spread_shocks=None, parts=False,
                                 host=False, curve_type=None):
    """Every credit desk's delta-gamma P&L under joint (curve, spread) shocks: `price_credit_sub_books` (one launch chain)
    and then `ladder_pnl` on the augmented rows (one kernel),

        delta . x + x' Gamma x / 2 + sum_g (cs01_g y_g + csg_g y_g^2 / 2 + y_g cross_g . x),

    ``x`` the curve shocks in bp (``shocks_bp [S, P]``), ``y`` the spread shocks in bp (``spread_shocks [S, G]`` in
    decimals, one column per bucket label in order of first appearance; None: none).  Returns `price_credit_sub_books`'
    dict plus ``"pnl" [B, S]`` and, with ``parts``, ``"delta_pnl"`` (first order, CS01 included) and ``"gamma_pnl"``.
    ``host=True`` runs both steps on their CPU twins; no GPU needed."""
    from .sub_book_ladders import price_credit_sub_books
    reqs = {RequestTypes.VALUE, RequestTypes.DELTA, RequestTypes.GAMMA}
    out = price_credit_sub_books(engine, ir_model, trades, spreads, keys, buckets, reqs, host=host, curve_type=curve_type)
    G = len(out["buckets"])
    if spread_shocks is not None and np.shape(np.atleast_2d(spread_shocks))[1] != G:
        raise LibError(f"spread_shocks must have shape [n_scenarios, {G}] or [{G}] (one column per bucket), not "
                       f"{list(np.shape(spread_shocks))}")
    shocks = credit_shock_matrix_bp(shocks_bp, (np.zeros((1, G)) if spread_shocks is None else spread_shocks) if G else None)
    ctx = None if host else engine._device_curve(ir_model)["ctx"]
    pnl = augmented_ladder_pnl(out["ladders"], shocks, parts=parts, host=host, ctx=ctx)
    out.update(pnl if parts else {"pnl": pnl})
    return out
