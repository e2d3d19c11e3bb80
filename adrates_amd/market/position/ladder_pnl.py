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
