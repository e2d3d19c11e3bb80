"""Monte Carlo delta-gamma VaR: ``ladders -> shocks -> P&L -> VaR / ES`` on one stream, for any scenario count.

The shocks are correlated normals made on the device from a factor of the covariance of the daily quote moves
(adr_shock_normal, csrc/shock_normal.hip): ``x_s = L z_s`` in basis points, ``z`` from Philox4x32-10 and Box-Muller, every
row a function of the seed and its index alone, so a set can be made in pieces and made again.  The P&L is `ladder_pnl`'s
kernel; the tail comes from adr_scenario_tail_select (csrc/tail_select.hip): a radix select of the ``k``-th smallest P&L
and then `tail_measures`' kernel on the ``k`` survivors, so a row may hold a million scenarios where `tail_measures` stops
at ``SCENARIO_TAIL_MAX`` - the limit is on the tail count now.

    >>> L = factor_from_covariance(cov_bp2)                      # [P, P]; n_factors=8: the leading 8 PCA columns
    >>> risk = sub_book_monte_carlo_var_es(engine, curve, trades, desk_keys, L, 262_144, level=0.99, seed=7)
    >>> risk["var"], risk["es"]                                  # [B] each

Credit and inflation desks price their augmented ladders themselves and pass the rows on; the factor matrix then has one
row per column of the augmented ladder (``Q = P + G`` quotes and spread buckets, or ``P_d + P_i`` quotes and breakevens),
in the ladder's order and in basis points:

    >>> out = price_credit_sub_books(engine, curve, trades, spreads, desk_keys, buckets, reqs)
    >>> monte_carlo_var_es(None, None, factor_from_covariance(cov_Q_bp2), 262_144, ladders=out["ladders"])
    >>> out = price_yoy_sub_books(engine, disc_curve, infl_curve, swaps, desk_keys, reqs)
    >>> monte_carlo_var_es(out["delta"], out["gamma"], factor_from_covariance(cov_Q_bp2), 262_144)
"""
from __future__ import annotations

import numpy as np

from ... import _native
from ...utils.error import LibError
from ...utils.global_types import RequestTypes
from .ladder_pnl import ladder_rows
from .scenarios import _tail_args, tail_count


def factor_from_covariance(cov_bp2, n_factors=None) -> np.ndarray:
    """``[P, F]``: a factor ``L`` of the covariance ``cov_bp2 [P, P]`` (bp squared) with ``L L' = cov``.  Without
    ``n_factors`` the lower Cholesky factor (``F = P``; a semi-definite matrix gets zero columns where its pivots vanish);
    with it the leading ``n_factors`` PCA columns ``V sqrt(lambda)``, largest eigenvalue first, ``L L'`` then being the best
    approximation of that rank.  NumPy on the host: the matrix is tiny.  A matrix that is not symmetric positive
    semi-definite to rounding is a `LibError`."""
    C = np.asarray(cov_bp2, dtype=np.float64)
    if C.ndim != 2 or C.shape[0] != C.shape[1] or C.shape[0] < 1 or not np.all(np.isfinite(C)):
        raise LibError(f"cov_bp2 must be a finite square matrix, not shape {list(C.shape)}")
    P = C.shape[0]
    scale = float(np.max(np.abs(C)))
    eps = np.finfo(np.float64).eps
    if np.max(np.abs(C - C.T)) > 8 * eps * scale:
        raise LibError("cov_bp2 is not symmetric")
    C = 0.5 * (C + C.T)
    lam, V = np.linalg.eigh(C)
    tol = 8 * P * eps * max(scale, float(lam[-1]))
    if lam[0] < -tol:
        raise LibError(f"cov_bp2 is not positive semi-definite: its smallest eigenvalue is {lam[0]:.3e}")
    if n_factors is not None:
        F = int(n_factors)
        if not 1 <= F <= P:
            raise LibError(f"n_factors must lie in 1 .. {P}, not {n_factors}")
        lead = np.argsort(-lam, kind="stable")[:F]
        return np.ascontiguousarray(V[:, lead] * np.sqrt(np.maximum(lam[lead], 0.0)))
    L = np.zeros((P, P))
    for j in range(P):                                  # column by column; a vanishing pivot leaves a zero column
        d = C[j, j] - L[j, :j] @ L[j, :j]
        if d > tol:
            L[j, j] = np.sqrt(d)
            L[j + 1:, j] = (C[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def monte_carlo_shocks(factor_bp, n_scenarios: int, seed: int, antithetic: bool = False, first_scenario: int = 0, host: bool = False,
                       ctx=None) -> np.ndarray:
    """``[S, P]``: ``n_scenarios`` correlated normal shocks ``factor_bp [P, F] @ z`` in basis points, the rows `ladder_pnl`
    takes.  Row ``s`` is global row ``first_scenario + s`` and depends on ``seed``, that index, the factor matrix and
    ``antithetic`` alone (``antithetic``: global rows ``2 i`` and ``2 i + 1`` are a draw and its exact negation).
    ``host=True``: the CPU twin - the same uniforms bit for bit, normals to a few ulp."""
    if host:
        return _native.shock_normal_host(factor_bp, n_scenarios, seed, antithetic, first_scenario)
    return _native.shock_normal(ctx or _native.default_context(), factor_bp, n_scenarios, seed, antithetic, first_scenario)


def tail_measures_select(rows, level: float = 0.99, base_col: int = -1, host: bool = False, ctx=None):
    """`tail_measures` without the row limit: ``(var [B], es [B])`` of ``rows [B, S]`` for any ``S`` (adr_scenario_tail_select;
    ``host=True``: its CPU twin, the same bits), with `tail_measures`' bits where it takes the rows.  The limit is on the
    tail: a `LibError` with ``ADR_ERR_UNSUPPORTED`` when ``tail_count(level, S)`` exceeds ``_native.SCENARIO_TAIL_MAX``."""
    rows, m, k = _tail_args(rows, base_col, level, 1)
    _check_tail_count(k, level, m)
    if host:
        return _native.scenario_tail_select_host(rows, k, base_col)
    return _native.scenario_tail_select(ctx or _native.default_context(), rows, k, base_col)


def _check_tail_count(k, level, m):
    if k > _native.SCENARIO_TAIL_MAX:
        raise LibError(f"a tail of {k} P&L values (level {level}, {m} values per row): at most {_native.SCENARIO_TAIL_MAX} "
                       "fit the tail kernel", status=_native.ADR_ERR_UNSUPPORTED)


def monte_carlo_var_es(delta, gamma, factor_bp, n_scenarios: int, level: float = 0.99, seed: int = 0, antithetic: bool = False,
                       host: bool = False, ctx=None, max_bytes: int = 2 ** 31, ladders=None) -> dict:
    """``{"var": [B], "es": [B]}``: the delta-gamma VaR and expected shortfall of ``B`` desks under ``n_scenarios`` normal
    shocks with factor matrix ``factor_bp [P, F]``.

    The ladders come as `ladder_pnl` takes them - ``delta [B, P]`` per bp, ``gamma [B, P, P]`` per bp squared or None - or
    as ready rows ``ladders [B, 1 + P + P P]`` (then ``delta`` and ``gamma`` are None): `price_credit_sub_books`' and
    `price_yoy_sub_books`' augmented rows go through unchanged beside a factor matrix of ``Q`` rows.  The shocks are made
    once (adr_shock_normal_dev); then adr_ladder_pnl_dev and adr_scenario_tail_select_dev run over tiles of desks, so that
    the ``[tile, S]`` P&L buffer stays under ``max_bytes``, all on one stream with torch tensors as buffers; only ``var``
    and ``es`` come back.  A desk's result depends on its ladder row and the shock set alone: the tiling changes no bit,
    and the result is `tail_measures_select` of `ladder_pnl` of `monte_carlo_shocks` (device shocks), bit for bit.
    ``host=True``: the three CPU twins, tile by tile; no GPU needed.  Where torch brings a HIP runtime of its own, import
    torch before the first call into this library, as the tools do."""
    if ladders is None:
        rows = ladder_rows(delta, gamma)
    else:
        if delta is not None or gamma is not None:
            raise LibError("give delta and gamma, or ladders, not both")
        rows = np.ascontiguousarray(ladders, dtype=np.float64)
    factor = np.ascontiguousarray(factor_bp, dtype=np.float64)
    if rows.ndim != 2 or factor.ndim != 2 or rows.shape[0] < 1 or rows.shape[1] != 1 + factor.shape[0] * (1 + factor.shape[0]):
        raise LibError(f"ladder rows [B, 1 + P + P P] and factor_bp [P, F] are needed, not {list(rows.shape)} and "
                       f"{list(factor.shape)}")
    (B, width), (P, F), S = rows.shape, factor.shape, int(n_scenarios)
    if S < 1:
        raise LibError("at least one scenario is needed")
    k = tail_count(level, S)
    _check_tail_count(k, level, S)
    tile = int(max(1, min(B, int(max_bytes) // (8 * S))))
    tiles = [(b0, min(tile, B - b0)) for b0 in range(0, B, tile)]
    if host:
        shocks = _native.shock_normal_host(factor, S, seed, antithetic, 0)
        out = np.empty((2, B))
        for b0, nb in tiles:
            pnl = _native.ladder_pnl_host(rows[b0:b0 + nb], shocks)["pnl"]
            out[0, b0:b0 + nb], out[1, b0:b0 + nb] = _native.scenario_tail_select_host(pnl, k)
        return {"var": out[0].copy(), "es": out[1].copy()}

    import torch
    ctx = ctx or _native.default_context()
    dev = torch.device("cuda", ctx.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    d_rows, d_factor, shocks, pnl, var_es = up(rows), up(factor), new(S, P), new(tile, S), new(2, B)
    work = torch.empty(max(_native.scenario_tail_select_work(nb, S, k) for _, nb in tiles), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    _native.shock_normal_dev(ctx, seed, 0, S, P, F, d_factor.data_ptr(), antithetic, shocks.data_ptr())
    for b0, nb in tiles:
        _native.ladder_pnl_dev(ctx, nb, P, d_rows.data_ptr() + 8 * width * b0, S, shocks.data_ptr(), pnl.data_ptr())
        _native.scenario_tail_select_dev(ctx, nb, S, pnl.data_ptr(), k, var_es.data_ptr() + 8 * b0, var_es.data_ptr() + 8 * (B + b0),
                                         work.data_ptr())
    ctx.sync()
    out = var_es.cpu().numpy()
    return {"var": out[0].copy(), "es": out[1].copy()}


def sub_book_monte_carlo_var_es(engine, ir_model, trades, keys, factor_bp, n_scenarios: int, level: float = 0.99, seed: int = 0,
                                antithetic: bool = False, host: bool = False) -> dict:
    """``{"labels": [...], "var": [B], "es": [B]}``: every desk's Monte Carlo delta-gamma VaR and ES straight from the
    trades - `price_sub_books` (one ladder launch) and then `monte_carlo_var_es` on ``ir_model``'s pillars (``factor_bp
    [P, F]``, one row per par quote).  ``trades`` and ``keys`` as `price_sub_books` takes them.  Credit and inflation desks:
    `price_credit_sub_books` or `price_yoy_sub_books`, then `monte_carlo_var_es` on the augmented rows (the module's
    docstring shows both)."""
    from .sub_book_ladders import price_sub_books
    reqs = {RequestTypes.VALUE, RequestTypes.DELTA, RequestTypes.GAMMA}
    out = price_sub_books(engine, ir_model, trades, keys, reqs, host=host)
    ctx = None if host else engine._device_curve(ir_model)["ctx"]
    risk = monte_carlo_var_es(out["delta"], out["gamma"], factor_bp, n_scenarios, level=level, seed=seed, antithetic=antithetic,
                              host=host, ctx=ctx)
    return {"labels": out["labels"], **risk}
