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

The firm's question - how much of the FIRM's VaR and expected shortfall each desk carries - is `monte_carlo_allocate_tail`:
the firm's P&L is `ladder_pnl` of one row, the fixed-order sum of the desks' rows; adr_scenario_tail_order (an ordered radix
select, ties to the lower scenario index) hands out the firm's ``k`` worst scenarios; every desk is priced at those ``k``
shock rows alone.  No ``[B, S]`` matrix is made, and the components add up to the firm's figures:

    >>> risk = sub_book_monte_carlo_allocate_tail(engine, curve, trades, desk_keys, L, 262_144, level=0.99, seed=7)
    >>> risk["var"], risk["es"], risk["comp_es"]                 # the firm's, and [B] shares with sum(comp_es) = es
    >>> monte_carlo_shocks(L, 1, 7, first_scenario=int(risk["scenarios"][0]))     # the firm's worst scenario, made again

Full revaluation on the same shocks: the scenario kernels read discount factors only, so the shock rows are turned into
``dfs [S, K]`` where the generator wrote them (adr_curve_dfs_shocked, csrc/curve_dfs.hip: the bootstrap scan, values only,
with the curve builder's bits) and priced per desk by the sub-book launch, a tile of scenarios at a time:

    >>> curves = ShockedCurves(model, "GBP_OIS_SONIA")
    >>> risk = monte_carlo_revalue_var_es(curves, trades, desk_keys, L, 262_144, level=0.99, seed=7)
    >>> gap = monte_carlo_explain_var_es(engine, curves, curve, trades, desk_keys, L, 262_144, seed=7)["gap_var"]

Credit and inflation desks, and all three product lines in one matrix of the firm's desks, are revalued under joint shock
rows by `monte_carlo_firm.FirmBook` and `monte_carlo_firm.monte_carlo_revalue_firm_var_es`.  That module holds the one
revaluation chain: `revalue_shocks_sub_books` and `monte_carlo_revalue_var_es` here check their own arguments, wrap the
trades in a `FirmBook` with a rates line alone and run it.
"""
from __future__ import annotations

import numpy as np

from ... import _native
from ...utils.error import LibError
from ...utils.global_types import CurveTypes, RequestTypes
from ..curves.curve_tables import build_engine_curve
from .ladder_pnl import ladder_rows
from .scenarios import _interp_value, _tail_args, compile_book, split_sub_books, tail_count


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


def _check_tail_count(k, level, m, limit=None):
    limit = _native.SCENARIO_TAIL_MAX if limit is None else limit
    if k > limit:
        raise LibError(f"a tail of {k} P&L values (level {level}, {m} values per row): at most {limit} "
                       "fit the tail kernel", status=_native.ADR_ERR_UNSUPPORTED)


def allocate_tail_select(rows, level: float = 0.99, base_col: int = -1, host: bool = False, ctx=None):
    """`allocate_tail` without the row limit, on the device for any width: ``{"var", "es", "comp_var" [B], "comp_es" [B]}`` of
    ``rows [B, S]`` (adr_scenario_tail_alloc_select; ``host=True``: its CPU twin, the same bits).  The firm's ``k`` worst
    scenarios come from the ordered tail select (adr_scenario_tail_order) on the fixed-order column sums, so the limit is on
    the tail: a `LibError` with ``ADR_ERR_UNSUPPORTED`` when ``tail_count(level, S)`` exceeds ``_native.SCENARIO_ALLOC_MAX``.
    Where `allocate_tail`'s kernel takes the rows the result has its bits; beyond, those of the rule as NumPy states it
    (`scenarios._allocate_tail_numpy`)."""
    rows, m, k = _tail_args(rows, base_col, level, 1)
    _check_tail_count(k, level, m, _native.SCENARIO_ALLOC_MAX)
    rows = np.ascontiguousarray(rows)
    if host:
        return _native.scenario_tail_alloc_select_host(rows, k, base_col)
    return _native.scenario_tail_alloc_select(ctx or _native.default_context(), rows, k, base_col)


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
    rows, factor = _ladder_args(delta, gamma, factor_bp, ladders)
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

    ctx = ctx or _native.default_context()
    torch, dev, up, new = _torch_buffers(ctx)
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


def _ladder_args(delta, gamma, factor_bp, ladders):
    """``(rows [B, 1 + P + P P], factor [P, F])`` as `monte_carlo_var_es` and `monte_carlo_allocate_tail` take them."""
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
    return rows, factor


def firm_ladder(ladders) -> np.ndarray:
    """``[1 + P + P P]``: the firm's ladder row, the fixed-order sum of the desks' rows ``ladders [B, 1 + P + P P]`` -
    `allocate_tail`'s column-sum rule (row ``b`` to slot ``b % 64`` in row order from 0.0, then the halving tree) on every
    column (adr_scenario_total_host; the device's kernel gives the same bits).  Delta-gamma P&L is linear in the row, so
    `ladder_pnl` of this row is the firm's P&L."""
    return _native.scenario_total_host(ladders)


def monte_carlo_allocate_tail(delta, gamma, factor_bp, n_scenarios: int, level: float = 0.99, seed: int = 0, antithetic: bool = False,
                              host: bool = False, ctx=None, max_bytes: int = 2 ** 31, ladders=None) -> dict:
    """``{"var", "es", "comp_var" [B], "comp_es" [B], "scenarios" [k]}``: the FIRM's Monte Carlo delta-gamma VaR and expected
    shortfall and how much of each every desk carries - the Euler allocation that adds up to the firm's figure - under
    ``n_scenarios`` normal shocks.  The arguments are `monte_carlo_var_es`'s, ``ladders=`` included.

    No ``[B, S]`` matrix is made.  Delta-gamma P&L is linear in the ladder row, so the firm's P&L under every shock is
    adr_ladder_pnl of ONE row, `firm_ladder` of the desks' rows (adr_scenario_total_dev); the ordered tail select
    (adr_scenario_tail_order_dev) hands out the firm's ``k = tail_count(level, n_scenarios)`` worst scenarios as indices in
    the firm's order - ties to the lower index - with the firm's ``var`` and ``es``; those shock rows are gathered
    (adr_shock_gather_dev) and every desk is priced at them alone, ``[tile, k]`` at a time under ``max_bytes``
    (adr_ladder_pnl_dev, then adr_tail_components_dev), all on one stream with torch tensors as buffers.  Only the results
    leave the device; ``scenarios`` are the global scenario indices in the firm's order, and a row of the shock set can be
    made again from ``seed`` and its index alone (`monte_carlo_shocks` with ``first_scenario``).

    Bit for bit, whatever the tiling: every output is the CPU twins' chain on the device's shocks; ``var`` and ``es`` are
    `monte_carlo_var_es` of the firm's row (``ladders=firm_ladder(rows)[None]``); ``comp_*`` are `allocate_tail`'s component
    sums over the columns ``scenarios`` of the full ``ladder_pnl(rows, shocks)``.  The firm's P&L comes from the firm's
    LADDER, not from column sums of desk P&Ls as in `allocate_tail_select` of that matrix: the two differ by rounding, at
    most ``(P P + P + B + 8) eps A_s`` with ``A_s`` the sum of the absolute terms of scenario ``s``, so the two agree on
    ``scenarios`` and ``comp_*`` wherever the firm's ``k + 1`` smallest totals lie further apart than that, and then on
    ``var`` and ``es`` to that rounding.  ``sum(comp_es)`` is ``es`` and ``sum(comp_var)`` is ``var`` to rounding.

    The ``k`` pairs are sorted in LDS: ``k > _native.SCENARIO_ALLOC_MAX`` is a `LibError` with ``ADR_ERR_UNSUPPORTED``
    (1 048 576 scenarios at 99 %; 99.5 % fits, and so do 786 432 at 99 %).  A NaN in the firm's row gives NaN everywhere and
    ``scenarios`` of -1.  ``host=True``: the CPU twins of every step on the host's shocks; no GPU needed."""
    rows, factor = _ladder_args(delta, gamma, factor_bp, ladders)
    (B, width), (P, F), S = rows.shape, factor.shape, int(n_scenarios)
    if S < 1:
        raise LibError("at least one scenario is needed")
    k = tail_count(level, S)
    _check_tail_count(k, level, S, _native.SCENARIO_ALLOC_MAX)
    tile = int(max(1, min(B, int(max_bytes) // (8 * k))))
    tiles = [(b0, min(tile, B - b0)) for b0 in range(0, B, tile)]
    if host:
        shocks = _native.shock_normal_host(factor, S, seed, antithetic, 0)
        tot = _native.ladder_pnl_host(firm_ladder(rows)[None], shocks)["pnl"]
        order, var, es = _native.scenario_tail_order_host(tot, k)
        gathered = _native.shock_gather_host(shocks, order[0])
        comp = np.empty((2, B))
        for b0, nb in tiles:
            comp[0, b0:b0 + nb], comp[1, b0:b0 + nb] = _native.tail_components_host(
                _native.ladder_pnl_host(rows[b0:b0 + nb], gathered)["pnl"])
        return {"var": float(var[0]), "es": float(es[0]), "comp_var": comp[0].copy(), "comp_es": comp[1].copy(), "scenarios": order[0].copy()}

    ctx = ctx or _native.default_context()
    torch, dev, up, new = _torch_buffers(ctx)
    d_rows, d_factor, firm, shocks, tot = up(rows), up(factor), new(width), new(S, P), new(S)
    gathered, pnl, out = new(k, P), new(tile, k), new(2, B + 1)         # out: [comp_var | var], [comp_es | es]
    order = torch.empty(k, dtype=torch.int64, device=dev)
    work = torch.empty(_native.scenario_tail_order_work(1, S, k), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    _native.scenario_total_dev(ctx, B, width, d_rows.data_ptr(), firm.data_ptr())
    _native.shock_normal_dev(ctx, seed, 0, S, P, F, d_factor.data_ptr(), antithetic, shocks.data_ptr())
    _native.ladder_pnl_dev(ctx, 1, P, firm.data_ptr(), S, shocks.data_ptr(), tot.data_ptr())
    _native.scenario_tail_order_dev(ctx, 1, S, tot.data_ptr(), k, order.data_ptr(), out.data_ptr() + 8 * B,
                                    out.data_ptr() + 8 * (2 * B + 1), work.data_ptr())
    _native.shock_gather_dev(ctx, k, P, shocks.data_ptr(), S, order.data_ptr(), gathered.data_ptr())
    for b0, nb in tiles:
        _native.ladder_pnl_dev(ctx, nb, P, d_rows.data_ptr() + 8 * width * b0, k, gathered.data_ptr(), pnl.data_ptr())
        _native.tail_components_dev(ctx, nb, k, pnl.data_ptr(), out.data_ptr() + 8 * b0, out.data_ptr() + 8 * (B + 1 + b0))
    ctx.sync()
    res, scenarios = out.cpu().numpy(), order.cpu().numpy()
    return {"var": float(res[0, B]), "es": float(res[1, B]), "comp_var": res[0, :B].copy(), "comp_es": res[1, :B].copy(),
            "scenarios": scenarios}


def sub_book_monte_carlo_allocate_tail(engine, ir_model, trades, keys, factor_bp, n_scenarios: int, level: float = 0.99, seed: int = 0,
                                       antithetic: bool = False, host: bool = False) -> dict:
    """`monte_carlo_allocate_tail` straight from the trades, with ``labels``: `price_sub_books` (one ladder launch) and then
    the chain on ``ir_model``'s pillars, as `sub_book_monte_carlo_var_es` does for the desks' own figures."""
    from .sub_book_ladders import price_sub_books
    reqs = {RequestTypes.VALUE, RequestTypes.DELTA, RequestTypes.GAMMA}
    out = price_sub_books(engine, ir_model, trades, keys, reqs, host=host)
    ctx = None if host else engine._device_curve(ir_model)["ctx"]
    risk = monte_carlo_allocate_tail(out["delta"], out["gamma"], factor_bp, n_scenarios, level=level, seed=seed, antithetic=antithetic,
                                     host=host, ctx=ctx)
    return {"labels": out["labels"], **risk}


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


# --------------------------------------------------------------------------- full revaluation on Monte Carlo shock rows
SCENARIO_LAUNCH_MAX = 65535 * 64         # scenarios of one sub-book launch (csrc/scenario_common.hpp, launch_grid)


class ShockedCurves:
    """What turns shock rows of ``model.curves[curve_name]``'s par quotes into discount factors: the base `EngineCurve`
    (the host builder's, without derivatives), its par rates, the interpolation scheme and, on first use on the device, a
    `_native.CurvePlan` on ``ctx`` (default: the default context).  No curve is built here - `ScenarioGrid` holds whole
    curves with their Jacobians for a few thousand scenarios; this holds the recipe for any number of them."""

    def __init__(self, model, curve_name: str, ctx=None):
        if curve_name not in model._curve_params_dict:
            raise ValueError(f"No stored parameters found for curve '{curve_name}'")
        self.model, self.curve_name = model, curve_name
        self.curve = getattr(model.curves, curve_name)
        self.method = _interp_value(self.curve._interp_type)
        self.base = build_engine_curve(self.curve.swap_rates, self.curve.swap_times, self.curve.year_fracs, with_hessian=False)
        self.rates = self.base.rates
        self._ctx, self._plan = ctx, None

    @property
    def n_pillars(self) -> int:
        return int(self.rates.size)

    @property
    def n_knots(self) -> int:
        return self.base.n_knots

    def context(self):
        if self._ctx is None:
            self._ctx = _native.default_context()
        return self._ctx

    def plan(self):
        if self._plan is None:
            self._plan = _native.CurvePlan(self.context(), self.method, self.base)
        return self._plan

    def dfs(self, shocks_bp, host: bool = False):
        """``(dfs [S, K], bad [S])`` of the shock rows ``shocks_bp [S, ld >= P]`` (adr_curve_dfs_shocked, or its CPU twin)."""
        if host:
            return _native.curve_dfs_shocked_host(self.base.acc, self.base.pillar, self.base.prev_idx, self.rates, shocks_bp)
        return _native.curve_dfs_shocked(self.context(), self.plan(), self.rates, shocks_bp)

    def _book(self, trades, keys):
        return split_sub_books(*compile_book(trades, self.curve._value_dt, CurveTypes[self.curve_name]), keys)

    def close(self):
        if self._plan is not None:
            self._plan.close()
            self._plan = None


def revalue_scenario_bytes(curves: ShockedCurves, n_trades: int, n_sub_books: int) -> int:
    """Bytes of scratch ONE scenario of a revaluation tile takes: its row of ``dfs`` (K doubles), the bootstrap's scratch
    (K + P), the sub-book launch's (adr_scenario_subbook_work: a double per chunk of 64 trades and desk) and its column of
    the ``[B, tile]`` rows."""
    return _scenario_bytes(curves, [(n_trades, n_sub_books)], n_sub_books)


def _scenario_bytes(curves, lines, n_desks, n_columns=0):
    """The same for any product lines ``(trades, sub-books)`` on one curve whose rows go into ``n_desks`` rows, with
    ``n_columns`` doubles of dense shock columns beside the ``dfs`` (`monte_carlo_firm.firm_scenario_bytes`)."""
    work = sum(_native.scenario_subbook_work(n, B, 1) for n, B in lines)
    return 8 * (2 * curves.n_knots + curves.n_pillars + n_columns + work + n_desks)


def _tile_of(per, B, S, max_bytes):
    """Scenarios per tile from the bytes ``per`` scenario: the ``[B, S + 1]`` rows and the tile's scratch stay under
    ``max_bytes``."""
    rows = 8 * B * (S + 1)
    if int(max_bytes) - rows < per:
        raise LibError(f"the [{B}, {S} + 1] P&L rows ({rows} bytes) and one scenario's scratch ({per} bytes) do not fit max_bytes = "
                       f"{int(max_bytes)}: raise it, or revalue fewer scenarios or desks at a time")
    return int(min(S, SCENARIO_LAUNCH_MAX, (int(max_bytes) - rows) // per))


def _raise_bad(count, first, also=""):
    """``also``: what else the flags of the caller stand for, beside a bad discount factor."""
    raise LibError(f"{count} scenario(s) give a discount factor that is not finite or not positive{also}, the first at index {first}: "
                   "the shocks are too large for the curve")


def _check_bad_dev(bad, also=""):
    """After the stream has drained: the `LibError` of the bad flags, counted on the device."""
    count = int(bad.count_nonzero())
    if count:
        _raise_bad(count, int(bad.nonzero()[0]), also)


def _torch_buffers(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    return torch, dev, up, new


def revalue_shocks_sub_books(curves: ShockedCurves, trades, keys, shocks_bp, host: bool = False, max_bytes: int = 2 ** 31) -> dict:
    """``{"labels": [...], "pnl": [B, S]}``: every desk's full-revaluation P&L under the explicit shock rows ``shocks_bp
    [S, P]`` (basis points on the par quotes; columns beyond ``P`` are not read).

    ``trades`` and ``keys`` as `ScenarioGrid.revalue_sub_books` takes them (`compile_book`, `split_sub_books`).  The
    scenarios are cut into tiles so that the tile's ``dfs``, the two scratch buffers, its ``[B, tile]`` rows and the ``[B, S
    + 1]`` result stay under ``max_bytes`` (`revalue_scenario_bytes` per scenario; a `LibError` when not even one fits); per
    tile the bootstrap (adr_curve_dfs_shocked_dev), the sub-book launch (adr_scenario_subbook_pv_dev) and the copy into the
    rows (adr_scenario_rows_merge_dev) run on one stream: the chain of `monte_carlo_firm.revalue_shocks_firm` on a `FirmBook`
    with a rates line alone, here with rows of any width.  The base PV is one more launch, on a zero shock row, whose
    ``dfs`` are the base curve's bits: a scenario's result does not depend on the launch it is priced in, so a zero shock
    row gives exactly 0.0 in every desk, the tiling changes no bit, and the P&L is `revalue_on_curves_sub_books`' on the
    same ``dfs`` with the base row appended, column minus last column.  What does not depend on the curve (an FRN coupon
    fixed and paid at the value time) cancels and is not added.  A scenario with a discount factor that is not finite or
    not positive is a `LibError` naming the count and the first index.  ``host=True``: the CPU twins; no GPU needed."""
    from .monte_carlo_firm import FirmBook, _revalue_pnl
    shocks = np.ascontiguousarray(shocks_bp, dtype=np.float64)
    if shocks.ndim != 2 or shocks.shape[0] < 1 or shocks.shape[1] < curves.n_pillars:
        raise LibError(f"shocks_bp must have shape [S >= 1, {curves.n_pillars} or more], not {list(shocks.shape)}")
    return _revalue_pnl(FirmBook(curves, rates=(trades, keys)), shocks, host, max_bytes, also="")


def monte_carlo_revalue_var_es(curves: ShockedCurves, trades, keys, factor_bp, n_scenarios: int, level: float = 0.99, seed: int = 0,
                               antithetic: bool = False, host: bool = False, max_bytes: int = 2 ** 31, allocate: bool = False) -> dict:
    """``{"labels": [...], "var": [B], "es": [B]}``: every desk's Monte Carlo VaR and expected shortfall by FULL
    revaluation under ``n_scenarios`` normal shocks with factor matrix ``factor_bp [P, F]`` - `monte_carlo_var_es`' shock
    rows (the same seed gives the same bits), priced as `revalue_shocks_sub_books` prices them.

    One stream, torch tensors as buffers: the shocks (adr_shock_normal_dev), the tiles of `revalue_shocks_sub_books` into
    ``rows [B, S + 1]`` with the base PV as column ``S``, then adr_scenario_tail_select_dev with ``base_col = S``; only the
    ``[B]`` vectors leave the device.  ``allocate=True`` adds adr_scenario_tail_alloc_select_dev on the same rows: the
    result is then ``{"labels", "var", "es", "firm_var", "firm_es", "comp_var" [B], "comp_es" [B]}`` - the firm's figures
    and every desk's share of them, which add up to them (`allocate_tail_select`).  The rows must fit the device: when
    ``[B, S + 1]`` and one scenario's scratch exceed ``max_bytes`` a `LibError` says so.  Bit for bit the result is
    `tail_measures_select` (and `allocate_tail_select`) of `revalue_shocks_sub_books`' rows on `monte_carlo_shocks`,
    whatever the tiling.  ``host=True``: the CPU twins on the host's shocks; no GPU needed."""
    from .monte_carlo_firm import FirmBook, _revalue_var_es
    factor = np.ascontiguousarray(factor_bp, dtype=np.float64)
    if factor.ndim != 2 or factor.shape[0] != curves.n_pillars:
        raise LibError(f"factor_bp [P, F] needs one row per par quote ({curves.n_pillars}), not {list(factor.shape)}")
    return _revalue_var_es(FirmBook(curves, rates=(trades, keys)), factor, n_scenarios, level, seed, antithetic, host, max_bytes, allocate,
                           also="")


def monte_carlo_explain_var_es(engine, curves: ShockedCurves, ir_model, trades, keys, factor_bp, n_scenarios: int, level: float = 0.99,
                               seed: int = 0, antithetic: bool = False, host: bool = False, max_bytes: int = 2 ** 31) -> dict:
    """The delta-gamma figures held against full revaluation on the SAME shock rows: ``{"labels", "full_var", "full_es",
    "dg_var", "dg_es", "gap_var", "gap_es"}``, ``[B]`` each - `monte_carlo_revalue_var_es` beside
    `sub_book_monte_carlo_var_es` on one seed (the generator gives both the same bits), ``gap = full - dg``: what the
    second-order expansion misses in the tail, where it is weakest.  ``ir_model``: the curve ``curves`` was made from, as
    `sub_book_monte_carlo_var_es` takes it."""
    trades, keys = (trades if hasattr(trades, "n_trades") else list(trades)), list(keys)
    full = monte_carlo_revalue_var_es(curves, trades, keys, factor_bp, n_scenarios, level=level, seed=seed, antithetic=antithetic,
                                      host=host, max_bytes=max_bytes)
    dg = sub_book_monte_carlo_var_es(engine, ir_model, trades, keys, factor_bp, n_scenarios, level=level, seed=seed,
                                     antithetic=antithetic, host=host)
    if dg["labels"] != full["labels"]:
        raise LibError("the two routes order the desks differently")
    return {"labels": full["labels"], "full_var": full["var"], "full_es": full["es"], "dg_var": dg["var"], "dg_es": dg["es"],
            "gap_var": full["var"] - dg["var"], "gap_es": full["es"] - dg["es"]}
