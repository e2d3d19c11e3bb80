"""Monte Carlo VaR by full revaluation for the whole firm: rates, credit and inflation desks under JOINT shock rows,
``shocks -> curves, spread shocks, breakevens -> three sub-book launches -> one [B, S + 1] matrix -> VaR / ES`` on one stream.

A joint row has ``Q = P + G + P_i`` columns in basis points: the OIS par quotes, the credit line's spread buckets, the
inflation curve's breakeven rates.  adr_curve_dfs_shocked_dev reads the first ``P`` where the generator left them;
adr_shock_columns_dev (csrc/shock_columns.hip) turns the other two ranges into what the credit and the YoY kernel read, a
dense ``dz [S, G]`` in decimals and ``b [S, P_i]`` of breakeven rates, with the bits of `shocked_spreads` and
`shocked_breakevens`; adr_scenario_rows_merge_dev puts the three launches' rows into the desks' rows, `combine_sub_book_rows`
on the device.

    >>> curves = ShockedCurves(model, "GBP_OIS_SONIA")
    >>> firm = FirmBook(curves, rates=(trades, keys), credit=(bonds, spreads, bond_keys, buckets), inflation=(yoy_book, yoy_keys))
    >>> cols = firm.columns                                      # where each block of the [Q, Q] covariance goes
    >>> risk = monte_carlo_revalue_firm_var_es(firm, factor_from_covariance(cov_Q_bp2), 262_144, level=0.99, seed=7)
    >>> gap = monte_carlo_explain_firm_var_es(engine, firm, L, 262_144, seed=7)["gap_var"]      # against delta-gamma

This is the library's one full-revaluation chain (`_firm_rows_host`, `_firm_rows_dev`, `_revalue_pnl`, `_revalue_var_es`).
`monte_carlo.revalue_shocks_sub_books` and `monte_carlo.monte_carlo_revalue_var_es` run it on a `FirmBook` with a rates line
alone; what they add is their own argument checks, shock rows wider than ``Q`` (the row stride goes in beside ``Q``) and a
bad-scenario message without the clause on breakevens.
"""
from __future__ import annotations

import contextlib

import numpy as np

from ... import _native
from ...utils.error import LibError
from ...utils.global_types import CurveTypes, RequestTypes
from ...utils.helpers import to_tenor
from .inflation_engine import inflation_inputs
from .monte_carlo import (ShockedCurves, _check_bad_dev, _check_tail_count, _raise_bad, _scenario_bytes, _tile_of, _torch_buffers,
                          monte_carlo_var_es)
from .scenarios import (_first_appearance, compile_credit_book, split_sub_books, split_yoy_sub_books, tail_count)

_ALSO_BAD = ", a breakeven rate at or below -100 % or a shock that is not finite"
_REQS = {RequestTypes.VALUE, RequestTypes.DELTA, RequestTypes.GAMMA}


class _Line:
    """One product line of a `FirmBook`: its kind, what the caller gave, its desk labels and ``sub_off``, the arrays its
    scenario entries take, and - once the firm's labels are known - the firm's row of each of its desks (``target``) and
    whether an earlier line has written that row (``add``)."""

    def __init__(self, kind, given, labels, sub_off, n, **arrays):
        self.kind, self.given, self.labels, self.sub_off, self.n = kind, given, list(labels), sub_off, int(n)
        self.__dict__.update(arrays)
        self.target = self.add = None

    @property
    def B(self):
        return len(self.labels)


class FirmBook:
    """The firm's books on one discount curve: up to three product lines, each cut into desks by its keys.

    ``curves``: the `ShockedCurves` every line discounts on, at its model's value date.  ``rates = (trades, keys)`` as
    `revalue_shocks_sub_books` takes them; ``credit = (trades, spreads, keys, buckets)`` as `compile_credit_book` and
    `split_sub_books` take them; ``inflation = (YoYBook or swaps, keys)`` - a list of swaps becomes a `YoYBook` on
    ``curves.model``, a `YoYBook` brings its own inflation curve and must discount on a curve of ``curves.curve_name``'s
    type at the same value date.  At least one line is needed; everything else is a `LibError`.

    The shock columns (``Q`` of them) are the ``P`` par quotes, then the credit line's ``G`` bucket labels in
    `compile_credit_book`'s order, then the inflation curve's ``P_i`` pillars; a missing line has no columns.  The desks
    (``labels``) are in order of first appearance over rates, credit, inflation; a label may occur in more than one line,
    and its row is then the sum of the lines' rows in that order (`combine_sub_book_rows`)."""

    def __init__(self, curves: ShockedCurves, rates=None, credit=None, inflation=None):
        if not isinstance(curves, ShockedCurves):
            raise LibError("curves must be a ShockedCurves")
        if rates is None and credit is None and inflation is None:
            raise LibError("a FirmBook needs at least one of rates, credit and inflation")
        self.curves = curves
        value_dt, curve_type = curves.curve._value_dt, CurveTypes[curves.curve_name]
        self.lines = []
        self.buckets, self.infl_curve = [], None
        if rates is not None:
            trades, keys = rates
            trades, keys = (trades if hasattr(trades, "n_trades") else list(trades)), list(keys)
            sb = curves._book(trades, keys)
            self.lines.append(_Line("rates", (trades, keys), sb.labels, sb.sub_off, sb.batch.n_trades, batch=sb.batch))
        if credit is not None:
            trades, spreads, keys, buckets = credit
            trades, keys = list(trades), list(keys)
            book = compile_credit_book(trades, value_dt, curve_type, spreads, buckets)
            sb = split_sub_books(book.batch, book.pv_const, book.order, keys)
            per = (book.z, book.bucket, book.fix_tau, book.flt_tau)
            if sb.perm is not None:
                per = (book.z[sb.perm], book.bucket[sb.perm], book.fix_tau[sb.fix_idx], book.flt_tau[sb.flt_idx])
            self.buckets = list(book.labels)
            self.lines.append(_Line("credit", (trades, spreads, keys, buckets), sb.labels, sb.sub_off, sb.batch.n_trades, batch=sb.batch,
                                    z=per[0], bucket=per[1], fix_tau=per[2], flt_tau=per[3]))
        if inflation is not None:
            from .yoy_book import YoYBook
            book, keys = inflation
            if not isinstance(book, YoYBook):
                book = YoYBook(book, curves.model)
            if book.curve_type.name != curves.curve_name:
                raise LibError(f"the YoY book discounts on {book.curve_type.name}, the firm on {curves.curve_name}")
            if book.model.value_dt != value_dt:
                raise LibError("the YoY book's model and the firm's curve have different value dates")
            sb = split_yoy_sub_books(*book._arrays(), list(keys))
            self.infl_curve = book.inflation_curve
            im, T, b0 = inflation_inputs(self.infl_curve)
            self.lines.append(_Line("inflation", (book, list(keys)), sb.labels, sb.sub_off, sb.sub_off[-1], fixed=sb.fixed,
                                    coupons=sb.coupons, im=im, T=T, b0=b0))
        self._index_desks()

    def _index_desks(self):
        """The firm's labels from the lines', and every line's rows of the firm's matrix."""
        self.labels, index = _first_appearance(lab for line in self.lines for lab in line.labels)
        seen = set()
        for line in self.lines:
            line.target = np.array([index[lab] for lab in line.labels], dtype=np.int64)
            line.add = np.array([lab in seen for lab in line.labels], dtype=np.int32)
            seen.update(line.labels)

    def line(self, kind):
        return next((line for line in self.lines if line.kind == kind), None)

    @property
    def n_desks(self) -> int:
        return len(self.labels)

    @property
    def n_columns(self) -> int:
        return self.columns["breakeven"].stop

    @property
    def columns(self) -> dict:
        """``{"curve", "spread", "breakeven"}``: the column ranges of a joint shock row (an absent line's is empty), and
        ``"buckets"`` and ``"infl_tenors"``, the labels of the last two - what the ``[Q, Q]`` covariance is built from."""
        P, G = self.curves.n_pillars, len(self.buckets)
        infl = self.line("inflation")
        Pi = 0 if infl is None else int(infl.T.size)
        return {"curve": range(0, P), "spread": range(P, P + G), "breakeven": range(P + G, P + G + Pi), "buckets": list(self.buckets),
                "infl_tenors": [] if infl is None else to_tenor(list(infl.T))}


def firm_scenario_bytes(firm: FirmBook) -> int:
    """Bytes of scratch ONE scenario of a firm's revaluation tile takes: `revalue_scenario_bytes`' row of ``dfs``, bootstrap
    scratch and column of the ``[B, tile]`` rows, the scenario's ``dz`` and ``b`` (``G + P_i`` doubles) and every line's
    sub-book scratch (adr_scenario_subbook_work)."""
    cols = firm.columns
    return _scenario_bytes(firm.curves, [(line.n, line.B) for line in firm.lines], firm.n_desks, len(cols["spread"]) + len(cols["breakeven"]))


def _tiles(S, tile):
    """``(first scenario, scenarios)`` per tile of the shock rows, then the zero row as column ``S``."""
    return [(s0, min(tile, S - s0)) for s0 in range(0, S, tile)] + [(S, 1)]


def _firm_rows_host(firm, shocks, tile, also):
    """``[B, S + 1]`` on the CPU twins: the desks' PVs under the joint shock rows ``[S, ld >= Q]``, tile by tile, and under
    the zero row last.  ``also``: `_raise_bad`'s."""
    c, cols = firm.curves, firm.columns
    S, ld = shocks.shape
    G, Pi = len(cols["spread"]), len(cols["breakeven"])
    rows = np.zeros((firm.n_desks, S + 1))
    zero = np.zeros((1, ld))
    count, first = 0, -1
    for s0, nt in _tiles(S, tile):
        x = zero if s0 == S else shocks[s0:s0 + nt]
        dfs, bad = c.dfs(x, host=True)
        dz = b = None
        if G:
            dz, bad = _native.shock_columns_host(x, cols["spread"].start, G, bad=bad)
        if Pi:
            b, bad = _native.shock_columns_host(x, cols["breakeven"].start, Pi, base=firm.line("inflation").b0, floor=-1.0, bad=bad)
        if bad.any() and count == 0:
            first = s0 + int(np.argmax(bad != 0))
        count += int(np.count_nonzero(bad))
        if count:                       # (once a scenario is bad only the flags of the rest are wanted)
            continue
        for line in firm.lines:
            if line.kind == "rates":
                out = _native.scenario_subbook_pv_host(c.method, c.base.times, dfs, line.batch, line.sub_off)
            elif line.kind == "credit":
                out = _native.credit_scenario_subbook_pv_host(c.method, c.base.times, dfs, dz, line.batch, line.z, line.bucket,
                                                              line.fix_tau, line.flt_tau, line.sub_off)
            else:
                out = _native.yoy_scenario_subbook_pv_host(c.method, c.base.times, dfs, line.im, line.T, b, line.fixed, line.coupons,
                                                           line.sub_off)
            _native.scenario_rows_merge_host(out["sub_pv"], rows, s0, line.target, line.add)
    if count:
        _raise_bad(count, first, also)
    return rows


def _firm_rows_dev(firm, stack, shocks_ptr, S, ld, tile, rows, bad, new, up):
    """Enqueue on the context's stream: ``rows [B, S + 1]`` (a torch tensor) of the desks' PVs under the device shock rows
    ``[S, ld >= Q]`` at ``shocks_ptr``, tile by tile, and under the zero row as column ``S``; ``bad [S + 1]`` int32 beside them.
    ``stack``: the `contextlib.ExitStack` that owns the uploaded batches.  Returns the buffers the stream still reads."""
    c, cols = firm.curves, firm.columns
    ctx, plan, K, P, B = c.context(), c.plan(), c.n_knots, c.n_pillars, firm.n_desks
    G, Pi = len(cols["spread"]), len(cols["breakeven"])
    ptr = lambda t: t.data_ptr() if t.numel() else 0
    times, base, zero = up(c.base.times), up(c.rates), up(np.zeros(ld))
    dfs, work_b, part = new(tile, K), new(_native.curve_dfs_shocked_work(plan, tile)), new(B, tile)
    dz, b = new(tile, G), new(tile, Pi)
    held = [times, base, zero, dfs, work_b, part, dz, b]
    launches, b0_ptr = [], 0
    for line in firm.lines:
        t = dict(plan=up(_native.scenario_subbook_plan(line.n, line.sub_off)), target=up(line.target), add=up(line.add),
                 work=new(_native.scenario_subbook_work(line.n, line.B, tile)))
        if line.kind == "inflation":
            fix_off, fix_tp, fix_pay, cpn_off, cpn = _native._yoy_legs(line.fixed, line.coupons)
            t.update(T=up(line.T), b0=up(line.b0), fix_off=up(fix_off), fix_tp=up(fix_tp), fix_pay=up(fix_pay), cpn_off=up(cpn_off),
                     cpn=up(cpn))
            sizes, b0_ptr = (fix_tp.size, cpn.shape[1]), t["b0"].data_ptr()
        else:
            trades = stack.enter_context(_native.DeviceTrades(ctx, line.batch))
            if line.kind == "credit":
                t.update(z=up(line.z), bucket=up(np.ascontiguousarray(line.bucket, dtype=np.int32)), fix_tau=up(line.fix_tau),
                         flt_tau=up(line.flt_tau))
                sizes = (line.fix_tau.size, line.flt_tau.size)
        ptrs = {k: ptr(v) for k, v in t.items()}
        ptrs.update(times=times.data_ptr(), dfs=dfs.data_ptr(), dz=ptr(dz), b=ptr(b))
        held.append(t)
        if line.kind == "rates":
            launch = lambda nt, trades=trades, p=ptrs, line=line: _native.scenario_subbook_pv_dev(
                ctx, c.method, K, p["times"], nt, p["dfs"], trades, line.B, p["plan"], part.data_ptr(), p["work"])
        elif line.kind == "credit":
            launch = lambda nt, trades=trades, p=ptrs, line=line, sizes=sizes: _native.credit_scenario_subbook_pv_dev(
                ctx, c.method, K, nt, G, nt if G else 1, nt, trades, sizes[0], sizes[1], line.B, p, part.data_ptr(), p["work"])
        else:
            launch = lambda nt, p=ptrs, line=line, sizes=sizes: _native.yoy_scenario_subbook_pv_dev(
                ctx, c.method, K, nt, line.im, Pi, nt, nt, line.n, sizes[0], sizes[1], line.B, p, part.data_ptr(), p["work"])
        launches.append((launch, line.B, ptrs["target"], ptrs["add"]))
    for s0, nt in _tiles(S, tile):
        x_ptr = zero.data_ptr() if s0 == S else shocks_ptr + 8 * ld * s0
        flags = bad.data_ptr() + 4 * s0
        _native.curve_dfs_shocked_dev(ctx, plan, base.data_ptr(), nt, ld, x_ptr, dfs.data_ptr(), work_b.data_ptr(), bad_ptr=flags)
        if G:
            _native.shock_columns_dev(ctx, nt, ld, x_ptr, P, G, dz.data_ptr(), bad_ptr=flags)
        if Pi:
            _native.shock_columns_dev(ctx, nt, ld, x_ptr, P + G, Pi, b.data_ptr(), base_ptr=b0_ptr, floor=-1.0, bad_ptr=flags)
        for launch, B_line, target, add in launches:
            launch(nt)
            _native.scenario_rows_merge_dev(ctx, B_line, nt, part.data_ptr(), B, S + 1, s0, rows.data_ptr(), target, add)
    return held


def _shock_rows(firm, shocks_bp):
    shocks = np.ascontiguousarray(shocks_bp, dtype=np.float64)
    Q = firm.n_columns
    if shocks.ndim != 2 or shocks.shape[0] < 1 or shocks.shape[1] != Q:
        raise LibError(f"shocks_bp must have shape [S >= 1, {Q}] (the firm's columns: FirmBook.columns), not {list(shocks.shape)}")
    return shocks


def revalue_shocks_firm(firm: FirmBook, shocks_bp, host: bool = False, max_bytes: int = 2 ** 31) -> dict:
    """``{"labels": [...], "pnl": [B, S], "columns": firm.columns}``: every desk's full-revaluation P&L under the explicit
    joint shock rows ``shocks_bp [S, Q]`` in basis points.

    Per tile of scenarios (`firm_scenario_bytes` each; the tile's scratch and the ``[B, S + 1]`` result stay under
    ``max_bytes``, a `LibError` when not even one scenario fits), on one stream: the bootstrap (adr_curve_dfs_shocked_dev
    with ``ld = Q``), adr_shock_columns_dev for the spread shocks and for the breakevens, read where the rows lie, the
    sub-book launch of every line and adr_scenario_rows_merge_dev of its rows into the desks'.  The base PV is one more
    pass on a zero row, whose ``dz`` is zero and whose ``b`` is the curve's breakevens bit for bit: a zero shock row gives
    exactly 0.0 in every desk, the tiling changes no bit, and the P&L is `combine_sub_book_rows` of the three
    ``*_on_curves_sub_books`` calls on the same ``dfs``, ``dz`` and ``b`` with the base appended, column minus last
    column.  What does not depend on the scenario (an FRN coupon fixed and paid at the value time) cancels and is not
    added.  A scenario with a bad discount factor, a breakeven at or below -100 % or a shock that is not finite is a
    `LibError` naming the count and the first index.  ``host=True``: the CPU twins end to end; no GPU needed."""
    return {**_revalue_pnl(firm, _shock_rows(firm, shocks_bp), host, max_bytes, _ALSO_BAD), "columns": firm.columns}


def _revalue_pnl(firm, shocks, host, max_bytes, also):
    """``{"labels", "pnl" [B, S]}`` under the checked shock rows ``shocks [S, ld >= Q]``: `revalue_shocks_firm`'s chain, and
    `revalue_shocks_sub_books`' on a rates-only firm.  ``also``: `_raise_bad`'s."""
    (S, ld), B = shocks.shape, firm.n_desks
    tile = _tile_of(firm_scenario_bytes(firm), B, S, max_bytes)
    if host:
        rows = _firm_rows_host(firm, shocks, tile, also)
    else:
        ctx = firm.curves.context()
        torch, dev, up, new = _torch_buffers(ctx)
        d_shocks = up(shocks)
        d_rows = torch.zeros((B, S + 1), dtype=torch.float64, device=dev)
        bad = torch.zeros(S + 1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        with contextlib.ExitStack() as stack:
            held = _firm_rows_dev(firm, stack, d_shocks.data_ptr(), S, ld, tile, d_rows, bad, new, up)
            ctx.sync()
        del held
        _check_bad_dev(bad, also)
        rows = d_rows.cpu().numpy()
    return {"labels": firm.labels, "pnl": rows[:, :-1] - rows[:, -1:]}


def monte_carlo_revalue_firm_var_es(firm: FirmBook, factor_bp, n_scenarios: int, level: float = 0.99, seed: int = 0,
                                    antithetic: bool = False, host: bool = False, max_bytes: int = 2 ** 31, allocate: bool = False) -> dict:
    """`monte_carlo_revalue_var_es` for a `FirmBook`: every desk's Monte Carlo VaR and expected shortfall by FULL
    revaluation under ``n_scenarios`` joint normal shocks with factor matrix ``factor_bp [Q, F]``, one row per column of
    ``firm.columns``.

    One stream: adr_shock_normal_dev with ``P = Q``, the tiles of `revalue_shocks_firm` into ``rows [B, S + 1]``, then
    adr_scenario_tail_select_dev with ``base_col = S`` and, with ``allocate``, adr_scenario_tail_alloc_select_dev; only
    the ``[B]`` vectors leave the device.  The result and the checks are `monte_carlo_revalue_var_es`': ``{"labels",
    "var", "es"}`` and with ``allocate`` also ``firm_var``, ``firm_es``, ``comp_var [B]`` and ``comp_es [B]``; bit for bit
    `tail_measures_select` (and `allocate_tail_select`) of `revalue_shocks_firm`'s rows on `monte_carlo_shocks`, whatever
    the tiling.  ``host=True``: the CPU twins on the host's shocks; no GPU needed."""
    factor = np.ascontiguousarray(factor_bp, dtype=np.float64)
    Q = firm.n_columns
    if factor.ndim != 2 or factor.shape[0] != Q:
        raise LibError(f"factor_bp [Q, F] needs one row per column of the firm's shock rows ({Q}), not {list(factor.shape)}")
    return _revalue_var_es(firm, factor, n_scenarios, level, seed, antithetic, host, max_bytes, allocate, _ALSO_BAD)


def _revalue_var_es(firm, factor, n_scenarios, level, seed, antithetic, host, max_bytes, allocate, also):
    """`monte_carlo_revalue_firm_var_es`' chain under the checked ``factor [Q, F]``, and `monte_carlo_revalue_var_es`' on a
    rates-only firm.  ``also``: `_raise_bad`'s."""
    (Q, F), S = factor.shape, int(n_scenarios)
    if S < 1:
        raise LibError("at least one scenario is needed")
    k = tail_count(level, S)
    _check_tail_count(k, level, S, _native.SCENARIO_ALLOC_MAX if allocate else None)
    B = firm.n_desks
    tile = _tile_of(firm_scenario_bytes(firm), B, S, max_bytes)
    if host:
        rows = _firm_rows_host(firm, _native.shock_normal_host(factor, S, seed, antithetic, 0), tile, also)
        var, es = _native.scenario_tail_select_host(rows, k, S)
        out = {"labels": firm.labels, "var": var, "es": es}
        if allocate:
            whole = _native.scenario_tail_alloc_select_host(rows, k, S)
            out.update(firm_var=whole["var"], firm_es=whole["es"], comp_var=whole["comp_var"], comp_es=whole["comp_es"])
        return out

    ctx = firm.curves.context()
    torch, dev, up, new = _torch_buffers(ctx)
    d_factor, shocks, res = up(factor), new(S, Q), new(4, B + 1)         # res: var, es, [comp_var | firm], [comp_es | firm]
    rows = torch.zeros((B, S + 1), dtype=torch.float64, device=dev)
    bad = torch.zeros(S + 1, dtype=torch.int32, device=dev)
    n_work = max(_native.scenario_tail_select_work(B, S + 1, k), _native.scenario_tail_alloc_select_work(B, S + 1, k) if allocate else 0)
    work = torch.empty(n_work, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    with contextlib.ExitStack() as stack:
        _native.shock_normal_dev(ctx, seed, 0, S, Q, F, d_factor.data_ptr(), antithetic, shocks.data_ptr())
        held = _firm_rows_dev(firm, stack, shocks.data_ptr(), S, Q, tile, rows, bad, new, up)
        at = lambda r, c=0: res.data_ptr() + 8 * (r * (B + 1) + c)
        _native.scenario_tail_select_dev(ctx, B, S + 1, rows.data_ptr(), k, at(0), at(1), work.data_ptr(), base_col=S)
        if allocate:
            _native.scenario_tail_alloc_select_dev(ctx, B, S + 1, rows.data_ptr(), k, at(2, B), at(3, B), at(2), at(3), work.data_ptr(),
                                                   base_col=S)
        ctx.sync()
    del held
    _check_bad_dev(bad, also)
    got = res.cpu().numpy()
    out = {"labels": firm.labels, "var": got[0, :B].copy(), "es": got[1, :B].copy()}
    if allocate:
        out.update(firm_var=float(got[2, B]), firm_es=float(got[3, B]), comp_var=got[2, :B].copy(), comp_es=got[3, :B].copy())
    return out


def embed_ladder_rows(rows, cols, Q: int) -> np.ndarray:
    """``[B, 1 + Q + Q Q]``: ladder rows ``[B, 1 + p + p p]`` on ``p`` columns scattered to the columns ``cols [p]`` of ``Q``;
    the PV slot stays, everything else is +0.0."""
    rows, cols = np.asarray(rows, dtype=np.float64), np.asarray(cols, dtype=np.int64).reshape(-1)
    p = cols.size
    if rows.ndim != 2 or rows.shape[1] != 1 + p + p * p or (p and (cols.min() < 0 or cols.max() >= Q)) or np.unique(cols).size != p:
        raise LibError(f"ladder rows [B, 1 + p + p p] and p distinct columns of {Q} are needed, not {list(rows.shape)} and {p} columns")
    out = np.zeros((rows.shape[0], 1 + Q + Q * Q))
    out[:, 0] = rows[:, 0]
    out[:, 1 + cols] = rows[:, 1:1 + p]
    gamma = out[:, 1 + Q:].reshape(-1, Q, Q)
    gamma[:, cols[:, None], cols[None, :]] = rows[:, 1 + p:].reshape(-1, p, p)
    return out


def firm_ladders(engine, firm: FirmBook, host: bool = False) -> np.ndarray:
    """``[B, 1 + Q + Q Q]``: the desks' delta-gamma ladders on the firm's ``Q`` shock columns, rows in the order of
    ``firm.labels``, as `monte_carlo_var_es` and `monte_carlo_allocate_tail` take them with ``ladders=``.

    Each line prices its own ladders (`price_sub_books`, `price_credit_sub_books`, `price_yoy_sub_books`: one launch chain
    each, on ``engine``; ``host=True``: their CPU twins) and its rows are embedded into the firm's columns by a NumPy scatter
    (`embed_ladder_rows`): rates rows to the curve columns, credit rows to curve + spread, YoY rows to curve + breakeven.  A
    desk's row is its first line's row with the later lines' added, in line order."""
    from .ladder_pnl import ladder_rows
    from .sub_book_ladders import price_credit_sub_books, price_sub_books, price_yoy_sub_books
    c, cols, Q = firm.curves, firm.columns, firm.n_columns
    curve_type = CurveTypes[c.curve_name]
    curve_cols = list(cols["curve"])
    out = [None] * firm.n_desks
    for line in firm.lines:
        if line.kind == "rates":
            got = price_sub_books(engine, c.curve, *line.given, _REQS, host=host, curve_type=curve_type)
            rows = ladder_rows(got["delta"], got["gamma"])
            rows[:, 0] = got["pv"]
            rows = embed_ladder_rows(rows, curve_cols, Q)
        elif line.kind == "credit":
            trades, spreads, keys, buckets = line.given
            got = price_credit_sub_books(engine, c.curve, trades, spreads, keys, buckets, _REQS, host=host, curve_type=curve_type)
            rows = embed_ladder_rows(got["ladders"], curve_cols + list(cols["spread"]), Q)
        else:
            book, keys = line.given
            got = price_yoy_sub_books(engine, c.curve, firm.infl_curve, book._arrays(), keys, _REQS, host=host)
            rows = embed_ladder_rows(got["ladders"], curve_cols + list(cols["breakeven"]), Q)
        if got["labels"] != line.labels:
            raise LibError("the ladders and the revaluation order the desks differently")
        for j, row in zip(line.target, rows):
            out[j] = row.copy() if out[j] is None else out[j] + row
    return np.stack(out)


def monte_carlo_explain_firm_var_es(engine, firm: FirmBook, factor_bp, n_scenarios: int, level: float = 0.99, seed: int = 0,
                                    antithetic: bool = False, host: bool = False, max_bytes: int = 2 ** 31) -> dict:
    """`monte_carlo_explain_var_es` for a `FirmBook`: ``{"labels", "full_var", "full_es", "dg_var", "dg_es", "gap_var",
    "gap_es"}``, ``[B]`` each - `monte_carlo_revalue_firm_var_es` beside `monte_carlo_var_es` on `firm_ladders`' rows, on one
    seed (the generator gives both the same joint shock rows), ``gap = full - dg``."""
    full = monte_carlo_revalue_firm_var_es(firm, factor_bp, n_scenarios, level=level, seed=seed, antithetic=antithetic, host=host,
                                           max_bytes=max_bytes)
    dg = monte_carlo_var_es(None, None, factor_bp, n_scenarios, level=level, seed=seed, antithetic=antithetic, host=host,
                            ctx=None if host else firm.curves.context(), ladders=firm_ladders(engine, firm, host=host))
    return {"labels": full["labels"], "full_var": full["var"], "full_es": full["es"], "dg_var": dg["var"], "dg_es": dg["es"],
            "gap_var": full["var"] - dg["var"], "gap_es": full["es"] - dg["es"]}
