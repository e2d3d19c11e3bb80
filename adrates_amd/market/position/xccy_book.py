"""A book of cross-currency basis swaps of one currency pair under joint scenarios: PV and P&L vectors, whole book and per desk.

Scenario ``s`` is a triple of curve rows - the domestic OIS curve, the foreign OIS curve and the XCCY curve - and a spot:

    PV[s] = dom[s] + frn[s] / spot_s + const_dom + const_for / spot_s

``dom``: the domestic legs on the domestic row (adr_scenario_pv*); ``frn``: the foreign legs with forwards off the foreign row
and discount factors off the XCCY row, in foreign currency (adr_xccy_scenario_pv*, csrc/xccy_scenario_pv.hip); the constants
are the flows dated at the value time (at the base spot their sum is `compile_xccy_legs`' ``pv_const``).  The legs are
compiled once; nothing but curve rows changes between calls.

The XCCY rows of shocked curves come from `shocked_xccy_dfs`: the values-only recurrence of `XccyCurve._bootstrap`, run for all
scenarios at once on the ENGINE grids of the two OIS curves (as `ScenarioGrid`'s rows are).  The base curve was bootstrapped
from the OIS curves' own nodes, so the zero-shock row of this chain is close to ``xccy._dfs`` but need not have its bits
(DESIGN.md has the measured gap): P&L is always taken against the zero-shock row of the SAME chain, priced as one more column
of the same launches, and zero shocks give exactly 0.0.  Spot is a conversion only: the rows are built at the base spot.
"""
from __future__ import annotations

import numpy as np

from ... import _native
from ...market.curves.curve_tables import build_engine_curve
from ...trades.compiler import TradeBatch
from ...utils.error import LibError
from .scenarios import ScenarioGrid, split_sub_books
from .xccy_engine import XccyTerms, compile_xccy_legs, raw_from_swaps, raw_from_terms


def _rows(pair):
    times, dfs = pair
    return np.ascontiguousarray(times, dtype=np.float64).reshape(-1), np.ascontiguousarray(np.atleast_2d(dfs), dtype=np.float64)


def engine_row(curve):
    """``(times, dfs [1, K])`` of an OIS curve on the engine grid (the host builder's, without derivatives)."""
    hit = getattr(curve, "_adr_engine_row", None)
    if hit is None:
        base = build_engine_curve(curve.swap_rates, curve.swap_times, curve.year_fracs, with_hessian=False)
        hit = curve._adr_engine_row = (base.times, base.dfs[None, :].copy())
    return hit


def lookup_rows(method, times, dfs, t) -> np.ndarray:
    """``D_s(t) [S, len(t)]`` on every row of ``dfs`` by the scenario kernel's arithmetic: each date is a unit fixed flow of
    a trade of its own through adr_scenario_pv_host (so the bits are what the kernels read at that date); ``t <= 0`` is 1."""
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    times, dfs = _rows((times, dfs))
    out = np.ones((dfs.shape[0], t.size))
    live = np.nonzero(t > 0.0)[0]
    if live.size:
        m = live.size
        off, zoff, none, ones = np.arange(m + 1, dtype=np.int64), np.zeros(m + 1, dtype=np.int64), np.zeros(0), np.ones(m)
        flows = TradeBatch(off, zoff, t[live], ones.copy(), none, none, none, none, ones.copy(), np.zeros(m), ones.copy(), ones.copy())
        out[:, live] = _native.scenario_pv_host(int(method), times, dfs, flows, per_trade=True)["pv"]
    return out


def _legs(raw):
    """`compile_xccy_legs`' two batches with the flows dated at the value time apart, each side in its own currency (its
    ``pv_const`` is ``const_dom + const_for / spot``): ``(domestic, foreign_legs, const_dom [n], const_for [n])``."""
    domestic, foreign_legs, _ = compile_xccy_legs(raw, 1.0)
    const_dom = _native.exchange_flows_host(raw.dom_exch_t, raw.dom_n, raw.dom_exch, raw.dom_sign, 1.0)[3]
    const_for = _native.exchange_flows_host(raw.for_exch_t, raw.for_n, raw.for_exch, raw.for_sign, 1.0)[3]
    return domestic, foreign_legs, const_dom, const_for


def calibration_legs(xccy):
    """The calibration swaps of ``xccy`` as `compile_xccy_legs` batches: ``(domestic, foreign_legs, const_dom [P], const_for
    [P])``, the constants (flows at the value time) each in its own currency."""
    return _legs(raw_from_swaps(xccy._used_swaps, xccy._value_dt, xccy._dc_type))


def _basis_rows(xccy, basis_shocks_bp):
    base = np.asarray(xccy.basis_spreads, dtype=np.float64)
    if basis_shocks_bp is None:
        return base[None, :]
    x = np.asarray(basis_shocks_bp, dtype=np.float64)
    if x.ndim == 1:
        x = np.repeat(x[:, None], base.size, axis=1)        # one parallel shift per scenario
    if x.ndim != 2 or x.shape[1] != base.size or x.shape[0] < 1:
        raise LibError(f"basis shocks must have shape [n_scenarios, {base.size}] or [n_scenarios], not {list(x.shape)}")
    return base[None, :] + x * 1e-4


def _scenario_count(*counts):
    S = max(counts)
    if any(c not in (1, S) for c in counts):
        raise LibError(f"scenario counts {list(counts)}: each input is one shared row or one row per scenario")
    return S


def shocked_xccy_dfs(xccy, dom=None, foreign=None, basis_shocks_bp=None):
    """The XCCY curve's discount factors under S scenarios: ``(times_x [K_x], dfs_x [S, K_x])``.

    ``dom`` / ``foreign``: ``(times, dfs [S, K])`` rows of the domestic / foreign OIS curve on its engine grid (None: not
    shocked - the base engine row); ``basis_shocks_bp`` ``[S, P_b]`` (or ``[S]``: parallel) added to the pillar spreads as
    ``basis + shock * 1e-4`` (None: not shocked).  Each input holds one row or S.

    The values-only recurrence of `XccyCurve._bootstrap` with arrays of length S in place of floats, one loop over the
    points: the calibration swaps' domestic-leg PVs come from adr_scenario_pv_host on the domestic rows, ``df_ois`` and the
    coupons' forwards from the foreign rows by the kernels' lookup (`lookup_rows`) at the times `_payment_points` records
    (the foreign curve's day count).  The rows are built at the curve's own spot."""
    points = xccy._points
    dc, fc = xccy._domestic_curve, xccy._foreign_curve
    d_t, d_rows = _rows(dom) if dom is not None else engine_row(dc)
    f_t, f_rows = _rows(foreign) if foreign is not None else engine_row(fc)
    basis = _basis_rows(xccy, basis_shocks_bp)
    S = _scenario_count(d_rows.shape[0], f_rows.shape[0], basis.shape[0])
    domestic, _, const_dom, _ = calibration_legs(xccy)
    pv_dom = _native.scenario_pv_host(dc._interp_type.value, d_t, d_rows, domestic, per_trade=True)["pv"] + const_dom[None, :]
    pv_dom = np.broadcast_to(pv_dom, (S, pv_dom.shape[1]))
    when = np.array([[p["t_ois"], p["t_start"], p["t_end"]] for p in points], dtype=np.float64)
    uniq, where = np.unique(when, return_inverse=True)
    D = np.broadcast_to(lookup_rows(fc._interp_type.value, f_t, f_rows, uniq), (S, uniq.size))
    where = where.reshape(when.shape)
    df_ois = lambda i: D[:, where[i, 0]]
    basis = np.broadcast_to(basis, (S, basis.shape[1]))
    spot = xccy._spot_fx
    zero = np.zeros(S)
    dfs, pv_known, cf_mat, prev = [], {}, {}, -1
    for i, p in enumerate(points):
        b = basis[:, p["swap"]]
        if p["is_exchange"]:
            base_cf = p["notional"] if p["is_last"] else -p["notional"]
        else:
            yf = p["year_frac"]
            fwd = (D[:, where[i, 1]] / D[:, where[i, 2]] - 1.0) / max(yf, 1e-10) if yf > 1e-10 else zero
            base_cf = fwd * yf * p["notional"] + (p["notional"] if p["is_last"] else 0.0)
        cashflow = base_cf + b * p["spread_sens"]
        if prev < 0:
            df_mid = df_ois(i) * np.exp(-b * p["time"])
        else:
            df_mid = dfs[prev] * (df_ois(i) / df_ois(prev)) * np.exp(-b * (p["time"] - points[prev]["time"]))
        if p["at_value_dt"]:
            contrib = cashflow * 1.0
        elif not p["is_maturity"]:
            contrib = cashflow * df_mid
        else:
            contrib = zero
        known = pv_known.get(p["swap"], zero) + contrib
        cf_last = cf_mat.get(p["swap"], zero) + (cashflow if p["is_maturity"] else zero)
        pv_known[p["swap"]], cf_mat[p["swap"]] = known, cf_last
        df_final = df_mid
        if p["is_maturity"]:
            den = spot * (-1.0 * cf_last)
            solved = np.abs(den) > 1e-12
            df_final = np.where(solved, -(pv_dom[:, p["swap"]] + spot * (-1.0 * known)) / np.where(solved, den, 1.0), df_mid)
        dfs.append(df_final)
        if not p["at_value_dt"]:
            prev = i
    out = np.ones((S, len(xccy._node_points) + 1))
    for k, i in enumerate(xccy._node_points):
        out[:, k + 1] = dfs[i]
    return np.asarray(xccy._times, dtype=np.float64), out


# ------------------------------------------------------------------------------------------------------------ the book
def _pair_curves(model, dom_index, for_index, dom_ccy, for_ccy):
    """The pair's curves as `xccy_engine._curves_for` finds them, without touching a device."""
    name = f"{for_ccy.name}_{dom_ccy.name}_BASIS"
    try:
        xccy = getattr(model.curves, name)
    except AttributeError:
        raise LibError(f"XCCY curve {name} not found in model.")
    return getattr(model.curves, dom_index.name), getattr(model.curves, for_index.name), xccy


class XccyBook:
    """Cross-currency basis swaps of ONE currency pair (`XccyBasisSwap` objects or `XccyTerms`) on ``model``'s two OIS curves
    and its XCCY curve; the legs are compiled once (`compile_xccy_legs`)."""

    def __init__(self, swaps_or_terms, model):
        one = lambda v: v[0] if isinstance(v, (list, tuple, np.ndarray)) else v
        if isinstance(swaps_or_terms, XccyTerms):
            t = swaps_or_terms
            pair = (one(t.domestic_floating_index), one(t.foreign_floating_index), one(t.domestic_currency), one(t.foreign_currency))
        else:
            swaps_or_terms = list(swaps_or_terms)
            if not swaps_or_terms:
                raise LibError("XccyBook needs at least one swap (the book's currency pair names its curves)")
            pairs = {(s._domestic_floating_index, s._foreign_floating_index, s._domestic_currency, s._foreign_currency)
                     for s in swaps_or_terms}
            if len(pairs) != 1:
                raise LibError("a book of cross-currency swaps must share its currencies and floating indices")
            pair = next(iter(pairs))
        self.model = model
        self.dom_index, self.for_index = pair[0], pair[1]
        self.dom_curve, self.for_curve, self.xccy = _pair_curves(model, *pair)
        self.spot = float(self.xccy._spot_fx)
        xdc = self.xccy._dc_type
        raw = (raw_from_terms(swaps_or_terms, model.value_dt, xdc) if isinstance(swaps_or_terms, XccyTerms)
               else raw_from_swaps(swaps_or_terms, model.value_dt, xdc))
        self.domestic, self.foreign_legs, self.const_dom, self.const_for = _legs(raw)

    def __len__(self):
        return int(self.domestic.n_trades)

    # ----------------------------------------------------------------------------------------------- scenario rows
    def _ois_rows(self, grid, curve, name, host):
        """``(times, dfs [S + 1, K])`` of one OIS curve with the unshocked row LAST, or its base row alone (None).  ``grid``: a
        `ScenarioGrid` on that curve (its rows and its host base curve) or par-quote shocks in basis points ``[S, P]``, turned
        into rows by `ShockedCurves.dfs` with a row of zeros appended: the base row goes through the same chain."""
        if grid is None:
            return engine_row(curve)
        if isinstance(grid, ScenarioGrid):
            if grid.curve_name != name or grid.model.value_dt != self.model.value_dt:
                raise LibError(f"the grid shocks {grid.curve_name}, this side of the book is on {name} (same value date needed)")
            return grid._with_base()
        from .monte_carlo import ShockedCurves
        x = np.atleast_2d(np.asarray(grid, dtype=np.float64))
        sc = ShockedCurves(self.model, name, ctx=None if host else _native.default_context())
        if x.shape[1] != sc.n_pillars:
            raise LibError(f"shocks of {name} must have shape [n_scenarios, {sc.n_pillars}], not {list(x.shape)}")
        try:
            dfs, bad = sc.dfs(np.vstack([x, np.zeros((1, x.shape[1]))]), host=host)
        finally:
            sc.close()
        if np.any(bad):
            raise LibError(f"scenario {int(np.nonzero(bad)[0][0])} of {name} has no curve (a discount factor is not positive)")
        return sc.base.times, dfs

    def scenario_rows(self, dom_grid=None, for_grid=None, basis_shocks_bp=None, spot=None, host=False):
        """``(dom, foreign, xccy, spot [S + 1], S)``: the three curves' ``(times, dfs)`` rows with the unshocked scenario as the
        LAST row (a curve that is not shocked holds its one base row) and the spots with the base spot last."""
        if dom_grid is None and for_grid is None and basis_shocks_bp is None and spot is None:
            raise LibError("no scenarios: give dom_grid, for_grid, basis_shocks_bp or spot")
        dom = self._ois_rows(dom_grid, self.dom_curve, self.dom_index.name, host)
        frn = self._ois_rows(for_grid, self.for_curve, self.for_index.name, host)
        shocks = None
        if basis_shocks_bp is not None:
            x = np.asarray(basis_shocks_bp, dtype=np.float64)
            shocks = np.concatenate([x, np.zeros((1,) + x.shape[1:])])
        spots = np.full(1, self.spot)
        if spot is not None:
            spots = np.concatenate([np.asarray(spot, dtype=np.float64).reshape(-1), [self.spot]])
            if not np.all(spots > 0.0):
                raise LibError("spot must be positive")
        xrows = shocked_xccy_dfs(self.xccy, dom if dom_grid is not None else None, frn if for_grid is not None else None, shocks)
        S1 = _scenario_count(np.atleast_2d(dom[1]).shape[0], np.atleast_2d(frn[1]).shape[0], xrows[1].shape[0], spots.size)
        return dom, frn, xrows, np.broadcast_to(spots, (S1,)), S1 - 1

    # ------------------------------------------------------------------------------------------------ revaluation
    def revalue(self, dom_grid=None, for_grid=None, basis_shocks_bp=None, spot=None, per_trade=False, host=False) -> dict:
        """The book's PV in domestic currency under joint scenarios: ``{"book_pv": [S]}`` and, with ``per_trade``, ``"pv" [S, n]``.

        ``dom_grid`` / ``for_grid``: a `ScenarioGrid` on the domestic / foreign OIS curve, or par-quote shocks in basis points
        ``[S, P]``; ``basis_shocks_bp``: ``[S, P_b]`` (or ``[S]``: parallel shifts) on the XCCY curve's pillar spreads; ``spot``:
        ``[S]`` spots (a conversion only).  What is None is not shocked; the counts of what is given must agree.  Two launches:
        the domestic legs on adr_scenario_pv*, the foreign legs on adr_xccy_scenario_pv*; ``host=True`` runs the CPU twins."""
        dom, frn, xr, spots, S = self.scenario_rows(dom_grid, for_grid, basis_shocks_bp, spot, host)
        out = revalue_xccy_on_curves(self, dom, frn, xr, spots, per_trade=per_trade, host=host)
        return {k: v[:S] for k, v in out.items()}

    def pnl(self, dom_grid=None, for_grid=None, basis_shocks_bp=None, spot=None, host=False) -> np.ndarray:
        """``[S]``: `revalue` minus the PV of the unshocked scenario, one more column of the same launches on the same
        chain's zero-shock rows: zero shocks give exactly 0.0."""
        dom, frn, xr, spots, S = self.scenario_rows(dom_grid, for_grid, basis_shocks_bp, spot, host)
        book = revalue_xccy_on_curves(self, dom, frn, xr, spots, host=host)["book_pv"]
        return book[:-1] - book[-1]

    def revalue_sub_books(self, keys, dom_grid=None, for_grid=None, basis_shocks_bp=None, spot=None, per_trade=False,
                          host=False) -> dict:
        """`revalue` per sub-book in the same two launches (adr_scenario_subbook_pv*, adr_xccy_scenario_subbook_pv*): ``keys``
        holds one hashable value per swap.  ``{"labels": [...], "sub_pv": [B, S]}``, labels in order of first appearance, and
        with ``per_trade`` ``"pv" [S, n]`` in the book's order."""
        dom, frn, xr, spots, S = self.scenario_rows(dom_grid, for_grid, basis_shocks_bp, spot, host)
        out = revalue_xccy_on_curves_sub_books(self, dom, frn, xr, keys, spots, per_trade=per_trade, host=host)
        return {k: (v if k == "labels" else v[:S] if k == "pv" else v[:, :S]) for k, v in out.items()}

    def pnl_sub_books(self, keys, dom_grid=None, for_grid=None, basis_shocks_bp=None, spot=None, host=False) -> np.ndarray:
        """``[B, S]``: `pnl` per sub-book (rows in the order of `revalue_sub_books`' labels); zero shocks give 0.0 in every row."""
        dom, frn, xr, spots, S = self.scenario_rows(dom_grid, for_grid, basis_shocks_bp, spot, host)
        sub = revalue_xccy_on_curves_sub_books(self, dom, frn, xr, keys, spots, host=host)["sub_pv"]
        return sub[:, :-1] - sub[:, -1:]


def _methods(book):
    return book.dom_curve._interp_type.value, book.for_curve._interp_type.value, book.xccy._interp_type.value


def _spots(book, spot, S):
    s = np.full(1, book.spot) if spot is None else np.asarray(spot, dtype=np.float64).reshape(-1)
    if s.size != 1 and S != 1 and s.size != S:
        raise LibError(f"{s.size} spots for {S} scenarios")
    return np.broadcast_to(s, (max(S, s.size),))


def _launch_pair(book, dom, frn, xr, domestic, foreign_legs, per_trade, host, ctx, sub_off=None):
    """The two launches on the curve rows: ``(domestic result, foreign result, S)``; a single domestic row is priced once."""
    (d_t, d_rows), (f_t, f_rows), (x_t, x_rows) = _rows(dom), _rows(frn), _rows(xr)
    S = _scenario_count(d_rows.shape[0], f_rows.shape[0], x_rows.shape[0])
    dm, fm, xm = _methods(book)
    sub = () if sub_off is None else (sub_off,)
    name = "scenario_subbook_pv" if sub else "scenario_pv"
    if host:
        d = getattr(_native, name + "_host")(dm, d_t, d_rows, domestic, *sub, per_trade=per_trade)
        f = getattr(_native, "xccy_" + name + "_host")(fm, f_t, f_rows, xm, x_t, x_rows, foreign_legs, *sub, per_trade=per_trade)
    else:
        ctx = ctx or _native.default_context()
        dom_tr, for_tr = _native.upload_many(ctx, [domestic, foreign_legs])
        try:
            d = getattr(_native, name)(ctx, dm, d_t, d_rows, dom_tr, *sub, per_trade=per_trade)
            f = getattr(_native, "xccy_" + name)(ctx, fm, f_t, f_rows, xm, x_t, x_rows, for_tr, *sub, per_trade=per_trade)
        finally:
            dom_tr.close(); for_tr.close()
    return d, f, S


def revalue_xccy_on_curves(book: XccyBook, dom, foreign, xccy, spot=None, per_trade=False, host=False, ctx=None) -> dict:
    """PVs of a compiled `XccyBook` under caller-supplied curve rows (historical simulation): ``dom``, ``foreign``, ``xccy`` are
    ``(times, dfs [S, K])`` pairs on the three curves' grids - each one shared row or one row per scenario; `shocked_xccy_dfs`
    makes XCCY rows that fit shocked OIS rows - and ``spot`` ``[S]`` or None (the base spot).  ``{"book_pv": [S]}`` and, with
    ``per_trade``, ``"pv" [S, n]``, in domestic currency."""
    d, f, S = _launch_pair(book, dom, foreign, xccy, book.domestic, book.foreign_legs, per_trade, host, ctx)
    spots = _spots(book, spot, S)
    const = float(book.const_dom.sum()) + float(book.const_for.sum()) / spots
    out = {"book_pv": d["book_pv"] + f["book_pv"] / spots + const}
    if per_trade:
        out["pv"] = d["pv"] + f["pv"] / spots[:, None] + (book.const_dom[None, :] + book.const_for[None, :] / spots[:, None])
    return out


def revalue_xccy_on_curves_sub_books(book: XccyBook, dom, foreign, xccy, keys, spot=None, per_trade=False, host=False,
                                     ctx=None) -> dict:
    """`revalue_xccy_on_curves` per sub-book in the same two launches: ``{"labels", "sub_pv" [B, S]}`` (and ``"pv" [S, n]`` in
    the book's order), rows in the shape `combine_sub_book_rows`, `tail_measures`, `tail_measures_select` and `allocate_tail`
    take.  Row ``b`` is the domestic sub-book row plus the foreign one over the spot: each has the bits of its whole-book call
    on that desk alone."""
    n = len(book)
    order = np.arange(n, dtype=np.int64)
    sd = split_sub_books(book.domestic, book.const_dom, order, keys)
    sf = split_sub_books(book.foreign_legs, book.const_for, order, keys)
    d, f, S = _launch_pair(book, dom, foreign, xccy, sd.batch, sf.batch, per_trade, host, ctx, sd.sub_off)
    spots = _spots(book, spot, S)
    cuts = list(zip(sd.sub_off[:-1], sd.sub_off[1:]))
    cd = np.array([float(sd.pv_const[lo:hi].sum()) for lo, hi in cuts])
    cf = np.array([float(sf.pv_const[lo:hi].sum()) for lo, hi in cuts])
    out = {"labels": sd.labels, "sub_pv": d["sub_pv"] + f["sub_pv"] / spots[None, :] + (cd[:, None] + cf[:, None] / spots[None, :])}
    if per_trade:
        pv = d["pv"] + f["pv"] / spots[:, None] + (sd.pv_const[None, :] + sf.pv_const[None, :] / spots[:, None])
        back = np.empty_like(pv)
        back[:, sd.order] = pv
        out["pv"] = back
    return out
