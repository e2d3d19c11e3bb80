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
from ...utils.helpers import to_tenor
from .engine import Engine
from .inflation_engine import inflation_inputs, price_yoy, yoy_curves
from .scenarios import (revalue_yoy_on_curves, revalue_yoy_on_curves_sub_books, shocked_breakevens, split_yoy_sub_books,
                        tail_count, yoy_book_arrays, _finish_yoy_sub_books)
from .sub_book_ladders import price_yoy_sub_books


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

    # ------------------------------------------------------------------------------------------ scenario revaluation
    def _arrays(self):
        """The book's fixed legs and YoY coupons, compiled once against the model's value date."""
        if getattr(self, "_compiled", None) is None:
            self._compiled = yoy_book_arrays(self.swaps, self.model.value_dt)
        return self._compiled

    def _breakeven_rows(self, grid, inflation_shocks, breakevens):
        """``b`` [S, P] or None (the inflation curve is not shocked), after checking the scenario counts."""
        if inflation_shocks is not None and breakevens is not None:
            raise LibError("give inflation_shocks or breakevens, not both")
        b = None
        if inflation_shocks is not None:
            b = np.array([shocked_breakevens(self.inflation_curve, s) for s in inflation_shocks], dtype=np.float64)
        elif breakevens is not None:
            b = np.asarray(breakevens, dtype=np.float64)
        P = len(self.inflation_curve.swap_times)
        if b is not None and (b.ndim != 2 or b.shape[1] != P or b.shape[0] < 1):
            raise LibError(f"breakeven scenarios must have shape [n_scenarios, {P}], not {list(b.shape)}")
        if grid is None and b is None:
            raise LibError("no scenarios: give a ScenarioGrid on the discount curve, inflation_shocks or breakevens")
        if grid is not None:
            if grid.curve_name != self.curve_type.name or grid.model.value_dt != self.model.value_dt:
                raise LibError(f"the grid shocks {grid.curve_name}, the book discounts on {self.curve_type.name} "
                               "(same value date needed)")
            if b is not None and b.shape[0] != len(grid):
                raise LibError(f"{len(grid)} discount scenarios but {b.shape[0]} inflation scenarios")
        return b

    def _revalue_in_place(self, grid, b, per_trade):
        """One launch of adr_yoy_scenario_pv_dev that reads the grid's discount factors where the device builder left
        them (adr_curve_set_arrays): only the book, the breakeven rows and the results cross the bus."""
        import torch
        ctx = grid._ctx
        arr = _native.curve_set_arrays(grid._set)
        (fix_off, fix_tp, fix_pay), book = self._arrays()
        cpn_off, cpn = _native.yoy_pack(book)
        im, T, b0 = inflation_inputs(self.inflation_curve)
        rows = b0[None, :] if b is None else b
        dev = torch.device("cuda", ctx.device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        t = {k: up(v) for k, v in dict(T=T, b=rows, fix_off=fix_off, fix_tp=fix_tp, fix_pay=fix_pay, cpn_off=cpn_off,
                                       cpn=cpn).items()}
        S, n = arr["S"], len(self.swaps)
        out_book = torch.empty(S, dtype=torch.float64, device=dev)
        pv = torch.empty((n, S), dtype=torch.float64, device=dev) if per_trade else None
        work = torch.empty(_native.yoy_scenario_pv_work(n, S), dtype=torch.float64, device=dev)
        ptrs = {k: v.data_ptr() if v.numel() else 0 for k, v in t.items()}
        ptrs.update(times=arr["times"], dfs=arr["dfs"])
        torch.cuda.synchronize(dev)
        _native.yoy_scenario_pv_dev(ctx, arr["method"], arr["K"], S, im, T.size, rows.shape[0], S, n, fix_tp.size, cpn.shape[1],
                                    ptrs, out_book.data_ptr(), work.data_ptr(), pv.data_ptr() if per_trade else 0)
        ctx.sync()
        out = {"book_pv": out_book.cpu().numpy()}
        if per_trade:
            out["pv"] = pv.cpu().numpy().T
        return out

    def revalue(self, grid=None, inflation_shocks=None, breakevens=None, per_trade: bool = False) -> dict:
        """The book's PV under joint scenarios, in ONE launch of csrc/yoy_scenario_pv.hip: ``{"book_pv": [S]}`` and,
        with ``per_trade``, ``"pv": [S, n]``.

        ``grid``: a `ScenarioGrid` on the book's discount curve - scenario s discounts on the grid's curve s, read in
        place on the device; None: the discount curve is not shocked.  ``inflation_shocks``: a list of shocks in basis
        points for `shocked_breakevens` (a float shifts every pillar, a dict the named tenors), or ``breakevens``: a
        ready ``[S, P]`` array of breakeven rates (historical simulation); neither: the inflation curve is not
        shocked.  Where both curves are shocked the counts must agree: scenario s is the PAIR (discount curve s,
        breakeven row s).  The result feeds `historical_var` / `expected_shortfall` through `pnl`."""
        b = self._breakeven_rows(grid, inflation_shocks, breakevens)
        if grid is not None:
            return self._revalue_in_place(grid, b, per_trade)
        host = self._engine._device_curve(self.curve)["host"]
        im, T, _ = inflation_inputs(self.inflation_curve)
        return revalue_yoy_on_curves(self.curve._interp_type.value, host.times, host.dfs, im, T, b, self._arrays(),
                                     self.model.value_dt, per_trade=per_trade, ctx=self._engine._device_curve(self.curve)["ctx"])

    def pnl(self, grid=None, inflation_shocks=None, breakevens=None) -> np.ndarray:
        """``[S]``: the book's PV under each scenario minus its PV on the unshocked pair, which the same launch prices
        as one more scenario row (as `ScenarioGrid.pnl` does: the grid's rows are downloaded once and the host
        builder's base curve appended), so the difference carries no noise between kernels and a zero shock gives
        exactly 0."""
        b = self._breakeven_rows(grid, inflation_shocks, breakevens)
        im, T, _ = inflation_inputs(self.inflation_curve)
        times, dfs, rows, ctx = self._base_pair(grid, b)
        book = revalue_yoy_on_curves(self.curve._interp_type.value, times, dfs, im, T, rows, self._arrays(),
                                     self.model.value_dt, ctx=ctx)["book_pv"]
        return book[:-1] - book[-1]

    def pnl_delta_gamma(self, grid=None, inflation_shocks=None, breakevens=None, cross: bool = False) -> np.ndarray:
        """``[S]``: `pnl` to second order from the book's ladders (`compute` with ``aggregate``), without a revaluation:
        the discount ladders under the grid's shocks plus the inflation ladders under the breakeven shocks in basis
        points (``inflation_shocks`` as they are, ``breakevens`` as ``(b - b0) * 1e4``) - two `ladder_pnl` calls.  There
        is no discount x inflation cross term, as in the engine's Greeks, so with both curves shocked the gap to `pnl`
        is second order.  ``cross=True`` takes the ladders of `compute_sub_books` with one desk instead, which hold the
        cross block: the gap to `pnl` is then third order under joint shocks too (`pnl_delta_gamma_sub_books`' row).
        Scenarios and their checks: see `revalue`."""
        if cross:
            return self.pnl_delta_gamma_sub_books([0] * len(self.swaps), grid, inflation_shocks, breakevens)["pnl"][0]
        from .ladder_pnl import ladder_pnl, shock_matrix_bp
        b = self._breakeven_rows(grid, inflation_shocks, breakevens)
        res = self.compute({RequestTypes.VALUE, RequestTypes.DELTA, RequestTypes.GAMMA}, per_trade=False, aggregate=True)
        ctx = self._engine._device_curve(self.curve)["ctx"]
        pnl = None
        if grid is not None:
            pnl = ladder_pnl(res["agg_delta"][None, :], res["agg_gamma"][None, :, :], grid.shocks_bp(), ctx=ctx)[0]
        if b is not None:
            if inflation_shocks is not None:
                x = shock_matrix_bp(res["infl_tenors"], inflation_shocks, 1.0)
            else:
                x = (b - inflation_inputs(self.inflation_curve)[2][None, :]) * 1e4
            infl = ladder_pnl(res["agg_infl_delta"][None, :], res["agg_infl_gamma"][None, :, :], x, ctx=ctx)[0]
            pnl = infl if pnl is None else pnl + infl
        return pnl

    # ---------------------------------------------------------------------------------------------------- sub-books
    def _sub_books_on_device(self, ctx, sb, method, times, dfs, b, per_trade=False, tail=None):
        """One launch of adr_yoy_scenario_subbook_pv_dev on the ctx's own stream.  ``times`` / ``dfs``: host arrays
        (``dfs [S_disc, K]``) or device pointers ``(K, S_disc, times_ptr, dfs_ptr)``; ``b [S_infl, P]``.  ``tail``:
        ``(base_col, k)`` chains adr_scenario_tail_dev behind it and returns ``(var, es)``; the rows then stay on the
        device."""
        import torch
        dev = torch.device("cuda", ctx.device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        fixed, book = sb.fixed, sb.coupons
        cpn_off, cpn = _native.yoy_pack(book)
        im, T, _ = inflation_inputs(self.inflation_curve)
        n, B = cpn_off.size - 1, sb.sub_off.size - 1
        held = dict(T=up(T), b=up(b), fix_off=up(fixed[0]), fix_tp=up(fixed[1]), fix_pay=up(fixed[2]), cpn_off=up(cpn_off),
                    cpn=up(cpn), plan=up(_native.scenario_subbook_plan(n, sb.sub_off)))
        if isinstance(times, tuple):
            K, S_disc, times_ptr, dfs_ptr = times
        else:
            held.update(times=up(np.asarray(times, dtype=np.float64)), dfs=up(np.atleast_2d(np.asarray(dfs, dtype=np.float64))))
            K, S_disc = held["times"].numel(), held["dfs"].shape[0]
            times_ptr, dfs_ptr = held["times"].data_ptr(), held["dfs"].data_ptr()
        S = max(S_disc, b.shape[0])
        ptrs = {k: v.data_ptr() if v.numel() else 0 for k, v in held.items()}
        ptrs.update(times=times_ptr, dfs=dfs_ptr)
        sub = torch.empty((B, S), dtype=torch.float64, device=dev)
        pv = torch.empty((n, S), dtype=torch.float64, device=dev) if per_trade else None
        work = torch.empty(_native.scenario_subbook_work(n, B, S), dtype=torch.float64, device=dev)
        var_es = torch.empty((2, B), dtype=torch.float64, device=dev) if tail else None
        torch.cuda.synchronize(dev)
        _native.yoy_scenario_subbook_pv_dev(ctx, method, K, S_disc, im, T.size, b.shape[0], S, n, fixed[1].size, cpn.shape[1], B,
                                            ptrs, sub.data_ptr(), work.data_ptr(), pv.data_ptr() if per_trade else 0)
        if tail:
            _native.scenario_tail_dev(ctx, B, S, sub.data_ptr(), tail[1], var_es[0].data_ptr(), var_es[1].data_ptr(),
                                      base_col=tail[0])
        ctx.sync()
        if tail:
            out = var_es.cpu().numpy()
            return out[0].copy(), out[1].copy()
        out = {"sub_pv": sub.cpu().numpy()}
        if per_trade:
            out["pv"] = pv.cpu().numpy().T
        return out

    def _split(self, keys):
        return split_yoy_sub_books(*self._arrays(), keys)

    def _base_pair(self, grid, b):
        """``(times, dfs, breakeven rows, ctx)`` with the unshocked pair appended as one more scenario (the grid's rows with
        the host builder's base curve, `ScenarioGrid._with_base`): what `pnl` and the sub-book forms price."""
        _, _, b0 = inflation_inputs(self.inflation_curve)
        if grid is not None:
            (times, dfs), ctx = grid._with_base(), grid._ctx
        else:
            cur = self._engine._device_curve(self.curve)
            times, dfs, ctx = cur["host"].times, cur["host"].dfs, cur["ctx"]
        return times, dfs, (b0 if b is None else np.vstack([b, b0[None, :]])), ctx

    def revalue_sub_books(self, keys, grid=None, inflation_shocks=None, breakevens=None, per_trade: bool = False) -> dict:
        """`revalue` per sub-book, in the SAME single launch: ``keys`` holds one hashable value per swap (a desk, a
        counterparty, a margin account).  Returns ``{"labels": [...], "sub_pv": [B, S]}`` - the labels in order of first
        appearance, row ``b`` bit for bit `revalue`'s ``book_pv`` of a `YoYBook` holding sub-book ``labels[b]`` alone - and,
        with ``per_trade``, ``"pv": [S, n]`` in the book's order.  Scenarios: see `revalue`."""
        b = self._breakeven_rows(grid, inflation_shocks, breakevens)
        im, T, b0 = inflation_inputs(self.inflation_curve)
        if grid is not None:
            sb = self._split(keys)
            arr = _native.curve_set_arrays(grid._set)
            out = self._sub_books_on_device(grid._ctx, sb, arr["method"], (arr["K"], arr["S"], arr["times"], arr["dfs"]), None,
                                            b0[None, :] if b is None else b, per_trade)
            return _finish_yoy_sub_books(out, sb, per_trade)
        cur = self._engine._device_curve(self.curve)
        return revalue_yoy_on_curves_sub_books(self.curve._interp_type.value, cur["host"].times, cur["host"].dfs, im, T, b,
                                               self._arrays(), keys, self.model.value_dt, per_trade=per_trade, ctx=cur["ctx"])

    def _pnl_sub_books(self, keys, grid, inflation_shocks, breakevens):
        """``(labels, pnl [B, S])`` of `pnl_sub_books`."""
        b = self._breakeven_rows(grid, inflation_shocks, breakevens)
        im, T, _ = inflation_inputs(self.inflation_curve)
        times, dfs, rows, ctx = self._base_pair(grid, b)
        sub = revalue_yoy_on_curves_sub_books(self.curve._interp_type.value, times, dfs, im, T, rows, self._arrays(), keys,
                                              self.model.value_dt, ctx=ctx)
        return sub["labels"], sub["sub_pv"][:, :-1] - sub["sub_pv"][:, -1:]

    def pnl_sub_books(self, keys, grid=None, inflation_shocks=None, breakevens=None) -> np.ndarray:
        """``[B, S]``: `pnl` per sub-book (rows in the order of `revalue_sub_books`' labels).  The unshocked pair is priced
        as one more column of the same launch, so a zero shock is exactly 0 in every row."""
        return self._pnl_sub_books(keys, grid, inflation_shocks, breakevens)[1]

    def sub_book_var_es(self, keys, level: float = 0.99, grid=None, inflation_shocks=None, breakevens=None) -> dict:
        """``{"labels": [...], "var": [B], "es": [B]}``: the sub-book launch and the tail kernel chained on one stream, so
        the ``[B, S]`` matrix never leaves the device.  The P&L is `pnl_sub_books`'; ``var`` and ``es`` are
        `tail_measures`'."""
        b = self._breakeven_rows(grid, inflation_shocks, breakevens)
        times, dfs, rows, ctx = self._base_pair(grid, b)
        rows, dfs = np.atleast_2d(rows), np.atleast_2d(dfs)
        S = max(rows.shape[0], dfs.shape[0]) - 1
        if S > _native.SCENARIO_TAIL_MAX:
            raise LibError(f"{S} scenarios: at most {_native.SCENARIO_TAIL_MAX} fit the tail kernel; use pnl_sub_books and "
                           "tail_measures")
        sb = self._split(keys)
        var, es = self._sub_books_on_device(ctx, sb, self.curve._interp_type.value, times, dfs, rows,
                                            tail=(S, tail_count(level, S)))
        return {"labels": sb.labels, "var": var, "es": es}

    # ------------------------------------------------------------------------------------------- sub-book Greeks
    def compute_sub_books(self, request_list, keys, host: bool = False) -> dict:
        """`compute` per sub-book from ONE launch chain (`price_yoy_sub_books`, adr_yoy_subbook_ladders): ``keys`` holds one
        hashable value per swap.  ``{"labels", "pv" [B], "delta" [B, Q], "gamma" [B, Q, Q], "tenors", "infl_tenors",
        "ladders"}`` on ``Q = P_d + P_i`` columns, the discount pillars first; ``gamma`` holds the discount block, the
        breakeven block and the discount x breakeven cross block, which `compute` does not have."""
        reqs = set(request_list)
        if not reqs & {RequestTypes.VALUE, RequestTypes.DELTA, RequestTypes.GAMMA}:
            raise LibError("YoYBook.compute_sub_books needs VALUE, DELTA or GAMMA")
        return price_yoy_sub_books(self._engine, self.curve, self.inflation_curve, self._arrays(), keys, reqs, host=host)

    def _joint_shocks_bp(self, grid, inflation_shocks, breakevens):
        """``[S, P_d + P_i]`` basis points (`yoy_shock_matrix_bp`); a curve that is not shocked has a row of zeros."""
        from .ladder_pnl import shock_matrix_bp, yoy_shock_matrix_bp
        b = self._breakeven_rows(grid, inflation_shocks, breakevens)
        b0 = inflation_inputs(self.inflation_curve)[2]
        x = np.zeros((1, len(self.curve.swap_times))) if grid is None else grid.shocks_bp()
        if inflation_shocks is not None:
            return yoy_shock_matrix_bp(x, infl_shocks_bp=shock_matrix_bp(to_tenor(list(self.inflation_curve.swap_times)),
                                                                         inflation_shocks, 1.0))
        return yoy_shock_matrix_bp(x, b0[None, :] if b is None else b, b0)

    def pnl_delta_gamma_sub_books(self, keys, grid=None, inflation_shocks=None, breakevens=None, parts: bool = False,
                                  cross: bool = True, host: bool = False) -> dict:
        """`pnl_sub_books` to second order without a revaluation: `compute_sub_books`' ladders (one launch chain) times the
        joint shocks (`ladder_pnl`, one kernel),

            delta . x + x' Gamma x / 2 + delta_i . y + y' Gamma_i y / 2 + y' C x,

        ``x`` the grid's par-quote shocks and ``y`` the breakeven moves in basis points, ``C`` the cross block.  Returns
        `compute_sub_books`' dict plus ``"pnl" [B, S]`` and, with ``parts``, ``"delta_pnl"`` and ``"gamma_pnl"``.
        ``cross=False`` leaves the cross block out: the engine's Greeks, second-order gap under joint shocks."""
        from .ladder_pnl import augmented_ladder_pnl
        shocks = self._joint_shocks_bp(grid, inflation_shocks, breakevens)
        out = self.compute_sub_books({RequestTypes.VALUE, RequestTypes.DELTA, RequestTypes.GAMMA}, keys, host=host)
        rows = out["ladders"]
        if not cross:
            P, Q = len(out["tenors"]), shocks.shape[1]
            g = rows.copy()[:, 1 + Q:].reshape(-1, Q, Q)
            g[:, :P, P:] = 0.0
            g[:, P:, :P] = 0.0
            rows = np.hstack([rows[:, :1 + Q], g.reshape(g.shape[0], Q * Q)])
        ctx = None if host else self._engine._device_curve(self.curve)["ctx"]
        pnl = augmented_ladder_pnl(rows, shocks, parts=parts, host=host, ctx=ctx)
        out.update(pnl if parts else {"pnl": pnl})
        return out

    def explain_sub_books(self, keys, grid=None, inflation_shocks=None, breakevens=None, cross: bool = True) -> dict:
        """P&L explain per inflation desk and scenario: ``{"labels", "full", "delta_pnl", "gamma_pnl", "unexplained"}``, all
        ``[B, S]`` - ``full`` is `pnl_sub_books`' full revaluation under the joint scenarios, the parts are
        `pnl_delta_gamma_sub_books`', and ``unexplained = full - (delta_pnl + gamma_pnl)``: third order in the shocks, second
        order with ``cross=False``."""
        keys = list(keys)
        labels, full = self._pnl_sub_books(keys, grid, inflation_shocks, breakevens)
        dg = self.pnl_delta_gamma_sub_books(keys, grid, inflation_shocks, breakevens, parts=True, cross=cross)
        assert dg["labels"] == labels and full.shape == dg["pnl"].shape, "the two routes order the desks differently"
        return {"labels": labels, "full": full, "delta_pnl": dg["delta_pnl"], "gamma_pnl": dg["gamma_pnl"],
                "unexplained": full - (dg["delta_pnl"] + dg["gamma_pnl"])}

    def sub_book_delta_gamma_var_es(self, keys, level: float = 0.99, grid=None, inflation_shocks=None, breakevens=None) -> dict:
        """``{"labels": [...], "var": [B], "es": [B]}`` of the delta-gamma P&L straight from the book: the ladder chain
        (adr_yoy_subbook_ladders_dev), the P&L kernel (adr_ladder_pnl_dev on the augmented rows) and the tail kernel
        (adr_scenario_tail_dev) on one stream, so neither the ladders nor the ``[B, S]`` matrix leave the device.  ``var``
        and ``es`` are `tail_measures`' of `pnl_delta_gamma_sub_books`' ``pnl``, bit for bit.  The buffers are torch tensors;
        where torch brings a HIP runtime of its own, import torch before the first call into this library, as the tools do."""
        import torch
        shocks_bp = self._joint_shocks_bp(grid, inflation_shocks, breakevens)
        S, Q = shocks_bp.shape
        if S > _native.SCENARIO_TAIL_MAX:
            raise LibError(f"{S} scenarios: at most {_native.SCENARIO_TAIL_MAX} fit the tail kernel; use "
                           "pnl_delta_gamma_sub_books and tail_measures")
        if Q > _native.LADDER_PNL_MAX_PILLARS:
            raise LibError(f"{Q} columns: at most {_native.LADDER_PNL_MAX_PILLARS} fit the P&L kernel")
        sb = self._split(keys)
        cur = self._engine._device_curve(self.curve)
        ctx, curve = cur["ctx"], cur["dev"]
        im, T, b0 = inflation_inputs(self.inflation_curve)
        cpn_off, cpn = _native.yoy_pack(sb.coupons)
        n, B = cpn_off.size - 1, sb.sub_off.size - 1
        dev = torch.device("cuda", ctx.device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
        bufs = dict(T=up(T), b=up(b0), fix_off=up(sb.fixed[0]), fix_tp=up(sb.fixed[1]), fix_pay=up(sb.fixed[2]), cpn_off=up(cpn_off),
                    cpn=up(cpn), plan=up(_native.scenario_subbook_plan(n, sb.sub_off)))
        shocks = up(shocks_bp)
        ladders, work = new(B, 1 + Q + Q * Q), new(_native.yoy_subbook_ladders_work(curve, T.size, n, B)[0])
        pnl, var_es = new(B, S), new(2, B)
        torch.cuda.synchronize(dev)
        _native.yoy_subbook_ladders_dev(ctx, curve, im, T.size, n, sb.fixed[1].size, cpn.shape[1], B,
                                        {k: v.data_ptr() if v.numel() else 0 for k, v in bufs.items()},
                                        _native.REQ_VALUE | _native.REQ_DELTA | _native.REQ_GAMMA, ladders.data_ptr(),
                                        work.data_ptr())
        _native.ladder_pnl_dev(ctx, B, Q, ladders.data_ptr(), S, shocks.data_ptr(), pnl.data_ptr())
        _native.scenario_tail_dev(ctx, B, S, pnl.data_ptr(), tail_count(level, S), var_es[0].data_ptr(), var_es[1].data_ptr(),
                                  base_col=-1)
        ctx.sync()
        out = var_es.cpu().numpy()
        return {"labels": sb.labels, "var": out[0].copy(), "es": out[1].copy()}
