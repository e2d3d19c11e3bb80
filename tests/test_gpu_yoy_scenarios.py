"""Inflation scenario revaluation on the GPU (csrc/yoy_scenario_pv.hip): the independent reference (C oracle + MpYoY)
and the host twin on the books of tests/_yoy_scenario_cases.py, launch shapes bit for bit against scenarios priced
alone, the global-memory fallback for tables that do not fit the LDS together, the device-array entry on a caller's
stream with guarded buffers and malformed offsets, and `YoYBook.revalue` / `pnl` against the per-scenario loop."""
import numpy as np
import pytest
import torch

from adrates_amd import _native
from adrates_amd.market.position.inflation_engine import inflation_inputs
from adrates_amd.market.position.scenarios import ScenarioGrid, historical_var, shocked_breakevens
from adrates_amd.market.position.yoy_book import YoYBook
from adrates_amd.trades.market_data import GBP_PX, INFL_PX, gbp_model, inflation_curve, random_yoy_book, yoy_model
from adrates_amd.utils import RequestTypes
from adrates_amd.utils.error import LibError
from adrates_amd.utils.helpers import to_tenor

from . import _scenario_cases as SC
from . import _yoy_cases as YC
from . import _yoy_scenario_cases as YS
from ._parity import REL_TOL, unit_notional_err

pytestmark = pytest.mark.gpu
VD = SC.VD
GUARD = -1.2345e300


def _both(ctx, case, times, dfs, T, b, fixed="case"):
    fixed = YS.fixed_legs(case) if isinstance(fixed, str) else fixed
    args = (case.disc[0], times, dfs, case.infl[0], T, b, fixed, case.book)
    return _native.yoy_scenario_pv(ctx, *args, per_trade=True), _native.yoy_scenario_pv_host(*args, per_trade=True)


def _row_errors(case, dev, host):
    """(per swap row on the row's own scale with the PV floor of tests/_yoy_cases.py, on the array's largest entry)."""
    a, b = dev.T, host.T                                        # [n, S]
    scale = np.maximum(np.max(np.abs(b), axis=1), YC.FLOORS["pv"] * case.notional)
    return float(np.max(np.max(np.abs(a - b), axis=1) / scale)), float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize("case", YS.cases(), ids=repr)
def test_device_against_independent_reference_and_host_twin(gpu_ctx, case):
    times, dfs, T, b = YS.scenario_pairs(case)
    dev, host = _both(gpu_ctx, case, times, dfs, T, b)
    e, s, name = YS.worst_error(case, dev["pv"])
    row, arr = _row_errors(case, dev["pv"], host["pv"])
    print(f"{case}: device against C oracle + MpYoY {e:.2e} (scenario {s}, {name}); against the twin {row:.2e} per row, "
          f"{arr:.2e} of the array")
    assert e <= REL_TOL, (name, s, e)
    assert row <= REL_TOL and arr <= 1e-13
    assert np.array_equal(dev["book_pv"], SC.book_sum(dev["pv"]))
    assert np.max(np.abs(dev["book_pv"] - host["book_pv"])) <= REL_TOL * np.sum(case.notional)


@pytest.mark.parametrize("case", [c for c in YC.lookup_cases() if c.disc[0] == YC.LF], ids=repr)
def test_bit_equal_to_the_twin_where_no_exp_is_involved(gpu_ctx, case):
    """LINEAR_FWD_RATES discounting with ts == te coupons: no exp and no log on either side."""
    times, dfs, T, b = YS.scenario_pairs(case)
    dev, host = _both(gpu_ctx, case, times, dfs, T, b, fixed=None)
    assert np.array_equal(dev["pv"], host["pv"]) and np.array_equal(dev["book_pv"], host["book_pv"])
    dev, host = _both(gpu_ctx, case, times, dfs, T, b)          # and with the fixed legs, which have no exp either
    assert np.array_equal(dev["pv"], host["pv"]) and np.array_equal(dev["book_pv"], host["book_pv"])


def _mixed_rows(rows, S, seed):
    """``S`` distinct positive rows between the given ones (geometric mixtures)."""
    mix = np.random.default_rng(seed).uniform(0.0, 1.0, size=(S, rows.shape[0]))
    return np.exp((mix / mix.sum(1, keepdims=True)) @ np.log(rows))


def _upload(arrs):
    dev = torch.device("cuda", 0)
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in arrs.items()}


def _run_dev(ctx, case, times, dfs, T, b, fixed, per_trade, stream=0, book=None):
    """adr_yoy_scenario_pv_dev into guarded buffers; returns (book [S], pv [S, n] or None) as numpy."""
    dfs, b = np.atleast_2d(dfs), np.atleast_2d(b)
    S = max(dfs.shape[0], b.shape[0])
    cpn_off, cpn = _native.yoy_pack(book or case.book)
    n = cpn_off.size - 1
    t = _upload(dict(times=times, dfs=dfs, T=T, b=b, fix_off=fixed[0], fix_tp=fixed[1], fix_pay=fixed[2], cpn_off=cpn_off, cpn=cpn))
    dev = t["times"].device
    out = torch.full((S + 8,), GUARD, dtype=torch.float64, device=dev)
    pv = torch.full((n * S + 8,), GUARD, dtype=torch.float64, device=dev)
    work = torch.empty(_native.yoy_scenario_pv_work(n, S), dtype=torch.float64, device=dev)
    ptrs = {k: v.data_ptr() if v.numel() else 0 for k, v in t.items()}
    torch.cuda.synchronize()
    _native.yoy_scenario_pv_dev(ctx, case.disc[0], times.size, dfs.shape[0], case.infl[0], T.size, b.shape[0], S, n,
                                fixed[1].size, cpn.shape[1], ptrs, out.data_ptr(), work.data_ptr(),
                                pv.data_ptr() if per_trade else 0, stream)
    torch.cuda.synchronize()
    assert torch.all(out[S:] == GUARD)
    assert torch.all(pv[n * S:] == GUARD) if per_trade else torch.all(pv == GUARD)      # pv is not written when NULL
    return out[:S].cpu().numpy(), (pv[:n * S].reshape(n, S).cpu().numpy().T if per_trade else None)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_launch_shapes_bit_for_bit(gpu_ctx, n):
    """n around ADR_SCENARIO_CHUNK (legs of 0, 1, 63, 64, 65, 128 and 129 coupons in every book), S in {1, 63, 64, 65,
    130}: every row equals the row of the same pair priced alone, broadcast rows included, and the padding lanes of a
    partial group write nothing."""
    case = YC.geometry_case(20, n, YC.LZ, YC.LZ, shift=n % 5)
    times, dfs8, T, b8 = YS.scenario_pairs(case)
    fixed = YS.fixed_legs(case)
    dfs, b = _mixed_rows(dfs8, 130, n), _mixed_rows(1.0 + b8, 130, n + 1) - 1.0
    alone = {s: _run_dev(gpu_ctx, case, times, dfs[s], T, b[s], fixed, True) for s in (0, 62, 63, 64, 129)}
    for S in (1, 63, 64, 65, 130):
        book, pv = _run_dev(gpu_ctx, case, times, dfs[:S], T, b[:S], fixed, True)
        book_only, _ = _run_dev(gpu_ctx, case, times, dfs[:S], T, b[:S], fixed, False)
        again, _ = _run_dev(gpu_ctx, case, times, dfs[:S], T, b[:S], fixed, False)
        assert np.array_equal(book, book_only) and np.array_equal(book, again)
        assert np.array_equal(book, SC.book_sum(pv))
        for s, (b1, p1) in alone.items():
            if s < S:
                assert np.array_equal(pv[s], p1[0]) and book[s] == b1[0], (S, s)
    shared_d = _run_dev(gpu_ctx, case, times, dfs[64], T, b[:65], fixed, True)
    shared_b = _run_dev(gpu_ctx, case, times, dfs[:65], T, b[64], fixed, True)
    assert np.array_equal(shared_d[1][64], alone[64][1][0]) and np.array_equal(shared_b[1][64], alone[64][1][0])
    rep = _run_dev(gpu_ctx, case, times, np.repeat(dfs[64:65], 65, axis=0), T, b[:65], fixed, True)
    assert np.array_equal(rep[1], shared_d[1]) and np.array_equal(rep[0], shared_d[0])
    host = _native.yoy_scenario_pv_host(case.disc[0], times, dfs[:65], case.infl[0], T, b[:65], fixed, case.book, per_trade=True)
    row, arr = _row_errors(case, pv[:65], host["pv"])
    assert row <= REL_TOL and arr <= 1e-13


@pytest.mark.parametrize("P,K,dm", [(1, None, YC.FF), (20, 264, YC.LZ), (64, 264, YC.LZ), (64, 264, YC.LF), (20, 856, YC.LZ),
                                    (20, 856, YC.LF), (64, None, YC.FF)])
def test_pillar_counts_and_the_global_table_fallback(gpu_ctx, P, K, dm):
    """P in {1, 20, 64}; K = 264 with P = 20 is the largest pair of the README curve that fits the LDS (148 200 bytes);
    P = 64 at K = 264 (171 080 bytes) and K = 856 do not fit: the discount rows are read from global memory."""
    im = YC.INFL_SCHEMES[P % 2]
    disc = (dm,) + YC.disc_grid(K)
    case = YC.Case(f"P = {P}, K = {K}", disc, (im,) + YC.pillars(P), YC.geometry_swaps(17, shift=P % 4))
    times, dfs, T, b = YS.scenario_pairs(case)
    dev, host = _both(gpu_ctx, case, times, dfs, T, b)
    e, s, name = YS.worst_error(case, dev["pv"])
    row, arr = _row_errors(case, dev["pv"], host["pv"])
    print(f"{case}, disc {YC.NAMES[dm]}: reference {e:.2e}, twin {row:.2e} per row")
    assert e <= REL_TOL and row <= REL_TOL and arr <= 1e-13, (name, s, e, row, arr)
    assert np.array_equal(dev["book_pv"], SC.book_sum(dev["pv"]))
    full = _both(gpu_ctx, case, times, _mixed_rows(dfs, 70, 5), T, _mixed_rows(1.0 + b, 70, 6) - 1.0)
    row, arr = _row_errors(case, full[0]["pv"], full[1]["pv"])  # a full group and a partial one
    assert row <= REL_TOL and arr <= 1e-13


def test_dev_entry_on_a_callers_stream_and_malformed_offsets(gpu_ctx):
    case = YC.knot_cases()[0]
    times, dfs, T, b = YS.scenario_pairs(case)
    fixed = YS.fixed_legs(case)
    first = _native.yoy_scenario_pv(gpu_ctx, 4, times, dfs, 4, T, b, fixed, case.book, per_trade=True)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    with torch.cuda.stream(stream):
        book, pv = _run_dev(gpu_ctx, case, times, dfs, T, b, fixed, True, stream.cuda_stream)
        book_only, none = _run_dev(gpu_ctx, case, times, dfs, T, b, fixed, False, stream.cuda_stream)
    assert none is None and np.array_equal(pv, first["pv"]) and np.array_equal(book, first["book_pv"])
    assert np.array_equal(book_only, book)
    # malformed offsets: the documented NaN path reads no flow of that swap; the neighbours keep their bits
    n, m = len(case.rows), int(case.book["cpn_off"][-1])
    for which, bad in (("cpn", (3, m + 5)), ("cpn", (2, -1)), ("fix", (5, 10 ** 6))):
        off_c, off_f = case.book["cpn_off"].copy(), fixed[0].copy()
        (off_c if which == "cpn" else off_f)[bad[0]] = bad[1]
        bk = dict(case.book, cpn_off=off_c)
        cpn_off, cpn = off_c, np.stack([case.book[k] for k in _native.YOY_FIELDS])
        t = _upload(dict(times=times, dfs=dfs, T=T, b=b, fix_off=off_f, fix_tp=fixed[1], fix_pay=fixed[2], cpn_off=cpn_off, cpn=cpn))
        S = dfs.shape[0]
        dev = t["times"].device
        out = torch.full((S,), GUARD, dtype=torch.float64, device=dev)
        pvt = torch.full((n, S), GUARD, dtype=torch.float64, device=dev)
        work = torch.empty(_native.yoy_scenario_pv_work(n, S), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        _native.yoy_scenario_pv_dev(gpu_ctx, 4, times.size, S, 4, T.size, S, S, n, fixed[1].size, m,
                                    {k: v.data_ptr() for k, v in t.items()}, out.data_ptr(), work.data_ptr(), pvt.data_ptr())
        torch.cuda.synchronize()
        got = pvt.cpu().numpy().T
        hit = [bad[0] - 1, bad[0]] if bad[0] < n else [bad[0] - 1]      # the swaps whose pair names the bad offset
        hit = [i for i in hit if i >= 0]
        nan = np.isnan(got).all(axis=0)
        assert nan[hit].all() and set(np.flatnonzero(nan)) <= set(hit), (which, bad, np.flatnonzero(nan))
        keep = ~nan
        assert np.array_equal(got[:, keep], first["pv"][:, keep]) and np.isnan(out.cpu().numpy()).all()
        del bk
    u = _upload(dict(times=times, dfs=dfs))
    with pytest.raises(LibError, match="work is NULL"):
        _native.yoy_scenario_pv_dev(gpu_ctx, 4, times.size, 8, 4, T.size, 8, 8, n, 0, 0,
                                    dict(times=u["times"].data_ptr(), dfs=u["dfs"].data_ptr(), T=1, b=1, fix_off=1, cpn_off=1), 1, 0)
    with pytest.raises(LibError, match="S_disc and S_infl"):
        _native.yoy_scenario_pv_dev(gpu_ctx, 4, times.size, 3, 4, T.size, 8, 8, n, 0, 0,
                                    dict(times=1, dfs=1, T=1, b=1, fix_off=1, cpn_off=1), 1, 1)


def test_book_revalue_against_the_per_scenario_loop(gpu_ctx):
    """2 000 swaps x 9 joint scenarios: one launch on the grid's device-resident discount factors against
    `YoYBook.compute([VALUE])` on a model rebuilt per scenario (one adr_yoy_risk launch, a host pass and one adr_price
    launch each).  The P&L of the zero shock is exactly 0."""
    swaps = random_yoy_book(VD, 2000, seed=13)
    notional = np.array([s._notional for s in swaps])
    model = yoy_model(VD)
    book = YoYBook(swaps, model)
    disc_shocks = [0.0, 0.01, -0.01, 0.5, -0.5, 2.0, -2.0, {"5Y": 0.25}, {"3M": -0.1, "30Y": 0.2}]      # percent
    infl_shocks = [0.0, 1.0, 50.0, -50.0, 200.0, -200.0, {"10Y": 100.0}, {"2Y": -25.0, "30Y": 40.0}, -1.0]  # basis points
    _, T, b0 = inflation_inputs(book.inflation_curve)
    tenors, names = to_tenor(list(T)), model._curve_params_dict["GBP_OIS_SONIA"]["tenor_list"]
    grid = ScenarioGrid(model, "GBP_OIS_SONIA", disc_shocks, with_gamma=False, ctx=gpu_ctx)
    try:
        one = book.revalue(grid=grid, inflation_shocks=infl_shocks, per_trade=True)
        assert one["pv"].shape == (9, 2000) and np.array_equal(one["book_pv"], SC.book_sum(one["pv"]))
        assert np.array_equal(book.revalue(grid=grid, inflation_shocks=infl_shocks)["book_pv"], one["book_pv"])
        worst = 0.0
        for s, (ds, ib) in enumerate(zip(disc_shocks, infl_shocks)):
            m = gbp_model(VD, px=[q + (ds.get(t, 0.0) if isinstance(ds, dict) else ds) for q, t in zip(GBP_PX, names)])
            px = [q + 0.01 * (ib.get(t, 0.0) if isinstance(ib, dict) else ib) for q, t in zip(INFL_PX, tenors)]
            m._curves_dict["GBP_RPI_INFLATION"] = inflation_curve(VD, px=px)
            loop = YoYBook(swaps, m).compute([RequestTypes.VALUE])["pv"]
            worst = max(worst, unit_notional_err(one["pv"][s], loop, notional))
        print(f"YoYBook.revalue against the per-scenario loop: {worst:.2e}")
        assert worst <= REL_TOL
        b_rows = np.array([shocked_breakevens(book.inflation_curve, s) for s in infl_shocks])
        hist = book.revalue(grid=grid, breakevens=b_rows, per_trade=True)
        assert np.array_equal(hist["pv"], one["pv"])
        only_d = book.revalue(grid=grid)["book_pv"]
        only_i = book.revalue(inflation_shocks=infl_shocks)["book_pv"]
        assert only_d[0] == one["book_pv"][0] == only_i[0] and only_d[5] != one["book_pv"][5] != only_i[5]
        pnl = book.pnl(grid=grid, inflation_shocks=infl_shocks)
        print(f"pnl of the zero shock: {pnl[0]!r}")
        assert pnl.shape == (9,) and pnl[0] == 0.0
        assert np.allclose(pnl[1:], one["book_pv"][1:] - one["book_pv"][0], rtol=0, atol=1e-10 * np.sum(notional))
        assert book.pnl(inflation_shocks=infl_shocks)[0] == 0.0 and book.pnl(grid=grid)[0] == 0.0
        assert historical_var(pnl, 0.75) == -np.sort(pnl)[2]
        with pytest.raises(LibError, match="no scenarios"):
            book.revalue()
        with pytest.raises(LibError, match="9 discount scenarios but 2 inflation scenarios"):
            book.revalue(grid=grid, inflation_shocks=[0.0, 1.0])
        with pytest.raises(LibError, match="not both"):
            book.pnl(inflation_shocks=[0.0], breakevens=b_rows)
        with pytest.raises(LibError, match="is not an OIS, a Bond or an FRN"):
            grid.revalue(swaps[:2])                             # the curve-only revaluation keeps refusing YoY swaps
    finally:
        grid.close()
