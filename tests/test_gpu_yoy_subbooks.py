"""YoY sub-books on the device: adr_yoy_scenario_subbook_pv, _dev and the `YoYBook` methods over them.  The CPU twin:
tests/test_yoy_subbook_host.py."""
import numpy as np
import pytest
import torch

from adrates_amd import _native
from adrates_amd.market.position.scenarios import ScenarioGrid, tail_count, tail_measures
from adrates_amd.market.position.yoy_book import YoYBook
from adrates_amd.trades.market_data import random_yoy_book, yoy_model
from adrates_amd.utils.error import LibError

from . import _scenario_cases as SC
from . import _yoy_cases as YC
from . import _yoy_scenario_cases as YS
from . import _yoy_subbook_cases as YB
from ._parity import REL_TOL

pytestmark = pytest.mark.gpu
VD = SC.VD
GUARD = -1.2345e300
TAIL = 16


@pytest.fixture(scope="module")
def E(gpu_ctx):
    return YB.Entries(gpu_ctx)


@pytest.fixture(scope="module")
def sized(E):
    """The device's result on the sized book (computed once, never changed), checked row by row."""
    return YB.check_sized_book(E, YB.sized_case(), SC.book_sum)


def test_every_sub_book_equals_itself_uploaded_alone(sized):
    case = YB.sized_case()
    times, dfs, T, b = YS.scenario_pairs(case)
    sub_off = YB.offsets(YB.SIZES)
    host = YB.Entries().sub(case, times, dfs, T, b, YS.fixed_legs(case), case.book, sub_off)["sub_pv"]
    err = np.max(np.abs(sized["sub_pv"] - host) / YB.gross(case, sub_off)[:, None])
    print(f"device vs host twin per gross notional: {err:.2e}")
    assert err <= REL_TOL


@pytest.mark.parametrize("case", YS.cases(), ids=repr)
def test_one_sub_book_is_the_parent(E, case):
    YB.check_one_sub_book_is_the_parent(E, case)


def test_scenario_counts_and_repeat_runs(E, sized):
    YB.check_scenario_counts(E)
    case = YB.sized_case()
    times, dfs, T, b = YS.scenario_pairs(case)
    again = E.sub(case, times, dfs, T, b, YS.fixed_legs(case), case.book, YB.offsets(YB.SIZES), per_trade=True)
    assert np.array_equal(again["sub_pv"], sized["sub_pv"]) and np.array_equal(again["pv"], sized["pv"], equal_nan=True)


def test_permuting_the_sub_books_permutes_the_rows(E, sized):
    YB.check_permutation(E, sized)


@pytest.mark.parametrize("P,K,dm", YB.FALLBACKS)
def test_tables_that_leave_the_lds(E, P, K, dm):
    case, out, sub_off = YB.check_fallback(E, P, K, dm, SC.book_sum)
    times, dfs, T, b = YS.scenario_pairs(case)
    host = YB.Entries().sub(case, times, dfs, T, b, YS.fixed_legs(case), case.book, sub_off)["sub_pv"]
    assert np.max(np.abs(out["sub_pv"] - host) / YB.gross(case, sub_off)[:, None]) <= REL_TOL


def test_rows_do_not_depend_on_the_sub_book_count_with_the_table_in_global_memory(E):
    """K = 856: three sub-books, one of them empty, against B = 1 launches of each on the global-table variant."""
    case = YB.fallback_case(20, 856, YC.LZ)
    times, dfs, T, b = YS.scenario_pairs(case)
    fixed, n = YS.fixed_legs(case), len(case.rows)
    out = E.sub(case, times, dfs, T, b, fixed, case.book, [0, 70, 70, n])["sub_pv"]
    for j, (lo, hi) in enumerate(((0, 70), (70, 70), (70, n))):
        if lo < hi:
            f, bk = YB.take(fixed, case.book, lo, hi)
            assert np.array_equal(out[j], E.sub(case, times, dfs, T, b, f, bk, [0, hi - lo])["sub_pv"][0])


def test_malformed_offsets_name_the_sub_book(E):
    YB.check_malformed_offsets(E, LibError, pytest.raises)


def test_dev_entry_on_a_callers_stream_into_guarded_buffers(gpu_ctx, E, sized):
    case = YB.sized_case()
    times, dfs, T, b = YB.wide_pairs(case, 65)
    fixed, sub_off = YS.fixed_legs(case), YB.offsets(YB.SIZES)
    B, n, S = len(YB.SIZES), len(case.rows), 65
    want = E.sub(case, times, dfs, T, b, fixed, case.book, sub_off, per_trade=True)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cpn_off, cpn = _native.yoy_pack(case.book)
    held = dict(times=up(times), dfs=up(dfs), T=up(T), b=up(b), fix_off=up(fixed[0]), fix_tp=up(fixed[1]), fix_pay=up(fixed[2]),
                cpn_off=up(cpn_off), cpn=up(cpn), plan=up(_native.scenario_subbook_plan(n, sub_off)))
    ptrs = {k: v.data_ptr() for k, v in held.items()}
    W = _native.scenario_subbook_work(n, B, S)
    guarded = lambda count: torch.full((count + TAIL,), GUARD, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(dev)
    args = (gpu_ctx, case.disc[0], times.size, S, case.infl[0], T.size, S, S, n, fixed[1].size, cpn.shape[1], B)
    k = 3
    for per_trade in (True, False):
        sub, work, pv, var, es = guarded(B * S), guarded(W), guarded(n * S), guarded(B), guarded(B)
        with torch.cuda.stream(stream):
            _native.yoy_scenario_subbook_pv_dev(*args, ptrs, sub.data_ptr(), work.data_ptr(), pv.data_ptr() if per_trade else 0,
                                                stream.cuda_stream)
            _native.scenario_tail_dev(gpu_ctx, B, S, sub.data_ptr(), k, var.data_ptr(), es.data_ptr(), base_col=S - 1,
                                      stream=stream.cuda_stream)
            stream.synchronize()
        for buf, count in ((sub, B * S), (work, W), (pv, n * S), (var, B), (es, B)):
            assert torch.all(buf[count:] == GUARD)
        assert np.array_equal(sub[:B * S].reshape(B, S).cpu().numpy(), want["sub_pv"])
        if per_trade:
            assert np.array_equal(pv[:n * S].reshape(n, S).cpu().numpy().T, want["pv"], equal_nan=True)
        else:
            assert torch.all(pv == GUARD)                                   # nothing asked for: the pattern is kept
        hv, he = _native.scenario_tail_host(want["sub_pv"], k, base_col=S - 1)
        assert np.array_equal(var[:B].cpu().numpy(), hv) and np.array_equal(es[:B].cpu().numpy(), he)
    with pytest.raises(LibError, match="plan is NULL"):
        _native.yoy_scenario_subbook_pv_dev(*args, dict(ptrs, plan=0), sub.data_ptr(), work.data_ptr())
    with pytest.raises(LibError, match="at least one sub-book"):
        _native.yoy_scenario_subbook_pv_dev(*args[:-1], 0, ptrs, sub.data_ptr(), work.data_ptr())


def test_book_methods(gpu_ctx):
    swaps = random_yoy_book(VD, 600, seed=13)
    model = yoy_model(VD)
    book = YoYBook(swaps, model)
    keys = [("rates", "inflation", "xva")[(i * 7 + i // 11) % 3] for i in range(len(swaps))]
    disc_shocks = [0.0, 0.01, -0.01, 0.5, -0.5, 2.0, -2.0, {"5Y": 0.25}, {"3M": -0.1, "30Y": 0.2}]
    infl_shocks = [0.0, 1.0, 50.0, -50.0, 200.0, -200.0, {"10Y": 100.0}, {"2Y": -25.0, "30Y": 40.0}, -1.0]
    grid = ScenarioGrid(model, "GBP_OIS_SONIA", disc_shocks, with_gamma=False, ctx=gpu_ctx)
    try:
        for kw in (dict(grid=grid, inflation_shocks=infl_shocks), dict(inflation_shocks=infl_shocks), dict(grid=grid)):
            out = book.revalue_sub_books(keys, per_trade=True, **kw)
            assert out["labels"] == ["rates", "inflation", "xva"]
            assert np.array_equal(out["pv"], book.revalue(per_trade=True, **kw)["pv"])          # the book's order
            pnl = book.pnl_sub_books(keys, **kw)
            assert pnl.shape == (3, 9) and np.all(pnl[:, 0] == 0.0)                             # a zero shock: exactly 0
            for j, lab in enumerate(out["labels"]):
                alone = YoYBook([s for s, k in zip(swaps, keys) if k == lab], model)
                assert np.array_equal(pnl[j], alone.pnl(**kw)), lab
                assert np.array_equal(out["sub_pv"][j], alone.revalue(**kw)["book_pv"]), lab
            got = book.sub_book_var_es(keys, level=0.75, **kw)
            var, es = tail_measures(pnl, 0.75, host=True)
            assert tail_count(0.75, 9) == 3 and got["labels"] == out["labels"]
            assert np.array_equal(got["var"], var) and np.array_equal(got["es"], es)
        with pytest.raises(LibError, match="keys needs one entry per swap"):
            book.pnl_sub_books(keys[:-1], inflation_shocks=infl_shocks)
        with pytest.raises(LibError, match="no scenarios"):
            book.revalue_sub_books(keys)
    finally:
        grid.close()
