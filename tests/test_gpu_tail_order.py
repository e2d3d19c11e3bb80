"""The ordered tail select (adr_scenario_tail_order*, csrc/tail_select.hip), the allocation of a matrix of any width, the
gather and the components (csrc/tail_order.hip) and `monte_carlo_allocate_tail` on the GPU, on the tables of the CPU suite
(tests/_tail_order_cases.py): the select against the independent NumPy statement, the twin's bits and the same bits from a
second run, the tie rows that decide the tie rule, the device-array entries in guarded buffers with a scratch of exactly
the stated size, the refusals; the allocation with adr_scenario_tail_alloc's bits where that takes the rows and
`_allocate_tail_numpy`'s beyond; the chain's three bit contracts whatever the tiling, its derived difference from the
matrix allocation and additivity."""
import numpy as np
import pytest
import torch

from adrates_amd import _native
from adrates_amd.market.position.ladder_pnl import augmented_ladder_pnl, ladder_pnl, ladder_rows
from adrates_amd.market.position.monte_carlo import (allocate_tail_select, factor_from_covariance, firm_ladder,
                                                     monte_carlo_allocate_tail, monte_carlo_shocks, monte_carlo_var_es,
                                                     sub_book_monte_carlo_allocate_tail)
from adrates_amd.market.position.scenarios import _allocate_tail_numpy, tail_count
from adrates_amd.utils.error import LibError
from adrates_amd.utils.global_types import RequestTypes

from . import _monte_carlo_cases as C
from . import _tail_alloc_cases as A
from . import _tail_order_cases as T

pytestmark = pytest.mark.gpu
GUARD = -7.25
TAIL = 16
REQS = {RequestTypes.VALUE, RequestTypes.DELTA, RequestTypes.GAMMA}


def guarded(a):
    """A device copy of ``a`` as doubles with 16 guard words behind it."""
    return torch.cat([torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).ravel()),
                      torch.full((TAIL,), GUARD, dtype=torch.float64)]).cuda()


def guards(n):
    return torch.full((n + TAIL,), GUARD, dtype=torch.float64, device="cuda")


def intact(t, n):
    return bool((t[n:] == GUARD).all())


# ------------------------------------------------------------------------------------------------------ ordered select
@pytest.mark.parametrize("m", T.WIDTHS)
def test_order_against_numpy_and_the_twin(gpu_ctx, m):
    """Every content and tail count of the table at width m: the statement's indices and bits, the twin's, and the same
    from a second run."""
    for content, B, k, base_col, rows in T.select_calls(m):
        dev = _native.scenario_tail_order(gpu_ctx, rows, k, base_col)
        assert T.same_order(dev, T.numpy_order(rows, base_col, k)), (content, B, k, base_col)
        assert T.same_order(dev, _native.scenario_tail_order_host(rows, k, base_col)), (content, B, k, base_col)
        if base_col == -1:
            assert T.same_order(dev, _native.scenario_tail_order(gpu_ctx, rows, k, base_col)), "two runs"


@pytest.mark.parametrize("case", T.TIE_CASES, ids=[c[0] for c in T.TIE_CASES])
def test_order_takes_the_lowest_ties(gpu_ctx, case):
    rows, k, taken = T.tie_call(case)
    got = _native.scenario_tail_order(gpu_ctx, rows, k)
    assert T.same_order(got, T.numpy_order(rows, -1, k))
    assert np.array_equal(np.sort(got[0][1]), np.sort(taken)), "exactly the lowest indices of the run"
    assert np.array_equal(got[0][0], np.arange(k)), "equal values: the first k indices in order"
    assert T.same_order(got, _native.scenario_tail_order(gpu_ctx, rows, k)), "two runs"
    alone = _native.scenario_tail_order(gpu_ctx, rows[1:2], k)             # one row: the segments of B = 1
    assert np.array_equal(alone[0][0], got[0][1]) and C.same_bits(alone[2], got[2][1:2])


def test_order_nan_rows_stand_alone(gpu_ctx):
    rows = C.pnl_rows("nan", 3, 40000, 400)
    order, var, es = _native.scenario_tail_order(gpu_ctx, rows, 400)
    assert np.all(order[1] == -1) and np.isnan(var[1]) and np.isnan(es[1])
    assert T.same_order((order, var, es), T.numpy_order(rows, -1, 400))


@pytest.mark.parametrize("B,m,k,base_col", [(3, 40000, 400, -1), (70, 16385, 164, 5), (1, 131075, 8192, 131075), (2500, 300, 3, -1),
                                            (1, 8193, 4097, -1)])
def test_order_dev_entry_in_guarded_buffers(gpu_ctx, B, m, k, base_col):
    """adr_scenario_tail_order_dev on a caller's stream with a scratch of exactly adr_scenario_tail_order_work bytes: the
    statement's indices and bits, the guard words behind the scratch, the rows and the outputs intact.  The shapes take
    one and several segments per row and rows beyond the blocks aimed at."""
    rows = C.with_base(C.pnl_rows("normal", B, m, k), base_col, "normal")
    S_tot = rows.shape[1]
    need = _native.scenario_tail_order_work(B, S_tot, k)
    assert need > 0 and need % 16 == 0
    d_rows, work, out = guarded(rows), guards(need // 8), torch.full((2, B + TAIL), GUARD, dtype=torch.float64, device="cuda")
    order = torch.full((B * k + TAIL,), -99, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    _native.scenario_tail_order_dev(gpu_ctx, B, S_tot, d_rows.data_ptr(), k, order.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                    work.data_ptr(), base_col=base_col, stream=stream.cuda_stream)
    stream.synchronize()
    got, idx = out.cpu().numpy(), order.cpu().numpy()
    assert T.same_order((idx[:B * k].reshape(B, k), got[0, :B], got[1, :B]), T.numpy_order(rows, base_col, k))
    assert np.all(got[:, B:] == GUARD) and np.all(idx[B * k:] == -99) and intact(work, need // 8) and intact(d_rows, rows.size)
    assert np.array_equal(d_rows[:-TAIL].cpu().numpy(), rows.ravel())


def test_order_refusals_on_the_device(gpu_ctx):
    rows = np.zeros((2, 20000))
    for k, base_col, status in ((8193, -1, -2), (0, -1, -1), (20001, -1, -1), (20000, 0, -1), (5, 20000, -1), (5, -2, -1)):
        for call in (_native.scenario_tail_order, _native.scenario_tail_alloc_select):
            with pytest.raises(LibError) as e:
                call(gpu_ctx, rows, k, base_col)
            assert e.value.status == status, (k, base_col)
    buf = guards(48)
    p = buf.data_ptr()
    for args in ((2, 8, p, 9, p, p, p, p), (2, 8, 0, 1, p, p, p, p), (2, 8, p, 1, 0, p, p, p), (2, 8, p, 1, p, 0, p, p),
                 (2, 8, p, 1, p, p, p, 0), (0, 8, p, 1, p, p, p, p)):
        with pytest.raises(LibError) as e:
            _native.scenario_tail_order_dev(gpu_ctx, *args)
        assert e.value.status == -1, args
    for args in ((2, 8, p, 9, p, p, p, p, p), (2, 8, 0, 1, p, p, p, p, p), (2, 8, p, 1, p, p, 0, p, p), (2, 8, p, 1, p, p, p, p, 0),
                 (0, 8, p, 1, p, p, p, p, p)):
        with pytest.raises(LibError) as e:
            _native.scenario_tail_alloc_select_dev(gpu_ctx, *args)
        assert e.value.status == -1, args
    with pytest.raises(LibError) as e:
        _native.scenario_tail_order_dev(gpu_ctx, 1, 20000, p, 8193, p, p, p, p)
    assert e.value.status == -2
    for call, args in ((_native.shock_gather_dev, (0, 2, p, 4, p, p)), (_native.shock_gather_dev, (1, 257, p, 4, p, p)),
                       (_native.shock_gather_dev, (1, 2, p, 4, 0, p)), (_native.tail_components_dev, (0, 2, p, p, p)),
                       (_native.tail_components_dev, (1, 2, p, 0, p)), (_native.scenario_total_dev, (0, 2, p, p)),
                       (_native.scenario_total_dev, (1, 2, p, 0))):
        with pytest.raises(LibError) as e:
            call(gpu_ctx, *args)
        assert e.value.status == -1, args
    gpu_ctx.sync()
    assert bool((buf == GUARD).all())


# ------------------------------------------------------------------------------------------------ gather and components
@pytest.mark.parametrize("B,k,P", [(1, 1, 1), (67, 130, 7), (130, 200, 32), (64, 64, 256)])
def test_gather_components_and_total_in_guarded_buffers(gpu_ctx, B, k, P):
    """The three small device entries on a caller's stream: the twins' bits, guards and inputs intact; a negative first
    index, or an index that is no row, gives NaN rows."""
    rng = np.random.default_rng([8, B, k, P])
    S = 3 * k + 5
    shocks, pnl = rng.standard_normal((S, P)), rng.standard_normal((B, k)) * 1e6
    idx = rng.permutation(S)[:k]
    stream = torch.cuda.Stream()
    d_shocks, d_pnl, d_order = guarded(shocks), guarded(pnl), torch.from_numpy(np.concatenate([idx, np.full(TAIL, -99)])).cuda()
    out, comp, tot = guards(k * P), torch.full((2, B + TAIL), GUARD, dtype=torch.float64, device="cuda"), guards(k)
    torch.cuda.synchronize()
    _native.shock_gather_dev(gpu_ctx, k, P, d_shocks.data_ptr(), S, d_order.data_ptr(), out.data_ptr(), stream=stream.cuda_stream)
    _native.tail_components_dev(gpu_ctx, B, k, d_pnl.data_ptr(), comp[0].data_ptr(), comp[1].data_ptr(), stream=stream.cuda_stream)
    _native.scenario_total_dev(gpu_ctx, B, k, d_pnl.data_ptr(), tot.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert C.same_bits(out[:k * P].cpu().numpy().reshape(k, P), shocks[idx]) and intact(out, k * P)
    got, want = comp.cpu().numpy(), _native.tail_components_host(pnl)
    assert C.same_bits(got[0, :B], want[0]) and C.same_bits(got[1, :B], want[1]) and np.all(got[:, B:] == GUARD)
    assert C.same_bits(tot[:k].cpu().numpy(), _native.scenario_total_host(pnl)) and intact(tot, k)
    assert C.same_bits(tot[:k].cpu().numpy(), A.slot_total(pnl))
    assert intact(d_shocks, S * P) and intact(d_pnl, B * k) and np.array_equal(d_order.cpu().numpy()[:k], idx)
    if k > 1:
        bad = idx.copy()
        bad[k - 1] = S
        d_order[:k] = torch.from_numpy(bad).cuda()
        torch.cuda.synchronize()
        _native.shock_gather_dev(gpu_ctx, k, P, d_shocks.data_ptr(), S, d_order.data_ptr(), out.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        assert C.same_bits(out[:k * P].cpu().numpy().reshape(k, P), _native.shock_gather_host(shocks, bad)) and intact(out, k * P)
        bad[0] = -1
        d_order[:k] = torch.from_numpy(bad).cuda()
        torch.cuda.synchronize()
        _native.shock_gather_dev(gpu_ctx, k, P, d_shocks.data_ptr(), S, d_order.data_ptr(), out.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        assert bool(torch.isnan(out[:k * P]).all()) and intact(out, k * P)


# ---------------------------------------------------------------------------------------------------- matrix allocation
@pytest.mark.parametrize("S", (1, 100, 1025, 8192))
def test_alloc_select_has_allocs_bits(gpu_ctx, S):
    """Where adr_scenario_tail_alloc takes the rows: its bits on the device and its host twin's."""
    for rows, base_col, k in A.calls(S):
        if rows.shape[0] <= 129:
            got = _native.scenario_tail_alloc_select(gpu_ctx, rows, k, base_col)
            assert T.same_alloc(got, _native.scenario_tail_alloc(gpu_ctx, rows, k, base_col)), (rows.shape, base_col, k)
            assert T.same_alloc(got, _native.scenario_tail_alloc_host(rows, k, base_col)), (rows.shape, base_col, k)
    for name, rows, base_col, k in A.special_calls():
        assert T.same_alloc(_native.scenario_tail_alloc_select(gpu_ctx, rows, k, base_col),
                            _native.scenario_tail_alloc_host(rows, k, base_col)), name
    for rows, base_col, k in A.nan_calls():
        got = _native.scenario_tail_alloc_select(gpu_ctx, rows, k, base_col)
        assert all(np.all(np.isnan(got[f])) for f in ("var", "es", "comp_var", "comp_es"))


@pytest.mark.parametrize("m", T.ALLOC_WIDE)
@pytest.mark.parametrize("B", T.ALLOC_ROWS)
def test_alloc_select_beyond_the_row_limit(gpu_ctx, B, m):
    """`_allocate_tail_numpy`'s bits, from the blocking entry and from the device-array entry on a caller's stream with a
    scratch of exactly the stated size between guards."""
    rows = T.alloc_matrix(B, m)
    for k in (1, tail_count(0.99, m), min(m, T.ORDER_MAX)):
        assert T.same_alloc(_native.scenario_tail_alloc_select(gpu_ctx, rows, k), _allocate_tail_numpy(rows, k, -1)), k
    with_base = np.ascontiguousarray(np.hstack([rows[:, :7], np.zeros((B, 1)), rows[:, 7:]]))
    want = _allocate_tail_numpy(with_base, 82, 7)
    assert T.same_alloc(_native.scenario_tail_alloc_select(gpu_ctx, with_base, 82, 7), want)
    assert T.same_alloc(allocate_tail_select(rows, 0.99, ctx=gpu_ctx), _allocate_tail_numpy(rows, tail_count(0.99, m), -1))
    need = _native.scenario_tail_alloc_select_work(B, m + 1, 82)
    assert need > 0 and need % 16 == 0
    d_rows, work, out = guarded(with_base), guards(need // 8), guards(2 * B + 2)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    p = out.data_ptr()
    _native.scenario_tail_alloc_select_dev(gpu_ctx, B, m + 1, d_rows.data_ptr(), 82, p, p + 8, p + 16, p + 16 + 8 * B, work.data_ptr(),
                                           base_col=7, stream=stream.cuda_stream)
    stream.synchronize()
    got = out.cpu().numpy()
    assert T.same_alloc({"var": got[0], "es": got[1], "comp_var": got[2:2 + B], "comp_es": got[2 + B:2 + 2 * B]}, want)
    assert intact(out, 2 * B + 2) and intact(work, need // 8) and intact(d_rows, with_base.size)
    assert np.array_equal(d_rows[:-TAIL].cpu().numpy(), with_base.ravel())


def test_alloc_select_on_tied_totals(gpu_ctx):
    """The firm's totals tie while the desk rows differ: the lower scenario indices win, as in NumPy's statement."""
    rows = T.tied_totals()
    for k in (30, 31, 82, 4097):
        assert T.same_alloc(_native.scenario_tail_alloc_select(gpu_ctx, rows, k), _allocate_tail_numpy(rows, k, -1)), k


# ------------------------------------------------------------------------------------------------ the blocking entries
@pytest.mark.parametrize("base_col", (-1, 0, 129))
def test_blocking_tail_entries_on_three_rows(gpu_ctx, base_col):
    """The five blocking tail entries on three rows of 130 columns with k = 2: an odd row count, so var, es and the
    components do not fill whole 16-byte units of the call's one device allocation.  Each against its host twin, bit for
    bit."""
    rows, k = T.alloc_matrix(3, 130), 2
    for name in ("scenario_tail", "scenario_tail_select"):
        dev, twin = getattr(_native, name)(gpu_ctx, rows, k, base_col), getattr(_native, name + "_host")(rows, k, base_col)
        assert C.same_bits(dev[0], twin[0]) and C.same_bits(dev[1], twin[1]), name
    assert T.same_order(_native.scenario_tail_order(gpu_ctx, rows, k, base_col), _native.scenario_tail_order_host(rows, k, base_col))
    for name in ("scenario_tail_alloc", "scenario_tail_alloc_select"):
        dev, twin = getattr(_native, name)(gpu_ctx, rows, k, base_col), getattr(_native, name + "_host")(rows, k, base_col)
        assert T.same_alloc(dev, twin), name


# -------------------------------------------------------------------------------------------------------------- chain
@pytest.mark.parametrize("P", [9, 32])
def test_chain_contracts(gpu_ctx, P):
    """`monte_carlo_allocate_tail` on 19 desks and 20 000 scenarios with tiles of 19, 8 and 1 desks.  Against the twins:
    every output is the CPU twins' chain on the device's shocks.  Firm figures: `monte_carlo_var_es` of the firm's row.
    Desk components: `components_of` on the columns `scenarios` of the full matrix.  Then the derived difference from the
    matrix allocation (part 2) and additivity; the ratios to the bounds are printed."""
    delta, gamma, L = T.chain_case(P)
    rows, S, k = ladder_rows(delta, gamma), T.CHAIN_S, T.CHAIN_K
    shocks = monte_carlo_shocks(L, S, T.CHAIN_SEED, ctx=gpu_ctx)
    want = T.twins_chain(rows, shocks, k, T.CHAIN_B)
    for desks in (19, 8, 1):
        got = monte_carlo_allocate_tail(delta, gamma, L, S, level=T.CHAIN_LEVEL, seed=T.CHAIN_SEED, ctx=gpu_ctx, max_bytes=desks * 8 * k)
        assert T.same_chain(got, want), desks
    assert got["scenarios"].shape == (k,) and got["scenarios"].dtype == np.int64
    firm = monte_carlo_var_es(None, None, L, S, level=T.CHAIN_LEVEL, seed=T.CHAIN_SEED, ctx=gpu_ctx, ladders=firm_ladder(rows)[None])
    assert C.same_bits(firm["var"], [got["var"]]) and C.same_bits(firm["es"], [got["es"]])
    pnl = ladder_pnl(delta, gamma, shocks, ctx=gpu_ctx)
    comp = T.components_of_columns(pnl, got["scenarios"])
    assert C.same_bits(got["comp_var"], comp[0]) and C.same_bits(got["comp_es"], comp[1])
    part2 = allocate_tail_select(pnl, T.CHAIN_LEVEL, ctx=gpu_ctx)
    T.check_cross_and_additivity(got, part2, pnl, delta, gamma, shocks, k, f"device, P = {P}")


def test_chain_on_the_antithetic_set(gpu_ctx):
    delta, gamma, L = T.chain_case(9)
    anti = monte_carlo_allocate_tail(delta, gamma, L, T.CHAIN_S, level=0.95, seed=T.CHAIN_SEED, antithetic=True, ctx=gpu_ctx)
    xa = monte_carlo_shocks(L, T.CHAIN_S, T.CHAIN_SEED, antithetic=True, ctx=gpu_ctx)
    assert T.same_chain(anti, T.twins_chain(ladder_rows(delta, gamma), xa, tail_count(0.95, T.CHAIN_S), T.CHAIN_B))
    with pytest.raises(LibError) as e:
        monte_carlo_allocate_tail(delta, gamma, L, 1048576, level=0.99, ctx=gpu_ctx)
    assert e.value.status == _native.ADR_ERR_UNSUPPORTED
    bad = delta.copy()
    bad[3, 2] = np.nan
    got = monte_carlo_allocate_tail(bad, gamma, L, 3000, ctx=gpu_ctx)
    assert np.isnan(got["var"]) and np.isnan(got["es"]) and np.all(np.isnan(got["comp_var"])) and np.all(np.isnan(got["comp_es"]))
    assert np.all(got["scenarios"] == -1)


def _check_ladders(gpu_ctx, ladders, Q, what):
    """Ready rows through `monte_carlo_allocate_tail` with a Q-row factor: the twins' chain and the full matrix's columns."""
    L = factor_from_covariance(C.covariance(Q), min(Q, 6))
    S = 20000
    got = monte_carlo_allocate_tail(None, None, L, S, level=0.99, seed=21, ctx=gpu_ctx, ladders=ladders)
    shocks = monte_carlo_shocks(L, S, 21, ctx=gpu_ctx)
    assert T.same_chain(got, T.twins_chain(np.ascontiguousarray(ladders), shocks, 200, 4)), what
    comp = T.components_of_columns(augmented_ladder_pnl(ladders, shocks, host=True), got["scenarios"])
    assert C.same_bits(got["comp_var"], comp[0]) and C.same_bits(got["comp_es"], comp[1]), what
    assert np.isfinite(got["var"]) and got["es"] >= got["var"], what


def test_sub_books_of_the_three_product_lines(gpu_ctx):
    """`sub_book_monte_carlo_allocate_tail` on the small mixed book equals the chain on `price_sub_books`' ladders with the
    same labels; one credit and one YoY augmented row set through ``ladders=`` with a Q-row factor."""
    from adrates_amd.market.position.engine import Engine
    from adrates_amd.market.position.sub_book_ladders import price_credit_sub_books, price_sub_books, price_yoy_sub_books
    from adrates_amd.market.position.yoy_book import YoYBook

    from . import _credit_ladder_cases as X
    from . import _ladder_pnl_cases as LC
    from . import _yoy_ladder_cases as Y
    model, ir = LC.gbp(LC.SCHEMES[0])
    book = LC.L.mixed_book(n_ois=60)
    keys = [5 * i // book.n_trades for i in range(book.n_trades)]          # five desks of consecutive trades
    P = len(ir.swap_rates)
    L = factor_from_covariance(C.covariance(P))
    eng = Engine(model)
    got = sub_book_monte_carlo_allocate_tail(eng, ir, book, keys, L, 20000, level=0.99, seed=3)
    lad = price_sub_books(eng, ir, book, keys, REQS)
    want = monte_carlo_allocate_tail(lad["delta"], lad["gamma"], L, 20000, seed=3, ctx=gpu_ctx)
    assert got["labels"] == lad["labels"] and T.same_chain(got, want)
    assert got["es"] >= got["var"] > 0.0

    trades, spreads, ckeys, buckets = X.explain_book()
    credit = price_credit_sub_books(eng, ir, trades, spreads, ckeys, buckets, REQS)
    _check_ladders(gpu_ctx, credit["ladders"], P + len(credit["buckets"]), "credit")

    ymodel, swaps, ykeys = Y.explain_book()
    yb = YoYBook(swaps, ymodel)
    yoy = price_yoy_sub_books(Engine(ymodel), yb.curve, yb.inflation_curve, swaps, ykeys, REQS)
    _check_ladders(gpu_ctx, yoy["ladders"], len(yoy["tenors"]) + len(yoy["infl_tenors"]), "inflation")
