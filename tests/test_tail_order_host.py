"""The ordered tail select, the allocation of a matrix of any width and the Monte Carlo tail allocation on their CPU twins
(adr_scenario_tail_order_host, adr_scenario_tail_alloc_select_host, adr_scenario_total_host, adr_shock_gather_host,
adr_tail_components_host; `monte_carlo_allocate_tail` with ``host=True``), on the tables of tests/_tail_order_cases.py:
the select against the independent NumPy statement with the tie rows that decide the tie rule, the refusals, the
allocation against adr_scenario_tail_alloc_host and `_allocate_tail_numpy`, and the chain's bit contracts, its derived
difference from the matrix allocation and additivity."""
import numpy as np
import pytest

from adrates_amd import _native
from adrates_amd.market.position.ladder_pnl import augmented_ladder_pnl, ladder_pnl, ladder_rows
from adrates_amd.market.position.monte_carlo import (allocate_tail_select, firm_ladder, monte_carlo_allocate_tail, monte_carlo_shocks,
                                                     monte_carlo_var_es, sub_book_monte_carlo_allocate_tail)
from adrates_amd.market.position.scenarios import _allocate_tail_numpy, allocate_tail, tail_count
from adrates_amd.utils.error import LibError
from adrates_amd.utils.global_types import RequestTypes

from . import _monte_carlo_cases as C
from . import _tail_alloc_cases as A
from . import _tail_order_cases as T

REQS = {RequestTypes.VALUE, RequestTypes.DELTA, RequestTypes.GAMMA}


# ------------------------------------------------------------------------------------------------------ ordered select
@pytest.mark.parametrize("m", T.WIDTHS)
def test_order_twin_against_numpy(native_lib, m):
    """Every content and tail count of the table at width m, the base columns as the table spreads them: the indices of
    the statement, var and es bit for bit, and adr_scenario_tail_select_host's var and es."""
    for content, B, k, base_col, rows in T.select_calls(m):
        got = _native.scenario_tail_order_host(rows, k, base_col)
        assert T.same_order(got, T.numpy_order(rows, base_col, k)), (content, B, k, base_col)
        sel = _native.scenario_tail_select_host(rows, k, base_col)
        assert C.same_bits(got[1], sel[0]) and C.same_bits(got[2], sel[1]), (content, B, k, base_col)


def test_order_twin_on_many_rows(native_lib):
    B, m = T.MANY_ROWS
    rows = C.pnl_rows("normal", B, m, 3)
    assert T.same_order(_native.scenario_tail_order_host(rows, 3), T.numpy_order(rows, -1, 3))


@pytest.mark.parametrize("case", T.TIE_CASES, ids=[c[0] for c in T.TIE_CASES])
def test_order_twin_takes_the_lowest_ties(native_lib, case):
    rows, k, taken = T.tie_call(case)
    got = _native.scenario_tail_order_host(rows, k)
    assert T.same_order(got, T.numpy_order(rows, -1, k))
    assert np.array_equal(np.sort(got[0][1]), np.sort(taken)), "exactly the lowest indices of the run"
    assert np.array_equal(got[0][0], np.arange(k)), "equal values: the first k indices in order"


def test_order_twin_nan_rows_stand_alone(native_lib):
    rows = C.pnl_rows("nan", 3, 8193, 82)
    order, var, es = _native.scenario_tail_order_host(rows, 82)
    assert np.all(order[1] == -1) and np.isnan(var[1]) and np.isnan(es[1])
    assert np.all(order[[0, 2]] >= 0) and np.all(np.isfinite(var[[0, 2]])) and np.all(np.isfinite(es[[0, 2]]))


def test_order_twin_refusals(native_lib):
    rows = np.zeros((2, 20000))
    for k, base_col, status in ((8193, -1, -2), (0, -1, -1), (20001, -1, -1), (20000, 0, -1), (5, 20000, -1), (5, -2, -1)):
        with pytest.raises(LibError) as e:
            _native.scenario_tail_order_host(rows, k, base_col)
        assert e.value.status == status, (k, base_col)
        with pytest.raises(LibError) as e:
            _native.scenario_tail_alloc_select_host(rows, k, base_col)
        assert e.value.status == status, (k, base_col)
    lib, p = _native.load(), _native._ptr
    order, v = np.zeros(4, dtype=np.int64), np.zeros(4)
    o = p(order, _native._i64p)
    assert lib.adr_scenario_tail_order_host(0, 8, p(rows), -1, 1, o, p(v), p(v)) == -1
    assert lib.adr_scenario_tail_order_host(2, 8, None, -1, 1, o, p(v), p(v)) == -1
    assert lib.adr_scenario_tail_order_host(2, 8, p(rows), -1, 1, None, p(v), p(v)) == -1
    assert lib.adr_scenario_tail_order_host(2, 8, p(rows), -1, 1, o, None, p(v)) == -1
    assert lib.adr_scenario_tail_alloc_select_host(2, 8, p(rows), -1, 1, p(v), p(v), None, p(v)) == -1
    assert lib.adr_shock_gather_host(0, 2, p(rows), 4, o, p(v)) == -1 and lib.adr_shock_gather_host(1, 257, p(rows), 4, o, p(v)) == -1
    assert lib.adr_tail_components_host(0, 2, p(rows), p(v), p(v)) == -1 and lib.adr_tail_components_host(1, 0, p(rows), p(v), p(v)) == -1
    assert lib.adr_scenario_total_host(0, 2, p(rows), -1, p(v)) == -1 and lib.adr_scenario_total_host(1, 2, p(rows), 2, p(v)) == -1
    assert _native.scenario_tail_order_work(1, 20000, 8193) == 0 and _native.scenario_tail_alloc_select_work(1, 20000, 8193) == 0
    assert _native.scenario_tail_order_work(1, 20000, 8192) % 16 == 0 and _native.scenario_tail_order_work(3, 20000, 200) > 0


# ------------------------------------------------------------------------------------------------ gather and components
def test_gather_and_components_twins(native_lib):
    rng = np.random.default_rng(8)
    shocks = rng.standard_normal((500, 7))
    order = rng.permutation(500)[:130]
    assert np.array_equal(_native.shock_gather_host(shocks, order), shocks[order])
    bad = order.copy()
    bad[5] = 500
    got = _native.shock_gather_host(shocks, bad)
    assert np.all(np.isnan(got[5])) and np.array_equal(np.delete(got, 5, 0), np.delete(shocks[order], 5, 0))
    bad[0] = -1
    assert np.all(np.isnan(_native.shock_gather_host(shocks, bad)))
    pnl = rng.standard_normal((67, 500)) * 1e6
    want = T.components_of_columns(pnl, order)
    got = _native.tail_components_host(np.ascontiguousarray(pnl[:, order]))
    assert C.same_bits(got[0], want[0]) and C.same_bits(got[1], want[1])
    rows = A.matrix(130, 300)
    assert C.same_bits(_native.scenario_total_host(rows), A.slot_total(rows))
    assert C.same_bits(_native.scenario_total_host(rows, 299), A.slot_total(A.pnl_of(rows, 299)))


# ---------------------------------------------------------------------------------------------------- matrix allocation
@pytest.mark.parametrize("S", (1, 100, 1025, 8192))
def test_alloc_select_twin_has_allocs_bits(native_lib, S):
    for rows, base_col, k in A.calls(S):
        if rows.shape[0] <= 129:
            assert T.same_alloc(_native.scenario_tail_alloc_select_host(rows, k, base_col),
                                _native.scenario_tail_alloc_host(rows, k, base_col)), (rows.shape, base_col, k)
    for name, rows, base_col, k in A.special_calls():
        assert T.same_alloc(_native.scenario_tail_alloc_select_host(rows, k, base_col),
                            _native.scenario_tail_alloc_host(rows, k, base_col)), name
    for rows, base_col, k in A.nan_calls():
        got = _native.scenario_tail_alloc_select_host(rows, k, base_col)
        assert all(np.all(np.isnan(got[f])) for f in ("var", "es", "comp_var", "comp_es"))


@pytest.mark.parametrize("m", T.ALLOC_WIDE)
@pytest.mark.parametrize("B", T.ALLOC_ROWS)
def test_alloc_select_twin_beyond_the_row_limit(native_lib, B, m):
    rows = T.alloc_matrix(B, m)
    for k in (1, tail_count(0.99, m), min(m, T.ORDER_MAX)):
        assert T.same_alloc(_native.scenario_tail_alloc_select_host(rows, k), _allocate_tail_numpy(rows, k, -1)), k
    with_base = np.ascontiguousarray(np.hstack([rows[:, :7], np.zeros((B, 1)), rows[:, 7:]]))
    assert T.same_alloc(_native.scenario_tail_alloc_select_host(with_base, 82, 7), _allocate_tail_numpy(with_base, 82, 7))
    got = allocate_tail_select(rows, 0.99, host=True)
    assert T.same_alloc(got, allocate_tail(rows, 0.99, host=True)), "allocate_tail goes to NumPy at this width"


def test_alloc_select_twin_on_tied_totals(native_lib):
    rows = T.tied_totals()
    tot = A.slot_total(rows)
    assert np.sum(tot == -5.0) == 30 and np.sum(tot == 0.0) == rows.shape[1] - 30 and len({r.tobytes() for r in rows}) == rows.shape[0]
    for k in (30, 31, 82, 4097):
        got = _native.scenario_tail_alloc_select_host(rows, k)
        assert T.same_alloc(got, _allocate_tail_numpy(rows, k, -1)), k
    with pytest.raises(LibError) as e:
        allocate_tail_select(np.zeros((2, 900000)), 0.99, host=True)
    assert e.value.status == _native.ADR_ERR_UNSUPPORTED


# -------------------------------------------------------------------------------------------------------------- chain
@pytest.mark.parametrize("P", [9, 32])
def test_chain_on_the_twins(native_lib, P):
    """`monte_carlo_allocate_tail` with host=True: the twins' chain step by step whatever the tiling, the firm's figures
    from `monte_carlo_var_es` of the firm's row, the components from the full matrix, the derived difference from the
    matrix allocation and additivity.  Observed here: the differences of var and es at most 0.002 of the bound, the sums
    of the components within 0.01 of theirs."""
    delta, gamma, L = T.chain_case(P)
    rows, S, k = ladder_rows(delta, gamma), T.CHAIN_S, T.CHAIN_K
    shocks = monte_carlo_shocks(L, S, T.CHAIN_SEED, host=True)
    want = T.twins_chain(rows, shocks, k, T.CHAIN_B)
    for desks in (19, 8, 1):
        got = monte_carlo_allocate_tail(delta, gamma, L, S, level=T.CHAIN_LEVEL, seed=T.CHAIN_SEED, host=True, max_bytes=desks * 8 * k)
        assert T.same_chain(got, want), desks
    assert got["scenarios"].shape == (k,) and got["scenarios"].dtype == np.int64
    firm = monte_carlo_var_es(None, None, L, S, level=T.CHAIN_LEVEL, seed=T.CHAIN_SEED, host=True, ladders=firm_ladder(rows)[None])
    assert C.same_bits(firm["var"], [got["var"]]) and C.same_bits(firm["es"], [got["es"]])
    pnl = ladder_pnl(delta, gamma, shocks, host=True)
    comp = T.components_of_columns(pnl, got["scenarios"])
    assert C.same_bits(got["comp_var"], comp[0]) and C.same_bits(got["comp_es"], comp[1])
    T.check_cross_and_additivity(got, allocate_tail_select(pnl, T.CHAIN_LEVEL, host=True), pnl, delta, gamma, shocks, k, f"host, P = {P}")
    anti = monte_carlo_allocate_tail(delta, gamma, L, S, level=0.95, seed=T.CHAIN_SEED, antithetic=True, host=True)
    xa = monte_carlo_shocks(L, S, T.CHAIN_SEED, antithetic=True, host=True)
    assert T.same_chain(anti, T.twins_chain(rows, xa, tail_count(0.95, S), T.CHAIN_B))


def test_chain_refusals_and_nan(native_lib):
    delta, gamma, L = T.chain_case(9)
    with pytest.raises(LibError) as e:
        monte_carlo_allocate_tail(delta, gamma, L, 1048576, level=0.99, host=True)
    assert e.value.status == _native.ADR_ERR_UNSUPPORTED
    assert tail_count(0.995, 1048576) <= T.ORDER_MAX and tail_count(0.99, 786432) <= T.ORDER_MAX
    with pytest.raises(LibError):
        monte_carlo_allocate_tail(delta, gamma, L, 1000, host=True, ladders=ladder_rows(delta, gamma))
    bad = delta.copy()
    bad[3, 2] = np.nan
    got = monte_carlo_allocate_tail(bad, gamma, L, 3000, host=True)
    assert np.isnan(got["var"]) and np.isnan(got["es"]) and np.all(np.isnan(got["comp_var"])) and np.all(np.isnan(got["comp_es"]))
    assert np.all(got["scenarios"] == -1)


def test_chain_on_augmented_rows(native_lib):
    """The ``ladders=`` route on a seeded augmented row set of width 1 + Q + Q Q with a Q-row factor of fewer columns."""
    Q, S = 13, 20000
    delta, gamma = C.ladders(7, Q, seed=12)
    ladders = ladder_rows(delta, gamma)
    from adrates_amd.market.position.monte_carlo import factor_from_covariance
    L = factor_from_covariance(C.covariance(Q), 6)
    got = monte_carlo_allocate_tail(None, None, L, S, seed=21, host=True, ladders=ladders)
    shocks = monte_carlo_shocks(L, S, 21, host=True)
    assert T.same_chain(got, T.twins_chain(ladders, shocks, 200, 7))
    comp = T.components_of_columns(augmented_ladder_pnl(ladders, shocks, host=True), got["scenarios"])
    assert C.same_bits(got["comp_var"], comp[0]) and C.same_bits(got["comp_es"], comp[1])


def test_sub_book_chain_on_the_twins(native_lib):
    from adrates_amd.market.position.engine import Engine
    from adrates_amd.market.position.sub_book_ladders import price_sub_books

    from . import _ladder_pnl_cases as LC
    model, ir = LC.gbp(LC.SCHEMES[0])
    book = LC.L.mixed_book(n_ois=60)
    keys = [5 * i // book.n_trades for i in range(book.n_trades)]
    from adrates_amd.market.position.monte_carlo import factor_from_covariance
    L = factor_from_covariance(C.covariance(len(ir.swap_rates)))
    eng = Engine(model)
    got = sub_book_monte_carlo_allocate_tail(eng, ir, book, keys, L, 20000, level=0.99, seed=3, host=True)
    lad = price_sub_books(eng, ir, book, keys, REQS, host=True)
    want = monte_carlo_allocate_tail(lad["delta"], lad["gamma"], L, 20000, seed=3, host=True)
    assert got["labels"] == lad["labels"] and T.same_chain(got, want)
    assert got["es"] >= got["var"] > 0.0
