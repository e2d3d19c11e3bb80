"""Monte Carlo delta-gamma VaR on the CPU: the shock generator's host twin (adr_shock_normal_host) against the published
Philox known answers, a Python-integer restatement of the uniforms (bit for bit) and an mpmath restatement of the normals
and the products (the issue's bounds); its independence of how a set is cut; the tail select's twin
(adr_scenario_tail_select_host) against NumPy, bit for bit; the Python layer on the host route.

Worst observed share of the bounds on the host (the record, not a limit): z 0.096 of 64 eps max(1, |z|), x 0.056 of
(64 + F) eps sum |f| max(1, |z|)."""
import numpy as np
import pytest

from adrates_amd import _native
from adrates_amd.market.position.ladder_pnl import ladder_pnl
from adrates_amd.market.position.monte_carlo import (factor_from_covariance, monte_carlo_shocks, monte_carlo_var_es,
                                                     sub_book_monte_carlo_var_es, tail_measures_select)
from adrates_amd.market.position.scenarios import tail_count, tail_measures
from adrates_amd.utils.error import LibError

from . import _monte_carlo_cases as C

host = _native.shock_normal_host


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------------------------------------------------- generator
@pytest.mark.parametrize("counter,key,want", C.KNOWN_ANSWERS)
def test_philox_known_answers(native_lib, counter, key, want):
    assert tuple(int(w) for w in _native.shock_words_host(counter, key)) == want
    assert C.philox(counter, key) == want, "the restatement itself"


@pytest.mark.parametrize("seed", C.SEEDS)
def test_uniforms_against_integer_arithmetic(native_lib, seed):
    """u1 and u2 of three pairs of every index row, bit for bit, with and without the antithetic pairing."""
    for g in C.INDICES:
        for anti, first in ((False, g), (True, 2 * g), (True, 2 * g + 1)):
            u = _native.shock_uniforms(1, 5, seed, anti, first)
            want = np.array([C.uniform_doubles(seed, g, i) for i in range(3)])
            assert np.array_equal(bits(u[0]), bits(want)), (seed, g, anti)
            assert np.all((u > 0.0) & (u <= 1.0))
    # the one rounding of the map: n + 0.5 is not a double from 2^52 on, and the restatement rounds the same way
    assert (2 * (2 ** 53 - 1) + 1) / 2 ** 54 == 1.0 and (2 * 0 + 1) / 2 ** 54 == 2.0 ** -54


def test_normals_and_products_against_mpmath(native_lib):
    """z through the identity factor and x through dense factors on the index rows of every seed."""
    worst_z = worst_x = 0.0
    for seed in C.SEEDS:
        for g in C.INDICES:
            z = host(np.eye(8), 1, seed, False, g)
            worst_z = max(worst_z, C.worst_z_ratio(seed, [g], z))
            for P, F in ((8, 8), (9, 5)):
                f = C.factor_matrix(P, F)
                worst_x = max(worst_x, C.worst_x_ratio(seed, [g], f, host(f, 1, seed, False, g)))
                worst_x = max(worst_x, C.worst_x_ratio(seed, [2 * g + 1], f, host(f, 1, seed, True, 2 * g + 1), True))
    print(f"host twin: worst |dz| {worst_z:.3f} of its bound, worst |dx| {worst_x:.3f} of its bound")
    assert worst_z <= 1.0 and worst_x <= 1.0


def test_rows_do_not_depend_on_the_cut(native_lib):
    f = C.factor_matrix(9, 5)
    for anti in (False, True):
        for first in (0, 7):
            whole = host(f, 200, 11, anti, first)
            at, pieces = first, []
            for n in (1, 63, 64, 72):
                pieces.append(host(f, n, 11, anti, at))
                at += n
            assert np.array_equal(bits(np.vstack(pieces)), bits(whole)), (anti, first)
            for S in (1, 63, 129):                                  # a row does not change with S
                assert np.array_equal(bits(host(f, S, 11, anti, first)), bits(whole[:S]))
            assert np.array_equal(bits(host(f, 50, 11, anti, first + 150)), bits(whole[150:]))
    # antithetic: odd global rows are the exact negation of the even rows before them - odd first_scenario, odd S
    x = host(f, 201, 11, True, 3)                                   # global rows 3 .. 203
    assert np.array_equal(bits(x[1:200:2]), bits(-x[2:201:2]))      # (3, 4) is no pair: x[1] and x[2] are rows (4, 5)
    even = host(f, 100, 11, True, 4)
    assert np.array_equal(bits(even[0::2]), bits(-even[1::2])) and np.array_equal(bits(even), bits(x[1:101]))
    plain = host(f, 4, 11, False, 2)
    assert np.array_equal(bits(even[0:8:2]), bits(plain)), "pair i of an antithetic set is row i of the plain one"


@pytest.mark.parametrize("P,F", C.GEOMETRY)
def test_geometry_against_the_reference(native_lib, P, F):
    f = C.factor_matrix(P, F)
    big = host(f, max(C.SCENARIOS), C.GEOMETRY_SEED)
    worst = C.worst_x_ratio(C.GEOMETRY_SEED, range(max(C.SCENARIOS)), f, big)
    print(f"host twin, P = {P}, F = {F}: worst |dx| {worst:.3f} of its bound")
    assert worst <= 1.0
    for S in C.SCENARIOS:
        assert np.array_equal(bits(host(f, S, C.GEOMETRY_SEED)), bits(big[:S])), S


def test_zero_rows_and_columns(native_lib):
    """A zero row gives +0.0 (-0.0 on the negated rows of an antithetic set); a zero column drops its normal exactly."""
    z = host(np.eye(3), 66, 5)
    f = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    x = host(f, 66, 5)
    assert np.array_equal(bits(x[:, 0]), bits(z[:, 0])) and np.array_equal(bits(x[:, 2]), bits(z[:, 2]))
    assert np.array_equal(bits(x[:, 1]), bits(np.zeros(66)))
    xa = host(f, 66, 5, True)
    assert np.array_equal(bits(xa[:, 1]), bits(np.where(np.arange(66) % 2 == 1, -0.0, 0.0)))
    assert np.array_equal(bits(xa[0::2]), bits(x[:33])) and np.array_equal(bits(xa[1::2]), bits(-x[:33]))


def test_generator_refusals(native_lib):
    lib, p = _native.load(), _native._ptr
    out, f = np.zeros((4, 4)), np.eye(4)
    call = lambda first, S, P, F, fac=f, o=out, anti=0: lib.adr_shock_normal_host(1, first, S, P, F, p(fac), anti, p(o))
    assert call(0, 4, 4, 4) == 0
    for args in ((0, 4, 3, 4), (0, 4, 257, 4), (0, 0, 4, 4), (0, -1, 4, 4), (-1, 4, 4, 4), (0, 4, 4, 0), (2 ** 63 - 2, 4, 4, 4)):
        assert call(*args) == -1, args
    assert call(0, 4, 4, 4, fac=None) == -1 and call(0, 4, 4, 4, o=None) == -1 and call(0, 4, 4, 4, anti=2) == -1
    with pytest.raises(LibError) as e:
        monte_carlo_shocks(np.zeros((2, 3)), 4, 1, host=True)
    assert e.value.status == -1 and "F <= P" in str(e.value)


def test_statistics_of_the_twin():
    """S = 65 536 draws of a fixed covariance with a fixed seed: means within 5 sigma / sqrt(S), covariance entries within
    5 sqrt((C_pp C_qq + C_pq^2) / S); antithetic means vanish to the rounding of the sum."""
    S, P = 65536, 8
    cov = C.covariance(P)
    L = factor_from_covariance(cov)
    assert np.allclose(L @ L.T, cov, rtol=1e-13, atol=0.0) and np.array_equal(L, np.tril(L))
    x = monte_carlo_shocks(L, S, 2026, host=True)
    sd = np.sqrt(np.diag(cov))
    assert np.all(np.abs(x.mean(0)) <= 5.0 * sd / np.sqrt(S)), x.mean(0) / (sd / np.sqrt(S))
    got = (x - x.mean(0)).T @ (x - x.mean(0)) / (S - 1)
    tol = 5.0 * np.sqrt((np.outer(np.diag(cov), np.diag(cov)) + cov ** 2) / S)
    assert np.all(np.abs(got - cov) <= tol), np.max(np.abs(got - cov) / tol)
    xa = monte_carlo_shocks(L, S, 2026, antithetic=True, host=True)
    assert np.all(np.abs(xa.sum(0)) <= S * 2.0 ** -52 * np.abs(xa).max(0))


def test_factor_from_covariance():
    cov = C.covariance(6)
    pca = factor_from_covariance(cov, 6)
    assert np.allclose(pca @ pca.T, cov, rtol=1e-12, atol=1e-12)
    lam = np.linalg.eigvalsh(cov)[::-1]
    two = factor_from_covariance(cov, 2)
    assert two.shape == (6, 2) and np.allclose((two ** 2).sum(0), lam[:2], rtol=1e-12)
    v = np.array([[1.0], [2.0], [-1.0]])
    semi = factor_from_covariance(v @ v.T)                          # rank one: a zero pivot leaves zero columns
    assert np.allclose(semi @ semi.T, v @ v.T, atol=1e-15) and not np.any(semi[:, 1:])
    for bad in (np.array([[1.0, 2.0], [2.0, 1.0]]), np.array([[1.0, 0.5], [0.4, 1.0]]), np.ones((2, 3)), np.array([[np.nan]])):
        with pytest.raises(LibError):
            factor_from_covariance(bad)
    with pytest.raises(LibError):
        factor_from_covariance(cov, 7)


# -------------------------------------------------------------------------------------------------------- tail select
@pytest.mark.parametrize("m", C.WIDTHS)
def test_tail_select_twin_against_numpy(native_lib, m):
    """Every content, base column and tail count of the table at width m: NumPy's bits, and adr_scenario_tail_host's
    where that takes the rows."""
    for content in C.CONTENTS:
        for B in ((1, 3) if content in ("normal", "nan") else (3,)):
            for k in C.tail_counts(m):
                pnl = C.pnl_rows(content, B, m, k)
                for base_col, width in C.base_cols(m):
                    rows = C.with_base(pnl, base_col, content)
                    assert rows.shape == (B, width)
                    ordered, nan = C.sorted_pnl(rows, base_col)
                    var, es = _native.scenario_tail_select_host(rows, k, base_col)
                    rv, re = C.numpy_tail(ordered, nan, k)
                    assert C.same_bits(var, rv) and C.same_bits(es, re), (content, B, k, base_col)
                    if content == "nan":
                        assert list(np.isnan(var)) == [b == min(1, B - 1) for b in range(B)]
                    if m <= C.TAIL_MAX:
                        tv, te = _native.scenario_tail_host(rows, k, base_col)
                        assert C.same_bits(var, tv) and C.same_bits(es, te), (content, B, k, base_col)


def test_tail_select_refusals(native_lib):
    rows = np.zeros((2, 20000))
    for k, base_col, status in ((16385, -1, -2), (0, -1, -1), (20001, -1, -1), (20000, 0, -1), (5, 20000, -1), (5, -2, -1)):
        with pytest.raises(LibError) as e:
            _native.scenario_tail_select_host(rows, k, base_col)
        assert e.value.status == status, (k, base_col)
    lib, p = _native.load(), _native._ptr
    out = np.zeros(2)
    assert lib.adr_scenario_tail_select_host(0, 5, p(rows), -1, 1, p(out), p(out)) == -1
    assert lib.adr_scenario_tail_select_host(2, 5, None, -1, 1, p(out), p(out)) == -1
    assert lib.adr_scenario_tail_select_host(2, 5, p(rows), -1, 1, None, p(out)) == -1
    assert _native.scenario_tail_select_work(0, 5, 1) == 0 and _native.scenario_tail_select_work(2, 20000, 16385) == 0
    assert _native.scenario_tail_select_work(2, 20000, 200) >= 2 * (200 * 8 + 2048 * 4)
    with pytest.raises(LibError) as e:                              # the Python layer: the limit is on the tail count
        tail_measures_select(np.zeros((1, 400000)), 0.95, host=True)
    assert e.value.status == _native.ADR_ERR_UNSUPPORTED
    assert tail_count(0.99, 1048576) <= _native.SCENARIO_TAIL_MAX


# -------------------------------------------------------------------------------------------------------- Python layer
def test_python_layer_on_the_host():
    """`tail_measures_select` is `tail_measures` where that has a kernel and goes on beyond; `monte_carlo_var_es` on the
    host route is the three twins in a row, whatever the tiling."""
    rows = C.pnl_rows("normal", 3, 3000, 30)
    for level in (0.99, 0.75):
        for a, b in zip(tail_measures_select(rows, level, host=True), tail_measures(rows, level, host=True)):
            assert C.same_bits(a, b)
    wide = C.pnl_rows("normal", 2, 40000, 400)
    var, es = tail_measures_select(wide, 0.99, host=True)
    ordered, nan = C.sorted_pnl(wide, -1)
    assert all(C.same_bits(a, b) for a, b in zip((var, es), C.numpy_tail(ordered, nan, tail_count(0.99, 40000))))
    delta, gamma = C.ladders(7, 9)
    L = factor_from_covariance(C.covariance(9))
    S = 20000
    shocks = monte_carlo_shocks(L, S, 5, antithetic=True, host=True)
    want = tail_measures_select(ladder_pnl(delta, gamma, shocks, host=True), 0.99, host=True)
    for max_bytes in (2 ** 31, 8 * S, 3 * 8 * S):
        got = monte_carlo_var_es(delta, gamma, L, S, seed=5, antithetic=True, host=True, max_bytes=max_bytes)
        assert C.same_bits(got["var"], want[0]) and C.same_bits(got["es"], want[1]), max_bytes
    from adrates_amd.market.position.ladder_pnl import ladder_rows
    again = monte_carlo_var_es(None, None, L, S, seed=5, antithetic=True, host=True, ladders=ladder_rows(delta, gamma))
    assert C.same_bits(again["var"], want[0]) and C.same_bits(again["es"], want[1])
    with pytest.raises(LibError, match="not both"):
        monte_carlo_var_es(delta, None, L, S, host=True, ladders=ladder_rows(delta, gamma))
    with pytest.raises(LibError):
        monte_carlo_var_es(delta, gamma, L[:8], S, host=True)


def test_sub_books_on_the_host():
    """`sub_book_monte_carlo_var_es` on the small mixed book: `price_sub_books`' ladders through `monte_carlo_var_es`."""
    from adrates_amd.market.position.engine import Engine
    from adrates_amd.market.position.sub_book_ladders import price_sub_books
    from adrates_amd.utils.global_types import RequestTypes

    from . import _ladder_pnl_cases as LC
    model, ir = LC.gbp(LC.SCHEMES[0])
    book = LC.L.mixed_book(n_ois=60)
    keys = [5 * i // book.n_trades for i in range(book.n_trades)]          # five desks of consecutive trades
    P = len(ir.swap_rates)
    L = factor_from_covariance(C.covariance(P), 4)
    eng = Engine(model)
    got = sub_book_monte_carlo_var_es(eng, ir, book, keys, L, 20000, level=0.99, seed=3, host=True)
    lad = price_sub_books(eng, ir, book, keys, {RequestTypes.VALUE, RequestTypes.DELTA, RequestTypes.GAMMA}, host=True)
    want = monte_carlo_var_es(lad["delta"], lad["gamma"], L, 20000, seed=3, host=True)
    assert got["labels"] == lad["labels"] and C.same_bits(got["var"], want["var"]) and C.same_bits(got["es"], want["es"])
    assert np.all(got["es"] >= got["var"]) and np.all(got["var"] > 0.0)
