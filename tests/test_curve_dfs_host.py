"""Discount factors of shocked curves and Monte Carlo VaR by full revaluation on the CPU twins
(adr_curve_dfs_shocked_host, csrc/curve_dfs.hip; market/position/monte_carlo.py with ``host=True``), on the tables of
tests/_curve_dfs_cases.py: the scan against its NumPy restatement and the host curve builder bit for bit, the flags and
refusals, the chain against `revalue_on_curves_sub_books`, whatever the tiling, and the third-order gap to delta-gamma."""
import numpy as np
import pytest

from adrates_amd import _native
from adrates_amd.market.curves.curve_tables import build_engine_curve
from adrates_amd.market.position.engine import Engine
from adrates_amd.market.position.ladder_pnl import delta_gamma_sub_books
from adrates_amd.market.position.monte_carlo import (ShockedCurves, allocate_tail_select, factor_from_covariance,
                                                     monte_carlo_explain_var_es, monte_carlo_revalue_var_es, monte_carlo_shocks,
                                                     revalue_scenario_bytes, revalue_shocks_sub_books,
                                                     sub_book_monte_carlo_var_es, tail_measures_select)
from adrates_amd.market.position.scenarios import revalue_on_curves_sub_books, tail_count
from adrates_amd.utils.error import LibError

from . import _curve_dfs_cases as C
from . import _tail_alloc_cases as TA


def twin(g, x):
    return _native.curve_dfs_shocked_host(g.acc, g.pillar, g.prev_idx, g.rates, x)


# ---------------------------------------------------------------------------------------------------------- bootstrap
@pytest.mark.parametrize("name", C.GRIDS)
def test_twin_has_the_restatements_bits(native_lib, name):
    g = C.grid(name)
    for S in C.SCENARIOS:
        x = C.rows(g.rates.size, S)
        dfs, bad = twin(g, x)
        assert dfs.shape == (S, g.n_knots) and np.array_equal(C.bits(dfs), C.bits(C.restate(g, x))), S
        assert bad.dtype == np.int32 and not bad.any()
    assert np.array_equal(C.bits(twin(g, np.zeros((1, g.rates.size)))[0][0]), C.bits(g.dfs)), "a zero row: the base curve's bits"


@pytest.mark.parametrize("name", C.MODEL_GRIDS)
def test_twin_has_the_host_builders_bits(native_lib, name):
    """Every entry against `build_engine_curve` at the shocked rates; on the 1 242-knot grid the three fixed rows and two
    drawn ones (the restatement above holds every row of it)."""
    g, c = C.grid(name), C.model_curve(name)
    x = C.rows(g.rates.size, 5 if name == "wide64" else max(C.SCENARIOS))
    dfs, _ = twin(g, x)
    for s in range(x.shape[0]):
        built = build_engine_curve(list(g.rates + x[s] * 1e-4), c.swap_times, c.year_fracs, with_hessian=False)
        assert np.array_equal(C.bits(dfs[s]), C.bits(built.dfs)), s


def test_extra_columns_are_not_read(native_lib):
    for name in ("semi_annual3", "gbp32"):
        g = C.grid(name)
        P = g.rates.size
        x = C.rows(P, 65)
        wide = np.hstack([x, np.full((65, 5), np.nan)])
        dfs, bad = twin(g, wide)
        assert np.array_equal(C.bits(dfs), C.bits(twin(g, x)[0])) and not bad.any()


@pytest.mark.parametrize("name", C.GRIDS)
def test_bad_rows_are_flagged_alone(native_lib, name):
    g = C.grid(name)
    x, flags = C.bad_rows(g)
    ref = C.restate(g, x)
    assert np.array_equal(C.is_bad(ref), flags == 1), "the restatement itself must give a bad discount factor there"
    assert np.any(ref[1][np.isfinite(ref[1])] <= 0.0) and np.isnan(ref[3]).any()
    dfs, bad = twin(g, x)
    assert np.array_equal(bad, flags)
    assert C.same_bits(dfs, ref), "a flagged row is written all the same"
    good = flags == 0
    assert np.array_equal(C.bits(dfs[good]), C.bits(twin(g, x[good])[0])), "the neighbours keep their bits"


def test_twin_refusals(native_lib):
    g = C.grid("semi_annual3")
    K, P = g.n_knots, g.rates.size
    x = C.rows(P, 4)
    pillar, prev = g.pillar.astype(np.int32), g.prev_idx.astype(np.int32)
    dfs, bad = np.empty((4, K)), np.empty(4, dtype=np.int32)
    p, ip = _native._ptr, lambda a: _native._ptr(a, _native._i32p)
    call = lambda **kw: _native._check(native_lib.adr_curve_dfs_shocked_host(*[{**dict(
        K=K, P=P, acc=p(g.acc), pillar=ip(pillar), prev=ip(prev), base=p(g.rates), S=4, ld=P, x=p(x), dfs=p(dfs), bad=ip(bad)), **kw}[k]
        for k in ("K", "P", "acc", "pillar", "prev", "base", "S", "ld", "x", "dfs", "bad")]), "adr_curve_dfs_shocked_host")
    call()
    call(bad=None)                                                  # the flags are optional
    for kw in (dict(acc=None), dict(pillar=None), dict(prev=None), dict(base=None), dict(x=None), dict(dfs=None), dict(S=0),
               dict(ld=P - 1), dict(base=p(np.array([0.03, np.inf, 0.04]))), dict(base=p(np.array([np.nan, 0.03, 0.04]))),
               dict(pillar=ip(np.where(np.arange(K) == 2, P, pillar).astype(np.int32))),
               dict(pillar=ip(np.where(np.arange(K) == 2, -1, pillar).astype(np.int32))),
               dict(prev=ip(np.where(np.arange(K) == 3, K, prev).astype(np.int32))),
               dict(prev=ip(np.where(np.arange(K) == 3, -2, prev).astype(np.int32)))):
        with pytest.raises(LibError) as e:
            call(**kw)
        assert e.value.status == -1, kw
    with pytest.raises(LibError):
        _native.curve_dfs_shocked_host(g.acc, g.pillar[:-1], g.prev_idx, g.rates, x)
    with pytest.raises(LibError):
        _native.curve_dfs_shocked_host(g.acc, g.pillar, g.prev_idx, g.rates, x[0])


# -------------------------------------------------------------------------------------------------------------- chain
@pytest.fixture(scope="module")
def chain(native_lib):
    """The model, its shocked-curve recipe, the factor, the host shock rows and the host chain's P&L, made once."""
    model, ir = C.LP.gbp(C.INTERP)
    curves = ShockedCurves(model, "GBP_OIS_SONIA")
    factor = factor_from_covariance(C.covariance(curves.n_pillars))
    x = monte_carlo_shocks(factor, C.CHAIN_S, C.SEED, host=True)
    pnl = revalue_shocks_sub_books(curves, C.chain_book(), C.chain_keys(), x, host=True)
    return dict(model=model, ir=ir, curves=curves, factor=factor, x=x, pnl=pnl)


def test_chain_has_the_bits_of_revaluation_on_the_twins_rows(chain):
    curves, x = chain["curves"], chain["x"]
    assert curves.base.hess is None and curves.n_knots == 264 and curves.n_pillars == 32
    assert chain["pnl"]["labels"] == [0, 1, 2, 3, 4] and chain["pnl"]["pnl"].shape == (5, C.CHAIN_S)
    dfs, bad = curves.dfs(np.vstack([x, np.zeros((1, 32))]), host=True)
    assert not bad.any() and np.array_equal(C.bits(dfs[-1]), C.bits(curves.base.dfs))
    sub = revalue_on_curves_sub_books(C.INTERP, curves.base.times, dfs, C.chain_book(), C.chain_keys(), C.VD, host=True)["sub_pv"]
    assert np.array_equal(C.bits(chain["pnl"]["pnl"]), C.bits(sub[:, :-1] - sub[:, -1:]))


def test_chain_does_not_depend_on_the_tiling(chain):
    curves, book, keys = chain["curves"], C.chain_book(), C.chain_keys()
    per, rows = revalue_scenario_bytes(curves, book.n_trades, 5), 8 * 5 * (C.CHAIN_S + 1)
    for tile in C.TILES:
        got = revalue_shocks_sub_books(curves, book, keys, chain["x"], host=True, max_bytes=rows + tile * per)
        assert np.array_equal(C.bits(got["pnl"]), C.bits(chain["pnl"]["pnl"])), tile
    with pytest.raises(LibError, match="do not fit max_bytes"):
        revalue_shocks_sub_books(curves, book, keys, chain["x"], host=True, max_bytes=rows + per - 1)


def test_zero_shock_row_is_exactly_zero(chain):
    x = chain["x"][:5].copy()
    x[2] = 0.0
    pnl = revalue_shocks_sub_books(chain["curves"], C.chain_book(), C.chain_keys(), x, host=True)["pnl"]
    assert np.array_equal(C.bits(pnl[:, 2]), C.bits(np.zeros(5))) and np.all(pnl[:, [0, 1, 3, 4]] != 0.0)


def test_columns_beyond_the_quotes_are_not_read(chain):
    """``shocks_bp [S, ld > P]``: three columns of NaN behind five of the chain's shock rows change no bit."""
    curves, book, keys, x = chain["curves"], C.chain_book(), C.chain_keys(), chain["x"][:5]
    want = revalue_shocks_sub_books(curves, book, keys, x, host=True)
    got = revalue_shocks_sub_books(curves, book, keys, np.hstack([x, np.full((5, 3), np.nan)]), host=True)
    assert got["labels"] == want["labels"] and np.all(want["pnl"] != 0.0) and np.array_equal(C.bits(got["pnl"]), C.bits(want["pnl"]))


def test_var_es_and_allocation_are_the_tail_entries_of_the_rows(chain):
    curves, book, keys, pnl = chain["curves"], C.chain_book(), C.chain_keys(), chain["pnl"]["pnl"]
    per = revalue_scenario_bytes(curves, book.n_trades, 5)
    for level in (0.99, 0.9):
        var, es = tail_measures_select(pnl, level, host=True)
        for max_bytes in (2 ** 31, 8 * 5 * (C.CHAIN_S + 1) + 64 * per):
            got = monte_carlo_revalue_var_es(curves, book, keys, chain["factor"], C.CHAIN_S, level=level, seed=C.SEED, host=True,
                                             max_bytes=max_bytes)
            assert sorted(got) == ["es", "labels", "var"] and got["labels"] == [0, 1, 2, 3, 4]
            assert np.array_equal(C.bits(got["var"]), C.bits(var)) and np.array_equal(C.bits(got["es"]), C.bits(es)), level
        got = monte_carlo_revalue_var_es(curves, book, keys, chain["factor"], C.CHAIN_S, level=level, seed=C.SEED, host=True, allocate=True)
        firm = allocate_tail_select(pnl, level, host=True)
        assert np.array_equal(C.bits(got["var"]), C.bits(var)) and np.array_equal(C.bits(got["es"]), C.bits(es))
        assert got["firm_var"] == firm["var"] and got["firm_es"] == firm["es"]
        assert np.array_equal(C.bits(got["comp_var"]), C.bits(firm["comp_var"])) and np.array_equal(C.bits(got["comp_es"]), C.bits(firm["comp_es"]))
        # the restatement of the allocation, and the components adding up to the firm's figures, as its own tests hold them
        TA.check(dict(var=got["firm_var"], es=got["firm_es"], comp_var=got["comp_var"], comp_es=got["comp_es"]), pnl, -1,
                 tail_count(level, C.CHAIN_S))


def test_bad_scenarios_raise(chain):
    curves, book, keys = chain["curves"], C.chain_book(), C.chain_keys()
    with pytest.raises(LibError, match=r"scenario\(s\) give a discount factor .* first at index \d+"):
        monte_carlo_revalue_var_es(curves, book, keys, chain["factor"] * 1e4, C.CHAIN_S, seed=C.SEED, host=True)
    x = chain["x"][:4].copy()
    x[1, 3], x[3, 0] = np.nan, np.nan
    with pytest.raises(LibError, match=r"2 scenario\(s\) .* first at index 1"):
        revalue_shocks_sub_books(curves, book, keys, x, host=True)
    with pytest.raises(LibError):
        revalue_shocks_sub_books(curves, book, keys, chain["x"][:, :31], host=True)
    with pytest.raises(LibError):
        monte_carlo_revalue_var_es(curves, book, keys, chain["factor"][:31], C.CHAIN_S, host=True)
    with pytest.raises(LibError):
        monte_carlo_revalue_var_es(curves, book, keys, chain["factor"], 0, host=True)


# ------------------------------------------------------------------------------------------ the reason for the feature
def test_gap_to_delta_gamma_is_third_order(chain):
    """The same seed with the factor L and with L / 2: the rows are exact halves, and the worst |full - delta-gamma| over
    the scenarios, per desk, falls by about 8.  Observed on the host twins: 8.229, 7.820, 7.893, 7.837, 7.844."""
    curves, book, keys, L = chain["curves"], C.chain_book(), C.chain_keys(), chain["factor"]
    engine = Engine(chain["model"])
    x, half = chain["x"], monte_carlo_shocks(0.5 * L, C.CHAIN_S, C.SEED, host=True)
    assert np.array_equal(C.bits(half), C.bits(0.5 * x))
    gap = []
    for rows, full in ((x, chain["pnl"]["pnl"]), (half, revalue_shocks_sub_books(curves, book, keys, half, host=True)["pnl"])):
        gap.append((full, delta_gamma_sub_books(engine, chain["ir"], book, keys, rows, host=True)["pnl"]))
    ratios = C.gap_ratios(*gap[0], *gap[1])
    print("host: gap ratios per desk", np.round(ratios, 3))
    assert np.all((C.GAP_BAND[0] < ratios) & (ratios < C.GAP_BAND[1])), ratios


def test_explain_sets_the_two_routes_side_by_side(chain):
    curves, book, keys, L = chain["curves"], C.chain_book(), C.chain_keys(), chain["factor"]
    got = monte_carlo_explain_var_es(Engine(chain["model"]), curves, chain["ir"], book, keys, L, C.CHAIN_S, level=0.9, seed=C.SEED, host=True)
    full = monte_carlo_revalue_var_es(curves, book, keys, L, C.CHAIN_S, level=0.9, seed=C.SEED, host=True)
    dg = sub_book_monte_carlo_var_es(Engine(chain["model"]), chain["ir"], book, keys, L, C.CHAIN_S, level=0.9, seed=C.SEED, host=True)
    assert got["labels"] == full["labels"] == dg["labels"]
    for key, ref in (("full_var", full["var"]), ("full_es", full["es"]), ("dg_var", dg["var"]), ("dg_es", dg["es"]),
                     ("gap_var", full["var"] - dg["var"]), ("gap_es", full["es"] - dg["es"])):
        assert np.array_equal(C.bits(got[key]), C.bits(ref)), key
    assert np.all(np.abs(got["gap_var"]) < 0.05 * np.abs(got["full_var"])), "the expansion describes these books at daily moves"
