"""Sub-books of a scenario revaluation on the CPU twins (adr_scenario_subbook_pv_host, adr_credit_scenario_subbook_pv_host,
adr_scenario_tail_host) and through ``host=True``: no GPU needed.  The device tests are tests/test_gpu_subbook_scenarios.py."""
import numpy as np
import pytest

from adrates_amd import _native
from adrates_amd.market.position.scenarios import (expected_shortfall, historical_var, revalue_credit_on_curves,
                                                   revalue_credit_on_curves_sub_books, revalue_on_curves,
                                                   revalue_on_curves_sub_books, split_sub_books, tail_measures)
from adrates_amd.utils import CurrencyTypes, CurveTypes, DayCountTypes, FrequencyTypes, InterpTypes
from adrates_amd.utils.error import LibError

from . import _credit_scenario_cases as CC
from . import _fixtures as F
from . import _scenario_cases as SC
from . import _subbook_cases as SB
from ._parity import REL_TOL

VD = SC.VD


@pytest.fixture(scope="module")
def curves():
    return SC.shocked_curves()


@pytest.fixture(scope="module")
def sized():
    """The sized book, its offsets and the twin's result on the 9 curves (computed once, never changed)."""
    times, dfs = SC.shocked_curves()
    batch, sub_off = SB.sized_book(), SB.offsets(SB.SIZES)
    out = _native.scenario_subbook_pv_host(4, times, dfs, batch, sub_off, per_trade=True)
    return batch, sub_off, out


def test_every_sub_book_equals_itself_priced_alone(curves, sized):
    times, dfs = curves
    batch, sub_off, out = sized
    parent = _native.scenario_pv_host(4, times, dfs, batch, per_trade=True)
    assert np.array_equal(out["pv"], parent["pv"])                       # per-trade rows: the parent's bits
    assert out["sub_pv"].shape == (len(SB.SIZES), dfs.shape[0])
    for b, (lo, hi) in enumerate(zip(sub_off[:-1], sub_off[1:])):
        if lo == hi:
            assert np.all(out["sub_pv"][b] == 0.0) and not np.any(np.signbit(out["sub_pv"][b]))
            continue
        alone = _native.scenario_pv_host(4, times, dfs, SB.take(batch, lo, hi))["book_pv"]
        assert np.array_equal(out["sub_pv"][b], alone), (b, lo, hi)
        assert np.array_equal(out["sub_pv"][b], SC.book_sum(out["pv"][:, lo:hi])), (b, lo, hi)


def test_oracle_parity_of_the_per_trade_rows(curves):
    times, dfs = curves
    batch = SC.books()["300 mixed OIS"]
    got = _native.scenario_subbook_pv_host(4, times, dfs, batch, SB.cuts(batch.n_trades, 7, 3), per_trade=True)
    err = SC.worst_unit_err(got["pv"], SC.oracle_pv(4, times, dfs, batch), batch)
    print(f"sub-book launch vs the C oracle: {err:.2e}")
    assert err <= REL_TOL


@pytest.mark.parametrize("scheme", SC.SCHEMES, ids=lambda s: s.name)
def test_one_sub_book_is_the_parent(curves, scheme):
    times, dfs = curves
    for name, batch in SC.books().items():
        parent = _native.scenario_pv_host(scheme.value, times, dfs, batch, per_trade=True)
        got = _native.scenario_subbook_pv_host(scheme.value, times, dfs, batch, [0, batch.n_trades], per_trade=True)
        assert np.array_equal(got["sub_pv"][0], parent["book_pv"]) and np.array_equal(got["pv"], parent["pv"]), name


def test_independence_of_threads_order_and_scenario_count(sized):
    batch, sub_off, out = sized
    times, dfs = SC.shocked_curves()
    again = _native.scenario_subbook_pv_host(4, times, dfs, batch, sub_off, per_trade=True, n_threads=3)
    assert np.array_equal(again["sub_pv"], out["sub_pv"]) and np.array_equal(again["pv"], out["pv"])
    order = np.random.default_rng(4).permutation(len(SB.SIZES))
    pbatch, poff = SB.permuted(batch, sub_off, order)
    moved = _native.scenario_subbook_pv_host(4, times, dfs, pbatch, poff)["sub_pv"]
    assert np.array_equal(moved, out["sub_pv"][order])
    wt, wide = SB.wide_curves()
    small, small_off = SB.take(batch, 0, 400), SB.offsets((0, 1, 63, 64, 0, 0, 65, 127, 80, 0))
    full = _native.scenario_subbook_pv_host(4, wt, wide, small, small_off)["sub_pv"]
    for S in SB.S_VALUES:
        assert np.array_equal(_native.scenario_subbook_pv_host(4, wt, wide[:S], small, small_off)["sub_pv"], full[:, :S]), S


def test_large_knot_grid():
    fine, rows, dz, case = CC.large_grid_call()
    assert fine.size == 856
    n = case.batch.n_trades
    sub_off = SB.cuts(n, 5, 11)
    got = _native.scenario_subbook_pv_host(4, fine, rows, case.batch, sub_off, per_trade=True)
    cgot = _native.credit_scenario_subbook_pv_host(4, fine, rows, dz, case.batch, case.z, case.bucket, case.fix_tau,
                                                   case.flt_tau, sub_off, per_trade=True)
    for b, (lo, hi) in enumerate(zip(sub_off[:-1], sub_off[1:])):
        if lo == hi:
            continue
        assert np.array_equal(got["sub_pv"][b], _native.scenario_pv_host(4, fine, rows, SB.take(case.batch, lo, hi))["book_pv"])
        assert np.array_equal(cgot["sub_pv"][b], CC.host_pv(4, fine, rows, dz, SB.take_case(case, lo, hi), False)["book_pv"])


@pytest.mark.parametrize("shape", ["joint", "shared spread row", "shared curve"])
def test_credit_sub_books_cut_across_buckets(curves, shape):
    times, dfs = curves
    G = 5
    dz = CC.spread_shocks(dfs.shape[0], G)
    if shape == "shared spread row":
        dz = dz[1:2]
    if shape == "shared curve":
        dfs = dfs[2:3]
    for scheme in SC.SCHEMES:
        for name, case in CC.cases(G).items():
            n = case.batch.n_trades
            sub_off = SB.cuts(n, 6, len(name))
            assert len({int(x) for lo, hi in zip(sub_off[:-1], sub_off[1:]) for x in case.bucket[lo:hi]}) > 1 or n < 4
            parent = CC.host_pv(scheme.value, times, dfs, dz, case)
            got = _native.credit_scenario_subbook_pv_host(scheme.value, times, dfs, dz, case.batch, case.z, case.bucket,
                                                          case.fix_tau, case.flt_tau, sub_off, per_trade=True)
            assert np.array_equal(got["pv"], parent["pv"]), name
            one = _native.credit_scenario_subbook_pv_host(scheme.value, times, dfs, dz, case.batch, case.z, case.bucket,
                                                          case.fix_tau, case.flt_tau, [0, n])
            assert np.array_equal(one["sub_pv"][0], parent["book_pv"]), name
            for b, (lo, hi) in enumerate(zip(sub_off[:-1], sub_off[1:])):
                if lo == hi:
                    assert np.all(got["sub_pv"][b] == 0.0) and not np.any(np.signbit(got["sub_pv"][b]))
                    continue
                alone = CC.host_pv(scheme.value, times, dfs, dz, SB.take_case(case, lo, hi), False)["book_pv"]
                assert np.array_equal(got["sub_pv"][b], alone), (name, b)
                assert np.array_equal(got["sub_pv"][b], SC.book_sum(got["pv"][:, lo:hi])), (name, b)


def test_offsets_that_are_refused(curves):
    times, dfs = curves
    batch = SC.lag_book(40, seed=3)
    case = CC.dress(batch, 3, 5)
    for bad, what in (([1, 20, 40], "start at 0"), ([0, 25, 20, 40], "decreases at sub-book 1"), ([0, 20, 39], "sub-book 1 ends at 39"),
                      ([0, 20, 41], "sub-book 1 ends at 41")):
        with pytest.raises(LibError, match=what):
            _native.scenario_subbook_pv_host(4, times, dfs, batch, bad)
        with pytest.raises(LibError, match=what):
            _native.credit_scenario_subbook_pv_host(4, times, dfs, None, batch, case.z, np.full(40, -1), case.fix_tau, case.flt_tau, bad)
        with pytest.raises(LibError, match=what):
            _native.scenario_subbook_plan(40, bad)
    with pytest.raises(LibError):
        _native.scenario_subbook_pv_host(4, times, dfs, batch, [0])
    plan = _native.scenario_subbook_plan(200, [0, 0, 130, 130, 200])
    assert list(plan[:5]) == [0, 0, 3, 3, 5] and list(plan[5:]) == [0, 64, 64, 128, 128, 130, 130, 194, 194, 200]
    assert _native.scenario_subbook_work(200, 4, 9) == (4 + 4) * 9


def test_tail_twin_against_numpy():
    for rows, base_col, k, nan_row in SB.tail_calls():
        var, es = _native.scenario_tail_host(rows, k, base_col)
        SB.check_tail(var, es, rows, base_col, k, nan_row)
    with pytest.raises(LibError, match="16384"):
        _native.scenario_tail_host(np.zeros((2, 16385)), 3)
    with pytest.raises(LibError, match="k must lie in 1 .. 10"):
        _native.scenario_tail_host(np.zeros((2, 11)), 11, base_col=4)
    with pytest.raises(LibError, match="base_col"):
        _native.scenario_tail_host(np.zeros((2, 11)), 1, base_col=11)


def test_tail_measures_levels_and_fallback():
    rng = np.random.default_rng(7)
    rows = rng.normal(0.0, 1e5, (4, 1001))
    for level in (0.99, 0.975, 0.5):
        var, es = tail_measures(rows, level, base_col=1000, host=True)
        pnl = rows[:, :-1] - rows[:, -1:]
        k = max(1, int(np.ceil(round((1.0 - level) * 1000, 9))))
        for b in range(4):
            assert var[b] == historical_var(pnl[b], level)
            assert abs(es[b] - expected_shortfall(pnl[b], level)) <= (k + 1) * 2.0 ** -52 * np.mean(np.abs(np.sort(pnl[b])[:k]))
    wide = rng.normal(0.0, 1.0, (2, 16385))
    wide[1, 5] = np.nan
    var, es = tail_measures(wide, 0.99, host=True)                        # too wide for the kernel: NumPy per row
    assert var[0] == historical_var(wide[0], 0.99) and es[0] == expected_shortfall(wide[0], 0.99)
    assert np.isnan(var[1]) and np.isnan(es[1])


def _mixed_list():
    rng = np.random.default_rng(12)
    swaps = [F.make_swap(VD, f"{int(m)}M", float(c), float(nn), pay=bool(p), payment_lag=int(lag))
             for m, c, nn, p, lag in zip(rng.integers(1, 361, 150), rng.uniform(0.01, 0.07, 150),
                                         np.round(rng.uniform(1e6, 5e7, 150), -5), rng.random(150) < 0.5,
                                         rng.choice([0, 0, 0, 2], 150))]
    bonds, quotes = F.random_bond_book(VD, 12, seed=2)
    frns, _ = F.random_frn_book(VD, 12, seed=3)
    trades = swaps + list(bonds) + list(frns)
    perm = rng.permutation(len(trades))
    trades = [trades[i] for i in perm]
    keys = [("desk", int(k)) for k in rng.integers(0, 5, len(trades))]
    return trades, keys


def test_python_surface_on_the_host(curves):
    times, dfs = curves
    trades, keys = _mixed_list()
    out = revalue_on_curves_sub_books(4, times, dfs, trades, keys, VD, per_trade=True, host=True)
    whole = revalue_on_curves(4, times, dfs, trades, VD, per_trade=True, host=True)
    assert np.array_equal(out["pv"], whole["pv"])                          # the caller's order
    firsts = []
    for k in keys:
        if k not in firsts:
            firsts.append(k)
    assert out["labels"] == firsts and out["sub_pv"].shape == (len(firsts), dfs.shape[0])
    for b, lab in enumerate(out["labels"]):
        mine = [t for t, k in zip(trades, keys) if k == lab]
        assert np.array_equal(out["sub_pv"][b], revalue_on_curves(4, times, dfs, mine, VD, host=True)["book_pv"]), lab
    # credit: sub-books that cut across the credit buckets
    spreads = [0.0 if type(t).__name__ == "OIS" else 0.004 + 0.0001 * (i % 7) for i, t in enumerate(trades)]
    buckets = [None if type(t).__name__ == "OIS" else ("AA", "BBB", None)[i % 3] for i, t in enumerate(trades)]
    shocks = np.array(([[0.0, 0.0], [0.001, -0.002], [0.0005, 0.003]] * 3)[:dfs.shape[0]])
    cout = revalue_credit_on_curves_sub_books(4, times, dfs, shocks, trades, spreads, buckets, keys, VD, per_trade=True, host=True)
    cwhole = revalue_credit_on_curves(4, times, dfs, shocks, trades, spreads, buckets, VD, per_trade=True, host=True)
    assert np.array_equal(cout["pv"], cwhole["pv"]) and cout["labels"] == firsts and cout["buckets"] == cwhole["labels"]
    for b, lab in enumerate(cout["labels"]):
        idx = [i for i, k in enumerate(keys) if k == lab]
        sub_buckets = [buckets[i] for i in idx]
        alone = revalue_credit_on_curves(4, times, dfs, _columns(shocks, cwhole["labels"], sub_buckets), [trades[i] for i in idx],
                                         [spreads[i] for i in idx], sub_buckets, VD, host=True)
        assert np.array_equal(cout["sub_pv"][b], alone["book_pv"]), lab


def _columns(shocks, labels, sub_buckets):
    """The shock columns of a sub-list's buckets, in ITS order of first appearance."""
    seen = []
    for lab in sub_buckets:
        if lab is not None and lab not in seen:
            seen.append(lab)
    return shocks[:, [labels.index(lab) for lab in seen]] if seen else None


def test_python_refusals(curves):
    times, dfs = curves
    trades, keys = _mixed_list()
    with pytest.raises(LibError, match="keys needs one entry per trade"):
        revalue_on_curves_sub_books(4, times, dfs, trades, keys[:-1], VD, host=True)
    batch = SC.lag_book(30, seed=3)
    with pytest.raises(LibError, match="sub-book 'a'.*reappears at trade 20"):
        revalue_on_curves_sub_books(4, times, dfs, batch, ["a"] * 10 + ["b"] * 10 + ["a"] * 10, VD, host=True)
    ok = revalue_on_curves_sub_books(4, times, dfs, batch, ["a"] * 10 + ["b"] * 20, VD, host=True)
    assert ok["labels"] == ["a", "b"]
    assert np.array_equal(ok["sub_pv"][1], _native.scenario_pv_host(4, times, dfs, SB.take(batch, 10, 30))["book_pv"])
    from adrates_amd.trades.rates.xccy_basis_swap import XccyBasisSwap
    xccy = XccyBasisSwap(effective_dt=VD, term_dt_or_tenor="7Y", domestic_notional=7_900_000, foreign_notional=10_000_000,
                         domestic_spread=0.0, foreign_spread=0.0040, domestic_freq_type=FrequencyTypes.ANNUAL,
                         foreign_freq_type=FrequencyTypes.SEMI_ANNUAL, domestic_dc_type=DayCountTypes.ACT_365F,
                         foreign_dc_type=DayCountTypes.ACT_360, domestic_floating_index=CurveTypes.GBP_OIS_SONIA,
                         foreign_floating_index=CurveTypes.USD_OIS_SOFR, domestic_currency=CurrencyTypes.GBP,
                         foreign_currency=CurrencyTypes.USD)
    with pytest.raises(LibError, match="cross-currency"):
        revalue_on_curves_sub_books(4, times, dfs, [trades[0], xccy], ["a", "b"], VD, host=True)
