"""Scenario revaluation on the CPU twin (adr_scenario_pv_host; no GPU): the C oracle scenario by scenario, the lookup
rule against the oracle's simple_interpolate, the documented order of the book sum, and the public functions
(`revalue_on_curves(host=True)`, `historical_var`, `expected_shortfall`) with their refusals."""
import numpy as np
import pytest

from adrates_amd import _native
from adrates_amd.market.position.scenarios import expected_shortfall, historical_var, revalue_on_curves
from adrates_amd.trades.compiler import compile_bonds, compile_frns, compile_ois
from adrates_amd.trades.credit.frn import FRN
from adrates_amd.utils import CurrencyTypes, CurveTypes, DayCountTypes, FrequencyTypes, InterpTypes
from adrates_amd.utils.error import LibError
from oracle import cavour_oracle as O

from . import _fixtures as F
from . import _scenario_cases as SC
from ._parity import REL_TOL

VD = SC.VD


@pytest.fixture(scope="module")
def curves():
    return SC.shocked_curves()


@pytest.fixture(scope="module")
def books():
    return SC.books()


@pytest.mark.parametrize("scheme", SC.SCHEMES, ids=lambda s: s.name)
def test_host_twin_matches_c_oracle(native_lib, curves, books, scheme):
    """Observed maximum over all books, schemes and scenarios: 1.8e-15."""
    times, dfs = curves
    for name, batch in books.items():
        got = _native.scenario_pv_host(scheme.value, times, dfs, batch, per_trade=True)
        assert got["pv"].shape == (dfs.shape[0], batch.n_trades) and got["book_pv"].shape == (dfs.shape[0],)
        err = SC.worst_unit_err(got["pv"], SC.oracle_pv(scheme.value, times, dfs, batch), batch)
        print(f"{scheme.name}, {name}: {err:.2e}")
        assert err <= REL_TOL, (name, err)
        assert np.any(got["pv"][0] != got["pv"][4])           # the scenarios do move the PVs


@pytest.mark.parametrize("scheme", SC.SCHEMES, ids=lambda s: s.name)
@pytest.mark.parametrize("late", [False, True], ids=["t0-knot", "first-knot-late"])
def test_lookup_rule_matches_simple_interpolate(native_lib, scheme, late):
    """On a knot, within 1e-11 of one, 1e-9 beside one, before the first knot, beyond the last, on a duplicated knot."""
    times = SC.LOOKUP_TIMES_LATE if late else SC.LOOKUP_TIMES
    dfs = SC.lookup_curves(times)
    dates = SC.LOOKUP_DATES
    df = lambda t, s: np.asarray(O.simple_interpolate(t, times, dfs[s], scheme.value), dtype=np.float64).reshape(-1)
    got = _native.scenario_pv_host(scheme.value, times, dfs, SC.one_flow_book(dates), per_trade=True)["pv"]
    for s in range(dfs.shape[0]):
        assert np.max(np.abs(got[s] - df(dates, s))) <= REL_TOL, (s, got[s], df(dates, s))
    assert np.array_equal(got[:, 3], dfs[:, 2]) or scheme.value != 2      # t = 1.0: the first of the equal knots
    # float coupons whose three dates come from the same list (rotated), payment lag included
    ts, te, tp = dates, np.roll(dates, 3), np.roll(dates, 5)
    got = _native.scenario_pv_host(scheme.value, times, dfs, SC.one_coupon_book(ts, te, tp), per_trade=True)["pv"]
    for s in range(dfs.shape[0]):
        ref = ((df(ts, s) / df(te, s) - 1.0) + 0.01) * df(tp, s)
        assert np.max(np.abs(got[s] - ref) / np.maximum(1.0, np.abs(ref))) <= REL_TOL, s


def test_book_sum_order_single_scenario_rows_and_threads(native_lib, curves, books):
    times, dfs = curves
    batch = books["300 mixed OIS"]
    rows = np.vstack([dfs] * 9)[:65]                          # 65 scenarios: one past a group of 64
    full = _native.scenario_pv_host(4, times, rows, batch, per_trade=True, n_threads=3)
    assert np.array_equal(full["book_pv"], SC.book_sum(full["pv"]))
    for s in (0, 7, 63, 64):
        one = _native.scenario_pv_host(4, times, rows[s], batch, per_trade=True)
        assert np.array_equal(one["pv"][0], full["pv"][s]) and one["book_pv"][0] == full["book_pv"][s]
    for threads in (1, 2, 16):
        again = _native.scenario_pv_host(4, times, rows, batch, per_trade=True, n_threads=threads)
        assert np.array_equal(again["pv"], full["pv"]) and np.array_equal(again["book_pv"], full["book_pv"])
    book_only = _native.scenario_pv_host(4, times, rows, batch)
    assert "pv" not in book_only and np.array_equal(book_only["book_pv"], full["book_pv"])


def _objects():
    bonds, _ = F.random_bond_book(VD, 4, seed=11)
    frns, _ = F.random_frn_book(VD, 4, seed=12)
    swaps = [F.make_swap(VD, "10Y", 0.045, 1e7), F.make_swap(VD, "87M", 0.04, 1e7, pay=False),
             F.make_swap(VD, "3Y", 0.04, 1e6, payment_lag=2, spread=0.001)]
    return swaps, bonds, frns


def test_revalue_on_curves_mixed_list_is_one_batch(native_lib, curves):
    times, dfs = curves
    swaps, bonds, frns = _objects()
    mixed = [swaps[0], bonds[0], frns[0], swaps[1], frns[1], bonds[1], swaps[2], bonds[2], frns[2], frns[3], bonds[3]]
    out = revalue_on_curves(InterpTypes.LINEAR_ZERO_RATES, times, dfs, mixed, VD, per_trade=True, host=True)
    assert out["pv"].shape == (dfs.shape[0], len(mixed))
    for j, t in enumerate(mixed):                             # every column is the trade priced alone, in the list's order
        alone = revalue_on_curves(4, times, dfs, [t], VD, per_trade=True, host=True)
        assert np.array_equal(alone["pv"][:, 0], out["pv"][:, j]), j
    # against the oracle, kind by kind (the FRN compiler's curve-independent amounts added)
    frn_batch, const = compile_frns(frns, VD)
    for objs, batch, add in ((swaps, compile_ois(swaps, VD), 0.0), (bonds, compile_bonds(bonds, VD), 0.0),
                             (frns, frn_batch, const)):
        got = revalue_on_curves(4, times, dfs, objs, VD, per_trade=True, host=True)["pv"]
        assert SC.worst_unit_err(got, SC.oracle_pv(4, times, dfs, batch) + add, batch) <= REL_TOL
    assert np.allclose(out["book_pv"], out["pv"].sum(axis=1), rtol=1e-13, atol=0)
    # a compiled batch goes through as it is; one curve may be given as a vector
    one = revalue_on_curves(4, times, dfs[2], compile_ois(swaps, VD), VD, host=True)
    assert one["book_pv"].shape == (1,) and "pv" not in one


def test_revalue_refusals(native_lib, curves):
    times, dfs = curves
    swaps, bonds, frns = _objects()
    host = dict(value_dt=VD, host=True)
    dual = FRN(VD, "2Y", 0.001, FrequencyTypes.QUARTERLY, DayCountTypes.ACT_360, CurrencyTypes.GBP, CurveTypes.USD_OIS_SOFR)
    with pytest.raises(LibError, match="trade 1 is a dual-curve FRN"):
        revalue_on_curves(4, times, dfs, [swaps[0], dual], **host)
    from adrates_amd.trades.rates.xccy_basis_swap import XccyBasisSwap
    xccy = XccyBasisSwap(effective_dt=VD, term_dt_or_tenor="7Y", domestic_notional=7_900_000, foreign_notional=10_000_000,
                         domestic_spread=0.0, foreign_spread=0.0040, domestic_freq_type=FrequencyTypes.ANNUAL,
                         foreign_freq_type=FrequencyTypes.SEMI_ANNUAL, domestic_dc_type=DayCountTypes.ACT_365F,
                         foreign_dc_type=DayCountTypes.ACT_360, domestic_floating_index=CurveTypes.GBP_OIS_SONIA,
                         foreign_floating_index=CurveTypes.USD_OIS_SOFR, domestic_currency=CurrencyTypes.GBP,
                         foreign_currency=CurrencyTypes.USD)
    with pytest.raises(LibError, match="trade 2 .*cross-currency"):
        revalue_on_curves(4, times, dfs, [swaps[0], bonds[0], xccy], **host)
    usd = F.make_swap(VD, "5Y", 0.04, 1e6, index=CurveTypes.USD_OIS_SOFR, ccy=CurrencyTypes.USD)
    with pytest.raises(LibError, match="trade 0 .*USD.* not on the grid's curve GBP_OIS_SONIA"):
        revalue_on_curves(4, times, dfs, [usd], **host)
    with pytest.raises(LibError, match="dfs must have shape"):
        revalue_on_curves(4, times, dfs[:, :-1], swaps, **host)
    bad = dfs.copy()
    bad[3, 17] = 0.0
    with pytest.raises(LibError, match="positive and finite .scenario 3, knot 17"):
        revalue_on_curves(4, times, bad, swaps, **host)
    with pytest.raises(LibError, match="Invalid interpolation scheme"):
        revalue_on_curves(3, times, dfs, swaps, **host)
    with pytest.raises(LibError):
        revalue_on_curves(4, times, dfs, [], **host)
    with pytest.raises(LibError, match="non-decreasing"):
        revalue_on_curves(4, times[::-1], dfs, swaps, **host)


def test_var_and_expected_shortfall_on_a_hand_made_vector():
    pnl = np.array([5.0, -12.0, 3.0, -1.0, 0.5, -30.0, 8.0, -7.0, 2.0, 1.0, -4.0, 6.0, -2.0, 9.0, 4.0, -3.0, 7.0, -9.0, 10.0, -20.0])
    # 20 scenarios: ceil(0.05 * 20) = 1, ceil(0.10 * 20) = 2, ceil(0.25 * 20) = 5, ceil(0.01 * 20) = 1
    assert historical_var(pnl, 0.95) == 30.0 and expected_shortfall(pnl, 0.95) == 30.0
    assert historical_var(pnl, 0.90) == 20.0 and expected_shortfall(pnl, 0.90) == 25.0
    assert historical_var(pnl, 0.75) == 7.0 and expected_shortfall(pnl, 0.75) == (30 + 20 + 12 + 9 + 7) / 5
    assert historical_var(pnl, 0.99) == 30.0
    assert historical_var(-pnl, 0.95) == 10.0                  # a book that only gains has a negative VaR
    assert historical_var(np.abs(pnl), 0.95) == -0.5
    with pytest.raises(ValueError):
        historical_var(pnl, 1.0)
    with pytest.raises(ValueError):
        expected_shortfall([], 0.99)
