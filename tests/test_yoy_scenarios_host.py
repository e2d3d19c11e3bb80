"""Inflation scenario revaluation without a GPU: the host twin of csrc/yoy_scenario_pv.hip (adr_yoy_scenario_pv_host: the
kernel's per-date and per-coupon code compiled for the CPU) and the Python layers above it.

  1. the twin against an evaluation that shares no code with it - the C oracle's fixed-flow PV plus the 60-digit MpYoY
     per scenario - on the WHOLE raw case table of tests/_yoy_cases.py with a fixed leg on every second swap, under the
     case's own curves and seven jointly shocked pairs, to REL_TOL per unit notional, every swap on its own notional;
  2. the twin against the shipped per-scenario route (adr_yoy_risk_host amounts -> compile_yoy_swaps ->
     adr_scenario_pv_host) on real swaps;
  3. broadcasting, 4. independence of S and the documented order of the book sum, bit for bit;
  5. the refusals of the host-array entry, empty legs, one swap, a book wholly in the past;
  6. the Python surface: revalue_yoy_on_curves against the torch restatement of the reference's engine on models rebuilt
     per scenario, shocked_breakevens, compile_yoy_fixed_legs, historical_var on the P&L vector.

Observed on the CPU: check 1 at most 2.8e-15 (64 monthly coupons beyond the last pillar), no case left out; check 2
1.1e-15; check 6 6.7e-16."""
import numpy as np
import pytest

from adrates_amd import _native
from adrates_amd.market.curves.curve_tables import build_engine_curve
from adrates_amd.market.position.inflation_engine import inflation_inputs
from adrates_amd.market.position.scenarios import (expected_shortfall, historical_var, revalue_yoy_on_curves,
                                                   shocked_breakevens)
from adrates_amd.trades.compiler import compile_yoy_coupons, compile_yoy_fixed_legs, compile_yoy_swaps
from adrates_amd.trades.market_data import INFL_PX, GBP_PX, gbp_model, inflation_curve, random_yoy_book, yoy_model
from adrates_amd.utils import InterpTypes, LibError
from adrates_amd.utils.helpers import to_tenor

from . import _scenario_cases as SC
from . import _yoy_cases as YC
from . import _yoy_scenario_cases as YS
from ._inflation_oracle import yoy_analytics
from ._parity import REL_TOL, unit_notional_err

VD = SC.VD


def _host(case, times, dfs, T, b, fixed="case", book="case", **kw):
    return _native.yoy_scenario_pv_host(case.disc[0], times, dfs, case.infl[0], T, b,
                                        YS.fixed_legs(case) if isinstance(fixed, str) else fixed,
                                        case.book if isinstance(book, str) else book, per_trade=True, **kw)


# ------------------------------------------------------------------------------------ 1. the independent reference
@pytest.mark.parametrize("case", YS.cases(), ids=repr)
def test_host_twin_against_independent_reference(case):
    """No case and no swap is left out of the comparison: the share left out is 0."""
    times, dfs, T, b = YS.scenario_pairs(case)
    assert dfs.shape[0] == b.shape[0] >= 8
    got = _host(case, times, dfs, T, b)
    ref = YS.reference(case)
    assert got["pv"].shape == ref.shape == (dfs.shape[0], len(case.rows))
    e, s, name = YS.worst_error(case, got["pv"], ref)
    print(f"{case}: host twin against C oracle + MpYoY {e:.2e} (scenario {s}, {name})")
    assert e <= REL_TOL, (name, s, e)
    assert np.all(np.isfinite(got["pv"])) and np.count_nonzero(got["pv"][0]) >= np.count_nonzero(ref[0])


# ------------------------------------------------------------------------------------------ 2. the shipped route
def _readme_pairs(curve_b):
    times, dfs = SC.shocked_curves()
    return times, dfs, YS.breakeven_rows(curve_b)[[1, 2, 3, 4, 5, 6, 7, 0]]


@pytest.mark.parametrize("dm", SC.SCHEMES, ids=lambda s: s.name)
@pytest.mark.parametrize("im", [InterpTypes.LINEAR_ZERO_RATES, InterpTypes.FLAT_FWD_RATES], ids=lambda s: s.name)
def test_consistent_with_the_per_scenario_route(dm, im):
    from adrates_amd.utils.global_types import InflationInterpTypes
    infl = inflation_curve(VD, InflationInterpTypes.LINEAR if im == InterpTypes.LINEAR_ZERO_RATES else InflationInterpTypes.FLAT)
    assert infl._interp_type == im
    _, T, b0 = inflation_inputs(infl)
    swaps = random_yoy_book(VD, 40, seed=11)
    notional = np.array([s._notional for s in swaps])
    times, dfs, b = _readme_pairs(b0)
    book, fixed = compile_yoy_coupons(swaps, VD), compile_yoy_fixed_legs(swaps, VD)
    got = _native.yoy_scenario_pv_host(dm.value, times, dfs, im.value, T, b, fixed, book, per_trade=True)["pv"]
    worst = 0.0
    for s in range(dfs.shape[0]):
        amounts = _native.yoy_risk_host((dm.value, times, dfs[s]), (im.value, T, b[s]), book, per_swap=False)["amount"]
        route = _native.scenario_pv_host(dm.value, times, dfs[s], compile_yoy_swaps(swaps, VD, amounts), per_trade=True)["pv"][0]
        worst = max(worst, unit_notional_err(got[s], route, notional))
    print(f"{dm.name} / {im.name}: one call against the per-scenario route {worst:.2e}")
    assert worst <= 1e-10


# ------------------------------------------------------------------------------------- 3. and 4. bits and orders
GEO = YC.geometry_case(20, 130, YC.LZ, YC.FF, shift=1)          # three chunks of ADR_SCENARIO_CHUNK swaps


def test_a_shared_row_equals_the_row_repeated():
    for case in (YC.knot_cases()[0], YC.knot_cases()[6], GEO):
        times, dfs, T, b = YS.scenario_pairs(case)
        S = dfs.shape[0]
        for k in (0, 3):
            both = _host(case, times, np.repeat(dfs[k:k + 1], S, axis=0), T, b)
            one = _host(case, times, dfs[k], T, b)
            assert np.array_equal(both["pv"], one["pv"]) and np.array_equal(both["book_pv"], one["book_pv"])
            both = _host(case, times, dfs, T, np.repeat(b[k:k + 1], S, axis=0))
            one = _host(case, times, dfs, T, b[k])
            assert np.array_equal(both["pv"], one["pv"]) and np.array_equal(both["book_pv"], one["book_pv"])
        one = _host(case, times, dfs[2], T, b[5])                # S = 1 from two shared rows: the pair (2, 5)
        mixed = b.copy()
        mixed[2] = b[5]
        assert one["pv"].shape == (1, len(case.rows)) and np.array_equal(one["pv"][0], _host(case, times, dfs, T, mixed)["pv"][2])


def test_scenarios_are_independent_and_the_book_sum_keeps_its_order():
    for case in (YC.knot_cases()[1], GEO):
        times, dfs, T, b = YS.scenario_pairs(case)
        full = _host(case, times, dfs, T, b)
        assert np.array_equal(full["book_pv"], SC.book_sum(full["pv"]))
        for s in range(dfs.shape[0]):
            alone = _host(case, times, dfs[s], T, b[s])
            assert np.array_equal(alone["pv"][0], full["pv"][s]) and alone["book_pv"][0] == full["book_pv"][s]
        threads = _host(case, times, dfs, T, b, n_threads=3)
        assert np.array_equal(threads["pv"], full["pv"]) and np.array_equal(threads["book_pv"], full["book_pv"])
        fixed = YS.fixed_legs(case)
        for i in (0, 1, 3, len(case.rows) - 1):                  # a swap alone is the swap inside the book
            lo, hi = int(fixed[0][i]), int(fixed[0][i + 1])
            solo = _host(case, times, dfs, T, b, fixed=(np.array([0, hi - lo]), fixed[1][lo:hi], fixed[2][lo:hi]),
                         book=YC.one_swap(case.book, i))
            assert np.array_equal(solo["pv"][:, 0], full["pv"][:, i]) and np.array_equal(solo["book_pv"], full["pv"][:, i])


def test_no_exponential_where_none_is_needed():
    """ts == te under LINEAR_FWD_RATES discounting: amount = scale * spread exactly, D(tp) linear in the knots."""
    case = YC.lookup_cases()[2]
    assert case.disc[0] == YC.LF
    times, dfs, T, b = YS.scenario_pairs(case)
    got = _host(case, times, dfs, T, b, fixed=None)["pv"]
    from oracle import cavour_oracle as O
    tp = case.book["tp"]
    for s in range(dfs.shape[0]):
        d = np.asarray(O.simple_interpolate(tp, times, dfs[s], YC.LF), dtype=np.float64).reshape(-1)
        assert np.max(np.abs(got[s] - np.where(tp > 0.0, d, 0.0))) <= 4 * np.finfo(float).eps
    assert np.array_equal(got, _host(case, times, dfs, T, b[::-1].copy(), fixed=None)["pv"])    # no inflation curve in it


# ------------------------------------------------------------------------------------------------ 5. refusals
def _small():
    case = YC.knot_cases()[0]
    times, dfs, T, b = YS.scenario_pairs(case)
    book = YC.raw_book([[(1.0, 0.0, 1.0, 1e6, 0.0), (2.0, 1.0, 2.0, 1e6, 0.0)], [(3.0, 2.0, 3.0, 1e6, 0.0)], []])
    fixed = (np.array([0, 2, 2, 3]), np.array([1.0, 2.0, 0.7]), np.array([-3e4, -1.03e6, 5.0]))
    return case, times, dfs, T, b, fixed, book


def test_host_array_entry_refusals():
    case, times, dfs, T, b, fixed, book = _small()
    call = lambda **kw: _host(case, kw.pop("times", times), kw.pop("dfs", dfs), kw.pop("T", T), kw.pop("b", b),
                              fixed=kw.pop("fixed", fixed), book=kw.pop("book", book))
    ok = call()
    assert ok["pv"].shape == (8, 3) and ok["pv"][0, 2] != 0.0
    with pytest.raises(LibError, match="offsets must be non-decreasing"):
        call(book=dict(book, cpn_off=np.array([0, 3, 2, 3])))
    with pytest.raises(LibError, match="cpn_off must run from 0 to m"):
        call(book=dict(book, cpn_off=np.array([1, 2, 3, 3])))
    with pytest.raises(LibError, match="offsets must be non-decreasing"):
        call(fixed=(np.array([0, 3, 2, 3]), fixed[1], fixed[2]))
    with pytest.raises(LibError, match="fix_off must run from 0"):
        call(fixed=(np.array([0, 2, 2, 2]), fixed[1], fixed[2]))
    for field in _native.YOY_FIELDS:
        v = book[field].copy()
        v[1] = np.nan
        with pytest.raises(LibError, match="coupon fields must be finite"):
            call(book=dict(book, **{field: v}))
    for k in (1, 2):
        v = [fixed[1].copy(), fixed[2].copy()]
        v[k - 1][0] = np.nan
        with pytest.raises(LibError, match="fixed-flow times and amounts must be finite"):
            call(fixed=(fixed[0], v[0], v[1]))
    for bad in (-1.0, -1.5, np.nan, np.inf):
        rows = b.copy()
        rows[5, 2] = bad
        with pytest.raises(LibError, match=r"breakeven rates must be finite and > -1 \(row 5, pillar 2\)"):
            call(b=rows)
    for bad in (0.0, -0.5, np.nan, np.inf):
        rows = dfs.copy()
        rows[3, 4] = bad
        with pytest.raises(LibError, match=r"discount factors must be positive and finite \(row 3, knot 4\)"):
            call(dfs=rows)
    for bad_T in ([1.0, 1.0, 2.0, 3.0, 4.0], [2.0, 1.0, 3.0, 4.0, 5.0], [0.0, 1.0, 2.0, 3.0, 4.0], [1.0, 2.0, 3.0, 4.0, np.nan]):
        with pytest.raises(LibError, match="pillar times must be increasing from > 0"):
            call(T=np.array(bad_T))
    with pytest.raises(LibError, match="knot times must be finite and non-decreasing"):
        call(times=times[::-1].copy())
    with pytest.raises(LibError, match="knot times must be finite and non-decreasing"):
        call(times=np.where(np.arange(times.size) == 3, np.nan, times))
    with pytest.raises(LibError, match="one shared row or one row per scenario"):
        call(dfs=dfs[:3])
    with pytest.raises(LibError, match="one shared row or one row per scenario"):
        call(b=b[:2])
    lib, p, ip = _native.load(), _native._ptr, _native._i64p
    off, cpn = _native.yoy_pack(book)
    fo = np.ascontiguousarray(fixed[0], dtype=np.int64)
    out = np.empty(8)

    def raw(S_disc=8, S_infl=8, S=8, im=4, dm=4, K=times.size, P=T.size):
        return lib.adr_yoy_scenario_pv_host(dm, K, p(times), S_disc, p(dfs), im, P, p(T), S_infl, p(b), S, 3, 3, p(fo, ip),
                                            p(fixed[1]), p(fixed[2]), 3, p(off, ip), p(cpn), None, p(out), 0)
    assert raw() == 0
    assert raw(S_disc=4) < 0 and b"S_disc and S_infl must each be 1" in lib.adr_last_error()
    assert raw(S_infl=2) < 0 and raw(S=0) < 0 and raw(K=1) < 0 and raw(K=4097) < 0 and raw(P=0) < 0 and raw(P=65) < 0
    assert raw(im=2) == raw(im=3) == raw(dm=3) and raw(im=2) < 0 and b"inflation scheme" in lib.adr_last_error()


def test_empty_legs_one_swap_and_a_book_in_the_past():
    case, times, dfs, T, b, fixed, book = _small()
    full = _host(case, times, dfs, T, b, fixed=fixed, book=book)["pv"]
    only_cpn = _host(case, times, dfs, T, b, fixed=None, book=book)
    only_fix = _host(case, times, dfs, T, b, fixed=fixed, book=None)
    assert np.array_equal(only_cpn["pv"][:, 2], np.zeros(8)) and np.array_equal(only_fix["pv"][:, 1], np.zeros(8))
    assert np.array_equal(only_fix["pv"] + only_cpn["pv"], full)         # pv = fixed sum + YoY sum, each from 0.0
    holder = YC.Case("fixed legs only", case.disc, case.infl, [("a", 1e6, []), ("b", 1e6, []), ("c", 1.0, [])])
    oracle = SC.oracle_pv(case.disc[0], times, dfs, YS.fixed_batch(holder, fixed))
    assert max(unit_notional_err(g, r, holder.notional) for g, r in zip(only_fix["pv"], oracle)) <= REL_TOL
    with pytest.raises(LibError, match="neither fixed legs nor YoY coupons"):
        _host(case, times, dfs, T, b, fixed=None, book=None)
    one = _host(case, times, dfs, T, b, fixed=(np.array([0, 2]), fixed[1][:2], fixed[2][:2]), book=YC.one_swap(book, 0))
    assert one["pv"].shape == (8, 1) and np.array_equal(one["pv"][:, 0], full[:, 0]) and np.array_equal(one["book_pv"], full[:, 0])
    past = YC.raw_book([[(-2.0 + k, -3.0 + k, -2.0 + k, 1e6, 0.01) for k in range(3)], [(0.0, -1.0, 0.0, -1e6, 0.0)]])
    gone = _host(case, times, dfs, T, b, fixed=(np.array([0, 2, 3]), np.array([-1.0, 0.0, -0.5]), np.array([1e4, 1e6, 7.0])), book=past)
    assert not gone["pv"].any() and not gone["book_pv"].any()


# ------------------------------------------------------------------------------------------- 6. the Python surface
def test_shocked_breakevens_and_fixed_leg_compiler():
    curve = inflation_curve(VD)
    _, T, b0 = inflation_inputs(curve)
    assert np.array_equal(shocked_breakevens(curve, 0.0), b0)
    assert np.allclose(shocked_breakevens(curve, 25.0) - b0, 25e-4, rtol=0, atol=1e-17)
    tenors = to_tenor(list(T))
    assert tenors[4] == "5Y" and len(set(tenors)) == len(tenors)   # the labels are to_tenor's, quirks included
    got = shocked_breakevens(curve, {"5Y": -10.0, tenors[-1]: 200.0})
    want = b0.copy()
    want[4] += -10.0 * 1e-4
    want[-1] += 200.0 * 1e-4
    assert np.array_equal(got, want)
    with pytest.raises(LibError, match="no pillar named"):
        shocked_breakevens(curve, {"11Y": 1.0})
    swaps = random_yoy_book(VD, 25, seed=5)
    book = compile_yoy_coupons(swaps, VD)
    off, tp, pay = compile_yoy_fixed_legs(swaps, VD)
    amounts = np.arange(1.0, book["tp"].size + 1.0) * 1e3       # any amounts: the merge is about times and signs
    batch = compile_yoy_swaps(swaps, VD, amounts)
    assert off[-1] + book["cpn_off"][-1] == batch.fix_off[-1]
    for i in range(len(swaps)):
        f, c = slice(off[i], off[i + 1]), slice(book["cpn_off"][i], book["cpn_off"][i + 1])
        flows = sorted(list(zip(tp[f], pay[f])) + list(zip(book["tp"][c], amounts[c])), key=lambda x: x[0])
        g = slice(batch.fix_off[i], batch.fix_off[i + 1])
        assert [t for t, _ in flows] == batch.fix_tp[g].tolist() and [a for _, a in flows] == batch.fix_pay[g].tolist()


def test_revalue_on_real_objects_against_rebuilt_models():
    swaps = random_yoy_book(VD, 6, seed=3)
    notional = np.array([s._notional for s in swaps])
    base = yoy_model(VD)
    infl = base.curves.GBP_RPI_INFLATION
    im, T, b0 = inflation_inputs(infl)
    disc_moves = [0.0, 0.5, -2.0, 0.25]                          # percent, on every OIS quote
    infl_moves = [0.0, -50.0, 200.0, {"10Y": 100.0, "2Y": -25.0}]   # basis points
    tenors = to_tenor(list(T))
    rows, b, ref = [], [], []
    for dq, ib in zip(disc_moves, infl_moves):
        m = gbp_model(VD, px=[q + dq for q in GBP_PX])
        px = [q + 0.01 * (ib.get(t, 0.0) if isinstance(ib, dict) else ib) for q, t in zip(INFL_PX, tenors)]
        shocked = inflation_curve(VD, px=px)
        disc = m.curves.GBP_OIS_SONIA
        built = build_engine_curve(disc.swap_rates, disc.swap_times, disc.year_fracs, with_hessian=False)
        rows.append(built.dfs)
        b.append(shocked_breakevens(infl, ib))
        assert np.max(np.abs(b[-1] - inflation_inputs(shocked)[2])) <= 1e-15
        ref.append([yoy_analytics(s, disc, shocked, want_gamma=False)["value"] for s in swaps])
    times, rows, b, ref = built.times, np.stack(rows), np.stack(b), np.array(ref)
    got = revalue_yoy_on_curves(InterpTypes.LINEAR_ZERO_RATES, times, rows, im, T, b, swaps, VD, per_trade=True, host=True)
    err = max(unit_notional_err(g, r, notional) for g, r in zip(got["pv"], ref))
    print(f"revalue_yoy_on_curves(host=True) against the engine restatement on rebuilt models: {err:.2e}")
    assert got["pv"].shape == (4, 6) and err <= REL_TOL
    assert np.array_equal(got["book_pv"], SC.book_sum(got["pv"]))
    only_infl = revalue_yoy_on_curves(4, times, rows[0], im, T, b, swaps, VD, per_trade=True, host=True)
    assert np.array_equal(only_infl["pv"][0], got["pv"][0]) and not np.array_equal(only_infl["pv"][2], got["pv"][2])
    pnl = only_infl["book_pv"][1:] - only_infl["book_pv"][0]
    var = historical_var(pnl, 0.5)
    assert var == -np.sort(pnl)[1] and expected_shortfall(pnl, 0.5) == -np.mean(np.sort(pnl)[:2])
    with pytest.raises(LibError, match="Invalid interpolation scheme"):
        revalue_yoy_on_curves(4, times, rows, InterpTypes.LINEAR_FWD_RATES, T, b, swaps, VD, host=True)
    with pytest.raises(LibError, match="no swaps"):
        revalue_yoy_on_curves(4, times, rows, im, T, b, [], VD, host=True)
