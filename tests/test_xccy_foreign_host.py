"""The cases of the two-curve foreign-leg tests (tests/_xccy_foreign_cases.py) and their reference
(tests/_xccy_foreign_reference.py) checked without a GPU, before tests/test_gpu_xccy_foreign.py holds the kernel to them:
  one curve twice   with one curve passed as both, delta_foreign + delta_basis and pv are `_price_reference.per_trade_reference`'s
                    delta and pv of the same batch, compared as exact rationals.  Both references round every mpmath operation
                    at 60 digits and order them differently (g / d of a sum against the sum of two g / d; c D(ts) D(tp) / D(te)
                    against (c D(ts) / D(te)) D(tp)), so the rationals part at the 60th digit: the difference is held to 1e-50 of
                    the gross, ten digits above that rounding and 34 below float64's.  Gross agrees entry by entry, to the same
                    1e-50, for every trade whose accruing coupons all have te != tp; a weighted coupon with te == tp is the plain
                    terms c D(ts) - c D(tp) there and the ratio over two tables here, whose gross is no smaller
  derivatives       g_f and g_x of one coupon against `mpmath.diff` of c D_f(ts) / D_f(te) D_x(tp) in the knots' log discount
                    factors of each table, at 120 digits, to 30 significant digits, under the five scheme pairs - the split
                    between the two ladders does not depend on the formulas having been typed correctly
  PV                the reference's pv is `_xccy_scenario_reference.reference`'s value on (times, dfs) with one row
  routing           `route_host` under mask 3 per trade puts every leg of every case on `lite_lag`, in `units_of` units: the
                    entry accepts the book; the 391-coupon leg and the plain unlagged leg do not route there
  segments          the counts books have five and three distinct row counts (the `kLiteSegments` and the three-segment
                    instantiation), every other book one
  LDS               `xc_lds_bytes` restates `lite_xc_kernel_lds_bytes`: every priced pair is within 160 KiB, and the hand-made
                    pairs sit just inside and just beyond it
  bounds            k reads only the inputs and is finite
"""
from fractions import Fraction

import numpy as np
import pytest
from mpmath import mp, mpf

from . import _ladder_reference as R
from . import _price_edge_cases as PE
from . import _price_lag_cases as PL
from . import _price_reference as PR
from . import _xccy_foreign_cases as XC
from . import _xccy_foreign_reference as XR
from . import _xccy_scenario_cases as XS
from . import _xccy_scenario_reference as XSR

CASES = XC.cases()
IDS = [c.id for c in CASES]
SAME = [c for c in CASES if c.name.startswith("one curve as both")]
TINY = Fraction(1, 10 ** 50)


def test_the_case_list():
    assert len(CASES) == 19 and len(SAME) == 2
    pairs = {(c.f_interp.value, c.x_interp.value) for c in CASES}
    assert set(XS.PAIRS) <= pairs and not pairs & set(XS.UNSUPPORTED)
    assert any(c.x_host.jac.shape[1] % 2 == 1 for c in CASES) and any(c.f_host.jac.shape[1] % 2 == 1 for c in CASES)
    assert any(c.f_host.jac.shape[1] != c.x_host.jac.shape[1] and c.f_host.times.size != c.x_host.times.size for c in CASES)
    for c in CASES:
        assert np.all(PE.lagged(c.batch)), c.id
        assert c.batch.flt_weight is None or c.name != "counts"


@pytest.mark.parametrize("case", SAME, ids=[c.id for c in SAME])
def test_one_curve_passed_twice_is_the_one_curve_reference(case):
    assert case.f_host is case.x_host and case.f_interp == case.x_interp
    new = XR.per_trade_reference(*case.args)
    old = PR.per_trade_reference(case.f_interp.value, case.f_host, case.batch)
    b = case.batch
    worst = Fraction(0)
    for i, (d, o) in enumerate(zip(new, old)):
        j = slice(int(b.flt_off[i]), int(b.flt_off[i + 1]))
        all_lagged = bool(np.all((b.flt_te[j] != b.flt_tp[j]) | ~(b.flt_alpha[j] > 0.0)))
        pairs = [(XR.rational(d["pv"], (0,)), XR.rational(o["pv"], (0,)))]
        for p in range(case.f_host.jac.shape[1]):
            (vf, af), (vx, ax) = XR.rational(d["delta_foreign"], (p,)), XR.rational(d["delta_basis"], (p,))
            pairs.append(((vf + vx, af + ax), XR.rational(o["delta"], (p,))))
        for (v, a), (w, g) in pairs:
            assert abs(v - w) <= TINY * max(a, g), (case.id, i)
            assert (a == 0) == (g == 0) or not all_lagged, (case.id, i)
            if all_lagged:
                assert abs(a - g) <= TINY * g, (case.id, i)
            else:
                assert a >= g * (1 - TINY), (case.id, i)
            if g:
                worst = max(worst, abs(v - w) / g)
    print(f"{case.id}: worst |new - old| / gross = {float(worst):.2e}")


DIFF_NODES = (("between knots", 0.6, 0.8, 0.9), ("a shared knot", 0.7, 1.2, 1.3), ("across the tables", 0.3, 1.2, 2.5),
              ("tp beyond the last knot", 1.7, 5.0, 7.5), ("paid at the value time", 0.5, 1.0, 0.0))


@pytest.mark.parametrize("pair", XS.PAIRS, ids=lambda p: f"{XS.NAMES[p[0]]} x {XS.NAMES[p[1]]}")
def test_the_two_ladders_sums_against_numerical_derivatives(pair):
    fm, xm = pair
    hf, hx = XC.host_of("lookup", XC.SCHEME[fm]), XC.host_of("lookup, a knot three times", XC.SCHEME[xm])
    old = mp.dps
    try:
        mp.dps = 120
        F = R._Curve(fm, hf.times, hf.dfs, hf.jac, None)
        X = R._Curve(xm, hx.times, hx.dfs, hx.jac, None)
        for name, ts, te, tp in DIFF_NODES:
            batch = PL.make_book([PL.weighted(PL.coupon(ts, te, tp, notional=1234567.25, spread=0.0, flt_sign=-1.0), 0.75)])
            sf, sx = R._Sums(F, False), R._Sums(X, False)
            assert XR._add_trade(F, X, sf, sx, batch, 0) == 2
            c = mpf("-1234567.25") * mpf("0.75")

            def D(cv, plan, ks, L):
                if cv.method == R.LINEAR_FWD:
                    return sum((wk * mp.exp(L[ks.index(k)]) for k, wk in plan), mpf(0))
                return mp.exp(sum((wk * L[ks.index(k)] for k, wk in plan), mpf(0)))

            ps, pe, pp = F.date(ts)[1], F.date(te)[1], X.date(tp)[1]
            kf, kx = sorted({k for plan in (ps, pe) for k, _ in plan}), sorted({k for k, _ in pp})
            Lf, Lx = tuple(F.L[k] for k in kf), tuple(X.L[k] for k in kx)
            value = lambda lf, lx: c * (D(F, ps, kf, lf) / D(F, pe, kf, lf) - 1) * D(X, pp, kx, lx)
            assert abs(value(Lf, Lx) - sx.pv) <= abs(c) * mpf(10) ** -100
            worst = mpf(0)
            for i, k in enumerate(kf):
                num = mp.diff(lambda *l: value(l, Lx), Lf, tuple(int(j == i) for j in range(len(kf))))
                worst = max(worst, abs(num - sf.g.get(k, mpf(0))) / abs(c))
                assert sf.g_abs.get(k, mpf(0)) >= abs(sf.g.get(k, mpf(0))) * (1 - mpf(10) ** -50)
            for i, k in enumerate(kx):
                num = mp.diff(lambda *l: value(Lf, l), Lx, tuple(int(j == i) for j in range(len(kx))))
                worst = max(worst, abs(num - sx.g.get(k, mpf(0))) / abs(c))
                assert sx.g_abs.get(k, mpf(0)) >= abs(sx.g.get(k, mpf(0))) * (1 - mpf(10) ** -50)
            assert set(sf.g) <= set(kf) and set(sx.g) <= set(kx)
            print(f"{XS.NAMES[fm]} x {XS.NAMES[xm]}, {name}: worst |analytic - numerical| / |c| = {mp.nstr(worst, 3)}")
            assert worst < mpf(10) ** -30, name
    finally:
        mp.dps = old


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_pv_is_the_scenario_references(case):
    ref = XR.per_trade_reference(*case.args)
    scen = XSR.reference(case.f_interp.value, case.f_host.times, case.f_host.dfs, case.x_interp.value, case.x_host.times,
                         case.x_host.dfs, case.batch)
    mp.dps = 60
    for i, d in enumerate(ref):
        pv = mpf(int(d["pv"].V[0])) * mpf(2) ** d["pv"].E
        gross = mpf(int(d["pv"].A[0])) * mpf(2) ** d["pv"].E
        assert abs(pv - scen.value[i][0]) <= mpf(10) ** -50 * max(gross, scen.gross[i][0]), (case.id, i)
        assert abs(gross - scen.gross[i][0]) <= mpf(10) ** -50 * gross, (case.id, i)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_leg_routes_to_the_payment_lag_rows(case):
    launches, cover = XC.route(case)
    assert np.all(cover == 1), case.id
    assert [(f, s, items) for f, s, items, _ in launches] == [("lite_lag", "lite_lag", XC.units_of(case.batch))], (case.id, launches)
    assert launches[0][3] == XC.blocks_for(XC.units_of(case.batch), 256)
    assert np.all(XC.rows_of(case.batch) > 0)
    assert XC.xc_lds_bytes(case.f_host, case.x_host) <= XC.LDS_BUDGET


def test_the_refused_books_do_not_route_there():
    case = CASES[0]
    for name, batch in XC.refused_books():
        launches, cover = XC.route(case, batch=batch)
        assert np.all(cover == 1) and {f for f, *_ in launches} - {"lite_lag"}, (name, launches)
        assert "lite_lag" in {f for f, *_ in launches}, name            # the lagged legs beside it would have been taken
    assert list(XC.rows_of(XC.refused_books()[0][1])) == [1, 1, 0]


def test_the_segment_books_have_the_row_counts_they_are_named_for():
    for case in CASES:
        rows = XC.rows_of(case.batch)
        m = np.diff(case.batch.flt_off)
        if case.name == "counts":
            assert list(m) == list(XC.COUNTS) and list(rows) == [1, 1, 1, 2, 2, 2, 3, 3, 4, 26, 26]
            assert len(set(rows)) == 5 > 3
        elif case.name == "short counts":
            assert list(m) == list(XC.SHORT_COUNTS) and list(rows) == [1, 1, 1, 2, 2, 2, 3, 3]
        else:
            assert set(rows) == {1}, case.id
    assert any(c.name == "counts" and c.f_interp == PE.LF for c in CASES) and any(c.name == "counts" and c.f_interp != PE.LF for c in CASES)
    assert [XC.cycled_units(s) for s in (1, 3, 4, 5)] == [1, 1, 2, 2]
    for n_cu in (1, 256, 304):
        sizes = XC.launch_sizes(n_cu)
        u = 12 * n_cu
        assert [XC.cycled_units(s) for s in sizes[4:]] == [u, u + 1, 2 * u + 1]
        assert [XC.blocks_for(XC.cycled_units(s), n_cu) for s in sizes[4:]] == [n_cu] * 3 and XC.blocks_for(u - 12, n_cu) == n_cu - 1
    book = XC.cycled_book(37)
    assert XC.units_of(book) == XC.cycled_units(37) and set(XC.rows_of(book)) == {1, 2}


def test_the_lds_pairs_sit_on_both_sides_of_the_budget():
    (f, inside), (_, beyond) = XC.lds_pairs()
    a, b = XC.xc_lds_bytes(f, inside), XC.xc_lds_bytes(f, beyond)
    print(f"K_f {f.times.size}, K_x {inside.times.size} | {beyond.times.size}: {a} <= {XC.LDS_BUDGET} < {b} bytes")
    assert a <= XC.LDS_BUDGET < b and beyond.times.size == inside.times.size + 1
    # the restatement against the library's own count of the one-curve delta instantiation's tables: the Jacobian table
    from adrates_amd import _native
    for h in (f, inside):
        assert _native.curve_tables_host(h.times, h.dfs, h.jac, h.hess)["lj"].shape[0] == XC.curve_sizes(h)[1]


def test_the_bound_reads_only_the_inputs():
    for case in CASES:
        stats = XR.trade_stats(*case.args)
        ref = XR.per_trade_reference(*case.args)
        assert [s["n"] for s in stats] == [d["n_terms"] for d in ref], case.id
        for s in stats:
            k = XR.trade_k(case.f_interp.value, case.x_interp.value, s)
            assert s["wr_f"] >= 1.0 and s["wr_x"] >= 1.0 and np.isfinite(s["cond_f"]) and np.isfinite(s["cond_x"])
            assert 20 <= k <= 80 + 20 * (s["cond_f"] + s["cond_x"]) * (1 + s["wr_f"] + s["wr_x"]) + 4 * s["n"] + 12 * (s["wr_f"] + s["wr_x"]), (case.id, k, s)
    assert XR.aggregate_sums(10, 1) == 28 and XR.aggregate_sums(10, 65) == 29
    with pytest.raises(AssertionError):
        XR.trade_k(R.LINEAR_FWD, R.FLAT_FWD, dict(n=1, cond_f=0.1, cond_x=0.1, wr_f=1.0, wr_x=1.0))
