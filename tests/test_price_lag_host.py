"""The cases of the payment-lag pricing tests (tests/_price_lag_cases.py) and the reference's ratio terms
(tests/_ladder_reference.py, "Ratio terms") checked without a GPU, before tests/test_gpu_price_lag.py holds the kernels to them:
  routing      `route_host` reports for every case and request exactly the families `_price_edge_cases.families` names, every
               trade once; the five payment-lag families and both variants of the general kernel are reached, and each side
               of every coupon-count boundary lands in the family it is named for
  derivatives  the reference's analytic g_k and H_kl of a ratio term against `mpmath.diff` of c D(ts) D(tp) / D(te) in the
               L_k, at 120 digits, to 30 significant digits - nodes on two, three (a shared knot), four and six distinct knots
               under every scheme.  This check does not depend on the formulas having been typed correctly.
  PV           the extended reference's PV is `_scenario_reference`'s value of the same batch, as mpmath numbers
  the oracle   oracle/port.c prices every book inside the bound - a trade with ratio terms under `trade_k("general_lag")`,
               the count of the general kernel's ratio nodes, the others under `bound_k` as tests/test_price_edges_host.py
               holds them; it refuses nothing.  The oracle's own lines differ (it differentiates A / B C / V in the knot
               discount factors and projects with jac and hess); its count is not taken: it stays inside the general
               kernel's with the shares below.
  bounds       k is finite, reads only the inputs and is larger for the families that count more

Worst shares of the bound observed for the C oracle (the test prints each): lag geometry 0.082 (the (8, 8) curve,
FLAT_FWD_RATES), structure 0.039, counts 0.060; 0.028 under LINEAR_FWD_RATES; no book is refused.  The module takes about
two minutes, the references built."""
import numpy as np
import pytest
from mpmath import mp, mpf

from adrates_amd import _native
from oracle import port

from . import _ladder_edge_cases as E
from . import _ladder_reference as R
from . import _price_edge_cases as PE
from . import _price_lag_cases as PL
from . import _price_reference as PR
from . import _scenario_reference as SR

CASES = PL.cases()
IDS = [c.id for c in CASES]
LAG_FAMILIES = ("fast_lag", "fast_lag_chained", "lite_lag", "knot_lag")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_case_reaches_the_kernels_it_is_named_for(case):
    layout, lds_rows = PE.layout_of(case.host)
    assert (layout, lds_rows) == PE.LAYOUTS[case.curve], (case.id, layout, lds_rows)
    assert case.host.jac.shape[1] <= 32 and R.compact_count(case.host.times) <= 256          # `knot_lag` wants Kc <= 256
    assert np.any(PE.lagged(case.batch))
    for name, mask, per_trade, aggregate in PE.REQUESTS:
        launches, cover = PL.route(case, mask, per_trade, aggregate)
        print(f"{case.id}, {name}: {launches}")
        assert np.all(cover == 1), (case.id, name)
        want = PE.families(case, mask, per_trade, aggregate)
        assert {f for f, *_ in launches} == set(want), (case.id, name, launches, sorted(set(want)))
        for fam in ("fast_lag", "general", "lite_lag", "knot_lag", "fast", "lite", "knot"):
            mine = [items for f, _, items, _ in launches if f == fam]
            if fam in ("lite", "lite_lag", "knot", "knot_lag"):       # a lite table's items are units of four trade slots
                assert len(mine) == (1 if fam in want else 0), (case.id, name, fam)
            elif fam in want:
                assert mine == [np.count_nonzero(want == fam)], (case.id, name, fam, launches)


def test_the_cases_reach_every_family_and_both_general_variants():
    reached, lds, l2 = set(), set(), set()
    for case in CASES:
        for name, mask, per_trade, aggregate in PE.REQUESTS:
            fams = PE.families(case, mask, per_trade, aggregate)
            reached |= {(f, case.interp == PE.LF) for f in fams}
            ratio = np.array([s["ratio"] > 0 for s in PR.trade_stats(case.interp.value, case.host, case.batch)])
            if mask & 4 and np.any((fams == "general") & ratio):
                (lds if PE.LAYOUTS[case.curve][1] else l2).add((case.curve, case.interp.name))
    assert {(f, False) for f in LAG_FAMILIES} | {("lite_lag", True), ("knot_lag", True), ("general", True), ("general", False)} <= reached
    assert not {(f, True) for f in ("fast_lag", "fast_lag_chained")} & reached               # log-linear schemes only
    # ratio nodes on the general kernel with GAMMA: LDS-resident rows (README 32 and 31 pillars, odd P; LINEAR_FWD_RATES) and
    # rows streamed from L2 (the (8, 8) and (12, 12) curves, the dense lookup tables)
    assert {("README 32", "LINEAR_FWD_RATES"), ("31 pillars", "LINEAR_ZERO_RATES"), ("README 32", "LINEAR_ZERO_RATES")} <= lds, lds
    assert {("epg 8", "FLAT_FWD_RATES"), ("core21 epg 12", "FLAT_FWD_RATES")} | {("lookup", s.name) for s in PE.SCHEMES} <= l2, l2
    # the fast variant's instantiations: the hub layout (README 32) and (12, 12); it wants an even pillar count, so the (7, 7)
    # curve of 17 pillars and the (8, 8) curve of 21 send their lagged trades to the general kernel
    fast = {PE.LAYOUTS[c.curve][0][1:] for c in CASES if "fast_lag" in PE.families(c, 7, True, False)}
    chained = {PE.LAYOUTS[c.curve][0][1:] for c in CASES if "fast_lag_chained" in PE.families(c, 7, True, False)}
    assert fast == {(7, 5, 1), (12, 12, 0)} == chained, (fast, chained)
    assert any(c.far_pairs for c in CASES) and any(not c.far_pairs and c.name.startswith("lag geometry") for c in CASES)


def test_each_side_of_every_count_boundary_lands_in_its_family():
    for case in CASES:
        if case.name not in ("counts", "short counts"):
            continue
        counts = PL.COUNTS if case.name == "counts" else PL.SHORT_COUNTS
        m = np.diff(case.batch.flt_off)
        assert list(m[:len(counts)]) == list(counts) and list(m[len(counts):]) == list(PL.WEIGHTED_COUNTS)
        packed_even_log = case.interp != PE.LF and case.host.jac.shape[1] % 2 == 0
        for (mask, per_trade, aggregate), col in (((7, True, False), 0), ((3, True, False), 1), ((1, True, False), 1), ((7, False, True), 2),
                                                  ((3, False, True), 2)):
            fams = PE.families(case, mask, per_trade, aggregate)
            launches, cover = PL.route(case, mask, per_trade, aggregate)
            assert {f for f, *_ in launches} == set(fams) and np.all(cover == 1)
            for i, c in enumerate(counts):
                want = PL.COUNT_FAMILIES[c][col]
                if col == 0 and not packed_even_log:
                    want = "general"
                assert fams[i] == want, (case.id, mask, per_trade, c, fams[i], want)
            want_weighted = {0: ["fast_lag", "fast_lag_chained"] if packed_even_log else ["general"] * 2, 1: ["lite_lag"] * 2, 2: ["knot_lag"] * 2}
            assert list(fams[len(counts):]) == want_weighted[col], (case.id, mask, per_trade)          # weighted legs of 32 | 33
        if packed_even_log:                     # the launches' sizes: nine one-row trades (eight lagged legs and a weighted one)
            rows = {f: items for f, _, items, _ in PL.route(case, 7)[0]}
            one_row = sum(1 for c in counts if c <= 32) + 1
            assert rows["fast_lag"] == one_row, rows


# ---------------------------------------------------------------------------------------------------- the derivatives
DIFF_TIMES = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 5.0, 7.0])
DIFF_NODES = (("two knots", 0.6, 0.8, 0.9), ("a shared knot", 0.7, 1.2, 1.3), ("four knots", 0.2, 2.4, 2.7), ("six knots", 0.3, 1.2, 2.5),
              ("te on a knot, tp beyond the last", 1.7, 5.0, 7.5), ("te and tp snap to one knot", 0.25, 2.0, 2.0 + 5e-11))


@pytest.mark.parametrize("interp", PE.SCHEMES, ids=lambda i: i.name)
def test_the_ratio_terms_derivatives_against_numerical_ones(interp):
    host = E.lookup_curve(DIFF_TIMES)
    old = mp.dps
    try:
        mp.dps = 120
        cv = R._Curve(interp.value, host.times, host.dfs, host.jac, host.hess)
        for name, ts, te, tp in DIFF_NODES:
            c = mpf("-1234567.25")
            sums = R._Sums(cv, True)
            sums.add_ratio(ts, te, tp, c)
            plans = [cv.date(t)[1] for t in (ts, te, tp)]
            ks = sorted({k for plan in plans for k, _ in plan})
            assert set(sums.g) == set(ks), name

            def D(plan, L):
                if interp == PE.LF:
                    return sum((wk * mp.exp(L[ks.index(k)]) for k, wk in plan), mpf(0))
                return mp.exp(sum((wk * L[ks.index(k)] for k, wk in plan), mpf(0)))

            f = lambda *L: c * D(plans[0], L) * D(plans[2], L) / D(plans[1], L)
            at = tuple(cv.L[k] for k in ks)
            assert abs(f(*at) - sums.pv) <= abs(sums.pv) * mpf(10) ** -100
            scale = abs(sums.pv)
            worst = mpf(0)
            for i, k in enumerate(ks):
                num = mp.diff(f, at, tuple(int(j == i) for j in range(len(ks))))
                worst = max(worst, abs(num - sums.g[k]) / scale)
                assert sums.g_abs[k] >= abs(sums.g[k]) * (1 - mpf(10) ** -50)
                for j, l in enumerate(ks):
                    num = mp.diff(f, at, tuple(int(q == i) + int(q == j) for q in range(len(ks))))
                    got = sums.H.get((k, l), mpf(0))
                    worst = max(worst, abs(num - got) / scale)
                    assert sums.H_abs.get((k, l), mpf(0)) >= abs(got) * (1 - mpf(10) ** -50), (name, k, l)
                    assert sums.H.get((l, k), mpf(0)) == got or abs(sums.H.get((l, k), mpf(0)) - got) <= scale * mpf(10) ** -100
            print(f"{interp.name}, {name}: {len(ks)} knots, worst |analytic - numerical| / |value| = {mp.nstr(worst, 3)}")
            assert worst < mpf(10) ** -30, (interp.name, name)
        distinct = {name: len({k for t in (ts, te, tp) for k, _ in cv.date(t)[1]}) for name, ts, te, tp in DIFF_NODES}
        assert [distinct[n] for n in ("two knots", "a shared knot", "four knots", "six knots")] == [2, 3, 4, 6], distinct
    finally:
        mp.dps = old


def test_a_same_date_pair_has_gross_zero_under_linear_fwd():
    """The reduced form: ts between two knots k, l reaches H_kl only through s_k s_l, which it does not hold - gross 0."""
    host = E.lookup_curve(DIFF_TIMES)
    mp.dps = 60
    cv = R._Curve(PE.LF.value, host.times, host.dfs, host.jac, host.hess)
    sums = R._Sums(cv, True)
    sums.add_ratio(0.3, 1.2, 2.5, mpf(1e6))
    assert (0, 1) not in sums.H_abs and (4, 5) not in sums.H_abs and sums.H_abs[(2, 3)] > 0 and sums.H[(2, 3)] > 0
    log = R._Sums(R._Curve(PE.FF.value, host.times, host.dfs, host.jac, host.hess), True)
    log.add_ratio(0.3, 1.2, 2.5, mpf(1e6))
    assert log.H_abs[(0, 1)] > 0


# ------------------------------------------------------------------------------------------ PV, the oracle, the bounds
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_pv_is_the_scenario_references(case):
    h, method = case.host, case.interp.value
    ref = PR.per_trade_reference(method, h, case.batch)
    scen = SR.reference(method, h.times, h.dfs, case.batch)
    mp.dps = 60
    for i, d in enumerate(ref):
        pv = mpf(int(d["pv"].V[0])) * mpf(2) ** d["pv"].E
        gross = mpf(int(d["pv"].A[0])) * mpf(2) ** d["pv"].E
        assert abs(pv - scen.value[i][0]) <= mpf(10) ** -50 * max(gross, scen.gross[i][0]), (case.id, i)
        assert (gross == 0) == (scen.gross[i][0] == 0), (case.id, i)


def oracle_ks(case, ref):
    stats = PR.trade_stats(case.interp.value, case.host, case.batch)
    return [PR.trade_k("general_lag", case.interp.value, s) if s["ratio"] else d["k"] for s, d in zip(stats, ref)]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_oracle_prices_every_new_book_inside_the_bound(case):
    h, method = case.host, case.interp.value
    ref = PR.per_trade_reference(method, h, case.batch)
    rows = port.price(method, h.times, h.dfs, h.jac, h.hess, case.batch)          # a refusal raises: the oracle refuses nothing here
    ks = oracle_ks(case, ref)
    got = {k: np.asarray(rows[k]) for k in R.RATES_BLOCKS}
    share = PR.rows_share(got, ref, ks, f"oracle {case.id}")
    zero = sum(int(np.count_nonzero(np.asarray(d["gamma"].A) == 0)) for d in ref)
    total = sum(d["gamma"].V.size for d in ref)
    print(f"C oracle, {case.id}: share of the bound {share:.3f} (k {min(ks)} to {max(ks)}); {zero} of {total} gamma entries have gross 0")
    assert share <= 1.0, case.id
    book = PR.book_reference(method, h, case.batch)
    for name in R.RATES_BLOCKS:
        k = PR.book_k(ref, book, ks, name, case.batch.n_trades)
        assert PR.share_elems(book[name], got[name].sum(0), k, f"oracle book {case.id} {name}") <= 1.0


def test_the_lag_bounds_read_only_the_inputs():
    case = [c for c in CASES if c.name == "counts" and c.interp == PE.LZ][0]
    method = case.interp.value
    ref = PR.per_trade_reference(method, case.host, case.batch)
    stats = PR.trade_stats(method, case.host, case.batch)
    assert [s["n"] for s in stats] == [d["n_terms"] for d in ref]
    m = np.diff(case.batch.flt_off)
    n_lag = len(PL.COUNTS)
    assert [s["ratio"] for s in stats[:n_lag]] == list(m[:n_lag]) and all(s["ratio"] == 0 for s in stats[n_lag:])
    for s in stats:
        assert s["cond_lag"] >= s["cond"] > 0.0 and np.isfinite(s["cond_lag"]) and s["wr"] >= 1.0
        ks = {fam: PR.trade_k(fam, method, s) for fam in ("fast", "fast_lag", "general", "general_lag", "lite", "lite_lag")}
        assert all(20 <= k <= 40 + 12 * s["cond_lag"] + 6 * s["n"] + 20 * s["wr"] for k in ks.values()), ks
        assert ks["fast_lag"] > ks["fast"] and ks["general_lag"] > ks["general"] and ks["general_lag"] > ks["fast_lag"] and ks["lite_lag"] > ks["lite"]
        assert PR.knot_trade_k(method, s, lag=True) > PR.knot_trade_k(method, s)
    assert PR.knot_lag_sums(stats, 107, 4) > PR.knot_sums(stats, 107, 4)
    # a weighted batch is another batch than the same one without weights
    plain = PL.make_book(PL.counts_trades())
    plain.flt_weight = None
    other = PR.per_trade_reference(method, case.host, plain)
    assert other is not ref and other[-1]["pv"].floats()[0] != ref[-1]["pv"].floats()[0]
