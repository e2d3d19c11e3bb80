"""The sub-book ladder host twins (adr_subbook_ladders_host, adr_credit_subbook_ladders_host, adr_yoy_subbook_ladders_host) and
the C oracle on the hand-made edge books (tests/_ladder_edge_cases.py) against the plain 60-digit reference
(tests/_ladder_reference.py), EVERY element: |got - value| <= k 2^-53 gross with k derived in the reference's docstring, and
+0.0 where gross is 0.  No GPU.

Worst observed shares of the bound over all cases and schemes (each test prints its own):
  rates      host twin 0.074   C oracle 0.062
  credit     host twin 0.023   C oracle 0.029
  inflation  host twin 0.110 / 0.111 / 0.118 under LINEAR_ZERO / FLAT_FWD / LINEAR_FWD discounting (k from 72 to 802; the
             worst is a discount-lookup desk of one swap); no entry has left the bound.  The inflation reference itself
             against the older torch / C oracle rows, on that oracle's scale: at most 1.8e-13 of 1e-10.
The slowest of the inflation tests takes 12 s (one discount scheme, all ten cases and their layouts, the references built).
One-line mutations of the shared host / device code, tried on the host twin and reverted; every one but the last, which is
unreachable, fails `test_yoy_host_twin_every_element`, and the last column says whether
tests/test_yoy_sub_book_ladders_host.py fails too:
  the last entry left out of `project_inflation`'s cross loop (e < Pi * P - 1)                                    yes
  si::kSnap 1e-8 in place of 1e-10                                                                                 no
  v = L'' without the coupon's coefficient on a merged slot                                                        yes
  the gate c.amount != 0.0 moved to cover the inflation adds as well                                               no
  t.wb dropped from M where d.a is the last of equal knots                                                         yes
  ... only where d.a is the last of three or more equal knots (the README grid has such runs too)                  yes
  ... only where d.a is the FIRST of equal knots: neither module fails, and none can - the lower knot of a two-knot
      lookup is the last of its run (searchsorted 'right'), so the mutated branch is never taken
Before oracle/port.c priced a coupon paid on its accrual end in its linear form it stood at 1.36 (rates) and 0.99 (credit) and
left entries without any term at 1e-19, so the 1e-12-level gaps of the older oracle comparisons
(tests/test_sub_book_ladders_host.py, tests/test_credit_sub_book_ladders_host.py and their GPU forms) were the oracle's: on the
credit geometry book's one-trade desk, the old 8.6e-12, the old oracle is 8.5e-12 from this reference on the old scale and the
host twin 3.9e-13 (DESIGN.md sections 19 and 21)."""
import numpy as np
import pytest

from adrates_amd import _native
from adrates_amd.utils.error import LibError

from . import _credit_ladder_cases as CL
from . import _ladder_edge_cases as E
from . import _ladder_reference as R
from . import _scenario_cases as SC
from . import _sub_book_ladder_cases as L
from . import _yoy_cases as YC
from . import _yoy_ladder_cases as Y


def host_rates(interp, case, sub_off):
    h = case.host
    return _native.subbook_ladders_host(interp.value, h.times, h.dfs, h.jac, h.hess, case.batch, sub_off)


def desk_sums(rows, sub_off, blocks):
    """The oracle's per-trade rows summed per desk in trade order."""
    return {k: np.array([np.asarray(rows[k][lo:hi]).sum(0) for lo, hi in zip(sub_off[:-1], sub_off[1:])]) for k in blocks}


@pytest.mark.parametrize("interp", E.SCHEMES, ids=lambda i: i.name)
def test_rates_host_twin_every_element(interp):
    worst = 0.0
    for case in E.rates_cases(interp):
        for layout, sub_off in case.layouts.items():
            ref = R.rates_reference(interp.value, case.host, case.batch, sub_off)
            share = R.worst_share(host_rates(interp, case, sub_off), ref, what=f"{case.name}/{layout}")
            print(f"host twin, {interp.name}, {case.name}/{layout}: share of the bound {share:.3f} (k up to {max(d['k'] for d in ref)})")
            assert share <= 1.0, (case.name, layout)
            worst = max(worst, share)
    print(f"host twin, {interp.name}: worst share {worst:.3f}")


@pytest.mark.parametrize("interp", E.SCHEMES, ids=lambda i: i.name)
def test_rates_oracle_every_element(interp):
    """oracle/port.c on the same books, the same reference and the same bound, +0.0 where gross is 0 included.  This test is
    what found the oracle's lost digits: it used to price every accruing coupon as D(ts) / D(te) D(tp) and to differentiate
    the three factors, and where te == tp the second partials in D(te) and D(tp) cancel only up to rounding.  On these books
    that form reached 1.36 of the bound (LINEAR_FWD_RATES, 65 pillars; 1.12 under LINEAR_ZERO_RATES on the folding book's
    trade 0) against the host twin's 0.08 and left up to 680 entries without any term at 1e-19 instead of +0.0.  port.c
    now prices a coupon paid on its accrual end as A + (s alpha - 1) C, and stays below 0.07."""
    worst, refused = 0.0, []
    for case in E.rates_cases(interp):
        try:
            rows = L.oracle_rows(interp.value, case.host, case.batch)
        except RuntimeError:
            refused.append(case.name)
            continue
        for layout, sub_off in case.layouts.items():
            ref = R.rates_reference(interp.value, case.host, case.batch, sub_off)
            share = R.worst_share(desk_sums(rows, sub_off, R.RATES_BLOCKS), ref, what=f"oracle {case.name}/{layout}")
            print(f"C oracle, {interp.name}, {case.name}/{layout}: share of the bound {share:.3f}")
            assert share <= 1.0, (case.name, layout)
            worst = max(worst, share)
    print(f"C oracle, {interp.name}: worst share {worst:.3f}; refused: {refused}")


def credit_got_blocks(got):
    return {k: got[k] for k in R.CREDIT_BLOCKS}


@pytest.mark.parametrize("interp", E.SCHEMES, ids=lambda i: i.name)
def test_credit_host_twin_every_element(interp):
    worst = 0.0
    for c in E.credit_cases(interp):
        ref = R.credit_reference(interp.value, c.host, c.case, c.G, c.sub_off)
        got = CL.host_ladders(interp.value, c.host, c.case, c.G, c.sub_off)
        CL.check_layout(got, c.host.jac.shape[1], c.G)
        share = R.worst_share(credit_got_blocks(got), ref, R.CREDIT_BLOCKS, what=c.name)
        print(f"credit host twin, {interp.name}, {c.name}: share of the bound {share:.3f} (k up to {max(d['k'] for d in ref)})")
        assert share <= 1.0, c.name
        worst = max(worst, share)
    print(f"credit host twin, {interp.name}: worst share {worst:.3f}")


def credit_oracle_blocks(rows, case, sub_off, G):
    """`_credit_ladder_cases.reference`'s per-trade rows summed per desk and per (desk, bucket) cell."""
    out = desk_sums(rows, sub_off, R.RATES_BLOCKS)
    P = np.asarray(rows["delta"]).shape[1]
    B = sub_off.size - 1
    out.update(cs01=np.zeros((B, G)), spread_gamma=np.zeros((B, G)), cross_gamma=np.zeros((B, G, P)))
    for b, (lo, hi) in enumerate(zip(sub_off[:-1], sub_off[1:])):
        for g in range(G):
            idx = lo + np.nonzero(case.bucket[lo:hi] == g)[0]
            out["cs01"][b, g] = rows["cs01"][idx].sum(0)
            out["spread_gamma"][b, g] = rows["spread_gamma"][idx].sum(0)
            out["cross_gamma"][b, g] = rows["cross"][idx].sum(0)
    return out


@pytest.mark.parametrize("interp", E.SCHEMES, ids=lambda i: i.name)
def test_credit_oracle_every_element(interp):
    """`_credit_ladder_cases.reference` (the C oracle on rescaled batches) under `test_rates_oracle_every_element`'s terms."""
    worst, refused = 0.0, []
    for c in E.credit_cases(interp):
        try:
            rows = CL.reference(interp.value, c.host, c.case)
        except RuntimeError:
            refused.append(c.name)
            continue
        ref = R.credit_reference(interp.value, c.host, c.case, c.G, c.sub_off)
        share = R.worst_share(credit_oracle_blocks(rows, c.case, c.sub_off, c.G), ref, R.CREDIT_BLOCKS, what=f"oracle {c.name}")
        print(f"credit C oracle, {interp.name}, {c.name}: share of the bound {share:.3f}")
        assert share <= 1.0, c.name
        worst = max(worst, share)
    print(f"credit C oracle, {interp.name}: worst share {worst:.3f}; refused: {refused}")


@pytest.mark.parametrize("interp", E.SCHEMES, ids=lambda i: i.name)
def test_yoy_host_twin_every_element(interp):
    worst = 0.0
    for c in E.yoy_cases(interp):
        for layout, sub_off in c.layouts.items():
            ref = R.yoy_reference(interp.value, c.host, c.infl, c.book, sub_off)
            share = E.check_yoy_rows(E.yoy_entry(interp, c, sub_off), ref, c, f"{c.name}/{layout}")
            print(f"inflation host twin, {interp.name}, {c.name}/{layout}: share of the bound {share:.3f} (k up to {max(d['k'] for d in ref)})")
            assert share <= 1.0, (c.name, layout)
            worst = max(worst, share)
    print(f"inflation host twin, {interp.name}: worst share {worst:.3f}")


@pytest.mark.parametrize("interp", E.SCHEMES, ids=lambda i: i.name)
def test_yoy_reference_against_the_oracle(interp):
    """The new reference held to the older one: `_yoy_ladder_cases.reference` (torch autodiff over the inflation factors, the
    C oracle for the PV and the discount block) gives one row per swap, and on every case it can price the 60-digit
    reference's desks, rounded to float64, are those rows summed per desk to the project's 1e-10 of `desk_errors`' scale.

    What the oracle can price: it is a float64 evaluation, so an element comes out of it with an error of up to
    k 2^-53 of the element's gross, and its scale - the largest sum of absolute per-swap entries of the desk's block - does
    not count the cancellation inside one swap.  Where 1e-10 of that scale is less than that error (a swap alone in its desk
    whose coupon amount is 0 or is cancelled by its own fixed flow, so that the PV is rounding and so is the scale; the
    breakeven entries of a coupon whose two held ends cancel beside a small discount gamma), the scale measures nothing and
    the element is held to k 2^-53 of its gross instead; the blocks with such elements are listed with their count."""
    worst, refused, cancelled = 0.0, [], []
    for c in E.yoy_cases(interp):
        if not c.want_gamma:
            continue                                         # the same book and curves as the first case
        try:
            rows = Y.reference(interp.value, c.host, c.infl, c.book)
        except RuntimeError:
            refused.append(c.name)
            continue
        for layout, sub_off in c.layouts.items():
            ref = R.yoy_reference(interp.value, c.host, c.infl, c.book, sub_off)
            gap = 0.0
            for b, (lo, hi) in enumerate(zip(sub_off[:-1], sub_off[1:])):
                for key in R.RATES_BLOCKS:
                    mine = ref[b][key].floats().reshape(-1)
                    r = np.asarray(rows[key][lo:hi]).reshape(hi - lo, mine.size)
                    scale = float(np.max(np.abs(r).sum(0))) if hi > lo else 0.0          # `desk_errors`' scale
                    noise = ref[b]["k"] * 2.0 ** -53 * ref[b][key].gross_floats().reshape(-1)
                    diff = np.abs(mine - r.sum(0))
                    if scale == 0.0 and not np.any(noise):            # an empty desk, a desk of dead flows: both are 0
                        assert not np.any(diff) and not np.any(mine), (c.name, layout, b, key)
                        continue
                    lost = Y.TOL * scale < noise
                    assert np.all(diff[lost] <= noise[lost]), (c.name, layout, b, key)
                    if np.any(lost):
                        cancelled.append(f"{c.name}/{layout} desk {b} {key}: {np.count_nonzero(lost)}")
                    if not np.all(lost):
                        gap = max(gap, float(np.max(diff[~lost])) / scale)
            print(f"inflation reference against the oracle, {interp.name}, {c.name}/{layout}: {gap:.2e}")
            assert gap <= Y.TOL, (c.name, layout)
            worst = max(worst, gap)
    print(f"inflation reference against the oracle, {interp.name}: worst {worst:.2e}; refused: {refused}; held to the gross: {cancelled}")

def test_the_books_take_the_branches_they_are_named_for():
    """The folding book's comments, checked on its arrays: which coupons chain, which fixed flows merge."""
    b = E.folding_book()
    fix = lambda i: slice(int(b.fix_off[i]), int(b.fix_off[i + 1]))
    flt = lambda i: slice(int(b.flt_off[i]), int(b.flt_off[i + 1]))
    chained = lambda i: np.array_equal(b.flt_ts[flt(i)][1:], b.flt_tp[flt(i)][:-1])
    merged = lambda i: [bool(c < b.flt_tp[flt(i)].size and b.flt_tp[flt(i)][c] == t) for c, t in enumerate(b.fix_tp[fix(i)])]
    assert all(chained(i) for i in (0, 1, 3, 4, 5, 6, 7, 8)) and not chained(2)
    assert b.spread[0] == 0.0 and b.spread[1] != 0.0
    assert b.flt_alpha[flt(3)][1] == 0.0 and b.flt_alpha[flt(4)][2] < 0.0
    assert b.flt_tp[flt(5)][0] == 0.0 and b.fix_tp[fix(5)][0] == 0.0 and b.flt_ts[flt(5)][0] < 0.0
    assert b.flt_tp[flt(6)][0] < 0.0 and b.flt_ts[flt(6)][1] == b.flt_tp[flt(6)][0] and b.flt_tp[flt(6)][1] > 0.0
    assert merged(7) == [True] * 3 and merged(8) == [False] * 2 and merged(9) == [True, True, False, False, False]
    assert all(t in b.flt_tp[flt(8)] for t in b.fix_tp[fix(8)])          # another index's dates
    assert b.flt_tp[flt(10)].size == 0 and b.fix_tp[fix(11)].size == 0
    for i in (12, 24):
        assert b.flt_tp[flt(i)].size == 0 and b.fix_tp[fix(i)].size == 0
    assert merged(13) == [True, True, False] and list(b.fix_pay[fix(13)]) == [0.0, 41000.0, 0.0]
    assert b.notional.min() == 1.0 and b.notional.max() == 1e8 and {-1.0, 1.0} == set(b.fix_sign) == set(b.flt_sign)
    legs, sub_off = E.long_leg_book()
    flows = [int(legs.flt_off[hi] - legs.flt_off[lo]) for lo, hi in zip(sub_off[:-1], sub_off[1:])]
    assert flows == [853, 64, 65, 128]
    for times in (SC.LOOKUP_TIMES, E.LOOKUP_TIMES_TRIPLE):
        tables = _native.curve_tables_host(times, E.lookup_curve(times).dfs, E.lookup_curve(times).jac, E.lookup_curve(times).hess)
        assert len(tables["knot_index"]) == R.compact_count(times) == 6
    # the cancelling pair is a desk of the "pairs" layout: value 0 and gross not 0 in the reference
    pairs = E.folding_layouts(b.n_trades)["pairs"]
    desk = int(np.nonzero(pairs[:-1] == 17)[0][0])
    assert pairs[desk + 1] == 19
    ref = R.rates_reference(E.SCHEMES[0].value, E.gbp_curve(E.SCHEMES[0]), b, pairs)[desk]
    assert abs(int(ref["pv"].V[0])) * 10 ** 50 < int(ref["pv"].A[0])          # 0 to the reference's 60 digits
    assert np.all(np.abs(ref["gamma"].V) * 10 ** 50 <= ref["gamma"].A) and np.any(ref["gamma"].A)
    the_inflation_books_take_the_branches_they_are_named_for()


def the_inflation_books_take_the_branches_they_are_named_for():
    """The inflation cases' names, checked on their arrays and on `_lookup_plan`'s decisions on the nodes x = [0, T5]."""
    from oracle.mp_oracle import _lookup_plan
    x = np.concatenate(([0.0], YC.T5))
    knots = lambda t, im: [k for k, _ in R._infl_slots(x, t, im)]              # the live slots of one date (knot 0 dropped)
    plan = lambda t, im=YC.FF: _lookup_plan(x, t, im)
    book = E.yoy_knot_book()
    cp = book.coupons
    first = lambda name: int(cp["cpn_off"][book.names.index(name)])
    sets = {}
    for name in book.names[:11]:
        j = first(name)
        assert cp["cpn_off"][book.names.index(name) + 1] == j + 1 and cp["tp"][j] == cp["te"][j]      # one coupon, paid at te
        sets[name] = (knots(cp["te"][j], YC.FF), knots(cp["ts"][j], YC.FF), j)
    merged = lambda name: len(set(sets[name][0]) | set(sets[name][1]))
    assert sets["one segment: two slots merge away"][:2] == ([2, 3], [2, 3])
    assert merged("te's lower knot is ts's upper knot: three knots") == 3 and merged("far-apart segments: four knots") == 4
    te, ts, j = sets["ts == te: every coefficient cancels"]
    assert te == ts and cp["ts"][j] == cp["te"][j]
    te, ts, j = sets["ts < 0 < te < T_1: knot 0 dropped"]
    assert plan(cp["ts"][j]) == ("flat", 0) and ts == [] and plan(cp["te"][j])[1:3] == (0, 1) and te == [1]
    j = sets["ts and te on pillars"][2]
    assert plan(cp["ts"][j]) == ("snap", 2) and plan(cp["te"][j]) == ("snap", 3)
    j = sets["ts and te within 1e-10 of pillars"][2]
    assert cp["ts"][j] != 2.0 and cp["te"][j] != 5.0 and plan(cp["ts"][j]) == ("snap", 2) and plan(cp["te"][j]) == ("snap", 3)
    j = sets["ts on the last pillar, te beyond"][2]
    assert plan(cp["ts"][j]) == ("snap", 5) and plan(cp["te"][j]) == ("flat", 5)
    j = sets["both beyond the last pillar"][2]
    assert plan(cp["ts"][j]) == plan(cp["te"][j]) == ("flat", 5) and knots(cp["te"][j], YC.LZ) == [5]
    j = sets["ts before T_1, te on T_1"][2]
    assert plan(cp["ts"][j])[1:3] == (0, 1) and plan(cp["te"][j]) == ("snap", 1)
    j = sets["ts == 0"][2]
    assert cp["ts"][j] == 0.0 and plan(0.0) == ("snap", 0) and sets["ts == 0"][1] == []
    i = book.names.index("all of the above in one swap")
    assert cp["cpn_off"][i + 1] - cp["cpn_off"][i] == 11
    i = book.names.index("seasoned: tp <= 0 masked")
    tp = cp["tp"][cp["cpn_off"][i]:cp["cpn_off"][i + 1]]
    assert tp[0] < 0.0 and np.count_nonzero(tp > 0.0) == 7
    i = book.names.index("paid at the value time")
    assert list(cp["tp"][cp["cpn_off"][i]:cp["cpn_off"][i + 1]]) == [0.0, 1.0]
    i = book.names.index("no coupons")
    assert cp["cpn_off"][i + 1] == cp["cpn_off"][i] and book.fixed[0][i + 1] == book.fixed[0][i]             # an empty swap
    assert list(np.diff(book.fixed[0])) == [i % 2 for i in range(book.n)]
    # the discount lookups: every date is both a coupon's and a fixed flow's payment date; the coupon has four live slots
    looks = E.yoy_lookup_book()
    assert np.array_equal(looks.coupons["tp"], E.YOY_LOOKUP_DATES) and np.array_equal(looks.fixed[1], E.YOY_LOOKUP_DATES)
    assert sorted(knots(12.0, YC.LZ) + knots(1.5, YC.LZ)) == [1, 2, 4, 5] and looks.n % 2 == 0
    for times in (SC.LOOKUP_TIMES, E.LOOKUP_TIMES_TRIPLE):
        kinds = [_lookup_plan(times, t, 1) for t in E.YOY_LOOKUP_DATES]
        first_of_run = int(np.nonzero(times == 1.0)[0][0])
        assert kinds[3] == ("snap", first_of_run) and kinds[13] == ("snap", first_of_run) and kinds[4][0] == "interp"
        assert kinds[4][1] == int(np.nonzero(times == 1.0)[0][-1]) and kinds[9] == ("flat", times.size - 1)
        assert E.YOY_LOOKUP_DATES[14] < 0.0 and E.YOY_LOOKUP_DATES[15] == 0.0
        assert np.all(E.lookup_curve(times).hess[1:] != 0.0) and np.all(E.lookup_curve(times).jac[1:] != 0.0)
    # the amount edges: the twin's amount of the first coupon is exactly 0.0 with two live slots, the second is cancelled
    for im in YC.INFL_SCHEMES:
        infl = (im, YC.T5, YC.B5)
        edges = E.yoy_amount_book(infl)
        ec = edges.coupons
        amount = _native.yoy_risk_host((YC.LF, np.array([0.0, 1.0]), np.array([1.0, 1.0])), infl, ec, 0)["amount"]
        assert amount[0] == 0.0 and not np.signbit(amount[0]) and ec["scale"][0] == 1e6 and ec["spread"][0] != 0.0
        assert knots(ec["te"][0], im) == [2, 3] and ec["tp"][0] > 0.0
        assert edges.fixed[1][0] == ec["tp"][1] and edges.fixed[2][0] == -amount[1] and amount[1] != 0.0
        assert ec["scale"][2] == 0.0 and edges.fixed[2][2] == 0.0 and edges.fixed[1][2] > 0.0
        assert ec["tp"][4] == 0.0 and edges.fixed[1][3] == 0.0 and ec["tp"][5] < 0.0 and edges.fixed[1][4] < 0.0
    chunks = E.yoy_chunk_book()
    off = L.offsets(E.YOY_CHUNK_SIZES)
    per_desk = lambda a: [int(a[hi] - a[lo]) for lo, hi in zip(off[:-1], off[1:])]
    assert per_desk(chunks.coupons["cpn_off"]) == [64, 65, 0, 71, 129, 26, 0] and per_desk(chunks.fixed[0]) == [0, 0, 0, 70, 0, 8, 0]
    assert off[-1] == chunks.n
    wide = [c for c in E.yoy_cases(E.SCHEMES[0]) if c.name.startswith("65 pillars")]
    assert [(c.host.jac.shape[1], c.infl[1].size) for c in wide] == [(65, 5), (65, 64)] and wide[0].book.n == sum(E.WIDE_DESKS)
    tables = _native.curve_tables_host(wide[0].host.times, wide[0].host.dfs, wide[0].host.jac, wide[0].host.hess)
    assert wide[0].host.times.size == 1292 and len(tables["knot_index"]) == R.compact_count(wide[0].host.times) == 116


def test_a_grid_that_starts_after_the_value_time_is_refused():
    """`_scenario_cases.LOOKUP_TIMES_LATE` (first knot at 0.25) is a grid of the scenario kernels only: the ladders' curve
    tables need the value-time knot (t = 0, D = 1), so 'a date before the first knot' is a negative date here (the folding
    book's trades 5 and 6)."""
    times = SC.LOOKUP_TIMES_LATE
    host = E.lookup_curve(times)
    host.dfs[0] = 1.0
    with pytest.raises(LibError, match="first knot must be the value time"):
        _native.subbook_ladders_host(E.SCHEMES[0].value, host.times, host.dfs, host.jac, host.hess, E.lookup_book(), np.array([0, 26]))


@pytest.mark.parametrize("interp", E.SCHEMES, ids=lambda i: i.name)
def test_a_value_time_hess_parts_the_oracle_from_the_kernels(interp):
    """The curve-table builder refuses jac[0] != 0 and takes hess[0] != 0.  The kernels price sum c D(t) (no division by
    D(0), curve_tables.cpp), so their gamma takes hess[0] only through nodes AT the value-time knot; the C oracle
    differentiates c D(t) / D(0) and so carries -PV hess[0] as well.  The host twin is held to the reference of ITS
    operation; the oracle's gamma differs from it by that term (DESIGN.md section 10 has the follow-up)."""
    times = SC.LOOKUP_TIMES
    host = E.lookup_curve(times, value_time_hess=True)
    book = E.lookup_book()
    sub_off = np.arange(book.n_trades + 1, dtype=np.int64)
    case = E.Case("lookup, hess[0] != 0", host, book, {})
    got = host_rates(interp, case, sub_off)
    share = R.worst_share(got, R.rates_reference(interp.value, host, book, sub_off), what=case.name)
    print(f"host twin, {interp.name}, {case.name}: share of the bound {share:.3f}")
    assert share <= 1.0
    rows = L.oracle_rows(interp.value, host, book)
    extra = -1e-8 * rows["pv"][:, None, None] * host.hess[0][None]
    gap = np.max(np.abs(rows["gamma"] - (got["gamma"] + extra)), axis=(1, 2)) / np.max(np.abs(rows["gamma"]), axis=(1, 2))
    weight = np.max(np.abs(extra), axis=(1, 2)) / np.max(np.abs(got["gamma"]), axis=(1, 2))
    assert np.max(gap) <= 1e-12 and np.median(weight) > 1e-3


@pytest.mark.parametrize("interp", E.SCHEMES, ids=lambda i: i.name)
def test_desks_alone_keep_their_bits_on_the_edge_books(interp):
    """The folding book's desks priced alone and in the book, bit for bit (the contract the GPU tests hold the device to)."""
    case = [c for c in E.rates_cases(interp) if c.name == "folding"][0]
    sub_off = case.layouts["pairs"]
    got = host_rates(interp, case, sub_off)
    for b, (lo, hi) in enumerate(zip(sub_off[:-1], sub_off[1:])):
        if hi == lo:
            continue
        alone = _native.subbook_ladders_host(interp.value, case.host.times, case.host.dfs, case.host.jac, case.host.hess,
                                             L.take(case.batch, int(lo), int(hi)), np.array([0, hi - lo]))
        assert L.same_bits({k: got[k][b:b + 1] for k in R.RATES_BLOCKS}, alone), f"desk {b}"
