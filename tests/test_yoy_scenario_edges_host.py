"""The inflation scenario host twins (adr_yoy_scenario_pv_host and the per-swap rows and desk rows of
adr_yoy_scenario_subbook_pv_host) on the hand-made edge books (tests/_yoy_scenario_edge_cases.py) against the plain 60-digit
reference (tests/_yoy_scenario_reference.py), EVERY element: |got - value| <= k 2^-53 gross with k derived in the reference's
docstring, and +0.0 where gross is 0.  The reference itself is held to the older one (C oracle + MpYoY) on the older cases.
No GPU.

Worst observed share of the bound over all cases, launch shapes and scheme pairs (each test prints its own, with the place):
host twin 0.080 (main, the coupon with ts = 0.25 and te = 0.125, both before the first pillar, LINEAR_FWD_RATES discounting,
LINEAR_ZERO_RATES inflation); k runs from 7 to 1 592.  No element left the bound, none with gross == 0 was -0.0, and no
rounding was recounted.  On the periods of a day and of 2^-12 years the worst share is 0.041, the same error against |value|
at most 1.7e-11 (`test_short_periods_on_record`).

One-line mutations of `make_slot` / `apply_slot` / `host_chunks`, each built into a scratch host library, run and reverted; the
first column is `test_host_twin_every_element` (6), `test_sub_books_threads_and_single_rows_keep_their_bits` (6) and
`test_short_periods_on_record` (1), the last the 73 tests of test_yoy_scenarios_host.py and test_yoy_subbook_host.py:
  a   `&& TS[i-1] != pte` dropped from the `prev` test                            12 fail      73 pass
  b   `&& TP[i-1] > 0` dropped from it                                            12 fail      73 pass
  c   `cpn &&` dropped from the kFixIsCpnTp condition                             13 pass      73 pass
  c'  `if (xt == fabs(tp))`                                                       12 fail      73 pass
  d   `Acc::le` reset where j % 64 == 0                                           12 fail      73 pass
  e   the coupon mask `tp >= 0`; the fixed-flow mask `xt >= 0`                    12 fail each 17 fail; 16 fail
  f   `is = N` where S_infl == 1                                                  6 fail       2 fail
  g   `a.le = le` moved out of the `!kTsIsTe` branch (0.0 for such a coupon)      13 pass      73 pass
  g+a both                                                                        12 fail      73 pass
c cannot show: without a live coupon `tp` is 0.0 or the dead coupon's own tp <= 0, and xt > 0; c' is the nearest edit that can (the
fixed flow at |tp| of a dead coupon).  g cannot show alone: only the NEXT index could read what a ts == te coupon wrote to
`Acc::le`, and conjunct a never lets it; with a dropped too it does."""
import numpy as np
import pytest

from adrates_amd import _native

from . import _scenario_cases as SC
from . import _yoy_scenario_cases as YS
from . import _yoy_scenario_edge_cases as E
from . import _yoy_scenario_reference as R

PAIRS = [(dm, im) for dm in E.DISC_SCHEMES for im in E.INFL_SCHEMES]
pair_id = lambda p: f"disc {E.NAMES[p[0]]} / infl {E.NAMES[p[1]]}"
SHORT = ("a period of one day", "a period of 2^-12 years", "a period of 2^-12 years across a pillar", "a leg of 2^-12-year periods")


def calls(case):
    """``(label, dfs, b)``: the case's joint pairs and, for the main case, a shared row on either side."""
    yield case.name, case.dfs, case.b
    if case.name == "main":
        for label, d, r in E.SHAPES:
            yield f"main, {label}", case.dfs[d], case.b[r]


def reference(dm, im, case, dfs, b):
    return R.reference(dm, case.times, dfs, im, case.T, b, case.fixed, case.book)


def host(dm, im, case, dfs, b, **kw):
    return _native.yoy_scenario_pv_host(dm, case.times, dfs, im, case.T, b, case.fixed, case.book, per_trade=True, **kw)


def test_the_books_take_the_branches_they_are_named_for():
    E.check_books()


@pytest.mark.parametrize("pair", PAIRS, ids=pair_id)
def test_host_twin_every_element(native_lib, pair):
    dm, im = pair
    top = (0.0, "")
    for case in E.cases():
        for label, dfs, b in calls(case):
            ref = reference(dm, im, case, dfs, b)
            got = host(dm, im, case, dfs, b)
            share, i, s, rel = ref.worst(got["pv"], label)
            print(f"host twin, {pair_id(pair)}, {label}: worst share of the bound {share:.3f} at swap {i} ({case.names[i]}), scenario {s} "
                  f"(k {ref.k.min()} .. {ref.k.max()})")
            assert share <= 1.0, (label, case.names[i], s)
            assert np.array_equal(got["book_pv"], SC.book_sum(got["pv"])), label
            top = max(top, (share, f"{label}, swap {i} ({case.names[i]}), scenario {s}"))
    print(f"host twin, {pair_id(pair)}: worst share {top[0]:.3f} at {top[1]}")


@pytest.mark.parametrize("pair", PAIRS, ids=pair_id)
def test_sub_books_threads_and_single_rows_keep_their_bits(native_lib, pair):
    """The sub-book twin's per-swap rows on the same bound; its desk rows the fixed-order sum of those rows over desks cut inside
    a chunk, an empty desk +0.0; thread counts 1, 3 and 16; the last scenario priced alone."""
    dm, im = pair
    for case in E.cases():
        ref = reference(dm, im, case, case.dfs, case.b)
        first = host(dm, im, case, case.dfs, case.b, n_threads=1)
        for threads in (3, 16):
            again = host(dm, im, case, case.dfs, case.b, n_threads=threads)
            assert np.array_equal(again["pv"], first["pv"]) and np.array_equal(again["book_pv"], first["book_pv"]), (case.name, threads)
        s = case.dfs.shape[0] - 1
        one = host(dm, im, case, case.dfs[s], case.b[s])
        assert np.array_equal(one["pv"][0], first["pv"][s]) and one["book_pv"][0] == first["book_pv"][s], case.name
        for threads in (1, 3):
            sub = _native.yoy_scenario_subbook_pv_host(dm, case.times, case.dfs, im, case.T, case.b, case.fixed, case.book, case.sub_off,
                                                       per_trade=True, n_threads=threads)
            assert ref.share(sub["pv"], case.name) <= 1.0 and np.array_equal(sub["pv"], first["pv"]), case.name
            for d, (lo, hi) in enumerate(zip(case.sub_off[:-1], case.sub_off[1:])):
                assert np.array_equal(sub["sub_pv"][d], SC.book_sum(sub["pv"][:, lo:hi])), (case.name, d)
                assert hi > lo or not np.any(sub["sub_pv"][d]) and not np.any(np.signbit(sub["sub_pv"][d]))


@pytest.mark.parametrize("case", YS.cases(), ids=repr)
def test_the_reference_agrees_with_the_older_one(case):
    """`_yoy_scenario_cases.reference` (C oracle for the fixed legs + MpYoY for the coupons, per scenario) on the whole older
    case table, at that reference's own accuracy: a swap without fixed flows is MpYoY's 60-digit value rounded to float64 once,
    so it lies within 2^-53 |value|; one with fixed flows adds the oracle's float64 discounting and one float64 add, which
    `bound_k` covers (it counts every rounding of pay * D(xt), the sum and the join)."""
    times, dfs, T, b = YS.scenario_pairs(case)
    fixed = YS.fixed_legs(case)
    ref = R.reference(case.disc[0], times, dfs, case.infl[0], T, b, fixed, case.book)
    old = YS.reference(case)
    assert ref.share(old, repr(case)) <= 1.0
    unit = R.mpf(2) ** -53
    plain = np.flatnonzero(np.diff(fixed[0]) == 0)
    assert plain.size
    for i in plain:
        for s in range(dfs.shape[0]):
            assert abs(R._mp(old[s, i]) - ref.value[i][s]) <= unit * abs(ref.value[i][s]), (case, case.names[i], s)


def test_short_periods_on_record(native_lib):
    """`y = exp(le - ls) - 1` for periods of a day and of 2^-12 years: the worst share of the bound and, for reading only, the
    same error against |value| (whether exp(x) - 1 should become expm1 is not decided here)."""
    case = E.cases()[0]
    idx = [case.names.index(n) for n in SHORT]
    for dm, im in PAIRS:
        ref = reference(dm, im, case, case.dfs, case.b)
        got = host(dm, im, case, case.dfs, case.b)["pv"]
        unit = R.mpf(2) ** -53
        worst = max((float(abs(R._mp(got[s, i]) - ref.value[i][s]) / (int(ref.k[i, s]) * unit * ref.gross[i][s])),
                     float(abs(R._mp(got[s, i]) - ref.value[i][s]) / abs(ref.value[i][s])), case.names[i], s)
                    for i in idx for s in range(ref.S) if ref.value[i][s] != 0)
        rel = max(float(abs(R._mp(got[s, i]) - ref.value[i][s]) / abs(ref.value[i][s])) for i in idx for s in range(ref.S) if ref.value[i][s] != 0)
        print(f"short periods, {pair_id((dm, im))}: worst share {worst[0]:.3f} ({worst[2]}, scenario {worst[3]}; {worst[1]:.1e} of |value| "
              f"there); worst error against |value| {rel:.1e}")
        assert worst[0] <= 1.0
