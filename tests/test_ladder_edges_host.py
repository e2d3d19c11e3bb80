"""The sub-book ladder host twins (adr_subbook_ladders_host, adr_credit_subbook_ladders_host) and the C oracle on the hand-made
edge books (tests/_ladder_edge_cases.py) against the plain 60-digit reference (tests/_ladder_reference.py), EVERY element:
|got - value| <= k 2^-53 gross with k derived in the reference's docstring, and +0.0 where gross is 0.  No GPU.

Worst observed shares of the bound over all cases and schemes (each test prints its own):
  rates   host twin 0.074   C oracle 0.062
  credit  host twin 0.023   C oracle 0.029
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
