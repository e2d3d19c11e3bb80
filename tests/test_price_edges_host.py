"""The cases of the per-trade pricing edge tests (tests/_price_edge_cases.py) checked without a GPU: that every case reaches the
kernel family, the fast-kernel instantiation and the general-kernel variant it is named for (`route_host`,
`curve_layout_host`), and that the C oracle (oracle/port.c) prices every new book inside the existing `bound_k` of the 60-digit
reference (tests/_ladder_reference.py), EVERY element, +0.0 where gross is 0 - which validates the reference and the books
before the GPU module (tests/test_gpu_price_edges.py) holds the kernels to the per-family bounds of tests/_price_reference.py.

Worst shares of `bound_k` observed for the C oracle (the test prints each): knot sweeps 0.079 (LINEAR_ZERO_RATES, the
(8, 8) curve), folding 0.055, long legs 0.018, lookups 0.062, row geometry 0.037; no case is refused.  The whole module
takes about 20 s, the references built."""
import numpy as np
import pytest

from adrates_amd import _native
from oracle import port

from . import _ladder_reference as R
from . import _price_edge_cases as PE
from . import _price_reference as PR

CASES = PE.cases()
IDS = [c.id for c in CASES]


def route(case, mask, per_trade, aggregate):
    h = case.host
    return _native.route_host(case.interp.value, h.times, h.dfs, h.jac, h.hess, case.batch, mask, per_trade=per_trade, aggregate=aggregate)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_case_reaches_the_kernels_it_is_named_for(case):
    layout, lds_rows = PE.layout_of(case.host)
    assert (layout, lds_rows) == PE.LAYOUTS[case.curve], (case.id, layout, lds_rows)
    assert case.host.jac.shape[1] <= 32 and case.batch.flt_weight is None
    live = case.batch.flt_alpha > 0.0
    assert np.array_equal(case.batch.flt_te[live], case.batch.flt_tp[live])          # no ratio node: the reference's domain
    cls = PE.row_class(case.batch)
    for name, mask, per_trade, aggregate in PE.REQUESTS:
        launches, cover = route(case, mask, per_trade, aggregate)
        assert np.all(cover == 1), (case.id, name)
        want = PE.families(case, mask, per_trade, aggregate)
        ran = {f: items for f, _, items, _ in launches}
        assert set(ran) == set(want), (case.id, name, launches)
        # the launches' sizes are those of the classes: one row per one-row trade, one list entry per general trade
        if "fast" in ran:
            assert ran["fast"] == np.count_nonzero(cls == "fast"), (case.id, name)
        if "general" in ran:
            assert ran["general"] == np.count_nonzero(want == "general"), (case.id, name)


def test_the_cases_cover_the_instantiations_and_both_general_variants():
    """Five fast instantiations / paths - (7, 5, hub) even and odd P, (7, 7), (8, 8), (12, 12), and the LINEAR_FWD_RATES
    compilation on three of them - and the general kernel with LDS-resident rows (README curve, legs of 385, 400 and 450
    coupons) and with rows streamed from L2 (the lookup tables; the (12, 12) curve's 385-coupon leg)."""
    fast, lds, l2 = set(), set(), set()
    for case in CASES:
        fams = set(PE.families(case, 7, True, False))
        layout, lds_rows = PE.LAYOUTS[case.curve]
        if fams & {"fast", "fast_chained"}:
            fast.add((layout[1:], case.host.jac.shape[1] % 2, case.interp == PE.LF))
        if "general" in fams:
            (lds if lds_rows else l2).add((case.curve, case.interp.name))
    assert {f[:2] for f in fast} == {((7, 5, 1), 0), ((7, 5, 1), 1), ((7, 7, 0), 1), ((8, 8, 0), 1), ((12, 12, 0), 0)}, fast
    assert {f[0] for f in fast if f[2]} == {(7, 5, 1), (7, 7, 0), (8, 8, 0)}
    assert {("README 32", s.name) for s in PE.SCHEMES} <= lds
    assert {("lookup", s.name) for s in PE.SCHEMES} | {("core21 epg 12", "FLAT_FWD_RATES")} <= l2
    chained = [c for c in CASES if c.name == "row geometry"][0]
    assert list(PE.row_class(chained.batch)) == ["fast"] * 3 + ["fast_chained"] * 6 + ["general"]
    rows = -(-np.diff(chained.batch.flt_off) // 32)
    assert [int(r) for r in rows[3:9]] == [PE.ROW_CHAINS[m] for m in PE.ROW_COUPONS[3:9]]
    seasoned = chained.batch.flt_tp[chained.batch.flt_off[1]:chained.batch.flt_off[2]]
    assert seasoned.size == 31 and np.count_nonzero(seasoned < 0.0) == 2
    assert {-1.0, 1.0} == set(chained.batch.flt_sign) == set(chained.batch.fix_sign) and np.all(chained.batch.spread != 0.0)
    fold = [c for c in CASES if c.name == "folding"][0]
    assert fold.batch.n_trades == 25                                            # one more than a block pass of 12 waves x 2 trades
    for size in PE.LAUNCH_SIZES:
        assert set(PE.row_class(PE.cycled_book(size))) == {"fast"}


def test_the_knot_sweep_covers_every_knot_and_interval():
    for case in CASES:
        if case.name != "knot sweep":
            continue
        x = np.unique(case.host.times)
        b = case.batch
        flows = b.fix_tp[b.fix_off[:-1][np.diff(b.fix_off) == 1]][:2 * x.size - 1]
        assert set(x[x > 0.0]) <= set(flows) and set(0.5 * (x[:-1] + x[1:])) <= set(flows) and flows.max() > x[-1]
        one = np.diff(b.flt_off) == 1
        ts, te = b.flt_ts[b.flt_off[:-1][one]], b.flt_tp[b.flt_off[:-1][one]]
        assert np.count_nonzero(one) == x.size - 2
        assert np.array_equal(np.searchsorted(x, te), np.searchsorted(x, ts) + 1)          # adjacent intervals
        assert np.all(b.spread[one] != 0.0) and {-1.0, 1.0} == set(b.flt_sign[one]) == set(b.fix_sign[~one][:flows.size])
        assert b.n_trades <= 400


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_oracle_prices_every_new_book_inside_the_bound(case):
    """oracle/port.c per trade against `rates_reference` under `bound_k`; the oracle may leave out only what it refuses
    (RuntimeError), and none of the bootstrapped-curve books."""
    h = case.host
    ref = PR.per_trade_reference(case.interp.value, h, case.batch)
    try:
        rows = port.price(case.interp.value, h.times, h.dfs, h.jac, h.hess, case.batch)
    except RuntimeError:
        assert case.curve == "lookup", f"the oracle refuses {case.id}"
        print(f"C oracle refuses {case.id}")
        return
    share = R.worst_share({k: np.asarray(rows[k]) for k in R.RATES_BLOCKS}, ref, what=f"oracle {case.id}")
    zero = sum(int(np.count_nonzero(np.asarray(d["gamma"].A) == 0)) for d in ref)
    total = sum(d["gamma"].V.size for d in ref)
    print(f"C oracle, {case.id}: share of the bound {share:.3f} (k up to {max(d['k'] for d in ref)}); "
          f"{zero} of {total} gamma entries have gross 0")
    assert share <= 1.0, case.id
    book = PR.book_reference(case.interp.value, h, case.batch)
    summed = {k: np.asarray(rows[k]).sum(0)[None] for k in R.RATES_BLOCKS}
    assert R.worst_share(summed, [book], what=f"oracle book {case.id}") <= 1.0


def test_the_family_bounds_read_only_the_inputs():
    """k per family on the README knot sweep: finite, larger for the families that count more, and built from the inputs
    alone (no result enters `trade_stats`)."""
    case = CASES[0]
    ref = PR.per_trade_reference(case.interp.value, case.host, case.batch)
    stats = PR.trade_stats(case.interp.value, case.host, case.batch)
    assert [s["n"] for s in stats] == [d["n_terms"] for d in ref]
    for fam in ("fast", "general", "lite"):
        ks = [PR.trade_k(fam, case.interp.value, s) for s in stats]
        assert all(20 <= k <= 200 for k in ks), (fam, min(ks), max(ks))
    assert all(PR.knot_trade_k(case.interp.value, s) >= PR.trade_k("lite", case.interp.value, s) - 2 * s["n"] for s in stats)
    book = PR.book_reference(case.interp.value, case.host, case.batch)
    ks = [PR.trade_k("fast", case.interp.value, s) for s in stats]
    k = PR.book_k(ref, book, ks, "delta", 0)
    assert all(0 <= int(v) <= max(ks) for v in k) and any(int(v) >= min(ks) for v in k)
