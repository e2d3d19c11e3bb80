"""The cases of the pricing edge tests beyond one pillar tile (tests/_price_wide_cases.py) checked without a GPU: that every
case takes the route it is named for under every request - the families of the plan and how often each trade is priced
(`route_host`, with the upload flags), the chunk count of the packed triangle (`curve_layout_host`) - and that the C oracle
(oracle/port.c) prices every new book inside the existing `bound_k` of the 60-digit reference (tests/_ladder_reference.py),
EVERY element, +0.0 where gross is 0: that validates the reference and the books at 33 to 97 pillars before the GPU module
(tests/test_gpu_price_wide.py) holds the wide and tiled launches to the bounds of tests/_price_reference.py.  Every test
prints its case's plan.

Worst shares of `bound_k` observed for the C oracle (the test prints each): dense lookup tables 0.078 (65 pillars), knot
sweeps 0.066 (40 pillars, FLAT_FWD_RATES), row geometry on 40 pillars 0.037; no case is refused.  The whole module takes
about 30 s, the references built."""
import numpy as np
import pytest

from oracle import port

from . import _ladder_reference as R
from . import _price_edge_cases as PE
from . import _price_reference as PR
from . import _price_wide_cases as PW

CASES = PW.cases()
IDS = [c.id for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_case_takes_the_route_it_is_named_for(case):
    P = case.host.jac.shape[1]
    assert 32 < P <= 97 and case.batch.flt_weight is None
    assert PW.chunks_of(case.host) == case.chunks, (case.id, PW.chunks_of(case.host))
    assert (case.route == "tiled") == (P > 64 or case.flags == PW.TILES)
    b = case.batch
    lagged = np.zeros(b.n_trades, dtype=bool)
    for t in range(b.n_trades):
        j = slice(b.flt_off[t], b.flt_off[t + 1])
        lagged[t] = np.any((b.flt_alpha[j] > 0.0) & (b.flt_te[j] != b.flt_tp[j]))
    assert list(np.nonzero(lagged)[0]) == list(case.lagged), case.id          # everything else is the reference's domain
    if case.lagged:
        d = case.domain
        assert d.n_trades == b.n_trades - 1 and np.array_equal(d.flt_tp, b.flt_tp[:d.flt_tp.size])
    for name, mask, per_trade, aggregate in PW.REQUESTS:
        launches, cover = PW.route(case, mask, per_trade, aggregate)
        print(f"{case.id}, {name}: {launches}")
        assert np.all(cover == 1), (case.id, name)
        want = PW.families(case, mask, per_trade, aggregate)
        assert {f for f, *_ in launches} == set(want), (case.id, name, launches)
        for fam in set(want):
            mine = [items for f, _, items, _ in launches if f == fam]
            if fam == "tiled":
                assert len(mine) == PW.tile_launches(P, mask) and set(mine) == {np.count_nonzero(want == fam)}, (case.id, name, launches)
            elif fam in ("wide", "lite_lag", "knot_lag"):
                assert mine == [np.count_nonzero(want == fam)], (case.id, name, launches)
    if case.lagged:
        # `any_ratio` is the batch's "some trade is lagged" (route.hpp, flag_lagged): the plan of a request without GAMMA shows
        # it - the lagged trade has a row of the lite kernel's payment-lag table - and with GAMMA one wide launch takes all
        assert "lite_lag" in {f for f, *_ in PW.route(case, 3)[0]}
        assert PW.route(case, 7)[0] == [("wide", "all", b.n_trades, -(-b.n_trades // PW.waves_per_block(case)))]


def test_the_cases_cover_the_wide_instantiations_and_the_tile_shapes():
    wide = [c for c in CASES if c.route == "wide"]
    # 7, 10 and 17 chunks: without the ratio-node path (log schemes, no lagged trade), with it (LINEAR_FWD_RATES; a lagged trade)
    assert {(c.chunks, c.interp == PE.LF, bool(c.lagged)) for c in wide} >= {(n, lf, lag) for n in (7, 10, 17) for lf, lag in
                                                                              ((False, False), (True, False), (False, True))}
    assert {c.host.jac.shape[1] for c in wide} >= {33, 41, 42, 49, 50, 63, 64, 40}
    assert PW.chunks_of(PW.dense_curve(51)) == 17                          # 49 is the last pillar count of 10 chunks
    geo = [c for c in wide if c.name == "row geometry"]
    assert len(geo) == 3
    for c in geo:
        assert PW.route(c, 7)[0] == [("wide", "all", 10, 2)]
        assert PW.route(c, 3)[0] == [("lite", "lite", 5, 1), ("wide", "nonlite", 1, 1)] and [f for f, *_ in PW.route(c, 1)[0]] == ["lite", "wide"]
        assert list(PW.families(c, 3, True, False)) == ["lite"] * 9 + ["wide"]
    tiled = [c for c in CASES if c.route == "tiled"]
    assert {(c.host.jac.shape[1], c.flags) for c in tiled} == {(65, 0), (96, 0), (97, 0), (33, 1), (64, 1), (40, 1)}
    sweep65 = [c for c in tiled if c.curve == "65 pillars"]
    assert [c.interp for c in sweep65] == list(PE.SCHEMES)
    for c in sweep65:
        n = c.batch.n_trades
        assert n == 195
        assert [len(PW.route(c, m)[0]) for m in (7, 3, 1)] == [6, 3, 1] and {f for f, *_ in PW.route(c, 7, False, True)[0]} == {"knot"}
    # the sparse curves leave most of gamma structurally empty, the dense ones nothing
    for c in CASES:
        live = np.asarray(c.host.hess)[1:] != 0.0
        assert np.all(live) if c.curve.startswith("dense") else np.mean(live) < 0.5, c.id


@pytest.mark.parametrize("P,flags", PW.LAUNCH_SHAPES)
def test_the_largest_launch_gives_a_wave_a_second_and_a_third_trade(P, flags):
    case = PW.launch_case(P, flags)
    sizes, cap, waves = PW.launch_sizes(case, 256)
    assert waves == (8 if case.route == "wide" and case.chunks <= 10 else 4)
    assert sizes[:2] == (1, 2) and sizes[2] == cap * waves and sizes[3:] == (sizes[2] + 1, 2 * sizes[2] + 1)
    for size in sizes:
        launches, cover = PW.route(case, 7, batch=PE.cycled_book(size))
        assert np.all(cover == 1) and {f for f, *_ in launches} == {case.route}
        blocks = launches[0][3]
        assert blocks == min(cap, -(-size // waves))
        print(f"{case.id}: {size} trades on {blocks} blocks of {waves} waves")
    # the grid strides over the trades: wave w takes trades w, w + grid, w + 2 grid ... - 2 grid + 1 trades give wave 0 three
    grid = cap * waves
    assert sizes[3] > grid and sizes[4] > 2 * grid and -(-sizes[4] // grid) == 3
    assert PW.launch_sizes(case, 128)[0][2] * 2 == sizes[2]                  # the sizes follow the device's CU count


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_oracle_prices_every_new_book_inside_the_bound(case):
    """oracle/port.c per trade against `rates_reference` under `bound_k`, and summed against the one-desk row; a lagged trade
    is outside the reference's domain: the oracle prices the other rows of that book to the same bits with and without it."""
    h, method = case.host, case.interp.value
    ref = PR.per_trade_reference(method, h, case.domain)
    rows = port.price(method, h.times, h.dfs, h.jac, h.hess, case.domain)
    got = {k: np.asarray(rows[k]) for k in R.RATES_BLOCKS}
    share = R.worst_share(got, ref, what=f"oracle {case.id}")
    zero = sum(int(np.count_nonzero(np.asarray(d["gamma"].A) == 0)) for d in ref)
    total = sum(d["gamma"].V.size for d in ref)
    print(f"C oracle, {case.id}: share of the bound {share:.3f} (k up to {max(d['k'] for d in ref)}); "
          f"{zero} of {total} gamma entries have gross 0")
    assert share <= 1.0, case.id
    book = PR.book_reference(method, h, case.domain)
    summed = {k: got[k].sum(0)[None] for k in R.RATES_BLOCKS}
    assert R.worst_share(summed, [book], what=f"oracle book {case.id}") <= 1.0
    if case.lagged:
        full = port.price(method, h.times, h.dfs, h.jac, h.hess, case.batch)
        n = case.domain.n_trades
        assert all(np.array_equal(PR.bits(np.asarray(full[k])[:n]), PR.bits(got[k])) for k in R.RATES_BLOCKS)
        assert np.any(np.asarray(full["gamma"])[n] != 0.0)


def test_the_wide_and_tiled_bounds_read_only_the_inputs():
    """k of `wide` is `general`'s less the merge, k of `tiled` is `general`'s; the wide reduction counts fewer adds than the
    block partials of the kernels of one tile."""
    case = CASES[0]
    stats = PR.trade_stats(case.interp.value, case.host, case.batch)
    for s in stats:
        g = PR.trade_k("general", case.interp.value, s)
        assert PR.trade_k("wide", case.interp.value, s) == g - 1 and PR.trade_k("tiled", case.interp.value, s) == g
    assert PR.aggregate_sums(26, 4, wide=True) == 26 + 12 + 1 and PR.aggregate_sums(26, 4) == 26 + 18 + 1
    assert PR.aggregate_sums(2049, 256, wide=True) == 2049 + 12 + 4
