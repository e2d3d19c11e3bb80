"""`adr_price` on trades with payment lag and per-coupon weights against the plain 60-digit reference
(tests/_ladder_reference.py, "Ratio terms"), EVERY element of pv, delta and gamma on the bound of its kernel family
(tests/_price_reference.py: `fast_lag`, `fast_lag_chained`, `lite_lag`, `knot_lag` and the general kernel's ratio nodes):
|got - value| <= k 2^-53 gross, and +0.0 where gross is 0.  The cases (tests/_price_lag_cases.py; tests/test_price_lag_host.py
asserts on the CPU which kernel prices each trade under each request) run under the six requests of
tests/_price_edge_cases.py; the aggregate is held to the reference's one-desk row with the reduction's count and the knot
passes' sums added, and the blocks a request does not ask for are not returned, or +0.0 in the aggregate.

Two launches.  Every launch runs twice, bit for bit - with one exception: an aggregate-only GAMMA request on a book whose ratio
nodes couple knots more than 16 apart on the compact grid.  The knot pass over the payment-lag rows keeps 16 pair bands per
knot in LDS and sends every pair farther apart to a dense overflow matrix in global memory, which all waves of the launch fill
with atomic adds (kernels_lite.hip, `pair_add`): the order of those adds, and with it the last bits of agg_gamma, depends on
scheduling.  There both runs are held to the bound (which counts any order of the adds) and not to each other; a book without
such pairs must repeat its bits.

Mirrors.  The fast kernel's payment-lag variant expands its packed ladder as the plain kernel does, both mirrors of a pair
from one number, and PATCHES the elements the packed ladder has no entry for from the special nodes' stash, (om v_r) v_c and
(om v_c) v_r each by its own product: gamma[p][q] and gamma[q][p] have the same bits on the packed pairs
(`_price_lag_cases.packed_pairs`: what one knot interval can create), per trade and in the aggregate of a plan whose launches
are all fast kernels.  The general kernel writes the blocks below the diagonal from the registers of their mirrors: the same
bits for every pair outside the diagonal 4 x 4 blocks.  Elsewhere - inside those blocks, on the patched elements, and in the
knot passes' projection, which forms every entry on its own - both sides are held to the bound.

Guarded buffers: `price_dev` on the structure book at 32 pillars (the fast variant) and 31 (the general kernel), 16 guard words
behind pv, delta, gamma and agg.  Launch shape: the one-row lagged trades of 1, 8 and 32 coupons cycled to launches of 1, 2,
one trade per group of the full grid, that plus 1 and twice that plus 1 (the grid read off the plan for the device's CU count),
and the same for a two-row chain of 33 coupons: every copy has the bits of its trade in the three-trade (one-trade) launch,
whose rows are held to the bound - the special nodes' stash belongs to a wave and a group, not to a position.

Worst shares of the bound observed on an MI355X, per family over all cases and schemes (every test prints its own):
  fast_lag 0.060   fast_lag_chained 0.009   general, ratio nodes 0.060 (0.028 under LINEAR_FWD_RATES)   lite_lag 0.113
  the plain trades of these books: fast 0.064, lite 0.025;  the base launches of the launch-shape check 0.035 / 0.004
  aggregate through the block partials 0.026   through the knot passes 0.011 (16 requests fill the overflow matrix)
The module found rounding dust on structural zeros under LINEAR_FWD_RATES in two places, both fixed with it: the general
kernel's ratio nodes per trade (2.5e-23 at gamma[0][1] to -4.0e-19 at gamma[2][16] on four books; kernels_general.hip,
`lindf_knots` and `add_cross`) and the knot pass over the payment-lag rows (1.6e-22 at agg_gamma[1][2] of the counts book;
kernels_lite.hip) - each wrote a date's own cross products twice with opposite signs.  No share above 1 under the log
schemes.  DESIGN.md section 33 has the k table, the instantiations reached and the mutations.  The slowest case takes 1.0 s
(the counts book, 17 trades of up to 391 coupons), the module 9 s; the launch-shape checks price up to 8193 trades."""
import time

import numpy as np
import pytest

from adrates_amd import _native

from . import _ladder_reference as R
from . import _price_edge_cases as PE
from . import _price_lag_cases as PL
from . import _price_reference as PR

pytestmark = pytest.mark.gpu

CASES = PL.cases()
N_CASES = 25
AGG = ("agg_pv", "agg_delta", "agg_gamma")
GUARD = 16
FAST = ("fast", "fast_chained", "fast_lag", "fast_lag_chained")


def price(ctx, dc, dt, mask, per_trade, aggregate):
    return _native.price(ctx, dc, dt, want_value=bool(mask & 1), want_delta=bool(mask & 2), want_gamma=bool(mask & 4),
                         per_trade=per_trade, aggregate=aggregate)


def device_curve(ctx, case):
    h = case.host
    return _native.DeviceCurve(ctx, case.interp.value, h.times, h.dfs, h.jac, h.hess)


def mirrors_agree(g, pairs):
    """gamma [..., P, P]: the entries of ``pairs`` have the bits of their mirrors."""
    g = np.asarray(g)
    return np.array_equal(PR.bits(g)[..., pairs], PR.bits(np.swapaxes(g, -1, -2))[..., pairs])


def aggregate_count(case, fams, launches, stats, n, Kc):
    """The adds between the trades' numbers and the aggregate: the block partials and their reduction, and the knot passes'."""
    sums = PR.aggregate_sums(n, sum(b for f, *_, b in launches if f not in ("knot", "knot_lag")))
    for fam, count in (("knot", PR.knot_sums), ("knot_lag", PR.knot_lag_sums)):
        if fam in fams:
            sums += count([stats[i] for i in np.nonzero(fams == fam)[0]], Kc, sum(b for f, *_, b in launches if f == fam))
    return sums


@pytest.mark.parametrize("which", range(N_CASES))
def test_every_element_of_every_request(gpu_ctx, which):
    case = CASES[which]
    t0 = time.perf_counter()
    h, method, batch = case.host, case.interp.value, case.batch
    n = batch.n_trades
    ref = PR.per_trade_reference(method, h, batch)
    book = PR.book_reference(method, h, batch)
    stats = PR.trade_stats(method, h, batch)
    Kc = R.compact_count(h.times)
    packed = PL.packed_pairs(h) if PE.LAYOUTS[case.curve][0][0] else None
    dc = device_curve(gpu_ctx, case)
    checked, worst = [], {}
    with _native.DeviceTrades(gpu_ctx, batch) as dt:
        for name, mask, per_trade, aggregate in PE.REQUESTS:
            what = f"{case.id}, {name}"
            fams = PE.families(case, mask, per_trade, aggregate)
            launches, cover = PL.route(case, mask, per_trade, aggregate)
            assert np.all(cover == 1) and {f for f, *_ in launches} == set(fams), (what, launches)
            got = price(gpu_ctx, dc, dt, mask, per_trade, aggregate)
            again = price(gpu_ctx, dc, dt, mask, per_trade, aggregate)
            ordered = not (case.far_pairs and not per_trade and mask & 4 and "knot_lag" in fams)      # module docstring, "Two launches"
            runs = [got]
            if ordered:
                assert PR.same_bits(got, again), f"{what}: two launches differ"
            else:
                assert PR.same_bits(got, again, ("agg_pv", "agg_delta")), f"{what}: two launches differ in pv or delta"
                runs.append(again)
            ks = PR.case_ks(method, h, batch, ref, fams)
            if per_trade:
                assert set(got) - set(AGG) == {b for b, bit in zip(PR.BLOCKS, (1, 2, 4)) if mask & bit}, what
                for fam in sorted(set(fams)):
                    rows = np.nonzero(fams == fam)[0]
                    share = 0.0
                    for block in PR.BLOCKS:
                        if block not in got:
                            continue
                        key = (block, fam, PR.bits(np.asarray(got[block])[rows]).tobytes())
                        known = [s for k_, s in checked if k_ == key]
                        if not known:
                            known = [PR.rows_share({block: got[block]}, ref, ks, what, rows)]
                            checked.append((key, known[0]))
                        share = max(share, known[0])
                    print(f"{what}: {fam} ({rows.size} trades, k {min(ks[i] for i in rows)} to {max(ks[i] for i in rows)}): share of the bound {share:.3f}")
                    assert share <= 1.0, (what, fam)
                    worst[fam] = max(worst.get(fam, 0.0), share)
                    if mask & 4:
                        g = got["gamma"][rows]
                        if fam in ("fast", "fast_chained"):
                            assert mirrors_agree(g, np.ones(g.shape[1:], dtype=bool)), f"{what}: the fast kernels' mirrors differ"
                        else:
                            assert mirrors_agree(g, PL.mirrored_pairs(case, fam)), f"{what}: {fam}: mirrors written from one number differ"
            else:
                assert set(got) == set(AGG), what
            if aggregate:
                sums = aggregate_count(case, fams, launches, stats, n, Kc)
                zero = [b for b, need in zip(PR.BLOCKS, (0, 6, 4)) if need and not mask & need]
                label = "aggregate of " + "+".join(sorted(set(fams)))
                for run in runs:
                    share = PR.book_share({k: np.asarray(run[k]) for k in AGG}, ref, book, ks, sums, zero, what)
                    print(f"{what}: {label} (sums {sums}{'' if ordered else ', atomic overflow matrix'}): share of the bound {share:.3f}")
                    assert share <= 1.0, what
                    worst[label] = max(worst.get(label, 0.0), share)
                if mask & 4 and packed is not None and set(fams) <= set(FAST):
                    pairs = packed if set(fams) & {"fast_lag", "fast_lag_chained"} else np.ones_like(packed)
                    assert mirrors_agree(got["agg_gamma"], pairs), f"{what}: the aggregate's mirrors differ"
    dc.close()
    print(f"{case.id}: worst shares " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())) + f"; {time.perf_counter() - t0:.1f} s")


@pytest.mark.parametrize("label", ("README 32", "31 pillars"))
def test_nothing_is_written_behind_the_buffers(gpu_ctx, label):
    """`price_dev` on the structure book into buffers with 16 guard words behind each: the guards are intact, what is in front
    of them has the bits of the blocking call, and with no per-trade gamma buffer the aggregate has the same bits."""
    import torch
    case = [c for c in CASES if c.name == "structure" and c.curve == label and c.interp == PE.LZ][0]
    fams = set(PE.families(case, 7, True, True))
    assert fams == ({"fast", "fast_lag"} if label == "README 32" else {"fast", "general"}), fams
    batch, P = case.batch, case.host.jac.shape[1]
    n = batch.n_trades
    dev = torch.device("cuda", 0)
    sizes = dict(pv=n, delta=n * P, gamma=n * P * P, agg=1 + P + P * P)
    dc = device_curve(gpu_ctx, case)
    with _native.DeviceTrades(gpu_ctx, batch) as dt:
        full = price(gpu_ctx, dc, dt, 7, True, True)
        want = dict(pv=full["pv"], delta=full["delta"].ravel(), gamma=full["gamma"].ravel(),
                    agg=np.concatenate([[full["agg_pv"]], full["agg_delta"], full["agg_gamma"].ravel()]))
        for with_gamma in (True, False):
            bufs = {k: torch.full((m + GUARD,), -7.25, dtype=torch.float64, device=dev) for k, m in sizes.items()}
            _native.price_dev(gpu_ctx, dc, dt, 7, bufs["pv"].data_ptr(), bufs["delta"].data_ptr(),
                              bufs["gamma"].data_ptr() if with_gamma else 0, bufs["agg"].data_ptr())
            gpu_ctx.sync()
            for k, m in sizes.items():
                out = bufs[k].cpu().numpy()
                assert np.all(out[m:] == -7.25), f"{label}, {k}: a guard word was written"
                if k == "gamma" and not with_gamma:
                    assert np.all(out == -7.25)
                    continue
                assert np.array_equal(PR.bits(out[:m]), PR.bits(want[k])), (label, k, with_gamma)
    dc.close()


@pytest.mark.parametrize("chain", (False, True), ids=("one row", "a chain of two rows"))
def test_a_lagged_trade_keeps_its_bits_at_every_position_and_launch_size(gpu_ctx, chain):
    """The lagged trades of 1, 8 and 32 coupons (or the chain of 33) in launches of 1, 2, w, w + 1 and 2 w + 1 trades (w: one
    trade per group of the full grid): every copy has the bits of its trade in the base launch, which is held to the bound."""
    import torch
    case = PL.launch_case(chain=chain)
    h, method = case.host, case.interp.value
    family = "fast_lag_chained" if chain else "fast_lag"
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    sizes, cap = PL.launch_sizes(case, n_cu, chain)
    ref = PR.per_trade_reference(method, h, case.batch)
    period = case.batch.n_trades
    ks = PR.case_ks(method, h, case.batch, ref, [family] * period)
    dc = device_curve(gpu_ctx, case)
    with _native.DeviceTrades(gpu_ctx, case.batch) as dt:
        base = price(gpu_ctx, dc, dt, 7, True, False)
    share = PR.rows_share(base, ref, ks, case.id)
    print(f"{case.id}: the base launch of {period}, share of the bound {share:.3f}; launches of {sizes} trades on at most {cap} blocks ({n_cu} CUs)")
    assert share <= 1.0
    assert all(s["ratio"] for s in PR.trade_stats(method, h, case.batch))
    P = h.jac.shape[1]
    for size in sizes:
        book = PL.cycled_book(size, chain)
        launches, cover = PL.route(case, 7, n_cu=n_cu, batch=book)
        assert {f for f, *_ in launches} == {family} and np.all(cover == 1), (size, launches)
        if not chain:
            assert launches[0][3] == min(cap, -(-(-(-size // 2)) // 8)), (size, launches)
        with _native.DeviceTrades(gpu_ctx, book) as dt:
            got = price(gpu_ctx, dc, dt, 7, True, False)
        assert got["gamma"].shape == (size, P, P) and set(got) == set(PR.BLOCKS)
        for block, rows in got.items():
            b = PR.bits(rows).reshape(size, -1)
            for r in range(min(period, size)):
                same = np.all(b[r::period] == PR.bits(base[block][r]).reshape(1, -1), axis=1)
                assert np.all(same), (case.id, size, block, f"copy {r + period * int(np.argmin(same))} of trade {r}")
        del got
    dc.close()


def test_the_case_count():
    assert len(CASES) == N_CASES
