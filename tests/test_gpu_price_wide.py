"""`adr_price` beyond one pillar tile against the plain 60-digit reference (tests/_ladder_reference.py), EVERY element of pv,
delta and gamma on the bound of its kernel family (tests/_price_reference.py, `wide` and `tiled`):
|got - value| <= k 2^-53 gross, and +0.0 where gross is 0.  The cases (tests/_price_wide_cases.py; tests/test_price_wide_host.py
asserts on the CPU which route and which chunk count each takes) run under the six requests of tests/_price_edge_cases.py,
every launch twice, bit for bit; the aggregate is held to the reference's one-desk row with the reduction's count added, and
the blocks a request does not ask for are +0.0.  Mirrors: the wide kernel holds the upper triangle alone and `wide_store_map`
writes both mirrors of an off-diagonal pair from one packed entry, so gamma[p][q] and gamma[q][p] have the same bits for
every p != q, per trade and in the aggregate; on tiles that holds for every pair outside the diagonal 4 x 4 blocks (an
off-diagonal tile is written twice from the same registers, as are the off-diagonal blocks of a diagonal tile), and inside
them both sides are held to the bound.  The knot pass's projection forms every entry on its own: both sides on the bound.
The dense 33- and 64-pillar tables and the 40-pillar sweep are priced on both routes, each held to the bound, not to each
other.  A lagged trade (outside the reference's domain) puts the other 26 trades of its book on the wide kernel's ratio-node
instantiations; the lagged row itself and the aggregate of that book are held to oracle/port.c on the scale of tests/_parity.py.

Guarded buffers: `price_dev` at 33, 49, 63 and 65 pillars and at 64 on tiles, 16 guard words behind pv, delta, gamma and agg -
the scalar-store path of an odd pillar count, the entries beyond P * P of the last band, the partial last tile.
Launch shape: the three one-row trades of the row geometry book cycled to launches of 1, 2, one trade per wave of the full
grid, that plus 1 and twice that plus 1 (from the plan's block count for the device's CU count) - every copy has the bits of
its trade in the three-trade launch, whose rows are held to the bound: the staged ladder of the wide kernel is stored during
the wave's next trade, and after the last one.

Worst shares of the bound observed on an MI355X, per family over all cases and schemes (every test prints its own):
  wide 0.191 (knot sweep, 40 pillars, LINEAR_FWD_RATES; 0.143 on the dense tables)   tiled 0.148 (knot sweep, 65 pillars)
  lite, 64-pillar instantiations 0.171   the three-trade launches of the launch-shape check 0.097 / 0.091 / 0.086
  aggregate through `reduce_wide_kernel` 0.020   through the tile reductions 0.017   through the knot pass 0.011
No share above 1, +0.0 on every structural zero (687 386 of the 823 875 gamma entries of the 65-pillar sweep), no finding;
DESIGN.md section 30 has the k table, the instantiations reached and the four mutations this module fails (one of which -
an entry of `wide_store_map` redirected to its neighbour - the older tests of these routes pass).  The slowest case takes
2.0 s, the module 19 s."""
import time

import numpy as np
import pytest

from adrates_amd import _native
from oracle import port

from . import _ladder_edge_cases as E
from . import _ladder_reference as R
from . import _price_edge_cases as PE
from . import _price_reference as PR
from . import _price_wide_cases as PW
from ._parity import assert_batch_parity

pytestmark = pytest.mark.gpu

CASES = PW.cases()
N_CASES = 38
AGG = ("agg_pv", "agg_delta", "agg_gamma")
GUARD = 16


def price(ctx, dc, dt, mask, per_trade, aggregate):
    return _native.price(ctx, dc, dt, want_value=bool(mask & 1), want_delta=bool(mask & 2), want_gamma=bool(mask & 4),
                         per_trade=per_trade, aggregate=aggregate)


def device_curve(ctx, case):
    h = case.host
    return _native.DeviceCurve(ctx, case.interp.value, h.times, h.dfs, h.jac, h.hess, flags=case.flags)


def mirrors_agree(g, pairs):
    """gamma [..., P, P]: the entries of ``pairs`` have the bits of their mirrors."""
    g = np.asarray(g)
    return np.array_equal(PR.bits(g)[..., pairs], PR.bits(np.swapaxes(g, -1, -2))[..., pairs])


def partial_blocks(case, launches):
    """Blocks one reduction sums: all of a wide plan's, one launch's on tiles (every tile launch has its own reduction)."""
    mine = [b for f, *_, b in launches if f not in ("knot", "knot_lag")]
    return (max(mine) if case.route == "tiled" else sum(mine)) if mine else 0


@pytest.mark.parametrize("which", range(N_CASES))
def test_every_element_of_every_request(gpu_ctx, which):
    case = CASES[which]
    t0 = time.perf_counter()
    h, method, batch, domain = case.host, case.interp.value, case.batch, case.domain
    n = domain.n_trades                                   # the rows of the reference's domain come first
    ref = PR.per_trade_reference(method, h, domain)
    book = PR.book_reference(method, h, domain)
    stats = PR.trade_stats(method, h, domain)
    Kc = R.compact_count(h.times)
    pairs = PW.mirrored_pairs(case)
    oracle = port.price(method, h.times, h.dfs, h.jac, h.hess, batch) if case.lagged else None
    dc = device_curve(gpu_ctx, case)
    checked, worst = [], {}
    with _native.DeviceTrades(gpu_ctx, batch) as dt:
        for name, mask, per_trade, aggregate in PW.REQUESTS:
            what = f"{case.id}, {name}"
            fams = PW.families(case, mask, per_trade, aggregate)
            launches, cover = PW.route(case, mask, per_trade, aggregate)
            assert np.all(cover == 1) and {f for f, *_ in launches} == set(fams), (what, launches)
            got = price(gpu_ctx, dc, dt, mask, per_trade, aggregate)
            again = price(gpu_ctx, dc, dt, mask, per_trade, aggregate)
            assert PR.same_bits(got, again), f"{what}: two launches differ"
            fams = fams[:n]
            ks = PR.case_ks(method, h, domain, ref, fams)
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
                    assert mirrors_agree(got["gamma"], pairs), f"{what}: mirrors written from one number differ"
                if case.lagged:
                    lag = list(case.lagged)
                    assert_batch_parity({k: np.asarray(v)[lag] for k, v in got.items() if k not in AGG},
                                        {k: np.asarray(v)[lag] for k, v in oracle.items()}, batch.notional[lag])
            if aggregate and case.lagged:
                assert np.allclose(got["agg_pv"], oracle["pv"].sum(), rtol=1e-10, atol=1e-3), what
                assert np.allclose(got["agg_delta"], oracle["delta"].sum(0), rtol=1e-10, atol=1e-6), what
                want_gamma = oracle["gamma"].sum(0) if mask & 4 else np.zeros_like(got["agg_gamma"])
                assert np.allclose(got["agg_gamma"], want_gamma, rtol=1e-10, atol=1e-9) and not np.any(np.signbit(got["agg_gamma"]) & (want_gamma == 0.0)), what
            elif aggregate:
                blocks = partial_blocks(case, launches)
                sums = PR.aggregate_sums(n, blocks, wide=case.route == "wide")
                if "knot" in fams:
                    sums += PR.knot_sums([stats[i] for i in np.nonzero(fams == "knot")[0]], Kc, sum(b for f, *_, b in launches if f == "knot"))
                zero = [b for b, need in zip(PR.BLOCKS, (0, 6, 4)) if need and not mask & need]
                share = PR.book_share({k: np.asarray(got[k]) for k in AGG}, ref, book, ks, sums, zero, what)
                label = "aggregate of " + "+".join(sorted(set(fams)))
                print(f"{what}: {label} (sums {sums}): share of the bound {share:.3f}")
                assert share <= 1.0, what
                worst[label] = max(worst.get(label, 0.0), share)
                if mask & 4 and "knot" not in fams:
                    assert mirrors_agree(got["agg_gamma"], pairs), f"{what}: the aggregate's mirrors differ"
    dc.close()
    print(f"{case.id}: worst shares " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())) + f"; {time.perf_counter() - t0:.1f} s")


@pytest.mark.parametrize("P,flags", PW.GUARDED)
def test_nothing_is_written_behind_the_buffers(gpu_ctx, P, flags):
    """`price_dev` on the dense table of P pillars into buffers with 16 guard words behind each: the guards are intact, what
    is in front of them has the bits of the blocking call, and with no per-trade gamma buffer the aggregate has the same bits."""
    import torch
    case = PW.launch_case(P, flags)
    batch = E.lookup_book()
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
                assert np.all(out[m:] == -7.25), f"{P} pillars, {k}: a guard word was written"
                if k == "gamma" and not with_gamma:
                    assert np.all(out == -7.25)
                    continue
                assert np.array_equal(PR.bits(out[:m]), PR.bits(want[k])), (P, flags, k, with_gamma)
    dc.close()


@pytest.mark.parametrize("P,flags", PW.LAUNCH_SHAPES)
def test_a_trade_keeps_its_bits_at_every_position_and_launch_size(gpu_ctx, P, flags):
    """The one-row trades of the row geometry book (1, 31 and 32 coupons) on the dense table of P pillars: the three-trade
    launch is held to the bound, and in launches of 1, 2, w, w + 1 and 2 w + 1 trades (w: one trade per wave of the full grid)
    every copy of a trade has those bits - first, second or third trade of its wave, stored by the next trade or by the final
    flush.  Nothing in the kernels makes a trade's arithmetic depend on its position."""
    import torch
    case = PW.launch_case(P, flags)
    h, method = case.host, case.interp.value
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    sizes, cap, waves = PW.launch_sizes(case, n_cu)
    ref = PR.per_trade_reference(method, h, case.batch)
    ks = PR.case_ks(method, h, case.batch, ref, [case.route] * 3)
    dc = device_curve(gpu_ctx, case)
    with _native.DeviceTrades(gpu_ctx, case.batch) as dt:
        base = price(gpu_ctx, dc, dt, 7, True, False)
    share = PR.rows_share(base, ref, ks, case.id)
    print(f"{case.id}: the three-trade launch, share of the bound {share:.3f}; launches of {sizes} trades on at most {cap} blocks of {waves} waves ({n_cu} CUs)")
    assert share <= 1.0
    for size in sizes:
        book = PE.cycled_book(size)
        launches, _ = PW.route(case, 7, n_cu=n_cu, batch=book)
        assert {f for f, *_ in launches} == {case.route} and launches[0][3] == min(cap, -(-size // waves)), (size, launches)
        with _native.DeviceTrades(gpu_ctx, book) as dt:
            got = price(gpu_ctx, dc, dt, 7, True, False)
        assert got["gamma"].shape == (size, P, P) and set(got) == set(PR.BLOCKS)
        for block, rows in got.items():
            b = PR.bits(rows).reshape(size, -1)
            for r in range(min(3, size)):
                same = np.all(b[r::3] == PR.bits(base[block][r]).reshape(1, -1), axis=1)
                assert np.all(same), (case.id, size, block, f"copy {r + 3 * int(np.argmin(same))} of trade {r}")
        del got
    dc.close()


def test_the_case_count():
    assert len(CASES) == N_CASES
