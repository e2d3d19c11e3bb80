"""`adr_price` on one pillar tile against the plain 60-digit reference (tests/_ladder_reference.py), EVERY element of pv, delta
and gamma on the bound of its kernel family (tests/_price_reference.py): |got - value| <= k 2^-53 gross, the sign bit clear where
gross is 0.  The cases (tests/_price_edge_cases.py; tests/test_price_edges_host.py asserts on the CPU which kernel each
reaches) run under six requests - mask 7 per trade, per trade + aggregate and aggregate only (the knot pass), mask 3 per trade
(the lite kernel) and aggregate only, mask 1 per trade -, every launch twice, bit for bit; the aggregate is held to the
reference's one-desk row with the reduction's count added.  Where the code writes both mirrors of gamma from one number (the
fast kernels' expansion of the packed ladder; the aggregate of a plan whose launches are all fast kernels) gamma[p][q] and
gamma[q][p] must have the same bits; the general kernel forms the two mirrors of a diagonal 4 x 4 block, and the knot pass's
projection every entry, on their own, so there both mirrors are held to the bound.

Worst shares of the bound observed on an MI355X, per family over all cases and schemes (every test prints its own):
  fast 0.158   fast_chained 0.010   general 0.107 (L2 rows; 0.001 on the legs of 385 to 450 coupons)   lite 0.221
  aggregate through the block partials 0.023   aggregate through the knot pass 0.013
The module found rounding dust on structural zeros of the general kernel's gamma under LINEAR_FWD_RATES (1.5e-24 at
gamma[0][1] of the 400-coupon leg), fixed in kernels_general.hip (`lindf_plain`); DESIGN.md section 24 has the finding, the
instantiations covered and the mutations this module fails.  The slowest case takes 0.8 s.
The launch-shape check prices the one-row trades of the row geometry book in launches of 1, 2, 3, 24, 25 and 49 rows (the book
cycled): a trade's pv, delta and gamma have the same bits at every position and in every batch size, for the fast kernel
(mask 7) and for the lite kernel (masks 3 and 1)."""
import numpy as np
import pytest

from adrates_amd import _native

from . import _ladder_reference as R
from . import _price_edge_cases as PE
from . import _price_reference as PR

pytestmark = pytest.mark.gpu

CASES = PE.cases()
N_CASES = 24


def price(ctx, dc, dt, mask, per_trade, aggregate):
    return _native.price(ctx, dc, dt, want_value=bool(mask & 1), want_delta=bool(mask & 2), want_gamma=bool(mask & 4),
                         per_trade=per_trade, aggregate=aggregate)


def device_curve(ctx, case):
    h = case.host
    return _native.DeviceCurve(ctx, case.interp.value, h.times, h.dfs, h.jac, h.hess)


def as_book(got):
    return {k: np.asarray(got[k]) for k in ("agg_pv", "agg_delta", "agg_gamma")}


@pytest.mark.parametrize("which", range(N_CASES))
def test_every_element_of_every_request(gpu_ctx, which):
    case = CASES[which]
    h, method, batch = case.host, case.interp.value, case.batch
    n = batch.n_trades
    ref = PR.per_trade_reference(method, h, batch)
    book = PR.book_reference(method, h, batch)
    stats = PR.trade_stats(method, h, batch)
    Kc = R.compact_count(h.times)
    dc = device_curve(gpu_ctx, case)
    checked = []                                  # (block, family per trade, bits) -> share: the same bits need no second pass
    worst = {}
    with _native.DeviceTrades(gpu_ctx, batch) as dt:
        for name, mask, per_trade, aggregate in PE.REQUESTS:
            what = f"{case.id}, {name}"
            fams = PE.families(case, mask, per_trade, aggregate)
            launches, cover = _native.route_host(method, h.times, h.dfs, h.jac, h.hess, batch, mask, per_trade=per_trade, aggregate=aggregate)
            assert np.all(cover == 1) and {f for f, *_ in launches} == set(fams), (what, launches)
            got = price(gpu_ctx, dc, dt, mask, per_trade, aggregate)
            again = price(gpu_ctx, dc, dt, mask, per_trade, aggregate)
            assert PR.same_bits(got, again), f"{what}: two launches differ"
            ks = PR.case_ks(method, h, batch, ref, fams)
            if per_trade:
                assert set(got) - {"agg_pv", "agg_delta", "agg_gamma"} == {b for b, bit in zip(PR.BLOCKS, (1, 2, 4)) if mask & bit}, what
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
                    fast = np.nonzero((fams == "fast") | (fams == "fast_chained"))[0]
                    g = got["gamma"][fast]
                    assert np.array_equal(PR.bits(g), PR.bits(np.swapaxes(g, 1, 2))), f"{what}: the fast kernels' mirrors differ"
            if aggregate:
                blocks = sum(b for *_, b in launches)
                sums = PR.aggregate_sums(n, blocks)
                if "knot" in fams:
                    sums += PR.knot_sums([stats[i] for i in np.nonzero(fams == "knot")[0]], Kc, blocks)
                zero = [b for b, need in zip(PR.BLOCKS, (0, 6, 4)) if need and not mask & need]
                share = PR.book_share(as_book(got), ref, book, ks, sums, zero, what)
                label = "aggregate of " + "+".join(sorted(set(fams)))
                print(f"{what}: {label} (sums {sums}): share of the bound {share:.3f}")
                assert share <= 1.0, what
                worst[label] = max(worst.get(label, 0.0), share)
                if mask & 4 and set(fams) <= {"fast", "fast_chained"}:
                    g = got["agg_gamma"]
                    assert np.array_equal(PR.bits(g), PR.bits(g.T)), f"{what}: the aggregate's mirrors differ"
    dc.close()
    print(f"{case.id}: worst shares " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("interp", PE.SCHEMES, ids=lambda i: i.name)
def test_a_trade_keeps_its_bits_at_every_position_and_batch_size(gpu_ctx, interp):
    """The one-row trades of the row geometry book (1, 31 and 32 coupons) cycled to launches of 1, 2, 3, 24, 25 and 49 rows:
    every copy of a trade has the bits of the trade in the row geometry book, whose rows the test above holds to the bound -
    under mask 7 (the fast kernel: either group of a wave, a block pass of 24 rows and one row more, a third pass), mask 3 and
    mask 1 (the lite kernel: any of the four groups of a wave)."""
    host = PE.curve("README 32", interp)
    dc = _native.DeviceCurve(gpu_ctx, interp.value, host.times, host.dfs, host.jac, host.hess)
    with _native.DeviceTrades(gpu_ctx, PE.row_geometry_book()) as dt:
        base = {mask: price(gpu_ctx, dc, dt, mask, True, False) for mask in (7, 3, 1)}
    for size in PE.LAUNCH_SIZES:
        book = PE.cycled_book(size)
        with _native.DeviceTrades(gpu_ctx, book) as dt:
            for mask in (7, 3, 1):
                fams = set(f for f, *_ in _native.route_host(interp.value, host.times, host.dfs, host.jac, host.hess, book, mask)[0])
                assert fams == ({"fast"} if mask == 7 else {"lite"}), (size, mask, fams)
                got = price(gpu_ctx, dc, dt, mask, True, False)
                for i in range(size):
                    for block, rows in got.items():
                        assert np.array_equal(PR.bits(rows[i]), PR.bits(base[mask][block][i % 3])), (interp.name, size, mask, i, block)
    dc.close()


def test_the_case_count():
    assert len(CASES) == N_CASES
