"""The device curve builder and its tables against the exact reference: `bootstrap_kernel`, `pack_kernel`
(csrc/curve_build.hip) and `curve_dfs_kernel` (csrc/curve_dfs.hip) on the grids and rows of tests/_curve_build_cases.py.

`bootstrap_kernel`: `CurvePlan.build(...).download(i)`, EVERY entry of dfs [K], jac [K, P] and hess [K, P, P] inside the running
error bound of the builders' operation sequence around the 60-digit jets of the value recurrence
(tests/_curve_reference.py: |got - value| <= e, a bound of 0 a structural zero), with the host builder's bits; two builds
repeat their bits, a row built alone has the bits of the same row at the end of five, and a plan without a Hessian gives the
same dfs and jac.  The two 64-pillar grids on either side of the `dpv_global` switch (K = 313: the PV01 gradients in LDS;
K = 314: through scratch) are held to the reference on the CPU (tests/test_curve_reference_host.py) and here to the host
builder's bits.
`curve_dfs_kernel`: the same rows as shocks at S = 1, 64 and 65 (a wave, and one lane of the next), every entry on the bound of
the scan at the rates base + x 1e-4 it forms; the rows that leave a negative factor must raise the flag, the others not.
`pack_kernel`: through the pricing judge (tests/_price_reference.py counts the table builder's log as 2 units and a table entry
as 4): three curves built on the device, the third priced with its downloaded arrays as the reference's curve - every element
of every block under the six requests of tests/_price_edge_cases.py.  Dense `lc_lanes` (the general kernel, the knot pass),
packed `ljc` / `lcc` and the `MiniKnot` records (the fast kernels), `lj` / `log_df` (lite), wide `lj64` / `lcflat` (33 and 40
pillars); the knot sweeps put a node on every knot and in every interval of the tables.

Worst shares of the bound observed on an MI355X (every test prints its own):
  `bootstrap_kernel`   dfs 0.704   jac 0.528   hess 0.515   (the host builder's bits in every case, so the host's shares)
  `curve_dfs_kernel`   0.686
  `pack_kernel` through pricing, per family: fast 0.141   fast_chained 0.004   fast_lag 0.034   general, ratio nodes 0.021
    lite 0.148   lite_lag 0.026   wide 0.150   aggregates through the block partials 0.017   through the knot passes 0.008
No share above 1 and no structural zero with a number on it: the module found no defect.  The slowest case takes 1.4 s (the
40-pillar grid, its reference included), the module 22 s.
Two deliberate edits of csrc/curve_build.hip were run against it and not kept.  `bootstrap_kernel`'s cross term without
dPp / v: all 18 cases run (semi_annual3, README 32, 33 pillars) fail the bound, hess at 5e14 to 1.3e15 of it, dfs and jac
unchanged, and none has the host builder's bits.  `pack_kernel`'s `lcc` gather: exchanging p and q changes no bit - the
Hessian's mirrors have the same bits (asserted above) and the product commutes - so no test can see it, and none does;
s_lj[p] s_lj[p] for s_lj[p] s_lj[q] in the same line fails all seven cases on the packed layout (numbers of 1e-5 on gamma
entries whose gross is 0) and passes the four that do not read `lcc` (wide, no Hessian).
DESIGN.md section 34 has the rules, the mutations the modules fail and the findings."""
import dataclasses
import time

import numpy as np
import pytest

from adrates_amd import _native

from . import _curve_build_cases as CB
from . import _curve_reference as CR
from . import _ladder_reference as R
from . import _price_edge_cases as PE
from . import _price_lag_cases as PL
from . import _price_reference as PR
from . import _price_wide_cases as PW

pytestmark = pytest.mark.gpu

AGG = ("agg_pv", "agg_delta", "agg_gamma")


def _download(plan, rates):
    cset = plan.build(np.atleast_2d(rates))
    try:
        return [cset.download(i) for i in range(len(cset))]
    finally:
        cset.close()


def _same(a, b, strict=True):
    eq = CB.strict_bits if strict else CB.same_bits
    return all((x is None and y is None) or eq(x, y) for x, y in zip(a, b))


def _build_checks(gpu_ctx, name, kind):
    """What every grid is held to whatever its size, `_host_bits` apart: two builds, alone against last of five, no Hessian.
    Returns the row's arrays."""
    rates = CB.row(name, kind)
    plan = _native.CurvePlan(gpu_ctx, CB.INTERP.value, CB.base(name, True))
    plain = _native.CurvePlan(gpu_ctx, CB.INTERP.value, CB.base(name, False))
    try:
        alone = _download(plan, rates)[0]
        # both mirrors of a Hessian entry are formed by the same operations on the same numbers
        assert CB.strict_bits(alone[2], np.swapaxes(alone[2], 1, 2)), (name, kind, "the Hessian's mirrors differ")
        assert _same(alone, _download(plan, rates)[0]), (name, kind, "two builds differ")
        assert _same(alone, _download(plan, CB.batch_of(name, kind))[4]), (name, kind, "alone and last of five differ")
        d0, j0, h0 = _download(plain, CB.batch_of(name, kind))[4]
        assert h0 is None and _same((d0, j0), alone[:2]), (name, kind, "a plan without a Hessian differs")
    finally:
        plan.close()
        plain.close()
    return alone


def _host_bits(name, kind, got):
    """The host builder starts its zeros at +0.0, the kernel multiplies them by -r / v: its bits, up to the sign of a zero."""
    return _same(got, CB.host_builder(name, CB.row(name, kind), True), strict=False)


@pytest.mark.parametrize("kind", CB.ROWS)
@pytest.mark.parametrize("name", CB.DEVICE_GRIDS)
def test_bootstrap_kernel_is_inside_the_bound_at_every_entry(gpu_ctx, name, kind):
    t0 = time.perf_counter()
    assert kind in CB.good_rows(name)
    g = CB.base(name, False)
    ref = CR.reference(g, CB.row(name, kind), 2)
    dfs, jac, hess = _build_checks(gpu_ctx, name, kind)
    host_bits = _host_bits(name, kind, (dfs, jac, hess))
    share = ref.share(dfs, jac, hess, what=f"{name}, {kind}")
    print(f"{name} (K = {g.n_knots}, P = {g.n_pillars}), {kind}: bootstrap_kernel, share of the bound "
          + ", ".join(f"{n} {s:.3f}" for n, s in share.items()) + f"; the host builder's bits: {'yes' if host_bits else 'NO'}; "
          + f"{time.perf_counter() - t0:.1f} s")
    assert max(share.values()) <= 1.0, (name, kind, share)
    assert host_bits, (name, kind, "not the host builder's bits")


@pytest.mark.parametrize("kind", CB.ROWS)
@pytest.mark.parametrize("name", CB.P64_GRIDS)
def test_bootstrap_kernel_on_either_side_of_the_scratch_switch(gpu_ctx, name, kind):
    dfs, jac, hess = _build_checks(gpu_ctx, name, kind)
    assert _host_bits(name, kind, (dfs, jac, hess)), (name, kind, "not the host builder's bits")
    assert hess.shape == (313 + CB.P64_GRIDS.index(name), 64, 64) and np.all(dfs > 0.0)


@pytest.mark.parametrize("S", CB.SCAN_S)
@pytest.mark.parametrize("name", CB.GRIDS)
def test_curve_dfs_kernel_is_inside_the_bound_and_raises_its_flag(gpu_ctx, name, S):
    g = CB.base(name, False)
    kinds, shocks = CB.scan_batch(name, S)
    plan = _native.CurvePlan(gpu_ctx, CB.INTERP.value, g)
    try:
        dfs, bad = _native.curve_dfs_shocked(gpu_ctx, plan, g.rates, shocks)
        again, bad2 = _native.curve_dfs_shocked(gpu_ctx, plan, g.rates, shocks)
    finally:
        plan.close()
    assert CB.strict_bits(dfs, again) and np.array_equal(bad, bad2), (name, S, "two launches differ")
    assert [int(b) for b in bad] == [int(k in CB.BAD_ROWS) for k in kinds], (name, S, kinds, bad)
    host, _ = _native.curve_dfs_shocked_host(g.acc, g.pillar, g.prev_idx, g.rates, shocks)
    assert CB.strict_bits(dfs, host), (name, S, "not the host scan's bits")
    worst = 0.0
    for s, kind in enumerate(kinds):
        worst = max(worst, CR.shocked_reference(g, g.rates, shocks[s]).share(dfs[s], what=f"{name}, row {s} ({kind})")["dfs"])
    print(f"{name}, S = {S}: curve_dfs_kernel, share of the bound {worst:.3f}")
    assert worst <= 1.0, (name, S)


# ------------------------------------------------------------------------------------------- pack_kernel, through pricing
def _pick(cases, name, curve, interp):
    found = [c for c in cases if c.name == name and c.curve == curve and c.interp == interp and not getattr(c, "flags", 0)]
    assert len(found) == 1, (name, curve, interp, len(found))
    return found[0]


def _price_cases():
    """(case, grid, families, with Hessian): one per kernel family and table layout."""
    ed, lag, wide = PE.cases(), PL.cases(), PW.cases()
    out = [(_pick(ed, "row geometry", "README 32", i), "README 32", PE.families, True) for i in PE.SCHEMES]    # fast, fast_chained, general, lite, knot
    out.append((_pick(ed, "knot sweep", "README 32", PE.FF), "README 32", PE.families, True))                  # every knot and interval
    out.append((_pick(ed, "knot sweep", "17 pillars", PE.LF), "17 pillars", PE.families, True))
    out.append((_pick(lag, "structure", "README 32", PE.LZ), "README 32", PE.families, True))                  # fast_lag, lite_lag, knot_lag
    out.append((_pick(lag, "structure", "README 32", PE.LF), "README 32", PE.families, True))                  # general, ratio nodes
    out.append((_pick(wide, "knot sweep", "33 pillars", PE.FF), "33 pillars", PW.families, True))
    out.append((_pick(wide, "knot sweep", "40 pillars", PE.LZ), "40 pillars", PW.families, True))
    out.append((_pick(ed, "row geometry", "README 32", PE.LZ), "README 32", PE.families, False))               # no Hessian: PV and delta
    out.append((_pick(wide, "knot sweep", "33 pillars", PE.FF), "33 pillars", PW.families, False))
    return out


PRICE_CASES = _price_cases()


def _price(ctx, dc, dt, mask, per_trade, aggregate):
    return _native.price(ctx, dc, dt, want_value=bool(mask & 1), want_delta=bool(mask & 2), want_gamma=bool(mask & 4),
                         per_trade=per_trade, aggregate=aggregate)


def _aggregate_count(case, fams, launches, stats, n, Kc):
    """The adds between the trades' numbers and the aggregate (tests/test_gpu_price_lag.py, tests/test_gpu_price_wide.py)."""
    route = getattr(case, "route", None)
    mine = [b for f, *_, b in launches if f not in ("knot", "knot_lag")]
    blocks = (max(mine) if route == "tiled" else sum(mine)) if mine else 0
    sums = PR.aggregate_sums(n, blocks, wide=route == "wide")
    for fam, count in (("knot", PR.knot_sums), ("knot_lag", PR.knot_lag_sums)):
        if fam in fams:
            sums += count([stats[i] for i in np.nonzero(fams == fam)[0]], Kc, sum(b for f, *_, b in launches if f == fam))
    return sums


@pytest.mark.parametrize("which", range(len(PRICE_CASES)))
def test_pack_kernel_tables_price_inside_the_bound(gpu_ctx, which):
    case, grid, families, with_hessian = PRICE_CASES[which]
    t0 = time.perf_counter()
    method, batch = case.interp.value, case.batch
    assert np.array_equal(case.host.times, CB.base(grid, True).times)
    m = CB.base(grid, True).rates
    rates = np.vstack([m * (1.0 + 0.01 * k) for k in range(3)])
    full = _native.CurvePlan(gpu_ctx, method, case.host)
    plan = full if with_hessian else _native.CurvePlan(gpu_ctx, method, dataclasses.replace(case.host, hess=None))
    full_set, cset = full.build(rates), None
    try:
        dfs, jac, hess = full_set.download(2)
        # the curve the reference reads: what `bootstrap_kernel` wrote, which `pack_kernel` read
        host = dataclasses.replace(case.host, dfs=dfs, jac=jac, hess=hess, rates=rates[2])
        cset = full_set if with_hessian else plan.build(rates)
        if not with_hessian:
            d0, j0, h0 = cset.download(2)
            assert h0 is None and CB.strict_bits(d0, dfs) and CB.strict_bits(j0, jac)
        case = dataclasses.replace(case, host=host)
        flags = getattr(case, "flags", 0)
        n = batch.n_trades
        ref = PR.per_trade_reference(method, host, batch)
        book = PR.book_reference(method, host, batch)
        stats = PR.trade_stats(method, host, batch)
        Kc = R.compact_count(host.times)
        dc = cset[2]
        worst, checked = {}, []
        with _native.DeviceTrades(gpu_ctx, batch) as dt:
            for name, mask, per_trade, aggregate in PE.REQUESTS:
                if mask & 4 and not with_hessian:
                    continue
                what = f"{case.id} on a built curve{'' if with_hessian else ' without a Hessian'}, {name}"
                fams = families(case, mask, per_trade, aggregate)
                launches, cover = _native.route_host(method, host.times, host.dfs, host.jac, host.hess if with_hessian else None, batch, mask,
                                                     per_trade=per_trade, aggregate=aggregate, curve_flags=flags)
                assert np.all(cover == 1) and {f for f, *_ in launches} == set(fams), (what, launches)
                got = _price(gpu_ctx, dc, dt, mask, per_trade, aggregate)
                far = getattr(case, "far_pairs", False) and not per_trade and mask & 4 and "knot_lag" in fams
                if not far:                         # (the overflow matrix's atomic adds: tests/test_gpu_price_lag.py)
                    assert PR.same_bits(got, _price(gpu_ctx, dc, dt, mask, per_trade, aggregate)), f"{what}: two launches differ"
                ks = PR.case_ks(method, host, batch, ref, fams)
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
                        print(f"{what}: {fam} ({rows.size} trades): share of the bound {share:.3f}")
                        assert share <= 1.0, (what, fam)
                        worst[fam] = max(worst.get(fam, 0.0), share)
                if aggregate:
                    sums = _aggregate_count(case, fams, launches, stats, n, Kc)
                    zero = [b for b, need in zip(PR.BLOCKS, (0, 6, 4)) if need and not mask & need]
                    share = PR.book_share({k: np.asarray(got[k]) for k in AGG}, ref, book, ks, sums, zero, what)
                    label = "aggregate of " + "+".join(sorted(set(fams)))
                    print(f"{what}: {label} (sums {sums}): share of the bound {share:.3f}")
                    assert share <= 1.0, what
                    worst[label] = max(worst.get(label, 0.0), share)
    finally:
        if cset is not None and cset is not full_set:
            cset.close()
        full_set.close()
        if plan is not full:
            plan.close()
        full.close()
    print(f"{case.id}{'' if with_hessian else ', no Hessian'}: worst shares " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items()))
          + f"; {time.perf_counter() - t0:.1f} s")
