"""The host curve builders against the exact reference (tests/_curve_reference.py), EVERY entry of dfs, jac and hess on the
running error bound of their own operation sequence: `build_engine_curve` with and without a Hessian on every grid and row of
tests/_curve_build_cases.py, `adr_curve_dfs_shocked_host` on the same rows as shocks (its bound counts the rounding of the
rates base + x 1e-4 it forms) with the rows that must raise its flag, and the judge itself: five wrong builders, each one
mutation of a test-local copy of the recurrences, each beyond the bound on at least one grid.  The GPU side of the same cases
is tests/test_gpu_curve_reference.py; DESIGN.md section 34 has the rules and the observed shares.

Worst shares of the bound observed (every test prints its own):
  `build_engine_curve`   dfs 0.704   jac 0.582   hess 0.562        `adr_curve_dfs_shocked_host`   0.686
The bound over u |entry| - its conditioning, not slack - is at most 4.4e2 (dfs), 8.5e2 (jac) and 1.9e3 (hess) on market rates
and grows on the steep rows, which bring a discount factor to 1e-3, to 3e8 (dfs) and 9e12 (hess) on README 32 and beyond
1e20 on entries of the 64-pillar grids that are small against their own terms.
Every mutation is beyond the bound on every grid that can show it: 2e13 to 1e15 of it; `late_predecessor` puts numbers on
structural zeros of the hand-made scan.
The jets' own cross-check - central differences at 110 digits, step 1e-30 - agrees with them to 4e-18 of the bound.
The 40-pillar grid is the slowest: about 5 s per row, nearly all of it the reference."""
import numpy as np
import pytest

from adrates_amd import _native

from . import _curve_build_cases as CB
from . import _curve_reference as CR


def _report(what, ref, share):
    units = ref.bound_in_units()
    print(f"{what}: share of the bound " + ", ".join(f"{n} {share[n]:.3f} [bound / u|entry| <= {units[n]:.3g}]" for n in share))


@pytest.mark.parametrize("kind", CB.ROWS)
@pytest.mark.parametrize("name", CB.GRIDS)
def test_the_host_builder_is_inside_the_bound_at_every_entry(name, kind):
    g = CB.base(name, False)
    assert kind in CB.good_rows(name)
    rates = CB.row(name, kind)
    ref = CR.reference(g, rates, 2)
    dfs, jac, hess = CB.host_builder(name, rates, True)
    share = ref.share(dfs, jac, hess, what=f"{name}, {kind}")
    _report(f"{name} (K = {g.n_knots}, P = {g.n_pillars}), {kind}", ref, share)
    assert max(share.values()) <= 1.0, (name, kind, share)
    # this module's copy of the operation sequence is the builder's: the bound is the bound of THIS program
    for n, got in zip(CR.ARRAYS, (dfs, jac, hess)):
        assert CB.same_bits(ref.replica[n], got), (name, kind, n)
    assert CB.strict_bits(hess, np.swapaxes(hess, 1, 2)), (name, kind, "the Hessian's mirrors differ")
    d1, j1, h1 = CB.host_builder(name, rates, False)
    assert h1 is None and CB.strict_bits(d1, dfs) and CB.strict_bits(j1, jac), (name, kind, "without a Hessian")
    assert max(ref.share(d1, j1, what=f"{name}, {kind}, no Hessian").values()) <= 1.0


@pytest.mark.parametrize("name", CB.GRIDS)
def test_the_host_scan_is_inside_the_bound_and_raises_its_flag(name):
    g = CB.base(name, False)
    for S in (1, 8):
        kinds, shocks = CB.scan_batch(name, S)
        dfs, bad = _native.curve_dfs_shocked_host(g.acc, g.pillar, g.prev_idx, g.rates, shocks)
        assert [int(b) for b in bad] == [int(k in CB.BAD_ROWS) for k in kinds], (name, kinds, bad)
        worst = 0.0
        for s, kind in enumerate(kinds):
            ref = CR.shocked_reference(g, g.rates, shocks[s])
            worst = max(worst, ref.share(dfs[s], what=f"{name}, {kind} as a shock")["dfs"])
        print(f"{name}, S = {S}: adr_curve_dfs_shocked_host, share of the bound {worst:.3f}")
        assert worst <= 1.0, (name, S)


def test_the_judge_rejects_each_wrong_builder():
    """Each mutation of the recurrences' copy is beyond the bound - or leaves a number on a structural zero - on at least one
    grid; the copy itself is inside it (and has the builder's bits: `_curve_build_cases.base`)."""
    grids = ("semi_annual3", "hand_made", "17 pillars")
    caught = {m: [] for m in CB.MUTATIONS}
    for name in grids:
        g = CB.base(name, False)
        ref = CR.reference(g, g.rates, 2)
        assert max(ref.share(*CB.restate_builder(g, g.rates)).values()) <= 1.0, name
        for m in CB.MUTATIONS:
            try:
                share = max(ref.share(*CB.restate_builder(g, g.rates, mutation=m), what=m).values())
            except AssertionError as e:
                assert "structural zero" in str(e), e
                share = float("inf")
            print(f"{m} on {name}: {share:.3g} of the bound")
            if share > 1.0:
                caught[m].append(name)
    assert all(caught.values()), caught
    assert caught["late_predecessor"] == ["hand_made"]          # the only grid with such a predecessor


def test_the_jets_agree_with_differences_of_sufficient_precision():
    """The jet arithmetic against central differences at 110 digits with step 1e-30, on the grids small enough for all
    pairs; the differences' noise is asserted to lie 2^-20 below the smallest bound."""
    for name, kind in (("semi_annual3", "market"), ("hand_made", "micro"), ("hand_made", "steep")):
        g = CB.base(name, False)
        P = g.n_pillars
        worst = CR.difference_check(g, CB.row(name, kind), [(p, q) for p in range(P) for q in range(p, P)])
        print(f"{name}, {kind}: differences against jets, {worst:.3g} of the bound")
        assert worst <= 2.0 ** -20
