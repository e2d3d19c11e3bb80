"""The sized YoY book, its slices and the sub-book calls shared by the YoY sub-book tests (tests/test_yoy_subbook_host.py,
CPU, and tests/test_gpu_yoy_subbooks.py, GPU) of adr_yoy_scenario_subbook_pv*."""
import functools

import numpy as np

from adrates_amd import _native

from . import _subbook_cases as SB
from . import _yoy_cases as YC
from . import _yoy_scenario_cases as YS

SIZES = SB.SIZES                           # (0, 1, 63, 64, 0, 0, 65, 127, 128, 129, 4097, 0): see tests/_subbook_cases.py
S_VALUES = SB.S_VALUES                     # 1, 63, 64, 65, 130
offsets = SB.offsets


def table_swaps():
    """Every swap of the raw case table that does not depend on its case's curves: the knot swaps (single coupons,
    seasoned legs, a swap without coupons) and a geometry book (legs of 1 .. 129 coupons, four empty swaps)."""
    return YC.knot_swaps() + YC.geometry_swaps(17, shift=1)


@functools.lru_cache(maxsize=None)
def sized_case(dm=YC.LZ, im=YC.LZ, K=None, P=20):
    """One batch of sum(SIZES) swaps tiled from `table_swaps`, with `_yoy_scenario_cases.fixed_legs` on every second swap:
    swaps with both legs, one leg or none."""
    swaps, n = table_swaps(), int(sum(SIZES))
    tiled = [(f"{i}: {swaps[i % len(swaps)][0]}",) + tuple(swaps[i % len(swaps)][1:]) for i in range(n)]
    return YC.Case(f"sized book, K = {K}, P = {P}, {YC.NAMES[im]} / disc {YC.NAMES[dm]}", (dm,) + YC.disc_grid(K),
                   (im,) + YC.pillars(P), tiled)


def take(fixed, book, lo, hi):
    """The swaps lo .. hi of ``(fixed, book)`` as a pair of their own."""
    f0, f1 = int(fixed[0][lo]), int(fixed[0][hi])
    c0, c1 = int(book["cpn_off"][lo]), int(book["cpn_off"][hi])
    sub = {k: book[k][c0:c1] for k in _native.YOY_FIELDS}
    sub["cpn_off"] = book["cpn_off"][lo:hi + 1] - c0
    return (fixed[0][lo:hi + 1] - f0, fixed[1][f0:f1], fixed[2][f0:f1]), sub


def permuted(fixed, book, sub_off, order):
    """The pair with its sub-books in the order ``order`` (each sub-book's swaps kept in order) and its offsets."""
    parts = [take(fixed, book, int(sub_off[b]), int(sub_off[b + 1])) for b in order]
    cat_off = lambda offs: np.concatenate([[0]] + [o[1:] + base for o, base in zip(
        offs, np.cumsum([0] + [int(o[-1]) for o in offs[:-1]]))]).astype(np.int64)
    fixed_p = (cat_off([p[0][0] for p in parts]), np.concatenate([p[0][1] for p in parts]), np.concatenate([p[0][2] for p in parts]))
    book_p = {k: np.concatenate([p[1][k] for p in parts]) for k in _native.YOY_FIELDS}
    book_p["cpn_off"] = cat_off([p[1]["cpn_off"] for p in parts])
    return fixed_p, book_p, offsets([int(sub_off[b + 1] - sub_off[b]) for b in order])


def gross(case, sub_off):
    """Gross notional per sub-book, at least 1."""
    a = np.abs(case.notional)
    return np.array([max(1.0, float(a[lo:hi].sum())) for lo, hi in zip(sub_off[:-1], sub_off[1:])])


def wide_pairs(case, S=130, seed=9):
    """``(times, dfs [S, K], T, b [S, P])``: S distinct pairs between the scenario pairs of the case."""
    times, dfs, T, b = YS.scenario_pairs(case)
    mix = lambda rows, sd: np.exp((lambda m: m / m.sum(1, keepdims=True))(
        np.random.default_rng(sd).uniform(0.0, 1.0, size=(S, rows.shape[0]))) @ np.log(rows))
    return times, mix(dfs, seed), T, mix(1.0 + b, seed + 1) - 1.0


class Entries:
    """The parent and the sub-book entry of one side: the host twins, or the device through ``ctx``."""

    def __init__(self, ctx=None):
        self.ctx = ctx

    def parent(self, case, times, dfs, T, b, fixed, book, per_trade=False):
        args = (case.disc[0], times, dfs, case.infl[0], T, b, fixed, book)
        if self.ctx is None:
            return _native.yoy_scenario_pv_host(*args, per_trade=per_trade)
        return _native.yoy_scenario_pv(self.ctx, *args, per_trade=per_trade)

    def sub(self, case, times, dfs, T, b, fixed, book, sub_off, per_trade=False):
        args = (case.disc[0], times, dfs, case.infl[0], T, b, fixed, book, sub_off)
        if self.ctx is None:
            return _native.yoy_scenario_subbook_pv_host(*args, per_trade=per_trade)
        return _native.yoy_scenario_subbook_pv(self.ctx, *args, per_trade=per_trade)


def check_sized_book(E, case, book_sum):
    """Every row against the parent on the sub-book alone, against the fixed-order sum of the launch's own per-swap rows,
    and the per-swap rows against the parent's; an empty sub-book is +0.0.  Returns the launch's result."""
    times, dfs, T, b = YS.scenario_pairs(case)
    fixed, book, sub_off = YS.fixed_legs(case), case.book, offsets(SIZES)
    out = E.sub(case, times, dfs, T, b, fixed, book, sub_off, per_trade=True)
    parent = E.parent(case, times, dfs, T, b, fixed, book, per_trade=True)
    assert np.array_equal(out["pv"], parent["pv"], equal_nan=True)
    assert out["sub_pv"].shape == (len(SIZES), dfs.shape[0])
    for j, (lo, hi) in enumerate(zip(sub_off[:-1], sub_off[1:])):
        if lo == hi:
            assert np.all(out["sub_pv"][j] == 0.0) and not np.any(np.signbit(out["sub_pv"][j])), j
            continue
        f, bk = take(fixed, book, lo, hi)
        alone = E.parent(case, times, dfs, T, b, f, bk)["book_pv"]
        assert np.array_equal(out["sub_pv"][j], alone), (j, lo, hi)
        assert np.array_equal(out["sub_pv"][j], book_sum(out["pv"][:, lo:hi])), (j, lo, hi)
    return out


def check_one_sub_book_is_the_parent(E, case):
    """B = 1 against the parent's book_pv, with each curve per scenario and shared (S_disc, S_infl in {1, S})."""
    times, dfs, T, b = YS.scenario_pairs(case)
    fixed, n = YS.fixed_legs(case), len(case.rows)
    for d, r in ((dfs, b), (dfs[3], b), (dfs, b[2]), (dfs[1], b[1])):
        parent = E.parent(case, times, d, T, r, fixed, case.book, per_trade=True)
        got = E.sub(case, times, d, T, r, fixed, case.book, [0, n], per_trade=True)
        assert np.array_equal(got["sub_pv"][0], parent["book_pv"], equal_nan=True), case
        assert np.array_equal(got["pv"], parent["pv"], equal_nan=True), case


def check_scenario_counts(E):
    """A row does not depend on S: 1, 63, 65 and 130 end in a partial group of 64."""
    case = sized_case()
    times, dfs, T, b = wide_pairs(case)
    small_off = offsets((0, 1, 63, 64, 0, 0, 65, 127, 80, 0))
    fixed, book = take(YS.fixed_legs(case), case.book, 0, 400)
    full = E.sub(case, times, dfs, T, b, fixed, book, small_off)["sub_pv"]
    for S in S_VALUES:
        assert np.array_equal(E.sub(case, times, dfs[:S], T, b[:S], fixed, book, small_off)["sub_pv"], full[:, :S]), S


def check_permutation(E, out):
    case = sized_case()
    times, dfs, T, b = YS.scenario_pairs(case)
    sub_off = offsets(SIZES)
    order = np.random.default_rng(4).permutation(len(SIZES))
    fixed_p, book_p, off_p = permuted(YS.fixed_legs(case), case.book, sub_off, order)
    assert np.array_equal(E.sub(case, times, dfs, T, b, fixed_p, book_p, off_p)["sub_pv"], out["sub_pv"][order])


def fallback_case(P, K, dm):
    """K = 856: the discount table leaves the LDS; P = 64 at K = 264 (171 080 bytes) does too."""
    im = YC.INFL_SCHEMES[P % 2]
    return YC.Case(f"P = {P}, K = {K}", (dm,) + YC.disc_grid(K), (im,) + YC.pillars(P), YC.geometry_swaps(150, shift=P % 4))


FALLBACKS = ((20, 856, YC.LZ), (20, 856, YC.LF), (64, 264, YC.LZ), (64, 264, YC.LF))


def check_fallback(E, P, K, dm, book_sum):
    case = fallback_case(P, K, dm)
    times, dfs, T, b = YS.scenario_pairs(case)
    fixed, n = YS.fixed_legs(case), len(case.rows)
    sub_off = SB.cuts(n, 5, 11)
    out = E.sub(case, times, dfs, T, b, fixed, case.book, sub_off, per_trade=True)
    assert np.array_equal(out["pv"], E.parent(case, times, dfs, T, b, fixed, case.book, per_trade=True)["pv"])
    for j, (lo, hi) in enumerate(zip(sub_off[:-1], sub_off[1:])):
        if lo < hi:
            f, bk = take(fixed, case.book, lo, hi)
            assert np.array_equal(out["sub_pv"][j], E.parent(case, times, dfs, T, b, f, bk)["book_pv"]), j
            assert np.array_equal(out["sub_pv"][j], book_sum(out["pv"][:, lo:hi])), j
    return case, out, sub_off


def check_malformed_offsets(E, LibError, raises):
    case = YC.knot_cases()[0]
    times, dfs, T, b = YS.scenario_pairs(case)
    fixed, n = YS.fixed_legs(case), len(case.rows)
    for bad, msg in (([0, 5, 3, n], r"decreases at sub-book 1 \(5 \.\. 3\)"), ([1, 5, n], "sub-book 0 starts at 1"),
                     ([0, 5, n - 1], f"sub-book 1 ends at {n - 1}"), ([0, 5, n + 1], f"sub-book 1 ends at {n + 1}")):
        with raises(LibError, match=msg):
            E.sub(case, times, dfs, T, b, fixed, case.book, bad)
