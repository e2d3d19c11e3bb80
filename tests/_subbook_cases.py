"""Sub-book layouts, slices and tail rows shared by the sub-book scenario tests (tests/test_subbook_scenarios_host.py,
CPU, and tests/test_gpu_subbook_scenarios.py, GPU)."""
import dataclasses

import numpy as np

from adrates_amd.market.position.scenarios import _permute_batch, expected_shortfall, historical_var, tail_count
from adrates_amd.trades import synthetic

from . import _credit_scenario_cases as CC
from . import _scenario_cases as SC

VD = SC.VD
# Trades per sub-book of ONE batch: every chunk edge (63, 64, 65, 127, 128, 129), 4 097 = 65 chunks, the first size at
# which a sub-book's slot index wraps, and empty sub-books first, in the middle two in a row, and last.
SIZES = (0, 1, 63, 64, 0, 0, 65, 127, 128, 129, 4097, 0)
S_VALUES = (1, 63, 64, 65, 130)


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def sized_book(seed=61):
    return synthetic.synthesize(VD, int(sum(SIZES)), seed=seed)


def take(batch, lo, hi):
    """The trades lo .. hi of a batch as a batch of their own."""
    return _permute_batch(batch, np.arange(lo, hi, dtype=np.int64))[0]


def take_case(case, lo, hi):
    """The same for a credit case: the batch with its spreads, buckets and spread times."""
    b = case.batch
    f0, f1, l0, l1 = int(b.fix_off[lo]), int(b.fix_off[hi]), int(b.flt_off[lo]), int(b.flt_off[hi])
    return CC.Case(take(b, lo, hi), case.z[lo:hi], case.bucket[lo:hi], case.fix_tau[f0:f1], case.flt_tau[l0:l1])


def permuted(batch, sub_off, order):
    """The batch with its sub-books in the order ``order`` (each sub-book's trades kept in order) and its offsets."""
    perm = np.concatenate([np.arange(sub_off[b], sub_off[b + 1], dtype=np.int64) for b in order] + [np.zeros(0, dtype=np.int64)])
    sizes = [int(sub_off[b + 1] - sub_off[b]) for b in order]
    return _permute_batch(batch, perm)[0], offsets(sizes)


def wide_curves(S=130, seed=5):
    """``(times, dfs [S, K])``: S distinct curves between the shocked curves of `_scenario_cases`."""
    times, dfs = SC.shocked_curves()
    mix = np.random.default_rng(seed).uniform(0.0, 1.0, size=(S, dfs.shape[0]))
    return times, np.exp((mix / mix.sum(1, keepdims=True)) @ np.log(dfs))


def cuts(n, B, seed):
    """B sub-books over n trades at random cuts (some may be empty), not aligned with anything."""
    rng = np.random.default_rng(seed)
    return np.concatenate([[0], np.sort(rng.integers(0, n + 1, B - 1)), [n]]).astype(np.int64)


def gross(batch, sub_off):
    """Gross notional per sub-book, at least 1."""
    a = np.abs(np.asarray(batch.notional))
    return np.array([max(1.0, float(a[lo:hi].sum())) for lo, hi in zip(sub_off[:-1], sub_off[1:])])


# ------------------------------------------------------------------------------------------------------------ tail rows
TAIL_S = (1, 2, 100, 1000, 1025, 16384)
TAIL_K = (1, 2, 10, None)                  # None: k = S


def tail_rows(S_tot, seed=0):
    """``(rows [B, S_tot], index of the row holding a NaN)``: three random rows, ties, an all-equal row, all zeros, a NaN."""
    rng = np.random.default_rng(1000 + S_tot + seed)
    rows = [rng.normal(0.0, 1e6, S_tot) for _ in range(3)]
    rows.append(rng.integers(-3, 4, S_tot).astype(np.float64) * 1e5)        # ties
    rows.append(np.full(S_tot, -1234.5))                                    # all equal
    rows.append(np.zeros(S_tot))
    nan = rng.normal(0.0, 1.0, S_tot)
    nan[S_tot // 2] = np.nan
    rows.append(nan)
    return np.stack(rows), len(rows) - 1


def pnl_of(rows, base_col):
    return rows if base_col < 0 else np.delete(rows, base_col, axis=1) - rows[:, base_col:base_col + 1]


def level_for(k, S):
    """A confidence level whose tail count is k of S."""
    level = 1.0 - (k - 0.5) / S
    assert tail_count(level, S) == k
    return level


def check_tail(var, es, rows, base_col, k, nan_row):
    """Item 6's expectations for one call: var is `historical_var` bit for bit, es agrees with `expected_shortfall`
    within (k + 1) 2^-52 mean|tail| (two sums of k terms in different orders differ by at most (k - 1) 2^-52 sum|x|; the
    division adds an ulp on each side); a row holding a NaN gives NaN in both."""
    pnl = pnl_of(rows, base_col)
    S = pnl.shape[1]
    level = level_for(k, S)
    for b, row in enumerate(pnl):
        if b == nan_row:
            assert np.isnan(var[b]) and np.isnan(es[b])
            continue
        tail = np.sort(row)[:k]
        assert var[b] == historical_var(row, level) and np.signbit(var[b]) == np.signbit(-tail[-1]), (b, k, base_col)
        bound = (k + 1) * 2.0 ** -52 * float(np.mean(np.abs(tail)))
        assert abs(es[b] - expected_shortfall(row, level)) <= bound, (b, k, base_col, es[b], expected_shortfall(row, level))


def tail_calls():
    """Every (rows, base_col, k, nan_row) of item 6: S P&L values per row, the base column first, last or absent."""
    for S in TAIL_S:
        for base in ("none", "first", "last"):
            S_tot = S if base == "none" else S + 1
            base_col = {"none": -1, "first": 0, "last": S_tot - 1}[base]
            rows, nan_row = tail_rows(S_tot)
            for k in sorted({S if k is None else k for k in TAIL_K if (k or S) <= S}):
                yield rows, base_col, k, nan_row
