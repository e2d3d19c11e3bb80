"""Matrices, the NumPy restatement and the checks shared by the tail allocation tests (tests/test_tail_alloc_host.py, CPU,
and tests/test_gpu_tail_alloc.py, GPU) of adr_scenario_tail_alloc*."""
import functools
import math

import numpy as np

from adrates_amd import _native

B_VALUES = (1, 2, 63, 64, 65, 129, 4097)       # one slot, around the 64 slots, the first wrap twice over, 65 rows a slot
S_VALUES = (1, 2, 100, 1000, 1025, 8192)       # P&L values per row: below, at and above powers of two, the LDS limit
K_VALUES = (1, 2, 10, None)                    # None: k = S
BASES = ("none", "first", "last")
EPS = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def _pool():
    return np.random.default_rng(77).normal(0.0, 1e6, (max(B_VALUES), max(S_VALUES) + 1))


def matrix(B, S_tot):
    """``rows [B, S_tot]`` cut from one pool of normal draws (computed once, never changed)."""
    return np.ascontiguousarray(_pool()[:B, :S_tot])


def base_column(base, S_tot):
    return {"none": -1, "first": 0, "last": S_tot - 1}[base]


def pnl_of(rows, base_col):
    return rows if base_col < 0 else np.delete(rows, base_col, axis=1) - rows[:, base_col:base_col + 1]


def key_of(v):
    """The tail kernel's total-order key of doubles: -0.0 before +0.0."""
    bits = np.ascontiguousarray(v, dtype=np.float64).view(np.int64)
    return bits ^ ((bits >> 63) & np.int64(0x7FFFFFFFFFFFFFFF))


def slot_total(pnl):
    """tot[e] in the stated order: row b to slot b % 64, each slot in row order from 0.0, then the halving tree."""
    slots = np.zeros((64, pnl.shape[1]))
    for q in range(64):
        for row in pnl[q::64]:
            slots[q] = slots[q] + row
    h = 32
    with np.errstate(invalid="ignore"):                     # inf - inf in the NaN cases
        while h:
            slots[:h] = slots[:h] + slots[h:2 * h]
            h //= 2
    return slots[0].copy()


def restate(pnl, k):
    """The rule of the issue in NumPy: ``(tot, order e_1 .. e_k, var_tot, es_tot, comp_var, comp_es)``."""
    tot = slot_total(pnl)
    B = pnl.shape[0]
    if np.any(np.isnan(tot)):
        return tot, None, np.nan, np.nan, np.full(B, np.nan), np.full(B, np.nan)
    order = np.lexsort((np.arange(tot.size), key_of(tot)))[:k]
    cols = np.ascontiguousarray(pnl[:, order].T)            # [k, B]
    es, comp = 0.0, np.zeros(B)
    for j, e in enumerate(order):
        es = es + tot[e]
        comp = comp + cols[j]
    return tot, order, -tot[order[-1]], -es / float(k), -cols[-1], -comp / float(k)


def same(a, b):
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.int64)[~np.isnan(a)], b.view(np.int64)[~np.isnan(b)]) and \
        np.array_equal(np.isnan(a), np.isnan(b))


def same_result(x, y):
    return all(same(x[f], y[f]) for f in ("var", "es", "comp_var", "comp_es"))


def check(got, rows, base_col, k):
    """One call against the restatement, adr_scenario_tail_host on the one-row matrix ``tot``, and additivity."""
    pnl = pnl_of(rows, base_col)
    B = pnl.shape[0]
    tot, order, var, es, comp_var, comp_es = restate(pnl, k)
    where = (rows.shape, base_col, k)
    if order is None:
        assert all(np.all(np.isnan(got[f])) for f in ("var", "es", "comp_var", "comp_es")), where
        return
    tv, te = _native.scenario_tail_host(tot[None, :], k)
    assert same(got["var"], tv) and same(got["es"], te), where
    assert same(got["var"], var) and same(got["es"], es), where
    assert same(got["comp_var"], comp_var) and same(got["comp_es"], comp_es), where
    # the rounding of the slot sum and the tree (B terms), the two k-term sums and the division
    tail = np.abs(pnl[:, order])
    bound_es = (B + 2 * k + 10) * EPS * float(tail.sum()) / k
    bound_var = (B + 10) * EPS * float(tail[:, -1].sum())
    assert abs(math.fsum(got["comp_es"]) - got["es"]) <= bound_es, where
    assert abs(math.fsum(got["comp_var"]) - got["var"]) <= bound_var, where


def k_values(S):
    return sorted({S if k is None else k for k in K_VALUES if (k or S) <= S})


def calls(S):
    """Every ``(rows, base_col, k)`` for rows of ``S`` P&L values: the cross product of B_VALUES, the k values and the
    base column first, last and absent up to B = 129; at B = 4 097 (a matrix of up to 268 MB) the three base columns
    take turns over the k values instead, so that the large shapes stay within seconds."""
    for B in B_VALUES:
        for i, k in enumerate(k_values(S)):
            for base in (BASES if B < 4097 else (BASES[(i + S) % 3],)):
                S_tot = S if base == "none" else S + 1
                yield matrix(B, S_tot), base_column(base, S_tot), k


def special_calls():
    """Ties at the k-th place, zero totals of both signs, equal rows, all-zero rows: ``(name, rows, base_col, k)``."""
    tie = np.array([[-10.0, -1.0, -2.0, 5.0, 6.0, 7.0], [0.0, -2.0, -1.0, 1.0, 1.0, 1.0]])      # tot[1] == tot[2] == -3
    yield "the k-th and the (k+1)-th tie", tie, -1, 2
    yield "the tie inside the tail", tie, -1, 3
    yield "the tie with a base column", np.hstack([tie + 4.0, np.full((2, 1), 4.0)]), 6, 2
    zeros = np.array([[1.0, -0.0, 0.0, -2.0, -0.0], [-1.0, -0.0, 0.0, 2.0, 0.0], [0.0, -0.0, -0.0, -0.0, 0.0]])
    for k in (1, 3, 5):
        yield f"zero totals, k = {k}", zeros, -1, k
    yield "zero P&L of both signs under a base column", np.hstack([zeros, zeros[:, :1]]), 5, 2
    row = np.random.default_rng(5).normal(0.0, 1e5, 40)
    yield "equal rows", np.tile(row, (70, 1)), -1, 4
    yield "all-zero rows", np.zeros((66, 33)), -1, 5
    yield "all-zero rows under a base column", np.zeros((3, 9)), 0, 8


def tie_expectation():
    """comp_var of the first special call: scenario 1, the lower index of the tie, is the k-th."""
    return np.array([1.0, 2.0])


def nan_calls():
    """One NaN anywhere - a P&L value, the base column, a row beyond the first slot round - gives NaN everywhere."""
    for B, S_tot, base_col, at in ((3, 50, -1, (1, 20)), (130, 17, 0, (129, 0)), (65, 100, 99, (64, 3)), (1, 1, -1, (0, 0))):
        rows = matrix(B, S_tot).copy()
        rows[at] = np.nan
        yield rows, base_col, max(1, min(3, S_tot - (base_col >= 0)))
    inf = matrix(2, 8).copy()
    inf[0, 3], inf[1, 3] = np.inf, -np.inf                  # the total of scenario 3 is NaN though no entry is
    yield inf, -1, 2
