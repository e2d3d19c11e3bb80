"""Books, scenario pairs and the independent reference shared by the inflation scenario revaluation tests
(tests/test_yoy_scenarios_host.py, CPU, and tests/test_gpu_yoy_scenarios.py, GPU) of csrc/yoy_scenario_pv.hip.

A book is a raw case of tests/_yoy_cases.py (the YoY coupons that reach every branch of the lookups) with a fixed leg
added to every second swap; a scenario is a pair (discount row, breakeven row): the case's own curves first, then
shocked pairs.  The reference is independent of the kernel's code: the C oracle's fixed-flow PV
(`_scenario_cases.oracle_pv`) plus the 60-digit `MpYoY(...).value()` of the YoY leg, per scenario and swap."""
import functools

import numpy as np

from adrates_amd.trades.compiler import TradeBatch
from oracle import mp_oracle as MP

from . import _scenario_cases as SC
from . import _yoy_cases as YC
from ._parity import unit_notional_err

BP = 1e-4


def cases():
    """The whole raw case table of tests/_yoy_cases.py: knot bookkeeping, discount lookups, launch geometry.  None is
    left out (the 60-digit reference of all of them takes about twenty seconds)."""
    return YC.all_cases()


def fixed_legs(case):
    """``(fix_off, fix_tp, fix_pay)``: a fixed leg for every second swap of ``case`` (the odd ones), signs folded in and
    a principal on the last flow, on the scale of the swap's notional.  By swap index modulo 4: 1 - one flow per coupon
    at the coupon's payment time (the kernel shares D(tp)); 3 - flows between the coupons' payment times, two more than
    coupons, the first at or before the value time (masked) and the last far out.  A swap without coupons gets three
    flows."""
    off, tp, pay = [0], [], []
    for i, rows in enumerate(case.rows):
        N = case.notional[i]
        sign = -1.0 if (i // 2) % 2 else 1.0
        if i % 2:
            t = np.array([r[0] for r in rows], dtype=np.float64)
            if t.size == 0:
                t = np.array([0.5, 1.5, 2.5])
            elif i % 4 == 3:
                t = np.concatenate(([-0.25 if i % 8 == 3 else 0.0], t + 0.013, [t[-1] + 7.3]))
            p = sign * 0.031 * N * np.ones(t.size) / max(1.0, t.size / 12.0)
            p[-1] += sign * 0.25 * N
            tp += t.tolist()
            pay += p.tolist()
        off.append(len(tp))
    return np.array(off, dtype=np.int64), np.array(tp, dtype=np.float64), np.array(pay, dtype=np.float64)


def breakeven_rows(b):
    """``[8, P]``: the base row, parallel shifts of +-200, +50 and -1 bp and single-pillar shifts of +200 bp (first),
    -200 bp (last) and +100 bp (middle)."""
    b = np.asarray(b, dtype=np.float64)
    rows = [b, b + 200 * BP, b - 200 * BP, b + 50 * BP, b - 1 * BP]
    for k, s in ((0, 200), (b.size - 1, -200), (b.size // 2, 100)):
        r = b.copy()
        r[k] += s * BP
        rows.append(r)
    return np.stack(rows)


def discount_rows(times, dfs, seed=17):
    """``[8, K]``: the base row, then zero-rate moves of it in the style of `_scenario_cases.lookup_curves`: parallel
    shifts of +-1, +-50, +-200 bp and one twist, each with +-5 bp of noise per knot (a repeated knot keeps a value of
    its own).  The t = 0 knot keeps its discount factor 1."""
    times, dfs = np.asarray(times, dtype=np.float64), np.asarray(dfs, dtype=np.float64)
    rng = np.random.default_rng(seed + times.size)
    rows = [dfs]
    for j, s in enumerate((1, -1, 50, -50, 200, -200, 0)):
        move = s * BP + rng.uniform(-5, 5, times.size) * BP
        if j == 6:
            move = move + 60 * BP * (times / max(times[-1], 1.0) - 0.5)
        rows.append(dfs * np.exp(-move * np.maximum(times, 0.0)))
    return np.stack(rows)


def scenario_pairs(case):
    """``(times, dfs [8, K], T, b [8, P])``: scenario 0 is the case's own pair; the shocked rows are paired crosswise (the
    largest discount move with a single-pillar breakeven move, and so on) so that every pair moves both curves."""
    (_, times, dfs), (_, T, b) = case.disc, case.infl
    d, r = discount_rows(times, dfs), breakeven_rows(b)
    order = [0, 5, 6, 7, 1, 2, 3, 4]
    return np.asarray(times, dtype=np.float64), d, np.asarray(T, dtype=np.float64), r[order]


def fixed_batch(case, fixed):
    """The fixed legs as a fixed-flows-only `TradeBatch` (sign +1: the signs are in the amounts) for the C oracle."""
    off, tp, pay = fixed
    n = off.size - 1
    e = np.zeros(0)
    return TradeBatch(off, np.zeros(n + 1, dtype=np.int64), tp, pay, e, e.copy(), e.copy(), e.copy(),
                      np.asarray(case.notional, dtype=np.float64), np.zeros(n), np.ones(n), np.ones(n))


@functools.lru_cache(maxsize=None)
def reference(case):
    """``[S, n]``: C oracle (fixed flows) + MpYoY (YoY leg) on every scenario pair of ``case``."""
    times, dfs, T, b = scenario_pairs(case)
    dm, im = case.disc[0], case.infl[0]
    fixed = fixed_legs(case)
    ref = SC.oracle_pv(dm, times, dfs, fixed_batch(case, fixed)) if fixed[1].size else np.zeros((dfs.shape[0], len(case.rows)))
    ref = np.array(ref, dtype=np.float64)
    for s in range(dfs.shape[0]):
        for i, rows in enumerate(case.rows):
            if rows:
                ref[s, i] += MP.MpYoY((dm, times, dfs[s]), (im, T, b[s]), rows).value()
    return ref


def worst_error(case, pv_sn, ref=None):
    """(error, scenario, swap name): the worst entry of ``pv [S, n]`` against `reference`, every swap on its own
    notional (`unit_notional_err`)."""
    ref = reference(case) if ref is None else ref
    worst = (0.0, -1, "")
    for s in range(ref.shape[0]):
        for i, name in enumerate(case.names):
            e = unit_notional_err(pv_sn[s, i], ref[s, i], case.notional[i])
            if not e <= worst[0]:
                worst = (e, s, name)
    return worst
