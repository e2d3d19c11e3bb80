"""The plain reference of the inflation scenario entries (adr_yoy_scenario_pv*, csrc/yoy_scenario_pv.hip, and the per-swap rows
of adr_yoy_scenario_subbook_pv*) and the bound the kernel and its host twin are held to, element by element
(tests/test_yoy_scenario_edges_host.py, CPU, and tests/test_gpu_yoy_scenario_edges.py, GPU).  It is the inflation sibling of
tests/_scenario_reference.py, takes its discount side (`_Rows`) and its `Reference` from there, and shares no code with the
kernel, with oracle/port.c or with `MpYoY`.

The operation.  The inputs are what the entries take, each an exact binary number: the two schemes, the knot times x_k and the
discount rows ``dfs [S_disc, K]``, the pillar times T_k and the breakeven rows ``b [S_infl, P]`` (a shared row is read by every
scenario), the fixed legs and the coupon book.  For every pair (swap i, scenario s)
  value = sum over the fixed flows with xt > 0 of  pay D(xt)
        + sum over the coupons with tp > 0 of      scale (exp(ln I(te) - ln I(ts)) - 1 + spread) D(tp)
(both masks strict).  D(t) is `_scenario_reference._Rows`: simple_interp.hpp's lookup rule on row s, its float64 decisions from
`oracle.mp_oracle._lookup_plan`.  ln I(t) is the same rule (`_Rows.plan`) on the nodes x = [0, T_1 .. T_P] with the ordinates
L_0 = 0, L_k = T_k ln(1 + b_k), taken at 60 digits from b_k as given (1 + b_k is exact here):
  FLAT_FWD_RATES     ln I = (1 - w) L_a + w L_b                              (a pillar alone: L_k)
  LINEAR_ZERO_RATES  ln I = t (1 - w) / max(x_a, 1e-15) L_a + t w / x_b L_b    (a pillar held at an end: t / x_k L_k)
and node 0 contributes 0 whatever its weight is (under LINEAR_ZERO_RATES that weight is t (1 - w) / 1e-15).  Everything that
depends on d or b runs in mpmath at 60 digits; D(t), ln I(t) and exp(ln I(te) - ln I(ts)) are cached per distinct date and row.

Gross.  ``gross`` is the same sum on absolute values with the terms as written: |scale| (exp(le - ls) + 1 + |spread|) D(tp) for
a coupon, |scale| |spread| D(tp) for one with ts == te, |pay| D(xt) for a fixed flow.  An element with gross == 0 (a swap
without a live flow, a coupon whose scale is 0.0 or -0.0) must be +0.0.

The bound |got - value| <= k 2^-53 gross, k = `bound_k`, one k per (swap, scenario).  The conventions are those of
tests/_scenario_reference.py: each rounding is ONE unit 2^-53 of the absolute sum it acts on (twice the unit roundoff, which
pays for every second-order term), a library function documented at one ulp is TWO units, and an absolute error of an exponent
is a relative error of the exp.  As the code performs them (simple_interp.hpp::log_weights, scenario_common.hpp::eval_df,
yoy_scenario_pv.hip::node_log, eval_ln_index, apply_slot, swap_pv), per term of a swap:
  D(t)      e_D of tests/_scenario_reference.py (`date_roundings`), unchanged: the discount side is the same code.  cond_D is
            the largest conditioning over the swap's live payment dates on the scenario's discount row
  L_k       ob = 1 + b_k (1): a relative error of ob is an ABSOLUTE error of log(ob), so it costs T_k units of 2^-53 on L_k
            whatever |L_k| is;  log (2) and T_k * log (1), relative to |L_k|                        T_k + 3 |L_k|
  ln I(t)   the weight W_k formed from w (e_w roundings: FLAT_FWD 1 - w: 1;  LINEAR_ZERO t (1 - w) / x_a: 3; w itself is the
            plan's float64 number, the same expression in the code), the product W_k L_k (1) and the sum of the two
            products (1), all relative to sum |W_k L_k|:     c(t) = sum_k |W_k| (T_k + (e_w + 5) |L_k|)   (units, absolute)
  ratio     x = le - ls (1), of |le - ls| <= sum |W_k L_k| over both dates; so x carries
                                                cond_y = sum over ts and te of sum_k |W_k| (T_k + (e_w + 6) |L_k|)
            units, which q = exp(x) takes as a relative error; the exp itself (2)                    ceil(cond_y) + 2
  coupon    q - 1 (1, of at most q + 1), + spread (1, of at most q + 1 + |spread|), scale * (1), * dp: the date and the
            product, e_D + 1                                                                  ceil(cond_y) + e_D + 6
            (a coupon with ts == te has y = 0 exactly and costs e_D + 3, a fixed flow pay * D(xt) costs e_D + 1: less).
            Where the code takes ln I(ts) from `Acc::le` or a fixed flow's D from the coupon's `dp`, it takes the number the
            date's own evaluation gives (the same date on the same table through the same expressions), so nothing is added
  sums      the running sums a.cpn and a.fix take the swap's live terms one after another, each from 0.0 (the first add is
            exact), and swap_pv joins the two (1): n_c - 1 + n_f - 1 + 1 roundings, each of at most gross   n_terms
`bound_k` adds these: k = ceil(cond_y) + e_D + 6 + n_terms with cond_y the largest over the swap's live coupons (0 where none
has ts != te).  Nothing in k is fitted to what the kernels return.  On the edge books (tests/_yoy_scenario_edge_cases.py) k
runs from 7 (a swap without flows under LINEAR_FWD_RATES; 10 for the smallest swap with a live flow) to 1 592 (one pillar at
T = 2 that holds b = -1 + 2^-20, |L| = 27.7, read under LINEAR_ZERO_RATES from a date held at 10: the weight is 5); on the main
book it stays below 400.  tests/test_yoy_scenario_edges_host.py prints the range of every case.
"""
import math

import numpy as np
from mpmath import mp, mpf

from . import _scenario_reference as R

FLAT_FWD, LINEAR_FWD, LINEAR_ZERO = R.FLAT_FWD, R.LINEAR_FWD, R.LINEAR_ZERO
YOY_FIELDS = ("tp", "ts", "te", "scale", "spread")
_mp = R._mp


def bound_k(disc_method, n_terms, cond_d, cond_y):
    """k of the module docstring: ``n_terms`` live terms of the swap, ``cond_d`` the largest conditioning of one of its payment
    dates on the scenario's discount row, ``cond_y`` the largest cond_y of one of its coupons on the scenario's breakeven row."""
    return math.ceil(cond_y) + R.date_roundings(disc_method, cond_d) + 6 + n_terms


class _Index(R._Rows):
    """ln I(t) on the rows of ``b``: `_Rows`' plans on x = [0, T], the ordinates L_k in place of ln d_k."""

    def __init__(self, method, T, b):
        assert int(method) in (FLAT_FWD, LINEAR_ZERO)
        self.method = int(method)
        self.T = np.ascontiguousarray(T, dtype=np.float64)
        self.x = np.concatenate(([0.0], self.T))
        self.b = np.ascontiguousarray(np.atleast_2d(b), dtype=np.float64)
        self.e_w = R._WEIGHT_ROUNDINGS[self.method]
        self._knot, self._plan, self._date, self._ratio = {}, {}, {}, {}

    def knot(self, r, k):
        """L_k of row r (k >= 1)."""
        key = (r, k)
        if key not in self._knot:
            self._knot[key] = _mp(self.T[k - 1]) * mp.log(1 + _mp(self.b[r, k - 1]))
        return self._knot[key]

    def date(self, t, r):
        """``(ln I, sum_k |W_k| (T_k + (e_w + 6) |L_k|))`` of date t on row r."""
        key = (t, r)
        if key not in self._date:
            ln, cond = mpf(0), mpf(0)
            for k, w in self.plan(t):
                if k == 0:
                    continue
                L = self.knot(r, k)
                ln += w * L
                cond += abs(w) * (_mp(self.T[k - 1]) + (self.e_w + 6) * abs(L))
            self._date[key] = (ln, cond)
        return self._date[key]

    def ratio(self, ts, te, r):
        """``(exp(ln I(te) - ln I(ts)), cond_y)``."""
        key = (ts, te, r)
        if key not in self._ratio:
            (ls, cs), (le, ce) = self.date(ts, r), self.date(te, r)
            self._ratio[key] = (mp.exp(le - ls), cs + ce)
        return self._ratio[key]


class Reference(R.Reference):
    """`_scenario_reference.Reference` (``share``, ``between``) with the place of the worst element."""

    def worst(self, got, what=""):
        """``(share, swap, scenario, |got - value| / |value| there)`` of the element of ``got [S, n]`` with the largest share of
        its bound; asserts that an element with gross == 0 is +0.0."""
        got = self._walk(got, what)
        unit = mpf(2) ** -53
        out = (0.0, -1, -1, 0.0)
        for i in range(self.n):
            for s in range(self.S):
                g = self.gross[i][s]
                if g == 0:
                    assert got[s, i] == 0.0 and not np.signbit(got[s, i]), f"{what} swap {i}, scenario {s}: gross is 0 but the entry is {got[s, i]!r}"
                    continue
                err = abs(_mp(got[s, i]) - self.value[i][s])
                share = float(err / (int(self.k[i, s]) * unit * g))
                if share > out[0]:
                    out = (share, i, s, float(err / abs(self.value[i][s])) if self.value[i][s] != 0 else math.inf)
        return out


    def apart(self, a, b, what=""):
        """`between` with its place: ``(share, swap, scenario)`` of the worst |a - b| / (k 2^-53 gross)."""
        a, b = self._walk(a, what), self._walk(b, what)
        unit = mpf(2) ** -53
        out = (0.0, -1, -1)
        for s, i in zip(*np.nonzero(a != b)):
            g = self.gross[i][s]
            assert g != 0, (what, i, s)
            out = max(out, (float(abs(_mp(a[s, i]) - _mp(b[s, i])) / (int(self.k[i, s]) * unit * g)), int(i), int(s)))
        return out


_CACHE, _DISC, _INFL = {}, {}, {}


def _legs(fixed, book, n=None):
    """``(fix_off, fix_tp, fix_pay, cpn_off, {field: array})`` with an absent leg empty."""
    if book is not None:
        cpn_off = np.asarray(book["cpn_off"], dtype=np.int64)
        n = cpn_off.size - 1
        cpn = {f: np.asarray(book[f], dtype=np.float64) for f in YOY_FIELDS}
    if fixed is not None:
        fix_off = np.asarray(fixed[0], dtype=np.int64)
        n = fix_off.size - 1
        fix_tp, fix_pay = np.asarray(fixed[1], dtype=np.float64), np.asarray(fixed[2], dtype=np.float64)
    else:
        fix_off, fix_tp, fix_pay = np.zeros(n + 1, dtype=np.int64), np.zeros(0), np.zeros(0)
    if book is None:
        cpn_off, cpn = np.zeros(n + 1, dtype=np.int64), {f: np.zeros(0) for f in YOY_FIELDS}
    assert fix_off.size == cpn_off.size
    return fix_off, fix_tp, fix_pay, cpn_off, cpn


def reference(disc_method, times, dfs, infl_method, T, b, fixed, book):
    """The `Reference` of one call: ``dfs`` and ``b`` one shared row or one row per scenario, ``fixed`` = (fix_off, fix_tp,
    fix_pay) or None, ``book`` = ``cpn_off`` and the fields YOY_FIELDS or None.  Built once per process for the same inputs; the
    two curve sides are cached on their own, so the six scheme pairs of a case share three discount and two inflation sides."""
    mp.dps = R.DPS
    times = np.ascontiguousarray(times, dtype=np.float64)
    dfs = np.ascontiguousarray(np.atleast_2d(dfs), dtype=np.float64)
    T = np.ascontiguousarray(T, dtype=np.float64)
    b = np.ascontiguousarray(np.atleast_2d(b), dtype=np.float64)
    fix_off, fix_tp, fix_pay, cpn_off, cpn = _legs(fixed, book)
    kd, ki = (int(disc_method),) + R._key(times, dfs), (int(infl_method),) + R._key(T, b)
    key = kd + ki + R._key(fix_off, fix_tp, fix_pay, cpn_off, *[cpn[f] for f in YOY_FIELDS])
    if key not in _CACHE:
        if kd not in _DISC:
            _DISC[kd] = R._Rows(disc_method, times, dfs)
        if ki not in _INFL:
            _INFL[ki] = _Index(infl_method, T, b)
        _CACHE[key] = _build(_DISC[kd], _INFL[ki], fix_off, fix_tp, fix_pay, cpn_off, cpn)
    return _CACHE[key]


def _build(rows, index, fix_off, fix_tp, fix_pay, cpn_off, cpn):
    S_disc, S_infl = rows.dfs.shape[0], index.b.shape[0]
    S = max(S_disc, S_infl)
    assert S_disc in (1, S) and S_infl in (1, S)
    n = fix_off.size - 1
    value, gross = [], []
    k = np.zeros((n, S), dtype=np.int64)
    zero = mpf(0)
    for i in range(n):
        fixed = [(float(fix_tp[j]), _mp(fix_pay[j])) for j in range(int(fix_off[i]), int(fix_off[i + 1])) if float(fix_tp[j]) > 0.0]
        coupons = [(float(cpn["tp"][j]), float(cpn["ts"][j]), float(cpn["te"][j]), _mp(cpn["scale"][j]), _mp(cpn["spread"][j]))
                   for j in range(int(cpn_off[i]), int(cpn_off[i + 1])) if float(cpn["tp"][j]) > 0.0]
        n_terms = len(fixed) + len(coupons)
        v_row, g_row = [], []
        for s in range(S):
            rd, ri = (s if S_disc == S else 0), (s if S_infl == S else 0)
            v, g, cond_d, cond_y = zero, zero, zero, zero
            for xt, pay in fixed:
                D, c = rows.date(xt, rd)
                cond_d = max(cond_d, c)
                v += pay * D
                g += abs(pay) * D
            for tp, ts, te, scale, spread in coupons:
                D, c = rows.date(tp, rd)
                cond_d = max(cond_d, c)
                if ts == te:
                    v += scale * spread * D
                    g += abs(scale) * abs(spread) * D
                else:
                    q, cy = index.ratio(ts, te, ri)
                    cond_y = max(cond_y, cy)
                    v += scale * ((q - 1) + spread) * D
                    g += abs(scale) * (q + 1 + abs(spread)) * D
            v_row.append(v)
            g_row.append(g)
            k[i, s] = bound_k(rows.method, n_terms, float(cond_d), float(cond_y))
        value.append(v_row)
        gross.append(g_row)
    return Reference(value, gross, k)
