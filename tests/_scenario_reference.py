"""The plain reference of the scenario revaluation entries that price ordinary cash flows (adr_scenario_pv*,
adr_credit_scenario_pv* and the per-trade rows of their sub-book forms) and the bound the kernels, their host twins and the C
oracle are held to, element by element (tests/test_scenario_edges_host.py, CPU, and tests/test_gpu_scenario_edges.py, GPU).  It
follows tests/_ladder_reference.py and shares no code with the kernels or with oracle/port.c.

The operation.  The inputs are what the entries take, each an exact binary number: the scheme, the knot times x_k, the
scenario rows ``dfs [S, K]``, a `TradeBatch` and, for credit, ``z``, ``bucket``, ``fix_tau``, ``flt_tau`` and ``dz [S, G]`` (a
shared row of ``dfs`` or ``dz`` is read by every scenario).  For every pair (trade i, scenario s)
  value = sum over the fixed flows with xt > 0 of     fix_sign pay D(xt) f(tau_x)
        + sum over the float coupons with tp >= 0 of  flt_sign N w ((D(ts) / D(te) - 1 when alpha > 0, else 0) + spread alpha) D(tp) f(tau_p)
with w = flt_weight (1 without weights) and, for credit, f(tau) = exp(-x tau), x = z_i + dz[s][bucket_i] (no shock for
bucket -1; f = 1 without spreads).  D(t) is simple_interp.hpp's lookup rule on row s, its float64 decisions (snap within 1e-10
to the first of equal knots, else the segment and weight of t + 1e-12, held at the ends) taken from
`oracle.mp_oracle._lookup_plan`; with L_k = ln d_k
  FLAT_FWD_RATES     ln D = (1 - w) L_a + w L_b                            (a knot alone: L_k)
  LINEAR_ZERO_RATES  ln D = t (1 - w) / max(x_a, 1e-15) L_a + t w / x_b L_b  (a knot held at an end: t / max(x_k, 1e-15) L_k)
  LINEAR_FWD_RATES   D = (1 - w) d_a + w d_b.
Everything that depends on d runs in mpmath at 60 digits; D(t) is cached per distinct (date, row).

Gross.  ``gross`` is the same sum on absolute values with the terms as written: |N w| (D(ts) / D(te) + 1 + |spread alpha|)
D(tp) f for an accruing coupon, |N w| |spread alpha| D(tp) f for one that does not accrue, |pay| D(xt) f for a fixed flow.  An
element with gross == 0 (a trade with no live flow is one) must be +0.0.

The bound |got - value| <= k 2^-53 gross, k = `bound_k`, one k per (trade, scenario).  Each rounding is counted as ONE unit
2^-53 of the absolute sum it acts on (twice the unit roundoff, which pays for every second-order term), a library function
documented at one ulp as TWO units.  As the code performs them (scenario_common.hpp, simple_interp.hpp, scenario_pv.hip,
credit_scenario_pv.hip), per term of a trade:
  weight    e_w roundings of a lookup weight formed from w (w itself is the plan's float64 number, the same expression in
            the code): FLAT_FWD 1 - w: 1;  LINEAR_ZERO t (1 - w) / x_a: 3;  LINEAR_FWD none (w is used as it is)
  date      (log schemes) D = exp(wa T_a + wb T_b): T = log(d), taken by the host twin on the host and by the kernel on
            the device, in the LDS table or lane by lane on the global-table path (2), the weight (e_w), a product (1), the
            sum (1), all relative to cond = |wa L_a| + |wb L_b|, and an absolute error of the argument is a relative one
            of the exp; the exp itself (2); a snapped date is exp(1.0 log(d)) and counts the same
                                                                                          e_D = ceil(cond (e_w + 4)) + 2
            (LINEAR_FWD) D = d_a + w (d_b - d_a): the difference (1) and the product (1) act on w |d_b - d_a|, which may
            exceed D where the curve falls steeply across a segment, so they are conditioned by cond = w |d_b - d_a| / D;
            the sum (1)                                                                           e_D = ceil(2 cond) + 1
            cond is the largest over the trade's live dates on the scenario's row, read off the inputs by the reference.
  coupon    q = D(ts) / D(te): two dates and the division, 2 e_D + 1 of q;  q - 1 (1), spread alpha (1), + sa (1), each of
            at most q + 1 + |sa|;  * dp: the third date and the product, e_D + 1;  * w (1)                  3 e_D + 6
            (a fixed flow, pay * D(xt), has e_D + 1, and a coupon that does not accrue e_D + 3: less).  Where the code takes
            D(ts) from the previous coupon's D(te), D(tp) from D(te) or a fixed flow's D from the coupon's D(tp), it takes
            the number the date's own evaluation gives, so nothing is added
  credit    x = z + dz (1) and x * tau (1), both of |x tau| <= zt; under the log schemes exp(raw - xt), the difference
            (1) of at most cond + zt, the exp being the date's own; under LINEAR_FWD exp(-xt) (2) and raw * (1).  One
            count serves the three schemes and the oracle's rescaled amounts, which take np.exp(-x tau) as LINEAR_FWD does
                                                                                               ceil(3 zt + cond) + 3
  sums      the running sums a.fix and a.flt take the trade's live terms one after another and trade_pv joins the two: any
            order of n numbers costs at most n roundings with the first add to 0.0; (flt_sign N) * a.flt (1); fix_sign
            is +-1                                                                                      n_terms + 1
`bound_k` adds these.  zt is the largest |x tau| over the trade's live flows in the scenario.  Nothing in k is fitted to
what the kernels return; on the edge books k runs from 10 to 222 (tests/test_scenario_edges_host.py has the shares).
"""
import math

import numpy as np
from mpmath import mp, mpf

from oracle.mp_oracle import _lookup_plan

FLAT_FWD, LINEAR_FWD, LINEAR_ZERO = 1, 2, 4
_WEIGHT_ROUNDINGS = {FLAT_FWD: 1, LINEAR_FWD: 0, LINEAR_ZERO: 3}
DPS = 60


def date_roundings(method, cond):
    """e_D of the module docstring: the units of one D(t) whose conditioning is ``cond``."""
    if int(method) == LINEAR_FWD:
        return math.ceil(2 * cond) + 1
    return math.ceil(cond * (_WEIGHT_ROUNDINGS[int(method)] + 4)) + 2


def bound_k(method, n_terms, cond, zt=None):
    """k of the module docstring: ``n_terms`` live terms of the trade, ``cond`` the largest conditioning of one of its dates
    on the scenario's row, ``zt`` the largest |x tau| (credit; None for the rates entries)."""
    e_d = date_roundings(method, cond)
    k = 3 * e_d + 6 + n_terms + 1
    if zt is not None:
        k += math.ceil(3 * zt + cond) + 3
    return k


def _mp(x):
    return mpf(float(x))


class _Rows:
    """D(t) on the rows of ``dfs``, cached per (date, row)."""

    def __init__(self, method, times, dfs):
        self.method = int(method)
        self.x = np.ascontiguousarray(times, dtype=np.float64)
        self.dfs = np.ascontiguousarray(np.atleast_2d(dfs), dtype=np.float64)
        self._knot, self._plan, self._date = {}, {}, {}

    def knot(self, r, k):
        """``(d_k, ln d_k)`` of row r."""
        key = (r, k)
        if key not in self._knot:
            d = _mp(self.dfs[r, k])
            self._knot[key] = (d, mp.log(d))
        return self._knot[key]

    def plan(self, t):
        """``[(k, weight)]``: the knots of one date and their weights (of L_k under the log schemes, of d_k under
        LINEAR_FWD_RATES), the weights in mpmath on `_lookup_plan`'s float64 decisions."""
        if t in self._plan:
            return self._plan[t]
        x, m = self.x, self.method
        held = lambda k: _mp(t) / _mp(max(float(x[k]), 1e-15)) if m == LINEAR_ZERO else mpf(1)
        p = _lookup_plan(x, t, m)
        if p[0] == "snap":
            knots = [(p[1], mpf(1))]
        elif p[0] == "flat":
            knots = [(p[1], held(p[1]))]
        else:
            _, a, b, w = p
            if w == 0.0:                                    # the dx guard: the lower knot's ordinate held
                knots = [(a, held(a))]
            elif m == LINEAR_ZERO:
                w = _mp(w)
                knots = [(a, _mp(t) * (1 - w) / _mp(max(float(x[a]), 1e-15))), (b, _mp(t) * w / _mp(float(x[b])))]
            else:
                w = _mp(w)
                knots = [(a, 1 - w), (b, w)]
        self._plan[t] = knots
        return knots

    def date(self, t, r):
        """``(D, cond)`` of date t on row r."""
        key = (t, r)
        if key in self._date:
            return self._date[key]
        knots = self.plan(t)
        if self.method == LINEAR_FWD:
            D = sum((wk * self.knot(r, k)[0] for k, wk in knots), mpf(0))
            cond = mpf(0)
            if len(knots) == 2:
                (a, _), (b, w) = knots
                cond = abs(w) * abs(self.knot(r, b)[0] - self.knot(r, a)[0]) / D
        else:
            parts = [wk * self.knot(r, k)[1] for k, wk in knots]
            D = mp.exp(sum(parts, mpf(0)))
            cond = sum((abs(p) for p in parts), mpf(0))
        self._date[key] = (D, cond)
        return self._date[key]


def _trade_flows(batch, i, fix_tau, flt_tau):
    """The live flows of trade i: ``fixed`` = [(xt, amount, tau)] with the sign applied, ``coupons`` = [(ts, te, tp, accrues,
    sn w, spread alpha, tau)], amounts in mpmath."""
    fixed, coupons = [], []
    fs = _mp(batch.fix_sign[i])
    for j in range(int(batch.fix_off[i]), int(batch.fix_off[i + 1])):
        xt = float(batch.fix_tp[j])
        if xt > 0.0:
            fixed.append((xt, fs * _mp(batch.fix_pay[j]), None if fix_tau is None else _mp(fix_tau[j])))
    sn = _mp(batch.flt_sign[i]) * _mp(batch.notional[i])
    spread = _mp(batch.spread[i])
    for j in range(int(batch.flt_off[i]), int(batch.flt_off[i + 1])):
        tp = float(batch.flt_tp[j])
        if not tp >= 0.0:
            continue
        al = float(batch.flt_alpha[j])
        w = mpf(1) if batch.flt_weight is None else _mp(batch.flt_weight[j])
        coupons.append((float(batch.flt_ts[j]), float(batch.flt_te[j]), tp, al > 0.0, sn * w, spread * _mp(al),
                        None if flt_tau is None else _mp(flt_tau[j])))
    return fixed, coupons


class Reference:
    """``value`` and ``gross`` ([n][S] lists of mpf) and ``k`` ([n, S] integers) of one call."""

    def __init__(self, value, gross, k):
        self.value, self.gross, self.k = value, gross, k
        self.n, self.S = k.shape

    def _walk(self, got, what):
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == (self.S, self.n), (what, got.shape, (self.S, self.n))      # the wrappers' pv is [S, n]
        assert np.all(np.isfinite(got)), f"{what}: not finite"
        return got

    def share(self, got, what=""):
        """The worst |got - value| / (k 2^-53 gross) over the elements of ``got [S, n]``; asserts that an element with
        gross == 0 is +0.0."""
        got = self._walk(got, what)
        unit = mpf(2) ** -53
        worst = mpf(0)
        for i in range(self.n):
            for s in range(self.S):
                g = self.gross[i][s]
                if g == 0:
                    assert got[s, i] == 0.0 and not np.signbit(got[s, i]), f"{what} trade {i}, scenario {s}: gross is 0 but the entry is {got[s, i]!r}"
                    continue
                worst = max(worst, abs(_mp(got[s, i]) - self.value[i][s]) / (int(self.k[i, s]) * unit * g))
        return float(worst)

    def between(self, a, b, what=""):
        """The worst |a - b| / (k 2^-53 gross) of two results; where gross is 0 both must be equal (`share` says +0.0 of each)."""
        a, b = self._walk(a, what), self._walk(b, what)
        unit = mpf(2) ** -53
        worst = mpf(0)
        for s, i in zip(*np.nonzero(a != b)):
            g = self.gross[i][s]
            assert g != 0, (what, i, s)
            worst = max(worst, abs(_mp(a[s, i]) - _mp(b[s, i])) / (int(self.k[i, s]) * unit * g))
        return float(worst)

    def unit_err(self, got, notional):
        """The project's older metric, max |got - value| / max(1, |value|) per unit notional (for reading only)."""
        got = self._walk(got, "")
        unit = [abs(_mp(v)) or mpf(1) for v in notional]
        return max(float(abs(_mp(got[s, i]) - self.value[i][s]) / unit[i] / max(mpf(1), abs(self.value[i][s]) / unit[i]))
                   for i in range(self.n) for s in range(self.S))


_CACHE = {}
_BATCH_FIELDS = ("fix_off", "flt_off", "fix_tp", "fix_pay", "flt_tp", "flt_ts", "flt_te", "flt_alpha", "notional", "spread",
                 "fix_sign", "flt_sign", "flt_weight")


def _key(*arrays):
    return tuple(None if a is None else (np.ascontiguousarray(a).tobytes(), np.asarray(a).shape) for a in arrays)


def reference(method, times, dfs, batch, credit=None):
    """The `Reference` of one call; ``credit`` = (z, bucket, fix_tau, flt_tau, dz) or None for the rates entries, ``dfs`` and
    ``dz`` one shared row or one row per scenario.  Built once per process for the same inputs."""
    dfs = np.ascontiguousarray(np.atleast_2d(dfs), dtype=np.float64)
    if credit is not None:
        z, bucket, fix_tau, flt_tau, dz = credit
        dz = np.zeros((1, 0)) if dz is None else np.ascontiguousarray(np.atleast_2d(dz), dtype=np.float64)
        credit = (np.asarray(z, dtype=np.float64), np.asarray(bucket), np.asarray(fix_tau, dtype=np.float64),
                  np.asarray(flt_tau, dtype=np.float64), dz)
    key = (int(method),) + _key(times, dfs, *[getattr(batch, f) for f in _BATCH_FIELDS], *(credit or ()))
    if key not in _CACHE:
        _CACHE[key] = _build(int(method), times, dfs, batch, credit)
    return _CACHE[key]


def _build(method, times, dfs, batch, credit):
    mp.dps = DPS
    rows = _Rows(method, times, dfs)
    S_disc = dfs.shape[0]
    S = S_disc if credit is None else max(S_disc, credit[4].shape[0])
    assert S_disc in (1, S) and (credit is None or credit[4].shape[0] in (1, S))
    n = batch.n_trades
    value, gross = [], []
    k = np.zeros((n, S), dtype=np.int64)
    zero, one = mpf(0), mpf(1)
    for i in range(n):
        fixed, coupons = _trade_flows(batch, i, *(credit[2:4] if credit is not None else (None, None)))
        n_terms = len(fixed) + len(coupons)
        v_row, g_row = [], []
        for s in range(S):
            r = s if S_disc == S else 0
            x = None
            if credit is not None:
                z, bucket, _, _, dz = credit
                x = _mp(z[i])
                if int(bucket[i]) >= 0:
                    x = x + _mp(dz[s if dz.shape[0] == S else 0, int(bucket[i])])
            factors = {}

            def f(tau):
                if x is None or x == 0:
                    return one
                if tau not in factors:
                    factors[tau] = mp.exp(-x * tau)
                return factors[tau]
            v, g, cond, zt = zero, zero, zero, zero
            for xt, amount, tau in fixed:
                D, c = rows.date(xt, r)
                cond = max(cond, c)
                term = amount * D * f(tau)
                v += term
                g += abs(term)
                if x is not None:
                    zt = max(zt, abs(x * tau))
            for ts, te, tp, accrues, snw, sa, tau in coupons:
                Dp, c = rows.date(tp, r)
                cond = max(cond, c)
                pay = Dp * f(tau)
                if accrues:
                    (Ds, cs), (De, ce) = rows.date(ts, r), rows.date(te, r)
                    cond = max(cond, cs, ce)
                    q = Ds / De
                    v += snw * ((q - 1) + sa) * pay
                    g += abs(snw) * (q + 1 + abs(sa)) * pay
                else:
                    v += snw * sa * pay
                    g += abs(snw) * abs(sa) * pay
                if x is not None:
                    zt = max(zt, abs(x * tau))
            v_row.append(v)
            g_row.append(g)
            k[i, s] = bound_k(method, n_terms, float(cond), None if credit is None else float(zt))
        value.append(v_row)
        gross.append(g_row)
    return Reference(value, gross, k)
