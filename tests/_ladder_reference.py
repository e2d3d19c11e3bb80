"""The plain reference of the sub-book ladders (adr_subbook_ladders*, adr_credit_subbook_ladders*, adr_yoy_subbook_ladders*)
and the bound the kernels, their host twins and the C oracle are held to, entry by entry (tests/test_ladder_edges_host.py,
CPU, and tests/test_gpu_ladder_edges.py, GPU).  It shares no code with the kernels or with oracle/port.c.

The operation.  The inputs are what `DeviceCurve` and the `_host` entries take, each an exact binary number: the scheme,
the knot times x_k, the knot discount factors d_k, ``jac [K, P]`` = J, ``hess [K, P, P]`` = C, a `TradeBatch`, ``sub_off`` and,
for credit, ``z``, ``bucket``, the spread times and ``G``.  A desk's PV is a sum of TERMS c D(t), one per cash flow and NOT
folded into nodes (oracle/mp_oracle.py's value level):
  fixed flow, counts when tp > 0:            c = fix_sign fix_pay at tp
  float coupon, counts when tp >= 0:         N w sign ((D(ts) / D(te) - 1 when alpha > 0) + spread alpha) D(tp), w the coupon's
                                             weight (1 without weights).  With te == tp (all the ladders take)
                                             D(ts) / D(te) D(tp) = D(ts) and the coupon is  +c at ts,  -c at tp  (both only when
                                             alpha > 0)  and  c spread alpha at tp, c = sn w.  With te != tp (payment lag; the
                                             pricing kernels only, tests/_price_reference.py) the first term is the RATIO term
                                             c D(ts) D(tp) / D(te)  (below, "Ratio terms").
Credit multiplies every term of a flow by f = exp(-z tau) of that flow.  D(t) is simple_interp.hpp's lookup rule, its float64
decisions (snap within 1e-10 to the first of equal knots, else the segment and weight of t + 1e-12, clamped at the ends)
taken from `oracle.mp_oracle._lookup_plan`; with L_k = ln d_k
  FLAT_FWD_RATES     ln D = (1 - w) L_a + w L_b                            (a knot alone: L_k)
  LINEAR_ZERO_RATES  ln D = t (1 - w) / max(x_a, 1e-15) L_a + t w / x_b L_b  (a knot held at an end: t / max(x_k, 1e-15) L_k)
  LINEAR_FWD_RATES   D = (1 - w) d_a + w d_b.
Everything that depends on d runs in mpmath at 60 digits.  The derivatives are analytic in the L_k: g_k = dPV/dL_k and the
banded H_kl = d2PV/dL_k dL_l, then with LJ = J / d and LC_k = C_k / d_k - J_k J_k^T / d_k^2
  delta = 1e-4 LJ^T g,      gamma = 1e-8 (LJ^T H LJ + sum_k g_k LC_k),
and for credit cs01 = 1e-4 dPV/dz, spread_gamma = 1e-8 d2PV/dz2, cross = 1e-4 d delta/dz per (desk, bucket) cell, from the
terms' amounts times -tau and tau^2.  The projection is done in exact integer arithmetic: g_k / d_k, g_k / d_k^2 and
H_kl / (d_k d_l) are formed in mpmath and taken apart into integer mantissas on one exponent without any rounding, J and C
are exact integers times a power of two, and the sums are Python integers (object arrays).  1e-4 and 1e-8 stay exact: a
result is an integer V with value = V 2^E / 10^s.

Ratio terms.  Log schemes: om = c exp(sum_k u_k L_k) with u the sum of the knot weights of ts (+), te (-) and tp (+) - up to six
knots, so H is not banded -, g_k += om u_k and H_kl += om u_k u_l.  Its gross takes the weights as written, before the merge:
|om| W_k and |om| W_k W_l with W_k the sum of the three dates' absolute weights at knot k (a two-day lag that puts te and tp in
one interval counts -b(te) + b(tp) as cancellation against gross, as the inflation side does for ts and te on one knot).
LINEAR_FWD_RATES: f = c S P / E with S, E, P linear in the d_k (weights s, e, p); the reduced form, which has no product of
two weights of one date but e's,
  df/dd_k = f (s_k / S - e_k / E + p_k / P)
  d2f/dd_k dd_l = f [(s_k p_l + p_k s_l) / (S P) - (s_k e_l + e_k s_l) / (S E) - (p_k e_l + e_k p_l) / (P E) + 2 e_k e_l / E^2]
brought into the L_k as the plain term is: g_k = d_k df/dd_k, H_kl = d_k d_l d2f/dd_k dd_l + [k == l] g_k.  Its gross is the sum
of the absolute values of exactly these terms, so an entry reached only through s_k s_l of one date has gross 0 and must be
+0.0.  ``cond`` of a ratio term: the sum of |weight L_k| over its three dates (LINEAR_FWD_RATES: the largest |L_k|).

Gross.  Every element comes with ``gross``: the sum of the absolute values of its terms written in the inputs - |c| f D(t)
through the absolute interpolation weights, and the tables as |J| / d, |C| / d and |J J^T| / d^2 separately, so the
subtraction inside LC counts as cancellation against gross.  It is computed by the same exact integer arithmetic on the
absolute values.  An element with gross == 0 must be +0.0.

The bound |got - value| <= k 2^-53 gross, k = `bound_k`.  Each rounding below is counted as ONE unit 2^-53 of the absolute
sum it acts on (twice the unit roundoff 2^-54, which pays for every second-order term), a library function with a documented
error of one ulp as TWO units (an ulp is at most 2^-52 of the value).  As the code performs them
(subbook_ladder_common.hpp, simple_interp.hpp, curve_tables.cpp):
  amount    sn (spread alpha - 1): 3 roundings; the next coupon's start and the fixed flow joined: 2 more            5
  weight    e_w roundings of a lookup weight formed from w (w itself is the plan's float64 number, the same expression
            in the code): FLAT_FWD 1 - w: 1;  LINEAR_ZERO t (1 - w) / x_a: 3;  LINEAR_FWD 1 - w: 1
  argument  (log schemes) s = wa L_a + wb L_b: L = log(d) from the table builder (2), the weight (e_w), a product (1), the
            sum (1), all relative to |wa L_a| + |wb L_b| <= cond, and an absolute error of s is a relative one of exp(s):
                                                                                                     cond (e_w + 4)
            (LINEAR_FWD) exp(L_k) on L_k = log(d_k): the table's log (2) conditioned by |L_k| <= cond:      2 cond
  exp       the device's and the host's exp, documented at one ulp or better                                          2
  products  (log schemes) amount exp(s): 1; om wa, (om wa) wa or (om wa) wb: 2, each with the weight's error again: 2 e_w
                                                                                                        1 + 2 + 2 e_w
            (LINEAR_FWD) 1 - w (e_w), amount (1 - w), the product with exp(L)                                 e_w + 2
  credit    f = exp(-(z tau)): the product conditioned by |z tau| <= zt, exp (2); x f (1); (-tau) xf (1) or
            tau (tau xf) (2)                                                                                   zt + 5
  sums      a knot's slot and the pv take the desk's nodes one after another inside a chunk, the chunk records go to 64
            slots and down a halving tree of 6 levels: any order of n numbers costs n - 1 roundings, the nodes number at
            most the desk's unfolded terms n_terms                                                        n_terms + 7
            credit sums chunks to cells and cells to desks: the second reduction                                   + 7
  tables    LJ = J / d: 1;  LC = C / d - LJ LJ: C / d (1), LJ LJ (2 + 1), the difference (1): at most 4 against
            |C| / d + |J J| / d^2
  project   the worst of the three terms of `gamma_step`: (D_k LJ) LJ: 2 (tables) + 2;  O_k (LJ LJ + LJ LJ): 2 + 1 + 1 + 1;
            w_k LC: 4 + 1                                                                                            5
            the adds: three per knot, a wave takes every eighth knot, then eight partial sums in order
                                                                                              3 ceil(Kc / 8) + 7
  scale     the constant 1e-4 or 1e-8 is not a binary number (1), the product (1)                                   2
Kc is the compact grid's length, read off the knot times: the first and the last knot of every run of equal times
(`compact_count`).  `bound_k` adds these and rounds the two conditioned terms up to an integer; the
same k is used for every element of a desk (pv and delta have fewer roundings than gamma).  cond and zt are read off the
inputs by the reference: the largest sum of |weight L_k| over the desk's terms and the largest |z tau|.

Inflation (adr_yoy_subbook_ladders*, `yoy_reference`).  The inputs add the inflation scheme, the pillar
times T_k and the breakeven rates b_k, fixed flows (tp, pay) and coupons (tp, ts, te, scale, spread).  The inflation nodes are
L_0 = 0 at x = 0 and L_k = T_k ln(1 + b_k); a coupon has ln(1 + y) = sum of w L_k over the slots of te (+w) and of ts (-w),
with the weights of `si::log_weights` on `_lookup_plan`'s float64 decisions on x = [0, T]: a snap 1; FLAT_FWD 1 - w and w;
LINEAR_ZERO t (1 - w) / max(x_a, 1e-15) and t w / x_b; a held end t / max(x_k, 1e-15) or 1; node 0 is left out.  It pays
amount = scale ((1 + y) - 1 + spread) at tp and counts when tp > 0, a fixed flow when tp > 0.  On the discount side both are
terms c D(tp) of the sums above (no division by D(0): the kernels have none), which gives pv, delta[:P_d] and
gamma[:P_d, :P_d].  On the inflation side, with g = scale (1 + y) D(tp), u_k = (sum of the slots' w at k) T_k / (1 + b_k)
and v_k = -(that sum) T_k / (1 + b_k)^2:
  delta[P_d + k] = 1e-4 sum g u_k,      gamma[P_d + k][P_d + l] = 1e-8 sum g (u_k u_l + [k == l] v_k),
and row k of the cross block is the projected delta, at 1e-8, of the first-order sums of the terms scale (1 + y) u_k D(tp)
(as credit's cross_gamma); both mirror positions are compared.  Gross takes the terms as written: the amount counts as
|scale| ((1 + y) + 1 + |spread|), a slot sum as sum |w| - before the merge of two slots on one knot, so where ts and te share a
knot the difference we.w - ws.w is cancellation -, u_k u_l and v_k separately, D(tp) and the tables as above.
The roundings the inflation side adds to a node's count above, as yoy_nodes.hpp and yoy_subbook_ladder.hip perform them
(e_w of the INFLATION scheme, W_k = sum |w| at knot k):
  make_node 1 + b_k (1): an ABSOLUTE error of one unit of ln(1 + b_k), so T_k units of L_k; log (2) and the product (1):
            3 |L_k|.  L' = T / (1 + b): 2;  L'' = -(T / ((1 + b) (1 + b))): 4
  describe  a coefficient: the weight (e_w) and the merge add (1), of W_k;  lnr = sum c_k L_k: the coefficient
            (e_w + 1) W_k |L_k|, the node W_k (T_k + 3 |L_k|), the product (1) and at most three adds (3) of
            sum W_k |L_k|: an absolute error of lnr, hence a relative one of 1 + y
                                                           cond_i = max over the coupons of sum W_k (T_k + (e_w + 8) |L_k|)
            exp                                                                                                        2
            the amount: (1 + y) - 1, + spread, scale x: 3 roundings of |scale| ((1 + y) + 1 + |spread|); less than what
            follows for a breakeven gamma entry, and one k serves the desk
            g = (scale 1.0) (1 + y) on the unit grid (1), times E = D(tp) in `add_coupon` (1; E itself: the node above)     2
            u = c L': e_w + 1, 2 and the product: e_w + 4;  v = c L'': e_w + 1, 4 and the product: e_w + 6
  gamma_term  u_k u_l: 2 (e_w + 4) + 1 of its gross;  v_k: e_w + 6 of its;  the add (1)                        2 e_w + 10
  add_coupon  g term (1); g u and (scale (1 + y)) u, s t.wa have fewer roundings than the line above                    1
  sums, cross_sum / delta_step, the tables and 1e-4 / 1e-8: the lines above (a desk's coupons and fixed flows are its
            n_terms; the breakeven blocks are scaled by one product each)
so `bound_k(..., infl=(scheme, cond_i))` adds ceil(cond_i) + 2 e_w + 15.  cond_i is large beside the rest - a coupon far out
on the curve has sum W_k T_k of 40 and more, because one rounding of 1 + b_k moves L_k by T_k units whatever ln(1 + b_k) is -
and k runs from about 70 to 800 on the edge books.  Nothing in it was fitted: the host twin's worst share is 0.12.
"""
import math

import numpy as np
from mpmath import mp, mpf

from oracle.mp_oracle import _lookup_plan

FLAT_FWD, LINEAR_FWD, LINEAR_ZERO = 1, 2, 4
_WEIGHT_ROUNDINGS = {FLAT_FWD: 1, LINEAR_FWD: 1, LINEAR_ZERO: 3}


def compact_count(times):
    """Kc: the knots that are the first or the last of a run of equal times."""
    x = np.asarray(times, dtype=np.float64)
    first = np.concatenate([[True], x[1:] != x[:-1]])
    last = np.concatenate([x[1:] != x[:-1], [True]])
    return int(np.count_nonzero(first | last))


def bound_k(method, n_terms, K, cond, zt=None, infl=None):
    """k of the module docstring: ``n_terms`` unfolded live terms of the desk, ``K`` = Kc knots, ``cond`` the largest
    sum |weight L_k| of a term, ``zt`` the largest |z tau| (credit; None for the rates ladders), ``infl`` =
    (inflation scheme, cond_i) with cond_i the largest  sum |w| (T_k + (e_w + 8) |L_k|)  over a coupon's inflation slots
    (inflation; None otherwise)."""
    e_w = _WEIGHT_ROUNDINGS[int(method)]
    amount, exp_ulp, tables_project, scale = 5, 2, 5, 2
    if int(method) == LINEAR_FWD:
        node = amount + math.ceil(2 * cond) + exp_ulp + (e_w + 2)
    else:
        node = amount + math.ceil(cond * (e_w + 4)) + exp_ulp + (1 + 2 + 2 * e_w)
    sums = n_terms + 7
    if zt is not None:
        node += math.ceil(zt) + 5
        sums += 7
    if infl is not None:
        node += math.ceil(infl[1]) + 2 + 2 + (2 * _WEIGHT_ROUNDINGS[int(infl[0])] + 10) + 1
    return node + sums + tables_project + 3 * ((K + 7) // 8) + 7 + scale


# ------------------------------------------------------------------------------------------------ exact integer helpers
def _mp(x):
    return mpf(float(x))


def _float_ints(a):
    """``(ints, e)``: the float64 array as Python integers with ``a == ints * 2 ** e`` exactly."""
    a = np.asarray(a, dtype=np.float64)
    m, ex = np.frexp(a)
    nz = a != 0.0
    lo = (int(ex[nz].min()) if np.any(nz) else 0) - 53
    m = (m * 2.0 ** 53).astype(np.int64)
    out = np.array([int(mm) << (int(ee) - 53 - lo) if mm else 0 for mm, ee in zip(m.ravel(), ex.ravel())], dtype=object)
    return out.reshape(a.shape), lo


def _mp_ints(values):
    """``(ints [n], e)``: mpf numbers as integers on one exponent, exactly (an mpf is mantissa * 2 ** exponent)."""
    parts = []
    for v in values:
        sign, man, ex, _ = mpf(v)._mpf_
        parts.append((-int(man) if sign else int(man), int(ex)))
    live = [ex for man, ex in parts if man]
    lo = min(live) if live else 0
    return np.array([man << (ex - lo) if man else 0 for man, ex in parts], dtype=object), lo


def _align(pieces):
    """The sum of ``(ints, e)`` pieces on their lowest exponent."""
    lo = min(e for _, e in pieces)
    total = 0
    for ints, e in pieces:
        total = total + ints * (1 << (e - lo))
    return total, lo


class Block:
    """Elements ``value = V 2^E / 10^s`` and ``gross = A 2^E / 10^s`` (``V``, ``A``: object arrays of Python integers)."""

    def __init__(self, V, A, E, s):
        self.V, self.A, self.E, self.s = np.asarray(V, dtype=object), np.asarray(A, dtype=object), E, s

    @staticmethod
    def of(value_piece, gross_piece, s):
        (v, ev), (a, ea) = value_piece, gross_piece
        lo = min(ev, ea)
        return Block(v * (1 << (ev - lo)), a * (1 << (ea - lo)), lo, s)

    def floats(self):
        """The values rounded to float64 (for reading and for comparisons that need no exactness)."""
        f = np.vectorize(lambda v: float(mpf(int(v)) * mpf(2) ** self.E / mpf(10) ** self.s), otypes=[np.float64])
        return f(self.V)

    def gross_floats(self):
        f = np.vectorize(lambda v: float(mpf(int(v)) * mpf(2) ** self.E / mpf(10) ** self.s), otypes=[np.float64])
        return f(self.A)

    def share(self, got, k, what=""):
        """The worst |got - value| / (k 2^-53 gross) over the elements, in exact integer arithmetic up to the final
        quotient; asserts that an element with gross == 0 is +0.0."""
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == self.V.shape, (what, got.shape, self.V.shape)
        assert np.all(np.isfinite(got)), f"{what}: not finite"
        m, ex = np.frexp(got)
        m = (m * 2.0 ** 53).astype(np.int64)
        worst = 0.0
        ten = 10 ** self.s
        for idx in np.ndindex(got.shape):
            V, A = int(self.V[idx]), int(self.A[idx])
            if A == 0:
                assert got[idx] == 0.0 and not np.signbit(got[idx]), f"{what}{list(idx)}: gross is 0 but the entry is {got[idx]!r}"
                continue
            sh = int(ex[idx]) - 53 - self.E                 # got 10^s / 2^E = m ten 2^sh
            g = int(m[idx]) * ten
            if sh >= 0:
                err, scale = abs((g << sh) - V), A
            else:
                err, scale = abs(g - (V << -sh)), A << -sh
            worst = max(worst, ((err << 83) // (k * scale)) / 2.0 ** 30)      # err 2^53 / (k gross), 30 binary digits kept
        return worst


    def between(self, a, b, k):
        """The worst |a - b| / (k 2^-53 gross) of two results, exactly; where gross is 0 both must be +0.0 (`share` says so
        of each)."""
        from fractions import Fraction
        a, b = np.asarray(a, dtype=np.float64).reshape(self.V.shape), np.asarray(b, dtype=np.float64).reshape(self.V.shape)
        unit = Fraction(k, 2 ** 53) * Fraction(2) ** self.E / 10 ** self.s
        worst = 0.0
        for idx in np.ndindex(a.shape):
            if a[idx] != b[idx]:
                assert int(self.A[idx]) != 0, idx
                worst = max(worst, float(abs(Fraction(float(a[idx])) - Fraction(float(b[idx]))) / (unit * int(self.A[idx]))))
        return worst


# ------------------------------------------------------------------------------------------------------------ the curve
class _Curve:
    def __init__(self, method, times, dfs, jac, hess):
        self.method = int(method)
        self.x = np.ascontiguousarray(times, dtype=np.float64)
        self.K = self.x.size
        self.d = [_mp(v) for v in np.asarray(dfs, dtype=np.float64)]
        self.L = [mp.log(v) for v in self.d]
        self.J = np.ascontiguousarray(jac, dtype=np.float64).reshape(self.K, -1)
        self.P = self.J.shape[1]
        self.C = None if hess is None else np.ascontiguousarray(hess, dtype=np.float64).reshape(self.K, self.P, self.P)
        self._dates = {}

    def date(self, t):
        """``(D, [(k, weight)], pieces)`` of one date: log schemes D = exp(sum weight L_k) and ``pieces`` is None;
        LINEAR_FWD_RATES D = sum of the pieces ``(k, share d_k)``.  ``cond``: sum |weight L_k| (LINEAR_FWD: max |L_k|)."""
        t = float(t)
        if t in self._dates:
            return self._dates[t]
        plan = _lookup_plan(self.x, t, self.method)
        x, m = self.x, self.method
        if plan[0] == "snap":
            knots = [(plan[1], mpf(1))]
        elif plan[0] == "flat":
            k = plan[1]
            knots = [(k, _mp(t) / _mp(max(float(x[k]), 1e-15)) if m == LINEAR_ZERO else mpf(1))]
        else:
            _, a, b, w = plan
            w = _mp(w)
            if m == LINEAR_ZERO:
                knots = [(a, _mp(t) * (1 - w) / _mp(max(float(x[a]), 1e-15))), (b, _mp(t) * w / _mp(max(float(x[b]), 1e-15)))]
            else:
                knots = [(a, 1 - w), (b, w)]
            knots = [(k, wk) for k, wk in knots if wk != 0]
        if m == LINEAR_FWD:
            pieces = [(k, wk * self.d[k]) for k, wk in knots]
            out = (sum((p for _, p in pieces), mpf(0)), knots, pieces, max(abs(self.L[k]) for k, _ in knots))
        else:
            s = sum((wk * self.L[k] for k, wk in knots), mpf(0))
            out = (mp.exp(s), knots, None, sum((abs(wk * self.L[k]) for k, wk in knots), mpf(0)))
        self._dates[t] = out
        return out


class _Sums:
    """pv, g_k and H_kl of a set of terms, and the same of their absolute values."""

    def __init__(self, curve, second):
        self.cv, self.second = curve, second
        self.pv, self.pv_abs = mpf(0), mpf(0)
        self.g, self.g_abs, self.H, self.H_abs = {}, {}, {}, {}
        self.n, self.cond = 0, mpf(0)

    def add(self, t, c, gross=None):
        """The term ``c D(t)``; ``gross``: what |c| counts as where c was formed by subtractions (default |c|)."""
        a = abs(c) if gross is None else gross
        if c == 0 and a == 0:
            return
        D, knots, pieces, cond = self.cv.date(t)
        self.n += 1
        self.cond = max(self.cond, cond)
        bump = lambda table, key, v: table.__setitem__(key, table.get(key, mpf(0)) + v)
        if pieces is not None:                              # LINEAR_FWD_RATES: two single-knot amounts, weight 1
            for k, p in pieces:
                v, va = c * p, a * abs(p)
                self.pv += v
                self.pv_abs += va
                bump(self.g, k, v)
                bump(self.g_abs, k, va)
                if self.second:
                    bump(self.H, (k, k), v)
                    bump(self.H_abs, (k, k), va)
            return
        om, oa = c * D, a * D
        self.pv += om
        self.pv_abs += oa
        for k, wk in knots:
            bump(self.g, k, om * wk)
            bump(self.g_abs, k, oa * abs(wk))
            if self.second:
                for l, wl in knots:
                    bump(self.H, (k, l), om * wk * wl)
                    bump(self.H_abs, (k, l), oa * abs(wk * wl))

    def add_ratio(self, ts, te, tp, c):
        """The ratio term ``c D(ts) D(tp) / D(te)`` (module docstring, "Ratio terms")."""
        if c == 0:
            return
        dates = [self.cv.date(t) for t in (ts, te, tp)]
        signs = (1, -1, 1)
        (Ds, _, ps, _), (De, _, pe, _), (Dp, _, pp, _) = dates
        om = c * Ds * Dp / De
        oa = abs(om)
        self.n += 1
        self.pv += om
        self.pv_abs += oa
        bump = lambda table, key, v: table.__setitem__(key, table.get(key, mpf(0)) + v)
        if ps is not None:                                  # LINEAR_FWD_RATES: the reduced form on the shares of S, E, P
            self.cond = max(self.cond, max(d[3] for d in dates))
            sh = [{k: p / D for k, p in pieces} for (D, _, pieces, _) in dates]          # s_k d_k / S, e_k d_k / E, p_k d_k / P
            for sg, part in zip(signs, sh):
                for k, v in part.items():
                    bump(self.g, k, sg * om * v)
                    bump(self.g_abs, k, oa * v)
                    if self.second:
                        bump(self.H, (k, k), sg * om * v)
                        bump(self.H_abs, (k, k), oa * v)
            if self.second:
                s_, e_, p_ = sh
                for a, b, coef in ((s_, p_, 1), (s_, e_, -1), (p_, e_, -1)):
                    for k, vk in a.items():
                        for l, vl in b.items():
                            for key in ((k, l), (l, k)):
                                bump(self.H, key, coef * om * vk * vl)
                                bump(self.H_abs, key, oa * vk * vl)
                for k, vk in e_.items():
                    for l, vl in e_.items():
                        bump(self.H, (k, l), 2 * om * vk * vl)
                        bump(self.H_abs, (k, l), 2 * oa * vk * vl)
            return
        self.cond = max(self.cond, sum((d[3] for d in dates), mpf(0)))
        u, W = {}, {}
        for sg, (_, knots, _, _) in zip(signs, dates):
            for k, wk in knots:
                bump(u, k, sg * wk)
                bump(W, k, abs(wk))
        for k in u:
            bump(self.g, k, om * u[k])
            bump(self.g_abs, k, oa * W[k])
            if self.second:
                for l in u:
                    bump(self.H, (k, l), om * u[k] * u[l])
                    bump(self.H_abs, (k, l), oa * W[k] * W[l])

    def add_term(self, t, c):
        """A term of `trade_terms`: a date, or the three dates of a ratio term."""
        if isinstance(t, tuple):
            self.add_ratio(*t, c)
        else:
            self.add(t, c)

    # -------------------------------------------------------------------------------------------------- projection
    def _project(self, g, H, J, C, sign, second):
        """``(delta piece, gamma piece or None)`` as ``(ints, e)`` before the powers of ten."""
        cv = self.cv
        ks = sorted(g)
        P = cv.P
        if not ks:
            zero = np.array([0] * P, dtype=object)
            return (zero, 0), ((np.array([0] * (P * P), dtype=object).reshape(P, P), 0) if second else None)
        Jk, eJ = J
        Jk = Jk[ks]
        gt, eg = _mp_ints([g[k] / cv.d[k] for k in ks])
        delta = (np.dot(gt, Jk), eg + eJ)
        if not second:
            return delta, None
        pos = {k: i for i, k in enumerate(ks)}
        g2, eg2 = _mp_ints([g[k] / (cv.d[k] * cv.d[k]) for k in ks])
        keys = sorted(H)
        ht, eH = _mp_ints([H[key] / (cv.d[key[0]] * cv.d[key[1]]) for key in keys])
        M = np.array([[0] * P for _ in ks], dtype=object)                    # Ht J, Ht banded
        for (k, l), v in zip(keys, ht):
            M[pos[k]] = M[pos[k]] + v * Jk[pos[l]]
        Ck, eC = C
        Ck = Ck[ks].reshape(len(ks), P * P)
        pieces = [(np.dot(Jk.T, M), eH + 2 * eJ), (np.dot(gt, Ck).reshape(P, P), eg + eC),
                  (sign * np.dot(Jk.T, g2[:, None] * Jk), eg2 + 2 * eJ)]
        return delta, _align(pieces)

    def blocks(self, tables, delta_scale=4, gamma_scale=8):
        """``(pv, delta, gamma)`` Blocks (gamma None without the second order)."""
        J, Ja, C, Ca = tables
        second = self.second and C is not None
        dv, gv = self._project(self.g, self.H, J, C, -1, second)
        da, ga = self._project(self.g_abs, self.H_abs, Ja, Ca, +1, second)
        pv = Block.of(_mp_ints([self.pv]), _mp_ints([self.pv_abs]), 0)
        return pv, Block.of(dv, da, delta_scale), (Block.of(gv, ga, gamma_scale) if second else None)


def _tables(cv):
    J = _float_ints(cv.J)
    Ja = (abs(J[0]), J[1])
    if cv.C is None:
        return J, Ja, None, None
    C = _float_ints(cv.C)
    return J, Ja, C, (abs(C[0]), C[1])


# ------------------------------------------------------------------------------------------------------------ the terms
def trade_terms(batch, i, z=None, fix_tau=None, flt_tau=None):
    """The unfolded terms ``(t, c, tau)`` of trade ``i`` (c an mpf, the spread factor not applied; tau None without
    spreads).  ``t`` is a date, or - an accruing coupon paid on another date than its accrual end - the tuple (ts, te, tp)
    of the ratio term c D(ts) D(tp) / D(te) (`_Sums.add_term`); with spreads (the credit ladders) such a coupon is out of
    scope.  A coupon's weight multiplies its c."""
    out = []
    for j in range(int(batch.fix_off[i]), int(batch.fix_off[i + 1])):
        tp = float(batch.fix_tp[j])
        if tp > 0.0:
            out.append((tp, _mp(batch.fix_sign[i]) * _mp(batch.fix_pay[j]), None if fix_tau is None else float(fix_tau[j])))
    sn = _mp(batch.flt_sign[i]) * _mp(batch.notional[i])
    for j in range(int(batch.flt_off[i]), int(batch.flt_off[i + 1])):
        tp, ts, te, al = (float(getattr(batch, name)[j]) for name in ("flt_tp", "flt_ts", "flt_te", "flt_alpha"))
        if al > 0.0 and z is not None:
            assert te == tp, "a ratio node: out of scope"
        if not tp >= 0.0:
            continue
        tau = None if flt_tau is None else float(flt_tau[j])
        c = sn if batch.flt_weight is None else sn * _mp(batch.flt_weight[j])
        if al > 0.0:
            out.append((ts if te == tp else (ts, te, tp), c, tau))
            out.append((tp, -c, tau))
        out.append((tp, c * _mp(batch.spread[i]) * _mp(al), tau))
    return [term for term in out if term[1] != 0]


def _key(*arrays):
    return tuple(None if a is None else (np.ascontiguousarray(a).tobytes(), np.asarray(a).shape) for a in arrays)


_BATCH_FIELDS = ("fix_off", "flt_off", "fix_tp", "fix_pay", "flt_tp", "flt_ts", "flt_te", "flt_alpha", "notional", "spread",
                 "fix_sign", "flt_sign", "flt_weight")
_CACHE = {}


def _cached(kind, method, host, batch, extra, build):
    key = (kind, int(method)) + _key(host.times, host.dfs, host.jac, host.hess, *[getattr(batch, f) for f in _BATCH_FIELDS], *extra)
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


def rates_reference(method, host, batch, sub_off):
    """Per desk ``{"pv", "delta", "gamma": Block, "k": int, "n_terms": int}``; ``host``: an object with times, dfs, jac,
    hess.  Built once per process for the same inputs."""
    sub_off = np.asarray(sub_off, dtype=np.int64)

    def build():
        mp.dps = 60
        cv = _Curve(method, host.times, host.dfs, host.jac, host.hess)
        tables = _tables(cv)
        desks = []
        for lo, hi in zip(sub_off[:-1], sub_off[1:]):
            sums = _Sums(cv, True)
            for i in range(int(lo), int(hi)):
                for t, c, _ in trade_terms(batch, i):
                    sums.add_term(t, c)
            pv, delta, gamma = sums.blocks(tables)
            desks.append({"pv": pv, "delta": delta, "gamma": gamma, "n_terms": sums.n,
                          "k": bound_k(method, sums.n, compact_count(cv.x), float(sums.cond))})
        return desks
    return _cached("rates", method, host, batch, (sub_off,), build)


def credit_reference(method, host, case, G, sub_off):
    """Per desk the rates blocks AT THE SPREADS plus ``cs01``, ``spread_gamma`` ([G] Blocks) and ``cross_gamma`` ([G, P]);
    ``case``: batch, z, bucket, fix_tau, flt_tau."""
    sub_off = np.asarray(sub_off, dtype=np.int64)
    batch = case.batch

    def build():
        mp.dps = 60
        cv = _Curve(method, host.times, host.dfs, host.jac, host.hess)
        tables = _tables(cv)
        P = cv.P
        desks = []
        for lo, hi in zip(sub_off[:-1], sub_off[1:]):
            at = _Sums(cv, True)
            first = [_Sums(cv, False) for _ in range(G)]
            second = [_Sums(cv, False) for _ in range(G)]
            zt = mpf(0)
            for i in range(int(lo), int(hi)):
                z, g = _mp(case.z[i]), int(case.bucket[i])
                for t, c, tau in trade_terms(batch, i, case.z, case.fix_tau, case.flt_tau):
                    tau = _mp(tau)
                    zt = max(zt, abs(z * tau))
                    cf = c * mp.exp(-z * tau)
                    at.add(t, cf)
                    if g >= 0:
                        first[g].add(t, -tau * cf)
                        second[g].add(t, tau * tau * cf)
            pv, delta, gamma = at.blocks(tables)
            cs, csg, cross = [], [], []
            for g in range(G):
                pv1, d1, _ = first[g].blocks(tables, delta_scale=8)
                pv2, _, _ = second[g].blocks(tables)
                cs.append(Block(pv1.V, pv1.A, pv1.E, 4))
                csg.append(Block(pv2.V, pv2.A, pv2.E, 8))
                cross.append(d1)
            stack = lambda blocks, shape: _stack(blocks, shape)
            desks.append({"pv": pv, "delta": delta, "gamma": gamma, "cs01": stack(cs, (G,)), "spread_gamma": stack(csg, (G,)),
                          "cross_gamma": stack(cross, (G, P)), "n_terms": at.n,
                          "k": bound_k(method, at.n, compact_count(cv.x), float(at.cond), float(zt))})
        return desks
    return _cached("credit", method, host, batch, (case.z, case.bucket, case.fix_tau, case.flt_tau, np.array([G]), sub_off), build)


# ------------------------------------------------------------------------------------------------------------ inflation
def _infl_slots(x, t, im):
    """``[(k, weight)]`` of ln I(t) on the inflation nodes x = [0, T] (`si::log_weights` on `_lookup_plan`'s float64
    decisions, the weights in mpmath); node 0 has L = 0 and is left out, as the code drops it."""
    plan = _lookup_plan(x, t, im)
    held = lambda k: _mp(t) / _mp(max(float(x[k]), 1e-15)) if im == LINEAR_ZERO else mpf(1)
    if plan[0] == "snap":
        slots = [(plan[1], mpf(1))]
    elif plan[0] == "flat":
        slots = [(plan[1], held(plan[1]))]
    else:
        _, a, b, w = plan
        w = _mp(w)
        if im == LINEAR_ZERO:
            slots = [(a, _mp(t) * (1 - w) / _mp(max(float(x[a]), 1e-15))), (b, _mp(t) * w / _mp(float(x[b])))]
        else:
            slots = [(a, 1 - w), (b, w)]
    return [(k, wk) for k, wk in slots if k > 0 and wk != 0]


def _place(shape, parts, s):
    """A Block of ``shape`` (zeros elsewhere) from ``(index, Block)`` parts of scale ``s`` on their lowest exponent."""
    lo = min((b.E for _, b in parts), default=0)
    V, A = np.empty(shape, dtype=object), np.empty(shape, dtype=object)
    V.fill(0)
    A.fill(0)
    for idx, b in parts:
        assert b.s == s
        V[idx] = b.V * (1 << (b.E - lo))
        A[idx] = b.A * (1 << (b.E - lo))
    return Block(V, A, lo, s)


def _mp_block(values, gross, shape, s):
    """A Block of ``shape`` from mpf values and their gross, exactly."""
    (v, ev), (a, ea) = _mp_ints(values), _mp_ints(gross)
    return Block.of((v.reshape(shape), ev), (a.reshape(shape), ea), s)


def yoy_reference(method, host, infl, book, sub_off):
    """Per desk ``{"pv", "delta" [Q], "gamma" [Q, Q]: Block, "k", "n_terms"}`` on Q = P_d + P_i, the discount pillars first
    (module docstring, "Inflation").  ``infl`` = (scheme, T, b); ``book``: ``fixed`` = (fix_off, fix_tp, fix_pay) and
    ``coupons`` = cpn_off, tp, ts, te, scale, spread as the entries take them.  Built once per process for the same inputs."""
    sub_off = np.asarray(sub_off, dtype=np.int64)
    im, T, b = int(infl[0]), np.ascontiguousarray(infl[1], dtype=np.float64), np.ascontiguousarray(infl[2], dtype=np.float64)
    fix_off, fix_tp, fix_pay = (np.asarray(a) for a in book.fixed)
    cp = book.coupons

    def build():
        mp.dps = 60
        cv = _Curve(method, host.times, host.dfs, host.jac, host.hess)
        tables = _tables(cv)
        P, Pi = cv.P, T.size
        x = np.concatenate(([0.0], T))
        Tk = [mpf(0)] + [_mp(t) for t in T]
        ob = [mpf(1)] + [1 + _mp(v) for v in b]
        L = [tk * mp.log(o) for tk, o in zip(Tk, ob)]
        e_wi = _WEIGHT_ROUNDINGS[im]
        desks = []
        for lo, hi in zip(sub_off[:-1], sub_off[1:]):
            disc = _Sums(cv, True)
            cross = {}
            bd, bd_abs, bg, bg_abs = {}, {}, {}, {}
            bump = lambda table, key, v: table.__setitem__(key, table.get(key, mpf(0)) + v)
            n_terms, cond, cond_i = 0, mpf(0), mpf(0)
            for i in range(int(lo), int(hi)):
                for j in range(int(fix_off[i]), int(fix_off[i + 1])):
                    if float(fix_tp[j]) > 0.0 and float(fix_pay[j]) != 0.0:
                        disc.add(float(fix_tp[j]), _mp(fix_pay[j]))
                        n_terms += 1
                for j in range(int(cp["cpn_off"][i]), int(cp["cpn_off"][i + 1])):
                    tp, ts, te = float(cp["tp"][j]), float(cp["ts"][j]), float(cp["te"][j])
                    if not tp > 0.0:
                        continue
                    n_terms += 1
                    scale, spread = _mp(cp["scale"][j]), _mp(cp["spread"][j])
                    coef, W = {}, {}
                    for k, wk in _infl_slots(x, te, im) + [(k, -wk) for k, wk in _infl_slots(x, ts, im)]:
                        bump(coef, k, wk)
                        bump(W, k, abs(wk))
                    one_y = mp.exp(sum((coef[k] * L[k] for k in coef), mpf(0)))
                    cond_i = max(cond_i, sum((W[k] * (Tk[k] + (e_wi + 8) * abs(L[k])) for k in W), mpf(0)))
                    disc.add(tp, scale * (one_y - 1 + spread), gross=abs(scale) * (one_y + 1 + abs(spread)))
                    D, _, pieces, cd = cv.date(tp)
                    cond = max(cond, cd)
                    Da = D if pieces is None else sum((abs(p) for _, p in pieces), mpf(0))
                    g, ga = scale * one_y * D, abs(scale) * one_y * Da
                    u = {k: coef[k] * Tk[k] / ob[k] for k in coef}
                    ua = {k: W[k] * Tk[k] / ob[k] for k in coef}
                    for k in coef:
                        bump(bd, k, g * u[k])
                        bump(bd_abs, k, ga * ua[k])
                        for l in coef:
                            bump(bg, (k, l), g * u[k] * u[l])
                            bump(bg_abs, (k, l), ga * ua[k] * ua[l])
                        bump(bg, (k, k), -g * u[k] / ob[k])                 # v_k = -(sum w) T_k / (1 + b_k)^2
                        bump(bg_abs, (k, k), ga * ua[k] / ob[k])
                        if k not in cross:
                            cross[k] = _Sums(cv, False)
                        cross[k].add(tp, scale * one_y * u[k], gross=abs(scale) * one_y * ua[k])
            pv, d_disc, g_disc = disc.blocks(tables)
            cond = max([cond, disc.cond] + [c.cond for c in cross.values()])
            Q = P + Pi
            flat = lambda table, keys: [table.get(key, mpf(0)) for key in keys]
            ks, kl = list(range(1, Pi + 1)), [(k, l) for k in range(1, Pi + 1) for l in range(1, Pi + 1)]
            delta = _place((Q,), [(slice(0, P), d_disc), (slice(P, Q), _mp_block(flat(bd, ks), flat(bd_abs, ks), (Pi,), 4))], 4)
            parts = [((slice(0, P), slice(0, P)), g_disc),
                     ((slice(P, Q), slice(P, Q)), _mp_block(flat(bg, kl), flat(bg_abs, kl), (Pi, Pi), 8))]
            for k, sums in cross.items():
                row = sums.blocks(tables, delta_scale=8)[1]
                parts += [((P + k - 1, slice(0, P)), row), ((slice(0, P), P + k - 1), row)]
            desks.append({"pv": pv, "delta": delta, "gamma": _place((Q, Q), parts, 8), "n_terms": n_terms,
                          "k": bound_k(method, n_terms, compact_count(cv.x), float(cond), infl=(im, float(cond_i)))})
        return desks
    key = ("yoy", int(method), im) + _key(host.times, host.dfs, host.jac, host.hess, T, b, fix_off, fix_tp, fix_pay,
                                          *[cp[f] for f in ("cpn_off", "tp", "ts", "te", "scale", "spread")], sub_off)
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


def _stack(blocks, shape):
    """Blocks of one scale stacked along a new first axis, on their lowest exponent."""
    if not blocks:
        empty = np.empty(shape, dtype=object)
        return Block(empty, empty.copy(), 0, 0)
    lo = min(b.E for b in blocks)
    V = np.array([b.V * (1 << (b.E - lo)) for b in blocks], dtype=object).reshape(shape)
    A = np.array([b.A * (1 << (b.E - lo)) for b in blocks], dtype=object).reshape(shape)
    return Block(V, A, lo, blocks[0].s)


def worst_between(a, b, ref, blocks):
    """`Block.between` over every element of every desk."""
    return max((desk[name].between(a[name][i], b[name][i], desk["k"]) for i, desk in enumerate(ref) for name in blocks), default=0.0)


RATES_BLOCKS = ("pv", "delta", "gamma")
CREDIT_BLOCKS = RATES_BLOCKS + ("cs01", "spread_gamma", "cross_gamma")


def worst_share(got, ref, blocks=RATES_BLOCKS, what=""):
    """The worst share of the bound over every element of every desk; ``got[block][desk]`` against ``ref[desk][block]``."""
    worst = 0.0
    for b, desk in enumerate(ref):
        for name in blocks:
            g = np.asarray(got[name][b])
            worst = max(worst, desk[name].share(g.reshape(desk[name].V.shape), desk["k"], f"{what} desk {b} {name}"))
    return worst
