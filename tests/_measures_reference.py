"""The plain reference of the bond and FRN measures entries (adr_bond_measures*, adr_frn_measures*) and the bound the kernels and
their host twins are held to, output by output (tests/test_measures_reference_host.py, CPU, and
tests/test_gpu_measures_reference.py, GPU).  It follows tests/_scenario_reference.py and tests/_ladder_reference.py and shares no
code with the kernels, with `interpolator._point` or with the numpy restatement of tests/_measures_cases.py.

The operation.  The inputs are the arrays the entries take, each read as an exact binary number; everything below runs in
mpmath at 60 digits.  b is the double nearest 1e-4, `small` the double nearest 1e-10.

D(t) on a node table (x_k, d_k), L_k = ln d_k - node_df.hpp's rule.  i is the first node with x_i >= t, n beyond the last
node; the comparisons are between doubles, so the choice is exact.
  t == x_0            d_0 as it stands (no rounding);  t < x_0: NaN
  LINEAR_ZERO_RATES   D = exp(t ((b - t) L_p / x_p + (t - a) L_q / x_q) / (b - a)):  first segment (i = 1) p = q = 1 (the first
                      node's zero rate held), a, b = x_0, x_1;  interior p, q = i - 1, i, a, b = x_p, x_q;  beyond the last node
                      p = q = n - 1 (the last node's zero rate held), a, b = x_{n-2}, x_{n-1}
  FLAT_FWD_RATES      D = exp(((x_q - t) L_p + (t - x_p) L_q) / (x_q - x_p)), p, q = i - 1, i, beyond the last node n - 2, n - 1
  LINEAR_FWD_RATES    first segment D = exp(t ln(d_1 + small) / (x_1 + small));  else with G_1 = L_{i-1} - L_{i-2}, h_1 = x_{i-1}
                      - x_{i-2}, G_2 = L_i - L_{i-1}, h = x_i - x_{i-1}:  D = d_{i-1} exp(w_1 G_1 + w_2 G_2), w_1 = (x_i - t)(t -
                      x_{i-1}) / (h h_1), w_2 = (t - x_{i-1})^2 / h^2;  beyond the last node D = d_{n-1} exp(w_1 G_1), w_1 = (t -
                      x_{n-1}) / h_1
A date exactly on a node x_i, i >= 1, takes the segment that ends there; nothing is special about it.

Bonds.  A_i = (cpn_i + max(prin_i, 0)) D(T_i) / D(T_s), P(x) = sum A_i exp(-x tau_i); dirty = 100 P(z) / face, clean = dirty -
acc100, dv01 = (P(z - b) - P(z + b)) / 2.  Y(y) = sum cpn_i exp(-y tau_i), plus face exp(-y tau_M) when tau_M > 0; the yield
solves Y(y) = P(z); duration = Y_1 / Y_0, convexity = Y_2 / Y_0 with Y_m = sum amount tau^m exp(-y tau).

FRNs.  rate_i = the first fixing where cpn_fix != 0, else (D_idx(ts_i) / D_idx(te_i) - 1) / ialpha_i, plus the margin, min with the
cap, max with the floor; A_i = rate_i alpha_i face D(T_i) / D(T_s); A_M = face D(T_M) / D(T_s) when T_M is not NaN.  PV(x) = sum
A_i exp(-x tau_i) + A_M exp(-x tau_M); dirty = 100 PV / face, clean = dirty - acc100, mod_duration = -(dirty(x + b) - dirty(x -
b)) / (2 b dirty(x)), dv01 = |PV(x + b) - PV(x)|.  Status 3 and NaN when a projected coupon's ts or te lies before the index
curve's first node.

Gross.  Every output has a ``gross``: the same sums on absolute values.  A bond flow counts (|cpn| + max(prin, 0)) D / D_s, a
projected coupon ((q + 1) / |ialpha| + |margin|) |alpha face| D / D_s with q = D_idx(ts) / D_idx(te) (a fixed one |ffr| +
|margin|), the way tests/_scenario_reference.py treats q - 1.  clean adds |acc100|; a difference of two prices has the sum of
their grosses; a quotient N / M has (gross_N + |N / M| gross_M) / |M|.  So dv01 and the FRN duration are bounded on the scale of
the gross price, not of themselves.

The bound |got - value| <= k 2^-53 gross, one k per output and instrument.  Each rounding is ONE unit 2^-53 of the absolute
sum it acts on, a library function documented at one ulp (exp, log) TWO units; every count ends with one more unit that pays
for all second-order terms (k 2^-53 < 1e-11 throughout).  As the code performs them (node_df.hpp, measures_common.hpp,
bond_measures.hip, frn_measures.hip):
  date      D = exp(E) or d exp(E).  An absolute error of E is a relative one of D, so the roundings of E count against
            cond = sum |weight L| (|weight G| under LINEAR_FWD), read off the inputs: beyond the last node the weights (b - t) /
            (b - a) and (t - a) / (b - a) have opposite signs and cond exceeds |E| many times (50Y flows on the 20Y table: 104
            under FLAT_FWD, 263 under LINEAR_ZERO)
              LINEAR_ZERO  log (2), / x (1), b - t (1), * (1), the sum (1), b - a (1), / (1), * t (1); exp (2)  ceil(9 cond) + 2
              FLAT_FWD     log (2), x_q - t (1), * (1), the sum (1), x_q - x_p (1), / (1); exp (2)              ceil(7 cond) + 2
              LINEAR_FWD   first segment: log (2), t * (1), x_1 + small (1), / (1) of cond = |E|; d_1 + small (1) is an
                           absolute error of the log, times |t| / (x_1 + small) <= 1; exp (2)
                                                                                  ceil(5 cond + |t| / (x_1 + small)) + 2
                           else: log (2), h_1 (1), / (1), x_i - t (1), * (1), the sum (1), h (1), / (1), t - x_{i-1} (1), * (1)
                           of cond; the divisions d_{i-1} / d_{i-2} and d_i / d_{i-1} (1 each) are absolute errors of G_1 and G_2
                           and count |w_1| + |w_2|; exp (2), d_{i-1} * (1)                ceil(11 cond + |w_1| + |w_2|) + 3
                           beyond the last node: log (2), h_1 (1), / (1), t - x_{n-1} (1), * (1)      ceil(6 cond + |w_1|) + 3
            The part of these that vanishes with cond = 0 is reported as "the share of k due to cond".
  amount    bond: cpn + prin (1), D(T) (e_D), D(T_s) (e_D), / (1), * (1)                        e_A = e_D(T) + e_D(T_s) + 3
            FRN: q = two index dates and / (2 e_D + 1); q - 1 (1), / ialpha (1), + margin (1), of the gross rate; min and
            max are exact and never widen an error; * alpha (1), * face (1), D(T) / D(T_s) (2 e_D + 1), * (1)
                                                               e_A = e_idx(ts) + e_idx(te) + e_D(T) + e_D(T_s) + 8
            (a fixed coupon: ffr + margin (1) instead, e_D(T) + e_D(T_s) + 5; the face A_M: e_D(T_M) + e_D(T_s) + 2).  The
            largest e_A over the instrument's flows is taken.
  term      A exp(-x tau): x * tau (1) of |x tau| <= zt, the largest over the flows; exp (2); * (1)            ceil(zt) + 3
            at x +- b: x +- b (1) and * tau (1), both of |(x +- b) tau| <= zt_b                             ceil(2 zt_b) + 3
  pass      a lane adds its ceil(n / 16) flows in order (the first to 0.0, exact), four butterfly levels follow: every flow
            passes through at most ceil(n / 16) + 4 adds and a level's partial sums never exceed the gross, and n flows take
            at most n adds that round; the face added after the pass (bond yield passes, FRN) one more
                                                                          s = min(n, ceil(n / 16) + 4) [+ 1]
  k_P = e_A + ceil(zt) + 3 + s + 1 is the count of P(x), PV(x); the bond's Y_0 has no e_A (its amounts are inputs).
  outputs   dirty k_P + 2 (/ face, * 100);  clean k_P + 3 on gross + |acc100|;  pv k_P;  bond dv01 k_P(x +- b) + 1 (the
            difference; / 2 is exact);  FRN dv01 k_P(x + b) + 1;  FRN mod_duration k_P(x +- b) + 4: numerator dirty + 2 each and
            the difference (1), denominator 2 b exact, * dirty (1), then / (1);  duration k_Y + 2 (e * tau, /), convexity
            k_Y + 3 (tau * tau, e * that, /).  A given z or DM is returned as it stands: k = 0, the bits of the quote.

Solved outputs (z from a clean price, the yield, the DM) are checked backwards at the root x the code returned: R = F(x) -
target, both exact, F = P, Y_0 or PV, against
  |R| <= (k_F gross_F(x) + k_T gross_T) 2^-53 + c 1e-15 max(1, |x|) |F'(x)|.
target = ((quote + acc100) / 100) face has k_T = 3 on gross_T = (|quote| + |acc100|) |face| / 100.  The yield's target is the
exact P(z) at the returned z; the code forms it as ((clean + acc100) / 100) face from its own clean: k_T = k_P + 6 (dirty 2,
clean 1, + acc100, / 100, * face) on gross_T = gross_P + |acc100 face| / 100.  Prices, dv01 and the FRN duration are held at
the returned z or DM, duration and convexity at the returned yield.

c = 1, from `solve`'s loop.  A turn evaluates f~ = F~(x) - target at the previous iterate x, steps to x' and stops when |x' -
x| <= 1e-15 max(1, |x'|); x' is returned and its residual never evaluated.
  - x' a Newton point, fl(x - fl(f~ / F~'(x))).  With R(x) = f~ + eps, |eps| the first term of the bound, Taylor gives
    R(x') = eps + f~ (1 - F'(x) / F~'(x) (1 + delta)) + F'' (x' - x)^2 / 2 + F'(x') O(2^-53 |x'|):  the middle terms are |F'| |x' -
    x| times a relative error of the derivative (k 2^-53 gross_F' / |F'|) or times tau_max |x' - x| / 2 (below 1e-13), the
    last the rounding of x' itself, 2^-53 / 1e-15 = 0.12 of the stop term.
  - x' the midpoint of the sign-change bracket [a, b] (the Newton point left it).  x is the end just moved, so b - a = 2 |x' - x|.
    The computed f~(a), f~(b) differ in sign; either R does too and has a root in [a, b], or the computed sign is wrong at an
    end, where then |R| <= eps.  So some x* in [a, b] has |R(x*)| <= eps and |R(x')| <= eps + |F'| (b - a) / 2: c = 1.
  The unbracketed loop takes Newton points only.  A crude reading (x within one step of the root, x' within another) gives 2;
  the loop gives 1.  For a bond the stop term is most of the allowance: up to 126 units of gross for z and 122 for the yield
  on the edge books (412 for the 600-flow bond at the bracket ends), against residuals of a few units - except where the
  midpoint case is taken.  That happens at the very end: a Newton step of a little over 1e-15 lands within an ulp of the root
  on its far side, the next Newton step is below half an ulp, so x' = x is not strictly inside [a, b] and the midpoint of a
  bracket 1.15e-15 wide is returned, 0.58e-15 from a root already found (residual 252 units on the host, 276 on the device).
  It is within the stop rule and within c = 1.  For an FRN a coupon's gross is (q + 1) / ialpha, some hundreds of times its
  rate, so the stop term is 0.35 .. 0.58 units of gross and the rounding terms are most of the allowance
  (tests/test_measures_reference_host.py prints residuals and stop terms).

Status.  0 when the exact F - target changes sign over the bracket ([-0.1, 0.5] for z, [-0.5, 0.5] for the yield, [-0.10, 0.20] for
the DM); 1 when it does not and a root exists; 2 when none does; 3 as above.  A root's existence is decided for flows of one
sign only - amounts >= 0 and tau > 0, where F falls from +inf to 0 and a root exists iff target > 0 - and the reference refuses
an unbracketed case of mixed signs.  It also refuses a case on the fence: the exact |F(lo) - target| and |F(hi) - target| must
exceed 1000 units 2^-53 of their gross.  The bond's status is the larger of z's and the yield's; with 2 from z, or 3, every
output is NaN; with 2 from the yield, ytm, duration and convexity are.

Nothing in k is fitted to what the kernels return.
"""
import math

import numpy as np
from mpmath import mp, mpf

FLAT_FWD, LINEAR_FWD, LINEAR_ZERO = 1, 2, 4
DPS = 60
U = mpf(2) ** -53
BUMP = mpf(0.0001)          # the double nearest 1e-4
SMALL = mpf(1e-10)          # node_df.hpp's regulariser, the double
STOP = mpf(1e-15)           # `solve`'s stop rule, the double
C_STOP = 1                  # c of the module docstring
FENCE = 1000                # units a bracket end must keep from the target

BOND_OUTPUTS = ("z", "dirty", "clean", "ytm", "duration", "convexity", "dv01")
FRN_OUTPUTS = ("dm", "dirty", "clean", "pv", "mod_duration", "dv01")
_CPN = ("cpn_T", "cpn_ts", "cpn_te", "cpn_ialpha", "cpn_alpha", "cpn_tau", "cpn_fix")


def _mp(x):
    return mpf(float(x))


def _ceil(x):
    return int(math.ceil(float(x)))


# ------------------------------------------------------------------------------------------------------------ D(t)
class Table:
    """D(t) on one node table under one scheme: ``date(t) -> (D, e_D, cond part of e_D)``, cached per t."""

    def __init__(self, method, x, d):
        self.method = int(method)
        assert self.method in (FLAT_FWD, LINEAR_FWD, LINEAR_ZERO)
        self.x = np.array(x, dtype=np.float64)
        self.d = np.array(d, dtype=np.float64)
        self.n = self.x.size
        assert self.n >= 2 and self.d.size == self.n and np.all(np.diff(self.x) > 0)
        self._L, self._date = {}, {}

    def L(self, k):
        if k not in self._L:
            self._L[k] = mp.log(_mp(self.d[k]))
        return self._L[k]

    def date(self, t):
        t = float(t)
        if t not in self._date:
            self._date[t] = self._eval(t)
        return self._date[t]

    def _eval(self, t):
        x, n = self.x, self.n
        if not t >= x[0]:
            return mpf("nan"), 0, 0
        if t == x[0]:
            return _mp(self.d[0]), 0, 0
        i = int(np.searchsorted(x, t, side="left"))          # the first node with x_i >= t; n beyond the last
        X, T = (lambda k: _mp(x[k])), _mp(t)
        if self.method == LINEAR_ZERO:
            if i == 1:
                p, q, a, b = 1, 1, X(0), X(1)
            elif i < n:
                p, q, a, b = i - 1, i, X(i - 1), X(i)
            else:
                p, q, a, b = n - 1, n - 1, X(n - 2), X(n - 1)
            assert x[p] != 0.0 and x[q] != 0.0
            parts = [T * (b - T) / (b - a) / X(p) * self.L(p), T * (T - a) / (b - a) / X(q) * self.L(q)]
            per, rest, flat, scale = 9, mpf(0), 2, mpf(1)
        elif self.method == FLAT_FWD:
            p, q = (i - 1, i) if i < n else (n - 2, n - 1)
            parts = [(X(q) - T) / (X(q) - X(p)) * self.L(p), (T - X(p)) / (X(q) - X(p)) * self.L(q)]
            per, rest, flat, scale = 7, mpf(0), 2, mpf(1)
        elif i == 1:
            parts = [T * mp.log(_mp(self.d[1]) + SMALL) / (X(1) + SMALL)]
            per, rest, flat, scale = 5, abs(T) / (X(1) + SMALL), 2, mpf(1)
        else:
            h1, G1 = X(i - 1) - X(i - 2), self.L(i - 1) - self.L(i - 2)
            if i < n:
                h, G2 = X(i) - X(i - 1), self.L(i) - self.L(i - 1)
                w1, w2 = (X(i) - T) * (T - X(i - 1)) / (h * h1), (T - X(i - 1)) ** 2 / (h * h)
                parts, per, rest = [w1 * G1, w2 * G2], 11, abs(w1) + abs(w2)
            else:
                w1 = (T - X(n - 1)) / h1
                parts, per, rest = [w1 * G1], 6, abs(w1)
            flat, scale = 3, _mp(self.d[i - 1])
        cond = sum((abs(v) for v in parts), mpf(0))
        units = _ceil(per * cond + rest)
        return scale * mp.exp(sum(parts, mpf(0))), units + flat, units


_TABLES = {}


def table(method, x, d):
    x, d = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(d, dtype=np.float64)
    key = (int(method), x.tobytes(), d.tobytes())
    if key not in _TABLES:
        _TABLES[key] = Table(method, x, d)
    return _TABLES[key]


# ------------------------------------------------------------------------------------------------------------ sums
def pass_adds(n):
    """s of the module docstring."""
    return min(n, -(-n // 16) + 4)


class Flows:
    """F(x) = sum A_i exp(-x tau_i) of one instrument: ``A`` the amounts, ``G`` their grosses, ``e_A`` the units of an amount
    (``e_cond`` of them due to cond), ``adds`` the roundings of the pass."""

    def __init__(self, A, G, tau, e_A, e_cond, adds):
        self.A, self.G, self.tau = list(A), list(G), [_mp(t) for t in tau]
        self.e_A, self.e_cond, self.adds = int(e_A), int(e_cond), int(adds)
        self.tmax = max((abs(t) for t in self.tau), default=mpf(0))
        self.one_sign = all(a >= 0 for a in self.A) and any(a > 0 for a in self.A) and all(t > 0 for t in self.tau)
        self._E, self._bump = {}, None

    def _exps(self, x):
        x = float(x)
        if x not in self._E:
            X = _mp(x)
            self._E[x] = [mp.exp(-X * t) for t in self.tau]
        return self._E[x]

    def _sums(self, E, power=0):
        if power == 0:
            return sum((a * e for a, e in zip(self.A, E)), mpf(0)), sum((a * e for a, e in zip(self.G, E)), mpf(0))
        v = sum((a * t ** power * e for a, t, e in zip(self.A, self.tau, E)), mpf(0))
        g = sum((a * abs(t) ** power * e for a, t, e in zip(self.G, self.tau, E)), mpf(0))
        return v, g

    def at(self, x, power=0):
        """``(sum A tau^power exp(-x tau), its gross)``."""
        return self._sums(self._exps(x), power)

    def slope(self, x):
        """F'(x)."""
        return -self.at(x, 1)[0]

    def bumped(self, x, sign):
        """``(F, gross)`` at x + sign b, b exact: exp(-(x + sign b) tau) = exp(-x tau) exp(-sign b tau)."""
        if self._bump is None:
            self._bump = [mp.exp(BUMP * t) for t in self.tau]
        E = [e / f if sign > 0 else e * f for e, f in zip(self._exps(x), self._bump)]
        return self._sums(E)

    def k(self, x):
        """k_P at x."""
        return self.e_A + _ceil(abs(_mp(x)) * self.tmax) + 3 + self.adds + 1

    def k_bumped(self, x):
        """k_P at x +- b."""
        return self.e_A + _ceil(2 * (abs(_mp(x)) + BUMP) * self.tmax) + 3 + self.adds + 1

    def status(self, target, g_T, lo, hi):
        """0, 1 or 2 of the module docstring for F = target on [lo, hi]."""
        sides = []
        for x in (lo, hi):
            v, g = self.at(x)
            assert abs(v - target) > FENCE * U * (g + g_T), f"a case on the fence: F({x}) - target = {float(v - target)!r}"
            sides.append(v - target)
        if sides[0] * sides[1] < 0:
            return 0
        if not self.one_sign:
            raise ValueError("no bracket and flows of mixed signs: the reference does not decide whether a root exists")
        return 1 if target > 0 else 2


class Report:
    """What a check found: the worst ratio |error| / allowance per output, the range of k, the stop rule's term in units of
    the gross, the shares of k due to cond, and the rows whose status is not the reference's."""

    def __init__(self, outputs):
        self.ratio = {o: 0.0 for o in outputs}
        self.k = {o: [None, None] for o in outputs}
        self.stop_units = {}
        self.residual_units = {}
        self.cond_share = [1.0, 0.0]
        self.status_want = []
        self.status_bad = []

    def _k(self, name, k):
        lo, hi = self.k[name]
        self.k[name] = [k if lo is None else min(lo, k), k if hi is None else max(hi, k)]

    def value(self, name, got, want, k, gross):
        got = float(got)
        self._k(name, k)
        r = math.inf if not math.isfinite(got) else float(abs(_mp(got) - want) / (k * U * gross))
        self.ratio[name] = max(self.ratio[name], r)

    def exact(self, name, got, want):
        """k = 0: the bits of ``want`` (NaN for NaN)."""
        got, want = float(got), float(want)
        same = (got != got and want != want) or (got == want and math.copysign(1, got) == math.copysign(1, want))
        self.ratio[name] = max(self.ratio[name], 0.0 if same else math.inf)

    def root(self, name, x, F, target, k_F, g_F, k_T, g_T, slope):
        self._k(name, k_F)
        if not math.isfinite(float(x)):
            self.ratio[name] = math.inf
            return
        stop = C_STOP * STOP * max(mpf(1), abs(_mp(x))) * abs(slope)
        allow = (k_F * g_F + k_T * g_T) * U + stop
        self.ratio[name] = max(self.ratio[name], float(abs(F - target) / allow))
        self.stop_units[name] = max(self.stop_units.get(name, 0.0), float(stop / (U * g_F)))
        self.residual_units[name] = max(self.residual_units.get(name, 0.0), float(abs(F - target) / (U * g_F)))

    def share(self, flows, k):
        s = flows.e_cond / k
        self.cond_share = [min(self.cond_share[0], s), max(self.cond_share[1], s)]

    def status(self, row, got, want):
        self.status_want.append(int(want))
        if int(got) != int(want):
            self.status_bad.append((row, int(got), int(want)))

    def worst(self):
        return max(self.ratio.values())

    def line(self, what):
        parts = [f"{o} {self.ratio[o]:.3g} (k {self.k[o][0]}..{self.k[o][1]})" if self.k[o][0] is not None
                 else f"{o} {self.ratio[o]:.3g}" for o in self.ratio]
        extra = "".join(f"; {o}: residual {self.residual_units[o]:.3g}, stop term {self.stop_units[o]:.3g} units of gross"
                        for o in self.stop_units)
        return (f"{what}: worst ratios " + ", ".join(parts) + extra +
                f"; cond's share of k_P {self.cond_share[0]:.2f}..{self.cond_share[1]:.2f}")

    def merge(self, other):
        for o, r in other.ratio.items():
            self.ratio[o] = max(self.ratio[o], r)
            for k in other.k[o]:
                if k is not None:
                    self._k(o, k)
        for mine, theirs in ((self.stop_units, other.stop_units), (self.residual_units, other.residual_units)):
            for o, v in theirs.items():
                mine[o] = max(mine.get(o, 0.0), v)
        self.cond_share = [min(self.cond_share[0], other.cond_share[0]), max(self.cond_share[1], other.cond_share[1])]
        self.status_want += other.status_want
        self.status_bad += other.status_bad
        return self


def _target(quote, acc, face):
    """``(target, k_T, gross_T)`` of a clean-price quote."""
    return (quote + acc) / 100 * face, 3, (abs(quote) + abs(acc)) / 100 * abs(face)


# ------------------------------------------------------------------------------------------------------------ bonds
class BondRef:
    """One bond: P on the curve, Y on its coupons and face."""

    def __init__(self, tab, book, b):
        lo, hi = int(book["flow_off"][b]), int(book["flow_off"][b + 1])
        Ds, e_s, c_s = tab.date(book["bond_Ts"][b])
        A, G, e_A, e_cond = [], [], 0, 0
        for i in range(lo, hi):
            D, e, c = tab.date(book["flow_T"][i])
            cpn, prin = _mp(book["flow_cpn"][i]), max(_mp(book["flow_prin"][i]), mpf(0))
            A.append((cpn + prin) * D / Ds)
            G.append((abs(cpn) + prin) * D / Ds)
            if e + e_s + 3 > e_A:
                e_A, e_cond = e + e_s + 3, c + c_s
        tau = [float(book["flow_tau"][i]) for i in range(lo, hi)]
        n = hi - lo
        self.P = Flows(A, G, tau, e_A, e_cond, pass_adds(n))
        self.face, self.acc = _mp(book["bond_face"][b]), _mp(book["bond_acc100"][b])
        cpn = [_mp(book["flow_cpn"][i]) for i in range(lo, hi)]
        tauM = float(book["bond_tauM"][b])
        paid = tauM > 0.0
        self.Y = Flows(cpn + [self.face] * paid, [abs(c) for c in cpn] + [abs(self.face)] * paid, tau + [tauM] * paid, 0, 0,
                       pass_adds(n) + paid)

    def check(self, rep, row, quote, quote_is_z, got, status):
        """Holds ``got`` (output -> float) and ``status`` of this bond to the reference, into ``rep``."""
        P, Y, face, acc = self.P, self.Y, self.face, self.acc
        nan = math.nan
        if quote_is_z:
            sz, z = 0, float(quote)
            rep.exact("z", got["z"], z)
        else:
            T, k_T, g_T = _target(_mp(quote), acc, face)
            sz = P.status(T, g_T, -0.1, 0.5)
            if sz == 2:
                rep.status(row, status, 2)
                for o in BOND_OUTPUTS:
                    rep.exact(o, got[o], nan)
                return
            z = float(got["z"])
            if not math.isfinite(z):
                rep.ratio["z"] = math.inf
                rep.status(row, status, sz)
                return
            v, g = P.at(z)
            rep.root("z", z, v, T, P.k(z), g, k_T, g_T, P.slope(z))
        k, kb = P.k(z), P.k_bumped(z)
        rep.share(P, k)
        (v, g), (vm, gm), (vp, gp) = P.at(z), P.bumped(z, -1), P.bumped(z, +1)
        dirty, gd = v / face * 100, g / abs(face) * 100
        rep.value("dirty", got["dirty"], dirty, k + 2, gd)
        rep.value("clean", got["clean"], dirty - acc, k + 3, gd + abs(acc))
        rep.value("dv01", got["dv01"], (vm - vp) / 2, kb + 1, (gm + gp) / 2)
        k_T, g_T = k + 6, g + abs(acc * face) / 100
        sy = Y.status(v, g_T, -0.5, 0.5)
        rep.status(row, status, max(sz, sy))
        if sy == 2:
            for o in ("ytm", "duration", "convexity"):
                rep.exact(o, got[o], nan)
            return
        y = float(got["ytm"])
        if not math.isfinite(y):
            rep.ratio["ytm"] = math.inf
            return
        (y0, g0), (y1, g1), (y2, g2) = Y.at(y), Y.at(y, 1), Y.at(y, 2)
        ky = Y.k(y)
        rep.root("ytm", y, y0, v, ky, g0, k_T, g_T, -y1)
        rep.value("duration", got["duration"], y1 / y0, ky + 2, (g1 + abs(y1 / y0) * g0) / abs(y0))
        rep.value("convexity", got["convexity"], y2 / y0, ky + 3, (g2 + abs(y2 / y0) * g0) / abs(y0))


_BONDS = {}


def _key(book, fields):
    return tuple(np.ascontiguousarray(book[f]).tobytes() for f in fields)


def bond_refs(method, node_t, node_df, book):
    """The `BondRef` of every bond of ``book`` (the quotes are not part of it); built once per process for the same inputs."""
    mp.dps = DPS
    tab = table(method, node_t, node_df)
    key = (id(tab),) + _key(book, ("flow_off", "flow_T", "flow_tau", "flow_cpn", "flow_prin", "bond_Ts", "bond_tauM",
                                   "bond_face", "bond_acc100"))
    if key not in _BONDS:
        _BONDS[key] = [BondRef(tab, book, b) for b in range(len(book["flow_off"]) - 1)]
    return _BONDS[key]


def check_bonds(method, node_t, node_df, book, quote_is_z, got):
    """The `Report` of ``got`` (adr_bond_measures' result: output -> array, and ``status``)."""
    mp.dps = DPS
    rep = Report(BOND_OUTPUTS)
    for b, ref in enumerate(bond_refs(method, node_t, node_df, book)):
        ref.check(rep, b, book["bond_quote"][b], quote_is_z, {o: float(got[o][b]) for o in BOND_OUTPUTS}, got["status"][b])
    return rep


# ------------------------------------------------------------------------------------------------------------ FRNs
class FrnRef:
    """One FRN: its coupons projected once, PV on the discount curve; ``bad`` when a forward needs the index curve before its
    first node."""

    def __init__(self, disc, index, book, b):
        lo, hi = int(book["cpn_off"][b]), int(book["cpn_off"][b + 1])
        f = lambda k: book[k][b]
        self.face, self.acc = _mp(f("frn_face")), _mp(f("frn_acc100"))
        margin, ffr = _mp(f("frn_margin")), _mp(f("frn_ffr"))
        cap, floor = float(f("frn_cap")), float(f("frn_floor"))
        Ds, e_s, c_s = disc.date(f("frn_Ts"))
        A, G, tau, e_A, e_cond = [], [], [], 0, 0
        self.bad = False
        for i in range(lo, hi):
            T, ts, te, ialpha, alpha, tau_i, fix = (float(book[k][i]) for k in _CPN)
            if fix != 0.0:
                rate, g_rate, e, c = ffr + margin, abs(ffr) + abs(margin), 1, 0
            else:
                if not (ts >= index.x[0] and te >= index.x[0]):
                    self.bad = True
                    break
                (D1, e1, c1), (D2, e2, c2) = index.date(ts), index.date(te)
                q = D1 / D2
                rate, g_rate = (q - 1) / _mp(ialpha) + margin, (q + 1) / abs(_mp(ialpha)) + abs(margin)
                e, c = e1 + e2 + 4, c1 + c2
            if math.isfinite(cap):
                rate = min(rate, _mp(cap))
            elif cap < 0:
                rate = mpf("-inf")
            if math.isfinite(floor):
                rate = max(rate, _mp(floor))
            elif floor > 0:
                rate = mpf("inf")
            g_rate = max(g_rate, abs(rate))
            D, e_p, c_p = disc.date(T)
            scale = _mp(alpha) * self.face * D / Ds
            A.append(rate * scale)
            G.append(g_rate * abs(scale))
            tau.append(tau_i)
            if e + e_p + e_s + 4 > e_A:
                e_A, e_cond = e + e_p + e_s + 4, c + c_p + c_s
        if self.bad:
            return
        TM = float(f("frn_TM"))
        paid = TM == TM
        if paid:
            D, e_p, c_p = disc.date(TM)
            A.append(self.face * D / Ds)
            G.append(abs(self.face) * D / Ds)
            tau.append(float(f("frn_tauM")))
            if e_p + e_s + 2 > e_A:
                e_A, e_cond = e_p + e_s + 2, c_p + c_s
        self.PV = Flows(A, G, tau, e_A, e_cond, pass_adds(hi - lo) + paid)

    def check(self, rep, row, quote, quote_is_dm, got, status):
        nan = math.nan
        if self.bad:
            rep.status(row, status, 3)
            for o in FRN_OUTPUTS:
                rep.exact(o, got[o], nan)
            return
        PV, face, acc = self.PV, self.face, self.acc
        if quote_is_dm:
            s, x = 0, float(quote)
            rep.exact("dm", got["dm"], x)
        else:
            T, k_T, g_T = _target(_mp(quote), acc, face)
            s = PV.status(T, g_T, -0.10, 0.20)
            rep.status(row, status, s)
            if s == 2:
                for o in FRN_OUTPUTS:
                    rep.exact(o, got[o], nan)
                return
            x = float(got["dm"])
            if not math.isfinite(x):
                rep.ratio["dm"] = math.inf
                return
            v, g = PV.at(x)
            rep.root("dm", x, v, T, PV.k(x), g, k_T, g_T, PV.slope(x))
        if quote_is_dm:
            rep.status(row, status, 0)
        k, kb = PV.k(x), PV.k_bumped(x)
        rep.share(PV, k)
        (v, g), (vm, gm), (vp, gp) = PV.at(x), PV.bumped(x, -1), PV.bumped(x, +1)
        pct = 100 / abs(face)
        dirty, gd = 100 * v / face, g * pct
        rep.value("dirty", got["dirty"], dirty, k + 2, gd)
        rep.value("clean", got["clean"], dirty - acc, k + 3, gd + abs(acc))
        rep.value("pv", got["pv"], v, k, g)
        rep.value("dv01", got["dv01"], abs(vp - v), kb + 1, gp + g)
        den = 2 * BUMP * dirty
        dur = -(100 * vp / face - 100 * vm / face) / den
        rep.value("mod_duration", got["mod_duration"], dur, kb + 4, (gp + gm) * pct / abs(den) + abs(dur) * gd / abs(dirty))


_FRNS = {}


def frn_refs(disc, index, book):
    """The `FrnRef` of every FRN of ``book``; ``disc`` and ``index`` are ``(method, node times, node dfs)``."""
    mp.dps = DPS
    d, i = table(*disc), table(*index)
    key = (id(d), id(i)) + _key(book, ("cpn_off",) + _CPN + ("frn_Ts", "frn_TM", "frn_tauM", "frn_face", "frn_margin", "frn_cap",
                                                              "frn_floor", "frn_ffr", "frn_acc100"))
    if key not in _FRNS:
        _FRNS[key] = [FrnRef(d, i, book, b) for b in range(len(book["cpn_off"]) - 1)]
    return _FRNS[key]


def check_frns(disc, index, book, quote_is_dm, got):
    """The `Report` of ``got`` (adr_frn_measures' result)."""
    mp.dps = DPS
    rep = Report(FRN_OUTPUTS)
    for b, ref in enumerate(frn_refs(disc, index, book)):
        ref.check(rep, b, book["frn_quote"][b], quote_is_dm, {o: float(got[o][b]) for o in FRN_OUTPUTS}, got["status"][b])
    return rep
