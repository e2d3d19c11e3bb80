"""The reference and the judge of the curve builders: `bootstrap_kernel` (csrc/curve_build.hip), `build_engine_curve`
(market/curves/curve_tables.py) and the values-only scans `curve_dfs_kernel` / `adr_curve_dfs_shocked_host`
(csrc/curve_dfs.hip) - tests/test_curve_reference_host.py (CPU) and tests/test_gpu_curve_reference.py (GPU).

Value.  d_i, its gradient and its Hessian in the par rates come from second-order Taylor (jet) arithmetic at 60 digits on the
VALUE recurrence alone,
    d = (1 - r Pp) / (1 + r a)   [1 / (1 + r a) where prev_idx < 0],   PV01 = Pp + a d,   Pp = PV01[prev_idx] if 0 <= prev_idx < i else 0
with generic jet + - x / (`Jet`): no derivative formula of the builders stands in this module's value path.  Jets are sparse
(a knot carries only the pillars its predecessor chain moves) and symmetric (the upper triangle is stored).  Jets have no
step: central differences at 60 digits with step 1e-20 leave 1e-60 / 1e-40 = 1e-20 of absolute noise on a second derivative,
more than the bound of a Hessian entry of size 1e-8; `difference_check` is the only place differences
are used, as a cross-check of the jet arithmetic itself, and asserts that its noise stays 2^-20 below the smallest bound.

Bound.  A running error analysis of the program under test, no fitted constant: `Bound` carries the float64 number the
builders' operation sequence produces (the header comments of curve_build.hip and curve_dfs.hip; contraction is off in both)
and a bound e on its distance from the same expression in exact arithmetic, by the rules (u = 2^-53, z^ the operation's
float64 result)
    x +- y   e_x + e_y + u |z^|
    x y      |x^| e_y + |y^| e_x + e_x e_y + u |z^|
    x / y    (e_x + |z^| e_y) / (|y^| - e_y) + u |z^|
evaluated in mpmath (libmp at 64 bits, every operation rounded away from the safe side: up, the denominator down).  An operation
with an exact zero for an operand (x^ = 0 and e_x = 0) is exact: x + 0 = x, x 0 = 0.  The bound follows the algorithm, the
value does not: were the builders' derivative recurrences wrong, the jets would say so by far more than the bound.
An entry whose bound is 0 is a structural zero: it must be 0.0, of either sign (the recurrences multiply zeros by -r / v).

Judge.  `Reference.share(dfs, jac, hess)`: |got - value| <= e at EVERY entry, the worst share per array.  The value is kept
as an unevaluated sum hi + lo of two float64 (what it leaves out, at most 2^-104 |hi|, is taken off the bound); an entry whose
share in float64 arithmetic is 0.99 or more is decided in exact rational arithmetic.
"""
import fractions
import functools

import mpmath
import numpy as np
from mpmath import libmp, mpf

DPS = 60
PREC = 64                       # of the bound's own arithmetic
UP, DOWN = "c", "f"
FZERO = libmp.fzero
ZERO = (0.0, FZERO)             # an exact zero
ONE = (1.0, FZERO)
BP = (1e-4, None)               # the scans' constant; its error is filled in below
ARRAYS = ("dfs", "jac", "hess")


# ------------------------------------------------------------------------------------------------------------------ value
class Jet:
    """A truncated second-order Taylor series in the par rates: ``v``, ``g {p: dv/dr_p}``, ``h {(p, q), p <= q: d2v/dr_p dr_q}``."""
    __slots__ = ("v", "g", "h")

    def __init__(self, v, g=None, h=None):
        self.v, self.g, self.h = v, g or {}, h or {}

    @staticmethod
    def lift(x):
        return x if isinstance(x, Jet) else Jet(mpf(x))

    def scaled(self, c):
        return Jet(c * self.v, {p: c * x for p, x in self.g.items()}, {k: c * x for k, x in self.h.items()})

    def __neg__(self):
        return self.scaled(mpf(-1))

    def __add__(self, o):
        o = Jet.lift(o)
        g, h = dict(self.g), dict(self.h)
        for p, x in o.g.items():
            g[p] = g[p] + x if p in g else x
        for k, x in o.h.items():
            h[k] = h[k] + x if k in h else x
        return Jet(self.v + o.v, g, h)

    __radd__ = __add__

    def __sub__(self, o):
        return self + (-Jet.lift(o))

    def __rsub__(self, o):
        return Jet.lift(o) + (-self)

    def __mul__(self, o):
        o = Jet.lift(o)
        if not o.g:
            return self.scaled(o.v)
        if not self.g:
            return o.scaled(self.v)
        out = self.scaled(o.v) + Jet(mpf(0), {p: self.v * x for p, x in o.g.items()}, {k: self.v * x for k, x in o.h.items()})
        out.v = self.v * o.v
        h = out.h
        for p, x in self.g.items():
            for q, y in o.g.items():
                k, t = ((p, q) if p <= q else (q, p)), x * y
                if p == q:
                    t = 2 * t
                h[k] = h[k] + t if k in h else t
        return out

    __rmul__ = __mul__

    def reciprocal(self):
        w = 1 / self.v
        w2 = -w * w
        out = Jet(w, {p: w2 * x for p, x in self.g.items()}, {k: w2 * x for k, x in self.h.items()})
        w3 = 2 * w * w * w
        items = sorted(self.g.items())
        for i, (p, x) in enumerate(items):
            for q, y in items[i:]:
                t = w3 * x * y
                out.h[(p, q)] = out.h[(p, q)] + t if (p, q) in out.h else t
        return out

    def __truediv__(self, o):
        return self * Jet.lift(o).reciprocal()

    def __rtruediv__(self, o):
        return Jet.lift(o) * self.reciprocal()


def scan_value(acc, pillar, prev_idx, rates, order):
    """The value recurrence on ``rates`` (mpf, exact): per knot the `Jet` of d_i - with pillar p as variable p for
    ``order`` >= 1 - in generic jet arithmetic."""
    r_jets = [Jet(r, {p: mpf(1)} if order else None) for p, r in enumerate(rates)]
    pv01, out = [], []
    for i in range(len(acc)):
        r, a, pi = r_jets[int(pillar[i])], mpf(float(acc[i])), int(prev_idx[i])
        Pp = pv01[pi] if 0 <= pi < i else Jet(mpf(0))
        d = (1 - r * Pp) / (1 + r * a) if pi >= 0 else 1 / (1 + r * a)
        if order < 2:
            d.h = {}
        pv01.append(Pp + a * d)
        out.append(d)
    return out


# ------------------------------------------------------------------------------------------------------------------ bound
def _mag(x):
    return libmp.from_float(abs(x))


def _unit(z):
    return libmp.mpf_shift(_mag(z), -53)


def _sum(*terms):
    out = terms[0]
    for t in terms[1:]:
        out = libmp.mpf_add(out, t, PREC, UP)
    return out


def _prod(a, b):
    return libmp.mpf_mul(a, b, PREC, UP)


def b_add(x, y, sign=1.0):
    """x + sign y."""
    (xh, ex), (yh, ey) = x, y
    if yh == 0.0 and ey == FZERO:
        return x
    if xh == 0.0 and ex == FZERO:
        return (sign * yh, ey)
    z = xh + sign * yh
    return (z, _sum(ex, ey, _unit(z)))


def b_sub(x, y):
    return b_add(x, y, -1.0)


def b_mul(x, y):
    (xh, ex), (yh, ey) = x, y
    z = xh * yh
    if (xh == 0.0 and ex == FZERO) or (yh == 0.0 and ey == FZERO):
        return (z, FZERO)
    terms = [_unit(z)]
    if ey != FZERO:
        terms.append(_prod(_mag(xh), ey))
    if ex != FZERO:
        terms.append(_prod(_mag(yh), ex))
        if ey != FZERO:
            terms.append(_prod(ex, ey))
    return (z, _sum(*terms))


def b_div(x, y):
    (xh, ex), (yh, ey) = x, y
    z = xh / yh
    if xh == 0.0 and ex == FZERO:
        return (z, FZERO)
    den = libmp.mpf_sub(_mag(yh), ey, PREC, DOWN)
    assert libmp.mpf_gt(den, FZERO), "the divisor's bound reaches 0: no finite bound"
    num = _sum(ex, _prod(_mag(z), ey)) if ey != FZERO else ex
    return (z, _sum(libmp.mpf_div(num, den, PREC, UP), _unit(z)) if num != FZERO else _unit(z))


def b_neg(x):
    return (-x[0], x[1])


_bp_exact = None


def shocked_rate_bound(base, x):
    """``base + x 1e-4`` as the scans form it (curve_dfs.hip, `shocked_rate`) against the exact base + x / 10^4: the
    constant's own error, the product and the sum."""
    global _bp_exact
    if _bp_exact is None:
        with mpmath.workdps(DPS):
            _bp_exact = libmp.mpf_abs((mpf(1e-4) - mpf(1) / 10 ** 4)._mpf_, PREC, UP)
    return b_add((float(base), FZERO), b_mul((float(x), FZERO), (1e-4, _bp_exact)))


def scan_bound(acc, pillar, prev_idx, rates, order):
    """The builders' operation sequence on ``rates`` - pairs (float64, bound) - in float64, with the running bound of every
    number: ``dfs [K]``, ``jac [K] of {p: pair}``, ``hess [K] of {(p, q), p <= q: pair}`` (both mirrors of a Hessian entry
    are formed by the same operations on the same numbers; entries not held are exact zeros)."""
    K = len(acc)
    pv, dpv, d2pv = [None] * K, [None] * K, [None] * K
    dfs, jac, hess = [], [], []
    for i in range(K):
        s, pi = int(pillar[i]), int(prev_idx[i])
        r, a = rates[s], (float(acc[i]), FZERO)
        has_prev = 0 <= pi < i
        Pp = pv[pi] if has_prev else ZERO
        v = b_add(ONE, b_mul(r, a))
        d = b_div(b_sub(ONE, b_mul(r, Pp)), v) if pi >= 0 else b_div(ONE, v)
        dfs.append(d)
        pv[i] = b_add(Pp, b_mul(a, d))
        if not order:
            continue
        f = b_div(b_neg(r), v)
        dPp = dpv[pi] if has_prev else {}
        dd = {t: b_mul(f, x) for t, x in dPp.items()}
        dd[s] = b_sub(dd.get(s, ZERO), b_div(b_add(Pp, b_mul(d, a)), v))
        jac.append(dd)
        dpv[i] = {t: b_add(dPp.get(t, ZERO), b_mul(a, x)) for t, x in dd.items()}
        if order < 2:
            continue
        av = b_div(a, v)
        cross = {t: b_mul(x, av) for t, x in dd.items()}
        if has_prev:
            cross = {t: b_add(x, b_div(dPp[t], v)) if t in dPp else x for t, x in cross.items()}
        h_prev = d2pv[pi] if has_prev else {}
        sup = sorted(dd)
        h, h2 = {}, {}
        for n, p in enumerate(sup):
            for q in sup[n:]:
                hp = h_prev.get((p, q), ZERO)
                e = b_mul(f, hp)
                if p == s:
                    e = b_sub(e, cross[q])
                if q == s:
                    e = b_sub(e, cross[p])
                h[(p, q)] = e
                h2[(p, q)] = b_add(hp, b_mul(a, e))
        hess.append(h)
        d2pv[i] = h2
    return dfs, jac, hess


# ------------------------------------------------------------------------------------------------------------------ judge
def _two(x):
    hi = float(x)
    return hi, float(x - mpf(hi))


class Reference:
    """Value (hi + lo) and bound of every entry of ``dfs [K]``, ``jac [K, P]`` and ``hess [K, P, P]`` (``order`` 0: dfs
    alone, 1: no hess), and ``replica``: the float64 arrays this module's copy of the operation sequence gives."""

    def __init__(self, K, P, order):
        self.K, self.P, self.order = K, P, order
        shapes = {"dfs": (K,), "jac": (K, P), "hess": (K, P, P)}
        self.names = ARRAYS[:order + 1]
        self.hi = {n: np.zeros(shapes[n]) for n in self.names}
        self.lo = {n: np.zeros(shapes[n]) for n in self.names}
        self.e = {n: np.zeros(shapes[n]) for n in self.names}           # the bound, rounded down to float64
        self.replica = {n: np.zeros(shapes[n]) for n in self.names}

    def _set(self, name, idx, value, pair):
        zh, e = pair
        self.replica[name][idx] = zh
        if e == FZERO:
            assert value == 0 and zh == 0.0, (name, idx, "a bound of 0 on a non-zero entry")
            return
        hi, lo = _two(value)
        # what hi + lo leaves of the value is at most 2^-104 |hi|: off the bound
        e = libmp.mpf_sub(e, libmp.mpf_shift(_mag(hi), -104), PREC, DOWN)
        ef = libmp.to_float(e, rnd=DOWN)
        assert ef > 0.0, (name, idx)
        self.hi[name][idx], self.lo[name][idx], self.e[name][idx] = hi, lo, ef

    def min_bound(self):
        return min(float(np.min(self.e[n][self.e[n] > 0.0])) for n in self.names)

    def bound_in_units(self):
        """Per array: the worst bound over u |entry| (its conditioning)."""
        out = {}
        for n in self.names:
            live = (self.e[n] > 0.0) & (self.hi[n] != 0.0)
            out[n] = float(np.max(self.e[n][live] / (2.0 ** -53 * np.abs(self.hi[n][live])))) if np.any(live) else 0.0
        return out

    def share_of(self, name, got, what=""):
        """The worst |got - value| / e over ``got``; asserts a structural zero to be 0.0."""
        got = np.asarray(got, dtype=np.float64)
        hi, lo, e = self.hi[name], self.lo[name], self.e[name]
        assert got.shape == hi.shape, (what, name, got.shape, hi.shape)
        assert np.all(np.isfinite(got)), f"{what} {name}: not finite"
        zero = e == 0.0
        bad = np.nonzero(zero & (got != 0.0))
        assert bad[0].size == 0, f"{what} {name}{[int(b[0]) for b in bad]}: a structural zero holds {got[bad][0]!r}"
        live = ~zero
        if not np.any(live):
            return 0.0
        share = np.zeros(got.shape)
        share[live] = np.abs((got[live] - hi[live]) - lo[live]) / e[live]
        for idx in zip(*np.nonzero(share >= 0.99)):         # float64 arithmetic cannot be trusted to decide these
            F = fractions.Fraction
            share[idx] = float(abs(F(float(got[idx])) - F(float(hi[idx])) - F(float(lo[idx]))) / F(float(e[idx])))
        return float(np.max(share))

    def share(self, dfs, jac=None, hess=None, what=""):
        """``{"dfs": ..., "jac": ..., "hess": ...}``: the worst share of the bound per array given."""
        got = {"dfs": dfs, "jac": jac, "hess": hess}
        return {n: self.share_of(n, got[n], what) for n in self.names if got[n] is not None}


def _assemble(acc, pillar, prev_idx, exact_rates, bound_rates, P, order):
    K = len(acc)
    with mpmath.workdps(DPS):
        jets = scan_value(acc, pillar, prev_idx, exact_rates, order)
        dfs, jac, hess = scan_bound(acc, pillar, prev_idx, bound_rates, order)
        ref = Reference(K, P, order)
        for i in range(K):
            ref._set("dfs", i, jets[i].v, dfs[i])
            if order:
                assert set(jets[i].g) <= set(jac[i]), (i, "a pillar the bound does not know")
                for p, pair in jac[i].items():
                    ref._set("jac", (i, p), jets[i].g.get(p, mpf(0)), pair)
            if order > 1:
                assert set(jets[i].h) <= set(hess[i]), (i, "a pillar pair the bound does not know")
                for (p, q), pair in hess[i].items():
                    value = jets[i].h.get((p, q), mpf(0))
                    ref._set("hess", (i, p, q), value, pair)
                    ref._set("hess", (i, q, p), value, pair)
    return ref


_CACHE = {}


def _key(*arrays):
    return tuple(np.ascontiguousarray(a).tobytes() for a in arrays)


def reference(grid, rates, order=2):
    """The `Reference` of the builders on ``grid`` (anything with acc, pillar, prev_idx) at the float64 par rates ``rates``."""
    rates = np.asarray(rates, dtype=np.float64)
    key = ("build", order) + _key(grid.acc, grid.pillar, grid.prev_idx, rates)
    if key not in _CACHE:
        with mpmath.workdps(DPS):
            exact = [mpf(float(r)) for r in rates]
        _CACHE[key] = _assemble(grid.acc, grid.pillar, grid.prev_idx, exact, [(float(r), FZERO) for r in rates], rates.size, order)
    return _CACHE[key]


def shocked_reference(grid, base, shocks_row):
    """The `Reference` (dfs alone) of the values-only scans at the exact rates base + x / 10^4, the rounding of the float64
    rates the scans form counted in the bound."""
    base, x = np.asarray(base, dtype=np.float64), np.asarray(shocks_row, dtype=np.float64)[:len(base)]
    key = ("scan",) + _key(grid.acc, grid.pillar, grid.prev_idx, base, x)
    if key not in _CACHE:
        with mpmath.workdps(DPS):
            exact = [mpf(float(b)) + mpf(float(s)) / 10 ** 4 for b, s in zip(base, x)]
        bound = [shocked_rate_bound(b, s) for b, s in zip(base, x)]
        _CACHE[key] = _assemble(grid.acc, grid.pillar, grid.prev_idx, exact, bound, base.size, 0)
    return _CACHE[key]


def exact_dfs(grid, rates):
    """The discount factors at the float64 ``rates`` as float64 roundings of the 60-digit values (for the case module's
    positivity check)."""
    with mpmath.workdps(DPS):
        return np.array([float(j.v) for j in scan_value(grid.acc, grid.pillar, grid.prev_idx, [mpf(float(r)) for r in rates], 0)])


# ------------------------------------------------------------------------------------------------- the jets' cross-check
def difference_check(grid, rates, pairs, dps=110, step_exp=-30):
    """Central differences of the value recurrence at ``dps`` digits and step 10^step_exp against the jets' Hessian on the
    pillar ``pairs``: the worst |difference - jet| over the reference's bound.  The differences' noise - rounding 10^-dps
    over step^2, truncation step^2 (the fourth derivatives here are far below 10^20) - must lie 2^-20 below the smallest
    non-zero bound of the case; asserted."""
    ref = reference(grid, rates, 2)
    noise = 10.0 ** (-dps - 2 * step_exp) + 10.0 ** (2 * step_exp + 20)
    assert noise <= 2.0 ** -20 * ref.min_bound(), (noise, ref.min_bound())
    worst = 0.0
    with mpmath.workdps(dps):
        h = mpf(10) ** step_exp
        base = [mpf(float(r)) for r in rates]

        def dfs_at(dp, dq, p, q):
            r = list(base)
            r[p] += dp * h
            r[q] += dq * h
            return [j.v for j in scan_value(grid.acc, grid.pillar, grid.prev_idx, r, 0)]
        mid = dfs_at(0, 0, 0, 0)
        for p, q in pairs:
            if p == q:
                up, dn = dfs_at(1, 0, p, p), dfs_at(-1, 0, p, p)
                fd = [(u - 2 * m + d) / (h * h) for u, m, d in zip(up, mid, dn)]
            else:
                pp, pm, mp_, mm = dfs_at(1, 1, p, q), dfs_at(1, -1, p, q), dfs_at(-1, 1, p, q), dfs_at(-1, -1, p, q)
                fd = [(a - b - c + d) / (4 * h * h) for a, b, c, d in zip(pp, pm, mp_, mm)]
            for i, x in enumerate(fd):
                e = ref.e["hess"][i, p, q]
                jet = mpf(float(ref.hi["hess"][i, p, q])) + mpf(float(ref.lo["hess"][i, p, q]))
                if e == 0.0:
                    assert abs(x) <= noise, (i, p, q, x)
                else:
                    worst = max(worst, float(abs(x - jet) / mpf(e)))
    return worst
