"""One case table for both sides of the Monte Carlo VaR tests (tests/test_monte_carlo_host.py, CPU, and
tests/test_gpu_monte_carlo.py, GPU): the generator's restatements - Philox4x32-10 and the uniform map in Python integers,
Box-Muller and the factor products in mpmath at 50 digits - with the bounds both sides are held to, and the rows of the
tail select with their independent NumPy statement.

Bounds (eps = 2^-52), as the issue derives them: u is exact; the angle fl(2 pi) u2 carries at most about 1e-15 absolute
error; r <= sqrt(106 ln 2), about 8.6; log, sqrt, cos and sin are a few ulp each, so

    |dz|   <= 64 eps max(1, |z|)                                  (about ten times the sum of those)
    |dx_p| <= (64 + F) eps sum_j |factor[p][j]| max(1, |z_j|)     (F more roundings in the products)
"""
import functools

import mpmath
import numpy as np

from adrates_amd.market.position.scenarios import tail_count

EPS = 2.0 ** -52
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the references of x are kept in 80-bit long doubles"

# ------------------------------------------------------------------------------------------------------- generator
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
# counter, key, output: the published known answers of Philox4x32-10 (Random123's kat_vectors)
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)
SEEDS = (0, 1, 2 ** 32, 2 ** 64 - 1)
INDICES = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3)              # generating scenarios, reached through first_scenario
GEOMETRY = ((1, 1), (2, 1), (3, 3), (32, 32), (33, 7), (64, 64), (65, 65), (256, 255), (256, 256))      # P, F
SCENARIOS = (1, 63, 64, 65, 129)
GEOMETRY_SEED = 20261020


def philox(counter, key):
    """Philox4x32-10 in Python integers."""
    c, k = list(counter), list(key)
    for r in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return tuple(c)


def words(seed, g, i):
    return philox((g & MASK, g >> 32, i, 0), (seed & MASK, seed >> 32))


def uniforms(seed, g, i):
    """(u1, u2) as exact rationals (2 n + 1) / 2^54, n the top 53 bits of a word pair."""
    w = words(seed, g, i)
    n1, n2 = ((w[1] << 32) | w[0]) >> 11, ((w[3] << 32) | w[2]) >> 11
    return (2 * n1 + 1, 2 * n2 + 1)                               # numerators over 2^54


def uniform_doubles(seed, g, i):
    """The same rounded to double once, to nearest even (Python's integer true division is correctly rounded)."""
    a, b = uniforms(seed, g, i)
    return a / 2 ** 54, b / 2 ** 54


def generating(row, antithetic):
    """(generating scenario, negated) of a global row."""
    return (row >> 1, bool(row & 1)) if antithetic else (row, False)


@functools.lru_cache(maxsize=None)
def normal_pair(seed, g, i):
    """(z0, z1) of pair i of generating scenario g in mpmath, 50 digits, from the DOUBLES u1 and u2 (u is exact in the
    library up to its one documented rounding, which the uniforms tests pin bit for bit)."""
    with mpmath.workdps(50):
        u1, u2 = (mpmath.mpf(v) for v in uniform_doubles(seed, g, i))
        r, a = mpmath.sqrt(-2 * mpmath.log(u1)), 2 * mpmath.pi * u2
        return r * mpmath.cos(a), r * mpmath.sin(a)


def to_ld(v):
    """An mpmath number as a long double (hi + lo of two doubles: 106 bits in, 64 kept)."""
    hi = float(v)
    return LD(hi) + LD(float(v - mpmath.mpf(hi)))


def normals(seed, rows, F, antithetic=False):
    """``[len(rows), F]`` long doubles: the reference normals of the global rows ``rows`` (before the antithetic sign)."""
    out = np.zeros((len(rows), F), dtype=LD)
    for s, row in enumerate(rows):
        g, _ = generating(row, antithetic)
        for j in range(F):
            out[s, j] = normal_pair_ld(seed, g, j // 2)[j % 2]
    return out


@functools.lru_cache(maxsize=None)
def normal_pair_ld(seed, g, i):
    with mpmath.workdps(50):
        z0, z1 = normal_pair(seed, g, i)
        return to_ld(z0), to_ld(z1)


def shocks(seed, rows, factor, antithetic=False):
    """(x [S, P], bound [S, P]) in long doubles: the reference shocks (a long-double dot product of the mpmath normals:
    F 2^-64 relative, nothing against the bound) and the issue's bound on them."""
    factor = np.asarray(factor, dtype=np.float64)
    z = normals(seed, rows, factor.shape[1], antithetic)
    x = z @ factor.astype(LD).T
    sign = np.array([-1.0 if generating(r, antithetic)[1] else 1.0 for r in rows], dtype=LD)
    bound = (64 + factor.shape[1]) * EPS * (np.maximum(1.0, np.abs(z)) @ np.abs(factor).astype(LD).T)
    return x * sign[:, None], bound


def worst_z_ratio(seed, rows, got, antithetic=False):
    """max |got - z| / (64 eps max(1, |z|)) for ``got [S, F]`` made with the identity factor."""
    z = normals(seed, rows, got.shape[1], antithetic)
    sign = np.array([-1.0 if generating(r, antithetic)[1] else 1.0 for r in rows], dtype=LD)
    return float(np.max(np.abs(got.astype(LD) - z * sign[:, None]) / (64 * EPS * np.maximum(1.0, np.abs(z)))))


def worst_x_ratio(seed, rows, factor, got, antithetic=False):
    x, bound = shocks(seed, rows, factor, antithetic)
    err = np.abs(got.astype(LD) - x)
    assert np.all(err[bound == 0] == 0), "a zero bound (a zero row of the factor matrix) wants an exact zero"
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)))


def factor_matrix(P, F, seed=3):
    """A dense [P, F] factor with entries of both signs and mixed scales (bp)."""
    rng = np.random.default_rng([seed, P, F])
    return rng.standard_normal((P, F)) * 10.0 ** rng.uniform(-2, 1.5, (P, 1))


def covariance(P, seed=9):
    """A fixed SPD covariance in bp^2 with correlations of both signs."""
    rng = np.random.default_rng([seed, P])
    A = rng.standard_normal((P, P + 3))
    vol = rng.uniform(2.0, 9.0, P)
    C = A @ A.T
    d = np.sqrt(np.diag(C))
    return C / np.outer(d, d) * np.outer(vol, vol)


# ------------------------------------------------------------------------------------------------------ tail select
WIDTHS = (1, 2, 16384, 16385, 40000, 65537, 131075)
CONTENTS = ("normal", "equal", "two_values", "low_bits", "zeros", "inf", "denormal", "negative", "nan")
TAIL_MAX = 16384


def tail_counts(m):
    return sorted({k for k in (1, 2, min(m, TAIL_MAX), tail_count(0.99, m)) if 1 <= k <= m})


def base_cols(m):
    """base_col and the width of the rows: -1, the first, a middle and the last column of m + 1."""
    return ((-1, m),) + tuple(sorted({(c, m + 1) for c in (0, (m + 1) // 2, m)}))


def _from_bits(bits):
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


def pnl_rows(content, B, m, k, seed=0):
    """``[B, m]`` P&L values of one kind; ``k`` places the ties of "two_values" around the k-th value."""
    rng = np.random.default_rng([seed, CONTENTS.index(content), B, m, k])
    normal = rng.standard_normal((B, m)) * 1e6
    if content == "normal":
        return normal
    if content == "equal":
        return np.full((B, m), 3.25)
    if content == "two_values":                                     # the k-th inside the run of ties, and one either side of it
        out = np.full((B, m), 7.5)
        for b, na in zip(range(B), (k // 2, k - 1, min(k, m))):
            out[b, rng.permutation(m)[:na]] = -2.25
        return out
    if content == "low_bits":                                       # equal in the top 53 bits, and equal in the low 11 only
        top = np.float64(-1.5).view(np.uint64)
        out = np.empty((B, m))
        for b in range(B):
            low = _from_bits(top + rng.integers(0, 2048, m, dtype=np.uint64))
            high = _from_bits((rng.integers(0, 2, m, dtype=np.uint64) << np.uint64(63)) | (rng.integers(1000, 1047, m, dtype=np.uint64) << np.uint64(52))
                              | (rng.integers(0, 2 ** 41, m, dtype=np.uint64) << np.uint64(11)) | np.uint64(0x2AB))
            out[b] = (low, high, np.where(rng.random(m) < 0.5, low, high))[b % 3]
        return out
    if content == "zeros":
        out = np.where(rng.random((B, m)) < 0.5, -0.0, 0.0)
        return np.where(rng.random((B, m)) < 0.02, np.sign(normal), out)
    if content == "inf":
        out = normal.copy()
        out[rng.random((B, m)) < 0.01] = -np.inf
        out[rng.random((B, m)) < 0.01] = np.inf
        return out
    if content == "denormal":
        return rng.integers(-4000, 4000, (B, m)).astype(np.float64) * 5e-324
    if content == "negative":
        return -np.abs(normal) - 1.0
    assert content == "nan"
    normal[min(1, B - 1), rng.integers(0, m)] = np.nan               # one NaN: that row alone is NaN
    return normal


def with_base(pnl, base_col, content, seed=0):
    """The rows adr_scenario_tail_select reads: ``pnl`` itself for base_col = -1, else the columns with the base column put
    in - 0.0, so that every value survives the subtraction to the bit, except for "normal", whose base is a draw (the
    reference subtracts it as the library does)."""
    if base_col < 0:
        return np.ascontiguousarray(pnl)
    B = pnl.shape[0]
    base = np.random.default_rng([seed, 77]).standard_normal((B, 1)) * 1e5 if content == "normal" else np.zeros((B, 1))
    moved = pnl + base if content == "normal" else pnl
    return np.ascontiguousarray(np.hstack([moved[:, :base_col], base, moved[:, base_col:]]))


def sorted_pnl(rows, base_col):
    """Every row's P&L in the total order of the doubles (-0.0 before +0.0), by NumPy: np.sort on the order-preserving
    integer image of the values.  NaN rows are marked by the second result."""
    pnl = rows if base_col < 0 else np.delete(rows, base_col, axis=1) - rows[:, base_col:base_col + 1]
    bits = np.ascontiguousarray(pnl).view(np.int64)
    keys = np.sort(bits ^ ((bits >> 63) & np.int64(2 ** 63 - 1)), axis=1)
    return (keys ^ ((keys >> 63) & np.int64(2 ** 63 - 1))).view(np.float64), np.isnan(pnl).any(axis=1)


def numpy_tail(ordered, nan, k):
    """(var, es) from the sorted rows: minus the k-th smallest, minus the sequential ascending sum of the k smallest over k."""
    with np.errstate(invalid="ignore", over="ignore"):
        total = np.cumsum(ordered[:, :k], axis=1)[:, -1]             # cumsum adds in order, from the first value
        var, es = -ordered[:, k - 1], -(0.0 + total) / float(k)
    var[nan], es[nan] = np.nan, np.nan
    return var, es


def same_bits(a, b):
    """Bit for bit, a NaN matching any NaN (the payload of an inf - inf is the hardware's)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb]))


# ------------------------------------------------------------------------------------------------------------ chain
def ladders(B, P, seed=4):
    """(delta [B, P], gamma [B, P, P]) of B random desks with symmetric gamma."""
    rng = np.random.default_rng([seed, B, P])
    delta = rng.standard_normal((B, P)) * 1e4
    g = rng.standard_normal((B, P, P)) * 30.0
    return delta, 0.5 * (g + g.transpose(0, 2, 1))
