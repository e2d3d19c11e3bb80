"""The cases of the two-curve foreign-leg tests (tests/test_xccy_foreign_host.py, CPU, and tests/test_gpu_xccy_foreign.py, GPU):
the smallest shapes that reach each branch of the XC instantiations of `price_lite_kernel` (csrc/kernels_lite.hip) through
`adr_price_xccy_foreign`.  A case is ``XcCase(name, foreign scheme, foreign label, foreign host curve, XCCY scheme, XCCY label,
XCCY host curve, batch)``; the curves are `_price_edge_cases.curve`'s and `_ladder_edge_cases.lookup_curve`'s.

Curve pairs (`PAIRS`): README 32 x 31 pillars (odd P_x: `delta2`'s scalar stores) LZ x FF; 31 x 17 pillars FF x LZ; 17 pillars x
README 32 FF x FF; README 32 x 31 pillars LF x LF; the 5-pillar lookup table x the lookup table with a knot three times (other
rows: another seed, discount factors raised to 1.3) under the five scheme pairs the kernel is built for
(`_xccy_scenario_cases.PAIRS`); and ONE curve passed as both (README 32 under LZ and under LF).

Books, tens of trades each.  Every trade holds an accruing coupon with te != tp or a weight != 1, so `flag_lagged`
(route.hpp) puts it in the payment-lag rows and the entry takes the book:
  lag geometry   one-coupon trades: ts / te on, between and 5e-11 beside the FOREIGN curve's knots at its short end, middle and
                 long end; tp on, between and 5e-11 beside the XCCY curve's knots likewise; tp beyond the last knot of the
                 shorter curve and within the longer (which is the foreign one in some pairs and the XCCY one in others), and
                 beyond both; a weighted coupon paid at tp = 0 (foreign sensitivity, no basis sensitivity); a seasoned coupon
                 (ts < 0 < tp); a coupon with tp < 0 (nothing live)
  structure      abutting lagged coupons (the previous lane's D_f(te) reused) with an exchange on the first coupon's tp
                 (`fix_merged`) and one on a date of its own, pay and receive; an accrual gap (a second start of its own in the
                 row); alpha = 0 as the first coupon and inside a leg; exchanges at xt = 0 and xt < 0 under a seasoned leg;
                 n_fix > n_flt with a fixed flow in the spare lane's slot and beyond; n_fix = 0; weights != 1, 0 and negative; a
                 weighted leg with te == tp everywhere; both signs; notionals from 1 to 1e9
  counts         legs of 1, 14, 15, 16, 29, 30, 31, 45, 46, 389 and 390 coupons (rows hold 15 coupons and a spare lane; 26 rows
                 end the table): five distinct row counts (1, 2, 3, 4, 26), the `kLiteSegments` instantiation
  short counts   the legs up to 45 coupons: three distinct row counts, the three-segment instantiation (as every other book)
  launch shape   three one-row trades and one two-row trade cycled through books of 1, 3, 4 and 5 trades and of u, u + 1 and
                 2 u + 1 units: a unit is four trade slots of one row count, u = 12 blocks the units one pass of the full grid
                 takes - `R::blocks_for`: min(ceil(units / 12), n_cu) blocks of twelve waves, one block per CU
Refused books (`refused_books`): a leg of 391 coupons beside lagged ones, and a plain unlagged leg beside lagged ones.
"""
import dataclasses
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

from adrates_amd import _native

from . import _ladder_edge_cases as E
from . import _price_edge_cases as PE
from . import _price_lag_cases as PL
from . import _scenario_cases as SC
from . import _xccy_scenario_cases as XS

LZ, FF, LF = PE.LZ, PE.FF, PE.LF
SCHEME = {XS.FF: FF, XS.LF: LF, XS.LZ: LZ}
LAG = PL.LAG
COUNTS = (1, 14, 15, 16, 29, 30, 31, 45, 46, 389, 390)
SHORT_COUNTS = (1, 14, 15, 16, 29, 30, 31, 45)
ROW_BUCKETS = (1, 2, 3, 4, 6, 8, 12, 16, 26)          # route.cpp, kLiteRowBuckets: lite rows per trade, rounded up
LITE_COUPONS = 15
XC_WAVES = 12                                         # kernels_lite.hip, ADR_LITE_XC_THREADS / 64
LDS_BUDGET = 160 * 1024
PAIRS = (("README 32", LZ, "31 pillars", FF), ("31 pillars", FF, "17 pillars", LZ), ("17 pillars", FF, "README 32", FF),
         ("README 32", LF, "31 pillars", LF))
SAME = (("README 32", LZ), ("README 32", LF))


@dataclasses.dataclass
class XcCase:
    name: str
    f_interp: object
    f_label: str
    f_host: object
    x_interp: object
    x_label: str
    x_host: object
    batch: object

    @property
    def id(self):
        return f"{self.name}, {self.f_label} {self.f_interp.name} x {self.x_label} {self.x_interp.name}"

    @property
    def args(self):
        return self.f_interp.value, self.f_host, self.x_interp.value, self.x_host, self.batch


@lru_cache(maxsize=None)
def host_of(label, interp):
    if label == "lookup":
        return E.lookup_curve(SC.LOOKUP_TIMES)
    if label == "lookup, a knot three times":             # other rows than the foreign table's: another seed, other discount factors
        h = E.lookup_curve(E.LOOKUP_TIMES_TRIPLE, seed=23)
        dfs = h.dfs ** 1.3
        scale = dfs / h.dfs
        return SimpleNamespace(times=h.times, dfs=dfs, jac=h.jac * scale[:, None], hess=h.hess * scale[:, None, None])
    return PE.curve(label, interp)


# ------------------------------------------------------------------------------------------------------------- geometry
def _around(x):
    """Dates on, between and 5e-11 beside the knots of ``x`` (distinct times) at its short end, middle and long end."""
    out = []
    for i in sorted({1, x.size // 2, x.size - 2}):
        a, b = x[i], x[i + 1] if i + 1 < x.size else x[i] + 1.0
        out += [a, a + 5e-11, a - 5e-11, a + 0.37 * (b - a)]
    return [float(t) for t in out if t > 0.0]


def geometry_trades(host_f, host_x):
    xf, xx = np.unique(np.asarray(host_f.times, dtype=np.float64)), np.unique(np.asarray(host_x.times, dtype=np.float64))
    trades = []
    add = lambda ts, te, tp, **kw: trades.append(PL.coupon(float(ts), float(te), float(tp), notional=1e6 + 1e4 * len(trades),
                                                           spread=0.0011 * (len(trades) % 2), flt_sign=(-1.0) ** len(trades), **kw))
    fd = _around(xf)
    for i, t in enumerate(fd):                            # ts, then te, on / beside / between the foreign knots
        add(t, t + 0.41, t + 0.41 + LAG)
        add(max(t - 0.33, 0.5 * t), t, t + LAG)
    for t in fd[:4]:                                      # ts AND te beside foreign knots: an accrual from knot to knot
        nxt = xf[np.searchsorted(xf, t + 1e-9)] if t + 1e-9 < xf[-1] else t + 1.0
        add(t, float(nxt), float(nxt) + LAG)
    for t in _around(xx):                                 # tp on / beside / between the XCCY knots
        add(max(t - 0.3, 0.4 * t), max(t - 0.05, 0.9 * t), t)
    Tf, Tx = float(xf[-1]), float(xx[-1])
    mid = 0.5 * (Tf + Tx) if Tf != Tx else Tf + 0.75      # beyond the shorter curve's last knot, within the longer's
    add(mid - 1.0, mid, mid + LAG)
    add(min(Tf, Tx) - 0.5, min(Tf, Tx) - 0.25, mid)       # the accrual within both, the payment beyond the shorter
    add(max(Tf, Tx) - 0.5, max(Tf, Tx) + 0.5, max(Tf, Tx) + 0.5 + LAG)      # beyond both
    trades.append(PL.weighted(PL.coupon(0.5, 1.0, 0.0, notional=2e6, spread=0.0, flt_sign=1.0), 0.93))      # paid at the value time
    add(-0.1, 0.15, 0.15 + LAG)                           # seasoned
    add(-0.5, -0.25, -0.24)                               # tp < 0: nothing live
    return trades


# ------------------------------------------------------------------------------------------------------------ structure
def structure_trades():
    t = []
    q = E.abutting(0.3, 0.25, 6)
    q[:, 2] += LAG
    ex = lambda flt, N: [(float(flt[0, 2]), -N), (float(flt[1, 2]) + 0.01, 0.25 * N), (float(flt[-1, 2]), N)]
    t.append(E.make_trade(fix=ex(q, 3e6), flt=q, notional=3e6, spread=0.0, fix_sign=-1.0, flt_sign=1.0))     # abutting; merged, own date
    t.append(E.make_trade(fix=ex(q, 3e6), flt=q, notional=3e6, spread=0.002, fix_sign=1.0, flt_sign=-1.0))
    g = E.chain([0.3, 0.85, 1.4, 2.2], 0.5)
    g[:, 2] += LAG
    t.append(E.make_trade(fix=[(0.31, -1e6), (float(g[1, 2]), 1e6)], flt=g, spread=0.001))          # gaps: starts of their own; the second exchange merged
    g2 = E.abutting(0.2, 0.5, 6)
    g2[3:, 0] += 0.01                                                                              # one gap: a second start inside the row
    g2[:, 2] += LAG
    t.append(E.make_trade(flt=g2, spread=0.0005, notional=1e9, flt_sign=1.0))
    z = E.abutting(0.2, 0.5, 5)
    z[:, 2] += LAG
    z[0, 3] = 0.0
    z[2, 3] = 0.0
    t.append(E.make_trade(flt=z, spread=0.003, notional=2e6, flt_sign=1.0))                        # alpha = 0 first and inside
    s5 = E.abutting(-0.3, 0.25, 5)
    s5[:, 2] += LAG
    t.append(E.make_trade(fix=[(0.0, -5e5), (-0.2, 7.0), (float(s5[-1, 2]), 5e5)], flt=s5, notional=5e5, spread=0.0007))      # xt = 0, xt < 0
    s3 = E.abutting(0.45, 1.0, 3)
    s3[:, 2] += LAG
    fix6 = [(float(s3[0, 2]), 100.0), (float(s3[1, 2]), 200.0), (2.0, 300.0), (2.6, 400.0), (3.1, 500.0), (9.5, 600.0)]
    t.append(E.make_trade(fix=fix6, flt=s3, notional=1.0, spread=0.01, fix_sign=-1.0, flt_sign=1.0))      # n_fix > n_flt: lane 3 is the spare lane's
    s = E.abutting(0.45, 1.0, 4)
    sl = s.copy()
    sl[:, 2] += LAG
    t.append(PL.weighted(E.make_trade(fix=[(float(sl[0, 2]), 41000.0)], flt=sl, spread=0.0005, flt_sign=1.0, fix_sign=-1.0), [0.97, 0.94, 0.91, 0.88]))
    t.append(PL.weighted(E.make_trade(flt=sl, spread=0.001), [1.0, 0.0, 1.0, 1.03]))               # w = 0 on one coupon; n_fix = 0
    t.append(PL.weighted(E.make_trade(flt=sl, spread=0.001, notional=5e5), [1.0, -0.5, 1.0, 1.0]))  # a negative w
    t.append(PL.weighted(E.make_trade(fix=[(float(s[-1, 2]), 1e6)], flt=s, spread=0.0005, notional=1e6), 0.97))      # weighted, te == tp everywhere
    t.append(PL.weighted(E.make_trade(flt=sl, spread=0.002, notional=3e3), 0.0))                   # every weight 0: nothing live
    return t


# --------------------------------------------------------------------------------------------------------------- counts
def counts_trades(counts=COUNTS):
    out = []
    for i, m in enumerate(counts):
        period = 0.25 if m <= 46 else 1.0 / 12.0
        leg = PL.lagged_leg(m, period, first=0.02 + 0.003 * i, notional=10.0 ** (i % 10), spread=0.0007 * (i % 2), pay_fixed=i % 2 == 0,
                            coupon_rate=0.0)
        N = leg["notional"]
        leg["fix"] = np.array([(float(leg["flt"][0, 2]), -N), (float(leg["flt"][-1, 2]), N)])      # the exchanges: the first merged
        out.append(leg)
    return out


def rows_of(batch):
    """Lite rows per trade as the upload buckets them (route.cpp, `lite_bucket`); 0: beyond the table."""
    m = np.maximum(np.diff(batch.flt_off), np.diff(batch.fix_off))
    rows = np.maximum(1, -(-m // LITE_COUPONS))
    return np.array([next((b for b in ROW_BUCKETS if b >= r), 0) for r in rows])


def units_of(batch):
    """Units (four trade slots of one row count) of the payment-lag row table."""
    rows = rows_of(batch)
    return int(sum(-(-np.count_nonzero(rows == b) // 4) for b in ROW_BUCKETS))


# ---------------------------------------------------------------------------------------------------------- launch shape
def launch_trades():
    one = [PL.lagged_leg(m, 0.25, first=0.02 + 0.003 * i, notional=1e6 * (i + 1), spread=0.0007 * (i % 2), pay_fixed=i % 2 == 0)
           for i, m in enumerate((1, 8, 15))]
    return one + [PL.lagged_leg(16, 0.25, first=0.031, notional=4e6, spread=0.0009, pay_fixed=False)]


def cycled_book(size):
    base = launch_trades()
    return PL.make_book([base[i % 4] for i in range(size)])


def cycled_units(size):
    two = size // 4
    return -(-(size - two) // 4) + -(-two // 4)


def blocks_for(units, n_cu):
    """`R::blocks_for(units, 12, n_cu)`: one block of twelve waves per CU."""
    return min(-(-units // XC_WAVES), n_cu)


def launch_sizes(n_cu):
    """Books of 1, 3, 4, 5 trades, then the smallest books of u, u + 1 and 2 u + 1 units, u = 12 n_cu."""
    u = XC_WAVES * n_cu
    out = [1, 3, 4, 5]
    for target in (u, u + 1, 2 * u + 1):
        size = 4 * target // 2
        while cycled_units(size) < target:
            size += 1
        while cycled_units(size - 1) >= target:
            size -= 1
        assert cycled_units(size) == target
        out.append(size)
    return out


# ------------------------------------------------------------------------------------------------------------------ LDS
LUT_PER_YEAR, LUT_MAX = 4.0, 512
REC_BYTES_PER_WAVE = 4 * (2 * 16 + 2) * 16
PILLAR_PAD = 32


def curve_sizes(host):
    """(K, Kc, n_lut) as `build_curve_tables` (curve_tables.cpp) derives them."""
    x = np.asarray(host.times, dtype=np.float64)
    n_lut = min(LUT_MAX, int(max(x[-1], 0.0) * LUT_PER_YEAR) + 2)
    from . import _ladder_reference as R
    return x.size, R.compact_count(x), n_lut


def xc_lds_bytes(host_f, host_x):
    """`lite_xc_kernel_lds_bytes` (kernels_lite.hip) restated: the delta instantiation's bytes at eight waves, four more waves'
    entry slots, the second curve's Jacobian table and search arrays; no less than the reduction's [12][1 + 64] doubles."""
    K, Kc, n_lut = curve_sizes(host_f)
    base = 8 * REC_BYTES_PER_WAVE + 8 * Kc * PILLAR_PAD + 8 * (2 * K + 2 * Kc) + 2 * (2 * K + 2 * n_lut)
    base = (max(base, 8 * 8 * (1 + PILLAR_PAD)) + 15) & ~15
    Kx, Kcx, n_lut_x = curve_sizes(host_x)
    total = base + (XC_WAVES - 8) * REC_BYTES_PER_WAVE + 8 * (Kcx * PILLAR_PAD + 2 * Kx + 2 * Kcx) + 2 * (2 * Kx + 2 * n_lut_x)
    return (max(total, 8 * XC_WAVES * (1 + 2 * PILLAR_PAD)) + 15) & ~15


def big_curve(K, seed):
    """A hand-made 5-pillar table of K distinct knots (but for `lookup_curves`' repeated value at knot 3) out to 6 years."""
    times = np.concatenate([[0.0], np.linspace(0.05, 6.0, K - 1)])
    return E.lookup_curve(times, seed=seed)


@lru_cache(maxsize=None)
def lds_pairs():
    """``(inside, beyond)``: two pairs of hand-made tables, the first just inside the LDS budget, the second just beyond it (a
    knot more on the XCCY side)."""
    Kf = 240
    f = big_curve(Kf, 31)
    Kx = 8
    while xc_lds_bytes(f, big_curve(Kx + 1, 32)) <= LDS_BUDGET:
        Kx += 1
    inside, beyond = big_curve(Kx, 32), big_curve(Kx + 1, 32)
    assert xc_lds_bytes(f, inside) <= LDS_BUDGET < xc_lds_bytes(f, beyond)
    return (f, inside), (f, beyond)


# ---------------------------------------------------------------------------------------------------------------- cases
@lru_cache(maxsize=None)
def cases():
    out = []
    mk = lambda name, fl, fi, xl, xi, trades: out.append(XcCase(name, fi, fl, host_of(fl, fi), xi, xl, host_of(xl, xi), PL.make_book(trades)))
    for fl, fi, xl, xi in PAIRS:
        mk("lag geometry", fl, fi, xl, xi, geometry_trades(host_of(fl, fi), host_of(xl, xi)))
        mk("structure", fl, fi, xl, xi, structure_trades())
    for fm, xm in XS.PAIRS:
        fi, xi = SCHEME[fm], SCHEME[xm]
        fl, xl = "lookup", "lookup, a knot three times"
        mk("lag geometry", fl, fi, xl, xi, geometry_trades(host_of(fl, fi), host_of(xl, xi)) + structure_trades())
    for label, interp in SAME:
        mk("one curve as both: lag geometry and structure", label, interp, label, interp,
           geometry_trades(host_of(label, interp), host_of(label, interp)) + structure_trades())
    mk("counts", *PAIRS[0], counts_trades())
    mk("counts", *PAIRS[3], counts_trades())
    mk("short counts", *PAIRS[1], counts_trades(SHORT_COUNTS))
    mk("short counts", *PAIRS[2], counts_trades(SHORT_COUNTS))
    return tuple(out)


def launch_case():
    fl, fi, xl, xi = PAIRS[0]
    return XcCase("launch shape", fi, fl, host_of(fl, fi), xi, xl, host_of(xl, xi), cycled_book(4))


def refused_books():
    """``[(name, batch)]``: books the entry refuses whole - a leg beyond the row table, a leg without lag or weights."""
    lagged = counts_trades((1, 15))
    return [("a leg of 391 coupons", PL.make_book(lagged + [PL.lagged_leg(391, 1.0 / 12.0, notional=2e6)])),
            ("an unlagged leg", PL.make_book(lagged + [PE.leg_trade(8, 0.25)]))]


def route(case, mask=3, per_trade=True, aggregate=False, n_cu=256, batch=None):
    h = case.f_host
    return _native.route_host(case.f_interp.value, h.times, h.dfs, h.jac, h.hess, case.batch if batch is None else batch, mask,
                              per_trade=per_trade, aggregate=aggregate, n_cu=n_cu)
