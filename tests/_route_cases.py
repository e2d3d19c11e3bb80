"""The cases of the launch-plan cross product (adrates_amd/csrc/route.hpp, make_plan): trade classes, the `edges` batch of
exact coupon counts, the curves of every pillar class and the mixes.  Shared by the CPU route table (test_route_table.py),
which checks that every trade is priced exactly once, and the GPU parity matrix (test_gpu_route_matrix.py), which prices
every cell with the HIP kernels against the C oracle."""
import numpy as np

from adrates_amd import _native
from adrates_amd.market.curves.curve_tables import build_engine_curve
from adrates_amd.trades.compiler import OISTerms, TradeBatch, compile_ois_terms
from adrates_amd.utils import BusDayAdjustTypes, CurrencyTypes, CurveTypes, DayCountTypes, FrequencyTypes, InterpTypes

from . import _fixtures as F

ALL = ("plain", "long", "very_long", "lag", "long_lag", "very_long_lag", "weighted")
MIXES = [ALL, ("plain",), ("lag",), ("long",), ("long_lag",), ("weighted",), ("plain", "very_long_lag"), ("very_long",), ("edges",)]
SCHEMES = (InterpTypes.LINEAR_ZERO_RATES, InterpTypes.FLAT_FWD_RATES, InterpTypes.LINEAR_FWD_RATES)
LDS_BUDGET = 160 * 1024          # what adr_curve_upload allows the general kernel's curve tables (capi.hip, kLdsBudget)


def batch(vd, classes):
    """A few trades of each requested class; returns (batch, class label per trade).  ("edges",): `edges_batch`."""
    if tuple(classes) == ("edges",):
        b, labels, _ = edges_batch()
        return b, labels
    spec = {          # class -> (float frequency, tenors in months, payment lag)
        "plain": (FrequencyTypes.ANNUAL, [7, 60, 133, 360], 0),
        "long": (FrequencyTypes.QUARTERLY, [130, 240, 360], 0),                  # 44-120 coupons: chained rows
        "very_long": (FrequencyTypes.MONTHLY, [400, 480], 0),                    # > 384 coupons: general kernel
        "lag": (FrequencyTypes.ANNUAL, [9, 48, 200, 360], 2),
        "long_lag": (FrequencyTypes.QUARTERLY, [150, 300], 2),                   # 50-100 coupons: chained payment-lag rows
        "very_long_lag": (FrequencyTypes.MONTHLY, [200, 360], 2),                # > 128 coupons with lag: the rest list
    }
    tenors, freqs, lags, labels = [], [], [], []
    for c in classes:
        if c == "weighted":
            continue
        f, months, lag = spec[c]
        for m in months:
            tenors.append(f"{m}M"); freqs.append(f); lags.append(lag); labels.append(c)
    n_w = 3 if "weighted" in classes else 0
    for m in (30, 96, 250)[:n_w]:
        tenors.append(f"{m}M"); freqs.append(FrequencyTypes.SEMI_ANNUAL); lags.append(0); labels.append("weighted")
    n = len(tenors)
    terms = OISTerms(effective_dt=vd, tenor=tenors, coupon=np.full(n, 0.04), notional=np.full(n, 1e7), pay_fixed=np.arange(n) % 2 == 0,
                     fixed_freq_type=FrequencyTypes.ANNUAL, fixed_dc_type=DayCountTypes.ACT_365F, floating_index=CurveTypes.GBP_OIS_SONIA,
                     currency=CurrencyTypes.GBP, float_freq_type=freqs, float_dc_type=DayCountTypes.ACT_365F, payment_lag=lags,
                     bd_type=BusDayAdjustTypes.MODIFIED_FOLLOWING)
    b = compile_ois_terms(terms, vd)
    if n_w:
        w = np.ones(b.flt_tp.shape[0])
        for t in range(n - n_w, n):
            w[b.flt_off[t]:b.flt_off[t + 1]] = 0.97          # per-coupon notional multipliers (the XCCY foreign leg)
        b.flt_weight = w
    return b, labels


# The `edges` class: (label, float coupons, period in years, first accrual start, payment lag in years).  Coupon counts sit on
# both sides of every boundary of the trade tables (route.hpp): 15 / 16 coupons per lite row, 32 / 33 per fast row, 45 / 46 and
# 120 / 121 lite-row buckets (3 / 4 and 8 / 9 rows of 15), 384 / 385 the longest chain of rows (kMaxChain), 128 / 129 the
# longest payment-lag chain (kMaxChainLag), 390 / 391 the longest payment-lag lite rows (26 x 15).  Periods of a quarter from
# t = 0 end exactly on the 1Y, 2Y and 10Y pillars (knot times 1.0, 2.0, 10.0 of every curve built from the README tenors);
# the 16-coupon leg starts in the past (its first coupon paid at t = -0.05 < 0); the 120 / 121-coupon legs run to 60 years,
# past the last pillar of every curve; the 1-coupon leg is paid today (t = 0, the first knot).
EDGES = [
    ("plain", 1, 0.25, -0.25, 0.0), ("plain", 15, 0.25, 0.0, 0.0), ("plain", 16, 0.25, -0.3, 0.0), ("plain", 32, 0.25, 0.0, 0.0),
    ("plain", 33, 0.25, 0.0, 0.0), ("plain", 45, 0.25, 0.0, 0.0), ("plain", 46, 0.25, 0.0, 0.0), ("plain", 120, 0.5, 0.0, 0.0),
    ("plain", 121, 0.5, 0.0, 0.0), ("plain", 384, 1 / 12, 0.0, 0.0), ("plain", 385, 1 / 12, 0.0, 0.0),
    ("lag", 32, 0.25, 0.0, 2 / 365), ("lag", 33, 0.25, 0.0, 2 / 365), ("lag", 128, 0.25, 0.0, 2 / 365),
    ("lag", 129, 0.25, 0.0, 2 / 365), ("lag", 390, 1 / 12, 0.0, 2 / 365), ("lag", 391, 1 / 12, 0.0, 2 / 365),
    ("weighted", 32, 0.5, 0.0, 0.0), ("weighted", 33, 0.5, 0.0, 0.0),
]


def edges_batch():
    """The `edges` trades as a TradeBatch built directly (coupon counts exact, independent of the calendar); returns (batch,
    labels "plain-385" ..., float coupon count per trade).  Fixed legs: annual flows on the float leg's span, never more than
    the float coupons, so the float count decides the trade's tables."""
    fix_off, flt_off = [0], [0]
    fix_tp, fix_pay, tp, ts, te, al, wt, labels, counts = [], [], [], [], [], [], [], [], []
    for kind, c, h, t0, lag in EDGES:
        b = t0 + h * np.arange(c + 1)
        if h == 0.25 and t0 == 0.0:
            assert b[4] == 1.0 and (c < 40 or b[40] == 10.0)           # period ends exactly on knot times
        ts += list(b[:-1]); te += list(b[1:]); tp += list(b[1:] + lag); al += list(np.diff(b))
        wt += [0.97 if kind == "weighted" else 1.0] * c
        years = max(1, min(c, int(np.ceil(b[-1] - max(t0, 0.0)))))
        fix_tp += list(b[-1] - np.arange(years)[::-1]); fix_pay += [1.0] * years
        fix_off.append(len(fix_tp)); flt_off.append(len(tp))
        labels.append(f"{kind}-{c}"); counts.append(c)
    n = len(EDGES)
    f = lambda a: np.asarray(a, dtype=np.float64)
    b = TradeBatch(np.asarray(fix_off, dtype=np.int64), np.asarray(flt_off, dtype=np.int64), f(fix_tp), 0.041 * f(fix_pay), f(tp),
                   f(ts), f(te), f(al), np.round(np.linspace(1e6, 3e7, n), -5), np.where(np.arange(n) % 3 == 0, 0.001, 0.0),
                   np.where(np.arange(n) % 2 == 0, 1.0, -1.0), np.where(np.arange(n) % 2 == 0, -1.0, 1.0), f(wt))
    assert b.flt_tp[0] == 0.0 and np.min(b.flt_tp) < 0.0 and np.max(b.flt_tp) > 60.0
    return b, labels, counts


# ------------------------------------------------------------------------------------------------------------------ curves
# label -> (pillars P, knots K, reachable knots Kc, LDS bytes adr_curve_upload checks) of the curve `curve_quotes` builds
CURVES = {
    32: (32, 264, 107, 37232), 31: (31, 263, 106, 36944), 17: (17, 161, 59, 33824), 40: (40, 407, 107, 66336),
    64: (64, 1242, 114, 80112), 96: (96, 1585, 178, 118528),
    33: (33, 188, 52, 34224), 63: (63, 1193, 112, 78448), 65: (65, 1292, 116, 81776),     # 65: three tiles, the last of one pillar
    128: (128, 1400, 196, 125952), 129: (129, 1410, 198, 127152),                          # four tiles exactly / five
    155: (155, 2021, 250, 162352),                          # the largest weekly-short-end curve the upload accepts (156: 163 872)
    256: (256, 257, 257, 144944),                           # single-period pillars: eight tiles, 36 tile pairs
}
REALISTIC_MAX = 155              # the most pillars of the weekly-short-end curves the upload accepts; one more is refused
SLOW = (128, 256)                # the largest curves of the GPU matrix, marked slow


def curve_quotes(label):
    """(quotes, tenors) of a curve of the route table."""
    from .test_gpu_many_pillars import forty_pillar_quotes, many_pillar_quotes, short_dated_quotes, weekly_pillar_quotes
    if label == 32:
        return list(F.GBP_PX), list(F.TENORS)
    if label == 31:
        return list(F.GBP_PX[:13]) + list(F.GBP_PX[14:]), list(F.TENORS[:13]) + list(F.TENORS[14:])
    if label == 17:
        return list(F.GBP_PX[8:9] + F.GBP_PX[14:30]), list(F.TENORS[8:9] + F.TENORS[14:30])
    if label == 40:
        return forty_pillar_quotes()
    if label in (33, 63, 64, 65, 96):
        return many_pillar_quotes(label)
    if label == 256:
        return short_dated_quotes(256)
    return weekly_pillar_quotes(label)


def engine_curve(vd, label, interp=InterpTypes.LINEAR_ZERO_RATES, with_hessian=True):
    """The host tables of a curve of the route table, with its pillar and knot counts checked against CURVES."""
    px, tenors = curve_quotes(label)
    curve = F.gbp_model(vd, interp, px=px, tenors=tenors).curves.GBP_OIS_SONIA
    host = build_engine_curve(curve.swap_rates, curve.swap_times, curve.year_fracs, with_hessian=with_hessian)
    assert len(np.unique(np.asarray(curve.swap_times))) == host.n_pillars          # no two pillars share a maturity
    assert curve_sizes(host) == CURVES[label], (label, curve_sizes(host))
    return host


def curve_sizes(host):
    """(P, K, Kc, LDS bytes the upload checks) of host curve tables."""
    info = _native.curve_layout_host(host.times, host.dfs, host.jac)
    kc = len(_native.curve_tables_host(host.times, host.dfs, host.jac)["knot_index"])
    return host.n_pillars, host.times.shape[0], kc, info["upload_lds_bytes"]


def curves(vd, interp=InterpTypes.LINEAR_ZERO_RATES, with_hessian=True):
    return {label: engine_curve(vd, label, interp, with_hessian) for label in CURVES}


def curve_flags(label):
    """Upload flags each curve is priced with: the 40-pillar curve on its wide layout and on 32-pillar tiles."""
    return (0, _native.DeviceCurve.PILLAR_TILES) if label == 40 else (0,)

# (family, scheme) pairs the CPU table produces over these curves and mixes: every family under every scheme, but the
# payment-lag variant of the fast kernel (one-row and chained) serves the log-linear schemes only (route.hpp, use_lag)
FAMILY_SCHEMES = ({(f, s.name) for f in _native.ROUTE_FAMILIES for s in SCHEMES}
                  - {("fast_lag", "LINEAR_FWD_RATES"), ("fast_lag_chained", "LINEAR_FWD_RATES")})
