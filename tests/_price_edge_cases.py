"""The cases of the per-trade pricing edge tests (tests/test_price_edges_host.py, CPU, and tests/test_gpu_price_edges.py, GPU):
`adr_price` on one pillar tile (P <= 32), trades whose accruing coupons are paid on their accrual end, no weights - the domain of
`_ladder_reference.rates_reference`.  Every case is ``PriceCase(name, scheme, curve label, host curve, batch)``; `LAYOUTS` holds
per curve label (packed_ok, entries per lane, core slots per lane, hub layout) and general_lds_rows as `curve_layout_host` must
report them: the CPU module asserts both and the kernel family of every request (`families`), so that the GPU module cannot
silently measure another kernel.

Curves (the instantiation of the fast gamma kernel each selects, `gamma_kernel_for`):
  README 32 pillars            (7, 5, hub)    all three schemes; LINEAR_FWD_RATES is a compilation of its own (kernels_fast_lindf.hip)
  31 pillars (`_route_cases`)  (7, 5, hub)    odd P: the matrix's last element is stored on its own, rows are 8-byte aligned
  17 pillars (`_route_cases`)  (7, 7)
  21 pillars, EPG8_TENORS      (8, 8)         11M, 1Y, 2Y ... 20Y: 20 core pillars
  32 pillars, CORE21_TENORS    (12, 12)       general_lds_rows 0: a trade beyond the chains takes the general kernel's L2 variant
  5-pillar lookup tables       packed_ok 0    dense hand-made tables: the general kernel's L2 variant, the lite kernel, the knot pass
The epg 18 shapes and the 25-core epg 12 shape need more than 160 KiB of LDS; the route sends those curves to the general
kernel, so no case asks for them."""
import dataclasses
from functools import lru_cache

import numpy as np

from adrates_amd import _native
from adrates_amd.market.curves.curve_tables import build_engine_curve
from adrates_amd.utils import InterpTypes

from . import _fixtures as F
from . import _ladder_edge_cases as E
from . import _route_cases as RC
from . import _scenario_cases as SC

VD = F.README_VALUE_DT
LZ, FF, LF = InterpTypes.LINEAR_ZERO_RATES, InterpTypes.FLAT_FWD_RATES, InterpTypes.LINEAR_FWD_RATES
SCHEMES = (LZ, FF, LF)

EPG8_TENORS = ["11M", "1Y"] + [f"{y}Y" for y in range(2, 21)]
EPG8_PX = [5.2, 5.18] + [4.6 - 0.02 * i for i in range(19)]
CORE21_TENORS = ["1W", "2W", "1M", "2M", "3M", "4M", "5M", "6M", "7M", "8M", "9M", "1Y"] + [f"{y}Y" for y in range(2, 19)] + ["20Y", "25Y", "30Y"]
CORE21_PX = [5.20 - 0.02 * i for i in range(12)] + [4.6 - 0.03 * i for i in range(20)]

# name -> (packed_ok, entries_per_lane, core_slots_per_lane, hub_layout), general_lds_rows
LAYOUTS = {"README 32": ((1, 7, 5, 1), 1), "31 pillars": ((1, 7, 5, 1), 1), "17 pillars": ((1, 7, 7, 0), 1),
           "epg 8": ((1, 8, 8, 0), 0), "core21 epg 12": ((1, 12, 12, 0), 0), "lookup": ((0, 0, 0, 0), 0)}

# requests of the GPU module: (name, mask, per_trade, aggregate)
REQUESTS = (("mask 7 per trade", 7, True, False), ("mask 7 per trade + aggregate", 7, True, True), ("mask 7 aggregate only", 7, False, True),
            ("mask 3 per trade", 3, True, False), ("mask 3 aggregate only", 3, False, True), ("mask 1 per trade", 1, True, False))

LAUNCH_SIZES = (1, 2, 3, 24, 25, 49)      # rows per launch of the launch-shape check: a block pass is 12 waves x 2 trades


@dataclasses.dataclass
class PriceCase:
    name: str
    interp: InterpTypes
    curve: str               # key of LAYOUTS
    host: object             # times, dfs, jac, hess
    batch: object            # TradeBatch

    @property
    def id(self):
        return f"{self.name}, {self.curve}, {self.interp.name}"


@lru_cache(maxsize=None)
def curve(label, interp):
    if label == "README 32":
        return RC.engine_curve(VD, 32, interp)
    if label == "31 pillars":
        return RC.engine_curve(VD, 31, interp)
    if label == "17 pillars":
        return RC.engine_curve(VD, 17, interp)
    px, tenors = (EPG8_PX, EPG8_TENORS) if label == "epg 8" else (CORE21_PX, CORE21_TENORS)
    c = F.gbp_model(VD, interp, px=px, tenors=tenors).curves.GBP_OIS_SONIA
    return build_engine_curve(c.swap_rates, c.swap_times, c.year_fracs)


def layout_of(host):
    """(packed_ok, epg, cpg, hub), general_lds_rows of a curve, as the library's host code lays it out."""
    i = _native.curve_layout_host(host.times, host.dfs, host.jac, host.hess)
    packed = i["packed_ok"]
    return (packed, i["entries_per_lane"] * packed, i["core_slots_per_lane"] * packed, i["hub_layout"] * packed), i["general_lds_rows"]


# ---------------------------------------------------------------------------------------------------------------- books
def annual_fix(first, last, pay):
    """Annual fixed flows ending on ``last``, none before ``first``."""
    n = max(1, int(np.floor(last - first + 1e-9)))
    return [(last - i, pay) for i in range(n)][::-1]


def leg_trade(m, period, first=0.02, notional=1e6, spread=0.0007, pay_fixed=True, coupon=0.04):
    """``m`` abutting coupons with a spread (interior nodes live) against an annual fixed leg."""
    flt = E.abutting(first, period, m)
    last = float(flt[-1, 2])
    sign = 1.0 if pay_fixed else -1.0
    return E.make_trade(fix=annual_fix(max(first, 0.0), last, coupon * notional), flt=flt, notional=notional, spread=spread,
                        fix_sign=-sign, flt_sign=sign)


ROW_COUPONS = (1, 31, 32, 33, 64, 65, 96, 97, 384, 385)
ROW_CHAINS = {33: 2, 64: 2, 65: 3, 96: 3, 97: 4, 384: 12}


def row_geometry_trades():
    """Coupon counts on both sides of every row and chain boundary: 1, 31, 32 coupons are one row of the fast table; 33 ... 384
    chains of 2, 2, 3, 3, 4 and 12 rows; 385 the general kernel.  Quarterly up to 97 coupons, monthly beyond (the curve ends at
    50Y); signs alternate; the 31-coupon leg is seasoned (its first two coupons paid in the past, the third accruing over the
    value time)."""
    out = []
    for i, m in enumerate(ROW_COUPONS):
        period = 0.25 if m <= 97 else 1.0 / 12.0
        first = -0.6 if m == 31 else 0.02 + 0.003 * i
        out.append(leg_trade(m, period, first=first, notional=1e6 * (i + 1), spread=0.0007 + 0.0001 * i, pay_fixed=i % 2 == 0))
    return out


def one_row_trades():
    return [t for t, m in zip(row_geometry_trades(), ROW_COUPONS) if m <= 32]


def row_geometry_book():
    return E.make_book(row_geometry_trades())


def cycled_book(size):
    """``size`` rows cycling the one-row trades of the row geometry book: trade i is one-row trade i mod 3."""
    base = one_row_trades()
    return E.make_book([base[i % len(base)] for i in range(size)])


def knot_sweep_trades(host):
    """One fixed flow on every distinct knot time > 0, at every midpoint of adjacent distinct knots and one beyond the last
    knot; then one one-coupon trade per pair of adjacent intervals (accrual start in one, accrual end = payment in the next,
    spread != 0).  Signs alternate.  A node on every knot and in every interval the packed layout was built for: every fringe
    pair, every short-end record, and every structural zero of the gamma matrix."""
    x = np.unique(np.asarray(host.times, dtype=np.float64))
    mids = 0.5 * (x[:-1] + x[1:])
    times = np.concatenate([x[x > 0.0], mids, [x[-1] + 7.5]])
    trades = [E.make_trade(fix=[(float(t), 1000.0 + 3.0 * i)], fix_sign=(-1.0) ** i) for i, t in enumerate(times)]
    for i in range(mids.size - 1):
        ts, te = float(mids[i]), float(mids[i + 1])
        trades.append(E.make_trade(flt=[(ts, te, te, te - ts)], notional=1e6 + 1e4 * i, spread=0.0011, flt_sign=(-1.0) ** i))
    return trades


def knot_sweep_book(host, beyond_the_chains=False):
    trades = knot_sweep_trades(host)
    if beyond_the_chains:                     # one leg of 385 coupons: the general kernel on this curve
        trades.append(leg_trade(385, 1.0 / 12.0, first=0.013, notional=2e6, spread=0.0009, pay_fixed=False))
    return E.make_book(trades)


# ---------------------------------------------------------------------------------------------------------------- cases
SWEEPS = (("README 32", LZ), ("README 32", FF), ("README 32", LF), ("31 pillars", LZ), ("17 pillars", LF), ("epg 8", LZ), ("epg 8", LF),
          ("core21 epg 12", FF))


@lru_cache(maxsize=None)
def cases():
    out = []
    for label, interp in SWEEPS:
        host = curve(label, interp)
        out.append(PriceCase("knot sweep", interp, label, host, knot_sweep_book(host, beyond_the_chains=label == "core21 epg 12")))
    for interp in SCHEMES:
        out.append(PriceCase("folding", interp, "README 32", curve("README 32", interp), E.folding_book()))
    out.append(PriceCase("folding", LZ, "epg 8", curve("epg 8", LZ), E.folding_book()))
    for interp in SCHEMES:
        out.append(PriceCase("long legs", interp, "README 32", curve("README 32", interp), E.long_leg_book()[0]))
    for interp in SCHEMES:
        for name, times in (("lookup", SC.LOOKUP_TIMES), ("lookup, a knot three times", E.LOOKUP_TIMES_TRIPLE)):
            out.append(PriceCase(name, interp, "lookup", E.lookup_curve(times), E.lookup_book()))
    for interp in SCHEMES:
        out.append(PriceCase("row geometry", interp, "README 32", curve("README 32", interp), row_geometry_book()))
    return out


def lagged(batch):
    """Per trade: a coupon accrues to another date than it is paid on, or carries a weight != 1 (route.hpp, flag_lagged)."""
    out = np.zeros(batch.n_trades, dtype=bool)
    for t in range(batch.n_trades):
        j = slice(int(batch.flt_off[t]), int(batch.flt_off[t + 1]))
        out[t] = np.any((batch.flt_alpha[j] > 0.0) & (batch.flt_te[j] != batch.flt_tp[j])) or (
            batch.flt_weight is not None and np.any(batch.flt_weight[j] != 1.0))
    return out


def row_class(batch):
    """Per trade "fast" (one row of 32 slots), "fast_chained" (2 to 12 rows) or "general" (route.cpp, trade_layout); a trade
    with payment lag or weights: "fast_lag" (one row), "fast_lag_chained" (2 to 4 rows: 128 coupons) or "lag_rest"."""
    m = np.maximum(np.diff(batch.flt_off), np.diff(batch.fix_off))
    rows = np.maximum(1, -(-m // 32))
    plain = np.where(rows == 1, "fast", np.where(rows <= 12, "fast_chained", "general"))
    return np.where(lagged(batch), np.where(rows == 1, "fast_lag", np.where(rows <= 4, "fast_lag_chained", "lag_rest")), plain)


def families(case, mask, per_trade, aggregate):
    """The kernel family that prices each trade of ``case`` under a request (route.hpp, make_plan, up to 32 pillars), [n] of
    str: with GAMMA per trade the fast kernels by row class where the curve has the packed layout, else the general kernel;
    PV / PV + delta per trade the lite kernel up to 384 coupons per leg; an aggregate-only request with DELTA or GAMMA the
    knot pass for those; the general kernel for what is left.  A trade with payment lag or weights: with GAMMA per trade the
    fast kernel's payment-lag variant up to 128 coupons where the curve has the packed layout, an even pillar count and a
    log-linear scheme; without GAMMA `lite_lag` up to 390 coupons per leg (26 rows of 15), aggregate-only `knot_lag` for those
    (every curve here has at most 256 reachable knots); the general kernel for what is left."""
    batch = case.batch
    cls = row_class(batch)
    lag = lagged(batch)
    packed = LAYOUTS[case.curve][0][0]
    m = np.maximum(np.diff(batch.flt_off), np.diff(batch.fix_off))
    in_table = np.where(lag, m <= 390, cls != "general")
    if not per_trade and mask & 6:
        return np.where(in_table, np.where(lag, "knot_lag", "knot"), "general")
    if mask & 4:
        use_lag = packed and case.interp != LF and case.host.jac.shape[1] % 2 == 0
        plain = cls if packed else np.full(cls.shape, "general")
        return np.where(lag, np.where(use_lag & (cls != "lag_rest"), cls, "general"), plain)
    return np.where(in_table, np.where(lag, "lite_lag", "lite"), "general")
