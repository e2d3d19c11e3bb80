"""The cases of the pricing edge tests beyond one pillar tile (tests/test_price_wide_host.py, CPU, and
tests/test_gpu_price_wide.py, GPU): `adr_price` on curves of 33 to 97 pillars - the wide variants of the general kernel
(33-64 pillars, kernels_general.hip `add_nodes_wide`, the packed upper triangle in 7 / 10 / 17 chunks of 128 entries, the
banded stores through `wide_store_map`, `reduce_wide_kernel`) and the general kernel once per pair of 32-pillar tiles (more
than 64 pillars, or `DeviceCurve.PILLAR_TILES`).  Books, requests and the reference are those of tests/_price_edge_cases.py;
a case adds the upload flags, the route and the chunk count `curve_layout_host` must report, and - the lagged cases - the
rows outside the reference's domain.

Dense hand-made curves (`lookup_curve`, every gamma entry of every trade live: every packed entry, band and store position
carries a number), the 26-trade lookup book:
  P = 33, 41 (7 chunks), 42, 49 (10 chunks), 50, 63, 64 (17 chunks); a knot three times at 41 and 64; all three schemes at 41,
  49 and 64;  tiled: 65 (the last tile has one pillar), 96 (three full tiles), 97; PILLAR_TILES at 33 (the second tile has one
  pillar) and at 64 (two full tiles)
Bootstrapped curves (sparse: the chunk masks `wide_knot_chunks`, the structural zeros), each with its own knot sweep:
  40 pillars under all three schemes (195 trades, 250 629 of 312 000 gamma entries have gross 0), 33 and 64 pillars under one
  scheme each; tiled: 65 pillars under all three schemes, the 40-pillar sweep under PILLAR_TILES
The row geometry book on the 40-pillar curve: ten trades on the wide kernel under mask 7; under masks 3 and 1 the lite kernel's
  64-pillar instantiations take their table and the 385-coupon leg alone reaches the wide kernel's delta-only and PV-only ones
The lookup book with one payment-lag coupon trade appended, P = 41, 49 and 64 under the log schemes: `any_ratio` is set, so the
  26 trades of the reference's domain are priced by the wide kernel's RATIO = true instantiations."""
import dataclasses
from functools import lru_cache

import numpy as np

from adrates_amd import _native

from . import _ladder_edge_cases as E
from . import _price_edge_cases as PE
from . import _route_cases as RC
from . import _scenario_cases as SC

VD, LZ, FF, LF, SCHEMES, REQUESTS = PE.VD, PE.LZ, PE.FF, PE.LF, PE.SCHEMES, PE.REQUESTS
TILES = _native.DeviceCurve.PILLAR_TILES

DENSE_WIDE = {33: 7, 41: 7, 42: 10, 49: 10, 50: 17, 63: 17, 64: 17}       # pillars -> chunks of the packed triangle
ALL_SCHEMES_AT = (41, 49, 64)
DENSE_TILED = (65, 96, 97)
LAG_AT = (41, 49, 64)
GUARDED = ((33, 0), (49, 0), (63, 0), (65, 0), (64, TILES))               # (pillars, flags) of the guarded-buffer check
LAUNCH_SHAPES = ((41, 0), (64, 0), (65, 0))                                # ... of the launch-shape check


@dataclasses.dataclass
class WideCase(PE.PriceCase):
    flags: int = 0           # upload flags (DeviceCurve)
    route: str = "wide"      # "wide" or "tiled"
    chunks: int = 0          # `wide_chunks` of the curve's layout (whatever the route)
    lagged: tuple = ()       # rows outside the reference's domain (a payment-lag coupon); ``batch`` holds them, ``ref_batch`` not
    ref_batch: object = None

    @property
    def id(self):
        return f"{self.name}, {self.curve}{' on tiles' if self.flags else ''}, {self.interp.name}"

    @property
    def domain(self):
        """The batch the reference is built on."""
        return self.ref_batch if self.ref_batch is not None else self.batch


@lru_cache(maxsize=None)
def dense_curve(P, triple=False):
    return E.lookup_curve(E.LOOKUP_TIMES_TRIPLE if triple else SC.LOOKUP_TIMES, P=P)


def lagged_trade():
    """One coupon accruing over [0.3, 0.8], paid two days after its accrual end: a ratio node."""
    ts, te = 0.3, 0.8
    return E.make_trade(flt=[(ts, te, te + 2.0 / 365.0, te - ts)], notional=2e6, spread=0.0013, flt_sign=1.0)


@lru_cache(maxsize=None)
def lagged_lookup_book():
    """The lookup book with the lagged trade as its last row."""
    from adrates_amd.market.position.scenarios import _concat_batches
    return _concat_batches([E.lookup_book(), E.make_book([lagged_trade()])])


@lru_cache(maxsize=None)
def engine_curve(P, interp):
    return RC.engine_curve(VD, P, interp)


def chunks_of(host):
    return _native.curve_layout_host(host.times, host.dfs, host.jac, host.hess)["wide_chunks"]


@lru_cache(maxsize=None)
def cases():
    out = []
    book = E.lookup_book()
    for P, nch in DENSE_WIDE.items():
        for interp in (SCHEMES if P in ALL_SCHEMES_AT else (LZ,)):
            out.append(WideCase("lookup", interp, f"dense {P}", dense_curve(P), book, chunks=nch))
    for P in (41, 64):
        out.append(WideCase("lookup, a knot three times", LZ, f"dense {P}", dense_curve(P, True), book, chunks=DENSE_WIDE[P]))
    for interp in SCHEMES:
        h = engine_curve(40, interp)
        out.append(WideCase("knot sweep", interp, "40 pillars", h, PE.knot_sweep_book(h), chunks=7))
    for P, interp, nch in ((33, FF, 7), (64, LF, 17)):
        h = engine_curve(P, interp)
        out.append(WideCase("knot sweep", interp, f"{P} pillars", h, PE.knot_sweep_book(h), chunks=nch))
    for interp in SCHEMES:
        out.append(WideCase("row geometry", interp, "40 pillars", engine_curve(40, interp), PE.row_geometry_book(), chunks=7))
    # ---- tiles
    for interp in SCHEMES:
        h = engine_curve(65, interp)
        out.append(WideCase("knot sweep", interp, "65 pillars", h, PE.knot_sweep_book(h), route="tiled"))
    for P in DENSE_TILED:
        out.append(WideCase("lookup", LZ, f"dense {P}", dense_curve(P), book, route="tiled"))
    for P in (33, 64):
        out.append(WideCase("lookup", LZ, f"dense {P}", dense_curve(P), book, flags=TILES, route="tiled", chunks=DENSE_WIDE[P]))
    h = engine_curve(40, LZ)
    out.append(WideCase("knot sweep", LZ, "40 pillars", h, PE.knot_sweep_book(h), flags=TILES, route="tiled", chunks=7))
    # ---- the wide kernel's ratio-node instantiations on the trades of the reference's domain
    for P in LAG_AT:
        for interp in (LZ, FF):
            out.append(WideCase("lookup + a lagged trade", interp, f"dense {P}", dense_curve(P), lagged_lookup_book(), chunks=DENSE_WIDE[P],
                                lagged=(book.n_trades,), ref_batch=book))
    return out


def route(case, mask, per_trade=True, aggregate=False, n_cu=256, batch=None):
    h = case.host
    return _native.route_host(case.interp.value, h.times, h.dfs, h.jac, h.hess, case.batch if batch is None else batch, mask,
                              per_trade=per_trade, aggregate=aggregate, n_cu=n_cu, curve_flags=case.flags)


def families(case, mask, per_trade, aggregate):
    """The kernel family that prices each trade of ``case`` under a request (route.hpp, make_plan, more than 32 pillars), [n]
    of str.  An aggregate-only request with DELTA or GAMMA: the knot pass for the trades of the lite table (up to 384 coupons
    per leg; `knot_lag` for a lagged trade).  Otherwise, wide route: the wide kernel with GAMMA, and without it the lite kernel
    for the trades of its tables (`lite_lag`: a lagged trade) and the wide kernel for the rest; tiled route: every trade on the
    general kernel, once per tile pair."""
    n = case.batch.n_trades
    in_table = PE.row_class(case.batch) != "general"
    lag = np.zeros(n, dtype=bool)
    lag[list(case.lagged)] = True
    rest = case.route
    if not per_trade and mask & 6:
        return np.where(in_table, np.where(lag, "knot_lag", "knot"), rest)
    if case.route == "wide" and not mask & 4:
        return np.where(in_table, np.where(lag, "lite_lag", "lite"), rest)
    return np.full(n, rest)


def tile_launches(P, mask):
    """Launches of the tiled route per request: every tile pair with GAMMA, the diagonal with DELTA, tile (0, 0) for PV alone."""
    T = -(-P // 32)
    return T * (T + 1) // 2 if mask & 4 else (T if mask & 2 else 1)


def mirrored_pairs(case):
    """[P, P] bool: the entries (p, q) whose mirror (q, p) the code writes from the same number - wide: every off-diagonal
    pair (one entry of the packed triangle, `wide_store_map`); tiled: every pair outside the diagonal 4 x 4 blocks (an
    off-diagonal tile is written twice by its launch, an off-diagonal block of a diagonal tile comes from the registers of
    the block above the diagonal; inside a diagonal block both sides are accumulated on their own)."""
    P = case.host.jac.shape[1]
    p = np.arange(P)
    if case.route == "wide":
        return p[:, None] != p[None, :]
    return p[:, None] // 4 != p[None, :] // 4


# --------------------------------------------------------------------------------------------------------- launch shapes
def waves_per_block(case):
    """Waves per block of the case's GAMMA kernel, read off the plan: a launch of 64 trades takes 64 / waves blocks."""
    launches, _ = route(case, 7, batch=PE.cycled_book(64))
    return 64 // launches[0][3]


def launch_sizes(case, n_cu):
    """1, 2, then one trade per wave of the full grid of a device of ``n_cu`` CUs (w), w + 1 and 2 w + 1: with 2 w + 1
    trades a wave prices a second trade and one wave a third - the wide kernel's staged ladder, whose stores are issued during
    the wave's next trade and, for its last, by the final flush.  The grid is the plan's, for a book no smaller than it."""
    waves = waves_per_block(case)
    cap = route(case, 7, n_cu=n_cu, batch=PE.cycled_book(n_cu * 64))[0][0][3]
    w = cap * waves
    return (1, 2, w, w + 1, 2 * w + 1), cap, waves


def launch_case(P, flags):
    return WideCase("launch shape", LZ, f"dense {P}", dense_curve(P), PE.cycled_book(3), flags=flags,
                    route="tiled" if (flags or P > 64) else "wide", chunks=DENSE_WIDE.get(P, 0))
