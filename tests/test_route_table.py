"""The launch plan of adr_price_dev (adrates_amd/csrc/route.hpp), enumerated on the CPU: for the cross product of trade
classes {plain, long, very long, payment lag, long payment lag, very long payment lag, weighted, edges (exact coupon counts on
both sides of every table boundary)} x pillar counts {17, 31, 32, 33, 40, 40 on tiles, 63, 64, 65, 96, 128, 129, 155 (the
largest realistic curve the upload takes), 256 (eight tiles)} x the three interpolation schemes x requests {V, VD, VDG} x
outputs {per trade, per trade + aggregate, aggregate only}, every trade of a mixed batch is priced by exactly one launch.  The
reference has a single route (Engine._compute_ois_natural, cavour/market/position/engine.py:153-215); here eleven kernel
families share the work, and every new route so far had cost a correctness fix in the routing - this test walks the table
without a GPU.  The cases live in _route_cases.py; test_gpu_route_matrix.py prices the same table on the GPU."""
import numpy as np
import pytest

from adrates_amd import _native

from . import _fixtures as F
from . import _route_cases as R
from ._route_cases import ALL
from ._route_cases import batch as _batch


def _curves(vd):
    return R.curves(vd, with_hessian=False)       # (route_host needs them only with GAMMA)


def test_every_trade_is_priced_exactly_once_over_the_route_table():
    vd = F.README_VALUE_DT
    batches = [(classes, *_batch(vd, classes)) for classes in R.MIXES]
    seen, pairs = set(), set()
    for P in R.CURVES:
        host = R.engine_curve(vd, P)             # (one at a time: the second derivatives of the 155-pillar curve are 390 MB)
        for classes, batch, labels in batches:
            for flags in R.curve_flags(P):
                for interp in R.SCHEMES:
                    for mask in range(1, 8):
                        for per_trade, aggregate in ((True, False), (True, True), (False, True)):
                            launches, cover = _native.route_host(interp.value, host.times, host.dfs, host.jac, host.hess, batch, mask,
                                                                 per_trade=per_trade, aggregate=aggregate, curve_flags=flags)
                            bad = [(labels[i], int(c)) for i, c in enumerate(cover) if c != 1]
                            assert not bad, (classes, P, flags, interp.name, mask, per_trade, aggregate, launches, bad)
                            seen.update(f for f, *_ in launches)
                            pairs.update((f, interp.name) for f, *_ in launches)
    assert seen == set(_native.ROUTE_FAMILIES), seen          # the table exercised every kernel family
    assert pairs == R.FAMILY_SCHEMES, pairs ^ R.FAMILY_SCHEMES   # ... and the (family, scheme) pairs the GPU matrix must run


def test_the_plans_of_the_reported_configurations():
    """The routes DESIGN.md section 5 states for the benchmark configurations."""
    vd = F.README_VALUE_DT
    host = R.engine_curve(vd, 32)
    plain, _ = _batch(vd, ("plain",))
    fam = lambda launches: [(f, s) for f, s, *_ in launches]
    r = lambda b, mask, **kw: fam(_native.route_host(4, host.times, host.dfs, host.jac, host.hess, b, mask, **kw)[0])
    assert r(plain, 7, aggregate=True) == [("fast", "rows")]                       # BASELINE configs[2]: the bench kernel
    assert r(plain, 3, aggregate=True) == [("lite", "lite")]                       # configs[1]
    assert r(plain, 7, per_trade=False, aggregate=True) == [("knot", "lite")]      # Portfolio.compute: the ladder alone
    lag, _ = _batch(vd, ("lag",))
    assert r(lag, 7) == [("fast_lag", "lagged")] and r(lag, 3) == [("lite_lag", "lite_lag")]
    assert fam(_native.route_host(2, host.times, host.dfs, host.jac, host.hess, lag, 7)[0]) == [("general", "general")]   # LINEAR_FWD_RATES
    mixed, _ = _batch(vd, ALL)
    assert r(mixed, 7, per_trade=False, aggregate=True)[-2:] == [("knot", "lite"), ("knot_lag", "lite_lag")]    # the projections add last
    assert r(lag, 7, per_trade=False, aggregate=True) == [("knot_lag", "lite_lag")]


def test_edge_trades_land_in_the_sets_their_coupon_counts_imply():
    """Each trade of the `edges` class alone, on the 32-pillar curve (packed layout, even pillar count): its coupon count
    decides its table (route.hpp, classify_trades / make_plan) on both sides of every boundary."""
    from adrates_amd.trades.compiler import TradeBatch
    vd = F.README_VALUE_DT
    host = R.engine_curve(vd, 32)
    edges, labels, counts = R.edges_batch()
    gamma_route = {"plain": lambda c: ("fast", "rows") if c <= 32 else ("fast_chained", "chained") if c <= 384 else ("general", "general"),
                   "lag": lambda c: ("fast_lag", "lagged") if c <= 32 else ("fast_lag_chained", "lagged_chained") if c <= 128
                   else ("general", "general")}      # (alone in its batch: no payment-lag rows, so the whole general list)
    gamma_route["weighted"] = gamma_route["lag"]
    delta_route = {"plain": lambda c: ("lite", "lite") if c <= 384 else ("general", "general"),
                   "lag": lambda c: ("lite_lag", "lite_lag") if c <= 390 else ("general", "general")}
    delta_route["weighted"] = delta_route["lag"]
    for t, (label, c) in enumerate(zip(labels, counts)):
        one = edges.slice(t, t + 1)
        assert isinstance(one, TradeBatch) and one.flt_off[1] == c
        kind = label.split("-")[0]
        for mask, expect in ((7, gamma_route[kind](c)), (3, delta_route[kind](c))):
            launches, cover = _native.route_host(4, host.times, host.dfs, host.jac, host.hess, one, mask)
            assert [(f, s) for f, s, *_ in launches] == [expect], (label, mask, launches)
            assert list(cover) == [1]


def test_curve_classes_and_the_upload_lds_limit():
    """The curves of the table have the pillar and knot counts _route_cases.CURVES records (checked in engine_curve), the
    tile counts their pillar counts imply, and the LDS the upload checks: the largest weekly-short-end curve fits, one
    pillar more does not; the 256-pillar curve of single-period pillars fits."""
    from adrates_amd.market.curves.curve_tables import build_engine_curve
    from .test_gpu_many_pillars import weekly_pillar_quotes
    vd = F.README_VALUE_DT
    curves = _curves(vd)
    for label, host in curves.items():
        P, K, Kc, lds = R.curve_sizes(host)
        assert lds <= R.LDS_BUDGET, label
    assert R.CURVES[R.REALISTIC_MAX][0] == R.REALISTIC_MAX
    px, tenors = weekly_pillar_quotes(R.REALISTIC_MAX + 1)
    c = F.gbp_model(vd, px=px, tenors=tenors).curves.GBP_OIS_SONIA
    past = build_engine_curve(c.swap_rates, c.swap_times, c.year_fracs, with_hessian=False)
    assert R.curve_sizes(past)[3] > R.LDS_BUDGET
    # tile launches: T diagonal tiles for delta, T (T + 1) / 2 tile pairs for gamma, T = ceil(P / 32)
    plain, _ = _batch(vd, ("plain",))
    for label in (65, 128, 129, 155, 256):
        T = -(-label // 32)
        host = curves[label]
        launches, _ = _native.route_host(4, host.times, host.dfs, host.jac, None, plain, 3)
        assert [f for f, *_ in launches] == ["tiled"] * T, label                     # delta: the diagonal tiles
        host = R.engine_curve(vd, label)
        launches, _ = _native.route_host(4, host.times, host.dfs, host.jac, host.hess, plain, 7)
        assert [f for f, *_ in launches] == ["tiled"] * (T * (T + 1) // 2), label
    assert -(-curves[256].n_pillars // 32) == 8
