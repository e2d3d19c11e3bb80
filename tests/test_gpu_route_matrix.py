"""The launch-plan cross product of test_route_table.py priced on the GPU: for every mix of trade classes, curve and scheme,
every request mask 1-7 and every output form {per trade, per trade + aggregate, aggregate only}, the HIP kernels against
the C oracle (oracle/port.c) at the project's 1e-10.  Each cell is priced twice and must repeat its bits (the one exception:
a plan with the knot-lag pass under a GAMMA request, whose overflow matrix takes atomic adds); the aggregate-only form must
agree with the per-trade + aggregate form of the same cell.  The last test checks that the matrix ran every kernel family and
every (family, scheme) pair the CPU table produces, and prints one coverage line."""
import ctypes as C
import time

import numpy as np
import pytest

from adrates_amd import _native
from adrates_amd.utils.error import LibError
from oracle import port

from . import _fixtures as F
from . import _route_cases as R
from ._parity import assert_batch_parity

pytestmark = pytest.mark.gpu

FORMS = ((True, False), (True, True), (False, True))          # (per_trade, aggregate)
PARAMS = [pytest.param(label, interp, marks=[pytest.mark.slow] if label in R.SLOW else [], id=f"{label}-{interp.name}")
          for label in R.CURVES for interp in R.SCHEMES]
_SEEN = dict(params=set(), cells=0, families=set(), pairs=set(), masks=set(), forms=set(), tiles=set(), repeats_1e13=0,
             oracle_s=0.0, t0=None)


def _price_again(ctx, dc, dt, mask, per_trade, aggregate):
    """adr_price with EVERY per-trade buffer offered (NaN-filled) whatever the mask: returns the buffers, for the bitwise
    repeat and for the check that the library leaves the outputs the mask does not ask for untouched."""
    n, P = dt.n_trades, dc.n_pillars
    bufs = dict(pv=np.full(n, np.nan), delta=np.full((n, P), np.nan), gamma=np.full((n, P, P), np.nan)) if per_trade else {}
    agg = np.full(1 + P + P * P, np.nan) if aggregate else None
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    rc = _native.load().adr_price(ctx._h, dc._h, dt._h, mask, p(bufs.get("pv")), p(bufs.get("delta")), p(bufs.get("gamma")), p(agg))
    assert rc == 0, _native.load().adr_last_error()
    if agg is not None:
        bufs.update(agg_pv=agg[0], agg_delta=agg[1:1 + P], agg_gamma=agg[1 + P:].reshape(P, P))
    return bufs


def _check_book(got, ref, mask, where):
    """include/adrates.h (adr_price): agg[0] is the book's PV whatever the mask; the delta block holds the book's delta when
    DELTA or GAMMA is requested, the gamma block its gamma with GAMMA; blocks not asked for are zeros.  Tolerances of
    test_gpu_many_pillars.py (test_more_than_64_pillars_on_tiles_vs_c_oracle)."""
    assert np.allclose(got["agg_pv"], ref["pv"].sum(), rtol=1e-10, atol=1e-3), where
    if mask & 6:
        assert np.allclose(got["agg_delta"], ref["delta"].sum(0), rtol=1e-10, atol=1e-6), where
    else:
        assert np.all(got["agg_delta"] == 0.0), where
    if mask & 4:
        assert np.allclose(got["agg_gamma"], ref["gamma"].sum(0), rtol=1e-10, atol=1e-9), where
    else:
        assert np.all(got["agg_gamma"] == 0.0), where


def _rel(a, b, terms=None):
    """max |a - b| relative to the largest entry of b - or, for sums, to the largest sum of the terms' magnitudes (a near-par
    book's PV total is a small difference of large trade PVs; its rounding scales with the trades')."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = float(np.max(np.abs(b)))
    if terms is not None:
        scale = max(scale, float(np.max(np.abs(np.asarray(terms)).sum(0))))
    return float(np.max(np.abs(a - b)) / max(scale, 1e-300))


@pytest.mark.parametrize("label,interp", PARAMS)
def test_route_matrix_vs_c_oracle(gpu_ctx, label, interp):
    if _SEEN["t0"] is None:
        _SEEN["t0"] = time.perf_counter()
    vd = F.README_VALUE_DT
    host = R.engine_curve(vd, label, interp)
    P = host.n_pillars
    for flags in R.curve_flags(label):
        dc = _native.DeviceCurve(gpu_ctx, interp.value, host.times, host.dfs, host.jac, host.hess, flags=flags)
        for classes in R.MIXES:
            b, labels = R.batch(vd, classes)
            t0 = time.perf_counter()
            ref = port.price(interp.value, host.times, host.dfs, host.jac, host.hess, b)          # mask 7, once per upload
            _SEEN["oracle_s"] += time.perf_counter() - t0
            dt = _native.DeviceTrades(gpu_ctx, b)
            for mask in range(1, 8):
                both = None
                for per_trade, aggregate in FORMS:
                    where = (label, flags, interp.name, classes, mask, per_trade, aggregate)
                    launches, cover = _native.route_host(interp.value, host.times, host.dfs, host.jac, host.hess, b, mask,
                                                         per_trade=per_trade, aggregate=aggregate, curve_flags=flags)
                    assert np.all(cover == 1), where
                    fams = {f for f, *_ in launches}
                    got = _native.price(gpu_ctx, dc, dt, want_value=bool(mask & 1), want_delta=bool(mask & 2),
                                        want_gamma=bool(mask & 4), per_trade=per_trade, aggregate=aggregate)
                    wanted = {k for k, bit in (("pv", 1), ("delta", 2), ("gamma", 4)) if per_trade and mask & bit}
                    assert set(got) == wanted | ({"agg_pv", "agg_delta", "agg_gamma"} if aggregate else set()), where
                    if wanted:
                        assert_batch_parity(got, {k: ref[k] for k in wanted}, b.notional)
                    if aggregate:
                        _check_book(got, ref, mask, where)
                    # the outputs the mask does not ask for stay untouched; what it asks for repeats bit for bit
                    again = _price_again(gpu_ctx, dc, dt, mask, per_trade, aggregate)
                    for k in ("pv", "delta", "gamma"):
                        if per_trade and k not in wanted:
                            assert np.all(np.isnan(again[k])), (where, k)
                    atomics = "knot_lag" in fams and mask & 4
                    for k, v in got.items():
                        if atomics:
                            # the knot-lag overflow matrix sums with atomic adds (kernels_lite.hip:254, unsafeAtomicAdd):
                            # its order, and so the last bits of the gamma ladder, varies from run to run
                            _SEEN["repeats_1e13"] += 1
                            assert _rel(again[k], v) <= 1e-13, (where, k)
                        else:
                            assert np.array_equal(np.asarray(again[k]), np.asarray(v)), (where, k)
                    # the aggregate-only form agrees with the per-trade + aggregate form of the same cell
                    if per_trade and aggregate:
                        both = got
                    elif not per_trade:
                        for k in ("agg_pv", "agg_delta", "agg_gamma"):
                            e = _rel(got[k], both[k], ref[k[4:]])
                            assert e <= 1e-12, (where, k, e)
                    _SEEN["cells"] += 1
                    _SEEN["masks"].add(mask)
                    _SEEN["forms"].add((per_trade, aggregate))
                    _SEEN["families"] |= fams
                    _SEEN["pairs"] |= {(f, interp.name) for f in fams}
                    n_tiles = sum(1 for f, *_ in launches if f == "tiled")
                    if n_tiles and mask & 4:
                        _SEEN["tiles"].add(-(-P // 32))
            dt.close()
        dc.close()
    _SEEN["params"].add((label, interp.name))


def test_upload_refuses_the_curve_just_past_the_lds_limit(gpu_ctx):
    """One pillar more than the largest weekly-short-end curve: its knot tables exceed the 160 KiB LDS the upload allows
    (ADR_ERR_UNSUPPORTED).  The same context then prices the largest curve that fits against the oracle."""
    from adrates_amd.market.curves.curve_tables import build_engine_curve
    from .test_gpu_many_pillars import weekly_pillar_quotes
    vd = F.README_VALUE_DT
    px, tenors = weekly_pillar_quotes(R.REALISTIC_MAX + 1)
    curve = F.gbp_model(vd, px=px, tenors=tenors).curves.GBP_OIS_SONIA
    past = build_engine_curve(curve.swap_rates, curve.swap_times, curve.year_fracs)
    assert R.curve_sizes(past)[3] > R.LDS_BUDGET
    with pytest.raises(LibError, match=r"\(-2\).*LDS"):
        _native.DeviceCurve(gpu_ctx, 4, past.times, past.dfs, past.jac, past.hess)
    del past
    host = R.engine_curve(vd, R.REALISTIC_MAX)
    dc = _native.DeviceCurve(gpu_ctx, 4, host.times, host.dfs, host.jac, host.hess)
    b, _ = R.batch(vd, R.ALL)
    dt = _native.DeviceTrades(gpu_ctx, b)
    ref = port.price(4, host.times, host.dfs, host.jac, host.hess, b)
    got = _native.price(gpu_ctx, dc, dt, aggregate=True)
    assert_batch_parity(got, ref, b.notional)
    _check_book(got, ref, 7, "the largest curve the upload takes")
    dt.close()
    dc.close()


def test_route_matrix_coverage():
    """After the whole matrix: every kernel family ran, every (family, scheme) pair of the CPU table, masks 1-7, the three
    output forms, and gamma on 2, 3, 4, 5 and 8 tiles (36 tile pairs at 256 pillars)."""
    expected = {(str(label), interp.name) for label in R.CURVES for interp in R.SCHEMES}
    ran = {(str(label), s) for label, s in _SEEN["params"]}
    if ran != expected:
        pytest.skip(f"only {len(ran)} of the {len(expected)} (curve, scheme) cases ran in this session")
    wall = time.perf_counter() - _SEEN["t0"]
    print(f"\nroute matrix: {_SEEN['cells']} cells, {len(_SEEN['families'])} families {sorted(_SEEN['families'])}, "
          f"{len(_SEEN['pairs'])} (family, scheme) pairs, masks {sorted(_SEEN['masks'])}, {len(_SEEN['forms'])} output forms, "
          f"tiles {sorted(_SEEN['tiles'])}, {_SEEN['repeats_1e13']} outputs held to 1e-13 (knot-lag atomics), "
          f"oracle {_SEEN['oracle_s']:.1f} s, wall {wall:.1f} s")
    assert _SEEN["families"] == set(_native.ROUTE_FAMILIES), _SEEN["families"]
    assert _SEEN["pairs"] == R.FAMILY_SCHEMES, _SEEN["pairs"] ^ R.FAMILY_SCHEMES
    assert _SEEN["masks"] == set(range(1, 8)) and _SEEN["forms"] == set(FORMS)
    assert _SEEN["tiles"] == {2, 3, 4, 5, 8}         # 40 on tiles, 65 / 96, 128, 129 / 155, 256 pillars
