"""Books, spreads, buckets and scenario pairs shared by the credit scenario-revaluation tests
(tests/test_credit_scenarios_host.py, CPU, and tests/test_gpu_credit_scenarios.py, GPU), and the reference both compare
with: the spread factor exp(-x tau) does not depend on the curve, so the reference is the existing C oracle
(`_scenario_cases.oracle_pv`) called per scenario on a batch rescaled on the host - ``fix_pay`` multiplied by the factor,
the float coupons taking it through ``flt_weight``."""
import ctypes as C
import dataclasses

import numpy as np

from adrates_amd import _native

from . import _scenario_cases as SC

BP = 1e-4
BUCKET_COUNTS = (1, 5, 32)


@dataclasses.dataclass
class Case:
    batch: object
    z: np.ndarray            # [n]
    bucket: np.ndarray       # [n] int32
    fix_tau: np.ndarray
    flt_tau: np.ndarray


def dress(batch, G, seed):
    """Spreads, buckets and spread times for a compiled batch: z from -50 bp to +800 bp, buckets 0 .. G - 1 with about a
    fifth of the trades unbucketed, about a fifth with no spread at all (z = 0, unbucketed: the kernel's plain path);
    spread times tau = t for the float coupons and, per trade, t or t * 365 / 365.25 for the fixed flows (the second
    keeps a fixed flow paid with a float coupon from sharing its factor)."""
    rng = np.random.default_rng(seed)
    n = batch.n_trades
    z = rng.uniform(-50 * BP, 800 * BP, n)
    bucket = rng.integers(0, G, n).astype(np.int32)
    z[0], bucket[0] = 800 * BP, G - 1                      # the ends of both ranges are always there
    if n > 1:
        z[1], bucket[1] = -50 * BP, 0
    kind = rng.random(n)
    kind[:2] = 1.0
    bucket[kind < 0.4] = -1
    z[kind < 0.2] = 0.0
    z[(kind >= 0.9) & (kind < 1.0)] = 0.0                  # z = 0 in a bucket: the shock alone
    scale = np.where(rng.random(n) < 0.5, 1.0, 365.0 / 365.25)
    fix_tau = batch.fix_tp * np.repeat(scale, np.diff(batch.fix_off))
    return Case(batch, z, bucket, fix_tau, batch.flt_tp.copy())


def cases(G):
    """name -> Case: the books of `_scenario_cases.books()` dressed with ``G`` buckets."""
    return {name: dress(b, G, 100 + 7 * i + G) for i, (name, b) in enumerate(SC.books().items())}


def spread_shocks(S, G, seed=17):
    """``[S, G]``: shocks within +-300 bp, both ends present, the first row zero."""
    rng = np.random.default_rng(seed + G)
    dz = rng.uniform(-300 * BP, 300 * BP, (S, G))
    dz[0] = 0.0
    dz[1 % S, 0] = 300 * BP
    dz[2 % S, G - 1] = -300 * BP
    return dz


def spreads_of(case, dz):
    """``x [S, n]`` = z + dz[s][bucket] (no shock for bucket -1), as the kernel forms it."""
    dz = np.atleast_2d(dz)
    shock = np.where(case.bucket[None, :] >= 0, dz[:, np.maximum(case.bucket, 0)], 0.0) if dz.shape[1] else 0.0
    return case.z[None, :] + shock


def rescaled(case, x):
    """The batch of one scenario with exp(-x tau) folded into the amounts (``x [n]``)."""
    b = case.batch
    xf = np.repeat(x, np.diff(b.fix_off))
    xl = np.repeat(x, np.diff(b.flt_off))
    w = np.ones(b.flt_tp.shape[0]) if b.flt_weight is None else b.flt_weight
    return dataclasses.replace(b, fix_pay=b.fix_pay * np.exp(-xf * case.fix_tau), flt_weight=w * np.exp(-xl * case.flt_tau))


def oracle_pv(method, times, dfs, dz, case):
    """``[S, n]``: the C oracle on the rescaled batch, one call per scenario; ``dfs`` and ``dz`` broadcast."""
    dfs, x = np.atleast_2d(dfs), spreads_of(case, dz)
    S = max(dfs.shape[0], x.shape[0])
    return np.stack([SC.oracle_pv(method, times, dfs[s % dfs.shape[0]], rescaled(case, x[s % x.shape[0]]))[0] for s in range(S)])


def host_pv(method, times, dfs, dz, case, per_trade=True, **kw):
    return _native.credit_scenario_pv_host(method, times, dfs, dz, case.batch, case.z, case.bucket, case.fix_tau, case.flt_tau,
                                           per_trade=per_trade, **kw)


def device_pv(ctx, method, times, dfs, dz, case, per_trade=True):
    dev = _native.DeviceTrades(ctx, case.batch)
    try:
        return _native.credit_scenario_pv(ctx, method, times, dfs, dz, dev, case.z, case.bucket, case.fix_tau, case.flt_tau,
                                          per_trade=per_trade)
    finally:
        dev.close()


def raw_host_call(method, times, S_disc, dfs, G, S_spr, dz, S, case):
    """adr_credit_scenario_pv_host with the counts as given (the Python wrapper derives them): the return code."""
    b = case.batch
    f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    p = lambda a, t=C.POINTER(C.c_double): None if a is None else a.ctypes.data_as(t)
    i64 = C.POINTER(C.c_int64)
    arrs = [f(a) for a in (times, dfs, dz, b.fix_tp, b.fix_pay, b.flt_tp, b.flt_ts, b.flt_te, b.flt_alpha, b.flt_weight,
                           b.notional, b.spread, b.fix_sign, b.flt_sign, case.z, case.fix_tau, case.flt_tau)]
    t, d, z, ftp, fpay, ltp, lts, lte, lal, lw, nn, sp, fs, ls, zz, ftau, ltau = arrs
    fo, lo = np.ascontiguousarray(b.fix_off, dtype=np.int64), np.ascontiguousarray(b.flt_off, dtype=np.int64)
    bucket = np.ascontiguousarray(case.bucket, dtype=np.int32)
    book = np.empty(S)
    return _native.load().adr_credit_scenario_pv_host(
        int(method), t.size, p(t), S_disc, p(d), G, S_spr, p(z), S, b.n_trades, p(fo, i64), p(lo, i64), p(ftp), p(fpay), p(ltp),
        p(lts), p(lte), p(lal), p(lw), p(nn), p(sp), p(fs), p(ls), p(zz), p(bucket, C.POINTER(C.c_int32)), p(ftau), p(ltau), None,
        p(book), 1)


def refusal_inputs(G=3):
    """A small valid call (payment-lag book, 4 scenarios) and the list of ``(what, field, mutate)`` that each turn one
    input into something the host-array entries must refuse."""
    times, dfs = SC.shocked_curves()
    case = dress(SC.lag_book(40, seed=3), G, 5)
    dz = spread_shocks(4, G)

    def set_at(name, idx, value):
        def mutate(kw):
            a = np.array(kw[name], dtype=np.float64 if name != "bucket" else np.int32)
            a.reshape(-1)[idx] = value
            kw[name] = a
        return mutate
    bad = [("non-finite z", set_at("z", 3, np.nan)), ("infinite z", set_at("z", 0, np.inf)),
           ("non-finite dz", set_at("dz", 5, np.nan)), ("non-finite fixed tau", set_at("fix_tau", 2, np.inf)),
           ("non-finite float tau", set_at("flt_tau", 7, np.nan)), ("bucket below -1", set_at("bucket", 4, -2)),
           ("bucket at G", set_at("bucket", 6, G)), ("zero discount factor", set_at("dfs", 9, 0.0)),
           ("negative discount factor", set_at("dfs", 300, -0.5)), ("non-finite discount factor", set_at("dfs", 11, np.nan))]
    return times, dfs[:4], dz, case, bad


def large_grid_call(S=8):
    """The README curve's knots refined to K = 856 (log-linear in between), S scenario rows, the 50-bond book, 32 buckets."""
    times, dfs = SC.shocked_curves()
    extra = np.setdiff1d(np.linspace(0.003, times[-1] - 0.003, 2000), times)[:856 - times.size]
    fine = np.sort(np.concatenate([times, extra]))
    rows = np.stack([np.exp(np.interp(fine, times, np.log(r))) for r in dfs[:S]])
    case = dress(SC.books()["50 bonds"], 32, 77)
    return fine, rows, spread_shocks(S, 32), case


def numpy_df(method, times, row, t):
    """D(t) by the oracle's Python restatement of simple_interpolate."""
    from oracle import cavour_oracle as O
    return np.asarray(O.simple_interpolate(np.asarray(t, dtype=np.float64), times, row, method), dtype=np.float64).reshape(-1)
