"""The hand-made books of the scenario edge tests (tests/test_scenario_edges_host.py, CPU, and
tests/test_gpu_scenario_edges.py, GPU): the smallest books that reach the branches of `make_slot` / `apply_slot` / `lane_slot`
in scenario_pv.hip and credit_scenario_pv.hip that no compiled book reaches - seasoned legs, coupons that do not accrue, the
64-coupon passes, payment lags, lookups inside a coupon, amounts that cancel - with the spread side dressed by hand.

Every date that has to EQUAL another one lies on a dyadic grid (multiples of 1/8 or 1/64 of a year), so equal dates are equal
bits by construction; `check_books` asserts, trade by trade, the property each trade exists for.  A case is
``Case(name, times, dfs, batch, sub_off)``; `credit_shapes` dresses it."""
import dataclasses
from functools import lru_cache

import numpy as np

from adrates_amd.trades.compiler import TradeBatch

from . import _credit_scenario_cases as CC
from . import _scenario_cases as SC

SCHEMES = SC.SCHEMES
BP = 1e-4
STEP = 0.125                 # the long legs' period


@dataclasses.dataclass
class Case:
    name: str
    times: np.ndarray
    dfs: np.ndarray          # [S, K]
    batch: TradeBatch
    sub_off: np.ndarray      # a layout whose cuts fall inside the trades' one chunk, with an empty sub-book
    names: tuple = ()        # one per trade


# ---------------------------------------------------------------------------------------------------------------- books
def trade(name, fix=(), flt=(), notional=1e6, spread=0.0, fix_sign=1.0, flt_sign=-1.0, weight=None, fix_tau=None, z=0.0, bucket=-1):
    """``fix``: (tp, pay) rows; ``flt``: (ts, te, tp, alpha) rows; ``weight``: one per coupon (default 1.0); ``fix_tau``: the
    fixed flows' spread times (default: their payment times; the coupons' are always their payment times); ``z`` and
    ``bucket`` (taken modulo G when not -1): the trade's spread side."""
    fix = np.array(fix, dtype=np.float64).reshape(-1, 2)
    flt = np.array(flt, dtype=np.float64).reshape(-1, 4)
    weight = np.ones(flt.shape[0]) if weight is None else np.asarray(weight, dtype=np.float64)
    fix_tau = fix[:, 0].copy() if fix_tau is None else np.asarray(fix_tau, dtype=np.float64)
    assert weight.shape == (flt.shape[0],) and fix_tau.shape == (fix.shape[0],)
    return dict(name=name, fix=fix, flt=flt, notional=notional, spread=spread, fix_sign=fix_sign, flt_sign=flt_sign, weight=weight,
                fix_tau=fix_tau, z=z, bucket=bucket)


def book(trades, weighted):
    fix = np.concatenate([t["fix"] for t in trades])
    flt = np.concatenate([t["flt"] for t in trades])
    off = lambda key: np.concatenate([[0], np.cumsum([t[key].shape[0] for t in trades])]).astype(np.int64)
    col = lambda key: np.array([t[key] for t in trades], dtype=np.float64)
    weight = np.concatenate([t["weight"] for t in trades])
    assert weighted or np.all(weight == 1.0)
    return TradeBatch(off("fix"), off("flt"), fix[:, 0].copy(), fix[:, 1].copy(), flt[:, 2].copy(), flt[:, 0].copy(), flt[:, 1].copy(),
                      flt[:, 3].copy(), col("notional"), col("spread"), col("fix_sign"), col("flt_sign"), weight if weighted else None)


def abutting(first, length, m, lag=0.0):
    """``m`` coupons (ts, te, tp, alpha) whose start IS the previous coupon's end (the same float64 number), paid ``lag``
    after their accrual end."""
    edges = first + length * np.arange(m + 1)
    assert np.all(edges * 64 == np.round(edges * 64))
    return np.stack([edges[:-1], edges[1:], edges[1:] + lag, np.full(m, length)], axis=1)


def on(coupons, idx, pay):
    """Fixed flows on those coupons' payment dates."""
    return [(float(coupons[i, 2]), pay) for i in idx]


def edge_trades():
    t = []
    # ---- seasoned legs
    se = abutting(-0.5, 0.25, 6)                              # te = -0.25 (dead), 0.0 (counts), 0.25, ...
    t.append(trade("seasoned, a coupon paid at the value time", fix=on(se, range(6), 9000.0), flt=se, spread=0.004, notional=4e6,
                   z=120 * BP, bucket=0))
    s2 = abutting(-0.375, 0.25, 5)                            # te = -0.125 (dead), 0.125, ...
    t.append(trade("seasoned, live fixed flows beside dead coupons", fix=[(0.5, 7000.0), (0.125, 7000.0), (0.375 + 1.0 / 256, 7000.0)],
                   flt=s2, spread=0.001, notional=2e6, fix_sign=-1.0, flt_sign=1.0, z=-50 * BP, bucket=1))
    dm = abutting(0.25, 0.5, 5)
    dm[2, 2] = -1.0                                           # a dead coupon in the middle of a live leg
    t.append(trade("a dead coupon mid-leg", flt=dm, spread=0.002, weight=[1.0, 0.5, 3.0, -1.0, 0.0], z=800 * BP, bucket=2))
    # ---- alpha at and below zero
    a0 = abutting(0.25, 0.5, 5)
    a0[2, 3] = 0.0
    t.append(trade("alpha == 0 mid-leg", fix=on(a0, (1, 2, 4), 5000.0), flt=a0, spread=0.003, notional=2e6,
                   weight=[1.0, -0.5, 2.5, 1.0, 0.0], z=0.0, bucket=3))
    an = abutting(0.25, 0.5, 5)
    an[1, 3] = -0.25
    t.append(trade("alpha < 0 mid-leg", flt=an, spread=0.003, notional=2e6, flt_sign=1.0, weight=[0.75, -2.0, 1.0, 1.0, 1.0],
                   z=30 * BP, bucket=-1))
    ends = abutting(0.125, 0.25, 5, lag=1.0 / 64)
    ends[0, 3], ends[4, 3] = 0.0, -0.5
    t.append(trade("alpha == 0 at coupon 0, alpha < 0 at the last, a payment lag", fix=on(ends, (0, 4), 100.0), flt=ends, spread=-0.01,
                   weight=[-1.5, 1.0, 1.0, 1.0, 0.25], z=0.0, bucket=-1))
    # ---- payment dates
    lag = abutting(0.5, 0.5, 6)
    lag[[1, 2, 4], 2] += 1.0 / 64                             # tp != te on coupons 1, 2, 4; tp == te on 0, 3, 5
    lag[3, 0] = np.nextafter(lag[2, 1], np.inf)               # one ulp after the previous accrual end
    lag[5, 0] = np.nextafter(lag[4, 1], -np.inf)              # one ulp before
    fx = on(lag, (0, 1, 2), 8000.0) + [(float(lag[3, 2]) + 1.0 / 256, 8000.0), (float(lag[4, 2]), 8000.0), (float(lag[5, 2]), 8000.0)]
    t.append(trade("payment lags, ts one ulp off te, fixed flows on and off the float dates", fix=fx, flt=lag, spread=0.0005, notional=3e6,
                   fix_tau=[fx[0][0], fx[1][0] * 0.75, fx[2][0], fx[3][0], fx[4][0] * 0.75, fx[5][0]], z=200 * BP, bucket=4))
    # ---- amounts
    ann = abutting(0.25, 1.0, 3)
    t.append(trade("notional 1", fix=on(ann, (0, 1, 2), 0.043), flt=ann, notional=1.0, spread=0.001, z=-50 * BP, bucket=0))
    t.append(trade("notional 1e9", fix=on(ann, (0, 1, 2), 4.3e7), flt=ann, notional=1e9, fix_sign=-1.0, flt_sign=1.0, z=800 * BP, bucket=1))
    t.append(trade("+p and -p on one date", fix=[(1.5, 12345.0), (1.5, -12345.0)], fix_sign=-1.0, flt_sign=1.0, z=50 * BP, bucket=2))
    par = abutting(0.25, 0.25, 8)
    t.append(trade("legs that cancel: a par floater against its notional exchange", fix=[(0.25, 5e6), (2.25, -5e6)], flt=par, notional=5e6,
                   flt_sign=1.0, fix_sign=-1.0, z=0.0, bucket=-1))
    # ---- leg counts
    t.append(trade("n_fix == 0", flt=abutting(0.0, 0.25, 6), spread=0.004, flt_sign=1.0, z=10 * BP, bucket=3))
    t.append(trade("n_flt == 0", fix=[(0.75 + i, 50000.0) for i in range(4)] + [(3.75, 1e6)], z=300 * BP, bucket=-1))
    t.append(trade("no live flow", fix=[(-2.0, 5.0), (-1.0, 5.0), (0.0, 5.0)], flt=abutting(-3.0, 1.0, 2), spread=0.01, z=40 * BP, bucket=0))
    t.append(trade("no live flow, both signs -1", fix=[(-2.0, 5.0)], flt=abutting(-3.0, 1.0, 2), spread=0.01, fix_sign=-1.0, flt_sign=-1.0))
    t.append(trade("two empty legs", z=15 * BP, bucket=1))
    t.append(trade("two empty legs, both signs -1", fix_sign=-1.0, flt_sign=-1.0))
    return t


def pass_trades():
    """The 64-coupon passes of the kernel's `base` loop: coupon 64 is lane 0 of the second pass."""
    leg = lambda m: abutting(STEP, STEP, m)
    t = [trade(f"{m} abutting coupons", flt=leg(m), spread=0.0, notional=1e6, z=25 * BP, bucket=i) for i, m in enumerate((64, 65, 128))]
    t.append(trade("129 coupons against 3 fixed flows", fix=on(leg(129), (0, 64, 128), 30000.0), flt=leg(129), spread=0.001, flt_sign=1.0,
                   fix_sign=-1.0, z=-50 * BP, bucket=3))
    a = leg(65)
    a[63, 3] = 0.0
    t.append(trade("65 coupons, coupon 63 does not accrue", flt=a, spread=0.002, z=800 * BP, bucket=4))
    d = leg(65)
    d[63, 2] = -1.0
    t.append(trade("65 coupons, coupon 63 dead", flt=d, spread=0.002, z=0.0, bucket=-1))
    b = leg(66)
    b[64, 3] = -0.125
    t.append(trade("66 coupons, alpha < 0 at coupon 64", flt=b, spread=0.002, notional=2e6, z=0.0, bucket=0))
    one = leg(1)
    t.append(trade("65 fixed flows against 1 coupon", fix=[(STEP * (j + 1), 1000.0 + j) for j in range(65)], flt=one, spread=0.001,
                   fix_tau=[STEP * (j + 1) * (1.0 if j % 2 else 0.75) for j in range(65)], z=100 * BP, bucket=-1))
    return t


LOOKUP_DATES = np.array([0.5, 0.5 + 1e-11, 2.0 - 1e-11, 1.0, 1.0 + 1e-9, 1.0 - 1e-9, -0.25, -0.125, 5.0, 7.0, 40.0, 0.75, 3.25, 0.0])


def lookup_trades():
    """Coupons whose three dates run through `LOOKUP_DATES` (on a knot, within 1e-11 of one, 1e-9 beside the duplicated knot,
    before the first knot, beyond the last): one trade per coupon and the same coupons as one leg."""
    d = LOOKUP_DATES
    t = []
    legs = []
    for r in (3, 5):
        ts, te, tp = d, np.roll(d, r), np.roll(d, 2 * r + 1)
        tp = np.where(tp < 0.0, 0.125, tp)
        legs.append(np.stack([ts, te, tp, np.ones(d.size)], axis=1))
    rows = np.concatenate(legs)
    for j, row in enumerate(rows):
        t.append(trade(f"coupon {j}", fix=[(float(row[1]), 1.0)], flt=row[None, :], notional=1.0, spread=0.01, flt_sign=1.0,
                       z=(j % 5) * 40 * BP, bucket=j % 3 - 1))
    t.append(trade("all coupons in one leg", fix=[(float(v), 1.0) for v in rows[:, 2]], flt=rows, notional=1.0, spread=0.01, z=60 * BP, bucket=1))
    return t


# --------------------------------------------------------------------------------------------------------------- curves
@lru_cache(maxsize=None)
def readme_rows(S):
    """``(times, dfs [S, K])``: rows between the shocked README curves as `test_launch_shapes_bit_for_bit` builds them, the
    last two by hand: negative rates (D > 1) and rates of about 20 %."""
    times, dfs = SC.shocked_curves()
    assert times[0] == 0.0 and np.all(dfs[:, 0] == 1.0)
    mix = np.random.default_rng(65).uniform(0.0, 1.0, size=(max(S - 2, 1), dfs.shape[0]))
    rows = np.exp((mix / mix.sum(1, keepdims=True)) @ np.log(dfs))
    rows[:, 0] = 1.0
    hand = np.stack([np.exp(0.004 * times), np.exp(-(0.2 + 0.001 * np.sin(times)) * times)])
    out = np.concatenate([rows[:S - 2], hand])
    assert out.shape[0] == S and np.all(out[:, 0] == 1.0) and np.all(out[-2, 1:] > 1.0)
    return times, out


@lru_cache(maxsize=None)
def fine_rows(S=3, K=340):
    """The README grid refined log-linearly to K > 315 knots (as `_credit_scenario_cases.large_grid_call` does): the table no
    longer fits the LDS and the lanes read their rows from global memory."""
    times, dfs = readme_rows(S)
    extra = np.setdiff1d(np.linspace(0.003, times[-1] - 0.003, 2000), times)[:K - times.size]
    fine = np.sort(np.concatenate([times, extra]))
    rows = np.stack([np.exp(np.interp(fine, times, np.log(r))) for r in dfs])
    rows[:, 0] = 1.0
    assert fine.size == K > 315
    return fine, rows


def lookup_rows():
    times = SC.LOOKUP_TIMES
    dfs = SC.lookup_curves(times, S=3)
    assert times[0] == 0.0 and np.all(dfs[:, 0] == 1.0) and times[2] == times[3]
    return times, dfs


# ---------------------------------------------------------------------------------------------------------------- cases
def _case(name, curves, trades, weighted, sub_off):
    times, dfs = curves
    b = book(trades, weighted)
    sub_off = np.asarray(sub_off, dtype=np.int64)
    assert sub_off[0] == 0 and sub_off[-1] == b.n_trades and np.any(np.diff(sub_off) == 0) and b.n_trades < 64
    return Case(name, times, dfs, b, sub_off, tuple(t["name"] for t in trades))


@lru_cache(maxsize=None)
def _trades(which):
    return {"edges": edge_trades, "passes": pass_trades, "lookups": lookup_trades}[which]()


@lru_cache(maxsize=None)
def cases():
    """The rates cases; S = 65 (one past a group of 64) on the edge book, fewer rows where the legs are long."""
    edges, passes, lookups = _trades("edges"), _trades("passes"), _trades("lookups")
    return (_case("edges", readme_rows(65), edges, True, [0, 1, 1, 3, 6, len(edges)]),
            _case("passes", readme_rows(5), passes, False, [0, 2, 4, 4, 5, len(passes)]),
            _case("lookups", lookup_rows(), lookups, False, [0, 0, 9, len(lookups)]),
            _case("edges, global table", fine_rows(), edges, True, [0, 2, 2, len(edges)]))


TRADES_OF = {"edges": "edges", "passes": "passes", "lookups": "lookups", "edges, global table": "edges"}
# (label, G, discount rows: "S" or 1, spread rows: "S" or 1)
CREDIT_SHAPES = (("joint, G = 5", 5, "S", "S"), ("a shared discount row, G = 1", 1, 1, "S"), ("a shared spread row, G = 5", 5, "S", 1))


def credit_dress(case, G):
    """The case's spread side: z and the bucket as the trades carry them (the bucket modulo G), the coupons' spread times
    their payment times, the fixed flows' the trades' own."""
    trades = _trades(TRADES_OF[case.name])
    z = np.array([t["z"] for t in trades])
    bucket = np.array([t["bucket"] if t["bucket"] < 0 else t["bucket"] % G for t in trades], dtype=np.int32)
    fix_tau = np.concatenate([t["fix_tau"] for t in trades])
    return CC.Case(case.batch, z, bucket, fix_tau, case.batch.flt_tp.copy())


def credit_call(case, shape, S_cap=None):
    """``(dfs, dz, CC.Case, G)`` of one credit shape of a case; ``S_cap``: fewer scenarios (the first rows and the last two,
    which are the hand-made ones)."""
    _, G, disc, spr = shape
    dfs = case.dfs
    if S_cap is not None and dfs.shape[0] > S_cap:
        dfs = np.concatenate([dfs[:S_cap - 2], dfs[-2:]])
    S = dfs.shape[0]
    dz = CC.spread_shocks(S, G)
    # the last row, the 20 % curve, is the shared discount row; the second spread row (+300 bp on bucket 0) the shared one
    return (dfs[-1:] if disc == 1 else dfs), (dz[1:2] if spr == 1 else dz), credit_dress(case, G), G


def check_books():
    """The trades' names, checked on their arrays."""
    c = {case.name: case for case in cases()}
    b = c["edges"].batch
    name = {n: i for i, n in enumerate(c["edges"].names)}
    fix = lambda i: slice(int(b.fix_off[i]), int(b.fix_off[i + 1]))
    flt = lambda i: slice(int(b.flt_off[i]), int(b.flt_off[i + 1]))
    leg = lambda i: (b.flt_ts[flt(i)], b.flt_te[flt(i)], b.flt_tp[flt(i)], b.flt_alpha[flt(i)])
    abuts = lambda i: np.array_equal(leg(i)[0][1:], leg(i)[1][:-1])
    i = name["seasoned, a coupon paid at the value time"]
    ts, te, tp, al = leg(i)
    assert abuts(i) and tp[0] < 0.0 and tp[1] == 0.0 and np.all(tp[2:] > 0.0) and ts[1] == te[0] and b.spread[i] != 0.0
    assert np.array_equal(b.fix_tp[fix(i)], tp)                # the fixed flow at 0.0 does not count, the coupon does
    i = name["seasoned, live fixed flows beside dead coupons"]
    ts, te, tp, al = leg(i)
    assert abuts(i) and tp[0] < 0.0 and tp[1] > 0.0 and ts[1] == te[0] and b.fix_tp[fix(i)][0] > 0.0
    assert b.fix_tp[fix(i)][1] == tp[1] and 0.0 < b.fix_tp[fix(i)][2] - tp[2] < 2.0 / 365      # on the float date, a day off it
    i = name["a dead coupon mid-leg"]
    ts, te, tp, al = leg(i)
    assert abuts(i) and tp[2] < 0.0 and np.all(np.delete(tp, 2) > 0.0)
    i = name["alpha == 0 mid-leg"]
    ts, te, tp, al = leg(i)
    w = b.flt_weight[flt(i)]
    assert abuts(i) and al[2] == 0.0 and np.all(np.delete(al, 2) > 0.0) and b.spread[i] != 0.0 and w[2] not in (0.0, 1.0)
    assert np.any(w < 0.0) and np.any(w == 0.0)
    i = name["alpha < 0 mid-leg"]
    ts, te, tp, al = leg(i)
    assert abuts(i) and al[1] < 0.0 and b.flt_weight[flt(i)][1] < 0.0 and b.spread[i] != 0.0
    i = name["alpha == 0 at coupon 0, alpha < 0 at the last, a payment lag"]
    ts, te, tp, al = leg(i)
    assert abuts(i) and al[0] == 0.0 and al[-1] < 0.0 and np.all(tp != te) and b.spread[i] != 0.0 and b.flt_weight[flt(i)][0] != 1.0
    i = name["payment lags, ts one ulp off te, fixed flows on and off the float dates"]
    ts, te, tp, al = leg(i)
    assert list(tp == te) == [True, False, False, True, False, True]
    assert list(ts[1:] == te[:-1]) == [True, True, False, True, False] and ts[3] == np.nextafter(te[2], 9.0) and ts[5] == np.nextafter(te[4], 0.0)
    assert list(b.fix_tp[fix(i)] == tp) == [True, True, True, False, True, True]
    i, j = name["notional 1"], name["notional 1e9"]
    assert b.notional[i] == 1.0 and b.notional[j] == 1e9 and j == i + 1
    i = name["+p and -p on one date"]
    assert b.fix_tp[fix(i)][0] == b.fix_tp[fix(i)][1] and b.fix_pay[fix(i)][0] == -b.fix_pay[fix(i)][1] != 0.0
    i = name["legs that cancel: a par floater against its notional exchange"]
    ts, te, tp, al = leg(i)
    assert abuts(i) and np.array_equal(tp, te) and list(b.fix_tp[fix(i)]) == [ts[0], te[-1]] and b.spread[i] == 0.0
    assert list(b.fix_sign[i] * b.fix_pay[fix(i)]) == [-b.flt_sign[i] * b.notional[i], b.flt_sign[i] * b.notional[i]]
    assert b.flt_tp[flt(name["n_fix == 0"])].size == 6 and b.fix_tp[fix(name["n_fix == 0"])].size == 0
    assert b.flt_tp[flt(name["n_flt == 0"])].size == 0 and b.fix_tp[fix(name["n_flt == 0"])].size == 5
    for n in ("no live flow", "no live flow, both signs -1"):
        i = name[n]
        assert b.fix_tp[fix(i)].size and np.all(b.fix_tp[fix(i)] <= 0.0) and leg(i)[2].size and np.all(leg(i)[2] < 0.0)
    for n in ("two empty legs", "two empty legs, both signs -1"):
        assert b.fix_tp[fix(name[n])].size == 0 and b.flt_tp[flt(name[n])].size == 0
    assert b.fix_sign[name["two empty legs, both signs -1"]] == b.flt_sign[name["no live flow, both signs -1"]] == -1.0
    # the fixed flow and the coupon of one index on one date with equal and with different spread times
    i = name["payment lags, ts one ulp off te, fixed flows on and off the float dates"]
    tau = credit_dress(c["edges"], 5).fix_tau[fix(i)]
    assert list(tau == b.fix_tp[fix(i)]) == [True, False, True, True, False, True]
    # the passes
    p = c["passes"].batch
    counts = list(zip(np.diff(p.fix_off), np.diff(p.flt_off)))
    assert counts == [(0, 64), (0, 65), (0, 128), (3, 129), (0, 65), (0, 65), (0, 66), (65, 1)]
    for i in range(7):
        sl = slice(int(p.flt_off[i]), int(p.flt_off[i + 1]))
        assert np.array_equal(p.flt_ts[sl][1:], p.flt_te[sl][:-1])
        if i not in (5,):
            assert np.all(p.flt_tp[sl] == p.flt_te[sl])
    al, tp = p.flt_alpha[int(p.flt_off[4]):int(p.flt_off[5])], p.flt_tp[int(p.flt_off[5]):int(p.flt_off[6])]
    assert al[63] == 0.0 and np.all(np.delete(al, 63) > 0.0) and tp[63] < 0.0 and np.all(np.delete(tp, 63) > 0.0)
    assert p.flt_alpha[int(p.flt_off[6]) + 64] < 0.0 and p.flt_weight is None and b.flt_weight is not None
    assert c["edges"].dfs.shape[0] == 65 and c["edges, global table"].times.size > 315
    flows = sum(int(x.batch.fix_off[-1] + x.batch.flt_off[-1]) for x in cases()[:3])
    assert flows < 1000, flows
    # the lookups: what `_lookup_plan` decides on the dates
    from oracle.mp_oracle import _lookup_plan
    x = c["lookups"].times
    kinds = [_lookup_plan(x, t, 1) for t in LOOKUP_DATES]
    assert kinds[0] == kinds[1] == ("snap", 1) and kinds[2] == ("snap", 4) and kinds[3] == ("snap", 2)
    assert kinds[4][:3] == ("interp", 3, 4) and kinds[5][:3] == ("interp", 1, 2) and kinds[6] == kinds[7] == ("flat", 0)
    assert kinds[8] == ("snap", 5) and kinds[9] == kinds[10] == ("flat", 5) and kinds[13] == ("snap", 0)
