"""The hand-made books of the sub-book ladder edge tests (tests/test_ladder_edges_host.py, CPU, and
tests/test_gpu_ladder_edges.py, GPU): the smallest shapes at which the lookup rule, the folding rules, the owner search and the
projection's loops can still go wrong.  Every case is ``Case(name, host curve, batch, layouts)`` with ``layouts`` a dict
name -> sub_off; a credit case adds the spread side and G; an inflation case (`YoYCase`) holds a raw YoY book, the
inflation curve and the request."""
import dataclasses
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

from adrates_amd import _native
from adrates_amd.market.curves.curve_tables import build_engine_curve
from adrates_amd.market.position.scenarios import _concat_batches
from adrates_amd.trades import synthetic
from adrates_amd.trades.compiler import TradeBatch

from . import _credit_ladder_cases as CL
from . import _fixtures as F
from . import _ladder_reference as R
from . import _scenario_cases as SC
from . import _sub_book_ladder_cases as L
from . import _yoy_cases as YC
from . import _yoy_ladder_cases as Y

VD = L.VD
SCHEMES = L.SCHEMES
BP = 1e-4
# LOOKUP_TIMES has a knot twice (both copies are kept: the second is a segment's lower end); with a knot three times the
# middle copy is unreachable and the compact grid is shorter than the raw one (K = 7, Kc = 6).
LOOKUP_TIMES_TRIPLE = np.array([0.0, 0.5, 1.0, 1.0, 1.0, 2.0, 5.0])


@dataclasses.dataclass
class Case:
    name: str
    host: object             # times, dfs, jac, hess
    batch: TradeBatch
    layouts: dict            # name -> sub_off


# ---------------------------------------------------------------------------------------------------------------- books
def make_trade(fix=(), flt=(), notional=1e6, spread=0.0, fix_sign=1.0, flt_sign=-1.0):
    """``fix``: (tp, pay) rows; ``flt``: (ts, te, tp, alpha) rows."""
    return dict(fix=np.array(fix, dtype=np.float64).reshape(-1, 2), flt=np.array(flt, dtype=np.float64).reshape(-1, 4),
                notional=notional, spread=spread, fix_sign=fix_sign, flt_sign=flt_sign)


def make_book(trades):
    fix = np.concatenate([t["fix"] for t in trades])
    flt = np.concatenate([t["flt"] for t in trades])
    off = lambda key: np.concatenate([[0], np.cumsum([t[key].shape[0] for t in trades])]).astype(np.int64)
    col = lambda key: np.array([t[key] for t in trades], dtype=np.float64)
    return TradeBatch(off("fix"), off("flt"), fix[:, 0].copy(), fix[:, 1].copy(), flt[:, 2].copy(), flt[:, 0].copy(), flt[:, 1].copy(),
                      flt[:, 3].copy(), col("notional"), col("spread"), col("fix_sign"), col("flt_sign"))


def chain(starts, length, alpha=None, tp=None):
    """Coupons (ts, te, tp, alpha) starting at ``starts``, each ``length`` long, paid on their accrual end."""
    starts = np.asarray(starts, dtype=np.float64)
    ends = starts + length
    alpha = np.full(starts.size, length) if alpha is None else np.asarray(alpha, dtype=np.float64)
    return np.stack([starts, ends, ends if tp is None else tp, alpha], axis=1)


def abutting(first, length, m):
    """``m`` coupons whose start IS the previous coupon's end (the same float64 number)."""
    edges = first + length * np.arange(m + 1)
    return np.stack([edges[:-1], edges[1:], edges[1:], np.full(m, length)], axis=1)


def folding_trades():
    """The folding book, one trade per branch of `float_nodes` / `fixed_node`."""
    semi = abutting(0.3, 0.5, 4)
    annual_fix = lambda coupon, m, first=1.3: [(first + i, coupon) for i in range(m)]
    on = lambda coupons, idx, pay: [(float(coupons[i, 2]), pay) for i in idx]       # fixed flows on those coupons' payment dates
    t = []
    # ---- coupon chains
    t.append(make_trade(flt=semi, notional=3e6))                               # 0 chained, spread 0: the interior amount is exactly 0, node off
    t.append(make_trade(flt=semi, notional=3e6, spread=0.002))                 # 1 chained, spread != 0: interior nodes carry N s alpha
    t.append(make_trade(flt=chain([0.3, 0.85, 1.4], 0.5), spread=0.001))       # 2 accrual periods that do not abut: every start its own node
    # ---- accrual and value-time edges
    a0 = abutting(0.2, 0.5, 4)
    a0[1, 3] = 0.0
    t.append(make_trade(flt=a0, spread=0.003, notional=2e6))                   # 3 alpha == 0 mid-leg: no forward, no start, amount 0 (+ the next start)
    an = abutting(0.2, 0.5, 4)
    an[2, 3] = -0.25
    t.append(make_trade(flt=an, spread=0.003, notional=2e6, flt_sign=1.0))     # 4 alpha < 0 mid-leg: only N s alpha, negative
    z0 = abutting(-0.25, 0.25, 3)
    t.append(make_trade(fix=[(0.0, 7000.0), (0.25, 7000.0), (0.5, 7000.0)], flt=z0, spread=0.001))
    #                                                                            5 tp == 0.0 on a float coupon (counts, its start before the first
    #                                                                              knot) and on the fixed flow of the same index (does not count)
    se = abutting(-0.6, 0.5, 4)
    t.append(make_trade(fix=[(-0.1, 9000.0), (0.4, 9000.0), (0.9, 9000.0), (1.4, 9000.0)], flt=se, spread=0.0015, notional=4e6))
    #                                                                            6 seasoned: the dead coupon's tp (-0.1) is the live successor's ts,
    #                                                                              so the node at a negative time carries sn
    # ---- fixed against float legs
    ann = abutting(0.3, 1.0, 3)
    t.append(make_trade(fix=on(ann, (0, 1, 2), 41000.0), flt=ann, spread=0.0005))   # 7 a fixed flow on the date of the coupon of the same index: merged
    t.append(make_trade(fix=on(semi, (1, 3), 38000.0), flt=semi))                 # 8 fixed flows on dates of coupons of ANOTHER index: two nodes
    #                                                                              each (fixed 1.3 = coupon 1's date, fixed 2.3 = coupon 3's); n_fix < n_flt
    t.append(make_trade(fix=on(abutting(0.3, 0.5, 2), (0, 1), 12000.0) + [(1.8, 12000.0), (2.3, 12000.0), (2.8, 12000.0)], flt=abutting(0.3, 0.5, 2), spread=0.001))
    #                                                                            9 n_fix > n_flt, the first two merged
    t.append(make_trade(fix=annual_fix(50000.0, 4, first=0.7) + [(3.7, 1e6)]))  # 10 n_flt == 0 (a bond)
    t.append(make_trade(flt=abutting(0.05, 0.25, 6), spread=0.004, flt_sign=1.0))   # 11 n_fix == 0
    t.append(make_trade())                                                     # 12 both legs empty, inside the chunk
    t.append(make_trade(fix=on(ann, (0,), 0.0) + on(ann, (1,), 41000.0) + [(5.0, 0.0)], flt=ann))     # 13 fix_pay == 0: merged (adds nothing) and alone (off)
    t.append(make_trade(fix=[(0.9, 0.0)]))                                     # 14 a trade whose only flow pays 0: nothing live
    # ---- signs and sizes
    t.append(make_trade(fix=on(ann, (0, 1, 2), 0.043), flt=ann, notional=1.0, spread=0.001))                     # 15 pay fixed, notional 1
    t.append(make_trade(fix=on(ann, (0, 1, 2), 4.3e6), flt=ann, notional=1e8, fix_sign=-1.0, flt_sign=1.0))      # 16 receive float off, notional 1e8
    t.append(make_trade(fix=annual_fix(43000.0, 5), flt=abutting(0.3, 0.5, 10), notional=1e6, spread=0.002))            # 17 ) two trades that cancel
    t.append(make_trade(fix=annual_fix(43000.0, 5), flt=abutting(0.3, 0.5, 10), notional=1e6, spread=0.002, fix_sign=-1.0, flt_sign=1.0))   # 18 ) exactly
    # ---- dates on and beside the curve's own knots
    t.append(make_trade(fix=[(1.0, 1000.0), (2.0, 1000.0), (60.0, 1000.0)], flt=abutting(0.0, 1.0, 3), notional=5e5))   # 19 on pillar dates, one beyond the last
    t.append(make_trade(fix=[(1.0 + 1e-11, 1000.0), (2.0 - 1e-9, 1000.0)], flt=chain([1.0 - 1e-11], 1.0 + 2e-11), notional=5e5))   # 20 snapping and just not
    t.append(make_trade(fix=[(0.5, 300.0)], flt=chain([0.5], 0.5, alpha=[0.0]), spread=0.01, fix_sign=-1.0))   # 21 one coupon that does not accrue: nothing from the float leg
    t.append(make_trade(fix=[(-2.0, 5.0), (-1.0, 5.0)], flt=abutting(-3.0, 1.0, 2)))                        # 22 matured: no live flow
    t.append(make_trade(fix=annual_fix(25000.0, 30, first=0.45), flt=abutting(0.45, 1.0, 30), notional=7e5, spread=0.0002, flt_sign=1.0, fix_sign=-1.0))   # 23 a 30-year swap
    t.append(make_trade())                                                     # 24 both legs empty, last in the chunk
    return t


def folding_book():
    return make_book(folding_trades())


def folding_layouts(n):
    pairs = np.concatenate([[0], np.arange(1, n, 2), [n, n]]).astype(np.int64)      # trade 0, then (1, 2), ..., (17, 18): the
    return {"each": np.arange(n + 1, dtype=np.int64), "all": np.array([0, n], dtype=np.int64), "pairs": pairs}      # cancelling pair; an empty desk last


def monthly_leg(m, gap, notional, spread, sign):
    ts = np.arange(m) / 12.0 + 0.01 + gap * np.arange(m)
    te = ts + 1.0 / 12.0
    return make_trade(fix=np.stack([te, np.full(m, 2500.0)], axis=1), flt=np.stack([ts, te, te, np.full(m, 1.0 / 12.0)], axis=1),
                      notional=notional, spread=spread, fix_sign=-sign, flt_sign=sign)


def long_leg_book():
    """``(batch, sub_off)``: `_scenario_cases.long_leg_book` without the lag (legs of 400 and 450 coupons around a 3-coupon
    and an empty trade: one owner spans seven 64-flow passes), then chunks of exactly 64, of 65 and of 128 float flows."""
    desks = [[monthly_leg(400, 0.0, 1e6, 0.0, 1.0), monthly_leg(3, 0.0, 2e6, 0.001, -1.0), make_trade(), monthly_leg(450, 1e-3, 3e6, 0.002, 1.0)],
             [monthly_leg(32, 0.0, 1e6, 0.001, 1.0), monthly_leg(32, 1e-3, 2e6, 0.0, -1.0)],
             [monthly_leg(32, 0.0, 1e6, 0.001, 1.0), make_trade(), monthly_leg(33, 1e-3, 2e6, 0.0, -1.0)],
             [monthly_leg(32, 0.0, 1e6 * (i + 1), 0.001 * i, (-1.0) ** i) for i in range(4)]]
    sub_off = np.concatenate([[0], np.cumsum([len(d) for d in desks])]).astype(np.int64)
    return make_book([t for d in desks for t in d]), sub_off


# --------------------------------------------------------------------------------------------------------------- curves
def lookup_curve(times, P=5, seed=17, value_time_hess=False):
    """A hand-made curve on a lookup grid: `_scenario_cases.lookup_curves`' discount factors (the duplicated knot carries
    another value), a dense jac and a symmetric hess without a zero entry, but for the value-time knot: the curve-table
    builder refuses a first-order sensitivity there (jac[0] = 0).  It takes a hess[0] != 0 (``value_time_hess``), under which
    the kernels, which leave the division by D(0) out, and the C oracle, which differentiates it, compute different gammas
    (tests/test_ladder_edges_host.py::test_a_value_time_hess_parts_the_oracle_from_the_kernels), so the cases keep hess[0] = 0."""
    rng = np.random.default_rng(seed)
    K = times.size
    dfs = SC.lookup_curves(times, S=1)[0]
    jac = rng.uniform(0.2, 2.0, (K, P)) * rng.choice([-1.0, 1.0], (K, P)) * -np.maximum(times, 0.05)[:, None] * dfs[:, None]
    jac[0] = 0.0
    hess = rng.uniform(0.1, 3.0, (K, P, P)) * rng.choice([-1.0, 1.0], (K, P, P))
    hess = (hess + np.swapaxes(hess, 1, 2)) * dfs[:, None, None]
    hess[np.abs(hess) < 1e-3] = 0.5
    if not value_time_hess:
        hess[0] = 0.0
    assert np.all(hess[1:] != 0.0) and np.array_equal(hess, np.swapaxes(hess, 1, 2))
    return SimpleNamespace(times=times.copy(), dfs=dfs, jac=jac, hess=hess)


def lookup_book():
    """A unit fixed flow per lookup date, then a coupon per date paid on its accrual end (another of the dates)."""
    d = SC.LOOKUP_DATES
    return _concat_batches([SC.one_flow_book(d), SC.one_coupon_book(d, np.roll(d, 3), np.roll(d, 3))])


def lookup_layouts(n):
    return {"each": np.arange(n + 1, dtype=np.int64), "twos": np.arange(0, n + 1, 2, dtype=np.int64), "all": np.array([0, n], dtype=np.int64)}


@lru_cache(maxsize=None)
def gbp_curve(interp, P=32):
    """The README GBP curve's arrays; ``P`` > 32: `tests/test_gpu_many_pillars.many_pillar_quotes`' wider curves."""
    if P == 32:
        return L.curve_arrays(interp)
    from .test_gpu_many_pillars import many_pillar_quotes
    px, tenors = many_pillar_quotes(P)
    curve = F.gbp_model(VD, interp, px=px, tenors=tenors).curves.GBP_OIS_SONIA
    return build_engine_curve(curve.swap_rates, curve.swap_times, curve.year_fracs)


WIDE_P = 65                       # the projection's column loop takes a second block of one column
WIDE_DESKS = (5, 4, 5, 4, 5, 4, 5, 4, 4)      # 9 desks of 40 trades: the projection's desk tile of 8, then a partial one


def wide_book():
    return L.with_notionals(synthetic.synthesize(VD, 40, seed=31), 31)


@lru_cache(maxsize=None)
def rates_cases(interp):
    """The rates cases of one scheme."""
    out = []
    for name, times in (("lookup", SC.LOOKUP_TIMES), ("lookup, a knot three times", LOOKUP_TIMES_TRIPLE)):
        book = lookup_book()
        out.append(Case(name, lookup_curve(times), book, lookup_layouts(book.n_trades)))
    fold = folding_book()
    out.append(Case("folding", gbp_curve(interp), fold, folding_layouts(fold.n_trades)))
    legs, sub_off = long_leg_book()
    out.append(Case("long legs", gbp_curve(interp), legs, {"desks": sub_off}))
    out.append(Case(f"{WIDE_P} pillars", gbp_curve(interp, WIDE_P), wide_book(), {"nine desks": L.offsets(WIDE_DESKS)}))
    return out


# ------------------------------------------------------------------------------------------------------------ inflation
@dataclasses.dataclass
class YoYCase:
    name: str
    host: object             # the discount curve: times, dfs, jac, hess
    infl: tuple              # (inflation scheme, T, b)
    book: object             # _yoy_ladder_cases.Book: fixed, coupons, names
    layouts: dict            # name -> sub_off
    want_gamma: bool = True


YOY_LOOKUP_DATES = np.concatenate((SC.LOOKUP_DATES, [1.0 + 5e-11, -0.25, 0.0]))      # ... beside the repeated knot, negative, zero
ONE_PILLAR = (np.array([3.0]), np.array([0.03]))


def each_and_all(n):
    return {"each": np.arange(n + 1, dtype=np.int64), "all": np.array([0, n], dtype=np.int64)}


def yoy_knot_book():
    """Every swap of `_yoy_cases.knot_swaps` (each coupon paid at ``te``) with a fixed flow on every second swap."""
    return Y.Book([(name, N, cpns, [(1.25 + 0.5 * i, 0.02 * N)] if i % 2 else []) for i, (name, N, cpns) in enumerate(YC.knot_swaps())])


def yoy_lookup_book():
    """Per lookup date ``tp`` one four-knot coupon (ts, te) = (1.5, 12.0) on T5 and one fixed flow, both paid at ``tp``."""
    return Y.Book([(f"tp = {tp!r}", 1e6, [(tp, 1.5, 12.0, 1e6 * (-1.0) ** i, 0.002)], [(tp, 2e4)]) for i, tp in enumerate(YOY_LOOKUP_DATES)])


def twin_amounts(infl, coupons):
    """The amounts as the twin's `describe` forms them (they do not depend on the discount curve)."""
    return _native.yoy_risk_host((YC.LF, np.array([0.0, 1.0]), np.array([1.0, 1.0])), infl, YC.raw_book([coupons]), 0)["amount"]


def yoy_amount_book(infl):
    """The branches of a coupon's amount; the first two swaps depend on the inflation curve through the twin's amounts."""
    c = YC._cpn
    y = float(twin_amounts(infl, [c(2.5, 3.5, 1.0)])[0])                       # (1 + y) - 1 in float64
    far = c(1.5, 12.0, 1e6, 0.002)
    return Y.Book([
        ("amount exactly 0.0, slots live", 1e6, [c(2.5, 3.5, 1e6, -y)], []),
        ("a fixed flow cancels the coupon's amount", 1e6, [far], [(12.0, -float(twin_amounts(infl, [far])[0]))]),
        ("scale == 0.0", 1e6, [c(2.5, 3.5, 0.0, 0.001)], [(3.5, 1e4)]),
        ("pay == 0.0", 1e6, [c(1.5, 3.0, -1e6, 0.001)], [(2.0, 0.0)]),
        ("tp == 0 on both legs", 1e6, [(0.0, -1.0, 0.0, 1e6, 0.001)], [(0.0, 5e5)]),
        ("tp < 0 on both legs", 1e6, [(-0.6, -1.6, -0.6, 1e6, 0.002)], [(-0.25, 5e5)]),
    ])


YOY_CHUNK_SIZES = (64, 65, 0, 2, 1, 2, 0)


def yoy_chunk_book():
    """Desks of 64 and of 65 one-coupon swaps cycling the singles of `_yoy_cases.knot_swaps`, an empty desk, the two long
    swaps of `_yoy_ladder_cases.edge_book` (70 coupons; 70 fixed flows), a swap of 129 coupons, the pair that cancels and
    an empty desk last."""
    singles = YC.knot_swaps()[:11]
    cycle = lambda n, at: [(f"{at + i}: {singles[(at + i) % 11][0]}",) + tuple(singles[(at + i) % 11][1:]) + ([],) for i in range(n)]
    edge, _ = Y.edge_book(1.0)
    fix_off, fix_tp, fix_pay = edge.fixed

    def pick(name):                                          # the swap of that name with its fixed flows
        i = next(i for i in range(edge.n) if edge.names[i].startswith(name))
        f = slice(int(fix_off[i]), int(fix_off[i + 1]))
        return edge.names[i], edge.notional[i], edge.rows[i], list(zip(fix_tp[f], fix_pay[f]))
    long_legs = [pick("70 monthly coupons"), pick("70 fixed flows")]
    pair = [pick("a swap"), pick("and its opposite")]
    return Y.Book(cycle(64, 0) + cycle(65, 64) + long_legs + [("129 coupons", 1e6, YC.leg(129, 0.31, 1e6 / 12.0, 0.001), [])] + pair)


@lru_cache(maxsize=None)
def yoy_cases(interp):
    """The inflation cases of one discount scheme; the inflation scheme is both in the first case and alternates after."""
    LZ, FF = YC.LZ, YC.FF
    gbp = gbp_curve(interp)
    knots = yoy_knot_book()
    out = [YoYCase(f"inflation knots, {YC.NAMES[im]}", gbp, (im, YC.T5, YC.B5), knots, each_and_all(knots.n)) for im in (LZ, FF)]
    one = Y.Book([s + ([],) for s in YC.single_pillar_swaps()])
    out.append(YoYCase("one pillar", gbp, (FF,) + ONE_PILLAR, one, each_and_all(one.n)))
    looks = yoy_lookup_book()
    for name, times, im in (("discount lookups", SC.LOOKUP_TIMES, LZ), ("discount lookups, a knot three times", LOOKUP_TIMES_TRIPLE, FF)):
        out.append(YoYCase(name, lookup_curve(times), (im, YC.T5, YC.B5), looks, lookup_layouts(looks.n)))
    amounts = yoy_amount_book((LZ, YC.T5, YC.B5))
    out.append(YoYCase("amount edges", gbp, (LZ, YC.T5, YC.B5), amounts, each_and_all(amounts.n)))
    out.append(YoYCase("chunks", gbp, (FF, YC.T5, YC.B5), yoy_chunk_book(), {"desks": L.offsets(YOY_CHUNK_SIZES)}))
    wide = Y.small_book()
    for P_i, im in ((5, LZ), (64, FF)):
        out.append(YoYCase(f"{WIDE_P} pillars, P_i = {P_i}", gbp_curve(interp, WIDE_P), Y.infl_curve(P_i, im), wide,
                           {"nine desks": L.offsets(WIDE_DESKS)}))
    out.append(YoYCase("delta only", gbp, (LZ, YC.T5, YC.B5), knots, each_and_all(knots.n), want_gamma=False))
    return out


def yoy_entry(interp, c, sub_off, ctx=None, dc=None):
    """The host twin's (or, with a ctx and an uploaded curve, the device's) rows of an inflation case."""
    return Y.Entries(interp.value, c.host, ctx, dc)(c.infl, c.book.fixed, c.book.coupons, sub_off, want_gamma=c.want_gamma)


def check_yoy_rows(got, ref, c, what):
    """The share of the bound over pv, delta and gamma, the layout, and +0.0 throughout a gamma that was not asked for."""
    Y.check_layout(got, c.host.jac.shape[1], c.infl[1].size, want_gamma=c.want_gamma)
    return R.worst_share(got, ref, R.RATES_BLOCKS if c.want_gamma else ("pv", "delta"), what=what)


# --------------------------------------------------------------------------------------------------------------- credit
@dataclasses.dataclass
class CreditCase:
    name: str
    host: object
    case: object             # _credit_scenario_cases.Case, ordered by (desk, bucket)
    G: int
    sub_off: np.ndarray


def zero_amount_trade():
    """A fixed flow +1000 and a coupon amount -1000 (alpha < 0, spread 1: no forward, no start) on one date.  At z = 0 with
    different spread times the node's amount a is exactly 0 and a1, a2 are not: the rates rule would switch it off."""
    return make_trade(fix=[(1.3, 1000.0)], flt=[(0.3, 1.3, 1.3, -1.0)], notional=1000.0, spread=1.0, fix_sign=1.0, flt_sign=1.0)


def dress(batch, desk, B, G, special=()):
    """Spread sides for a hand-made batch: z cycles through 0, -50 bp, 800 bp and 120 bp; the fixed flows' spread time is
    t * 365 / 365.25 (merged parts carry different tau), every fifth trade's spread times are all 0; buckets cycle through
    -1 .. G - 2 and the trades ``special`` sit alone in bucket G - 1 at z = 0.  Returns the case ordered by cell."""
    n = batch.n_trades
    z = np.array([0.0, -50 * BP, 800 * BP, 120 * BP])[np.arange(n) % 4]
    bucket = (np.arange(n) % G - 1).astype(np.int32)
    fix_tau = batch.fix_tp * (365.0 / 365.25)
    flt_tau = batch.flt_tp.copy()
    for i in range(4, n, 5):
        fix_tau[int(batch.fix_off[i]):int(batch.fix_off[i + 1])] = 0.0
        flt_tau[int(batch.flt_off[i]):int(batch.flt_off[i + 1])] = 0.0
    for i in special:
        z[i], bucket[i] = 0.0, G - 1
        flt_tau[int(batch.flt_off[i]):int(batch.flt_off[i + 1])] = batch.flt_tp[int(batch.flt_off[i]):int(batch.flt_off[i + 1])]
        fix_tau[int(batch.fix_off[i]):int(batch.fix_off[i + 1])] = batch.fix_tp[int(batch.fix_off[i]):int(batch.fix_off[i + 1])] * (365.0 / 365.25)
    case, sub_off, _ = CL.order_by_cells(CL.Case(batch, z, bucket, fix_tau, flt_tau), desk, B)
    return case, sub_off


@lru_cache(maxsize=None)
def credit_cases(interp):
    out = []
    trades = folding_trades() + [zero_amount_trade()]
    fold = make_book(trades)
    n, G = fold.n_trades, 4
    for name, desk, B in (("folding, two desks", np.arange(n) % 2, 2), ("folding, one desk", np.zeros(n, dtype=np.int64), 1)):
        case, sub_off = dress(fold, desk, B, G, special=(n - 1,))
        out.append(CreditCase(name, gbp_curve(interp), case, G, sub_off))
    legs, leg_off = long_leg_book()
    desk = np.repeat(np.arange(leg_off.size - 1), np.diff(leg_off))
    case, sub_off = dress(legs, desk, leg_off.size - 1, 3)
    out.append(CreditCase("long legs", gbp_curve(interp), case, 3, sub_off))
    wide = wide_book()
    desk = np.repeat(np.arange(len(WIDE_DESKS)), WIDE_DESKS)
    for G in (25, 32):                                       # Q = 65 and Q = 72 on 40 pillars
        case, sub_off = dress(wide, desk, len(WIDE_DESKS), G)
        out.append(CreditCase(f"40 pillars, G = {G}", gbp_curve(interp, 40), case, G, sub_off))
    return out
