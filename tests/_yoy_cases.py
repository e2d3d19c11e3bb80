"""One table of raw YoY books for the CPU tests (tests/test_yoy_third_evaluation.py) and the GPU tests
(tests/test_gpu_yoy_edges.py) of csrc/yoy_risk.hip, and the comparison with the 60-digit third evaluation
(oracle/mp_oracle.py::MpYoY) that both use.  No market objects: a case is the kernel's raw inputs, and every swap is
named by what it reaches in `describe()`, `si::locate`, `si::log_weights`, `si::df` or the launch geometry."""
import functools

import numpy as np

from adrates_amd import _native
from oracle import mp_oracle as MP

from . import _scenario_cases as SC
from ._parity import ladder_err, unit_notional_err

LZ, FF, LF = 4, 1, 2                                            # LINEAR_ZERO_RATES, FLAT_FWD_RATES, LINEAR_FWD_RATES
DISC_SCHEMES = (LZ, FF, LF)
INFL_SCHEMES = (LZ, FF)
NAMES = {LZ: "LINEAR_ZERO", FF: "FLAT_FWD", LF: "LINEAR_FWD"}
PILLAR_EDGES = (1, 8, 9, 16, 17, 32, 33, 64)                    # around every kernel instantiation's P * P <= 64 * kSlots
LEG_EDGES = (0, 1, 63, 64, 65, 128, 129)                        # around the staging passes of 64 coupons
MAX_KNOTS = 4096                                                # ADR_YOY_MAX_KNOTS
FULL_MATRIX = 9                                                 # up to this P every gamma pair is differenced
BOOK_EDGES = (1, 15, 16, 17, 33)                                # around the chunks of ADR_YOY_CHUNK = 16 swaps
FLOORS = {"pv": 1e-4, "delta": 1e-8, "gamma": 1e-12}            # the ladder floors of tests/_parity.py::trade_errors


def raw_book(rows):
    """A coupon book from per-swap lists of (tp, ts, te, scale, spread)."""
    off, cols = [0], {k: [] for k in _native.YOY_FIELDS}
    for cpns in rows:
        for c in cpns:
            for k, v in zip(_native.YOY_FIELDS, c):
                cols[k].append(float(v))
        off.append(len(cols["tp"]))
    out = {"cpn_off": np.array(off, dtype=np.int64)}
    out.update({k: np.array(v, dtype=np.float64) for k, v in cols.items()})
    return out


def one_swap(book, i):
    """Swap ``i`` of a raw book as a book of its own."""
    lo, hi = int(book["cpn_off"][i]), int(book["cpn_off"][i + 1])
    out = {k: v[lo:hi] for k, v in book.items() if k != "cpn_off"}
    out["cpn_off"] = np.array([0, hi - lo], dtype=np.int64)
    return out


def disc_grid(K=None):
    """A discount grid from t = 0 with repeated knot times (the engine grid keeps duplicates; the duplicate carries
    another value, and the first of equal knots wins a snap)."""
    if K is None:
        times = np.array([0.0, 0.25, 0.5, 1.0, 1.0, 2.0, 3.0, 5.0, 7.0, 10.0, 10.0, 15.0, 20.0, 30.0, 50.0])
    else:
        times = np.linspace(0.0, 60.0, K)
    zero = 0.02 + 0.015 * np.sin(0.37 * np.arange(times.size)) ** 2
    dfs = np.exp(-zero * times)
    if K is None:
        dfs[4] *= 0.9995
        dfs[10] *= 1.0004
    return times, dfs


class Case:
    """``disc`` / ``infl``: the kernel's curve inputs; ``rows``: per swap the coupons (tp, ts, te, scale, spread);
    ``names`` and ``notional``: per swap."""

    def __init__(self, name, disc, infl, swaps):
        self.name, self.disc, self.infl = name, disc, infl
        self.names = [s[0] for s in swaps]
        self.notional = np.array([float(s[1]) for s in swaps])
        self.rows = [list(s[2]) for s in swaps]
        self.book = raw_book(self.rows)
        self.P = int(np.asarray(infl[1]).size)

    def index(self, swap_name):
        return self.names.index(swap_name)

    def __repr__(self):
        return self.name


# ------------------------------------------------------------------------------------------------- knot bookkeeping
T5 = np.array([1.0, 2.0, 5.0, 10.0, 20.0])
B5 = np.array([0.031, 0.032, 0.034, 0.035, 0.036])


def _cpn(ts, te, scale, spread=0.0, tp=None):
    return (te if tp is None else tp, ts, te, scale, spread)


def knot_swaps():
    """Single coupons that each reach one branch of describe()'s knot bookkeeping on T5, then all of them in one swap
    (the gamma block accumulates over different knot sets) and a seasoned leg."""
    singles = [
        ("one segment: two slots merge away", 1e6, [_cpn(2.5, 3.5, 1e6, 0.001)]),
        ("te's lower knot is ts's upper knot: three knots", 2e6, [_cpn(1.5, 3.0, -2e6)]),
        ("far-apart segments: four knots", 1e6, [_cpn(1.5, 12.0, 1e6, 0.002)]),
        ("ts == te: every coefficient cancels", 7e5, [_cpn(3.3, 3.3, 7e5, 0.0125)]),
        ("ts < 0 < te < T_1: knot 0 dropped", 1e6, [_cpn(-0.4, 0.6, -1e6, 0.001)]),
        ("ts and te on pillars", 3e6, [_cpn(2.0, 5.0, 3e6)]),
        ("ts and te within 1e-10 of pillars", 3e6, [_cpn(2.0 + 3e-11, 5.0 - 4e-11, 3e6)]),
        ("ts on the last pillar, te beyond", 1e6, [_cpn(20.0, 21.0, 1e6, 0.001)]),
        ("both beyond the last pillar", 1e6, [_cpn(22.0, 23.5, -1e6, 0.003)]),
        ("ts before T_1, te on T_1", 1.0, [_cpn(0.25, 1.0, 1.0)]),
        ("ts == 0", 1e8, [_cpn(0.0, 1.0, 1e8, 0.001)]),
    ]
    together = [c for _, _, cpns in singles for c in cpns]
    seasoned = [(-0.6 + k, -1.6 + k, -0.6 + k, 1e6, 0.002) for k in range(8)]   # tp = -0.6 and ts < 0 first
    at_value_time = [(0.0, -1.0, 0.0, 1e6, 0.001), (1.0, 0.0, 1.0, 1e6, 0.001)]  # tp == 0 is masked (strict)
    return singles + [("all of the above in one swap", 1e8, together), ("seasoned: tp <= 0 masked", 1e6, seasoned),
                      ("paid at the value time", 1e6, at_value_time), ("no coupons", 1.0, [])]


def single_pillar_swaps():
    return [("P = 1: before the pillar", 1e6, [_cpn(0.5, 1.5, 1e6, 0.001)]),
            ("P = 1: across the pillar", 1e6, [_cpn(2.5, 3.5, -1e6)]),
            ("P = 1: te on the pillar", 1e3, [_cpn(2.0, 3.0, 1e3)]),
            ("P = 1: beyond the pillar", 1e6, [_cpn(4.0, 5.0, 1e6, 0.002)]),
            ("P = 1: ts < 0", 1e6, [_cpn(-0.5, 0.5, 1e6)]),
            ("P = 1: a leg", 1e7, [(k / 2.0, k / 2.0 - 1.0, k / 2.0, 5e6, 0.001) for k in range(1, 12)])]


@functools.lru_cache(maxsize=None)
def knot_cases():
    out = []
    for j, im in enumerate(INFL_SCHEMES):
        for dm in DISC_SCHEMES:
            disc = (dm,) + disc_grid()
            out.append(Case(f"knots {NAMES[im]} / disc {NAMES[dm]}", disc, (im, T5, B5), knot_swaps()))
        out.append(Case(f"one pillar {NAMES[im]}", (DISC_SCHEMES[j],) + disc_grid(), (im, np.array([3.0]), np.array([0.03])),
                        single_pillar_swaps()))
    return out


# ------------------------------------------------------------------------------- discount lookups through the kernel
def lookup_grids():
    """name -> (times, dfs, payment times): pv of a unit coupon with ts == te and spread 1 is D(tp) / D(0)."""
    t_dup = SC.LOOKUP_TIMES
    d_dup = SC.lookup_curves(t_dup)[0]
    t2, d2 = np.array([0.0, 10.0]), np.array([1.0, 0.71])
    tk, dk = disc_grid(MAX_KNOTS)
    k = 2000
    dates_k = np.array([tk[1], tk[k], tk[k] + 3e-11, tk[k] - 3e-11, tk[k] + 1e-9, 0.5 * (tk[k] + tk[k + 1]), 0.25 * tk[1],
                        tk[-2] + 1e-3, tk[-1], tk[-1] + 1e-11, tk[-1] + 5.0, -0.5, 0.0])
    dates_2 = np.array([1e-11, 1e-9, 0.3, 5.0, 10.0 - 1e-11, 10.0, 10.0 + 1e-9, 25.0, -1.0, 0.0])
    return {"repeated knots, K = 6": (t_dup, d_dup, np.concatenate((SC.LOOKUP_DATES, [-0.25, 0.0]))),
            "K = 2": (t2, d2, dates_2), "K = 4096": (tk, dk, dates_k)}


@functools.lru_cache(maxsize=None)
def lookup_cases():
    out = []
    for name, (times, dfs, dates) in lookup_grids().items():
        for dm in DISC_SCHEMES:
            swaps = [(f"tp = {tp!r}", 1.0, [(tp, 1.7, 1.7, 1.0, 1.0)]) for tp in dates]
            out.append(Case(f"lookup {name} {NAMES[dm]}", (dm, times, dfs), (LZ, T5, B5), swaps))
    return out


def lookup_reference(case):
    """``D(tp) / D(0)`` by `cavour_oracle.simple_interpolate` for the live swaps of a lookup case, 0 for the masked."""
    from oracle import cavour_oracle as O
    dm, times, dfs = case.disc
    tp = case.book["tp"]
    d = np.asarray(O.simple_interpolate(tp, times, dfs, dm), dtype=np.float64).reshape(-1)
    d0 = float(O.simple_interpolate(0.0, times, dfs, dm))
    return np.where(tp > 0.0, d / d0, 0.0)


# ---------------------------------------------------------------------------------------------------------- geometry
def pillars(P, seed=0):
    rng = np.random.default_rng(100 + P + seed)
    T = np.linspace(0.5, 40.0, P) if P > 1 else np.array([3.0])
    return T, 0.03 + 0.006 * np.sin(0.2 * T) + rng.uniform(-2e-4, 2e-4, P)


def leg(L, start, scale, spread, lag=0.0):
    """``L`` monthly coupons on the year-on-year ratio, the first paid at ``start + 1/12 + lag``."""
    te = start + np.arange(1, L + 1) / 12.0
    return [(e + lag, e - 1.0, e, scale, spread) for e in te]


def geometry_swaps(n, shift=0):
    """``n`` swaps: legs of LEG_EDGES coupons in turn, empty swaps first, inside a chunk, at a chunk's end and last,
    seasoned legs, alternating signs and notionals from 1 to 1e8."""
    out = []
    empty = {0, 7, 15, n - 1} if n > 1 else set()
    for i in range(n):
        L = 0 if i in empty else [x for x in LEG_EDGES if x][(i + shift) % 6]
        if n == 1:
            L = LEG_EDGES[-1]
        N = 10.0 ** ((i + shift) % 9)
        sign = -1.0 if i % 2 else 1.0
        start = (-1.6, 0.0, 0.31, 2.05, 17.0, 33.0)[(i + 2 * shift) % 6]   # seasoned ... beyond the last pillar
        out.append((f"swap {i}: {L} coupons from {start}", N, leg(L, start, sign * N / 12.0, 0.001 * (i % 3), (i % 2) * 2.0 / 365.0)))
    return out


def geometry_case(P, n, im, dm=LZ, shift=0):
    return Case(f"P = {P}, n = {n}, {NAMES[im]} / disc {NAMES[dm]}", (dm,) + disc_grid(), (im,) + pillars(P),
                geometry_swaps(n, shift))


@functools.lru_cache(maxsize=None)
def geometry_cases():
    """One 17-swap book (two chunks, the second of one empty swap) per pillar-count edge; the schemes alternate."""
    return [geometry_case(P, 17, INFL_SCHEMES[j % 2], DISC_SCHEMES[j % 3], shift=j) for j, P in enumerate(PILLAR_EDGES)]


def all_cases():
    return knot_cases() + lookup_cases() + geometry_cases()


# ------------------------------------------------------------------------------------------- the 60-digit comparison
@functools.lru_cache(maxsize=None)
def _third(case, i):
    """The MpYoY of swap ``i`` with its value, amounts and full delta, and a cache of gamma pairs."""
    t = MP.MpYoY(case.disc, case.infl, case.rows[i])
    return dict(mp=t, value=t.value(), amount=t.amounts(), delta=t.delta(), gamma={}, touched=t.touched())


def third_gamma(case, i, pairs):
    ref = _third(case, i)
    need = sorted(set(pairs) - set(ref["gamma"]))
    ref["gamma"].update(ref["mp"].gamma(need))
    return {pq: ref["gamma"][pq] for pq in pairs}


def gamma_pairs(ref_delta, other, P):
    """Every pair for P <= FULL_MATRIX (the P <= 8 instantiation and its edge at 9 included).  Beyond that, as tests/test_mp_third_evaluation.py chooses: all pairs among the four
    largest-delta pillars, the six largest entries of the other side's matrix wherever they are, and the pairs of two
    zero-delta pillars with the largest-delta one."""
    if P <= FULL_MATRIX:
        return [(p, q) for p in range(P) for q in range(p, P)]
    live = [int(p) for p in np.argsort(-np.abs(ref_delta), kind="stable")[:4]]
    pairs = {(min(p, q), max(p, q)) for p in live for q in live}
    for flat in np.argsort(-np.abs(np.triu(other)).ravel(), kind="stable")[:6]:
        pairs.add((int(flat // P), int(flat % P)))
    for p in np.flatnonzero(ref_delta == 0.0)[:2]:
        pairs.add((min(int(p), live[0]), max(int(p), live[0])))
    return sorted(pairs)


def swap_errors(case, i, amount, pv, delta, gamma):
    """The worst error of one swap's outputs against MpYoY on that swap's own notional: per unit notional
    (`unit_notional_err`) and ladder-relative with the floors of `trade_errors` (tests/_parity.py).  Asserts the exact
    zeros: pillars that no live coupon's lookups name have a zero delta entry and zero gamma rows and columns."""
    ref, n, P = _third(case, i), case.notional[i], case.P
    errs = {}
    if len(case.rows[i]):
        errs["amount"] = unit_notional_err(amount, ref["amount"], n)
    else:
        assert pv == 0.0 and not np.any(delta) and not np.any(gamma), (case, case.names[i])
    errs["pv"] = max(unit_notional_err(pv, ref["value"], n), ladder_err(pv, ref["value"], FLOORS["pv"] * n))
    errs["delta"] = max(unit_notional_err(delta, ref["delta"], n), ladder_err(delta, ref["delta"], FLOORS["delta"] * n))
    pairs = gamma_pairs(ref["delta"], gamma, P)
    want = third_gamma(case, i, pairs)
    w = np.array([want[pq] for pq in pairs] * 2)
    g = np.array([gamma[p, q] for p, q in pairs] + [gamma[q, p] for p, q in pairs])
    errs["gamma"] = max(unit_notional_err(g, w, n), ladder_err(g, w, FLOORS["gamma"] * n))
    dead = sorted(set(range(P)) - set(ref["touched"]))
    assert not np.any(ref["delta"][dead]) and all(v == 0.0 for (p, q), v in want.items() if p in dead or q in dead)
    assert not np.any(delta[dead]) and not np.any(gamma[dead, :]) and not np.any(gamma[:, dead]), (case, case.names[i])
    if P > FULL_MATRIX:                                         # the entries that were not differenced: zero by structure
        sampled = np.zeros((P, P), dtype=bool)
        for p, q in pairs:
            sampled[p, q] = sampled[q, p] = True
        live = np.zeros(P, dtype=bool)
        live[ref["touched"]] = True
        assert not np.any(gamma[~(live[:, None] & live[None, :]) & ~sampled])
    return errs


def case_errors(case, got):
    """``{swap name: errors}`` of a `yoy_risk` / `yoy_risk_host` result with per-swap rows against MpYoY."""
    off = case.book["cpn_off"]
    return {case.names[i]: swap_errors(case, i, got["amount"][off[i]:off[i + 1]], got["pv"][i], got["delta"][i], got["gamma"][i])
            for i in range(len(case.rows))}


def worst(errors):
    """(error, swap name, measure) of the largest entry of `case_errors`."""
    return max(((e, name, k) for name, d in errors.items() for k, e in d.items()), default=(0.0, "", ""))


def row_errors(case, dev, host):
    """Per swap row, each on its own scale: the worst |device - twin| / max(max |twin row|, the ladder floor)."""
    out = 0.0
    for key in ("pv", "delta", "gamma"):
        a = np.asarray(dev[key]).reshape(len(case.rows), -1)
        b = np.asarray(host[key]).reshape(len(case.rows), -1)
        if a.size:
            scale = np.maximum(np.max(np.abs(b), axis=1), FLOORS[key] * case.notional)
            out = max(out, float(np.max(np.max(np.abs(a - b), axis=1) / scale)))
    off = case.book["cpn_off"]
    per = np.repeat(case.notional, np.diff(off))
    if per.size:
        out = max(out, float(np.max(np.abs(dev["amount"] - host["amount"]) / np.maximum(np.abs(host["amount"]), 1e-4 * per))))
    return out


def fixed_order_sum(rows, chunk=16):
    """The documented order of agg (include/adrates.h) on per-swap rows [n, R]: chunks of ADR_YOY_CHUNK swaps summed in
    order from 0.0, chunk j added to lane j % 64 in order, then a halving tree over the 64 lanes."""
    rows = np.asarray(rows, dtype=np.float64)
    lanes = [np.zeros(rows.shape[1]) for _ in range(64)]
    for j, lo in enumerate(range(0, rows.shape[0], chunk)):
        acc = np.zeros(rows.shape[1])
        for r in rows[lo:lo + chunk]:
            acc = acc + r
        lanes[j % 64] = lanes[j % 64] + acc
    h = 32
    while h >= 1:
        for c in range(h):
            lanes[c] = lanes[c] + lanes[c + h]
        h //= 2
    return lanes[0]
