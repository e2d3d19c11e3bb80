"""The cases of the cross-currency scenario tests (tests/test_xccy_scenarios_host.py, CPU, and tests/test_gpu_xccy_scenarios.py,
GPU): the smallest shapes that reach each branch of csrc/xccy_scenario_pv.hip.

Books.  ``edges``, ``passes`` and ``lookups`` are the hand-made books of tests/_scenario_edge_cases.py (seasoned legs, flows at
and before the value time, alpha <= 0, payment lags, flt_weight, legs of 0, 1, 64, 65, 128 and 129 coupons, dates on, near,
before and beyond knots and beside a repeated knot, both signs, notionals from 1 to 1e9); ``counts(n)`` are books of n = 1, 63,
64, 65 and 129 swaps with a leg of 63 coupons, notionals 1 .. 1e8 with both signs, and empty swaps first, inside a chunk and at
the end of a chunk.

Tables.  `table(K, S, seed)`: K knots from t = 0 and S rows of positive discount factors (one of them above 1).  (K_f, K_x) =
(2, 2) and (40, 5) sit in LDS together; (300, 40) and (40, 300) leave room for the smaller table alone (the XCCY one, the
foreign one); (4096, 4096) for neither.  A case is ``Case(name, for_method, times_f, dfs_f, x_method, times_x, dfs_x, batch,
sub_off)``; ``dfs_f`` / ``dfs_x`` hold one shared row or S.
"""
import dataclasses
from functools import lru_cache

import numpy as np

from adrates_amd.trades.compiler import TradeBatch

from . import _scenario_cases as SC
from . import _scenario_edge_cases as EC

FF, LF, LZ = 1, 2, 4
NAMES = {FF: "FLAT_FWD", LF: "LINEAR_FWD", LZ: "LINEAR_ZERO"}
PAIRS = ((FF, FF), (FF, LZ), (LZ, FF), (LZ, LZ), (LF, LF))          # every pair the kernel is built for
UNSUPPORTED = ((LF, FF), (LF, LZ), (FF, LF), (LZ, LF))
LDS_BUDGET = 160 * 1024


def lds_mode(Kf, Kx):
    """The source header's rule: which tables sit in LDS."""
    size = lambda f, x: 8 * (Kf + Kx + 64 * (Kf * f + Kx * x))
    if size(1, 1) <= LDS_BUDGET:
        return "both"
    if Kf <= Kx and size(1, 0) <= LDS_BUDGET:
        return "foreign"
    if Kx < Kf and size(0, 1) <= LDS_BUDGET:
        return "xccy"
    return "neither"


@dataclasses.dataclass
class Case:
    name: str
    for_method: int
    times_f: np.ndarray
    dfs_f: np.ndarray
    x_method: int
    times_x: np.ndarray
    dfs_x: np.ndarray
    batch: TradeBatch
    sub_off: np.ndarray

    def __repr__(self):
        return (f"{self.name}, {NAMES[self.for_method]} x {NAMES[self.x_method]}, K = ({self.times_f.size}, {self.times_x.size}), "
                f"rows ({self.dfs_f.shape[0]}, {self.dfs_x.shape[0]})")

    @property
    def args(self):
        return (self.for_method, self.times_f, self.dfs_f, self.x_method, self.times_x, self.dfs_x)

    @property
    def S(self):
        return max(self.dfs_f.shape[0], self.dfs_x.shape[0])


@lru_cache(maxsize=None)
def table(K, S, seed):
    """``(times [K], dfs [S, K])``: knots on multiples of 1/8 (so the books' dyadic dates meet some of them) out to 8 .. 30
    years - the longest legs end beyond the last knot - and smooth zero rates per row, the last row negative (D > 1)."""
    if K == 2:
        times = np.array([0.0, 30.0])
    elif K <= 8:
        times = np.concatenate([[0.0], 0.5 * 4.0 ** np.arange(K - 1)])[:K]
    else:
        step = 0.25 if K <= 64 else (0.125 if K <= 512 else 1.0 / 128)
        times = step * np.arange(K)
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(0.01, 0.06, size=S), rng.uniform(-0.01, 0.01, size=S)
    a[-1] = -0.004
    zero = a[:, None] + b[:, None] * np.sin(times[None, :] / 3.0 + seed)
    dfs = np.exp(-zero * times[None, :])
    assert times.size == K and np.all(np.diff(times) > 0) and np.all(dfs[:, 0] == 1.0) and np.all(dfs > 0)
    return times, dfs


def lookup_tables(S=3):
    """Both curves on the grid with the repeated knot, different rows."""
    t = SC.LOOKUP_TIMES
    return (t, SC.lookup_curves(t, S=S, seed=9)), (t, SC.lookup_curves(t, S=S, seed=10))


# ---------------------------------------------------------------------------------------------------------------- books
@lru_cache(maxsize=None)
def counts_book(n):
    """n swaps: swap j has j % 4 + 1 quarterly coupons from a dyadic start, a payment lag on every third, the two notional
    exchanges as fixed flows, notional 10^(j % 9) and alternating signs; swap 5 (where there is one) carries a leg of 63
    coupons; empty swaps first (0), inside a chunk (7, 30) and at the end of a chunk (63, 127, n - 1)."""
    empty = {0, 7, 30, 63, 127, n - 1} if n > 1 else set()
    trades = []
    for j in range(n):
        if j in empty:
            trades.append(EC.trade(f"empty {j}", fix_sign=-1.0 if j % 2 else 1.0, flt_sign=-1.0))
            continue
        m = 63 if j == 5 else j % 4 + 1
        leg = EC.abutting(0.125 * (j % 5), 0.25 if m < 63 else 0.125, m, lag=(1.0 / 64 if j % 3 == 0 else 0.0))
        N = 10.0 ** (j % 9)
        sign = 1.0 if j % 2 else -1.0
        trades.append(EC.trade(f"swap {j}", fix=[(float(leg[0, 0]) + 1.0 / 64, -N), (float(leg[-1, 1]), N)], flt=leg, notional=N,
                               spread=(j % 7 - 3) * 1e-3, fix_sign=sign, flt_sign=sign))
    return EC.book(trades, False)


def _sub_off(n):
    """Sub-books with an empty one first, cuts inside the chunks and one on a chunk's end."""
    cuts = sorted({0, 0, min(n, 1), n // 3, min(n, 64), n})
    return np.array([0] + cuts, dtype=np.int64)


def _book(which):
    trades = EC._trades(which)
    return EC.book(trades, which == "edges")


def _case(name, pair, f, x, batch, sub_off=None):
    (tf, df), (tx, dx) = f, x
    sub_off = _sub_off(batch.n_trades) if sub_off is None else np.asarray(sub_off, dtype=np.int64)
    assert sub_off[0] == 0 and sub_off[-1] == batch.n_trades and np.all(np.diff(sub_off) >= 0) and np.any(np.diff(sub_off) == 0)
    return Case(name, pair[0], tf, np.atleast_2d(df), pair[1], tx, np.atleast_2d(dx), batch, sub_off)


@lru_cache(maxsize=None)
def cases():
    """The cases whose tables sit in LDS together."""
    edges, passes, lookups = _book("edges"), _book("passes"), _book("lookups")
    out = []
    for pair in PAIRS:
        out.append(_case("edges", pair, table(40, 3, 1), table(5, 3, 2), edges))
        out.append(_case("lookups", pair, *lookup_tables(), lookups))
    out.append(_case("edges", (FF, LZ), table(2, 3, 3), table(2, 3, 4), edges))
    out.append(_case("passes", (LZ, FF), table(40, 2, 5), table(5, 2, 6), passes))
    out.append(_case("passes", (LF, LF), table(2, 2, 7), table(2, 2, 8), passes))
    f, x = table(40, 3, 1), table(5, 3, 2)
    out.append(_case("edges, shared foreign row", (FF, FF), (f[0], f[1][1:2]), x, edges))
    out.append(_case("edges, shared XCCY row", (LZ, LZ), f, (x[0], x[1][2:3]), edges))
    out.append(_case("edges, one scenario", (LF, LF), (f[0], f[1][:1]), (x[0], x[1][:1]), edges))
    for n in (1, 63, 64, 65, 129):
        out.append(_case(f"{n} swaps", PAIRS[n % 5], table(40, 2, 9), table(5, 2, 10), counts_book(n)))
    assert all(lds_mode(c.times_f.size, c.times_x.size) == "both" for c in out)
    return tuple(out)


@lru_cache(maxsize=None)
def lds_cases():
    """Every book where only one table fits the LDS (each way round) and where neither does."""
    out = []
    shapes = (("xccy", 300, 40), ("foreign", 40, 300), ("neither", 4096, 4096))
    for j, (mode, Kf, Kx) in enumerate(shapes):
        assert lds_mode(Kf, Kx) == mode
        f, x = table(Kf, 2, 11 + j), table(Kx, 2, 21 + j)
        for i, (name, batch) in enumerate((("edges", _book("edges")), ("passes", _book("passes")), ("lookups", _book("lookups")),
                                           ("65 swaps", counts_book(65)))):
            out.append(_case(f"{name}, LDS: {mode}", PAIRS[(i + 2 * j) % 5], f, x, batch))
    return tuple(out)


def mixed_rows(rows, S, seed):
    """``S`` distinct positive rows between the given ones (geometric mixtures); the first knot stays 1."""
    mix = np.random.default_rng(seed).uniform(0.0, 1.0, size=(S, rows.shape[0]))
    out = np.exp((mix / mix.sum(1, keepdims=True)) @ np.log(rows))
    out[:, 0] = 1.0
    return out


def take(batch, lo, hi):
    """The trades lo .. hi - 1 of a batch as a batch of their own."""
    f0, f1, l0, l1 = int(batch.fix_off[lo]), int(batch.fix_off[hi]), int(batch.flt_off[lo]), int(batch.flt_off[hi])
    w = None if batch.flt_weight is None else batch.flt_weight[l0:l1].copy()
    return TradeBatch(batch.fix_off[lo:hi + 1] - f0, batch.flt_off[lo:hi + 1] - l0, batch.fix_tp[f0:f1].copy(), batch.fix_pay[f0:f1].copy(),
                      batch.flt_tp[l0:l1].copy(), batch.flt_ts[l0:l1].copy(), batch.flt_te[l0:l1].copy(), batch.flt_alpha[l0:l1].copy(),
                      batch.notional[lo:hi].copy(), batch.spread[lo:hi].copy(), batch.fix_sign[lo:hi].copy(), batch.flt_sign[lo:hi].copy(), w)
