"""The hand-made books of the inflation scenario edge tests (tests/test_yoy_scenario_edges_host.py, CPU, and
tests/test_gpu_yoy_scenario_edges.py, GPU): the smallest books that reach the shortcuts only csrc/yoy_scenario_pv.hip has
(`make_slot` / `apply_slot` / `lane_slot`: ln I(ts) taken from `Acc::le`, its hand-over between two 64-index passes, ts == te,
a fixed flow that shares the coupon's D(tp), shared rows on either side, the global discount table, legs of unequal length,
node 0 of the inflation table) and the places where `exp(le - ls) - 1` cancels.

Dates, pillars, knots and amounts are dyadic, so dates that have to be EQUAL are equal bits by construction and every input is
the number it is written as; `check_books` asserts, swap by swap, the property each swap is named for.  A coupon is a row
(tp, ts, te, scale, spread), a fixed flow (xt, pay).  A case is ``Case(name, times, dfs, T, b, fixed, book, sub_off, names)``."""
import dataclasses
from functools import lru_cache

import numpy as np

from . import _yoy_cases as YC

DISC_SCHEMES, INFL_SCHEMES, NAMES = YC.DISC_SCHEMES, YC.INFL_SCHEMES, YC.NAMES
TP, TS, TE, SCALE, SPREAD = range(5)
STEP = 0.125                                   # the long legs' period
NEAR, OUT = 2.0 ** -35, 2.0 ** -33             # 2.9e-11: snaps to a pillar; 1.2e-10: just outside the 1e-10 window
TINY_B = -1.0 + 2.0 ** -20
PAY = -32768.0
T8 = np.array([0.5, 1.0, 2.0, 3.0, 5.0, 8.0, 16.0, 32.0])
T64 = 0.5 * np.arange(1, 65)
T5 = np.array([1.0, 2.0, 3.0, 4.0, 5.0])       # pillars 1, 3, 5, 7, 9 of T64


@dataclasses.dataclass
class Case:
    name: str
    times: np.ndarray
    dfs: np.ndarray          # [S, K]
    T: np.ndarray
    b: np.ndarray            # [S, P]
    fixed: tuple             # (fix_off, fix_tp, fix_pay)
    book: dict               # cpn_off and the fields of _native.YOY_FIELDS
    sub_off: np.ndarray      # desks with cuts inside a chunk and an empty desk
    names: tuple = ()        # one per swap

    @property
    def n(self):
        return len(self.names)

    def coupons(self, i):
        """[m, 5] rows (tp, ts, te, scale, spread) of swap i."""
        sl = slice(int(self.book["cpn_off"][i]), int(self.book["cpn_off"][i + 1]))
        return np.stack([self.book[f][sl] for f in ("tp", "ts", "te", "scale", "spread")], axis=1)

    def flows(self, i):
        """[m, 2] rows (xt, pay) of swap i."""
        sl = slice(int(self.fixed[0][i]), int(self.fixed[0][i + 1]))
        return np.stack([self.fixed[1][sl], self.fixed[2][sl]], axis=1)


# ---------------------------------------------------------------------------------------------------------------- books
def swap(name, cpn=(), fix=()):
    return dict(name=name, cpn=np.array(cpn, dtype=np.float64).reshape(-1, 5), fix=np.array(fix, dtype=np.float64).reshape(-1, 2))


def assemble(swaps):
    """``(fixed, book, names)`` of a list of `swap`s."""
    off = lambda key: np.concatenate([[0], np.cumsum([s[key].shape[0] for s in swaps])]).astype(np.int64)
    cpn, fix = np.concatenate([s["cpn"] for s in swaps]), np.concatenate([s["fix"] for s in swaps])
    book = {"cpn_off": off("cpn")}
    book.update({f: cpn[:, j].copy() for j, f in enumerate(("tp", "ts", "te", "scale", "spread"))})
    return (off("fix"), fix[:, 0].copy(), fix[:, 1].copy()), book, tuple(s["name"] for s in swaps)


def tiling(first, period, m, scale=1e6, spread=0.0, lag=0.0):
    """``m`` coupons whose start IS the previous coupon's end (the same float64 number), paid ``lag`` after their end."""
    edges = first + period * np.arange(m + 1)
    assert np.all(edges * 4096 == np.round(edges * 4096))
    return np.stack([edges[1:] + lag, edges[:-1], edges[1:], np.full(m, scale), np.full(m, spread)], axis=1)


def on(cpn, idx, pay=PAY):
    """Fixed flows on those coupons' payment dates."""
    return [(float(cpn[i, TP]), pay) for i in idx]


def annual():
    return tiling(0.25, 1.0, 6, 1e6, 0.0078125)                 # ends 1.25 .. 6.25


def tiling_swaps():
    """The gates of `kTsIsPrevTe` and of `kFixIsCpnTp`."""
    t = []
    a = annual()
    t.append(swap("a tiling annual leg, a fixed flow with every coupon", a, on(a, range(6))))
    d = annual()
    d[2, TP] = 0.0
    t.append(swap("coupon 2 dead (tp == 0) before a coupon that starts on its end", d, on(d, range(6))))      # and a fixed flow at 0.0
    d = annual()
    d[2, TP] = -1.0
    t.append(swap("coupon 2 dead (tp < 0) before a coupon that starts on its end, a fixed flow at |tp|", d,
                  on(d, (0, 1)) + [(1.0, PAY)] + on(d, (3, 4, 5))))
    d = annual()
    d[0, TP] = -0.5
    t.append(swap("coupon 0 dead before a coupon that starts on its end", d))
    e = annual()
    e[2, TS] = e[2, TE]
    t.append(swap("coupon 2 has ts == te before a coupon that starts on its end", e, on(e, (1, 2, 3))))
    m = np.insert(annual(), 3, [7.0, 7.0, 7.0, 5e5, 0.015625], axis=0)
    t.append(swap("ts == te elsewhere, inserted in a tiling run", m, on(m, (3,))))
    r = annual()
    r[1, [TS, TE]] = r[1, [TE, TS]]
    t.append(swap("te < ts on coupon 1", r))
    r = r.copy()
    r[2, TS] = r[1, TE]
    t.append(swap("te < ts on coupon 1 and coupon 2 starts on that end", r, on(r, (2,))))
    t.append(swap("a leg that ends at 3.25", tiling(0.25, 1.0, 3, -2e6, 0.001953125)))
    t.append(swap("coupon 0 starts at 3.25, the previous swap's last end", tiling(3.25, 1.0, 3, -2e6, 0.001953125)))
    a = annual()
    t.append(swap("fixed flows on the NEXT coupon's payment date", a, on(a, range(1, 6)) + [(8.0, PAY)]))
    t.append(swap("fixed flows on the PREVIOUS coupon's payment date", a, [(0.75, PAY)] + on(a, range(5))))
    t.append(swap("fixed flows one ulp beside the payment dates", a,
                  [(float(np.nextafter(a[i, TP], np.inf if i % 2 else -np.inf)), PAY) for i in range(6)]))
    lagged = tiling(0.25, 1.0, 6, 1e6, 0.0, lag=1.0 / 64)
    t.append(swap("a payment lag, fixed flows on the coupons' ENDS", lagged, [(float(v), PAY) for v in lagged[:, TE]]))
    return t


DAY = 1.0 / 365.0


def cancellation_swaps():
    """Where `exp(le - ls) - 1` and the sums cancel; row 0 of `breakeven_rows` is 2^-5 on every pillar."""
    return [
        swap("a period of one day", [(3.0 + DAY, 3.0, 3.0 + DAY, 1e9, 0.0)]),
        swap("a period of 2^-12 years", [(4.0, 3.5, 3.5 + 2.0 ** -12, 1e9, 0.0)]),
        swap("a period of 2^-12 years across a pillar", [(3.0, 3.0 - 2.0 ** -13, 3.0 + 2.0 ** -13, -1e9, 0.0)]),
        swap("a leg of 2^-12-year periods", tiling(6.0, 2.0 ** -12, 4, 1e9, 0.0), [(6.0 + 2.0 ** -12, 64.0)]),
        swap("spread == -y on row 0", [(2.0, 1.0, 2.0, 1e6, -0.03125)]),
        swap("spread one ulp beside -y on row 0", [(2.0, 1.0, 2.0, 1e6, float(np.nextafter(-0.03125, 0.0)))]),
        swap("two coupons of opposite scale", [(2.5, 1.5, 2.5, 1e6, 0.0), (2.5, 1.5, 2.5, -1e6, 0.0)]),
        swap("a coupon against the fixed flow that pays 2^-5 of it", [(2.0, 1.0, 2.0, 1e6, 0.0)], [(2.0, -31250.0)]),
        swap("scale == 0.0 with live dates", [(2.5, 1.5, 2.5, 0.0, 0.015625)]),
        swap("scale == -0.0 with live dates, a dead fixed flow", [(2.5, 1.5, 2.5, -0.0, 0.015625)], [(-1.0, 5.0)]),
        swap("scale == -0.0, ts == te, pay == -0.0", [(2.5, 1.5, 1.5, -0.0, 0.015625)], [(2.5, -0.0)]),
        swap("inside the segment whose ends have equal L on row 4", [(1.75, 1.25, 1.75, 1e6, 0.0)]),
        swap("no flows"),
        swap("every flow dead", [(0.0, 1.0, 2.0, 1e6, 0.01), (-1.0, 2.0, 3.0, 1e6, 0.01)], [(0.0, 5.0), (-2.0, 5.0)]),
    ]


def lookup_dates(T):
    first, last, P = float(T[0]), float(T[-1]), T.size
    mid = 0.5 * (T[P // 2 - 1] + T[P // 2]) if P > 1 else 0.75 * first
    return np.array([0.0, -0.5, first / 2, first, first + NEAR, first - NEAR, first + OUT, first - OUT, float(mid), last,
                     last + NEAR, last - OUT, last + OUT, last + 8.0, last + 1.0, first / 4])


def lookup_swaps(T):
    """Coupons whose ts and te run through `lookup_dates` (at 0, before 0, before the first pillar, on a pillar, within 1e-10
    of one and just outside, between pillars, beyond the last): one swap per coupon and the same coupons as one leg."""
    d = lookup_dates(T)
    rows = []
    for r in (3, 7):
        te, tp = np.roll(d, r), np.roll(d, 2 * r + 1)
        rows.append(np.stack([np.where(tp <= 0.0, 0.125, tp), d, te, np.ones(d.size), np.full(d.size, 0.015625)], axis=1))
    rows = np.concatenate(rows)
    t = [swap(f"ts = {float(row[TS])!r}, te = {float(row[TE])!r}", row[None, :], [(float(row[TE]), 1.0)]) for row in rows]
    t.append(swap("all lookup coupons in one leg", rows, [(float(v), 1.0) for v in rows[:, TP]]))
    return t


def pass_swaps():
    """The 64-index passes of the kernel's `base` loop: index 64 is lane 0 of the second pass, and it reads index 63 from
    global memory; legs of unequal length."""
    leg = lambda m: tiling(STEP, STEP, m, 125000.0, 0.0009765625)
    t = [swap(f"{m} tiling coupons", leg(m)) for m in (63, 64, 65, 128, 129)]
    d = leg(65)
    d[63, TP] = -1.0
    t.append(swap("65 coupons, coupon 63 dead", d))
    e = leg(65)
    e[63, TS] = e[63, TE]
    t.append(swap("65 coupons, coupon 63 has ts == te", e))
    f = leg(129)
    f[63, TS] = f[63, TE]
    f[127, TP] = 0.0
    t.append(swap("129 coupons, coupon 63 has ts == te and coupon 127 is dead", f, on(f, (0, 1, 2))))
    for nf in (0, 1, 65, 130):
        for nc in (0, 1, 64, 129):
            t.append(swap(f"n_fix = {nf}, n_cpn = {nc}", leg(nc), [(STEP * (j + 2) + (j % 2) / 64.0, 1000.0 + j) for j in range(nf)]))
    t.append(swap("every flow dead", [(0.0, 1.0, 2.0, 1e6, 0.01), (-1.0, 2.0, 3.0, 1e6, 0.01)], [(0.0, 5.0), (-2.0, 5.0)]))
    return t


def grid_swaps():
    """Flows for the 264-knot grid whose inflation dates all lie ON pillars that `T5` and `T64` share (or at 0), so the small
    curve, which leaves the discount table in LDS, and the large one, which sends it to global memory, price the same numbers;
    the payment dates lie on knots, between knots, before the first interior knot and beyond the last."""
    a = tiling(1.0, 1.0, 4, 1e6, 0.0078125)
    b = tiling(1.0, 1.0, 4, -3e6, 0.0, lag=1.0 / 64)
    c = np.array([(0.125, 0.0, 1.0, 1e6, 0.0), (70.0, 5.0, 1.0, 1e6, 0.0), (65.75, 2.0, 4.0, 1e6, 0.0), (33.0, 3.0, 3.0, 1e6, 0.03125)])
    return [swap("annual coupons on the common pillars, paid on knots, with fixed flows", a, on(a, range(4))),
            swap("the same paid between knots, fixed flows on the knots", b, [(float(v), PAY) for v in b[:, TE]]),
            swap("from 0, te < ts, the last knot, beyond it, ts == te", c, [(65.75, 1e6), (66.0, 1e6)]),
            swap("70 fixed flows out to 66 years against 2 coupons", a[:2], [(0.9375 * (j + 1) + 0.0625, 1000.0 + j) for j in range(70)])]


# --------------------------------------------------------------------------------------------------------------- curves
def discount_rows(times, S):
    """``[S, K]`` distinct rows; a repeated knot carries a value of its own (the first of equal knots wins a snap); the last
    two rows by hand: negative rates (D > 1) and rates of about 20 %."""
    s, k = np.arange(S)[:, None], np.arange(times.size)[None, :]
    rows = np.exp(-(0.02 + 0.0004 * s + 0.012 * np.sin(0.37 * k + 0.9 * s) ** 2) * times[None, :])
    if S >= 3:
        rows[-2] = np.exp(0.004 * times)
        rows[-1] = np.exp(-(0.2 + 0.001 * np.sin(times)) * times)
    rep = np.flatnonzero(times[1:] == times[:-1]) + 1
    rows[:, rep] *= 0.9995
    assert times[0] == 0.0 and np.all(rows[:, 0] == 1.0)
    return rows


def breakeven_rows(T, S):
    """``[S, P]`` distinct dyadic rows.  With S >= 6 the first five are by hand: 2^-5 on every pillar; 0 exactly (L = 0);
    negative; b = -1 + 2^-20 on one pillar; a large b, with two pillars of equal L where T has 1 and 2 (1 ln 4 = 2 ln 2).  With
    fewer rows: a generic row, the zero row, and the row with -1 + 2^-20 (S >= 3)."""
    P = T.size
    s, k = np.arange(max(S, 6))[:, None], np.arange(P)[None, :]
    b = np.round((0.03 + 0.004 * np.sin(0.7 * k + 1.3 * s) + 0.0002 * s) * 2.0 ** 20) / 2.0 ** 20
    b[0] = 0.03125
    b[1] = 0.0
    b[2] = -0.0078125 - k[0] * 2.0 ** -10
    b[3, min(2, P - 1)] = TINY_B
    b[4, 0] = 3.0
    if P >= 3 and T[1] == 1.0 and T[2] == 2.0:
        b[4, 1], b[4, 2] = 3.0, 1.0
    if S >= 6:
        return b[:S].copy()
    return b[[5, 1, 3][:S]].copy()


GRID15 = YC.disc_grid()[0]                      # 15 knots from 0 to 50 years, 1.0 and 10.0 twice
GRID2 = np.array([0.0, 16.0])
GRID264 = 0.25 * np.arange(264)                 # with P = 64 the two tables need 171 080 bytes: the discount rows stay global


# ---------------------------------------------------------------------------------------------------------------- cases
def _case(name, times, T, S, swaps, sub_off, b=None):
    fixed, book, names = assemble(swaps)
    sub_off = np.asarray(sub_off, dtype=np.int64)
    assert sub_off[0] == 0 and sub_off[-1] == len(names) and np.all(np.diff(sub_off) >= 0) and np.any(np.diff(sub_off) == 0)
    return Case(name, times, discount_rows(times, S), T, breakeven_rows(T, S) if b is None else b, fixed, book, sub_off, names)


@lru_cache(maxsize=None)
def cases():
    """main: 65 scenario pairs, more than 64 swaps (a second chunk); the others three pairs."""
    main = tiling_swaps() + cancellation_swaps() + lookup_swaps(T8)
    pad = [swap(f"padding {j}", tiling(0.25 + j, 0.5, 2, 1e6, 0.0), [(1.0 + j, PAY)]) for j in range(max(0, 66 - len(main)))]
    main = main + pad
    n = len(main)
    passes, one, many, grid = pass_swaps(), lookup_swaps(np.array([2.0])) + tiling_swaps()[:3], lookup_swaps(T64), grid_swaps()
    b64 = breakeven_rows(T64, 3)
    return (_case("main", GRID15, T8, 65, main, [0, 0, 5, 40, 64, 64, n - 1, n]),
            _case("passes", GRID15, T8, 3, passes, [0, 3, 3, 9, len(passes)]),
            _case("one pillar, two knots", GRID2, np.array([2.0]), 3, one, [0, 0, 20, len(one)]),
            _case("64 pillars", GRID15, T64, 3, many, [0, 7, 7, len(many)]),
            _case("264 knots, 64 pillars: the global table", GRID264, T64, 3, grid, [0, 1, 1, len(grid)], b64),
            _case("264 knots, 5 pillars: the LDS table", GRID264, T5, 3, grid, [0, 1, 1, len(grid)], b64[:, 1:10:2].copy()))


# (label, discount rows, breakeven rows) of the main case: a shared row on one side, all 65 on the other
SHAPES = (("a shared discount row", slice(64, 65), slice(None)), ("a shared breakeven row", slice(None), slice(2, 3)))


def lds_bytes(K, P, table=True):
    """`yscen::lds_bytes`."""
    return 8 * (K + (P + 1) + (P + 1) * 64 + (K * 64 if table else 0))


def check_books():
    """The swaps' names, checked on their arrays."""
    from oracle.mp_oracle import _lookup_plan
    c = {case.name: case for case in cases()}
    main = c["main"]
    at = {name: i for i, name in enumerate(main.names)}
    tiles = lambda r: np.array_equal(r[1:, TS], r[:-1, TE])
    assert main.n > 64 and main.dfs.shape == (65, 15) and main.b.shape == (65, 8) and np.any(np.diff(main.times) == 0.0)
    assert list(main.sub_off[:6]) == [0, 0, 5, 40, 64, 64]
    r = main.coupons(at["a tiling annual leg, a fixed flow with every coupon"])
    assert tiles(r) and np.all(r[:, TP] == r[:, TE]) and np.array_equal(main.flows(0)[:, 0], r[:, TP])
    for name, dead in (("coupon 2 dead (tp == 0) before a coupon that starts on its end", 0.0),
                       ("coupon 2 dead (tp < 0) before a coupon that starts on its end, a fixed flow at |tp|", -1.0)):
        r, f = main.coupons(at[name]), main.flows(at[name])
        assert tiles(r) and r[2, TP] == dead and r[3, TS] == r[2, TE] and r[2, TS] != r[2, TE] and np.all(np.delete(r[:, TP], 2) > 0.0)
        assert f[2, 0] == abs(dead) and f[2, 1] != 0.0
    r = main.coupons(at["coupon 0 dead before a coupon that starts on its end"])
    assert r[0, TP] < 0.0 and r[1, TS] == r[0, TE] and r[1, TP] > 0.0
    r = main.coupons(at["coupon 2 has ts == te before a coupon that starts on its end"])
    assert r[2, TS] == r[2, TE] == r[3, TS] and r[2, TP] > 0.0 and r[1, TE] != r[2, TE]
    r = main.coupons(at["ts == te elsewhere, inserted in a tiling run"])
    assert r[3, TS] == r[3, TE] and r[4, TS] == r[2, TE] != r[3, TE] and tiles(np.delete(r, 3, axis=0))
    r = main.coupons(at["te < ts on coupon 1"])
    assert r[1, TE] < r[1, TS] and r[2, TS] != r[1, TE]
    r = main.coupons(at["te < ts on coupon 1 and coupon 2 starts on that end"])
    assert r[1, TE] < r[1, TS] and r[2, TS] == r[1, TE]
    i = at["coupon 0 starts at 3.25, the previous swap's last end"]
    assert main.coupons(i)[0, TS] == main.coupons(i - 1)[-1, TE] == 3.25
    i = at["fixed flows on the NEXT coupon's payment date"]
    assert np.array_equal(main.flows(i)[:5, 0], main.coupons(i)[1:, TP]) and not np.any(main.flows(i)[:, 0] == main.coupons(i)[:, TP])
    i = at["fixed flows on the PREVIOUS coupon's payment date"]
    assert np.array_equal(main.flows(i)[1:, 0], main.coupons(i)[:5, TP]) and not np.any(main.flows(i)[:, 0] == main.coupons(i)[:, TP])
    i = at["fixed flows one ulp beside the payment dates"]
    assert all(x in (np.nextafter(v, -9.0), np.nextafter(v, 9.0)) for x, v in zip(main.flows(i)[:, 0], main.coupons(i)[:, TP]))
    i = at["a payment lag, fixed flows on the coupons' ENDS"]
    assert np.array_equal(main.flows(i)[:, 0], main.coupons(i)[:, TE]) and np.all(main.coupons(i)[:, TP] > main.coupons(i)[:, TE])
    # cancellation: row 0 is 2^-5 everywhere, so a year between the pillars 1 and 2 has y = 2^-5 exactly
    assert np.all(main.b[0] == 0.03125) and np.all(main.b[1] == 0.0) and np.all(main.b[2] < 0.0) and main.b[3, 2] == TINY_B
    assert main.b[4, 0] == main.b[4, 1] == 3.0 and main.b[4, 2] == 1.0 and main.T[1] == 1.0 and main.T[2] == 2.0
    r = main.coupons(at["spread == -y on row 0"])
    assert (r[0, TS], r[0, TE]) == (1.0, 2.0) and r[0, SPREAD] == -main.b[0, 1]
    r = main.coupons(at["two coupons of opposite scale"])
    assert np.array_equal(r[0, :3], r[1, :3]) and r[0, SCALE] == -r[1, SCALE] != 0.0
    for name, sign in (("scale == 0.0 with live dates", False), ("scale == -0.0 with live dates, a dead fixed flow", True)):
        r = main.coupons(at[name])
        assert r[0, SCALE] == 0.0 and bool(np.signbit(r[0, SCALE])) == sign and r[0, TP] > 0.0 and r[0, TS] != r[0, TE]
    r = main.coupons(at["a period of one day"])
    assert 0.0 < r[0, TE] - r[0, TS] < 1.0 / 364
    assert main.coupons(at["no flows"]).size == 0 and main.flows(at["no flows"]).size == 0
    i = at["every flow dead"]
    assert main.coupons(i).size and main.flows(i).size and np.all(main.coupons(i)[:, TP] <= 0.0) and np.all(main.flows(i)[:, 0] <= 0.0)
    # the lookups, as `_lookup_plan` decides them on x = [0, T]
    for case in (main, c["one pillar, two knots"], c["64 pillars"]):
        x, d, P = np.concatenate(([0.0], case.T)), lookup_dates(case.T), case.T.size
        kinds = [_lookup_plan(x, float(t), 1) for t in d]
        assert kinds[0] == ("snap", 0) and kinds[1] == ("flat", 0) and kinds[2][:3] == ("interp", 0, 1) and kinds[3] == kinds[4] == kinds[5] == ("snap", 1)
        assert kinds[6][0] == "interp" or P == 1 and kinds[6] == ("flat", 1)
        assert kinds[7][:3] == ("interp", 0, 1) and kinds[9] == kinds[10] == ("snap", P) and kinds[11][:3] == ("interp", P - 1, P)
        assert kinds[12] == kinds[13] == kinds[14] == ("flat", P) and (P == 1 or kinds[8][:3] == ("interp", P // 2, P // 2 + 1))
        assert sum(n.startswith("ts = ") for n in case.names) == 32 and "all lookup coupons in one leg" in case.names
    # the passes and the unequal legs
    p = c["passes"]
    counts = [(p.flows(i).shape[0], p.coupons(i).shape[0]) for i in range(p.n)]
    assert counts[:8] == [(0, 63), (0, 64), (0, 65), (0, 128), (0, 129), (0, 65), (0, 65), (3, 129)]
    assert counts[8:24] == [(nf, nc) for nf in (0, 1, 65, 130) for nc in (0, 1, 64, 129)]
    for i in range(8):
        r = p.coupons(i)
        assert np.array_equal(r[1:, TS], r[:-1, TE]) or i in (6, 7)
    assert p.coupons(5)[63, TP] < 0.0 and p.coupons(5)[64, TS] == p.coupons(5)[63, TE]
    r = p.coupons(6)
    assert r[63, TS] == r[63, TE] == r[64, TS] and r[63, TP] > 0.0
    r = p.coupons(7)
    assert r[63, TS] == r[63, TE] == r[64, TS] and r[127, TP] == 0.0 and r[128, TS] == r[127, TE]
    f = p.flows(23)
    assert list(f[:129, 0] == p.coupons(23)[:, TP]) == [j % 2 == 0 for j in range(129)]
    # the two tables of the 264-knot grid: one leaves the LDS, one fits; identical flows on common pillars
    g, l = c["264 knots, 64 pillars: the global table"], c["264 knots, 5 pillars: the LDS table"]
    assert lds_bytes(264, 64) == 171080 > 160 * 1024 >= lds_bytes(264, 5) and lds_bytes(15, 64) <= 160 * 1024
    assert g.fixed[1] is not l.fixed[1] and np.array_equal(g.fixed[1], l.fixed[1]) and all(np.array_equal(g.book[k], l.book[k]) for k in g.book)
    common = set(l.T) | {0.0}
    live = g.book["ts"] != g.book["te"]
    assert set(g.book["ts"][live]) | set(g.book["te"][live]) <= common and set(l.T) <= set(g.T)
    assert np.array_equal(l.b, g.b[:, [int(np.flatnonzero(g.T == t)[0]) for t in l.T]])
    assert c["one pillar, two knots"].times.size == 2 and c["one pillar, two knots"].T.size == 1
    flows = sum(int(x.fixed[0][-1] + x.book["cpn_off"][-1]) for x in cases())
    assert flows < 4000, flows
