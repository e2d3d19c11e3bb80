"""Tables, the exact reference and the revaluation book shared by the delta-gamma P&L tests
(tests/test_ladder_pnl_host.py, CPU, and tests/test_gpu_ladder_pnl.py, GPU)."""
from fractions import Fraction
from functools import lru_cache

import numpy as np

from adrates_amd.market.curves.curve_tables import build_engine_curve

from . import _fixtures as F
from . import _sub_book_ladder_cases as L

VD = L.VD
SCHEMES = L.SCHEMES
TILE = 8                                    # desks per wave of the kernel (csrc/ladder_pnl.hip: kDesks); a block takes 8 tiles
PILLARS = (1, 2, 31, 32, 33, 64, 65, 256)
SCENARIOS = (1, 63, 64, 65, 129)
DESKS = (1, TILE - 1, TILE, TILE + 1, 8 * TILE - 1, 8 * TILE, 8 * TILE + 1)
# (P, S, B) of the tables held to exact arithmetic, every element: each P, each S, B around the desk tile, and B S about
# ten at P = 256.  The kernel takes every tile once (no loop over tiles), so there is no B beyond one pass of the grid.
EXACT_TABLES = ((1, 129, 9), (2, 65, 8), (31, 63, 1), (32, 1, 9), (32, 64, 1), (33, 2, 7), (64, 3, 2), (65, 1, 8), (256, 5, 2))
PARTS = ("pnl", "delta_pnl", "gamma_pnl")


def table(P, S, B, seed=0):
    """``(ladders [B, 1 + P + P P], shocks [S, P])``: both signs, magnitudes from 1e-3 to 1e8 log-uniform, gamma not
    symmetric (every entry drawn on its own), a PV slot that must not matter."""
    rng = np.random.default_rng([seed, P, S, B])
    draw = lambda *shape: 10.0 ** rng.uniform(-3.0, 8.0, shape) * rng.choice([-1.0, 1.0], shape)
    return draw(B, 1 + P + P * P), draw(S, P)


def split(ladders, P):
    return ladders[:, 1:1 + P], ladders[:, 1 + P:].reshape(-1, P, P)


def _ints(a):
    """``(integers, e)`` with ``a == integers * 2 ** e`` exactly (Python ints in an object array)."""
    a = np.asarray(a, dtype=np.float64)
    m, e = np.frexp(a)
    lo = int(e.min()) - 53
    m = (m * 2.0 ** 53).astype(np.int64)
    ints = np.array([int(mm) << (int(ee) - 53 - lo) for mm, ee in zip(m.ravel(), e.ravel())], dtype=object).reshape(a.shape)
    return ints, lo


def exact_element(delta, gamma, x):
    """One desk under one scenario in exact rational arithmetic: ``{part: (value, gross)}`` as Fractions, ``gross`` the
    sum of the absolute terms of that part."""
    (d, ed), (g, eg), (xi, ex) = _ints(delta), _ints(gamma), _ints(x)
    two = Fraction(2)
    scale_d, scale_g = two ** (ed + ex), two ** (eg + 2 * ex) / 2
    dv, dg = Fraction(int(d @ xi)) * scale_d, Fraction(int(abs(d) @ abs(xi))) * scale_d
    gv, gg = Fraction(int(xi @ g @ xi)) * scale_g, Fraction(int(abs(xi) @ abs(g) @ abs(xi))) * scale_g
    return {"pnl": (dv + gv, dg + gg), "delta_pnl": (dv, dg), "gamma_pnl": (gv, gg)}


@lru_cache(maxsize=None)
def exact_table(P, S, B):
    """The exact values and grosses of every element of ``table(P, S, B)``, computed once per process."""
    ladders, shocks = table(P, S, B)
    delta, gamma = split(ladders, P)
    return [[exact_element(delta[b], gamma[b], shocks[s]) for s in range(S)] for b in range(B)]


def worst_error(P, S, B, got):
    """The worst |got - exact| / ((P^2 + P + 8) 2^-53 gross) over the elements and the three parts: at most 1 under the
    bound, which is the worst case of ANY order of summing those terms with one rounding per operation."""
    ref = exact_table(P, S, B)
    unit = Fraction(P * P + P + 8, 2 ** 53)
    worst = 0.0
    for part in PARTS:
        for b in range(B):
            for s in range(S):
                value, gross = ref[b][s][part]
                err = abs(Fraction(float(got[part][b, s])) - value)
                worst = max(worst, float(err / (unit * gross)))
    return worst


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


# ------------------------------------------------------------------------------------------- against full revaluation
SUB_OFF = lambda n: np.array([0, 1, 120, 120, 310, 360, n, n], dtype=np.int64)
STEPS = (4.0, 8.0, 16.0)                                    # basis points


def desk_keys(n):
    """One key per trade for the desks ``SUB_OFF(n)``; the three empty desks hold no trade, so no key names them."""
    off = SUB_OFF(n)
    return [int(b) for b in np.repeat(np.arange(off.size - 1), np.diff(off))]


def directions(P):
    return (np.ones(P), np.random.default_rng(1).standard_normal(P), np.linspace(-1.0, 1.0, P))


def shock_rows(P):
    """``[10, P]`` basis points: ``h u`` for the three directions (rows 3 i + j: direction i, step j), then the zero shock."""
    return np.array([h * u for u in directions(P) for h in STEPS] + [np.zeros(P)])


def shocked_dfs(curve, shocks_bp):
    """``(times, dfs [S + 1, K])``: the host builder's curves on the shocked par rates, the base curve last."""
    rates = np.array(curve.swap_rates, dtype=np.float64)
    built = [build_engine_curve(list(rates + x * 1e-4), curve.swap_times, curve.year_fracs, with_hessian=False)
             for x in list(shocks_bp) + [np.zeros(rates.size)]]
    return built[0].times, np.stack([b.dfs for b in built])


def check_orders(full, delta_pnl, gamma_pnl, what):
    """The two bands of every desk (row) and direction on the columns of `shock_rows`: the residual of delta-gamma is
    third order (the ratio of doubled shocks is 8: in [7, 9]), that of delta alone second order (4: in [3, 5]), and the
    zero shock is exactly 0 in both routes.  Returns the observed ranges."""
    r, rd = full - (delta_pnl + gamma_pnl), full - delta_pnl
    assert np.all(full[:, 9] == 0.0) and np.all(delta_pnl[:, 9] == 0.0) and np.all(gamma_pnl[:, 9] == 0.0), what
    lo3 = hi3 = lo2 = hi2 = None
    for b in range(full.shape[0]):
        for i in range(3):
            for j in (0, 1):
                a, c = 3 * i + j, 3 * i + j + 1
                q3, q2 = r[b, c] / r[b, a], rd[b, c] / rd[b, a]
                assert 7.0 <= q3 <= 9.0, f"{what}: desk {b}, direction {i}, {STEPS[j]} -> {STEPS[j + 1]} bp: delta-gamma ratio {q3}"
                assert 3.0 <= q2 <= 5.0, f"{what}: desk {b}, direction {i}, {STEPS[j]} -> {STEPS[j + 1]} bp: delta-only ratio {q2}"
                lo3, hi3 = min(q3, lo3 or q3), max(q3, hi3 or q3)
                lo2, hi2 = min(q2, lo2 or q2), max(q2, hi2 or q2)
    print(f"{what}: delta-gamma ratio {lo3:.3f} - {hi3:.3f}, delta-only ratio {lo2:.3f} - {hi2:.3f}")
    return (lo3, hi3), (lo2, hi2)


def gbp(interp):
    model = F.gbp_model(VD, interp)
    return model, model.curves.GBP_OIS_SONIA
