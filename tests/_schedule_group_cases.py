"""Books for the schedule-group tests: hand-made swaps whose schedules, amounts and signs are chosen
trade by trade, and the recombination of a batch's ladders from its groups' basis ladders."""
import copy

import numpy as np

from adrates_amd.market.curves.curve_tables import build_engine_curve
from adrates_amd.market.position.scenarios import _concat_batches
from adrates_amd.trades import synthetic
from adrates_amd.trades.compiler import TradeBatch
from adrates_amd.utils import InterpTypes
from oracle import port

from . import _fixtures as F

VD = F.README_VALUE_DT
SCHEMES = [InterpTypes.LINEAR_ZERO_RATES, InterpTypes.FLAT_FWD_RATES, InterpTypes.LINEAR_FWD_RATES]
R = 16                                   # the store pass's default segment (records per wavefront)


def curve_arrays(interp, **kw):
    curve = F.gbp_model(VD, interp, **kw).curves.GBP_OIS_SONIA
    return build_engine_curve(curve.swap_rates, curve.swap_times, curve.year_fracs)


def swap(years, n_flt, n_fix, notional, coupon, spread=0.0, pay=False, bump=None):
    """One spot-starting swap of ``years`` years: ``n_flt`` float coupons, ``n_fix`` fixed coupons whose accruals are
    unequal in a way that depends on the schedule alone, so trades of one schedule have proportional - not equal - fixed
    payments.  ``bump``: (coupon index, factor) applied to one fixed payment."""
    edges = years * np.arange(n_flt + 1) / n_flt
    tau = years / max(n_fix, 1) * (1.0 + 0.01 * np.sin(1.0 + np.arange(n_fix)))
    fix_tp = years * np.arange(1, n_fix + 1) / max(n_fix, 1)
    pay_ = notional * coupon * tau
    if bump is not None:
        pay_[bump[0]] *= bump[1]
    s = -1.0 if pay else 1.0
    return TradeBatch(np.array([0, n_fix]), np.array([0, n_flt]), fix_tp, pay_, edges[1:].copy(), edges[:-1].copy(), edges[1:].copy(),
                      np.diff(edges), np.array([float(notional)]), np.array([float(spread)]), np.array([s]), np.array([-s]))


def group(size, years, n_flt, n_fix, seed, spread=0.0):
    """``size`` swaps of one schedule: random notionals and coupons, pay and receive."""
    rng = np.random.default_rng(seed)
    return [swap(years, n_flt, n_fix, float(np.round(rng.uniform(1e6, 5e7), -5)), float(rng.uniform(0.01, 0.07)), spread,
                 pay=bool(rng.random() < 0.5)) for _ in range(size)]


def edge_book(filler=3000):
    """The FORCE batch of the GPU test.  Returns ``(batch, marks)``; ``marks`` names the trades the test looks at."""
    pieces, marks = [], {}

    def add(name, trades):
        marks[name] = (len(pieces), len(pieces) + len(trades))
        pieces.extend(trades)

    # group sizes around the segment length, each on a schedule of its own (7 .. 13 annual coupons)
    for k, size in enumerate((1, 2, 3, R - 1, R, R + 1, 2 * R + 1)):
        add(f"size{size}", group(size, 7.0 + k + 0.37, 7 + k, 7 + k, seed=100 + k))
    # coupon counts: 1, 2, 30 and 32 coupons per leg group; 33 coupons make a chained trade, never grouped
    for m in (1, 2, 30, 32):
        add(f"coupons{m}", group(3, 0.9 * m if m > 2 else 0.4 * m, m, m, seed=200 + m))
    add("coupons33", group(2, 29.7, 33, 33, seed=233))
    # a semi-annual fixed leg against an annual float leg: the fixed coupons fall between the float nodes
    add("semi", group(5, 9.5, 10, 20, seed=300))
    add("spread", group(4, 6.25, 7, 7, seed=301, spread=0.0015))
    add("spread_other", group(2, 6.25, 7, 7, seed=302, spread=0.0025))
    # a zero-coupon member (a whole fixed leg of zeros), a member whose last payment alone is zero (never grouped), and a
    # member with one payment 1 % off the group's shape (never grouped)
    base = group(6, 11.6, 12, 12, seed=303)
    base[2] = swap(11.6, 12, 12, 2.3e7, 0.0)
    base[3] = swap(11.6, 12, 12, 1.7e7, 0.03, bump=(11, 0.0))
    base[4] = swap(11.6, 12, 12, 3.1e7, 0.04, pay=True, bump=(5, 1.01))
    add("mixed", base)
    # a group whose first trade is the zero-coupon one: the shape comes from the next member
    add("zero_first", [swap(4.8, 5, 5, 1.1e7, 0.0)] + group(3, 4.8, 5, 5, seed=304))
    book = _concat_batches(pieces)
    if filler:
        marks["filler"] = (book.n_trades, book.n_trades + filler)
        book = _concat_batches([book, synthetic.synthesize(VD, filler, kind="offgrid", seed=9)])
    return book, marks


def auto_book():
    """A batch that takes the route under AUTO with only some of its groups in use: 34 000 ongrid trades on 30 schedules
    (the groups of 64 trades and more), 3 000 offgrid trades on some 340 schedules (groups below 64, a few trades falling
    into the large ones) and the edge book.  The large groups' numbers lie scattered among the small ones', so a group's
    number among all groups and among those in use differ almost everywhere.  Returns ``(batch, marks)``, the marks those
    of `edge_book` moved to their place in this batch."""
    edge, marks = edge_book(filler=0)
    head = [synthetic.synthesize(VD, 3000, kind="offgrid", seed=9), synthetic.synthesize(VD, 34000, kind="ongrid", seed=11)]
    at = sum(b.n_trades for b in head)
    return _concat_batches(head + [edge]), {k: (lo + at, hi + at) for k, (lo, hi) in marks.items()}


def all_grouped_book():
    """40 schedules of 3 trades each and nothing else: under FORCE no plain row is left outside the groups."""
    return _concat_batches([t for k in range(40) for t in group(3, 5.37 + 0.5 * k, 5 + k % 7, 5 + k % 7, seed=400 + k)])


def tiny_books():
    """Batches of one or two blocks of the fast row launch (24 rows per block), by name: ``one_block_one_outside`` - 4
    trades of one schedule and one of another; ``one_block_all_grouped`` - 3 trades of one schedule; ``two_blocks`` - 2
    trades of one schedule and 46 on a schedule of their own each."""
    singles = [group(1, 3.21 + 0.53 * k, 3 + k % 9, 3 + k % 9, seed=600 + k)[0] for k in range(46)]
    return {"one_block_one_outside": _concat_batches(group(4, 6.37, 6, 6, seed=500) + group(1, 4.61, 5, 5, seed=501)),
            "one_block_all_grouped": _concat_batches(group(3, 7.37, 7, 7, seed=502)),
            "two_blocks": _concat_batches(group(2, 9.37, 9, 9, seed=503) + singles)}


def many_groups_book(groups=4100):
    """``groups`` groups of 2 on one schedule, told apart by their spreads."""
    return _concat_batches([t for k in range(groups) for t in group(2, 8.37, 8, 8, seed=k, spread=1e-7 * k)])


def no_group_book():
    """5 trades on 5 schedules: nothing to group."""
    return _concat_batches([group(1, 4.4 + k, 4 + k, 4 + k, seed=700 + k)[0] for k in range(5)])


def short_curve_quotes(P):
    """The README quotes at 1Y, 2Y, ..., 8Y (``P`` = 8) or 9Y (``P`` = 9): ``(px, tenors)``."""
    idx = [14] + list(range(16, 15 + P))
    return [F.GBP_PX[i] for i in idx], [F.TENORS[i] for i in idx]


def flipped(b):
    out = copy.deepcopy(b)
    out.fix_sign, out.flt_sign = -b.fix_sign, -b.flt_sign
    return out


def doubled(b):
    out = copy.deepcopy(b)
    out.fix_pay, out.notional = 2.0 * b.fix_pay, 2.0 * b.notional
    return out


def recombined(method, host, group_of, cF, cX, basis):
    """The grouped trades' ladders from the basis trades' (priced by the C oracle): rows of the ungrouped trades are NaN."""
    tb = TradeBatch(**{k: v for k, v in basis.items() if k != "n_trades"})
    ref = port.price(method, host.times, host.dfs, host.jac, host.hess, tb)
    out = {}
    g = np.where(group_of >= 0, group_of, 0)
    for key in ("pv", "delta", "gamma"):
        b = ref[key].reshape(tb.n_trades, -1)
        rows = cF[:, None] * b[2 * g] + cX[:, None] * b[2 * g + 1]
        rows[group_of < 0] = np.nan
        out[key] = rows.reshape((len(g),) + ref[key].shape[1:])
    return out
