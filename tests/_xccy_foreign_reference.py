"""The plain reference of the two-curve foreign-leg launch (`adr_price_xccy_foreign`, `adr_price_xccy_foreign_dev`: the XC
instantiations of `price_lite_kernel`, csrc/kernels_lite.hip) and the bound the kernel is held to, element by element
(tests/test_xccy_foreign_host.py, CPU, and tests/test_gpu_xccy_foreign.py, GPU).  Built on tests/_ladder_reference.py: its
`_Curve` (D(t) on `oracle.mp_oracle._lookup_plan`'s float64 decisions, in mpmath at 60 digits), its terms, its exact-integer
projection and its `Block`.  It shares no code with the kernel.

The operation (include/adrates.h).  Two host curves - the foreign OIS curve (scheme, times, dfs, jac J_f [K_f, P_f]) gives
D_f(t), the XCCY curve (scheme, times, dfs, jac J_x [K_x, P_x]) gives D_x(t) - and a `TradeBatch`, weights included.  Per trade
  fixed flow, counts when xt > 0:     fix_sign pay D_x(xt)
  coupon, counts when tp >= 0:        flt_sign N w ((D_f(ts) / D_f(te) - 1 when alpha > 0, else 0) + spread alpha) D_x(tp)
  pv             the sum of these
  delta_foreign  = 1e-4 LJ_f^T g_f,  g_f = d pv / d L_f from the ratio D_f(ts) / D_f(te) only, the XCCY curve held fixed
  delta_basis    = 1e-4 LJ_x^T g_x,  g_x = d pv / d L_x from every D_x factor, the foreign curve held fixed
with L = ln d the knots' log discount factors and LJ = J / d.  The terms are those of `_ladder_reference.trade_terms`, the ratio
term split over the two tables: with c = flt_sign N w an accruing coupon is  c R D_x(tp),  -c D_x(tp)  and  c spread alpha D_x(tp),
R = D_f(ts) / D_f(te).  The first, om = c R D_x(tp), is the only term the foreign rates move: under a log scheme
g_f,k += om u_k with u = b(ts) - b(te) the merged knot weights; under LINEAR_FWD_RATES the reduced first-order form
d ln F / d ln d_k on each table, g_f,k += om (s_k d_k / S - e_k d_k / E).  On the XCCY table all three are plain terms c' D_x(tp)
of `_Sums.add`.  The projection is `_Sums._project`'s exact integer arithmetic; 1e-4 stays exact.

Gross (the conventions of tests/_ladder_reference.py and tests/_xccy_scenario_reference.py): the terms as written, absolute
weights before the merge - |om| (|b(ts)|_k + |b(te)|_k) on the foreign table, so a two-day accrual inside one interval counts
b(ts) - b(te) as cancellation against gross - and |N w| (R + 1 + |spread alpha|) D_x for an accruing coupon on pv and on the
XCCY table; the tables as |J| / d.  An element with gross 0 must be +0.0: a coupon paid AT the value time (tp = 0) has foreign
sensitivity and no basis sensitivity (D_x(0) = 1 sits on the value-time knot, whose Jacobian row is zero), a trade with
nothing live has pv +0.0.

The bound |got - value| <= k 2^-53 gross.  The conventions are tests/_price_reference.py's: one rounding is ONE unit 2^-53 of
the absolute sum it acts on, a contracted FMA counts as its unfused pair, the device's exp and log (one ulp) as TWO units; one
k serves every element of a trade.  The lite kernel forms a lookup's w as (tau - x_a) inv_dx (INV_DX), so a weight costs
e_w' = e_w + ceil(3 wr) with e_w = 1 (FLAT_FWD, LINEAR_FWD: 1 - w) or 4 (LINEAR_ZERO: t (1 - w) inv_x) and wr what an absolute
error of w does to the lower knot's weight in units of the gross (`_price_reference._amplification`, here without the gamma
entries: the launch has none).  Both are PER TABLE - e_f' from the trade's ts and te on the foreign curve, e_x' from its tp and
xt on the XCCY curve -, and so is cond: cond_f the largest |weight L|(ts) + |weight L|(te) of an accruing coupon, cond_x the
largest |weight L| of a payment or exchange date (LINEAR_FWD_RATES: the largest |L_k| on each table).  n is the trade's
unfolded live terms.  As the XC branch performs them, log schemes:
  lookups   `factor()`: fma(ba, L_a, bb L_b) - L from the table builder's log (2), the weight (e'), the product, the sum:
            (e' + 4) of its own |weight L|, on each table
  R         ls - le (1): cond_f (e_f' + 5) as a relative error of exp(ls - le); exp (2)          ceil(cond_f (e_f' + 5)) + 2
  dx        exp(lp) (2) on the XCCY lookup                                                       ceil(cond_x (e_x' + 4)) + 2
  w_not     sl N cw                                                                                                        2
  amount    (R - 1) (1) + spread al (1, 1), times w_not (1); the fma of a merged exchange (1); the product with dx (1)     6
            against |c| (R + 1 + |spread alpha|) D_x, which holds R's and dx's own errors
  om_r      w_not dx R: two products - fewer than the amount's line
                                                  node = 10 + ceil(cond_f (e_f' + 5)) + ceil(cond_x (e_x' + 4))
  entries   foreign: om_e = next_om - om_r (1; both are terms of the gross), times the weight (e_f' + 1), fma(c, LJ, d): the
            table's LJ = J / d (1) and the product (1): e_f' + 4.  The start's om_r b(ts) has one fewer.  A chained start takes
            the previous lane's L(te), the spare lane looks the row's first start up itself: the same numbers a lookup of
            their own gives.  Basis: om_b times the weight (e_x' + 1), LJ and the product (2): e_x' + 3; an exchange on a
            date of its own is qa exp() with qa = sf xpay: fewer than a coupon's        entry = max(e_f' + 4, e_x' + 3)
  sums      pv: one add per node and row_sum's four: any order of m numbers costs m - 1 roundings, m <= n.  Foreign ladder:
            a ratio term leaves at most four entries (its start's two, its end's two) into d0 / e0 and an accruing coupon
            has at least two terms: 2 n.  Basis ladder: two entries per node, at most n nodes: 2 n.  d + e (1), 1e-4: the
            constant and the product (2)                                                                         2 n + 3
                                                                          k = node + entry + 2 n + 3          [log schemes]
LINEAR_FWD_RATES (both tables; `factor()` returns F = ba D_a + bb D_b and replaces the weights by g = (ba D_a, bb D_b) / F):
  factor    a part ba exp(L_a): the table's log under exp (2 cond), exp (2), the weight (e'), the product: e' + 2 cond + 3;
            F one more: e' + 2 cond + 4;  inv = 1 / F and g = part inv: 2 e' + 4 cond + 9
  R         ls / le: two factors and the division: 2 e_f' + 4 cond_f + 9;   dx = lp: e_x' + 2 cond_x + 4
  w_not 2, amount 6 as above            node = 2 e_f' + e_x' + ceil(4 cond_f) + ceil(2 cond_x) + 21
  entries   foreign: the difference (1), times g_f, LJ and the product (2): 2 e_f' + 4 cond_f + 13; basis: om_b g_x, LJ and the
            product: 2 e_x' + 4 cond_x + 12                                   entry = the larger, the conds rounded up
                                                                          k = node + entry + 2 n + 3
The aggregates (`block_partials`, `block_partials2`, `reduce_partials_kernel`): a wave adds its trades' numbers (at most
n_trades - 1 adds over all waves), its four groups by two shuffles (2), the block its twelve waves in order (11), the reduction
strides over the blocks (ceil(blocks / 64) - 1) and runs its butterfly (6):   sums = n_trades + 17 + ceil(blocks / 64),
and an element of the book is held to `_price_reference.book_k`: ceil(sum_t k_t gross_t / gross_book) + sums.
Nothing in k is fitted to a result.  On the edge books k runs from 21 to about 100 for a trade whose dates sit well inside
their intervals and to 8 700 for an accrual end a few days before a knot forty years out (w / (1 - w) = 731: its wr, times
cond_f = 2.9).  The GPU module prints the worst share it observes;
on an MI355X the worst over all cases was 0.198 under the log schemes and 0.065 under LINEAR_FWD_RATES per trade, 0.028 in the
aggregates (tests/test_gpu_xccy_foreign.py has the shares per scheme pair).
"""
import math

import numpy as np
from mpmath import mp, mpf

from oracle.mp_oracle import _lookup_plan

from . import _ladder_reference as R
from . import _price_reference as PR

FLAT_FWD, LINEAR_FWD, LINEAR_ZERO = R.FLAT_FWD, R.LINEAR_FWD, R.LINEAR_ZERO
E_W = PR.E_W
BLOCKS = ("pv", "delta_foreign", "delta_basis")
_bump = lambda table, key, v: table.__setitem__(key, table.get(key, mpf(0)) + v)


def _coupons(batch, i):
    """Trade i's live coupons ``(ts, te, tp, accrues, c, c spread alpha)`` and live fixed flows ``(xt, amount)``, mpf amounts."""
    fixed = []
    for j in range(int(batch.fix_off[i]), int(batch.fix_off[i + 1])):
        xt = float(batch.fix_tp[j])
        if xt > 0.0:
            fixed.append((xt, R._mp(batch.fix_sign[i]) * R._mp(batch.fix_pay[j])))
    sn = R._mp(batch.flt_sign[i]) * R._mp(batch.notional[i])
    coupons = []
    for j in range(int(batch.flt_off[i]), int(batch.flt_off[i + 1])):
        tp, ts, te, al = (float(getattr(batch, name)[j]) for name in ("flt_tp", "flt_ts", "flt_te", "flt_alpha"))
        if not tp >= 0.0:
            continue
        c = sn if batch.flt_weight is None else sn * R._mp(batch.flt_weight[j])
        coupons.append((ts, te, tp, al > 0.0, c, c * R._mp(batch.spread[i]) * R._mp(al)))
    return fixed, coupons


def _add_trade(F, X, sf, sx, batch, i):
    """Trade i's terms into the foreign sums ``sf`` (g only) and the XCCY sums ``sx`` (pv and g); returns its live terms."""
    fixed, coupons = _coupons(batch, i)
    n = 0
    for xt, amount in fixed:
        if amount != 0:
            sx.add(xt, amount)
            n += 1
    for ts, te, tp, accrues, c, csa in coupons:
        if c == 0:
            continue
        if accrues:
            (Ds, ks, ps, _), (De, ke, pe, _) = F.date(ts), F.date(te)
            q = Ds / De
            sx.add(tp, c * q)                                   # c R D_x(tp): every D_x factor moves the basis ladder
            sx.add(tp, -c)
            n += 2
            Dp, _, pp, _ = X.date(tp)
            om = c * q * Dp
            oa = abs(c) * q * (Dp if pp is None else sum((abs(p) for _, p in pp), mpf(0)))
            if ps is not None:                                   # LINEAR_FWD_RATES: d ln F / d ln d_k, the reduced first-order form
                for sg, D, pieces in ((1, Ds, ps), (-1, De, pe)):
                    for k, p in pieces:
                        _bump(sf.g, k, sg * om * p / D)
                        _bump(sf.g_abs, k, oa * abs(p) / D)
            else:
                u, W = {}, {}
                for sg, knots in ((1, ks), (-1, ke)):
                    for k, wk in knots:
                        _bump(u, k, sg * wk)
                        _bump(W, k, abs(wk))
                for k in u:
                    _bump(sf.g, k, om * u[k])
                    _bump(sf.g_abs, k, oa * W[k])
        if csa != 0:
            sx.add(tp, csa)
            n += 1
    return n


def reference(for_method, host_f, x_method, host_x, batch, sub_off):
    """Per desk ``{"pv", "delta_foreign" [P_f], "delta_basis" [P_x]: Block, "n_terms"}``.  Built once per process for the same
    inputs."""
    sub_off = np.asarray(sub_off, dtype=np.int64)

    def build():
        mp.dps = 60
        F = R._Curve(for_method, host_f.times, host_f.dfs, host_f.jac, None)
        X = R._Curve(x_method, host_x.times, host_x.dfs, host_x.jac, None)
        tf, tx = R._tables(F), R._tables(X)
        desks = []
        for lo, hi in zip(sub_off[:-1], sub_off[1:]):
            sf, sx = R._Sums(F, False), R._Sums(X, False)
            n = sum(_add_trade(F, X, sf, sx, batch, i) for i in range(int(lo), int(hi)))
            pv, basis, _ = sx.blocks(tx)
            _, foreign, _ = sf.blocks(tf)
            desks.append({"pv": pv, "delta_foreign": foreign, "delta_basis": basis, "n_terms": n})
        return desks
    extra = (np.array([int(x_method)]), host_x.times, host_x.dfs, host_x.jac, sub_off)
    return R._cached("xccy foreign", for_method, host_f, batch, extra, build)


def per_trade_reference(for_method, host_f, x_method, host_x, batch):
    return reference(for_method, host_f, x_method, host_x, batch, np.arange(batch.n_trades + 1, dtype=np.int64))


def book_reference(for_method, host_f, x_method, host_x, batch):
    return reference(for_method, host_f, x_method, host_x, batch, np.array([0, batch.n_trades], dtype=np.int64))[0]


# ---------------------------------------------------------------------------------------------------------------- the bound
def _table_stats(method, host, dates_of):
    """Per trade ``(cond, wr)`` on one table; ``dates_of(i)`` yields the groups of dates whose conds add (a coupon's ts and
    te) - read off the inputs alone."""
    method = int(method)
    cv = R._Curve(method, host.times, host.dfs, host.jac, None)
    x, d = cv.x, np.asarray(host.dfs, dtype=np.float64)
    A = np.abs(np.asarray(host.jac, dtype=np.float64)) / d[:, None]
    L = np.abs(np.log(d))
    seen = {}

    def amp(t):
        if t not in seen:
            plan = _lookup_plan(x, t, method)
            out = 1.0
            if plan[0] == "interp" and 0.0 < float(plan[3]) < 1.0:
                _, a, b, w = plan
                w = float(w)
                if method == LINEAR_FWD:
                    wa, wb, La, Lb = (1.0 - w) * d[a], w * d[b], (1.0 - w) * d[a], w * d[b]
                elif method == LINEAR_ZERO:
                    wa, wb = t * (1.0 - w) / max(x[a], 1e-15), t * w / max(x[b], 1e-15)
                    La, Lb = abs(wa) * L[a], abs(wb) * L[b]
                else:
                    wa, wb, La, Lb = 1.0 - w, w, (1.0 - w) * L[a], w * L[b]
                out = max(1.0, PR._amplification(w / (1.0 - w), abs(wa), abs(wb), A[a], A[b], None, None, La, Lb))
            seen[t] = out
        return seen[t]

    def stats(i):
        cond, wr = 0.0, 1.0
        for group in dates_of(i):
            conds = [float(cv.date(t)[3]) for t in group]
            cond = max(cond, max(conds) if method == LINEAR_FWD else sum(conds))
            wr = max(wr, max(amp(float(t)) for t in group))
        return cond, wr
    return stats


def trade_stats(for_method, host_f, x_method, host_x, batch):
    """Per trade ``{"n", "cond_f", "wr_f", "cond_x", "wr_x"}`` (module docstring), from the inputs alone."""
    def build():
        mp.dps = 60
        live = [_coupons(batch, i) for i in range(batch.n_trades)]
        f_stats = _table_stats(for_method, host_f, lambda i: [(ts, te) for ts, te, _, acc, c, _ in live[i][1] if acc and c != 0])
        x_stats = _table_stats(x_method, host_x, lambda i: [(xt,) for xt, a in live[i][0] if a != 0] +
                               [(tp,) for _, _, tp, acc, c, csa in live[i][1] if c != 0 and (acc or csa != 0)])
        out = []
        for i, (fixed, coupons) in enumerate(live):
            n = sum(1 for _, a in fixed if a != 0) + sum((2 if acc else 0) + (1 if csa != 0 else 0) for *_, acc, c, csa in coupons if c != 0)
            (cf, wf), (cx, wx) = f_stats(i), x_stats(i)
            out.append(dict(n=n, cond_f=cf, wr_f=wf, cond_x=cx, wr_x=wx))
        return out
    extra = (np.array([int(x_method)]), host_x.times, host_x.dfs, host_x.jac)
    return R._cached("xccy foreign stats", for_method, host_f, batch, extra, build)


def trade_k(for_method, x_method, st):
    """k of one trade (module docstring)."""
    fm, xm = int(for_method), int(x_method)
    assert (fm == LINEAR_FWD) == (xm == LINEAR_FWD), "both curves on LINEAR_FWD_RATES or neither"
    ef, ex = E_W[fm] + math.ceil(3 * st["wr_f"]), E_W[xm] + math.ceil(3 * st["wr_x"])
    cf, cx, n = st["cond_f"], st["cond_x"], st["n"]
    if fm == LINEAR_FWD:
        node = 2 * ef + ex + math.ceil(4 * cf) + math.ceil(2 * cx) + 21
        entry = max(2 * ef + math.ceil(4 * cf) + 13, 2 * ex + math.ceil(4 * cx) + 12)
    else:
        node = 10 + math.ceil(cf * (ef + 5)) + math.ceil(cx * (ex + 4))
        entry = max(ef + 4, ex + 3)
    return node + entry + 2 * n + 3


def case_ks(for_method, host_f, x_method, host_x, batch):
    return [trade_k(for_method, x_method, st) for st in trade_stats(for_method, host_f, x_method, host_x, batch)]


def aggregate_sums(n_trades, blocks):
    """The adds between the trades' numbers and an aggregate's element (module docstring)."""
    return n_trades + 17 + -(-max(blocks, 1) // 64)


def rows_share(got, ref, ks, what, rows=None):
    """The worst share of the bound over the per-trade blocks ``got`` holds, trade by trade on its own k."""
    worst = 0.0
    for i in (range(len(ref)) if rows is None else rows):
        for name in BLOCKS:
            if name in got:
                g = np.asarray(got[name][i])
                worst = max(worst, ref[i][name].share(g.reshape(ref[i][name].V.shape), ks[i], f"{what} trade {i} {name}"))
    return worst


def book_share(got, ref, book, ks, sums, what, names=BLOCKS):
    """The worst share of the aggregates' blocks ``names`` (``got[name]``) against the one-desk row on `book_k`."""
    worst = 0.0
    for name in names:
        g = np.asarray(got[name], dtype=np.float64)
        worst = max(worst, PR.share_elems(book[name], g, PR.book_k(ref, book, ks, name, sums), f"{what} agg {name}"))
    return worst


def rational(block, idx=()):
    """``(value, gross)`` of one element as exact `Fraction`s."""
    from fractions import Fraction
    unit = Fraction(2) ** block.E / 10 ** block.s
    return int(block.V[idx]) * unit, int(block.A[idx]) * unit
