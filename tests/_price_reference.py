"""The bound the per-trade pricing kernels (`adr_price`: kernels_fast.hip, kernels_fast_lindf.hip, kernels_general.hip,
kernels_lite.hip, kernels_knot.hip) are held to, element by element, on trades whose accruing coupons are paid on their accrual
end: on one pillar tile (tests/test_price_edges_host.py, CPU, and tests/test_gpu_price_edges.py, GPU) and on the wide and tiled
routes of 33 to 97 pillars (tests/test_price_wide_host.py and tests/test_gpu_price_wide.py; the families `wide` and `tiled`);
and, on one pillar tile, on trades with payment lag and per-coupon weights (tests/test_price_lag_host.py and
tests/test_gpu_price_lag.py; "Payment lag and weights" below).

The value and the gross of every element are `_ladder_reference.rates_reference`'s: per trade with ``sub_off = arange(n + 1)``,
for the aggregate the one-desk row ``[0, n]``.  What is derived here is k of  |got - value| <= k 2^-53 gross  per kernel family,
because the pricing kernels do other arithmetic than the ladder kernels `bound_k` counts.  The conventions are the same: one
rounding is ONE unit 2^-53 of the absolute sum it acts on, a contracted FMA counts as its unfused pair, the device's exp and log
(one ulp) as TWO units; one k serves every element of a trade (pv and delta have fewer roundings than gamma).  Three numbers are
read off the inputs per trade (`trade_stats`), none off a result:
  n      the trade's unfolded live terms (a kernel's nodes are sums of terms, so it has at most n nodes)
  cond   the largest sum |weight L_k| of a term (LINEAR_FWD_RATES: the largest |L_k|), as in `bound_k`
  wr     what an absolute error of w does to the lower knot's weight 1 - w, in units of the gross: over the trade's two-knot
         lookups the largest of  w / (1 - w)  times the lower knot's share of an element's gross (`_amplification`: the share is
         small where both knots move the same pillars, and 1 where the lower knot alone moves one); at least 1

The weight e_w (curve_lookup.hpp, `curve_lookup_at`; w is the plan's float64 number, the same expression):
  FLAT_FWD 1 - w: 1;  LINEAR_FWD 1 - w: 1;  LINEAR_ZERO t (1 - w) inv_x: inv_x = 1 / x is a rounded table entry (1), 1 - w,
  two products: 4.
  The lite kernel and the knot pass (INV_DX) form w as (tau - x_a) inv_dx, not by the division: inv_dx (1), the product (1) and
  the reference's own quotient (1) part the two w by 3 units of w, and 1 - w turns them into 3 w / (1 - w) units of the lower
  knot's weight, 3 wr of the gross:                                                                               e_w' = e_w + ceil(3 wr)

The node (every family; kernels_fast.hip "fold the coupons into nodes", the same lines in kernels_lite.hip and
kernels_general.hip):
  amount    sl N (spread al - 1): 3; the next coupon's start joined: 1; the fixed flow by fma: 1                            5
  argument  fma(ba, L_a, bb L_b): L from the table builder's log (2), the weight (e_w), a product, the sum: cond (e_w + 4)
  exp       2;  omega = amount exp(): 1                                                                                   3
  LINEAR_FWD_RATES (fast, lite, knot): the knot's amount qa ba exp(L_a): exp's argument is the table's log: 2 cond; exp 2; the
  weight e_w and two products                                                                     5 + 2 cond + 4 + e_w
                                                                               node = 8 + ceil(cond (e_w + 4))  [log schemes]

fast, fast_chained (kernels_fast.hip, the walk; gamma is the worst element):
  v = fma(wb, ub, wa ua): a Jacobian entry LJ = J / d (1), the weight (e_w), the product, the add: e_w + 3 of |wa ua| + |wb ub|
  rank-one  fma(om u_i, v_q, acc): v twice, om u_i (1), the product (1)                                          2 e_w + 8
  convexity fma(coa, LC, acc): coa = om wa (e_w + 1) [+ the carried right-knot weight: 1], a packed row entry is a copy of LC
            (4, `bound_k`'s "tables"), the product: e_w + 7 of its own gross - less than the line above, as is a short-end
            record's coef lc[j]
  sums      an entry takes at most three adds per node (the rank-one term and two rows, or a row and a short-end number)    3 n
  scale     acc 1e-8: the constant (1), the product (1)                                                                   2
                                                                                       k = node + 2 e_w + 10 + 3 n
  LINEAR_FWD_RATES (kernels_fast_lindf.hip): coa = amount + carry (1), coa u_i (LJ 1 + 1), times u_q (LJ 1 + 1): 5; coa LC: 6;
  two knots per node, a rank-one term and a row each: 4 n                             k = 9 + e_w + ceil(2 cond) + 8 + 4 n

general (kernels_general.hip, `add_nodes`; both variants - the LDS-resident rows add one final add per entry):
  log schemes: v = fma(bb_i, lj_i, v): e_w + 3; vr = om v (1), fma(vr, vc): 2 e_w + 8; coef = om bb (e_w + 1), the tile (4), the
  product; three adds per node, the merge of the flat convexity sums (1)               k = node + 2 e_w + 10 + 3 n + 1
  LINEAR_FWD_RATES: a plain node is walked as two single-knot nodes of amounts a (1 - w) d_a and a w d_b (`lindf_plain`; the
  node of the fast kernels above): v is the knot's Jacobian row itself (1), vr = om v (1), fma(vr, vc) (LJ 1 + 1): 4; the
  amount times the tile: 5; a rank-one term and a row per knot: 4 n, the merge        k = 9 + e_w + ceil(2 cond) + 8 + 4 n + 1
  (Until this bound was applied the kernel priced such a node in the form of its ratio nodes, om (v v^T + rho_a rho_b
  (LJ_a - LJ_b)(LJ_a - LJ_b)^T) on the shares rho of D: the cross products rho_a rho_b LJ_a,p LJ_b,q of the two parts cancel
  only up to rounding, and a date between two short-end knots that move different pillars left 1e-21 to 1e-24 on gamma
  entries no term reaches.  tests/test_gpu_price_edges.py found it on the legs of 385, 400 and 450 coupons.)

wide (kernels_general.hip, `add_nodes_wide`, the WIDE result block; 33-64 pillars, tests/test_gpu_price_wide.py): the node is
  built by the lines the general kernel runs; gamma, the packed upper triangle, is the worst element:
  v = fma(bb_i, lj64_i, v), lane p on pillar p: a Jacobian entry (1), the weight (e_w), the product, the add            e_w + 3
  the hand-off holds v and om v (1); rank-one fma(wa.x, vb, acc): (om v_a) v_b - v twice, om v (1), the product (1)  2 e_w + 8
  convexity fma(cc_0, la, fma(cc_1, lb, acc)): cc = om bb (e_w + 1), a packed row entry is a copy of LC (4), the product:
            e_w + 6 of its own gross, less than the line above; a chunk the mask skips holds zeros for both knots (no rounding)
  sums      the rank-one add and one add per knot's row                                                                    3 n
  scale     g = acc 1e-8 (the constant, the product) on its way to the staging area; `flush_gamma` and `wide_store_map` copy  2
  no merge: the rows are added straight into the packed registers               k = node + 2 e_w + 10 + 3 n  (`general` less 1)
  LINEAR_FWD_RATES: `lindf_plain` walks the two single-knot nodes with b = (1, 0): v = fma(0, lj, fma(1, lj_k, 0)) is the
  Jacobian entry itself (1), om v (1), the product with v_b (1 + 1): 4; cf LC: 5; a rank-one term and a row per knot: 4 n
                                                                                     k = 9 + e_w + ceil(2 cond) + 8 + 4 n
  pv (wave_sum: 6 adds and one per 64 coupons) and delta (fma(om, v, acc): e_w + 4, n adds, 1e-4: 2) stay below gamma's count.
  The delta-only and PV-only instantiations (masks 3 and 1, the trades outside the lite table) run the same lines.

tiled (more than 64 pillars or PILLAR_TILES: `price_general_kernel` without WIDE, rows streamed from L2, one launch per tile
  pair): `add_nodes` with the row tile's v in lanes 0-31 and the column tile's in lanes 32-63 of the hand-off buffer - the
  arithmetic of an element is that of `general`'s L2 variant, whichever launch writes it (pv: tile (0, 0); delta: the diagonal
  launches; an off-diagonal tile and its mirror: one launch, one number)                                       k = `general`'s

lite (kernels_lite.hip, `sweep`; PV and delta): ca = omega ba (e_w' + 1), fma(ca, LJ, d): LJ (1), the product (1); a node
  leaves two entries: 2 n adds, d0 + e0 (1), 1e-4 (2)                                  k = node' + e_w' + 6 + 2 n
  (node' = the node with e_w'; LINEAR_FWD_RATES likewise with its node)

knot (kernels_lite.hip KNOT instantiations, kernels_knot.hip; the book's aggregate): a trade's part of the sums w_k += ca,
  D_k += ca ba, O_k += ca bb holds a product more than its node (ca ba: 2 e_w' + 2); the projection: fma(dk ap, aq, s) - two
  Jacobian entries (2), two products (2); the band term ok fma(ap, bq, bp aq): 2 + 2 + 1 against the same two-knot gross, one
  more: 2 e_w' + 7; wk LC: e_w' + 1 + 4 + 1                                            k_t = node' + 2 e_w' + 7  per trade
  and the sums: a wave's table takes at most N adds (N = the unfolded terms of all the pass's trades), the block sums its 8
  waves (7), `knot_reduce_kernel` strides over the blocks and runs a butterfly (ceil(blocks / 64) - 1 + 6); three adds per knot
  of a projection wave's share ceil(Kc / 16), fifteen adds of the waves' sums, agg += (1), 1e-8 (2)
                             sums = N + 7 + ceil(blocks / 64) + 5 + 3 ceil(Kc / 16) + 18

Payment lag and weights (tests/_price_lag_cases.py, tests/test_price_lag_host.py and tests/test_gpu_price_lag.py; one pillar tile).
A coupon paid on another date than its accrual end is the RATIO node c D(ts) D(tp) / D(te), c = sl N w, plus the payment node
-c (1 - spread al) D(tp); the reference has its terms (tests/_ladder_reference.py, "Ratio terms").  `trade_stats` reads two
more numbers off the inputs: ``ratio``, the trade's ratio terms, and ``cond_lag``, the largest |L(ts)| + |L(te)| + |L(tp)| in
weighted-knot form over the trade's accruing coupons, te == tp included - the payment-lag variants of the fast and lite
kernels and the knot pass form exp(L(ts) - L(te) + L(tp)) for every accruing coupon of their rows (where te == tp the folded
weights -b(te) + b(tp) are exactly 0: the same two numbers).  ``cond`` of a ratio term is that sum too (LINEAR_FWD_RATES: the
largest |L_k|).  The node of a payment-lag family under a log scheme:
  amount    c = sl N w: 2; the payment node's c (spread al - 1): 3 more, the fixed flow by fma: 1                          6
  argument  three lookups fma(ba, L_a, bb L_b), each (e_w + 4) of its own |weight L|; their signed sum: 2 adds (fast, lite,
            knot: ls - le + lp) or the one fma chain over the six knots, 5 adds and no separate lookups (general: e_w + 3
            per product and 5) of the whole sum cond                                    cond (e_w + 6)  /  cond (e_w + 8)
  exp       2;  omega = c exp(): 1                                                                                        3
                                                                         node_lag = 9 + ceil(cond (e_w + 6 or 8))

fast_lag, fast_lag_chained (kernels_fast.hip, LAG: the chunk passes and the date record):
  v         a record's fma(wb, ub, wa ua): LJ (1), the weight (e_w) - the date record's has the accrual end's folded in,
            ba -= e_ba (1) -, the product, the add: e_w + 4; vacc takes the start's and the end's (2), v1 = vacc + vr (1)
                                                                                                                  e_w + 7
  rank-one  fma(om u_i, v_q, acc): v twice, om u_i (1), the product (1)                                        2 e_w + 16
  convexity coef = fma(om, wa, fma(om_p, wpa, om_s wsa)): the weight (e_w + 1), three products and two adds, the carried
            weight (1), a packed row entry (4), the product: e_w + 12 of its own gross - less than the line above
  special   a node without a packed entry for (r, c) leaves {v, om}; the output phase adds (om 1e-8) v_r v_c: v twice
            (2 e_w + 14), the constant and three products (4) - the rank-one line with its scale, no more
  sums      per coupon an entry takes the date record's rank-one term and the payment node's (2) and one row or short-end
            number per record and knot (6): 8 adds for at least two terms (the ratio term and -c D(tp))               4 n
  scale     acc 1e-8                                                                                                      2
                                                                          k = node_lag(e_w + 6) + 2 e_w + 18 + 4 n

general, a trade with ratio terms (kernels_general.hip, `add_nodes<6, ...>`; `general_lag` in `trade_k`; both variants):
  v         fma(bb_i, lj_i, v) over six knots: LJ (1), the weight (e_w), te's folded into tp's entry b[jx] += b[i] (1), the
            product, five adds                                                                                    e_w + 8
  rank-one  vr = om v (1), fma(vr, vc): v twice, two products                                                  2 e_w + 18
  convexity cf = om b (e_w + 2), the start weights handed to the previous coupon's entries (1), the payment node's joined
            (1), the tile (4), the product: e_w + 9 of its own gross, less
  sums      per coupon the rank-one term, six tiles, and the payment node's rank-one term and two tiles: 10 adds for at
            least two terms                                                                                             5 n
  scale 2, the merge of the flat convexity sums 1                     k = node_lag(e_w + 8) + 2 e_w + 20 + 5 n + 1
  LINEAR_FWD_RATES (`lindf_knots` and `add_cross`: the weights rho = d ln D / d ln d_k of each date): a lookup's
  d = da + w (db - da) on da = exp(L_a): 2 cond + 2 each, the difference, the product, the sum: 2 cond + 5; ln d = log(d): 2
  units of |ln d| <= cond and d's own: 4 cond + 5 per date, 12 cond + 15 for three, the two adds of l (of at most 3 cond): 6
  cond; exp (2), c (2), the product (1)                                                     node = ceil(18 cond) + 20
  rho_b = w db / d: 4 cond + 9; rho_a = 1 - rho_b takes rho_b's ABSOLUTE error, which `wr` brings into units of the gross
                                                                                     e_rho = ceil((4 cond + 9) wr)
  a knot's single-knot node: the amount om rho_k (e_rho + 1; te's folded into tp's: 1), v the Jacobian entry itself (1),
  vr = om v (1), fma(vr, vc) (LJ 1 + 1): e_rho + 6; the cross term om (x y^T + y x^T): x and y are fma chains over the node's
  knots (LJ, e_rho, the product, at most five adds: e_rho + 7), om x (1), the product (1): 2 e_rho + 16 - the line that counts
  sums      per coupon six single-knot nodes (a rank-one term and a row each: 12), two cross terms of two products (4) and
            the payment node's two knots (4): 20 adds for at least two terms, the merge 1; scale 2
                                                          k = ceil(18 cond) + 20 + 2 e_rho + 18 + 10 n + 1
  (Until this bound was applied the kernel walked such a node in the rho form of ln f, om (v v^T + sum over the dates of
  +-rho_a rho_b (LJ_a - LJ_b)(LJ_a - LJ_b)^T): the products rho_a rho_b LJ_a,p LJ_b,q of ONE date stand in v v^T and in the
  date's correction with opposite signs and cancel only up to rounding - 2e-23 to 4e-19 on gamma entries no term reaches, and
  on the others an error the reference's gross does not hold.  tests/test_gpu_price_lag.py found it on four books; DESIGN.md
  section 33.)

lite_lag (kernels_lite.hip, LAG; PV and delta; INV_DX, so e_w' = e_w + ceil(3 wr)):
  node_lag with e_w' and (e_w' + 6); a chained start takes the previous lane's L(te): the same number
  entries   om_r b(ts): e_w' + 1; the end's (next_om - om_r) b(te): the difference (1), e_w' + 1; the date's (om_r + om_p)
            b(tp) likewise: e_w' + 2;  fma(c, LJ, d): LJ (1), the product (1)                                     e_w' + 4
  sums      three sweeps of two entries per coupon: 6 adds for at least two terms: 3 n; d0 + e0 (1), 1e-4 (2)
                                                                          k = node_lag' + e_w' + 7 + 3 n
  LINEAR_FWD_RATES ("effective log weights"): a factor F = ba D_a + bb D_b: a part ba exp(L_a) is e_w' + 2 cond + 3, F one
  more, g = part (1 / F): 2 e_w' + 4 cond + 9; om_r = c ls lp / le: three factors (e_w' + 2 cond + 4), c (2), three
  operations; the entry om g (1 + 1), LJ and the product (2); the sums as above
                                                          k = 5 e_w' + ceil(10 cond) + 33 + 3 n

knot_lag (kernels_lite.hip KNOT + LAG, kernels_knot.hip): a trade's part of W += om_r u_k u_l holds the merge of the date's
  weights into the end's cc[2] += cc[4] (1) and two weights and two products: 2 e_w' + 5; the projection's two Jacobian
  entries and two products, the band term one more: 2 e_w' + 8 with the node           k_t = node_lag' + 2 e_w' + 8
  LINEAR_FWD_RATES: om_r (3 (e_w' + 2 cond + 4) + 5), two effective weights (2 (2 e_w' + 4 cond + 9)), two products, the
  projection (5)                                                          k_t = 7 e_w' + ceil(14 cond) + 42
  (the sums are the general kernel's reduced form in knot space: a knot's own amount on the diagonal, products of two
  different factors' weights on the pairs.  Until this bound was applied they were u u^T plus `factor_curvature`, the rho
  form: -w and +w on one pair of knots from every coupon of an interval, 1.6e-22 on a structural zero of agg_gamma.)
  sums      a table entry takes at most 7 adds per coupon (log schemes: three squares or pairs of the ratio node on one slot
            and the payment node's; LINEAR_FWD_RATES: four diagonal amounts and three pairs at distance 0): 4 N for at least
            two terms each; the block's 8 waves (7) and
            `knot_reduce_kernel` as for `knot`; the projection adds D_k and w_k LC per knot of a wave's share (2 ceil(Kc /
            16)) and one term per non-zero pair entry, band or overflow matrix - at most 15 per ratio node and one per
            payment node (15 R + N); the waves' sums (15), agg += (1), 1e-8 (2)
                             sums = 4 N + 7 + ceil(blocks / 64) + 5 + 2 ceil(Kc / 16) + 15 R + N + 18  (`knot_lag_sums`)
  The overflow matrix (pairs of knots more than 16 apart) is filled with atomic adds from every wave: the order of those
  adds, and so the last bits of an aggregate-only gamma, depend on scheduling - any order of m numbers costs m - 1 roundings,
  which the 4 N above holds.

aggregate (the one-desk row): trade t arrives with an error of at most k_t units of ITS gross, so an element of the book is
  held to  k = ceil(sum_t k_t gross_t / gross_book) + sums  of the book's gross (`book_k`; exact integer arithmetic) - one
  trade with a large k_t (a date 1e-9 before a knot under INV_DX) then weighs on the book only by its own gross.  The block
  partials (`reduce_partials_kernel`): a wave adds its trades (at most n_trades - 1 adds over all waves), its groups (1), the
  block its waves in order (11: the fast kernel's 12 waves are the most), the reduction strides and runs its butterfly
  (ceil(blocks / 64) - 1 + 6), the knot pass adds its projection to it (1)
                             sums = n_trades + 18 + ceil(blocks / 64)  (+ the knot pass's sums where it runs)
  wide (a plan whose launches with block partials are all wide-kernel launches): a wave adds its trades into `total` (at most
  n_trades - 1 adds over all waves; a packed entry outside the triangle adds 0.0), the block adds its waves in order (7: eight
  waves up to 10 chunks and without GAMMA, four beyond), `reduce_wide_kernel` strides over the blocks and runs its butterfly
  (ceil(blocks / 64) - 1 + 6) and reads each element through the store map (a copy), the knot pass adds its projection (1)
                             sums = n_trades + 12 + ceil(blocks / 64)  (+ the knot pass's sums where it runs)
  tiled: every tile launch is followed by its own `reduce_partials_kernel` over the launch's blocks, which writes the tile
  (and, off the diagonal, its mirror from the same number) - no element is summed over launches; four waves per block (3):
  inside the count of the block partials above, which is used as it stands.  The knot pass's projection is one kernel for
  every pillar count (`lj_at`, `lc_at`; columns in blocks of 64): `knot_sums` as it stands.
"""
import math

import numpy as np

from oracle.mp_oracle import _lookup_plan

from . import _ladder_reference as R

FLAT_FWD, LINEAR_FWD, LINEAR_ZERO = R.FLAT_FWD, R.LINEAR_FWD, R.LINEAR_ZERO
E_W = {FLAT_FWD: 1, LINEAR_FWD: 1, LINEAR_ZERO: 4}
BLOCKS = R.RATES_BLOCKS


def per_trade_reference(method, host, batch):
    return R.rates_reference(method, host, batch, np.arange(batch.n_trades + 1, dtype=np.int64))


def book_reference(method, host, batch):
    return R.rates_reference(method, host, batch, np.array([0, batch.n_trades], dtype=np.int64))[0]


def _amplification(s, wa, wb, A, B, GA, GB, La, Lb):
    """What an ABSOLUTE error of the upper weight does to the lower one, in units of the reference's gross: the lower weight
    wa moves by s = (upper / lower) times the upper weight's relative error, and the largest share of that in an element's
    gross is taken over the argument (log schemes: |wa L_a| of |wa L_a| + |wb L_b|; LINEAR_FWD_RATES: wa of wa + wb), the delta
    entries wa A_p of wa A_p + wb B_p, and the gamma entries - the convexity part wa GC_a and the second-order products
    2 a_p a_q + a_p b_q + b_p a_q (a = wa A, b = wb B) of wa GC_a + wb GC_b + (a_p + b_p)(a_q + b_q).  A, B: |LJ| of the two
    knots; GA, GB: their |C| / d + |J J^T| / d^2."""
    a, b = wa * A, wb * B
    worst = La / (La + Lb) if La + Lb > 0.0 else 0.0
    live = a + b > 0.0
    if np.any(live):
        worst = max(worst, float(np.max(a[live] / (a + b)[live])))
    if GA is not None:
        num = wa * GA + 2.0 * np.outer(a, a) + np.outer(a, b) + np.outer(b, a)
        den = wa * GA + wb * GB + np.outer(a + b, a + b)
        live = den > 0.0
        if np.any(live):
            worst = max(worst, float(np.max(num[live] / den[live])))
    return s * worst


def trade_stats(method, host, batch):
    """Per trade ``{"n", "cond", "wr"}`` (module docstring), from the inputs alone."""
    def build():
        R.mp.dps = 60
        method_ = int(method)
        cv = R._Curve(method_, host.times, host.dfs, host.jac, host.hess)
        x, d = cv.x, np.asarray(host.dfs, dtype=np.float64)
        A = np.abs(np.asarray(host.jac, dtype=np.float64)) / d[:, None]
        L = np.abs(np.log(d))
        hess = None if host.hess is None else np.abs(np.asarray(host.hess, dtype=np.float64))
        gc = lambda k: None if hess is None else hess[k] / d[k] + np.outer(A[k], A[k])
        seen = {}

        def lookup(t):
            if t not in seen:
                plan = _lookup_plan(x, t, method_)
                amp = 1.0
                if plan[0] == "interp" and 0.0 < float(plan[3]) < 1.0:
                    _, a, b, w = plan
                    w = float(w)
                    if method_ == LINEAR_FWD:
                        wa, wb, La, Lb = (1.0 - w) * d[a], w * d[b], (1.0 - w) * d[a], w * d[b]
                    elif method_ == LINEAR_ZERO:
                        wa, wb = t * (1.0 - w) / max(x[a], 1e-15), t * w / max(x[b], 1e-15)
                        La, Lb = abs(wa) * L[a], abs(wb) * L[b]
                    else:
                        wa, wb, La, Lb = 1.0 - w, w, (1.0 - w) * L[a], w * L[b]
                    wa, wb = abs(wa), abs(wb)
                    amp = max(1.0, _amplification(w / (1.0 - w), wa, wb, A[a], A[b], gc(a), gc(b), La, Lb))
                seen[t] = amp
            return seen[t]
        out = []
        for i in range(batch.n_trades):
            st = dict(n=0, cond=0.0, wr=1.0, ratio=0)
            for t, c, _ in R.trade_terms(batch, i):
                st["n"] += 1
                dates = t if isinstance(t, tuple) else (t,)
                conds = [float(cv.date(d)[3]) for d in dates]
                if isinstance(t, tuple):
                    st["ratio"] += 1
                st["cond"] = max(st["cond"], max(conds) if method_ == LINEAR_FWD else sum(conds))
                st["wr"] = max(st["wr"], max(lookup(float(d)) for d in dates))
            # the payment-lag variants form exp(L(ts) - L(te) + L(tp)) for EVERY accruing coupon, te == tp included
            st["cond_lag"] = st["cond"]
            st["weighted"] = batch.flt_weight is not None and bool(np.any(batch.flt_weight[int(batch.flt_off[i]):int(batch.flt_off[i + 1])] != 1.0))
            for j in range(int(batch.flt_off[i]), int(batch.flt_off[i + 1])):
                live = float(batch.flt_alpha[j]) > 0.0 and float(batch.flt_tp[j]) >= 0.0
                if live and method_ != LINEAR_FWD and (batch.flt_weight is None or float(batch.flt_weight[j]) != 0.0):
                    three = sum(float(cv.date(float(getattr(batch, f)[j]))[3]) for f in ("flt_ts", "flt_te", "flt_tp"))
                    st["cond_lag"] = max(st["cond_lag"], three)
            out.append(st)
        return out
    return R._cached("price stats", method, host, batch, (), build)


def _node(method, cond, e_w):
    if int(method) == LINEAR_FWD:
        return 9 + e_w + math.ceil(2 * cond)
    return 8 + math.ceil(cond * (e_w + 4))


def trade_k(family, method, st):
    """k of one trade priced by ``family`` ("fast", "fast_chained", "general", "wide", "tiled", "lite"; with payment lag or
    weights "fast_lag", "fast_lag_chained", "lite_lag" and "general_lag", the general kernel on a trade with ratio terms)."""
    method = int(method)
    e_w, n, cond = E_W[method], st["n"], st["cond"]
    if family in ("fast", "fast_chained", "general", "wide", "tiled"):
        merge = 1 if family in ("general", "tiled") else 0
        if method == LINEAR_FWD:
            return _node(method, cond, e_w) + 8 + 4 * n + merge
        return _node(method, cond, e_w) + 2 * e_w + 10 + 3 * n + merge
    if family == "lite":
        e_w += math.ceil(3 * st["wr"])
        return _node(method, cond, e_w) + e_w + 6 + 2 * n
    if family in ("fast_lag", "fast_lag_chained"):
        assert method != LINEAR_FWD, "the payment-lag variant of the fast kernel serves the log-linear schemes"
        return _node_lag(st["cond_lag"], e_w, 6) + 2 * e_w + 18 + 4 * n
    if family == "general_lag":
        if method == LINEAR_FWD:
            e_rho = math.ceil((4 * cond + 9) * st["wr"])
            return math.ceil(18 * cond) + 20 + 2 * e_rho + 18 + 10 * n + 1
        return _node_lag(cond, e_w, 8) + 2 * e_w + 20 + 5 * n + 1
    if family == "lite_lag":
        e_w += math.ceil(3 * st["wr"])
        if method == LINEAR_FWD:
            return 5 * e_w + math.ceil(10 * cond) + 33 + 3 * n
        return _node_lag(st["cond_lag"], e_w, 6) + e_w + 7 + 3 * n
    raise ValueError(family)


def _node_lag(cond, e_w, adds):
    """The node of a payment-lag family under a log scheme: 9 + ceil(cond (e_w + adds)) (module docstring)."""
    return 9 + math.ceil(cond * (e_w + adds))


def knot_trade_k(method, st, lag=False):
    """k_t of one trade in the knot pass (``lag``: the pass over the payment-lag rows)."""
    e_w = E_W[int(method)] + math.ceil(3 * st["wr"])
    if lag and int(method) == LINEAR_FWD:
        return 7 * e_w + math.ceil(14 * st["cond"]) + 42
    if lag:
        return _node_lag(st["cond_lag"], e_w, 6) + 2 * e_w + 8
    return _node(method, st["cond"], e_w) + 2 * e_w + 7


def knot_sums(stats, Kc, blocks):
    return sum(s["n"] for s in stats) + 7 + -(-max(blocks, 1) // 64) + 5 + 3 * (-(-Kc // 16)) + 18


def knot_lag_sums(stats, Kc, blocks):
    """The adds of the pass over the payment-lag rows and its share of the projection (module docstring, `knot_lag`)."""
    N, ratios = sum(s["n"] for s in stats), sum(s["ratio"] for s in stats)
    return 4 * N + 7 + -(-max(blocks, 1) // 64) + 5 + 2 * (-(-Kc // 16)) + 15 * ratios + N + 18


def aggregate_sums(n_trades, blocks, wide=False):
    """The adds of the block partials and their reduction; ``wide``: every launch with partials is a wide-kernel launch."""
    return n_trades + (12 if wide else 18) + -(-max(blocks, 1) // 64)


def book_k(ref, book, ks, name, sums):
    """Per element of the book's block ``name``: ceil(sum_t k_t gross_t / gross_book) + sums, object array of int."""
    lo = min([book[name].E] + [d[name].E for d in ref])
    num = None
    for k, d in zip(ks, ref):
        part = d[name].A * (int(k) << (d[name].E - lo))
        num = part if num is None else num + part
    den = book[name].A * (1 << (book[name].E - lo))
    out = np.empty(den.shape, dtype=object)
    for idx in np.ndindex(den.shape):
        out[idx] = (-(-int(num[idx]) // int(den[idx])) if den[idx] else 0) + sums
    return out


def share_elems(block, got, k, what=""):
    """`Block.share` with k per element (object array of int)."""
    got = np.asarray(got, dtype=np.float64).reshape(block.V.shape)
    assert np.all(np.isfinite(got)), f"{what}: not finite"
    m, ex = np.frexp(got)
    m = (m * 2.0 ** 53).astype(np.int64)
    worst, ten = 0.0, 10 ** block.s
    for idx in np.ndindex(got.shape):
        V, A = int(block.V[idx]), int(block.A[idx])
        if A == 0:
            assert got[idx] == 0.0 and not np.signbit(got[idx]), f"{what}{list(idx)}: gross is 0 but the entry is {got[idx]!r}"
            continue
        sh = int(ex[idx]) - 53 - block.E
        g = int(m[idx]) * ten
        if sh >= 0:
            err, scale = abs((g << sh) - V), A
        else:
            err, scale = abs(g - (V << -sh)), A << -sh
        worst = max(worst, ((err << 83) // (int(k[idx]) * scale)) / 2.0 ** 30)
    return worst


def case_ks(method, host, batch, ref, fams):
    """k_t per trade for the families ``fams`` [n]."""
    stats = trade_stats(method, host, batch)
    out = []
    for i, fam in enumerate(fams):
        if fam in ("knot", "knot_lag"):
            out.append(knot_trade_k(method, stats[i], lag=fam == "knot_lag"))
            continue
        # the general kernel walks a trade with ratio terms through `add_nodes<6, ...>`: its own count
        # (a weighted coupon paid on its accrual end is a plain node of amount N w: one product more)
        plain_weighted = fam == "general" and not stats[i]["ratio"] and stats[i]["weighted"]
        out.append(trade_k("general_lag" if fam == "general" and stats[i]["ratio"] else fam, method, stats[i]) + int(plain_weighted))
    return out


def rows_share(got, ref, ks, what, rows=None):
    """The worst share over the per-trade blocks ``got`` holds (pv, delta, gamma), trade by trade on its own k; returns
    ``(share, {family-less worst per block})``."""
    worst = 0.0
    for i in (range(len(ref)) if rows is None else rows):
        for name in BLOCKS:
            if name in got:
                g = np.asarray(got[name][i])
                worst = max(worst, ref[i][name].share(g.reshape(ref[i][name].V.shape), ks[i], f"{what} trade {i} {name}"))
    return worst


def book_share(got, ref, book, ks, sums, zero, what):
    """The worst share of the aggregate ``agg_pv / agg_delta / agg_gamma`` against the one-desk row on `book_k`; the blocks
    ``zero`` (not asked for) must be +0.0 throughout."""
    worst = 0.0
    for name in BLOCKS:
        g = np.asarray(got["agg_" + name], dtype=np.float64)
        if name in zero:
            assert not np.any(g) and not np.any(np.signbit(g)), f"{what} agg_{name}: not asked for, not +0.0"
            continue
        worst = max(worst, share_elems(book[name], g, book_k(ref, book, ks, name, sums), f"{what} agg_{name}"))
    return worst


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b, keys=None):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in (keys if keys is not None else a))
