"""The plain reference of the cross-currency scenario entries (adr_xccy_scenario_pv* and the per-trade rows of their sub-book
forms) and the bound the kernel and its host twin are held to, element by element (tests/test_xccy_scenarios_host.py, CPU, and
tests/test_gpu_xccy_scenarios.py, GPU).  Built on tests/_scenario_reference.py's `_Rows` (D(t) on a table, in mpmath at 60
digits on `oracle.mp_oracle._lookup_plan`'s float64 decisions) and `Reference` (the element-by-element judge); it shares no
code with the kernel.

The operation.  Two tables: the foreign OIS rows ``dfs_f [S_f, K_f]`` on ``times_f`` with scheme ``for_method`` give Df(t), the
XCCY rows ``dfs_x [S_x, K_x]`` on ``times_x`` with ``x_method`` give Dx(t); a shared row is read by every scenario.  For every
pair (trade i, scenario s)
  value = sum over the fixed flows with xt > 0 of     fix_sign pay Dx(xt)
        + sum over the float coupons with tp >= 0 of  flt_sign N w ((Df(ts) / Df(te) - 1 when alpha > 0, else 0) + spread alpha) Dx(tp)
and ``gross`` is the same sum on absolute values with the terms as written: |N w| (Df(ts) / Df(te) + 1 + |spread alpha|) Dx(tp)
for an accruing coupon, |N w| |spread alpha| Dx(tp) for one that does not accrue, |pay| Dx(xt) for a fixed flow.  An element
with gross == 0 must be +0.0.

The bound |got - value| <= k 2^-53 gross, by that module's conventions (a rounding is ONE unit 2^-53 of the absolute sum it
acts on, a library function at one ulp TWO).  With e_f = `date_roundings(for_method, cond_f)` and e_x = `date_roundings(x_method,
cond_x)`, cond_f / cond_x the largest conditioning of the trade's live dates on the scenario's foreign / XCCY row:
  coupon    q = Df(ts) / Df(te): two date evaluations on the foreign table and the division, 2 e_f + 1;  q - 1 (1), spread alpha
            (1), + sa (1): the two adds and the product;  * Dx(tp): one date on the XCCY table and the product, e_x + 1;  * w (1)
                                                                                                      2 e_f + e_x + 6
            (a fixed flow, pay * Dx(xt), has e_x + 1, a coupon that does not accrue e_x + 3: less).  Where the code takes Df(ts)
            from the previous coupon's Df(te) or a fixed flow's Dx from the coupon's Dx(tp), it takes the number the date's own
            evaluation gives, so nothing is added
  sums      the running sums, the join and (flt_sign N) * a.flt                                          n_terms + 1
  k = 2 e_f + e_x + 6 + n_terms + 1.  With one table passed as both curves this is `_scenario_reference.bound_k`.  Nothing in k
is fitted to what the code returns.
"""
import numpy as np
from mpmath import mp, mpf

from ._scenario_reference import DPS, Reference, _Rows, _key, _trade_flows, _BATCH_FIELDS, date_roundings


def bound_k(for_method, x_method, n_terms, cond_f, cond_x):
    return 2 * date_roundings(for_method, cond_f) + date_roundings(x_method, cond_x) + 6 + n_terms + 1


_CACHE = {}


def reference(for_method, times_f, dfs_f, x_method, times_x, dfs_x, batch) -> Reference:
    """The `Reference` of one call; ``dfs_f`` and ``dfs_x`` one shared row or one row per scenario.  Built once per process for
    the same inputs."""
    dfs_f = np.ascontiguousarray(np.atleast_2d(dfs_f), dtype=np.float64)
    dfs_x = np.ascontiguousarray(np.atleast_2d(dfs_x), dtype=np.float64)
    key = (int(for_method), int(x_method)) + _key(times_f, dfs_f, times_x, dfs_x, *[getattr(batch, f) for f in _BATCH_FIELDS])
    if key not in _CACHE:
        _CACHE[key] = _build(int(for_method), times_f, dfs_f, int(x_method), times_x, dfs_x, batch)
    return _CACHE[key]


def _build(fm, times_f, dfs_f, xm, times_x, dfs_x, batch):
    mp.dps = DPS
    F, X = _Rows(fm, times_f, dfs_f), _Rows(xm, times_x, dfs_x)
    S = max(dfs_f.shape[0], dfs_x.shape[0])
    assert dfs_f.shape[0] in (1, S) and dfs_x.shape[0] in (1, S)
    n = batch.n_trades
    value, gross = [], []
    k = np.zeros((n, S), dtype=np.int64)
    zero = mpf(0)
    for i in range(n):
        fixed, coupons = _trade_flows(batch, i, None, None)
        n_terms = len(fixed) + len(coupons)
        v_row, g_row = [], []
        for s in range(S):
            rf, rx = (s if dfs_f.shape[0] == S else 0), (s if dfs_x.shape[0] == S else 0)
            v, g, cond_f, cond_x = zero, zero, zero, zero
            for xt, amount, _ in fixed:
                D, c = X.date(xt, rx)
                cond_x = max(cond_x, c)
                v += amount * D
                g += abs(amount * D)
            for ts, te, tp, accrues, snw, sa, _ in coupons:
                Dp, c = X.date(tp, rx)
                cond_x = max(cond_x, c)
                if accrues:
                    (Ds, cs), (De, ce) = F.date(ts, rf), F.date(te, rf)
                    cond_f = max(cond_f, cs, ce)
                    q = Ds / De
                    v += snw * ((q - 1) + sa) * Dp
                    g += abs(snw) * (q + 1 + abs(sa)) * Dp
                else:
                    v += snw * sa * Dp
                    g += abs(snw) * abs(sa) * Dp
            v_row.append(v)
            g_row.append(g)
            k[i, s] = bound_k(fm, xm, n_terms, float(cond_f), float(cond_x))
        value.append(v_row)
        gross.append(g_row)
    return Reference(value, gross, k)
