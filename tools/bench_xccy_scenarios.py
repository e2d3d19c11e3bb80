#!/usr/bin/env python3
"""Cross-currency scenario revaluation benchmark: the `bench_xccy` book of distinct GBP/USD basis swaps
(adrates_amd/trades/synthetic_xccy.py) under S = 64 and 1 024 joint scenarios - par-quote shocks of the SONIA and the SOFR
curve and basis shocks, the XCCY rows from `shocked_xccy_dfs` - book PV per scenario.

Two routes for the same numbers, timed in the same process and alternating, three repetitions each, inputs resident:
  chain  adr_scenario_pv_dev on the domestic legs + adr_xccy_scenario_pv_dev on the foreign legs, all S scenarios at once;
  loop   the route the chain replaces: per scenario upload that scenario's curves (adr_curve_upload: the foreign OIS row, the
         XCCY row and, since the joint scenarios shock it too, the domestic row), then
         adr_price_xccy_foreign_dev and adr_price_dev (VALUE, book sums only); the uploads are also timed alone.
Times are between HIP events on one stream; the spread is (max - min) / median over the repetitions.  The two routes' book
PVs must agree to 1e-10 per unit notional (asserted).  The host work in front of the chain - the shocked OIS rows and
`shocked_xccy_dfs` - is reported in seconds beside it: it is paid once per scenario set, on the CPU.

What bounds the kernel is reported as counts, not as a share of peak: exponentials per scenario and swap by the kernel's
sharing rules (one per distinct date of a coupon on its table), and the bytes of the two LDS tables per block.
usage: bench_xccy_scenarios.py [n_swaps] [out.json]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from adrates_amd import _native
from adrates_amd.market.position.xccy_book import XccyBook, revalue_xccy_on_curves
from adrates_amd.trades import synthetic_xccy as SX
from adrates_amd.trades.market_data import GBP_PX, README_VALUE_DT as vd, TENORS, USD_PX

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                               "profiles", "xccy_scenario_bench.json")
REPS, S_LIST = 3, (64, 1024)
dev = torch.device("cuda", 0)
ctx = _native.default_context(0)
stream = torch.cuda.Stream(dev)
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def shocks(S, P, seed, size):
    """Parallel shifts of up to +-``size`` bp with twists of up to a third of that along the pillars."""
    rng = np.random.default_rng(seed)
    slope = np.linspace(-1.0, 1.0, P)
    return rng.uniform(-size, size, S)[:, None] + rng.uniform(-size / 3, size / 3, S)[:, None] * slope[None, :]


def exps_per_swap(b):
    """Exponentials one scenario costs per swap of the foreign legs under a log scheme, by make_slot's rules: D_f(te) per
    accruing live coupon, D_f(ts) where it is not the previous coupon's D_f(te), D_x(tp) per live coupon, D_x per live fixed
    flow that is not paid on the coupon of its index."""
    live, acc = b.flt_tp >= 0.0, b.flt_alpha > 0.0
    first = np.zeros(b.flt_tp.size, dtype=bool)
    first[b.flt_off[:-1][b.flt_off[:-1] < b.flt_tp.size]] = True
    inherits = np.concatenate(([False], (b.flt_te[:-1] == b.flt_ts[1:]) & live[:-1] & acc[:-1])) & ~first
    cpn = live & acc
    return (int(np.sum(cpn)) + int(np.sum(cpn & ~inherits)) + int(np.sum(live)) + int(np.sum(b.fix_tp > 0.0))) / b.n_trades


def timed_pair(new, old, k):
    with torch.cuda.stream(stream):
        new(); old()
        stream.synchronize()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(k)]
        for a, b, c, d in ev:
            a.record(stream); new(); b.record(stream)
            c.record(stream); old(); d.record(stream)
    torch.cuda.synchronize()
    t_new, t_old = [a.elapsed_time(b) for a, b, _, _ in ev], [c.elapsed_time(d) for _, _, c, d in ev]
    spread = lambda t: (max(t) - min(t)) / float(np.median(t))
    return float(np.median(t_new)), float(np.median(t_old)), spread(t_new), spread(t_old)


model = SX.build_market(vd, GBP_PX, USD_PX, TENORS)
terms, _ = SX.draw_terms(vd, n)
t0 = time.perf_counter()
book = XccyBook(terms, model)
compile_s = time.perf_counter() - t0
dom_tr, for_tr = _native.upload_many(ctx, [book.domestic, book.foreign_legs])
dm, fm, xm = (c._interp_type.value for c in (book.dom_curve, book.for_curve, book.xccy))
total_notional = float(np.sum(np.abs(book.domestic.notional)))
Pd, Pf, Pb = len(book.dom_curve.swap_times), len(book.for_curve.swap_times), len(book.xccy.swap_times)
result = {"swaps": n, "reps": REPS, "host_compile_legs_s": compile_s, "exp_per_swap_and_scenario": exps_per_swap(book.foreign_legs),
          "foreign_coupons_per_swap": book.foreign_legs.flt_tp.size / n, "cases": []}
for S in S_LIST:
    t0 = time.perf_counter()
    dom, frn, xr, spots, _ = book.scenario_rows(shocks(S, Pd, S, 100.0), shocks(S, Pf, S + 1, 100.0), shocks(S, Pb, S + 2, 10.0), host=True)
    rows_s = time.perf_counter() - t0
    (d_t, d_rows), (f_t, f_rows), (x_t, x_rows) = [(np.asarray(t), np.asarray(r)[:S]) for t, r in (dom, frn, xr)]
    t = {k: up(v) for k, v in dict(times_d=d_t, dfs_d=d_rows, times_f=f_t, dfs_f=f_rows, times_x=x_t, dfs_x=x_rows).items()}
    ptrs = {k: v.data_ptr() for k, v in t.items()}
    out_d, out_f = torch.zeros(S, dtype=torch.float64, device=dev), torch.zeros(S, dtype=torch.float64, device=dev)
    work_d = torch.empty(_native.scenario_pv_work(n, S), dtype=torch.float64, device=dev)
    work_f = torch.empty(_native.xccy_scenario_pv_work(n, S), dtype=torch.float64, device=dev)

    def chain():
        _native.scenario_pv_dev(ctx, dm, d_t.size, ptrs["times_d"], S, ptrs["dfs_d"], dom_tr, out_d.data_ptr(), work_d.data_ptr(), 0,
                                stream.cuda_stream)
        _native.xccy_scenario_pv_dev(ctx, fm, f_t.size, S, xm, x_t.size, S, S, for_tr, ptrs, out_f.data_ptr(), work_f.data_ptr(), 0,
                                     stream.cuda_stream)

    # the loop's curves carry a two-pillar all-zero Jacobian (VALUE only): agg rows are [pv, delta[2], gamma[2][2]]
    agg_d, agg_f = (torch.zeros((S, 7), dtype=torch.float64, device=dev) for _ in range(2))
    agg_x = torch.zeros(7, dtype=torch.float64, device=dev)
    zero_jac = [np.zeros((k.size, 2)) for k in (d_t, f_t, x_t)]

    def uploads(s):
        return (_native.DeviceCurve(ctx, dm, d_t, d_rows[s], zero_jac[0]), _native.DeviceCurve(ctx, fm, f_t, f_rows[s], zero_jac[1]),
                _native.DeviceCurve(ctx, xm, x_t, x_rows[s], zero_jac[2]))

    def loop(price=True):
        for s in range(S):
            cd, cf, cx = uploads(s)
            if price:
                _native.price_xccy_foreign_dev(ctx, cf, cx, for_tr, _native.REQ_VALUE, 0, 0, 0, agg_f[s].data_ptr(),
                                               agg_x.data_ptr(), stream.cuda_stream)
                _native.price_dev(ctx, cd, dom_tr, _native.REQ_VALUE, 0, 0, 0, agg_d[s].data_ptr(), stream.cuda_stream)
                stream.synchronize()                    # the curves are freed when they go out of scope
            cd.close(); cf.close(); cx.close()

    ms_chain, ms_loop, sp_chain, sp_loop = timed_pair(chain, loop, REPS)
    _, ms_up, _, sp_up = timed_pair(lambda: None, lambda: loop(False), REPS)
    const = float(book.const_dom.sum()) + float(book.const_for.sum()) / book.spot
    a_ = (out_d + out_f / book.spot).cpu().numpy() + const
    b_ = (agg_d[:, 0] + agg_f[:, 0] / book.spot).cpu().numpy() + const
    err = float(np.max(np.abs(a_ - b_)) / total_notional)
    assert err <= 1e-10, f"the two routes' book PVs differ by {err:.3e} per unit notional"
    layer = revalue_xccy_on_curves(book, (d_t, d_rows), (f_t, f_rows), (x_t, x_rows), ctx=ctx)["book_pv"]
    assert np.array_equal(layer, a_) or np.max(np.abs(layer - a_)) <= 1e-12 * total_notional
    case = {"scenarios": S, "knots": [int(d_t.size), int(f_t.size), int(x_t.size)],
            "lds_table_bytes_per_block": 8 * 64 * int(f_t.size + x_t.size),
            "chain": {"ms": ms_chain, "spread": sp_chain, "scenario_swaps_per_s": n * S / ms_chain * 1e3},
            "loop_upload_and_price_per_scenario": {"ms": ms_loop, "spread": sp_loop, "scenario_swaps_per_s": n * S / ms_loop * 1e3,
                                                   "curve_uploads_per_scenario": 3, "ms_uploads_alone": ms_up, "spread_uploads_alone": sp_up},
            "speedup": ms_loop / ms_chain, "faster_by_more_than_the_spread": bool(ms_loop / ms_chain - 1.0 > max(sp_chain, sp_loop)),
            "host_scenario_rows_s": rows_s, "routes_agree_unit_notional": err}
    result["cases"].append(case)
    print(json.dumps(case), flush=True)
dom_tr.close(); for_tr.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps({"written": out_path, "cases": len(result["cases"])}))
