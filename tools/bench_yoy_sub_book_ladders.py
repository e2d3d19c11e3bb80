"""Inflation sub-book Greeks benchmark: a million YoY swaps (tiled from two hundred) on the README GBP curve,
LINEAR_ZERO_RATES, and a 12-pillar RPI inflation curve, cut into B = 1, 100 and 1 000 equal desks and 1 000 geometric ones;
PV + delta and PV + delta + gamma.

Timed, inputs resident, medians of warm repetitions between HIP events, the routes of a comparison alternating in one
process (the method of tools/bench_credit_sub_book_ladders.py):
  * the ONE chain, adr_yoy_subbook_ladders_dev (knot sums with the inflation tables and M, desk sum, two projections);
  * (a) the loop it replaces: per desk one adr_yoy_risk_dev with ADR_YOY_AGG on the desk's coupons plus one aggregate-only
    adr_price_dev on the desk's fixed-flow batch (the projected amounts as fixed flows), uploaded beforehand, launches alone
    (B = 100 and 1 000; at B = 1 it is the whole-book route);
  * (b) adr_subbook_ladders_dev on the fixed-flow batch and the same desks: what the chain costs without the inflation
    tables - the ratio is their price.
The loop has no cross block; the chain's other blocks are compared with it.
usage: bench_yoy_sub_book_ladders.py [reps] [out.json] [n]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from adrates_amd import _native
from adrates_amd.market.curves.curve_tables import build_engine_curve
from adrates_amd.market.position.inflation_engine import inflation_inputs
from adrates_amd.market.position.scenarios import _gather_offsets, _permute_batch, yoy_book_arrays
from adrates_amd.trades.compiler import TradeBatch
from adrates_amd.trades.market_data import INFL_PX, INFL_TENORS, README_VALUE_DT, random_yoy_book, yoy_model
from adrates_amd.utils import InterpTypes

reps = max(3, int(sys.argv[1]) if len(sys.argv) > 1 else 7)
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "yoy_sub_book_ladders_bench.json")
n = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
dev = torch.device("cuda", 0)
ctx = _native.default_context(0)
stream = torch.cuda.Stream(dev)
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def sizes_of(B, dist):
    if dist == "equal":
        sizes = np.full(B, n // B, dtype=np.int64)
    else:                                           # geometric: the first desk about 1 / (1 - r) times the mean's share
        r = 1.0 - 10.0 / B if B > 10 else 0.5
        w = r ** np.arange(B)
        sizes = np.maximum(1, np.floor(n * w / w.sum())).astype(np.int64)
    sizes[0] += n - int(sizes.sum())
    assert sizes.min() >= 1 and sizes.sum() == n
    return sizes


def timed(fns, k):
    """Per route: (median ms, (max - min) / median) of k alternating repetitions, each between its own events."""
    with torch.cuda.stream(stream):
        for f in fns:
            f()
        stream.synchronize()
        ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(k)]
        for row in ev:
            for f, (a, b) in zip(fns, row):
                a.record(stream); f(); b.record(stream)
    torch.cuda.synchronize()
    out = []
    for j in range(len(fns)):
        t = [row[j][0].elapsed_time(row[j][1]) for row in ev]
        out.append({"ms": float(np.median(t)), "spread": (max(t) - min(t)) / float(np.median(t))})
    return out


# a 12-pillar inflation curve: twelve of the RPI quotes
INFL_12 = ("1Y", "2Y", "3Y", "5Y", "7Y", "10Y", "12Y", "15Y", "20Y", "25Y", "30Y", "40Y")
model = yoy_model(README_VALUE_DT, InterpTypes.LINEAR_ZERO_RATES, tenors=list(INFL_12),
                  px=[INFL_PX[INFL_TENORS.index(t)] for t in INFL_12])
curve, infl = model.curves.GBP_OIS_SONIA, model.curves.GBP_RPI_INFLATION
method = curve._interp_type.value
host = build_engine_curve(curve.swap_rates, curve.swap_times, curve.year_fracs)
dc = _native.DeviceCurve(ctx, method, host.times, host.dfs, host.jac, host.hess)
im, T, b = inflation_inputs(infl)
P, Pi, K = dc.n_pillars, T.size, host.times.size
Q = P + Pi

# the book: 200 YoY swaps, tiled
seed_fixed, seed_cpn = yoy_book_arrays(random_yoy_book(README_VALUE_DT, 200, seed=13), README_VALUE_DT)
pick = np.random.default_rng(1).integers(0, 200, n)
fix_off, fi = _gather_offsets(seed_fixed[0], pick)
cpn_off, ci = _gather_offsets(seed_cpn["cpn_off"], pick)
fixed = (fix_off, seed_fixed[1][fi], seed_fixed[2][fi])
coupons = dict({k: np.asarray(seed_cpn[k], dtype=np.float64)[ci] for k in _native.YOY_FIELDS}, cpn_off=cpn_off)
_, cpn = _native.yoy_pack(coupons)
m, n_fix = cpn.shape[1], fixed[1].size
amount = _native.yoy_risk(ctx, (method, host.times, host.dfs), (im, T, b), coupons, 0)["amount"]
# the fixed-flow batch: per swap its fixed flows, then its coupons' amounts at their payment times
flow_off = (fix_off + cpn_off).astype(np.int64)
tp, pay = np.empty(n_fix + m), np.empty(n_fix + m)
at_fix = np.repeat(flow_off[:-1] - fix_off[:-1], np.diff(fix_off)) + np.arange(n_fix)
at_cpn = np.repeat(flow_off[:-1] + np.diff(fix_off) - cpn_off[:-1], np.diff(cpn_off)) + np.arange(m)
tp[at_fix], pay[at_fix], tp[at_cpn], pay[at_cpn] = fixed[1], fixed[2], coupons["tp"], amount
e = np.zeros(0)
flows = TradeBatch(flow_off, np.zeros(n + 1, dtype=np.int64), tp, pay, e, e.copy(), e.copy(), e.copy(), np.ones(n), np.zeros(n),
                   np.ones(n), np.ones(n))
flow_trades = _native.DeviceTrades(ctx, flows)
bufs = dict(T=up(T), b=up(b), fix_off=up(fix_off), fix_tp=up(fixed[1]), fix_pay=up(fixed[2]), cpn_off=up(cpn_off), cpn=up(cpn),
            times=up(host.times), dfs=up(host.dfs))
result = {"reps": reps, "swaps": n, "seed_swaps": 200, "coupons": int(m), "fixed_flows": int(n_fix), "pillars": P,
          "inflation_pillars": Pi, "knots": int(K), "scheme": "LINEAR_ZERO_RATES", "cases": []}
REQUESTS = (("pv_delta", 3), ("pv_delta_gamma", 7))
R = 1 + Pi + Pi * Pi

for B, dist in ((1, "equal"), (100, "equal"), (1000, "equal"), (1000, "geometric")):
    sizes = sizes_of(B, dist)
    sub_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    bufs["plan"] = up(_native.scenario_subbook_plan(n, sub_off))
    ptrs = {k: v.data_ptr() for k, v in bufs.items()}
    words, chunks = _native.yoy_subbook_ladders_work(dc, Pi, n, B)
    out = torch.zeros((B, 1 + Q + Q * Q), dtype=torch.float64, device=dev)
    work = torch.empty(words, dtype=torch.float64, device=dev)
    plain = torch.zeros((B, 1 + P + P * P), dtype=torch.float64, device=dev)
    plain_work = torch.empty(_native.subbook_ladders_work(dc, n, B)[0], dtype=torch.float64, device=dev)
    case = {"sub_books": B, "sizes": dist, "largest": int(sizes.max()), "smallest": int(sizes.min()), "chunk_rows": chunks,
            "work_bytes": 8 * words}
    pieces = [flow_trades] if B == 1 else [_native.DeviceTrades(ctx, _permute_batch(flows, np.arange(lo, hi, dtype=np.int64))[0])
                                           for lo, hi in zip(sub_off[:-1], sub_off[1:])]
    rows = torch.zeros((B, 1 + P + P * P), dtype=torch.float64, device=dev)
    agg = torch.zeros((B, R), dtype=torch.float64, device=dev)
    risk_work = torch.empty(_native.yoy_risk_work(int(sizes.max()), Pi), dtype=torch.float64, device=dev)
    for name, mask in REQUESTS:
        one = lambda: _native.yoy_subbook_ladders_dev(ctx, dc, im, Pi, n, n_fix, m, B, ptrs, mask, out.data_ptr(), work.data_ptr(),
                                                      stream.cuda_stream)
        fixed_only = lambda: _native.subbook_ladders_dev(ctx, dc, flow_trades, B, ptrs["plan"], mask, plain.data_ptr(),
                                                         plain_work.data_ptr(), stream.cuda_stream)

        def loop():
            for d, piece in enumerate(pieces):
                lo, hi = int(sub_off[d]), int(sub_off[d + 1])
                p = dict(ptrs, cpn_off=ptrs["cpn_off"] + 8 * lo)          # the desk's offsets index the whole coupon arrays
                _native.yoy_risk_dev(ctx, method, K, im, Pi, hi - lo, m, p, mask | _native.YOY_AGG,
                                     {"agg": agg[d].data_ptr(), "work": risk_work.data_ptr()}, stream.cuda_stream)
                _native.price_dev(ctx, dc, piece, mask, agg_ptr=rows[d].data_ptr(), stream=stream.cuda_stream)
        t = timed([one, loop, fixed_only], reps)
        entry = dict(zip(("one_chain", "loop_of_yoy_risk_and_aggregate_only", "fixed_flow_sub_book_ladders"), t))
        entry["ratio_to_fixed_flow_ladders"] = t[0]["ms"] / t[2]["ms"]
        entry["speedup_over_loop"] = t[1]["ms"] / t[0]["ms"]
        entry["margin"] = max(t[0]["spread"], t[1]["spread"])
        entry["faster_by_more_than_the_spread"] = bool(t[1]["ms"] / t[0]["ms"] - 1.0 > entry["margin"])
        g = out[:, 1 + Q:].reshape(B, Q, Q)
        got_d = torch.cat([out[:, :1 + P], g[:, :P, :P].reshape(B, P * P)], dim=1)
        got_i = torch.cat([out[:, 1 + P:1 + Q], g[:, P:, P:].reshape(B, Pi * Pi)], dim=1)
        worst = lambda a, c: float(((a - c).abs().amax(0) / c.abs().amax(0).clamp_min(1e-300)).max().item())
        entry["worst_difference_over_largest_row_entry"] = {"discount": worst(got_d, rows), "inflation": worst(got_i, agg[:, 1:])}
        case[name] = entry
    if B > 1:
        for piece in pieces:
            piece.close()
    result["cases"].append(case)
    print(json.dumps(case), flush=True)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps({"written": out_path}))
