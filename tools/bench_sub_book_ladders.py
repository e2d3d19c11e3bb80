"""Sub-book Greeks benchmark: the benchmark book (`synthesize`, off-grid OIS, a million trades) on the README GBP curve,
LINEAR_ZERO_RATES, cut into B = 1, 100, 1 000 and 10 000 sub-books of equal and of skewed (geometric) sizes; PV + delta and
PV + delta + gamma.

Timed, inputs resident, medians of warm repetitions between HIP events, the routes of a comparison alternating in one
process (the method of tools/bench_subbooks.py):
  * the ONE launch chain, adr_subbook_ladders_dev (knot sums, sub-book sum, projection per sub-book);
  * (a) one aggregate-only adr_price_dev over the whole book: the floor for B = 1;
  * (b) the route this replaces: one aggregate-only adr_price_dev per sub-book on batches uploaded beforehand, launches
    alone.  Timed at B = 100 and B = 1 000; at B = 10 000 it needs ten thousand uploads before it starts and is left out.
usage: bench_sub_book_ladders.py [reps] [out.json] [n]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from adrates_amd import _native
from adrates_amd.market.curves.curve_tables import build_engine_curve
from adrates_amd.market.position.scenarios import _permute_batch
from adrates_amd.trades import synthetic
from adrates_amd.trades.market_data import README_VALUE_DT, gbp_model
from adrates_amd.utils import InterpTypes

reps = max(3, int(sys.argv[1]) if len(sys.argv) > 1 else 7)
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "sub_book_ladders_bench.json")
n = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
LOOP_MAX_B = 1000
dev = torch.device("cuda", 0)
ctx = _native.default_context(0)
stream = torch.cuda.Stream(dev)


def sizes_of(B, dist):
    if dist == "equal":
        sizes = np.full(B, n // B, dtype=np.int64)
    else:                                           # geometric: the first sub-book about 1 / (1 - r) times the mean's share
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
        out.append((float(np.median(t)), (max(t) - min(t)) / float(np.median(t))))
    return out


curve = gbp_model(README_VALUE_DT, InterpTypes.LINEAR_ZERO_RATES).curves.GBP_OIS_SONIA
host = build_engine_curve(curve.swap_rates, curve.swap_times, curve.year_fracs)
dc = _native.DeviceCurve(ctx, curve._interp_type.value, host.times, host.dfs, host.jac, host.hess)
P = dc.n_pillars
stride = 1 + P + P * P
batch = synthetic.synthesize(README_VALUE_DT, n)
trades = _native.DeviceTrades(ctx, batch)
result = {"reps": reps, "trades": n, "pillars": P, "knots": int(host.times.size), "scheme": "LINEAR_ZERO_RATES", "cases": []}
REQUESTS = (("pv_delta", 3), ("pv_delta_gamma", 7))

for B, dist in ((1, "equal"), (100, "equal"), (100, "geometric"), (1000, "equal"), (1000, "geometric"), (10000, "equal"),
                (10000, "geometric")):
    sizes = sizes_of(B, dist)
    sub_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    plan = torch.from_numpy(_native.scenario_subbook_plan(n, sub_off)).to(dev)
    out = torch.zeros((B, stride), dtype=torch.float64, device=dev)
    work = torch.empty(_native.subbook_ladders_work(dc, n, B)[0], dtype=torch.float64, device=dev)
    case = {"sub_books": B, "sizes": dist, "largest": int(sizes.max()), "smallest": int(sizes.min()), "chunks": int(plan[B].item())}
    pieces = []
    if 1 < B <= LOOP_MAX_B:
        pieces = [_native.DeviceTrades(ctx, _permute_batch(batch, np.arange(lo, hi, dtype=np.int64))[0])
                  for lo, hi in zip(sub_off[:-1], sub_off[1:])]
    rows = torch.zeros((max(1, len(pieces)), stride), dtype=torch.float64, device=dev)
    for name, mask in REQUESTS:
        one = lambda: _native.subbook_ladders_dev(ctx, dc, trades, B, plan.data_ptr(), mask, out.data_ptr(), work.data_ptr(),
                                                  stream.cuda_stream)
        routes = [one]
        if B == 1:
            routes.append(lambda: _native.price_dev(ctx, dc, trades, mask, agg_ptr=rows.data_ptr(), stream=stream.cuda_stream))
        elif pieces:
            def loop():
                for b, piece in enumerate(pieces):
                    _native.price_dev(ctx, dc, piece, mask, agg_ptr=rows[b].data_ptr(), stream=stream.cuda_stream)
            routes.append(loop)
        t = timed(routes, reps)
        entry = {"one_launch": {"ms": t[0][0], "spread": t[0][1]}}
        if len(routes) > 1:
            key = "aggregate_only_whole_book" if B == 1 else "loop_of_aggregate_only"
            entry[key] = {"ms": t[1][0], "spread": t[1][1]}
            entry["speedup"] = t[1][0] / t[0][0]
            entry["margin"] = max(t[0][1], t[1][1])
            entry["faster_by_more_than_the_spread"] = bool(t[1][0] / t[0][0] - 1.0 > entry["margin"])
            scale = rows.abs().amax(0).clamp_min(1e-300)
            entry["worst_difference_over_largest_row_entry"] = float(((out - rows).abs().amax(0) / scale).max().item())
        case[name] = entry
    for piece in pieces:
        piece.close()
    result["cases"].append(case)
    print(json.dumps(case), flush=True)
trades.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps({"written": out_path}))
