"""Delta-gamma P&L benchmark (adr_ladder_pnl_dev, csrc/ladder_pnl.hip): B desks' ladders under S = 1 024 scenarios.

Timed, inputs resident, medians of warm repetitions between HIP events, the routes of a comparison alternating in one
process (the method of tools/bench_sub_book_ladders.py):
  * the kernel, P&L alone and with both parts, at P = 32 for B = 100, 1 000 and 10 000 and at P = 64 for B = 1 000;
  * (a) what a user writes today on the same device tensors: D @ X.T + 0.5 * einsum('sp,bpq,sq->bs', X, G, X);
  * (b) for context, on the million-trade benchmark book cut into 1 000 desks: the full revaluation of every desk
    (adr_scenario_subbook_pv_dev) against the ladders (adr_subbook_ladders_dev) followed by the kernel.
The kernel's share of the fp64 vector peak counts 2 B S (P^2 + P) flops over 78.6 TFLOP/s.
usage: bench_ladder_pnl.py [reps] [out.json] [n] [S]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from adrates_amd import _native
from adrates_amd.market.position.scenarios import ScenarioGrid
from adrates_amd.trades import synthetic
from adrates_amd.trades.market_data import README_VALUE_DT, TENORS, gbp_model
from adrates_amd.utils import InterpTypes

reps = max(3, int(sys.argv[1]) if len(sys.argv) > 1 else 7)
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "ladder_pnl_bench.json")
n = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
S = int(sys.argv[4]) if len(sys.argv) > 4 else 1024
PEAK = 78.6e12
dev = torch.device("cuda", 0)
ctx = _native.default_context(0)
stream = torch.cuda.Stream(dev)


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


result = {"reps": reps, "scenarios": S, "cases": []}
for P, B in ((32, 100), (32, 1000), (32, 10000), (64, 1000)):
    rng = np.random.default_rng([P, B])
    ladders = torch.from_numpy(rng.standard_normal((B, 1 + P + P * P))).to(dev)
    X = torch.from_numpy(rng.standard_normal((S, P)) * 25.0).to(dev)
    D, G = ladders[:, 1:1 + P].contiguous(), ladders[:, 1 + P:].reshape(B, P, P).contiguous()
    pnl, part_d, part_g = (torch.zeros((B, S), dtype=torch.float64, device=dev) for _ in range(3))
    held = {}
    kernel = lambda: _native.ladder_pnl_dev(ctx, B, P, ladders.data_ptr(), S, X.data_ptr(), pnl.data_ptr(), stream=stream.cuda_stream)
    parts = lambda: _native.ladder_pnl_dev(ctx, B, P, ladders.data_ptr(), S, X.data_ptr(), pnl.data_ptr(), part_d.data_ptr(),
                                           part_g.data_ptr(), stream=stream.cuda_stream)

    def expression():
        held["out"] = D @ X.T + 0.5 * torch.einsum("sp,bpq,sq->bs", X, G, X)
    t = timed([kernel, expression, parts], reps)
    flops = 2.0 * B * S * (P * P + P)
    case = {"pillars": P, "desks": B, "kernel": t[0], "torch_expression": t[1], "kernel_with_parts": t[2],
            "speedup": t[1]["ms"] / t[0]["ms"], "margin": max(t[0]["spread"], t[1]["spread"]),
            "share_of_fp64_vector_peak": flops / (t[0]["ms"] * 1e-3) / PEAK,
            "worst_difference_over_largest_entry": float(((pnl - held["out"]).abs().max() / held["out"].abs().max()).item())}
    case["not_slower_by_more_than_the_spread"] = bool(t[0]["ms"] <= t[1]["ms"] * (1.0 + case["margin"]))
    result["cases"].append(case)
    print(json.dumps(case), flush=True)
    del held, ladders, X, D, G, pnl, part_d, part_g
    torch.cuda.empty_cache()

# (b) the million-trade book in 1 000 desks: full revaluation against ladders + kernel
B = 1000
rng = np.random.default_rng(S)
slope = np.linspace(-1.0, 1.0, len(TENORS))
par, twist = rng.uniform(-0.25, 0.25, S), rng.uniform(-0.1, 0.1, S)
shocks = [{t: float(par[i] + twist[i] * slope[k]) for k, t in enumerate(TENORS)} for i in range(S)]         # percent
model = gbp_model(README_VALUE_DT, InterpTypes.LINEAR_ZERO_RATES)
grid = ScenarioGrid(model, "GBP_OIS_SONIA", shocks, ctx=ctx)
arr = _native.curve_set_arrays(grid._set)
dc = grid._ladder_curve()
P = dc.n_pillars
batch = synthetic.synthesize(README_VALUE_DT, n)
trades = _native.DeviceTrades(ctx, batch)
sub_off = np.linspace(0, n, B + 1).astype(np.int64)
plan = torch.from_numpy(_native.scenario_subbook_plan(n, sub_off)).to(dev)
sub = torch.zeros((B, S), dtype=torch.float64, device=dev)
swork = torch.empty(_native.scenario_subbook_work(n, B, S), dtype=torch.float64, device=dev)
ladders = torch.zeros((B, 1 + P + P * P), dtype=torch.float64, device=dev)
lwork = torch.empty(_native.subbook_ladders_work(dc, n, B)[0], dtype=torch.float64, device=dev)
X = torch.from_numpy(grid.shocks_bp()).to(dev)
pnl = torch.zeros((B, S), dtype=torch.float64, device=dev)
full = lambda: _native.scenario_subbook_pv_dev(ctx, arr["method"], arr["K"], arr["times"], S, arr["dfs"], trades, B, plan.data_ptr(),
                                               sub.data_ptr(), swork.data_ptr(), 0, stream.cuda_stream)
ladder = lambda: _native.subbook_ladders_dev(ctx, dc, trades, B, plan.data_ptr(), 7, ladders.data_ptr(), lwork.data_ptr(),
                                            stream.cuda_stream)
kernel = lambda: _native.ladder_pnl_dev(ctx, B, P, ladders.data_ptr(), S, X.data_ptr(), pnl.data_ptr(), stream=stream.cuda_stream)
t = timed([full, ladder, kernel], reps)
gap = (sub - ladders[:, :1]) - pnl                  # both against the same base PV: the ladders' own
context = {"trades": n, "desks": B, "pillars": P, "shocks": "parallel within +-25 bp plus a twist within +-10 bp",
           "full_revaluation": t[0], "sub_book_ladders": t[1], "ladder_pnl": t[2],
           "speedup": t[0]["ms"] / (t[1]["ms"] + t[2]["ms"]),
           "worst_unexplained_over_largest_pnl": float((gap.abs().max() / pnl.abs().max()).item())}
result["book_context"] = context
print(json.dumps(context), flush=True)
trades.close()
grid.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps({"written": out_path}))
