"""Sub-book scenario benchmark: the benchmark book (`synthesize`, off-grid OIS, a million trades) on the README GBP curve
under S = 1 024 par-rate scenarios, cut into B = 1, 100, 1 000 and 10 000 sub-books of equal and of skewed (geometric)
sizes.

Timed, inputs resident, medians of warm repetitions between HIP events, the routes of a comparison alternating in one
process (the method of tools/bench_scenarios.py):
  * the ONE launch, adr_scenario_subbook_pv_dev (pricing kernel + sub-book sum), book rows only;
  * the tail kernel, adr_scenario_tail_dev, on the [B, S] rows it leaves;
  * the route it replaces: one adr_scenario_pv_dev per sub-book on sub-books uploaded beforehand.  The loop is timed for
    B = 100 and B = 1 000; at B = 10 000 it needs ten thousand uploads before it starts and is left out;
  * the cost of the feature: the launch at B = 1 against adr_scenario_pv_dev on the same batch and S;
  * the tail kernel at B = 10 000 against downloading the [B, S] matrix and sorting it with NumPy.
usage: bench_subbooks.py [reps] [out.json] [n] [S]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from adrates_amd import _native
from adrates_amd.market.position.scenarios import ScenarioGrid, _permute_batch, tail_count
from adrates_amd.trades import synthetic
from adrates_amd.trades.market_data import README_VALUE_DT, TENORS, gbp_model
from adrates_amd.utils import InterpTypes

reps = max(3, int(sys.argv[1]) if len(sys.argv) > 1 else 5)
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "subbook_scenarios_bench.json")
n = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
S = int(sys.argv[4]) if len(sys.argv) > 4 else 1024
LOOP_MAX_B = 1000
dev = torch.device("cuda", 0)
ctx = _native.default_context(0)
stream = torch.cuda.Stream(dev)


def shocks(count):
    rng = np.random.default_rng(count)
    slope = np.linspace(-1.0, 1.0, len(TENORS))
    par, twist = rng.uniform(-1.5, 1.5, count), rng.uniform(-0.5, 0.5, count)
    return [{t: float(par[i] + twist[i] * slope[k]) for k, t in enumerate(TENORS)} for i in range(count)]


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


model = gbp_model(README_VALUE_DT, InterpTypes.LINEAR_ZERO_RATES)
grid = ScenarioGrid(model, "GBP_OIS_SONIA", shocks(S), with_gamma=False, ctx=ctx)
arr = _native.curve_set_arrays(grid._set)
K = arr["K"]
batch = synthetic.synthesize(README_VALUE_DT, n)
trades = _native.DeviceTrades(ctx, batch)
k_tail = tail_count(0.99, S)
result = {"reps": reps, "trades": n, "scenarios": S, "knots": K, "scheme": "LINEAR_ZERO_RATES", "tail_k": k_tail, "cases": []}

for B, dist in ((1, "equal"), (100, "equal"), (100, "geometric"), (1000, "equal"), (1000, "geometric"), (10000, "equal"),
                (10000, "geometric")):
    sizes = sizes_of(B, dist)
    sub_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    plan = torch.from_numpy(_native.scenario_subbook_plan(n, sub_off)).to(dev)
    sub = torch.zeros((B, S), dtype=torch.float64, device=dev)
    work = torch.empty(_native.scenario_subbook_work(n, B, S), dtype=torch.float64, device=dev)
    var, es = torch.zeros(B, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.float64, device=dev)
    one = lambda: _native.scenario_subbook_pv_dev(ctx, arr["method"], K, arr["times"], S, arr["dfs"], trades, B, plan.data_ptr(),
                                                  sub.data_ptr(), work.data_ptr(), 0, stream.cuda_stream)
    tail = lambda: _native.scenario_tail_dev(ctx, B, S, sub.data_ptr(), k_tail, var.data_ptr(), es.data_ptr(), -1, stream.cuda_stream)
    case = {"sub_books": B, "sizes": dist, "largest": int(sizes.max()), "smallest": int(sizes.min()),
            "chunks": int(plan[B].item())}
    routes = [one, tail]
    if B == 1:
        book = torch.zeros(S, dtype=torch.float64, device=dev)
        pwork = torch.empty(_native.scenario_pv_work(n, S), dtype=torch.float64, device=dev)
        routes.append(lambda: _native.scenario_pv_dev(ctx, arr["method"], K, arr["times"], S, arr["dfs"], trades, book.data_ptr(),
                                                      pwork.data_ptr(), 0, stream.cuda_stream))
    elif B <= LOOP_MAX_B:
        pieces = [_native.DeviceTrades(ctx, _permute_batch(batch, np.arange(lo, hi, dtype=np.int64))[0])
                  for lo, hi in zip(sub_off[:-1], sub_off[1:])]
        rows = torch.zeros((B, S), dtype=torch.float64, device=dev)
        lwork = torch.empty(_native.scenario_pv_work(int(sizes.max()), S), dtype=torch.float64, device=dev)

        def loop():
            for b, piece in enumerate(pieces):
                _native.scenario_pv_dev(ctx, arr["method"], K, arr["times"], S, arr["dfs"], piece, rows[b].data_ptr(),
                                        lwork.data_ptr(), 0, stream.cuda_stream)
        routes.append(loop)
    t = timed(routes, reps)
    case["one_launch"] = {"ms": t[0][0], "spread": t[0][1], "scenario_trades_per_s": n * S / t[0][0] * 1e3}
    case["tail_kernel"] = {"ms": t[1][0], "spread": t[1][1]}
    if B == 1:
        case["parent_adr_scenario_pv_dev"] = {"ms": t[2][0], "spread": t[2][1]}
        case["cost_of_the_feature"] = t[0][0] / t[2][0] - 1.0
        case["margin"] = max(t[0][1], t[2][1])
        case["bits_equal_parent"] = bool(torch.equal(sub[0], book))
    elif B <= LOOP_MAX_B:
        case["loop_of_adr_scenario_pv_dev"] = {"ms": t[2][0], "spread": t[2][1]}
        case["speedup"] = t[2][0] / t[0][0]
        case["bits_equal_loop"] = bool(torch.equal(sub, rows))
        for piece in pieces:
            piece.close()
    if B == 10000:
        t0 = time.perf_counter()
        host = sub.cpu().numpy()
        t1 = time.perf_counter()
        part = np.sort(np.partition(host, k_tail - 1, axis=1)[:, :k_tail], axis=1)
        nv, ne = -part[:, -1], -part.mean(axis=1)
        t2 = time.perf_counter()
        case["download_and_numpy"] = {"download_ms": (t1 - t0) * 1e3, "numpy_partition_ms": (t2 - t1) * 1e3}
        case["tail_agrees_with_numpy"] = bool(np.array_equal(var.cpu().numpy(), nv) and
                                              np.allclose(es.cpu().numpy(), ne, rtol=1e-13, atol=0.0))
    result["cases"].append(case)
    print(json.dumps(case), flush=True)
base = result["cases"][0]["one_launch"]["ms"]
result["growth_from_one_sub_book"] = {f"{c['sub_books']} {c['sizes']}": c["one_launch"]["ms"] / base for c in result["cases"]}
trades.close()
grid.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps({"written": out_path, "growth": result["growth_from_one_sub_book"]}))
