"""YoY sub-book benchmark: a million YoY swaps (`random_yoy_book`, a few hundred distinct swaps tiled) on the 20-pillar RPI
curve and the README GBP OIS curve under S = 1 024 joint scenarios, cut into B = 1, 100, 1 000 and 10 000 sub-books of
equal and of skewed (geometric) sizes, and the tail allocation kernel on [10 000, 1 024] rows.

Without arguments the tool is a driver: every case below runs as a process of its own under `timeout -k 10`, the cases
chained so that the first one that fails or runs out of time ends the run, and the cases' results are gathered into
profiles/yoy_subbook_bench.json.  With `--case NAME` it runs that case and prints one JSON line.

Timed, inputs resident, medians of warm repetitions between HIP events, the routes of a comparison alternating in one
process (the method of tools/bench_subbooks.py):
  * the ONE launch, adr_yoy_scenario_subbook_pv_dev (pricing kernel + sub-book sum), sub-book rows only;
  * B = 1: against the parent, adr_yoy_scenario_pv_dev, on the same book and S - the cost of the feature, judged against
    the (max - min) / median of either route in the same run;
  * B = 100 and 1 000: against one adr_yoy_scenario_pv_dev per sub-book (every sub-book's arrays uploaded beforehand);
  * the allocation, adr_scenario_tail_alloc_dev at B = 10 000, S = 1 024, k = 11, against downloading the [B, S] matrix
    and allocating with NumPy (column sums, argpartition, a gather).
usage: bench_yoy_subbooks.py [--case NAME] [--reps R] [--out out.json] [--n N] [--scenarios S] [--limit SECONDS]"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

CASES = ("1-equal", "100-equal", "100-geometric", "1000-equal", "1000-geometric", "10000-equal", "10000-geometric", "allocation")
LOOP_MAX_B = 1000
ap = argparse.ArgumentParser()
ap.add_argument("--case", choices=CASES)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yoy_subbook_bench.json"))
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--scenarios", type=int, default=1024)
ap.add_argument("--distinct", type=int, default=400)
ap.add_argument("--limit", type=int, default=170, help="seconds a case may take")
args = ap.parse_args()
reps, n, S = max(5, args.reps), args.n, args.scenarios

if args.case is None:
    result = {"reps": reps, "swaps": n, "scenarios": S, "cases": []}
    for name in CASES:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(reps),
               "--n", str(n), "--scenarios", str(S), "--distinct", str(args.distinct)]
        run = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if run.returncode != 0:                     # nothing more is started on the GPU after a failure
            sys.exit(f"case {name} ended with status {run.returncode}; the cases after it were not run")
        case = json.loads(run.stdout.strip().splitlines()[-1])
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
    base = result["cases"][0]["one_launch"]["ms"]
    result["growth_from_one_sub_book"] = {c["case"]: c["one_launch"]["ms"] / base for c in result["cases"] if "one_launch" in c}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"written": args.out, "growth": result["growth_from_one_sub_book"]}))
    sys.exit(0)

import torch
from adrates_amd import _native
from adrates_amd.market.position.inflation_engine import inflation_inputs
from adrates_amd.market.position.scenarios import ScenarioGrid, tail_count
from adrates_amd.market.position.yoy_book import tile_yoy_book
from adrates_amd.trades.compiler import compile_yoy_coupons, compile_yoy_fixed_legs
from adrates_amd.trades.market_data import README_VALUE_DT, TENORS, random_yoy_book, yoy_model

dev = torch.device("cuda", 0)
ctx = _native.default_context(0)
stream = torch.cuda.Stream(dev)
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


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


if args.case == "allocation":
    B, k = 10000, tail_count(0.99, S)
    rows = np.random.default_rng(8).normal(0.0, 1e6, (B, S))
    rows_t = up(rows)
    tot, cv, ce = torch.zeros(2, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.float64, device=dev), \
        torch.zeros(B, dtype=torch.float64, device=dev)
    work = torch.empty(S, dtype=torch.float64, device=dev)
    alloc = lambda: _native.scenario_tail_alloc_dev(ctx, B, S, rows_t.data_ptr(), k, tot[0:1].data_ptr(), tot[1:2].data_ptr(),
                                                    cv.data_ptr(), ce.data_ptr(), work.data_ptr(), -1, stream.cuda_stream)
    t = timed([alloc], reps)
    host_ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        host = rows_t.cpu().numpy()
        t1 = time.perf_counter()
        firm = host.sum(axis=0)
        worst = np.argpartition(firm, k - 1)[:k]
        worst = worst[np.argsort(firm[worst], kind="stable")]
        n_es, n_var = -host[:, worst].mean(axis=1), -host[:, worst[-1]]
        t2 = time.perf_counter()
        host_ms.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
    twin = _native.scenario_tail_alloc_host(rows, k)
    case = {"case": "allocation", "rows": B, "scenarios": S, "k": k,
            "adr_scenario_tail_alloc_dev": {"ms": t[0][0], "spread": t[0][1], "input_GBps": B * S * 8 / t[0][0] / 1e6},
            "download_and_numpy": {"download_ms": float(np.median([h[0] for h in host_ms])),
                                   "numpy_ms": float(np.median([h[1] for h in host_ms]))},
            "bits_equal_host_twin": bool(np.array_equal(cv.cpu().numpy(), twin["comp_var"]) and
                                         np.array_equal(ce.cpu().numpy(), twin["comp_es"]) and
                                         tot.cpu().numpy().tolist() == [twin["var"], twin["es"]]),
            "agrees_with_numpy": bool(np.array_equal(cv.cpu().numpy(), n_var) and
                                      np.allclose(ce.cpu().numpy(), n_es, rtol=1e-12, atol=1e-6))}
    print(json.dumps(case), flush=True)
    sys.exit(0)

B, dist = int(args.case.split("-")[0]), args.case.split("-")[1]


def disc_shocks(count):
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


model = yoy_model()
im, T, b0 = inflation_inputs(model.curves.GBP_RPI_INFLATION)
P = T.size
swaps = random_yoy_book(README_VALUE_DT, args.distinct, seed=17)
base_cpn, base_fix = compile_yoy_coupons(swaps, README_VALUE_DT), compile_yoy_fixed_legs(swaps, README_VALUE_DT)
grid = ScenarioGrid(model, "GBP_OIS_SONIA", disc_shocks(S), with_gamma=False, ctx=ctx)
arr = _native.curve_set_arrays(grid._set)
K, dm = arr["K"], arr["method"]
rng = np.random.default_rng(S + 1)
slope = np.linspace(-1.0, 1.0, P)
b_t = up(b0[None, :] + (rng.uniform(-100, 100, S)[:, None] + rng.uniform(-30, 30, S)[:, None] * slope[None, :]) * 1e-4)
r = -(-n // args.distinct)
big = tile_yoy_book(base_cpn, r)
m = int(big["cpn_off"][n])
cpn_off = big["cpn_off"][:n + 1]
cpn = np.stack([big[f][:m] for f in _native.YOY_FIELDS])
fix_off = np.concatenate(([0], np.cumsum(np.tile(np.diff(base_fix[0]), r)[:n]))).astype(np.int64)
mf = int(fix_off[-1])
fix_tp, fix_pay = np.tile(base_fix[1], r)[:mf], np.tile(base_fix[2], r)[:mf]
t = {k: up(v) for k, v in dict(T=T, fix_off=fix_off, fix_tp=fix_tp, fix_pay=fix_pay, cpn_off=cpn_off, cpn=cpn).items()}
sizes = sizes_of(B, dist)
sub_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
plan = up(_native.scenario_subbook_plan(n, sub_off))
ptrs = {k: v.data_ptr() for k, v in t.items()}
ptrs.update(times=arr["times"], dfs=arr["dfs"], b=b_t.data_ptr(), plan=plan.data_ptr())
sub = torch.zeros((B, S), dtype=torch.float64, device=dev)
work = torch.empty(_native.scenario_subbook_work(n, B, S), dtype=torch.float64, device=dev)
one = lambda: _native.yoy_scenario_subbook_pv_dev(ctx, dm, K, S, im, P, S, S, n, mf, m, B, ptrs, sub.data_ptr(), work.data_ptr(), 0,
                                                  stream.cuda_stream)
case = {"case": args.case, "sub_books": B, "sizes": dist, "largest": int(sizes.max()), "smallest": int(sizes.min()),
        "chunks": int(plan[B].item()), "knots": K, "inflation_pillars": P, "coupons_per_swap": m / n}
routes = [one]
if B == 1:
    book = torch.zeros(S, dtype=torch.float64, device=dev)
    pwork = torch.empty(_native.yoy_scenario_pv_work(n, S), dtype=torch.float64, device=dev)
    routes.append(lambda: _native.yoy_scenario_pv_dev(ctx, dm, K, S, im, P, S, S, n, mf, m, ptrs, book.data_ptr(), pwork.data_ptr(), 0,
                                                      stream.cuda_stream))
elif B <= LOOP_MAX_B:
    # one launch per desk: the sub-book's offsets rebased, its flows read where the whole book's lie
    pieces = []
    for lo, hi in zip(sub_off[:-1], sub_off[1:]):
        fo, co = up(fix_off[lo:hi + 1] - fix_off[lo]), up(cpn_off[lo:hi + 1] - cpn_off[lo])
        sub_cpn = up(cpn[:, cpn_off[lo]:cpn_off[hi]])
        p = dict(ptrs, fix_off=fo.data_ptr(), cpn_off=co.data_ptr(), cpn=sub_cpn.data_ptr(),
                 fix_tp=ptrs["fix_tp"] + 8 * int(fix_off[lo]), fix_pay=ptrs["fix_pay"] + 8 * int(fix_off[lo]))
        pieces.append((int(hi - lo), int(fix_off[hi] - fix_off[lo]), int(cpn_off[hi] - cpn_off[lo]), p, (fo, co, sub_cpn)))
    rows = torch.zeros((B, S), dtype=torch.float64, device=dev)
    lwork = torch.empty(_native.yoy_scenario_pv_work(int(sizes.max()), S), dtype=torch.float64, device=dev)

    def loop():
        for j, (nb, mfb, mb, p, _) in enumerate(pieces):
            _native.yoy_scenario_pv_dev(ctx, dm, K, S, im, P, S, S, nb, mfb, mb, p, rows[j].data_ptr(), lwork.data_ptr(), 0,
                                        stream.cuda_stream)
    routes.append(loop)
tm = timed(routes, reps)
case["one_launch"] = {"ms": tm[0][0], "spread": tm[0][1], "scenario_swaps_per_s": n * S / tm[0][0] * 1e3}
if B == 1:
    case["parent_adr_yoy_scenario_pv_dev"] = {"ms": tm[1][0], "spread": tm[1][1]}
    case["cost_of_the_feature"] = tm[0][0] / tm[1][0] - 1.0
    case["margin"] = max(tm[0][1], tm[1][1])
    case["bits_equal_parent"] = bool(torch.equal(sub[0], book))
elif B <= LOOP_MAX_B:
    case["loop_of_adr_yoy_scenario_pv_dev"] = {"ms": tm[1][0], "spread": tm[1][1]}
    case["speedup"] = tm[1][0] / tm[0][0]
    case["bits_equal_loop"] = bool(torch.equal(sub, rows))
grid.close()
print(json.dumps(case), flush=True)
