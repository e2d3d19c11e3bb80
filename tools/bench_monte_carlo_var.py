"""Monte Carlo delta-gamma VaR benchmark (adr_shock_normal_dev, csrc/shock_normal.hip; adr_scenario_tail_select_dev,
csrc/tail_select.hip): B desks' ladders on P = F = 32 pillars under S normal scenarios.

Timed on one device, inputs resident, medians of warm repetitions between HIP events with the routes of a comparison
alternating in one process (the method of tools/bench_ladder_pnl.py); host routes by the host clock around work that ends
in a synchronise, ONCE per case (they take seconds), so they carry no spread:
  1. shock generation alone, against numpy.random.Generator.standard_normal @ factor.T plus the upload;
  2. adr_scenario_tail_select_dev alone, against the route the library had for such rows - download [B, S] and
     `tail_measures`' NumPy branch (rows of 16 384: its kernel through the blocking entry, upload included) - and at
     S = 16 384 against adr_scenario_tail_dev, which sorts the whole row in LDS and bounds the overhead of the rounds;
  3. the whole chain shocks -> adr_ladder_pnl_dev -> select on one stream, and `monte_carlo_var_es` end to end by the
     host clock (allocations, uploads and the download of var and es included).
The select reads the [B, S] matrix seven times (six count rounds and the gather); its bytes/s count 7 * 8 B S over the
time of the whole entry (scans, tail kernel and NaN patch included) against the 8 TB/s roofline of HBM.  Combinations
whose P&L matrix would exceed max_bytes (2 GiB) untiled are skipped, and so is the host route above 1.1e8 values.
usage: bench_monte_carlo_var.py [reps] [out.json]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from adrates_amd import _native
from adrates_amd.market.position.monte_carlo import factor_from_covariance, monte_carlo_var_es
from adrates_amd.market.position.scenarios import tail_count, tail_measures

reps = max(3, int(sys.argv[1]) if len(sys.argv) > 1 else 7)
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "monte_carlo_var_bench.json")
P = F = 32
LEVEL, MAX_BYTES, HOST_VALUES, ROOFLINE = 0.99, 2 ** 31, 1.1e8, 8e12
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


def host_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


rng = np.random.default_rng(2026)
A = rng.standard_normal((P, P + 4))
cov = A @ A.T * 4.0                                                 # bp^2
L = factor_from_covariance(cov)
d_L = torch.from_numpy(L).to(dev)
result = {"reps": reps, "pillars": P, "factors": F, "level": LEVEL, "max_bytes": MAX_BYTES, "shocks": [], "cases": [], "skipped": []}

# 1. shock generation alone
for S in (16384, 65536, 262144, 1048576):
    x = torch.empty((S, P), dtype=torch.float64, device=dev)
    gen = lambda: _native.shock_normal_dev(ctx, 7, 0, S, P, F, d_L.data_ptr(), False, x.data_ptr(), stream=stream.cuda_stream)
    t = timed([gen], reps)[0]

    def numpy_route():
        z = np.random.default_rng(7).standard_normal((S, F))
        x.copy_(torch.from_numpy(z @ L.T))
    numpy_route()
    case = {"scenarios": S, "kernel": t, "numpy_and_upload_ms": host_ms(numpy_route),
            "stored_bytes_per_s": 8.0 * S * P / (t["ms"] * 1e-3), "normals_per_s": S * F / (t["ms"] * 1e-3)}
    case["speedup"] = case["numpy_and_upload_ms"] / t["ms"]
    result["shocks"].append(case)
    print(json.dumps(case), flush=True)
    del x

# 2. and 3. the select alone and the whole chain
for B in (1, 100, 1000):
    ladders = torch.from_numpy(rng.standard_normal((B, 1 + P + P * P)) * np.r_[0.0, np.full(P, 1e4), np.full(P * P, 30.0)]).to(dev)
    for S in (16384, 65536, 262144, 1048576):
        if 8 * B * S > MAX_BYTES:
            result["skipped"].append({"desks": B, "scenarios": S, "why": f"the [B, S] P&L matrix of {8 * B * S} bytes exceeds max_bytes untiled"})
            continue
        k = tail_count(LEVEL, S)
        x = torch.empty((S, P), dtype=torch.float64, device=dev)
        pnl = torch.empty((B, S), dtype=torch.float64, device=dev)
        var_es, whole = torch.zeros((2, B), dtype=torch.float64, device=dev), torch.zeros((2, B), dtype=torch.float64, device=dev)
        work = torch.empty(_native.scenario_tail_select_work(B, S, k), dtype=torch.uint8, device=dev)
        q = stream.cuda_stream
        gen = lambda: _native.shock_normal_dev(ctx, 7, 0, S, P, F, d_L.data_ptr(), False, x.data_ptr(), stream=q)
        price = lambda: _native.ladder_pnl_dev(ctx, B, P, ladders.data_ptr(), S, x.data_ptr(), pnl.data_ptr(), stream=q)
        select = lambda: _native.scenario_tail_select_dev(ctx, B, S, pnl.data_ptr(), k, var_es[0].data_ptr(), var_es[1].data_ptr(),
                                                          work.data_ptr(), stream=q)
        sort = lambda: _native.scenario_tail_dev(ctx, B, S, pnl.data_ptr(), k, whole[0].data_ptr(), whole[1].data_ptr(), stream=q)

        def chain():
            gen(); price(); select()
        routes = [select, chain, price] + ([sort] if S <= _native.SCENARIO_TAIL_MAX else [])
        t = timed(routes, reps)
        case = {"desks": B, "scenarios": S, "tail_count": k, "select": t[0], "chain": t[1], "ladder_pnl": t[2],
                "select_bytes_per_s": 7.0 * 8.0 * B * S / (t[0]["ms"] * 1e-3)}
        case["select_share_of_roofline"] = case["select_bytes_per_s"] / ROOFLINE
        if len(t) > 3:
            case["tail_kernel_whole_row"] = t[3]
            case["select_over_whole_row_sort"] = t[0]["ms"] / t[3]["ms"]
            case["same_bits_as_whole_row_sort"] = bool(torch.equal(var_es.view(torch.int64), whole.view(torch.int64)))
        if B * S <= HOST_VALUES:
            held = {}

            def host_route():
                held["out"] = tail_measures(pnl.cpu().numpy(), LEVEL, ctx=ctx)
            case["download_and_numpy_ms"] = host_ms(host_route)
            case["select_speedup_over_host_route"] = case["download_and_numpy_ms"] / t[0]["ms"]
            case["var_equals_host_route"] = bool(np.array_equal(held["out"][0], var_es[0].cpu().numpy()))
        else:
            case["download_and_numpy_ms"] = None                   # not measured: above 1.1e8 values it takes a minute
        delta = ladders[:, 1:1 + P].cpu().numpy()
        gamma = ladders[:, 1 + P:].reshape(B, P, P).cpu().numpy()
        end_to_end = lambda: monte_carlo_var_es(delta, gamma, L, S, level=LEVEL, seed=7, ctx=ctx, max_bytes=MAX_BYTES)
        end_to_end()
        case["monte_carlo_var_es_host_clock_ms"] = host_ms(end_to_end)
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
        del x, pnl, work
        torch.cuda.empty_cache()

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps({"written": out_path}))
