"""Monte Carlo tail allocation benchmark (adr_scenario_tail_order_dev, csrc/tail_select.hip; adr_shock_gather_dev and
adr_tail_components_dev, csrc/tail_order.hip): the firm's VaR and ES and every desk's share under S normal scenarios, B
desks' ladders on P = F = 32 pillars, level 0.99.

Timed on one device and one stream, inputs and buffers resident, medians of warm repetitions between HIP events with the
routes of a case alternating in one process (the method of tools/bench_monte_carlo_var.py); host routes by the host clock
around work that ends in a synchronise, ONCE per case (they take seconds), so they carry no spread:
  1. the ordered select alone on a [1, S] row (the firm's P&L);
  2. the whole chain: column sums of the ladder rows, shocks, the firm's P&L, ordered select, gather, and per tile of desks
     adr_ladder_pnl_dev on the k gathered shocks and the components;
  3. the two routes the library has for the same answer without it, from the same shocks: the full-matrix device route
     (adr_ladder_pnl_dev on [B, S], then adr_scenario_tail_alloc_select_dev) where the matrix stays under FULL_BYTES, and
     at B = 100 tiles of adr_ladder_pnl_dev, the download and `_allocate_tail_numpy` by the host clock;
  4. the yardstick: `monte_carlo_var_es`' device steps on the same desks (shocks, then adr_ladder_pnl_dev and
     adr_scenario_tail_select_dev per tile under max_bytes), and `monte_carlo_allocate_tail` end to end by the host clock.
The chain prices 1 + B k / S ladder rows' worth of [*, S] P&L where the yardstick prices B.
usage: bench_monte_carlo_alloc.py [reps] [out.json] [B,B,..] [S,S,..]"""
import json, os, socket, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from adrates_amd import _native
from adrates_amd.market.position.monte_carlo import factor_from_covariance, monte_carlo_allocate_tail
from adrates_amd.market.position.scenarios import _allocate_tail_numpy, tail_count

reps = max(3, int(sys.argv[1]) if len(sys.argv) > 1 else 7)
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "monte_carlo_alloc_bench.json")
DESKS = tuple(int(v) for v in sys.argv[3].split(",")) if len(sys.argv) > 3 else (100, 1000, 10000)
SCENARIOS = tuple(int(v) for v in sys.argv[4].split(",")) if len(sys.argv) > 4 else (65536, 262144, 786432)
P = F = 32
LEVEL, MAX_BYTES, FULL_BYTES, HOST_DESKS = 0.99, 2 ** 31, 2 ** 33, 100
dev = torch.device("cuda", 0)
ctx = _native.default_context(0)
stream = torch.cuda.Stream(dev)
q = stream.cuda_stream


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


def new(*shape, dtype=torch.float64):
    return torch.empty(shape, dtype=dtype, device=dev)


def tiles_of(B, per_desk_bytes):
    tile = int(max(1, min(B, MAX_BYTES // per_desk_bytes)))
    return tile, [(b0, min(tile, B - b0)) for b0 in range(0, B, tile)]


rng = np.random.default_rng(2026)
A = rng.standard_normal((P, P + 4))
L = factor_from_covariance(A @ A.T * 4.0)                           # bp^2
d_L = torch.from_numpy(L).to(dev)
width = 1 + P + P * P
result = {"reps": reps, "pillars": P, "factors": F, "level": LEVEL, "max_bytes": MAX_BYTES, "full_matrix_bytes": FULL_BYTES,
          "box": {"host": socket.gethostname(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                  "hip": getattr(torch.version, "hip", None)}, "cases": [], "not_measured": []}

for B in DESKS:
    rows = rng.standard_normal((B, width)) * np.r_[0.0, np.full(P, 1e4), np.full(P * P, 30.0)]
    ladders = torch.from_numpy(rows).to(dev)
    for S in SCENARIOS:
        k = tail_count(LEVEL, S)
        x, firm, tot, gathered = new(S, P), new(width), new(S), new(k, P)
        order, out = new(k, dtype=torch.int64), new(2, B + 1)
        tile_k, tiles_k = tiles_of(B, 8 * k)
        tile_s, tiles_s = tiles_of(B, 8 * S)
        pnl_k, pnl_s, var_es = new(tile_k, k), new(tile_s, S), new(2, B)
        work = new(_native.scenario_tail_order_work(1, S, k), dtype=torch.uint8)
        work_s = new(max(_native.scenario_tail_select_work(nb, S, k) for _, nb in tiles_s), dtype=torch.uint8)
        lp, wp = ladders.data_ptr(), 8 * width

        def gen():
            _native.shock_normal_dev(ctx, 7, 0, S, P, F, d_L.data_ptr(), False, x.data_ptr(), stream=q)

        def select():
            _native.scenario_tail_order_dev(ctx, 1, S, tot.data_ptr(), k, order.data_ptr(), out.data_ptr() + 8 * B,
                                            out.data_ptr() + 8 * (2 * B + 1), work.data_ptr(), stream=q)

        def chain():
            _native.scenario_total_dev(ctx, B, width, lp, firm.data_ptr(), stream=q)
            gen()
            _native.ladder_pnl_dev(ctx, 1, P, firm.data_ptr(), S, x.data_ptr(), tot.data_ptr(), stream=q)
            select()
            _native.shock_gather_dev(ctx, k, P, x.data_ptr(), S, order.data_ptr(), gathered.data_ptr(), stream=q)
            for b0, nb in tiles_k:
                _native.ladder_pnl_dev(ctx, nb, P, lp + wp * b0, k, gathered.data_ptr(), pnl_k.data_ptr(), stream=q)
                _native.tail_components_dev(ctx, nb, k, pnl_k.data_ptr(), out.data_ptr() + 8 * b0, out.data_ptr() + 8 * (B + 1 + b0),
                                            stream=q)

        def var_es_chain():
            gen()
            for b0, nb in tiles_s:
                _native.ladder_pnl_dev(ctx, nb, P, lp + wp * b0, S, x.data_ptr(), pnl_s.data_ptr(), stream=q)
                _native.scenario_tail_select_dev(ctx, nb, S, pnl_s.data_ptr(), k, var_es.data_ptr() + 8 * b0,
                                                 var_es.data_ptr() + 8 * (B + b0), work_s.data_ptr(), stream=q)

        routes, names = [chain, select, var_es_chain], ["chain", "ordered_select", "monte_carlo_var_es_steps"]
        full = 8 * B * S <= FULL_BYTES
        if full:
            pnl_full = pnl_s if tile_s == B else new(B, S)
            out_full = new(2, B + 1)
            work_full = new(_native.scenario_tail_alloc_select_work(B, S, k), dtype=torch.uint8)

            def full_matrix():
                gen()
                _native.ladder_pnl_dev(ctx, B, P, lp, S, x.data_ptr(), pnl_full.data_ptr(), stream=q)
                p = out_full.data_ptr()
                _native.scenario_tail_alloc_select_dev(ctx, B, S, pnl_full.data_ptr(), k, p + 8 * B, p + 8 * (2 * B + 1), p,
                                                       p + 8 * (B + 1), work_full.data_ptr(), stream=q)
            routes.append(full_matrix)
            names.append("full_matrix_device_route")
        else:
            result["not_measured"].append({"desks": B, "scenarios": S, "route": "full_matrix_device_route",
                                           "why": f"the [B, S] P&L matrix of {8 * B * S} bytes exceeds {FULL_BYTES}"})
        t = timed(routes, reps)
        case = {"desks": B, "scenarios": S, "tail_count": k, "desks_per_tile_chain": tile_k, "desks_per_tile_var_es": tile_s,
                "ladder_rows_priced_chain": 1.0 + B * k / S, "ladder_rows_priced_var_es": float(B)}
        case.update(dict(zip(names, t)))
        case["chain_over_var_es_steps"] = case["chain"]["ms"] / case["monte_carlo_var_es_steps"]["ms"]
        if full:
            # the same components bit for bit; the firm's figures differ by the documented rounding
            a, b = out.cpu().numpy(), out_full.cpu().numpy()
            case["components_equal_full_matrix_route"] = bool(np.array_equal(a[:, :B].view(np.int64), b[:, :B].view(np.int64)))
            case["firm_var_es_rel_difference"] = [float(abs(a[i, B] - b[i, B]) / abs(b[i, B])) for i in (0, 1)]
            case["full_matrix_over_chain"] = case["full_matrix_device_route"]["ms"] / case["chain"]["ms"]
            if pnl_full is not pnl_s:
                del pnl_full
            del work_full
        if B == HOST_DESKS:
            held = {}

            def host_route():
                pnl = np.empty((B, S))
                for b0, nb in tiles_s:
                    _native.ladder_pnl_dev(ctx, nb, P, lp + wp * b0, S, x.data_ptr(), pnl_s.data_ptr(), stream=q)
                    stream.synchronize()
                    pnl[b0:b0 + nb] = pnl_s[:nb].cpu().numpy()
                held["out"] = _allocate_tail_numpy(pnl, k, -1)
            gen()
            case["tiles_download_numpy_ms"] = host_ms(host_route)
            case["numpy_route_over_chain"] = case["tiles_download_numpy_ms"] / case["chain"]["ms"]
            case["components_equal_numpy_route"] = bool(np.array_equal(held["out"]["comp_es"], out[1, :B].cpu().numpy()))
        else:
            result["not_measured"].append({"desks": B, "scenarios": S, "route": "tiles_download_numpy",
                                           "why": f"timed at B = {HOST_DESKS} only"})
        delta, gamma = rows[:, 1:1 + P], rows[:, 1 + P:].reshape(B, P, P)
        end_to_end = lambda: monte_carlo_allocate_tail(delta, gamma, L, S, level=LEVEL, seed=7, ctx=ctx, max_bytes=MAX_BYTES)
        end_to_end()
        case["monte_carlo_allocate_tail_host_clock_ms"] = host_ms(end_to_end)
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
        del x, tot, gathered, pnl_k, pnl_s, work, work_s
        torch.cuda.empty_cache()

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps({"written": out_path}))
