"""Monte Carlo VaR by full revaluation benchmark (adr_curve_dfs_shocked_dev, csrc/curve_dfs.hip, and
adr_scenario_rows_place_dev, csrc/shock_columns.hip; `monte_carlo_revalue_var_es`' chain): n synthetic off-grid OIS on the README GBP curve (K = 264 knots,
P = F = 32), cut into B desks of equal size, under S normal scenarios, level 0.99.

Timed on one device and one stream, inputs and buffers resident, medians of warm repetitions between HIP events:
  1. the bootstrap alone: adr_curve_dfs_shocked_dev over the S shock rows, tile by tile;
  2. the chain - shocks, then per tile of scenarios the bootstrap, adr_scenario_subbook_pv_dev and the copy into the
     [B, S + 1] rows, the base column, adr_scenario_tail_select_dev - and its split, from events between the steps of the
     same run (so the parts add up to the chain but for the events themselves);
  3. the route the library had for the same figures before: `ScenarioGrid(..., with_gamma=False)` over the SAME shock rows
     as a Python list of `Shock` dicts, then `pnl_sub_books`, then `tail_measures_select`, by the host clock, ONCE (it takes
     seconds, so it carries no spread), at B = COMPARE_DESKS and the largest S of the list whose curve set the device
     takes (a refused allocation moves on to the next smaller S; which S it was is recorded).
usage: bench_monte_carlo_revalue.py [reps] [out.json] [n,n,..] [S,S,..] [B,B,..] [largest S of the comparison]"""
import json, os, socket, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from adrates_amd import _native
from adrates_amd.market.position.monte_carlo import (ShockedCurves, _tile_of, factor_from_covariance, revalue_scenario_bytes,
                                                     tail_measures_select)
from adrates_amd.market.position.scenarios import ScenarioGrid, tail_count
from adrates_amd.trades import synthetic
from adrates_amd.trades.market_data import README_VALUE_DT, TENORS, gbp_model
from adrates_amd.utils import InterpTypes
from adrates_amd.utils.error import LibError

ints = lambda i, default: tuple(int(v) for v in sys.argv[i].split(",")) if len(sys.argv) > i else default
reps = max(3, int(sys.argv[1]) if len(sys.argv) > 1 else 5)
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "monte_carlo_revalue_bench.json")
TRADES, SCENARIOS, DESKS = ints(3, (100_000, 1_000_000)), ints(4, (16384, 65536, 262144)), ints(5, (1, 100, 1000))
COMPARE_MAX = int(sys.argv[6]) if len(sys.argv) > 6 else max(SCENARIOS)
LEVEL, MAX_BYTES, COMPARE_DESKS, SEED = 0.99, 2 ** 33, 100, 7
dev = torch.device("cuda", 0)
ctx = _native.default_context(0)
stream = torch.cuda.Stream(dev)
q = stream.cuda_stream
new = lambda *shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device=dev)
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
event = lambda: torch.cuda.Event(enable_timing=True)

model = gbp_model(README_VALUE_DT, InterpTypes.FLAT_FWD_RATES)
curves = ShockedCurves(model, "GBP_OIS_SONIA", ctx=ctx)
plan, K, P = curves.plan(), curves.n_knots, curves.n_pillars
rng = np.random.default_rng(2026)
A = rng.standard_normal((P, P + 4))
L = factor_from_covariance(A @ A.T * 4.0)                           # bp^2: a daily move of about 12 bp per quote
d_L, d_times, d_base, d_zero = up(L), up(curves.base.times), up(curves.rates), up(np.zeros(P))
result = {"reps": reps, "knots": K, "pillars": P, "level": LEVEL, "max_bytes": MAX_BYTES,
          "box": {"host": socket.gethostname(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                  "hip": getattr(torch.version, "hip", None)}, "cases": [], "comparison": [], "not_measured": []}


def stats(t):
    return {"ms": float(np.median(t)), "spread": (max(t) - min(t)) / float(np.median(t))}


def host_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


for n in TRADES:
    batch = synthetic.synthesize(README_VALUE_DT, n, seed=11)
    with _native.DeviceTrades(ctx, batch) as trades:
        for B in DESKS:
            sub_off = np.linspace(0, n, B + 1).astype(np.int64)
            d_plan = up(_native.scenario_subbook_plan(n, sub_off))
            for S in SCENARIOS:
                try:
                    tile = _tile_of(revalue_scenario_bytes(curves, n, B), B, S, MAX_BYTES)
                except LibError as e:
                    result["not_measured"].append({"trades": n, "desks": B, "scenarios": S, "why": str(e)})
                    continue
                k = tail_count(LEVEL, S)
                tiles = [(s0, min(tile, S - s0)) for s0 in range(0, S, tile)]
                x, rows, var_es = new(S, P), new(B, S + 1), new(2, B)
                dfs, work_b, part = new(tile, K), new(_native.curve_dfs_shocked_work(plan, tile)), new(B, tile)
                work_s = new(_native.scenario_subbook_work(n, B, tile))
                work_t = new(_native.scenario_tail_select_work(B, S + 1, k), dtype=torch.uint8)
                bad = torch.zeros(S + 1, dtype=torch.int32, device=dev)

                def boot(s0, nt, x_ptr):
                    _native.curve_dfs_shocked_dev(ctx, plan, d_base.data_ptr(), nt, P, x_ptr, dfs.data_ptr(), work_b.data_ptr(),
                                                  bad_ptr=bad.data_ptr() + 4 * s0, stream=q)

                def price(s0, nt):
                    _native.scenario_subbook_pv_dev(ctx, curves.method, K, d_times.data_ptr(), nt, dfs.data_ptr(), trades, B,
                                                    d_plan.data_ptr(), part.data_ptr(), work_s.data_ptr(), stream=q)
                    _native.scenario_rows_place_dev(ctx, B, nt, part.data_ptr(), S + 1, s0, rows.data_ptr(), stream=q)

                def chain(marks=None):
                    """The chain; ``marks``: a list that takes (part, start event, end event) of every step."""
                    def step(name, f, *args):
                        a, b = event(), event()
                        if marks is not None:
                            a.record(stream)
                        f(*args)
                        if marks is not None:
                            b.record(stream)
                            marks.append((name, a, b))
                    step("shocks", _native.shock_normal_dev, ctx, SEED, 0, S, P, P, d_L.data_ptr(), False, x.data_ptr(), q)
                    for s0, nt in tiles:
                        step("bootstrap", boot, s0, nt, x.data_ptr() + 8 * P * s0)
                        step("pricing", price, s0, nt)
                    step("bootstrap", boot, S, 1, d_zero.data_ptr())
                    step("pricing", price, S, 1)
                    step("tail", _native.scenario_tail_select_dev, ctx, B, S + 1, rows.data_ptr(), k, var_es.data_ptr(),
                         var_es.data_ptr() + 8 * B, work_t.data_ptr(), S, q)

                def bootstrap_alone():
                    for s0, nt in tiles:
                        boot(s0, nt, x.data_ptr() + 8 * P * s0)

                with torch.cuda.stream(stream):
                    chain()
                    bootstrap_alone()
                    stream.synchronize()
                    runs = []
                    for _ in range(reps):
                        marks, a, b, c = [], event(), event(), event()
                        a.record(stream); chain(marks); b.record(stream); bootstrap_alone(); c.record(stream)
                        runs.append((marks, a, b, c))
                torch.cuda.synchronize()
                assert int(bad.count_nonzero()) == 0
                parts = {name: stats([sum(s.elapsed_time(e) for m, s, e in marks if m == name) for marks, *_ in runs])
                         for name in ("shocks", "bootstrap", "pricing", "tail")}
                case = {"trades": n, "desks": B, "scenarios": S, "tail_count": k, "scenarios_per_tile": tile, "tiles": len(tiles),
                        "scenario_bytes": revalue_scenario_bytes(curves, n, B), "dfs_bytes": 8 * K * S,
                        "chain": stats([a.elapsed_time(b) for _, a, b, _ in runs]),
                        "bootstrap_alone": stats([b.elapsed_time(c) for _, _, b, c in runs]), "split": parts}
                case["bootstrap_share_of_chain"] = parts["bootstrap"]["ms"] / case["chain"]["ms"]
                case["bootstrap_GB_per_s_of_dfs"] = 8e-6 * K * S / case["bootstrap_alone"]["ms"]
                result["cases"].append(case)
                print(json.dumps(case), flush=True)

                if B == COMPARE_DESKS and S == max((s for s in SCENARIOS if s <= COMPARE_MAX), default=0):
                    chain_var = var_es[0].cpu().numpy()
                    shocks_bp = x.cpu().numpy()
                    keys = [int(b) for b in np.repeat(np.arange(B), np.diff(sub_off))]
                    for Sc in sorted((s for s in SCENARIOS if s <= COMPARE_MAX), reverse=True):
                        rec = {"trades": n, "desks": B, "scenarios": Sc}
                        try:
                            # quotes are in percent: 100 bp per unit
                            t_list, shocks = host_ms(lambda: [dict(zip(TENORS, row)) for row in (shocks_bp[:Sc] / 100.0).tolist()])
                            t_grid, grid = host_ms(lambda: ScenarioGrid(model, "GBP_OIS_SONIA", shocks, with_gamma=False, ctx=ctx))
                        except (LibError, RuntimeError, MemoryError) as e:
                            rec["refused"] = str(e)[:200]
                            result["comparison"].append(rec)
                            continue
                        t_pnl, pnl = host_ms(lambda: grid.pnl_sub_books(batch, keys))
                        t_tail, (var, es) = host_ms(lambda: tail_measures_select(pnl, LEVEL, ctx=ctx))
                        grid.close()
                        rec.update(shock_list_ms=t_list, scenario_grid_ms=t_grid, pnl_sub_books_ms=t_pnl, tail_measures_select_ms=t_tail,
                                   total_ms=t_list + t_grid + t_pnl + t_tail)
                        if Sc == S:
                            rec["var_rel_difference_to_chain"] = float(np.max(np.abs(var - chain_var) / np.abs(chain_var)))
                            rec["over_chain"] = rec["total_ms"] / case["chain"]["ms"]
                        result["comparison"].append(rec)
                        print(json.dumps(rec), flush=True)
                        break
                del x, rows, dfs, work_b, part, work_s, work_t
                torch.cuda.empty_cache()

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps({"written": out_path}))
