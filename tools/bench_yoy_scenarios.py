"""Inflation scenario revaluation benchmark: a book of YoY swaps (`random_yoy_book`, annual coupons, 5-30Y; a few hundred
distinct swaps compiled once and tiled to 200 000 and a million) on the 20-pillar RPI curve and the README GBP OIS
curve (32 pillars, 264 knots) under S joint scenarios - par-rate shifts and twists of the OIS curve bootstrapped by the
device builder, paired with breakeven shifts and twists - book PV only and, where the rows fit in memory, per swap.

Two routes for the same numbers, timed in the same process and alternating: ONE launch of adr_yoy_scenario_pv_dev, and
the best device-side route without it - per scenario one adr_yoy_risk_dev(VALUE, ADR_YOY_AGG) on that scenario's pair
(the inflation leg of the book), plus ONE adr_scenario_pv_dev over the fixed legs for all S.  Times are medians of warm
repetitions between HIP events, inputs resident.  The two routes' book PVs of the timed run must agree to 1e-10 per
unit notional (asserted).

The share of the fp64 vector peak uses an instruction count computed from the book by the kernel's own sharing rules:
per scenario one exp per live coupon's D(tp) and one per YoY ratio, with the fp64 instructions each expands to on
gfx950 counted from the ISA as tools/bench_scenarios.py counts them (exp: 19), 3 per weighted sum of two knots (two
mul, one add: contraction is off), 6 per coupon for (y + spread) scale D and the sums, 2 per fixed flow; against
78.6 TFLOP/s = 39.3 T fp64 instructions per second.
usage: bench_yoy_scenarios.py [reps] [out.json] [n_big] [n_small] [distinct]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from adrates_amd import _native
from adrates_amd.market.position.inflation_engine import inflation_inputs
from adrates_amd.market.position.scenarios import ScenarioGrid
from adrates_amd.market.position.yoy_book import tile_yoy_book
from adrates_amd.trades.compiler import TradeBatch, compile_yoy_coupons, compile_yoy_fixed_legs
from adrates_amd.trades.market_data import README_VALUE_DT, TENORS, random_yoy_book, yoy_model

FP64_INSTR_PER_S = 78.6e12 / 2
EXP_INSTR, SUM_INSTR = 19, 3
reps = max(3, int(sys.argv[1]) if len(sys.argv) > 1 else 7)
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                               "profiles", "yoy_scenario_bench.json")
n_big = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
n_small = int(sys.argv[4]) if len(sys.argv) > 4 else 200_000
distinct = int(sys.argv[5]) if len(sys.argv) > 5 else 400
S_LIST = (64, 256, 1024)
dev = torch.device("cuda", 0)
ctx = _native.default_context(0)
stream = torch.cuda.Stream(dev)


def disc_shocks(S):
    """Parallel shifts of up to +-150 bp combined with twists of up to +-50 bp between the short and the long end."""
    rng = np.random.default_rng(S)
    slope = np.linspace(-1.0, 1.0, len(TENORS))
    par, twist = rng.uniform(-1.5, 1.5, S), rng.uniform(-0.5, 0.5, S)
    return [{t: float(par[i] + twist[i] * slope[k]) for k, t in enumerate(TENORS)} for i in range(S)]


def breakeven_rows(b0, S):
    """Breakeven shifts of up to +-100 bp with twists of up to +-30 bp along the pillars."""
    rng = np.random.default_rng(S + 1)
    slope = np.linspace(-1.0, 1.0, b0.size)
    return b0[None, :] + (rng.uniform(-100, 100, S)[:, None] + rng.uniform(-30, 30, S)[:, None] * slope[None, :]) * 1e-4


def instr_per_scenario(fix_off, fix_tp, book):
    """fp64 vector instructions one scenario of the book costs, by the kernel's rules for what is shared."""
    tp, ts, te = book["tp"], book["ts"], book["te"]
    off = book["cpn_off"]
    first = np.zeros(tp.size, dtype=bool)
    first[off[:-1][off[:-1] < tp.size]] = True
    live, flat = tp > 0.0, ts == te
    tiled = np.concatenate(([False], (te[:-1] == ts[1:]) & live[:-1] & ~flat[:-1])) & ~first
    ratio = live & ~flat
    sums = int(np.sum(ratio)) + int(np.sum(ratio & ~tiled))                   # ln I(te), and ln I(ts) where not inherited
    nf, nc = np.diff(fix_off), np.diff(off)
    idx_in = np.arange(fix_tp.size) - np.repeat(fix_off[:-1], nf)
    has = idx_in < np.repeat(nc, nf)
    partner = np.where(has, np.repeat(off[:-1], nf) + idx_in, 0)
    shared = has & (tp[partner] == fix_tp) & live[partner] if tp.size else np.zeros(fix_tp.size, dtype=bool)
    fix_live = fix_tp > 0.0
    dates = int(np.sum(live)) + int(np.sum(fix_live & ~shared))               # discount factors evaluated
    instr = dates * (EXP_INSTR + SUM_INSTR) + int(np.sum(ratio)) * (EXP_INSTR + 1) + sums * SUM_INSTR + \
        int(np.sum(live)) * 6 + int(np.sum(fix_live)) * 2
    return instr, dates + int(np.sum(ratio))


def timed_pair(new, old, k):
    """Medians (ms) of k alternating repetitions of the two routes, each between its own events, after a warm-up of both."""
    with torch.cuda.stream(stream):
        new(); old()
        stream.synchronize()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(k)]
        for a, b, c, d in ev:
            a.record(stream); new(); b.record(stream)
            c.record(stream); old(); d.record(stream)
    torch.cuda.synchronize()
    t_new = [a.elapsed_time(b) for a, b, _, _ in ev]
    t_old = [c.elapsed_time(d) for _, _, c, d in ev]
    spread = lambda t: (max(t) - min(t)) / float(np.median(t))
    return float(np.median(t_new)), float(np.median(t_old)), spread(t_new), spread(t_old)


model = yoy_model()
infl = model.curves.GBP_RPI_INFLATION
im, T, b0 = inflation_inputs(infl)
P = T.size
swaps = random_yoy_book(README_VALUE_DT, distinct, seed=17)
base_cpn = compile_yoy_coupons(swaps, README_VALUE_DT)
base_fix = compile_yoy_fixed_legs(swaps, README_VALUE_DT)
base_notional = np.array([s._notional for s in swaps])
grid = ScenarioGrid(model, "GBP_OIS_SONIA", disc_shocks(max(S_LIST)), with_gamma=False, ctx=ctx)
arr = _native.curve_set_arrays(grid._set)
K, dm = arr["K"], arr["method"]
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
result = {"reps": reps, "fp64_instr_per_s_peak": FP64_INSTR_PER_S, "distinct_swaps": distinct, "cases": []}
for n in (n_big, n_small):
    r = -(-n // distinct)
    big = tile_yoy_book(base_cpn, r)
    m = int(big["cpn_off"][n])
    book = {k: (v[:n + 1] if k == "cpn_off" else v[:m]) for k, v in big.items()}
    counts = np.tile(np.diff(base_fix[0]), r)[:n]
    fix_off = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    mf = int(fix_off[-1])
    fix_tp, fix_pay = np.tile(base_fix[1], r)[:mf], np.tile(base_fix[2], r)[:mf]
    notional = np.tile(base_notional, r)[:n]
    total_notional = float(np.sum(notional))
    cpn_off, cpn = _native.yoy_pack(book)
    e = np.zeros(0)
    fixed_trades = _native.DeviceTrades(ctx, TradeBatch(fix_off, np.zeros(n + 1, dtype=np.int64), fix_tp, fix_pay, e, e.copy(),
                                                        e.copy(), e.copy(), notional, np.zeros(n), np.ones(n), np.ones(n)))
    t = {k: up(v) for k, v in dict(T=T, fix_off=fix_off, fix_tp=fix_tp, fix_pay=fix_pay, cpn_off=cpn_off, cpn=cpn).items()}
    instr, evals = instr_per_scenario(fix_off, fix_tp, book)
    for S in S_LIST:
        b_t = up(breakeven_rows(b0, S))
        ptrs = {k: v.data_ptr() for k, v in t.items()}
        ptrs.update(times=arr["times"], dfs=arr["dfs"], b=b_t.data_ptr())
        out = torch.zeros(S, dtype=torch.float64, device=dev)
        work = torch.empty(_native.yoy_scenario_pv_work(n, S), dtype=torch.float64, device=dev)
        agg = torch.zeros((S, 1 + P + P * P), dtype=torch.float64, device=dev)
        risk_work = torch.empty(_native.yoy_risk_work(n, P), dtype=torch.float64, device=dev)
        fix_book = torch.zeros(S, dtype=torch.float64, device=dev)
        fix_work = torch.empty(_native.scenario_pv_work(n, S), dtype=torch.float64, device=dev)
        new = lambda pv=0: _native.yoy_scenario_pv_dev(ctx, dm, K, S, im, P, S, S, n, mf, m, ptrs, out.data_ptr(), work.data_ptr(),
                                                       pv, stream.cuda_stream)

        def old():
            for s in range(S):
                _native.yoy_risk_dev(ctx, dm, K, im, P, n, m,
                                     dict(times=arr["times"], dfs=arr["dfs"] + 8 * K * s, T=ptrs["T"], b=ptrs["b"] + 8 * P * s,
                                          cpn_off=ptrs["cpn_off"], cpn=ptrs["cpn"]),
                                     _native.REQ_VALUE | _native.YOY_AGG, dict(agg=agg[s].data_ptr(), work=risk_work.data_ptr()),
                                     stream.cuda_stream)
            _native.scenario_pv_dev(ctx, dm, K, arr["times"], S, arr["dfs"], fixed_trades, fix_book.data_ptr(), fix_work.data_ptr(),
                                    0, stream.cuda_stream)

        ms_new, ms_old, sp_new, sp_old = timed_pair(new, old, reps)
        a_, b_ = out.cpu().numpy() / total_notional, (agg[:, 0] + fix_book).cpu().numpy() / total_notional
        err = float(np.max(np.abs(a_ - b_) / np.maximum(1.0, np.abs(b_))))
        rel = float(np.max(np.abs(a_ - b_) / np.abs(b_)))
        assert err <= 1e-10, f"the two routes' book PVs differ by {err:.3e} per unit notional"
        case = {"swaps": n, "scenarios": S, "knots": K, "inflation_pillars": P, "coupons_per_swap": m / n,
                "fixed_flows_per_swap": mf / n, "exp_per_swap": evals / n,
                "book_only": {"ms": ms_new, "spread": sp_new, "scenario_swaps_per_s": n * S / ms_new * 1e3, "fp64_instr": instr * S,
                              "share_of_fp64_vector_peak": instr * S / (ms_new * 1e-3) / FP64_INSTR_PER_S},
                "loop_of_yoy_risk_dev_plus_fixed_legs": {"ms": ms_old, "spread": sp_old, "scenario_swaps_per_s": n * S / ms_old * 1e3},
                "speedup": ms_old / ms_new, "faster_by_more_than_the_spread": bool(ms_old / ms_new - 1.0 > max(sp_new, sp_old)),
                "routes_agree_unit_notional": err, "routes_agree_relative": rel}
        if S * n * 8 < 8e9:
            pv = torch.empty((n, S), dtype=torch.float64, device=dev)
            ms_pt, _, sp_pt, _ = timed_pair(lambda: new(pv.data_ptr()), lambda: None, reps)
            case["per_swap_rows"] = {"ms": ms_pt, "spread": sp_pt, "scenario_swaps_per_s": n * S / ms_pt * 1e3,
                                     "output_GBps": n * S * 8 / ms_pt / 1e6}
            del pv
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
        del out, work, agg, risk_work, fix_book, fix_work, b_t
    fixed_trades.close()
grid.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps({"written": out_path, "cases": len(result["cases"])}))
