"""Scenario revaluation benchmark: the benchmark book (`synthesize`, off-grid OIS; a million and 100 000 trades) on the
README GBP curve under S par-rate scenarios (parallel shifts and twists, bootstrapped by the device builder), book PV
only and with per-trade rows, LINEAR_ZERO_RATES and LINEAR_FWD_RATES.

Two routes for the same request, timed in the same process and alternating: ONE launch of adr_scenario_pv_dev on the
set's discount factors, and the per-scenario loop it replaces - adr_price_dev(VALUE, aggregate only) once per curve of the
set on one stream, which is `ScenarioGrid.price(aggregate=True)` without its host copies.  Times are medians of warm
repetitions between HIP events, inputs resident.  The two routes' book PVs of the timed run are compared.

The share of the fp64 vector peak uses an instruction count computed from the batch: per scenario and trade the
exponentials (one per distinct date, as the kernel's flags decide) and divisions (one per accruing coupon), with the
fp64 instructions each expands to on gfx950 counted from the ISA (exp: 19 - 13 fma, mul, rndne, ldexp, cvt, 2 cmp;
division: 11; plus 2 per date for the weighted sum and 5 per coupon / 2 per fixed flow for the leg arithmetic), against
78.6 TFLOP/s = 39.3 T fp64 instructions per second (an fma counts two flops).  Trade bytes are read once per scenario
group of 64 and are small beside that: the kernel is bound by fp64 issue, not by memory.
usage: bench_scenarios.py [reps] [out.json] [n_big] [n_small]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from adrates_amd import _native
from adrates_amd.market.position.scenarios import ScenarioGrid
from adrates_amd.trades import synthetic
from adrates_amd.trades.market_data import README_VALUE_DT, gbp_model
from adrates_amd.utils import InterpTypes

FP64_INSTR_PER_S = 78.6e12 / 2
EXP_INSTR, DIV_INSTR = 19, 11
reps = max(3, int(sys.argv[1]) if len(sys.argv) > 1 else 7)
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                               "profiles", "scenario_pv_bench.json")
n_big = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
n_small = int(sys.argv[4]) if len(sys.argv) > 4 else 100_000
S_LIST = (64, 256, 1024)
dev = torch.device("cuda", 0)
ctx = _native.default_context(0)
stream = torch.cuda.Stream(dev)


def shocks(S):
    """Parallel shifts of up to +-150 bp combined with twists of up to +-50 bp between the short and the long end."""
    rng = np.random.default_rng(S)
    from adrates_amd.trades.market_data import TENORS
    slope = np.linspace(-1.0, 1.0, len(TENORS))
    par, twist = rng.uniform(-1.5, 1.5, S), rng.uniform(-0.5, 0.5, S)
    return [{t: float(par[i] + twist[i] * slope[k]) for k, t in enumerate(TENORS)} for i in range(S)]


def instr_per_scenario(batch, log_scheme):
    """fp64 vector instructions one scenario of the book costs, by the kernel's rules for which dates share a value."""
    tp, ts, te, al = batch.flt_tp, batch.flt_ts, batch.flt_te, batch.flt_alpha
    first = np.zeros(tp.size, dtype=bool)
    first[batch.flt_off[:-1][batch.flt_off[:-1] < tp.size]] = True
    live, accr = tp >= 0.0, al > 0.0
    prev_ok = np.concatenate(([False], (te[:-1] == ts[1:]) & live[:-1] & accr[:-1])) & ~first
    dates = np.sum(live & accr & ~prev_ok) + np.sum(live & accr) + np.sum(live & accr & (tp != te)) + np.sum(live & ~accr)
    # a fixed flow shares the float coupon's payment date when both have the same index and time
    nf, nl = np.diff(batch.fix_off), np.diff(batch.flt_off)
    idx_in = np.arange(batch.fix_tp.size) - np.repeat(batch.fix_off[:-1], nf)
    has = idx_in < np.repeat(nl, nf)
    partner = np.where(has, np.repeat(batch.flt_off[:-1], nf) + idx_in, 0)
    shared = has & (tp[partner] == batch.fix_tp) & live[partner] if tp.size else np.zeros(batch.fix_tp.size, dtype=bool)
    fix_live = batch.fix_tp > 0.0
    dates += np.sum(fix_live & ~shared)
    coupons, flows = int(np.sum(live)), int(np.sum(fix_live))
    per_date = (EXP_INSTR if log_scheme else 0) + 2
    return int(dates) * per_date + int(np.sum(live & accr)) * DIV_INSTR + coupons * 5 + flows * 2, int(dates)


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


result = {"reps": reps, "fp64_instr_per_s_peak": FP64_INSTR_PER_S, "cases": []}
for interp in (InterpTypes.LINEAR_ZERO_RATES, InterpTypes.LINEAR_FWD_RATES):
    model = gbp_model(README_VALUE_DT, interp)
    grid = ScenarioGrid(model, "GBP_OIS_SONIA", shocks(max(S_LIST)), with_gamma=False, ctx=ctx)
    arr = _native.curve_set_arrays(grid._set)
    K, P = arr["K"], grid._plan.n_pillars
    for n in (n_big, n_small):
        batch = synthetic.synthesize(README_VALUE_DT, n)
        trades = _native.DeviceTrades(ctx, batch)
        instr, dates = instr_per_scenario(batch, interp != InterpTypes.LINEAR_FWD_RATES)
        total_notional = float(np.sum(np.abs(batch.notional)))
        for S in S_LIST:
            book = torch.zeros(S, dtype=torch.float64, device=dev)
            work = torch.empty(_native.scenario_pv_work(n, S), dtype=torch.float64, device=dev)
            agg = torch.zeros((S, 1 + P + P * P), dtype=torch.float64, device=dev)
            curves = [grid.device_curve(i) for i in range(S)]
            new = lambda pv=0: _native.scenario_pv_dev(ctx, arr["method"], K, arr["times"], S, arr["dfs"], trades,
                                                       book.data_ptr(), work.data_ptr(), pv, stream.cuda_stream)

            def old():
                for i in range(S):
                    _native.price_dev(ctx, curves[i], trades, _native.REQ_VALUE, 0, 0, 0, agg[i].data_ptr(), stream.cuda_stream)

            ms_new, ms_old, sp_new, sp_old = timed_pair(new, old, reps)
            a, b = book.cpu().numpy() / total_notional, agg[:, 0].cpu().numpy() / total_notional
            err = float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))
            rel = float(np.max(np.abs(a - b) / np.abs(b)))                    # book PVs are far below the total notional
            case = {"scheme": interp.name, "trades": n, "scenarios": S, "knots": K, "dates_per_trade": dates / n,
                    "book_only": {"ms": ms_new, "spread": sp_new, "scenario_trades_per_s": n * S / ms_new * 1e3,
                                  "fp64_instr": instr * S, "share_of_fp64_vector_peak": instr * S / (ms_new * 1e-3) / FP64_INSTR_PER_S,
                                  "bound": "fp64 vector issue"},
                    "loop_of_adr_price_dev": {"ms": ms_old, "spread": sp_old, "scenario_trades_per_s": n * S / ms_old * 1e3},
                    "speedup": ms_old / ms_new, "routes_agree_unit_notional": err, "routes_agree_relative": rel}
            if S * n * 8 < 8e9:
                pv = torch.empty((n, S), dtype=torch.float64, device=dev)
                with torch.cuda.stream(stream):
                    ms_pt, _, sp_pt, _ = timed_pair(lambda: new(pv.data_ptr()), lambda: None, reps)
                case["per_trade_rows"] = {"ms": ms_pt, "spread": sp_pt, "scenario_trades_per_s": n * S / ms_pt * 1e3,
                                          "output_GBps": n * S * 8 / ms_pt / 1e6}
                del pv
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
            del book, work, agg
        trades.close()
    grid.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps({"written": out_path, "cases": len(result["cases"])}))
