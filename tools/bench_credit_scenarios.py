"""Credit scenario revaluation benchmark: a book of bonds and FRNs (`random_bond_book`, `random_frn_book`; 400 distinct
trades compiled once by `compile_credit_book` and tiled to 200 000 and a million) at z-spreads / discount margins in 8
buckets, on the README GBP OIS curve (32 pillars, 264 knots) under S joint scenarios - par-rate shifts and twists
bootstrapped by the device builder, paired with spread shocks of up to +-300 bp per bucket - book PV only.

Three routes, timed in the same process and alternating, medians of warm repetitions between HIP events, inputs resident:
  new  ONE launch of adr_credit_scenario_pv_dev;
  (a)  what the library offered before it: per scenario one weighted upload of the batch rescaled by exp(-x tau) on the
       host and one adr_price_dev(VALUE, aggregate only) on that scenario's curve.  The S launches are timed on ONE
       resident rescaled batch ("pricing alone": the amounts do not change a launch's time); the rescale and the upload
       are timed on the host clock (median of 3) and reported per scenario, and "with uploads" adds S of them;
  (b)  adr_scenario_pv_dev on the same batch: the same work without spreads, so new / (b) is the price of the spread.
The new route's book PV of one scenario must agree with (a)'s on that scenario's rescaled batch to 1e-10 per unit
notional (asserted).

The share of the fp64 vector peak uses an instruction count computed from the book by the kernel's own sharing rules:
per scenario one exp per discount factor evaluated (a float coupon: D(te), the spread-discounted D(tp), and D(ts) where
it is not the previous coupon's D(te); a fixed flow: one, unless it shares the coupon's), the fp64 instructions each
expands to on gfx950 counted as tools/bench_scenarios.py counts them (exp: 19), 3 per weighted sum of two knots, 2 for
x tau and its subtraction, a division (10) and 5 per coupon, 2 per fixed flow; against 78.6 TFLOP/s = 39.3 T fp64
instructions per second.
usage: bench_credit_scenarios.py [reps] [out.json] [n_big] [n_small] [distinct]"""
import dataclasses, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from adrates_amd import _native
from adrates_amd.market.position.scenarios import ScenarioGrid, compile_credit_book
from adrates_amd.trades.compiler import TradeBatch
from adrates_amd.trades.market_data import README_VALUE_DT, TENORS, gbp_model, random_bond_book, random_frn_book
from adrates_amd.utils import CurveTypes

FP64_INSTR_PER_S = 78.6e12 / 2
EXP_INSTR, SUM_INSTR, DIV_INSTR = 19, 3, 10
reps = max(3, int(sys.argv[1]) if len(sys.argv) > 1 else 7)
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                               "profiles", "credit_scenario_bench.json")
n_big = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
n_small = int(sys.argv[4]) if len(sys.argv) > 4 else 200_000
distinct = int(sys.argv[5]) if len(sys.argv) > 5 else 400
S_LIST = (64, 256, 1024)
G = 8
dev = torch.device("cuda", 0)
ctx = _native.default_context(0)
stream = torch.cuda.Stream(dev)


def disc_shocks(S):
    """Parallel shifts of up to +-150 bp combined with twists of up to +-50 bp between the short and the long end."""
    rng = np.random.default_rng(S)
    slope = np.linspace(-1.0, 1.0, len(TENORS))
    par, twist = rng.uniform(-1.5, 1.5, S), rng.uniform(-0.5, 0.5, S)
    return [{t: float(par[i] + twist[i] * slope[k]) for k, t in enumerate(TENORS)} for i in range(S)]


def tile(book, n):
    """The compiled credit book repeated to ``n`` trades: (batch, z, bucket, fix_tau, flt_tau)."""
    b = book.batch
    r = -(-n // b.n_trades)
    def flows(off, *arrays):
        counts = np.tile(np.diff(off), r)[:n]
        new_off = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
        return new_off, [np.tile(a, r)[:int(new_off[-1])] for a in arrays]
    fix_off, (fix_tp, fix_pay, fix_tau) = flows(b.fix_off, b.fix_tp, b.fix_pay, book.fix_tau)
    flt_off, (flt_tp, flt_ts, flt_te, flt_al, flt_tau) = flows(b.flt_off, b.flt_tp, b.flt_ts, b.flt_te, b.flt_alpha, book.flt_tau)
    per = lambda a: np.tile(a, r)[:n]
    batch = TradeBatch(fix_off, flt_off, fix_tp, fix_pay, flt_tp, flt_ts, flt_te, flt_al, per(b.notional), per(b.spread),
                       per(b.fix_sign), per(b.flt_sign))
    return batch, per(book.z), per(book.bucket), fix_tau, flt_tau


def rescaled(batch, x, fix_tau, flt_tau):
    """One scenario's batch with exp(-x tau) folded into the amounts: what route (a) uploads per scenario."""
    xf, xl = np.repeat(x, np.diff(batch.fix_off)), np.repeat(x, np.diff(batch.flt_off))
    return dataclasses.replace(batch, fix_pay=batch.fix_pay * np.exp(-xf * fix_tau), flt_weight=np.exp(-xl * flt_tau))


def instr_per_scenario(batch):
    """fp64 vector instructions one scenario of the book costs (LINEAR_ZERO_RATES), by the kernel's sharing rules."""
    tp, ts, te, al = batch.flt_tp, batch.flt_ts, batch.flt_te, batch.flt_alpha
    first = np.zeros(tp.size, dtype=bool)
    first[batch.flt_off[:-1][batch.flt_off[:-1] < tp.size]] = True
    live = tp >= 0.0
    accr = live & (al > 0.0)
    inherited = np.concatenate(([False], (te[:-1] == ts[1:]) & accr[:-1])) & ~first
    evals = 2 * int(np.sum(accr)) + int(np.sum(accr & ~inherited)) + int(np.sum(live & ~accr))
    fix_live = batch.fix_tp > 0.0
    evals += int(np.sum(fix_live))                       # spread times differ from the coupons': no fixed flow shares
    folds = int(np.sum(live)) + int(np.sum(fix_live))
    return evals * (EXP_INSTR + SUM_INSTR) + folds * 2 + int(np.sum(accr)) * DIV_INSTR + int(np.sum(live)) * 5 + \
        int(np.sum(fix_live)) * 2, evals


def timed(routes, k):
    """Medians (ms) and spreads of k alternating repetitions of the routes, each between its own events, after a warm-up."""
    with torch.cuda.stream(stream):
        for r in routes:
            r()
        stream.synchronize()
        ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in routes] for _ in range(k)]
        for row in ev:
            for (a, b), r in zip(row, routes):
                a.record(stream); r(); b.record(stream)
    torch.cuda.synchronize()
    t = [[row[i][0].elapsed_time(row[i][1]) for row in ev] for i in range(len(routes))]
    return [(float(np.median(x)), (max(x) - min(x)) / float(np.median(x))) for x in t]


model = gbp_model(README_VALUE_DT)
bonds, _ = random_bond_book(README_VALUE_DT, distinct // 2, seed=17)
frns, _ = random_frn_book(README_VALUE_DT, distinct - distinct // 2, seed=18)
rng = np.random.default_rng(19)
spreads = np.concatenate([rng.uniform(-50e-4, 800e-4, len(bonds)), rng.uniform(-50e-4, 300e-4, len(frns))])
labels = [f"bucket {i}" for i in rng.integers(0, G, distinct)]
base = compile_credit_book(bonds + frns, README_VALUE_DT, CurveTypes.GBP_OIS_SONIA, spreads, labels)
assert len(base.labels) == G
grid = ScenarioGrid(model, "GBP_OIS_SONIA", disc_shocks(max(S_LIST)), with_gamma=False, ctx=ctx)
arr = _native.curve_set_arrays(grid._set)
K, P, method = arr["K"], grid._plan.n_pillars, arr["method"]
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
result = {"reps": reps, "fp64_instr_per_s_peak": FP64_INSTR_PER_S, "distinct_trades": distinct, "buckets": G, "cases": []}
for n in (n_big, n_small):
    batch, z, bucket, fix_tau, flt_tau = tile(base, n)
    n_fix, n_flt = int(batch.fix_off[-1]), int(batch.flt_off[-1])
    total_notional = float(np.sum(np.abs(batch.notional)))
    trades = _native.DeviceTrades(ctx, batch)
    t = dict(z=up(z), bucket=up(bucket.astype(np.int32)), fix_tau=up(fix_tau), flt_tau=up(flt_tau))
    instr, evals = instr_per_scenario(batch)
    dz_all = np.random.default_rng(n).uniform(-300e-4, 300e-4, (max(S_LIST), G))
    check_s = 1
    x = z + dz_all[check_s][bucket]
    host_ms, upload_ms = [], []
    scaled_dev = None
    for _ in range(3):                                   # route (a)'s per-scenario host work, on the host clock
        if scaled_dev is not None:
            scaled_dev.close()
        t0 = time.perf_counter()
        scaled = rescaled(batch, x, fix_tau, flt_tau)
        t1 = time.perf_counter()
        scaled_dev = _native.DeviceTrades(ctx, scaled)
        _native.load().adr_sync(ctx._h)
        host_ms.append((t1 - t0) * 1e3)
        upload_ms.append((time.perf_counter() - t1) * 1e3)
    per_scenario_ms = float(np.median(host_ms)) + float(np.median(upload_ms))
    for S in S_LIST:
        dz_t = up(dz_all[:S])
        ptrs = {k: v.data_ptr() for k, v in t.items()}
        ptrs.update(times=arr["times"], dfs=arr["dfs"], dz=dz_t.data_ptr())
        book = torch.zeros(S, dtype=torch.float64, device=dev)
        work = torch.empty(_native.credit_scenario_pv_work(n, S), dtype=torch.float64, device=dev)
        plain = torch.zeros(S, dtype=torch.float64, device=dev)
        plain_work = torch.empty(_native.scenario_pv_work(n, S), dtype=torch.float64, device=dev)
        agg = torch.zeros((S, 1 + P + P * P), dtype=torch.float64, device=dev)
        curves = [grid.device_curve(i) for i in range(S)]
        new = lambda: _native.credit_scenario_pv_dev(ctx, method, K, S, G, S, S, trades, n_fix, n_flt, ptrs, book.data_ptr(),
                                                     work.data_ptr(), 0, stream.cuda_stream)

        def loop():
            for i in range(S):
                _native.price_dev(ctx, curves[i], scaled_dev, _native.REQ_VALUE, 0, 0, 0, agg[i].data_ptr(), stream.cuda_stream)

        no_spread = lambda: _native.scenario_pv_dev(ctx, method, K, arr["times"], S, arr["dfs"], trades, plain.data_ptr(),
                                                    plain_work.data_ptr(), 0, stream.cuda_stream)
        (ms_new, sp_new), (ms_a, sp_a), (ms_b, sp_b) = timed([new, loop, no_spread], reps)
        a_, b_ = float(book[check_s]) / total_notional, float(agg[check_s, 0]) / total_notional
        err = abs(a_ - b_) / max(1.0, abs(b_))
        assert err <= 1e-10, f"the routes' book PVs of scenario {check_s} differ by {err:.3e} per unit notional"
        case = {"trades": n, "scenarios": S, "knots": K, "buckets": G, "fixed_flows_per_trade": n_fix / n,
                "float_coupons_per_trade": n_flt / n, "exp_per_trade": evals / n,
                "credit_scenario_pv_dev": {"ms": ms_new, "spread": sp_new, "scenario_trades_per_s": n * S / ms_new * 1e3,
                                           "fp64_instr": instr * S,
                                           "share_of_fp64_vector_peak": instr * S / (ms_new * 1e-3) / FP64_INSTR_PER_S},
                "a_loop_of_adr_price_dev_pricing_alone": {"ms": ms_a, "spread": sp_a},
                "a_per_scenario_rescale_and_upload_ms": per_scenario_ms,
                "a_with_uploads_ms": ms_a + S * per_scenario_ms,
                "b_scenario_pv_dev_no_spreads": {"ms": ms_b, "spread": sp_b},
                "speedup_over_a_pricing_alone": ms_a / ms_new, "speedup_over_a_with_uploads": (ms_a + S * per_scenario_ms) / ms_new,
                "beats_a_pricing_alone_by_more_than_the_spread": bool(ms_a / ms_new - 1.0 > max(sp_new, sp_a)),
                "price_of_the_spread_new_over_b": ms_new / ms_b, "routes_agree_unit_notional": err}
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
        del book, work, plain, plain_work, agg, dz_t
    scaled_dev.close()
    trades.close()
grid.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps({"written": out_path, "cases": len(result["cases"])}))
