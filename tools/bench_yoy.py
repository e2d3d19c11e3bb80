"""YoY inflation swap benchmark.  The inflation side, the adr_yoy_risk kernel (projected amounts, inflation-leg PV,
inflation-curve delta and gamma), on about 200 000 YoY swaps - annual coupons, 5-30Y, a 20-pillar inflation curve, the
32-pillar GBP OIS curve's knot grid - per swap with and without gammas and for the book only; then a million swaps for
the book only.  The discount side, the same 200 000 swaps' fixed flows through the pricing route, separately.  A few
hundred distinct swaps are compiled once and their arrays tiled.  Times are medians of warm launches between HIP
events, inputs already on the device.
usage: bench_yoy.py [n_swaps] [n_big] [distinct] [reps]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from adrates_amd import _native
from adrates_amd.market.curves.curve_tables import build_engine_curve
from adrates_amd.market.position.inflation_engine import inflation_inputs
from adrates_amd.market.position.yoy_book import tile_yoy_book
from adrates_amd.market.position.engine import Engine
from adrates_amd.trades.compiler import TradeBatch, compile_yoy_coupons, compile_yoy_swaps
from adrates_amd.trades.market_data import README_VALUE_DT, random_yoy_book, yoy_model

HBM_BYTES_PER_S = 8e12

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
n_big = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
distinct = int(sys.argv[3]) if len(sys.argv) > 3 else 400
reps = max(10, int(sys.argv[4]) if len(sys.argv) > 4 else 20)
dev = torch.device("cuda", 0)
ctx = _native.default_context(0)
model = yoy_model()
disc_c, infl_c = model.curves.GBP_OIS_SONIA, model.curves.GBP_RPI_INFLATION
grid = build_engine_curve(disc_c.swap_rates, disc_c.swap_times, disc_c.year_fracs)
im, T, b = inflation_inputs(infl_c)
P = T.size
base = compile_yoy_coupons(random_yoy_book(README_VALUE_DT, distinct, seed=17), README_VALUE_DT)
s = torch.cuda.Stream(dev)
ALL3 = _native.REQ_VALUE | _native.REQ_DELTA | _native.REQ_GAMMA


def book_of(count):
    big = tile_yoy_book(base, -(-count // distinct))
    m = int(big["cpn_off"][count])
    return {k: (v[:count + 1] if k == "cpn_off" else v[:m]) for k, v in big.items()}


def timed(launch, k):
    """Median ms of k launches on stream s, each between its own pair of events, after 3 warm-up launches."""
    with torch.cuda.stream(s):
        for _ in range(3):
            launch()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(k)]
        for a, e in ev:
            a.record(s)
            launch()
            e.record(s)
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(e) for a, e in ev]))


def run(count, modes):
    book = book_of(count)
    off, cpn = _native.yoy_pack(book)
    m = cpn.shape[1]
    ins = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
           dict(times=grid.times, dfs=grid.dfs, T=T, b=b, cpn_off=off, cpn=cpn).items()}
    ptrs = {k: v.data_ptr() for k, v in ins.items()}
    res = {"swaps": count, "coupons": m, "coupons_per_swap": m / count, "inflation_pillars": P, "discount_knots": grid.times.size}
    for name, mask in modes:
        per, agg = bool(mask & _native.YOY_PER_SWAP), bool(mask & _native.YOY_AGG)
        gam = bool(mask & _native.REQ_GAMMA)
        o = {"amount": torch.empty(m, dtype=torch.float64, device=dev)}
        if per:
            o.update(pv=torch.empty(count, dtype=torch.float64, device=dev),
                     delta=torch.empty((count, P), dtype=torch.float64, device=dev))
            if gam:
                o["gamma"] = torch.empty((count, P, P), dtype=torch.float64, device=dev)
        if agg:
            o.update(agg=torch.empty(1 + P + P * P, dtype=torch.float64, device=dev),
                     work=torch.empty(_native.yoy_risk_work(count, P), dtype=torch.float64, device=dev))
        optr = {k: v.data_ptr() for k, v in o.items()}
        torch.cuda.synchronize()
        ms = timed(lambda: _native.yoy_risk_dev(ctx, LZ, grid.times.size, im, P, count, m, ptrs, mask, optr,
                                                s.cuda_stream), reps)
        # bytes the kernel must move: 5 doubles per coupon and the offsets in, the amounts and the requested rows out
        rows = (1 + P + (P * P if gam else 0)) * count if per else 0
        chunks = -(-count // _native.YOY_CHUNK)
        scratch = 2 * chunks * (1 + P + P * P) if agg else 0
        moved = 8 * (5 * m + (count + 1) + m + rows + scratch)
        res[name] = {"ms": ms, "swaps_per_s": count / ms * 1e3, "bytes": moved, "GBps": moved / ms / 1e6,
                     "fraction_of_8TBps": moved / (ms * 1e-3) / HBM_BYTES_PER_S}
        del o
    return res


LZ = disc_c._interp_type.value
PER = _native.YOY_PER_SWAP
# the inflation side (adr_yoy_risk) alone; the discount side is timed below
result = {"book": run(n, [("infl_pv+delta, per-swap", _native.REQ_VALUE | _native.REQ_DELTA | PER),
                          ("infl_pv+delta+gamma, per-swap", ALL3 | PER),
                          ("infl_pv+delta+gamma, aggregate", ALL3 | _native.YOY_AGG)])}
result["big_book"] = run(n_big, [("infl_pv+delta+gamma, aggregate", ALL3 | _native.YOY_AGG)])

# the discount side of the same 200k book through the pricing route: fixed flows carrying the projected amounts
swaps = random_yoy_book(README_VALUE_DT, distinct, seed=17)
amounts = _native.yoy_risk_host((LZ, grid.times, grid.dfs), (im, T, b), base, per_swap=False)["amount"]
tb = compile_yoy_swaps(swaps, README_VALUE_DT, amounts)
copies = -(-n // distinct)
fl = np.tile(tb.fix_off[1:] - tb.fix_off[:-1], copies)[:n]
fo = np.concatenate(([0], np.cumsum(fl))).astype(np.int64)
kf = int(fo[-1])
tile = lambda a, k: np.tile(a, copies)[:k]
empty = np.zeros(0)
big_tb = TradeBatch(fo, np.zeros(n + 1, dtype=np.int64), tile(tb.fix_tp, kf), tile(tb.fix_pay, kf), empty, empty, empty,
                    empty, tile(tb.notional, n), np.zeros(n), np.ones(n), np.ones(n))
cur = Engine(model)._device_curve(disc_c)
dtr = _native.DeviceTrades(ctx, big_tb)
Pd = cur["dev"].n_pillars
agg = torch.empty(1 + Pd + Pd * Pd, dtype=torch.float64, device=dev)
pv = torch.empty(n, dtype=torch.float64, device=dev)
delta = torch.empty((n, Pd), dtype=torch.float64, device=dev)
gamma = torch.empty((n, Pd, Pd), dtype=torch.float64, device=dev)
result["discount_side"] = {
    "swaps": n, "flows": kf,
    "pv+delta, per-swap_ms": timed(lambda: _native.price_dev(ctx, cur["dev"], dtr, 3, pv.data_ptr(), delta.data_ptr(), 0, 0,
                                                             s.cuda_stream), reps),
    "pv+delta+gamma, per-swap_ms": timed(lambda: _native.price_dev(ctx, cur["dev"], dtr, 7, pv.data_ptr(), delta.data_ptr(),
                                                                   gamma.data_ptr(), 0, s.cuda_stream), reps),
    "pv+delta+gamma, aggregate_ms": timed(lambda: _native.price_dev(ctx, cur["dev"], dtr, 7, 0, 0, 0, agg.data_ptr(),
                                                                    s.cuda_stream), reps)}
dtr.close()
print(json.dumps(result))
