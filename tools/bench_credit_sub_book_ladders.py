"""Credit sub-book Greeks benchmark: a million bonds and lag-free FRNs (tiled from a few hundred) at their spreads on the
README GBP curve, LINEAR_ZERO_RATES, G = 8 buckets, cut into B = 1, 100 and 1 000 equal desks and 1 000 geometric ones;
PV + delta and PV + delta + gamma.

Timed, inputs resident, medians of warm repetitions between HIP events, the routes of a comparison alternating in one
process (the method of tools/bench_sub_book_ladders.py):
  * the ONE chain, adr_credit_subbook_ladders_dev (knot sums with the fourth table, cell sum, desk sum, two projections);
  * (a) adr_subbook_ladders_dev on the same batch and desks: the riskless ladders - the price of the spread and of the
    fourth table is the ratio;
  * (b) the only route there was for at-spread desk ladders: one batch per desk with exp(-z tau) folded into its amounts,
    uploaded beforehand, and one aggregate-only adr_price_dev per desk, launches alone (B = 100 and 1 000);
  * (c) for CS01 and spread gamma only: adr_credit_scenario_subbook_pv_dev with 2 G + 1 spread scenarios.
Also, for context, adr_ladder_pnl_dev on the augmented ladders (Q = P + G) under S = 1 024 joint shocks.
usage: bench_credit_sub_book_ladders.py [reps] [out.json] [n]"""
import dataclasses, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from adrates_amd import _native
from adrates_amd.market.curves.curve_tables import build_engine_curve
from adrates_amd.market.position.scenarios import _concat_batches, _permute_batch
from adrates_amd.trades.compiler import compile_bonds, compile_frns
from adrates_amd.trades.market_data import README_VALUE_DT, gbp_model, random_bond_book, random_frn_book
from adrates_amd.utils import InterpTypes

reps = max(3, int(sys.argv[1]) if len(sys.argv) > 1 else 7)
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "credit_sub_book_ladders_bench.json")
n = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
G, S_PNL = 8, 1024
dev = torch.device("cuda", 0)
ctx = _native.default_context(0)
stream = torch.cuda.Stream(dev)
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def sizes_of(B, dist):
    if dist == "equal":
        sizes = np.full(B, n // B, dtype=np.int64)
    else:                                           # geometric: the first desk about 1 / (1 - r) times the mean's share
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
        out.append({"ms": float(np.median(t)), "spread": (max(t) - min(t)) / float(np.median(t))})
    return out


curve = gbp_model(README_VALUE_DT, InterpTypes.LINEAR_ZERO_RATES).curves.GBP_OIS_SONIA
method = curve._interp_type.value
host = build_engine_curve(curve.swap_rates, curve.swap_times, curve.year_fracs)
dc = _native.DeviceCurve(ctx, method, host.times, host.dfs, host.jac, host.hess)
P = dc.n_pillars
Q = P + G

# the book: 200 bonds and the lag-free ones of 400 FRNs, tiled; tau = t for every flow
frns = compile_frns(random_frn_book(README_VALUE_DT, 400, seed=6)[0], README_VALUE_DT)[0]
frns = _permute_batch(frns, np.nonzero(~_native.ratio_flags_host(frns))[0])[0]
seed_book = _concat_batches([compile_bonds(random_bond_book(README_VALUE_DT, 200, seed=5)[0], README_VALUE_DT), frns])
m = seed_book.n_trades
rng = np.random.default_rng(1)
pick = rng.integers(0, m, n)
z_all = rng.uniform(-50e-4, 800e-4, n)
bucket_all = rng.integers(-1, G, n).astype(np.int32)
result = {"reps": reps, "trades": n, "seed_trades": m, "pillars": P, "buckets": G, "knots": int(host.times.size),
          "scheme": "LINEAR_ZERO_RATES", "cases": []}
REQUESTS = (("pv_delta", 3), ("pv_delta_gamma", 7))

for B, dist in ((1, "equal"), (100, "equal"), (1000, "equal"), (1000, "geometric")):
    sizes = sizes_of(B, dist)
    sub_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    desk = np.repeat(np.arange(B, dtype=np.int64), sizes)
    order = np.lexsort((bucket_all, desk))                  # the (desk, bucket) order the entry asks for
    batch, fi, li = _permute_batch(seed_book, pick[order])
    z, bucket = z_all[order], bucket_all[order]
    fix_tau, flt_tau = np.ascontiguousarray(batch.fix_tp), np.ascontiguousarray(batch.flt_tp)
    trades = _native.DeviceTrades(ctx, batch)
    cell_off, desk_cell_off, cell_bucket = _native.credit_subbook_cells(bucket, sub_off)
    C = int(cell_bucket.size)
    bufs = {"z": up(z), "bucket": up(bucket), "fix_tau": up(fix_tau), "flt_tau": up(flt_tau),
            "cell_plan": up(_native.scenario_subbook_plan(n, cell_off)), "desk_cell_off": up(desk_cell_off),
            "cell_bucket": up(cell_bucket), "plan": up(_native.scenario_subbook_plan(n, sub_off)), "times": up(host.times),
            "dfs": up(host.dfs)}
    h = 1e-4
    dz = np.zeros((2 * G + 1, G))
    for g in range(G):
        dz[1 + 2 * g, g], dz[2 + 2 * g, g] = h, -h
    bufs["dz"] = up(dz)
    ptrs = {k: v.data_ptr() for k, v in bufs.items()}
    out = torch.zeros((B, 1 + Q + Q * Q), dtype=torch.float64, device=dev)
    work = torch.empty(_native.credit_subbook_ladders_work(dc, n, B, C)[0], dtype=torch.float64, device=dev)
    plain = torch.zeros((B, 1 + P + P * P), dtype=torch.float64, device=dev)
    plain_work = torch.empty(_native.subbook_ladders_work(dc, n, B)[0], dtype=torch.float64, device=dev)
    S_c = 2 * G + 1
    sub_pv = torch.zeros((B, S_c), dtype=torch.float64, device=dev)
    scen_work = torch.empty(_native.scenario_subbook_work(n, B, S_c), dtype=torch.float64, device=dev)
    case = {"sub_books": B, "sizes": dist, "largest": int(sizes.max()), "smallest": int(sizes.min()), "cells": C,
            "chunks": int(bufs["cell_plan"][C].item())}
    pieces = []
    if B > 1:                                               # route (b): exp(-z tau) folded into each desk's amounts
        ff = np.exp(-np.repeat(z, np.diff(batch.fix_off)) * fix_tau)
        fl = np.exp(-np.repeat(z, np.diff(batch.flt_off)) * flt_tau)
        w = np.ones(flt_tau.size) if batch.flt_weight is None else batch.flt_weight
        scaled = dataclasses.replace(batch, fix_pay=batch.fix_pay * ff, flt_weight=w * fl)
        pieces = [_native.DeviceTrades(ctx, _permute_batch(scaled, np.arange(lo, hi, dtype=np.int64))[0])
                  for lo, hi in zip(sub_off[:-1], sub_off[1:])]
    rows = torch.zeros((max(1, len(pieces)), 1 + P + P * P), dtype=torch.float64, device=dev)
    for name, mask in REQUESTS:
        one = lambda: _native.credit_subbook_ladders_dev(ctx, dc, trades, fix_tau.size, flt_tau.size, G, B, C, ptrs, mask,
                                                         out.data_ptr(), work.data_ptr(), stream.cuda_stream)
        riskless = lambda: _native.subbook_ladders_dev(ctx, dc, trades, B, ptrs["plan"], mask, plain.data_ptr(),
                                                       plain_work.data_ptr(), stream.cuda_stream)
        routes, names = [one, riskless], ["one_chain", "riskless_sub_book_ladders"]
        if pieces:
            def loop():
                for b, piece in enumerate(pieces):
                    _native.price_dev(ctx, dc, piece, mask, agg_ptr=rows[b].data_ptr(), stream=stream.cuda_stream)
            routes.append(loop)
            names.append("loop_of_aggregate_only_on_rescaled_batches")
        if mask == 7:
            routes.append(lambda: _native.credit_scenario_subbook_pv_dev(ctx, method, host.times.size, 1, G, S_c, S_c, trades,
                                                                         fix_tau.size, flt_tau.size, B, ptrs, sub_pv.data_ptr(),
                                                                         scen_work.data_ptr(), stream=stream.cuda_stream))
            names.append("spread_bump_and_revalue")
        t = timed(routes, reps)
        entry = dict(zip(names, t))
        entry["ratio_to_riskless"] = t[0]["ms"] / t[1]["ms"]
        if pieces:
            entry["speedup_over_loop"] = t[2]["ms"] / t[0]["ms"]
            entry["margin"] = max(t[0]["spread"], t[2]["spread"])
            entry["faster_by_more_than_the_spread"] = bool(t[2]["ms"] / t[0]["ms"] - 1.0 > entry["margin"])
            got = torch.cat([out[:, :1 + P], out[:, 1 + Q:].reshape(B, Q, Q)[:, :P, :P].reshape(B, P * P)], dim=1)
            scale = rows.abs().amax(0).clamp_min(1e-300)
            entry["worst_difference_over_largest_row_entry"] = float(((got - rows).abs().amax(0) / scale).max().item())
        if mask == 7:
            entry["speedup_over_bump_and_revalue"] = t[-1]["ms"] / t[0]["ms"]
            fd = (sub_pv[:, 1::2] - sub_pv[:, 2::2]) / 2.0
            cs01 = out[:, 1 + P:1 + Q]
            entry["cs01_vs_central_difference"] = float(((fd - cs01).abs().max() / cs01.abs().max()).item())
        case[name] = entry
    if B == 1000 and dist == "equal":                       # context: the P&L step on these ladders
        shocks = up(np.random.default_rng(2).normal(0.0, 5.0, (S_PNL, Q)))
        pnl = torch.empty((B, S_PNL), dtype=torch.float64, device=dev)
        t = timed([lambda: _native.ladder_pnl_dev(ctx, B, Q, out.data_ptr(), S_PNL, shocks.data_ptr(), pnl.data_ptr(),
                                                  stream=stream.cuda_stream)], reps)
        case["ladder_pnl_on_augmented_rows"] = dict(t[0], columns=Q, scenarios=S_PNL)
    for piece in pieces:
        piece.close()
    trades.close()
    result["cases"].append(case)
    print(json.dumps(case), flush=True)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps({"written": out_path}))
