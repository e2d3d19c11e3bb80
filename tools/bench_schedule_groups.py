#!/usr/bin/env python3
"""Measurements behind the schedule-group route's constants, on the benchmark's curve:
  segments   the 1 M-trade bench book (360 groups): the whole pricing call at R = 4 .. 64 records per wavefront, one wavefront
             per segment and a persistent grid walking them, against the direct route;
  min_group  262 144 trades in equal groups of s trades (s = 2 .. 64; distinct spreads split the 360 maturities): grouped
             against direct - the smallest s from which the grouped route is not slower;
  min_grouped  the book's natural groups, n = 2 048 .. 262 144 trades in all: the same by total count.
Variants are launched in turn (8 launches per round after 2 unrecorded ones), medians of the per-round averages in ms."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from adrates_amd import _native
from adrates_amd.market.curves.curve_tables import build_engine_curve
from adrates_amd.trades import synthetic
from adrates_amd.trades.market_data import README_VALUE_DT, gbp_model

FORCE, OFF = _native.SCHEDULE_GROUPS_FORCE, _native.SCHEDULE_GROUPS_OFF
P = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="segments,min_group,min_grouped")
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    curve = gbp_model().curves.GBP_OIS_SONIA
    host = build_engine_curve(curve.swap_rates, curve.swap_times, curve.year_fracs)
    ctx = _native.Context(0)
    dc = _native.DeviceCurve(ctx, 4, host.times, host.dfs, host.jac, host.hess)
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)

    def timed(variants, n):
        """variants: {name: DeviceTrades}; one set of output buffers for all."""
        pv = torch.empty(n, dtype=torch.float64, device=dev)
        de = torch.empty((n, P), dtype=torch.float64, device=dev)
        ga = torch.empty((n, P, P), dtype=torch.float64, device=dev)
        ag = torch.empty(1 + P + P * P, dtype=torch.float64, device=dev)
        def launch(t, k):
            for _ in range(k):
                _native.price_dev(ctx, dc, t, 7, pv.data_ptr(), de.data_ptr(), ga.data_ptr(), ag.data_ptr(), s.cuda_stream)
        res = {v: [] for v in variants}
        with torch.cuda.stream(s):
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.3:
                for t in variants.values():
                    launch(t, 4)
                torch.cuda.synchronize()
            for _ in range(args.rounds):
                for v, t in variants.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    launch(t, 2)
                    a.record(s); launch(t, 8); b.record(s)
                    torch.cuda.synchronize()
                    res[v].append(a.elapsed_time(b) / 8)
        return {v: round(statistics.median(x), 4) for v, x in res.items()}

    def upload(batch, mode, segment=None, blocks=0):
        t0 = time.perf_counter()
        t = _native.DeviceTrades(ctx, batch)
        ms = (time.perf_counter() - t0) * 1e3
        t.set_schedule_groups(mode, segment, blocks)
        return t, ms

    out = {}
    what = args.what.split(",")
    if "segments" in what:
        n = 1_000_000
        batch = synthetic.synthesize(README_VALUE_DT, n)
        variants, up = {}, []
        variants["direct"], ms = upload(batch, OFF); up.append(ms)
        for R in (4, 8, 16, 32, 64):
            variants[f"R={R}"], ms = upload(batch, FORCE, R); up.append(ms)
        for R, blocks in ((16, 2048), (32, 2048), (32, 1024), (256, 2048)):
            variants[f"R={R}, persistent {blocks} blocks"], ms = upload(batch, FORCE, R, blocks); up.append(ms)
        out["segments"] = timed(variants, n)
        out["upload_ms"] = [round(x, 1) for x in up]
        for t in variants.values():
            t.close()
        print(json.dumps(out), flush=True)
    if "min_group" in what:
        n = 262_144
        base = synthetic.synthesize(README_VALUE_DT, n, seed=3)
        months = np.round(base.flt_tp[base.flt_off[1:] - 1] * 12.0).astype(np.int64)     # the maturity, for the split
        order = np.argsort(months, kind="stable")
        rank = np.empty(n, dtype=np.int64)
        for m in np.unique(months):
            idx = order[months[order] == m]
            rank[idx] = np.arange(idx.size)
        rows = {}
        for size in (2, 4, 6, 8, 10, 12, 16, 24, 32, 64):
            import copy
            b = copy.copy(base)
            b.spread = 1e-7 * (rank // size)
            g, ms = upload(b, FORCE)
            d, _ = upload(b, OFF)
            r = timed({"grouped": g, "direct": d}, n)
            r["groups"] = g.schedule_groups_info()["used_groups"]
            rows[size] = r
            g.close(); d.close()
        out["min_group"] = rows
        print(json.dumps({"min_group": rows}), flush=True)
    if "min_grouped" in what:
        rows = {}
        for n in (2048, 4096, 8192, 16384, 32768, 65536, 131072, 262144):
            b = synthetic.synthesize(README_VALUE_DT, n, seed=4)
            g, _ = upload(b, FORCE)
            info = g.schedule_groups_info()
            d, _ = upload(b, OFF)
            r = timed({"grouped": g, "direct": d}, n)
            r["groups"], r["grouped_trades"] = info["used_groups"], info["used_trades"]
            rows[n] = r
            g.close(); d.close()
        out["min_grouped"] = rows
        print(json.dumps({"min_grouped": rows}), flush=True)


if __name__ == "__main__":
    main()
