"""FRN book benchmark: the adr_frn_measures kernel (DM from a clean price, prices, modified duration, dv01) on a million
FRNs, and the book's curve Greeks through the pricing route.  A few hundred distinct FRNs are compiled once and their
arrays tiled; every copy gets its own clean price.  Times are medians of warm launches between HIP events.
usage: bench_frns.py [n_frns] [distinct] [reps]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from adrates_amd import _native
from adrates_amd.market.position.frn_book import FRNBook, tile_frn_measures
from adrates_amd.trades.compiler import TradeBatch, compile_frns
from adrates_amd.trades.market_data import README_VALUE_DT, gbp_model, random_frn_book

HBM_BYTES_PER_S = 8e12

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
distinct = int(sys.argv[2]) if len(sys.argv) > 2 else 400
reps = max(20, int(sys.argv[3]) if len(sys.argv) > 3 else 30)
dev = torch.device("cuda", 0)
ctx = _native.default_context(0)
model = gbp_model()
frns, dm_true = random_frn_book(README_VALUE_DT, distinct, seed=11)
book = FRNBook(frns, model)
prices = _native.frn_measures_host(*book.inputs(dms=dm_true))["clean"]
disc, index, base, _ = book.inputs(clean_prices=prices)
copies = -(-n // distinct)
big = tile_frn_measures(base, copies)
big = {k: (v[:n + 1] if k == "cpn_off" else v[:n] if k in _native.FRN_FIELDS else v[:int(big["cpn_off"][n])])
       for k, v in big.items()}
big["frn_quote"] = big["frn_quote"] + np.random.default_rng(5).uniform(-0.25, 0.25, size=n)   # a price per copy
off, cpn, frn = _native.frn_pack(big)
m = cpn.shape[1]

host = {"disc_t": disc[1], "disc_df": disc[2], "index_t": index[1], "index_df": index[2], "cpn_off": off, "cpn": cpn,
        "frn": frn}
t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in host.items()}
out = torch.empty((len(_native.FRN_OUTPUTS), n), dtype=torch.float64, device=dev)
status = torch.empty(n, dtype=torch.int32, device=dev)
ptrs = {k: v.data_ptr() for k, v in t.items()}
s = torch.cuda.Stream(dev)
torch.cuda.synchronize()


def timed(launch, k):
    """Median ms of k launches on stream s, each between its own pair of events, after 5 warm-up launches."""
    with torch.cuda.stream(s):
        for _ in range(5):
            launch()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(k)]
        for a, b in ev:
            a.record(s)
            launch()
            b.record(s)
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


ms = timed(lambda: _native.frn_measures_dev(ctx, disc[0], disc[1].size, index[0], index[1].size, n, m, ptrs, False,
                                            out.data_ptr(), status.data_ptr(), s.cuda_stream), reps)
st = status.cpu().numpy()
res = {"frns": n, "distinct_frns": distinct, "coupons": m, "coupons_per_frn": m / n, "launches": reps,
       "status_counts": {str(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))}}
# bytes the kernel must move: 7 doubles per coupon, 11 doubles and an offset per FRN in, 6 doubles and a status out
bytes_moved = 7 * 8 * m + (11 * 8 + 8) * n + (6 * 8 + 4) * n
res["measures"] = {"ms": ms, "frns_per_s": n / ms * 1e3, "bytes": bytes_moved,
                   "GBps": bytes_moved / ms / 1e6, "fraction_of_8TBps": bytes_moved / (ms * 1e-3) / HBM_BYTES_PER_S}

# curve Greeks of the same book through the pricing route (float coupons, fixed flows for the principal and fixings)
tb, _ = compile_frns(frns, README_VALUE_DT)       # coupons paid on the value date are a host-side PV constant: untimed
fl = np.tile(tb.fix_off[1:] - tb.fix_off[:-1], copies)[:n]
ll = np.tile(tb.flt_off[1:] - tb.flt_off[:-1], copies)[:n]
fo = np.concatenate(([0], np.cumsum(fl))).astype(np.int64)
lo = np.concatenate(([0], np.cumsum(ll))).astype(np.int64)
kf, kl = int(fo[-1]), int(lo[-1])
tile = lambda a, k: np.tile(a, copies)[:k]
big_tb = TradeBatch(fo, lo, tile(tb.fix_tp, kf), tile(tb.fix_pay, kf), tile(tb.flt_tp, kl), tile(tb.flt_ts, kl),
                    tile(tb.flt_te, kl), tile(tb.flt_alpha, kl), tile(tb.notional, n), tile(tb.spread, n), np.ones(n),
                    np.ones(n))
cur = book._engine._device_curve(book.curve)
dtr = _native.DeviceTrades(ctx, big_tb)
P = cur["dev"].n_pillars
agg = torch.empty(1 + P + P * P, dtype=torch.float64, device=dev)
pv = torch.empty(n, dtype=torch.float64, device=dev)
delta = torch.empty((n, P), dtype=torch.float64, device=dev)
res["greeks"] = {
    "value+delta+gamma, aggregate_ms": timed(lambda: _native.price_dev(ctx, cur["dev"], dtr, 7, 0, 0, 0, agg.data_ptr(),
                                                                        s.cuda_stream), reps),
    "value+delta, per-frn_ms": timed(lambda: _native.price_dev(ctx, cur["dev"], dtr, 3, pv.data_ptr(), delta.data_ptr(), 0, 0,
                                                                s.cuda_stream), reps),
    "input_bytes": dtr.input_bytes}
dtr.close()
print(json.dumps(res))
