"""Bond book benchmark: the adr_bond_measures kernel (z from a clean price, prices, dv01, yield, duration, convexity) on a
million bonds, and the book's curve Greeks through the pricing route.  A few hundred distinct bonds are compiled once and
their arrays tiled; every copy gets its own clean prices.  Times are medians of warm launches between HIP events.
usage: bench_bonds.py [n_bonds] [distinct] [reps]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from adrates_amd import _native
from adrates_amd.market.position.bond_book import BondBook, tile_bond_measures
from adrates_amd.trades.compiler import TradeBatch, compile_bonds
from adrates_amd.trades.market_data import README_VALUE_DT, gbp_model, random_bond_book
from adrates_amd.utils import RequestTypes

HBM_BYTES_PER_S = 8e12

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
distinct = int(sys.argv[2]) if len(sys.argv) > 2 else 400
reps = max(20, int(sys.argv[3]) if len(sys.argv) > 3 else 30)
dev = torch.device("cuda", 0)
ctx = _native.default_context(0)
model = gbp_model()
curve = model.curves.GBP_OIS_SONIA
bonds, z_true = random_bond_book(README_VALUE_DT, distinct, seed=11)
prices = np.array([b.clean_price(README_VALUE_DT, curve, z, README_VALUE_DT) for b, z in zip(bonds, z_true)])
book = BondBook(bonds, model)
method, node_t, node_df, base, _ = book.inputs(clean_prices=prices)
copies = -(-n // distinct)
big = tile_bond_measures(base, copies)
big = {k: (v[:n + 1] if k == "flow_off" else v[:n] if k in _native.BOND_FIELDS else v[:int(big["flow_off"][n])])
       for k, v in big.items()}
big["bond_quote"] = big["bond_quote"] + np.random.default_rng(5).uniform(-0.25, 0.25, size=n)   # a price per copy
m = int(big["flow_off"][-1])

t = {"node_t": torch.from_numpy(node_t).to(dev), "node_df": torch.from_numpy(node_df).to(dev)}
for k, v in big.items():
    t[k] = torch.from_numpy(np.ascontiguousarray(v)).to(dev)
out = torch.empty((len(_native.BOND_OUTPUTS), n), dtype=torch.float64, device=dev)
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


ms = timed(lambda: _native.bond_measures_dev(ctx, method, node_t.size, n, ptrs, False, out.data_ptr(), status.data_ptr(),
                                             s.cuda_stream), reps)
st = status.cpu().numpy()
res = {"bonds": n, "distinct_bonds": distinct, "flows": m, "flows_per_bond": m / n, "launches": reps,
       "status_counts": {str(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))}}
# bytes the kernel must move: 4 doubles per flow, 5 doubles and an offset per bond in, 7 doubles and a status out
bytes_moved = 32 * m + (5 * 8 + 8) * n + (7 * 8 + 4) * n
res["measures"] = {"ms": ms, "bonds_per_s": n / ms * 1e3, "bytes": bytes_moved,
                   "GBps": bytes_moved / ms / 1e6, "fraction_of_8TBps": bytes_moved / (ms * 1e-3) / HBM_BYTES_PER_S}

# curve Greeks of the same book through the pricing route (fixed flows, face on the last flow)
tb = compile_bonds(bonds, README_VALUE_DT)
lens = np.tile(tb.fix_off[1:] - tb.fix_off[:-1], copies)[:n]
fo = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
k_fix = int(fo[-1])
empty = np.zeros(0)
big_tb = TradeBatch(fo, np.zeros(n + 1, dtype=np.int64), np.tile(tb.fix_tp, copies)[:k_fix], np.tile(tb.fix_pay, copies)[:k_fix],
                    empty, empty, empty, empty, np.tile(tb.notional, copies)[:n], np.zeros(n), np.ones(n), np.ones(n))
cur = book._engine._device_curve(curve)
dtr = _native.DeviceTrades(ctx, big_tb)
P = cur["dev"].n_pillars
agg = torch.empty(1 + P + P * P, dtype=torch.float64, device=dev)
pv = torch.empty(n, dtype=torch.float64, device=dev)
delta = torch.empty((n, P), dtype=torch.float64, device=dev)
res["greeks"] = {
    "value+delta+gamma, aggregate_ms": timed(lambda: _native.price_dev(ctx, cur["dev"], dtr, 7, 0, 0, 0, agg.data_ptr(),
                                                                        s.cuda_stream), reps),
    "value+delta, per-bond_ms": timed(lambda: _native.price_dev(ctx, cur["dev"], dtr, 3, pv.data_ptr(), delta.data_ptr(), 0, 0,
                                                                 s.cuda_stream), reps),
    "input_bytes": dtr.input_bytes}
dtr.close()
print(json.dumps(res))
