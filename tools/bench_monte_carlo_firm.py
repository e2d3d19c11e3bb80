"""Monte Carlo full revaluation of a firm, benchmark (adr_shock_columns_dev and adr_scenario_rows_merge_dev,
csrc/shock_columns.hip; `monte_carlo_revalue_firm_var_es`' chain): the README GBP curve (K = 264 knots, P = 32), G = 8
spread buckets and a 12-pillar RPI curve (Q = 52 shock columns), n trades per line - synthetic off-grid OIS, and a few
hundred distinct bonds + FRNs and YoY swaps tiled - in B desks of equal size that every line shares, level 0.99.

  1. the two new kernels alone at the largest S, resident buffers, medians of warm repetitions between HIP events on one
     stream: adr_shock_columns_dev for dz [S, 8] and for b [S, 12] out of the [S, 52] rows, adr_scenario_rows_merge_dev of a
     [B, S] tile into [B, S + 1] (copy and add);
  2. the chain, `monte_carlo_revalue_firm_var_es`, at every S of the list, by the HOST clock around the public call: the
     uploads of the three books, the allocations and the download of the [B] vectors are inside;
  3. the route the chain replaces, at the smallest S, by the host clock: download the shock rows, `ShockedCurves.dfs` on
     them, NumPy slices for dz and b, `revalue_on_curves_sub_books`, the credit sub-book launch (the entry
     `revalue_credit_on_curves_sub_books` calls - the function itself takes trade objects, and the tiled book has none),
     `revalue_yoy_on_curves_sub_books`, `combine_sub_book_rows` and `tail_measures_select`; its var must have the chain's bits;
  4. `monte_carlo_revalue_var_es` on the rates book, host clock, under the key `parent` as before: it wraps the book in a
     rates-only `FirmBook` and runs the same chain, so there is no ratio to take; that a rates-only `FirmBook` gives its var
     and es bits is still asserted.
usage: bench_monte_carlo_firm.py [reps] [out.json] [n per line] [S,S,..] [desks]"""
import json, os, socket, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from adrates_amd import _native
from adrates_amd.market.position.monte_carlo import (ShockedCurves, factor_from_covariance, monte_carlo_revalue_var_es,
                                                     monte_carlo_shocks, tail_measures_select)
from adrates_amd.market.position.monte_carlo_firm import FirmBook, _Line, firm_scenario_bytes, monte_carlo_revalue_firm_var_es
from adrates_amd.market.position.scenarios import combine_sub_book_rows, revalue_on_curves_sub_books, revalue_yoy_on_curves_sub_books
from adrates_amd.market.position.yoy_book import YoYBook, tile_yoy_book
from adrates_amd.trades import synthetic
from adrates_amd.trades.compiler import TradeBatch
from adrates_amd.trades.market_data import (INFL_PX, INFL_TENORS, README_VALUE_DT, gbp_model, random_bond_book, random_frn_book,
                                            random_yoy_book, yoy_model)
from adrates_amd.utils import InterpTypes

reps = max(3, int(sys.argv[1]) if len(sys.argv) > 1 else 3)
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(root, "profiles", "monte_carlo_firm_bench.json")
N = int(sys.argv[3]) if len(sys.argv) > 3 else 100_000
SCENARIOS = tuple(int(v) for v in sys.argv[4].split(",")) if len(sys.argv) > 4 else (16384, 262144)
B = int(sys.argv[5]) if len(sys.argv) > 5 else 100
LEVEL, MAX_BYTES, SEED, DISTINCT, G = 0.99, 2 ** 33, 7, 400, 8
PILLARS_12 = ("1Y", "2Y", "3Y", "5Y", "7Y", "10Y", "12Y", "15Y", "20Y", "30Y", "40Y", "50Y")
VD, INTERP = README_VALUE_DT, InterpTypes.FLAT_FWD_RATES
dev = torch.device("cuda", 0)
ctx = _native.default_context(0)
stream = torch.cuda.Stream(dev)
q = stream.cuda_stream
new = lambda *shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device=dev)
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
assert N % DISTINCT == 0 and N % B == 0


def stats(t):
    return {"ms": float(np.median(t)), "spread": (max(t) - min(t)) / float(np.median(t)), "runs": len(t)}


def host_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def events_ms(fns, k):
    """Per function: the times (ms) of ``k`` alternating repetitions, each between its own events, after a warm-up."""
    with torch.cuda.stream(stream):
        for f in fns:
            f()
        stream.synchronize()
        ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(k)]
        for row in ev:
            for (a, b), f in zip(row, fns):
                a.record(stream); f(); b.record(stream)
    torch.cuda.synchronize()
    return [[row[i][0].elapsed_time(row[i][1]) for row in ev] for i in range(len(fns))]


def tile_credit(line, n):
    """The credit line's compiled book repeated to ``n`` trades (tools/bench_credit_scenarios.py: tile)."""
    b = line.batch
    r = n // b.n_trades
    def flows(off, *arrays):
        counts = np.tile(np.diff(off), r)
        return np.concatenate(([0], np.cumsum(counts))).astype(np.int64), [np.tile(a, r) for a in arrays]
    fix_off, (fix_tp, fix_pay, fix_tau) = flows(b.fix_off, b.fix_tp, b.fix_pay, line.fix_tau)
    flt_off, (flt_tp, flt_ts, flt_te, flt_al, flt_tau) = flows(b.flt_off, b.flt_tp, b.flt_ts, b.flt_te, b.flt_alpha, line.flt_tau)
    per = lambda a: np.tile(a, r)
    batch = TradeBatch(fix_off, flt_off, fix_tp, fix_pay, flt_tp, flt_ts, flt_te, flt_al, per(b.notional), per(b.spread),
                       per(b.fix_sign), per(b.flt_sign))
    return dict(batch=batch, z=per(line.z), bucket=per(line.bucket), fix_tau=fix_tau, flt_tau=flt_tau)


def tile_yoy(line, n):
    r = n // line.n
    off = np.concatenate(([0], np.cumsum(np.tile(np.diff(line.fixed[0]), r)))).astype(np.int64)
    return dict(fixed=(off, np.tile(line.fixed[1], r), np.tile(line.fixed[2], r)), coupons=tile_yoy_book(line.coupons, r), im=line.im,
                T=line.T, b0=line.b0)


model = gbp_model(VD, INTERP)
picks = [INFL_TENORS.index(t) for t in PILLARS_12]
infl_model = yoy_model(VD, INTERP, tenors=list(PILLARS_12), px=[INFL_PX[i] for i in picks])
curves = ShockedCurves(model, "GBP_OIS_SONIA", ctx=ctx)
K, P = curves.n_knots, curves.n_pillars
sub_off = np.linspace(0, N, B + 1).astype(np.int64)
keys = [int(b) for b in np.repeat(np.arange(B), np.diff(sub_off))]
rates_batch = synthetic.synthesize(VD, N, seed=11)
rng = np.random.default_rng(19)
bonds, _ = random_bond_book(VD, DISTINCT // 2, seed=17)
frns, _ = random_frn_book(VD, DISTINCT - DISTINCT // 2, seed=18)
spreads = np.concatenate([rng.uniform(-50e-4, 800e-4, len(bonds)), rng.uniform(-50e-4, 300e-4, len(frns))])
buckets = [f"bucket {i % G}" for i in range(DISTINCT)]
yoy = YoYBook(random_yoy_book(VD, DISTINCT, seed=13), infl_model)
firm = FirmBook(curves, rates=(rates_batch, keys), credit=(bonds + frns, spreads, [0] * DISTINCT, buckets), inflation=(yoy, [0] * DISTINCT))
for i, line in enumerate(firm.lines):                   # the distinct trades tiled to N per line, in the B desks of the rates line
    if line.kind != "rates":
        firm.lines[i] = _Line(line.kind, None, range(B), sub_off, N, **(tile_credit if line.kind == "credit" else tile_yoy)(line, N))
firm._index_desks()
cols, Q = firm.columns, firm.n_columns
Pi = len(cols["breakeven"])
assert (P, len(cols["spread"]), Pi, Q, firm.n_desks) == (32, G, 12, 52, B)
A = rng.standard_normal((Q, Q + 4))
L = factor_from_covariance(A @ A.T * 4.0)               # bp^2: a daily move of about 15 bp per column
result = {"reps": reps, "knots": K, "columns": {"curve": P, "spread": G, "breakeven": Pi}, "level": LEVEL, "max_bytes": MAX_BYTES,
          "trades_per_line": N, "distinct_credit_trades": DISTINCT, "distinct_yoy_swaps": DISTINCT, "desks": B,
          "scenario_bytes": firm_scenario_bytes(firm),
          "box": {"host": socket.gethostname(), "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                  "hip": getattr(torch.version, "hip", None)}}

# ---------------------------------------------------------------------------------------------- 1. the kernels alone
S = max(SCENARIOS)
x = up(monte_carlo_shocks(L, S, SEED, ctx=ctx))
dz, b, d_b0 = new(S, G), new(S, Pi), up(firm.line("inflation").b0)
bad = torch.zeros(S, dtype=torch.int32, device=dev)
tile, rows = new(B, S), new(B, S + 1)
target, add0, add1 = up(np.arange(B, dtype=np.int64)), up(np.zeros(B, dtype=np.int32)), up(np.ones(B, dtype=np.int32))
tile.normal_(); rows.zero_()
fns = [lambda: _native.shock_columns_dev(ctx, S, Q, x.data_ptr(), P, G, dz.data_ptr(), bad_ptr=bad.data_ptr(), stream=q),
       lambda: _native.shock_columns_dev(ctx, S, Q, x.data_ptr(), P + G, Pi, b.data_ptr(), base_ptr=d_b0.data_ptr(), floor=-1.0,
                                         bad_ptr=bad.data_ptr(), stream=q),
       lambda: _native.scenario_rows_merge_dev(ctx, B, S, tile.data_ptr(), B, S + 1, 0, rows.data_ptr(), target.data_ptr(),
                                               add0.data_ptr(), stream=q),
       lambda: _native.scenario_rows_merge_dev(ctx, B, S, tile.data_ptr(), B, S + 1, 0, rows.data_ptr(), target.data_ptr(),
                                               add1.data_ptr(), stream=q)]
names = ("shock_columns_dz", "shock_columns_b", "rows_merge_copy", "rows_merge_add")
moved = (8 * S * 2 * G, 8 * S * 2 * Pi, 8 * B * S * 2, 8 * B * S * 3)          # bytes read + written, the flags and maps aside
result["kernels"] = {"scenarios": S}
for name, t, nbytes in zip(names, events_ms(fns, max(reps, 5)), moved):
    result["kernels"][name] = dict(stats(t), bytes=nbytes, GB_per_s=nbytes * 1e-6 / float(np.median(t)))
assert int(bad.count_nonzero()) == 0
print(json.dumps(result["kernels"]), flush=True)
del x, dz, b, tile, rows
torch.cuda.empty_cache()

# ------------------------------------------------------------------------------------------------------ 2. the chain
result["chain"] = []
chain_out = {}
for S in SCENARIOS:
    call = lambda: monte_carlo_revalue_firm_var_es(firm, L, S, level=LEVEL, seed=SEED, max_bytes=MAX_BYTES)
    call()
    t = []
    for _ in range(reps):
        ms, chain_out[S] = host_ms(call)
        t.append(ms)
    rec = dict(stats(t), scenarios=S, clock="host, around the public call")
    result["chain"].append(rec)
    print(json.dumps(rec), flush=True)

# ------------------------------------------------------------------------------------------- 3. the route it replaces
S = min(SCENARIOS)
credit, infl = firm.line("credit"), firm.line("inflation")
d_x = up(monte_carlo_shocks(L, S, SEED, ctx=ctx))
torch.cuda.synchronize()


def old_route():
    steps = {}
    steps["download_ms"], xs = host_ms(lambda: np.vstack([d_x.cpu().numpy(), np.zeros((1, Q))]))
    steps["dfs_ms"], (dfs, flags) = host_ms(lambda: curves.dfs(xs))
    steps["slices_ms"], (s_dz, s_b) = host_ms(lambda: (xs[:, P:P + G] * 1e-4, infl.b0 + xs[:, P + G:] * 1e-4))
    times = curves.base.times
    steps["rates_ms"], r = host_ms(lambda: revalue_on_curves_sub_books(INTERP, times, dfs, rates_batch, keys, VD, ctx=ctx))

    def credit_launch():
        with _native.DeviceTrades(ctx, credit.batch) as trades:
            return _native.credit_scenario_subbook_pv(ctx, curves.method, times, dfs, s_dz, trades, credit.z, credit.bucket,
                                                      credit.fix_tau, credit.flt_tau, sub_off)
    steps["credit_ms"], c = host_ms(credit_launch)
    steps["yoy_ms"], y = host_ms(lambda: revalue_yoy_on_curves_sub_books(INTERP, times, dfs, infl.im, infl.T, s_b,
                                                                         (infl.fixed, infl.coupons), keys, VD, ctx=ctx))
    steps["combine_ms"], rows = host_ms(lambda: combine_sub_book_rows([(r["labels"], r["sub_pv"]), (list(range(B)), c["sub_pv"]),
                                                                       (y["labels"], y["sub_pv"])])["rows"])
    steps["tail_ms"], (var, es) = host_ms(lambda: tail_measures_select(rows, LEVEL, base_col=S, ctx=ctx))
    assert not flags.any()
    return steps, var, es


old_route()
runs = [old_route() for _ in range(reps)]
total = [sum(steps.values()) for steps, _, _ in runs]
chain_ms = next(c["ms"] for c in result["chain"] if c["scenarios"] == S)
same = all(np.array_equal(v.view(np.int64), chain_out[S]["var"].view(np.int64)) and np.array_equal(e.view(np.int64), chain_out[S]["es"].view(np.int64))
           for _, v, e in runs)
assert same, "the route the chain replaces gives other bits"
result["replaced_route"] = dict(stats(total), scenarios=S, steps={k: float(np.median([s[k] for s, _, _ in runs])) for k in runs[0][0]},
                                same_var_es_bits_as_chain=same, over_chain=float(np.median(total)) / chain_ms)
print(json.dumps(result["replaced_route"]), flush=True)
del d_x

# ----------------------------------------------------------------- 4. the rates entry point, a wrapper of the same chain
rates_firm = FirmBook(curves, rates=(rates_batch, keys))
L32 = L[:P, :P].copy()
result["rates_only"] = []
for S in SCENARIOS:
    call = lambda: monte_carlo_revalue_var_es(curves, rates_batch, keys, L32, S, level=LEVEL, seed=SEED, max_bytes=MAX_BYTES)
    want = monte_carlo_revalue_firm_var_es(rates_firm, L32, S, level=LEVEL, seed=SEED, max_bytes=MAX_BYTES)
    call()
    t = []
    for _ in range(reps):
        ms, out = host_ms(call)
        t.append(ms)
    same = all(np.array_equal(want[k].view(np.int64), out[k].view(np.int64)) for k in ("var", "es"))
    assert same and want["labels"] == out["labels"], "a rates-only firm gives other bits than monte_carlo_revalue_var_es"
    rec = {"scenarios": S, "parent": stats(t), "same_var_es_bits": same}
    result["rates_only"].append(rec)
    print(json.dumps(rec), flush=True)

result["not_measured"] = [
    "the chain's split by step and by line: its launches run on the context's own stream, which the tool cannot put events on",
    "the chain with resident books: the host clock includes the uploads of the three books and the allocations of every call",
    "trade objects in the replaced route's credit step: the tiled book has none, so compile_credit_book's time is left out, in its favour",
    "more than one repetition count, desk count or book size; other interpolation schemes; more than one device",
]
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps({"written": out_path}))
