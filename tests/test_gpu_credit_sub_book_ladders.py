"""Credit sub-book Greeks on the GPU (adr_credit_subbook_ladders*): the desks' augmented ladders of one launch chain against
the C oracle on rescaled batches, the host twin, the desks priced alone (bit for bit), and the delta-gamma P&L they give
against full revaluation under joint (curve, spread) shocks."""
import numpy as np
import pytest
import torch

from adrates_amd import _native
from adrates_amd.market.position.scenarios import ScenarioGrid, tail_measures
from adrates_amd.utils import InterpTypes
from adrates_amd.utils.error import LibError

from . import _credit_ladder_cases as X
from . import _fixtures as F
from . import _ladder_pnl_cases as C
from . import _sub_book_ladder_cases as L
from .test_gpu_parity_batch import _device_curve
from .test_gpu_sub_book_ladders import _curve_for

pytestmark = pytest.mark.gpu


def check_book(ctx, method, host, dc, case, G, sub_off, what, key=None):
    """Device against the oracle's sums and against the host twin, both at 1e-10 of the desk's or cell's absolute sums; two
    launches bit for bit; the layout of the augmented rows."""
    ref = X.reference(method, host, case, key)
    got = X.device_ladders(ctx, dc, case, G, sub_off)
    again = X.device_ladders(ctx, dc, case, G, sub_off)
    twin = X.host_ladders(method, host, case, G, sub_off)
    e_ref, e_twin = X.errors(got, ref, case, sub_off, G), X.between(got, twin, ref, case, sub_off, G)
    print(f"{what}: device vs oracle desks {e_ref['desk']:.2e} cells {e_ref['cell']:.2e}, device vs host twin {e_twin:.2e}")
    assert e_ref["desk"] <= 1e-10 and e_ref["cell"] <= 1e-10 and e_twin <= 1e-10
    assert X.same_bits(got, again), "two launches differ"
    X.check_layout(got, dc.n_pillars, G)
    return got


@pytest.mark.parametrize("G", (0, 1, 32))
@pytest.mark.parametrize("interp", L.SCHEMES)
def test_geometry(gpu_ctx, interp, G):
    """Desks of GEOMETRY_SIZES trades, bonds and lag-free FRNs mixed: one cell of 65 trades (two chunks), one desk of G + 1
    cells, one all unbucketed, one that lacks most buckets.  Observed on an MI355X, worst over the schemes and G (bound
    1e-10): against the oracle desks 3.6e-13 (the one-trade desk's gamma, an FRN whose gamma nets far below its gross; 8.6e-12
    before oracle/port.c priced coupons paid on their accrual end in linear form - the oracle's own error, see
    tests/test_ladder_edges_host.py), cells 8.1e-15; against the host twin 3.5e-15."""
    curve = F.gbp_model(L.VD, interp).curves.GBP_OIS_SONIA
    host, dc = _device_curve(gpu_ctx, curve)
    case, sub_off = X.geometry_case(G)
    got = check_book(gpu_ctx, interp.value, host, dc, case, G, sub_off, f"geometry {interp.name} G = {G}", ("geometry", interp, G))
    for b in range(len(X.GEOMETRY_SIZES)):
        lo, hi = int(sub_off[b]), int(sub_off[b + 1])
        if hi == lo:
            row = got["ladders"][b]
            assert not np.any(row) and not np.any(np.signbit(row)), f"empty desk {b}"
            continue
        alone = X.device_ladders(gpu_ctx, dc, X.take(case, lo, hi), G, np.array([0, hi - lo]))
        assert X.same_bits(X.row_of(got, b), alone), f"desk {b} alone"


@pytest.mark.parametrize("interp", L.SCHEMES)
def test_no_spread_against_the_sub_book_ladder(gpu_ctx, interp):
    """z = 0, G = 0 against adr_subbook_ladders on the same batch and desks.  On the host the two twins agree bit for bit
    (tests/test_credit_sub_book_ladders_host.py); on the device they do NOT (observed on an MI355X: the two knot kernels are
    different programs, and the order in which the lanes' LDS adds of a chunk land is a property of each): PV and delta
    have the same bits, 1 to 3 of the 7 168 gamma entries differ, by at most 5.8e-18 of the desk's absolute sums.  So the
    rows are held to the project's 1e-10 on that scale and the count of differing entries is printed."""
    curve = F.gbp_model(L.VD, interp).curves.GBP_OIS_SONIA
    host, dc = _device_curve(gpu_ctx, curve)
    case, sub_off = X.geometry_case(0)
    n = case.batch.n_trades
    case = X.Case(case.batch, np.zeros(n), np.full(n, -1, dtype=np.int32), case.fix_tau, case.flt_tau)
    got = X.device_ladders(gpu_ctx, dc, case, 0, sub_off)
    with _native.DeviceTrades(gpu_ctx, case.batch) as dt:
        want = _native.subbook_ladders(gpu_ctx, dc, dt, sub_off)
    ref = L.oracle_rows(interp.value, host, case.batch)
    worst = L.rows_errors(got, want, ref, sub_off)
    differ = {k: int(np.sum(np.asarray(got[k]).view(np.int64) != np.asarray(want[k]).view(np.int64))) for k in ("pv", "delta", "gamma")}
    print(f"z = 0, G = 0 vs adr_subbook_ladders, {interp.name}: {worst:.2e}; entries whose bits differ: {differ}")
    assert worst <= 1e-10


@pytest.mark.parametrize("pillars,G", [(17, 5), (32, 32), (40, 3), ("weekly", 2)])
def test_pillar_layouts(gpu_ctx, pillars, G):
    """P = 17 with G = 5 (odd Q), P = 32 with G = 32 (Q = 64), P = 40 (the wide lj_at / lc_at layout) and the curve with the
    weekly short end, whose four tables fit the LDS budget (the refusal would be the test if they did not).  Observed on an
    MI355X: at most 3.2e-13 (desks) and 3.6e-14 (cells) against the oracle, 9.3e-15 against the host twin."""
    curve = F.gbp_model(L.VD, InterpTypes.LINEAR_ZERO_RATES).curves.GBP_OIS_SONIA if pillars == 32 else _curve_for(pillars)
    host, dc = _device_curve(gpu_ctx, curve)
    if pillars != "weekly":
        assert dc.n_pillars == pillars
    book = X.take(X.geometry_case(0)[0], 0, 200).batch
    rng = np.random.default_rng(G)
    case = X.spreads_for(book, np.where(rng.random(200) < 0.3, -1, rng.integers(0, G, 200)), 50 + G)
    case, sub_off, _ = X.order_by_cells(case, np.repeat([0, 1, 2], [70, 1, 129]), 3)
    check_book(gpu_ctx, 4, host, dc, case, G, sub_off, f"{pillars} pillars, G = {G} (Kc from {host.times.size} knots)")


def test_more_chunks_than_waves_of_the_grid(gpu_ctx):
    """128 desks of 33 one-trade cells: 4 224 chunks, more than the grid has waves (16 x the compute units), so waves take a
    second chunk on re-zeroed tables - all four of them.  Observed on an MI355X: 2.9e-14 (desks) and 4.0e-13 (cells: the
    scale of a one-trade cell is that trade alone) against the oracle, 7.7e-15 against the host twin."""
    interp = InterpTypes.LINEAR_ZERO_RATES
    curve = F.gbp_model(L.VD, interp).curves.GBP_OIS_SONIA
    host, dc = _device_curve(gpu_ctx, curve)
    G, B = 32, 128
    n = B * (G + 1)
    base = X.geometry_case(0)[0]
    book = X.permute(base, np.arange(n) % base.batch.n_trades).batch
    case = X.spreads_for(book, np.tile(np.arange(-1, G), B), 61)
    sub_off = np.arange(0, n + 1, G + 1).astype(np.int64)
    cell_off, desk_cell_off, cell_bucket = _native.credit_subbook_cells(case.bucket, sub_off)
    plan = _native.scenario_subbook_plan(n, cell_off)
    assert cell_bucket.size == n and plan[n] == n > 16 * 256
    got = check_book(gpu_ctx, interp.value, host, dc, case, G, sub_off, "128 desks, 4 224 one-trade cells")
    for b in (0, 127):
        lo, hi = int(sub_off[b]), int(sub_off[b + 1])
        alone = X.device_ladders(gpu_ctx, dc, X.take(case, lo, hi), G, np.array([0, hi - lo]))
        assert X.same_bits(X.row_of(got, b), alone), f"desk {b} alone"


def test_requests(gpu_ctx):
    """VALUE + DELTA runs the kernel without the gamma tables (8 Kc bytes per wave): the gamma blocks are zeros, PV, delta
    and CS01 agree with the oracle; VALUE alone leaves the PV."""
    interp = InterpTypes.FLAT_FWD_RATES
    curve = F.gbp_model(L.VD, interp).curves.GBP_OIS_SONIA
    host, dc = _device_curve(gpu_ctx, curve)
    G = 32
    case, sub_off = X.geometry_case(G)
    ref = X.reference(interp.value, host, case, ("geometry", interp, G))
    full = X.device_ladders(gpu_ctx, dc, case, G, sub_off)
    d_only = X.device_ladders(gpu_ctx, dc, case, G, sub_off, want_gamma=False)
    v_only = X.device_ladders(gpu_ctx, dc, case, G, sub_off, want_delta=False, want_gamma=False)
    for k in ("gamma", "spread_gamma", "cross_gamma"):
        assert not np.any(d_only[k]) and not np.any(np.signbit(d_only[k])), k
    assert np.any(d_only["cs01"]) and not np.any(v_only["ladders"][:, 1:])
    filled = dict(d_only, gamma=full["gamma"], spread_gamma=full["spread_gamma"], cross_gamma=full["cross_gamma"])
    e = X.errors(filled, ref, case, sub_off, G)
    assert e["desk"] <= 1e-10 and e["cell"] <= 1e-10
    e = X.errors(dict(full, pv=v_only["pv"]), ref, case, sub_off, G)
    assert e["desk"] <= 1e-10
    twin = X.host_ladders(interp.value, host, case, G, sub_off, want_gamma=False)
    assert X.between(d_only, twin, ref, case, sub_off, G) <= 1e-10


def test_dev_entry_in_guarded_buffers(gpu_ctx):
    """adr_credit_subbook_ladders_dev on a caller's stream and buffers: 16 words behind `out` and behind the scratch keep
    their pattern, and the rows have the blocking entry's bits."""
    interp = InterpTypes.LINEAR_ZERO_RATES
    curve = F.gbp_model(L.VD, interp).curves.GBP_OIS_SONIA
    host, dc = _device_curve(gpu_ctx, curve)
    G = 32
    case, sub_off = X.geometry_case(G)
    B, Q, n = len(X.GEOMETRY_SIZES), dc.n_pillars + G, case.batch.n_trades
    stride = 1 + Q + Q * Q
    cell_off, desk_cell_off, cell_bucket = _native.credit_subbook_cells(case.bucket, sub_off)
    n_cells = cell_bucket.size
    work, chunks = _native.credit_subbook_ladders_work(dc, n, B, n_cells)
    assert chunks == (n + 63) // 64 + n_cells
    guard = 16
    out = torch.full((B * stride + guard,), -7.25, dtype=torch.float64, device="cuda")
    scratch = torch.full((work + guard,), -7.25, dtype=torch.float64, device="cuda")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    bufs = {"z": up(case.z), "bucket": up(case.bucket), "fix_tau": up(case.fix_tau), "flt_tau": up(case.flt_tau),
            "cell_plan": up(_native.scenario_subbook_plan(n, cell_off)), "desk_cell_off": up(desk_cell_off), "cell_bucket": up(cell_bucket)}
    stream = torch.cuda.Stream()
    with _native.DeviceTrades(gpu_ctx, case.batch) as dt:
        _native.credit_subbook_ladders_dev(gpu_ctx, dc, dt, case.fix_tau.size, case.flt_tau.size, G, B, n_cells,
                                           {k: v.data_ptr() for k, v in bufs.items()}, 7, out.data_ptr(), scratch.data_ptr(),
                                           stream.cuda_stream)
        stream.synchronize()
        want = _native.credit_subbook_ladders(gpu_ctx, dc, dt, case.z, case.bucket, case.fix_tau, case.flt_tau, G, sub_off)
    rows = out[:B * stride].cpu().numpy().reshape(B, stride)
    assert X.same_bits({"ladders": rows}, want)
    assert bool((out[B * stride:] == -7.25).all()) and bool((scratch[work:] == -7.25).all())


def test_refusals(gpu_ctx):
    interp = InterpTypes.LINEAR_ZERO_RATES
    curve = F.gbp_model(L.VD, interp).curves.GBP_OIS_SONIA
    host, dc = _device_curve(gpu_ctx, curve)
    case, sub_off = X.geometry_case(5)
    bad = X.Case(case.batch, case.z, case.bucket.copy(), case.fix_tau, case.flt_tau)
    j = int(sub_off[5]) + 40
    bad.bucket[j] = bad.bucket[j - 1] - 1 if bad.bucket[j - 1] >= 0 else 4
    bad.bucket[j - 1] = max(bad.bucket[j - 1], bad.bucket[j] + 1)
    with pytest.raises(LibError, match=f"sub-book 5 is not ordered by bucket: trade {j} ") as e:
        X.device_ladders(gpu_ctx, dc, bad, 5, sub_off)
    assert e.value.status == -1
    with pytest.raises(LibError, match="ADR_CREDIT_MAX_BUCKETS"):
        X.device_ladders(gpu_ctx, dc, case, 33, sub_off)
    z = case.z.copy()
    z[7] = np.nan
    with pytest.raises(LibError, match=r"trade 7\)"):
        X.device_ladders(gpu_ctx, dc, X.Case(case.batch, z, case.bucket, case.fix_tau, case.flt_tau), 5, sub_off)


@pytest.mark.parametrize("interp", L.SCHEMES)
def test_explain_against_full_revaluation(gpu_ctx, interp):
    """`ScenarioGrid.explain_credit_sub_books` on bond, FRN and OIS desks under joint shocks h (u, v), h = 4, 8, 16 bp: the
    unexplained P&L is third order per desk and direction, the gap of delta alone second order, the zero pair exactly 0;
    the chained VaR / ES has `tail_measures`' bits.  The desk-directions left out are `_credit_ladder_cases.EXPLAIN_DROPPED`
    (out of band in the reference itself).  Observed on the device: the host route's ranges."""
    model, ir = C.gbp(interp)
    tenors = model._curve_params_dict["GBP_OIS_SONIA"]["tenor_list"]
    trades, spreads, keys, buckets = X.explain_book()
    G = len(X.EXPLAIN_BUCKETS)
    x, dz = X.joint_shock_rows(len(tenors), G)
    shocks = [{t: v / 100.0 for t, v in zip(tenors, row)} for row in x]          # the same shocks in percent
    grid = ScenarioGrid(model, "GBP_OIS_SONIA", shocks, ctx=gpu_ctx)
    try:
        ex = grid.explain_credit_sub_books(trades, spreads, keys, buckets, dz)
        assert all(ex[k].shape == (5, 19) for k in ("full", "delta_pnl", "gamma_pnl", "unexplained"))
        assert C.same_bits(ex["full"], grid.pnl_credit_sub_books(trades, spreads, keys, buckets, dz))
        assert C.same_bits(ex["unexplained"], ex["full"] - (ex["delta_pnl"] + ex["gamma_pnl"]))
        X.check_orders(ex["labels"], ex["full"], ex["delta_pnl"], ex["gamma_pnl"], f"device, {interp.name}",
                       X.EXPLAIN_DROPPED.get(interp.name, ()))
        dg = grid.pnl_credit_delta_gamma_sub_books(trades, spreads, keys, buckets, dz)
        assert C.same_bits(dg["pnl"], ex["delta_pnl"] + ex["gamma_pnl"]) and "delta_pnl" not in dg
        for level in (0.99, 0.75):
            chained = grid.sub_book_credit_delta_gamma_var_es(trades, spreads, keys, buckets, dz, level)
            var, es = tail_measures(dg["pnl"], level, ctx=gpu_ctx)
            assert chained["labels"] == dg["labels"]
            assert C.same_bits(chained["var"], var) and C.same_bits(chained["es"], es), level
        one = grid.pnl_credit_delta_gamma(trades, spreads, buckets, dz)
        whole = grid.pnl_credit_delta_gamma_sub_books(trades, spreads, ["all"] * len(trades), buckets, dz)
        assert one.shape == (19,) and C.same_bits(one, whole["pnl"][0])
    finally:
        grid.close()
