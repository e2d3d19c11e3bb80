"""Scenario revaluation on the GPU (csrc/scenario_pv.hip): the C oracle and the host twin on the books of
tests/_scenario_cases.py, launch shapes (partial scenario groups, short and long batches) bit for bit against scenarios
priced alone, `ScenarioGrid.revalue` / `pnl` against the per-scenario loop, the device-array entry on a caller's stream
and inside a HIP graph, and a knot grid too large for the LDS table."""
import subprocess
import sys

import numpy as np
import pytest
import torch

from adrates_amd import _native
from adrates_amd.market.curves.curve_tables import build_engine_curve
from adrates_amd.market.position.scenarios import ScenarioGrid
from adrates_amd.trades import synthetic
from adrates_amd.trades.credit.frn import FRN
from adrates_amd.utils import CurrencyTypes, CurveTypes, DayCountTypes, FrequencyTypes, InterpTypes, RequestTypes
from adrates_amd.utils.error import LibError

from . import _fixtures as F
from . import _scenario_cases as SC
from ._parity import REL_TOL, unit_notional_err

pytestmark = pytest.mark.gpu
VD = SC.VD
GUARD = -1.2345e300


@pytest.fixture(scope="module")
def curves():
    return SC.shocked_curves()


@pytest.fixture(scope="module")
def books():
    return SC.books()


@pytest.mark.parametrize("scheme", SC.SCHEMES, ids=lambda s: s.name)
def test_device_matches_c_oracle_and_host_twin(gpu_ctx, curves, books, scheme):
    """Observed: against the oracle 2.6e-15, against the host twin 2.3e-15 per unit notional."""
    times, dfs = curves
    for name, batch in books.items():
        dev = _native.DeviceTrades(gpu_ctx, batch)
        try:
            got = _native.scenario_pv(gpu_ctx, scheme.value, times, dfs, dev, per_trade=True)
        finally:
            dev.close()
        host = _native.scenario_pv_host(scheme.value, times, dfs, batch, per_trade=True)
        e_oracle = SC.worst_unit_err(got["pv"], SC.oracle_pv(scheme.value, times, dfs, batch), batch)
        e_host = SC.worst_unit_err(got["pv"], host["pv"], batch)
        print(f"{scheme.name}, {name}: oracle {e_oracle:.2e}, host twin {e_host:.2e}")
        assert e_oracle <= REL_TOL and e_host <= REL_TOL, (name, e_oracle, e_host)
        assert np.array_equal(got["book_pv"], SC.book_sum(got["pv"]))              # the documented order, bit for bit
        scale = np.sum(np.abs(batch.notional))
        assert np.max(np.abs(got["book_pv"] - host["book_pv"])) <= REL_TOL * scale


@pytest.mark.parametrize("scheme", [InterpTypes.LINEAR_ZERO_RATES, InterpTypes.LINEAR_FWD_RATES], ids=lambda s: s.name)
def test_lookup_rule_on_the_device(gpu_ctx, scheme):
    from oracle import cavour_oracle as O
    times = SC.LOOKUP_TIMES
    dfs = SC.lookup_curves(times)
    dev = _native.DeviceTrades(gpu_ctx, SC.one_flow_book(SC.LOOKUP_DATES))
    got = _native.scenario_pv(gpu_ctx, scheme.value, times, dfs, dev, per_trade=True)["pv"]
    dev.close()
    live = SC.LOOKUP_DATES > 0.0
    for s in range(dfs.shape[0]):
        ref = np.asarray(O.simple_interpolate(SC.LOOKUP_DATES, times, dfs[s], scheme.value), dtype=np.float64).reshape(-1)
        assert np.max(np.abs(got[s] - ref)[live]) <= REL_TOL


def _run_dev(ctx, method, times_t, dfs_t, trades, n, S, per_trade, stream=0):
    """adr_scenario_pv_dev into guarded buffers; returns (book [S], pv [n, S] or None) as numpy."""
    dev = dfs_t.device
    book = torch.full((S + 8,), GUARD, dtype=torch.float64, device=dev)
    pv = torch.full((n * S + 8,), GUARD, dtype=torch.float64, device=dev) if per_trade else None
    work = torch.empty(_native.scenario_pv_work(n, S), dtype=torch.float64, device=dev)
    _native.scenario_pv_dev(ctx, method, times_t.numel(), times_t.data_ptr(), S, dfs_t.data_ptr(), trades, book.data_ptr(),
                            work.data_ptr(), pv.data_ptr() if per_trade else 0, stream)
    torch.cuda.synchronize()
    assert torch.all(book[S:] == GUARD)
    if per_trade:
        assert torch.all(pv[n * S:] == GUARD)
    return book[:S].cpu().numpy(), (pv[:n * S].reshape(n, S).cpu().numpy() if per_trade else None)


@pytest.mark.parametrize("n", [1, 63, 4097])
def test_launch_shapes_bit_for_bit(gpu_ctx, curves, n):
    """S in {1, 63, 64, 65, 130}: every row equals the row of the same scenario priced alone; the padding lanes of a
    partial group write nothing (guard words behind the outputs keep their pattern)."""
    times, dfs = curves
    rng = np.random.default_rng(n)
    mix = rng.uniform(0.0, 1.0, size=(130, dfs.shape[0]))
    rows = np.exp((mix / mix.sum(1, keepdims=True)) @ np.log(dfs))                # 130 distinct curves between the shocks
    batch = synthetic.synthesize(VD, n, seed=40 + n)
    trades = _native.DeviceTrades(gpu_ctx, batch)
    dev = torch.device("cuda", 0)
    times_t = torch.from_numpy(times).to(dev)
    alone = {}
    for s in (0, 62, 63, 64, 129):
        row_t = torch.from_numpy(rows[s:s + 1].copy()).to(dev)
        alone[s] = _run_dev(gpu_ctx, 4, times_t, row_t, trades, n, 1, True)
    for S in (1, 63, 64, 65, 130):
        dfs_t = torch.from_numpy(rows[:S].copy()).to(dev)
        book, pv = _run_dev(gpu_ctx, 4, times_t, dfs_t, trades, n, S, True)
        book_only, _ = _run_dev(gpu_ctx, 4, times_t, dfs_t, trades, n, S, False)
        assert np.array_equal(book, book_only)
        assert np.array_equal(book, SC.book_sum(pv.T))
        for s, (b1, p1) in alone.items():
            if s < S:
                assert np.array_equal(pv[:, s], p1[:, 0]) and book[s] == b1[0], (S, s)
    host = _native.scenario_pv_host(4, times, rows[:65], batch, per_trade=True)
    assert SC.worst_unit_err(pv.T[:65], host["pv"], batch) <= REL_TOL
    trades.close()


def test_grid_revalue_against_the_per_scenario_loop(gpu_ctx):
    """2 000 swaps x 9 scenarios: one launch against `ScenarioGrid.price` (the lite / fast kernel family, one launch
    per scenario).  The device builder reproduces the host builder's discount factors bit for bit
    (tests/test_gpu_curve_build.py), so the P&L of a zero shock is exactly 0."""
    model = F.gbp_model(VD)
    rng = np.random.default_rng(8)
    swaps = [F.make_swap(VD, f"{int(m)}M", float(c), float(nn), pay=bool(p), payment_lag=int(lag))
             for m, c, nn, p, lag in zip(rng.integers(1, 361, 2000), rng.uniform(0.01, 0.07, 2000),
                                         np.round(rng.uniform(1e6, 5e7, 2000), -5), rng.random(2000) < 0.5,
                                         rng.choice([0, 0, 0, 2], 2000))]
    shocks = [0.0, 0.01, -0.01, 0.5, -0.5, 2.0, -2.0, {"5Y": 0.25}, {"3M": -0.1, "30Y": 0.2}]
    grid = ScenarioGrid(model, "GBP_OIS_SONIA", shocks, with_gamma=False, ctx=gpu_ctx)
    try:
        loop = grid.price(swaps, [RequestTypes.VALUE])["pv"]
        one = grid.revalue(swaps, per_trade=True)
        notional = np.array([s._notional for s in swaps])
        err = max(unit_notional_err(a, b, notional) for a, b in zip(one["pv"], loop))
        print(f"revalue vs the per-scenario loop: {err:.2e}")
        assert one["pv"].shape == loop.shape == (9, 2000) and err <= REL_TOL
        assert np.array_equal(grid.revalue(swaps)["book_pv"], one["book_pv"])
        pnl = grid.pnl(swaps)
        assert pnl.shape == (9,) and abs(pnl[0]) <= REL_TOL * np.sum(notional)
        print(f"pnl of the zero shock: {pnl[0]!r}")
        assert pnl[0] == 0.0                                   # the builder's base curve has the host builder's bits
        assert np.allclose(pnl[1:], one["book_pv"][1:] - one["book_pv"][0], rtol=0, atol=1e-10 * np.sum(notional))
        assert pnl[5] != 0.0 and np.sign(pnl[5]) == -np.sign(pnl[6])
        # a mixed book in one batch, and the refusals
        bonds, _ = F.random_bond_book(VD, 3, seed=2)
        frns, _ = F.random_frn_book(VD, 3, seed=3)
        mixed = [swaps[0], bonds[0], frns[0], frns[1], swaps[1], bonds[1]]
        got = grid.revalue(mixed, per_trade=True)["pv"]
        ref = InterpTypes.LINEAR_ZERO_RATES.value
        from adrates_amd.market.position.scenarios import revalue_on_curves
        want = revalue_on_curves(ref, grid.base.times, grid._dfs(), mixed, VD, per_trade=True, host=True)["pv"]
        assert np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))) <= 1e-10
        dual = FRN(VD, "2Y", 0.001, FrequencyTypes.QUARTERLY, DayCountTypes.ACT_360, CurrencyTypes.GBP, CurveTypes.USD_OIS_SOFR)
        with pytest.raises(LibError, match="dual-curve FRN"):
            grid.revalue([swaps[0], dual])
        usd = F.make_swap(VD, "5Y", 0.04, 1e6, index=CurveTypes.USD_OIS_SOFR, ccy=CurrencyTypes.USD)
        with pytest.raises(LibError, match="not on the grid's curve"):
            grid.pnl([usd])
        from adrates_amd.trades.rates.xccy_basis_swap import XccyBasisSwap
        xccy = XccyBasisSwap(effective_dt=VD, term_dt_or_tenor="7Y", domestic_notional=7_900_000, foreign_notional=10_000_000,
                             domestic_spread=0.0, foreign_spread=0.0040, domestic_freq_type=FrequencyTypes.ANNUAL,
                             foreign_freq_type=FrequencyTypes.SEMI_ANNUAL, domestic_dc_type=DayCountTypes.ACT_365F,
                             foreign_dc_type=DayCountTypes.ACT_360, domestic_floating_index=CurveTypes.GBP_OIS_SONIA,
                             foreign_floating_index=CurveTypes.USD_OIS_SOFR, domestic_currency=CurrencyTypes.GBP,
                             foreign_currency=CurrencyTypes.USD)
        with pytest.raises(LibError, match="cross-currency"):
            grid.revalue([xccy])
        with pytest.raises(LibError):
            _native.scenario_pv(gpu_ctx, 4, grid.base.times, grid._dfs()[:, :-1], None)
    finally:
        grid.close()


def test_run_to_run_bits_and_callers_stream(gpu_ctx, curves, books):
    times, dfs = curves
    batch = books["payment lag"]
    trades = _native.DeviceTrades(gpu_ctx, batch)
    n, S = batch.n_trades, dfs.shape[0]
    dev = torch.device("cuda", 0)
    times_t, dfs_t = torch.from_numpy(times).to(dev), torch.from_numpy(dfs).to(dev)
    first = _native.scenario_pv(gpu_ctx, 1, times, dfs, trades, per_trade=True)
    again = _native.scenario_pv(gpu_ctx, 1, times, dfs, trades, per_trade=True)
    assert np.array_equal(first["pv"], again["pv"]) and np.array_equal(first["book_pv"], again["book_pv"])
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        book, pv = _run_dev(gpu_ctx, 1, times_t, dfs_t, trades, n, S, True, stream.cuda_stream)
    assert np.array_equal(pv.T, first["pv"]) and np.array_equal(book, first["book_pv"])
    with pytest.raises(LibError, match="work is NULL"):
        _native.scenario_pv_dev(gpu_ctx, 1, times.size, times_t.data_ptr(), S, dfs_t.data_ptr(), trades, dfs_t.data_ptr(), 0)
    with pytest.raises(LibError, match="knots"):
        _native.scenario_pv_dev(gpu_ctx, 1, 5000, times_t.data_ptr(), S, dfs_t.data_ptr(), trades, dfs_t.data_ptr(), 1)
    trades.close()


_GRAPH_CHILD = r"""
import numpy as np, torch
from adrates_amd import _native
from adrates_amd.trades import synthetic
from tests import _scenario_cases as SC
times, dfs = SC.shocked_curves()
ctx = _native.default_context(0)
n, S = 700, dfs.shape[0]
trades = _native.DeviceTrades(ctx, synthetic.synthesize(SC.VD, n, seed=5))
dev = torch.device("cuda", 0)
t, d = torch.from_numpy(times).to(dev), torch.from_numpy(dfs).to(dev)
book = torch.zeros(S, dtype=torch.float64, device=dev)
pv = torch.zeros((n, S), dtype=torch.float64, device=dev)
work = torch.empty(_native.scenario_pv_work(n, S), dtype=torch.float64, device=dev)
stream = torch.cuda.Stream(dev)
launch = lambda: _native.scenario_pv_dev(ctx, 4, times.size, t.data_ptr(), S, d.data_ptr(), trades, book.data_ptr(),
                                         work.data_ptr(), pv.data_ptr(), stream.cuda_stream)
with torch.cuda.stream(stream):
    launch()
    stream.synchronize()
    eager = (book.clone(), pv.clone())
    book.zero_(); pv.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        launch()
    graph.replay()
    stream.synchronize()
assert torch.equal(book, eager[0]) and torch.equal(pv, eager[1]) and float(pv.abs().max()) > 0.0
print("graph replay ok")
"""


def test_dev_entry_can_be_captured_into_a_hip_graph():
    """adr_scenario_pv_dev neither allocates nor synchronises: its two kernels, one chain, captured on a stream and
    replayed give the eager launch's bits.  In a child process, so that a failed capture cannot poison this one."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _GRAPH_CHILD], cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "graph replay ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("scheme", [InterpTypes.LINEAR_ZERO_RATES, InterpTypes.LINEAR_FWD_RATES], ids=lambda s: s.name)
def test_knot_grid_beyond_the_lds_table(gpu_ctx, scheme):
    """K > 315 knots: 64 scenarios x K doubles no longer fit the LDS next to the knot times; the lanes read their
    scenario's row from global memory.  The weekly-short-end curve of tests/test_gpu_many_pillars.py, 64 scenarios."""
    from .test_gpu_many_pillars import weekly_pillar_quotes
    px, tenors = weekly_pillar_quotes(100)
    curve = F.gbp_model(VD, scheme, px=px, tenors=tenors).curves.GBP_OIS_SONIA
    rates = np.array(curve.swap_rates)
    rng = np.random.default_rng(3)
    rows = [build_engine_curve(list(rates + rng.uniform(-50, 50) * 1e-4 + rng.uniform(-5, 5, rates.size) * 1e-4),
                               curve.swap_times, curve.year_fracs, with_hessian=False) for _ in range(8)]
    times = rows[0].times
    assert times.size > 320
    mix = rng.uniform(0.0, 1.0, size=(64, 8))
    dfs = np.exp((mix / mix.sum(1, keepdims=True)) @ np.log(np.stack([r.dfs for r in rows])))
    batch = SC.lag_book(300, seed=31)
    trades = _native.DeviceTrades(gpu_ctx, batch)
    got = _native.scenario_pv(gpu_ctx, scheme.value, times, dfs, trades, per_trade=True)
    trades.close()
    err = SC.worst_unit_err(got["pv"], SC.oracle_pv(scheme.value, times, dfs, batch), batch)
    print(f"K = {times.size}, {scheme.name}: {err:.2e}")
    assert err <= REL_TOL
    assert np.array_equal(got["book_pv"], SC.book_sum(got["pv"]))
