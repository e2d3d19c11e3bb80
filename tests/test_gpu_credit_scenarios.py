"""Credit scenario revaluation on the GPU (csrc/credit_scenario_pv.hip): the C oracle on rescaled batches and the host
twin on the books of tests/_credit_scenario_cases.py, the reduction to adr_scenario_pv, launch shapes bit for bit against
scenarios priced alone through the device-array entry into guarded buffers, the global-table fallback, trades that
cannot be read, the host-array entry's refusals, and `ScenarioGrid.revalue_credit` / `pnl_credit` with the book
wrappers."""
import numpy as np
import pytest
import torch

from adrates_amd import _native
from adrates_amd.market.position.bond_book import BondBook
from adrates_amd.market.position.frn_book import FRNBook
from adrates_amd.market.position.scenarios import (ScenarioGrid, compile_credit_book, revalue_credit_on_curves,
                                                   revalue_on_curves, shocked_spreads)
from adrates_amd.utils import CurveTypes, InterpTypes
from adrates_amd.utils.error import LibError

from . import _credit_scenario_cases as CC
from . import _fixtures as F
from . import _scenario_cases as SC
from ._parity import REL_TOL, unit_notional_err

pytestmark = pytest.mark.gpu
VD = SC.VD
BP = CC.BP
GUARD = -1.2345e300
LZR = InterpTypes.LINEAR_ZERO_RATES.value


@pytest.fixture(scope="module")
def curves():
    return SC.shocked_curves()


@pytest.mark.parametrize("G", CC.BUCKET_COUNTS)
@pytest.mark.parametrize("scheme", SC.SCHEMES, ids=lambda s: s.name)
def test_device_matches_c_oracle_and_host_twin(gpu_ctx, curves, scheme, G):
    """Six books x eight (curve, spread shock) pairs per scheme and bucket count, each trade on its own notional.
    Observed maxima: against the oracle 2.6e-15, against the host twin 2.4e-15 per unit notional."""
    times, dfs = curves
    dz = CC.spread_shocks(dfs.shape[0], G)
    for name, case in CC.cases(G).items():
        got = CC.device_pv(gpu_ctx, scheme.value, times, dfs, dz, case)
        host = CC.host_pv(scheme.value, times, dfs, dz, case)
        e_oracle = SC.worst_unit_err(got["pv"], CC.oracle_pv(scheme.value, times, dfs, dz, case), case.batch)
        e_host = SC.worst_unit_err(got["pv"], host["pv"], case.batch)
        print(f"{scheme.name}, G = {G}, {name}: oracle {e_oracle:.2e}, host twin {e_host:.2e}")
        assert e_oracle <= REL_TOL and e_host <= REL_TOL, (name, e_oracle, e_host)
        assert np.array_equal(got["book_pv"], SC.book_sum(got["pv"]))              # the documented order, bit for bit
        assert np.max(np.abs(got["book_pv"] - host["book_pv"])) <= REL_TOL * np.sum(np.abs(case.batch.notional))


@pytest.mark.parametrize("scheme", SC.SCHEMES, ids=lambda s: s.name)
def test_no_spread_reduces_to_scenario_pv_on_the_device(gpu_ctx, curves, scheme):
    """All z = 0 and no buckets, G = 0 and dz = NULL: adr_scenario_pv's results on the same uploaded batch."""
    times, dfs = curves
    for name, batch in SC.books().items():
        n = batch.n_trades
        dev = _native.DeviceTrades(gpu_ctx, batch)
        try:
            got = _native.credit_scenario_pv(gpu_ctx, scheme.value, times, dfs, None, dev, np.zeros(n), np.full(n, -1),
                                             batch.fix_tp, batch.flt_tp, per_trade=True)
            ref = _native.scenario_pv(gpu_ctx, scheme.value, times, dfs, dev, per_trade=True)
        finally:
            dev.close()
        err = SC.worst_unit_err(got["pv"], ref["pv"], batch)
        print(f"{scheme.name}, {name}: against adr_scenario_pv {err:.2e}, bit for bit {np.array_equal(got['pv'], ref['pv'])}")
        assert err <= REL_TOL
        assert np.max(np.abs(got["book_pv"] - ref["book_pv"])) <= REL_TOL * np.sum(np.abs(batch.notional))


def _objects():
    bonds, _ = F.random_bond_book(VD, 6, seed=11)
    frns, _ = F.random_frn_book(VD, 8, seed=12)
    swaps = [F.make_swap(VD, t, c, nn, pay=p, payment_lag=lag) for t, c, nn, p, lag in
             (("5Y", 0.04, 1e7, True, 0), ("18M", 0.05, 2e6, False, 2), ("30Y", 0.035, 5e6, True, 0))]
    return swaps, bonds, frns


def test_ois_rows_of_a_mixed_book_on_the_device(gpu_ctx, curves):
    times, dfs = curves
    swaps, bonds, frns = _objects()
    mixed = [bonds[0], swaps[0], frns[0], swaps[1], bonds[1], frns[1], swaps[2]]
    spreads = [0.012, 0.0, 0.004, 0.0, -0.002, 0.03, 0.0]
    buckets = ["A", None, "B", None, "A", None, None]
    dz = CC.spread_shocks(8, 2)
    got = revalue_credit_on_curves(LZR, times, dfs, dz, mixed, spreads, buckets, VD, per_trade=True, ctx=gpu_ctx)
    host = revalue_credit_on_curves(LZR, times, dfs, dz, mixed, spreads, buckets, VD, per_trade=True, host=True)
    alone = revalue_on_curves(LZR, times, dfs, swaps, VD, per_trade=True, ctx=gpu_ctx)["pv"]
    rows = got["pv"][:, [1, 3, 6]]
    print("OIS rows of the mixed book bit for bit on the device:", np.array_equal(rows, alone))
    assert unit_notional_err(rows, alone, np.array([s._notional for s in swaps])) <= REL_TOL
    notional = np.array([float(getattr(t, "_face_value", None) or t._notional) for t in mixed])
    assert unit_notional_err(got["pv"], host["pv"], notional[None, :]) <= REL_TOL


class _Dev:
    """One case's arrays on the device, for adr_credit_scenario_pv_dev."""

    def __init__(self, ctx, case, times):
        self.ctx, self.case = ctx, case
        self.dev = torch.device("cuda", 0)
        up = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev, dt)
        self.trades = _native.DeviceTrades(ctx, case.batch)
        self.times = up(times)
        self.z, self.bucket = up(case.z), up(case.bucket, torch.int32)
        self.fix_tau, self.flt_tau = up(case.fix_tau), up(case.flt_tau)
        self.n = case.batch.n_trades

    def run(self, method, dfs, dz, S, per_trade, n_fix=None, n_flt=None, bucket=None, stream=0):
        """Into guarded buffers; returns (book [S], pv [n, S] or None) and checks the words behind the outputs."""
        n = self.n
        up = lambda a: torch.from_numpy(np.ascontiguousarray(np.atleast_2d(a))).to(self.dev)
        dfs_t = up(dfs)
        dz_t = None if dz is None else up(dz)
        book = torch.full((S + 8,), GUARD, dtype=torch.float64, device=self.dev)
        pv = torch.full((n * S + 8,), GUARD, dtype=torch.float64, device=self.dev)
        work = torch.empty(_native.credit_scenario_pv_work(n, S), dtype=torch.float64, device=self.dev)
        ptrs = dict(times=self.times.data_ptr(), dfs=dfs_t.data_ptr(), dz=0 if dz_t is None else dz_t.data_ptr(),
                    z=self.z.data_ptr(), bucket=(self.bucket if bucket is None else bucket).data_ptr(),
                    fix_tau=self.fix_tau.data_ptr() if self.fix_tau.numel() else 0,
                    flt_tau=self.flt_tau.data_ptr() if self.flt_tau.numel() else 0)
        _native.credit_scenario_pv_dev(self.ctx, method, self.times.numel(), dfs_t.shape[0], 0 if dz_t is None else dz_t.shape[1],
                                       1 if dz_t is None else dz_t.shape[0], S, self.trades,
                                       self.fix_tau.numel() if n_fix is None else n_fix,
                                       self.flt_tau.numel() if n_flt is None else n_flt, ptrs, book.data_ptr(), work.data_ptr(),
                                       pv.data_ptr() if per_trade else 0, stream)
        torch.cuda.synchronize()
        assert torch.all(book[S:] == GUARD)
        assert torch.all(pv[n * S:] == GUARD) if per_trade else torch.all(pv == GUARD)       # not requested: untouched
        return book[:S].cpu().numpy(), (pv[:n * S].reshape(n, S).cpu().numpy() if per_trade else None)

    def close(self):
        self.trades.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_launch_shapes_bit_for_bit(gpu_ctx, curves, n):
    """n across the chunk of 64, S in {1, 63, 64, 65, 130}: every row equals the row of the same scenario priced alone,
    with a shared row or with S copies of it; the padding lanes of a partial group write nothing."""
    times, dfs = curves
    rng = np.random.default_rng(n)
    mix = rng.uniform(0.0, 1.0, size=(130, dfs.shape[0]))
    rows = np.exp((mix / mix.sum(1, keepdims=True)) @ np.log(dfs))
    bonds, _ = F.random_bond_book(VD, (n + 1) // 2, seed=n)
    frns, _ = F.random_frn_book(VD, n // 2, seed=n + 1) if n > 1 else ([], None)
    book = compile_credit_book(bonds + frns, VD, CurveTypes.GBP_OIS_SONIA, rng.uniform(-50 * BP, 800 * BP, n),
                               [None if i % 5 == 0 else i % 7 for i in range(n)])
    case = CC.Case(book.batch, book.z, book.bucket, book.fix_tau, book.flt_tau)
    G = len(book.labels)
    dz = rng.uniform(-300 * BP, 300 * BP, (130, max(G, 1)))[:, :G]
    d = _Dev(gpu_ctx, case, times)
    try:
        alone = {s: d.run(LZR, rows[s], dz[s] if G else None, 1, True) for s in (0, 62, 63, 64, 129)}
        for S in (1, 63, 64, 65, 130):
            bk, pv = d.run(LZR, rows[:S], dz[:S] if G else None, S, True)
            bk_only, _ = d.run(LZR, rows[:S], dz[:S] if G else None, S, False)
            assert np.array_equal(bk, bk_only) and np.array_equal(bk, SC.book_sum(pv.T))
            for s, (b1, p1) in alone.items():
                if s < S:
                    assert np.array_equal(pv[:, s], p1[:, 0]) and bk[s] == b1[0], (S, s)
        # broadcasting: a shared row against S copies of it, on either side
        S = 65
        a = d.run(LZR, rows[3], dz[:S] if G else None, S, True)
        b = d.run(LZR, np.repeat(rows[3:4], S, axis=0), dz[:S] if G else None, S, True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        if G:
            a = d.run(LZR, rows[:S], dz[7], S, True)
            b = d.run(LZR, rows[:S], np.repeat(dz[7:8], S, axis=0), S, True)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        again = d.run(LZR, rows[:S], dz[:S] if G else None, S, True)
        assert np.array_equal(again[1], pv[:, :S]) and np.array_equal(again[0], bk[:S])                # run to run
        host = CC.host_pv(LZR, times, rows[:65], dz[:65] if G else None, case)
        assert SC.worst_unit_err(pv.T[:65], host["pv"], case.batch) <= REL_TOL
    finally:
        d.close()


@pytest.mark.parametrize("scheme", [InterpTypes.LINEAR_ZERO_RATES, InterpTypes.LINEAR_FWD_RATES], ids=lambda s: s.name)
def test_global_table_fallback(gpu_ctx, scheme):
    """K = 856 with G = 32: 8 (65 K + 64 G) bytes exceed the LDS budget (K <= 283 fits with 32 buckets), so the spread
    table stays in LDS and the lanes read their discount rows from global memory."""
    times, dfs, dz, case = CC.large_grid_call(S=8)
    got = CC.device_pv(gpu_ctx, scheme.value, times, dfs, dz, case)
    err = SC.worst_unit_err(got["pv"], CC.oracle_pv(scheme.value, times, dfs, dz, case), case.batch)
    e_host = SC.worst_unit_err(got["pv"], CC.host_pv(scheme.value, times, dfs, dz, case)["pv"], case.batch)
    print(f"K = {times.size}, G = 32, {scheme.name}: oracle {err:.2e}, host twin {e_host:.2e}")
    assert times.size == 856 and err <= REL_TOL and e_host <= REL_TOL
    assert np.array_equal(got["book_pv"], SC.book_sum(got["pv"]))


def test_trades_that_cannot_be_read_get_nan_and_nothing_else_moves(gpu_ctx, curves):
    """Through the device-array entry, which checks scalars only: a trade whose flows end beyond the spread-time
    arrays' counts, or whose bucket is outside -1 .. G - 1, reads nothing and gets a NaN PV; every other trade keeps
    its bits.  The arrays themselves are full-sized: nothing is read out of bounds either way."""
    times, dfs = curves
    G = 5
    case = CC.cases(G)["50 FRNs"]
    dz = CC.spread_shocks(8, G)
    d = _Dev(gpu_ctx, case, times)
    try:
        n = d.n
        _, good = d.run(LZR, dfs, dz, 8, True)
        assert np.all(np.isfinite(good))
        short_fix = int(case.batch.fix_off[n - 3])                   # the last three trades' fixed flows do not fit
        bk, pv = d.run(LZR, dfs, dz, 8, True, n_fix=short_fix)
        cut = np.asarray(case.batch.fix_off[1:]) > short_fix
        assert cut.sum() == 3 and np.all(np.isnan(pv[cut])) and np.array_equal(pv[~cut], good[~cut])
        assert np.all(np.isnan(bk))                                  # the NaN carries into the book
        short_flt = int(case.batch.flt_off[10])
        _, pv = d.run(LZR, dfs, dz, 8, True, n_flt=short_flt)
        cut = np.asarray(case.batch.flt_off[1:]) > short_flt
        assert np.all(np.isnan(pv[cut])) and np.array_equal(pv[~cut], good[~cut])
        bad = case.bucket.copy()
        bad[4], bad[20] = G, -2
        _, pv = d.run(LZR, dfs, dz, 8, True, bucket=torch.from_numpy(bad).to(d.dev))
        keep = np.ones(n, dtype=bool)
        keep[[4, 20]] = False
        assert np.all(np.isnan(pv[~keep])) and np.array_equal(pv[keep], good[keep])
        with pytest.raises(LibError, match="work is NULL"):
            _native.credit_scenario_pv_dev(gpu_ctx, LZR, times.size, 8, G, 8, 8, d.trades, 0, 0, dict(times=1, dfs=1, dz=1, z=1, bucket=1),
                                           1, 0)
        with pytest.raises(LibError, match="buckets"):
            _native.credit_scenario_pv_dev(gpu_ctx, LZR, times.size, 8, 33, 8, 8, d.trades, 0, 0, dict(times=1, dfs=1, dz=1, z=1, bucket=1),
                                           1, 1)
        with pytest.raises(LibError, match="1 .a shared row. or S"):
            _native.credit_scenario_pv_dev(gpu_ctx, LZR, times.size, 3, G, 8, 8, d.trades, 0, 0, dict(times=1, dfs=1, dz=1, z=1, bucket=1),
                                           1, 1)
    finally:
        d.close()


def test_the_host_array_entry_refuses_what_it_can_read(gpu_ctx):
    times, dfs, dz, case, bad = CC.refusal_inputs()
    dev = _native.DeviceTrades(gpu_ctx, case.batch)
    base = dict(dfs=dfs, dz=dz, z=case.z, bucket=case.bucket, fix_tau=case.fix_tau, flt_tau=case.flt_tau)
    call = lambda kw: _native.credit_scenario_pv(gpu_ctx, LZR, times, kw["dfs"], kw["dz"], dev, kw["z"], kw["bucket"],
                                                 kw["fix_tau"], kw["flt_tau"])
    try:
        assert np.all(np.isfinite(call(base)["book_pv"]))
        for what, mutate in bad:
            kw = dict(base)
            mutate(kw)
            with pytest.raises(LibError):
                call(kw)
                pytest.fail(f"{what} was accepted")
        with pytest.raises(LibError, match="shared row"):
            _native.credit_scenario_pv(gpu_ctx, LZR, times, dfs[:3], dz, dev, case.z, case.bucket, case.fix_tau, case.flt_tau)
        # the C entry itself, with counts the wrapper would not pass
        lib, p = _native.load(), _native._ptr
        book = np.empty(4)
        z, bucket = np.ascontiguousarray(case.z), np.ascontiguousarray(case.bucket, dtype=np.int32)
        raw = lambda S_disc, S_spr, S: lib.adr_credit_scenario_pv(
            gpu_ctx._h, LZR, times.size, p(times), S_disc, p(dfs), dz.shape[1], S_spr, p(dz), S, dev._h, p(z), p(bucket, _native._i32p),
            case.fix_tau.size, p(case.fix_tau), case.flt_tau.size, p(case.flt_tau), None, p(book))
        assert raw(4, 4, 4) == 0 and raw(1, 1, 4) == 0
        assert raw(2, 4, 4) < 0 and raw(4, 3, 4) < 0
    finally:
        dev.close()


def test_grid_revalue_credit_pnl_and_the_book_wrappers(gpu_ctx):
    """`ScenarioGrid.revalue_credit` on the grid's device-resident curves against the host twin on the downloaded ones;
    `pnl_credit` of a zero curve shock with a zero spread shock is exactly 0; `BondBook.revalue` and `FRNBook.revalue`
    are the same call.  The gap between the market value and the PV at `measures()`' z is printed, not asserted
    (measures solves z on the curve's own nodes with ACT/ACT times)."""
    model = F.gbp_model(VD)
    swaps, _, _ = _objects()
    bonds, _ = F.random_bond_book(VD, 40, seed=4)
    frns, _ = F.random_frn_book(VD, 40, seed=5)
    shocks = [0.0, 0.01, -0.5, 2.0, {"5Y": 0.25}, 0.0]
    grid = ScenarioGrid(model, "GBP_OIS_SONIA", shocks, with_gamma=False, ctx=gpu_ctx)
    try:
        bb, fb = BondBook(bonds, model), FRNBook(frns, model)
        rng = np.random.default_rng(1)
        mb = bb.measures(clean_prices=rng.uniform(85.0, 115.0, len(bonds)), ctx=gpu_ctx)
        mf = fb.measures(clean_prices=rng.uniform(97.0, 103.0, len(frns)), ctx=gpu_ctx)
        ok_b, ok_f = mb["status"] < 2, mf["status"] < 2
        z = np.where(ok_b, mb["z"], 0.01)
        dm = np.where(ok_f, mf["dm"], 0.002)
        trades = bonds + swaps + frns
        spreads = np.concatenate([z, np.zeros(len(swaps)), dm])
        buckets = [f"issuer {i % 6}" for i in range(len(bonds))] + [None] * len(swaps) + [f"bank {i % 3}" if i % 4 else None for i in range(len(frns))]
        labels = compile_credit_book(trades, VD, CurveTypes.GBP_OIS_SONIA, spreads, buckets).labels
        dz = np.stack([shocked_spreads(labels, s) for s in (0.0, 10.0, {"issuer 2": 150.0}, -25.0, {"bank 1": 40.0, "issuer 0": -40.0}, 100.0)])
        got = grid.revalue_credit(trades, spreads, buckets, dz, per_trade=True)
        want = revalue_credit_on_curves(LZR, grid.base.times, grid._dfs(), dz, trades, spreads, buckets, VD, per_trade=True, host=True)
        notional = np.array([float(getattr(t, "_face_value", None) or t._notional) for t in trades])
        err = unit_notional_err(got["pv"], want["pv"], notional[None, :])
        print(f"revalue_credit against the host twin: {err:.2e}")
        assert got["labels"] == labels and got["pv"].shape == (6, len(trades)) and err <= REL_TOL
        assert np.array_equal(grid.revalue_credit(trades, spreads, buckets, dz)["book_pv"], got["book_pv"])
        # the set's curves read in place against the same rows uploaded from the host: the same bits
        up = revalue_credit_on_curves(LZR, grid.base.times, grid._dfs(), dz, trades, spreads, buckets, VD, per_trade=True, ctx=gpu_ctx)
        assert np.array_equal(up["pv"], got["pv"]) and np.array_equal(up["book_pv"], got["book_pv"])
        pnl = grid.pnl_credit(trades, spreads, buckets, dz)
        print(f"pnl_credit of the zero pair: {pnl[0]!r}")
        assert pnl.shape == (6,) and pnl[0] == 0.0
        assert pnl[5] < 0.0                                           # +100 bp of spread on an unshocked curve: a loss
        assert np.allclose(pnl[1:], got["book_pv"][1:] - got["book_pv"][0], rtol=0, atol=1e-10 * np.sum(notional))
        assert np.all(grid.pnl_credit(trades, spreads, buckets)[[0, 5]] == 0.0)      # no spread shocks at all
        shared = grid.pnl_credit(trades, spreads, buckets, dz[5])                  # one row for every scenario
        assert shared[0] == pnl[5]
        # the wrappers
        bz = bb.revalue(grid, z, buckets[:len(bonds)], dz[:, :6], per_trade=True)
        assert np.array_equal(bz["pv"], got["pv"][:, :len(bonds)])
        fz = fb.revalue(grid, dm, per_trade=True)
        assert fz["pv"].shape == (6, len(frns)) and fz["labels"] == []
        with pytest.raises(LibError, match="spread-shock rows"):
            grid.revalue_credit(trades, spreads, buckets, dz[:4])
        with pytest.raises(LibError, match="one column per bucket"):
            grid.revalue_credit(trades, spreads, buckets, dz[:, :3])
        # recorded, not asserted: the PV at measures()' spread against the market value it was solved from
        # (bullet bonds only: the engine's bond route pays the whole face at maturity, `compile_bonds`, so an amortizer's
        # z from `measures`, which follows its repayment schedule, belongs to other cash flows)
        ok_b = ok_b & np.array([np.count_nonzero(np.asarray(b._principal_payments, dtype=np.float64)) <= 1 for b in bonds])
        base_b = bz["pv"][0][ok_b] / np.array([b._face_value for b in bonds])[ok_b] * 100.0
        gap_b = np.max(np.abs(base_b - mb["dirty"][ok_b]))
        base_f = fz["pv"][0][ok_f] / np.array([f._face_value for f in frns])[ok_f] * 100.0
        gap_f = np.max(np.abs(base_f - mf["dirty"][ok_f]))
        print(f"gap to the dirty price per 100 at measures()' spread: bonds {gap_b:.3e}, FRNs {gap_f:.3e}")
    finally:
        grid.close()
