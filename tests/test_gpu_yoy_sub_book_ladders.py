"""Inflation sub-book Greeks on the GPU (adr_yoy_subbook_ladders*): the desks' augmented ladders of one launch chain against
the torch oracle, the host twin, the desks priced alone (bit for bit), the non-blocking entry on caller buffers, and the
delta-gamma P&L they give against full revaluation under joint (discount, breakeven) shocks.

Observed on an MI355X (bound 1e-10 of a desk's sum of absolute per-swap entries; oracle / host twin): geometry book 2.4e-15 /
2.8e-15 over the six scheme pairs, edge book 1.1e-15 / 4.3e-16, shapes 1.2e-14 / 1.7e-15, 600 one-swap desks 1.2e-14 / 4.3e-15;
residual ratios under joint shocks 7.606 - 8.066 with the cross block, 3.967 - 4.012 without it."""
import numpy as np
import pytest
import torch

from adrates_amd import _native
from adrates_amd.market.position.scenarios import ScenarioGrid, tail_measures
from adrates_amd.utils.error import LibError
from adrates_amd.utils.global_types import RequestTypes

from . import _ladder_pnl_cases as C
from . import _sub_book_ladder_cases as L
from . import _yoy_cases as YC
from . import _yoy_ladder_cases as Y
from .test_gpu_parity_batch import _device_curve

pytestmark = pytest.mark.gpu


def _entries(ctx, interp, P=32):
    curve, host = Y.disc_curve(interp, P)
    host2, dc = _device_curve(ctx, curve)
    assert np.array_equal(host2.dfs, host.dfs)
    return host, dc, Y.Entries(interp.value, host, ctx, dc), Y.Entries(interp.value, host)


def check_book(E, twin_of, interp, infl, book, sub_off, what, key=None):
    """Device against the oracle's sums and against the host twin, both at 1e-10 of the desk's absolute sums; the layout."""
    ref = Y.reference(interp.value, E.host, infl, book, key)
    got = E(infl, book.fixed, book.coupons, sub_off)
    twin = twin_of(infl, book.fixed, book.coupons, sub_off)
    e_ref, e_twin = L.desk_errors(got, ref, sub_off), Y.between(got, twin, ref, sub_off)
    print(f"{what}: device vs oracle {e_ref:.2e}, device vs host twin {e_twin:.2e}")
    assert e_ref <= Y.TOL and e_twin <= Y.TOL
    Y.check_layout(got, E.host.jac.shape[1], np.asarray(infl[1]).size)
    return got, twin, ref


@pytest.mark.parametrize("im", Y.INFL_SCHEMES)
@pytest.mark.parametrize("interp", Y.SCHEMES)
def test_geometry(gpu_ctx, interp, im):
    """Desks of 1, 63, 64, 0, 65, 129, 0 swaps under the six scheme pairs: the oracle, the host twin, the bit contract (a desk
    alone with B = 1, permuted desks, a second launch, an empty desk +0.0) and the discount block against
    adr_subbook_ladders_host on the equivalent fixed-flow batch - held to 1e-10, the count of differing entries printed: the
    device's LDS adds land in another order than the twin's loop (observed: 2.8e-15 at most; 4-5 of the 7 PVs, 70-79 of the
    224 deltas and 670-789 of the 7 168 gammas differ in their last bits)."""
    host, dc, E, twin_of = _entries(gpu_ctx, interp)
    infl, book, sub_off = Y.infl_curve(12, im), Y.geometry_book(), Y.offsets(Y.GEOMETRY_SIZES)
    got, twin, ref = check_book(E, twin_of, interp, infl, book, sub_off, f"geometry {interp.name} / {YC.NAMES[im]}",
                                ("geometry", interp, im))
    Y.check_contract(E, infl, book, sub_off, got)
    amount = _native.yoy_risk_host((interp.value, host.times, host.dfs), infl, book.coupons, 0)["amount"]
    want = _native.subbook_ladders_host(interp.value, host.times, host.dfs, host.jac, host.hess,
                                        Y.equivalent_batch(book.fixed, book.coupons, amount), sub_off)
    P = 32
    mine = {"pv": got["pv"], "delta": got["delta"][:, :P], "gamma": got["gamma"][:, :P, :P]}
    cut = {k: np.asarray(ref[k])[(slice(None),) + (slice(0, P),) * (np.asarray(ref[k]).ndim - 1)] for k in ("pv", "delta", "gamma")}
    worst = L.rows_errors(mine, want, cut, sub_off)
    differ = {k: int(np.sum(Y.bits(mine[k]) != Y.bits(want[k]))) for k in mine}
    print(f"discount block vs adr_subbook_ladders_host, {interp.name}: {worst:.2e}; entries whose bits differ: {differ}")
    assert worst <= Y.TOL


@pytest.mark.parametrize("interp", Y.SCHEMES)
def test_edge_book(gpu_ctx, interp):
    """The hand-made swaps of `_yoy_ladder_cases.edge_book` in three desks and one desk per swap."""
    host, dc, E, twin_of = _entries(gpu_ctx, interp)
    book, sub_off = Y.edge_book(float(host.times[40]))
    for im in Y.INFL_SCHEMES:
        infl = Y.infl_curve(5, im)
        got, _, ref = check_book(E, twin_of, interp, infl, book, sub_off, f"edge book {interp.name} / {YC.NAMES[im]}")
        Y.check_contract(E, infl, book, sub_off, got)
        each_off = np.arange(book.n + 1)
        each = E(infl, book.fixed, book.coupons, each_off)
        assert L.desk_errors(each, ref, each_off) <= Y.TOL
        dead = [book.names.index(k) for k in ("tp == 0: dead coupon and dead fixed flow", "no coupons, no flows")]
        assert not np.any(each["ladders"][dead]) and not np.any(np.signbit(each["ladders"][dead]))


@pytest.mark.parametrize("P", [17, 32, 40])
@pytest.mark.parametrize("P_i", [1, 12, 64])
def test_shapes(gpu_ctx, P, P_i):
    interp = Y.SCHEMES[(P + P_i) % 3]
    im = Y.INFL_SCHEMES[P_i % 2]
    host, dc, E, twin_of = _entries(gpu_ctx, interp, P)
    assert dc.n_pillars == P
    check_book(E, twin_of, interp, Y.infl_curve(P_i, im), Y.small_book(), Y.offsets(Y.SMALL_SIZES),
               f"P_d = {P}, P_i = {P_i}, {interp.name} / {YC.NAMES[im]}")


def test_requests_leave_blocks_zero(gpu_ctx):
    interp = Y.SCHEMES[1]
    host, dc, E, twin_of = _entries(gpu_ctx, interp)
    infl, book, sub_off = Y.infl_curve(12, YC.FF), Y.small_book(), Y.offsets(Y.SMALL_SIZES)
    ref = Y.reference(interp.value, host, infl, book)
    full = E(infl, book.fixed, book.coupons, sub_off)
    d_only = E(infl, book.fixed, book.coupons, sub_off, want_gamma=False)
    v_only = E(infl, book.fixed, book.coupons, sub_off, want_delta=False, want_gamma=False)
    Y.check_layout(d_only, 32, 12, want_gamma=False)
    Y.check_layout(v_only, 32, 12, want_delta=False, want_gamma=False)
    assert Y.between(d_only, dict(full, gamma=d_only["gamma"]), ref, sub_off) <= Y.TOL
    assert Y.between(v_only, dict(full, delta=v_only["delta"], gamma=v_only["gamma"]), ref, sub_off) <= Y.TOL
    twin = twin_of(infl, book.fixed, book.coupons, sub_off, hess=False, want_gamma=False)
    assert Y.between(d_only, twin, ref, sub_off) <= Y.TOL


def test_more_chunks_than_waves(gpu_ctx):
    """600 desks of one swap on a 64-pillar inflation curve: a wave's tables take 90 632 bytes (Kc = 107), so a block has one
    wave, a compute unit one block and the grid at most 256 waves - fewer than the 600 chunks, so waves take further chunks."""
    interp = Y.SCHEMES[0]
    host, dc, E, twin_of = _entries(gpu_ctx, interp)
    swaps = YC.geometry_swaps(23, shift=1)
    book = Y.Book([(f"{i}: {swaps[(i + 1) % 23][0]}",) + tuple(swaps[(i + 1) % 23][1:]) for i in range(600)])
    sub_off = np.arange(601)
    check_book(E, twin_of, interp, Y.infl_curve(64, YC.LZ), book, sub_off, "600 one-swap desks, P_i = 64")


def _dev_call(ctx, dc, infl, fixed, coupons, sub_off, cpn_off=None, guard=16):
    """adr_yoy_subbook_ladders_dev on a caller's stream and buffers with ``guard`` words behind `out` and the scratch, which
    must keep their pattern.  ``cpn_off``: coupon offsets to upload in place of the book's (the entry checks scalars only)."""
    im, T, b = infl
    good_off, cpn = _native.yoy_pack(coupons)
    n, B, Pi = good_off.size - 1, len(sub_off) - 1, np.asarray(T).size
    Q = dc.n_pillars + Pi
    stride = 1 + Q + Q * Q
    work, chunks = _native.yoy_subbook_ladders_work(dc, Pi, n, B)
    assert chunks == (n + 63) // 64 + B
    out = torch.full((B * stride + guard,), -7.25, dtype=torch.float64, device="cuda")
    scratch = torch.full((work + guard,), -7.25, dtype=torch.float64, device="cuda")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    bufs = dict(T=up(T), b=up(b), fix_off=up(fixed[0]), fix_tp=up(fixed[1]), fix_pay=up(fixed[2]),
                cpn_off=up(good_off if cpn_off is None else cpn_off), cpn=up(cpn),
                plan=up(_native.scenario_subbook_plan(n, np.asarray(sub_off, dtype=np.int64))))
    stream = torch.cuda.Stream()
    _native.yoy_subbook_ladders_dev(ctx, dc, im, Pi, n, fixed[1].size, cpn.shape[1], B, {k: v.data_ptr() for k, v in bufs.items()},
                                    7, out.data_ptr(), scratch.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert bool((out[B * stride:] == -7.25).all()) and bool((scratch[work:] == -7.25).all()), "guard words were written"
    return out[:B * stride].cpu().numpy().reshape(B, stride)


def test_dev_entry_in_guarded_buffers_and_malformed_offsets(gpu_ctx):
    """The non-blocking entry has the blocking entry's bits and leaves the guard words alone.  Coupon offsets that cannot be
    right - a swap whose range ends past m; its chunk reads nothing of it - give NaN in that swap's desk and leave every
    other row's bits."""
    interp = Y.SCHEMES[0]
    host, dc, E, _ = _entries(gpu_ctx, interp)
    infl, book, sub_off = Y.infl_curve(12, YC.LZ), Y.geometry_book(), Y.offsets(Y.GEOMETRY_SIZES)
    want = E(infl, book.fixed, book.coupons, sub_off)
    rows = _dev_call(gpu_ctx, dc, infl, book.fixed, book.coupons, sub_off)
    assert np.array_equal(Y.bits(rows), Y.bits(want["ladders"]))
    bad = book.coupons["cpn_off"].copy()
    j = int(sub_off[4]) + 3                                   # a swap of desk 4 (65 swaps, two chunks)
    bad[j + 1] = bad[-1] + 1000                               # swap j ends past m, swap j + 1 begins there
    got = _dev_call(gpu_ctx, dc, infl, book.fixed, book.coupons, sub_off, cpn_off=bad)
    assert np.all(np.isnan(got[4]))
    others = [d for d in range(len(sub_off) - 1) if d != 4]
    assert np.array_equal(Y.bits(got[others]), Y.bits(want["ladders"][others]))


def test_refusals(gpu_ctx):
    interp = Y.SCHEMES[0]
    host, dc, E, _ = _entries(gpu_ctx, interp)
    infl, book, sub_off = Y.infl_curve(12, YC.LZ), Y.small_book(), Y.offsets(Y.SMALL_SIZES)
    im, T, b = infl
    for code, match, bad in ((-2, "inflation scheme must be", (YC.LF, T, b)),
                             (-2, "1 .. ADR_YOY_MAX_PILLARS", (YC.LZ, np.append(YC.pillars(64)[0], 41.0), np.append(YC.pillars(64)[1], 0.03))),
                             (-1, "pillar times must be increasing", (YC.LZ, T[::-1].copy(), b))):
        with pytest.raises(LibError, match=match) as e:
            E(bad, book.fixed, book.coupons, sub_off)
        assert e.value.status == code
    with pytest.raises(LibError, match=r"decreases at sub-book 1 \(5 \.\. 3\)"):
        E(infl, book.fixed, book.coupons, [0, 5, 3, book.n])
    no_hess = _native.DeviceCurve(gpu_ctx, interp.value, host.times, host.dfs, host.jac, None)
    try:
        bare = Y.Entries(interp.value, host, gpu_ctx, no_hess)
        with pytest.raises(LibError, match="GAMMA requested but the curve was uploaded without hess") as e:
            bare(infl, book.fixed, book.coupons, sub_off)
        assert e.value.status == -1
        d_only = bare(infl, book.fixed, book.coupons, sub_off, want_gamma=False)
        assert Y.same_bits(d_only, E(infl, book.fixed, book.coupons, sub_off, want_gamma=False))
    finally:
        no_hess.close()
    with pytest.raises(LibError, match="adr_yoy_subbook_ladders_work"):
        _native.yoy_subbook_ladders_work(dc, 65, book.n, 4)


@pytest.mark.parametrize("interp", Y.SCHEMES)
def test_explain_against_full_revaluation(gpu_ctx, interp):
    """`YoYBook.explain_sub_books` on a two-desk book under joint shocks h (u, v), h = 4, 8, 16 bp: with the cross block the
    unexplained P&L is third order per desk and direction (ratio under doubling in [7, 9]), without it second order
    ([3, 5]); the zero pair is exactly 0; the chained VaR / ES has `tail_measures`' bits; `pnl_delta_gamma(cross=True)` is the
    one-desk row.  The bands and the (empty) list of dropped desk-directions come from the oracle-derived ladders
    (tests/test_yoy_sub_book_ladders_host.py)."""
    from adrates_amd.market.position.yoy_book import YoYBook
    from adrates_amd.trades.market_data import random_yoy_book, yoy_model
    from .test_yoy_sub_book_ladders_host import EXPLAIN_DROPPED
    model = yoy_model(Y.VD, interp)
    swaps = random_yoy_book(Y.VD, 24, seed=13)
    keys = ["rates" if i % 3 else "linkers" for i in range(24)]
    book = YoYBook(swaps, model)
    tenors = model._curve_params_dict["GBP_OIS_SONIA"]["tenor_list"]
    infl_tenors = book.compute_sub_books({RequestTypes.VALUE}, keys)["infl_tenors"]
    x, y = Y.joint_shock_rows(len(tenors), len(infl_tenors))
    shocks = [{t: v / 100.0 for t, v in zip(tenors, row)} for row in x]          # the same shocks in percent
    infl_shocks = [{t: float(v) for t, v in zip(infl_tenors, row)} for row in y]  # basis points
    grid = ScenarioGrid(model, "GBP_OIS_SONIA", shocks, ctx=gpu_ctx)
    try:
        ex = book.explain_sub_books(keys, grid=grid, inflation_shocks=infl_shocks)
        assert ex["labels"] == ["linkers", "rates"] and all(ex[k].shape == (2, 19) for k in ("full", "delta_pnl", "gamma_pnl"))
        assert C.same_bits(ex["full"], book.pnl_sub_books(keys, grid=grid, inflation_shocks=infl_shocks))
        Y.check_bands(ex["labels"], ex["full"], ex["delta_pnl"], ex["gamma_pnl"], f"device, {interp.name}, cross", True, EXPLAIN_DROPPED)
        no = book.explain_sub_books(keys, grid=grid, inflation_shocks=infl_shocks, cross=False)
        Y.check_bands(no["labels"], no["full"], no["delta_pnl"], no["gamma_pnl"], f"device, {interp.name}, no cross", False,
                      EXPLAIN_DROPPED)
        dg = book.pnl_delta_gamma_sub_books(keys, grid=grid, inflation_shocks=infl_shocks)
        assert C.same_bits(dg["pnl"], ex["delta_pnl"] + ex["gamma_pnl"]) and "delta_pnl" not in dg
        for level in (0.99, 0.75):
            chained = book.sub_book_delta_gamma_var_es(keys, level, grid=grid, inflation_shocks=infl_shocks)
            var, es = tail_measures(dg["pnl"], level, ctx=gpu_ctx)
            assert chained["labels"] == dg["labels"]
            assert C.same_bits(chained["var"], var) and C.same_bits(chained["es"], es), level
        one = book.pnl_delta_gamma(grid=grid, inflation_shocks=infl_shocks, cross=True)
        whole = book.pnl_delta_gamma_sub_books(["all"] * 24, grid=grid, inflation_shocks=infl_shocks)
        assert one.shape == (19,) and C.same_bits(one, whole["pnl"][0])
        old = book.pnl_delta_gamma(grid=grid, inflation_shocks=infl_shocks)
        assert old.shape == (19,) and not C.same_bits(old, one)
    finally:
        grid.close()
