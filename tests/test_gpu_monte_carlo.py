"""Monte Carlo delta-gamma VaR on the GPU (adr_shock_normal*, csrc/shock_normal.hip; adr_scenario_tail_select*,
csrc/tail_select.hip), on the tables of the CPU suite: the device's uniforms with the twin's bits, its normals and shocks
held to the mpmath reference (not to the twin), the cut of a set and the antithetic pairing, the device-array entries in
guarded buffers; the tail select with the twin's bits on every row of the table and adr_scenario_tail's where that takes
the rows; the chain `monte_carlo_var_es` against its three steps, whatever the tiling, for rates, credit and inflation desks."""
import numpy as np
import pytest
import torch

from adrates_amd import _native
from adrates_amd.market.position.ladder_pnl import augmented_ladder_pnl, ladder_pnl
from adrates_amd.market.position.monte_carlo import (factor_from_covariance, monte_carlo_shocks, monte_carlo_var_es,
                                                     sub_book_monte_carlo_var_es, tail_measures_select)
from adrates_amd.utils.error import LibError
from adrates_amd.utils.global_types import RequestTypes

from . import _monte_carlo_cases as C

pytestmark = pytest.mark.gpu
GUARD = -7.25
REQS = {RequestTypes.VALUE, RequestTypes.DELTA, RequestTypes.GAMMA}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------------------------------------------------- generator
def test_uniforms_have_the_twins_bits(gpu_ctx):
    for seed in C.SEEDS:
        for g in C.INDICES:
            for anti, first in ((False, g), (True, 2 * g + 1)):
                dev = _native.shock_uniforms(3, 5, seed, anti, first, ctx=gpu_ctx)
                assert np.array_equal(bits(dev), bits(_native.shock_uniforms(3, 5, seed, anti, first))), (seed, g, anti)
                assert np.array_equal(bits(dev[0]), bits(np.array([C.uniform_doubles(seed, g, i) for i in range(3)])))
    for anti in (False, True):                                      # several blocks, an odd pair count
        dev = _native.shock_uniforms(700, 7, 99, anti, 12345, ctx=gpu_ctx)
        assert np.array_equal(bits(dev), bits(_native.shock_uniforms(700, 7, 99, anti, 12345)))


def test_normals_and_products_against_mpmath(gpu_ctx):
    """The index rows of every seed: z through the identity factor, x through dense factors, the device held to the
    reference.  Observed on the device: z 0.096 of its bound, x 0.056 (the host twin's figures)."""
    dev = lambda f, seed, anti, first: _native.shock_normal(gpu_ctx, f, 1, seed, anti, first)
    worst_z = worst_x = 0.0
    for seed in C.SEEDS:
        for g in C.INDICES:
            worst_z = max(worst_z, C.worst_z_ratio(seed, [g], dev(np.eye(8), seed, False, g)))
            for P, F in ((8, 8), (9, 5)):
                f = C.factor_matrix(P, F)
                worst_x = max(worst_x, C.worst_x_ratio(seed, [g], f, dev(f, seed, False, g)))
                worst_x = max(worst_x, C.worst_x_ratio(seed, [2 * g + 1], f, dev(f, seed, True, 2 * g + 1), True))
    print(f"device: worst |dz| {worst_z:.3f} of its bound, worst |dx| {worst_x:.3f} of its bound")
    assert worst_z <= 1.0 and worst_x <= 1.0


@pytest.mark.parametrize("P,F", C.GEOMETRY)
def test_geometry_against_the_reference(gpu_ctx, P, F):
    """Every scenario count of the table as a launch of its own: the reference's bound, and the bits of the same rows in
    the largest launch."""
    f = C.factor_matrix(P, F)
    big = _native.shock_normal(gpu_ctx, f, max(C.SCENARIOS), C.GEOMETRY_SEED)
    worst = C.worst_x_ratio(C.GEOMETRY_SEED, range(max(C.SCENARIOS)), f, big)
    print(f"device, P = {P}, F = {F}: worst |dx| {worst:.3f} of its bound")
    assert worst <= 1.0
    for S in C.SCENARIOS:
        assert np.array_equal(bits(_native.shock_normal(gpu_ctx, f, S, C.GEOMETRY_SEED)), bits(big[:S])), S
    assert np.array_equal(bits(_native.shock_normal(gpu_ctx, f, max(C.SCENARIOS), C.GEOMETRY_SEED)), bits(big)), "two runs"


def test_rows_do_not_depend_on_the_cut(gpu_ctx):
    dev = lambda f, S, anti, first: _native.shock_normal(gpu_ctx, f, S, 11, anti, first)
    f = C.factor_matrix(9, 5)
    for anti in (False, True):
        for first in (0, 7):
            whole = dev(f, 200, anti, first)
            at, pieces = first, []
            for n in (1, 63, 64, 72):
                pieces.append(dev(f, n, anti, at))
                at += n
            assert np.array_equal(bits(np.vstack(pieces)), bits(whole)), (anti, first)
            assert np.array_equal(bits(dev(f, 50, anti, first + 150)), bits(whole[150:]))
    x = dev(f, 201, True, 3)                                        # global rows 3 .. 203: x[1] and x[2] are the pair (4, 5)
    assert np.array_equal(bits(x[1:200:2]), bits(-x[2:201:2]))
    assert np.array_equal(bits(dev(f, 4, False, 2)), bits(x[1:9:2])), "pair i of an antithetic set is row i of the plain one"
    # a zero row is +0.0, -0.0 on the negated rows; a zero column drops its normal exactly
    z = _native.shock_normal(gpu_ctx, np.eye(3), 66, 5)
    g = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    xz, xa = _native.shock_normal(gpu_ctx, g, 66, 5), _native.shock_normal(gpu_ctx, g, 66, 5, True)
    assert np.array_equal(bits(xz[:, [0, 2]]), bits(z[:, [0, 2]])) and np.array_equal(bits(xz[:, 1]), bits(np.zeros(66)))
    assert np.array_equal(bits(xa[:, 1]), bits(np.where(np.arange(66) % 2 == 1, -0.0, 0.0)))


@pytest.mark.parametrize("P,F,S", [(33, 7, 129), (65, 65, 65), (256, 256, 65)])
def test_shock_dev_entry_in_guarded_buffers(gpu_ctx, P, F, S):
    """adr_shock_normal_dev on a caller's stream: the blocking entry's bits, 16 guard words behind each buffer intact."""
    f = C.factor_matrix(P, F)
    tail = 16
    fac = torch.cat([torch.from_numpy(f.ravel()), torch.full((tail,), GUARD, dtype=torch.float64)]).cuda()
    out = torch.full((S * P + tail,), GUARD, dtype=torch.float64, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    _native.shock_normal_dev(gpu_ctx, 17, 1000, S, P, F, fac.data_ptr(), True, out.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[S * P:] == GUARD) and bool((fac[-tail:] == GUARD).all())
    assert np.array_equal(bits(got[:S * P].reshape(S, P)), bits(_native.shock_normal(gpu_ctx, f, S, 17, True, 1000)))
    assert np.array_equal(fac[:-tail].cpu().numpy(), f.ravel())


def test_generator_refusals_on_the_device(gpu_ctx):
    buf = torch.full((64,), GUARD, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    for args in ((0, 4, 3, 4, p, False, p), (0, 4, 257, 4, p, False, p), (0, 0, 4, 4, p, False, p), (-1, 4, 4, 4, p, False, p),
                 (0, 4, 4, 4, 0, False, p), (0, 4, 4, 4, p, False, 0)):
        with pytest.raises(LibError) as e:
            _native.shock_normal_dev(gpu_ctx, 1, *args)
        assert e.value.status == -1, args
    with pytest.raises(LibError) as e:
        _native.shock_normal(gpu_ctx, np.zeros((2, 3)), 4, 1)
    assert e.value.status == -1
    gpu_ctx.sync()
    assert bool((buf == GUARD).all())


# -------------------------------------------------------------------------------------------------------- tail select
@pytest.mark.parametrize("m", C.WIDTHS)
def test_tail_select_has_the_twins_bits(gpu_ctx, m):
    """Every content, base column and tail count of the table at width m: the twin's bits, adr_scenario_tail's on the
    device where that takes the rows, and the same bits from a second run."""
    for content in C.CONTENTS:
        for B in ((1, 3) if content in ("normal", "nan") else (3,)):
            for k in C.tail_counts(m):
                pnl = C.pnl_rows(content, B, m, k)
                for base_col, _ in C.base_cols(m):
                    rows = C.with_base(pnl, base_col, content)
                    dev = _native.scenario_tail_select(gpu_ctx, rows, k, base_col)
                    twin = _native.scenario_tail_select_host(rows, k, base_col)
                    assert C.same_bits(dev[0], twin[0]) and C.same_bits(dev[1], twin[1]), (content, B, k, base_col)
                    if m <= C.TAIL_MAX:
                        whole = _native.scenario_tail(gpu_ctx, rows, k, base_col)
                        assert C.same_bits(dev[0], whole[0]) and C.same_bits(dev[1], whole[1]), (content, B, k, base_col)
                    if base_col == -1:
                        again = _native.scenario_tail_select(gpu_ctx, rows, k, base_col)
                        assert C.same_bits(dev[0], again[0]) and C.same_bits(dev[1], again[1]), "two runs"


@pytest.mark.parametrize("B,m,k,base_col", [(3, 40000, 400, -1), (70, 16385, 164, 5), (1, 131075, 16384, 131075), (2500, 300, 3, -1)])
def test_select_dev_entry_in_guarded_buffers(gpu_ctx, B, m, k, base_col):
    """adr_scenario_tail_select_dev on a caller's stream with a scratch of exactly adr_scenario_tail_select_work bytes:
    the twin's bits, the guard words behind the scratch, the rows and the outputs intact.  The shapes take one and several
    segments per row, rows beyond the blocks aimed at, and adr_scenario_tail_dev's bits where that takes the rows."""
    rows = C.with_base(C.pnl_rows("normal", B, m, k), base_col, "normal")
    S_tot = rows.shape[1]
    tail = 16
    need = _native.scenario_tail_select_work(B, S_tot, k)
    assert need > 0 and need % 8 == 0
    d_rows = torch.cat([torch.from_numpy(rows.ravel()), torch.full((tail,), GUARD, dtype=torch.float64)]).cuda()
    work = torch.full((need // 8 + tail,), GUARD, dtype=torch.float64, device="cuda")
    out = torch.full((2, B + tail), GUARD, dtype=torch.float64, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    _native.scenario_tail_select_dev(gpu_ctx, B, S_tot, d_rows.data_ptr(), k, out[0].data_ptr(), out[1].data_ptr(), work.data_ptr(),
                                     base_col=base_col, stream=stream.cuda_stream)
    stream.synchronize()
    got = out.cpu().numpy()
    twin = _native.scenario_tail_select_host(rows, k, base_col)
    assert C.same_bits(got[0, :B], twin[0]) and C.same_bits(got[1, :B], twin[1])
    assert np.all(got[:, B:] == GUARD) and bool((work[need // 8:] == GUARD).all()) and bool((d_rows[-tail:] == GUARD).all())
    assert np.array_equal(d_rows[:-tail].cpu().numpy(), rows.ravel())
    if m <= C.TAIL_MAX:
        _native.scenario_tail_dev(gpu_ctx, B, S_tot, d_rows.data_ptr(), k, out[0].data_ptr(), out[1].data_ptr(), base_col=base_col,
                                  stream=stream.cuda_stream)
        stream.synchronize()
        whole = out.cpu().numpy()
        assert C.same_bits(whole[0, :B], twin[0]) and C.same_bits(whole[1, :B], twin[1])


def test_tail_select_refusals_on_the_device(gpu_ctx):
    rows = np.zeros((2, 20000))
    for k, base_col, status in ((16385, -1, -2), (0, -1, -1), (20001, -1, -1), (20000, 0, -1), (5, 20000, -1)):
        with pytest.raises(LibError) as e:
            _native.scenario_tail_select(gpu_ctx, rows, k, base_col)
        assert e.value.status == status, (k, base_col)
    buf = torch.full((64,), GUARD, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    for args in ((2, 8, p, 9, p, p, p), (2, 8, 0, 1, p, p, p), (2, 8, p, 1, 0, p, p), (2, 8, p, 1, p, p, 0), (0, 8, p, 1, p, p, p)):
        with pytest.raises(LibError) as e:
            _native.scenario_tail_select_dev(gpu_ctx, *args)
        assert e.value.status == -1, args
    gpu_ctx.sync()
    assert bool((buf == GUARD).all())


# -------------------------------------------------------------------------------------------------------------- chain
@pytest.mark.parametrize("P", [9, 32])
def test_chain_against_its_steps(gpu_ctx, P):
    """`monte_carlo_var_es` on 19 desks and 20 000 scenarios: `tail_measures_select` of `ladder_pnl` of the device's shocks,
    both on their twins, bit for bit, with tiles of 1, 8 and 19 desks."""
    B, S = 19, 20000
    delta, gamma = C.ladders(B, P)
    L = factor_from_covariance(C.covariance(P))
    shocks = monte_carlo_shocks(L, S, 7, host=False, ctx=gpu_ctx)
    want = tail_measures_select(ladder_pnl(delta, gamma, shocks, host=True), 0.99, host=True)
    for desks in (19, 8, 1):
        got = monte_carlo_var_es(delta, gamma, L, S, level=0.99, seed=7, ctx=gpu_ctx, max_bytes=desks * 8 * S)
        assert C.same_bits(got["var"], want[0]) and C.same_bits(got["es"], want[1]), desks
    dev = tail_measures_select(ladder_pnl(delta, gamma, shocks, ctx=gpu_ctx), 0.99, ctx=gpu_ctx)
    assert C.same_bits(dev[0], want[0]) and C.same_bits(dev[1], want[1])
    anti = monte_carlo_var_es(delta, gamma, L, S, level=0.95, seed=7, antithetic=True, ctx=gpu_ctx)
    xa = monte_carlo_shocks(L, S, 7, antithetic=True, ctx=gpu_ctx)
    ref = tail_measures_select(ladder_pnl(delta, gamma, xa, host=True), 0.95, host=True)
    assert C.same_bits(anti["var"], ref[0]) and C.same_bits(anti["es"], ref[1])
    with pytest.raises(LibError) as e:
        monte_carlo_var_es(delta, gamma, L, 400000, level=0.95, ctx=gpu_ctx)
    assert e.value.status == _native.ADR_ERR_UNSUPPORTED


def _check_ladders(gpu_ctx, ladders, Q, what):
    """Ready rows through `monte_carlo_var_es` with a Q-row factor against the three steps."""
    L = factor_from_covariance(C.covariance(Q), min(Q, 6))
    S = 20000
    got = monte_carlo_var_es(None, None, L, S, level=0.99, seed=21, ctx=gpu_ctx, ladders=ladders)
    shocks = monte_carlo_shocks(L, S, 21, ctx=gpu_ctx)
    want = tail_measures_select(augmented_ladder_pnl(ladders, shocks, host=True), 0.99, host=True)
    assert C.same_bits(got["var"], want[0]) and C.same_bits(got["es"], want[1]), what
    assert np.all(np.isfinite(got["var"])) and np.all(got["es"] >= got["var"]), what


def test_sub_books_of_the_three_product_lines(gpu_ctx):
    """`sub_book_monte_carlo_var_es` on the small mixed book; one credit and one YoY augmented ladder with a Q-row factor."""
    from adrates_amd.market.position.engine import Engine
    from adrates_amd.market.position.sub_book_ladders import price_credit_sub_books, price_sub_books, price_yoy_sub_books
    from adrates_amd.market.position.yoy_book import YoYBook

    from . import _credit_ladder_cases as X
    from . import _ladder_pnl_cases as LC
    from . import _yoy_ladder_cases as Y
    model, ir = LC.gbp(LC.SCHEMES[0])
    book = LC.L.mixed_book(n_ois=60)
    keys = [5 * i // book.n_trades for i in range(book.n_trades)]          # five desks of consecutive trades
    P = len(ir.swap_rates)
    L = factor_from_covariance(C.covariance(P))
    eng = Engine(model)
    got = sub_book_monte_carlo_var_es(eng, ir, book, keys, L, 20000, level=0.99, seed=3)
    lad = price_sub_books(eng, ir, book, keys, REQS)
    want = monte_carlo_var_es(lad["delta"], lad["gamma"], L, 20000, seed=3, ctx=gpu_ctx)
    assert got["labels"] == lad["labels"] and C.same_bits(got["var"], want["var"]) and C.same_bits(got["es"], want["es"])
    assert np.all(got["es"] >= got["var"]) and np.all(got["var"] > 0.0)

    trades, spreads, ckeys, buckets = X.explain_book()
    credit = price_credit_sub_books(eng, ir, trades, spreads, ckeys, buckets, REQS)
    _check_ladders(gpu_ctx, credit["ladders"], P + len(credit["buckets"]), "credit")

    ymodel, swaps, ykeys = Y.explain_book()
    yb = YoYBook(swaps, ymodel)
    yoy = price_yoy_sub_books(Engine(ymodel), yb.curve, yb.inflation_curve, swaps, ykeys, REQS)
    Q = len(yoy["tenors"]) + len(yoy["infl_tenors"])
    _check_ladders(gpu_ctx, yoy["ladders"], Q, "inflation")
    direct = monte_carlo_var_es(yoy["delta"], yoy["gamma"], factor_from_covariance(C.covariance(Q), min(Q, 6)), 20000, seed=21,
                                ctx=gpu_ctx)
    again = monte_carlo_var_es(None, None, factor_from_covariance(C.covariance(Q), min(Q, 6)), 20000, seed=21, ctx=gpu_ctx,
                               ladders=yoy["ladders"])
    assert C.same_bits(direct["var"], again["var"]) and C.same_bits(direct["es"], again["es"])
