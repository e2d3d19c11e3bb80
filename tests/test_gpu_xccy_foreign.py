"""`adr_price_xccy_foreign` - the XC instantiations of `price_lite_kernel` (csrc/kernels_lite.hip), the foreign leg of a
cross-currency book on two curves in one launch - against the plain 60-digit reference (tests/_xccy_foreign_reference.py),
EVERY element of pv, delta_foreign and delta_basis of every case (tests/_xccy_foreign_cases.py; tests/test_xccy_foreign_host.py
asserts on the CPU that the entry will take each book) on the counted bound |got - value| <= k 2^-53 gross, and +0.0 where
gross is 0.  Every case runs under masks 3, 1 and 2, per trade without and with the aggregates, and aggregates only; only the
blocks asked for are returned (a buffer of a block that is not asked for keeps its fill), and every launch runs twice, bit for
bit: this path has no atomics.

Aggregates: agg_foreign = [pv total, delta_foreign sums, zeros], agg_basis = [+0.0, delta_basis sums, zeros], held to the
reference's one-desk row with the sums counted (`aggregate_sums`); the gamma parts are +0.0; the PV total is there under every
mask; under a mask without DELTA words 1 .. P of both are +0.0.  The kernel is only built with DELTA, so its block records
always carry the delta sums: until this module the reduction wrote them under VALUE alone.  `adr_price_xccy_foreign_dev` now
passes the request to `reduce_partials_kernel`, which drops them in the same pass (capi.hip; include/adrates.h says so).

One curve passed twice: delta_foreign + delta_basis and pv meet `adr_price`'s mask-3 result (`lite_lag`) for the same batch -
both are held to their references, which tests/test_xccy_foreign_host.py holds to each other, and their exact difference to
the sum of the two bounds.  `adr_price_xccy_foreign_dev` on a caller's stream into buffers with 16 guard words behind each of
the five outputs: the guards are intact and the bits are the blocking entry's; a null delta_foreign with a live delta_basis
and the reverse write only the live one; n = 0 zeroes exactly the aggregates' words.  Launch shape: three one-row trades and a
two-row trade cycled through books of 1, 3, 4, 5 trades and of u, u + 1 and 2 u + 1 units (u = 12 blocks, the grid read off
the device's CU count): every copy has the bits of its trade in the four-trade launch, which is held to the bound.  Refusals
leave the outputs untouched: GAMMA, LINEAR_FWD_RATES beside a log scheme both ways, a 33-pillar curve on either side, a leg of
391 coupons, an unlagged leg (-2 each), curves of another context (ADR_ERR_INVALID).  `adr_curve_upload` admits hand-made
tables large enough for two of them to exceed the LDS of a CU: a pair of 240 and 230 knots just inside the 160 KiB (163 568
bytes) is held to the bound, the pair with one knot more (163 872 bytes) is refused with -2.

Worst shares of the bound observed on an MI355X (every test prints its own), per trade | aggregates:
  LINEAR_ZERO x FLAT_FWD  0.109 | 0.021     FLAT_FWD x LINEAR_ZERO  0.198 | 0.020     FLAT_FWD x FLAT_FWD  0.126 | 0.025
  LINEAR_ZERO x LINEAR_ZERO  0.101 | 0.028  LINEAR_FWD x LINEAR_FWD  0.065 | 0.011
  one curve as both 0.082 (LINEAR_FWD_RATES 0.050), and |two-curve launch - adr_price| at most 0.044 of the sum of the two
  bounds;  the base launch of the launch-shape check 0.049;  the pair just inside the LDS budget 0.098 | 0.005
No share above 1, no dust on a structural zero: the kernel needed no change.  The parent's library fails all 19 cases on the
VALUE-only aggregates alone.  DESIGN.md section 35 has the k table, the instantiations reached (all four XC ones) and the
mutations.  The slowest test takes 0.6 s (the counts books, 11 legs of up to 390 coupons, nearly all of it the reference), the
module 6 s; the launch-shape check prices up to 24 577 trades on 256 CUs."""
import time
from fractions import Fraction

import numpy as np
import pytest

from adrates_amd import _native

from . import _ladder_edge_cases as E
from . import _price_edge_cases as PE
from . import _price_lag_cases as PL
from . import _price_reference as PR
from . import _xccy_foreign_cases as XC
from . import _xccy_foreign_reference as XR
from . import _xccy_scenario_cases as XS

pytestmark = pytest.mark.gpu

CASES = XC.cases()
N_CASES = 19
GUARD = 16
FILL = -7.25
REQUESTS = tuple((mask, per_trade, aggregate) for mask in (3, 1, 2) for per_trade, aggregate in ((True, False), (True, True), (False, True)))


def device_curve(ctx, interp, h):
    return _native.DeviceCurve(ctx, interp.value, h.times, h.dfs, h.jac, h.hess)


def call(ctx, cf, cx, dt, mask, per_trade=True, aggregate=False):
    """`adr_price_xccy_foreign` with EVERY buffer of the request's shape handed in, filled with FILL: ``(status, buffers)`` -
    pv, delta_foreign, delta_basis (None unless ``per_trade``), agg_foreign, agg_basis (None unless ``aggregate``), whole."""
    n, Pf, Px = dt.n_trades, cf.n_pillars, cx.n_pillars
    full = lambda *shape: np.full(shape, FILL)
    out = dict(pv=full(n) if per_trade else None, delta_foreign=full(n, Pf) if per_trade else None, delta_basis=full(n, Px) if per_trade else None,
               agg_foreign=full(1 + Pf + Pf * Pf) if aggregate else None, agg_basis=full(1 + Px + Px * Px) if aggregate else None)
    rc = _native.load().adr_price_xccy_foreign(ctx._h, cf._h, cx._h, dt._h, int(mask), *[_native._ptr(out[k]) for k in
                                               ("pv", "delta_foreign", "delta_basis", "agg_foreign", "agg_basis")])
    return rc, out


def split(out, Pf, Px):
    """The aggregates of `call` taken apart: ``({"pv", "delta_foreign", "delta_basis"}, the words that must be +0.0)``."""
    af, ax = out["agg_foreign"], out["agg_basis"]
    return dict(pv=af[:1], delta_foreign=af[1:1 + Pf], delta_basis=ax[1:1 + Px]), np.concatenate([af[1 + Pf:], ax[:1], ax[1 + Px:]])


def plus_zero(a):
    return not np.any(a) and not np.any(np.signbit(a))


def check_request(ctx, cf, cx, dt, case, mask, per_trade, aggregate, ref, book, ks, n_cu, what):
    """One request, twice: the blocks asked for on the bound, the others untouched or +0.0; returns (per-trade, aggregate) shares."""
    Pf, Px, n = cf.n_pillars, cx.n_pillars, dt.n_trades
    rc, got = call(ctx, cf, cx, dt, mask, per_trade, aggregate)
    rc2, again = call(ctx, cf, cx, dt, mask, per_trade, aggregate)
    assert rc == 0 and rc2 == 0, (what, rc, rc2)
    for k in got:
        assert (got[k] is None) == (again[k] is None) and (got[k] is None or np.array_equal(PR.bits(got[k]), PR.bits(again[k]))), f"{what}: two launches differ in {k}"
    shares = [0.0, 0.0]
    if per_trade:
        asked = {"pv": mask & 1, "delta_foreign": mask & 2, "delta_basis": mask & 2}
        for k, want in asked.items():
            if not want:
                assert np.all(got[k] == FILL), f"{what}: {k} is not asked for and was written"
        shares[0] = XR.rows_share({k: got[k] for k, want in asked.items() if want}, ref, ks, what)
    if aggregate:
        blocks, zeros = split(got, Pf, Px)
        assert plus_zero(zeros), f"{what}: agg_basis[0] or a gamma part is not +0.0"
        names = ["pv"]
        if mask & 2:
            names += ["delta_foreign", "delta_basis"]
        else:
            assert plus_zero(blocks["delta_foreign"]) and plus_zero(blocks["delta_basis"]), f"{what}: no DELTA asked for, the aggregates' delta parts are not +0.0"
        sums = XR.aggregate_sums(n, XC.blocks_for(XC.units_of(case.batch), n_cu))
        shares[1] = XR.book_share(blocks, ref, book, ks, sums, what, names)
    return shares


@pytest.mark.parametrize("which", range(N_CASES))
def test_every_element_of_every_request(gpu_ctx, which):
    import torch
    case = CASES[which]
    t0 = time.perf_counter()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    ref, book, ks = XR.per_trade_reference(*case.args), XR.book_reference(*case.args), XR.case_ks(*case.args)
    t_ref = time.perf_counter() - t0
    cf, cx = device_curve(gpu_ctx, case.f_interp, case.f_host), device_curve(gpu_ctx, case.x_interp, case.x_host)
    worst = [0.0, 0.0]
    with _native.DeviceTrades(gpu_ctx, case.batch) as dt:
        for mask, per_trade, aggregate in REQUESTS:
            what = f"{case.id}, mask {mask}{', per trade' if per_trade else ''}{', aggregates' if aggregate else ''}"
            shares = check_request(gpu_ctx, cf, cx, dt, case, mask, per_trade, aggregate, ref, book, ks, n_cu, what)
            print(f"{what}: share of the bound {shares[0]:.3f} per trade, {shares[1]:.3f} aggregates")
            assert max(shares) <= 1.0, what
            worst = [max(a, b) for a, b in zip(worst, shares)]
    cf.close(); cx.close()
    print(f"{case.id}: {case.batch.n_trades} trades, k {min(ks)} to {max(ks)}, worst shares {worst[0]:.3f} per trade, {worst[1]:.3f} aggregates; "
          f"{time.perf_counter() - t0:.1f} s ({t_ref:.1f} s the reference)")


@pytest.mark.parametrize("which", range(2))
def test_one_curve_passed_twice_meets_adr_price(gpu_ctx, which):
    case = [c for c in CASES if c.name.startswith("one curve as both")][which]
    method, h, batch = case.f_interp.value, case.f_host, case.batch
    assert set(PE.families(PL.LagCase(case.name, case.f_interp, case.f_label, h, batch), 3, True, False)) == {"lite_lag"}
    ref, ks = XR.per_trade_reference(*case.args), XR.case_ks(*case.args)
    old = PR.per_trade_reference(method, h, batch)
    old_ks = PR.case_ks(method, h, batch, old, ["lite_lag"] * batch.n_trades)
    dc = device_curve(gpu_ctx, case.f_interp, h)
    with _native.DeviceTrades(gpu_ctx, batch) as dt:
        rc, got = call(gpu_ctx, dc, dc, dt, 3)
        one = _native.price(gpu_ctx, dc, dt, want_value=True, want_delta=True, want_gamma=False, per_trade=True, aggregate=False)
    dc.close()
    assert rc == 0
    a = XR.rows_share(got, ref, ks, case.id)
    b = PR.rows_share(one, old, old_ks, case.id)
    print(f"{case.id}: share of the bound, the two-curve launch {a:.3f}, adr_price {b:.3f}")
    assert a <= 1.0 and b <= 1.0
    worst = Fraction(0)
    unit = Fraction(1, 2 ** 53)
    for i in range(batch.n_trades):
        two = [(Fraction(float(got["pv"][i])), [XR.rational(ref[i]["pv"], (0,))[1]], Fraction(float(one["pv"][i])), XR.rational(old[i]["pv"], (0,))[1])]
        for p in range(h.jac.shape[1]):
            two.append((Fraction(float(got["delta_foreign"][i, p])) + Fraction(float(got["delta_basis"][i, p])),
                        [XR.rational(ref[i]["delta_foreign"], (p,))[1], XR.rational(ref[i]["delta_basis"], (p,))[1]],
                        Fraction(float(one["delta"][i, p])), XR.rational(old[i]["delta"], (p,))[1]))
        for mine, gross, theirs, old_gross in two:
            bound = unit * (ks[i] * sum(gross) + old_ks[i] * old_gross)
            assert abs(mine - theirs) <= bound, (case.id, i)
            if bound:
                worst = max(worst, abs(mine - theirs) / bound)
    print(f"{case.id}: |two-curve launch - adr_price| is at most {float(worst):.3f} of the sum of the two bounds")


def test_the_dev_entry_writes_nothing_behind_its_buffers(gpu_ctx):
    import torch
    case = [c for c in CASES if c.name == "structure" and c.f_label == "README 32" and c.f_interp == PE.LZ][0]
    Pf, Px, n = case.f_host.jac.shape[1], case.x_host.jac.shape[1], case.batch.n_trades
    assert Px % 2 == 1
    dev = torch.device("cuda", 0)
    sizes = dict(pv=n, delta_foreign=n * Pf, delta_basis=n * Px, agg_foreign=1 + Pf + Pf * Pf, agg_basis=1 + Px + Px * Px)
    cf, cx = device_curve(gpu_ctx, case.f_interp, case.f_host), device_curve(gpu_ctx, case.x_interp, case.x_host)
    stream = torch.cuda.Stream(device=dev)

    def run(dt, mask, live):
        bufs = {k: torch.full((m + GUARD,), FILL, dtype=torch.float64, device=dev) for k, m in sizes.items()}
        torch.cuda.synchronize()
        _native.price_xccy_foreign_dev(gpu_ctx, cf, cx, dt, mask, *[bufs[k].data_ptr() if k in live else 0 for k in sizes], stream=stream.cuda_stream)
        stream.synchronize()
        return {k: bufs[k].cpu().numpy() for k in sizes}

    with _native.DeviceTrades(gpu_ctx, case.batch) as dt:
        rc, want = call(gpu_ctx, cf, cx, dt, 3, True, True)
        assert rc == 0
        for live in (tuple(sizes), ("pv", "delta_basis", "agg_basis"), ("delta_foreign", "agg_foreign"), ("delta_basis",), ("delta_foreign",)):
            out = run(dt, 3, live)
            for k, m in sizes.items():
                assert np.all(out[k][m:] == FILL), f"{k}: a guard word was written ({live})"
                if k in live:
                    assert np.array_equal(PR.bits(out[k][:m]), PR.bits(want[k].ravel())), (k, live)
                else:
                    assert np.all(out[k] == FILL), f"{k} is null in {live} and was written"
    with _native.DeviceTrades(gpu_ctx, XS.take(case.batch, 0, 0)) as empty:
        assert empty.n_trades == 0
        out = run(empty, 3, tuple(sizes))
        for k, m in sizes.items():
            if k.startswith("agg"):
                assert plus_zero(out[k][:m]) and np.all(out[k][m:] == FILL), k
            else:
                assert np.all(out[k] == FILL), k
    cf.close(); cx.close()


def test_a_trade_keeps_its_bits_at_every_position_and_launch_size(gpu_ctx):
    import torch
    case = XC.launch_case()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    sizes = XC.launch_sizes(n_cu)
    ref, ks = XR.per_trade_reference(*case.args), XR.case_ks(*case.args)
    cf, cx = device_curve(gpu_ctx, case.f_interp, case.f_host), device_curve(gpu_ctx, case.x_interp, case.x_host)
    with _native.DeviceTrades(gpu_ctx, case.batch) as dt:
        rc, base = call(gpu_ctx, cf, cx, dt, 3)
    assert rc == 0
    share = XR.rows_share(base, ref, ks, case.id)
    print(f"{case.id}: the base launch of 4 trades, share of the bound {share:.3f}; launches of {sizes} trades, {n_cu} CUs")
    assert share <= 1.0
    for size in sizes:
        book = XC.cycled_book(size)
        launches, cover = XC.route(case, n_cu=n_cu, batch=book)
        units = XC.cycled_units(size)
        assert launches == [("lite_lag", "lite_lag", units, XC.blocks_for(units, n_cu))] and np.all(cover == 1), (size, launches)
        with _native.DeviceTrades(gpu_ctx, book) as dt:
            rc, got = call(gpu_ctx, cf, cx, dt, 3)
            rc2, again = call(gpu_ctx, cf, cx, dt, 3)
        assert rc == 0 and rc2 == 0
        for k in XR.BLOCKS:
            b = PR.bits(got[k]).reshape(size, -1)
            assert np.array_equal(b, PR.bits(again[k]).reshape(size, -1)), (size, k)
            for r in range(min(4, size)):
                same = np.all(b[r::4] == PR.bits(base[k][r]).reshape(1, -1), axis=1)
                assert np.all(same), (size, k, f"copy {r + 4 * int(np.argmin(same))} of trade {r}")
    cf.close(); cx.close()


def test_refusals_leave_the_outputs_untouched(gpu_ctx):
    case = CASES[0]
    lf = [c for c in CASES if c.f_interp == PE.LF and c.f_label == "README 32"][0]
    wide = E.gbp_curve(PE.FF, 33)
    assert wide.jac.shape[1] == 33
    cf, cx = device_curve(gpu_ctx, case.f_interp, case.f_host), device_curve(gpu_ctx, case.x_interp, case.x_host)
    c_lf, c_wide = device_curve(gpu_ctx, PE.LF, lf.f_host), device_curve(gpu_ctx, PE.FF, wide)
    other = _native.Context(0)
    o_f, o_x = device_curve(other, case.f_interp, case.f_host), device_curve(other, case.x_interp, case.x_host)

    def refused(what, ctx, a, b, dt, mask, status):
        rc, out = call(ctx, a, b, dt, mask, True, True)
        assert rc == status, (what, rc)
        assert all(np.all(v == FILL) for v in out.values()), f"{what}: an output was written"

    with _native.DeviceTrades(gpu_ctx, case.batch) as dt:
        rc, _ = call(gpu_ctx, cf, cx, dt, 3, True, True)
        assert rc == 0
        refused("GAMMA", gpu_ctx, cf, cx, dt, 7, -2)
        refused("LINEAR_FWD_RATES x a log scheme", gpu_ctx, c_lf, cx, dt, 3, -2)
        refused("a log scheme x LINEAR_FWD_RATES", gpu_ctx, cf, c_lf, dt, 3, -2)
        refused("33 pillars, foreign", gpu_ctx, c_wide, cx, dt, 3, -2)
        refused("33 pillars, XCCY", gpu_ctx, cf, c_wide, dt, 3, -2)
        refused("curves of another context", gpu_ctx, o_f, o_x, dt, 3, -1)
        refused("trades of another context", other, o_f, o_x, dt, 3, -1)
    for name, batch in XC.refused_books():
        with _native.DeviceTrades(gpu_ctx, batch) as dt:
            refused(name, gpu_ctx, cf, cx, dt, 3, -2)
    for c in (cf, cx, c_lf, c_wide, o_f, o_x):
        c.close()
    other.close()


def test_the_lds_budget_from_both_sides(gpu_ctx):
    import torch
    (f, inside), (_, beyond) = XC.lds_pairs()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    case = XC.XcCase("just inside the LDS budget", PE.LZ, f"{f.times.size} knots", f, PE.FF, f"{inside.times.size} knots", inside,
                     PL.make_book(XC.geometry_trades(f, inside) + XC.structure_trades()))
    ref, book, ks = XR.per_trade_reference(*case.args), XR.book_reference(*case.args), XR.case_ks(*case.args)
    cf, cx, cb = device_curve(gpu_ctx, PE.LZ, f), device_curve(gpu_ctx, PE.FF, inside), device_curve(gpu_ctx, PE.FF, beyond)
    with _native.DeviceTrades(gpu_ctx, case.batch) as dt:
        shares = check_request(gpu_ctx, cf, cx, dt, case, 3, True, True, ref, book, ks, n_cu, case.id)
        print(f"{case.id}: {XC.xc_lds_bytes(f, inside)} bytes, share of the bound {shares[0]:.3f} per trade, {shares[1]:.3f} aggregates")
        assert max(shares) <= 1.0
        rc, out = call(gpu_ctx, cf, cb, dt, 3, True, True)
        assert rc == -2 and all(np.all(v == FILL) for v in out.values()), (rc, XC.xc_lds_bytes(f, beyond))
    for c in (cf, cx, cb):
        c.close()


def test_the_case_count():
    assert len(CASES) == N_CASES
