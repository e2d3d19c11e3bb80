"""Inflation sub-book Greeks on the CPU: the host twin adr_yoy_subbook_ladders_host against the torch oracle
(`_yoy_ladder_cases.reference`), against the entries it must agree with (adr_subbook_ladders_host, adr_yoy_risk_host), against
central differences and against full revaluation (adr_yoy_scenario_subbook_pv_host).  No GPU needed.

Observed worst figures (share of a desk's sum of absolute per-swap entries; the bound is 1e-10): geometry book 3.1e-15 over
the six scheme pairs, edge book 1.3e-15, shapes 1.2e-14 (P_i = 1), breakeven block against adr_yoy_risk_host 2.2e-15.  Cross
block against central differences at +-1 bp: 4.7e-8 of the desks' absolute sums, derived bound 1.4e-5.  Residual ratios under
joint shocks, oracle-derived ladders and host twin alike: 7.606 - 8.066 with the cross block, 3.967 - 4.007 without it
(DESIGN.md section 23)."""
import numpy as np
import pytest

from adrates_amd import _native
from adrates_amd.utils.error import LibError
from adrates_amd.utils.global_types import RequestTypes

from . import _ladder_edge_cases as LE
from . import _ladder_pnl_cases as C
from . import _sub_book_ladder_cases as L
from . import _yoy_cases as YC
from . import _yoy_ladder_cases as Y

GEO_OFF = Y.offsets(Y.GEOMETRY_SIZES)


def _case(interp, im, P=32, P_i=12, book=None, sizes=Y.GEOMETRY_SIZES):
    curve, host = Y.disc_curve(interp, P)
    book = book or Y.geometry_book()
    infl = Y.infl_curve(P_i, im)
    return host, infl, book, Y.offsets(sizes), Y.Entries(interp.value, host)


@pytest.mark.parametrize("im", Y.INFL_SCHEMES)
@pytest.mark.parametrize("interp", Y.SCHEMES)
def test_geometry_book_against_the_oracle(interp, im):
    """Desks of 1, 63, 64, 0, 65, 129, 0 swaps, the three discount schemes times the two inflation schemes: every row within
    1e-10 of the oracle's, the layout, and the bit contract (a desk alone, permuted desks, a second call)."""
    host, infl, book, sub_off, E = _case(interp, im)
    ref = Y.reference(interp.value, host, infl, book, key=("geometry", interp, im))
    got = E(infl, book.fixed, book.coupons, sub_off)
    worst = L.desk_errors(got, ref, sub_off)
    print(f"geometry book, {interp.name} / {YC.NAMES[im]}: {worst:.2e}")
    assert worst <= Y.TOL
    Y.check_layout(got, 32, 12)
    Y.check_contract(E, infl, book, sub_off, got)


@pytest.mark.parametrize("interp", Y.SCHEMES)
def test_edge_book_against_the_oracle(interp):
    """The hand-made swaps: one coupon, passes of more than 64 coupons and of more than 64 fixed flows, knot 0 dropped, te on
    a pillar, merged slots, a coefficient that cancels, dead coupons and flows at tp == 0 and before, tp on a discount knot
    and beyond the last, an empty swap, a pair that cancels (its desk's row is 0 to the bound's scale)."""
    curve, host = Y.disc_curve(interp)
    book, sub_off = Y.edge_book(float(host.times[40]))
    for im in Y.INFL_SCHEMES:
        infl = Y.infl_curve(5, im)
        E = Y.Entries(interp.value, host)
        ref = Y.reference(interp.value, host, infl, book)
        got = E(infl, book.fixed, book.coupons, sub_off)
        worst = L.desk_errors(got, ref, sub_off)
        print(f"edge book, {interp.name} / {YC.NAMES[im]}: {worst:.2e}")
        assert worst <= Y.TOL
        Y.check_layout(got, 32, 5)
        Y.check_contract(E, infl, book, sub_off, got)
        each = E(infl, book.fixed, book.coupons, np.arange(book.n + 1))         # one desk per swap
        assert L.desk_errors(each, ref, np.arange(book.n + 1)) <= Y.TOL
        dead = [book.names.index(k) for k in ("tp == 0: dead coupon and dead fixed flow", "no coupons, no flows")]
        assert not np.any(each["ladders"][dead]) and not np.any(np.signbit(each["ladders"][dead]))


@pytest.mark.parametrize("P", [17, 32, 40])
@pytest.mark.parametrize("P_i", [1, 12, 64])
def test_shapes(P, P_i):
    interp = Y.SCHEMES[(P + P_i) % 3]
    im = Y.INFL_SCHEMES[P_i % 2]
    host, infl, book, sub_off, E = _case(interp, im, P, P_i, Y.small_book(), Y.SMALL_SIZES)
    ref = Y.reference(interp.value, host, infl, book)
    got = E(infl, book.fixed, book.coupons, sub_off)
    worst = L.desk_errors(got, ref, sub_off)
    print(f"P_d = {P}, P_i = {P_i}, {interp.name} / {YC.NAMES[im]}: {worst:.2e}")
    assert worst <= Y.TOL
    Y.check_layout(got, P, P_i)


def test_requests_leave_blocks_zero():
    interp = Y.SCHEMES[0]
    host, infl, book, sub_off, E = _case(interp, YC.LZ, book=Y.small_book(), sizes=Y.SMALL_SIZES)
    full = E(infl, book.fixed, book.coupons, sub_off)
    d_only = E(infl, book.fixed, book.coupons, sub_off, hess=False, want_gamma=False)
    v_only = E(infl, book.fixed, book.coupons, sub_off, hess=False, want_delta=False, want_gamma=False)
    Y.check_layout(d_only, 32, 12, want_gamma=False)
    Y.check_layout(v_only, 32, 12, want_delta=False, want_gamma=False)
    ref = Y.reference(interp.value, host, infl, book)
    zero_gamma = dict(ref, gamma=np.zeros_like(ref["gamma"]))
    assert L.desk_errors(dict(d_only, gamma=full["gamma"] * 0.0), dict(zero_gamma), sub_off) <= Y.TOL
    assert np.array_equal(Y.bits(v_only["pv"]), Y.bits(d_only["pv"])) and np.array_equal(Y.bits(v_only["pv"]), Y.bits(full["pv"]))
    assert Y.between(d_only, dict(full, gamma=d_only["gamma"]), ref, sub_off) <= Y.TOL


@pytest.mark.parametrize("interp", Y.SCHEMES)
def test_discount_block_has_the_bits_of_the_fixed_flow_batch(interp):
    """The discount block and the PV against adr_subbook_ladders_host on the batch that holds, per swap, its fixed flows
    followed by its coupons' amounts (adr_yoy_risk_host's, the same code) as fixed flows: bit for bit."""
    host, infl, book, sub_off, E = _case(interp, YC.LZ)
    got = E(infl, book.fixed, book.coupons, sub_off)
    amount = _native.yoy_risk_host((interp.value, host.times, host.dfs), infl, book.coupons, 0)["amount"]
    want = _native.subbook_ladders_host(interp.value, host.times, host.dfs, host.jac, host.hess,
                                        Y.equivalent_batch(book.fixed, book.coupons, amount), sub_off)
    P = 32
    assert np.array_equal(Y.bits(got["pv"]), Y.bits(want["pv"]))
    assert np.array_equal(Y.bits(got["delta"][:, :P]), Y.bits(want["delta"]))
    assert np.array_equal(Y.bits(got["gamma"][:, :P, :P]), Y.bits(want["gamma"]))


@pytest.mark.parametrize("im", Y.INFL_SCHEMES)
def test_inflation_block_against_the_aggregate_of_yoy_risk(im):
    """The breakeven delta and gamma of every desk against adr_yoy_risk_host's aggregate on the desk alone, within 1e-10 of
    the desk's absolute per-swap sums (the two sum in different orders and scale at different points)."""
    interp = Y.SCHEMES[0]
    host, infl, book, sub_off, E = _case(interp, im)
    got = E(infl, book.fixed, book.coupons, sub_off)
    P, worst = 32, 0.0
    for j, (lo, hi) in enumerate(zip(sub_off[:-1], sub_off[1:])):
        if lo == hi:
            continue
        _, coupons = Y.take(book.fixed, book.coupons, int(lo), int(hi))
        r = _native.yoy_risk_host((interp.value, host.times, host.dfs), infl, coupons, 7, per_swap=True, aggregate=True)
        for mine, agg, per in ((got["delta"][j, P:], r["agg_delta"], r["delta"]), (got["gamma"][j, P:, P:], r["agg_gamma"], r["gamma"])):
            scale = float(np.max(np.abs(per).sum(0)))
            if scale == 0.0:                                   # a desk without a live coupon
                assert not np.any(mine) and not np.any(agg)
                continue
            worst = max(worst, float(np.max(np.abs(mine - agg))) / scale)
    print(f"inflation block against adr_yoy_risk_host, {YC.NAMES[im]}: {worst:.2e}")
    assert worst <= Y.TOL


def test_cross_block_against_central_differences():
    """Every cross entry of the geometry desks against central differences of adr_yoy_scenario_subbook_pv_host at joint bumps
    of +-1 bp of one par quote and one breakeven rate, (PV++ - PV+- - PV-+ + PV--) / 4 per bp^2.

    Tolerance: every term of the PV is an amount times exp of a form that is linear in the zero rates and in ln(1 + b) with
    coefficients of at most T = 64 years (the longest date of the book, 44 years, with room for the bootstrap's weights), so
    each further derivative in either rate costs at most a factor T; the truncation term of the central difference,
    h^2 / 6 (d4 / dr3 db + d4 / dr db3), is then at most (h T)^2 / 3 = 1.4e-5 of the desk's sum of absolute per-swap cross
    entries (h = 1e-4).  The four PV sums carry n 2^-53 of the desk's sum of |PV| each (n swaps), divided by 4 h^2 in bp."""
    interp = Y.SCHEMES[0]
    curve, host = Y.disc_curve(interp)
    infl = Y.infl_curve(12, YC.LZ)
    im, T, b = infl
    book, sub_off = Y.geometry_book(), GEO_OFF
    ref = Y.reference(interp.value, host, infl, book, key=("geometry", interp, YC.LZ))
    got = Y.Entries(interp.value, host)(infl, book.fixed, book.coupons, sub_off)
    P, Pi = 32, 12
    bumps = [s * np.eye(P)[p] for p in range(P) for s in (1.0, -1.0)]
    times, dfs = C.shocked_dfs(curve, bumps)                                      # rows 2 p (+), 2 p + 1 (-), the base last
    d_rows = np.array([dfs[2 * p + sd] for p in range(P) for k in range(Pi) for sd in (0, 0, 1, 1)])
    b_rows = np.array([b + sb * 1e-4 * np.eye(Pi)[k] for p in range(P) for k in range(Pi) for sb in (1.0, -1.0, 1.0, -1.0)])
    pv = _native.yoy_scenario_subbook_pv_host(interp.value, times, d_rows, im, T, b_rows, book.fixed, book.coupons, sub_off,
                                              per_trade=True)
    sub = pv["sub_pv"].reshape(len(sub_off) - 1, P, Pi, 4)
    fd = (sub[..., 0] - sub[..., 1] - sub[..., 2] + sub[..., 3]) / 4.0             # [B, P_d, P_i]
    worst = 0.0
    for j, (lo, hi) in enumerate(zip(sub_off[:-1], sub_off[1:])):
        if lo == hi:
            assert not np.any(fd[j])
            continue
        scale = float(np.max(np.abs(ref["gamma"][lo:hi, :P, P:]).sum(0)))
        rounding = (hi - lo) * 2.0 ** -53 * float(np.max(np.abs(pv["pv"][:, lo:hi]).sum(1)))
        tol = (1e-4 * 64.0) ** 2 / 3.0 * scale + rounding
        err = float(np.max(np.abs(fd[j] - got["gamma"][j, :P, P:])))
        assert scale > 0.0 and err <= tol, (j, err, tol)
        worst = max(worst, err / scale)
    print(f"cross block against central differences: {worst:.2e} of the desks' absolute sums (bound 1.4e-05 plus rounding)")


# (desk label, direction) pairs whose REFERENCE leaves a band (`_yoy_ladder_cases.check_bands` on the oracle-derived ladders):
# none on this book.
EXPLAIN_DROPPED = ()


@pytest.mark.parametrize("source", ["oracle", "host twin"])
def test_bands_against_full_revaluation(source):
    """A two-desk YoY book under joint shocks h (u, v), h = 4, 8, 16 bp (u: the three curve directions, v: all ones or a ramp
    over the inflation pillars): the residual of the delta-gamma P&L against adr_yoy_scenario_subbook_pv_host is third order
    with the cross block (ratio under doubling in [7, 9]) and second order without it ([3, 5]) - the cross term is right and
    needed.  First on the oracle-derived ladders (which fix the bands and the dropped desk-directions), then on the twin's."""
    from adrates_amd.market.position.inflation_engine import inflation_inputs, yoy_curves
    from adrates_amd.market.position.ladder_pnl import augmented_ladder_pnl, yoy_shock_matrix_bp
    from adrates_amd.market.position.scenarios import split_yoy_sub_books, yoy_book_arrays
    model, swaps, keys = Y.explain_book()
    disc, infl_c, _, _ = yoy_curves(model, swaps[0]._inflation_index._currency, swaps[0]._inflation_index._index_type.name)
    interp = disc._interp_type
    host = L.curve_arrays(interp)
    im, T, b = inflation_inputs(infl_c)
    sb = split_yoy_sub_books(*yoy_book_arrays(swaps, model.value_dt), keys)
    P, Pi = host.jac.shape[1], T.size
    Q = P + Pi
    x, y = Y.joint_shock_rows(P, Pi)
    times, dfs = C.shocked_dfs(disc, x[:-1])
    full = _native.yoy_scenario_subbook_pv_host(interp.value, times, dfs, im, T, np.vstack([b + y[:-1] * 1e-4, b[None, :]]),
                                                sb.fixed, sb.coupons, sb.sub_off)["sub_pv"]
    full = full - full[:, -1:]
    if source == "oracle":
        book = Y.Book.__new__(Y.Book)
        book.fixed, book.coupons, book.n = sb.fixed, sb.coupons, len(swaps)
        rows = Y.desk_rows(Y.reference(interp.value, host, (im, T, b), book), sb.sub_off)
    else:
        rows = Y.Entries(interp.value, host)((im, T, b), sb.fixed, sb.coupons, sb.sub_off)["ladders"]
    shocks = yoy_shock_matrix_bp(x, b[None, :] + y * 1e-4, b)
    assert np.allclose(shocks[:, P:], y, rtol=0.0, atol=1e-9) and np.array_equal(shocks[:, :P], x)
    exact = yoy_shock_matrix_bp(x, infl_shocks_bp=y)
    with_c = augmented_ladder_pnl(rows, exact, parts=True, host=True)
    without = augmented_ladder_pnl(Y.without_cross(rows, P, Q), exact, parts=True, host=True)
    Y.check_bands(sb.labels, full, with_c["delta_pnl"], with_c["gamma_pnl"], f"{source}, cross", True, EXPLAIN_DROPPED)
    Y.check_bands(sb.labels, full, without["delta_pnl"], without["gamma_pnl"], f"{source}, no cross", False, EXPLAIN_DROPPED)


def test_refusals():
    interp = Y.SCHEMES[0]
    host, infl, book, sub_off, E = _case(interp, YC.LZ, book=Y.small_book(), sizes=Y.SMALL_SIZES)
    im, T, b = infl

    def refused(code, match, infl=infl, fixed=book.fixed, coupons=book.coupons, off=sub_off, **kw):
        with pytest.raises(LibError, match=match) as e:
            E(infl, fixed, coupons, off, **kw)
        assert e.value.status == code, (e.value.status, match)

    refused(-2, "inflation scheme must be", infl=(YC.LF, T, b))
    T65, b65 = YC.pillars(64)[0], YC.pillars(64)[1]
    refused(-2, "1 .. ADR_YOY_MAX_PILLARS", infl=(YC.LZ, np.append(T65, 41.0), np.append(b65, 0.03)))
    refused(-1, "GAMMA requested but hess is NULL", hess=False)
    refused(-1, "pillar times must be increasing", infl=(YC.LZ, T[::-1].copy(), b))
    bad = dict(book.coupons, scale=book.coupons["scale"].copy())
    bad["scale"][3] = np.nan
    refused(-1, "coupon fields must be finite", coupons=bad)
    off = book.coupons["cpn_off"].copy()
    off[5] = off[6] + 1
    refused(-1, "offsets must be non-decreasing", coupons=dict(book.coupons, cpn_off=off))
    n = book.n
    for bad_off, msg in (([0, 5, 3, n], r"decreases at sub-book 1 \(5 \.\. 3\)"), ([1, 5, n], "sub-book 0 starts at 1"),
                         ([0, 5, n - 1], f"sub-book 1 ends at {n - 1}"), ([0, 5, n + 1], f"sub-book 1 ends at {n + 1}")):
        refused(-1, msg, off=bad_off)
    # a curve pair whose tables for one wave do not fit the LDS: 300 knots x 64 inflation pillars
    big = LE.lookup_curve(np.linspace(0.0, 60.0, 300))
    with pytest.raises(LibError, match=r"300 knots x 64 inflation pillars\) do not fit the 160 KiB LDS") as e:
        Y.Entries(interp.value, big)((YC.LZ, T65, b65), book.fixed, book.coupons, sub_off)
    assert e.value.status == -2
    Y.Entries(interp.value, big)((YC.LZ, T65, b65), book.fixed, book.coupons, sub_off, want_gamma=False)   # [w, di] fits


def test_python_surface_on_the_host():
    """`price_yoy_sub_books` on swap objects against the entry on the compiled book; `YoYBook.compute_sub_books` and
    `pnl_delta_gamma_sub_books` on the host route; `yoy_shock_matrix_bp`'s checks."""
    from adrates_amd.market.position.engine import Engine
    from adrates_amd.market.position.inflation_engine import inflation_inputs
    from adrates_amd.market.position.ladder_pnl import augmented_ladder_pnl, yoy_shock_matrix_bp
    from adrates_amd.market.position.scenarios import split_yoy_sub_books, yoy_book_arrays
    from adrates_amd.market.position.sub_book_ladders import price_yoy_sub_books
    from adrates_amd.market.position.yoy_book import YoYBook
    model, swaps, keys = Y.explain_book()
    yb = YoYBook(swaps, model)
    reqs = {RequestTypes.VALUE, RequestTypes.DELTA, RequestTypes.GAMMA}
    res = price_yoy_sub_books(Engine(model), yb.curve, yb.inflation_curve, swaps, keys, reqs, host=True)
    host = L.curve_arrays(yb.curve._interp_type)
    infl = inflation_inputs(yb.inflation_curve)
    sb = split_yoy_sub_books(*yoy_book_arrays(swaps, model.value_dt), keys)
    raw = Y.Entries(yb.curve._interp_type.value, host)(infl, sb.fixed, sb.coupons, sb.sub_off)
    P, Pi = host.jac.shape[1], infl[1].size
    assert res["labels"] == ["linkers", "rates"] and len(res["tenors"]) == P and len(res["infl_tenors"]) == Pi
    assert all(np.array_equal(Y.bits(res[k]), Y.bits(raw[k])) for k in ("pv", "delta", "gamma", "ladders"))
    assert Y.same_bits(yb.compute_sub_books(reqs, keys, host=True), res)
    v_only = yb.compute_sub_books({RequestTypes.VALUE}, keys, host=True)
    assert not np.any(v_only["delta"]) and not np.any(v_only["gamma"]) and np.array_equal(v_only["pv"], res["pv"])
    steps = [4.0, 8.0, 0.0]
    dg = yb.pnl_delta_gamma_sub_books(keys, inflation_shocks=steps, parts=True, host=True)
    shocks = yoy_shock_matrix_bp(np.zeros((1, P)), infl_shocks_bp=np.outer(steps, np.ones(Pi)))
    want = augmented_ladder_pnl(res["ladders"], shocks, parts=True, host=True)
    assert all(np.array_equal(Y.bits(dg[k]), Y.bits(want[k])) for k in ("pnl", "delta_pnl", "gamma_pnl"))
    assert np.all(dg["pnl"][:, 2] == 0.0)
    no_cross = yb.pnl_delta_gamma_sub_books(keys, inflation_shocks=steps, cross=False, host=True)["pnl"]
    assert np.array_equal(Y.bits(no_cross), Y.bits(dg["pnl"]))                    # no discount shock: the cross block is idle
    with pytest.raises(LibError, match="keys needs one entry per swap"):
        yb.compute_sub_books(reqs, keys[:-1], host=True)
    with pytest.raises(LibError, match="VALUE, DELTA or GAMMA"):
        yb.compute_sub_books(set(), keys, host=True)
    with pytest.raises(LibError, match="breakevens \\(with b0\\) or infl_shocks_bp"):
        yoy_shock_matrix_bp(np.zeros((1, P)))
    with pytest.raises(LibError, match="one shared row or one row per"):
        yoy_shock_matrix_bp(np.zeros((2, P)), infl_shocks_bp=np.zeros((3, Pi)))
