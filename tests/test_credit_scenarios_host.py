"""Credit scenario revaluation on the CPU (adr_credit_scenario_pv_host, the kernel's host twin: the same per-date and
per-coupon code in the same order): parity with the C oracle on rescaled batches, the reduction to adr_scenario_pv,
the formula restated in numpy from the objects' dates, independence of a scenario's row from everything around it, the
geometry edges, the refusals, and the Python layer (`compile_credit_book`, `shocked_spreads`,
`revalue_credit_on_curves`)."""
import numpy as np
import pytest

from adrates_amd import _native
from adrates_amd.market.position.scenarios import (compile_book, compile_credit_book, revalue_credit_on_curves,
                                                   revalue_on_curves, shocked_spreads)
from adrates_amd.trades.credit.bond import SPREAD_DAYS_IN_YEAR
from adrates_amd.utils import CurveTypes, InterpTypes
from adrates_amd.utils.day_count import DayCount
from adrates_amd.utils.error import LibError

from . import _credit_scenario_cases as CC
from . import _fixtures as F
from . import _scenario_cases as SC
from ._parity import REL_TOL, unit_notional_err

VD = SC.VD
BP = CC.BP
LZR = InterpTypes.LINEAR_ZERO_RATES.value


@pytest.fixture(scope="module")
def curves():
    return SC.shocked_curves()


@pytest.mark.parametrize("G", CC.BUCKET_COUNTS)
@pytest.mark.parametrize("scheme", SC.SCHEMES, ids=lambda s: s.name)
def test_host_twin_matches_the_c_oracle_on_rescaled_batches(curves, scheme, G):
    """Six books x eight (curve, spread shock) pairs per scheme and bucket count, each trade on its own notional.
    Observed maximum: 2.1e-15 per unit notional."""
    times, dfs = curves
    dz = CC.spread_shocks(dfs.shape[0], G)
    for name, case in CC.cases(G).items():
        got = CC.host_pv(scheme.value, times, dfs, dz, case)
        err = SC.worst_unit_err(got["pv"], CC.oracle_pv(scheme.value, times, dfs, dz, case), case.batch)
        print(f"{scheme.name}, G = {G}, {name}: host twin against the oracle {err:.2e}")
        assert err <= REL_TOL, (name, err)
        assert np.array_equal(got["book_pv"], SC.book_sum(got["pv"]))              # the documented order, bit for bit


@pytest.mark.parametrize("scheme", SC.SCHEMES, ids=lambda s: s.name)
def test_no_spread_reduces_to_scenario_pv(curves, scheme):
    """All z = 0 and no buckets: adr_scenario_pv's results (here bit for bit: the plain path restates its arithmetic);
    G = 0 with dz = NULL is accepted."""
    times, dfs = curves
    for name, batch in SC.books().items():
        n = batch.n_trades
        case = CC.Case(batch, np.zeros(n), np.full(n, -1, dtype=np.int32), batch.fix_tp.copy(), batch.flt_tp.copy())
        got = CC.host_pv(scheme.value, times, dfs, None, case)
        ref = _native.scenario_pv_host(scheme.value, times, dfs, batch, per_trade=True)
        err = SC.worst_unit_err(got["pv"], ref["pv"], batch)
        print(f"{scheme.name}, {name}: against adr_scenario_pv_host {err:.2e}, bit for bit {np.array_equal(got['pv'], ref['pv'])}")
        assert err <= REL_TOL
        assert np.max(np.abs(got["book_pv"] - ref["book_pv"])) <= REL_TOL * np.sum(np.abs(batch.notional))
        # buckets that nobody is in, and a z of exactly zero inside a bucket with a zero shock, change nothing either
        with_g = CC.host_pv(scheme.value, times, dfs, np.zeros((1, 4)), case)
        assert np.array_equal(with_g["pv"], got["pv"])


def _objects():
    bonds, _ = F.random_bond_book(VD, 6, seed=11)
    frns, _ = F.random_frn_book(VD, 8, seed=12)
    swaps = [F.make_swap(VD, t, c, nn, pay=p, payment_lag=lag) for t, c, nn, p, lag in
             (("5Y", 0.04, 1e7, True, 0), ("18M", 0.05, 2e6, False, 2), ("30Y", 0.035, 5e6, True, 0))]
    return swaps, bonds, frns


def test_ois_rows_of_a_mixed_book_are_the_rows_of_the_ois_alone(curves):
    """In a mixed book the OIS (z = 0, unbucketed) take the plain path: their rows are those `revalue_on_curves` gives
    the same OIS in a book without credit trades - recorded: bit for bit."""
    times, dfs = curves
    swaps, bonds, frns = _objects()
    mixed = [bonds[0], swaps[0], frns[0], swaps[1], bonds[1], frns[1], swaps[2]]
    spreads = [0.012, 0.0, 0.004, 0.0, -0.002, 0.03, 0.0]
    buckets = ["A", None, "B", None, "A", None, None]
    dz = np.stack([shocked_spreads(["A", "B"], s) for s in (0.0, 25.0, {"A": -40.0}, {"B": 300.0}, -300.0, 1.0, {"A": 5.0, "B": -5.0}, 100.0)])
    got = revalue_credit_on_curves(LZR, times, dfs, dz, mixed, spreads, buckets, VD, per_trade=True, host=True)
    assert got["labels"] == ["A", "B"] and got["pv"].shape == (8, 7)
    alone = revalue_on_curves(LZR, times, dfs, swaps, VD, per_trade=True, host=True)["pv"]
    rows = got["pv"][:, [1, 3, 6]]
    print("OIS rows of the mixed book bit for bit:", np.array_equal(rows, alone))
    assert unit_notional_err(rows, alone, np.array([s._notional for s in swaps])) <= REL_TOL


def _df(method, times, row, t):
    return CC.numpy_df(method, times, row, t)


def _bond_formula(b, method, times, row, x):
    """sum_f pay_f D(tp_f) exp(-x (dt_f - VD) / SPREAD_DAYS_IN_YEAR) over tp_f > 0, the face on the last flow."""
    dc = DayCount(b._dc_type)
    tp = np.array([dc.year_frac(VD, d)[0] for d in b._payment_dts])
    tau = np.array([(d - VD) / SPREAD_DAYS_IN_YEAR for d in b._payment_dts])
    pay = np.array([float(c) for c in b._coupon_payments])
    pay[-1] += float(b._face_value)
    live = tp > 0.0
    return float(np.sum(pay[live] * _df(method, times, row, tp[live]) * np.exp(-x * tau[live])))


def _frn_formula(f, method, times, row, x):
    """Coupons face ((D(ts) / D(te) - 1) + margin alpha) D(tp) exp(-x tp) (a first fixing replaces coupon 0's forward),
    the face at maturity, every time a year fraction from VD in the FRN's day count; a coupon paid at VD is undiscounted."""
    dc = DayCount(f._dc_type)
    yf = lambda dts: np.array([dc.year_frac(VD, d)[0] for d in dts])
    tp, ts, te = yf(f._payment_dts), yf(f._start_accrued_dts), yf(f._end_accrued_dts)
    al = np.array(f._year_fracs, dtype=np.float64)
    face, margin = float(f._face_value), float(f._quoted_margin)
    total = 0.0
    for j in range(tp.size):
        if tp[j] < 0.0:
            continue
        if j == 0 and f._first_fixing_rate is not None:
            fwd_al = f._first_fixing_rate * al[j]
        elif tp[j] == 0.0:
            fwd_al = 0.0
        else:
            fwd_al = _df(method, times, row, [ts[j]])[0] / _df(method, times, row, [te[j]])[0] - 1.0
        disc = 1.0 if tp[j] == 0.0 else _df(method, times, row, [tp[j]])[0] * np.exp(-x * tp[j])
        total += face * (fwd_al + margin * al[j]) * disc
    tm = dc.year_frac(VD, f._maturity_dt)[0]
    if tm > 0.0:
        total += face * _df(method, times, row, [tm])[0] * np.exp(-x * tm)
    return total


@pytest.mark.parametrize("scheme", SC.SCHEMES, ids=lambda s: s.name)
def test_single_bonds_and_frns_against_the_formula_in_numpy(curves, scheme):
    times, dfs = curves
    _, bonds, frns = _objects()
    dz = np.array([[0.0], [150 * BP], [-300 * BP], [1 * BP]])
    worst = 0.0
    for k, t in enumerate(bonds + frns):
        z = (-50 + 850 * k / (len(bonds) + len(frns) - 1)) * BP
        got = revalue_credit_on_curves(scheme, times, dfs[:4], dz, [t], [z], ["issuer"], VD, per_trade=True, host=True)
        formula = _bond_formula if k < len(bonds) else _frn_formula
        ref = np.array([formula(t, scheme.value, times, dfs[s], z + dz[s, 0]) for s in range(4)])
        worst = max(worst, unit_notional_err(got["pv"][:, 0], ref, float(t._face_value)))
        assert np.array_equal(got["book_pv"], got["pv"][:, 0])
    print(f"{scheme.name}: host twin against the numpy restatement {worst:.2e}")
    assert worst <= REL_TOL


def test_one_bp_of_spread_moves_a_bond_by_its_spread_dv01(curves):
    """+1 bp on every bucket lowers a bond's PV; the size is the central difference of the formula itself in numpy."""
    times, dfs = curves
    _, bonds, _ = _objects()
    dz = np.array([[0.0], [BP], [-BP]])
    for b, z in zip(bonds, (0.0, 0.01, 0.08, -0.005, 0.03, 0.002)):
        pv = revalue_credit_on_curves(LZR, times, dfs[0], dz, [b], [z], ["g"], VD, per_trade=True, host=True)["pv"][:, 0]
        f = lambda x: _bond_formula(b, LZR, times, dfs[0], x)
        face = float(b._face_value)
        assert pv[1] < pv[0] < pv[2]
        assert abs((pv[1] - pv[2]) / 2 - (f(z + BP) - f(z - BP)) / 2) <= REL_TOL * face
        dc = DayCount(b._dc_type)
        life = max((d - VD) / SPREAD_DAYS_IN_YEAR for d in b._payment_dts)
        assert 0.0 < (pv[0] - pv[1]) <= 1.001 * BP * life * pv[0]                   # at most its longest flow's duration


def test_a_row_depends_on_nothing_around_it(curves):
    """A scenario's row does not depend on S, on the other scenarios, on broadcasting or on the threads; runs repeat
    bit for bit."""
    times, dfs = curves
    G = 5
    case = CC.cases(G)["50 FRNs"]
    dz = CC.spread_shocks(8, G)
    full = CC.host_pv(LZR, times, dfs, dz, case)
    again = CC.host_pv(LZR, times, dfs, dz, case, n_threads=3)
    assert np.array_equal(full["pv"], again["pv"]) and np.array_equal(full["book_pv"], again["book_pv"])
    for s in (0, 3, 7):
        alone = CC.host_pv(LZR, times, dfs[s], dz[s], case)
        assert np.array_equal(alone["pv"][0], full["pv"][s]) and alone["book_pv"][0] == full["book_pv"][s]
    perm = [5, 2, 7, 0]
    some = CC.host_pv(LZR, times, dfs[perm], dz[perm], case)
    assert np.array_equal(some["pv"], full["pv"][perm])
    # a shared row against S copies of it, on either side
    shared_d = CC.host_pv(LZR, times, dfs[2], dz, case)
    copies_d = CC.host_pv(LZR, times, np.repeat(dfs[2:3], 8, axis=0), dz, case)
    assert np.array_equal(shared_d["pv"], copies_d["pv"]) and np.array_equal(shared_d["book_pv"], copies_d["book_pv"])
    shared_z = CC.host_pv(LZR, times, dfs, dz[4], case)
    copies_z = CC.host_pv(LZR, times, dfs, np.repeat(dz[4:5], 8, axis=0), case)
    assert np.array_equal(shared_z["pv"], copies_z["pv"]) and np.array_equal(shared_z["book_pv"], copies_z["book_pv"])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_geometry_edges_on_the_host(curves, n):
    """n across the chunk of 64 and S across the scenario group of 64: every row equals the scenario priced alone and
    book_pv the restated fixed-order sum."""
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
    dz = rng.uniform(-300 * BP, 300 * BP, (130, G))
    full = CC.host_pv(LZR, times, rows, dz, case)
    assert np.array_equal(full["book_pv"], SC.book_sum(full["pv"]))
    for S in (1, 63, 64, 65):
        part = CC.host_pv(LZR, times, rows[:S], dz[:S] if G else None, case)
        assert np.array_equal(part["pv"], full["pv"][:S]) and np.array_equal(part["book_pv"], full["book_pv"][:S])
    err = SC.worst_unit_err(full["pv"][:3], CC.oracle_pv(LZR, times, rows[:3], dz[:3], case), case.batch)
    assert err <= REL_TOL


def test_large_knot_grid_with_32_buckets(curves):
    """K = 856 knots with G = 32: on the device the discount rows no longer fit the LDS; the host twin prices the same
    call (tests/test_gpu_credit_scenarios.py runs it on the device)."""
    times, dfs, dz, case = CC.large_grid_call()
    got = CC.host_pv(LZR, times, dfs, dz, case)
    err = SC.worst_unit_err(got["pv"], CC.oracle_pv(LZR, times, dfs, dz, case), case.batch)
    print(f"K = {times.size}, G = 32: host twin against the oracle {err:.2e}")
    assert times.size == 856 and err <= REL_TOL


def test_the_host_entry_refuses_what_it_can_read():
    times, dfs, dz, case, bad = CC.refusal_inputs()
    base = dict(dfs=dfs, dz=dz, z=case.z, bucket=case.bucket, fix_tau=case.fix_tau, flt_tau=case.flt_tau)
    call = lambda kw: _native.credit_scenario_pv_host(LZR, times, kw["dfs"], kw["dz"], case.batch, kw["z"], kw["bucket"],
                                                      kw["fix_tau"], kw["flt_tau"])
    assert np.all(np.isfinite(call(base)["book_pv"]))
    for what, mutate in bad:
        kw = dict(base)
        mutate(kw)
        with pytest.raises(LibError):
            call(kw)
            pytest.fail(f"{what} was accepted")
    # a broadcast count other than 1 or S, on either side; more buckets than ADR_CREDIT_MAX_BUCKETS; a bad scheme
    G = dz.shape[1]
    assert CC.raw_host_call(LZR, times, 4, dfs, G, 4, dz, 4, case) == 0
    assert CC.raw_host_call(LZR, times, 1, dfs, G, 1, dz, 4, case) == 0
    assert CC.raw_host_call(LZR, times, 2, dfs, G, 4, dz, 4, case) < 0
    assert CC.raw_host_call(LZR, times, 4, dfs, G, 3, dz, 4, case) < 0
    assert CC.raw_host_call(LZR, times, 4, dfs, 33, 1, np.zeros(33), 4, case) < 0
    assert CC.raw_host_call(3, times, 4, dfs, G, 4, dz, 4, case) < 0
    with pytest.raises(LibError, match="shared row"):
        _native.credit_scenario_pv_host(LZR, times, dfs[:3], dz, case.batch, case.z, case.bucket, case.fix_tau, case.flt_tau)
    with pytest.raises(LibError, match="one entry per"):
        _native.credit_scenario_pv_host(LZR, times, dfs, dz, case.batch, case.z, case.bucket, case.fix_tau[:-1], case.flt_tau)


def test_compile_credit_book_and_shocked_spreads():
    swaps, bonds, frns = _objects()
    mixed = [frns[0], bonds[0], swaps[0], frns[1], bonds[1]]
    spreads = [0.004, 0.012, 0.0, 0.03, -0.002]
    book = compile_credit_book(mixed, VD, CurveTypes.GBP_OIS_SONIA, spreads, ["x", ("y", 1), None, "x", None])
    batch, const, order = compile_book(mixed, VD, CurveTypes.GBP_OIS_SONIA)
    assert np.array_equal(book.order, order) and list(order) == [2, 1, 4, 0, 3]          # OIS, bonds, FRNs
    assert np.array_equal(book.batch.fix_tp, batch.fix_tp) and np.array_equal(book.batch.flt_tp, batch.flt_tp)
    assert (book.pv_const is None) == (const is None)
    assert book.labels == ["x", ("y", 1)]
    assert np.array_equal(book.z, np.array(spreads)[order]) and list(book.bucket) == [-1, 1, -1, 0, 0]
    fo, lo = batch.fix_off, batch.flt_off
    assert np.all(book.fix_tau[fo[0]:fo[1]] == 0.0) and np.all(book.flt_tau[lo[0]:lo[1]] == 0.0)          # the OIS
    want = [(d - VD) / SPREAD_DAYS_IN_YEAR for d in bonds[0]._payment_dts]
    assert np.array_equal(book.fix_tau[fo[1]:fo[2]], want)
    assert np.array_equal(book.fix_tau[fo[3]:], batch.fix_tp[fo[3]:]) and np.array_equal(book.flt_tau[lo[3]:], batch.flt_tp[lo[3]:])
    with pytest.raises(LibError, match="OIS"):
        compile_credit_book(mixed, VD, CurveTypes.GBP_OIS_SONIA, [0.004, 0.012, 0.001, 0.03, -0.002])
    with pytest.raises(LibError, match="OIS"):
        compile_credit_book(mixed, VD, CurveTypes.GBP_OIS_SONIA, spreads, [None, None, "x", None, None])
    with pytest.raises(LibError, match="finite"):
        compile_credit_book(mixed, VD, CurveTypes.GBP_OIS_SONIA, [0.004, np.nan, 0.0, 0.03, -0.002])
    many, _ = F.random_bond_book(VD, 33, seed=2)
    assert len(compile_credit_book(many[:32], VD, CurveTypes.GBP_OIS_SONIA, 0.01, list(range(32))).labels) == 32
    with pytest.raises(LibError, match="at most 32"):
        compile_credit_book(many, VD, CurveTypes.GBP_OIS_SONIA, 0.01, list(range(33)))
    with pytest.raises(LibError, match="carries no dates"):
        compile_credit_book(batch, VD, CurveTypes.GBP_OIS_SONIA, 0.0)
    assert np.array_equal(shocked_spreads(["a", "b", "c"], 25.0), np.full(3, 25e-4))
    assert np.allclose(shocked_spreads(["a", "b", "c"], {"c": -10.0, "a": 1.0}), [1e-4, 0.0, -10e-4], rtol=0, atol=1e-18)
    with pytest.raises(LibError, match="no bucket named"):
        shocked_spreads(["a", "b"], {"d": 1.0})
    # an FRN coupon paid at the value time keeps its undiscounted amount whatever the spread
    times, dfs = SC.shocked_curves()
    for f in frns:
        a = revalue_credit_on_curves(LZR, times, dfs[:2], None, [f], [0.0], None, VD, per_trade=True, host=True)["pv"]
        b = revalue_on_curves(LZR, times, dfs[:2], [f], VD, per_trade=True, host=True)["pv"]
        assert np.array_equal(a, b)
