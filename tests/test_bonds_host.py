"""Fixed-rate bonds on the host: schedules, the reference's bond properties, the scalar solvers against an independent
high-precision restatement, the fixed-flows batch against the C oracle, and adr_bond_measures_host against the scalar
methods.  No GPU."""
import mpmath
import numpy as np
import pytest

from adrates_amd import _native
from adrates_amd.market.position.bond_book import BondBook
from adrates_amd.trades.compiler import compile_bonds
from adrates_amd.trades.credit.bond import Bond
from adrates_amd.market.curves.curve_tables import build_engine_curve
from adrates_amd.utils import (CurrencyTypes, Date, DayCountTypes, FrequencyTypes, InstrumentTypes, InterpTypes,
                               LibError)
from adrates_amd.utils.helpers import times_from_dates
from oracle import cavour_oracle as O
from oracle import port

from . import _fixtures as F
from ._bonds import random_book, scalar_measures

GBP = CurrencyTypes.GBP
SCHEMES = (InterpTypes.FLAT_FWD_RATES, InterpTypes.LINEAR_FWD_RATES, InterpTypes.LINEAR_ZERO_RATES)
VD = F.README_VALUE_DT        # 30 Apr 2024


# ------------------------------------------------------------------------------------------------ schedules
def test_semi_annual_act365f_schedule():
    b = Bond(Date(15, 1, 2024), "2Y", 0.05, FrequencyTypes.SEMI_ANNUAL, DayCountTypes.ACT_365F, GBP)
    assert b.derivative_type == InstrumentTypes.BOND and b._num_coupons == 4
    assert b._payment_dts == [Date(15, 7, 2024), Date(15, 1, 2025), Date(15, 7, 2025), Date(15, 1, 2026)]
    days = [182, 184, 181, 184]
    assert b._year_fracs == [d / 365 for d in days]
    assert b._coupon_payments == [d / 365 * 0.05 * 100.0 for d in days]
    assert b._principal_payments == [0.0, 0.0, 0.0, 100.0]
    # 30 Apr 2024 lies in the first period: 106 days accrued on the face
    assert b.accrued_interest(VD) == 106 / 365 * 0.05 * 100.0


def test_annual_thirty360_end_of_month_schedule():
    b = Bond(Date(28, 2, 2023), "3Y", 0.04, FrequencyTypes.ANNUAL, DayCountTypes.THIRTY_360_BOND, GBP, end_of_month=True)
    # end of month rolls to 29 Feb 2024; 28 Feb 2026 is a Saturday and follows to Monday 2 Mar
    assert b._payment_dts == [Date(29, 2, 2024), Date(28, 2, 2025), Date(2, 3, 2026)]
    assert b._year_fracs == [361 / 360, 359 / 360, 364 / 360]
    assert b._coupon_payments == [f * 0.04 * 100.0 for f in (361 / 360, 359 / 360, 364 / 360)]


def test_payment_lag_moves_payment_not_accrual():
    b = Bond(Date(15, 1, 2024), "1Y", 0.05, FrequencyTypes.ANNUAL, DayCountTypes.ACT_365F, GBP, payment_lag=3)
    assert b._accrual_end_dts == [Date(15, 1, 2025)]
    assert b._payment_dts == [Date(20, 1, 2025)]          # Wed + 3 business days over a weekend
    assert b._year_fracs == [366 / 365]


def test_equal_principal_amortizer():
    assert Bond.generate_equal_principal_schedule(100.0, 4) == [75.0, 50.0, 25.0, 0.0]
    b = Bond(Date(15, 1, 2024), "2Y", 0.06, FrequencyTypes.ANNUAL, DayCountTypes.ACT_365F, GBP,
             amortization_schedule=[50.0, 0.0])
    assert b._principal_schedule == [100.0, 50.0, 0.0]
    assert b._principal_payments == [50.0, 50.0]
    assert b._coupon_payments == [366 / 365 * 0.06 * 100.0, 365 / 365 * 0.06 * 50.0]


def test_annuity_amortizer():
    sched = Bond.generate_annuity_schedule(100.0, 2, 0.10, FrequencyTypes.ANNUAL)
    payment = 100.0 * 0.1 * 1.21 / 0.21                    # 57.619...
    assert sched[0] == pytest.approx(100.0 - (payment - 10.0), abs=1e-12)
    assert sched[1] == pytest.approx(0.0, abs=1e-12)
    semi = Bond.generate_annuity_schedule(100.0, 4, 0.08, FrequencyTypes.SEMI_ANNUAL)   # 4% per period
    assert semi[0] == pytest.approx(100.0 - (100.0 * 0.04 / (1 - 1.04 ** -4) - 4.0), abs=1e-12)
    assert Bond.generate_annuity_schedule(100.0, 4, 0.0, FrequencyTypes.ANNUAL) == [75.0, 50.0, 25.0, 0.0]
    with pytest.raises(LibError):
        Bond.generate_annuity_schedule(100.0, 0, 0.05, FrequencyTypes.ANNUAL)


def test_zero_coupon_bond():
    for b in (Bond(Date(15, 1, 2024), "5Y", 0.0, FrequencyTypes.ANNUAL, DayCountTypes.ACT_365F, GBP),
              Bond(Date(15, 1, 2024), "5Y", 0.05, FrequencyTypes.ZERO, DayCountTypes.ACT_365F, GBP)):
        assert b._payment_dts == [Date(15, 1, 2029)] and b._coupon_payments == [0.0]
        assert b._principal_payments == [100.0] and b._num_coupons == 0
        assert b.accrued_interest(VD) == 0.0 and b.current_yield() == 0.0


def test_bad_amortization_length_raises():
    with pytest.raises(LibError):
        Bond(Date(15, 1, 2024), "2Y", 0.06, FrequencyTypes.ANNUAL, DayCountTypes.ACT_365F, GBP,
             amortization_schedule=[50.0, 25.0, 0.0])
    with pytest.raises(LibError):
        Bond(Date(15, 1, 2024), Date(15, 1, 2024), 0.06, FrequencyTypes.ANNUAL, DayCountTypes.ACT_365F, GBP)


# ------------------------------------------------------------------------------------------------ properties
@pytest.fixture(scope="module")
def gbp():
    return F.gbp_model()


def test_reference_bond_properties(gbp):
    curve = gbp.curves.GBP_OIS_SONIA
    b5 = Bond(VD, "5Y", 0.05, FrequencyTypes.ANNUAL, DayCountTypes.ACT_365F, GBP)
    assert 95.0 < b5.value(VD, curve) < 105.0                            # coupon near the curve: near par
    seasoned = Bond(Date(15, 1, 2024), "5Y", 0.05, FrequencyTypes.SEMI_ANNUAL, DayCountTypes.ACT_365F, GBP)
    assert seasoned.dirty_price(VD, curve) >= seasoned.clean_price(VD, curve)
    durations = [Bond(VD, t, 0.05, FrequencyTypes.ANNUAL, DayCountTypes.ACT_365F, GBP).duration(VD, curve)
                 for t in ("2Y", "5Y", "10Y", "30Y")]
    assert 0.0 < durations[1] < 5.0 and all(a < b for a, b in zip(durations, durations[1:]))
    # dv01 as the reference's test defines it: the value after a 1bp rise of the quotes minus the value before
    up = gbp.scenario("GBP_OIS_SONIA", shock=0.01).curves.GBP_OIS_SONIA
    dv01 = b5.value(VD, up) - b5.value(VD, curve)
    assert -1.0 < dv01 < -0.001
    # the z-spread dv01 / cs01 of the bond methods are positive and equal
    assert b5.dv01(VD, curve) > 0.0 and b5.cs01(VD, curve, 0.01) == b5.dv01(VD, curve, 0.01)
    assert b5.duration(VD, curve, "modified") == b5.duration(VD, curve, "macaulay")
    with pytest.raises(ValueError):
        b5.duration(VD, curve, "effective")


def test_z_spread_reprices_and_spreads(gbp):
    curve = gbp.curves.GBP_OIS_SONIA
    b = Bond(Date(15, 1, 2024), "7Y", 0.045, FrequencyTypes.SEMI_ANNUAL, DayCountTypes.ACT_365F, GBP)
    z = b.z_spread(VD, curve, 97.25)
    assert b.clean_price(VD, curve, z, VD) == pytest.approx(97.25, abs=1e-9)
    y = b.yield_to_maturity(VD, 97.25)
    assert b.i_spread(VD, curve, 97.25) == y - curve.zero_rate(b._maturity_dt, b._freq_type, b._dc_type)
    assert b.g_spread(VD, curve, 97.25) == b.i_spread(VD, curve, 97.25)


# ------------------------------------------------------------------------------------------------ solvers vs mpmath
def _mp_z(bond, curve, settle, clean):
    """z from an independent 30-digit restatement of `Bond.value` on the curve's node discount factors."""
    acc = mpmath.mpf(bond.accrued_interest(settle)) / bond._face_value * 100
    target = (mpmath.mpf(clean) + acc) / 100 * bond._face_value
    ds = mpmath.mpf(curve.df(settle))
    flows = []
    for i, dt in enumerate(bond._payment_dts):
        if dt > settle:
            amt = mpmath.mpf(bond._coupon_payments[i]) + max(mpmath.mpf(bond._principal_payments[i]), 0)
            flows.append((amt * mpmath.mpf(curve.df(dt)) / ds, mpmath.mpf(dt - settle) / mpmath.mpf("365.25")))
    return mpmath.findroot(lambda z: sum(a * mpmath.exp(-z * t) for a, t in flows) - target, mpmath.mpf("0.01"))


def _mp_ytm(bond, settle, clean):
    acc = mpmath.mpf(bond.accrued_interest(settle)) / bond._face_value * 100
    target = (mpmath.mpf(clean) + acc) / 100 * bond._face_value
    flows = [(mpmath.mpf(bond._coupon_payments[i]), mpmath.mpf(dt - settle) / mpmath.mpf("365.25"))
             for i, dt in enumerate(bond._payment_dts) if dt > settle]
    flows.append((mpmath.mpf(bond._face_value), mpmath.mpf(bond._maturity_dt - settle) / mpmath.mpf("365.25")))
    return mpmath.findroot(lambda y: sum(a * mpmath.exp(-y * t) for a, t in flows) - target, mpmath.mpf("0.05"))


@pytest.mark.parametrize("scheme", SCHEMES, ids=lambda s: s.name)
def test_host_solvers_match_mpmath(scheme):
    curve = F.gbp_model(interp=scheme).curves.GBP_OIS_SONIA
    cases = [(Bond(Date(15, 1, 2024), "10Y", 0.04, FrequencyTypes.SEMI_ANNUAL, DayCountTypes.ACT_365F, GBP), 96.5),
             (Bond(Date(28, 2, 2023), "30Y", 0.05, FrequencyTypes.ANNUAL, DayCountTypes.THIRTY_360_BOND, GBP,
                   end_of_month=True), 104.0),
             (Bond(Date(1, 5, 2024), "5Y", 0.0, FrequencyTypes.ANNUAL, DayCountTypes.ACT_365F, GBP), 81.0)]
    for bond, clean in cases:
        with mpmath.workdps(30):                 # local precision: other modules rely on mpmath's global setting
            z, y = float(_mp_z(bond, curve, VD, clean)), float(_mp_ytm(bond, VD, clean))
        assert abs(bond.z_spread(VD, curve, clean) - z) < 1e-11
        assert abs(bond.yield_to_maturity(VD, clean) - y) < 1e-11


# ------------------------------------------------------------------------------------------------ face folding
@pytest.mark.parametrize("scheme", SCHEMES, ids=lambda s: s.name)
def test_compile_bonds_matches_fixed_leg_with_principal(scheme):
    curve = F.gbp_model(interp=scheme).curves.GBP_OIS_SONIA
    bonds = [Bond(Date(15, 1, 2024), "10Y", 0.04, FrequencyTypes.SEMI_ANNUAL, DayCountTypes.ACT_365F, GBP),
             Bond(Date(1, 5, 2024), "5Y", 0.0, FrequencyTypes.ANNUAL, DayCountTypes.ACT_365F, GBP),
             Bond(Date(15, 1, 2020), "6Y", 0.03, FrequencyTypes.QUARTERLY, DayCountTypes.ACT_360, GBP,
                  face_value=1e6, amortization_schedule=Bond.generate_equal_principal_schedule(1e6, 24)),
             Bond(Date(15, 1, 2024), "3Y", 0.05, FrequencyTypes.ANNUAL, DayCountTypes.ACT_365F, GBP, payment_lag=2),
             Bond(Date(1, 5, 2024), "50Y", 0.03, FrequencyTypes.MONTHLY, DayCountTypes.ACT_365F, GBP)]
    batch = compile_bonds(bonds, VD)
    assert batch.n_trades == 5 and batch.flt_tp.size == 0 and np.all(batch.flt_off == 0)
    assert np.array_equal(batch.notional, [b._face_value for b in bonds])
    assert int(batch.fix_off[-1]) == sum(len(b._payment_dts) for b in bonds)
    host = build_engine_curve(curve.swap_rates, curve.swap_times, curve.year_fracs)
    method = curve._interp_type.value
    got = port.price(method, host.times, host.dfs, host.jac, host.hess, batch)
    cache = O.cached_curve(curve.swap_rates, curve.swap_times, curve.year_fracs)
    for i, b in enumerate(bonds):
        tp = times_from_dates(b._payment_dts, VD, b._dc_type)
        ref = O._leg_analytics(lambda d: O.price_fixed_leg(d, cache["times"], method, tp, b._coupon_payments,
                                                           b._face_value, 1.0), cache)
        face = b._face_value
        assert abs(got["pv"][i] - ref["value"]) / face < 1e-10
        assert np.max(np.abs(got["delta"][i] - ref["delta"])) / face < 1e-10
        assert np.max(np.abs(got["gamma"][i] - ref["gamma"])) / face < 1e-10
    # the 600-flow bond goes through the launch plan like any other trade
    _, cover = _native.route_host(method, host.times, host.dfs, host.jac, host.hess, batch, 7)
    assert np.all(cover == 1)
    with pytest.raises(LibError):
        compile_bonds([F.make_swap(VD, "2Y", 0.04)], VD)


# ------------------------------------------------------------------------------------------------ adr_bond_measures_host
TOL_ABS = {"z": 1e-11, "ytm": 1e-11}
TOL_REL = {"dirty": 1e-10, "clean": 1e-10, "duration": 1e-9, "convexity": 1e-9, "dv01": 1e-9}


def check_against_scalar(got, i, ref):
    for k, tol in TOL_ABS.items():
        assert abs(got[k][i] - ref[k]) <= tol, (i, k, got[k][i], ref[k])
    for k, tol in TOL_REL.items():
        assert abs(got[k][i] - ref[k]) <= tol * abs(ref[k]), (i, k, got[k][i], ref[k])


@pytest.fixture(scope="module")
def random_book_2000(gbp):
    bonds, z_true = random_book(VD, 2000)
    book = BondBook(bonds, gbp)
    curve = gbp.curves.GBP_OIS_SONIA
    prices = np.array([b.clean_price(VD, curve, z, VD) for b, z in zip(bonds, z_true)])
    scalar = [scalar_measures(b, curve, VD, clean_price=p) for b, p in zip(bonds, prices)]
    return book, prices, scalar


def test_measures_host_matches_scalar_methods_from_prices(random_book_2000):
    book, prices, scalar = random_book_2000
    got = _native.bond_measures_host(*book.inputs(clean_prices=prices))
    # status 1: seasoned amortizers, whose yield prices the FULL face and lies beyond the bracket's 50%
    assert got["status"].dtype == np.int32 and np.all(got["status"] <= 1) and np.mean(got["status"] == 0) > 0.9
    for i, ref in enumerate(scalar):
        check_against_scalar(got, i, ref)


def test_measures_host_matches_scalar_methods_from_z(random_book_2000):
    book, _, scalar = random_book_2000
    z = np.array([s["z"] for s in scalar])
    got = _native.bond_measures_host(*book.inputs(z_spreads=z))
    assert np.array_equal(got["z"], z) and np.all(got["status"] <= 1)
    for i, ref in enumerate(scalar):
        check_against_scalar(got, i, ref)


def test_measures_host_fallback_and_no_root(gbp):
    """A clean price of 5 needs z > 0.5: no sign change on the bracket, and the fallback converges (status 1), as the
    host's newton does.  A negative clean price has no root (the PV is positive for every z): status 2, NaN outputs,
    and the host methods raise."""
    curve = gbp.curves.GBP_OIS_SONIA
    bonds = [Bond(Date(15, 1, 2024), "10Y", 0.04, FrequencyTypes.SEMI_ANNUAL, DayCountTypes.ACT_365F, GBP),
             Bond(Date(1, 5, 2024), "50Y", 0.03, FrequencyTypes.MONTHLY, DayCountTypes.ACT_365F, GBP),
             Bond(Date(10, 5, 2023), "1Y", 0.04, FrequencyTypes.ANNUAL, DayCountTypes.ACT_365F, GBP)]
    book = BondBook(bonds, gbp)
    got = _native.bond_measures_host(*book.inputs(clean_prices=5.0))
    assert np.all(got["status"] == 1)
    for i, b in enumerate(bonds):
        z = b.z_spread(VD, curve, 5.0)
        assert z > 0.5 and abs(got["z"][i] - z) < 1e-9
        assert abs(got["ytm"][i] - b.yield_to_maturity(VD, got["clean"][i])) < 1e-9
    # a positive price always has a root: 400 is reached below the bracket (fallback) or inside it
    high = _native.bond_measures_host(*book.inputs(clean_prices=400.0))
    assert list(high["status"]) == [1, 0, 1]
    assert abs(high["z"][2] - bonds[2].z_spread(VD, curve, 400.0)) < 1e-9
    bad = _native.bond_measures_host(*book.inputs(clean_prices=-10.0))
    assert np.all(bad["status"] == 2)
    for k in _native.BOND_OUTPUTS:
        assert np.all(np.isnan(bad[k]))
    for b in bonds:
        with pytest.raises(RuntimeError):
            b.z_spread(VD, curve, -10.0)
        with pytest.raises(RuntimeError):
            b.yield_to_maturity(VD, -10.0)


def test_measures_host_is_exact_restatement_of_itself_per_bond(random_book_2000):
    """A bond's results do not depend on the rest of the batch: each bond alone gives the same bits."""
    book, prices, _ = random_book_2000
    method, nt, nd, arr, is_z = book.inputs(clean_prices=prices)
    full = _native.bond_measures_host(method, nt, nd, arr, is_z)
    off = arr["flow_off"]
    for i in (0, 17, 1999):
        one = {"flow_off": np.array([0, off[i + 1] - off[i]])}
        for k in _native.BOND_FLOW_FIELDS:
            one[k] = arr[k][off[i]:off[i + 1]]
        for k in _native.BOND_FIELDS:
            one[k] = arr[k][i:i + 1]
        alone = _native.bond_measures_host(method, nt, nd, one, is_z)
        for k in _native.BOND_OUTPUTS:
            assert alone[k][0] == full[k][i] or (np.isnan(alone[k][0]) and np.isnan(full[k][i]))


def test_measures_argument_checks(random_book_2000):
    book, prices, _ = random_book_2000
    method, nt, nd, arr, is_z = book.inputs(clean_prices=prices)
    with pytest.raises(LibError):
        _native.bond_measures_host(3, nt, nd, arr, is_z)                       # PCHIP-style schemes are not implemented
    with pytest.raises(LibError):
        _native.bond_measures_host(method, nt[:1], nd[:1], arr, is_z)          # one node
    with pytest.raises(LibError):
        _native.bond_measures_host(method, nt[::-1].copy(), nd, arr, is_z)     # unsorted nodes
    bad = dict(arr, flow_T=arr["flow_T"].copy())
    bad["flow_T"][3] = -1.0
    with pytest.raises(LibError):
        _native.bond_measures_host(method, nt, nd, bad, is_z)
    with pytest.raises(LibError):
        book.inputs()
    with pytest.raises(LibError):
        BondBook([Bond(VD, "2Y", 0.04, FrequencyTypes.ANNUAL, DayCountTypes.ACT_365F, GBP),
                  Bond(VD, "2Y", 0.04, FrequencyTypes.ANNUAL, DayCountTypes.ACT_365F, CurrencyTypes.USD)], F.gbp_model())


def test_engine_dispatch_without_gpu(gbp):
    """Only `Bond` instances reach the bond engine, and only on a currency with a default OIS curve; both checks come
    before any device work."""
    from adrates_amd.market.position.engine import Engine

    class NotABond:
        derivative_type = InstrumentTypes.BOND
    with pytest.raises(LibError):
        Engine(gbp).compute(NotABond(), [])
    chf = Bond(VD, "5Y", 0.02, FrequencyTypes.ANNUAL, DayCountTypes.ACT_365F, CurrencyTypes.CHF)
    with pytest.raises(LibError):
        Engine(gbp).compute(chf, [])
    with pytest.raises(LibError):
        BondBook([chf], gbp)
