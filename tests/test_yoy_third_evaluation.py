"""The YoY inflation kernel's third evaluation (oracle/mp_oracle.py::MpYoY): the inflation leg's PV restated in 60-digit
arithmetic and differenced with respect to the breakeven rates - nothing in it differentiates.  On the case table of
tests/_yoy_cases.py (describe()'s knot bookkeeping, discount lookups, launch-geometry edges), without a GPU:

  - the torch restatement (tests/_inflation_oracle.py::infl_side: autodiff and the reference's chain rule) against MpYoY
    to the 1e-12 of tests/test_mp_third_evaluation.py;
  - the kernel's host twin (adr_yoy_risk_host: the device's describe(), si::locate, si::log_weights, si::df compiled for
    the CPU) against MpYoY and `simple_interpolate`, every entry on its own swap's notional, to REL_TOL;
  - the refusals of the host-array entries.

Observed on the CPU: infl_side against MpYoY 2.3e-13 under the floors of tests/test_mp_third_evaluation.py (ladders that
vanish are held together absolutely instead, see the first test: 0.6 eps of their terms), the host twin against MpYoY
4.5e-12 (the gamma of year-on-year coupons beyond the last LINEAR_ZERO pillar, where y = b_P exactly and the gamma's two
terms cancel to zero: the rounding of 1e-8 n T^2 against the ladder floor of 1e-12 n) and 7.5e-14 elsewhere; against
`simple_interpolate` 1.1e-16."""
import numpy as np
import pytest
import torch

from adrates_amd import _native
from adrates_amd.utils import LibError

from oracle import mp_oracle as MP

from . import _yoy_cases as YC
from ._inflation_oracle import infl_side
from ._parity import REL_TOL
from .test_mp_third_evaluation import TOL, _err

CASES = YC.knot_cases() + YC.geometry_cases()


def _exponents(infl, t):
    """``{pillar: a}`` with ln I(t) = sum a_k ln(1 + b_k): the lookup's weights (decided on the times alone, by
    `mp_oracle._lookup_plan`) times T_k."""
    im, T, _ = infl
    x = np.concatenate(([0.0], np.asarray(T, dtype=np.float64)))
    plan = MP._lookup_plan(x, float(t), im)
    lz = im == YC.LZ
    if plan[0] == "snap":
        w = {plan[1]: 1.0}
    elif plan[0] == "flat":
        w = {plan[1]: t / max(x[plan[1]], 1e-15) if lz else 1.0}
    else:
        _, lo, hi, u = plan
        w = {lo: t * (1.0 - u) / max(x[lo], 1e-15), hi: t * u / x[hi]} if lz else {lo: 1.0 - u, hi: u}
    return {k - 1: v * x[k] for k, v in w.items() if k > 0}


def _zero_ladders(infl, rows):
    """(delta, gamma): whether the swap's delta / gamma vanish, identically or to within 1e-9 of their terms (the lookup
    at t + 1e-12 makes an exponent 1 - 1e-12 where te sits on a FLAT_FWD pillar).  A live coupon is
    scale ((prod (1 + b_k) ** e_k) - 1 + spread) D with e = a(te) - a(ts): no delta when every e_k is 0 (ts == te; both
    beyond the last FLAT_FWD pillar), and no gamma either when one e_k is 1 and the others 0, because then y = b_k
    exactly (a year-on-year coupon beyond the last LINEAR_ZERO pillar, or inside (0, T_1) of a one-pillar FLAT_FWD
    curve)."""
    no_delta = no_gamma = True
    for tp, ts, te, scale, spread in rows:
        if not tp > 0.0:
            continue
        e_s, e_e = _exponents(infl, ts), _exponents(infl, te)
        e = [e_e.get(k, 0.0) - e_s.get(k, 0.0) for k in set(e_s) | set(e_e)]
        live = [v for v in e if abs(v) > 1e-9]
        no_delta &= not live
        no_gamma &= not live or (len(live) == 1 and abs(live[0] - 1.0) < 1e-9)
    return no_delta, no_gamma


def _gross(rows, T):
    """(B_d, B_g): the size of the terms a delta / gamma entry is a sum of.  A delta entry adds g u_k 1e-4 per coupon, a
    gamma entry g (u_k u_l + [k = l] v_k) 1e-8, with |u| <= t_c and |v| <= t_c^2 for t_c = the later of te, ts and the
    pillar that closes their segment: B_d = 1e-4 sum |scale| t_c, B_g = 1e-8 sum |scale| t_c^2."""
    T = np.asarray(T, dtype=np.float64)
    bd = bg = 0.0
    for tp, ts, te, scale, spread in rows:
        t = max(ts, te, 0.0)
        t = max([t] + [float(x) for x in T[T >= t][:1]])
        bd, bg = bd + 1e-4 * abs(scale) * t, bg + 1e-8 * abs(scale) * t * t
    return bd, bg


ZERO_EPS = 16 * np.finfo(np.float64).eps


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_autodiff_oracle_agrees_with_high_precision_differences(case):
    """TOL = 1e-12 with `_err` and its floors (1e-4 n, 1e-8 n, 1e-12 n) as tests/test_mp_third_evaluation.py has them, on
    every ladder that does not vanish identically.  Where one does (`_zero_ladders`, decided on the times alone: 39 of the 200 swaps with coupons),
    float64 autodiff leaves the rounding of terms that cancel, not zero, and a relative bound on a floor of 1e-12 n
    cannot hold: measured with the project's floors, up to 6.1e-10 (gamma of 128 year-on-year coupons beyond the pillar
    of a one-pillar LINEAR_ZERO curve) and 6.9e-12 (delta of the ts == te coupon).  There the two references are held
    together absolutely instead: every entry within 16 eps of the gross terms (`_gross`); observed 0.6 eps at most."""
    (dm, times, dfs), (im, T, b) = case.disc, case.infl
    worst = worst_zero = 0.0
    for i, rows in enumerate(case.rows):
        if not rows:
            continue
        a = np.array(rows)
        ad = infl_side(torch.as_tensor(dfs), times, dm, T, b, im, a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4])
        ref, n = YC._third(case, i), case.notional[i]
        pairs = YC.gamma_pairs(ref["delta"], ad["gamma"], case.P)
        want = YC.third_gamma(case, i, pairs)
        want = np.array([want[pq] for pq in pairs])
        have = np.array([ad["gamma"][pq] for pq in pairs])
        no_delta, no_gamma = _zero_ladders(case.infl, rows)
        bd, bg = _gross(rows, T)
        e = _err(ref["value"], ad["value"], n, 1e-4)
        for zero, got, exp, floor, gross in ((no_delta, ref["delta"], ad["delta"], 1e-8, bd), (no_gamma, want, have, 1e-12, bg)):
            if zero:
                z = np.max(np.abs(np.asarray(got) - np.asarray(exp))) / gross
                assert z <= ZERO_EPS, (case.names[i], z)
                worst_zero = max(worst_zero, z)
            else:
                e = max(e, _err(got, exp, n, floor))
        assert e <= TOL, (case.names[i], e)
        dead = sorted(set(range(case.P)) - set(ref["touched"]))
        assert not np.any(ad["delta"][dead]) and not np.any(ad["gamma"][dead]) and not np.any(ref["delta"][dead])
        worst = max(worst, e)
    print(f"{case}: infl_side against MpYoY {worst:.2e}; vanishing ladders {worst_zero / np.finfo(float).eps:.2g} eps of the gross terms")


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_host_twin_against_third_evaluation(case):
    got = _native.yoy_risk_host(case.disc, case.infl, case.book)
    e, name, key = YC.worst(YC.case_errors(case, got))
    print(f"{case}: host twin against MpYoY {e:.2e} ({name}, {key})")
    assert e <= REL_TOL, (name, key, e)


@pytest.mark.parametrize("case", [c for c in YC.knot_cases() if c.P == 5], ids=repr)
def test_host_twin_exact_cases(case):
    got = _native.yoy_risk_host(case.disc, case.infl, case.book)
    off, im = case.book["cpn_off"], case.infl[0]
    zero_y = ["ts == te: every coefficient cancels"] + (["both beyond the last pillar"] if im == YC.FF else [])
    for name in zero_y:                                         # y = 0 exactly: amount = scale * spread, no Greeks
        i = case.index(name)
        (tp, ts, te, scale, spread), = case.rows[i]
        assert got["amount"][off[i]] == scale * spread, name
        assert not got["delta"][i].any() and not got["gamma"][i].any(), name
    if im == YC.LZ:                                             # the rate of the last pillar is held: only it moves
        i = case.index("both beyond the last pillar")
        assert got["delta"][i][-1] != 0.0 and not got["delta"][i][:-1].any()
    i = case.index("ts < 0 < te < T_1: knot 0 dropped")         # I(ts) = 1: only T_1 carries the coupon
    assert got["delta"][i][0] != 0.0 and not got["delta"][i][1:].any() and np.count_nonzero(got["gamma"][i]) == 1
    i, j = case.index("ts and te on pillars"), case.index("ts and te within 1e-10 of pillars")
    assert got["pv"][i] != 0.0 and np.array_equal(got["delta"][i] != 0.0, [False, True, True, False, False])
    assert np.array_equal(got["delta"][i] != 0.0, got["delta"][j] != 0.0)   # snapped: the node itself, no weights
    i = case.index("seasoned: tp <= 0 masked")                  # projected, but no PV, delta or gamma from tp <= 0
    assert got["amount"][off[i]] != 0.0
    live = _native.yoy_risk_host(case.disc, case.infl, YC.raw_book([case.rows[i][1:]]))
    assert got["pv"][i] == live["pv"][0] and np.array_equal(got["gamma"][i], live["gamma"][0])
    i = case.index("paid at the value time")
    live = _native.yoy_risk_host(case.disc, case.infl, YC.raw_book([case.rows[i][1:]]))
    assert got["pv"][i] == live["pv"][0] and np.array_equal(got["delta"][i], live["delta"][0])


@pytest.mark.parametrize("case", YC.lookup_cases(), ids=repr)
def test_host_twin_discount_lookups(case):
    """pv = D(tp) / D(0) through si::df against `cavour_oracle.simple_interpolate` directly, and against MpYoY."""
    got = _native.yoy_risk_host(case.disc, case.infl, case.book)
    ref = YC.lookup_reference(case)
    assert np.all(got["amount"] == 1.0) and np.count_nonzero(ref) >= ref.size - 3
    e = float(np.max(np.abs(got["pv"] - ref)))
    print(f"{case}: si::df against simple_interpolate {e:.2e}")
    assert e <= REL_TOL and np.array_equal(got["pv"] == 0.0, ref == 0.0)
    assert not got["delta"].any() and not got["gamma"].any()
    e, name, key = YC.worst(YC.case_errors(case, got))
    assert e <= REL_TOL, (name, key, e)


def test_mixed_notionals_are_judged_per_swap():
    """The metric's point: in a book of notionals from 1 to 1e8 a relative error of 1e-6 in the smallest swap's PV
    is seen, where a metric on the scale of the array (1e-13 of its largest entry) passes it."""
    case = YC.geometry_cases()[1]
    got = _native.yoy_risk_host(case.disc, case.infl, case.book)
    i = int(np.argmin(np.where(got["pv"] != 0.0, np.abs(got["pv"]), np.inf)))
    assert np.max(np.abs(got["pv"])) > 1e6 * abs(got["pv"][i])
    bad = {k: v.copy() for k, v in got.items()}
    bad["pv"][i] *= 1.0 + 1e-6
    assert abs(bad["pv"][i] - got["pv"][i]) <= 1e-13 * np.max(np.abs(got["pv"]))
    off = case.book["cpn_off"]
    e = YC.swap_errors(case, i, bad["amount"][off[i]:off[i + 1]], bad["pv"][i], bad["delta"][i], bad["gamma"][i])
    assert e["pv"] > 1e3 * REL_TOL


# --------------------------------------------------------------------------------------------------------- refusals
def _call(disc=None, infl=None, book=None):
    case = YC.knot_cases()[0]
    return _native.yoy_risk_host(disc or case.disc, infl or case.infl, book or case.book)


def _book(**changes):
    book = YC.raw_book([[(1.0, 0.0, 1.0, 1e6, 0.0), (2.0, 1.0, 2.0, 1e6, 0.0)], [(3.0, 2.0, 3.0, 1e6, 0.0)], []])
    book.update(changes)
    return book


def test_host_array_entry_refusals():
    with pytest.raises(LibError, match="cpn_off must run from 0 to m"):
        _call(book=_book(cpn_off=np.array([1, 2, 3, 3])))
    with pytest.raises(LibError, match="coupon offsets must be non-decreasing"):
        _call(book=_book(cpn_off=np.array([0, 3, 2, 3])))
    for field in _native.YOY_FIELDS:
        for bad in (np.nan, np.inf, -np.inf):
            v = _book()[field]
            v[1] = bad
            with pytest.raises(LibError, match="coupon fields must be finite"):
                _call(book=_book(**{field: v}))
    im = YC.LZ
    for T in ([1.0, 1.0, 2.0], [2.0, 1.0, 3.0], [0.0, 1.0, 2.0], [-1.0, 1.0, 2.0], [1.0, 2.0, np.nan]):
        with pytest.raises(LibError, match="pillar times must be increasing from > 0"):
            _call(infl=(im, np.array(T), np.full(3, 0.03)))
    for b in (-1.0, -1.5, np.nan, np.inf):
        with pytest.raises(LibError, match="rates finite and > -1"):
            _call(infl=(im, np.array([1.0, 2.0, 3.0]), np.array([0.03, b, 0.03])))
    with pytest.raises(LibError, match=r"needs 2 \.\. ADR_YOY_MAX_KNOTS \(4096\) knots"):
        _call(disc=(YC.LZ, np.array([0.0]), np.array([1.0])))
    t, d = YC.disc_grid(4097)
    with pytest.raises(LibError, match=r"needs 2 \.\. ADR_YOY_MAX_KNOTS \(4096\) knots"):
        _call(disc=(YC.LZ, t, d))
    with pytest.raises(LibError, match=r"needs 1 \.\. ADR_YOY_MAX_PILLARS \(64\) pillars"):
        _call(infl=(im, np.zeros(0), np.zeros(0)))
    t, d = YC.disc_grid()
    for bad_t, bad_d in ((t[::-1].copy(), d), (t, -d), (t, np.where(np.arange(t.size) == 3, np.nan, d))):
        with pytest.raises(LibError, match="knot times must be finite and non-decreasing, dfs positive"):
            _call(disc=(YC.LZ, bad_t, bad_d))
    got = _call(book=_book())                                   # the book itself is fine
    assert got["pv"][2] == 0.0 and got["pv"][0] != 0.0
