"""The host twin of the cross-currency scenario kernel (adr_xccy_scenario_pv_host, adr_xccy_scenario_subbook_pv_host; no GPU):
every element against the 60-digit reference on its counted bound (tests/_xccy_scenario_reference.py), the same-table identity
with adr_scenario_pv_host, broadcasting, the sub-book rows and the entry's refusals.  The device runs the same cases in
tests/test_gpu_xccy_scenarios.py."""
import dataclasses

import numpy as np
import pytest

from adrates_amd import _native
from adrates_amd.utils.error import LibError

from . import _scenario_cases as SC
from . import _xccy_scenario_cases as XC
from ._xccy_scenario_reference import reference

CASES = XC.cases() + XC.lds_cases()
ERR_INVALID = -1          # ADR_ERR_INVALID (include/adrates.h)


def _host(case, **kw):
    return _native.xccy_scenario_pv_host(*case.args, case.batch, per_trade=True, **kw)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_host_twin_against_the_reference_on_the_bound(case):
    """Every element |got - value| <= k 2^-53 gross; an element with gross == 0 is +0.0 (`Reference.share` asserts it); the
    book sum has the documented order."""
    ref = reference(*case.args, case.batch)
    out = _host(case)
    share = ref.share(out["pv"], repr(case))
    print(f"{case}: k {int(ref.k.min())} .. {int(ref.k.max())}, worst error {share:.3f} of the bound")
    assert share <= 1.0
    assert np.array_equal(out["book_pv"], SC.book_sum(out["pv"]))
    again = _host(case, n_threads=3)
    assert np.array_equal(again["pv"], out["pv"]) and np.array_equal(again["book_pv"], out["book_pv"])


@pytest.mark.parametrize("case", [c for c in XC.cases() if c.dfs_f.shape[0] == c.dfs_x.shape[0]], ids=repr)
def test_same_table_as_both_curves_has_the_rates_entrys_bits(case):
    """One table and one scheme passed as both curves: adr_scenario_pv_host's bits, whichever table of the case it is."""
    for method, times, dfs in ((case.for_method, case.times_f, case.dfs_f), (case.x_method, case.times_x, case.dfs_x)):
        one = _native.scenario_pv_host(method, times, dfs, case.batch, per_trade=True)
        two = _native.xccy_scenario_pv_host(method, times, dfs, method, times, dfs, case.batch, per_trade=True)
        assert np.array_equal(one["pv"], two["pv"]) and np.array_equal(one["book_pv"], two["book_pv"])
        assert not np.any(np.signbit(two["pv"][two["pv"] == 0.0]))


@pytest.mark.parametrize("case", [c for c in XC.cases() if "shared" in c.name or "one scenario" in c.name], ids=repr)
def test_broadcast_rows_equal_explicit_rows(case):
    S = 3
    rep = lambda rows: np.repeat(rows, S, axis=0) if rows.shape[0] == 1 else rows
    wide = XC.Case(case.name, case.for_method, case.times_f, rep(case.dfs_f), case.x_method, case.times_x, rep(case.dfs_x),
                   case.batch, case.sub_off)
    a, b = _host(case), _host(wide)
    if case.S == 1:
        assert all(np.array_equal(b["pv"][s], a["pv"][0]) and b["book_pv"][s] == a["book_pv"][0] for s in range(S))
    else:
        assert np.array_equal(a["pv"], b["pv"]) and np.array_equal(a["book_pv"], b["book_pv"])


@pytest.mark.parametrize("case", [c for c in CASES if c.name.startswith(("edges", "65 swaps", "129 swaps", "1 swaps", "passes"))][::2],
                         ids=repr)
def test_sub_book_rows_are_the_desks_own_book(case):
    sub = _native.xccy_scenario_subbook_pv_host(*case.args, case.batch, case.sub_off, per_trade=True)
    whole = _host(case)
    assert np.array_equal(sub["pv"], whole["pv"])
    for b, (lo, hi) in enumerate(zip(case.sub_off[:-1], case.sub_off[1:])):
        if lo == hi:
            assert np.all(sub["sub_pv"][b] == 0.0) and not np.any(np.signbit(sub["sub_pv"][b]))
            continue
        alone = _native.xccy_scenario_pv_host(*case.args, XC.take(case.batch, int(lo), int(hi)))
        assert np.array_equal(sub["sub_pv"][b], alone["book_pv"]), b


def test_refusals():
    case = XC.cases()[0]
    b = case.batch
    for fm, xm in XC.UNSUPPORTED:
        with pytest.raises(LibError, match="LINEAR_FWD_RATES") as e:
            _native.xccy_scenario_pv_host(fm, case.times_f, case.dfs_f, xm, case.times_x, case.dfs_x, b)
        assert e.value.status == _native.ADR_ERR_UNSUPPORTED
    with pytest.raises(LibError, match="scheme must be"):
        _native.xccy_scenario_pv_host(3, case.times_f, case.dfs_f, 1, case.times_x, case.dfs_x, b)
    with pytest.raises(LibError, match="one shared row or one row per scenario"):
        _native.xccy_scenario_pv_host(1, case.times_f, case.dfs_f[:2], 1, case.times_x, case.dfs_x, b)
    bad = case.dfs_x.copy()
    bad[1, 2] = -1.0
    with pytest.raises(LibError, match=r"XCCY row 1, knot 2"):
        _native.xccy_scenario_pv_host(1, case.times_f, case.dfs_f, 1, case.times_x, bad, b)
    bad = case.dfs_f.copy()
    bad[2, 7] = np.nan
    with pytest.raises(LibError, match=r"foreign row 2, knot 7"):
        _native.xccy_scenario_pv_host(1, case.times_f, bad, 1, case.times_x, case.dfs_x, b)
    with pytest.raises(LibError, match="non-decreasing"):
        _native.xccy_scenario_pv_host(1, case.times_f, case.dfs_f, 1, case.times_x[::-1].copy(), case.dfs_x, b)
    with pytest.raises(LibError, match="knot grid needs"):
        _native.xccy_scenario_pv_host(1, case.times_f[:1], case.dfs_f[:, :1], 1, case.times_x, case.dfs_x, b)
    signs = b.flt_sign.copy()
    signs[3] = 0.5
    with pytest.raises(LibError, match="leg signs"):
        _native.xccy_scenario_pv_host(*case.args, dataclasses.replace(b, flt_sign=signs))
    with pytest.raises(LibError, match="sub-book"):
        _native.xccy_scenario_subbook_pv_host(*case.args, b, np.array([0, 5, 3, b.n_trades]))
    # the raw entry: S_f / S_x that are neither 1 nor S, and a NULL output
    lib = _native.load()
    args = _native._curve_args(1, case.times_f, case.dfs_f) + _native._curve_args(1, case.times_x, case.dfs_x)
    batch_args = _native._batch_args(*_native._batch_arrays(b))
    out = np.empty(5)
    assert lib.adr_xccy_scenario_pv_host(*args, 5, *batch_args, None, _native._ptr(out), 1) == ERR_INVALID
    assert lib.adr_xccy_scenario_pv_host(*args, 3, *batch_args, None, None, 1) == ERR_INVALID
