"""The scenario host twins (adr_scenario_pv_host, adr_credit_scenario_pv_host and the per-trade rows and sub-book rows of their
sub-book forms) and the C oracle on the hand-made edge books (tests/_scenario_edge_cases.py) against the plain 60-digit
reference (tests/_scenario_reference.py), EVERY element: |got - value| <= k 2^-53 gross with k derived in the reference's
docstring, and +0.0 where gross is 0.  No GPU.

Worst observed shares of the bound over all cases, schemes and credit shapes (each test prints its own); k runs from 10
(LINEAR_FWD_RATES, a short trade) to 214 (LINEAR_ZERO_RATES, 129 coupons out to 16 years on the 20 % row) on the rates calls
and from 13 to 222 on the credit calls:
  rates      host twin 0.067   C oracle 0.067      (device on an MI355X 0.067, device vs host twin 0.049)
  credit     host twin 0.068   C oracle 0.051      (device 0.094, device vs host twin 0.090)
On the project's older scale the rates twin is within 1.2e-15 per unit notional of the reference.  No rounding was miscounted and
the oracle never left the bound.  The one finding: `trade_pv` returned -0.0 for a trade without a live flow whose leg signs
are both -1 (fix_sign * 0.0 + (flt_sign * N) * 0.0 is -0.0 + -0.0), where an element with gross == 0 must be +0.0; it now ends
in `+ 0.0`, which changes no other value.

One-line mutations of `make_slot` / `apply_slot`, each made in scenario_pv.hip and credit_scenario_pv.hip together, built, run
on the host twins and reverted.  Every one fails `test_rates_host_twin_every_element` and `test_credit_host_twin_every_element`
under all three schemes (6 failures of this module's 17 tests); the last column is the 54 tests of test_scenario_pv_host.py,
test_credit_scenarios_host.py and test_subbook_scenarios_host.py:
  1  `&& g.flt_tp[i - 1] >= 0.0` dropped from the kTsIsPrevTe gate                              fails     54 pass
  2  `&& g.flt_alpha[i - 1] > 0.0` dropped from the same gate                                   fails     54 pass
  3  `flt = tp >= 0.0` -> `tp > 0.0`                                                            fails     54 pass
  4  `if (al > 0.0)` -> `al >= 0.0`                                                             fails     54 pass
  5  a coupon that does not accrue is not multiplied by `s.w`                                   fails     54 pass
  6  the term of a coupon that does not accrue set to zero (`term = 0.0 * dp`)                  fails     54 pass
  7  `a.de = de` removed                                                                        fails     21 fail
`if (flt && xt == tp)` -> `if (xt == tp)` changes no result (a dead coupon keeps its negative tp, a missing one has tp = 0.0
and xt > 0): unreachable, not counted."""
import numpy as np
import pytest

from adrates_amd import _native

from . import _credit_scenario_cases as CC
from . import _scenario_cases as SC
from . import _scenario_edge_cases as E
from . import _scenario_reference as R

CREDIT_S = 9                 # scenarios of a credit call on the 65-row case: seven rows between the shocks and the two by hand


def test_the_books_take_the_branches_they_are_named_for():
    E.check_books()


@pytest.mark.parametrize("scheme", E.SCHEMES, ids=lambda s: s.name)
def test_rates_host_twin_every_element(native_lib, scheme):
    worst = 0.0
    for c in E.cases():
        ref = R.reference(scheme.value, c.times, c.dfs, c.batch)
        got = _native.scenario_pv_host(scheme.value, c.times, c.dfs, c.batch, per_trade=True)
        share = ref.share(got["pv"], f"{c.name}")
        print(f"host twin, {scheme.name}, {c.name}: share of the bound {share:.3f} (k {ref.k.min()} .. {ref.k.max()}), "
              f"per unit notional {ref.unit_err(got['pv'], c.batch.notional):.1e}")
        assert share <= 1.0, c.name
        assert np.array_equal(got["book_pv"], SC.book_sum(got["pv"])), c.name
        worst = max(worst, share)
    print(f"host twin, {scheme.name}: worst share {worst:.3f}")


@pytest.mark.parametrize("scheme", E.SCHEMES, ids=lambda s: s.name)
def test_rates_oracle_every_element(native_lib, scheme):
    """oracle/port.c, one call per scenario, on the same books, the same reference and the same bound."""
    worst = 0.0
    for c in E.cases():
        ref = R.reference(scheme.value, c.times, c.dfs, c.batch)
        got = SC.oracle_pv(scheme.value, c.times, c.dfs, c.batch)
        share = ref.share(got, f"oracle {c.name}")
        print(f"C oracle, {scheme.name}, {c.name}: share of the bound {share:.3f}")
        assert share <= 1.0, c.name
        worst = max(worst, share)
    print(f"C oracle, {scheme.name}: worst share {worst:.3f}")


def _credit_calls():
    for c in E.cases():
        for shape in E.CREDIT_SHAPES:
            dfs, dz, case, G = E.credit_call(c, shape, CREDIT_S)
            yield c, shape[0], dfs, dz, case, G


def credit_ref(scheme, c, dfs, dz, case):
    return R.reference(scheme.value, c.times, dfs, c.batch, (case.z, case.bucket, case.fix_tau, case.flt_tau, dz))


@pytest.mark.parametrize("scheme", E.SCHEMES, ids=lambda s: s.name)
def test_credit_host_twin_every_element(native_lib, scheme):
    worst = 0.0
    for c, label, dfs, dz, case, G in _credit_calls():
        ref = credit_ref(scheme, c, dfs, dz, case)
        got = CC.host_pv(scheme.value, c.times, dfs, dz, case)
        share = ref.share(got["pv"], f"{c.name} / {label}")
        print(f"credit host twin, {scheme.name}, {c.name} / {label}: share of the bound {share:.3f} (k {ref.k.min()} .. {ref.k.max()})")
        assert share <= 1.0, (c.name, label)
        assert np.array_equal(got["book_pv"], SC.book_sum(got["pv"])), (c.name, label)
        worst = max(worst, share)
    print(f"credit host twin, {scheme.name}: worst share {worst:.3f}")


@pytest.mark.parametrize("scheme", E.SCHEMES, ids=lambda s: s.name)
def test_credit_oracle_every_element(native_lib, scheme):
    """`_credit_scenario_cases.oracle_pv` (the C oracle on the amounts rescaled by np.exp(-x tau)) on the same bound."""
    worst = 0.0
    for c, label, dfs, dz, case, G in _credit_calls():
        ref = credit_ref(scheme, c, dfs, dz, case)
        share = ref.share(CC.oracle_pv(scheme.value, c.times, dfs, dz, case), f"oracle {c.name} / {label}")
        print(f"credit C oracle, {scheme.name}, {c.name} / {label}: share of the bound {share:.3f}")
        assert share <= 1.0, (c.name, label)
        worst = max(worst, share)
    print(f"credit C oracle, {scheme.name}: worst share {worst:.3f}")


def test_a_plain_trade_takes_the_rates_arithmetic(native_lib):
    """z == 0 and bucket == -1 is the credit source's plain path: those trades' rows are the rates twin's, bit for bit."""
    for c in E.cases():
        dfs, dz, case, G = E.credit_call(c, E.CREDIT_SHAPES[0], CREDIT_S)
        plain = (case.z == 0.0) & (case.bucket == -1)
        assert np.any(plain) and not np.all(plain)
        got = CC.host_pv(4, c.times, dfs, dz, case)["pv"]
        rates = _native.scenario_pv_host(4, c.times, dfs, c.batch, per_trade=True)["pv"]
        assert np.array_equal(got[:, plain], rates[:, plain]) and not np.array_equal(got[:, ~plain], rates[:, ~plain])


@pytest.mark.parametrize("scheme", E.SCHEMES, ids=lambda s: s.name)
def test_threads_single_rows_and_sub_books_keep_their_bits(native_lib, scheme):
    """Thread counts 1, 3 and 16, scenario 64 of the 65-row call priced alone, and the sub-book rows: the fixed-order sum of the
    call's own per-trade rows over a layout whose cuts fall inside the trades' chunk, an empty sub-book among them."""
    for c in E.cases():
        first = _native.scenario_pv_host(scheme.value, c.times, c.dfs, c.batch, per_trade=True, n_threads=1)
        dfs, dz, case, G = E.credit_call(c, E.CREDIT_SHAPES[0], CREDIT_S)
        credit = CC.host_pv(scheme.value, c.times, dfs, dz, case, n_threads=1)
        for threads in (3, 16):
            again = _native.scenario_pv_host(scheme.value, c.times, c.dfs, c.batch, per_trade=True, n_threads=threads)
            assert np.array_equal(again["pv"], first["pv"]) and np.array_equal(again["book_pv"], first["book_pv"]), (c.name, threads)
            again = CC.host_pv(scheme.value, c.times, dfs, dz, case, n_threads=threads)
            assert np.array_equal(again["pv"], credit["pv"]) and np.array_equal(again["book_pv"], credit["book_pv"]), (c.name, threads)
        s = c.dfs.shape[0] - 1
        one = _native.scenario_pv_host(scheme.value, c.times, c.dfs[s], c.batch, per_trade=True)
        assert np.array_equal(one["pv"][0], first["pv"][s]) and one["book_pv"][0] == first["book_pv"][s], c.name
        for threads in (1, 3):
            sub = _native.scenario_subbook_pv_host(scheme.value, c.times, c.dfs, c.batch, c.sub_off, per_trade=True, n_threads=threads)
            csub = _native.credit_scenario_subbook_pv_host(scheme.value, c.times, dfs, dz, c.batch, case.z, case.bucket, case.fix_tau,
                                                           case.flt_tau, c.sub_off, per_trade=True, n_threads=threads)
            assert np.array_equal(sub["pv"], first["pv"]) and np.array_equal(csub["pv"], credit["pv"]), c.name
            for b, (lo, hi) in enumerate(zip(c.sub_off[:-1], c.sub_off[1:])):
                assert np.array_equal(sub["sub_pv"][b], SC.book_sum(sub["pv"][:, lo:hi])), (c.name, b)
                assert np.array_equal(csub["sub_pv"][b], SC.book_sum(csub["pv"][:, lo:hi])), (c.name, b)
                assert hi > lo or not np.any(sub["sub_pv"][b]) and not np.any(np.signbit(sub["sub_pv"][b]))
