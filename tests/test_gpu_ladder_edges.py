"""The sub-book ladder kernels (adr_subbook_ladders, adr_credit_subbook_ladders, adr_yoy_subbook_ladders) on the hand-made edge books
(tests/_ladder_edge_cases.py) against the plain 60-digit reference (tests/_ladder_reference.py), EVERY element, on the bound
derived there; against their host twins element by element on the same bound; two launches bit for bit.  The reference of a
case is built once per process and shared with nothing else: the CPU module (tests/test_ladder_edges_host.py) holds the host
twins and the C oracle to it.

Worst observed shares of the bound on an MI355X over all cases and schemes (each test prints its own):
  rates      device vs reference 0.071   device vs host twin 0.038
  credit     device vs reference 0.023   device vs host twin 0.015
  inflation  device vs reference 0.110 / 0.111 / 0.118   device vs host twin 0.015 / 0.027 / 0.054
             (LINEAR_ZERO / FLAT_FWD / LINEAR_FWD discounting; the host twin stands at 0.110 / 0.111 / 0.118)
Everything the inflation test asserts is shown on the host twin first (tests/test_ladder_edges_host.py, which also has the
mutations): the twin runs the same node, sum and projection code, so only the order of the LDS adds and the device's exp / log
differ, and a device entry beyond the bound where the twin is inside would be a finding in yoy_subbook_knot_kernel,
yoy_infl_kernel or project_curve_block<true>.  None was found: that form of the projection now runs with P_d = 65 (a second
column block of one curve column) and Q = 129 (a third of one column), and one wave per block at P_i = 64.  The slowest case
(65 pillars, P_i = 64) takes 1.8 s."""
import pytest

from adrates_amd import _native

from . import _credit_ladder_cases as CL
from . import _ladder_edge_cases as E
from . import _ladder_reference as R
from . import _sub_book_ladder_cases as L
from . import _yoy_ladder_cases as Y

pytestmark = pytest.mark.gpu

RATES_CASES = range(5)
CREDIT_CASES = range(5)
YOY_CASES = range(10)


def device_curve(ctx, interp, host):
    return _native.DeviceCurve(ctx, interp.value, host.times, host.dfs, host.jac, host.hess)


@pytest.mark.parametrize("which", RATES_CASES)
@pytest.mark.parametrize("interp", E.SCHEMES, ids=lambda i: i.name)
def test_rates_device_every_element(gpu_ctx, interp, which):
    case = E.rates_cases(interp)[which]
    h = case.host
    dc = device_curve(gpu_ctx, interp, h)
    with _native.DeviceTrades(gpu_ctx, case.batch) as dt:
        for layout, sub_off in case.layouts.items():
            ref = R.rates_reference(interp.value, h, case.batch, sub_off)
            got = _native.subbook_ladders(gpu_ctx, dc, dt, sub_off)
            again = _native.subbook_ladders(gpu_ctx, dc, dt, sub_off)
            twin = _native.subbook_ladders_host(interp.value, h.times, h.dfs, h.jac, h.hess, case.batch, sub_off)
            share = R.worst_share(got, ref, what=f"{case.name}/{layout}")
            gap = R.worst_between(got, twin, ref, R.RATES_BLOCKS)
            print(f"device, {interp.name}, {case.name}/{layout}: share of the bound {share:.3f}, device vs host twin {gap:.3f}")
            assert share <= 1.0 and gap <= 1.0, (case.name, layout)
            assert L.same_bits(got, again), "two launches differ"


@pytest.mark.parametrize("which", CREDIT_CASES)
@pytest.mark.parametrize("interp", E.SCHEMES, ids=lambda i: i.name)
def test_credit_device_every_element(gpu_ctx, interp, which):
    c = E.credit_cases(interp)[which]
    dc = device_curve(gpu_ctx, interp, c.host)
    ref = R.credit_reference(interp.value, c.host, c.case, c.G, c.sub_off)
    got = CL.device_ladders(gpu_ctx, dc, c.case, c.G, c.sub_off)
    again = CL.device_ladders(gpu_ctx, dc, c.case, c.G, c.sub_off)
    twin = CL.host_ladders(interp.value, c.host, c.case, c.G, c.sub_off)
    CL.check_layout(got, dc.n_pillars, c.G)
    share = R.worst_share(got, ref, R.CREDIT_BLOCKS, what=c.name)
    gap = R.worst_between(got, twin, ref, R.CREDIT_BLOCKS)
    print(f"credit device, {interp.name}, {c.name}: share of the bound {share:.3f}, device vs host twin {gap:.3f}")
    assert share <= 1.0 and gap <= 1.0, c.name
    assert CL.same_bits(got, again), "two launches differ"


@pytest.mark.parametrize("which", YOY_CASES)
@pytest.mark.parametrize("interp", E.SCHEMES, ids=lambda i: i.name)
def test_yoy_device_every_element(gpu_ctx, interp, which):
    c = E.yoy_cases(interp)[which]
    dc = device_curve(gpu_ctx, interp, c.host)
    blocks = R.RATES_BLOCKS if c.want_gamma else ("pv", "delta")
    for layout, sub_off in c.layouts.items():
        ref = R.yoy_reference(interp.value, c.host, c.infl, c.book, sub_off)
        got = E.yoy_entry(interp, c, sub_off, gpu_ctx, dc)
        again = E.yoy_entry(interp, c, sub_off, gpu_ctx, dc)
        twin = E.yoy_entry(interp, c, sub_off)
        share = E.check_yoy_rows(got, ref, c, f"{c.name}/{layout}")
        gap = R.worst_between(got, twin, ref, blocks)
        print(f"inflation device, {interp.name}, {c.name}/{layout}: share of the bound {share:.3f}, device vs host twin {gap:.3f}")
        assert share <= 1.0 and gap <= 1.0, (c.name, layout)
        assert Y.same_bits(got, again), "two launches differ"


def test_the_case_counts():
    assert len(E.rates_cases(E.SCHEMES[0])) == len(RATES_CASES) and len(E.credit_cases(E.SCHEMES[0])) == len(CREDIT_CASES)
    assert len(E.yoy_cases(E.SCHEMES[0])) == len(YOY_CASES)
