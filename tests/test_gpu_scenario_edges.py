"""The scenario kernels that price ordinary cash flows (csrc/scenario_pv.hip, csrc/credit_scenario_pv.hip and the kSub route of
their sub-book entries) on the hand-made edge books (tests/_scenario_edge_cases.py) against the plain 60-digit reference
(tests/_scenario_reference.py), EVERY element, on the bound derived there; against their host twins element by element on
the same bound; two launches bit for bit; guard words behind ``pv`` and ``book_pv``; ``book_pv`` and the sub-book rows the
fixed-order sum of the launch's own rows; the last scenario of a launch (scenario 64 of the 65-row case) priced alone.  The
reference of a case is built once per process; the CPU module (tests/test_scenario_edges_host.py) holds the host twins and the
C oracle to it and has the mutations.

Worst observed shares of the bound on an MI355X over all cases, schemes and credit shapes (each test prints its own); k runs
from 10 to 214 on the rates calls and from 13 to 222 on the credit calls:
  rates      device vs reference 0.067   device vs host twin 0.049   (the host twin stands at 0.067, the C oracle at 0.067)
  credit     device vs reference 0.094   device vs host twin 0.090   (the host twin stands at 0.068, the C oracle at 0.051)
Under LINEAR_FWD_RATES, which has no exp, the rates device rows are the twin's bit for bit.  The whole module takes 5 s, its
slowest case 0.4 s.  Before `trade_pv` ended in `+ 0.0` both the device and the twin returned -0.0 for a trade without a live
flow whose leg signs are both -1 (the case "no live flow, both signs -1"): the one finding of these tests."""
import numpy as np
import pytest
import torch

from adrates_amd import _native

from . import _credit_scenario_cases as CC
from . import _scenario_cases as SC
from . import _scenario_edge_cases as E
from . import _scenario_reference as R
from .test_gpu_credit_scenarios import _Dev
from .test_gpu_scenario_pv import _run_dev

pytestmark = pytest.mark.gpu

CASES = range(4)
CREDIT_S = 9                 # as tests/test_scenario_edges_host.py; the joint shape of the 65-row case runs all 65


def sub_rows_are_the_sums(sub, pv, sub_off, what):
    assert np.array_equal(sub["pv"], pv), what
    for b, (lo, hi) in enumerate(zip(sub_off[:-1], sub_off[1:])):
        assert np.array_equal(sub["sub_pv"][b], SC.book_sum(pv[:, lo:hi])), (what, b)


@pytest.mark.parametrize("which", CASES)
@pytest.mark.parametrize("scheme", E.SCHEMES, ids=lambda s: s.name)
def test_rates_device_every_element(gpu_ctx, scheme, which):
    c = E.cases()[which]
    m, S, n = scheme.value, c.dfs.shape[0], c.batch.n_trades
    ref = R.reference(m, c.times, c.dfs, c.batch)
    twin = _native.scenario_pv_host(m, c.times, c.dfs, c.batch, per_trade=True)
    with _native.DeviceTrades(gpu_ctx, c.batch) as trades:
        got = _native.scenario_pv(gpu_ctx, m, c.times, c.dfs, trades, per_trade=True)
        again = _native.scenario_pv(gpu_ctx, m, c.times, c.dfs, trades, per_trade=True)
        share, gap = ref.share(got["pv"], c.name), ref.between(got["pv"], twin["pv"], c.name)
        print(f"device, {scheme.name}, {c.name}: share of the bound {share:.3f}, device vs host twin {gap:.3f} "
              f"(k {ref.k.min()} .. {ref.k.max()})")
        assert share <= 1.0 and gap <= 1.0, c.name
        assert np.array_equal(got["pv"], again["pv"]) and np.array_equal(got["book_pv"], again["book_pv"]), "two launches differ"
        assert np.array_equal(got["book_pv"], SC.book_sum(got["pv"]))
        dev = torch.device("cuda", 0)
        times_t, dfs_t = torch.from_numpy(c.times).to(dev), torch.from_numpy(np.ascontiguousarray(c.dfs)).to(dev)
        book, pv = _run_dev(gpu_ctx, m, times_t, dfs_t, trades, n, S, True)          # checks the guard words
        assert np.array_equal(pv.T, got["pv"]) and np.array_equal(book, got["book_pv"])
        book_only, _ = _run_dev(gpu_ctx, m, times_t, dfs_t, trades, n, S, False)
        assert np.array_equal(book_only, book)
        last_t = torch.from_numpy(c.dfs[S - 1:S].copy()).to(dev)
        b1, p1 = _run_dev(gpu_ctx, m, times_t, last_t, trades, n, 1, True)
        assert np.array_equal(p1[:, 0], got["pv"][S - 1]) and b1[0] == got["book_pv"][S - 1], f"scenario {S - 1} alone"
        sub = _native.scenario_subbook_pv(gpu_ctx, m, c.times, c.dfs, trades, c.sub_off, per_trade=True)
        sub_rows_are_the_sums(sub, got["pv"], c.sub_off, c.name)


@pytest.mark.parametrize("which", CASES)
@pytest.mark.parametrize("scheme", E.SCHEMES, ids=lambda s: s.name)
def test_credit_device_every_element(gpu_ctx, scheme, which):
    c = E.cases()[which]
    m = scheme.value
    for shape in E.CREDIT_SHAPES:
        dfs, dz, case, G = E.credit_call(c, shape, None if shape is E.CREDIT_SHAPES[0] else CREDIT_S)
        S = max(dfs.shape[0], dz.shape[0])
        what = f"{c.name} / {shape[0]}"
        ref = R.reference(m, c.times, dfs, c.batch, (case.z, case.bucket, case.fix_tau, case.flt_tau, dz))
        twin = CC.host_pv(m, c.times, dfs, dz, case)
        got = CC.device_pv(gpu_ctx, m, c.times, dfs, dz, case)
        again = CC.device_pv(gpu_ctx, m, c.times, dfs, dz, case)
        share, gap = ref.share(got["pv"], what), ref.between(got["pv"], twin["pv"], what)
        print(f"credit device, {scheme.name}, {what}, S = {S}: share of the bound {share:.3f}, device vs host twin {gap:.3f} "
              f"(k {ref.k.min()} .. {ref.k.max()})")
        assert share <= 1.0 and gap <= 1.0, what
        assert np.array_equal(got["pv"], again["pv"]) and np.array_equal(got["book_pv"], again["book_pv"]), "two launches differ"
        assert np.array_equal(got["book_pv"], SC.book_sum(got["pv"]))
        if shape is not E.CREDIT_SHAPES[0]:
            continue
        d = _Dev(gpu_ctx, case, c.times)
        try:
            book, pv = d.run(m, dfs, dz, S, True)                                   # checks the guard words
            assert np.array_equal(pv.T, got["pv"]) and np.array_equal(book, got["book_pv"])
            b1, p1 = d.run(m, dfs[S - 1:S], dz[S - 1:S], 1, True)
            assert np.array_equal(p1[:, 0], got["pv"][S - 1]) and b1[0] == got["book_pv"][S - 1], f"scenario {S - 1} alone"
            sub = _native.credit_scenario_subbook_pv(gpu_ctx, m, c.times, dfs, dz, d.trades, case.z, case.bucket, case.fix_tau,
                                                     case.flt_tau, c.sub_off, per_trade=True)
            sub_rows_are_the_sums(sub, got["pv"], c.sub_off, what)
        finally:
            d.close()


def test_the_case_count_and_the_launch_shapes():
    cases = E.cases()
    assert len(cases) == len(CASES) and cases[0].dfs.shape[0] == 65 and cases[3].times.size > 315
    E.check_books()
