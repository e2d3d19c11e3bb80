"""The inflation scenario kernel (csrc/yoy_scenario_pv.hip and the kSub route of its sub-book entries) on the hand-made edge
books (tests/_yoy_scenario_edge_cases.py) against the plain 60-digit reference (tests/_yoy_scenario_reference.py), EVERY
element, on the bound derived there; against the host twin element by element on the same bound; two launches bit for bit;
guard words behind ``pv``, ``book_pv`` and ``sub_pv``; ``book_pv`` and the desk rows the fixed-order sum of the launch's own
rows; the last scenario of a launch priced alone; a shared row on either side; the LDS table against the global one on the same
flows.  The reference of a case is built once per process; the CPU module (tests/test_yoy_scenario_edges_host.py) holds the host
twin to it, checks the reference against the older one and has the mutations.

Worst observed shares of the bound on an MI355X over all cases, launch shapes and scheme pairs (each test prints its own, with
the place); k runs from 7 to 1 592:
  device vs reference 0.080   main, the coupon with ts = 0.25 and te = 0.125, scenario 23, LINEAR_FWD_RATES discounting and
                              LINEAR_ZERO_RATES inflation (the host twin stands at 0.080 on the same element)
  device vs host twin 0.076   main with a shared discount row, the coupon inside the segment whose ends have equal L on
                              breakeven row 4, scenario 12, LINEAR_FWD_RATES / FLAT_FWD_RATES
The global table and the LDS table differ by 0.000 of the bound on the common flows.  The whole module takes 6.5 s, its slowest
test 0.5 s.  No element left the bound and none with gross == 0 was -0.0: these tests have no finding."""
import numpy as np
import pytest
import torch

from adrates_amd import _native

from . import _scenario_cases as SC
from . import _yoy_scenario_edge_cases as E
from . import _yoy_scenario_reference as R
from .test_yoy_scenario_edges_host import PAIRS, host, pair_id, reference

pytestmark = pytest.mark.gpu
GUARD = -1.2345e300
TAIL = 8
CASES = range(6)


def device(ctx, dm, im, case, dfs, b):
    return _native.yoy_scenario_pv(ctx, dm, case.times, dfs, im, case.T, b, case.fixed, case.book, per_trade=True)


def run_dev(ctx, dm, im, case, dfs, b, per_trade, sub_off=None):
    """adr_yoy_scenario_pv_dev, or adr_yoy_scenario_subbook_pv_dev with ``sub_off``, into guarded buffers: ``(book [S] or sub_pv
    [B, S], pv [S, n] or None)`` as numpy."""
    dfs, b = np.atleast_2d(dfs), np.atleast_2d(b)
    S = max(dfs.shape[0], b.shape[0])
    cpn_off, cpn = _native.yoy_pack(case.book)
    n = cpn_off.size - 1
    arrs = dict(times=case.times, dfs=dfs, T=case.T, b=b, fix_off=case.fixed[0], fix_tp=case.fixed[1], fix_pay=case.fixed[2],
                cpn_off=cpn_off, cpn=cpn)
    B = 0 if sub_off is None else len(sub_off) - 1
    if B:
        arrs["plan"] = _native.scenario_subbook_plan(n, sub_off)
    dev = torch.device("cuda", 0)
    held = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in arrs.items()}
    ptrs = {k: v.data_ptr() if v.numel() else 0 for k, v in held.items()}
    rows = max(B, 1)
    W = _native.scenario_subbook_work(n, B, S) if B else _native.yoy_scenario_pv_work(n, S)
    guarded = lambda count: torch.full((count + TAIL,), GUARD, dtype=torch.float64, device=dev)
    out, pv, work = guarded(rows * S), guarded(n * S), guarded(W)
    torch.cuda.synchronize()
    head = (ctx, dm, case.times.size, dfs.shape[0], im, case.T.size, b.shape[0], S, n, case.fixed[1].size, cpn.shape[1])
    if B:
        _native.yoy_scenario_subbook_pv_dev(*head, B, ptrs, out.data_ptr(), work.data_ptr(), pv.data_ptr() if per_trade else 0)
    else:
        _native.yoy_scenario_pv_dev(*head, ptrs, out.data_ptr(), work.data_ptr(), pv.data_ptr() if per_trade else 0)
    torch.cuda.synchronize()
    assert torch.all(out[rows * S:] == GUARD) and torch.all(work[W:] == GUARD)
    assert torch.all(pv[n * S:] == GUARD) if per_trade else torch.all(pv == GUARD)          # pv is not written when NULL
    res = out[:rows * S].cpu().numpy()
    return (res.reshape(B, S) if B else res), (pv[:n * S].reshape(n, S).cpu().numpy().T if per_trade else None)


def held_to_the_reference(ctx, dm, im, case, dfs, b, label):
    """The blocking entry on the bound, against the twin on the bound, twice bit for bit, the book sum; returns its result."""
    ref = reference(dm, im, case, dfs, b)
    twin = host(dm, im, case, dfs, b)
    got, again = device(ctx, dm, im, case, dfs, b), device(ctx, dm, im, case, dfs, b)
    share, i, s, _ = ref.worst(got["pv"], label)
    gap, gi, gs = ref.apart(got["pv"], twin["pv"], label)
    print(f"device, {pair_id((dm, im))}, {label}: worst share of the bound {share:.3f} at swap {i} ({case.names[i]}), scenario {s}; "
          f"device vs host twin {gap:.3f} at swap {gi} ({case.names[gi] if gi >= 0 else 'none differs'}), scenario {gs} "
          f"(k {ref.k.min()} .. {ref.k.max()})")
    assert share <= 1.0 and gap <= 1.0, (label, case.names[i], s, gi, gs)
    assert np.array_equal(got["pv"], again["pv"]) and np.array_equal(got["book_pv"], again["book_pv"]), "two launches differ"
    assert np.array_equal(got["book_pv"], SC.book_sum(got["pv"]))
    return got


@pytest.mark.parametrize("which", CASES)
@pytest.mark.parametrize("pair", PAIRS, ids=pair_id)
def test_device_every_element(gpu_ctx, pair, which):
    dm, im = pair
    c = E.cases()[which]
    S = c.dfs.shape[0]
    got = held_to_the_reference(gpu_ctx, dm, im, c, c.dfs, c.b, c.name)
    book, pv = run_dev(gpu_ctx, dm, im, c, c.dfs, c.b, True)                          # checks the guard words
    assert np.array_equal(pv, got["pv"]) and np.array_equal(book, got["book_pv"])
    book_only, _ = run_dev(gpu_ctx, dm, im, c, c.dfs, c.b, False)
    assert np.array_equal(book_only, book)
    b1, p1 = run_dev(gpu_ctx, dm, im, c, c.dfs[S - 1], c.b[S - 1], True)
    assert np.array_equal(p1[0], got["pv"][S - 1]) and b1[0] == got["book_pv"][S - 1], f"scenario {S - 1} alone"
    sub = _native.yoy_scenario_subbook_pv(gpu_ctx, dm, c.times, c.dfs, im, c.T, c.b, c.fixed, c.book, c.sub_off, per_trade=True)
    assert np.array_equal(sub["pv"], got["pv"]), c.name
    for d, (lo, hi) in enumerate(zip(c.sub_off[:-1], c.sub_off[1:])):
        assert np.array_equal(sub["sub_pv"][d], SC.book_sum(got["pv"][:, lo:hi])), (c.name, d)
        assert hi > lo or not np.any(sub["sub_pv"][d]) and not np.any(np.signbit(sub["sub_pv"][d]))
    rows, pv = run_dev(gpu_ctx, dm, im, c, c.dfs, c.b, True, c.sub_off)               # the guard words behind sub_pv
    assert np.array_equal(rows, sub["sub_pv"]) and np.array_equal(pv, got["pv"])


@pytest.mark.parametrize("pair", PAIRS, ids=pair_id)
def test_a_shared_row_on_either_side(gpu_ctx, pair):
    """S_disc = 1 with S_infl = 65 and the reverse, the shared row neither row 0 nor the scenario's own."""
    dm, im = pair
    c = E.cases()[0]
    joint = device(gpu_ctx, dm, im, c, c.dfs, c.b)["pv"]
    for label, d, r in E.SHAPES:
        dfs, b = c.dfs[d], c.b[r]
        assert {dfs.shape[0], b.shape[0]} == {1, 65}
        got = held_to_the_reference(gpu_ctx, dm, im, c, dfs, b, f"main, {label}")
        book, pv = run_dev(gpu_ctx, dm, im, c, dfs, b, True)
        assert np.array_equal(pv, got["pv"]) and np.array_equal(book, got["book_pv"])
        s = 64 if dfs.shape[0] == 1 else 2                                             # the scenario whose own pair this is
        assert np.array_equal(got["pv"][s], joint[s]) and not np.array_equal(got["pv"][0], joint[0])


@pytest.mark.parametrize("pair", PAIRS, ids=pair_id)
def test_the_lds_table_and_the_global_table_agree(gpu_ctx, pair):
    """The 264-knot grid with 64 pillars (the discount rows stay in global memory) and with the 5 pillars the flows touch (both
    tables in LDS): the same numbers by construction, so the two launches are held to each other on the bound."""
    dm, im = pair
    g, l = E.cases()[4], E.cases()[5]
    assert E.lds_bytes(g.times.size, g.T.size) > 160 * 1024 >= E.lds_bytes(l.times.size, l.T.size)
    ref_g, ref_l = reference(dm, im, g, g.dfs, g.b), reference(dm, im, l, l.dfs, l.b)
    assert all(abs(ref_g.value[i][s] - ref_l.value[i][s]) <= R.mpf(10) ** -50 * ref_g.gross[i][s] for i in range(g.n) for s in range(3))
    a, b = device(gpu_ctx, dm, im, g, g.dfs, g.b), device(gpu_ctx, dm, im, l, l.dfs, l.b)
    gap = ref_g.between(a["pv"], b["pv"], "global vs LDS")
    print(f"{pair_id(pair)}: global table vs LDS table {gap:.3f} of the bound")
    assert gap <= 1.0


def test_the_case_count_and_the_launch_shapes():
    cases = E.cases()
    assert len(cases) == len(CASES) and cases[0].dfs.shape[0] == 65 and cases[0].n > 64 and cases[4].times.size == 264
    E.check_books()
