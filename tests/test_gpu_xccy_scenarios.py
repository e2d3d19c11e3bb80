"""Cross-currency scenario revaluation on the GPU (csrc/xccy_scenario_pv.hip): every element against the 60-digit reference on
its counted bound over all case books and all three LDS modes (tests/_xccy_scenario_cases.py, _xccy_scenario_reference.py), the
host twin, run-to-run bits, a scenario alone against the same scenario inside S = 129, sub-book bits, the device-array entries
into guarded buffers on a caller's stream, and `XccyBook.revalue` on the device against ``host=True``."""
import numpy as np
import pytest
import torch

from adrates_amd import _native
from adrates_amd.utils.error import LibError

from . import _scenario_cases as SC
from . import _xccy_scenario_cases as XC
from ._xccy_scenario_reference import reference

pytestmark = pytest.mark.gpu
GUARD = -1.2345e300
CASES = XC.cases() + XC.lds_cases()


def _device(ctx, case, legs=None):
    with _native.DeviceTrades(ctx, case.batch if legs is None else legs) as tr:
        return _native.xccy_scenario_pv(ctx, *case.args, tr, per_trade=True)


def _array_error(dev, host):
    """The YoY scenario tests' per-array measure: the largest difference on the array's largest entry."""
    return float(np.max(np.abs(dev - host)) / max(np.max(np.abs(host)), 1e-300))


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_device_against_the_reference_and_the_host_twin(gpu_ctx, case):
    ref = reference(*case.args, case.batch)
    dev = _device(gpu_ctx, case)
    host = _native.xccy_scenario_pv_host(*case.args, case.batch, per_trade=True)
    share, twin = ref.share(dev["pv"], repr(case)), _array_error(dev["pv"], host["pv"])
    print(f"{case}: k {int(ref.k.min())} .. {int(ref.k.max())}, device {share:.3f} of the bound, {twin:.2e} of the array off the twin")
    assert share <= 1.0
    assert twin <= 1e-13 and _array_error(dev["book_pv"], host["book_pv"]) <= 1e-13
    assert np.array_equal(dev["book_pv"], SC.book_sum(dev["pv"]))
    if case.for_method == XC.LF:                    # no exp and no log on either side
        assert np.array_equal(dev["pv"], host["pv"]) and np.array_equal(dev["book_pv"], host["book_pv"])
    again = _device(gpu_ctx, case)
    assert np.array_equal(again["pv"], dev["pv"]) and np.array_equal(again["book_pv"], dev["book_pv"])


def _upload(arrs):
    dev = torch.device("cuda", 0)
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in arrs.items()}


def _run_dev(ctx, case, tr, dfs_f, dfs_x, per_trade, stream=0, sub_off=None):
    """adr_xccy_scenario_pv_dev (``sub_off``: the sub-book form) into guarded buffers: ``(book [S] or sub_pv [B, S], pv [S, n] or
    None)``.  What is not asked for keeps its pattern, and so do the words after every output."""
    dfs_f, dfs_x = np.atleast_2d(dfs_f), np.atleast_2d(dfs_x)
    S, n = max(dfs_f.shape[0], dfs_x.shape[0]), tr.n_trades
    B = 1 if sub_off is None else len(sub_off) - 1
    arrs = dict(times_f=case.times_f, dfs_f=dfs_f, times_x=case.times_x, dfs_x=dfs_x)
    if sub_off is not None:
        arrs["plan"] = _native.scenario_subbook_plan(n, sub_off)
    t = _upload(arrs)
    dev = t["times_f"].device
    out = torch.full((B * S + 8,), GUARD, dtype=torch.float64, device=dev)
    pv = torch.full((n * S + 8,), GUARD, dtype=torch.float64, device=dev)
    words = _native.xccy_scenario_pv_work(n, S) if sub_off is None else _native.scenario_subbook_work(n, B, S)
    work = torch.full((words + 8,), GUARD, dtype=torch.float64, device=dev)
    ptrs = {k: v.data_ptr() for k, v in t.items()}
    head = (ctx, case.for_method, case.times_f.size, dfs_f.shape[0], case.x_method, case.times_x.size, dfs_x.shape[0], S, tr)
    torch.cuda.synchronize()
    if sub_off is None:
        _native.xccy_scenario_pv_dev(*head, ptrs, out.data_ptr(), work.data_ptr(), pv.data_ptr() if per_trade else 0, stream)
    else:
        _native.xccy_scenario_subbook_pv_dev(*head, B, ptrs, out.data_ptr(), work.data_ptr(), pv.data_ptr() if per_trade else 0, stream)
    torch.cuda.synchronize()
    assert torch.all(out[B * S:] == GUARD) and torch.all(work[words:] == GUARD)
    assert torch.all(pv[n * S:] == GUARD) if per_trade else torch.all(pv == GUARD)
    book = out[:B * S].cpu().numpy()
    return (book if sub_off is None else book.reshape(B, S)), (pv[:n * S].reshape(n, S).cpu().numpy().T if per_trade else None)


@pytest.mark.parametrize("shape", [(40, 5), (300, 40), (4096, 4096)], ids=lambda s: f"K = {s}, LDS: {XC.lds_mode(*s)}")
def test_a_scenario_alone_against_the_same_scenario_inside_129(gpu_ctx, shape):
    """S in {1, 63, 64, 65, 129} in every LDS mode: each row has the bits of its pair priced alone, broadcast rows included, and
    the padding lanes of a partial group write nothing (`_run_dev`'s guards); the rows priced alone meet the reference."""
    Kf, Kx = shape
    pair = XC.PAIRS[(Kf // 40) % 5]
    (tf, f2), (tx, x2) = XC.table(Kf, 3, 31), XC.table(Kx, 3, 32)
    batch = XC._book("edges")
    case = XC.Case("edges", pair[0], tf, f2, pair[1], tx, x2, batch, XC._sub_off(batch.n_trades))
    dfs_f, dfs_x = XC.mixed_rows(f2, 129, 1), XC.mixed_rows(x2, 129, 2)
    picks = (0, 62, 63, 64, 128)
    with _native.DeviceTrades(gpu_ctx, batch) as tr:
        alone = {s: _run_dev(gpu_ctx, case, tr, dfs_f[s], dfs_x[s], True) for s in picks}
        for S in (1, 63, 64, 65, 129):
            book, pv = _run_dev(gpu_ctx, case, tr, dfs_f[:S], dfs_x[:S], True)
            book_only, none = _run_dev(gpu_ctx, case, tr, dfs_f[:S], dfs_x[:S], False)
            assert none is None and np.array_equal(book, book_only) and np.array_equal(book, SC.book_sum(pv))
            for s, (b1, p1) in alone.items():
                if s < S:
                    assert np.array_equal(pv[s], p1[0]) and book[s] == b1[0], (S, s)
        shared_f = _run_dev(gpu_ctx, case, tr, dfs_f[64], dfs_x[:65], True)
        shared_x = _run_dev(gpu_ctx, case, tr, dfs_f[:65], dfs_x[64], True)
        assert np.array_equal(shared_f[1][64], alone[64][1][0]) and np.array_equal(shared_x[1][64], alone[64][1][0])
        rep = _run_dev(gpu_ctx, case, tr, np.repeat(dfs_f[64:65], 65, axis=0), dfs_x[:65], True)
        assert np.array_equal(rep[1], shared_f[1]) and np.array_equal(rep[0], shared_f[0])
    idx = list(picks)
    ref = reference(pair[0], tf, dfs_f[idx], pair[1], tx, dfs_x[idx], batch)
    assert ref.share(np.stack([alone[s][1][0] for s in picks]), "rows priced alone") <= 1.0


@pytest.mark.parametrize("case", [c for c in CASES if c.name.startswith(("edges, LDS", "129 swaps", "65 swaps", "passes"))], ids=repr)
def test_sub_book_rows_have_the_bits_of_the_desk_alone(gpu_ctx, case):
    with _native.DeviceTrades(gpu_ctx, case.batch) as tr:
        sub = _native.xccy_scenario_subbook_pv(gpu_ctx, *case.args, tr, case.sub_off, per_trade=True)
        whole = _native.xccy_scenario_pv(gpu_ctx, *case.args, tr, per_trade=True)
        dev_rows, dev_pv = _run_dev(gpu_ctx, case, tr, case.dfs_f, case.dfs_x, True, sub_off=case.sub_off)
        rows_only, none = _run_dev(gpu_ctx, case, tr, case.dfs_f, case.dfs_x, False, sub_off=case.sub_off)
    assert np.array_equal(sub["pv"], whole["pv"]) and np.array_equal(dev_pv, whole["pv"]) and none is None
    assert np.array_equal(dev_rows, sub["sub_pv"]) and np.array_equal(rows_only, sub["sub_pv"])
    for b, (lo, hi) in enumerate(zip(case.sub_off[:-1], case.sub_off[1:])):
        if lo == hi:
            assert np.all(sub["sub_pv"][b] == 0.0) and not np.any(np.signbit(sub["sub_pv"][b]))
            continue
        alone = _device(gpu_ctx, case, XC.take(case.batch, int(lo), int(hi)))
        assert np.array_equal(sub["sub_pv"][b], alone["book_pv"]), b


def test_dev_entry_on_a_callers_stream(gpu_ctx):
    case = XC.cases()[0]
    first = _device(gpu_ctx, case)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    with _native.DeviceTrades(gpu_ctx, case.batch) as tr:
        with torch.cuda.stream(stream):
            book, pv = _run_dev(gpu_ctx, case, tr, case.dfs_f, case.dfs_x, True, stream.cuda_stream)
            book_only, none = _run_dev(gpu_ctx, case, tr, case.dfs_f, case.dfs_x, False, stream.cuda_stream)
        assert none is None and np.array_equal(pv, first["pv"]) and np.array_equal(book, first["book_pv"])
        assert np.array_equal(book_only, book)
        head = (gpu_ctx, 1, case.times_f.size, 3, 1, case.times_x.size, 3, 3, tr)
        with pytest.raises(LibError, match="work is NULL"):
            _native.xccy_scenario_pv_dev(*head, dict(times_f=1, dfs_f=1, times_x=1, dfs_x=1), 1, 0)
        with pytest.raises(LibError, match="S_f and S_x"):
            _native.xccy_scenario_pv_dev(gpu_ctx, 1, case.times_f.size, 2, 1, case.times_x.size, 3, 3, tr,
                                         dict(times_f=1, dfs_f=1, times_x=1, dfs_x=1), 1, 1)
        with pytest.raises(LibError, match="LINEAR_FWD_RATES") as e:
            _native.xccy_scenario_pv_dev(gpu_ctx, 2, case.times_f.size, 3, 1, case.times_x.size, 3, 3, tr,
                                         dict(times_f=1, dfs_f=1, times_x=1, dfs_x=1), 1, 1)
        assert e.value.status == _native.ADR_ERR_UNSUPPORTED
        with pytest.raises(LibError, match="plan is NULL"):
            _native.xccy_scenario_subbook_pv_dev(*head, 2, dict(times_f=1, dfs_f=1, times_x=1, dfs_x=1), 1, 1)


def test_book_revalue_on_the_device_against_the_host_twins(gpu_ctx):
    from adrates_amd.market.position.xccy_book import XccyBook
    from .test_xccy_book_host import joint_shocks, small_book
    model, swaps, keys = small_book()
    book = XccyBook(swaps, model)
    kw = joint_shocks(model)
    dev, host = book.revalue(per_trade=True, **kw), book.revalue(per_trade=True, host=True, **kw)
    notional = np.array([s._domestic_notional for s in swaps])
    assert np.max(np.abs(dev["pv"] - host["pv"]) / notional[None, :]) <= 1e-10
    assert np.max(np.abs(dev["book_pv"] - host["book_pv"])) <= 1e-10 * notional.sum()
    sub_d, sub_h = book.revalue_sub_books(keys, **kw), book.revalue_sub_books(keys, host=True, **kw)
    assert sub_d["labels"] == sub_h["labels"] and np.max(np.abs(sub_d["sub_pv"] - sub_h["sub_pv"])) <= 1e-10 * notional.sum()
    zero = {k: (None if v is None else np.zeros_like(np.asarray(v, dtype=np.float64))) for k, v in kw.items()}
    assert np.all(book.pnl(**zero) == 0.0) and np.all(book.pnl_sub_books(keys, **zero) == 0.0)
