"""The tail allocation on the device (adr_scenario_tail_alloc, _dev): bit for bit against the CPU twin and the NumPy
restatement of tests/_tail_alloc_cases.py.  The CPU twin itself: tests/test_tail_alloc_host.py."""
import numpy as np
import pytest
import torch

from adrates_amd import _native
from adrates_amd.market.position.scenarios import allocate_tail, tail_count
from adrates_amd.utils.error import LibError

from . import _tail_alloc_cases as TA

pytestmark = pytest.mark.gpu
GUARD = -1.2345e300
TAIL = 16


@pytest.mark.parametrize("S", TA.S_VALUES)
def test_shapes_against_the_host_twin_and_the_restatement(gpu_ctx, S):
    for rows, base_col, k in TA.calls(S):
        got = _native.scenario_tail_alloc(gpu_ctx, rows, k, base_col)
        assert TA.same_result(got, _native.scenario_tail_alloc_host(rows, k, base_col)), (rows.shape, base_col, k)
        TA.check(got, rows, base_col, k)


def test_ties_zeros_equal_rows_and_nan(gpu_ctx):
    for name, rows, base_col, k in TA.special_calls():
        got = _native.scenario_tail_alloc(gpu_ctx, rows, k, base_col)
        assert TA.same_result(got, _native.scenario_tail_alloc_host(rows, k, base_col)), name
        TA.check(got, rows, base_col, k)
        if name == "the k-th and the (k+1)-th tie":
            assert np.array_equal(got["comp_var"], TA.tie_expectation()) and got["var"] == 3.0
    for rows, base_col, k in TA.nan_calls():
        got = _native.scenario_tail_alloc(gpu_ctx, rows, k, base_col)
        assert all(np.all(np.isnan(got[f])) for f in ("var", "es", "comp_var", "comp_es")), (rows.shape, base_col)


def test_limit_and_the_numpy_fallback(gpu_ctx):
    wide = TA.matrix(5, 8193)
    with pytest.raises(LibError, match=r"\(-2\).*8192"):                  # ADR_ERR_UNSUPPORTED
        _native.scenario_tail_alloc(gpu_ctx, wide, 3)
    k = tail_count(0.999, 8193)
    TA.check(allocate_tail(wide, 0.999, ctx=gpu_ctx), wide, -1, k)        # NumPy under the same rule
    fits = allocate_tail(wide, 0.99, base_col=0, ctx=gpu_ctx)             # 8 192 values beside the base column: the kernel
    assert TA.same_result(fits, _native.scenario_tail_alloc_host(wide, tail_count(0.99, 8192), 0))


def test_dev_entry_on_a_callers_stream_into_guarded_buffers(gpu_ctx):
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    guarded = lambda count: torch.full((count + TAIL,), GUARD, dtype=torch.float64, device=dev)
    for B, S_tot, base_col, k in ((129, 1025, -1, 10), (65, 101, 100, 100), (1, 1, -1, 1), (4097, 64, 0, 2)):
        rows = TA.matrix(B, S_tot)
        rows_t = torch.from_numpy(rows).to(dev)
        var, es, cv, ce, work = guarded(1), guarded(1), guarded(B), guarded(B), guarded(S_tot)
        with torch.cuda.stream(stream):
            _native.scenario_tail_alloc_dev(gpu_ctx, B, S_tot, rows_t.data_ptr(), k, var.data_ptr(), es.data_ptr(), cv.data_ptr(),
                                            ce.data_ptr(), work.data_ptr(), base_col=base_col, stream=stream.cuda_stream)
            stream.synchronize()
        for buf, count in ((var, 1), (es, 1), (cv, B), (ce, B), (work, S_tot)):
            assert torch.all(buf[count:] == GUARD), (B, S_tot, count)
        got = {"var": var[:1].cpu().numpy(), "es": es[:1].cpu().numpy(), "comp_var": cv[:B].cpu().numpy(),
               "comp_es": ce[:B].cpu().numpy()}
        assert TA.same_result(got, _native.scenario_tail_alloc_host(rows, k, base_col)), (B, S_tot)
        assert torch.equal(rows_t.cpu(), torch.from_numpy(rows))
    with pytest.raises(LibError, match="work is NULL"):
        _native.scenario_tail_alloc_dev(gpu_ctx, 1, 1, rows_t.data_ptr(), 1, var.data_ptr(), es.data_ptr(), cv.data_ptr(),
                                        ce.data_ptr(), 0)
