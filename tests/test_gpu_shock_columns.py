"""The shock-column and row-merge kernels on the GPU (adr_shock_columns*, adr_scenario_rows_merge_dev,
csrc/shock_columns.hip) on the tables of tests/_firm_revalue_cases.py: the device-array entries in guarded buffers against
their CPU twins bit for bit, the flags set and kept, the rows a merge does not name left alone, and the scalar refusals."""
import numpy as np
import pytest
import torch

from adrates_amd import _native
from adrates_amd.utils.error import LibError

from . import _firm_revalue_cases as FC
from .test_gpu_monte_carlo import GUARD
from .test_gpu_monte_carlo_revalue import guard_intact, guarded

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("col0,n,extra", FC.COLUMN_CUTS)
@pytest.mark.parametrize("S", FC.COLUMN_S)
def test_columns_dev_in_guarded_buffers(gpu_ctx, S, col0, n, extra):
    """adr_shock_columns_dev on a caller's stream, without a base and with one: the twin's bits, 16 guard words intact
    behind every buffer; a NaN and a breakeven below the floor set their rows' flags, a flag that was set stays."""
    ld = col0 + n + extra
    x = FC.column_rows(S, ld)
    flags = np.zeros(S, dtype=np.int32)
    flags[S // 2] = 7
    if S > 2:
        x[S - 1, col0 + n - 1], x[1, col0] = np.nan, -3e4              # (row 1: base - 3 < -1)
    base = FC.column_base(n)
    shocks, d_base = guarded(x), guarded(base)
    stream = torch.cuda.Stream()
    for with_base in (False, True):
        out, bad = guarded(np.full(S * n, GUARD)), guarded(flags, torch.int32)
        torch.cuda.synchronize()
        _native.shock_columns_dev(gpu_ctx, S, ld, shocks.data_ptr(), col0, n, out.data_ptr(), base_ptr=d_base.data_ptr() if with_base else 0,
                                  floor=-1.0 if with_base else None, bad_ptr=bad.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        ref, ref_bad = _native.shock_columns_host(x, col0, n, base=base if with_base else None, floor=-1.0 if with_base else None, bad=flags)
        assert guard_intact(out, S * n) and guard_intact(bad, S) and guard_intact(shocks, x.size) and guard_intact(d_base, n)
        assert FC.same_bits(out[:S * n].cpu().numpy().reshape(S, n), ref), with_base
        assert np.array_equal(bad[:S].cpu().numpy(), ref_bad) and ref_bad[S // 2] in (1, 7)
        if S > 2:
            assert ref_bad[S - 1] == 1 and (ref_bad[1] == 1) == with_base
        again = guarded(np.full(S * n, GUARD))                          # without the flags: the same columns
        _native.shock_columns_dev(gpu_ctx, S, ld, shocks.data_ptr(), col0, n, again.data_ptr(), base_ptr=d_base.data_ptr() if with_base else 0,
                                  floor=-1.0 if with_base else None, stream=stream.cuda_stream)
        stream.synchronize()
        assert guard_intact(again, S * n) and FC.same_bits(again.cpu().numpy(), out.cpu().numpy())
    assert np.array_equal(FC.bits(shocks[:x.size].cpu().numpy()), FC.bits(x.ravel())), "the shock rows are only read"


def test_columns_blocking_entry(gpu_ctx):
    x, base = FC.column_rows(257, 44), FC.column_base(12)
    x[5, 41] = np.inf
    for kw in (dict(), dict(base=base, floor=-1.0), dict(base=base, floor=-1.0, bad=np.arange(257) % 3)):
        out, bad = _native.shock_columns(gpu_ctx, x, 32, 12, **kw)
        ref, ref_bad = _native.shock_columns_host(x, 32, 12, **kw)
        assert FC.same_bits(out, ref) and np.array_equal(bad, ref_bad) and bad[5] == 1


@pytest.mark.parametrize("B,S_tile,S_tot", FC.MERGE_SHAPES)
def test_merge_dev_leaves_the_other_rows_and_columns(gpu_ctx, B, S_tile, S_tot):
    """Permuted targets, copy and add mixed, one target out of range: the twin's bits, everything else untouched."""
    tile, rows, s0, target, add, B_tot = FC.merge_case(B, S_tile, S_tot)
    d_tile, d_target, d_add = guarded(tile), guarded(target, torch.int64), guarded(add, torch.int32)
    stream = torch.cuda.Stream()
    for flags, d_flags in ((add, d_add.data_ptr()), (None, 0)):
        d_rows = guarded(rows)
        torch.cuda.synchronize()
        _native.scenario_rows_merge_dev(gpu_ctx, B, S_tile, d_tile.data_ptr(), B_tot, S_tot, s0, d_rows.data_ptr(), d_target.data_ptr(),
                                        d_flags, stream=stream.cuda_stream)
        stream.synchronize()
        want = _native.scenario_rows_merge_host(tile, rows.copy(), s0, target, flags)
        got = d_rows[:rows.size].cpu().numpy().reshape(rows.shape)
        assert guard_intact(d_rows, rows.size) and np.array_equal(FC.bits(got), FC.bits(want))
        named = np.zeros(rows.shape, dtype=bool)
        named[target[(target >= 0) & (target < B_tot)], s0:s0 + S_tile] = True
        assert np.array_equal(FC.bits(got[~named]), FC.bits(rows[~named])) and np.count_nonzero(named) == (B - (B > 1)) * S_tile
    assert guard_intact(d_tile, tile.size) and guard_intact(d_target, B) and guard_intact(d_add, B)


def test_dev_entry_refusals(gpu_ctx):
    buf = torch.full((4096,), GUARD, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    for S, ld, x, col0, n, out in ((0, 4, p, 0, 2, p), (4, 4, p, 0, 0, p), (4, 4, p, -1, 2, p), (4, 4, p, 3, 2, p), (4, 1, p, 0, 2, p),
                                   (4, 4, 0, 0, 2, p), (4, 4, p, 0, 2, 0)):
        with pytest.raises(LibError) as e:
            _native.shock_columns_dev(gpu_ctx, S, ld, x, col0, n, out)
        assert e.value.status == -1, (S, ld, col0, n)
    for args in ((0, 4, p, 3, 8, 0, p, p), (2, 0, p, 3, 8, 0, p, p), (2, 4, p, 0, 8, 0, p, p), (2, 4, p, 3, 0, 0, p, p), (2, 4, p, 3, 8, 5, p, p),
                 (2, 4, p, 3, 8, -1, p, p), (2, 4, 0, 3, 8, 0, p, p), (2, 4, p, 3, 8, 0, 0, p), (2, 4, p, 3, 8, 0, p, 0)):
        with pytest.raises(LibError) as e:
            _native.scenario_rows_merge_dev(gpu_ctx, *args)
        assert e.value.status == -1, args
    with pytest.raises(LibError) as e:
        _native.shock_columns(gpu_ctx, np.zeros((4, 4)), 3, 2)
    assert e.value.status == -1
    gpu_ctx.sync()
    assert bool((buf == GUARD).all())
