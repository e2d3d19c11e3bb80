"""The CPU twins of the shock-column and row-merge entries (adr_shock_columns_host, adr_scenario_rows_merge_host,
csrc/shock_columns.hip) on the tables of tests/_firm_revalue_cases.py: the columns against NumPy's two-step arithmetic bit for
bit, on inputs a fused multiply-add would round differently; signed zeros; the flags; the merge against
`combine_sub_book_rows`; the refusals."""
import numpy as np
import pytest

from adrates_amd import _native
from adrates_amd.market.position.scenarios import combine_sub_book_rows
from adrates_amd.utils.error import LibError

from . import _firm_revalue_cases as FC


@pytest.mark.parametrize("col0,n,extra", FC.COLUMN_CUTS)
def test_columns_have_numpys_two_step_bits(native_lib, col0, n, extra):
    """``b0 + x[:, c0:c0 + n] * 1e-4`` and ``x * 1e-4``: a rounded product, then a rounded sum."""
    ld, base = col0 + n + extra, FC.column_base(n)
    seen = 0
    for S in FC.COLUMN_S:
        x = FC.column_rows(S, ld)
        cut = x[:, col0:col0 + n]
        seen += int(np.count_nonzero(FC.fma_differs(base, cut)))
        out, bad = _native.shock_columns_host(x, col0, n, base=base, floor=-1.0)
        assert out.shape == (S, n) and np.array_equal(FC.bits(out), FC.bits(base[None, :] + cut * 1e-4)), S
        assert bad.dtype == np.int32 and not bad.any()
        out, bad = _native.shock_columns_host(x, col0, n)
        assert np.array_equal(FC.bits(out), FC.bits(cut * 1e-4)) and not bad.any(), S
    assert seen >= 1, "no entry of the inputs tells a fused multiply-add from the two roundings"


def test_fused_values_would_differ(native_lib):
    """One rounding and two differ where the sum lands next to a tie, at less than one entry in a hundred: the table's
    widest cut holds 21 of them, and the twin gives the two-step value at every one."""
    x, base = FC.column_rows(257, 44)[:, 32:44], FC.column_base(12)
    differs = FC.fma_differs(base, x)
    assert np.count_nonzero(differs) >= 10
    out, _ = _native.shock_columns_host(x, 0, 12, base=base)
    one = np.array([[FC.fused(b, v) for b, v in zip(base, row)] for row in x])
    assert np.all(out[differs] != one[differs]) and np.array_equal(out[~differs], one[~differs])


def test_signed_zeros(native_lib):
    """Without a base a -0.0 shock stays -0.0; a base of zeros makes it +0.0: the sum is done, not skipped."""
    x = np.array([[-0.0, 0.0, 1.0, -1.0]])
    bare, _ = _native.shock_columns_host(x, 0, 4)
    zeros, _ = _native.shock_columns_host(x, 0, 4, base=np.zeros(4))
    assert np.array_equal(np.signbit(bare[0]), [True, False, False, True])
    assert np.array_equal(np.signbit(zeros[0]), [False, False, False, True])
    assert np.array_equal(bare, zeros) and np.array_equal(FC.bits(bare[:, 1:]), FC.bits(zeros[:, 1:]))
    assert np.array_equal(FC.bits(bare), FC.bits(x * 1e-4)) and np.array_equal(FC.bits(zeros), FC.bits(np.zeros(4) + x * 1e-4))


def test_flags(native_lib):
    """NaN, +inf and -inf, a breakeven of exactly -1 and one just above it; a flag that is set stays set; without a floor
    -1 passes; a column outside the cut is not looked at."""
    base = np.array([0.03, 0.0])
    x = np.zeros((8, 3))
    x[:, 2] = np.nan                                    # beyond the cut
    x[1, 0], x[2, 1], x[3, 0] = np.nan, np.inf, -np.inf
    x[4, 1] = -1e4                                      # -1e4 * 1e-4 rounds to -1 exactly; the assertion below holds the table to it
    x[5, 1] = -1e4 * (1.0 - 2.0 ** -40)
    x[6, 0] = 1e300
    out, bad = _native.shock_columns_host(x, 0, 2, base=base, floor=-1.0, bad=[0, 0, 0, 0, 0, 0, 0, 5])
    assert out[4, 1] == -1.0 and -1.0 < out[5, 1] < -1.0 + 1e-9, "the table must hit -1 exactly and stay just above it"
    assert np.array_equal(bad, [0, 1, 1, 1, 1, 0, 0, 5]) and np.isfinite(out[6, 0])
    assert FC.same_bits(out, base[None, :] + x[:, :2] * 1e-4), "a flagged row is written all the same"
    _, bad = _native.shock_columns_host(x, 0, 2, base=base)
    assert np.array_equal(bad, [0, 1, 1, 1, 0, 0, 0, 0]), "no floor"
    _, bad = _native.shock_columns_host(x, 0, 2, base=base, floor=-0.5)
    assert np.array_equal(bad, [0, 1, 1, 1, 1, 1, 0, 0]), "another floor"
    _, bad = _native.shock_columns_host(x, 0, 3)
    assert bad.all()


@pytest.mark.parametrize("B,S_tile,S_tot", FC.MERGE_SHAPES)
def test_merge_twin(native_lib, B, S_tile, S_tot):
    tile, rows, s0, target, add, _ = FC.merge_case(B, S_tile, S_tot)
    got = _native.scenario_rows_merge_host(tile, rows.copy(), s0, target, add)
    assert np.array_equal(FC.bits(got), FC.bits(FC.merge_numpy(tile, rows, s0, target, add)))
    got = _native.scenario_rows_merge_host(tile, rows.copy(), s0, target)
    assert np.array_equal(FC.bits(got), FC.bits(FC.merge_numpy(tile, rows, s0, target, None))), "add NULL: every row copied"


def test_merge_twin_is_combine_sub_book_rows(native_lib):
    """Three parts with shared labels, merged one after another in list order."""
    rng = np.random.default_rng(3)
    parts = [(["a", "b", "c"], rng.standard_normal((3, 70))), (["c", "d", "a"], rng.standard_normal((3, 70))),
             (["e", "a"], rng.standard_normal((2, 70)))]
    want = combine_sub_book_rows(parts)
    rows, seen = np.full((5, 70), np.nan), set()
    for labs, part in parts:
        _native.scenario_rows_merge_host(part, rows, 0, [want["labels"].index(lab) for lab in labs], [lab in seen for lab in labs])
        seen.update(labs)
    assert want["labels"] == ["a", "b", "c", "d", "e"] and np.array_equal(FC.bits(rows), FC.bits(want["rows"]))


def test_twin_refusals(native_lib):
    x, rows, tile = np.zeros((4, 6)), np.zeros((3, 8)), np.ones((2, 4))
    for args in ((-1, 2), (0, 0), (5, 2), (0, 7)):
        with pytest.raises(LibError) as e:
            _native.shock_columns_host(x, *args)
        assert e.value.status == -1, args
    for call in (lambda: _native.shock_columns_host(x[0], 0, 2), lambda: _native.shock_columns_host(x, 0, 2, base=np.zeros(3)),
                 lambda: _native.shock_columns_host(x, 0, 2, bad=np.zeros(3)),
                 lambda: _native.scenario_rows_merge_host(tile, rows, 0, [0]),
                 lambda: _native.scenario_rows_merge_host(tile, rows, 0, [0, 1], [1]),
                 lambda: _native.scenario_rows_merge_host(tile, rows.astype(np.float32), 0, [0, 1])):
        with pytest.raises(LibError):
            call()
    for s0, target in ((5, [0, 1]), (-1, [0, 1]), (0, [1, 1]), (2, [2, 2])):
        with pytest.raises(LibError) as e:
            _native.scenario_rows_merge_host(tile, rows, s0, target)
        assert e.value.status == -1, (s0, target)
    assert not rows.any(), "a refused call writes nothing"
    _native.scenario_rows_merge_host(tile, rows, 4, [7, -3])               # two targets out of range are no repeat
    assert not rows.any()
