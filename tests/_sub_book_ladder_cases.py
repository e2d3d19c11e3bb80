"""Books, desk layouts and comparisons shared by the sub-book ladder tests (tests/test_sub_book_ladders_host.py, CPU, and
tests/test_gpu_sub_book_ladders.py, GPU)."""
import numpy as np

from adrates_amd.market.curves.curve_tables import build_engine_curve
from adrates_amd.market.position.scenarios import _concat_batches, _permute_batch
from adrates_amd.trades import synthetic
from adrates_amd.trades.compiler import compile_bonds, compile_frns
from oracle import port

from . import _fixtures as F
from . import _scenario_cases as SC

VD = SC.VD
SCHEMES = SC.SCHEMES
# Trades per desk of the geometry book: every chunk edge, an empty desk inside and last.
GEOMETRY_SIZES = (1, 63, 64, 0, 65, 129, 0)


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def take(batch, lo, hi):
    return _permute_batch(batch, np.arange(lo, hi, dtype=np.int64))[0]


def shifted(batch, trades, years):
    """The batch with every date of ``trades`` moved ``years`` back: seasoned trades (some flows in the past), or, far
    enough back, trades with no live flow."""
    for i in trades:
        f = slice(int(batch.fix_off[i]), int(batch.fix_off[i + 1]))
        l = slice(int(batch.flt_off[i]), int(batch.flt_off[i + 1]))
        batch.fix_tp[f] -= years
        for name in ("flt_tp", "flt_ts", "flt_te"):
            getattr(batch, name)[l] -= years
    return batch


def with_notionals(batch, seed):
    """Notionals from 1 to 1e8, log-uniform."""
    batch.notional = 10.0 ** np.random.default_rng(seed).uniform(0.0, 8.0, batch.n_trades)
    return batch


def mixed_book(n_ois=300, seed=3):
    """Lag-free OIS off and on the grid (every seventh seasoned by 0.4 years), 50 bonds and 50 FRNs, both signs."""
    ois = _concat_batches([synthetic.synthesize(VD, n_ois // 2, kind="offgrid", seed=seed),
                           synthetic.synthesize(VD, n_ois - n_ois // 2, kind="ongrid", seed=seed + 1)])
    ois = with_notionals(shifted(ois, range(0, ois.n_trades, 7), 0.4), seed)
    bonds, _ = F.random_bond_book(VD, 50, seed=5)
    return _concat_batches([ois, compile_bonds(bonds, VD), lag_free_frns(50)])


def lag_free_frns(n, seed=6):
    """The first ``n`` FRNs of a random book whose coupons are all paid on their accrual end."""
    from adrates_amd.market.position.sub_book_ladders import has_ratio_node
    frns, _ = F.random_frn_book(VD, 4 * n, seed=seed)
    batch = compile_frns(frns, VD)[0]
    keep = np.nonzero(~has_ratio_node(batch))[0][:n]
    assert keep.size == n
    return _permute_batch(batch, keep)[0]


def geometry_book(seed=11):
    """sum(GEOMETRY_SIZES) lag-free OIS; trades 5 and 70 have no live flow, every ninth is seasoned."""
    b = synthetic.synthesize(VD, int(sum(GEOMETRY_SIZES)), seed=seed)
    shifted(b, range(0, b.n_trades, 9), 0.3)
    shifted(b, (5, 70), 60.0)
    return with_notionals(b, seed)


def curve_arrays(interp):
    curve = F.gbp_model(VD, interp).curves.GBP_OIS_SONIA
    return build_engine_curve(curve.swap_rates, curve.swap_times, curve.year_fracs)


def oracle_rows(method, host, batch):
    return port.price(method, host.times, host.dfs, host.jac, host.hess, batch)


def desk_errors(got, ref, sub_off):
    """Worst |desk row - sum of the per-trade rows| over the desk's sum of absolute per-trade entries (assert_book's scale
    in tests/test_gpu_aggregate_only.py), over the desks and the three blocks."""
    worst = 0.0
    for b, (lo, hi) in enumerate(zip(sub_off[:-1], sub_off[1:])):
        for key in ("pv", "delta", "gamma"):
            r = np.asarray(ref[key][lo:hi])
            g = np.asarray(got[key][b])
            if hi == lo:
                assert not np.any(g) and not np.any(np.signbit(g)), f"empty desk {b} {key}"
                continue
            scale = float(np.max(np.abs(r).sum(0)))
            worst = max(worst, float(np.max(np.abs(g - r.sum(0)))) / max(scale, 1e-300))
    return worst


def rows_errors(got, want, ref, sub_off):
    """Worst |got - want| per desk on the same scale (the oracle's absolute sums of that desk)."""
    worst = 0.0
    for b, (lo, hi) in enumerate(zip(sub_off[:-1], sub_off[1:])):
        if hi == lo:
            continue
        for key in ("pv", "delta", "gamma"):
            scale = float(np.max(np.abs(np.asarray(ref[key][lo:hi])).sum(0)))
            worst = max(worst, float(np.max(np.abs(np.asarray(got[key][b]) - np.asarray(want[key][b])))) / max(scale, 1e-300))
    return worst


def same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.int64), np.asarray(b[k]).view(np.int64)) for k in ("pv", "delta", "gamma"))
