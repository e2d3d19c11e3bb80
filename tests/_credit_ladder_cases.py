"""Books, desk and bucket layouts, the reference and the comparisons shared by the credit sub-book ladder tests
(tests/test_credit_sub_book_ladders_host.py, CPU, and tests/test_gpu_credit_sub_book_ladders.py, GPU).

Every output of adr_credit_subbook_ladders is linear in the flows' amounts, so the reference is the C oracle
(`_sub_book_ladder_cases.oracle_rows`) on the batch rescaled as `_credit_scenario_cases.rescaled` does it - ``fix_pay`` and
``flt_weight`` times a weight per flow: ``f = exp(-z tau)`` gives PV, delta and gamma at the spreads, ``-tau f`` gives
``cs01 = 1e-4 PV`` and ``cross = 1e-4 delta``, ``tau^2 f`` gives ``spread_gamma = 1e-8 PV`` - summed per desk and per cell."""
import dataclasses

import numpy as np

from adrates_amd import _native
from adrates_amd.market.position.scenarios import _concat_batches, _permute_batch
from adrates_amd.trades.compiler import compile_bonds

from . import _credit_scenario_cases as CC
from . import _fixtures as F
from . import _sub_book_ladder_cases as L

BP = CC.BP
Case = CC.Case
GEOMETRY_SIZES = L.GEOMETRY_SIZES
BLOCKS = ("pv", "delta", "gamma", "cs01", "spread_gamma", "cross_gamma")


def permute(case, perm):
    """The case with trade j = trade perm[j]."""
    batch, fi, li = _permute_batch(case.batch, np.asarray(perm, dtype=np.int64))
    return Case(batch, case.z[perm], case.bucket[perm], case.fix_tau[fi], case.flt_tau[li])


def take(case, lo, hi):
    return permute(case, np.arange(lo, hi, dtype=np.int64))


def order_by_cells(case, desk, B):
    """``(case ordered by (desk, bucket) with a stable sort, sub_off, perm)``; ``desk [n]``: the desk number per trade, of
    ``B`` desks."""
    desk = np.asarray(desk, dtype=np.int64)
    perm = np.lexsort((case.bucket, desk))                 # stable: the last key is the primary one
    sub_off = np.searchsorted(desk[perm], np.arange(B + 1), side="left").astype(np.int64)
    return permute(case, perm), sub_off, perm


def credit_book(n_bonds, n_frns, seed):
    """Bonds and lag-free FRNs mixed by a fixed shuffle (no spreads yet)."""
    bonds, _ = F.random_bond_book(L.VD, n_bonds, seed=seed)
    both = _concat_batches([compile_bonds(bonds, L.VD), L.lag_free_frns(n_frns, seed=seed + 1)])
    return _permute_batch(both, np.random.default_rng(seed).permutation(both.n_trades))[0]


def spreads_for(batch, bucket, seed):
    """z from -50 to 800 bp with both ends present and every sixth trade at z = 0; spread times tau = t for the float
    coupons and, per trade, t or t * 365 / 365.25 for the fixed flows."""
    rng = np.random.default_rng(seed)
    n = batch.n_trades
    z = rng.uniform(-50 * BP, 800 * BP, n)
    z[::6] = 0.0
    z[n // 2] = 800 * BP
    z[n - 1] = -50 * BP
    scale = np.where(rng.random(n) < 0.5, 1.0, 365.0 / 365.25)
    fix_tau = batch.fix_tp * np.repeat(scale, np.diff(batch.fix_off))
    return Case(batch, z, np.asarray(bucket, dtype=np.int32), fix_tau, batch.flt_tp.copy())


def geometry_buckets(G):
    """Buckets for desks of GEOMETRY_SIZES trades: desk 0 one trade in bucket 0; desk 1 (63) only the first and the last
    bucket (it lacks the others); desk 2 (64) all unbucketed; desk 4 (65) ONE cell of 65 trades, two chunks; desk 5 (129)
    every one of the G + 1 cells, the unbucketed one included."""
    out = []
    for b, size in enumerate(GEOMETRY_SIZES):
        j = np.arange(size)
        if b == 1:
            raw = np.where(j % 3 == 0, 0, G - 1)
        elif b == 2:
            raw = np.full(size, -1)
        elif b == 4:
            raw = np.full(size, G // 2)
        elif b == 5:
            raw = j % (G + 1) - 1
        else:
            raw = np.zeros(size, dtype=np.int64)
        out.append(np.where(raw < G, raw, -1) if G > 0 else np.full(size, -1))
    return np.concatenate(out).astype(np.int32)


_BOOKS = {}


def geometry_case(G):
    """``(case, sub_off)``: sum(GEOMETRY_SIZES) bonds and lag-free FRNs in desks of those sizes, ordered by cell."""
    if "geometry" not in _BOOKS:
        _BOOKS["geometry"] = credit_book(200, int(sum(GEOMETRY_SIZES)) - 200, seed=21)
    book = _BOOKS["geometry"]
    desk = np.repeat(np.arange(len(GEOMETRY_SIZES)), GEOMETRY_SIZES)
    case, sub_off, _ = order_by_cells(spreads_for(book, geometry_buckets(G), 40 + G), desk, len(GEOMETRY_SIZES))
    return case, sub_off


def mixed_case(G, B=5):
    """``(case, sub_off)``: `_sub_book_ladder_cases.mixed_book` dressed by `_credit_scenario_cases.dress`, its trades dealt
    to ``B`` desks at random and ordered by cell."""
    if "mixed" not in _BOOKS:
        _BOOKS["mixed"] = L.mixed_book()
    case = CC.dress(_BOOKS["mixed"], G, 300 + G)
    desk = np.random.default_rng(G).integers(0, B, case.batch.n_trades)
    desk[:B] = np.arange(B)
    case, sub_off, _ = order_by_cells(case, desk, B)
    return case, sub_off


def weighted(case, fix_w, flt_w):
    b = case.batch
    w = np.ones(b.flt_tp.shape[0]) if b.flt_weight is None else b.flt_weight
    return dataclasses.replace(b, fix_pay=b.fix_pay * fix_w, flt_weight=w * flt_w)


_REF = {}


def reference(method, host, case, key=None):
    """Per-trade rows of the oracle: ``pv [n]``, ``delta [n, P]``, ``gamma [n, P, P]`` at the spreads, ``cs01 [n]``,
    ``spread_gamma [n]``, ``cross [n, P]``.  ``key``: computed once per key and shared."""
    if key is not None and key in _REF:
        return _REF[key]
    b = case.batch
    zf, zl = np.repeat(case.z, np.diff(b.fix_off)), np.repeat(case.z, np.diff(b.flt_off))
    ff, fl = np.exp(-zf * case.fix_tau), np.exp(-zl * case.flt_tau)
    at = L.oracle_rows(method, host, weighted(case, ff, fl))
    d1 = L.oracle_rows(method, host, weighted(case, -case.fix_tau * ff, -case.flt_tau * fl))
    d2 = L.oracle_rows(method, host, weighted(case, case.fix_tau ** 2 * ff, case.flt_tau ** 2 * fl))
    ref = {"pv": np.asarray(at["pv"]), "delta": np.asarray(at["delta"]), "gamma": np.asarray(at["gamma"]),
           "cs01": 1e-4 * np.asarray(d1["pv"]), "cross": 1e-4 * np.asarray(d1["delta"]), "spread_gamma": 1e-8 * np.asarray(d2["pv"])}
    if key is not None:
        _REF[key] = ref
    return ref


def errors(got, ref, case, sub_off, G):
    """Worst |entry - sum of the per-trade entries| over the sum of their absolute values (`desk_errors`' scale), over the
    desks' curve blocks and the cells' spread entries, as ``{"desk": .., "cell": ..}``.  Asserts that an empty desk and a
    bucket a desk does not hold are +0.0 with no sign bit."""
    worst = {"desk": L.desk_errors(got, ref, sub_off), "cell": 0.0}
    for b, (lo, hi) in enumerate(zip(sub_off[:-1], sub_off[1:])):
        for g in range(G):
            idx = lo + np.nonzero(case.bucket[lo:hi] == g)[0]
            mine = {"cs01": got["cs01"][b, g], "spread_gamma": got["spread_gamma"][b, g], "cross": got["cross_gamma"][b, g]}
            for k, v in mine.items():
                v = np.asarray(v)
                if idx.size == 0:
                    assert not np.any(v) and not np.any(np.signbit(v)), f"desk {b} holds no bucket {g}: {k}"
                    continue
                r = np.asarray(ref[k][idx])
                scale = float(np.max(np.abs(r).sum(0)))
                worst["cell"] = max(worst["cell"], float(np.max(np.abs(v - r.sum(0)))) / max(scale, 1e-300))
    return worst


def check_layout(got, P, G):
    """The augmented rows against the blocks: symmetric cross terms bit for bit, a diagonal spread block, zeros elsewhere."""
    Q = P + G
    rows = got["ladders"]
    assert rows.shape[1] == 1 + Q + Q * Q
    g = rows[:, 1 + Q:].reshape(-1, Q, Q)
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)
    assert np.array_equal(bits(g[:, :P, P:]), bits(np.swapaxes(g[:, P:, :P], 1, 2))), "cross rows and columns differ"
    assert np.array_equal(bits(g[:, P:, :P]), bits(got["cross_gamma"]))
    ss = g[:, P:, P:].copy()
    ss[:, np.arange(G), np.arange(G)] = 0.0
    assert not np.any(ss) and not np.any(np.signbit(ss)), "the spread-spread block is not diagonal"
    assert np.array_equal(bits(rows[:, 0]), bits(got["pv"])) and np.array_equal(bits(rows[:, 1 + P:1 + Q]), bits(got["cs01"]))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a["ladders"]).view(np.int64), np.ascontiguousarray(b["ladders"]).view(np.int64))


def row_of(got, b):
    return {"ladders": got["ladders"][b:b + 1]}


def host_ladders(method, host, case, G, sub_off, hess=True, **kw):
    return _native.credit_subbook_ladders_host(method, host.times, host.dfs, host.jac, host.hess if hess else None, case.batch,
                                               case.z, case.bucket, case.fix_tau, case.flt_tau, G, sub_off, **kw)


def device_ladders(ctx, dc, case, G, sub_off, **kw):
    with _native.DeviceTrades(ctx, case.batch) as dt:
        return _native.credit_subbook_ladders(ctx, dc, dt, case.z, case.bucket, case.fix_tau, case.flt_tau, G, sub_off, **kw)


def between(got, want, ref, case, sub_off, G):
    """Worst |got - want| on `errors`' scales (the device against the host twin)."""
    diff = {k: np.asarray(got[k]) - np.asarray(want[k]) for k in BLOCKS}
    worst = 0.0
    for b, (lo, hi) in enumerate(zip(sub_off[:-1], sub_off[1:])):
        if hi == lo:
            continue
        for k in ("pv", "delta", "gamma"):
            scale = float(np.max(np.abs(np.asarray(ref[k][lo:hi])).sum(0)))
            worst = max(worst, float(np.max(np.abs(diff[k][b]))) / max(scale, 1e-300))
        for g in range(G):
            idx = lo + np.nonzero(case.bucket[lo:hi] == g)[0]
            if idx.size == 0:
                continue
            for k, r in (("cs01", "cs01"), ("spread_gamma", "spread_gamma"), ("cross_gamma", "cross")):
                scale = float(np.max(np.abs(ref[r][idx]).sum(0)))
                worst = max(worst, float(np.max(np.abs(diff[k][b, g]))) / max(scale, 1e-300))
    return worst


# ------------------------------------------------------------------------------------------- against full revaluation
STEPS = (4.0, 8.0, 16.0)                                    # basis points
EXPLAIN_BUCKETS = ("AA", "A", "BBB", "HY")
# (desk label, direction) pairs, by scheme, that leave the bands in the REFERENCE itself - the oracle-derived ladders against
# adr_credit_scenario_subbook_pv_host, `out_of_band` - because the desk's third-order term nearly cancels in that
# direction: bad inputs, not checked; 1 of 30 per scheme at most (the limit is one in ten).  Under LINEAR_FWD_RATES the
# reference's delta-gamma ratios of desk ("frns", 1) in direction 3 (linspace curve move, spreads together) are 7.06, 5.89.
EXPLAIN_DROPPED = {"LINEAR_FWD_RATES": ((("frns", 1), 3),)}


def explain_book():
    """``(trades, spreads, keys, buckets)``: long-only bonds in two desks, lag-free FRNs in two desks and one OIS desk, the
    kinds interleaved in the list; bonds and FRNs in four rating buckets, z from 20 to 400 bp."""
    from adrates_amd.market.position.sub_book_ladders import has_ratio_node
    from adrates_amd.trades.compiler import compile_frns
    from adrates_amd.trades.market_data import make_swap
    bonds, _ = F.random_bond_book(L.VD, 14, seed=5)
    frns, _ = F.random_frn_book(L.VD, 60, seed=6)
    frns = [f for f, r in zip(frns, has_ratio_node(compile_frns(frns, L.VD)[0])) if not r][:10]
    assert len(frns) == 10
    swaps = [make_swap(L.VD, t, 0.04 + 0.001 * i, 1e6 * (i + 1), pay=bool(i % 2)) for i, t in enumerate(("2Y", "87M", "10Y", "30Y", "5Y"))]
    rng = np.random.default_rng(9)
    rows = [(b, float(rng.uniform(20, 400)) * BP, ("bonds", i % 2), EXPLAIN_BUCKETS[i % 4]) for i, b in enumerate(bonds)]
    rows += [(f, float(rng.uniform(20, 400)) * BP, ("frns", i % 2), EXPLAIN_BUCKETS[(i + i // 4) % 4]) for i, f in enumerate(frns)]
    rows += [(s, 0.0, "ois", None) for s in swaps]
    rows = [rows[i] for i in np.random.default_rng(10).permutation(len(rows))]
    return tuple(list(col) for col in zip(*rows))


def joint_directions(P, G):
    """``[(u [P], v [G])]``: every curve direction of `_ladder_pnl_cases.directions` with the spreads all moving together
    and with a ramp over the buckets."""
    from ._ladder_pnl_cases import directions
    return [(u, v) for u in directions(P) for v in (np.ones(G), np.linspace(0.5, 2.0, G))]


def joint_shock_rows(P, G):
    """``(x [S, P] bp, dz [S, G] decimals)``: ``h (u, v)`` for every direction and step (rows 3 i + j: direction i, step
    j), then the zero pair."""
    pairs = [(h * u, h * v) for u, v in joint_directions(P, G) for h in STEPS] + [(np.zeros(P), np.zeros(G))]
    return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs]) * BP


def out_of_band(labels, full, delta_pnl, gamma_pnl):
    """The (desk label, direction) pairs that leave either band - for computing EXPLAIN_DROPPED from the reference."""
    r, rd = full - (delta_pnl + gamma_pnl), full - delta_pnl
    bad = []
    for b, label in enumerate(labels):
        for i in range((full.shape[1] - 1) // 3):
            q = [(r[b, 3 * i + j + 1] / r[b, 3 * i + j], rd[b, 3 * i + j + 1] / rd[b, 3 * i + j]) for j in (0, 1)]
            if not all(7.0 <= q3 <= 9.0 and 3.0 <= q2 <= 5.0 for q3, q2 in q):
                bad.append((label, i, q))
    return bad


def check_orders(labels, full, delta_pnl, gamma_pnl, what, dropped=()):
    """`_ladder_pnl_cases.check_orders` for the joint directions: per desk and direction the residual of delta-gamma is
    third order (ratio at doubled shocks in [7, 9]), that of delta alone second order ([3, 5]); the zero pair is exactly 0."""
    r, rd = full - (delta_pnl + gamma_pnl), full - delta_pnl
    last = full.shape[1] - 1
    n_dir = last // 3
    assert len(dropped) * 10 <= len(labels) * n_dir
    assert np.all(full[:, last] == 0.0) and np.all(delta_pnl[:, last] == 0.0) and np.all(gamma_pnl[:, last] == 0.0), what
    q3s, q2s = [], []
    for b, label in enumerate(labels):
        for i in range(n_dir):
            if (label, i) in dropped:
                continue
            for j in (0, 1):
                a, c = 3 * i + j, 3 * i + j + 1
                q3, q2 = r[b, c] / r[b, a], rd[b, c] / rd[b, a]
                assert 7.0 <= q3 <= 9.0, f"{what}: desk {label}, direction {i}, {STEPS[j]} -> {STEPS[j + 1]} bp: delta-gamma ratio {q3}"
                assert 3.0 <= q2 <= 5.0, f"{what}: desk {label}, direction {i}, {STEPS[j]} -> {STEPS[j + 1]} bp: delta-only ratio {q2}"
                q3s.append(q3)
                q2s.append(q2)
    print(f"{what}: delta-gamma ratio {min(q3s):.3f} - {max(q3s):.3f}, delta-only ratio {min(q2s):.3f} - {max(q2s):.3f}")
    return (min(q3s), max(q3s)), (min(q2s), max(q2s))
