"""The schedule-group route of adr_price_dev on a FORCE batch built around its edges: group sizes
around the store pass's segment, 1 to 32 coupons and a chained 33-coupon trade, a semi-annual fixed leg, spreads, a
zero-coupon member, an outlier 1 % off its group's shape, pay and receive - against oracle/port.c, against the direct route,
and through the route's bit contracts.  Then the configurations that batch never reaches (AUTO with only the large
groups in use, batches without a plain row outside the groups, one and two row blocks, more groups than aggregate slices,
the persistent grid, 8 and 9 pillars, one batch on several curves), each held to `standard_checks`, and the store pass's
arithmetic contract, rebuilt on the CPU from the basis ladders."""
import math
from fractions import Fraction

import numpy as np
import pytest

from adrates_amd import _native
from adrates_amd.trades.compiler import TradeBatch
from oracle import port

from . import _fixtures as F
from . import _schedule_group_cases as S
from ._parity import REL_TOL, assert_batch_parity

pytestmark = pytest.mark.gpu
FORCE, OFF, AUTO = _native.SCHEDULE_GROUPS_FORCE, _native.SCHEDULE_GROUPS_OFF, _native.SCHEDULE_GROUPS_AUTO
MIN_GROUP = {FORCE: 2, AUTO: 64}         # the smallest group a mode uses (capi.hip, kScheduleMinGroup)


@pytest.fixture(scope="module")
def book():
    return S.edge_book()


def device_curve(ctx, interp, **kw):
    host = S.curve_arrays(interp, **kw)
    return host, _native.DeviceCurve(ctx, interp.value, host.times, host.dfs, host.jac, host.hess)


def price(ctx, dc, trades, mask=7, agg=True, stream=0, fill=None, guard=False):
    """adr_price_dev into fresh device buffers; ``fill``: what the buffers hold before the call; ``guard``: the delta and
    gamma buffers get one more row than the batch has trades, returned as ``guard``."""
    import torch
    dev = torch.device("cuda", 0)
    n, P = trades.n_trades, dc.n_pillars
    new = (lambda *shape: torch.full(shape, fill, dtype=torch.float64, device=dev)) if fill is not None else \
          (lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev))
    m = n + 1 if guard else n
    delta, gamma = new(m, P), new(m, P, P)
    out = dict(pv=new(n), delta=delta[:n], gamma=gamma[:n], agg=new(1 + P + P * P) if agg else None)
    if guard:
        out["guard"] = (delta[n], gamma[n])
    _native.price_dev(ctx, dc, trades, mask, out["pv"].data_ptr(), out["delta"].data_ptr(), out["gamma"].data_ptr(),
                      out["agg"].data_ptr() if agg else 0, stream)
    ctx.sync()
    return out


def host_rows(out):
    return {k: out[k].cpu().numpy() for k in ("pv", "delta", "gamma")}


def same_bits(a, b, keys=("pv", "delta", "gamma", "agg")):
    import torch
    return all(torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)) for k in keys if a[k] is not None)


def forced(ctx, batch, segment=None):
    trades = _native.DeviceTrades(ctx, batch)
    trades.set_schedule_groups(FORCE, segment)
    return trades


def in_use(batch, mode):
    """Per trade: whether it lies in a group that ``mode`` uses (from the host search)."""
    group_of, *_ = _native.schedule_groups_host(batch)
    sizes = np.bincount(group_of[group_of >= 0], minlength=1)
    return (group_of >= 0) & (sizes >= MIN_GROUP[mode])[np.maximum(group_of, 0)]


def device_parity(got, ref, notional, tol=REL_TOL):
    """`assert_batch_parity` (tests/_parity.py, the same metric term by term) on device tensors: books whose gamma output
    is too large to be compared on the host more than once."""
    import torch
    n = torch.as_tensor(np.abs(np.asarray(notional, dtype=np.float64)), device=got["pv"].device)
    worst = 0.0
    for key, floor in (("pv", 1e-4), ("delta", 1e-8), ("gamma", 1e-12)):
        a, b = got[key].reshape(len(n), -1), ref[key].reshape(len(n), -1)
        d = (a - b).abs()
        scale = torch.maximum(b.abs().amax(1), floor * n)
        unit = (d / n[:, None] / torch.clamp(b.abs() / n[:, None], min=1.0)).amax(1)
        e = float(torch.maximum((d.amax(1) / scale).max(), unit.max()))
        assert e <= tol, f"{key}: worst trade {int(torch.argmax(d.amax(1) / scale))} error {e:.3e} > {tol}"
        worst = max(worst, e)
    return worst


def rows_equal(a, b, idx, keys=("pv", "delta", "gamma")):
    """The trades ``idx`` (a bool array over the batch) carry the same bits in both results."""
    import torch
    at = torch.as_tensor(np.flatnonzero(idx), device=a["pv"].device)
    return all(torch.equal(a[k].index_select(0, at).view(torch.int64), b[k].index_select(0, at).view(torch.int64)) for k in keys)


def standard_checks(ctx, dc, host, interp, batch, trades, mode, ref=None):
    """What every configuration of the route is held to.  ``trades`` is active under ``mode`` and is so again afterwards.
    (a) per-trade parity with oracle/port.c and (b) with the same batch set to OFF at REL_TOL, (c) gamma exactly symmetric,
    (d) the aggregate within 1e-10 of the per-trade sums and of the OFF aggregate, (e) a second run into buffers filled with
    -7.0 repeats the first run's bits (the first run's were filled with 3.0: every element is written, and the guard row
    past the last trade's delta and gamma is not), (f) the trades outside the groups in use carry the OFF run's bits.
    Returns the grouped and the OFF result and the two parity figures."""
    import torch
    P = dc.n_pillars
    assert trades.schedule_groups_info()["active"]
    got = price(ctx, dc, trades, fill=3.0, guard=True)
    again = price(ctx, dc, trades, fill=-7.0, guard=True)
    assert same_bits(got, again)                                                                        # (e)
    for run, fill in ((got, 3.0), (again, -7.0)):
        assert all(bool((g == fill).all()) for g in run["guard"])
    if ref is None:
        ref = port.price(interp.value, host.times, host.dfs, host.jac, host.hess, batch)
    worst = assert_batch_parity(host_rows(got), ref, batch.notional, tol=REL_TOL)                       # (a)
    trades.set_schedule_groups(OFF)
    assert not trades.schedule_groups_info()["active"]
    direct = price(ctx, dc, trades, fill=3.0)
    trades.set_schedule_groups(mode)
    assert trades.schedule_groups_info()["active"]
    vs_direct = device_parity(got, direct, batch.notional)                                              # (b)
    ga, de, pv, ag = got["gamma"], got["delta"], got["pv"], got["agg"]
    assert torch.equal(ga, ga.transpose(1, 2))                                                          # (c)
    assert float((ag[1 + P:].view(P, P) - ga.sum(0)).abs().max()) <= 1e-10 * float(ga.abs().sum(0).max())   # (d)
    assert float((ag[1:1 + P] - de.sum(0)).abs().max()) <= 1e-10 * float(de.abs().sum(0).max())
    assert abs(float(ag[0] - pv.sum())) <= 1e-10 * float(pv.abs().sum())
    assert float((ag - direct["agg"]).abs().max()) <= 1e-10 * float(direct["agg"].abs().max())
    outside = ~in_use(batch, mode)                                                                      # (f)
    if outside.any():                    # (a plain row's bits do not depend on which rows share its table: DESIGN.md section 22)
        assert rows_equal(got, direct, outside)
    return got, direct, worst, vs_direct


@pytest.mark.parametrize("interp", S.SCHEMES)
def test_grouped_route_vs_oracle_and_direct_route(gpu_ctx, book, interp):
    import torch
    batch, marks = book
    host, dc = device_curve(gpu_ctx, interp)
    P = dc.n_pillars
    trades = forced(gpu_ctx, batch)
    info = trades.schedule_groups_info()
    group_of, *_ = _native.schedule_groups_host(batch)
    assert info["active"] and info["segment"] == S.R and info["used_groups"] == info["groups"] == group_of.max() + 1
    assert info["used_trades"] == info["grouped"] == int((group_of >= 0).sum()) < batch.n_trades
    got = price(gpu_ctx, dc, trades)
    again = price(gpu_ctx, dc, trades, fill=0.0)
    assert same_bits(got, again)                                         # two runs: the same bits, the aggregate included
    ref = port.price(interp.value, host.times, host.dfs, host.jac, host.hess, batch)
    worst = assert_batch_parity(host_rows(got), ref, batch.notional, tol=REL_TOL)
    # the direct route on the same batch
    trades.set_schedule_groups(OFF)
    assert not trades.schedule_groups_info()["active"]
    direct = price(gpu_ctx, dc, trades)
    vs_direct = assert_batch_parity(host_rows(got), host_rows(direct), batch.notional, tol=REL_TOL)
    lo, hi = marks["coupons33"]                                          # chained trades: the same launch on both routes
    assert torch.equal(got["gamma"][lo:hi], direct["gamma"][lo:hi]) and torch.equal(got["pv"][lo:hi], direct["pv"][lo:hi])
    ga, de, pv, ag = got["gamma"], got["delta"], got["pv"], got["agg"]
    assert torch.equal(ga, ga.transpose(1, 2))                           # exactly symmetric
    assert float((ag[1 + P:].view(P, P) - ga.sum(0)).abs().max()) <= 1e-10 * float(ga.abs().sum(0).max())
    assert float((ag[1:1 + P] - de.sum(0)).abs().max()) <= 1e-10 * float(de.abs().sum(0).max())
    assert abs(float(ag[0] - pv.sum())) <= 1e-10 * float(pv.abs().sum())
    scale = float(direct["agg"].abs().max())
    assert float((ag - direct["agg"]).abs().max()) <= 1e-10 * scale
    trades.close()
    print(f"{interp.name}: grouped vs oracle {worst:.2e}, vs the direct route {vs_direct:.2e}")


def test_signs_and_doubling_are_exact(gpu_ctx, book):
    import torch
    batch, _ = book
    _, dc = device_curve(gpu_ctx, S.SCHEMES[0])
    runs = []
    for b in (batch, S.flipped(batch), S.doubled(batch)):
        trades = forced(gpu_ctx, b)
        assert trades.schedule_groups_info()["active"]
        runs.append(price(gpu_ctx, dc, trades))
        trades.close()
    base, neg, twice = runs
    for k in ("pv", "delta", "gamma", "agg"):
        assert float((base[k] + neg[k]).abs().max()) == 0.0, k
        assert torch.equal(twice[k], 2.0 * base[k]), k


def test_calls_that_keep_the_direct_route_and_masks_without_value(gpu_ctx, book):
    import torch
    batch, _ = book
    host, dc = device_curve(gpu_ctx, S.SCHEMES[0])
    ref = port.price(4, host.times, host.dfs, host.jac, host.hess, batch)
    trades = forced(gpu_ctx, batch)
    full = price(gpu_ctx, dc, trades)
    # without agg_dev the call takes the direct route: the bits of an OFF batch
    no_agg = price(gpu_ctx, dc, trades, agg=False)
    assert_batch_parity(host_rows(no_agg), ref, batch.notional, tol=REL_TOL)
    # GAMMA alone, DELTA + GAMMA and VALUE + GAMMA: pv / delta are left as they were, what is written equals the full
    # request's bits (VALUE + GAMMA: the store pass runs without a delta pointer and writes the PV)
    for mask, untouched, written in ((4, ("pv", "delta"), ("gamma", "agg")), (6, ("pv",), ("delta", "gamma")),
                                     (5, ("delta",), ("pv", "gamma", "agg"))):
        part = price(gpu_ctx, dc, trades, mask=mask, fill=-7.0)
        for k in untouched:
            assert bool((part[k] == -7.0).all()), (mask, k)
        for k in written:
            if k == "agg":                                               # (whatever the mask: the book's pv, delta, gamma)
                assert float((part[k] - full[k]).abs().max()) <= 1e-10 * float(full[k].abs().max())
            else:
                assert torch.equal(part[k], full[k]), (mask, k)
    trades.set_schedule_groups(OFF)
    direct = price(gpu_ctx, dc, trades, agg=False)
    assert same_bits(no_agg, direct, keys=("pv", "delta", "gamma"))
    trades.close()


def test_segment_lengths_and_a_captured_graph(gpu_ctx, book):
    import torch
    batch, _ = book
    _, dc = device_curve(gpu_ctx, S.SCHEMES[0])
    trades = forced(gpu_ctx, batch)
    base = price(gpu_ctx, dc, trades)
    for segment in (1, 4, 33):                                           # the cut into waves changes no bit
        trades.set_schedule_groups(FORCE, segment)
        assert trades.schedule_groups_info()["segment"] == segment
        assert same_bits(price(gpu_ctx, dc, trades), base)
    trades.set_schedule_groups(FORCE, 0)
    # a grouped call captured into a graph replays to the eager bits
    dev = torch.device("cuda", 0)
    n, P = batch.n_trades, dc.n_pillars
    pv, de = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros((n, P), dtype=torch.float64, device=dev)
    ga, ag = torch.zeros((n, P, P), dtype=torch.float64, device=dev), torch.zeros(1 + P + P * P, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(dev)
    launch = lambda: _native.price_dev(gpu_ctx, dc, trades, 7, pv.data_ptr(), de.data_ptr(), ga.data_ptr(), ag.data_ptr(),
                                       stream.cuda_stream)
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            launch()
        graph.replay()
        stream.synchronize()
    assert same_bits(dict(pv=pv, delta=de, gamma=ga, agg=ag), base)
    trades.close()


@pytest.mark.parametrize("P", [28, 31])
def test_fewer_pillars_even_and_odd(gpu_ctx, book, P):
    """Curves on the first 28 and 31 README tenors keep the packed layout: partial bands of the 16-byte path (784 elements)
    and the 8-byte path of an odd matrix (961 elements, trades 8-byte aligned)."""
    import torch
    batch, _ = book
    base = F.readme_model()._curve_params_dict["GBP_OIS_SONIA"]
    interp = S.SCHEMES[0]
    host, dc = device_curve(gpu_ctx, interp, px=list(base["px_list"][:P]), tenors=list(base["tenor_list"][:P]))
    assert dc.n_pillars == P
    launches, _ = _native.route_host(interp.value, host.times, host.dfs, host.jac, host.hess, batch, 7, True, True)
    assert launches[0][:2] == ("fast", "rows")
    trades = forced(gpu_ctx, batch)
    got = price(gpu_ctx, dc, trades, fill=-7.0)
    ref = port.price(interp.value, host.times, host.dfs, host.jac, host.hess, batch)
    assert_batch_parity(host_rows(got), ref, batch.notional, tol=REL_TOL)
    assert torch.equal(got["gamma"], got["gamma"].transpose(1, 2))
    ga, ag = got["gamma"], got["agg"]
    assert float((ag[1 + P:].view(P, P) - ga.sum(0)).abs().max()) <= 1e-10 * float(ga.abs().sum(0).max())
    trades.close()


def test_auto_needs_enough_grouped_trades(gpu_ctx, book):
    batch, _ = book
    trades = _native.DeviceTrades(gpu_ctx, batch)                        # AUTO: a few thousand trades are below min_grouped
    info = trades.schedule_groups_info()
    assert info["groups"] >= 300 and not info["active"] and info["used_trades"] == 0
    trades.set_schedule_groups(FORCE)
    assert trades.schedule_groups_info()["active"]
    trades.set_schedule_groups(AUTO)
    assert not trades.schedule_groups_info()["active"]
    trades.close()


# ------------------------------------------------------------------ the configurations the edge book never reaches

@pytest.fixture(scope="module")
def auto_case():
    batch, marks = S.auto_book()
    interp = S.SCHEMES[0]
    host = S.curve_arrays(interp)
    return batch, marks, interp, host, port.price(interp.value, host.times, host.dfs, host.jac, host.hess, batch)


def test_auto_uses_the_large_groups_only(gpu_ctx, auto_case):
    """AUTO as the benchmark runs it, except that most groups found are NOT in use: the groups in use are renumbered, the
    small groups' trades go to the ungrouped table with the few trades outside every group.  Then FORCE on the same
    object: every group in use, the trades outside every group keep their bits."""
    import torch
    batch, marks, interp, host, ref = auto_case
    dc = _native.DeviceCurve(gpu_ctx, interp.value, host.times, host.dfs, host.jac, host.hess)
    assert dc.n_pillars == 32
    group_of, *_ = _native.schedule_groups_host(batch)
    used = in_use(batch, AUTO)
    trades = _native.DeviceTrades(gpu_ctx, batch)                        # no knob set
    info = trades.schedule_groups_info()
    assert info["active"] and info["used_groups"] == 30 and info["groups"] == 374 == group_of.max() + 1
    assert info["used_trades"] == int(used.sum()) and info["grouped"] == int((group_of >= 0).sum())
    got, direct, worst, vs_direct = standard_checks(gpu_ctx, dc, host, interp, batch, trades, AUTO, ref=ref)
    print(f"AUTO book: grouped vs oracle {worst:.2e}, vs the direct route {vs_direct:.2e}")
    del direct
    trades.set_schedule_groups(FORCE)
    info = trades.schedule_groups_info()
    assert info["active"] and info["used_groups"] == 374 and info["used_trades"] == info["grouped"]
    every = price(gpu_ctx, dc, trades, fill=-7.0)
    dev = got["pv"].device
    worst = device_parity(every, {k: torch.as_tensor(ref[k], device=dev) for k in ("pv", "delta", "gamma")}, batch.notional)
    print(f"AUTO book under FORCE: grouped vs oracle {worst:.2e}")
    lo, hi = marks["coupons33"]
    chained = np.zeros(batch.n_trades, dtype=bool)
    chained[lo:hi] = True
    assert rows_equal(every, got, chained)                               # the same launch under every mode
    assert rows_equal(every, got, group_of < 0)                          # ... and an ungrouped table of 6 rows, not 2 868
    trades.close()


# the book, the blocks of the fast row launch, whether plain rows stay outside the groups
FORCE_BOOKS = [("all_grouped", 5, False), ("one_block_one_outside", 1, True), ("one_block_all_grouped", 1, False),
               ("two_blocks", 2, True), ("many_groups", 256, False)]


@pytest.mark.parametrize("name,blocks,outside", FORCE_BOOKS, ids=[b[0] for b in FORCE_BOOKS])
def test_force_books_around_the_aggregate_records(gpu_ctx, name, blocks, outside):
    """The groups' share of the aggregate goes to the block records the ungrouped launch leaves free.  ``all_grouped``: no
    ungrouped launch, 5 records, 3 slices of the 40 groups, 2 records zeroed.  ``one_block_one_outside``: one record, taken by
    the ungrouped launch - the share is ADDED to it.  ``one_block_all_grouped``: one record, one slice.  ``two_blocks``: 46
    ungrouped rows want two blocks and get one, which walks them with a stride.  ``many_groups``: 4 100 groups want 257
    slices of 16, get 256, and slice 0 makes a second pass."""
    batch = {"all_grouped": S.all_grouped_book, "many_groups": S.many_groups_book}.get(name, lambda: S.tiny_books()[name])()
    interp = S.SCHEMES[0]
    host, dc = device_curve(gpu_ctx, interp)
    launches, _ = _native.route_host(interp.value, host.times, host.dfs, host.jac, host.hess, batch, 7, True, True)
    assert launches == [("fast", "rows", batch.n_trades, blocks)]
    used = in_use(batch, FORCE)
    assert bool((~used).any()) == outside
    trades = forced(gpu_ctx, batch)
    info = trades.schedule_groups_info()
    assert info["active"] and info["used_groups"] == info["groups"] and info["used_trades"] == int(used.sum())
    if name == "all_grouped":
        assert info["used_trades"] == batch.n_trades and info["groups"] == 40
    if name == "many_groups":
        assert info["groups"] == 4100 > 16 * 256 and info["used_trades"] == batch.n_trades
    if name == "two_blocks":
        assert int((~used).sum()) == 46 > 24                             # more ungrouped rows than one block's 24
    got, _, worst, vs_direct = standard_checks(gpu_ctx, dc, host, interp, batch, trades, FORCE)
    # once more on the object that has priced three times: whatever the earlier calls left in the records, the same bits
    assert same_bits(price(gpu_ctx, dc, trades, fill=0.0), got)
    trades.close()
    print(f"{name}: grouped vs oracle {worst:.2e}, vs the direct route {vs_direct:.2e}")


@pytest.mark.parametrize("which", ["edge", "all_grouped"])
def test_persistent_grid_changes_no_bit(gpu_ctx, book, which):
    """adr_trades_set_schedule_segment with a block count: the store pass walks its segments with the grid's stride."""
    batch = book[0] if which == "edge" else S.all_grouped_book()
    _, dc = device_curve(gpu_ctx, S.SCHEMES[0])
    trades = forced(gpu_ctx, batch)
    assert trades.schedule_groups_info()["blocks"] == 0
    base = price(gpu_ctx, dc, trades, fill=-7.0)
    for segment, blocks in ((16, 1), (1, 3), (33, 2), (16, batch.n_trades + 7)):      # (the last: more blocks than segments)
        trades.set_schedule_groups(FORCE, segment, blocks)
        info = trades.schedule_groups_info()
        assert info["active"] and info["segment"] == segment and info["blocks"] == blocks
        assert same_bits(price(gpu_ctx, dc, trades, fill=-7.0), base), (segment, blocks)
    trades.close()


@pytest.mark.parametrize("interp", S.SCHEMES)
@pytest.mark.parametrize("P", [8, 9])
def test_eight_and_nine_pillars(gpu_ctx, P, interp):
    """The fewest pillars the fast route takes (7 give the general kernel).  8: 64 matrix elements - lanes 0 .. 31 of the first
    band of the 16-byte path and nothing else; 9: 81 elements - the 8-byte path's first band and 17 lanes of its second."""
    batch, _ = S.edge_book(filler=50)
    px, tenors = S.short_curve_quotes(P)
    host, dc = device_curve(gpu_ctx, interp, px=px, tenors=tenors)
    assert dc.n_pillars == P
    launches, _ = _native.route_host(interp.value, host.times, host.dfs, host.jac, host.hess, batch, 7, True, True)
    assert launches[0][:2] == ("fast", "rows")
    host7 = S.curve_arrays(interp, px=px[:7], tenors=tenors[:7])
    launches7, _ = _native.route_host(interp.value, host7.times, host7.dfs, host7.jac, host7.hess, batch, 7, True, True)
    assert launches7[0][0] == "general"
    trades = forced(gpu_ctx, batch)
    _, _, worst, vs_direct = standard_checks(gpu_ctx, dc, host, interp, batch, trades, FORCE)
    trades.close()
    print(f"{P} pillars, {interp.name}: grouped vs oracle {worst:.2e}, vs the direct route {vs_direct:.2e}")


def test_one_batch_on_several_curves(gpu_ctx):
    """The basis buffers are sized for 32 pillars and laid out by each call's pillar count; a curve of more than 32 pillars
    leaves the route alone."""
    from .test_gpu_many_pillars import forty_pillar_quotes
    batch, _ = S.edge_book(filler=50)
    interp = S.SCHEMES[0]
    host32, dc32 = device_curve(gpu_ctx, interp)
    px, tenors = S.short_curve_quotes(9)
    host9, dc9 = device_curve(gpu_ctx, interp, px=px, tenors=tenors)
    trades = forced(gpu_ctx, batch)
    first = price(gpu_ctx, dc32, trades, fill=-7.0)
    standard_checks(gpu_ctx, dc9, host9, interp, batch, trades, FORCE)
    assert same_bits(price(gpu_ctx, dc32, trades, fill=-7.0), first)
    px, tenors = forty_pillar_quotes()
    host40, dc40 = device_curve(gpu_ctx, interp, px=px, tenors=tenors)
    assert dc40.n_pillars == 40 and trades.schedule_groups_info()["active"]
    wide = price(gpu_ctx, dc40, trades, fill=-7.0)
    off = _native.DeviceTrades(gpu_ctx, batch)
    off.set_schedule_groups(OFF)
    assert same_bits(wide, price(gpu_ctx, dc40, off, fill=-7.0))
    ref = port.price(interp.value, host40.times, host40.dfs, host40.jac, host40.hess, batch)
    assert_batch_parity(host_rows(wide), ref, batch.notional, tol=REL_TOL)
    off.close()
    trades.close()


def test_a_batch_without_a_group_stays_on_the_direct_route(gpu_ctx):
    batch = S.no_group_book()
    interp = S.SCHEMES[0]
    host, dc = device_curve(gpu_ctx, interp)
    trades = forced(gpu_ctx, batch)
    info = trades.schedule_groups_info()
    assert not info["active"] and info["groups"] == 0 and info["used_groups"] == 0 and info["used_trades"] == 0
    got = price(gpu_ctx, dc, trades, fill=-7.0)
    ref = port.price(interp.value, host.times, host.dfs, host.jac, host.hess, batch)
    assert_batch_parity(host_rows(got), ref, batch.notional, tol=REL_TOL)
    trades.set_schedule_groups(OFF)
    assert same_bits(price(gpu_ctx, dc, trades, fill=-7.0), got)
    trades.close()


def fma_once(x, y, z):
    """x * y + z rounded once, element by element (exact rational arithmetic where the interpreter has no math.fma)."""
    fma = getattr(math, "fma", None)
    x, y, z = np.broadcast_arrays(x, y, z)
    out = x * y + z                                                      # exact - signed zeros included - where x * y is 0
    for i in np.flatnonzero((x * y != 0.0).ravel()):
        a, b, c = float(x.flat[i]), float(y.flat[i]), float(z.flat[i])
        r = fma(a, b, c) if fma else float(Fraction(a) * Fraction(b) + Fraction(c))
        out.flat[i] = r if r != 0.0 else a * b + c                       # (an exact cancellation: +0 either way)
    return out


def test_store_pass_is_one_product_and_one_fma(gpu_ctx):
    """out = fma(cX, BX, cF * BF), element by element and bit for bit: the groups' basis trades priced as a batch of their own
    (OFF), recombined on the CPU with one correctly rounded product and one correctly rounded fused multiply-add."""
    batch = S.all_grouped_book()
    group_of, cF, cX, basis = _native.schedule_groups_host(batch)
    assert group_of.min() >= 0
    _, dc = device_curve(gpu_ctx, S.SCHEMES[0])
    pseudo = _native.DeviceTrades(gpu_ctx, TradeBatch(**{k: v for k, v in basis.items() if k != "n_trades"}))
    pseudo.set_schedule_groups(OFF)
    ladders = host_rows(price(gpu_ctx, dc, pseudo, fill=-7.0))
    trades = forced(gpu_ctx, batch)
    got = host_rows(price(gpu_ctx, dc, trades, fill=-7.0))
    for key in ("pv", "delta", "gamma"):
        b = ladders[key].reshape(basis["n_trades"], -1)
        want = fma_once(cX[:, None], b[2 * group_of + 1], cF[:, None] * b[2 * group_of])
        assert np.array_equal(want.view(np.int64), got[key].reshape(batch.n_trades, -1).view(np.int64)), key
    pseudo.close()
    trades.close()
