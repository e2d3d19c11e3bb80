"""The schedule-group route of adr_price_dev on a FORCE batch built around its edges: group sizes
around the store pass's segment, 1 to 32 coupons and a chained 33-coupon trade, a semi-annual fixed leg, spreads, a
zero-coupon member, an outlier 1 % off its group's shape, pay and receive - against oracle/port.c, against the direct route,
and through the route's bit contracts."""
import numpy as np
import pytest

from adrates_amd import _native
from oracle import port

from . import _fixtures as F
from . import _schedule_group_cases as S
from ._parity import REL_TOL, assert_batch_parity

pytestmark = pytest.mark.gpu
FORCE, OFF, AUTO = _native.SCHEDULE_GROUPS_FORCE, _native.SCHEDULE_GROUPS_OFF, _native.SCHEDULE_GROUPS_AUTO


@pytest.fixture(scope="module")
def book():
    return S.edge_book()


def device_curve(ctx, interp, **kw):
    host = S.curve_arrays(interp, **kw)
    return host, _native.DeviceCurve(ctx, interp.value, host.times, host.dfs, host.jac, host.hess)


def price(ctx, dc, trades, mask=7, agg=True, stream=0, fill=None):
    """adr_price_dev into fresh device buffers; ``fill``: what the buffers hold before the call."""
    import torch
    dev = torch.device("cuda", 0)
    n, P = trades.n_trades, dc.n_pillars
    new = (lambda *shape: torch.full(shape, fill, dtype=torch.float64, device=dev)) if fill is not None else \
          (lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev))
    out = dict(pv=new(n), delta=new(n, P), gamma=new(n, P, P), agg=new(1 + P + P * P) if agg else None)
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
    # GAMMA alone and DELTA + GAMMA: pv / delta are left as they were, what is written equals the full request's bits
    for mask, untouched, written in ((4, ("pv", "delta"), ("gamma", "agg")), (6, ("pv",), ("delta", "gamma"))):
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
