"""Concurrent adr_price_dev calls on ONE batch (include/adrates.h, the stream rules of adr_price_dev): calls without agg_dev
on a batch without payment-lag or weighted coupons may run on different streams at once.  The batch caches the launch plan
of its last (curve class, request); two host threads that alternate requests on it rebuild that plan while the other walks
its own (csrc/capi.hip, adr_trades::plan_for).  Every result must equal the serial one bit for bit."""
import threading

import pytest

from adrates_amd import _native
from adrates_amd.trades import synthetic
from adrates_amd.utils import FrequencyTypes

from . import _fixtures as F
from .test_gpu_parity_batch import _device_curve

pytestmark = pytest.mark.gpu

CALLS = 36          # per thread, alternating masks 3 and 7


def test_two_threads_alternating_requests_on_one_batch(gpu_ctx):
    import torch
    vd = F.README_VALUE_DT
    curve = F.gbp_model(vd).curves.GBP_OIS_SONIA
    host, dc = _device_curve(gpu_ctx, curve)
    batch = synthetic.synthesize(vd, 3000, kind="offgrid", seed=91, freq=FrequencyTypes.QUARTERLY)   # 1-32 and 33-120 coupons
    # plain and long trades, no payment lag: the one-row and the chained fast tables under GAMMA, the lite table without it
    launches, _ = _native.route_host(curve._interp_type.value, host.times, host.dfs, host.jac, host.hess, batch, 7)
    assert sorted(f for f, *_ in launches) == ["fast", "fast_chained"], launches
    assert [f for f, *_ in _native.route_host(curve._interp_type.value, host.times, host.dfs, host.jac, host.hess, batch, 3)[0]] == ["lite"]
    dt = _native.DeviceTrades(gpu_ctx, batch)
    dev, n, P = torch.device("cuda", 0), batch.n_trades, dc.n_pillars

    def buffers():
        return (torch.empty(n, dtype=torch.float64, device=dev), torch.empty((n, P), dtype=torch.float64, device=dev),
                torch.empty((n, P, P), dtype=torch.float64, device=dev))

    def call(mask, bufs, stream):
        pv, de, ga = bufs
        _native.price_dev(gpu_ctx, dc, dt, mask, pv.data_ptr(), de.data_ptr(), ga.data_ptr() if mask & 4 else 0, 0, stream)

    # the serial results, one call after the other on one stream
    ref = {}
    for mask in (3, 7):
        ref[mask] = buffers()
        call(mask, ref[mask], 0)
        gpu_ctx.sync()
    assert torch.isfinite(ref[7][2]).all() and bool((ref[7][2] != 0).any())

    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    start = threading.Barrier(2)
    bad, errors = [], []

    def worker(k):
        try:
            st, bufs = streams[k], buffers()
            start.wait()
            for i in range(CALLS):
                mask = (3, 7)[(i + k) % 2]            # the two threads ask for different requests at the same time
                call(mask, bufs, st.cuda_stream)
                st.synchronize()
                got = bufs if mask == 7 else bufs[:2]
                if not all(torch.equal(a, b) for a, b in zip(got, ref[mask])):
                    bad.append((k, i, mask))
        except Exception as e:          # (reported below: an exception in a thread would not fail the test)
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert not bad, bad
    dt.close()
    dc.close()
