"""bench.py --dump-outputs: the files hold what the timed path computed in its last step - the rows of the seeded trade
sample and the portfolio ladder equal the library's own blocking call on the same seeded portfolio."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from adrates_amd import _native
from adrates_amd.trades import synthetic

from . import _fixtures as F
from .test_gpu_parity_batch import _device_curve

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_hold_the_last_timed_step(gpu_ctx, tmp_path):
    n, steps = 20000, 4
    out_dir = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--trades", str(n), "--steps",
                          str(steps), "--warmup", "1", "--min-warmup-ms", "0", "--cpu-baseline-seconds", "0",
                          "--dump-outputs", str(out_dir)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-2500:])
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["ms_per_step"] > 0.0 and d["parity_spot_check"]["ok"]

    files = sorted(os.listdir(out_dir))
    assert files == ["agg.npy", "delta.npy", "gamma.npy", "pv.npy", "trade_index.npy"]
    assert sum(os.path.getsize(out_dir / f) for f in files) <= 64e6
    got = {f[:-4]: np.load(out_dir / f) for f in files}
    assert all(a.dtype == np.float64 for a in got.values())
    idx = got["trade_index"].astype(np.int64)
    assert len(idx) == 4096 and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < n

    curve = F.gbp_model(F.README_VALUE_DT).curves.GBP_OIS_SONIA
    _, dc = _device_curve(gpu_ctx, curve)
    batch, _ = synthetic.shard_of_portfolio(F.README_VALUE_DT, n, 0, 1)
    want = _native.price(gpu_ctx, dc, _native.DeviceTrades(gpu_ctx, batch), aggregate=True)
    P = dc.n_pillars
    assert got["delta"].shape == (4096, P) and got["gamma"].shape == (4096, P, P)
    for key in ("pv", "delta", "gamma"):
        w = want[key][idx]
        assert np.max(np.abs(got[key] - w)) <= 1e-12 * np.max(np.abs(w)), key
    agg = np.concatenate([[want["agg_pv"]], want["agg_delta"], want["agg_gamma"].ravel()])
    assert got["agg"].shape == agg.shape
    assert np.max(np.abs(got["agg"] - agg)) <= 1e-12 * np.max(np.abs(agg))
