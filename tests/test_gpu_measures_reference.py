"""adr_bond_measures and adr_frn_measures on the GPU held to the plain 60-digit reference of tests/_measures_reference.py - not to
their host twins: every output of every instrument on its counted bound, the solved outputs by their exact residual at the
root the device returned, the status by the exact sign change.  The same books, curves and solver edges as
tests/test_measures_reference_host.py (the references are built once per process and shared with it), each through one
launch of the `_dev` entry on a caller's stream into guarded buffers.  That a result does not depend on its position in a
launch is tests/test_gpu_measures_edges.py's, bit for bit, and is not repeated here.

Measured on an MI355X (the worst |error| / allowance over all cases; nothing beyond <= 1.0 is asserted; k as on the host):
  bonds  z 0.127, dirty 0.180, clean 0.170, ytm 0.523, duration 0.104, convexity 0.0834, dv01 0.0858;  residuals up to 4.35
         units of gross for z and 276 for the yield (the midpoint case of tests/_measures_reference.py; stop term 412)
  FRNs   dm 0.0883, dirty 0.096, clean 0.0456, pv 0.106, mod_duration 0.0697, dv01 0.0454;  the DM's residual up to 1.77
         units of gross
To three digits these are the host twins' figures but for the yield: the device's exp and log differ from the host's in few
enough last bits that the same elements are the worst.  The 34 tests take 22 s, most of it the host-side mpmath."""
import numpy as np
import pytest
import torch

from adrates_amd import _native

from . import _measures_cases as C
from . import _measures_reference as R
from .test_measures_edges_host import CURVE_CASES, PAIR_CASES, ids
from .test_measures_reference_host import TOTAL, bond_books, frn_books, hold, node_books

pytestmark = pytest.mark.gpu

GUARD = -1.2345e300
GUARD_STATUS = -77
TAIL = 16                           # guard words behind every output


def _launch(launch, inputs, outputs, n):
    """One `_dev` launch on a stream of the caller's: ``inputs`` (name -> array) on the device, ``out [len(outputs), n]`` and
    ``status [n]`` with TAIL guard words behind each, which must keep their pattern."""
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in inputs.items()}
    out = torch.full((len(outputs) * n + TAIL,), GUARD, dtype=torch.float64, device=dev)
    status = torch.full((n + TAIL,), GUARD_STATUS, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    launch({k: v.data_ptr() for k, v in t.items()}, out.data_ptr(), status.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert torch.all(out[len(outputs) * n:] == GUARD) and torch.all(status[n:] == GUARD_STATUS)
    o = out[:len(outputs) * n].cpu().numpy().reshape(len(outputs), n)
    got = {k: o[i] for i, k in enumerate(outputs)}
    got["status"] = status[:n].cpu().numpy()
    return got


def bond_dev(ctx, method, nt, nd, book, is_z):
    n = book["bond_quote"].size
    return _launch(lambda p, out, status, s: _native.bond_measures_dev(ctx, method, nt.size, n, p, is_z, out, status, s),
                   dict(book, node_t=nt, node_df=nd), _native.BOND_OUTPUTS, n)


def frn_dev(ctx, disc, index, book, is_dm):
    off, cpn, frn = _native.frn_pack(book)
    n, m = frn.shape[1], cpn.shape[1]
    return _launch(lambda p, out, status, s: _native.frn_measures_dev(ctx, disc[0], disc[1].size, index[0], index[1].size, n, m,
                                                                      p, is_dm, out, status, s),
                   {"disc_t": disc[1], "disc_df": disc[2], "index_t": index[1], "index_df": index[2], "cpn_off": off,
                    "cpn": cpn, "frn": frn}, _native.FRN_OUTPUTS, n)


@pytest.mark.parametrize("case", CURVE_CASES, ids=ids)
def test_bond_device_within_the_bound(gpu_ctx, case):
    for what, args, is_z, status in bond_books(*case):
        hold(R.check_bonds(*args, is_z, bond_dev(gpu_ctx, *args, is_z)), f"device, {ids(case)}, {what}", "bond device", status)


@pytest.mark.parametrize("case", PAIR_CASES, ids=ids)
def test_frn_device_within_the_bound(gpu_ctx, case):
    for what, args, is_dm, status in frn_books(*case):
        hold(R.check_frns(*args, is_dm, frn_dev(gpu_ctx, *args, is_dm)), f"device, {ids(case)}, {what}", "frn device", status)


@pytest.mark.parametrize("scheme", C.SCHEMES, ids=lambda s: s.name)
def test_device_on_node_times_within_the_bound(gpu_ctx, scheme):
    bond, frn = node_books(scheme)
    hold(R.check_bonds(*bond, True, bond_dev(gpu_ctx, *bond, True)), f"device, {scheme.name}, bonds on nodes", "bond device",
         [0, 0])
    hold(R.check_frns(*frn, True, frn_dev(gpu_ctx, *frn, True)), f"device, {scheme.name}, FRNs on nodes", "frn device", [0, 3])


def test_worst_ratios_of_the_device():
    """Prints what the tests above found, all cases merged (run the module with -s to read it)."""
    for what in ("bond device", "frn device"):
        if what in TOTAL:
            print(TOTAL[what].line(what + ", all cases"))
            assert TOTAL[what].worst() <= 1.0
