"""adr_bond_measures and adr_frn_measures on the GPU at the edges of their launch geometry (tests/_measures_cases.py):
flows past the register windows, re-read from global memory; every scheme; curves that extrapolate; node tables of 2,
257 and 1024 entries (one to four LDS staging passes); dual curves of different schemes and sizes; partially filled
last blocks.  Against the scalar `Bond` / `FRN` methods and the numpy restatement, against the host twins, and
against themselves at every position in a launch."""
import numpy as np
import pytest
import torch

from adrates_amd import _native
from adrates_amd.utils import LibError

from . import _measures_cases as C
from .test_gpu_bonds import same_measures as same_bond_measures
from .test_gpu_frns import same_measures as same_frn_measures
from .test_measures_edges_host import CURVE_CASES, PAIR_CASES, check_against_scalar, check_frn_rows, check_restated, ids

pytestmark = pytest.mark.gpu


def bond_run(ctx, method, nt, nd, book, is_z):
    got = _native.bond_measures(ctx, method, nt, nd, book, is_z)
    host = _native.bond_measures_host(method, nt, nd, book, is_z)
    assert np.array_equal(got["status"], host["status"])
    same_bond_measures(got, host, book["bond_face"])
    return got


def frn_run(ctx, disc, index, book, is_dm):
    got = _native.frn_measures(ctx, disc, index, book, is_dm)
    host = _native.frn_measures_host(disc, index, book, is_dm)
    assert np.array_equal(got["status"], host["status"])
    same_frn_measures(got, host)
    return got


@pytest.mark.parametrize("case", CURVE_CASES, ids=ids)
def test_bond_device_matches_scalar_methods_and_host(gpu_ctx, case):
    curve, prices, refs = C.bond_refs(*case)
    bonds = [b for _, b, _ in C.edge_bonds()]
    for quote, is_z in ((C.BOND_Z, True), (prices, False)):
        got = bond_run(gpu_ctx, *C.bond_arrays(bonds, curve, quote), is_z)
        assert np.all(got["status"] <= 1)
        for i, ref in enumerate(refs):
            check_against_scalar(got, i, ref)


@pytest.mark.parametrize("case", PAIR_CASES, ids=ids)
def test_frn_device_matches_scalar_methods_and_host(gpu_ctx, case):
    disc, index, prices, refs = C.frn_refs(*case)
    frns = [f for _, f, _ in C.edge_frns()]
    got = frn_run(gpu_ctx, *C.frn_arrays(frns, disc, index, C.FRN_DM), True)
    assert np.all(got["status"] == 0) and np.array_equal(got["dm"], C.FRN_DM)
    check_frn_rows(got, refs, C.FRN_DM)
    got = frn_run(gpu_ctx, *C.frn_arrays(frns, disc, index, prices), False)
    assert np.all(got["status"] == 0)
    check_frn_rows(got, refs, C.FRN_DM)


@pytest.mark.parametrize("scheme", C.SCHEMES, ids=lambda s: s.name)
def test_raw_node_time_cases_match_restatement(gpu_ctx, scheme):
    t, d, book = C.bonds_on_nodes()
    got = bond_run(gpu_ctx, scheme.value, t, d, book, True)
    assert np.all(got["status"] == 0)
    check_restated(got, C.restate_bonds_z(scheme.value, t, d, book), _native.BOND_OUTPUTS)
    (dt, dd), (it, idf), fbook = C.frns_on_nodes()
    disc, index = (scheme.value, dt, dd), (C.index_scheme(scheme).value, it, idf)
    got = frn_run(gpu_ctx, disc, index, fbook, True)
    assert list(got["status"]) == [0, 3]              # coupon #400's start lies before the index curve's first node
    check_restated(got, C.restate_frns_dm(disc, index, fbook), _native.FRN_OUTPUTS)


def test_1025_nodes_refused_on_device(gpu_ctx):
    t, d = C.too_many_nodes()
    curve = C.curves(C.SCHEMES[0])["nodes_1024"]
    method, nt, nd, book = C.bond_arrays([b for _, b, _ in C.edge_bonds()], curve, C.BOND_Z)
    with pytest.raises(LibError, match=r"\(-2\)"):
        _native.bond_measures(gpu_ctx, method, t, d, book, True)
    disc, index, arr = C.frn_arrays([f for _, f, _ in C.edge_frns()], curve, curve, C.FRN_DM)
    for bad in (((disc[0], t, d), index), (disc, (index[0], t, d))):
        with pytest.raises(LibError, match=r"\(-2\)"):
            _native.frn_measures(gpu_ctx, *bad, arr, True)
    # the non-blocking entry points refuse the table before they read any pointer; the other arrays are null, so an
    # entry point that let the table through would refuse them (-1) rather than launch
    with pytest.raises(LibError, match=r"\(-2\)"):
        _native.bond_measures_dev(gpu_ctx, method, C.MAX_NODES + 1, 1, {k: 0 for k in ("node_t", "node_df", "flow_off")
                                  + _native.BOND_FLOW_FIELDS + _native.BOND_FIELDS}, True, 0, 0)
    two = _device({"t": t[:2], "d": d[:2]})
    for dn, i_n in ((C.MAX_NODES + 1, 2), (2, C.MAX_NODES + 1)):
        ptrs = {k: 0 for k in ("disc_t", "disc_df", "index_t", "index_df", "cpn_off", "cpn", "frn")}
        side = "disc" if dn == 2 else "index"                      # the accepted curve gets real nodes
        ptrs[side + "_t"], ptrs[side + "_df"] = two["t"].data_ptr(), two["d"].data_ptr()
        with pytest.raises(LibError, match=r"\(-2\)"):
            _native.frn_measures_dev(gpu_ctx, method, dn, method, i_n, 1, 1, ptrs, True, 0, 0)


# ------------------------------------------------------------------------------------------------ non-blocking form
def _device(host):
    dev = torch.device("cuda", 0)
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in host.items()}


def _finish(out, status, stream, ref, outputs):
    stream.synchronize()
    o, st = out.cpu().numpy(), status.cpu().numpy()
    assert np.array_equal(st, ref["status"])
    for i, k in enumerate(outputs):
        assert np.array_equal(o[i], ref[k], equal_nan=True), k


@pytest.mark.parametrize("is_z", [True, False], ids=["z", "clean"])
def test_bond_measures_dev_equals_blocking_on_1024_nodes(gpu_ctx, is_z):
    curve, prices, _ = C.bond_refs(C.SCHEMES[1], "nodes_1024")
    method, nt, nd, book = C.bond_arrays([b for _, b, _ in C.edge_bonds()], curve, C.BOND_Z if is_z else prices)
    ref = _native.bond_measures(gpu_ctx, method, nt, nd, book, is_z)
    t = _device(dict(book, node_t=nt, node_df=nd))
    n = book["bond_quote"].size
    out = torch.empty((len(_native.BOND_OUTPUTS), n), dtype=torch.float64, device="cuda:0")
    status = torch.empty(n, dtype=torch.int32, device="cuda:0")
    s = torch.cuda.Stream(torch.device("cuda", 0))
    torch.cuda.synchronize()
    _native.bond_measures_dev(gpu_ctx, method, nt.size, n, {k: v.data_ptr() for k, v in t.items()}, is_z,
                              out.data_ptr(), status.data_ptr(), s.cuda_stream)
    _finish(out, status, s, ref, _native.BOND_OUTPUTS)


@pytest.mark.parametrize("pair", [("nodes_1024", "nodes_257"), ("short_20y", "nodes_1024")], ids=ids)
def test_frn_measures_dev_equals_blocking_on_dual_curves(gpu_ctx, pair):
    disc, index, prices, _ = C.frn_refs(C.SCHEMES[2], *pair)
    d, i, book = C.frn_arrays([f for _, f, _ in C.edge_frns()], disc, index, prices)
    ref = _native.frn_measures(gpu_ctx, d, i, book, False)
    off, cpn, frn = _native.frn_pack(book)
    t = _device({"disc_t": d[1], "disc_df": d[2], "index_t": i[1], "index_df": i[2], "cpn_off": off, "cpn": cpn,
                 "frn": frn})
    n = frn.shape[1]
    out = torch.empty((len(_native.FRN_OUTPUTS), n), dtype=torch.float64, device="cuda:0")
    status = torch.empty(n, dtype=torch.int32, device="cuda:0")
    s = torch.cuda.Stream(torch.device("cuda", 0))
    torch.cuda.synchronize()
    _native.frn_measures_dev(gpu_ctx, d[0], d[1].size, i[0], i[1].size, n, cpn.shape[1],
                             {k: v.data_ptr() for k, v in t.items()}, False, out.data_ptr(), status.data_ptr(),
                             s.cuda_stream)
    _finish(out, status, s, ref, _native.FRN_OUTPUTS)


# ------------------------------------------------------------------------------------------------ launch shapes
def _launch_shapes(edge, filler, keys, run):
    """Every edge case at every lane-group slot of a block and on both sides of a block boundary (behind 0 .. 15
    fillers), alone (n = 1) and in launches of n = 15, 17 and 4097 that cycle through the cases (4097: 256 full blocks
    and one instrument in the last): each gives the bits of the unpadded launch."""
    k = edge[keys[0]].size - 1
    base = run(edge)
    names = _native.BOND_OUTPUTS if keys == C.BOND_KEYS else _native.FRN_OUTPUTS

    def same(got, rows):
        assert np.array_equal(got["status"], base["status"][rows])
        for o in names:
            assert np.array_equal(got[o], base[o][rows], equal_nan=True), o

    for pad in range(16):
        got = run(C.concat(C.take(filler, np.arange(pad), keys), edge, keys))
        same({o: v[pad:] for o, v in got.items()}, np.arange(k))
    for i in range(k):
        same(run(C.take(edge, [i], keys)), [i])
    for n in (15, 17, 4097):
        rows = np.arange(n) % k
        same(run(C.take(edge, rows, keys)), rows)


@pytest.mark.parametrize("is_z", [True, False], ids=["z", "clean"])
def test_bond_results_do_not_depend_on_launch_shape(gpu_ctx, is_z):
    curve, prices, _ = C.bond_refs(C.SCHEMES[0], "nodes_257")
    method, nt, nd, edge = C.bond_arrays([b for _, b, _ in C.edge_bonds()], curve, C.BOND_Z if is_z else prices)
    filler = C.bond_arrays(C.filler_bonds(), curve, 0.01 if is_z else 99.0)[3]
    _launch_shapes(edge, filler, C.BOND_KEYS, lambda book: _native.bond_measures(gpu_ctx, method, nt, nd, book, is_z))


@pytest.mark.parametrize("is_dm", [True, False], ids=["dm", "clean"])
def test_frn_results_do_not_depend_on_launch_shape(gpu_ctx, is_dm):
    disc, index, prices, _ = C.frn_refs(C.SCHEMES[1], "gbp", "short_20y")
    d, i, edge = C.frn_arrays([f for _, f, _ in C.edge_frns()], disc, index, C.FRN_DM if is_dm else prices)
    filler = C.frn_arrays(C.filler_frns(), disc, index, 0.01 if is_dm else 99.0)[2]
    _launch_shapes(edge, filler, C.FRN_KEYS, lambda book: _native.frn_measures(gpu_ctx, d, i, book, is_dm))
