"""adr_bond_measures_host and adr_frn_measures_host on the edge books and curves of tests/_measures_cases.py: flow counts
around the kernels' lane and register windows, every interpolation scheme, curves that extrapolate, 2-node and
1024-node tables, dual curves of different schemes and sizes.  Against the scalar `Bond` / `FRN` methods on the same
curve objects, and against the numpy restatement for raw arrays no instrument produces.  No GPU."""
import numpy as np
import pytest

from adrates_amd import _native
from adrates_amd.utils import LibError

from . import _measures_cases as C
from .test_bonds_host import check_against_scalar
from .test_frn_host import check_rows

CURVE_CASES = [(s, c) for s in C.SCHEMES for c in C.CURVES]
PAIR_CASES = [(s,) + p for s in C.SCHEMES for p in C.frn_curve_pairs()]
ids = lambda case: "-".join(x if isinstance(x, str) else x.name for x in case)


def test_edge_books_have_their_live_counts():
    bonds, frns = C.edge_bonds(), C.edge_frns()
    book = C.bond_arrays([b for _, b, _ in bonds], C.curves(C.SCHEMES[0])["gbp"], 0.0)[3]
    assert C.live_counts(book["flow_off"]) == [n for *_, n in bonds] == [1, 15, 16, 17, 127, 128, 129, 144, 600]
    assert book["bond_acc100"][3] == 0.0 and not book["bond_tauM"][3] < 0          # settles on a coupon date
    assert np.any(book["flow_prin"][book["flow_off"][5]:book["flow_off"][6] - 1] > 0)  # amortizing
    c = C.curves(C.SCHEMES[0])
    arr = C.frn_arrays([f for _, f, _ in frns], c["gbp"], c["short_20y"], 0.0)[2]
    assert C.live_counts(arr["cpn_off"]) == [n for *_, n in frns] == [1, 17, 383, 384, 385, 600]
    assert np.isnan(arr["frn_TM"][0]) and np.all(np.isfinite(arr["frn_TM"][1:]))    # principal paid before settlement
    assert arr["cpn_fix"][arr["cpn_off"][:-1]].tolist() == [1, 1, 0, 1, 0, 0]        # seasoned: a first fixing
    assert np.isfinite(arr["frn_cap"]).sum() == 2 and np.isfinite(arr["frn_floor"]).sum() == 2


def test_edge_curves_cover_node_df_branches():
    for scheme in C.SCHEMES:
        c = C.curves(scheme)
        sizes = {k: v._times.size for k, v in c.items()}
        assert sizes["two_node"] == 2 and sizes["nodes_257"] == 257 and sizes["nodes_1024"] == C.MAX_NODES
        assert all(v._interp_type == scheme for v in c.values())
        last_flow = C.bond_arrays([C.edge_bonds()[-1][1]], c["gbp"], 0.0)[3]["flow_T"][-1]
        for k in ("short_20y", "two_node", "nodes_257"):
            assert c[k]._times[-1] < last_flow, k                                            # extrapolation
        assert c["nodes_1024"]._times[-1] > last_flow
    for d, i in C.frn_curve_pairs():
        assert C.curves(C.SCHEMES[0])[d]._times.size != C.curves(C.SCHEMES[0])[i]._times.size


@pytest.mark.parametrize("case", CURVE_CASES, ids=ids)
def test_bond_host_matches_scalar_methods(case):
    curve, prices, refs = C.bond_refs(*case)
    bonds = [b for _, b, _ in C.edge_bonds()]
    for quote, is_z in ((C.BOND_Z, True), (prices, False)):
        method, nt, nd, book = C.bond_arrays(bonds, curve, quote)
        got = _native.bond_measures_host(method, nt, nd, book, is_z)
        assert np.all(got["status"] <= 1), got["status"]
        for i, ref in enumerate(refs):
            check_against_scalar(got, i, ref)


def check_frn_rows(got, refs, dm):
    for i, ref in enumerate(refs):
        check_rows(got, i, ref)
    # the DM that reprices a clean price: its error is the price's relative error (1e-14) over the price's sensitivity
    # to the DM, the modified duration
    dur = np.array([r["mod_duration"] for r in refs])
    assert np.all(np.abs(got["dm"] - dm) <= 1e-14 / dur + 1e-15), np.abs(got["dm"] - dm) * dur


@pytest.mark.parametrize("case", PAIR_CASES, ids=ids)
def test_frn_host_matches_scalar_methods(case):
    disc, index, prices, refs = C.frn_refs(*case)
    frns = [f for _, f, _ in C.edge_frns()]
    d, i, book = C.frn_arrays(frns, disc, index, C.FRN_DM)
    assert d[0] != i[0] and d[1].size != i[1].size                                  # two schemes, two node counts
    got = _native.frn_measures_host(d, i, book, True)
    assert np.all(got["status"] == 0) and np.array_equal(got["dm"], C.FRN_DM)
    check_frn_rows(got, refs, C.FRN_DM)
    d, i, book = C.frn_arrays(frns, disc, index, prices)
    got = _native.frn_measures_host(d, i, book, False)
    assert np.all(got["status"] == 0)
    check_frn_rows(got, refs, C.FRN_DM)


def check_restated(got, ref, outputs):
    """The kernels' tolerances against an independent reference: the bond's TOL_ABS / TOL_REL, the FRN's 1e-12."""
    if outputs == _native.BOND_OUTPUTS:
        for i in range(ref["z"].size):
            check_against_scalar(got, i, {k: ref[k][i] for k in outputs})
    else:
        for i in range(ref["pv"].size):
            if ref["status"][i] == 0:
                check_rows(got, i, {k: ref[k][i] for k in outputs})


@pytest.mark.parametrize("scheme", C.SCHEMES, ids=lambda s: s.name)
def test_bonds_on_node_times_host_matches_restatement(scheme):
    t, d, book = C.bonds_on_nodes()
    ref = C.restate_bonds_z(scheme.value, t, d, book)
    got = _native.bond_measures_host(scheme.value, t, d, book, True)
    assert np.all(got["status"] == 0)
    check_restated(got, ref, _native.BOND_OUTPUTS)


@pytest.mark.parametrize("scheme", C.SCHEMES, ids=lambda s: s.name)
def test_frns_on_node_times_host_matches_restatement(scheme):
    (dt, dd), (it, idf), book = C.frns_on_nodes()
    disc, index = (scheme.value, dt, dd), (C.index_scheme(scheme).value, it, idf)
    ref = C.restate_frns_dm(disc, index, book)
    assert list(ref["status"]) == [0, 3]
    got = _native.frn_measures_host(disc, index, book, True)
    assert list(got["status"]) == [0, 3]
    assert all(np.isnan(got[k][1]) for k in _native.FRN_OUTPUTS)
    check_restated(got, ref, _native.FRN_OUTPUTS)


def test_1025_nodes_refused_by_host_twins():
    t, d = C.too_many_nodes()
    curve = C.curves(C.SCHEMES[0])["nodes_1024"]
    method, nt, nd, book = C.bond_arrays([b for _, b, _ in C.edge_bonds()], curve, C.BOND_Z)
    with pytest.raises(LibError, match=r"\(-2\)"):
        _native.bond_measures_host(method, t, d, book, True)
    _native.bond_measures_host(method, t[:-1], d[:-1], book, True)                   # 1024 nodes are accepted
    disc, index, arr = C.frn_arrays([f for _, f, _ in C.edge_frns()], curve, curve, C.FRN_DM)
    for bad in (((disc[0], t, d), index), (disc, (index[0], t, d))):
        with pytest.raises(LibError, match=r"\(-2\)"):
            _native.frn_measures_host(*bad, arr, True)
