"""csrc/yoy_risk.hip on the GPU at its edges (the case table of tests/_yoy_cases.py):

  - the device against the 60-digit third evaluation (oracle/mp_oracle.py::MpYoY) and `simple_interpolate` directly,
    every entry on its own swap's notional, and against the host twin per array and per swap row;
  - every kernel instantiation's pillar counts x legs across the staging passes x books across the chunk ends, each
    swap bit for bit the swap priced alone, agg the documented sum of the rows;
  - request masks through adr_yoy_risk_dev into guarded buffers, malformed offsets, n = 0, a caller's stream.

Observed on an MI355X: against MpYoY 4.5e-12 (the cancelling gamma of year-on-year coupons
beyond the last LINEAR_ZERO pillar, see tests/test_yoy_third_evaluation.py) and 7.5e-14 elsewhere, against
`simple_interpolate` 1.1e-16, against the host twin per swap row 2.3e-14."""
import itertools

import numpy as np
import pytest
import torch

from adrates_amd import _native

from . import _yoy_cases as YC
from ._parity import REL_TOL
from .test_gpu_inflation import _close_bits

pytestmark = pytest.mark.gpu
GUARD = -1.2345e300
TAIL = 16                                                       # one reduction block's width behind every buffer
V, D, G = _native.REQ_VALUE, _native.REQ_DELTA, _native.REQ_GAMMA
PER, AGG = _native.YOY_PER_SWAP, _native.YOY_AGG
ALL3 = V | D | G
ROWS = ("amount", "pv", "delta", "gamma")


# ------------------------------------------------------------------------------------- against the third evaluation
@pytest.mark.parametrize("case", YC.all_cases(), ids=repr)
def test_device_against_third_evaluation_and_host_twin(gpu_ctx, case):
    dev = _native.yoy_risk(gpu_ctx, case.disc, case.infl, case.book, aggregate=True)
    host = _native.yoy_risk_host(case.disc, case.infl, case.book, aggregate=True)
    e, name, key = YC.worst(YC.case_errors(case, dev))
    e_row = YC.row_errors(case, dev, host)
    print(f"{case}: device against MpYoY {e:.2e} ({name}, {key}), against the host twin per row {e_row:.2e}")
    assert e <= REL_TOL, (name, key, e)
    for k in ROWS + ("agg_delta", "agg_gamma"):
        _close_bits(dev[k], host[k])
    _close_bits([dev["agg_pv"]], [host["agg_pv"]])
    assert e_row <= REL_TOL
    if case.name.startswith("lookup"):
        ref = YC.lookup_reference(case)
        e_df = float(np.max(np.abs(dev["pv"] - ref)))
        print(f"{case}: si::df on the device against simple_interpolate {e_df:.2e}")
        assert e_df <= REL_TOL and np.array_equal(dev["pv"] == 0.0, ref == 0.0) and np.all(dev["amount"] == 1.0)


# ------------------------------------------------------------------------------------------------- launch geometry
@pytest.mark.parametrize("P", YC.PILLAR_EDGES)
def test_every_instantiation_edge_bit_for_bit(gpu_ctx, P):
    for j, n in enumerate(YC.BOOK_EDGES):
        case = YC.geometry_case(P, n, YC.INFL_SCHEMES[(P + j) % 2], YC.DISC_SCHEMES[j % 3], shift=j)
        lens = set(np.diff(case.book["cpn_off"]).tolist())
        assert n < 33 or lens == set(YC.LEG_EDGES)
        got = _native.yoy_risk(gpu_ctx, case.disc, case.infl, case.book, aggregate=True)
        host = _native.yoy_risk_host(case.disc, case.infl, case.book, aggregate=True)
        assert got["gamma"].shape == (n, P, P)
        for k in ROWS + ("agg_delta", "agg_gamma"):
            _close_bits(got[k], host[k])
        assert YC.row_errors(case, got, host) <= REL_TOL
        off = case.book["cpn_off"]
        for i in range(n):
            alone = _native.yoy_risk(gpu_ctx, case.disc, case.infl, YC.one_swap(case.book, i))
            assert alone["pv"][0] == got["pv"][i], (n, i)
            assert np.array_equal(alone["delta"][0], got["delta"][i]) and np.array_equal(alone["gamma"][0], got["gamma"][i]), (n, i)
            assert np.array_equal(alone["amount"], got["amount"][off[i]:off[i + 1]]), (n, i)
        rows = np.concatenate([got["pv"][:, None], got["delta"], got["gamma"].reshape(n, P * P)], axis=1)
        agg = np.concatenate([[got["agg_pv"]], got["agg_delta"], got["agg_gamma"].ravel()])
        np.testing.assert_array_equal(agg, YC.fixed_order_sum(rows))


# --------------------------------------------------------------------------------------- the device-array entry
def _run_dev(ctx, case, mask, off=None, pad=0, stream=0, n=None):
    """adr_yoy_risk_dev with every output pointer given, into buffers filled with GUARD that carry TAIL words more than
    the entry may write; returns them whole, as numpy.  ``off``: other offsets than the book's; ``pad``: finite coupon
    words behind cpn.  ``stream``: torch's current stream, as the caller's.  It is kept busy while the GUARD fills and the
    entry are enqueued and is the only thing waited for, so work that the entry put on any other stream would run before
    the fills and be overwritten by them."""
    dev = torch.device("cuda", 0)
    book_off, cpn = _native.yoy_pack(case.book)
    off = book_off if off is None else np.asarray(off, dtype=np.int64)
    n, m, P = (off.size - 1 if n is None else n), cpn.shape[1], case.P
    cu = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a)).to(dtype=dt, device=dev)
    (dm, times, dfs), (im, T, b) = case.disc, case.infl
    ins = dict(times=cu(times), dfs=cu(dfs), T=cu(T), b=cu(b), cpn_off=cu(off, torch.int64),
               cpn=cu(np.concatenate((cpn.ravel(), np.ones(pad)))))
    sizes = dict(amount=m, pv=n, delta=n * P, gamma=n * P * P, agg=1 + P + P * P, work=_native.yoy_risk_work(n, P))
    if stream:                                                  # hold the caller's stream back: the fills wait behind this
        torch.cuda.synchronize()
        torch.cuda._sleep(200_000_000)
    outs = {k: torch.full((v + TAIL,), GUARD, dtype=torch.float64, device=dev) for k, v in sizes.items()}
    if not stream:
        torch.cuda.synchronize()
    _native.yoy_risk_dev(ctx, dm, np.asarray(times).size, im, P, n, m, {k: v.data_ptr() for k, v in ins.items()}, mask,
                         {k: v.data_ptr() for k, v in outs.items()}, stream)
    if stream:
        torch.cuda.current_stream().synchronize()               # the caller's stream alone, no device-wide wait
    else:
        ctx.sync()
        torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in outs.items()}
    for k, v in sizes.items():
        assert np.all(out[k][v:] == GUARD), f"tail words behind {k} were written"
    return out, sizes


def _untouched(a):
    return bool(np.all(a == GUARD))


MEASURES = {"V": V, "D": D, "G": G, "V|D": V | D, "D|G": D | G, "V|D|G": ALL3}
MODES = {"per swap": PER, "agg": AGG, "both": PER | AGG, "neither": 0}


@pytest.mark.parametrize("P", [1, 9])                           # R = 3 and 91: not multiples of the reduction's 16
def test_request_masks_into_guarded_buffers(gpu_ctx, P):
    case = YC.geometry_case(P, 17, YC.LZ, YC.FF, shift=2)
    full, size = _run_dev(gpu_ctx, case, ALL3 | PER | AGG)
    n, R = 17, 1 + P + P * P
    assert R % 16 and not any(_untouched(full[k][:size[k]]) for k in ROWS + ("agg",))
    blocking = _native.yoy_risk(gpu_ctx, case.disc, case.infl, case.book, aggregate=True)
    for k in ROWS:
        assert np.array_equal(full[k][:size[k]], blocking[k].ravel()), k
    rows = np.concatenate([blocking["pv"][:, None], blocking["delta"], blocking["gamma"].reshape(n, P * P)], axis=1)
    np.testing.assert_array_equal(full["agg"][:R], YC.fixed_order_sum(rows))
    slots = {V: slice(0, 1), D: slice(1, 1 + P), G: slice(1 + P, R)}
    for (mname, meas), (rname, mode) in itertools.product(MEASURES.items(), MODES.items()):
        got, _ = _run_dev(gpu_ctx, case, meas | mode)
        tag = f"{mname}, {rname}"
        assert np.array_equal(got["amount"], full["amount"]), tag            # written whenever given
        for key, bit in (("pv", V), ("delta", D), ("gamma", G)):
            if (mode & PER) and (meas & bit):
                assert np.array_equal(got[key], full[key]), (tag, key)
            else:
                assert _untouched(got[key]), (tag, key)
        if mode & AGG:
            host = _native.yoy_risk_host(case.disc, case.infl, case.book, req_mask=meas, per_swap=bool(mode & PER), aggregate=True)
            twin = np.concatenate([[host["agg_pv"]], host["agg_delta"], host["agg_gamma"].ravel()])
            for bit, sl in slots.items():
                if meas & bit:
                    assert np.array_equal(got["agg"][sl], full["agg"][sl]), (tag, bit)
                else:                                           # what the host twin puts there: 0.0 (include/adrates.h)
                    assert np.array_equal(got["agg"][sl], twin[sl]) and not got["agg"][sl].any(), (tag, bit)
        else:
            assert _untouched(got["agg"]) and _untouched(got["work"]), tag


def test_empty_book_with_agg_writes_agg_alone(gpu_ctx):
    case = YC.Case("no swaps", (YC.LZ,) + YC.disc_grid(), (YC.FF,) + YC.pillars(9), [])
    got, size = _run_dev(gpu_ctx, case, ALL3 | PER | AGG, off=np.zeros(1, dtype=np.int64), n=0)
    assert size["agg"] == 91 and not got["agg"][:91].any() and _untouched(got["agg"][91:])
    assert all(_untouched(got[k]) for k in ROWS + ("work",))
    got, _ = _run_dev(gpu_ctx, case, ALL3 | PER, off=np.zeros(1, dtype=np.int64), n=0)
    assert all(_untouched(got[k]) for k in ROWS + ("agg", "work"))


def test_malformed_offsets_on_the_device_entry(gpu_ctx):
    """A decreasing cpn_off pair and an end beyond m between good swaps.  The guard reads nothing for such a swap; the
    coupon tensor is padded and the outputs carry tail words so that every index a kernel without the guard would
    touch (coupons up to m + 6 in each of the five fields) still lies in memory this test allocated."""
    P, m, over = 9, 30, 7
    cpns = YC.leg(m, 0.31, 1e6 / 12.0, 0.001)
    case = YC.Case("malformed", (YC.LF,) + YC.disc_grid(), (YC.LZ,) + YC.pillars(P), [("all coupons", 1e6, cpns)])
    off = [0, 10, 5, 15, m + over, 20, 30]                      # good, decreasing, good, beyond m, decreasing, good
    good, bad = {0: (0, 10), 2: (5, 15), 5: (20, 30)}, (1, 3, 4)
    assert over < TAIL
    got, size = _run_dev(gpu_ctx, case, ALL3 | PER | AGG, off=off, pad=5 * over + 64)
    n = len(off) - 1
    pv, delta, gamma = got["pv"][:n], got["delta"][:n * P].reshape(n, P), got["gamma"][:n * P * P].reshape(n, P * P)
    for i in bad:
        assert np.isnan(pv[i]) and not delta[i].any() and not gamma[i].any(), i
    for i, (lo, hi) in good.items():
        alone = _native.yoy_risk(gpu_ctx, case.disc, case.infl, YC.raw_book([cpns[lo:hi]]))
        assert alone["pv"][0] == pv[i] and np.array_equal(alone["delta"][0], delta[i]), i
        assert np.array_equal(alone["gamma"][0].ravel(), gamma[i]) and np.array_equal(alone["amount"], got["amount"][lo:hi]), i
    assert _untouched(got["amount"][15:20])                     # coupons of no well-formed swap: not described
    agg = got["agg"][:size["agg"]]
    assert np.isnan(agg[0])
    rows = np.concatenate([delta, gamma], axis=1)
    np.testing.assert_array_equal(agg[1:], YC.fixed_order_sum(rows))


def test_device_entry_on_the_callers_stream(gpu_ctx):
    """Bit for bit the blocking entry, with the outputs read after the caller's stream alone: an entry that enqueued on
    the context's stream instead would find its outputs refilled with the guard pattern (see `_run_dev`)."""
    case = YC.geometry_case(17, 33, YC.FF, YC.LZ, shift=1)
    ref = _native.yoy_risk(gpu_ctx, case.disc, case.infl, case.book, aggregate=True)
    side = torch.cuda.Stream(device=0)
    with torch.cuda.stream(side):
        got, size = _run_dev(gpu_ctx, case, ALL3 | PER | AGG, stream=side.cuda_stream)
    P = case.P
    for k in ROWS:
        assert np.array_equal(got[k][:size[k]], ref[k].ravel()), k
    agg = got["agg"][:size["agg"]]
    assert agg[0] == ref["agg_pv"] and np.array_equal(agg[1:1 + P], ref["agg_delta"])
    assert np.array_equal(agg[1 + P:], ref["agg_gamma"].ravel())
