"""Floating-rate notes on the GPU: the engine's curve Greeks against the torch-autodiff restatement of the reference's
FRN engine (tests/_frn_oracle.py), dual-curve values, portfolios, and the adr_frn_measures kernel against its host
twin."""
import numpy as np
import pytest
import torch

from adrates_amd import _native
from adrates_amd.market.portfolio.portfolio import Portfolio
from adrates_amd.market.position.frn_book import FRNBook, tile_frn_measures
from adrates_amd.market.position.position import Position
from adrates_amd.trades.credit import FRN, Bond
from adrates_amd.trades.market_data import random_frn_book
from adrates_amd.utils import (BusDayAdjustTypes, CurrencyTypes, CurveTypes, Date, DayCountTypes, FrequencyTypes,
                               InterpTypes, LibError, RequestTypes, SwapTypes)

from . import _fixtures as F
from ._frn_oracle import frn_analytics

pytestmark = pytest.mark.gpu
GBP, USD = CurrencyTypes.GBP, CurrencyTypes.USD
VD = F.README_VALUE_DT
SCHEMES = (InterpTypes.FLAT_FWD_RATES, InterpTypes.LINEAR_FWD_RATES, InterpTypes.LINEAR_ZERO_RATES)
ALL = [RequestTypes.VALUE, RequestTypes.DELTA, RequestTypes.GAMMA, RequestTypes.CASHFLOWS]
Q = FrequencyTypes.QUARTERLY


def _frns(ccy=GBP, index=CurveTypes.GBP_OIS_SONIA, vd=VD):
    s = Date(15, 1, 2024) if vd == VD else Date(15, 9, 2024)
    mk = lambda issue, tenor, freq, dc, **kw: FRN(issue, tenor, kw.pop("margin", 0.005), freq, dc, ccy, index, **kw)
    return {
        "5y_quarterly_act360": mk(vd, "5Y", Q, DayCountTypes.ACT_360),
        "semi_annual": mk(vd, "3Y", FrequencyTypes.SEMI_ANNUAL, DayCountTypes.ACT_365F, margin=0.0025),
        "seasoned_fixing": mk(s, "5Y", Q, DayCountTypes.ACT_360, first_fixing_rate=0.05),
        "seasoned_no_fixing": mk(s, "5Y", Q, DayCountTypes.ACT_360),
        "lag2": mk(vd, "4Y", Q, DayCountTypes.ACT_365F, payment_lag=2, face_value=1e6),
        "new_with_fixing": mk(vd, "2Y", Q, DayCountTypes.ACT_365F, first_fixing_rate=0.045),
        "capped": mk(vd, "5Y", Q, DayCountTypes.ACT_360, cap_rate=0.02),
        "30y_quarterly": mk(vd, "30Y", Q, DayCountTypes.ACT_360, face_value=1e6),
    }


def _usd_curve_args(interp):
    return dict(name="USD_OIS_SOFR", px_list=list(F.USD_PX), tenor_list=list(F.TENORS), spot_days=0,
                swap_type=SwapTypes.PAY, fixed_dcc_type=DayCountTypes.ACT_360, fixed_freq_type=FrequencyTypes.ANNUAL,
                float_freq_type=FrequencyTypes.ANNUAL, float_dc_type=DayCountTypes.ACT_360,
                bus_day_type=BusDayAdjustTypes.MODIFIED_FOLLOWING, interp_type=interp)


@pytest.mark.parametrize("scheme", SCHEMES, ids=lambda s: s.name)
def test_position_matches_oracle(gpu_ctx, scheme):
    model = F.gbp_model(interp=scheme)
    curve = model.curves.GBP_OIS_SONIA
    frns = _frns()
    for name, f in frns.items():
        reqs = ALL if name != "seasoned_no_fixing" else ALL[:3]     # its cash flows come from `value`, which raises
        res = f.position(model).compute(reqs)
        ref = frn_analytics(f, curve)
        face = f._face_value
        assert abs(res.value.amount - ref["value"]) / face < 1e-10, name
        assert np.max(np.abs(res.risk.risk_ladder - ref["delta"])) / face < 1e-10, name
        assert np.max(np.abs(res.gamma.risk_ladder - ref["gamma"])) / face < 1e-10, name
        assert res.risk.curve_type == CurveTypes.GBP_OIS_SONIA and len(res.risk.tenors) == len(curve.swap_times)
        if name == "seasoned_no_fixing":
            with pytest.raises(LibError):
                f.position(model).compute([RequestTypes.CASHFLOWS])
            continue
        items = res.cashflows.cashflows
        f.value(VD, curve, curve)
        coupons = [c for c in f._coupon_payments if abs(c) > 1e-10]
        assert len(items) == len(coupons) + 1 and items[-1].leg_type == "Principal", name
        assert items[-1].discount_factor == f._payment_dfs[-1] and items[-1].amount == face
        assert all(i.leg_type == "Floating_Coupon" for i in items[:-1])
    capped, plain = frns["capped"].position(model).compute(ALL[:3]), frns["5y_quarterly_act360"].position(model).compute(ALL[:3])
    assert capped.value.amount == plain.value.amount                         # the engine ignores the cap
    assert np.array_equal(capped.risk.risk_ladder, plain.risk.risk_ladder)


def test_usd_sofr_docstring_frn(gpu_ctx):
    model = F.usd_model()
    f = _frns(USD, CurveTypes.USD_OIS_SOFR, F.TEST_VALUE_DT)["5y_quarterly_act360"]
    res = f.position(model).compute(ALL[:3])
    ref = frn_analytics(f, model.curves.USD_OIS_SOFR)
    assert abs(res.value.amount - ref["value"]) / 100.0 < 1e-10
    assert np.max(np.abs(res.risk.risk_ladder - ref["delta"])) / 100.0 < 1e-10
    assert res.risk.curve_type == CurveTypes.USD_OIS_SOFR


def test_dual_curve_value_and_delta_raises(gpu_ctx):
    """A GBP FRN on SOFR: discounted on SONIA, forwards off the SOFR curve's engine tables (_float_leg_jax with a
    separate index curve); delta and gamma raise as in the reference."""
    from oracle import cavour_oracle as O
    from adrates_amd.utils.helpers import times_from_dates
    model = F.gbp_model()
    model.build_curve(**_usd_curve_args(InterpTypes.FLAT_FWD_RATES))
    disc, index = model.curves.GBP_OIS_SONIA, model.curves.USD_OIS_SOFR
    for f in (FRN(VD, "5Y", 0.005, Q, DayCountTypes.ACT_360, GBP, CurveTypes.USD_OIS_SOFR),
              FRN(VD, "3Y", 0.002, Q, DayCountTypes.ACT_365F, GBP, CurveTypes.USD_OIS_SOFR, first_fixing_rate=0.05,
                  payment_lag=2)):
        res = f.position(model).compute([RequestTypes.VALUE])
        dc = f._dc_type
        t = lambda dts: np.array([times_from_dates(d, VD, dc) for d in dts])
        dcache = O.cached_curve(disc.swap_rates, disc.swap_times, disc.year_fracs, derivatives=False)
        icache = O.cached_curve(index.swap_rates, index.swap_times, index.year_fracs, derivatives=False)
        idf = lambda x: O.simple_interpolate(x, icache["times"], icache["dfs"], index._interp_type.value).numpy()
        ddf = lambda x: O.simple_interpolate(x, dcache["times"], dcache["dfs"], disc._interp_type.value).numpy()
        al = np.array(f._year_fracs)
        fwd = (idf(t(f._start_accrued_dts)) / idf(t(f._end_accrued_dts)) - 1.0) / al
        if f._first_fixing_rate is not None:
            fwd[0] = f._first_fixing_rate
        tp = t(f._payment_dts)
        pv = float(np.sum(np.where(tp >= 0, (fwd + f._quoted_margin) * al * 100.0 * ddf(tp) / ddf(0.0), 0.0)))
        tm = times_from_dates(f._maturity_dt, VD, dc)
        pv += 100.0 * float(ddf(tm)) if tm > 0 else 0.0
        assert abs(res.value.amount - pv) / 100.0 < 1e-10
        with pytest.raises(LibError, match="Dual-curve FRN delta/gamma"):
            f.position(model).compute([RequestTypes.VALUE, RequestTypes.DELTA])
    with pytest.raises(LibError):
        FRNBook([f], model).compute([RequestTypes.GAMMA])


def test_portfolio_of_frns_bonds_and_ois_is_sum_of_singles(gpu_ctx):
    model = F.gbp_model()
    reqs = [RequestTypes.VALUE, RequestTypes.DELTA, RequestTypes.GAMMA]
    frns = list(_frns().values())
    positions = [Position(f, model) for f in frns]
    positions += [Position(Bond(VD, "10Y", 0.045, FrequencyTypes.SEMI_ANNUAL, DayCountTypes.ACT_365F, GBP), model),
                  Position(F.make_swap(VD, "10Y", 0.045, 1e6), model), Position(F.make_swap(VD, "3Y", 0.04, 1e6, pay=False), model)]
    # a coupon paid on the value date: its PV is added on the host in the aggregate as in the singles
    positions.append(Position(FRN(Date(30, 1, 2024), "2Y", 0.01, Q, DayCountTypes.ACT_365F, GBP, CurveTypes.GBP_OIS_SONIA),
                              model))
    total = Portfolio(positions).compute(reqs)
    singles = [p.compute(reqs) for p in positions]
    scale = 1e6
    assert abs(total.value.amount - sum(s.value.amount for s in singles)) / scale < 1e-10
    assert np.max(np.abs(total.risk.risk_ladder - sum(s.risk.risk_ladder for s in singles))) / scale < 1e-10
    assert np.max(np.abs(total.gamma.risk_ladder - sum(s.gamma.risk_ladder for s in singles))) / scale < 1e-10
    book = FRNBook(frns, model).compute(reqs, per_trade=True, aggregate=True)
    assert np.allclose(book["pv"], [s.value.amount for s in singles[:len(frns)]], rtol=0, atol=1e-14 * 1e6)
    assert book["agg_pv"] == pytest.approx(sum(s.value.amount for s in singles[:len(frns)]), rel=1e-12)


# ------------------------------------------------------------------------------------------------ adr_frn_measures
def close(a, b, rel=1e-12, scale=None):
    a, b = np.asarray(a), np.asarray(b)
    both_nan = np.isnan(a) & np.isnan(b)
    scale = np.maximum(1.0, np.abs(b)) if scale is None else scale
    return bool(np.all(both_nan | (np.abs(a - b) <= rel * scale)))


def same_measures(got, ref):
    """The GPU and its host twin differ only by their exp / log.  dv01 and duration are differences of two prices, so
    their error is measured on the scale of the price (the PV, and 1 / (2 bp))."""
    for k in _native.FRN_OUTPUTS:
        scale = {"dv01": np.maximum(1.0, np.abs(ref["pv"])), "mod_duration": 1.0 / (2 * 0.0001)}.get(k)
        assert close(got[k], ref[k], scale=scale), k


@pytest.fixture(scope="module")
def book_2000():
    model = F.gbp_model()
    curve = model.curves.GBP_OIS_SONIA
    frns, dm = random_frn_book(VD, 2000)
    book = FRNBook(frns, model)
    prices = _native.frn_measures_host(*book.inputs(dms=dm))["clean"]
    return book, prices, dm, curve


@pytest.mark.parametrize("mode", ["clean", "dm"])
def test_measures_gpu_matches_host(gpu_ctx, book_2000, mode):
    book, prices, dm, _ = book_2000
    kw = {"clean_prices": prices} if mode == "clean" else {"dms": dm}
    got = book.measures(**kw, ctx=gpu_ctx)
    host = _native.frn_measures_host(*book.inputs(**kw))
    assert np.array_equal(got["status"], host["status"]) and np.all(got["status"] == 0)
    same_measures(got, host)
    if mode == "clean":
        assert np.max(np.abs(got["dm"] - dm)) < 1e-12
    again = book.measures(**kw, ctx=gpu_ctx)
    for k in _native.FRN_OUTPUTS + ("status",):
        assert np.array_equal(again[k], got[k], equal_nan=True), k          # bit for bit from run to run


def test_measures_statuses_match_host(gpu_ctx):
    model = F.gbp_model()
    frns = [FRN(VD, "5Y", 0.005, Q, DayCountTypes.ACT_365F, GBP, CurveTypes.GBP_OIS_SONIA),
            FRN(Date(15, 1, 2024), "3Y", 0.005, Q, DayCountTypes.ACT_360, GBP, CurveTypes.GBP_OIS_SONIA)]
    book = FRNBook(frns, model)
    for quote in (40.0, -10.0, 99.0):
        got = book.measures(clean_prices=quote, dm_guess=0.1, ctx=gpu_ctx)
        host = _native.frn_measures_host(*book.inputs(clean_prices=quote, dm_guess=0.1))
        assert np.array_equal(got["status"], host["status"]) and got["status"][1] == 3
        same_measures(got, host)
    assert list(book.measures(clean_prices=-10.0, ctx=gpu_ctx)["status"]) == [2, 3]


def test_measures_dev_equals_host_arrays(gpu_ctx, book_2000):
    book, prices, _, _ = book_2000
    disc, index, arr, is_dm = book.inputs(clean_prices=prices)
    ref = _native.frn_measures(gpu_ctx, disc, index, arr, is_dm)
    off, cpn, frn = _native.frn_pack(arr)
    dev = torch.device("cuda", 0)
    host = {"disc_t": disc[1], "disc_df": disc[2], "index_t": index[1], "index_df": index[2], "cpn_off": off, "cpn": cpn,
            "frn": frn}
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in host.items()}
    n = len(prices)
    out = torch.empty((len(_native.FRN_OUTPUTS), n), dtype=torch.float64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    _native.frn_measures_dev(gpu_ctx, disc[0], disc[1].size, index[0], index[1].size, n, cpn.shape[1],
                             {k: v.data_ptr() for k, v in t.items()}, is_dm, out.data_ptr(), status.data_ptr(),
                             s.cuda_stream)
    s.synchronize()
    o, st = out.cpu().numpy(), status.cpu().numpy()
    assert np.array_equal(st, ref["status"])
    for i, k in enumerate(_native.FRN_OUTPUTS):
        assert np.array_equal(o[i], ref[k], equal_nan=True), k


def test_measures_one_million_frns(gpu_ctx, book_2000):
    """Every copy of an FRN with the same quote gives the same bits, whatever its place in the launch; the statuses
    match the host twin's."""
    book, prices, _, _ = book_2000
    base = dict(book.arrays)
    base["frn_quote"], base["frn_guess"] = prices, np.zeros(len(prices))
    reps = 500
    big = tile_frn_measures(base, reps)
    n = big["frn_quote"].size
    assert n == 1_000_000
    disc, index, _, _ = book.inputs(clean_prices=prices)
    got = _native.frn_measures(gpu_ctx, disc, index, big, False)
    host = _native.frn_measures_host(disc, index, base, False)
    assert np.array_equal(got["status"], np.tile(host["status"], reps))
    for k in _native.FRN_OUTPUTS:
        rows = got[k].reshape(reps, len(prices))
        assert np.array_equal(rows, np.broadcast_to(rows[0], rows.shape), equal_nan=True), k
    same_measures({k: got[k][:len(prices)] for k in _native.FRN_OUTPUTS}, host)
