"""oracle/port.c (batched C restatement, knot-DF space) against the torch.func oracle."""
import numpy as np
import pytest

from adrates_amd.trades import synthetic
from adrates_amd.trades.compiler import compile_ois
from adrates_amd.utils import DayCountTypes, FrequencyTypes, InterpTypes
from oracle import cavour_oracle as O
from oracle import port

from . import _fixtures as F
from ._parity import oracle_price, trade_errors


@pytest.mark.parametrize("interp", [InterpTypes.LINEAR_ZERO_RATES, InterpTypes.FLAT_FWD_RATES, InterpTypes.LINEAR_FWD_RATES])
def test_port_matches_ad_oracle(interp):
    vd = F.README_VALUE_DT
    curve = F.gbp_model(vd, interp).curves.GBP_OIS_SONIA
    cache = O.cached_curve(curve.swap_rates, curve.swap_times, curve.year_fracs)
    swaps = [F.make_swap(vd, "10Y", 0.045, 1e7), F.make_swap(vd, "55Y", 0.039, 5e6, pay=False),
             F.make_swap(vd, "5Y", 0.04, 1e6, fixed_freq=FrequencyTypes.SEMI_ANNUAL),
             F.make_swap(vd, "3Y", 0.04, 1e6, payment_lag=2, spread=0.002),
             F.make_swap(vd, "6Y", 0.04, 1e6, float_dc=DayCountTypes.THIRTY_E_360, pay=False),
             F.make_swap(vd, "1W", 0.052014), F.make_swap(vd, "1D", 0.05)]
    terms = synthetic.draw_terms(12, "offgrid", seed=5)
    swaps += synthetic.swaps_from_terms(vd, *terms)
    refs = oracle_price(curve, swaps, vd, cache)
    got = port.price(interp.value, cache["times"], cache["dfs"], cache["jac"], cache["hess"], compile_ois(swaps, vd))
    for i, (r, s) in enumerate(zip(refs, swaps)):
        e = trade_errors(got["pv"][i], got["delta"][i], got["gamma"][i], r["value"], r["delta"], r["gamma"],
                         s._notional)
        assert e < 1e-12, (i, e)


def test_port_threads_agree():
    vd = F.README_VALUE_DT
    curve = F.readme_model().curves.GBP_OIS_SONIA
    cache = O.cached_curve(curve.swap_rates, curve.swap_times, curve.year_fracs)
    b = synthetic.synthesize(vd, 3000, seed=3)
    one = port.price(4, cache["times"], cache["dfs"], cache["jac"], cache["hess"], b, n_threads=1)
    many = port.price(4, cache["times"], cache["dfs"], cache["jac"], cache["hess"], b, n_threads=4)
    for k in ("pv", "delta", "gamma"):
        assert np.array_equal(one[k], many[k])


def test_port_prices_long_legs_on_curves_of_more_than_1024_knots():
    """Monthly legs of 400 / 480 coupons touch up to 2 + 6 x 480 knots; on the 96-pillar curve (K = 1 585) each thread's
    local-knot scratch is sized from the batch (every such trade used to be refused).  Against the autodiff restatement."""
    from ._route_cases import batch, engine_curve
    vd = F.README_VALUE_DT
    host = engine_curve(vd, 96)
    assert host.times.shape[0] > 1024
    b, labels = batch(vd, ("very_long", "plain"))
    assert labels[:2] == ["very_long", "very_long"] and 2 + 6 * int(np.diff(b.flt_off).max()) > 1024
    got = port.price(4, host.times, host.dfs, host.jac, host.hess, b)
    cache = dict(times=host.times, dfs=host.dfs, jac=host.jac, hess=host.hess)
    for t in (0, 1, 3):
        f0, f1, l0, l1 = int(b.fix_off[t]), int(b.fix_off[t + 1]), int(b.flt_off[t]), int(b.flt_off[t + 1])
        fixed = dict(payment_times=b.fix_tp[f0:f1], payments=b.fix_pay[f0:f1], principal=0.0, leg_sign=float(b.fix_sign[t]))
        floating = dict(payment_times=b.flt_tp[l0:l1], start_times=b.flt_ts[l0:l1], end_times=b.flt_te[l0:l1],
                        pay_alphas=b.flt_alpha[l0:l1], spread=float(b.spread[t]), notional=float(b.notional[t]), principal=0.0,
                        leg_sign=float(b.flt_sign[t]))
        r = O.ois_analytics(cache, 4, fixed, floating)
        e = trade_errors(got["pv"][t], got["delta"][t], got["gamma"][t], r["value"], r["delta"], r["gamma"], b.notional[t])
        assert e < 1e-12, (labels[t], e)
