"""Year-on-year inflation swaps in the valuation engine: VALUE, two-curve DELTA / GAMMA and CASHFLOWS.

Restates cavour/market/position/engine.py:986-1408 (`_compute_yoy_iis`).  The reference differentiates each curve with
the other held fixed and leaves the discount x inflation cross gamma at zero, so the work splits in two:

- inflation side: one launch of adr_yoy_risk (csrc/yoy_risk.hip) projects every YoY amount and returns the inflation
  leg's delta and gamma with respect to the breakeven rates, in closed form;
- discount side: with the inflation curve fixed a YoY swap is a fixed-flows-only trade - the fixed coupons plus the
  projected amounts the kernel wrote, bit for bit - priced through the OIS route as bonds are
  (`trades/compiler.py::compile_yoy_swaps`).  Its PV is the swap's VALUE.

Quirks kept on purpose:
- the engine ignores the inflation index: no lag, no fixings, no base CPI and no seasonality.  Each coupon is
  ``N alpha (I(te) / I(ts) - 1 + spread) D(tp) / D(tv)`` with ``ts = te.add_months(-12)``, all times in the swap's day
  count from the model's value date, on the inflation curve's nodes read by simple_interpolate.  `YoYInflationSwap.value`
  goes through the index instead, so the two PVs differ;
- the discount curve is chosen by currency, the inflation curve by ``(currency, index_type.name)``; both are read from
  ``model.curves`` (the user puts the inflation curve into the model's curve dict);
- CASHFLOWS values the swap with `value` on the curves' own nodes and reports the fixed leg's payments.  The YoY items
  need ``_payment_pvs`` on the YoY leg, which keeps its results in ``_pvs`` instead, so none are reported;
- a ZCIS has no ``derivative_type`` and never reaches this path.
"""
from __future__ import annotations

import numpy as np

from ... import _native
from ...requests.results import AnalyticsResult, CashflowItem, Cashflows, Delta, Gamma, Risk, Valuation
from ...trades.compiler import compile_yoy_coupons, compile_yoy_swaps
from ...utils.currency import CurrencyTypes
from ...utils.error import LibError
from ...utils.global_types import CurveTypes, InterpTypes, RequestTypes, SwapTypes
from ...utils.helpers import to_tenor

DISCOUNT_CURVES = {CurrencyTypes.GBP: "GBP_OIS_SONIA", CurrencyTypes.USD: "USD_OIS_SOFR", CurrencyTypes.EUR: "EUR_OIS_ESTR"}
INFLATION_CURVES = {
    (CurrencyTypes.GBP, "UK_RPI"): "GBP_RPI_INFLATION",
    (CurrencyTypes.GBP, "UK_CPI"): "GBP_CPI_INFLATION",
    (CurrencyTypes.USD, "US_CPI_U"): "USD_CPI_INFLATION",
    (CurrencyTypes.EUR, "EUR_HICP"): "EUR_HICP_INFLATION",
}
_INFL_SCHEMES = (InterpTypes.LINEAR_ZERO_RATES, InterpTypes.FLAT_FWD_RATES)


def yoy_curves(model, currency, index_type_name):
    """``(discount curve, inflation curve, discount CurveTypes, inflation CurveTypes)`` of a YoY swap
    (engine.py:997-1045, 1187-1202)."""
    if currency not in DISCOUNT_CURVES:
        raise LibError(f"No default OIS curve for currency {currency}")
    disc_name = DISCOUNT_CURVES[currency]
    disc = getattr(model.curves, disc_name, None)
    if disc is None:
        raise LibError(f"Discount curve {disc_name} not found in model")
    key = (currency, index_type_name)
    if key not in INFLATION_CURVES:
        raise LibError(f"No inflation curve mapping for {currency.name} {index_type_name}. "
                       f"Add to model.curves as {currency.name}_{index_type_name}_INFLATION")
    infl_name = INFLATION_CURVES[key]
    infl = getattr(model.curves, infl_name, None)
    if infl is None:
        raise LibError(f"Inflation curve {infl_name} not found in model")
    return disc, infl, CurveTypes[disc_name], CurveTypes[infl_name]


def inflation_inputs(infl):
    """``(interp method, pillar times T, breakeven rates b)`` of an inflation curve, for adr_yoy_risk."""
    if infl._interp_type not in _INFL_SCHEMES:
        raise LibError("Invalid interpolation scheme.")
    return (infl._interp_type.value, np.asarray(infl.swap_times, dtype=np.float64),
            np.array([z._fixed_rate for z in infl._used_swaps], dtype=np.float64))


def price_yoy(engine, disc, infl, swaps, reqs, per_trade=True, aggregate=False, ctx=None):
    """Both sides of a YoY book: one adr_yoy_risk launch, then one discount-side batch through the route.

    Returns ``pv`` / ``agg_pv`` (the swaps' total PV), ``delta`` / ``gamma`` / ``agg_*`` on the discount curve,
    ``infl_pv``, ``infl_delta``, ``infl_gamma`` (and ``agg_infl_*``) from the kernel, ``amount`` [m], and the tenors."""
    cur = engine._device_curve(disc)
    host = cur["host"]
    value_dt = engine.model.value_dt                        # engine.py:1085: times from the model's value date
    book = compile_yoy_coupons(swaps, value_dt)
    mask = sum(r for q, r in ((RequestTypes.VALUE, _native.REQ_VALUE), (RequestTypes.DELTA, _native.REQ_DELTA),
                              (RequestTypes.GAMMA, _native.REQ_GAMMA)) if q in reqs)
    k = _native.yoy_risk(ctx or cur["ctx"], (disc._interp_type.value, host.times, host.dfs), inflation_inputs(infl), book,
                         mask, per_swap=per_trade, aggregate=aggregate)
    dev_trades = _native.DeviceTrades(cur["ctx"], compile_yoy_swaps(swaps, value_dt, k["amount"]))
    try:
        out = _native.price(cur["ctx"], cur["dev"], dev_trades,
                            want_value=RequestTypes.VALUE in reqs,
                            want_delta=RequestTypes.DELTA in reqs,
                            want_gamma=RequestTypes.GAMMA in reqs,
                            per_trade=per_trade, aggregate=aggregate)
    finally:
        dev_trades.close()
    out["amount"] = k["amount"]
    for name in ("pv", "delta", "gamma"):
        if per_trade:
            out["infl_" + name] = k[name]
        if aggregate:
            out["agg_infl_" + name] = k["agg_" + name]
    out["tenors"] = cur["tenors"]
    out["infl_tenors"] = to_tenor(list(infl.swap_times))
    return out


def compute_yoy(engine, swap, reqs):
    """`Engine.compute` for a `YoYInflationSwap` (engine.py:986-1408)."""
    currency = swap._inflation_index._currency
    disc, infl, disc_type, infl_type = yoy_curves(engine.model, currency, swap._inflation_index._index_type.name)
    value = delta = gamma = cashflows = None
    if reqs & {RequestTypes.VALUE, RequestTypes.DELTA, RequestTypes.GAMMA}:
        res = price_yoy(engine, disc, infl, [swap], reqs)
        if RequestTypes.VALUE in reqs:
            value = Valuation(amount=float(res["pv"][0]), currency=currency)
        if RequestTypes.DELTA in reqs:
            delta = Risk([Delta(risk_ladder=np.array(res["delta"][0]), tenors=res["tenors"], currency=currency,
                                curve_type=disc_type),
                          Delta(risk_ladder=np.array(res["infl_delta"][0]), tenors=res["infl_tenors"], currency=currency,
                                curve_type=infl_type)])
        if RequestTypes.GAMMA in reqs:
            gamma = Risk([Gamma(risk_ladder=np.array(res["gamma"][0]), tenors=res["tenors"], currency=currency,
                                curve_type=disc_type),
                          Gamma(risk_ladder=np.array(res["infl_gamma"][0]), tenors=res["infl_tenors"], currency=currency,
                                curve_type=infl_type)])
    if RequestTypes.CASHFLOWS in reqs:
        cashflows = yoy_cashflows(engine, swap, disc, infl, currency)
    return AnalyticsResult(value=value, risk=delta, gamma=gamma, cashflows=cashflows)


def yoy_cashflows(engine, swap, disc, infl, currency):
    """engine.py:1355-1406: `value` at the model's value date, then the fixed leg's items and - where the YoY leg has
    ``_payment_pvs``, which it never has - its items."""
    swap.value(engine.model.value_dt, disc, infl)
    fixed_type = "Fixed_Pay" if swap._fixed_leg_type == SwapTypes.PAY else "Fixed_Rec"
    items = engine._extract_leg_cashflows(swap._fixed_leg, fixed_type)
    leg = swap._inflation_leg
    yoy_type = "YoY_Inflation_Rec" if swap._fixed_leg_type == SwapTypes.PAY else "YoY_Inflation_Pay"
    if getattr(leg, "_payment_pvs", None):
        sign = +1.0 if "Rec" in yoy_type else -1.0
        for i, pay_dt in enumerate(leg._payment_dts):
            notional = float(leg._notional)
            rate = float(leg._yoy_rates[i]) + float(leg._spread)
            items.append(CashflowItem(payment_date=pay_dt, notional=notional, payment_fraction=rate,
                                      accrual_period=float(leg._year_fracs[i]), amount=sign * float(leg._payments[i]),
                                      discount_factor=float(leg._payment_dfs[i]),
                                      discounted_amount=sign * float(leg._payment_pvs[i]), leg_type=yoy_type))
    return Cashflows(items, currency)
