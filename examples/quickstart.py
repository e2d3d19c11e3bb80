#!/usr/bin/env python3
"""The reference README's sections 1-3 (build a curve, price an OIS with VALUE / DELTA / GAMMA, aggregate a
portfolio) with `cavour.` replaced by `adrates_amd.`, followed by what this implementation adds on the same path:
a scenario grid bootstrapped and priced on the GPU, a book revalued under 250 scenarios (VaR / ES), the CASHFLOWS request and the vectorised trade compiler.

Run on an MI355X after `python -c "import __graft_entry__ as g; g.build()"`:  python examples/quickstart.py
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401  (the device-chained calls below hold their buffers in torch tensors: load torch's HIP runtime first)

from adrates_amd.market.curves.interpolator import InterpTypes
from adrates_amd.market.portfolio.portfolio import Portfolio
from adrates_amd.market.position.scenarios import (ScenarioGrid, bump_ladder, expected_shortfall, finite_difference_delta,
                                                   historical_var)
from adrates_amd.models.models import Model
from adrates_amd.trades.compiler import OISTerms, compile_ois_terms
from adrates_amd.trades.rates.ois import OIS
from adrates_amd.utils.calendar import BusDayAdjustTypes
from adrates_amd.utils.currency import CurrencyTypes
from adrates_amd.utils.date import Date
from adrates_amd.utils.day_count import DayCountTypes
from adrates_amd.utils.frequency import FrequencyTypes
from adrates_amd.utils.global_types import CurveTypes, RequestTypes, SwapTypes

# ---- 1. curve (README.md:60-101)
value_dt = Date(30, 4, 2024)
px_list = [5.1998, 5.2014, 5.2003, 5.2027, 5.2023, 5.19281, 5.1656, 5.1482, 5.1342, 5.1173, 5.1013, 5.0862, 5.0701,
           5.054, 5.0394, 4.8707, 4.75483, 4.532, 4.3628, 4.2428, 4.16225, 4.1132, 4.08505, 4.0762, 4.078, 4.0961,
           4.12195, 4.1315, 4.113, 4.07724, 3.984, 3.88]
tenor_list = ["1D", "1W", "2W", "1M", "2M", "3M", "4M", "5M", "6M", "7M", "8M", "9M", "10M", "11M", "12M", "18M", "2Y",
              "3Y", "4Y", "5Y", "6Y", "7Y", "8Y", "9Y", "10Y", "12Y", "15Y", "20Y", "25Y", "30Y", "40Y", "50Y"]
model = Model(value_dt)
model.build_curve(name="GBP_OIS_SONIA", px_list=px_list, tenor_list=tenor_list, spot_days=0,
                  swap_type=SwapTypes.PAY, fixed_dcc_type=DayCountTypes.ACT_365F,
                  fixed_freq_type=FrequencyTypes.ANNUAL, float_freq_type=FrequencyTypes.ANNUAL,
                  float_dc_type=DayCountTypes.ACT_365F, bus_day_type=BusDayAdjustTypes.MODIFIED_FOLLOWING,
                  interp_type=InterpTypes.LINEAR_ZERO_RATES)
curve = model.curves.GBP_OIS_SONIA
print(f"5Y discount factor: {curve.df_ad(5.0):.6f}")

# ---- 2. one swap: VALUE, DELTA, GAMMA (README.md:105-160)
swap = OIS(effective_dt=value_dt, term_dt_or_tenor="10Y", fixed_leg_type=SwapTypes.PAY, fixed_coupon=0.045,
           fixed_freq_type=FrequencyTypes.ANNUAL, fixed_dc_type=DayCountTypes.ACT_365F,
           floating_index=CurveTypes.GBP_OIS_SONIA, currency=CurrencyTypes.GBP, notional=10_000_000,
           bd_type=BusDayAdjustTypes.MODIFIED_FOLLOWING, float_freq_type=FrequencyTypes.ANNUAL,
           float_dc_type=DayCountTypes.ACT_365F)
res = swap.position(model).compute([RequestTypes.VALUE, RequestTypes.DELTA, RequestTypes.GAMMA, RequestTypes.CASHFLOWS])
print(f"PV {res.value.amount:,.2f} {res.value.currency.name}   total delta {res.risk.value.amount:,.4f} per bp"
      f"   total gamma {res.gamma.value.amount:.6f} per bp^2")
print("10Y bucket delta:", dict(zip(res.risk.tenors, res.risk.risk_ladder))["10Y"])
print(res.cashflows, "| fixed leg PV", f"{res.cashflows.fixed().total_pv:,.2f}")

# ---- 3. portfolio (README.md:164-230)
others = [OIS(value_dt, t, SwapTypes.RECEIVE, c, FrequencyTypes.ANNUAL, DayCountTypes.ACT_365F, CurveTypes.GBP_OIS_SONIA,
              CurrencyTypes.GBP, notional=n, bd_type=BusDayAdjustTypes.MODIFIED_FOLLOWING,
              float_freq_type=FrequencyTypes.ANNUAL, float_dc_type=DayCountTypes.ACT_365F)
          for t, c, n in (("87M", 0.04, 1e7), ("3M", 0.05, 2e6), ("30Y", 0.039, 5e6))]
book = Portfolio([s.position(model) for s in [swap] + others]).compute([RequestTypes.VALUE, RequestTypes.DELTA,
                                                                        RequestTypes.GAMMA])
print(f"portfolio PV {book.value.amount:,.2f}, delta {book.risk.value.amount:,.4f}, gamma {book.gamma.value.amount:.6f}")

# ---- scenario grid: 65 shocked curves bootstrapped (with Jacobians) and priced on the GPU
grid = ScenarioGrid(model, "GBP_OIS_SONIA", bump_ladder(tenor_list, 1.0), with_gamma=False)
pv = grid.price([swap] + others, [RequestTypes.VALUE])["pv"]
fd = finite_difference_delta(pv, 1.0)
print("bump-and-reprice vs analytic 10Y delta of the first swap:", fd[0][24], "vs", res.risk.risk_ladder[24])
grid.close()

# ---- full revaluation: a 1 000-swap book under 250 parallel + twist shocks in one launch, then VaR and ES
rng = np.random.default_rng(7)
slope = np.linspace(-1.0, 1.0, len(tenor_list))
shocks = [{t: float(par + twist * slope[k]) for k, t in enumerate(tenor_list)}       # in the quotes' units: percent
          for par, twist in zip(rng.normal(0.0, 0.08, 250), rng.normal(0.0, 0.04, 250))]
book_swaps = [OIS(value_dt, f"{int(m)}M", SwapTypes.PAY if p else SwapTypes.RECEIVE, float(c), FrequencyTypes.ANNUAL,
                  DayCountTypes.ACT_365F, CurveTypes.GBP_OIS_SONIA, CurrencyTypes.GBP, notional=float(nn),
                  bd_type=BusDayAdjustTypes.MODIFIED_FOLLOWING, float_freq_type=FrequencyTypes.ANNUAL,
                  float_dc_type=DayCountTypes.ACT_365F)
              for m, c, nn, p in zip(rng.integers(1, 361, 1000), rng.uniform(0.03, 0.05, 1000),
                                     np.round(rng.uniform(1e6, 5e7, 1000), -5), rng.random(1000) < 0.5)]
grid = ScenarioGrid(model, "GBP_OIS_SONIA", shocks, with_gamma=False)
pnl = grid.pnl(book_swaps)
print(f"1 000 swaps x 250 scenarios: 99% VaR {historical_var(pnl, 0.99):,.0f}, 97.5% ES {expected_shortfall(pnl, 0.975):,.0f} GBP "
      f"(worst scenario {pnl.min():,.0f}, best {pnl.max():,.0f})")

# ---- the same launch per desk: one key per trade, one P&L row, VaR and ES per sub-book (rows never leave the GPU)
desks = [f"desk {int(d)}" for d in rng.integers(0, 8, len(book_swaps))]
per_desk = grid.sub_book_var_es(book_swaps, desks, level=0.99)
worst = int(np.argmax(per_desk["var"]))
print(f"8 desks: largest 99% VaR {per_desk['var'][worst]:,.0f} GBP ({per_desk['labels'][worst]}), its ES "
      f"{per_desk['es'][worst]:,.0f}; sum of desk VaRs {per_desk['var'].sum():,.0f} against the book's "
      f"{historical_var(pnl, 0.99):,.0f}")

# ---- the desks' intraday number without revaluing: their delta and gamma ladders times the shocks, and what that leaves out
explain = grid.explain_sub_books(book_swaps, desks)                # full revaluation, delta P&L, gamma P&L, unexplained: [8, 250] each
dg_tail = grid.sub_book_delta_gamma_var_es(book_swaps, desks, level=0.99)      # ladders -> P&L -> VaR / ES, all on the device
print(f"delta-gamma 99% VaR of {per_desk['labels'][worst]}: {dg_tail['var'][worst]:,.0f} GBP against {per_desk['var'][worst]:,.0f} "
      f"by full revaluation; largest unexplained P&L {np.abs(explain['unexplained']).max():,.0f} GBP of a largest move of "
      f"{np.abs(explain['full']).max():,.0f}")

# ---- inflation swaps under JOINT scenarios: the same 250 OIS curves, each paired with a breakeven move (basis points)
from adrates_amd.market.position.yoy_book import YoYBook
from adrates_amd.trades.market_data import inflation_curve, random_yoy_book
model._curves_dict["GBP_RPI_INFLATION"] = inflation_curve(value_dt)
yoy_book = YoYBook(random_yoy_book(value_dt, 500, seed=3), model)
breakeven_moves = [float(x) for x in rng.normal(0.0, 12.0, 250)]
yoy_pnl = yoy_book.pnl(grid=grid, inflation_shocks=breakeven_moves)
print(f"500 YoY swaps x 250 joint scenarios: 99% VaR {historical_var(yoy_pnl, 0.99):,.0f}, 97.5% ES "
      f"{expected_shortfall(yoy_pnl, 0.975):,.0f} GBP; breakevens alone: 99% VaR "
      f"{historical_var(yoy_book.pnl(inflation_shocks=breakeven_moves), 0.99):,.0f} GBP")

# ---- a bond book at its z-spreads under JOINT scenarios: the same 250 OIS curves, each paired with a spread move per issuer
from adrates_amd.market.position.bond_book import BondBook
from adrates_amd.market.position.scenarios import shocked_spreads
from adrates_amd.trades.market_data import random_bond_book
bonds, _ = random_bond_book(value_dt, 300, seed=5)
bond_book = BondBook(bonds, model)
z = bond_book.measures(clean_prices=rng.uniform(90.0, 110.0, len(bonds)))["z"]       # the spreads the market prices imply
z = np.where(np.isfinite(z), z, 0.0)                                                  # (no root: priced on the curve)
issuers = [f"issuer {i % 8}" for i in range(len(bonds))]
labels = list(dict.fromkeys(issuers))                                                 # buckets in order of first appearance
spread_moves = np.stack([shocked_spreads(labels, {lab: float(m) for lab, m in zip(labels, row)})   # basis points
                         for row in rng.normal(0.0, 15.0, (250, len(labels)))])
credit_pnl = grid.pnl_credit(bonds, z, issuers, spread_moves)
print(f"300 bonds x 250 joint scenarios: 99% VaR {historical_var(credit_pnl, 0.99):,.0f}, 97.5% ES "
      f"{expected_shortfall(credit_pnl, 0.975):,.0f}; rates alone: 99% VaR "
      f"{historical_var(grid.pnl_credit(bonds, z, issuers), 0.99):,.0f}")

# ---- the bond desks' credit Greeks from one launch chain: CS01 per issuer, and the joint delta-gamma P&L set beside the revaluation
bond_desks = [f"credit desk {i % 3}" for i in range(len(bonds))]
cs = grid.pnl_credit_delta_gamma_sub_books(bonds, z, bond_desks, issuers, spread_moves)           # ladders at the spreads + spread Greeks
cr = grid.explain_credit_sub_books(bonds, z, bond_desks, issuers, spread_moves)                   # against pnl_credit_sub_books
print(f"{cs['labels'][0]}: CS01 by issuer {np.round(cs['cs01'][0], 0).tolist()} GBP per bp, DV01 {cs['delta'][0].sum():,.0f}; "
      f"largest unexplained P&L of the 3 desks {np.abs(cr['unexplained']).max():,.0f} GBP of a largest move of "
      f"{np.abs(cr['full']).max():,.0f}")

# ---- firm-wide: desks across the OIS book and the YoY book, their P&L rows added by label, the firm's ES split among them
from adrates_amd.market.position.scenarios import allocate_tail, combine_sub_book_rows
yoy_desks = [("desk 0", "desk 1", "inflation desk")[i % 3] for i in range(len(yoy_book))]
firm = combine_sub_book_rows([                                      # labels are numbered by first appearance in each call
    (list(dict.fromkeys(desks)), grid.pnl_sub_books(book_swaps, desks)),
    (list(dict.fromkeys(yoy_desks)), yoy_book.pnl_sub_books(yoy_desks, grid=grid, inflation_shocks=breakeven_moves))])
alloc = allocate_tail(firm["rows"], level=0.975)                    # the Euler allocation: each desk's mean loss in the firm's tail
top = int(np.argmax(alloc["comp_es"]))
print(f"{len(firm['labels'])} desks across rates and inflation: firm 97.5% ES {alloc['es']:,.0f} GBP = sum of the desks' shares "
      f"{alloc['comp_es'].sum():,.0f}; the largest share {alloc['comp_es'][top]:,.0f} ({firm['labels'][top]})")
grid.close()

# ---- a million trades from their terms, without a million Python objects
n = 1_000_000
rng = np.random.default_rng(1)
t0 = time.perf_counter()
months = rng.integers(1, 361, n)
names = {m: f"{m}M" for m in range(1, 361)}
batch = compile_ois_terms(OISTerms(value_dt, [names[int(m)] for m in months], rng.uniform(0.01, 0.07, n),
                                   np.round(rng.uniform(1e6, 5e7, n), -5), rng.random(n) < 0.5, FrequencyTypes.ANNUAL,
                                   DayCountTypes.ACT_365F, CurveTypes.GBP_OIS_SONIA, CurrencyTypes.GBP,
                                   float_freq_type=FrequencyTypes.ANNUAL, float_dc_type=DayCountTypes.ACT_365F,
                                   bd_type=BusDayAdjustTypes.MODIFIED_FOLLOWING), value_dt)
print(f"compiled {batch.n_trades:,} trades in {time.perf_counter() - t0:.1f} s")
from adrates_amd import _native
from adrates_amd.market.curves.curve_tables import build_engine_curve
host = build_engine_curve(curve.swap_rates, curve.swap_times, curve.year_fracs)
ctx = _native.default_context()
dc = _native.DeviceCurve(ctx, curve._interp_type.value, host.times, host.dfs, host.jac, host.hess)
dt = _native.DeviceTrades(ctx, batch)
t0 = time.perf_counter()
agg = _native.price(ctx, dc, dt, per_trade=False, aggregate=True)
print(f"portfolio ladder of {n:,} trades (PV + delta + gamma, aggregated on the device) in "
      f"{1e3 * (time.perf_counter() - t0):.1f} ms: PV {agg['agg_pv']:,.0f}, delta {agg['agg_delta'].sum():,.1f}")

# ---- cross-currency: a USD curve, the GBP/USD basis curve, a basis swap and an OIS under USD collateral
from adrates_amd.trades.rates.xccy_basis_swap import XccyBasisSwap
from adrates_amd.utils import CollateralType
usd_px = [5.35, 5.32, 5.31, 5.29, 5.27, 5.25, 5.23, 5.21, 5.19, 5.17, 5.15, 5.13, 5.11, 5.09, 5.07, 4.95, 4.85, 4.70,
          4.58, 4.48, 4.41, 4.36, 4.32, 4.29, 4.27, 4.28, 4.30, 4.32, 4.31, 4.29, 4.24, 4.18]
model.build_curve(name="USD_OIS_SOFR", px_list=usd_px, tenor_list=tenor_list, spot_days=0, swap_type=SwapTypes.PAY,
                  fixed_dcc_type=DayCountTypes.ACT_360, fixed_freq_type=FrequencyTypes.ANNUAL,
                  float_freq_type=FrequencyTypes.ANNUAL, float_dc_type=DayCountTypes.ACT_360,
                  bus_day_type=BusDayAdjustTypes.MODIFIED_FOLLOWING, interp_type=InterpTypes.FLAT_FWD_RATES)
basis_tenors = ["1Y", "2Y", "3Y", "5Y", "7Y", "10Y", "15Y", "20Y", "30Y"]
basis_bp = [25.0, 28.0, 30.0, 34.0, 36.0, 39.0, 42.0, 45.0, 48.0]
for name, dom, frn, spreads, fx in (("USD_GBP_BASIS", "GBP_OIS_SONIA", "USD_OIS_SOFR", basis_bp, 0.79),
                                    ("GBP_USD_XCCY", "USD_OIS_SOFR", "GBP_OIS_SONIA", [-b for b in basis_bp], 1 / 0.79)):
    model.build_xccy_curve(name=name, domestic_curve_name=dom, foreign_curve_name=frn, basis_spreads=spreads,
                           tenor_list=basis_tenors, spot_fx=fx,
                           domestic_dc_type=DayCountTypes.ACT_365F if dom.startswith("GBP") else DayCountTypes.ACT_360,
                           foreign_dc_type=DayCountTypes.ACT_360 if dom.startswith("GBP") else DayCountTypes.ACT_365F,
                           interp_type=InterpTypes.FLAT_FWD_RATES)
xccy = XccyBasisSwap(effective_dt=value_dt, term_dt_or_tenor="7Y", domestic_notional=7_900_000, foreign_notional=10_000_000,
                     domestic_spread=0.0, foreign_spread=0.0040, domestic_freq_type=FrequencyTypes.ANNUAL,
                     foreign_freq_type=FrequencyTypes.SEMI_ANNUAL, domestic_dc_type=DayCountTypes.ACT_365F,
                     foreign_dc_type=DayCountTypes.ACT_360, domestic_floating_index=CurveTypes.GBP_OIS_SONIA,
                     foreign_floating_index=CurveTypes.USD_OIS_SOFR, domestic_currency=CurrencyTypes.GBP,
                     foreign_currency=CurrencyTypes.USD)
x = xccy.position(model).compute([RequestTypes.VALUE, RequestTypes.DELTA, RequestTypes.GAMMA])
print(f"7Y GBP/USD basis swap: PV {x.value.amount:,.2f} GBP; delta per bp - SONIA {x.risk.GBP_OIS_SONIA.value.amount:,.2f}, "
      f"SOFR {x.risk.USD_OIS_SOFR.value.amount:,.2f}, basis {x.risk.USD_GBP_BASIS.value.amount:,.2f}; "
      f"basis gamma {x.gamma.USD_GBP_BASIS.value.amount:.4f}")
cross = x.gamma.cross_gamma(CurveTypes.USD_OIS_SOFR, CurveTypes.USD_GBP_BASIS)     # d2 PV / d(SOFR quote) d(basis spread), per bp^2
print(f"foreign OIS x basis cross-gamma: {cross.risk_matrix.shape[0]} x {cross.risk_matrix.shape[1]} ladder, total "
      f"{cross.value.amount:.6f} {cross.value.currency.name}")
c = swap.position(model).compute([RequestTypes.VALUE, RequestTypes.DELTA], collateral_type=CollateralType.USD)
print(f"the 10Y OIS under USD collateral: PV {c.value.amount:,.2f} {c.value.currency.name} "
      f"(vs {res.value.amount / 0.79:,.2f} converted at spot), basis delta {c.risk.USD_GBP_BASIS.value.amount:,.2f} per bp")
