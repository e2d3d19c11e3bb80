"""Market inputs and builders shared by the benchmark, the tools, the examples and the tests (inputs only; no
expected values).

The two 32-pillar quote sets are the market inputs the reference's own tests and README use
(tests/test_ois_request_types.py:36-51, 88-103; README.md:69-78)."""

from ..models.models import Model
from .rates.ois import OIS
from ..utils import (BusDayAdjustTypes, CurrencyTypes, CurveTypes, Date, DayCountTypes, FrequencyTypes, InterpTypes,
                     SwapTypes)

GBP_PX = [5.1998, 5.2014, 5.2003, 5.2027, 5.2023, 5.19281,
          5.1656, 5.1482, 5.1342, 5.1173, 5.1013, 5.0862,
          5.0701, 5.054, 5.0394, 4.8707, 4.75483, 4.532,
          4.3628, 4.2428, 4.16225, 4.1132, 4.08505, 4.0762,
          4.078, 4.0961, 4.12195, 4.1315, 4.113, 4.07724, 3.984, 3.88]
USD_PX = [5.3500, 5.3200, 5.3100, 5.2900, 5.2700, 5.2500,
          5.2300, 5.2100, 5.1900, 5.1700, 5.1500, 5.1300,
          5.1100, 5.0900, 5.0700, 4.9500, 4.8500, 4.7000,
          4.5800, 4.4800, 4.4100, 4.3600, 4.3200, 4.2900,
          4.2700, 4.2800, 4.3000, 4.3200, 4.3100, 4.2900, 4.2400, 4.1800]
TENORS = ["1D", "1W", "2W", "1M", "2M", "3M", "4M", "5M", "6M",
          "7M", "8M", "9M", "10M", "11M", "1Y", "18M", "2Y",
          "3Y", "4Y", "5Y", "6Y", "7Y", "8Y", "9Y", "10Y",
          "12Y", "15Y", "20Y", "25Y", "30Y", "40Y", "50Y"]

README_VALUE_DT = Date(30, 4, 2024)
TEST_VALUE_DT = Date(17, 12, 2024)


def gbp_model(value_dt=README_VALUE_DT, interp=InterpTypes.LINEAR_ZERO_RATES, px=None, tenors=None,
              freq=FrequencyTypes.ANNUAL):
    m = Model(value_dt)
    m.build_curve(name="GBP_OIS_SONIA", px_list=list(px or GBP_PX), tenor_list=list(tenors or TENORS),
                  spot_days=0, swap_type=SwapTypes.PAY, fixed_dcc_type=DayCountTypes.ACT_365F,
                  fixed_freq_type=freq, float_freq_type=freq, float_dc_type=DayCountTypes.ACT_365F,
                  bus_day_type=BusDayAdjustTypes.MODIFIED_FOLLOWING, interp_type=interp)
    return m


def readme_model():
    return gbp_model()


def usd_model(value_dt=TEST_VALUE_DT, interp=InterpTypes.LINEAR_ZERO_RATES):
    m = Model(value_dt)
    m.build_curve(name="USD_OIS_SOFR", px_list=list(USD_PX), tenor_list=list(TENORS), spot_days=0,
                  swap_type=SwapTypes.PAY, fixed_dcc_type=DayCountTypes.ACT_360,
                  fixed_freq_type=FrequencyTypes.ANNUAL, float_freq_type=FrequencyTypes.ANNUAL,
                  float_dc_type=DayCountTypes.ACT_360, bus_day_type=BusDayAdjustTypes.MODIFIED_FOLLOWING,
                  interp_type=interp)
    return m


def make_swap(effective_dt, tenor, coupon, notional=1e6, pay=True, dc=DayCountTypes.ACT_365F,
              index=CurveTypes.GBP_OIS_SONIA, ccy=CurrencyTypes.GBP, fixed_freq=FrequencyTypes.ANNUAL,
              float_freq=FrequencyTypes.ANNUAL, float_dc=None, payment_lag=0, spread=0.0):
    return OIS(effective_dt=effective_dt, term_dt_or_tenor=tenor,
               fixed_leg_type=SwapTypes.PAY if pay else SwapTypes.RECEIVE, fixed_coupon=coupon,
               fixed_freq_type=fixed_freq, fixed_dc_type=dc, floating_index=index, currency=ccy,
               notional=notional, payment_lag=payment_lag, float_spread=spread,
               bd_type=BusDayAdjustTypes.MODIFIED_FOLLOWING, float_freq_type=float_freq,
               float_dc_type=float_dc or dc)


def random_bond_book(value_dt, n, seed=7, currency=CurrencyTypes.GBP):
    """``n`` fixed-rate bonds: bullet, zero-coupon (10%) and equal-principal amortizers (20% of the coupon bonds), issued
    up to five years before ``value_dt`` on 1Y-30Y tenors, with payment lags of 0-2 days and none maturing within a month;
    and a z-spread per bond between -2% and 6%."""
    import numpy as np
    from .credit.bond import Bond
    tenors = ["1Y", "2Y", "3Y", "5Y", "7Y", "10Y", "15Y", "20Y", "30Y"]
    freqs = [FrequencyTypes.ANNUAL, FrequencyTypes.SEMI_ANNUAL, FrequencyTypes.QUARTERLY]
    dcs = [DayCountTypes.ACT_365F, DayCountTypes.ACT_360, DayCountTypes.THIRTY_360_BOND]
    rng = np.random.default_rng(seed)
    bonds = []
    while len(bonds) < n:
        issue = value_dt.add_days(-int(rng.integers(0, 5 * 365)))
        tenor, freq, dc = (tenors[int(rng.integers(len(tenors)))], freqs[int(rng.integers(len(freqs)))],
                           dcs[int(rng.integers(len(dcs)))])
        kind = rng.random()
        coupon = 0.0 if kind < 0.1 else round(float(rng.uniform(0.005, 0.08)), 4)
        face = float(rng.choice([100.0, 1000.0, 1e6]))
        lag = int(rng.integers(0, 3))
        b = Bond(issue, tenor, coupon, freq, dc, currency, face_value=face, payment_lag=lag)
        if b._payment_dts[-1] <= value_dt.add_days(30):
            continue
        if kind > 0.8 and coupon > 0.0:
            b = Bond(issue, tenor, coupon, freq, dc, currency, face_value=face, payment_lag=lag,
                     amortization_schedule=Bond.generate_equal_principal_schedule(face, b._num_coupons))
        bonds.append(b)
    return bonds, rng.uniform(-0.02, 0.06, size=n)


def random_frn_book(value_dt, n, seed=7, currency=CurrencyTypes.GBP):
    """``n`` single-curve FRNs on ``currency``'s OIS index: 1Y-30Y tenors, monthly to annual coupons, ACT/360 or
    ACT/365F, margins of -50 to 300bp, payment lags of 0-2 days, faces of 100, 1 000 or 1 000 000.  About 30% are
    seasoned (issued up to five years before ``value_dt``, with a first fixing of 3-6%; none matures within a month, and
    every coupon after the fixed one starts on or after ``value_dt``), the rest issued within ten days after it; about
    10% are capped at 4-8%, 10% floored at 0-2% and 5% both.  Also returns a DM per FRN, between -1% and 4%."""
    import numpy as np
    from .credit.frn import FRN
    index = {CurrencyTypes.GBP: CurveTypes.GBP_OIS_SONIA, CurrencyTypes.USD: CurveTypes.USD_OIS_SOFR,
             CurrencyTypes.EUR: CurveTypes.EUR_OIS_ESTR}[currency]
    tenors = ["1Y", "2Y", "3Y", "4Y", "5Y", "7Y", "10Y", "12Y", "15Y", "20Y", "25Y", "30Y"]
    freqs = [FrequencyTypes.MONTHLY, FrequencyTypes.QUARTERLY, FrequencyTypes.SEMI_ANNUAL, FrequencyTypes.ANNUAL]
    dcs = [DayCountTypes.ACT_360, DayCountTypes.ACT_365F]
    rng = np.random.default_rng(seed)
    frns = []
    while len(frns) < n:
        seasoned = rng.random() < 0.3
        issue = value_dt.add_days(-int(rng.integers(1, 5 * 365)) if seasoned else int(rng.integers(0, 10)))
        tenor, freq, dc = (tenors[int(rng.integers(len(tenors)))], freqs[int(rng.integers(len(freqs)))],
                           dcs[int(rng.integers(len(dcs)))])
        margin = round(float(rng.uniform(-0.005, 0.03)), 5)
        kind = rng.random()
        cap = round(float(rng.uniform(0.04, 0.08)), 4) if kind < 0.1 or kind > 0.95 else None
        floor = round(float(rng.uniform(0.0, 0.02)), 4) if 0.1 <= kind < 0.2 or kind > 0.95 else None
        f = FRN(issue, tenor, margin, freq, dc, currency, index, face_value=float(rng.choice([100.0, 1000.0, 1e6])),
                payment_lag=int(rng.integers(0, 3)), cap_rate=cap, floor_rate=floor,
                first_fixing_rate=round(float(rng.uniform(0.03, 0.06)), 5) if seasoned else None)
        if f._payment_dts[-1] <= value_dt.add_days(30):
            continue
        live = [i for i, d in enumerate(f._payment_dts) if d > value_dt]
        if seasoned and f._end_accrued_dts[live[0]] < value_dt:
            continue                                  # the next coupon would need the index before its value date
        frns.append(f)
    return frns, rng.uniform(-0.01, 0.04, size=n)


# inflation: a UK RPI breakeven curve of 20 ZCIS pillars (1Y-50Y, 3.1-3.6%)
INFL_TENORS = ["1Y", "2Y", "3Y", "4Y", "5Y", "6Y", "7Y", "8Y", "9Y", "10Y",
               "12Y", "15Y", "20Y", "25Y", "30Y", "35Y", "40Y", "45Y", "50Y", "60Y"]
INFL_PX = [3.10, 3.18, 3.24, 3.29, 3.33, 3.36, 3.39, 3.41, 3.43, 3.45,
           3.47, 3.50, 3.53, 3.55, 3.56, 3.57, 3.58, 3.58, 3.59, 3.60]


def rpi_index(value_dt=README_VALUE_DT, base_index=360.0, lag_months=3, interp=None, seasonality=None):
    """A UK RPI index with monthly fixings for the 24 months up to ``value_dt`` (rising 0.25% a month), so that every
    lagged YoY start of a swap starting on ``value_dt`` has a fixing."""
    from ..market.indices.inflation_index import InflationIndex
    from ..utils.global_types import InflationIndexTypes, InflationInterpTypes
    idx = InflationIndex(InflationIndexTypes.UK_RPI, value_dt.add_months(-24), base_index, CurrencyTypes.GBP, lag_months,
                         interp or InflationInterpTypes.LINEAR, seasonality)
    for k in range(1, 25):
        idx.add_fixing(value_dt.add_months(-24 + k), base_index * (1.0 + 0.0025 * k))
    return idx


def inflation_curve(value_dt=README_VALUE_DT, interp=None, tenors=None, px=None, index=None, base_cpi=380.0):
    """The GBP RPI inflation curve from par ZCIS quotes in percent (`INFL_TENORS` / `INFL_PX` by default)."""
    from ..market.curves.inflation_curve import InflationCurve
    from ..utils.global_types import InflationIndexTypes, InflationInterpTypes
    from .rates.zcis import ZeroCouponInflationSwap
    index = index or rpi_index(value_dt)
    swaps = [ZeroCouponInflationSwap(value_dt, t, SwapTypes.PAY, p / 100.0, index)
             for t, p in zip(tenors or INFL_TENORS, px or INFL_PX)]
    return InflationCurve(value_dt, swaps, base_cpi, CurrencyTypes.GBP, InflationIndexTypes.UK_RPI,
                          interp_type=interp or InflationInterpTypes.LINEAR, check_refit=True)


def yoy_model(value_dt=README_VALUE_DT, interp=InterpTypes.LINEAR_ZERO_RATES, infl_interp=None, **curve_kw):
    """`gbp_model` with the RPI inflation curve put into the model's curve dict as GBP_RPI_INFLATION."""
    m = gbp_model(value_dt, interp)
    m._curves_dict["GBP_RPI_INFLATION"] = inflation_curve(value_dt, infl_interp, **curve_kw)
    return m


def random_yoy_book(value_dt, n, seed=7, index=None):
    """``n`` YoY RPI swaps: annual coupons, 5Y-30Y, effective up to a year before to a month after ``value_dt``, pay
    or receive fixed at 2.5-4%, notionals of 1-100 million, inflation spreads of -20 to 20bp, ACT/365F or ACT/ACT."""
    import numpy as np
    from .rates.yoy_inflation_swap import YoYInflationSwap
    index = index or rpi_index(value_dt)
    rng = np.random.default_rng(seed)
    dcs = [DayCountTypes.ACT_365F, DayCountTypes.ACT_ACT_ISDA]
    out = []
    for _ in range(n):
        eff = value_dt.add_days(int(rng.integers(-365, 31)))
        out.append(YoYInflationSwap(eff, f"{int(rng.integers(5, 31))}Y",
                                    SwapTypes.PAY if rng.random() < 0.5 else SwapTypes.RECEIVE,
                                    round(float(rng.uniform(0.025, 0.04)), 5), index, FrequencyTypes.ANNUAL,
                                    notional=float(rng.choice([1e6, 1e7, 1e8])),
                                    inflation_spread=round(float(rng.uniform(-0.002, 0.002)), 5),
                                    dc_type=dcs[int(rng.integers(len(dcs)))]))
    return out
