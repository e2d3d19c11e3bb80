"""Books and scenario curves shared by the scenario-revaluation tests (tests/test_scenario_pv_host.py, CPU, and
tests/test_gpu_scenario_pv.py, GPU), and the C-oracle loop both compare with."""
import numpy as np

from adrates_amd.market.curves.curve_tables import build_engine_curve
from adrates_amd.market.position.scenarios import _concat_batches
from adrates_amd.trades import synthetic
from adrates_amd.trades.compiler import OISTerms, TradeBatch, compile_bonds, compile_frns, compile_ois_terms
from adrates_amd.utils import BusDayAdjustTypes, CurrencyTypes, CurveTypes, DayCountTypes, FrequencyTypes, InterpTypes
from oracle import port

from . import _fixtures as F
from ._parity import unit_notional_err

VD = F.README_VALUE_DT
SCHEMES = (InterpTypes.LINEAR_ZERO_RATES, InterpTypes.FLAT_FWD_RATES, InterpTypes.LINEAR_FWD_RATES)
BP = 1e-4


def shocked_curves(curve=None):
    """``(times [K], dfs [S, K])``: the host builder's curves for parallel shifts of +-1, +-50 and +-200 bp and for two
    single-tenor bumps (5Y +25 bp, 3M -10 bp) of the README GBP curve's par rates.  The bootstrap does not depend on the
    interpolation scheme."""
    curve = curve or F.gbp_model(VD).curves.GBP_OIS_SONIA
    rates = np.array(curve.swap_rates, dtype=np.float64)
    rows = [rates + s * BP for s in (1, -1, 50, -50, 200, -200)]
    for tenor, s in (("5Y", 25), ("3M", -10)):
        bumped = rates.copy()
        bumped[F.TENORS.index(tenor)] += s * BP
        rows.append(bumped)
    built = [build_engine_curve(list(r), curve.swap_times, curve.year_fracs, with_hessian=False) for r in rows]
    return built[0].times, np.stack([b.dfs for b in built])


def lag_book(n=200, seed=21, weighted=False):
    """Annual / semi-annual OIS, a third with a two-day payment lag, some with a spread; ``weighted``: per-coupon
    notional multipliers as the cross-currency assembly produces them."""
    rng = np.random.default_rng(seed)
    terms = OISTerms(effective_dt=VD, tenor=[f"{int(m)}M" for m in rng.integers(1, 481, n)],
                     coupon=rng.uniform(0.01, 0.07, n), notional=np.round(rng.uniform(1e6, 5e7, n), -5),
                     pay_fixed=rng.random(n) < 0.5, fixed_freq_type=FrequencyTypes.ANNUAL, fixed_dc_type=DayCountTypes.ACT_365F,
                     floating_index=CurveTypes.GBP_OIS_SONIA, currency=CurrencyTypes.GBP,
                     float_freq_type=[[FrequencyTypes.ANNUAL, FrequencyTypes.SEMI_ANNUAL][i] for i in rng.integers(0, 2, n)],
                     float_dc_type=DayCountTypes.ACT_365F, float_spread=np.where(rng.random(n) < 0.3, 0.0015, 0.0),
                     payment_lag=rng.choice([0, 0, 2], size=n), bd_type=BusDayAdjustTypes.MODIFIED_FOLLOWING)
    batch = compile_ois_terms(terms, VD)
    if weighted:
        batch.flt_weight = rng.uniform(0.5, 1.5, batch.flt_tp.shape[0])
    return batch


def long_leg_book():
    """Three hand-made trades: monthly legs of 400 and 450 coupons (beyond the 390 of the row tables), the second with
    a payment lag and accrual periods that do not abut, and an ordinary 3-coupon trade between them."""
    def trade(m, lag, gap):
        ts = np.arange(m) / 12.0 + 0.01 + gap * np.arange(m)
        te = ts + 1.0 / 12.0
        return dict(fix_tp=te + lag, fix_pay=np.full(m, 2500.0), flt_tp=te + lag, flt_ts=ts, flt_te=te,
                    flt_alpha=np.full(m, 1.0 / 12.0))
    parts = [trade(400, 0.0, 0.0), trade(3, 0.0, 0.0), trade(450, 2.0 / 365.0, 1e-3)]
    cat = lambda k: np.concatenate([p[k] for p in parts])
    off = np.cumsum([0] + [p["fix_tp"].size for p in parts]).astype(np.int64)
    return TradeBatch(off, off.copy(), cat("fix_tp"), cat("fix_pay"), cat("flt_tp"), cat("flt_ts"), cat("flt_te"),
                      cat("flt_alpha"), np.array([1e6, 2e6, 3e6]), np.array([0.0, 0.001, 0.002]),
                      np.array([-1.0, 1.0, -1.0]), np.array([1.0, -1.0, 1.0]))


def books():
    """name -> batch: the cases of the issue's check 1."""
    bonds, _ = F.random_bond_book(VD, 50, seed=5)
    frns, _ = F.random_frn_book(VD, 50, seed=6)
    return {
        "300 mixed OIS": _concat_batches([synthetic.synthesize(VD, 150, kind="offgrid", seed=3),
                                          synthetic.synthesize(VD, 150, kind="ongrid", seed=4)]),
        "payment lag": lag_book(),
        "weighted": lag_book(120, seed=22, weighted=True),
        "50 bonds": compile_bonds(bonds, VD),
        "50 FRNs": compile_frns(frns, VD)[0],
        "long legs": long_leg_book(),
    }


def oracle_pv(method, times, dfs, batch):
    """``[S, n]``: the C oracle's PV, one call per scenario, no derivatives (a zero Jacobian of the right shape)."""
    zero = np.zeros((np.asarray(times).size, 1))
    return np.stack([port.price(method, times, row, zero, None, batch, want_delta=False, want_gamma=False)["pv"]
                     for row in np.atleast_2d(dfs)])


def worst_unit_err(got, ref, batch):
    """The project's parity metric over all scenarios: max |a - b| / max(1, |b|) per unit notional."""
    return max(unit_notional_err(g, r, batch.notional) for g, r in zip(got, ref))


def book_sum(pv_sn, chunk=64):
    """The documented order of book_pv on rows ``pv [S, n]``: chunks of 64 trades summed in trade order from 0.0, chunk
    j added to slot j % 64 in order, then a halving tree over the 64 slots."""
    S, n = pv_sn.shape
    out = np.empty(S)
    for s in range(S):
        chunks = []
        for lo in range(0, n, chunk):
            acc = 0.0
            for v in pv_sn[s, lo:lo + chunk]:
                acc = acc + float(v)
            chunks.append(acc)
        slots = [0.0] * 64
        for j, v in enumerate(chunks):
            slots[j % 64] = slots[j % 64] + v
        h = 32
        while h >= 1:
            for cl in range(h):
                slots[cl] = slots[cl] + slots[cl + h]
            h //= 2
        out[s] = slots[0]
    return out


# knots with a duplicated time, and the dates that exercise simple_interpolate's lookup rule on them
LOOKUP_TIMES = np.array([0.0, 0.5, 1.0, 1.0, 2.0, 5.0])
LOOKUP_TIMES_LATE = np.array([0.25, 0.5, 1.0, 1.0, 2.0, 5.0])          # first knot after the value time
LOOKUP_DATES = np.array([0.5, 0.5 + 1e-11, 2.0 - 1e-11, 1.0, 1.0 + 1e-9, 1.0 - 1e-9, 0.1, 0.2499, 5.0, 7.0, 40.0, 0.75, 3.3])


def lookup_curves(times, S=3, seed=9):
    rng = np.random.default_rng(seed)
    zero = rng.uniform(0.01, 0.06, size=(S, times.size))
    dfs = np.exp(-zero * np.maximum(times, 0.0)[None, :])
    dfs[:, 3] = dfs[:, 2] * 0.999                  # the duplicated knot carries another value: the first one wins
    return dfs


def one_flow_book(dates):
    """A unit fixed flow per date: pv = D(date)."""
    n = dates.size
    off = np.arange(n + 1, dtype=np.int64)
    e = np.zeros(0)
    return TradeBatch(off, np.zeros(n + 1, dtype=np.int64), dates.copy(), np.ones(n), e, e.copy(), e.copy(), e.copy(),
                      np.ones(n), np.zeros(n), np.ones(n), np.ones(n))


def one_coupon_book(ts, te, tp):
    """A float coupon per row with alpha = 1, spread 0.01, notional 1: pv = ((D(ts) / D(te) - 1) + 0.01) D(tp)."""
    n = ts.size
    off = np.arange(n + 1, dtype=np.int64)
    e = np.zeros(0)
    return TradeBatch(np.zeros(n + 1, dtype=np.int64), off, e, e.copy(), tp.copy(), ts.copy(), te.copy(), np.ones(n),
                      np.ones(n), np.full(n, 0.01), np.ones(n), np.ones(n))
