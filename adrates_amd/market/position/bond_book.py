"""A book of bonds on one currency's OIS curve: batched spread / yield measures and curve Greeks.

`BondBook.measures` is `Bond.z_spread`, `dirty_price`, `clean_price`, `yield_to_maturity`, `duration`,
`convexity` and `dv01` (= `cs01`) for every bond at once, in one launch of the adr_bond_measures kernel
(csrc/bond_measures.hip) on the curve's OWN node set - the same nodes `DiscountCurve.df` reads.
`BondBook.compute` is the engine's VALUE / DELTA / GAMMA for every bond in one fixed-flows-only batch.

The per-bond arrays are compiled on the host: per flow paid after settlement its curve time (ACT/ACT ISDA from
the curve's value date, as `DiscountCurve.df`), its spread time (days from settlement / 365.25, as the bond's
spread and yield methods), coupon and principal; per bond the curve time of settlement, the spread time of the
UNADJUSTED maturity, the face and the accrued interest per 100.
"""
from __future__ import annotations

from typing import Iterable

import numpy as np

from ... import _native
from ...trades.credit.bond import SPREAD_DAYS_IN_YEAR, Bond
from ...utils.day_count import DayCount, DayCountTypes
from ...utils.error import LibError
from ...utils.global_types import InterpTypes, RequestTypes
from .engine import Engine, bond_curve_type, price_bonds

_NODE_INTERP = (InterpTypes.FLAT_FWD_RATES, InterpTypes.LINEAR_FWD_RATES, InterpTypes.LINEAR_ZERO_RATES)


def compile_bond_measures(bonds, curve, settlement_dt) -> dict:
    """Inputs of adr_bond_measures for ``bonds`` settling on ``settlement_dt`` against ``curve``'s own nodes:
    ``flow_off`` and the fields of `_native.BOND_FLOW_FIELDS` / `_native.BOND_FIELDS` except the quote."""
    act = DayCount(DayCountTypes.ACT_ACT_ISDA)
    curve_time = lambda dt: act.year_frac(curve._value_dt, dt)[0]
    off, T, tau, cpn, prin = [0], [], [], [], []
    Ts, tauM, face, acc = [], [], [], []
    ts = curve_time(settlement_dt)
    for b in bonds:
        for i, dt in enumerate(b._payment_dts):
            if dt > settlement_dt:                      # flows on or before settlement are not paid
                T.append(curve_time(dt))
                tau.append((dt - settlement_dt) / SPREAD_DAYS_IN_YEAR)
                cpn.append(float(b._coupon_payments[i]))
                prin.append(float(b._principal_payments[i]))
        off.append(len(T))
        Ts.append(ts)
        tauM.append((b._maturity_dt - settlement_dt) / SPREAD_DAYS_IN_YEAR)   # <= 0: matured, no face in the yield
        face.append(float(b._face_value))
        acc.append(b._accrued_per_100(settlement_dt))
    f64 = lambda a: np.array(a, dtype=np.float64)
    return {"flow_off": np.array(off, dtype=np.int64), "flow_T": f64(T), "flow_tau": f64(tau), "flow_cpn": f64(cpn),
            "flow_prin": f64(prin), "bond_Ts": f64(Ts), "bond_tauM": f64(tauM), "bond_face": f64(face),
            "bond_acc100": f64(acc)}


def tile_bond_measures(book: dict, reps: int) -> dict:
    """``reps`` copies of a compiled book (`compile_bond_measures` output, with or without ``bond_quote``), one after
    another - a large book from a few distinct bonds, for benchmarks and scale tests."""
    off = np.asarray(book["flow_off"], dtype=np.int64)
    counts = np.tile(off[1:] - off[:-1], reps)
    out = {"flow_off": np.concatenate(([0], np.cumsum(counts))).astype(np.int64)}
    for k in _native.BOND_FLOW_FIELDS + _native.BOND_FIELDS:
        if k in book:
            out[k] = np.tile(np.asarray(book[k], dtype=np.float64), reps)
    return out


class BondBook:
    """Bonds of ONE currency priced together against ``model``'s OIS curve for that currency."""

    def __init__(self, bonds: Iterable[Bond], model, settlement_dt=None):
        self.bonds = list(bonds)
        if not self.bonds:
            raise LibError("BondBook needs at least one bond")
        for b in self.bonds:
            if not isinstance(b, Bond):
                raise LibError(f"BondBook takes Bond objects, not {type(b).__name__}")
        currencies = {b._currency for b in self.bonds}
        if len(currencies) != 1:
            raise LibError("BondBook holds bonds of one currency; make one book per currency")
        self.model = model
        self.curve_type = bond_curve_type(self.bonds[0])
        self.currency = self.bonds[0]._currency
        self.curve = getattr(model.curves, self.curve_type.name)
        if self.curve._interp_type not in _NODE_INTERP:
            raise LibError("Invalid interpolation scheme.")
        self.settlement_dt = self.curve._value_dt if settlement_dt is None else settlement_dt
        self._arrays = None
        self._engine = Engine(model)

    def __len__(self):
        return len(self.bonds)

    @property
    def arrays(self) -> dict:
        """The compiled per-flow / per-bond inputs (without quotes); built once."""
        if self._arrays is None:
            self._arrays = compile_bond_measures(self.bonds, self.curve, self.settlement_dt)
        return self._arrays

    def inputs(self, clean_prices=None, z_spreads=None):
        """``(interp method, node times, node dfs, book arrays with bond_quote, quote_is_z)`` for adr_bond_measures."""
        if (clean_prices is None) == (z_spreads is None):
            raise LibError("give exactly one of clean_prices and z_spreads")
        quote = clean_prices if z_spreads is None else z_spreads
        book = dict(self.arrays)
        book["bond_quote"] = np.broadcast_to(np.asarray(quote, dtype=np.float64), (len(self.bonds),)).copy()
        return (self.curve._interp_type.value, np.asarray(self.curve._times, dtype=np.float64),
                np.asarray(self.curve._dfs, dtype=np.float64), book, z_spreads is not None)

    def measures(self, clean_prices=None, z_spreads=None, ctx=None) -> dict:
        """Per-bond arrays ``z``, ``dirty``, ``clean``, ``ytm``, ``duration`` (Macaulay), ``convexity``, ``dv01`` (= cs01)
        and ``status`` in one launch.  With ``clean_prices`` (per 100 face) z is solved; with ``z_spreads`` it is
        given.  status 0: solved inside the bracket; 1: by the fallback; 2: no root - the dependent outputs are NaN
        where the scalar `Bond` methods raise."""
        method, node_t, node_df, book, is_z = self.inputs(clean_prices, z_spreads)
        return _native.bond_measures(ctx or _native.default_context(), method, node_t, node_df, book, is_z)

    def compute(self, request_list, per_trade=True, aggregate=False) -> dict:
        """VALUE / DELTA / GAMMA of every bond (``pv``, ``delta``, ``gamma``) and / or of the book (``agg_pv``,
        ``agg_delta``, ``agg_gamma``) in one batch, as `_native.price` returns them, plus ``tenors``."""
        reqs = set(request_list)
        if not reqs & {RequestTypes.VALUE, RequestTypes.DELTA, RequestTypes.GAMMA}:
            raise LibError("BondBook.compute needs VALUE, DELTA or GAMMA")
        out = price_bonds(self._engine, self.curve, self.bonds, reqs, per_trade=per_trade, aggregate=aggregate)
        out["curve_type"], out["currency"] = self.curve_type, self.currency
        return out

    def revalue(self, grid, z_spreads, buckets=None, spread_shocks=None, per_trade=False) -> dict:
        """The book's PV at the z-spreads ``z_spreads`` (one per bond, e.g. ``measures(...)["z"]``) under every
        scenario of ``grid``, a `ScenarioGrid` of this book's curve, paired with ``spread_shocks``:
        `ScenarioGrid.revalue_credit`."""
        return grid.revalue_credit(self.bonds, z_spreads, buckets=buckets, spread_shocks=spread_shocks, per_trade=per_trade)
