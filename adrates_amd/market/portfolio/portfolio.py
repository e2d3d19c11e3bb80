"""Portfolio of positions (cavour/market/portfolio/portfolio.py:8-66).

The reference prices position by position in a Python loop and adds the result
objects; here positions that share a curve go to the GPU as one batch and the
sums are formed on the device (per-block partials, fixed-order final sum).
Mixed portfolios fall back to combining the per-curve aggregates with the same
``+`` the reference uses, so mismatched curves/currencies raise as they do there.
"""
from typing import Iterable, List

from ...requests.results import AnalyticsResult
from ...utils.global_types import InstrumentTypes, RequestTypes
from ..position.engine import (Engine, bond_curve_type, frn_is_single_curve, is_bond, is_frn, price_batch, price_bonds,
                               price_frns, wrap_result)
from ..position.position import Position
from ..position.sub_book_ladders import price_sub_books


class Portfolio:
    def __init__(self, positions: Iterable[Position] | None = None) -> None:
        self._positions: List[Position] = list(positions or [])

    def add_position(self, position: Position) -> None:
        self._positions.append(position)

    def positions(self) -> List[Position]:
        return list(self._positions)

    def compute(self, request_list: Iterable[RequestTypes]) -> AnalyticsResult:
        """Aggregate VALUE / DELTA / GAMMA over all positions."""
        reqs = set(request_list)
        groups = {}   # (model id, curve, currency, OIS_SWAP, BOND or FRN) -> positions, in first-seen order
        singles = []  # everything else (dual-curve FRNs among them): priced one by one and added with `+`, as the reference does
        for pos in self._positions:
            d = pos.derivative
            if d.derivative_type == InstrumentTypes.BOND and is_bond(d):
                # bonds of one model and currency: one fixed-flows-only launch on that currency's OIS curve
                key = (id(pos.model), bond_curve_type(d), d._currency, InstrumentTypes.BOND)
                groups.setdefault(key, []).append(pos)
                continue
            if d.derivative_type == InstrumentTypes.FRN and is_frn(d) and frn_is_single_curve(d):
                # single-curve FRNs of one model and currency: one float-leg launch on that currency's OIS curve
                key = (id(pos.model), bond_curve_type(d), d._currency, InstrumentTypes.FRN)
                groups.setdefault(key, []).append(pos)
                continue
            if d.derivative_type != InstrumentTypes.OIS_SWAP:
                singles.append(pos)
                continue
            key = (id(pos.model), d._floating_index, d._currency, InstrumentTypes.OIS_SWAP)
            groups.setdefault(key, []).append(pos)

        total_val = total_delta = total_gamma = None
        for pos in singles:
            # cross-currency swaps return `Risk` containers, which have no `+` in the reference either
            # (requests/results.py:839-942): two of them with DELTA / GAMMA raise TypeError there and here;
            # books of XCCY swaps go through xccy_engine.price_xccy_batch(aggregate=True) instead
            res = pos.compute(request_list)
            if RequestTypes.VALUE in reqs:
                total_val = res.value if total_val is None else total_val + res.value
            if RequestTypes.DELTA in reqs:
                total_delta = res.risk if total_delta is None else total_delta + res.risk
            if RequestTypes.GAMMA in reqs:
                total_gamma = res.gamma if total_gamma is None else total_gamma + res.gamma
        for (_, curve_type, currency, kind), members in groups.items():
            model = members[0].model
            ir_model = getattr(model.curves, curve_type.name)
            engine = members[0]._engine
            pricer = {InstrumentTypes.BOND: price_bonds, InstrumentTypes.FRN: price_frns}.get(kind, price_batch)
            res = pricer(engine, ir_model, [p.derivative for p in members], reqs, per_trade=False, aggregate=True)
            part = wrap_result(res, 0, reqs, res["tenors"], currency, curve_type, aggregate=True)
            if RequestTypes.VALUE in reqs:
                total_val = part.value if total_val is None else total_val + part.value
            if RequestTypes.DELTA in reqs:
                total_delta = part.risk if total_delta is None else total_delta + part.risk
            if RequestTypes.GAMMA in reqs:
                total_gamma = part.gamma if total_gamma is None else total_gamma + part.gamma
        return AnalyticsResult(value=total_val, risk=total_delta, gamma=total_gamma)

    def compute_sub_books(self, request_list: Iterable[RequestTypes], keys) -> dict:
        """`compute` per sub-book: ``keys`` holds one hashable key per position, and the result is ``{"labels": [...],
        "results": [AnalyticsResult, ...]}`` with the labels in order of first appearance.

        Positions are grouped by (model, curve, currency) as `compute` groups them, and each group is ONE launch
        (`price_sub_books`); a desk's results are combined across groups with the `+` `compute` uses, so mismatched
        curves raise as they do there.  A position `compute` prices on its own (cross-currency swaps, dual-curve FRNs,
        YoY swaps) is refused with a `ValueError` naming the first of them."""
        reqs = set(request_list)
        keys = list(keys)
        if len(keys) != len(self._positions):
            raise ValueError(f"keys needs one entry per position ({len(self._positions)}), not {len(keys)}")
        labels = list(dict.fromkeys(keys))
        groups = {}   # (model id, curve, currency) -> (positions, their keys), in first-seen order
        for i, (pos, key) in enumerate(zip(self._positions, keys)):
            d = pos.derivative
            kind = d.derivative_type
            if kind == InstrumentTypes.BOND and is_bond(d):
                curve_type = bond_curve_type(d)
            elif kind == InstrumentTypes.FRN and is_frn(d) and frn_is_single_curve(d):
                curve_type = bond_curve_type(d)
            elif kind == InstrumentTypes.OIS_SWAP:
                curve_type = d._floating_index
            else:
                raise ValueError(f"position {i} ({type(d).__name__}) is priced on its own by compute and has no place in a "
                                 "sub-book launch")
            members = groups.setdefault((id(pos.model), curve_type, d._currency), ([], []))
            members[0].append(pos)
            members[1].append(key)
        totals = {label: [None, None, None] for label in labels}
        for (_, curve_type, currency), (members, member_keys) in groups.items():
            ir_model = getattr(members[0].model.curves, curve_type.name)
            res = price_sub_books(members[0]._engine, ir_model, [p.derivative for p in members], member_keys, reqs,
                                  curve_type=curve_type)
            for b, label in enumerate(res["labels"]):
                row = {"agg_pv": res["pv"][b], "agg_delta": res["delta"][b], "agg_gamma": res["gamma"][b]}
                part = wrap_result(row, 0, reqs, res["tenors"], currency, curve_type, aggregate=True)
                tot = totals[label]
                for j, (want, piece) in enumerate(((RequestTypes.VALUE, part.value), (RequestTypes.DELTA, part.risk),
                                                   (RequestTypes.GAMMA, part.gamma))):
                    if want in reqs:
                        tot[j] = piece if tot[j] is None else tot[j] + piece
        return {"labels": labels, "results": [AnalyticsResult(value=v, risk=d, gamma=g) for v, d, g in
                                              (totals[label] for label in labels)]}
