"""Torch restatement of the reference's single-curve FRN engine (`pv_fn_combined`, cavour/market/position/engine.py:
700-880): `_float_leg_jax` with the first-fixing override on coupon 0 of the whole schedule, plus the face at the
adjusted maturity under a strict ``>`` mask, differentiated by `_leg_analytics`.  Test infrastructure only."""
import numpy as np
import torch

from adrates_amd.utils.helpers import times_from_dates
from oracle import cavour_oracle as O


def frn_pv_fn(frn, cache, method, value_dt):
    """``d -> PV`` over the engine's knot discount factors."""
    times = cache["times"]
    dc = frn._dc_type
    tp = np.array([times_from_dates(d, value_dt, dc) for d in frn._payment_dts], dtype=np.float64)
    ts = np.array([times_from_dates(d, value_dt, dc) for d in frn._start_accrued_dts], dtype=np.float64)
    te = np.array([times_from_dates(d, value_dt, dc) for d in frn._end_accrued_dts], dtype=np.float64)
    al = np.array(frn._year_fracs, dtype=np.float64)
    tm = times_from_dates(frn._maturity_dt, value_dt, dc)
    face, margin, ffr = frn._face_value, frn._quoted_margin, frn._first_fixing_rate
    k0 = 0 if ffr is None else 1                       # the override replaces coupon 0's forward

    def pv(d):
        total = torch.zeros((), dtype=torch.float64)
        if k0 < tp.size:
            m = tp.size - k0
            total = total + O.float_leg(d, times, method, tp[k0:], ts[k0:], te[k0:], al[k0:], np.full(m, margin),
                                        np.full(m, face), 0.0, 1.0)
        if ffr is not None and tp[0] >= 0.0:
            rel = O.simple_interpolate(tp[0], times, d, method) / O.simple_interpolate(0.0, times, d, method)
            total = total + (ffr + margin) * al[0] * face * rel
        # the principal: price_fixed_leg's mask is the engine's `maturity_time > value_time`
        return total + O.price_fixed_leg(d, times, method, [tm], [0.0], face, 1.0)
    return pv


def frn_analytics(frn, curve, want_gamma=True):
    """VALUE, DELTA and GAMMA of a single-curve FRN on ``curve`` (an OIS curve of the model)."""
    cache = O.cached_curve(curve.swap_rates, curve.swap_times, curve.year_fracs)
    return O._leg_analytics(frn_pv_fn(frn, cache, curve._interp_type.value, curve._value_dt), cache, want_gamma)
