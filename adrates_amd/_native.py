"""ctypes binding of libadrates_hip.so (C-ABI: include/adrates.h).

There is deliberately no CPU fallback: if the shared library has not been built
or no HIP device is usable, every pricing entry point raises.  Build the library
with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C adrates_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .utils.error import LibError

# ADRATES_HIP_LIB lets a tuning run point at an alternative build of the same library
_LIB_PATH = os.environ.get("ADRATES_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                               "libadrates_hip.so")
_lib = None

REQ_VALUE, REQ_DELTA, REQ_GAMMA = 1, 2, 4
SCHEDULE_GROUPS_AUTO, SCHEDULE_GROUPS_OFF, SCHEDULE_GROUPS_FORCE = 0, 1, 2      # adr_trades_set_schedule_groups
ADR_ERR_UNSUPPORTED = -2     # a `LibError` raised by `_check` carries the library's code as ``status``
MAX_PILLARS = 256            # ADR_MAX_PILLARS (uploaded curves); the device curve builder: 64

_dp = C.POINTER(C.c_double)
_i64p = C.POINTER(C.c_int64)
_i32p = C.POINTER(C.c_int32)
_vp = C.c_void_p

_SIGNATURES = {
    "adr_version": (C.c_int, []),
    "adr_last_error": (C.c_char_p, []),
    "adr_device_count": (C.c_int, []),
    "adr_init": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "adr_free_ctx": (None, [_vp]),
    "adr_sync": (C.c_int, [_vp]),
    "adr_curve_upload": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.POINTER(_vp)]),
    "adr_curve_upload_ex": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_uint32, C.POINTER(_vp)]),
    "adr_free_curve": (None, [_vp]),
    "adr_curve_pillars": (C.c_int, [_vp]),
    "adr_curve_tables_host": (C.c_int, [C.c_int, C.c_int, _dp, _dp, _dp, _dp, _i32p, _dp, _dp, _dp]),
    "adr_curve_layout_host": (C.c_int, [C.c_int, C.c_int, _dp, _dp, _dp, _dp, _i64p]),
    "adr_curve_plan_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _dp, _dp, _i32p, _i32p, _dp, _dp, _dp,
                                        C.POINTER(_vp)]),
    "adr_free_curve_plan": (None, [_vp]),
    "adr_curve_set_build": (C.c_int, [_vp, _vp, C.c_int, _dp, C.POINTER(_vp)]),
    "adr_curve_set_size": (C.c_int, [_vp]),
    "adr_curve_set_get": (_vp, [_vp, C.c_int]),
    "adr_curve_set_download": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp]),
    "adr_free_curve_set": (None, [_vp]),
    "adr_trades_upload": (C.c_int, [_vp, C.c_int64, _i64p, _i64p, _dp, _dp, _dp, _dp, _dp, _dp,
                                    _dp, _dp, _dp, _dp, C.POINTER(_vp)]),
    "adr_trades_upload_weighted": (C.c_int, [_vp, C.c_int64, _i64p, _i64p, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                             _dp, _dp, _dp, _dp, C.POINTER(_vp)]),
    "adr_free_trades": (None, [_vp]),
    "adr_trades_count": (C.c_int64, [_vp]),
    "adr_trades_input_bytes": (C.c_int64, [_vp]),
    "adr_trades_set_schedule_groups": (C.c_int, [_vp, C.c_int]),
    "adr_trades_set_schedule_segment": (C.c_int, [_vp, C.c_int, C.c_int]),
    "adr_trades_schedule_groups_info": (C.c_int, [_vp, _i64p]),
    "adr_schedule_groups_host": (C.c_int, [C.c_int64, _i64p, _i64p] + [_dp] * 11 + [_i32p, _dp, _dp, _i64p, _i64p] + [_dp] * 8),
    "adr_price": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _dp, _dp, _dp, _dp]),
    "adr_price_dev": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp]),
    "adr_allreduce_agg": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp]),
    "adr_price_xccy_foreign": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _dp, _dp, _dp, _dp, _dp]),
    "adr_price_xccy_foreign_dev": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "adr_route_host": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_uint32, C.c_int64, _i64p, _i64p, _dp, _dp, _dp, _dp,
                                 C.c_uint32, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int]),
    "adr_rccl_unique_id": (C.c_int, [_vp]),
    "adr_rccl_comm_init": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.POINTER(_vp)]),
    "adr_rccl_comm_destroy": (None, [_vp]),
    "adr_curve_df": (C.c_int, [_vp, _vp, C.c_int64, _dp, _dp]),
    "adr_curve_df_dev": (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, _vp]),
    "adr_leg_counts_host": (C.c_int, [C.c_int64, _i64p, _i64p, _i64p, _i64p]),
    "adr_leg_times_host": (C.c_int, [C.c_int64, _i64p, _i64p, _i64p, _i64p, C.c_int, C.c_int, _dp, C.c_int64, C.c_double,
                                     _i64p, _dp, _dp, _dp, _dp, C.POINTER(C.c_uint8)]),
    "adr_exchange_flows_host": (C.c_int, [C.c_int64, _dp, _dp, C.POINTER(C.c_uint8), _dp, C.c_double, _i64p, _dp, _dp, _dp]),
    "adr_xccy_assemble_host": (C.c_int, [C.c_int64, _i64p, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.c_double, _dp,
                                         C.POINTER(C.c_uint8), _i64p, _dp, _dp, _dp, _dp, _i64p, _dp, _dp, _dp]),
    "adr_bond_measures": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, C.c_int64, _i64p, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                    _dp, C.c_int, _dp, _i32p]),
    "adr_bond_measures_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                        _vp, _vp, C.c_int, _vp, _vp, _vp]),
    "adr_bond_measures_host": (C.c_int, [C.c_int, C.c_int, _dp, _dp, C.c_int64, _i64p, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                         _dp, C.c_int, _dp, _i32p]),
    "adr_frn_measures": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int64, C.c_int64, _i64p,
                                   _dp, _dp, C.c_int, _dp, _i32p]),
    "adr_frn_measures_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, _vp, C.c_int64, C.c_int64, _vp,
                                       _vp, _vp, C.c_int, _vp, _vp, _vp]),
    "adr_frn_measures_host": (C.c_int, [C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int64, C.c_int64, _i64p,
                                        _dp, _dp, C.c_int, _dp, _i32p]),
    "adr_yoy_risk": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int64, C.c_int64, _i64p, _dp,
                               C.c_uint32, _dp, _dp, _dp, _dp, _dp]),
    "adr_yoy_risk_work": (C.c_int64, [C.c_int64, C.c_int]),
    "adr_yoy_risk_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, _vp, C.c_int64, C.c_int64, _vp, _vp,
                                   C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "adr_yoy_risk_host": (C.c_int, [C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int64, C.c_int64, _i64p, _dp,
                                    C.c_uint32, _dp, _dp, _dp, _dp, _dp]),
    "adr_scenario_pv": (C.c_int, [_vp, C.c_int, C.c_int, _dp, C.c_int, _dp, _vp, _dp, _dp]),
    "adr_scenario_pv_work": (C.c_int64, [C.c_int64, C.c_int]),
    "adr_scenario_pv_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "adr_scenario_pv_set": (C.c_int, [_vp, _vp, _vp, _dp, _dp]),
    "adr_curve_set_arrays": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_vp),
                                       C.POINTER(_vp)]),
    "adr_scenario_pv_host": (C.c_int, [C.c_int, C.c_int, _dp, C.c_int, _dp, C.c_int64, _i64p, _i64p] + [_dp] * 11 +
                             [_dp, _dp, C.c_int]),
    "adr_yoy_scenario_pv": (C.c_int, [_vp, C.c_int, C.c_int, _dp, C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, _dp, C.c_int,
                                      C.c_int64, C.c_int64, _i64p, _dp, _dp, C.c_int64, _i64p, _dp, _dp, _dp]),
    "adr_yoy_scenario_pv_work": (C.c_int64, [C.c_int64, C.c_int]),
    "adr_yoy_scenario_pv_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int,
                                          C.c_int64, C.c_int64, _vp, _vp, _vp, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "adr_yoy_scenario_pv_host": (C.c_int, [C.c_int, C.c_int, _dp, C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, _dp, C.c_int,
                                           C.c_int64, C.c_int64, _i64p, _dp, _dp, C.c_int64, _i64p, _dp, _dp, _dp, C.c_int]),
    "adr_xccy_scenario_pv": (C.c_int, [_vp] + [C.c_int, C.c_int, _dp, C.c_int, _dp] * 2 + [C.c_int, _vp, _dp, _dp]),
    "adr_xccy_scenario_pv_work": (C.c_int64, [C.c_int64, C.c_int]),
    "adr_xccy_scenario_pv_dev": (C.c_int, [_vp] + [C.c_int, C.c_int, _vp, C.c_int, _vp] * 2 + [C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "adr_xccy_scenario_pv_host": (C.c_int, [C.c_int, C.c_int, _dp, C.c_int, _dp] * 2 + [C.c_int, C.c_int64, _i64p, _i64p] +
                                  [_dp] * 11 + [_dp, _dp, C.c_int]),
    "adr_xccy_scenario_subbook_pv": (C.c_int, [_vp] + [C.c_int, C.c_int, _dp, C.c_int, _dp] * 2 +
                                     [C.c_int, _vp, C.c_int64, _i64p, _dp, _dp]),
    "adr_xccy_scenario_subbook_pv_dev": (C.c_int, [_vp] + [C.c_int, C.c_int, _vp, C.c_int, _vp] * 2 +
                                         [C.c_int, _vp, C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    "adr_xccy_scenario_subbook_pv_host": (C.c_int, [C.c_int, C.c_int, _dp, C.c_int, _dp] * 2 + [C.c_int, C.c_int64, _i64p, _i64p] +
                                          [_dp] * 11 + [C.c_int64, _i64p, _dp, _dp, C.c_int]),
    "adr_credit_scenario_pv": (C.c_int, [_vp, C.c_int, C.c_int, _dp, C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, _vp, _dp,
                                         _i32p, C.c_int64, _dp, C.c_int64, _dp, _dp, _dp]),
    "adr_credit_scenario_pv_set": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _dp, _vp, _dp, _i32p, C.c_int64, _dp, C.c_int64, _dp,
                                             _dp, _dp]),
    "adr_credit_scenario_pv_work": (C.c_int64, [C.c_int64, C.c_int]),
    "adr_credit_scenario_pv_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp,
                                             _vp, C.c_int64, _vp, C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    "adr_credit_scenario_pv_host": (C.c_int, [C.c_int, C.c_int, _dp, C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, C.c_int64,
                                              _i64p, _i64p] + [_dp] * 11 + [_dp, _i32p, _dp, _dp, _dp, _dp, C.c_int]),
    "adr_scenario_subbook_plan": (C.c_int64, [C.c_int64, C.c_int64, _i64p, _i64p]),
    "adr_scenario_subbook_work": (C.c_int64, [C.c_int64, C.c_int64, C.c_int]),
    "adr_scenario_subbook_pv": (C.c_int, [_vp, C.c_int, C.c_int, _dp, C.c_int, _dp, _vp, C.c_int64, _i64p, _dp, _dp]),
    "adr_scenario_subbook_pv_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    "adr_scenario_subbook_pv_set": (C.c_int, [_vp, _vp, _vp, C.c_int64, _i64p, _dp, _dp]),
    "adr_scenario_subbook_pv_host": (C.c_int, [C.c_int, C.c_int, _dp, C.c_int, _dp, C.c_int64, _i64p, _i64p] + [_dp] * 11 +
                                     [C.c_int64, _i64p, _dp, _dp, C.c_int]),
    "adr_scenario_subbook_var_es": (C.c_int, [_vp, C.c_int, C.c_int, _dp, C.c_int, _dp, _vp, C.c_int64, _i64p, C.c_int, C.c_int,
                                              _dp, _dp]),
    "adr_credit_scenario_subbook_pv": (C.c_int, [_vp, C.c_int, C.c_int, _dp, C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, _vp,
                                                 _dp, _i32p, C.c_int64, _dp, C.c_int64, _dp, C.c_int64, _i64p, _dp, _dp]),
    "adr_credit_scenario_subbook_pv_set": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _dp, _vp, _dp, _i32p, C.c_int64, _dp, C.c_int64,
                                                     _dp, C.c_int64, _i64p, _dp, _dp]),
    "adr_credit_scenario_subbook_pv_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int,
                                                     _vp, _vp, _vp, C.c_int64, _vp, C.c_int64, _vp, C.c_int64, _vp, _vp, _vp,
                                                     _vp, _vp]),
    "adr_credit_scenario_subbook_pv_host": (C.c_int, [C.c_int, C.c_int, _dp, C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int,
                                                      C.c_int64, _i64p, _i64p] + [_dp] * 11 +
                                            [_dp, _i32p, _dp, _dp, C.c_int64, _i64p, _dp, _dp, C.c_int]),
    "adr_scenario_tail": (C.c_int, [_vp, C.c_int64, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp]),
    "adr_scenario_tail_dev": (C.c_int, [_vp, C.c_int64, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "adr_scenario_tail_host": (C.c_int, [C.c_int64, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp]),
    "adr_yoy_scenario_subbook_pv": (C.c_int, [_vp, C.c_int, C.c_int, _dp, C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, _dp,
                                              C.c_int, C.c_int64, C.c_int64, _i64p, _dp, _dp, C.c_int64, _i64p, _dp, C.c_int64,
                                              _i64p, _dp, _dp]),
    "adr_yoy_scenario_subbook_pv_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp,
                                                  C.c_int, C.c_int64, C.c_int64, _vp, _vp, _vp, C.c_int64, _vp, _vp, C.c_int64,
                                                  _vp, _vp, _vp, _vp, _vp]),
    "adr_yoy_scenario_subbook_pv_host": (C.c_int, [C.c_int, C.c_int, _dp, C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, _dp,
                                                   C.c_int, C.c_int64, C.c_int64, _i64p, _dp, _dp, C.c_int64, _i64p, _dp,
                                                   C.c_int64, _i64p, _dp, _dp, C.c_int]),
    "adr_scenario_tail_alloc": (C.c_int, [_vp, C.c_int64, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp]),
    "adr_scenario_tail_alloc_dev": (C.c_int, [_vp, C.c_int64, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "adr_scenario_tail_alloc_host": (C.c_int, [C.c_int64, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp]),
    "adr_trades_ratio_flags_host": (C.c_int, [C.c_int64, _i64p, _dp, _dp, _dp, _dp, C.POINTER(C.c_uint8)]),
    "adr_subbook_ladders_work": (C.c_int64, [_vp, C.c_int64, C.c_int64, C.c_uint32, _i64p]),
    "adr_subbook_ladders": (C.c_int, [_vp, _vp, _vp, C.c_int64, _i64p, C.c_uint32, _dp]),
    "adr_subbook_ladders_dev": (C.c_int, [_vp, _vp, _vp, C.c_int64, _vp, C.c_uint32, _vp, _vp, _vp]),
    "adr_subbook_ladders_host": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int64, _i64p, _i64p] + [_dp] * 11 +
                                 [C.c_int64, _i64p, C.c_uint32, _dp]),
    "adr_credit_subbook_ladders_work": (C.c_int64, [_vp, C.c_int64, C.c_int64, C.c_int64, C.c_uint32, _i64p]),
    "adr_credit_subbook_ladders": (C.c_int, [_vp, _vp, _vp, _dp, _i32p, C.c_int64, _dp, C.c_int64, _dp, C.c_int, C.c_int64, _i64p,
                                             C.c_uint32, _dp]),
    "adr_credit_subbook_ladders_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int64, _vp, C.c_int64, _vp, C.c_int, C.c_int64,
                                                 C.c_int64, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp]),
    "adr_credit_subbook_ladders_host": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int64, _i64p, _i64p] +
                                        [_dp] * 11 + [_dp, _i32p, _dp, _dp, C.c_int, C.c_int64, _i64p, C.c_uint32, _dp]),
    "adr_yoy_subbook_ladders_work": (C.c_int64, [_vp, C.c_int, C.c_int64, C.c_int64, C.c_uint32, _i64p]),
    "adr_yoy_subbook_ladders": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _dp, _dp, C.c_int64, C.c_int64, _i64p, _dp, _dp, C.c_int64,
                                          _i64p, _dp, C.c_int64, _i64p, C.c_uint32, _dp]),
    "adr_yoy_subbook_ladders_dev": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, _vp, C.c_int64, C.c_int64, _vp, _vp, _vp, C.c_int64,
                                              _vp, _vp, C.c_int64, _vp, C.c_uint32, _vp, _vp, _vp]),
    "adr_yoy_subbook_ladders_host": (C.c_int, [C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int64,
                                               C.c_int64, _i64p, _dp, _dp, C.c_int64, _i64p, _dp, C.c_int64, _i64p, C.c_uint32, _dp]),
    "adr_ladder_pnl": (C.c_int, [_vp, C.c_int64, C.c_int, _dp, C.c_int, _dp, _dp, _dp, _dp]),
    "adr_ladder_pnl_dev": (C.c_int, [_vp, C.c_int64, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "adr_ladder_pnl_host": (C.c_int, [C.c_int64, C.c_int, _dp, C.c_int, _dp, _dp, _dp, _dp]),
    "adr_shock_normal": (C.c_int, [_vp, C.c_uint64, C.c_int64, C.c_int, C.c_int, C.c_int, _dp, C.c_int, _dp]),
    "adr_shock_normal_dev": (C.c_int, [_vp, C.c_uint64, C.c_int64, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp]),
    "adr_shock_normal_host": (C.c_int, [C.c_uint64, C.c_int64, C.c_int, C.c_int, C.c_int, _dp, C.c_int, _dp]),
    "adr_shock_words_host": (None, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "adr_shock_uniforms": (C.c_int, [_vp, C.c_uint64, C.c_int64, C.c_int, C.c_int, C.c_int, _dp]),
    "adr_shock_uniforms_host": (C.c_int, [C.c_uint64, C.c_int64, C.c_int, C.c_int, C.c_int, _dp]),
    "adr_scenario_tail_select": (C.c_int, [_vp, C.c_int64, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp]),
    "adr_scenario_tail_select_dev": (C.c_int, [_vp, C.c_int64, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "adr_scenario_tail_select_host": (C.c_int, [C.c_int64, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp]),
    "adr_scenario_tail_select_work": (C.c_int64, [C.c_int64, C.c_int, C.c_int]),
    "adr_scenario_tail_order": (C.c_int, [_vp, C.c_int64, C.c_int, _dp, C.c_int, C.c_int, _i64p, _dp, _dp]),
    "adr_scenario_tail_order_dev": (C.c_int, [_vp, C.c_int64, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "adr_scenario_tail_order_host": (C.c_int, [C.c_int64, C.c_int, _dp, C.c_int, C.c_int, _i64p, _dp, _dp]),
    "adr_scenario_tail_order_work": (C.c_int64, [C.c_int64, C.c_int, C.c_int]),
    "adr_scenario_tail_alloc_select": (C.c_int, [_vp, C.c_int64, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp]),
    "adr_scenario_tail_alloc_select_dev": (C.c_int, [_vp, C.c_int64, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "adr_scenario_tail_alloc_select_host": (C.c_int, [C.c_int64, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp]),
    "adr_scenario_tail_alloc_select_work": (C.c_int64, [C.c_int64, C.c_int, C.c_int]),
    "adr_scenario_total_dev": (C.c_int, [_vp, C.c_int64, C.c_int, _vp, C.c_int, _vp, _vp]),
    "adr_scenario_total_host": (C.c_int, [C.c_int64, C.c_int, _dp, C.c_int, _dp]),
    "adr_shock_gather_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, _vp]),
    "adr_shock_gather_host": (C.c_int, [C.c_int, C.c_int, _dp, C.c_int, _i64p, _dp]),
    "adr_tail_components_dev": (C.c_int, [_vp, C.c_int64, C.c_int, _vp, _vp, _vp, _vp]),
    "adr_tail_components_host": (C.c_int, [C.c_int64, C.c_int, _dp, _dp, _dp]),
    "adr_curve_dfs_shocked": (C.c_int, [_vp, _vp, _dp, C.c_int, C.c_int, _dp, _dp, _i32p]),
    "adr_curve_dfs_shocked_dev": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "adr_curve_dfs_shocked_work": (C.c_int64, [_vp, C.c_int]),
    "adr_curve_dfs_shocked_host": (C.c_int, [C.c_int, C.c_int, _dp, _i32p, _i32p, _dp, C.c_int, C.c_int, _dp, _dp, _i32p]),
    "adr_scenario_rows_place_dev": (C.c_int, [_vp, C.c_int64, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp]),
    "adr_shock_columns": (C.c_int, [_vp, C.c_int, C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, C.c_double, _dp, _i32p]),
    "adr_shock_columns_dev": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, C.c_double, _vp, _vp, _vp]),
    "adr_shock_columns_host": (C.c_int, [C.c_int, C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int, C.c_double, _dp, _i32p]),
    "adr_scenario_rows_merge_dev": (C.c_int, [_vp, C.c_int64, C.c_int, _vp, C.c_int64, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "adr_scenario_rows_merge_host": (C.c_int, [C.c_int64, C.c_int, _dp, C.c_int64, C.c_int, C.c_int, _dp, _i64p, _i32p]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def library_path() -> str:
    return _LIB_PATH


def load():
    """Load the shared library (no GPU needed for this step) and declare the
    argument types of every entry point."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise LibError(f"HIP extension not built: {_LIB_PATH} is missing "
                       "(run __graft_entry__.build() or make -C adrates_amd/csrc); "
                       "there is no CPU fallback for the pricing path")
    lib = C.CDLL(_LIB_PATH)
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def _check(rc: int, what: str):
    if rc < 0:
        msg = load().adr_last_error().decode("utf-8", "replace")
        raise LibError(f"{what} failed ({rc}): {msg}", status=rc)
    return rc


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a, typ=_dp):
    return None if a is None else a.ctypes.data_as(typ)


class Context:
    """One per GPU/process: owns the device selection, a stream and scratch."""

    def __init__(self, device: int = 0):
        lib = load()
        h = _vp()
        _check(lib.adr_init(int(device), C.byref(h)), "adr_init")
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            load().adr_free_ctx(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _check(load().adr_sync(self._h), "adr_sync")


class DeviceCurve:
    """Curve tables resident on the GPU (adr_curve_upload)."""

    PILLAR_TILES = 1      # ADR_CURVE_PILLAR_TILES (include/adrates.h)

    def __init__(self, ctx: Context, interp_method: int, times, dfs, jac, hess=None, flags: int = 0):
        times, dfs, jac = _f64(times), _f64(dfs), _f64(jac)
        K, P = jac.shape
        if times.shape != (K,) or dfs.shape != (K,):
            raise LibError("curve arrays have inconsistent shapes")
        hess_c = None
        if hess is not None:
            hess_c = _f64(hess)
            if hess_c.shape != (K, P, P):
                raise LibError("hess must have shape [K, P, P]")
        h = _vp()
        _check(load().adr_curve_upload_ex(ctx._h, int(interp_method), K, P, _ptr(times), _ptr(dfs), _ptr(jac),
                                          _ptr(hess_c), int(flags), C.byref(h)), "adr_curve_upload")
        self._h, self._ctx = h, ctx
        self.n_pillars, self.n_knots = P, K
        self.has_hess = hess is not None

    def close(self):
        if getattr(self, "_h", None):
            load().adr_free_curve(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CurvePlan:
    """Rate-independent half of a curve build (adr_curve_plan_create): the bootstrap scan of one knot grid
    and the table layout of its base curve.  ``host`` is an `EngineCurve` (curve_tables.build_engine_curve)."""

    def __init__(self, ctx: Context, interp_method: int, host):
        times, dfs, jac = _f64(host.times), _f64(host.dfs), _f64(host.jac)
        K, P = jac.shape
        acc = _f64(host.acc)
        pillar = np.ascontiguousarray(host.pillar, dtype=np.int32)
        prev_idx = np.ascontiguousarray(host.prev_idx, dtype=np.int32)
        if acc.shape != (K,) or pillar.shape != (K,) or prev_idx.shape != (K,):
            raise LibError("scan arrays must have one entry per knot")
        hess_c = _f64(host.hess) if host.hess is not None else None
        h = _vp()
        _check(load().adr_curve_plan_create(ctx._h, int(interp_method), K, P, _ptr(times), _ptr(acc),
                                            _ptr(pillar, _i32p), _ptr(prev_idx, _i32p), _ptr(dfs), _ptr(jac),
                                            _ptr(hess_c), C.byref(h)), "adr_curve_plan_create")
        self._h, self._ctx = h, ctx
        self.n_pillars, self.n_knots = P, K
        self.has_hess = hess_c is not None

    def build(self, rates) -> "CurveSet":
        """Bootstrap one curve per row of ``rates`` [S, P] (decimal par rates) on the GPU."""
        return CurveSet(self, rates)

    def close(self):
        if getattr(self, "_h", None):
            load().adr_free_curve_plan(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _SetCurve:
    """A curve owned by a `CurveSet`; accepted wherever a `DeviceCurve` is."""

    def __init__(self, handle, owner):
        self._h, self._owner = handle, owner        # keeps the set (and its plan) alive
        self.n_pillars, self.n_knots, self.has_hess = owner.n_pillars, owner.n_knots, owner.has_hess


class CurveSet:
    """Curves bootstrapped together on the GPU (adr_curve_set_build)."""

    def __init__(self, plan: CurvePlan, rates):
        rates = _f64(np.atleast_2d(rates))
        if rates.ndim != 2 or rates.shape[1] != plan.n_pillars:
            raise LibError("rates must have shape [n_scenarios, n_pillars]")
        h = _vp()
        _check(load().adr_curve_set_build(plan._ctx._h, plan._h, rates.shape[0], _ptr(rates), C.byref(h)),
               "adr_curve_set_build")
        self._h, self._plan, self._ctx = h, plan, plan._ctx
        self.n_pillars, self.n_knots, self.has_hess = plan.n_pillars, plan.n_knots, plan.has_hess
        self.n_curves = rates.shape[0]

    def __len__(self):
        return self.n_curves

    def __getitem__(self, i: int) -> _SetCurve:
        if not 0 <= i < self.n_curves:
            raise IndexError(i)
        return _SetCurve(_vp(load().adr_curve_set_get(self._h, int(i))), self)

    def download(self, i: int):
        """Dense arrays of scenario ``i``: ``dfs [K]``, ``jac [K, P]``, ``hess [K, P, P]`` (None without hess)."""
        K, P = self.n_knots, self.n_pillars
        dfs, jac = np.empty(K), np.empty((K, P))
        hess = np.empty((K, P, P)) if self.has_hess else None
        _check(load().adr_curve_set_download(self._h, int(i), _ptr(dfs), _ptr(jac), _ptr(hess)),
               "adr_curve_set_download")
        return dfs, jac, hess

    def close(self):
        if getattr(self, "_h", None):
            load().adr_free_curve_set(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceTrades:
    """A batch of OIS trades resident on the GPU (adr_trades_upload)."""

    def __init__(self, ctx: Context, batch):
        b = batch
        n = int(b.n_trades)
        arrs = dict(fix_off=np.ascontiguousarray(b.fix_off, dtype=np.int64),
                    flt_off=np.ascontiguousarray(b.flt_off, dtype=np.int64))
        for name in ("fix_tp", "fix_pay", "flt_tp", "flt_ts", "flt_te", "flt_alpha",
                     "notional", "spread", "fix_sign", "flt_sign"):
            arrs[name] = _f64(getattr(b, name))
        if arrs["fix_off"].shape != (n + 1,) or arrs["flt_off"].shape != (n + 1,):
            raise LibError("offset arrays must have n_trades + 1 entries")
        weight = getattr(b, "flt_weight", None)      # per-coupon notional multipliers (XCCY assembly) or None
        if weight is not None:
            weight = _f64(weight)
            if weight.shape != arrs["flt_tp"].shape:
                raise LibError("flt_weight must have one entry per float coupon")
        h = _vp()
        _check(load().adr_trades_upload_weighted(
            ctx._h, n, _ptr(arrs["fix_off"], _i64p), _ptr(arrs["flt_off"], _i64p),
            _ptr(arrs["fix_tp"]), _ptr(arrs["fix_pay"]), _ptr(arrs["flt_tp"]), _ptr(arrs["flt_ts"]),
            _ptr(arrs["flt_te"]), _ptr(arrs["flt_alpha"]), _ptr(weight), _ptr(arrs["notional"]), _ptr(arrs["spread"]),
            _ptr(arrs["fix_sign"]), _ptr(arrs["flt_sign"]), C.byref(h)), "adr_trades_upload")
        self._h, self._ctx = h, ctx
        self.n_trades = n

    @property
    def input_bytes(self) -> int:
        return int(load().adr_trades_input_bytes(self._h))

    def set_schedule_groups(self, mode: int, segment: int | None = None, blocks: int = 0) -> None:
        """The schedule-group route of this batch (adr_trades_set_schedule_groups): ``SCHEDULE_GROUPS_AUTO`` / ``_OFF`` /
        ``_FORCE``; ``segment``: records per wavefront of the store pass (0 = default) and ``blocks``: its persistent grid
        (0 = one wavefront per segment) - adr_trades_set_schedule_segment.
        Rebuilds device tables: not while a pricing call on the batch is in flight."""
        if segment is not None:
            _check(load().adr_trades_set_schedule_segment(self._h, int(segment), int(blocks)), "adr_trades_set_schedule_segment")
        _check(load().adr_trades_set_schedule_groups(self._h, int(mode)), "adr_trades_set_schedule_groups")

    def schedule_groups_info(self) -> dict:
        """adr_trades_schedule_groups_info: groups of two or more trades found at upload, trades in them, whether the route
        is active, the groups / trades it uses and the segment length."""
        info = np.zeros(7, dtype=np.int64)
        _check(load().adr_trades_schedule_groups_info(self._h, _ptr(info, _i64p)), "adr_trades_schedule_groups_info")
        return {"groups": int(info[0]), "grouped": int(info[1]), "active": bool(info[2]), "used_groups": int(info[3]),
                "used_trades": int(info[4]), "segment": int(info[5]), "blocks": int(info[6])}

    def close(self):
        if getattr(self, "_h", None):
            load().adr_free_trades(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def schedule_groups_host(batch):
    """The schedule groups of ``batch`` on the host (adr_schedule_groups_host; no GPU needed).  Returns ``(group_of [n],
    cF [n], cX [n], basis)``: ``basis`` holds the arrays of a batch of 2 G pseudo-trades (2g: the float leg of group g per
    unit notional, 2g + 1: its fixed leg per unit of the last payment), named as a batch's attributes."""
    n = int(batch.n_trades)
    a = {k: _f64(getattr(batch, k)) for k in ("fix_tp", "fix_pay", "flt_tp", "flt_ts", "flt_te", "flt_alpha", "notional", "spread",
                                              "fix_sign", "flt_sign")}
    fo, lo = np.ascontiguousarray(batch.fix_off, dtype=np.int64), np.ascontiguousarray(batch.flt_off, dtype=np.int64)
    w = getattr(batch, "flt_weight", None)
    w = _f64(w) if w is not None else None
    group_of, cF, cX = np.full(n, -1, dtype=np.int32), np.zeros(n), np.zeros(n)
    bfo, blo = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    n_fix, n_flt = len(a["fix_tp"]), len(a["flt_tp"])
    bf = [np.zeros(n_fix) for _ in range(2)]
    bl = [np.zeros(n_flt) for _ in range(4)]
    b_notional, b_spread = np.zeros(n), np.zeros(n)
    G = _check(load().adr_schedule_groups_host(
        n, _ptr(fo, _i64p), _ptr(lo, _i64p), _ptr(a["fix_tp"]), _ptr(a["fix_pay"]), _ptr(a["flt_tp"]), _ptr(a["flt_ts"]),
        _ptr(a["flt_te"]), _ptr(a["flt_alpha"]), _ptr(w), _ptr(a["notional"]), _ptr(a["spread"]), _ptr(a["fix_sign"]),
        _ptr(a["flt_sign"]), _ptr(group_of, _i32p), _ptr(cF), _ptr(cX), _ptr(bfo, _i64p), _ptr(blo, _i64p), _ptr(bf[0]), _ptr(bf[1]),
        _ptr(bl[0]), _ptr(bl[1]), _ptr(bl[2]), _ptr(bl[3]), _ptr(b_notional), _ptr(b_spread)), "adr_schedule_groups_host")
    m = 2 * G
    bfo, blo = bfo[:m + 1].copy(), blo[:m + 1].copy()
    basis = dict(n_trades=m, fix_off=bfo, flt_off=blo, fix_tp=bf[0][:bfo[-1]].copy(), fix_pay=bf[1][:bfo[-1]].copy(),
                 flt_tp=bl[0][:blo[-1]].copy(), flt_ts=bl[1][:blo[-1]].copy(), flt_te=bl[2][:blo[-1]].copy(),
                 flt_alpha=bl[3][:blo[-1]].copy(), notional=b_notional[:m].copy(), spread=b_spread[:m].copy(),
                 fix_sign=np.ones(m), flt_sign=np.ones(m))
    return group_of, cF, cX, basis


def upload_many(ctx: Context, batches):
    """`DeviceTrades` of several batches at once, one host thread per batch (adr_trades_upload may be called from several
    threads on one ctx; ctypes releases the GIL): validation and classification of one batch overlap the copies and the
    device-side table builds of the others - the three batches of a cross-currency book in about half the serial time."""
    batches = list(batches)
    if len(batches) <= 1:
        return [DeviceTrades(ctx, b) for b in batches]
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=len(batches)) as pool:
        return list(pool.map(lambda b: DeviceTrades(ctx, b), batches))


def price(ctx: Context, curve: DeviceCurve, trades: DeviceTrades, want_value=True, want_delta=True,
          want_gamma=True, per_trade=True, aggregate=False):
    """Blocking pricing call returning numpy arrays (adr_price).

    Returns a dict with ``pv [n]``, ``delta [n, P]``, ``gamma [n, P, P]`` (when
    ``per_trade``) and ``agg_pv``, ``agg_delta [P]``, ``agg_gamma [P, P]`` (when
    ``aggregate``)."""
    n, P = trades.n_trades, curve.n_pillars
    mask = (REQ_VALUE if want_value else 0) | (REQ_DELTA if want_delta else 0) | (REQ_GAMMA if want_gamma else 0)
    pv = np.empty(n) if (per_trade and want_value) else None
    delta = np.empty((n, P)) if (per_trade and want_delta) else None
    gamma = np.empty((n, P, P)) if (per_trade and want_gamma) else None
    agg = np.empty(1 + P + P * P) if aggregate else None
    _check(load().adr_price(ctx._h, curve._h, trades._h, mask, _ptr(pv), _ptr(delta), _ptr(gamma), _ptr(agg)),
           "adr_price")
    out = {}
    if pv is not None:
        out["pv"] = pv
    if delta is not None:
        out["delta"] = delta
    if gamma is not None:
        out["gamma"] = gamma
    if agg is not None:
        out["agg_pv"] = float(agg[0])
        out["agg_delta"] = agg[1:1 + P].copy()
        out["agg_gamma"] = agg[1 + P:].reshape(P, P).copy()
    return out


def price_xccy_foreign(ctx: Context, foreign_curve: DeviceCurve, xccy_curve: DeviceCurve, legs: DeviceTrades, want_value=True,
                       want_delta=True, per_trade=True, aggregate=False):
    """The foreign legs of a cross-currency book on two curves in one launch (adr_price_xccy_foreign): ``pv [n]``,
    ``delta_foreign [n, P_f]``, ``delta_basis [n, P_x]`` in FOREIGN currency (per trade), ``agg_pv``, ``agg_delta_foreign``,
    ``agg_delta_basis`` (book).  Raises `LibError` (ADR_ERR_UNSUPPORTED) for books the launch does not take."""
    n, Pf, Px = legs.n_trades, foreign_curve.n_pillars, xccy_curve.n_pillars
    mask = (REQ_VALUE if want_value else 0) | (REQ_DELTA if want_delta else 0)
    pv = np.empty(n) if (per_trade and want_value) else None
    df = np.empty((n, Pf)) if (per_trade and want_delta) else None
    dx = np.empty((n, Px)) if (per_trade and want_delta) else None
    af = np.empty(1 + Pf + Pf * Pf) if aggregate else None
    ax = np.empty(1 + Px + Px * Px) if aggregate else None
    _check(load().adr_price_xccy_foreign(ctx._h, foreign_curve._h, xccy_curve._h, legs._h, mask, _ptr(pv), _ptr(df), _ptr(dx),
                                         _ptr(af), _ptr(ax)), "adr_price_xccy_foreign")
    out = {}
    if pv is not None:
        out["pv"] = pv
    if df is not None:
        out["delta_foreign"], out["delta_basis"] = df, dx
    if aggregate:
        out["agg_pv"] = float(af[0])
        out["agg_delta_foreign"], out["agg_delta_basis"] = af[1:1 + Pf].copy(), ax[1:1 + Px].copy()
    return out


def price_xccy_foreign_dev(ctx: Context, foreign_curve: DeviceCurve, xccy_curve: DeviceCurve, legs: DeviceTrades, mask: int, pv_ptr=0,
                           delta_foreign_ptr=0, delta_basis_ptr=0, agg_foreign_ptr=0, agg_basis_ptr=0, stream=0):
    """Non-blocking form (adr_price_xccy_foreign_dev): device pointers as integers."""
    _check(load().adr_price_xccy_foreign_dev(ctx._h, foreign_curve._h, xccy_curve._h, legs._h, int(mask), _vp(pv_ptr or None),
                                             _vp(delta_foreign_ptr or None), _vp(delta_basis_ptr or None),
                                             _vp(agg_foreign_ptr or None), _vp(agg_basis_ptr or None), _vp(stream or None)),
           "adr_price_xccy_foreign_dev")


def price_dev(ctx: Context, curve: DeviceCurve, trades: DeviceTrades, mask: int, pv_ptr=0, delta_ptr=0,
              gamma_ptr=0, agg_ptr=0, stream=0):
    """Non-blocking pricing into caller-owned device buffers (adr_price_dev);
    pointers are integers (e.g. ``tensor.data_ptr()``), ``stream`` a hipStream_t
    handle (0 = the context's own stream)."""
    _check(load().adr_price_dev(ctx._h, curve._h, trades._h, int(mask), _vp(pv_ptr or None), _vp(delta_ptr or None),
                                _vp(gamma_ptr or None), _vp(agg_ptr or None), _vp(stream or None)), "adr_price_dev")


def curve_df(ctx: Context, curve: DeviceCurve, t):
    """Discount factors at the times ``t`` off an uploaded curve, evaluated on the GPU (adr_curve_df): the batched
    `InterpolatorAd.simple_interpolate`.  Scalars in, scalar out."""
    tt = _f64(np.atleast_1d(t))
    out = np.empty_like(tt)
    _check(load().adr_curve_df(ctx._h, curve._h, tt.size, _ptr(tt), _ptr(out)), "adr_curve_df")
    return float(out[0]) if np.ndim(t) == 0 else out.reshape(np.shape(t))


def _curve_arrays(times, dfs, jac, hess, shapes=False):
    """``(times, dfs, jac, hess or None, K, P)`` as contiguous float64 arrays; ``shapes``: refuse arrays that do not fit
    jac's ``[K, P]``."""
    times, dfs, jac = _f64(times), _f64(dfs), _f64(jac)
    K, P = jac.shape
    if shapes and (times.shape != (K,) or dfs.shape != (K,)):
        raise LibError("curve arrays have inconsistent shapes")
    hess = None if hess is None else _f64(hess)
    if shapes and hess is not None and hess.shape != (K, P, P):
        raise LibError("hess must have shape [K, P, P]")
    return times, dfs, jac, hess, K, P


def curve_tables_host(times, dfs, jac, hess=None):
    """Log-space tables of the reachable knots, computed by the library's host
    code (no GPU needed) - used by the CPU tests."""
    times, dfs, jac, hess_c, K, P = _curve_arrays(times, dfs, jac, hess)
    lib = load()
    kc = _check(lib.adr_curve_tables_host(K, P, _ptr(times), _ptr(dfs), _ptr(jac), _ptr(hess_c),
                                          None, None, None, None), "adr_curve_tables_host")
    idx = np.empty(kc, dtype=np.int32)
    log_df = np.empty(kc)
    lj = np.empty((kc, P))
    lc = np.empty((kc, P, P)) if hess is not None else None
    _check(lib.adr_curve_tables_host(K, P, _ptr(times), _ptr(dfs), _ptr(jac), _ptr(hess_c),
                                     _ptr(idx, _i32p), _ptr(log_df), _ptr(lj), _ptr(lc)), "adr_curve_tables_host")
    return dict(knot_index=idx, log_df=log_df, lj=lj, lc=lc)


def curve_layout_host(times, dfs, jac, hess=None):
    """LDS layout the fast kernels would use for this curve (diagnostic; no GPU needed)."""
    times, dfs, jac, hess_c, K, P = _curve_arrays(times, dfs, jac, hess)
    info = np.zeros(16, dtype=np.int64)
    _check(load().adr_curve_layout_host(K, P, _ptr(times), _ptr(dfs), _ptr(jac), _ptr(hess_c), _ptr(info, _i64p)),
           "adr_curve_layout_host")
    keys = ("packed_ok", "core_pillars", "core_pairs", "packed_entries", "entries_per_lane", "core_rows",
            "mini_knots", "lds_bytes", "general_lds_bytes", "general_lds_rows", "core_slots_per_lane", "hub_layout",
            "wide_chunks", "wide_lds_bytes", "wide_max_knot_chunks", "upload_lds_bytes")
    return dict(zip(keys, (int(v) for v in info)))


def leg_times_host(effective, termination, months_per_period, payment_lag, bd_value, weekend_calendar, denominator,
                   value_serial, payment_denominator=None):
    """Coupon schedules of many legs (adr_leg_counts_host + adr_leg_times_host; threads on the host, no GPU):
    ``(off, tp, ts, te, alpha, plain)`` - CSR offsets over the coupons, payment / accrual start / accrual end times as year
    fractions from ``value_serial``, accrual fractions, and the mask of legs with strictly increasing dates."""
    i64 = lambda a, n: np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.int64), (n,)))
    eff = np.ascontiguousarray(effective, dtype=np.int64)
    n = eff.shape[0]
    term, mpp, lag = i64(termination, n), i64(months_per_period, n), i64(payment_lag, n)
    den = np.ascontiguousarray(np.broadcast_to(np.asarray(denominator, dtype=np.float64), (n,)))
    counts = np.empty(n, dtype=np.int64)
    lib = load()
    _check(lib.adr_leg_counts_host(n, _ptr(eff, _i64p), _ptr(term, _i64p), _ptr(mpp, _i64p), _ptr(counts, _i64p)),
           "adr_leg_counts_host")
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    m = int(off[-1])
    tp, ts, te, al = (np.empty(m) for _ in range(4))
    plain = np.empty(n, dtype=np.uint8)
    _check(lib.adr_leg_times_host(n, _ptr(eff, _i64p), _ptr(term, _i64p), _ptr(mpp, _i64p), _ptr(lag, _i64p), int(bd_value),
                                  1 if weekend_calendar else 0, _ptr(den), int(value_serial),
                                  float(payment_denominator or 0.0), _ptr(off, _i64p), _ptr(tp), _ptr(ts), _ptr(te), _ptr(al),
                                  _ptr(plain, C.POINTER(C.c_uint8))), "adr_leg_times_host")
    return off, tp, ts, te, al, plain.astype(bool)


def exchange_flows_host(exch_t, notional, on, sign, scale):
    """Notional exchanges of n legs (adr_exchange_flows_host): ``(off, flow_tp, flow_pay, pv_const)``."""
    exch_t = _f64(exch_t).reshape(-1)
    notional, sign = _f64(notional), _f64(sign)
    n = notional.shape[0]
    on = np.ascontiguousarray(on, dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.int64)
    tp, pay, const = np.empty(2 * n), np.empty(2 * n), np.empty(n)
    _check(load().adr_exchange_flows_host(n, _ptr(exch_t), _ptr(notional), _ptr(on, C.POINTER(C.c_uint8)), _ptr(sign), float(scale),
                                          _ptr(off, _i64p), _ptr(tp), _ptr(pay), _ptr(const)), "adr_exchange_flows_host")
    k = int(off[-1])
    return off, tp[:k], pay[:k], const


def xccy_assemble_host(for_off, tp_x, ts, te, alpha, disc, growth, for_n, for_spread, for_sign, spot, exch_t, exch_on,
                       pv_const):
    """Foreign-leg batches of a cross-currency book (adr_xccy_assemble_host): ``(rates_off, rates_ts, rates_te, rates_alpha,
    rates_weight, flows_off, flows_tp, flows_pay, pv_const)``; ``pv_const`` comes in with the domestic constants.
    ``disc`` [m + 1]: D_x at the payment times, then at the value time; ``growth`` [2 m]: D_f at the accrual starts, then ends."""
    for_off = np.ascontiguousarray(for_off, dtype=np.int64)
    n, m = for_off.shape[0] - 1, int(for_off[-1])
    cols = [_f64(a) for a in (tp_x, ts, te, alpha, disc, growth, for_n, for_spread, for_sign)]
    exch_t = _f64(exch_t).reshape(-1)
    exch_on = np.ascontiguousarray(exch_on, dtype=np.uint8)
    pv = np.array(pv_const, dtype=np.float64)
    r_off, f_off = np.empty(n + 1, dtype=np.int64), np.empty(n + 1, dtype=np.int64)
    r_ts, r_te, r_al, r_w = (np.empty(m) for _ in range(4))
    f_tp, f_pay = np.empty(m + 2 * n), np.empty(m + 2 * n)
    u8 = C.POINTER(C.c_uint8)
    _check(load().adr_xccy_assemble_host(n, _ptr(for_off, _i64p), *(_ptr(a) for a in cols), float(spot), _ptr(exch_t),
                                         _ptr(exch_on, u8), _ptr(r_off, _i64p), _ptr(r_ts), _ptr(r_te), _ptr(r_al), _ptr(r_w),
                                         _ptr(f_off, _i64p), _ptr(f_tp), _ptr(f_pay), _ptr(pv)), "adr_xccy_assemble_host")
    if n == 0:
        r_off[:] = 0; f_off[:] = 0
    kr, kf = int(r_off[-1]), int(f_off[-1])
    return r_off, r_ts[:kr], r_te[:kr], r_al[:kr], r_w[:kr], f_off, f_tp[:kf], f_pay[:kf], pv


BOND_OUTPUTS = ("z", "dirty", "clean", "ytm", "duration", "convexity", "dv01")     # rows of adr_bond_measures' out
BOND_FLOW_FIELDS = ("flow_T", "flow_tau", "flow_cpn", "flow_prin")
BOND_FIELDS = ("bond_Ts", "bond_tauM", "bond_face", "bond_acc100", "bond_quote")


def _bond_arrays(node_t, node_df, book):
    """Contiguous copies of a bond book's arrays (keys: ``flow_off``, BOND_FLOW_FIELDS, BOND_FIELDS)."""
    node_t, node_df = _f64(node_t), _f64(node_df)
    if node_t.ndim != 1 or node_t.shape != node_df.shape:
        raise LibError("node_t and node_df must be 1-D arrays of one length")
    arr = {"flow_off": np.ascontiguousarray(book["flow_off"], dtype=np.int64)}
    n = arr["flow_off"].shape[0] - 1
    if n < 0:
        raise LibError("flow_off needs n_bonds + 1 entries")
    for k in BOND_FLOW_FIELDS + BOND_FIELDS:
        arr[k] = _f64(book[k]).reshape(-1)
    m = int(arr["flow_off"][-1]) if n > 0 else 0
    if any(arr[k].shape != (m,) for k in BOND_FLOW_FIELDS) or any(arr[k].shape != (n,) for k in BOND_FIELDS):
        raise LibError("bond arrays have inconsistent lengths")
    return node_t, node_df, arr, n


def _bond_result(out, status):
    res = {k: out[i] for i, k in enumerate(BOND_OUTPUTS)}
    res["status"] = status
    return res


def bond_measures(ctx: Context, interp_method: int, node_t, node_df, book, quote_is_z: bool):
    """Spread and yield measures of a bond book on the GPU (adr_bond_measures, blocking).  ``book``: a mapping with
    ``flow_off`` and the fields BOND_FLOW_FIELDS + BOND_FIELDS.  Returns a dict of arrays, keys BOND_OUTPUTS + ``status``."""
    node_t, node_df, a, n = _bond_arrays(node_t, node_df, book)
    out, status = np.empty((len(BOND_OUTPUTS), n)), np.empty(n, dtype=np.int32)
    _check(load().adr_bond_measures(ctx._h, int(interp_method), node_t.size, _ptr(node_t), _ptr(node_df), n,
                                    _ptr(a["flow_off"], _i64p), *(_ptr(a[k]) for k in BOND_FLOW_FIELDS + BOND_FIELDS),
                                    1 if quote_is_z else 0, _ptr(out), _ptr(status, _i32p)), "adr_bond_measures")
    return _bond_result(out, status)


def bond_measures_host(interp_method: int, node_t, node_df, book, quote_is_z: bool):
    """The same per-bond code on the CPU (adr_bond_measures_host; no GPU needed)."""
    node_t, node_df, a, n = _bond_arrays(node_t, node_df, book)
    out, status = np.empty((len(BOND_OUTPUTS), n)), np.empty(n, dtype=np.int32)
    _check(load().adr_bond_measures_host(int(interp_method), node_t.size, _ptr(node_t), _ptr(node_df), n,
                                         _ptr(a["flow_off"], _i64p), *(_ptr(a[k]) for k in BOND_FLOW_FIELDS + BOND_FIELDS),
                                         1 if quote_is_z else 0, _ptr(out), _ptr(status, _i32p)), "adr_bond_measures_host")
    return _bond_result(out, status)


def bond_measures_dev(ctx: Context, interp_method: int, n_nodes: int, n_bonds: int, ptrs, quote_is_z: bool, out_ptr: int,
                      status_ptr: int, stream=0):
    """Non-blocking form (adr_bond_measures_dev): ``ptrs`` maps ``node_t``, ``node_df``, ``flow_off`` and the fields of
    BOND_FLOW_FIELDS + BOND_FIELDS to device pointers (integers, e.g. ``tensor.data_ptr()``); ``out_ptr``: float64
    [len(BOND_OUTPUTS), n_bonds], ``status_ptr``: int32 [n_bonds]."""
    keys = ("node_t", "node_df", "flow_off") + BOND_FLOW_FIELDS + BOND_FIELDS
    p = [_vp(int(ptrs[k]) or None) for k in keys]
    _check(load().adr_bond_measures_dev(ctx._h, int(interp_method), int(n_nodes), p[0], p[1], int(n_bonds), *p[2:],
                                        1 if quote_is_z else 0, _vp(out_ptr or None), _vp(status_ptr or None),
                                        _vp(stream or None)), "adr_bond_measures_dev")


FRN_OUTPUTS = ("dm", "dirty", "clean", "pv", "mod_duration", "dv01")          # rows of adr_frn_measures' out
FRN_FLOW_FIELDS = ("cpn_T", "cpn_ts", "cpn_te", "cpn_ialpha", "cpn_alpha", "cpn_tau", "cpn_fix")   # rows of its cpn
FRN_FIELDS = ("frn_Ts", "frn_TM", "frn_tauM", "frn_face", "frn_margin", "frn_cap", "frn_floor", "frn_ffr", "frn_acc100",
              "frn_quote", "frn_guess")                                        # rows of its frn


def _frn_nodes(curve):
    method, node_t, node_df = curve
    node_t, node_df = _f64(node_t), _f64(node_df)
    if node_t.ndim != 1 or node_t.shape != node_df.shape:
        raise LibError("node_t and node_df must be 1-D arrays of one length")
    return int(method), node_t, node_df


def frn_pack(book):
    """``(cpn_off, cpn [len(FRN_FLOW_FIELDS), m], frn [len(FRN_FIELDS), n])``: the field-major arrays adr_frn_measures
    reads, from a mapping with ``cpn_off`` and the fields FRN_FLOW_FIELDS + FRN_FIELDS."""
    off = np.ascontiguousarray(book["cpn_off"], dtype=np.int64)
    n = off.shape[0] - 1
    if n < 0:
        raise LibError("cpn_off needs n_frns + 1 entries")
    m = int(off[-1]) if n > 0 else 0
    cpn = np.empty((len(FRN_FLOW_FIELDS), m))
    frn = np.empty((len(FRN_FIELDS), n))
    for rows, fields, size in ((cpn, FRN_FLOW_FIELDS, m), (frn, FRN_FIELDS, n)):
        for k, name in enumerate(fields):
            v = np.asarray(book[name], dtype=np.float64).reshape(-1)
            if v.shape != (size,):
                raise LibError(f"FRN array {name} has {v.size} entries, not {size}")
            rows[k] = v
    return off, cpn, frn


def _frn_result(out, status):
    res = {k: out[i] for i, k in enumerate(FRN_OUTPUTS)}
    res["status"] = status
    return res


def frn_measures(ctx: Context, disc, index, book, quote_is_dm: bool):
    """Discount margins and prices of an FRN book on the GPU (adr_frn_measures, blocking).  ``disc`` / ``index``:
    ``(interp method, node times, node dfs)`` of the two curves; ``book``: a mapping with ``cpn_off`` and the fields
    FRN_FLOW_FIELDS + FRN_FIELDS.  Returns a dict of arrays, keys FRN_OUTPUTS + ``status``."""
    (dm, dt, dd), (im, it, idf) = _frn_nodes(disc), _frn_nodes(index)
    off, cpn, frn = frn_pack(book)
    n, m = frn.shape[1], cpn.shape[1]
    out, status = np.empty((len(FRN_OUTPUTS), n)), np.empty(n, dtype=np.int32)
    _check(load().adr_frn_measures(ctx._h, dm, dt.size, _ptr(dt), _ptr(dd), im, it.size, _ptr(it), _ptr(idf), n, m,
                                   _ptr(off, _i64p), _ptr(cpn), _ptr(frn), 1 if quote_is_dm else 0, _ptr(out),
                                   _ptr(status, _i32p)), "adr_frn_measures")
    return _frn_result(out, status)


def frn_measures_host(disc, index, book, quote_is_dm: bool):
    """The same per-FRN code on the CPU (adr_frn_measures_host; no GPU needed)."""
    (dm, dt, dd), (im, it, idf) = _frn_nodes(disc), _frn_nodes(index)
    off, cpn, frn = frn_pack(book)
    n, m = frn.shape[1], cpn.shape[1]
    out, status = np.empty((len(FRN_OUTPUTS), n)), np.empty(n, dtype=np.int32)
    _check(load().adr_frn_measures_host(dm, dt.size, _ptr(dt), _ptr(dd), im, it.size, _ptr(it), _ptr(idf), n, m,
                                        _ptr(off, _i64p), _ptr(cpn), _ptr(frn), 1 if quote_is_dm else 0, _ptr(out),
                                        _ptr(status, _i32p)), "adr_frn_measures_host")
    return _frn_result(out, status)


def frn_measures_dev(ctx: Context, disc_method: int, disc_n: int, index_method: int, index_n: int, n_frns: int,
                     n_coupons: int, ptrs, quote_is_dm: bool, out_ptr: int, status_ptr: int, stream=0):
    """Non-blocking form (adr_frn_measures_dev): ``ptrs`` maps ``disc_t``, ``disc_df``, ``index_t``, ``index_df``,
    ``cpn_off``, ``cpn`` and ``frn`` (the arrays of `frn_pack`) to device pointers (integers, e.g. ``tensor.data_ptr()``);
    ``out_ptr``: float64 [len(FRN_OUTPUTS), n_frns], ``status_ptr``: int32 [n_frns]."""
    p = {k: _vp(int(ptrs[k]) or None) for k in ("disc_t", "disc_df", "index_t", "index_df", "cpn_off", "cpn", "frn")}
    _check(load().adr_frn_measures_dev(ctx._h, int(disc_method), int(disc_n), p["disc_t"], p["disc_df"], int(index_method),
                                       int(index_n), p["index_t"], p["index_df"], int(n_frns), int(n_coupons),
                                       p["cpn_off"], p["cpn"], p["frn"], 1 if quote_is_dm else 0, _vp(out_ptr or None),
                                       _vp(status_ptr or None), _vp(stream or None)), "adr_frn_measures_dev")


YOY_FIELDS = ("tp", "ts", "te", "scale", "spread")       # rows of adr_yoy_risk's cpn
YOY_PER_SWAP, YOY_AGG = 8, 16                               # ADR_YOY_PER_SWAP, ADR_YOY_AGG
YOY_CHUNK = 16                                              # ADR_YOY_CHUNK
YOY_MAX_PILLARS = 64


def yoy_pack(book):
    """``(cpn_off, cpn [len(YOY_FIELDS), m])``: the field-major arrays adr_yoy_risk reads, from a mapping with
    ``cpn_off`` and the per-coupon fields YOY_FIELDS."""
    off = np.ascontiguousarray(book["cpn_off"], dtype=np.int64)
    n = off.shape[0] - 1
    if n < 0:
        raise LibError("cpn_off needs n_swaps + 1 entries")
    m = int(off[-1]) if n > 0 else 0
    cpn = np.empty((len(YOY_FIELDS), m))
    for k, name in enumerate(YOY_FIELDS):
        v = np.asarray(book[name], dtype=np.float64).reshape(-1)
        if v.shape != (m,):
            raise LibError(f"YoY array {name} has {v.size} entries, not {m}")
        cpn[k] = v
    return off, cpn


def _yoy_call(fn, head, disc, infl, book, req_mask, per_swap, aggregate):
    (dm, dt, dd), (im, T, b) = _frn_nodes(disc), _frn_nodes(infl)
    off, cpn = yoy_pack(book)
    n, m, P = off.shape[0] - 1, cpn.shape[1], T.size
    mask = int(req_mask) | (YOY_PER_SWAP if per_swap else 0) | (YOY_AGG if aggregate else 0)
    out = {"amount": np.empty(m)}
    if per_swap:
        out.update(pv=np.zeros(n), delta=np.zeros((n, P)), gamma=np.zeros((n, P, P)))
    if aggregate:
        out["agg"] = np.zeros(1 + P + P * P)
    g = lambda k: _ptr(out.get(k))
    _check(fn(*head, dm, dt.size, _ptr(dt), _ptr(dd), im, P, _ptr(T), _ptr(b), n, m, _ptr(off, _i64p), _ptr(cpn), mask,
              g("amount"), g("pv"), g("delta"), g("gamma"), g("agg")), fn.__name__)
    if aggregate:
        a = out.pop("agg")
        out.update(agg_pv=float(a[0]), agg_delta=a[1:1 + P].copy(), agg_gamma=a[1 + P:].reshape(P, P).copy())
    return out


def yoy_risk(ctx: Context, disc, infl, book, req_mask=REQ_VALUE | REQ_DELTA | REQ_GAMMA, per_swap=True, aggregate=False):
    """Projected amounts, inflation-leg PVs and inflation-curve ladders of a YoY swap book on the GPU (adr_yoy_risk,
    blocking).  ``disc``: ``(interp method, knot times, knot dfs)`` of the engine's discount grid; ``infl``:
    ``(interp method, pillar times T, breakeven rates b)``; ``book``: ``cpn_off`` and the fields YOY_FIELDS.  Returns
    ``amount`` [m], and per swap ``pv``, ``delta`` [n, P] (per bp), ``gamma`` [n, P, P] (per bp^2) and / or the book's
    ``agg_pv``, ``agg_delta``, ``agg_gamma``."""
    return _yoy_call(load().adr_yoy_risk, (ctx._h,), disc, infl, book, req_mask, per_swap, aggregate)


def yoy_risk_host(disc, infl, book, req_mask=REQ_VALUE | REQ_DELTA | REQ_GAMMA, per_swap=True, aggregate=False):
    """`yoy_risk` on the CPU (adr_yoy_risk_host): the same per-swap code and reduction order; no GPU needed."""
    return _yoy_call(load().adr_yoy_risk_host, (), disc, infl, book, req_mask, per_swap, aggregate)


def yoy_risk_work(n_swaps: int, n_pillars: int) -> int:
    """Doubles of scratch `yoy_risk_dev` needs for ``YOY_AGG``."""
    return int(load().adr_yoy_risk_work(int(n_swaps), int(n_pillars)))


def yoy_risk_dev(ctx: Context, disc_method: int, K: int, infl_method: int, P: int, n_swaps: int, n_coupons: int, ptrs,
                 req_mask: int, out_ptrs, stream=0):
    """Non-blocking form (adr_yoy_risk_dev): ``ptrs`` maps ``times``, ``dfs``, ``T``, ``b``, ``cpn_off`` and ``cpn`` to
    device pointers (integers, e.g. ``tensor.data_ptr()``); ``out_ptrs`` maps any of ``amount``, ``pv``, ``delta``,
    ``gamma``, ``agg`` and ``work`` (`yoy_risk_work` doubles) to device pointers; ``req_mask`` includes YOY_PER_SWAP /
    YOY_AGG as wanted."""
    p = {k: _vp(int(ptrs[k]) or None) for k in ("times", "dfs", "T", "b", "cpn_off", "cpn")}
    o = {k: _vp(int(out_ptrs.get(k, 0)) or None) for k in ("amount", "pv", "delta", "gamma", "agg", "work")}
    _check(load().adr_yoy_risk_dev(ctx._h, int(disc_method), int(K), p["times"], p["dfs"], int(infl_method), int(P), p["T"],
                                   p["b"], int(n_swaps), int(n_coupons), p["cpn_off"], p["cpn"], int(req_mask), o["amount"],
                                   o["pv"], o["delta"], o["gamma"], o["agg"], o["work"], _vp(stream or None)),
           "adr_yoy_risk_dev")


SCENARIO_CHUNK = 64                                         # ADR_SCENARIO_CHUNK
SCENARIO_MAX_KNOTS = 4096


def _scenario_curves(times, dfs):
    times = _f64(times).reshape(-1)
    dfs = _f64(np.atleast_2d(dfs))
    if dfs.ndim != 2 or dfs.shape[1] != times.size:
        raise LibError(f"dfs must have shape [n_scenarios, {times.size}] (one row per scenario, one column per knot), "
                       f"not {list(dfs.shape)}")
    return times, dfs


# The scenario entries share one argument list, in this order: the curves (host arrays, or a context and a `CurveSet`), the
# credit scenario group, the trades (a handle, or the host arrays of a `TradeBatch`), the credit per-trade group, the
# sub-books, then ``pv``, the output and, on the host, ``n_threads``.  One helper per group returns its arguments.
def _curve_args(method, times, dfs):
    return [int(method), times.size, _ptr(times), dfs.shape[0], _ptr(dfs)]


def _spread_args(dz):
    return [dz.shape[1], dz.shape[0], _ptr(dz) if dz.size else None]


def _batch_args(n, fo, lo, a, w):
    """`_batch_arrays`' result as the _host entries take it."""
    p = lambda *names: [_ptr(a[k]) for k in names]
    return ([n, _ptr(fo, _i64p), _ptr(lo, _i64p)] + p("fix_tp", "fix_pay", "flt_tp", "flt_ts", "flt_te", "flt_alpha") + [_ptr(w)] +
            p("notional", "spread", "fix_sign", "flt_sign"))


def _credit_trade_args(z, bucket, fix_tau, flt_tau, counts):
    """``counts``: beside a trades handle the entries take the two flow counts, beside host arrays they know them."""
    if counts:
        return [_ptr(z), _ptr(bucket, _i32p), fix_tau.size, _ptr(fix_tau), flt_tau.size, _ptr(flt_tau)]
    return [_ptr(z), _ptr(bucket, _i32p), _ptr(fix_tau), _ptr(flt_tau)]


def _scenario_call(fn, args, n, S, per_trade, sub=None, tail=()):
    """Call a blocking or host scenario entry with ``args``, the sub-book group of ``sub`` (`_sub_offsets`' pair; None: the
    whole book), the outputs it allocates and ``tail``: ``book_pv [S]`` or ``sub_pv [B, S]`` and, with ``per_trade``,
    ``pv [S, n]``."""
    pv = np.empty((n, S)) if per_trade else None
    if sub is None:
        key, out = "book_pv", np.empty(S)
    else:
        key, out = "sub_pv", np.empty((sub[1], S))
        args = args + [sub[1], _ptr(sub[0], _i64p)]
    _check(fn(*args, _ptr(pv), _ptr(out), *tail), fn.__name__)
    res = {key: out}
    if per_trade:
        res["pv"] = pv.T                # the library's rows are per trade ([n, S]); a view, no copy
    return res


def _dev(p):
    """A device pointer given as an integer (0: none) as the ``_dev`` entries take it."""
    return _vp(int(p) or None)


def _dev_of(ptrs):
    """The same by name, from a mapping of names to device pointers (a name left out: none)."""
    return lambda k: _dev(ptrs.get(k, 0))


def scenario_pv(ctx: Context, method: int, times, dfs, trades: DeviceTrades, per_trade=False):
    """PVs of an uploaded batch under the scenario curves ``dfs [S, K]`` on the knots ``times [K]`` (adr_scenario_pv,
    blocking): ``book_pv [S]`` and, with ``per_trade``, ``pv [S, n]``."""
    times, dfs = _scenario_curves(times, dfs)
    return _scenario_call(load().adr_scenario_pv, [ctx._h] + _curve_args(method, times, dfs) + [trades._h], trades.n_trades,
                          dfs.shape[0], per_trade)


def _batch_arrays(batch):
    """The arrays of a `TradeBatch` as the _host entries take them: ``(n, fix_off, flt_off, values dict, flt_weight)``."""
    n = int(batch.n_trades)
    fo = np.ascontiguousarray(batch.fix_off, dtype=np.int64)
    lo = np.ascontiguousarray(batch.flt_off, dtype=np.int64)
    if fo.shape != (n + 1,) or lo.shape != (n + 1,):
        raise LibError("offset arrays must have n_trades + 1 entries")
    a = {k: _f64(getattr(batch, k)) for k in ("fix_tp", "fix_pay", "flt_tp", "flt_ts", "flt_te", "flt_alpha", "notional",
                                              "spread", "fix_sign", "flt_sign")}
    w = getattr(batch, "flt_weight", None)
    w = None if w is None else _f64(w)
    if w is not None and w.shape != a["flt_tp"].shape:
        raise LibError("flt_weight must have one entry per float coupon")
    return n, fo, lo, a, w


def scenario_pv_host(method: int, times, dfs, batch, per_trade=False, n_threads=0):
    """`scenario_pv` on the CPU (adr_scenario_pv_host) for a `TradeBatch`: the same per-trade arithmetic and the same
    order of the book sum; no GPU needed."""
    times, dfs = _scenario_curves(times, dfs)
    arrays = _batch_arrays(batch)
    return _scenario_call(load().adr_scenario_pv_host, _curve_args(method, times, dfs) + _batch_args(*arrays), arrays[0],
                          dfs.shape[0], per_trade, tail=(int(n_threads),))


def scenario_pv_set(ctx: Context, curve_set: CurveSet, trades: DeviceTrades, per_trade=False):
    """`scenario_pv` on the curves of a `CurveSet`, read where the device builder left them (adr_scenario_pv_set)."""
    return _scenario_call(load().adr_scenario_pv_set, [ctx._h, curve_set._h, trades._h], trades.n_trades, len(curve_set),
                          per_trade)


def curve_set_arrays(curve_set: CurveSet) -> dict:
    """``method``, ``K``, ``S`` and the device pointers ``times`` [K] and ``dfs`` [S, K] of a set (adr_curve_set_arrays)."""
    m, K, S, t, d = C.c_int(), C.c_int(), C.c_int(), _vp(), _vp()
    _check(load().adr_curve_set_arrays(curve_set._h, C.byref(m), C.byref(K), C.byref(S), C.byref(t), C.byref(d)),
           "adr_curve_set_arrays")
    return dict(method=m.value, K=K.value, S=S.value, times=t.value or 0, dfs=d.value or 0)


def scenario_pv_work(n_trades: int, n_scenarios: int) -> int:
    """Doubles of scratch `scenario_pv_dev` needs."""
    return int(load().adr_scenario_pv_work(int(n_trades), int(n_scenarios)))


def scenario_pv_dev(ctx: Context, method: int, K: int, times_ptr: int, S: int, dfs_ptr: int, trades: DeviceTrades,
                    book_ptr: int, work_ptr: int, pv_ptr: int = 0, stream=0):
    """Non-blocking form (adr_scenario_pv_dev): device pointers (integers) of ``times`` [K], ``dfs`` [S, K], the outputs
    ``book_pv`` [S] and ``pv`` [n, S] (trade-major; 0: not wanted) and `scenario_pv_work` doubles of scratch."""
    _check(load().adr_scenario_pv_dev(ctx._h, int(method), int(K), _dev(times_ptr), int(S), _dev(dfs_ptr), trades._h,
                                      _dev(pv_ptr), _dev(book_ptr), _dev(work_ptr), _vp(stream or None)), "adr_scenario_pv_dev")


def _yoy_legs(fixed, book):
    """``(fix_off, fix_tp, fix_pay, cpn_off, cpn)`` of a YoY book from the fixed legs ``(fix_off, fix_tp, fix_pay)`` (None: no
    fixed flows) and the coupon book (``cpn_off`` and YOY_FIELDS; None: no coupons)."""
    if fixed is None and book is None:
        raise LibError("neither fixed legs nor YoY coupons")
    if book is not None:
        cpn_off, cpn = yoy_pack(book)
    if fixed is not None:
        fix_off = np.ascontiguousarray(fixed[0], dtype=np.int64)
        fix_tp, fix_pay = _f64(fixed[1]).reshape(-1), _f64(fixed[2]).reshape(-1)
        if fix_off.ndim != 1 or fix_off.size < 1 or fix_tp.shape != fix_pay.shape:
            raise LibError("fixed legs are (fix_off [n + 1], fix_tp, fix_pay) with one amount per time")
    else:
        fix_off, fix_tp, fix_pay = np.zeros_like(cpn_off), np.zeros(0), np.zeros(0)
    if book is None:
        cpn_off, cpn = np.zeros_like(fix_off), np.zeros((len(YOY_FIELDS), 0))
    if fix_off.shape != cpn_off.shape:
        raise LibError(f"fix_off describes {fix_off.size - 1} swaps, cpn_off {cpn_off.size - 1}")
    return fix_off, fix_tp, fix_pay, cpn_off, cpn


def _yoy_scenario_inputs(times, dfs, T, b, fixed, book):
    """The arrays of adr_yoy_scenario_pv from ``dfs`` [S, K] or [K], ``b`` [S, P] or [P], the fixed legs ``(fix_off,
    fix_tp, fix_pay)`` (None: no fixed flows) and the coupon book (``cpn_off`` and YOY_FIELDS; None: no coupons)."""
    times, dfs = _scenario_curves(times, dfs)
    T = _f64(T).reshape(-1)
    b = _f64(np.atleast_2d(b))
    if b.ndim != 2 or b.shape[1] != T.size:
        raise LibError(f"b must have shape [n_scenarios, {T.size}] or [{T.size}] (one column per pillar), not {list(b.shape)}")
    S = max(dfs.shape[0], b.shape[0])
    if dfs.shape[0] not in (1, S) or b.shape[0] not in (1, S):
        raise LibError(f"{dfs.shape[0]} discount rows and {b.shape[0]} breakeven rows: each must be one shared row or "
                       "one row per scenario")
    fix_off, fix_tp, fix_pay, cpn_off, cpn = _yoy_legs(fixed, book)
    return times, dfs, T, b, S, fix_off, fix_tp, fix_pay, cpn_off, cpn


def _yoy_scenario_call(fn, head, tail, disc_method, times, dfs, infl_method, T, b, fixed, book, per_trade, *sub_off):
    """The four blocking and host YoY entries: ``head`` the context or nothing, ``tail`` ``n_threads`` or nothing,
    ``sub_off`` given for the sub-book entries."""
    times, dfs, T, b, S, fix_off, fix_tp, fix_pay, cpn_off, cpn = _yoy_scenario_inputs(times, dfs, T, b, fixed, book)
    sub = _sub_offsets(*sub_off) if sub_off else None
    n = fix_off.size - 1
    args = [*head, *_curve_args(disc_method, times, dfs), int(infl_method), T.size, _ptr(T), b.shape[0], _ptr(b), S, n,
            fix_tp.size, _ptr(fix_off, _i64p), _ptr(fix_tp), _ptr(fix_pay), cpn.shape[1], _ptr(cpn_off, _i64p), _ptr(cpn)]
    return _scenario_call(fn, args, n, S, per_trade, sub, tail)


def yoy_scenario_pv(ctx: Context, disc_method: int, times, dfs, infl_method: int, T, b, fixed, book, per_trade=False):
    """PVs of a YoY swap book under scenario PAIRS (adr_yoy_scenario_pv, blocking): discount rows ``dfs`` [S, K] or one
    shared row [K] on the knots ``times``, breakeven rows ``b`` [S, P] or one shared row [P] on the pillars ``T``.
    ``fixed``: ``(fix_off, fix_tp, fix_pay)`` (`compile_yoy_fixed_legs`) or None; ``book``: ``cpn_off`` and the fields
    YOY_FIELDS (`compile_yoy_coupons`) or None.  Returns ``book_pv`` [S] and, with ``per_trade``, ``pv`` [S, n]."""
    return _yoy_scenario_call(load().adr_yoy_scenario_pv, (ctx._h,), (), disc_method, times, dfs, infl_method, T, b, fixed,
                              book, per_trade)


def yoy_scenario_pv_host(disc_method: int, times, dfs, infl_method: int, T, b, fixed, book, per_trade=False, n_threads=0):
    """`yoy_scenario_pv` on the CPU (adr_yoy_scenario_pv_host): the same per-coupon arithmetic and the same order of the
    book sum; no GPU needed."""
    return _yoy_scenario_call(load().adr_yoy_scenario_pv_host, (), (int(n_threads),), disc_method, times, dfs, infl_method,
                              T, b, fixed, book, per_trade)


def yoy_scenario_pv_work(n_swaps: int, n_scenarios: int) -> int:
    """Doubles of scratch `yoy_scenario_pv_dev` needs."""
    return int(load().adr_yoy_scenario_pv_work(int(n_swaps), int(n_scenarios)))


def yoy_scenario_pv_dev(ctx: Context, disc_method: int, K: int, S_disc: int, infl_method: int, P: int, S_infl: int, S: int,
                        n_swaps: int, n_fix: int, n_coupons: int, ptrs, book_ptr: int, work_ptr: int, pv_ptr: int = 0,
                        stream=0):
    """Non-blocking form (adr_yoy_scenario_pv_dev): ``ptrs`` maps ``times`` [K], ``dfs`` [S_disc, K], ``T`` [P], ``b``
    [S_infl, P], ``fix_off``, ``fix_tp``, ``fix_pay``, ``cpn_off`` and ``cpn`` to device pointers (integers; the value
    arrays of an empty leg may be 0); outputs ``book_pv`` [S] and ``pv`` [n, S] (swap-major; 0: not wanted);
    `yoy_scenario_pv_work` doubles of scratch."""
    g = _dev_of(ptrs)
    _check(load().adr_yoy_scenario_pv_dev(ctx._h, int(disc_method), int(K), g("times"), int(S_disc), g("dfs"), int(infl_method),
                                          int(P), g("T"), int(S_infl), g("b"), int(S), int(n_swaps), int(n_fix), g("fix_off"),
                                          g("fix_tp"), g("fix_pay"), int(n_coupons), g("cpn_off"), g("cpn"), _dev(pv_ptr),
                                          _dev(book_ptr), _dev(work_ptr), _vp(stream or None)), "adr_yoy_scenario_pv_dev")


def _xccy_scenario_curves(times_f, dfs_f, times_x, dfs_x):
    """The two curve groups of adr_xccy_scenario_pv from ``dfs_f`` [S, K_f] or [K_f] and ``dfs_x`` [S, K_x] or [K_x], and S."""
    times_f, dfs_f = _scenario_curves(times_f, dfs_f)
    times_x, dfs_x = _scenario_curves(times_x, dfs_x)
    S = max(dfs_f.shape[0], dfs_x.shape[0])
    if dfs_f.shape[0] not in (1, S) or dfs_x.shape[0] not in (1, S):
        raise LibError(f"{dfs_f.shape[0]} foreign rows and {dfs_x.shape[0]} XCCY rows: each must be one shared row or one row per "
                       "scenario")
    return times_f, dfs_f, times_x, dfs_x, S


def _xccy_scenario_call(fn, head, trades, tail, for_method, times_f, dfs_f, x_method, times_x, dfs_x, n, per_trade, *sub_off):
    """The four blocking and host XCCY entries: ``head`` the context or nothing, ``trades`` the handle or the host arrays,
    ``tail`` ``n_threads`` or nothing, ``sub_off`` given for the sub-book entries."""
    times_f, dfs_f, times_x, dfs_x, S = _xccy_scenario_curves(times_f, dfs_f, times_x, dfs_x)
    sub = _sub_offsets(*sub_off) if sub_off else None
    args = [*head, *_curve_args(for_method, times_f, dfs_f), *_curve_args(x_method, times_x, dfs_x), S, *trades]
    return _scenario_call(fn, args, n, S, per_trade, sub, tail)


def xccy_scenario_pv(ctx: Context, for_method: int, times_f, dfs_f, x_method: int, times_x, dfs_x, legs: DeviceTrades,
                     per_trade=False):
    """PVs of the foreign legs of a cross-currency book under scenario PAIRS (adr_xccy_scenario_pv, blocking): foreign OIS
    rows ``dfs_f`` [S, K_f] or one shared row on the knots ``times_f`` (the forwards), XCCY rows ``dfs_x`` [S, K_x] or one
    shared row on ``times_x`` (the discount factors); ``legs``: the uploaded foreign-leg batch (`compile_xccy_legs`).
    Returns ``book_pv`` [S] and, with ``per_trade``, ``pv`` [S, n], in FOREIGN currency."""
    return _xccy_scenario_call(load().adr_xccy_scenario_pv, (ctx._h,), (legs._h,), (), for_method, times_f, dfs_f, x_method,
                               times_x, dfs_x, legs.n_trades, per_trade)


def xccy_scenario_pv_host(for_method: int, times_f, dfs_f, x_method: int, times_x, dfs_x, batch, per_trade=False, n_threads=0):
    """`xccy_scenario_pv` on the CPU (adr_xccy_scenario_pv_host) for a `TradeBatch`: the same per-coupon arithmetic and the
    same order of the book sum; no GPU needed."""
    arrays = _batch_arrays(batch)
    return _xccy_scenario_call(load().adr_xccy_scenario_pv_host, (), _batch_args(*arrays), (int(n_threads),), for_method, times_f,
                               dfs_f, x_method, times_x, dfs_x, arrays[0], per_trade)


def xccy_scenario_pv_work(n_trades: int, n_scenarios: int) -> int:
    """Doubles of scratch `xccy_scenario_pv_dev` needs."""
    return int(load().adr_xccy_scenario_pv_work(int(n_trades), int(n_scenarios)))


def _xccy_dev_curves(for_method, K_f, S_f, x_method, K_x, S_x, ptrs):
    g = _dev_of(ptrs)
    return [int(for_method), int(K_f), g("times_f"), int(S_f), g("dfs_f"), int(x_method), int(K_x), g("times_x"), int(S_x),
            g("dfs_x")]


def xccy_scenario_pv_dev(ctx: Context, for_method: int, K_f: int, S_f: int, x_method: int, K_x: int, S_x: int, S: int,
                         legs: DeviceTrades, ptrs, book_ptr: int, work_ptr: int, pv_ptr: int = 0, stream=0):
    """Non-blocking form (adr_xccy_scenario_pv_dev): ``ptrs`` maps ``times_f`` [K_f], ``dfs_f`` [S_f, K_f], ``times_x`` [K_x]
    and ``dfs_x`` [S_x, K_x] to device pointers (integers); outputs ``book_pv`` [S] and ``pv`` [n, S] (trade-major; 0: not
    wanted); `xccy_scenario_pv_work` doubles of scratch."""
    _check(load().adr_xccy_scenario_pv_dev(ctx._h, *_xccy_dev_curves(for_method, K_f, S_f, x_method, K_x, S_x, ptrs), int(S),
                                           legs._h, _dev(pv_ptr), _dev(book_ptr), _dev(work_ptr), _vp(stream or None)),
           "adr_xccy_scenario_pv_dev")


CREDIT_MAX_BUCKETS = 32                                     # ADR_CREDIT_MAX_BUCKETS


def _credit_spread_inputs(dz, z, bucket, fix_tau, flt_tau, n, n_fix, n_flt):
    """The spread side of adr_credit_scenario_pv: ``dz`` [S, G], [G] or None (no buckets), ``z`` [n], ``bucket`` [n]
    (int32, -1: not shocked), ``fix_tau`` / ``flt_tau`` one spread time per fixed flow / float coupon of the batch."""
    dz = np.zeros((1, 0)) if dz is None else _f64(np.atleast_2d(dz))
    if dz.ndim != 2:
        raise LibError(f"dz must have shape [n_scenarios, n_buckets] or [n_buckets], not {list(dz.shape)}")
    z = _f64(z).reshape(-1)
    bucket = np.ascontiguousarray(bucket, dtype=np.int32).reshape(-1)
    fix_tau, flt_tau = _f64(fix_tau).reshape(-1), _f64(flt_tau).reshape(-1)
    if z.size != n or bucket.size != n:
        raise LibError(f"z and bucket need one entry per trade ({n}), not {z.size} and {bucket.size}")
    if fix_tau.size != n_fix or flt_tau.size != n_flt:
        raise LibError(f"fix_tau / flt_tau need one entry per fixed flow ({n_fix}) / float coupon ({n_flt}), not "
                       f"{fix_tau.size} / {flt_tau.size}")
    return dz, z, bucket, fix_tau, flt_tau


def _credit_counts(n_disc, n_spr):
    S = max(n_disc, n_spr)
    if n_disc not in (1, S) or n_spr not in (1, S):
        raise LibError(f"{n_disc} discount rows and {n_spr} spread-shock rows: each must be one shared row or one row per "
                       "scenario")
    return S


def _credit_call(fn, ctx, method, times, dfs, dz, trades, z, bucket, fix_tau, flt_tau, per_trade, *sub_off):
    """The two blocking credit entries on host curves and an uploaded batch; ``sub_off`` given for the sub-book entry."""
    times, dfs = _scenario_curves(times, dfs)
    sub = _sub_offsets(*sub_off) if sub_off else None
    n = trades.n_trades
    dz, *per = _credit_spread_inputs(dz, z, bucket, fix_tau, flt_tau, n, np.size(fix_tau), np.size(flt_tau))
    S = _credit_counts(dfs.shape[0], dz.shape[0])
    args = [ctx._h] + _curve_args(method, times, dfs) + _spread_args(dz) + [S, trades._h] + _credit_trade_args(*per, counts=True)
    return _scenario_call(fn, args, n, S, per_trade, sub)


def _credit_set_call(fn, ctx, curve_set, dz, trades, z, bucket, fix_tau, flt_tau, per_trade, *sub_off):
    """The same on the curves of a `CurveSet`."""
    sub = _sub_offsets(*sub_off) if sub_off else None
    n, S = trades.n_trades, len(curve_set)
    dz, *per = _credit_spread_inputs(dz, z, bucket, fix_tau, flt_tau, n, np.size(fix_tau), np.size(flt_tau))
    if dz.shape[0] not in (1, S):
        raise LibError(f"{dz.shape[0]} spread-shock rows for a set of {S} curves: one shared row or one row per curve")
    args = [ctx._h, curve_set._h] + _spread_args(dz) + [trades._h] + _credit_trade_args(*per, counts=True)
    return _scenario_call(fn, args, n, S, per_trade, sub)


def _credit_host_call(fn, method, times, dfs, dz, batch, z, bucket, fix_tau, flt_tau, per_trade, n_threads, *sub_off):
    """The same on the CPU for a `TradeBatch`."""
    times, dfs = _scenario_curves(times, dfs)
    sub = _sub_offsets(*sub_off) if sub_off else None
    arrays = _batch_arrays(batch)
    n, a = arrays[0], arrays[3]
    dz, *per = _credit_spread_inputs(dz, z, bucket, fix_tau, flt_tau, n, a["fix_tp"].size, a["flt_tp"].size)
    S = _credit_counts(dfs.shape[0], dz.shape[0])
    args = _curve_args(method, times, dfs) + _spread_args(dz) + [S] + _batch_args(*arrays) + _credit_trade_args(*per, counts=False)
    return _scenario_call(fn, args, n, S, per_trade, sub, (int(n_threads),))


def credit_scenario_pv(ctx: Context, method: int, times, dfs, dz, trades: DeviceTrades, z, bucket, fix_tau, flt_tau,
                       per_trade=False):
    """PVs of an uploaded batch under scenario PAIRS (adr_credit_scenario_pv, blocking): discount rows ``dfs`` [S, K] or
    one shared row [K] on the knots ``times``, spread shocks ``dz`` [S, G], one shared row [G] or None; per trade the
    spread ``z`` and the bucket (-1: not shocked), per flow the spread times in the batch's flow order.  Returns
    ``book_pv`` [S] and, with ``per_trade``, ``pv`` [S, n]."""
    return _credit_call(load().adr_credit_scenario_pv, ctx, method, times, dfs, dz, trades, z, bucket, fix_tau, flt_tau,
                        per_trade)


def credit_scenario_pv_set(ctx: Context, curve_set: CurveSet, dz, trades: DeviceTrades, z, bucket, fix_tau, flt_tau,
                           per_trade=False):
    """`credit_scenario_pv` on the curves of a `CurveSet`, read in place where `curve_set_arrays` finds them
    (adr_credit_scenario_pv_set): one scenario per curve of the set; ``dz`` has that many rows, one shared row or is None."""
    return _credit_set_call(load().adr_credit_scenario_pv_set, ctx, curve_set, dz, trades, z, bucket, fix_tau, flt_tau,
                            per_trade)


def credit_scenario_pv_host(method: int, times, dfs, dz, batch, z, bucket, fix_tau, flt_tau, per_trade=False, n_threads=0):
    """`credit_scenario_pv` on the CPU (adr_credit_scenario_pv_host) for a `TradeBatch`: the same per-coupon arithmetic
    and the same order of the book sum; no GPU needed."""
    return _credit_host_call(load().adr_credit_scenario_pv_host, method, times, dfs, dz, batch, z, bucket, fix_tau, flt_tau,
                             per_trade, n_threads)


def credit_scenario_pv_work(n_trades: int, n_scenarios: int) -> int:
    """Doubles of scratch `credit_scenario_pv_dev` needs."""
    return int(load().adr_credit_scenario_pv_work(int(n_trades), int(n_scenarios)))


def credit_scenario_pv_dev(ctx: Context, method: int, K: int, S_disc: int, G: int, S_spr: int, S: int, trades: DeviceTrades,
                           n_fix: int, n_flt: int, ptrs, book_ptr: int, work_ptr: int, pv_ptr: int = 0, stream=0):
    """Non-blocking form (adr_credit_scenario_pv_dev): ``ptrs`` maps ``times`` [K], ``dfs`` [S_disc, K], ``dz`` [S_spr, G]
    (0 when G = 0), ``z`` [n], ``bucket`` [n] (int32), ``fix_tau`` [n_fix] and ``flt_tau`` [n_flt] to device pointers
    (integers); outputs ``book_pv`` [S] and ``pv`` [n, S] (trade-major; 0: not wanted); `credit_scenario_pv_work`
    doubles of scratch."""
    g = _dev_of(ptrs)
    _check(load().adr_credit_scenario_pv_dev(ctx._h, int(method), int(K), g("times"), int(S_disc), g("dfs"), int(G), int(S_spr),
                                             g("dz"), int(S), trades._h, g("z"), g("bucket"), int(n_fix), g("fix_tau"),
                                             int(n_flt), g("flt_tau"), _dev(pv_ptr), _dev(book_ptr), _dev(work_ptr),
                                             _vp(stream or None)), "adr_credit_scenario_pv_dev")


_default_ctx = {}


# ---------------------------------------------------------------------------------------------------------- sub-books
SCENARIO_TAIL_MAX = 16384


def _sub_offsets(sub_off):
    sub_off = np.ascontiguousarray(sub_off, dtype=np.int64).reshape(-1)
    if sub_off.size < 2:
        raise LibError("sub_off needs B + 1 entries for B >= 1 sub-books")
    return sub_off, sub_off.size - 1


def scenario_subbook_plan(n_trades: int, sub_off) -> np.ndarray:
    """The chunk plan of the sub-books ``sub_off [B + 1]`` (adr_scenario_subbook_plan): the int64 array the ``_dev``
    entries read on the device.  Offsets that do not run from 0 to ``n_trades`` or that decrease raise `LibError`."""
    sub_off, B = _sub_offsets(sub_off)
    size = _check(load().adr_scenario_subbook_plan(int(n_trades), B, _ptr(sub_off, _i64p), None), "adr_scenario_subbook_plan")
    plan = np.empty(size, dtype=np.int64)
    _check(load().adr_scenario_subbook_plan(int(n_trades), B, _ptr(sub_off, _i64p), _ptr(plan, _i64p)), "adr_scenario_subbook_plan")
    return plan


def scenario_subbook_work(n_trades: int, n_sub_books: int, n_scenarios: int) -> int:
    """Doubles of scratch the sub-book ``_dev`` entries need."""
    return int(load().adr_scenario_subbook_work(int(n_trades), int(n_sub_books), int(n_scenarios)))


def scenario_subbook_pv(ctx: Context, method: int, times, dfs, trades: DeviceTrades, sub_off, per_trade=False):
    """`scenario_pv` per sub-book in one launch (adr_scenario_subbook_pv, blocking): sub-book ``b`` holds the trades
    ``sub_off[b] .. sub_off[b + 1]``.  ``sub_pv [B, S]`` and, with ``per_trade``, ``pv [S, n]``."""
    times, dfs = _scenario_curves(times, dfs)
    sub = _sub_offsets(sub_off)
    return _scenario_call(load().adr_scenario_subbook_pv, [ctx._h] + _curve_args(method, times, dfs) + [trades._h],
                          trades.n_trades, dfs.shape[0], per_trade, sub)


def scenario_subbook_pv_set(ctx: Context, curve_set: CurveSet, trades: DeviceTrades, sub_off, per_trade=False):
    """`scenario_subbook_pv` on the curves of a `CurveSet`, read where the device builder left them."""
    sub = _sub_offsets(sub_off)
    return _scenario_call(load().adr_scenario_subbook_pv_set, [ctx._h, curve_set._h, trades._h], trades.n_trades,
                          len(curve_set), per_trade, sub)


def scenario_subbook_pv_host(method: int, times, dfs, batch, sub_off, per_trade=False, n_threads=0):
    """`scenario_subbook_pv` on the CPU (adr_scenario_subbook_pv_host) for a `TradeBatch`: the same arithmetic and the
    same order of every sub-book's sum; no GPU needed."""
    times, dfs = _scenario_curves(times, dfs)
    sub = _sub_offsets(sub_off)
    arrays = _batch_arrays(batch)
    return _scenario_call(load().adr_scenario_subbook_pv_host, _curve_args(method, times, dfs) + _batch_args(*arrays),
                          arrays[0], dfs.shape[0], per_trade, sub, (int(n_threads),))


def scenario_subbook_pv_dev(ctx: Context, method: int, K: int, times_ptr: int, S: int, dfs_ptr: int, trades: DeviceTrades,
                            B: int, plan_ptr: int, sub_pv_ptr: int, work_ptr: int, pv_ptr: int = 0, stream=0):
    """Non-blocking form (adr_scenario_subbook_pv_dev): device pointers (integers) of ``times`` [K], ``dfs`` [S, K], the
    uploaded `scenario_subbook_plan`, the outputs ``sub_pv`` [B, S] and ``pv`` [n, S] (0: not wanted) and
    `scenario_subbook_work` doubles of scratch."""
    _check(load().adr_scenario_subbook_pv_dev(ctx._h, int(method), int(K), _dev(times_ptr), int(S), _dev(dfs_ptr), trades._h,
                                              int(B), _dev(plan_ptr), _dev(pv_ptr), _dev(sub_pv_ptr), _dev(work_ptr),
                                              _vp(stream or None)), "adr_scenario_subbook_pv_dev")


def scenario_subbook_var_es(ctx: Context, method: int, times, dfs, trades: DeviceTrades, sub_off, k: int, base_col: int = -1):
    """``(var [B], es [B])`` of the sub-books' rows, the launch and the tail kernel in one chain
    (adr_scenario_subbook_var_es): the ``[B, S]`` rows stay on the device.  ``base_col`` and ``k``: see `scenario_tail`."""
    times, dfs = _scenario_curves(times, dfs)
    sub_off, B = _sub_offsets(sub_off)
    var, es = np.empty(B), np.empty(B)
    _check(load().adr_scenario_subbook_var_es(ctx._h, *_curve_args(method, times, dfs), trades._h, B, _ptr(sub_off, _i64p),
                                              int(base_col), int(k), _ptr(var), _ptr(es)), "adr_scenario_subbook_var_es")
    return var, es


def credit_scenario_subbook_pv(ctx: Context, method: int, times, dfs, dz, trades: DeviceTrades, z, bucket, fix_tau, flt_tau,
                               sub_off, per_trade=False):
    """`credit_scenario_pv` per sub-book in one launch (adr_credit_scenario_subbook_pv, blocking): ``sub_pv [B, S]`` and,
    with ``per_trade``, ``pv [S, n]``."""
    return _credit_call(load().adr_credit_scenario_subbook_pv, ctx, method, times, dfs, dz, trades, z, bucket, fix_tau,
                        flt_tau, per_trade, sub_off)


def credit_scenario_subbook_pv_set(ctx: Context, curve_set: CurveSet, dz, trades: DeviceTrades, z, bucket, fix_tau, flt_tau,
                                   sub_off, per_trade=False):
    """`credit_scenario_subbook_pv` on the curves of a `CurveSet` (adr_credit_scenario_subbook_pv_set)."""
    return _credit_set_call(load().adr_credit_scenario_subbook_pv_set, ctx, curve_set, dz, trades, z, bucket, fix_tau,
                            flt_tau, per_trade, sub_off)


def credit_scenario_subbook_pv_host(method: int, times, dfs, dz, batch, z, bucket, fix_tau, flt_tau, sub_off, per_trade=False,
                                    n_threads=0):
    """`credit_scenario_subbook_pv` on the CPU (adr_credit_scenario_subbook_pv_host) for a `TradeBatch`."""
    return _credit_host_call(load().adr_credit_scenario_subbook_pv_host, method, times, dfs, dz, batch, z, bucket, fix_tau,
                             flt_tau, per_trade, n_threads, sub_off)


def credit_scenario_subbook_pv_dev(ctx: Context, method: int, K: int, S_disc: int, G: int, S_spr: int, S: int,
                                   trades: DeviceTrades, n_fix: int, n_flt: int, B: int, ptrs, sub_pv_ptr: int, work_ptr: int,
                                   pv_ptr: int = 0, stream=0):
    """Non-blocking form (adr_credit_scenario_subbook_pv_dev): ``ptrs`` as `credit_scenario_pv_dev` takes them plus
    ``plan``, the uploaded `scenario_subbook_plan`; outputs ``sub_pv`` [B, S] and ``pv`` [n, S] (0: not wanted);
    `scenario_subbook_work` doubles of scratch."""
    g = _dev_of(ptrs)
    _check(load().adr_credit_scenario_subbook_pv_dev(ctx._h, int(method), int(K), g("times"), int(S_disc), g("dfs"), int(G),
                                                     int(S_spr), g("dz"), int(S), trades._h, g("z"), g("bucket"), int(n_fix),
                                                     g("fix_tau"), int(n_flt), g("flt_tau"), int(B), g("plan"), _dev(pv_ptr),
                                                     _dev(sub_pv_ptr), _dev(work_ptr), _vp(stream or None)),
           "adr_credit_scenario_subbook_pv_dev")


def _tail_rows(rows):
    rows = _f64(np.atleast_2d(rows))
    if rows.ndim != 2 or rows.shape[0] < 1 or rows.shape[1] < 1:
        raise LibError(f"rows must have shape [n_rows, n_columns], not {list(rows.shape)}")
    return rows


def _tail_call(fn, head, rows, k, base_col):
    rows = _tail_rows(rows)
    var, es = np.empty(rows.shape[0]), np.empty(rows.shape[0])
    _check(fn(*head, rows.shape[0], rows.shape[1], _ptr(rows), int(base_col), int(k), _ptr(var), _ptr(es)), fn.__name__)
    return var, es


def scenario_tail(ctx: Context, rows, k: int, base_col: int = -1):
    """``(var [B], es [B])`` of ``rows [B, S]`` on the device (adr_scenario_tail, blocking): minus the ``k``-th smallest
    P&L, and minus the mean of the ``k`` smallest.  ``base_col >= 0``: the P&L is every other column minus that one."""
    return _tail_call(load().adr_scenario_tail, (ctx._h,), rows, k, base_col)


def scenario_tail_host(rows, k: int, base_col: int = -1):
    """`scenario_tail` on the CPU (adr_scenario_tail_host): the same sums in the same order, hence the same bits."""
    return _tail_call(load().adr_scenario_tail_host, (), rows, k, base_col)


def scenario_tail_dev(ctx: Context, B: int, S_tot: int, rows_ptr: int, k: int, var_ptr: int, es_ptr: int, base_col: int = -1,
                      stream=0):
    """Non-blocking form (adr_scenario_tail_dev): device pointers of ``rows`` [B, S_tot], ``var`` [B] and ``es`` [B]."""
    _check(load().adr_scenario_tail_dev(ctx._h, int(B), int(S_tot), _dev(rows_ptr), int(base_col), int(k), _dev(var_ptr),
                                        _dev(es_ptr), _vp(stream or None)), "adr_scenario_tail_dev")


def yoy_scenario_subbook_pv(ctx: Context, disc_method: int, times, dfs, infl_method: int, T, b, fixed, book, sub_off,
                            per_trade=False):
    """`yoy_scenario_pv` per sub-book in one launch (adr_yoy_scenario_subbook_pv, blocking): sub-book ``b`` holds the swaps
    ``sub_off[b] .. sub_off[b + 1]``.  ``sub_pv [B, S]`` and, with ``per_trade``, ``pv [S, n]``."""
    return _yoy_scenario_call(load().adr_yoy_scenario_subbook_pv, (ctx._h,), (), disc_method, times, dfs, infl_method, T, b,
                              fixed, book, per_trade, sub_off)


def yoy_scenario_subbook_pv_host(disc_method: int, times, dfs, infl_method: int, T, b, fixed, book, sub_off, per_trade=False,
                                 n_threads=0):
    """`yoy_scenario_subbook_pv` on the CPU (adr_yoy_scenario_subbook_pv_host): the same arithmetic and the same order of
    every sub-book's sum; no GPU needed."""
    return _yoy_scenario_call(load().adr_yoy_scenario_subbook_pv_host, (), (int(n_threads),), disc_method, times, dfs,
                              infl_method, T, b, fixed, book, per_trade, sub_off)


def yoy_scenario_subbook_pv_dev(ctx: Context, disc_method: int, K: int, S_disc: int, infl_method: int, P: int, S_infl: int,
                                S: int, n_swaps: int, n_fix: int, n_coupons: int, B: int, ptrs, sub_pv_ptr: int, work_ptr: int,
                                pv_ptr: int = 0, stream=0):
    """Non-blocking form (adr_yoy_scenario_subbook_pv_dev): ``ptrs`` as `yoy_scenario_pv_dev` takes them plus ``plan``, the
    uploaded `scenario_subbook_plan`; outputs ``sub_pv`` [B, S] and ``pv`` [n, S] (0: not wanted); `scenario_subbook_work`
    doubles of scratch."""
    g = _dev_of(ptrs)
    _check(load().adr_yoy_scenario_subbook_pv_dev(ctx._h, int(disc_method), int(K), g("times"), int(S_disc), g("dfs"),
                                                  int(infl_method), int(P), g("T"), int(S_infl), g("b"), int(S), int(n_swaps),
                                                  int(n_fix), g("fix_off"), g("fix_tp"), g("fix_pay"), int(n_coupons),
                                                  g("cpn_off"), g("cpn"), int(B), g("plan"), _dev(pv_ptr), _dev(sub_pv_ptr),
                                                  _dev(work_ptr), _vp(stream or None)), "adr_yoy_scenario_subbook_pv_dev")


SCENARIO_ALLOC_MAX = 8192                                   # ADR_SCENARIO_ALLOC_MAX


def xccy_scenario_subbook_pv(ctx: Context, for_method: int, times_f, dfs_f, x_method: int, times_x, dfs_x, legs: DeviceTrades,
                             sub_off, per_trade=False):
    """`xccy_scenario_pv` per sub-book in one launch (adr_xccy_scenario_subbook_pv, blocking): sub-book ``b`` holds the
    trades ``sub_off[b] .. sub_off[b + 1]``.  Returns ``sub_pv`` [B, S] and, with ``per_trade``, ``pv`` [S, n]."""
    return _xccy_scenario_call(load().adr_xccy_scenario_subbook_pv, (ctx._h,), (legs._h,), (), for_method, times_f, dfs_f,
                               x_method, times_x, dfs_x, legs.n_trades, per_trade, sub_off)


def xccy_scenario_subbook_pv_host(for_method: int, times_f, dfs_f, x_method: int, times_x, dfs_x, batch, sub_off,
                                  per_trade=False, n_threads=0):
    """`xccy_scenario_subbook_pv` on the CPU (adr_xccy_scenario_subbook_pv_host): the same arithmetic and the same order of
    every sum; no GPU needed."""
    arrays = _batch_arrays(batch)
    return _xccy_scenario_call(load().adr_xccy_scenario_subbook_pv_host, (), _batch_args(*arrays), (int(n_threads),), for_method,
                               times_f, dfs_f, x_method, times_x, dfs_x, arrays[0], per_trade, sub_off)


def xccy_scenario_subbook_pv_dev(ctx: Context, for_method: int, K_f: int, S_f: int, x_method: int, K_x: int, S_x: int, S: int,
                                 legs: DeviceTrades, B: int, ptrs, sub_pv_ptr: int, work_ptr: int, pv_ptr: int = 0, stream=0):
    """Non-blocking form (adr_xccy_scenario_subbook_pv_dev): ``ptrs`` as `xccy_scenario_pv_dev` takes them plus ``plan``, the
    uploaded `scenario_subbook_plan`; output ``sub_pv`` [B, S]; `scenario_subbook_work` doubles of scratch."""
    _check(load().adr_xccy_scenario_subbook_pv_dev(ctx._h, *_xccy_dev_curves(for_method, K_f, S_f, x_method, K_x, S_x, ptrs),
                                                   int(S), legs._h, int(B), _dev_of(ptrs)("plan"), _dev(pv_ptr), _dev(sub_pv_ptr),
                                                   _dev(work_ptr), _vp(stream or None)), "adr_xccy_scenario_subbook_pv_dev")


def _alloc_call(fn, head, rows, k, base_col):
    rows = _tail_rows(rows)
    B = rows.shape[0]
    tot, comp_var, comp_es = np.empty(2), np.empty(B), np.empty(B)
    _check(fn(*head, B, rows.shape[1], _ptr(rows), int(base_col), int(k), _ptr(tot[0:1]), _ptr(tot[1:2]), _ptr(comp_var),
              _ptr(comp_es)), fn.__name__)
    return {"var": float(tot[0]), "es": float(tot[1]), "comp_var": comp_var, "comp_es": comp_es}


def scenario_tail_alloc(ctx: Context, rows, k: int, base_col: int = -1):
    """The firm's tail and its Euler allocation to the rows of ``rows [B, S]`` on the device (adr_scenario_tail_alloc,
    blocking): ``var`` and ``es`` of the column sums, and per row ``comp_var`` (its P&L in the firm's ``k``-th worst
    scenario, negated) and ``comp_es`` (minus its mean P&L over the firm's ``k`` worst scenarios)."""
    return _alloc_call(load().adr_scenario_tail_alloc, (ctx._h,), rows, k, base_col)


def scenario_tail_alloc_host(rows, k: int, base_col: int = -1):
    """`scenario_tail_alloc` on the CPU (adr_scenario_tail_alloc_host): the same sums in the same order, the same bits."""
    return _alloc_call(load().adr_scenario_tail_alloc_host, (), rows, k, base_col)


def scenario_tail_alloc_dev(ctx: Context, B: int, S_tot: int, rows_ptr: int, k: int, var_ptr: int, es_ptr: int,
                            comp_var_ptr: int, comp_es_ptr: int, work_ptr: int, base_col: int = -1, stream=0):
    """Non-blocking form (adr_scenario_tail_alloc_dev): device pointers of ``rows`` [B, S_tot], ``var`` [1], ``es`` [1],
    ``comp_var`` [B], ``comp_es`` [B] and ``S_tot`` doubles of scratch."""
    _check(load().adr_scenario_tail_alloc_dev(ctx._h, int(B), int(S_tot), _dev(rows_ptr), int(base_col), int(k), _dev(var_ptr),
                                              _dev(es_ptr), _dev(comp_var_ptr), _dev(comp_es_ptr), _dev(work_ptr),
                                              _vp(stream or None)), "adr_scenario_tail_alloc_dev")


# ------------------------------------------------------------------------------------------------- sub-book Greeks
def _request_mask(want_delta, want_gamma):
    return REQ_VALUE | (REQ_DELTA if want_delta else 0) | (REQ_GAMMA if want_gamma else 0)


def _ladder_rows(out, P):
    """``out [B, 1 + P + P P]`` as ``pv [B]``, ``delta [B, P]``, ``gamma [B, P, P]``."""
    return {"pv": out[:, 0].copy(), "delta": out[:, 1:1 + P].copy(), "gamma": out[:, 1 + P:].reshape(-1, P, P).copy()}


def ratio_flags_host(batch) -> np.ndarray:
    """``[n]`` bool: the trade has a ratio node - a float coupon that accrues and is not paid on its accrual end, or a
    per-coupon notional other than 1 (adr_trades_ratio_flags_host: the rule the upload applies)."""
    n, fo, lo, a, w = _batch_arrays(batch)
    out = np.zeros(n, dtype=np.uint8)
    _check(load().adr_trades_ratio_flags_host(n, _ptr(lo, _i64p), _ptr(a["flt_tp"]), _ptr(a["flt_te"]), _ptr(a["flt_alpha"]),
                                              _ptr(w), _ptr(out, C.POINTER(C.c_uint8))), "adr_trades_ratio_flags_host")
    return out.astype(bool)


def subbook_ladders(ctx: Context, curve: DeviceCurve, trades: DeviceTrades, sub_off, want_delta=True, want_gamma=True):
    """The PV, delta and gamma ladders of every sub-book of an uploaded batch from one launch chain (adr_subbook_ladders,
    blocking): sub-book ``b`` holds the trades ``sub_off[b] .. sub_off[b + 1]``.  Returns ``pv [B]``, ``delta [B, P]``,
    ``gamma [B, P, P]``; what was not requested is zeros.  A batch with a ratio node (payment lag, per-coupon notional)
    raises `LibError` (ADR_ERR_UNSUPPORTED) naming the trade."""
    sub_off, B = _sub_offsets(sub_off)
    P = curve.n_pillars
    out = np.empty((B, 1 + P + P * P))
    _check(load().adr_subbook_ladders(ctx._h, curve._h, trades._h, B, _ptr(sub_off, _i64p), _request_mask(want_delta, want_gamma),
                                      _ptr(out)), "adr_subbook_ladders")
    return _ladder_rows(out, P)


def subbook_ladders_host(interp_method: int, times, dfs, jac, hess, batch, sub_off, want_delta=True, want_gamma=True):
    """`subbook_ladders` on the CPU (adr_subbook_ladders_host) for a `TradeBatch` and the curve arrays `DeviceCurve`
    takes: the same node and projection code, chunks and summation orders; no GPU needed."""
    sub_off, B = _sub_offsets(sub_off)
    times, dfs, jac, hess, K, P = _curve_arrays(times, dfs, jac, hess, shapes=True)
    out = np.empty((B, 1 + P + P * P))
    _check(load().adr_subbook_ladders_host(int(interp_method), K, P, _ptr(times), _ptr(dfs), _ptr(jac), _ptr(hess),
                                           *_batch_args(*_batch_arrays(batch)), B, _ptr(sub_off, _i64p),
                                           _request_mask(want_delta, want_gamma), _ptr(out)), "adr_subbook_ladders_host")
    return _ladder_rows(out, P)


def subbook_ladders_work(curve: DeviceCurve, n_trades: int, n_sub_books: int, want_gamma=True):
    """``(doubles of scratch, rows of chunk records it holds)`` of `subbook_ladders_dev` (adr_subbook_ladders_work)."""
    chunks = C.c_int64(0)
    work = load().adr_subbook_ladders_work(curve._h, int(n_trades), int(n_sub_books), _request_mask(True, want_gamma),
                                           C.cast(C.byref(chunks), _i64p))
    if work <= 0:
        raise LibError("adr_subbook_ladders_work: a curve, at least one trade and at least one sub-book are needed")
    return int(work), int(chunks.value)


def subbook_ladders_dev(ctx: Context, curve: DeviceCurve, trades: DeviceTrades, B: int, plan_ptr: int, mask: int, out_ptr: int,
                        work_ptr: int, stream=0):
    """Non-blocking form (adr_subbook_ladders_dev): device pointers (integers) of the uploaded `scenario_subbook_plan` -
    built once per (batch, sub_off) and reused -, the output ``[B, 1 + P + P P]`` and `subbook_ladders_work` doubles of
    scratch."""
    _check(load().adr_subbook_ladders_dev(ctx._h, curve._h, trades._h, int(B), _dev(plan_ptr), int(mask), _dev(out_ptr),
                                          _dev(work_ptr), _vp(stream or None)), "adr_subbook_ladders_dev")


# ------------------------------------------------------------------------------------------ credit sub-book Greeks
def _credit_ladder_rows(out, P, G):
    """``out [B, 1 + Q + Q Q]`` (Q = P + G) as its blocks; ``ladders`` is ``out`` itself, what `ladder_pnl` takes beside
    shock rows ``[x_bp (P), dz * 1e4 (G)]``."""
    Q = P + G
    g = out[:, 1 + Q:].reshape(-1, Q, Q)
    diag = np.arange(P, Q)
    return {"pv": out[:, 0].copy(), "delta": out[:, 1:1 + P].copy(), "gamma": g[:, :P, :P].copy(), "cs01": out[:, 1 + P:1 + Q].copy(),
            "spread_gamma": g[:, diag, diag].copy(), "cross_gamma": g[:, P:, :P].copy(), "ladders": out}


def _credit_ladder_inputs(z, bucket, fix_tau, flt_tau, G, n, n_fix, n_flt):
    _, z, bucket, fix_tau, flt_tau = _credit_spread_inputs(None, z, bucket, fix_tau, flt_tau, n, n_fix, n_flt)
    return z, bucket, fix_tau, flt_tau, int(G)


def credit_subbook_cells(bucket, sub_off):
    """The (sub-book, bucket) cells of a batch ordered by (sub-book, bucket), as `credit_subbook_ladders_dev` takes them:
    ``(cell_off [C + 1], desk_cell_off [B + 1], cell_bucket [C])`` - only cells that hold trades exist, and
    ``scenario_subbook_plan(n, cell_off)`` is the chunk plan over them."""
    sub_off, B = _sub_offsets(sub_off)
    bucket = np.ascontiguousarray(bucket, dtype=np.int32).reshape(-1)
    n = bucket.size
    if sub_off[0] != 0 or sub_off[-1] != n or np.any(np.diff(sub_off) < 0):
        raise LibError(f"sub_off must run from 0 to the trade count {n} without decreasing")
    desk = np.repeat(np.arange(B, dtype=np.int64), np.diff(sub_off))
    back = np.nonzero((desk[1:] == desk[:-1]) & (bucket[1:] < bucket[:-1]))[0]
    if back.size:
        i = int(back[0]) + 1
        raise LibError(f"sub-book {int(desk[i])} is not ordered by bucket: trade {i} (bucket {int(bucket[i])}) follows bucket "
                       f"{int(bucket[i - 1])}")
    start = np.ones(n, dtype=bool)
    start[1:] = (desk[1:] != desk[:-1]) | (bucket[1:] != bucket[:-1])
    first = np.nonzero(start)[0]
    cell_off = np.concatenate([first, [n]]).astype(np.int64)
    desk_cell_off = np.searchsorted(desk[first], np.arange(B + 1), side="left").astype(np.int64)
    return cell_off, desk_cell_off, bucket[first].copy()


def credit_subbook_ladders(ctx: Context, curve: DeviceCurve, trades: DeviceTrades, z, bucket, fix_tau, flt_tau, G: int, sub_off,
                           want_delta=True, want_gamma=True):
    """The ladders of every sub-book of an uploaded credit batch AT ITS SPREADS plus the spread Greeks per bucket, from one
    launch chain (adr_credit_subbook_ladders, blocking).  ``z [n]``, ``bucket [n]`` (int32, -1: none) and the spread times
    per flow as `credit_scenario_pv` takes them; the batch must be ordered by (sub-book, bucket).  Returns ``pv [B]``,
    ``delta [B, P]``, ``gamma [B, P, P]``, ``cs01 [B, G]``, ``spread_gamma [B, G]``, ``cross_gamma [B, G, P]`` and the
    augmented rows ``ladders [B, 1 + Q + Q Q]``, Q = P + G; what was not requested is zeros."""
    sub_off, B = _sub_offsets(sub_off)
    z, bucket, fix_tau, flt_tau, G = _credit_ladder_inputs(z, bucket, fix_tau, flt_tau, G, trades.n_trades, np.size(fix_tau),
                                                           np.size(flt_tau))
    P = curve.n_pillars
    Q = P + max(G, 0)
    out = np.empty((B, 1 + Q + Q * Q))
    _check(load().adr_credit_subbook_ladders(ctx._h, curve._h, trades._h, *_credit_trade_args(z, bucket, fix_tau, flt_tau, True), G,
                                             B, _ptr(sub_off, _i64p), _request_mask(want_delta, want_gamma), _ptr(out)),
           "adr_credit_subbook_ladders")
    return _credit_ladder_rows(out, P, G)


def credit_subbook_ladders_host(interp_method: int, times, dfs, jac, hess, batch, z, bucket, fix_tau, flt_tau, G: int, sub_off,
                                want_delta=True, want_gamma=True):
    """`credit_subbook_ladders` on the CPU (adr_credit_subbook_ladders_host) for a `TradeBatch` and the curve arrays
    `DeviceCurve` takes: the same node, sum and projection code, chunks and orders; no GPU needed."""
    sub_off, B = _sub_offsets(sub_off)
    times, dfs, jac, hess, K, P = _curve_arrays(times, dfs, jac, hess, shapes=True)
    arrays = _batch_arrays(batch)
    n, a = arrays[0], arrays[3]
    z, bucket, fix_tau, flt_tau, G = _credit_ladder_inputs(z, bucket, fix_tau, flt_tau, G, n, a["fix_tp"].size, a["flt_tp"].size)
    Q = P + max(G, 0)
    out = np.empty((B, 1 + Q + Q * Q))
    _check(load().adr_credit_subbook_ladders_host(int(interp_method), K, P, _ptr(times), _ptr(dfs), _ptr(jac), _ptr(hess),
                                                  *_batch_args(*arrays), *_credit_trade_args(z, bucket, fix_tau, flt_tau, False),
                                                  G, B, _ptr(sub_off, _i64p), _request_mask(want_delta, want_gamma), _ptr(out)),
           "adr_credit_subbook_ladders_host")
    return _credit_ladder_rows(out, P, G)


def credit_subbook_ladders_work(curve: DeviceCurve, n_trades: int, n_sub_books: int, n_cells: int, want_gamma=True):
    """``(doubles of scratch, rows of chunk records it holds)`` of `credit_subbook_ladders_dev`
    (adr_credit_subbook_ladders_work)."""
    chunks = C.c_int64(0)
    work = load().adr_credit_subbook_ladders_work(curve._h, int(n_trades), int(n_sub_books), int(n_cells),
                                                  _request_mask(True, want_gamma), C.cast(C.byref(chunks), _i64p))
    if work <= 0:
        raise LibError("adr_credit_subbook_ladders_work: a curve, at least one trade and sub-book and 1 .. n_trades cells are needed")
    return int(work), int(chunks.value)


def credit_subbook_ladders_dev(ctx: Context, curve: DeviceCurve, trades: DeviceTrades, n_fix: int, n_flt: int, G: int, B: int,
                               n_cells: int, ptrs, mask: int, out_ptr: int, work_ptr: int, stream=0):
    """Non-blocking form (adr_credit_subbook_ladders_dev): ``ptrs`` maps ``z`` [n], ``bucket`` [n] (int32), ``fix_tau``
    [n_fix], ``flt_tau`` [n_flt], ``cell_plan`` (`scenario_subbook_plan` over `credit_subbook_cells`' ``cell_off``),
    ``desk_cell_off`` [B + 1] and ``cell_bucket`` [C] (int32) to device pointers (integers); the output
    ``[B, 1 + Q + Q Q]`` and `credit_subbook_ladders_work` doubles of scratch."""
    g = _dev_of(ptrs)
    _check(load().adr_credit_subbook_ladders_dev(ctx._h, curve._h, trades._h, g("z"), g("bucket"), int(n_fix), g("fix_tau"),
                                                 int(n_flt), g("flt_tau"), int(G), int(B), int(n_cells), g("cell_plan"),
                                                 g("desk_cell_off"), g("cell_bucket"), int(mask), _dev(out_ptr), _dev(work_ptr),
                                                 _vp(stream or None)), "adr_credit_subbook_ladders_dev")


# --------------------------------------------------------------------------------------- inflation sub-book Greeks
def _yoy_ladder_rows(out, P, Pi):
    """``out [B, 1 + Q + Q Q]`` (Q = P + Pi) as its blocks; ``ladders`` is ``out`` itself, what `ladder_pnl` takes beside
    shock rows ``[x_bp (P), (b - b0) * 1e4 (Pi)]``."""
    Q = P + Pi
    g = out[:, 1 + Q:].reshape(-1, Q, Q)
    return {"pv": out[:, 0].copy(), "delta": out[:, 1:1 + P].copy(), "gamma": g[:, :P, :P].copy(),
            "infl_delta": out[:, 1 + P:1 + Q].copy(), "infl_gamma": g[:, P:, P:].copy(), "cross_gamma": g[:, P:, :P].copy(),
            "ladders": out}


def _yoy_ladder_inputs(T, b, fixed, book):
    """The inflation curve and the book as the YoY ladder entries take them: one breakeven row, both legs' arrays."""
    T, b = _f64(T).reshape(-1), _f64(b).reshape(-1)
    if b.shape != T.shape:
        raise LibError(f"b must hold one breakeven rate per pillar ({T.size}), not {list(b.shape)}")
    return (T, b) + _yoy_legs(fixed, book)


def yoy_subbook_ladders(ctx: Context, curve: DeviceCurve, infl_method: int, T, b, fixed, book, sub_off, want_delta=True,
                        want_gamma=True):
    """The augmented ladders of every sub-book of a YoY book from one launch chain (adr_yoy_subbook_ladders, blocking):
    ``curve`` the uploaded discount curve, ``(infl_method, T [Pi], b [Pi])`` the inflation curve, ``fixed`` and ``book`` as
    `yoy_scenario_subbook_pv` takes them.  Returns ``pv [B]``, ``delta [B, P]``, ``gamma [B, P, P]`` (discount), ``infl_delta
    [B, Pi]``, ``infl_gamma [B, Pi, Pi]`` (breakeven), ``cross_gamma [B, Pi, P]`` and the augmented rows ``ladders
    [B, 1 + Q + Q Q]``, Q = P + Pi; what was not requested is zeros."""
    sub_off, B = _sub_offsets(sub_off)
    T, b, fix_off, fix_tp, fix_pay, cpn_off, cpn = _yoy_ladder_inputs(T, b, fixed, book)
    P, Pi = curve.n_pillars, T.size
    Q = P + Pi
    out = np.empty((B, 1 + Q + Q * Q))
    _check(load().adr_yoy_subbook_ladders(ctx._h, curve._h, int(infl_method), Pi, _ptr(T), _ptr(b), fix_off.size - 1, fix_tp.size,
                                          _ptr(fix_off, _i64p), _ptr(fix_tp), _ptr(fix_pay), cpn.shape[1], _ptr(cpn_off, _i64p),
                                          _ptr(cpn), B, _ptr(sub_off, _i64p), _request_mask(want_delta, want_gamma), _ptr(out)),
           "adr_yoy_subbook_ladders")
    return _yoy_ladder_rows(out, P, Pi)


def yoy_subbook_ladders_host(interp_method: int, times, dfs, jac, hess, infl_method: int, T, b, fixed, book, sub_off,
                             want_delta=True, want_gamma=True):
    """`yoy_subbook_ladders` on the CPU (adr_yoy_subbook_ladders_host) for the discount curve's arrays as `DeviceCurve` takes
    them: the same node, sum and projection code, chunks and orders; no GPU needed."""
    sub_off, B = _sub_offsets(sub_off)
    times, dfs, jac, hess, K, P = _curve_arrays(times, dfs, jac, hess, shapes=True)
    T, b, fix_off, fix_tp, fix_pay, cpn_off, cpn = _yoy_ladder_inputs(T, b, fixed, book)
    Pi = T.size
    Q = P + Pi
    out = np.empty((B, 1 + Q + Q * Q))
    _check(load().adr_yoy_subbook_ladders_host(int(interp_method), K, P, _ptr(times), _ptr(dfs), _ptr(jac), _ptr(hess),
                                               int(infl_method), Pi, _ptr(T), _ptr(b), fix_off.size - 1, fix_tp.size,
                                               _ptr(fix_off, _i64p), _ptr(fix_tp), _ptr(fix_pay), cpn.shape[1],
                                               _ptr(cpn_off, _i64p), _ptr(cpn), B, _ptr(sub_off, _i64p),
                                               _request_mask(want_delta, want_gamma), _ptr(out)), "adr_yoy_subbook_ladders_host")
    return _yoy_ladder_rows(out, P, Pi)


def yoy_subbook_ladders_work(curve: DeviceCurve, n_infl_pillars: int, n_swaps: int, n_sub_books: int, want_gamma=True):
    """``(doubles of scratch, rows of chunk records it holds)`` of `yoy_subbook_ladders_dev` (adr_yoy_subbook_ladders_work)."""
    chunks = C.c_int64(0)
    work = load().adr_yoy_subbook_ladders_work(curve._h, int(n_infl_pillars), int(n_swaps), int(n_sub_books),
                                               _request_mask(True, want_gamma), C.cast(C.byref(chunks), _i64p))
    if work <= 0:
        raise LibError("adr_yoy_subbook_ladders_work: a curve, 1 .. 64 inflation pillars and at least one swap and sub-book are "
                       "needed")
    return int(work), int(chunks.value)


def yoy_subbook_ladders_dev(ctx: Context, curve: DeviceCurve, infl_method: int, P_i: int, n_swaps: int, n_fix: int, n_coupons: int,
                            B: int, ptrs, mask: int, out_ptr: int, work_ptr: int, stream=0):
    """Non-blocking form (adr_yoy_subbook_ladders_dev): ``ptrs`` maps ``T`` [P_i], ``b`` [P_i], ``fix_off``, ``fix_tp``,
    ``fix_pay``, ``cpn_off``, ``cpn`` and ``plan`` (the uploaded `scenario_subbook_plan`) to device pointers (integers; the
    value arrays of an empty leg may be 0); the output ``[B, 1 + Q + Q Q]`` and `yoy_subbook_ladders_work` doubles of
    scratch."""
    g = _dev_of(ptrs)
    _check(load().adr_yoy_subbook_ladders_dev(ctx._h, curve._h, int(infl_method), int(P_i), g("T"), g("b"), int(n_swaps), int(n_fix),
                                              g("fix_off"), g("fix_tp"), g("fix_pay"), int(n_coupons), g("cpn_off"), g("cpn"),
                                              int(B), g("plan"), int(mask), _dev(out_ptr), _dev(work_ptr), _vp(stream or None)),
           "adr_yoy_subbook_ladders_dev")


# --------------------------------------------------------------------------------------- delta-gamma P&L of ladders
LADDER_PNL_MAX_PILLARS = 256                                # ADR_LADDER_PNL_MAX_PILLARS


def _ladder_pnl_call(fn, head, ladders, shocks_bp, want):
    ladders, shocks_bp = _f64(ladders), _f64(shocks_bp)
    if ladders.ndim != 2 or shocks_bp.ndim != 2:
        raise LibError(f"ladders [B, 1 + P + P P] and shocks_bp [S, P] are needed, not {list(ladders.shape)} and "
                       f"{list(shocks_bp.shape)}")
    (B, width), (S, P) = ladders.shape, shocks_bp.shape
    if width != 1 + P + P * P:
        raise LibError(f"ladder rows of {width} entries do not match shocks of {P} pillars (1 + P + P P = {1 + P + P * P})")
    names = ("pnl", "delta_pnl", "gamma_pnl")
    out = {k: np.empty((B, S)) for k, w in zip(names, want) if w}
    _check(fn(*head, B, P, _ptr(ladders), S, _ptr(shocks_bp), *[_ptr(out.get(k)) for k in names]), fn.__name__)
    return out


def ladder_pnl(ctx: Context, ladders, shocks_bp, want=(True, False, False)):
    """Delta-gamma P&L of ladder rows under a shock set on the device (adr_ladder_pnl, blocking).  ``ladders
    [B, 1 + P + P P]``: rows ``[pv, delta[P] per bp, gamma[P][P] per bp^2]`` as `subbook_ladders` and ``price``'s ``agg``
    lay them out; ``shocks_bp [S, P]``: the move of every par quote per scenario, in basis points.  ``want``: which of
    ``pnl``, ``delta_pnl`` (``delta . x``) and ``gamma_pnl`` (``x' gamma x / 2``) to return, ``[B, S]`` each."""
    return _ladder_pnl_call(load().adr_ladder_pnl, (ctx._h,), ladders, shocks_bp, want)


def ladder_pnl_host(ladders, shocks_bp, want=(True, False, False)):
    """`ladder_pnl` on the CPU (adr_ladder_pnl_host): the same fused multiply-adds in the same order, the same bits."""
    return _ladder_pnl_call(load().adr_ladder_pnl_host, (), ladders, shocks_bp, want)


def ladder_pnl_dev(ctx: Context, B: int, P: int, ladders_ptr: int, S: int, shocks_ptr: int, pnl_ptr: int = 0,
                   delta_pnl_ptr: int = 0, gamma_pnl_ptr: int = 0, stream=0):
    """Non-blocking form (adr_ladder_pnl_dev): device pointers of ``ladders`` [B, 1 + P + P P], ``shocks_bp`` [S, P] and
    the outputs [B, S] (0: not wanted, not touched)."""
    _check(load().adr_ladder_pnl_dev(ctx._h, int(B), int(P), _dev(ladders_ptr), int(S), _dev(shocks_ptr), _dev(pnl_ptr),
                                     _dev(delta_pnl_ptr), _dev(gamma_pnl_ptr), _vp(stream or None)), "adr_ladder_pnl_dev")


# ------------------------------------------------------------------------- Monte Carlo shocks and the tail of wide rows
def _shock_args(factor_bp, n_scenarios, seed, first_scenario):
    factor = _f64(factor_bp)
    if factor.ndim != 2:
        raise LibError(f"factor_bp must have shape [n_pillars, n_factors], not {list(factor.shape)}")
    seed, first = int(seed), int(first_scenario)
    if not 0 <= seed < 2 ** 64 or not -2 ** 63 <= first < 2 ** 63:
        raise LibError(f"seed must fit a uint64 and first_scenario an int64, not {seed}, {first}")
    S = int(n_scenarios)
    return factor, seed, first, S, np.empty((max(S, 0), factor.shape[0]))


def shock_normal(ctx: Context, factor_bp, n_scenarios: int, seed: int, antithetic: bool = False, first_scenario: int = 0):
    """``[S, P]``: correlated normal shocks ``factor_bp [P, F] @ z`` in basis points on the device (adr_shock_normal,
    blocking): Philox4x32-10 and Box-Muller, row ``s`` a function of ``seed``, ``first_scenario + s``, the factor matrix
    and ``antithetic`` alone."""
    factor, seed, first, S, out = _shock_args(factor_bp, n_scenarios, seed, first_scenario)
    _check(load().adr_shock_normal(ctx._h, seed, first, S, factor.shape[0], factor.shape[1], _ptr(factor), int(bool(antithetic)),
                                   _ptr(out)), "adr_shock_normal")
    return out


def shock_normal_host(factor_bp, n_scenarios: int, seed: int, antithetic: bool = False, first_scenario: int = 0):
    """`shock_normal` on the CPU (adr_shock_normal_host): the same code; the uniforms have the same bits, the normals each
    side's ``log``, ``sqrt``, ``cos`` and ``sin``."""
    factor, seed, first, S, out = _shock_args(factor_bp, n_scenarios, seed, first_scenario)
    _check(load().adr_shock_normal_host(seed, first, S, factor.shape[0], factor.shape[1], _ptr(factor), int(bool(antithetic)),
                                        _ptr(out)), "adr_shock_normal_host")
    return out


def shock_normal_dev(ctx: Context, seed: int, first_scenario: int, S: int, P: int, F: int, factor_ptr: int, antithetic: bool,
                     out_ptr: int, stream=0):
    """Non-blocking form (adr_shock_normal_dev): device pointers of ``factor`` [P, F] and ``out`` [S, P]."""
    _check(load().adr_shock_normal_dev(ctx._h, int(seed), int(first_scenario), int(S), int(P), int(F), _dev(factor_ptr),
                                       int(bool(antithetic)), _dev(out_ptr), _vp(stream or None)), "adr_shock_normal_dev")


def shock_words_host(counter, key) -> np.ndarray:
    """The Philox4x32-10 block of ``counter [4]`` and ``key [2]`` (uint32 words), as the generator computes it (a test hook)."""
    c, k, w = (C.c_uint32 * 4)(*[int(v) for v in counter]), (C.c_uint32 * 2)(*[int(v) for v in key]), (C.c_uint32 * 4)()
    load().adr_shock_words_host(c, k, w)
    return np.array(list(w), dtype=np.uint32)


def shock_uniforms(n_scenarios: int, n_factors: int, seed: int, antithetic: bool = False, first_scenario: int = 0, ctx=None):
    """``[S, ceil(F / 2), 2]``: the uniforms ``(u1, u2)`` behind every pair of normals (a test hook); ``ctx=None``: the host
    twin's, else the device's."""
    S, F = int(n_scenarios), int(n_factors)
    u = np.empty((max(S, 0), max((F + 1) // 2, 0), 2))
    if ctx is None:
        rc = load().adr_shock_uniforms_host(int(seed), int(first_scenario), S, F, int(bool(antithetic)), _ptr(u))
    else:
        rc = load().adr_shock_uniforms(ctx._h, int(seed), int(first_scenario), S, F, int(bool(antithetic)), _ptr(u))
    _check(rc, "adr_shock_uniforms")
    return u


def scenario_tail_select(ctx: Context, rows, k: int, base_col: int = -1):
    """`scenario_tail` for rows of any width (adr_scenario_tail_select, blocking): a radix select of the ``k``-th smallest
    P&L, then the tail kernel on the ``k`` survivors; ``k <= SCENARIO_TAIL_MAX``."""
    return _tail_call(load().adr_scenario_tail_select, (ctx._h,), rows, k, base_col)


def scenario_tail_select_host(rows, k: int, base_col: int = -1):
    """`scenario_tail_select` on the CPU (adr_scenario_tail_select_host): the same bits."""
    return _tail_call(load().adr_scenario_tail_select_host, (), rows, k, base_col)


def scenario_tail_select_work(B: int, S_tot: int, k: int) -> int:
    """Bytes of scratch `scenario_tail_select_dev` needs (0 for sizes it refuses)."""
    return int(load().adr_scenario_tail_select_work(int(B), int(S_tot), int(k)))


def scenario_tail_select_dev(ctx: Context, B: int, S_tot: int, rows_ptr: int, k: int, var_ptr: int, es_ptr: int, work_ptr: int,
                             base_col: int = -1, stream=0):
    """Non-blocking form (adr_scenario_tail_select_dev): device pointers of ``rows`` [B, S_tot], ``var`` [B], ``es`` [B] and
    ``work`` (`scenario_tail_select_work` bytes, 16-byte aligned)."""
    _check(load().adr_scenario_tail_select_dev(ctx._h, int(B), int(S_tot), _dev(rows_ptr), int(base_col), int(k), _dev(var_ptr),
                                               _dev(es_ptr), _dev(work_ptr), _vp(stream or None)), "adr_scenario_tail_select_dev")


# ------------------------------------------------------------------ the ordered tail select and the allocation around it
def _order_call(fn, head, rows, k, base_col):
    rows = _tail_rows(rows)
    B = rows.shape[0]
    order, var, es = np.empty((B, max(int(k), 0)), dtype=np.int64), np.empty(B), np.empty(B)
    _check(fn(*head, B, rows.shape[1], _ptr(rows), int(base_col), int(k), _ptr(order, _i64p), _ptr(var), _ptr(es)), fn.__name__)
    return order, var, es


def scenario_tail_order(ctx: Context, rows, k: int, base_col: int = -1):
    """``(order [B, k] int64, var [B], es [B])`` of ``rows [B, S]`` on the device (adr_scenario_tail_order, blocking): every
    row's ``k`` worst P&L indices ordered by (value, index) - ties to the lower index - and `scenario_tail_select`'s ``var``
    and ``es``; ``k <= SCENARIO_ALLOC_MAX``.  A row holding a NaN: -1 and NaN."""
    return _order_call(load().adr_scenario_tail_order, (ctx._h,), rows, k, base_col)


def scenario_tail_order_host(rows, k: int, base_col: int = -1):
    """`scenario_tail_order` on the CPU (adr_scenario_tail_order_host): the same bits."""
    return _order_call(load().adr_scenario_tail_order_host, (), rows, k, base_col)


def scenario_tail_order_work(B: int, S_tot: int, k: int) -> int:
    """Bytes of scratch `scenario_tail_order_dev` needs (0 for sizes it refuses)."""
    return int(load().adr_scenario_tail_order_work(int(B), int(S_tot), int(k)))


def scenario_tail_order_dev(ctx: Context, B: int, S_tot: int, rows_ptr: int, k: int, order_ptr: int, var_ptr: int, es_ptr: int,
                            work_ptr: int, base_col: int = -1, stream=0):
    """Non-blocking form (adr_scenario_tail_order_dev): device pointers of ``rows`` [B, S_tot], ``order`` [B, k] int64,
    ``var`` [B], ``es`` [B] and ``work`` (`scenario_tail_order_work` bytes, 16-byte aligned)."""
    _check(load().adr_scenario_tail_order_dev(ctx._h, int(B), int(S_tot), _dev(rows_ptr), int(base_col), int(k), _dev(order_ptr),
                                              _dev(var_ptr), _dev(es_ptr), _dev(work_ptr), _vp(stream or None)),
           "adr_scenario_tail_order_dev")


def scenario_tail_alloc_select(ctx: Context, rows, k: int, base_col: int = -1):
    """`scenario_tail_alloc` for rows of any width (adr_scenario_tail_alloc_select, blocking): the limit is on the tail,
    ``k <= SCENARIO_ALLOC_MAX``."""
    return _alloc_call(load().adr_scenario_tail_alloc_select, (ctx._h,), rows, k, base_col)


def scenario_tail_alloc_select_host(rows, k: int, base_col: int = -1):
    """`scenario_tail_alloc_select` on the CPU (adr_scenario_tail_alloc_select_host): the same bits."""
    return _alloc_call(load().adr_scenario_tail_alloc_select_host, (), rows, k, base_col)


def scenario_tail_alloc_select_work(B: int, S_tot: int, k: int) -> int:
    """Bytes of scratch `scenario_tail_alloc_select_dev` needs (0 for sizes it refuses)."""
    return int(load().adr_scenario_tail_alloc_select_work(int(B), int(S_tot), int(k)))


def scenario_tail_alloc_select_dev(ctx: Context, B: int, S_tot: int, rows_ptr: int, k: int, var_ptr: int, es_ptr: int,
                                   comp_var_ptr: int, comp_es_ptr: int, work_ptr: int, base_col: int = -1, stream=0):
    """Non-blocking form (adr_scenario_tail_alloc_select_dev): device pointers as `scenario_tail_alloc_dev` takes them, with
    ``work`` of `scenario_tail_alloc_select_work` bytes, 16-byte aligned."""
    _check(load().adr_scenario_tail_alloc_select_dev(ctx._h, int(B), int(S_tot), _dev(rows_ptr), int(base_col), int(k),
                                                     _dev(var_ptr), _dev(es_ptr), _dev(comp_var_ptr), _dev(comp_es_ptr),
                                                     _dev(work_ptr), _vp(stream or None)), "adr_scenario_tail_alloc_select_dev")


def scenario_total_host(rows, base_col: int = -1):
    """``tot [m]``: the fixed-order column sums of ``rows [B, S]`` (adr_scenario_total_host), `scenario_tail_alloc`'s firm
    totals; of ladder rows, the firm's ladder row."""
    rows = _tail_rows(rows)
    tot = np.empty(max(rows.shape[1] - (1 if base_col >= 0 else 0), 0))
    _check(load().adr_scenario_total_host(rows.shape[0], rows.shape[1], _ptr(rows), int(base_col), _ptr(tot)), "adr_scenario_total_host")
    return tot


def scenario_total_dev(ctx: Context, B: int, S_tot: int, rows_ptr: int, tot_ptr: int, base_col: int = -1, stream=0):
    """Non-blocking form (adr_scenario_total_dev): device pointers of ``rows`` [B, S_tot] and ``tot`` [m]."""
    _check(load().adr_scenario_total_dev(ctx._h, int(B), int(S_tot), _dev(rows_ptr), int(base_col), _dev(tot_ptr),
                                         _vp(stream or None)), "adr_scenario_total_dev")


def shock_gather_host(shocks_bp, order):
    """``[k, P]``: the rows ``order [k]`` of ``shocks_bp [S, P]`` (adr_shock_gather_host); NaN everywhere when ``order[0]``
    is negative."""
    shocks_bp, order = _f64(shocks_bp), np.ascontiguousarray(order, dtype=np.int64).reshape(-1)
    if shocks_bp.ndim != 2:
        raise LibError(f"shocks_bp must have shape [n_scenarios, n_pillars], not {list(shocks_bp.shape)}")
    out = np.empty((order.size, shocks_bp.shape[1]))
    _check(load().adr_shock_gather_host(order.size, shocks_bp.shape[1], _ptr(shocks_bp), shocks_bp.shape[0], _ptr(order, _i64p),
                                        _ptr(out)), "adr_shock_gather_host")
    return out


def shock_gather_dev(ctx: Context, k: int, P: int, shocks_ptr: int, S: int, order_ptr: int, out_ptr: int, stream=0):
    """Non-blocking form (adr_shock_gather_dev): device pointers of ``shocks`` [S, P], ``order`` [k] int64 and ``out`` [k, P]."""
    _check(load().adr_shock_gather_dev(ctx._h, int(k), int(P), _dev(shocks_ptr), int(S), _dev(order_ptr), _dev(out_ptr),
                                       _vp(stream or None)), "adr_shock_gather_dev")


def tail_components_host(pnl):
    """``(comp_var [B], comp_es [B])`` of ``pnl [B, k]``, every row's P&L at the firm's ``k`` worst scenarios in the firm's
    order (adr_tail_components_host): minus the last column, and minus the sequential sum over ``k``."""
    pnl = _tail_rows(pnl)
    comp_var, comp_es = np.empty(pnl.shape[0]), np.empty(pnl.shape[0])
    _check(load().adr_tail_components_host(pnl.shape[0], pnl.shape[1], _ptr(pnl), _ptr(comp_var), _ptr(comp_es)),
           "adr_tail_components_host")
    return comp_var, comp_es


def tail_components_dev(ctx: Context, B: int, k: int, pnl_ptr: int, comp_var_ptr: int, comp_es_ptr: int, stream=0):
    """Non-blocking form (adr_tail_components_dev): device pointers of ``pnl`` [B, k], ``comp_var`` [B] and ``comp_es`` [B]."""
    _check(load().adr_tail_components_dev(ctx._h, int(B), int(k), _dev(pnl_ptr), _dev(comp_var_ptr), _dev(comp_es_ptr),
                                          _vp(stream or None)), "adr_tail_components_dev")


# ------------------------------------------------------------ discount factors of shocked curves (csrc/curve_dfs.hip)
def _dfs_shocked_args(base_rates, shocks_bp):
    """``(base [P], shocks [S, ld])`` as the blocking and host entries take them."""
    base, shocks = _f64(base_rates).reshape(-1), _f64(shocks_bp)
    if shocks.ndim != 2:
        raise LibError(f"shocks_bp must have shape [n_scenarios, ld], not {list(shocks.shape)}")
    return base, shocks


def curve_dfs_shocked(ctx: Context, plan: CurvePlan, base_rates, shocks_bp):
    """``(dfs [S, K], bad [S] int32)``: the discount factors of ``plan``'s grid at the rates ``base_rates [P] +
    shocks_bp[s, :P] * 1e-4`` on the device (adr_curve_dfs_shocked, blocking), with `CurvePlan.build`'s bits at those
    rates; ``bad[s]``: a discount factor of row ``s`` is not finite or not positive.  Columns of ``shocks_bp`` beyond
    ``P`` are not read."""
    base, shocks = _dfs_shocked_args(base_rates, shocks_bp)
    if base.size != plan.n_pillars:
        raise LibError(f"base_rates needs one entry per pillar ({plan.n_pillars}), not {base.size}")
    S, ld = shocks.shape
    dfs, bad = np.empty((S, plan.n_knots)), np.empty(S, dtype=np.int32)
    _check(load().adr_curve_dfs_shocked(ctx._h, plan._h, _ptr(base), S, ld, _ptr(shocks), _ptr(dfs), _ptr(bad, _i32p)),
           "adr_curve_dfs_shocked")
    return dfs, bad


def curve_dfs_shocked_host(acc, pillar, prev_idx, base_rates, shocks_bp):
    """`curve_dfs_shocked` on the CPU (adr_curve_dfs_shocked_host) from the scan arrays of an `EngineCurve`: the same
    operations in the same order, the same bits; no GPU and no plan."""
    base, shocks = _dfs_shocked_args(base_rates, shocks_bp)
    acc = _f64(acc).reshape(-1)
    pillar, prev_idx = (np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in (pillar, prev_idx))
    if pillar.size != acc.size or prev_idx.size != acc.size:
        raise LibError("scan arrays must have one entry per knot")
    S, ld = shocks.shape
    dfs, bad = np.empty((S, acc.size)), np.empty(S, dtype=np.int32)
    _check(load().adr_curve_dfs_shocked_host(acc.size, base.size, _ptr(acc), _ptr(pillar, _i32p), _ptr(prev_idx, _i32p), _ptr(base),
                                             S, ld, _ptr(shocks), _ptr(dfs), _ptr(bad, _i32p)), "adr_curve_dfs_shocked_host")
    return dfs, bad


def curve_dfs_shocked_work(plan: CurvePlan, n_scenarios: int) -> int:
    """Doubles of scratch `curve_dfs_shocked_dev` needs (0 for sizes it refuses)."""
    return int(load().adr_curve_dfs_shocked_work(plan._h, int(n_scenarios)))


def curve_dfs_shocked_dev(ctx: Context, plan: CurvePlan, base_ptr: int, S: int, ld: int, shocks_ptr: int, dfs_ptr: int,
                          work_ptr: int, bad_ptr: int = 0, stream=0):
    """Non-blocking form (adr_curve_dfs_shocked_dev): device pointers of ``base_rates`` [P], ``shocks_bp`` [S, ld], ``dfs``
    [S, K], ``bad`` [S] int32 (0: not wanted) and `curve_dfs_shocked_work` doubles of scratch."""
    _check(load().adr_curve_dfs_shocked_dev(ctx._h, plan._h, _dev(base_ptr), int(S), int(ld), _dev(shocks_ptr), _dev(dfs_ptr),
                                            _dev(bad_ptr), _dev(work_ptr), _vp(stream or None)), "adr_curve_dfs_shocked_dev")


def scenario_rows_place_dev(ctx: Context, B: int, S_tile: int, tile_ptr: int, S_tot: int, s0: int, rows_ptr: int, stream=0):
    """``rows[b, s0 + s] = tile[b, s]`` on the device (adr_scenario_rows_place_dev, csrc/shock_columns.hip: the merge kernel
    without a row map): device pointers of ``tile`` [B, S_tile] and ``rows`` [B, S_tot]."""
    _check(load().adr_scenario_rows_place_dev(ctx._h, int(B), int(S_tile), _dev(tile_ptr), int(S_tot), int(s0), _dev(rows_ptr),
                                              _vp(stream or None)), "adr_scenario_rows_place_dev")


# ------------------------------------------- shock columns and the merge of sub-book rows (csrc/shock_columns.hip)
def _shock_columns_call(fn, head, shocks_bp, col0, n, base, floor, bad):
    shocks = _f64(shocks_bp)
    if shocks.ndim != 2:
        raise LibError(f"shocks_bp must have shape [n_scenarios, ld], not {list(shocks.shape)}")
    base = None if base is None else _f64(base).reshape(-1)
    if base is not None and base.size != int(n):
        raise LibError(f"base needs one entry per column ({int(n)}), not {base.size}")
    S, ld = shocks.shape
    bad = np.zeros(S, dtype=np.int32) if bad is None else np.ascontiguousarray(bad, dtype=np.int32).reshape(-1).copy()
    if bad.size != S:
        raise LibError(f"bad needs one flag per scenario ({S}), not {bad.size}")
    out = np.empty((S, max(int(n), 0)))
    _check(fn(*head, S, ld, _ptr(shocks), int(col0), int(n), _ptr(base), int(floor is not None), float(floor or 0.0), _ptr(out),
              _ptr(bad, _i32p)), fn.__name__)
    return out, bad


def shock_columns(ctx: Context, shocks_bp, col0: int, n: int, base=None, floor=None, bad=None):
    """``(out [S, n], bad [S] int32)``: ``base + shocks_bp[:, col0:col0 + n] * 1e-4`` (``base`` None: the product itself) on
    the device (adr_shock_columns, blocking), a rounded product and a rounded sum - NumPy's bits.  ``bad[s]`` is 1 where an
    entry of row ``s`` is not finite or, with ``floor``, is ``<= floor``; a flag of the ``bad`` passed in stays set."""
    return _shock_columns_call(load().adr_shock_columns, (ctx._h,), shocks_bp, col0, n, base, floor, bad)


def shock_columns_host(shocks_bp, col0: int, n: int, base=None, floor=None, bad=None):
    """`shock_columns` on the CPU (adr_shock_columns_host): the same bits; no GPU needed."""
    return _shock_columns_call(load().adr_shock_columns_host, (), shocks_bp, col0, n, base, floor, bad)


def shock_columns_dev(ctx: Context, S: int, ld: int, shocks_ptr: int, col0: int, n: int, out_ptr: int, base_ptr: int = 0,
                      floor=None, bad_ptr: int = 0, stream=0):
    """Non-blocking form (adr_shock_columns_dev): device pointers of ``shocks_bp`` [S, ld], ``base`` [n] (0: none), ``out``
    [S, n] and ``bad`` [S] int32 (0: not wanted); ``floor`` None: no floor."""
    _check(load().adr_shock_columns_dev(ctx._h, int(S), int(ld), _dev(shocks_ptr), int(col0), int(n), _dev(base_ptr),
                                        int(floor is not None), float(floor or 0.0), _dev(out_ptr), _dev(bad_ptr),
                                        _vp(stream or None)), "adr_shock_columns_dev")


def scenario_rows_merge_host(tile, rows, s0: int, target, add=None):
    """``rows[target[b], s0 + s] = tile[b, s]``, or ``+=`` where ``add[b]`` is not 0, IN PLACE on ``rows [B_tot, S_tot]``
    (float64, C-contiguous) (adr_scenario_rows_merge_host); a target outside the rows skips its row, a repeated one is
    refused.  Returns ``rows``."""
    tile = _f64(np.atleast_2d(tile))
    if not (isinstance(rows, np.ndarray) and rows.dtype == np.float64 and rows.ndim == 2 and rows.flags.c_contiguous):
        raise LibError("rows must be a C-contiguous float64 array [B_tot, S_tot]: it is written in place")
    target = np.ascontiguousarray(target, dtype=np.int64).reshape(-1)
    add = None if add is None else np.ascontiguousarray(add, dtype=np.int32).reshape(-1)
    if tile.ndim != 2 or target.size != tile.shape[0] or (add is not None and add.size != tile.shape[0]):
        raise LibError(f"target and add need one entry per row of the tile ({tile.shape[0] if tile.ndim == 2 else '?'})")
    _check(load().adr_scenario_rows_merge_host(tile.shape[0], tile.shape[1], _ptr(tile), rows.shape[0], rows.shape[1], int(s0),
                                               _ptr(rows), _ptr(target, _i64p), _ptr(add, _i32p)), "adr_scenario_rows_merge_host")
    return rows


def scenario_rows_merge_dev(ctx: Context, B: int, S_tile: int, tile_ptr: int, B_tot: int, S_tot: int, s0: int, rows_ptr: int,
                            target_ptr: int, add_ptr: int = 0, stream=0):
    """Non-blocking form (adr_scenario_rows_merge_dev): device pointers of ``tile`` [B, S_tile], ``rows`` [B_tot, S_tot],
    ``target`` [B] int64 (distinct) and ``add`` [B] int32 (0: copy every row)."""
    _check(load().adr_scenario_rows_merge_dev(ctx._h, int(B), int(S_tile), _dev(tile_ptr), int(B_tot), int(S_tot), int(s0),
                                              _dev(rows_ptr), _dev(target_ptr), _dev(add_ptr), _vp(stream or None)),
           "adr_scenario_rows_merge_dev")


def set_default_context(ctx: Context, device: int | None = None) -> None:
    """Make ``ctx`` the context `default_context` hands out (for hosts that create their own, e.g. one per rank)."""
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
        n = load().adr_device_count()
        if n > 0:
            device %= n
    _default_ctx[device] = ctx


def default_context(device: int | None = None) -> Context:
    """Process-wide context for ``device`` (default: LOCAL_RANK or 0)."""
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
        n = load().adr_device_count()
        if n > 0:
            device %= n
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


def build_identity() -> dict:
    """What is running: sha256 of the loaded shared library and of the sources it is built from (adrates_amd/csrc/* and
    include/adrates.h, names and contents, sorted).  Evidence files under profiles/ carry the same two hashes
    (tools/profile_summary.py), and bench.py reports a counter-derived figure only when the source hash matches."""
    import glob
    import hashlib
    root = os.path.dirname(os.path.abspath(__file__))
    src = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(root, "csrc", "*.hip")) + glob.glob(os.path.join(root, "csrc", "*.hpp")) +
                   glob.glob(os.path.join(root, "csrc", "*.cpp")) + [os.path.join(root, "csrc", "Makefile"),
                                                                    os.path.join(os.path.dirname(root), "include", "adrates.h")])
    for f in files:
        if os.path.exists(f):
            src.update(os.path.basename(f).encode())
            with open(f, "rb") as fh:
                src.update(fh.read())
    lib = None
    if os.path.exists(_LIB_PATH):
        with open(_LIB_PATH, "rb") as fh:
            lib = hashlib.sha256(fh.read()).hexdigest()
    return {"source_sha256": src.hexdigest(), "lib_sha256": lib, "lib": os.path.relpath(_LIB_PATH, os.path.dirname(root))}


ROUTE_FAMILIES = ("lite", "lite_lag", "fast", "fast_chained", "fast_lag", "fast_lag_chained", "general", "wide", "tiled", "knot",
                  "knot_lag")
ROUTE_SETS = ("lite", "lite_lag", "rows", "chained", "lagged", "lagged_chained", "general", "general_b", "rest", "nonlite",
              "nonlite_b", "all")


def route_host(interp_method: int, times, dfs, jac, hess, batch, req_mask: int, per_trade=True, aggregate=False, n_cu=256,
               curve_flags=0):
    """The launch plan adr_price_dev would replay for this curve, batch and request, and how often it prices each trade
    (adr_route_host; no GPU needed).  Returns ``(launches, cover)``: launches = [(family, set, items, blocks)], names from
    ROUTE_FAMILIES / ROUTE_SETS; cover [n] int32."""
    times, dfs, jac, hess_c, K, P = _curve_arrays(times, dfs, jac, hess)
    n = batch.n_trades
    fo, lo = np.ascontiguousarray(batch.fix_off, dtype=np.int64), np.ascontiguousarray(batch.flt_off, dtype=np.int64)
    tp, te, al = _f64(batch.flt_tp), _f64(batch.flt_te), _f64(batch.flt_alpha)
    w = None if batch.flt_weight is None else _f64(batch.flt_weight)
    cover = np.zeros(max(n, 1), dtype=np.int32)
    rows = np.zeros((64, 4), dtype=np.int32)          # (a 256-pillar curve with GAMMA: 36 tile-pair launches + the knot passes)
    got = _check(load().adr_route_host(int(interp_method), K, P, _ptr(times), _ptr(dfs), _ptr(jac), _ptr(hess_c), int(curve_flags), n,
                                       _ptr(fo, _i64p), _ptr(lo, _i64p), _ptr(tp), _ptr(te), _ptr(al), _ptr(w), int(req_mask),
                                       1 if per_trade else 0, 1 if aggregate else 0, int(n_cu),
                                       cover.ctypes.data_as(C.POINTER(C.c_int32)), rows.ctypes.data_as(C.POINTER(C.c_int32)), 64),
                 "adr_route_host")
    launches = [(ROUTE_FAMILIES[f], ROUTE_SETS[s_], int(items), int(blocks)) for f, s_, items, blocks in rows[:min(got, 64)]]
    return launches, cover[:n]
