"""ctypes mirror of include/hbvx.h and a thin handle around a loaded library.

This is the binding a maintainer of the reference would add to call the C ABI
from Python.  Struct layouts are verified against the
library's own `hbvx_sizeof()` at load time.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple, Optional

ABI_VERSION = 10
MAX_PARAM = 20
GAGE_MAXLEN = 72
NSTATE = 5
MAX_FLUX = 12
UH_MAXLEN = 15

# enum hbvx_model
MODEL_HBV10, MODEL_HBV11P, MODEL_HBV20, MODEL_HBVADJ, MODEL_HOURLY = 0, 1, 2, 3, 4

# enum hbvx_traj_layout
TRAJ_ROWS, TRAJ_PACKED, TRAJ_CKPT = 0, 1, 2     # traj_layout = kind | (K << 8) for TRAJ_CKPT

# enum hbvx_flux
(F_QSIM, F_Q0, F_Q1, F_Q2, F_AET, F_SWE, F_RECHARGE, F_EXCS, F_EVAPFACTOR, F_TOSOIL, F_PERC,
 F_CAPILLARY) = range(12)

PARAM_SLOTS = ["parBETA", "parFC", "parK0", "parK1", "parK2", "parLP", "parPERC", "parUZL",
               "parTT", "parCFMAX", "parCFR", "parCWH", "parBETAET", "parC", "parRT", "parAC",
               "parF0", "parFMIN", "parALPHA"]

_fp = C.c_void_p  # every float*/uint8_t* travels as an address


class ParamSrc(C.Structure):
    _fields_ = [("dyn", _fp), ("sta", _fp), ("drop", _fp),
                ("dyn_t_stride", C.c_int64), ("dyn_b_stride", C.c_int64),
                ("sta_b_stride", C.c_int64), ("lo", C.c_float), ("hi", C.c_float)]


class ParamGrad(C.Structure):
    _fields_ = [("dyn", _fp), ("sta", _fp),
                ("dyn_t_stride", C.c_int64), ("dyn_b_stride", C.c_int64),
                ("sta_b_stride", C.c_int64)]


class Desc(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("model", C.c_int32), ("T", C.c_int32),
                ("B", C.c_int32), ("M", C.c_int32), ("n_param", C.c_int32),
                ("raw_sigmoid", C.c_int32), ("ch_prcp", C.c_int32), ("ch_tmean", C.c_int32),
                ("ch_pet", C.c_int32), ("nearzero", C.c_float), ("adj_stop", C.c_int32),
                ("x", _fp), ("x_t_stride", C.c_int64), ("x_b_stride", C.c_int64),
                ("ac", _fp), ("elev", _fp), ("muwts", _fp),
                ("mu_t_stride", C.c_int64), ("mu_b_stride", C.c_int64),
                ("state_in", _fp), ("p", ParamSrc * MAX_PARAM),
                ("adj_gtol", C.c_float), ("adj_max_iter", C.c_int32)]


class FwdOut(C.Structure):
    _fields_ = [("flux", _fp), ("state_out", _fp), ("traj", _fp), ("aux", _fp),
                ("n_flux", C.c_int32), ("traj_layout", C.c_int32),
                ("zero_ptr", _fp), ("zero_bytes", C.c_uint64), ("zero_state", _fp)]


class BwdIO(C.Structure):
    _fields_ = [("traj", _fp), ("aux", _fp), ("grad_flux", _fp), ("grad_flux4", _fp),
                ("grad_state_out", _fp), ("grad_x", _fp),
                ("grad_muwts", _fp), ("grad_state_in", _fp),
                ("n_flux", C.c_int32), ("traj_layout", C.c_int32),
                ("g", ParamGrad * MAX_PARAM),
                ("workspace", _fp), ("workspace_bytes", C.c_uint64), ("store_gate", _fp)]


class ParamTan(C.Structure):
    _fields_ = [("dyn", _fp), ("sta", _fp),
                ("dyn_t_stride", C.c_int64), ("dyn_b_stride", C.c_int64),
                ("sta_b_stride", C.c_int64)]


class TanIO(C.Structure):
    """hbvx_tan_io: the tangents of one forward-mode call (include/hbvx.h)."""
    _fields_ = [("x", _fp), ("muwts", _fp), ("state_in", _fp), ("p", ParamTan * MAX_PARAM),
                ("tan_flux", _fp), ("tan_state_out", _fp), ("n_flux", C.c_int32), ("reserved0", C.c_int32)]


class TanBatch(C.Structure):
    """hbvx_tan_batch: the tangents of a forward-mode call over n_dir directions (include/hbvx.h)."""
    _fields_ = [("n_dir", C.c_int32), ("n_flux", C.c_int32), ("flux_mask", C.c_uint32), ("dyn_t0", C.c_int32),
                ("x", _fp), ("x_d_stride", C.c_int64), ("muwts", _fp), ("mu_d_stride", C.c_int64),
                ("state_in", _fp), ("state_d_stride", C.c_int64), ("p", ParamTan * MAX_PARAM),
                ("dyn_d_stride", C.c_int64 * MAX_PARAM), ("sta_d_stride", C.c_int64 * MAX_PARAM),
                ("tan_flux", _fp), ("tan_state_out", _fp)]


class RouteDesc(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("T", C.c_int32), ("B", C.c_int32),
                ("S", C.c_int32), ("L", C.c_int32), ("raw_sigmoid", C.c_int32),
                ("ra", _fp), ("rb", _fp), ("r_stride", C.c_int64),
                ("a_lo", C.c_float), ("a_hi", C.c_float), ("b_lo", C.c_float),
                ("b_hi", C.c_float)]


class GageDesc(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("T", C.c_int32), ("U", C.c_int32), ("G", C.c_int32),
                ("NPAIR", C.c_int32), ("L", C.c_int32), ("lag_uh", C.c_int32),
                ("reserved0", C.c_int32),
                ("pair_unit", _fp), ("gage_ptr", _fp), ("pair_gage", _fp), ("unit_ptr", _fp),
                ("unit_pairs", _fp), ("areas", _fp), ("denom", _fp), ("dp", _fp),
                ("a_lo", C.c_float), ("a_hi", C.c_float), ("b_lo", C.c_float), ("b_hi", C.c_float),
                ("tau_lo", C.c_float), ("tau_hi", C.c_float)]


class GramDesc(C.Structure):
    """hbvx_gram_desc: C series on a [T,B] grid, series_stride elements apart (include/hbvx.h)."""
    _fields_ = [("abi_version", C.c_int32), ("T", C.c_int32), ("B", C.c_int32), ("C", C.c_int32),
                ("series_stride", C.c_int64)]


class PopSrc(C.Structure):
    """hbvx_pop_src: where the candidates' static values of one parameter lie (include/hbvx.h)."""
    _fields_ = [("sta", _fp), ("c_stride", C.c_int64), ("b_stride", C.c_int64)]


class Pop(C.Structure):
    """hbvx_pop: the candidates, the observations and the outputs of hbvx_population_cost (include/hbvx.h)."""
    _fields_ = [("n_cand", C.c_int32), ("t_first", C.c_int32), ("p", PopSrc * MAX_PARAM),
                ("route", C.POINTER(RouteDesc)), ("ra", _fp), ("rb", _fp),
                ("r_c_stride", C.c_int64), ("r_b_stride", C.c_int64),
                ("target", _fp), ("w", _fp), ("cost", _fp), ("sim", _fp)]


POP_T_NONE, POP_T_SQRT, POP_T_LOG = 0, 1, 2     # enum hbvx_pop_transform
POP_TRANSFORMS = {"none": POP_T_NONE, "sqrt": POP_T_SQRT, "log": POP_T_LOG}


class PopStats(C.Structure):
    """hbvx_pop_stats: hbvx_pop, the transform, its per-basin shift / eps and the three moment outputs (include/hbvx.h)."""
    _fields_ = [("pop", Pop), ("transform", C.c_int32), ("shift", _fp), ("eps", _fp),
                ("s1", _fp), ("s2", _fp), ("s3", _fp)]


# the series hbvx_population_joint can score beside streamflow: enum hbvx_flux indices of the module's output keys
POP_AUX_SERIES = {"srflow_no_rout": 1, "ssflow_no_rout": 2, "gwflow_no_rout": 3, "AET_hydro": 4, "SWE": 5}


class PopJoint(C.Structure):
    """hbvx_pop_joint: hbvx_pop_stats for the flow term, and the aux term -- which flux, its target / weights / shift and
    its four sums, optionally its series (include/hbvx.h)."""
    _fields_ = [("flow", PopStats), ("aux_series", C.c_int32), ("aux_target", _fp), ("aux_w", _fp), ("aux_shift", _fp),
                ("aux_sse", _fp), ("aux_s1", _fp), ("aux_s2", _fp), ("aux_s3", _fp), ("aux_sim", _fp)]


POP_NO_AUX = -1     # HBVX_POP_NO_AUX: hbvx_population_period without an aux term
# the storages hbvx_adj_population_period can score beside streamflow: HBVX_ADJ_AUX_*, the index of the solved state
ADJ_POP_AUX_SERIES = {"SNOWPACK": 0, "MELTWATER": 1, "SM": 2, "SUZ": 3, "SLZ": 4}


class PopPeriod(C.Structure):
    """hbvx_pop_period: hbvx_pop_joint with targets, weights and series per period, and the two calendars -- counts and
    device arrays of int32 closing days relative to t_first (include/hbvx.h)."""
    _fields_ = [("joint", PopJoint), ("n_flow_periods", C.c_int32), ("flow_end", _fp),
                ("n_aux_periods", C.c_int32), ("aux_end", _fp)]


class LstmDesc(C.Structure):
    """include/hbvx_lstm.h"""
    _fields_ = [("abi_version", C.c_int32), ("T", C.c_int32), ("B", C.c_int32), ("H", C.c_int32)]


LSTM_ABI_VERSION = 1
LSTM_HIDDEN_SIZES = (64, 128, 256)     # what the HIP library instantiates

class PopEntry(NamedTuple):
    """What ops.population needs to know about one population export."""
    struct: type                    # Pop, PopStats, PopJoint or PopPeriod: the export's second argument
    implicit: bool                  # the export is HbvAdj's: it takes a record of the implicit scheme only
    aux_series: Optional[dict]      # the aux series it can score beside the flow, None where it has no aux term


POPULATION = {"hbvx_population_cost": PopEntry(Pop, False, None),
              "hbvx_population_stats": PopEntry(PopStats, False, None),
              "hbvx_adj_population_cost": PopEntry(Pop, True, None),
              "hbvx_adj_population_stats": PopEntry(PopStats, True, None),
              "hbvx_population_joint": PopEntry(PopJoint, False, POP_AUX_SERIES),
              "hbvx_population_period": PopEntry(PopPeriod, False, POP_AUX_SERIES),
              "hbvx_adj_population_period": PopEntry(PopPeriod, True, ADJ_POP_AUX_SERIES)}


def pop_levels(args):
    """(PopPeriod, PopJoint, PopStats, Pop) as they nest in `args` -- PopPeriod.joint.flow.pop, entered at the type of
    `args` (PopFdc / PopEvents .flow and PopEns .s enter at PopStats) -- with None for the levels above it.  The inner ones are views of `args`' memory."""
    levels = {type(args): args}
    for field in ("joint", "flow", "s", "pop"):
        if hasattr(args, field):
            args = getattr(args, field)
            levels[type(args)] = args
    return tuple(levels.get(st) for st in (PopPeriod, PopJoint, PopStats, Pop))


_int, _u64, _str, _vp, _i32, _i64, _P = C.c_int, C.c_uint64, C.c_char_p, C.c_void_p, C.c_int32, C.c_int64, C.POINTER
_POP_SIZEOF = {Pop: 10, PopStats: 11, PopJoint: 12, PopPeriod: 13}

# Every export the binding calls, in the order it is looked up: (name, required, restype, argtypes, layout), layout None
# or (hbvx_sizeof index, the struct that must have that size).  A library may lack a row that is not required (the CPU
# restatement under oracle/ has the required ones only); a call that needs one raises HbvxError naming it.
SIGNATURES = [
    ("hbvx_zero", True, _int, [_vp, _u64, _vp], None),
    ("hbvx_zero_except", True, _int, [_vp, _i64, _i32, _i64, _i64, _i32, C.c_uint32, _vp], None),
    ("hbvx_preferred_traj_layout", True, _int, [_P(Desc)], None),
    ("hbvx_lstm_workspace_bytes", True, _u64, [_P(LstmDesc)], None),
    ("hbvx_lstm_forward", True, _int, [_P(LstmDesc), _fp, _fp, _fp, _fp, _fp, _vp, _u64, _vp], None),
    ("hbvx_lstm_backward", True, _int, [_P(LstmDesc), _fp, _fp, _fp, _fp, _fp, _vp, _u64, _vp], None),
    ("hbvx_lstm_check", True, _int, [_P(LstmDesc), _vp, _vp], None),
    ("hbvx_version", True, _int, [], None),
    ("hbvx_last_error", True, _str, [], None),
    ("hbvx_backend", True, _str, [], None),
    ("hbvx_sizeof", True, _u64, [_int], None),
    ("hbvx_forward", True, _int, [_P(Desc), _P(FwdOut), _vp], None),
    ("hbvx_backward", True, _int, [_P(Desc), _P(BwdIO), _vp], None),
    ("hbvx_backward_workspace_bytes", True, _u64, [_P(Desc)], None),
    ("hbvx_ckpt_workspace_bytes", True, _u64, [_P(Desc), _i32], None),
    ("hbvx_route_forward", True, _int, [_P(RouteDesc), _fp, _fp, _fp, _vp], None),
    ("hbvx_route_workspace_bytes", True, _u64, [_P(RouteDesc)], None),
    ("hbvx_route_backward", True, _int, [_P(RouteDesc), _fp, _fp, _fp, _fp, _fp, _fp, _fp, _u64, _vp], None),
    ("hbvx_adj_forward", True, _int, [_P(Desc), _P(FwdOut), _vp], None),
    ("hbvx_adj_backward", True, _int, [_P(Desc), _P(BwdIO), _vp], None),
    ("hbvx_bfi", True, _int, [_i32, _i32, _fp, _fp, C.c_float, _fp, _vp], None),
    ("hbvx_gage_route_forward", True, _int, [_P(GageDesc), _fp, _fp, _fp, _vp, _u64, _vp], None),
    ("hbvx_gage_route_backward", True, _int, [_P(GageDesc), _fp, _fp, _fp, _fp, _fp, _vp, _u64, _vp], None),
    ("hbvx_gage_route_workspace_bytes", True, _u64, [_P(GageDesc)], None),
    ("hbvx_zero_in_launch", True, _int, [], None),
    ("hbvx_zero_rest", True, _int, [_vp, _u64, _vp, _vp], None),
    ("hbvx_last_dispatch", True, _str, [_int], None),
    ("hbvx_lstm_forward_hx", False, _int, [_P(LstmDesc), _fp, _fp, _fp, _fp, _fp, _fp, _fp, _vp, _u64, _vp], None),
    ("hbvx_lstm_backward_hx", False, _int, [_P(LstmDesc), _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _vp, _u64, _vp], None),
    ("hbvx_forward_tangent", False, _int, [_P(Desc), _P(TanIO), _vp], (7, TanIO)),
    ("hbvx_route_tangent", False, _int, [_P(RouteDesc), _fp, _fp, _fp, _fp, _fp, _fp, _vp], None),
    ("hbvx_bfi_tangent", False, _int, [_i32, _i32, _fp, _fp, _fp, _fp, C.c_float, _fp, _vp], None),
    ("hbvx_lstm_tangent", False, _int,
     [_P(LstmDesc), _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _vp, _u64, _vp], None),
    ("hbvx_forward_tangent_batch", False, _int, [_P(Desc), _P(TanBatch), _vp], (8, TanBatch)),
    ("hbvx_route_tangent_batch", False, _int,
     [_P(RouteDesc), _i32, _fp, _fp, _fp, _i64, _fp, _fp, _i64, _fp, _vp], None),
    ("hbvx_bfi_tangent_batch", False, _int, [_i32, _i32, _i32, _fp, _fp, _fp, _fp, _i64, C.c_float, _fp, _vp], None),
    ("hbvx_lstm_tangent_batch", False, _int,
     [_P(LstmDesc), _i32, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _vp, _u64, _vp], None),
    ("hbvx_lstm_tangent_batch_workspace_bytes", False, _u64, [_P(LstmDesc), _i32], None),
    ("hbvx_hourly_tangent_batch", False, _int, [_P(Desc), _P(TanBatch), _vp], (8, TanBatch)),
    ("hbvx_gage_route_tangent_batch", False, _int,
     [_P(GageDesc), _i32, _fp, _fp, _fp, _i64, _fp, _i64, _fp, _vp, _u64, _vp], None),
    ("hbvx_gage_route_tangent_workspace_bytes", False, _u64, [_P(GageDesc), _i32], None),
    ("hbvx_adj_tangent_batch", False, _int, [_P(Desc), _P(TanBatch), _fp, _vp], (8, TanBatch)),
    ("hbvx_gram", False, _int, [_P(GramDesc), _fp, _fp, _fp, _fp, _fp, _fp, _vp, _u64, _vp], (9, GramDesc)),
    ("hbvx_gram_workspace_bytes", False, _u64, [_P(GramDesc)], None),
    ("hbvx_quadform", False, _int, [_P(GramDesc), _fp, _fp, _fp, _vp, _u64, _vp], (9, GramDesc)),
    ("hbvx_quadform_workspace_bytes", False, _u64, [_P(GramDesc)], None),
] + [(_name, False, _int, [_P(Desc), _P(_e.struct), _vp], (_POP_SIZEOF[_e.struct], _e.struct))
     for _name, _e in POPULATION.items()]

EXPORTS = [row[0] for row in SIGNATURES if row[1]]
OPTIONAL_EXPORTS = [row[0] for row in SIGNATURES if not row[1]]

GAGE_POP_ABI_VERSION = 1    # HBVX_GAGE_POP_ABI_VERSION


class PopRunoff(C.Structure):
    """hbvx_pop_runoff: the candidates' static values and the [P,T,B] runoff they give (include/hbvx_gage_pop.h)."""
    _fields_ = [("abi_version", C.c_int32), ("n_cand", C.c_int32), ("p", PopSrc * MAX_PARAM), ("runoff", _fp)]


class GagePop(C.Structure):
    """hbvx_gage_pop: the candidates' runoff and routing parameters, the calendar, the observations per gage and the
    [P,G] outputs of hbvx_gage_population_stats (include/hbvx_gage_pop.h)."""
    _fields_ = [("abi_version", C.c_int32), ("n_cand", C.c_int32), ("runoff", _fp), ("runoff_c_stride", C.c_int64),
                ("dp", _fp), ("uh", _fp), ("transform", C.c_int32), ("n_periods", C.c_int32),
                ("period_end", C.c_void_p),     # const int32_t *: an address like the float pointers, of another type
                ("target", _fp), ("w", _fp), ("shift", _fp), ("eps", _fp),
                ("sse", _fp), ("s1", _fp), ("s2", _fp), ("s3", _fp), ("sim", _fp), ("series", _fp)]


# The exports of include/hbvx_gage_pop.h, rows as in SIGNATURES (all optional); the layout index is
# hbvx_gage_pop_sizeof's, not hbvx_sizeof's.
GAGE_POP_SIGNATURES = [
    ("hbvx_gage_pop_sizeof", False, _u64, [_int], None),
    ("hbvx_hourly_population_runoff", False, _int, [_P(Desc), _P(PopRunoff), _vp], (0, PopRunoff)),
    ("hbvx_gage_population_workspace_bytes", False, _u64, [_P(GageDesc), _P(GagePop)], (1, GagePop)),
    ("hbvx_gage_population_stats", False, _int, [_P(GageDesc), _P(GagePop), _vp, _u64, _vp], (1, GagePop)),
]


GAGE_EVENTS_ABI_VERSION = 1     # HBVX_GAGE_EVENTS_ABI_VERSION


class GageEvents(C.Structure):
    """hbvx_gage_events: the [P,T,G] hourly gage series, the [E,G] event windows and the [P,E,G] peaks, hours of the peak
    and volumes of hbvx_gage_population_events (include/hbvx_gage_events.h)."""
    _fields_ = [("abi_version", C.c_int32), ("n_cand", C.c_int32), ("T", C.c_int32), ("G", C.c_int32),
                ("n_events", C.c_int32), ("series", _fp),
                ("start", C.c_void_p), ("end", C.c_void_p),     # const int32_t *: addresses like the float pointers
                ("peak", _fp), ("peak_hour", C.c_void_p), ("volume", _fp)]


# The exports of include/hbvx_gage_events.h, rows as in SIGNATURES (all optional); the layout index is
# hbvx_gage_events_sizeof's.
GAGE_EVENTS_SIGNATURES = [
    ("hbvx_gage_events_sizeof", False, _u64, [_int], None),
    ("hbvx_gage_population_events", False, _int, [_P(GageEvents), _vp], (0, GageEvents)),
]


POP_FDC_ABI_VERSION = 1     # HBVX_POP_FDC_ABI_VERSION
POP_FDC_MAX_THR = 32        # HBVX_POP_FDC_MAX_THR

GAGE_FDC_ABI_VERSION = 1    # HBVX_GAGE_FDC_ABI_VERSION
GAGE_QUANT_MAX_T = 16384    # HBVX_GAGE_QUANT_MAX_T


class GageFdc(C.Structure):
    """hbvx_gage_fdc: the [P,T,G] hourly gage series, the [T,G] mask of the scored hours, and the [K,G] thresholds with
    their [P,K,G] counts and volumes (hbvx_gage_population_fdc) or the [K,G] ranks with their [P,K,G] quantiles
    (hbvx_gage_population_quantiles) -- include/hbvx_gage_fdc.h; K <= POP_FDC_MAX_THR."""
    _fields_ = [("abi_version", C.c_int32), ("n_cand", C.c_int32), ("T", C.c_int32), ("G", C.c_int32),
                ("n_lev", C.c_int32), ("series", _fp),
                ("scored", C.c_void_p),         # const uint8_t *: an address like the float pointers, of another type
                ("thr", _fp), ("count", C.c_void_p), ("volume", _fp),
                ("rank", C.c_void_p), ("quantile", _fp)]


# The exports of include/hbvx_gage_fdc.h, rows as in SIGNATURES (all optional); the layout index is
# hbvx_gage_fdc_sizeof's.
GAGE_FDC_SIGNATURES = [
    ("hbvx_gage_fdc_sizeof", False, _u64, [_int], None),
    ("hbvx_gage_population_fdc", False, _int, [_P(GageFdc), _vp], (0, GageFdc)),
    ("hbvx_gage_quantiles_workspace_bytes", False, _u64, [C.c_int32, C.c_int32, C.c_int32], None),
    ("hbvx_gage_population_quantiles", False, _int, [_P(GageFdc), _fp, _u64, _vp], (0, GageFdc)),
]


class PopFdc(C.Structure):
    """hbvx_pop_fdc: hbvx_pop_stats for the flow, the K thresholds per basin and the [P,K,B] exceedance counts and volumes
    of hbvx_population_fdc (include/hbvx_pop_fdc.h)."""
    _fields_ = [("abi_version", C.c_int32), ("n_thr", C.c_int32), ("flow", PopStats), ("thr", _fp),
                ("count", C.c_void_p),          # int32_t *: an address like the float pointers, of another type
                ("volume", _fp)]


# The exports of include/hbvx_pop_fdc.h, rows as in SIGNATURES (all optional; in neither SIGNATURES nor POPULATION); the
# layout index is hbvx_pop_fdc_sizeof's.
POP_FDC_SIGNATURES = [
    ("hbvx_pop_fdc_sizeof", False, _u64, [_int], None),
    ("hbvx_population_fdc", False, _int, [_P(Desc), _P(PopFdc), _vp], (0, PopFdc)),
]
POP_FDC_ENTRY = PopEntry(PopFdc, False, None)       # what ops.population_fdc needs to know about hbvx_population_fdc


POP_EVENTS_ABI_VERSION = 1  # HBVX_POP_EVENTS_ABI_VERSION


class PopEvents(C.Structure):
    """hbvx_pop_events: hbvx_pop_stats for the flow, the [E,B] event windows in scored days and the [P,E,B] peaks, days
    of the peak and volumes of hbvx_population_events (include/hbvx_pop_events.h)."""
    _fields_ = [("abi_version", C.c_int32), ("n_events", C.c_int32), ("flow", PopStats),
                ("start", C.c_void_p), ("end", C.c_void_p),     # const int32_t *: addresses like the float pointers
                ("peak", _fp), ("peak_day", C.c_void_p), ("volume", _fp)]


# The exports of include/hbvx_pop_events.h, rows as in SIGNATURES (all optional; in neither SIGNATURES nor POPULATION, as
# POP_FDC_SIGNATURES); the layout index is hbvx_pop_events_sizeof's.
POP_EVENTS_SIGNATURES = [
    ("hbvx_pop_events_sizeof", False, _u64, [_int], None),
    ("hbvx_population_events", False, _int, [_P(Desc), _P(PopEvents), _vp], (0, PopEvents)),
]
POP_EVENTS_ENTRY = PopEntry(PopEvents, False, None)     # what ops.population_events needs to know about the export


POP_ENS_HIST = 14           # HBVX_POP_ENS_HIST: the days of routing history a particle carries


class PopEns(C.Structure):
    """hbvx_pop_ens: hbvx_pop_stats over the window t_begin .. t_end-1, and per particle the storages, the routing
    history, the ancestor and the forcing perturbations of hbvx_population_ensemble (include/hbvx_pop_ens.h)."""
    _fields_ = [("s", PopStats), ("t_begin", C.c_int32), ("t_end", C.c_int32), ("n_src", C.c_int32),
                ("src_first", C.c_int32), ("state_in", _fp), ("state_out", _fp), ("hist_in", _fp), ("hist_out", _fp),
                ("ancestor", C.c_void_p),       # const int32_t *: an address like the float pointers, of another type
                ("p_mul", _fp), ("t_add", _fp), ("pm_c_stride", C.c_int64), ("pm_t_stride", C.c_int64),
                ("ta_c_stride", C.c_int64), ("ta_t_stride", C.c_int64)]


# The export of include/hbvx_pop_ens.h, a row as in SIGNATURES (optional; in neither SIGNATURES nor POPULATION, as
# POP_FDC_SIGNATURES); the layout index is hbvx_sizeof's.
POP_ENS_SIGNATURES = [
    ("hbvx_population_ensemble", False, _int, [_P(Desc), _P(PopEns), _vp], (14, PopEns)),
]
POP_ENS_ENTRY = PopEntry(PopEns, False, None)       # what ops.population_ensemble needs to know about the export


ENKF_MAX_ARRAYS = 4         # HBVX_ENKF_MAX_ARRAYS
ENKF_METHODS = {"perturbed": 0, "sqrt": 1}      # HBVX_ENKF_PERTURBED, HBVX_ENKF_SQRT


class EnkfArray(C.Structure):
    """hbvx_enkf_array: one array of particle values, [P,n] in and out, element e of basin (e / M) % B, floored at lo."""
    _fields_ = [("in_", _fp), ("out", _fp), ("n", C.c_int64), ("M", C.c_int32), ("lo", C.c_float)]


class Enkf(C.Structure):
    """hbvx_enkf: the analysis step of hbvx_enkf_update (include/hbvx_enkf.h)."""
    _fields_ = [("P", C.c_int32), ("B", C.c_int32), ("method", C.c_int32), ("n_arrays", C.c_int32),
                ("inflation", C.c_double), ("y", _fp), ("y_stride", C.c_int64), ("obs", _fp), ("obs_var", _fp),
                ("active", _fp), ("eps", _fp),
                ("status", C.c_void_p), ("stats", C.c_void_p),      # int32_t * / double *: addresses of another type
                ("a", EnkfArray * ENKF_MAX_ARRAYS)]


# The exports of include/hbvx_enkf.h, rows as in SIGNATURES (optional; a table of its own, as POP_EVENTS_SIGNATURES); the
# layout index is hbvx_enkf_sizeof's.
ENKF_SIGNATURES = [
    ("hbvx_enkf_sizeof", False, _u64, [_int], None),
    ("hbvx_enkf_update", False, _int, [_P(Enkf), _vp], (0, Enkf)),
]


# The export of include/hbvx_route_rows.h, a row as in SIGNATURES (optional, no struct of its own).
ROUTE_ROWS_SIGNATURES = [
    ("hbvx_route_backward_rows", False, _int, [_P(RouteDesc), _fp, _fp, _fp, _fp, _i32, _fp, _fp, _fp, _u64, _vp], None),
]

# The export of include/hbvx_live_rows.h, a row as in SIGNATURES (optional, no struct of its own).
E_UNSUPPORTED = -3      # HBVX_E_UNSUPPORTED
LIVE_ROWS_SIGNATURES = [
    ("hbvx_backward_live", False, _int, [_P(Desc), _P(BwdIO), _i32, _vp], None),
]


class HbvxError(RuntimeError):
    pass


class Library:
    """A loaded implementation of include/hbvx.h."""

    def __init__(self, path: str):
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        self.path = path
        self.dll = C.CDLL(path)
        d = self.dll
        for name in EXPORTS:
            if not hasattr(d, name):
                raise HbvxError(f"{path}: missing export {name}")
        self.missing = [name for name in OPTIONAL_EXPORTS +
                        [row[0] for row in GAGE_POP_SIGNATURES + ROUTE_ROWS_SIGNATURES + LIVE_ROWS_SIGNATURES +
                         POP_FDC_SIGNATURES + GAGE_EVENTS_SIGNATURES + POP_EVENTS_SIGNATURES + GAGE_FDC_SIGNATURES +
                         POP_ENS_SIGNATURES + ENKF_SIGNATURES]
                        if not hasattr(d, name)]
        checked = set()             # (sizeof export, index): several exports share a struct
        # the required rows come first, and each table's sizeof export before the rows that name a layout: it is bound by then
        for name, _, restype, argtypes, layout, sizeof in [row + ("hbvx_sizeof",) for row in SIGNATURES] + \
                [row + ("hbvx_gage_pop_sizeof",) for row in GAGE_POP_SIGNATURES] + \
                [row + ("hbvx_sizeof",) for row in ROUTE_ROWS_SIGNATURES + LIVE_ROWS_SIGNATURES + POP_ENS_SIGNATURES] + \
                [row + ("hbvx_enkf_sizeof",) for row in ENKF_SIGNATURES] + \
                [row + ("hbvx_pop_fdc_sizeof",) for row in POP_FDC_SIGNATURES] + \
                [row + ("hbvx_gage_events_sizeof",) for row in GAGE_EVENTS_SIGNATURES] + \
                [row + ("hbvx_pop_events_sizeof",) for row in POP_EVENTS_SIGNATURES] + \
                [row + ("hbvx_gage_fdc_sizeof",) for row in GAGE_FDC_SIGNATURES]:
            if name in self.missing:
                continue
            fn = getattr(d, name)
            fn.restype, fn.argtypes = restype, argtypes
            if layout is not None and (sizeof, layout[0]) not in checked and sizeof not in self.missing:
                checked.add((sizeof, layout[0]))
                which, st = layout
                got = getattr(d, sizeof)(which)
                if got != C.sizeof(st):
                    raise HbvxError(f"{path}: layout mismatch for {st.__name__}: {got} != {C.sizeof(st)}")
        if d.hbvx_version() != ABI_VERSION:
            raise HbvxError(f"{path}: ABI version {d.hbvx_version()} != {ABI_VERSION}")
        for which, st in enumerate([Desc, FwdOut, BwdIO, RouteDesc, ParamSrc, ParamGrad, GageDesc]):
            if d.hbvx_sizeof(which) != C.sizeof(st):
                raise HbvxError(f"{path}: layout mismatch for {st.__name__}: "
                                f"{d.hbvx_sizeof(which)} != {C.sizeof(st)}")
        self.backend = d.hbvx_backend().decode()

    @property
    def is_device(self) -> bool:
        return self.backend.startswith("hip")

    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self.dll.hbvx_last_error().decode(errors="replace")
            raise HbvxError(f"{what} failed ({rc}): {msg}")

    def forward(self, desc: Desc, out: FwdOut, stream: int):
        self._check(self.dll.hbvx_forward(C.byref(desc), C.byref(out), C.c_void_p(stream)),
                    "hbvx_forward")

    def backward(self, desc: Desc, io: BwdIO, stream: int):
        self._check(self.dll.hbvx_backward(C.byref(desc), C.byref(io), C.c_void_p(stream)),
                    "hbvx_backward")

    def backward_live(self, desc: Desc, io: BwdIO, n_live4: int, stream: int) -> bool:
        """hbvx_backward with io.grad_flux4 of n_live4 rows (include/hbvx_live_rows.h).  False: the library refused
        the call before launching anything (HBVX_E_UNSUPPORTED: no kernel that knows about the missing rows takes
        it) -- clear the dead rows of a [4,T,B] buffer and call `backward`."""
        self.require("hbvx_backward_live")
        if not 1 <= n_live4 <= 4:
            raise ValueError(f"n_live4 must be 1 .. 4, got {n_live4}")
        rc = self.dll.hbvx_backward_live(C.byref(desc), C.byref(io), n_live4, C.c_void_p(stream))
        if rc == E_UNSUPPORTED:
            return False
        self._check(rc, "hbvx_backward_live")
        return True

    def zero_rest(self, ptr: int, nbytes: int, state_ptr: int, stream: int):
        """Zero what the forward's launch left of FwdOut.zero_ptr (include/hbvx.h)."""
        self._check(self.dll.hbvx_zero_rest(C.c_void_p(ptr), nbytes, C.c_void_p(state_ptr), C.c_void_p(stream)), "hbvx_zero_rest")

    def zero_in_launch(self) -> bool:
        """Whether the last forward call of this thread wrote FwdOut.zero_ptr inside its own launch (include/hbvx.h)."""
        return bool(self.dll.hbvx_zero_in_launch())

    def last_dispatch(self, direction: int) -> str:
        """Kernel family of the last forward (0) / adjoint (1) call (diagnostic, include/hbvx.h)."""
        return self.dll.hbvx_last_dispatch(direction).decode()

    def preferred_traj_layout(self, desc: Desc) -> int:
        return int(self.dll.hbvx_preferred_traj_layout(C.byref(desc)))

    def ckpt_workspace_bytes(self, desc: Desc, K: int) -> int:
        return int(self.dll.hbvx_ckpt_workspace_bytes(C.byref(desc), K))

    def backward_workspace_bytes(self, desc: Desc) -> int:
        return int(self.dll.hbvx_backward_workspace_bytes(C.byref(desc)))

    def adj_forward(self, desc: Desc, out: FwdOut, stream: int):
        self._check(self.dll.hbvx_adj_forward(C.byref(desc), C.byref(out), C.c_void_p(stream)),
                    "hbvx_adj_forward")

    def adj_backward(self, desc: Desc, io: BwdIO, stream: int):
        self._check(self.dll.hbvx_adj_backward(C.byref(desc), C.byref(io), C.c_void_p(stream)),
                    "hbvx_adj_backward")

    def gage_route_workspace_bytes(self, r: GageDesc) -> int:
        return int(self.dll.hbvx_gage_route_workspace_bytes(C.byref(r)))

    def gage_route_forward(self, r: GageDesc, qs: int, uh: int, out: int, ws, ws_bytes: int, stream: int):
        self._check(self.dll.hbvx_gage_route_forward(C.byref(r), qs, uh, out, ws, C.c_uint64(ws_bytes),
                                                     C.c_void_p(stream)), "hbvx_gage_route_forward")

    def gage_route_backward(self, r: GageDesc, qs: int, uh: int, go: int, gqs: int, gdp: int, ws,
                            ws_bytes: int, stream: int):
        self._check(self.dll.hbvx_gage_route_backward(C.byref(r), qs, uh, go, gqs, gdp, ws,
                                                      C.c_uint64(ws_bytes), C.c_void_p(stream)),
                    "hbvx_gage_route_backward")

    def zero(self, ptr: int, nbytes: int, stream: int):
        self._check(self.dll.hbvx_zero(ptr, C.c_uint64(nbytes), C.c_void_p(stream)), "hbvx_zero")

    def zero_except(self, ptr: int, rows: int, width: int, r0: int, r1: int, group_w: int, keep: int,
                    stream: int):
        self._check(self.dll.hbvx_zero_except(ptr, rows, width, r0, r1, group_w, C.c_uint32(keep),
                                              C.c_void_p(stream)), "hbvx_zero_except")

    def lstm_workspace_bytes(self, r: LstmDesc) -> int:
        return int(self.dll.hbvx_lstm_workspace_bytes(C.byref(r)))

    def lstm_forward(self, r: LstmDesc, w_hh: int, gx: int, gates: int, c_all: int, h_all: int, ws,
                     ws_bytes: int, stream: int):
        self._check(self.dll.hbvx_lstm_forward(C.byref(r), w_hh, gx, gates, c_all, h_all, ws,
                                               C.c_uint64(ws_bytes), C.c_void_p(stream)), "hbvx_lstm_forward")

    def lstm_backward(self, r: LstmDesc, w_hh: int, gates: int, c_all: int, gh: int, gg: int, ws,
                      ws_bytes: int, stream: int):
        self._check(self.dll.hbvx_lstm_backward(C.byref(r), w_hh, gates, c_all, gh, gg, ws,
                                                C.c_uint64(ws_bytes), C.c_void_p(stream)), "hbvx_lstm_backward")

    def require(self, name: str):
        """Raises HbvxError if this library lacks the optional export `name`."""
        if name in self.missing:
            raise HbvxError(f"{self.path}: missing export {name} (backend {self.backend!r})")

    def lstm_forward_hx(self, r: LstmDesc, w_hh: int, gx: int, h0, c0, gates: int, c_all: int, h_all: int, ws,
                        ws_bytes: int, stream: int):
        self.require("hbvx_lstm_forward_hx")
        self._check(self.dll.hbvx_lstm_forward_hx(C.byref(r), w_hh, gx, h0, c0, gates, c_all, h_all, ws,
                                                  C.c_uint64(ws_bytes), C.c_void_p(stream)), "hbvx_lstm_forward_hx")

    def lstm_backward_hx(self, r: LstmDesc, w_hh: int, gates: int, c0, c_all: int, gh: int, gc_last, gg: int, gc0,
                         ws, ws_bytes: int, stream: int):
        self.require("hbvx_lstm_backward_hx")
        self._check(self.dll.hbvx_lstm_backward_hx(C.byref(r), w_hh, gates, c0, c_all, gh, gc_last, gg, gc0, ws,
                                                   C.c_uint64(ws_bytes), C.c_void_p(stream)), "hbvx_lstm_backward_hx")

    def lstm_tangent(self, r: LstmDesc, w_hh: int, gates: int, c0, c_all: int, gx_t: int, h0_t, c0_t, h_t: int,
                     c_t_last, ws, ws_bytes: int, stream: int):
        self.require("hbvx_lstm_tangent")
        self._check(self.dll.hbvx_lstm_tangent(C.byref(r), w_hh, gates, c0, c_all, gx_t, h0_t, c0_t, h_t, c_t_last, ws,
                                               C.c_uint64(ws_bytes), C.c_void_p(stream)), "hbvx_lstm_tangent")

    def lstm_tangent_batch_workspace_bytes(self, r: LstmDesc, n_dir: int) -> int:
        self.require("hbvx_lstm_tangent_batch_workspace_bytes")
        return int(self.dll.hbvx_lstm_tangent_batch_workspace_bytes(C.byref(r), n_dir))

    def lstm_tangent_batch(self, r: LstmDesc, n_dir: int, w_hh: int, gates: int, c0, c_all: int, gx_t: int, h0_t,
                           c0_t, h_t: int, c_t_last, ws, ws_bytes: int, stream: int):
        self.require("hbvx_lstm_tangent_batch")
        self._check(self.dll.hbvx_lstm_tangent_batch(C.byref(r), n_dir, w_hh, gates, c0, c_all, gx_t, h0_t, c0_t, h_t,
                                                     c_t_last, ws, C.c_uint64(ws_bytes), C.c_void_p(stream)),
                    "hbvx_lstm_tangent_batch")

    def forward_tangent(self, desc: Desc, io: TanIO, stream: int):
        self.require("hbvx_forward_tangent")
        self._check(self.dll.hbvx_forward_tangent(C.byref(desc), C.byref(io), C.c_void_p(stream)), "hbvx_forward_tangent")

    def route_tangent(self, r: RouteDesc, q: int, uh: int, q_dot, ra_dot, rb_dot, q_rout_dot: int, stream: int):
        self.require("hbvx_route_tangent")
        self._check(self.dll.hbvx_route_tangent(C.byref(r), q, uh, q_dot, ra_dot, rb_dot, q_rout_dot,
                                                C.c_void_p(stream)), "hbvx_route_tangent")

    def bfi_tangent(self, T: int, B: int, qs: int, q2: int, qs_dot, q2_dot, nearzero: float, out: int, stream: int):
        self.require("hbvx_bfi_tangent")
        self._check(self.dll.hbvx_bfi_tangent(T, B, qs, q2, qs_dot, q2_dot, C.c_float(nearzero), out,
                                              C.c_void_p(stream)), "hbvx_bfi_tangent")

    def forward_tangent_batch(self, desc: Desc, tb: TanBatch, stream: int):
        self.require("hbvx_forward_tangent_batch")
        self._check(self.dll.hbvx_forward_tangent_batch(C.byref(desc), C.byref(tb), C.c_void_p(stream)),
                    "hbvx_forward_tangent_batch")

    def route_tangent_batch(self, r: RouteDesc, n_dir: int, q: int, uh: int, q_dot, q_dot_ds: int, ra_dot, rb_dot,
                            r_ds: int, q_rout_dot: int, stream: int):
        self.require("hbvx_route_tangent_batch")
        self._check(self.dll.hbvx_route_tangent_batch(C.byref(r), n_dir, q, uh, q_dot, q_dot_ds, ra_dot, rb_dot, r_ds,
                                                      q_rout_dot, C.c_void_p(stream)), "hbvx_route_tangent_batch")

    def bfi_tangent_batch(self, T: int, B: int, n_dir: int, qs: int, q2: int, qs_dot, q2_dot, dot_ds: int,
                          nearzero: float, out: int, stream: int):
        self.require("hbvx_bfi_tangent_batch")
        self._check(self.dll.hbvx_bfi_tangent_batch(T, B, n_dir, qs, q2, qs_dot, q2_dot, dot_ds, C.c_float(nearzero),
                                                    out, C.c_void_p(stream)), "hbvx_bfi_tangent_batch")

    def hourly_tangent_batch(self, desc: Desc, tb: TanBatch, stream: int):
        self.require("hbvx_hourly_tangent_batch")
        self._check(self.dll.hbvx_hourly_tangent_batch(C.byref(desc), C.byref(tb), C.c_void_p(stream)),
                    "hbvx_hourly_tangent_batch")

    def adj_tangent_batch(self, desc: Desc, tb: TanBatch, traj, stream: int):
        self.require("hbvx_adj_tangent_batch")
        self._check(self.dll.hbvx_adj_tangent_batch(C.byref(desc), C.byref(tb), traj, C.c_void_p(stream)),
                    "hbvx_adj_tangent_batch")

    def gram_workspace_bytes(self, g: GramDesc) -> int:
        self.require("hbvx_gram_workspace_bytes")
        return int(self.dll.hbvx_gram_workspace_bytes(C.byref(g)))

    def gram(self, g: GramDesc, s: int, w, r, gram: int, rhs, cost, ws, ws_bytes: int, stream: int):
        self.require("hbvx_gram")
        self._check(self.dll.hbvx_gram(C.byref(g), s, w, r, gram, rhs, cost, ws, C.c_uint64(ws_bytes),
                                       C.c_void_p(stream)), "hbvx_gram")

    def quadform_workspace_bytes(self, g: GramDesc) -> int:
        self.require("hbvx_quadform_workspace_bytes")
        return int(self.dll.hbvx_quadform_workspace_bytes(C.byref(g)))

    def quadform(self, g: GramDesc, s: int, m: int, q: int, ws, ws_bytes: int, stream: int):
        self.require("hbvx_quadform")
        self._check(self.dll.hbvx_quadform(C.byref(g), s, m, q, ws, C.c_uint64(ws_bytes), C.c_void_p(stream)),
                    "hbvx_quadform")

    def gage_route_tangent_workspace_bytes(self, r: GageDesc, n_dir: int) -> int:
        self.require("hbvx_gage_route_tangent_workspace_bytes")
        return int(self.dll.hbvx_gage_route_tangent_workspace_bytes(C.byref(r), n_dir))

    def gage_route_tangent_batch(self, r: GageDesc, n_dir: int, qs: int, uh: int, qs_dot, qs_dot_ds: int, dp_dot,
                                 dp_dot_ds: int, out_dot: int, ws, ws_bytes: int, stream: int):
        self.require("hbvx_gage_route_tangent_batch")
        self._check(self.dll.hbvx_gage_route_tangent_batch(C.byref(r), n_dir, qs, uh, qs_dot, qs_dot_ds, dp_dot,
                                                           dp_dot_ds, out_dot, ws, C.c_uint64(ws_bytes),
                                                           C.c_void_p(stream)), "hbvx_gage_route_tangent_batch")

    def hourly_population_runoff(self, desc, pr, stream: int):
        """hbvx_hourly_population_runoff; `desc` / `pr` may be None (the ABI's own refusals are under test)."""
        self.require("hbvx_hourly_population_runoff")
        self._check(self.dll.hbvx_hourly_population_runoff(None if desc is None else C.byref(desc),
                                                           None if pr is None else C.byref(pr), C.c_void_p(stream)),
                    "hbvx_hourly_population_runoff")

    def gage_population_workspace_bytes(self, r, gp) -> int:
        self.require("hbvx_gage_population_workspace_bytes")
        return int(self.dll.hbvx_gage_population_workspace_bytes(None if r is None else C.byref(r),
                                                                 None if gp is None else C.byref(gp)))

    def gage_population_stats(self, r, gp, ws, ws_bytes: int, stream: int):
        """hbvx_gage_population_stats; `r` / `gp` may be None (the ABI's own refusals are under test)."""
        self.require("hbvx_gage_population_stats")
        self._check(self.dll.hbvx_gage_population_stats(None if r is None else C.byref(r),
                                                        None if gp is None else C.byref(gp), ws, C.c_uint64(ws_bytes),
                                                        C.c_void_p(stream)), "hbvx_gage_population_stats")

    def gage_population_events(self, ev, stream: int):
        """hbvx_gage_population_events; `ev` may be None (the ABI's own refusals are under test)."""
        self.require("hbvx_gage_population_events")
        self._check(self.dll.hbvx_gage_population_events(None if ev is None else C.byref(ev), C.c_void_p(stream)),
                    "hbvx_gage_population_events")

    def gage_population_fdc(self, gf, stream: int):
        """hbvx_gage_population_fdc; `gf` may be None (the ABI's own refusals are under test)."""
        self.require("hbvx_gage_population_fdc")
        self._check(self.dll.hbvx_gage_population_fdc(None if gf is None else C.byref(gf), C.c_void_p(stream)),
                    "hbvx_gage_population_fdc")

    def gage_quantiles_workspace_bytes(self, n_cand: int, T: int, G: int) -> int:
        self.require("hbvx_gage_quantiles_workspace_bytes")
        return int(self.dll.hbvx_gage_quantiles_workspace_bytes(n_cand, T, G))

    def gage_population_quantiles(self, gf, ws, ws_bytes: int, stream: int):
        """hbvx_gage_population_quantiles; `gf` may be None (the ABI's own refusals are under test)."""
        self.require("hbvx_gage_population_quantiles")
        self._check(self.dll.hbvx_gage_population_quantiles(None if gf is None else C.byref(gf), ws, C.c_uint64(ws_bytes),
                                                            C.c_void_p(stream)), "hbvx_gage_population_quantiles")

    def lstm_check(self, r: LstmDesc, ws, stream: int):
        self._check(self.dll.hbvx_lstm_check(C.byref(r), ws, C.c_void_p(stream)), "hbvx_lstm_check")

    def bfi(self, T: int, B: int, qs: int, q2: int, nearzero: float, out: int, stream: int):
        self._check(self.dll.hbvx_bfi(T, B, qs, q2, C.c_float(nearzero), out, C.c_void_p(stream)),
                    "hbvx_bfi")

    def route_forward(self, r: RouteDesc, q: int, uh: int, q_rout: int, stream: int):
        self._check(self.dll.hbvx_route_forward(C.byref(r), q, uh, q_rout, C.c_void_p(stream)),
                    "hbvx_route_forward")

    def route_workspace_bytes(self, r: RouteDesc) -> int:
        return int(self.dll.hbvx_route_workspace_bytes(C.byref(r)))

    def route_backward(self, r: RouteDesc, q: int, uh: int, gqr: int, gq: int, gra, grb,
                       ws, ws_bytes: int, stream: int):
        self._check(self.dll.hbvx_route_backward(C.byref(r), q, uh, gqr, gq, gra, grb, ws,
                                                 C.c_uint64(ws_bytes), C.c_void_p(stream)),
                    "hbvx_route_backward")

    def enkf_update(self, e, stream: int) -> int:
        """hbvx_enkf_update; `e` may be None (the ABI's own refusals are under test).  Raises HbvxError with the
        library's text on a negative return code."""
        self.require("hbvx_enkf_update")
        self._check(self.dll.hbvx_enkf_update(None if e is None else C.byref(e), C.c_void_p(stream)), "hbvx_enkf_update")

    def route_backward_rows(self, r: RouteDesc, q: int, uh: int, gqr: int, gq: int, gq_rows: int, gra, grb,
                            ws, ws_bytes: int, stream: int):
        """hbvx_route_backward into a grad_q of gq_rows >= r.S rows: the launch zeroes the rows from r.S on."""
        self.require("hbvx_route_backward_rows")
        self._check(self.dll.hbvx_route_backward_rows(C.byref(r), q, uh, gqr, gq, gq_rows, gra, grb, ws,
                                                      C.c_uint64(ws_bytes), C.c_void_p(stream)),
                    "hbvx_route_backward_rows")


def _population_method(entry: str, struct=None):
    struct = struct or POPULATION[entry].struct

    def call(self, desc, args, stream: int):
        self.require(entry)
        self._check(getattr(self.dll, entry)(None if desc is None else C.byref(desc),
                                             None if args is None else C.byref(args), C.c_void_p(stream)), entry)
    call.__name__ = entry[len("hbvx_"):]
    call.__doc__ = (f"{entry}; `desc` / `args` (its {struct.__name__}) may be None (the ABI's own "
                    "refusals are under test).")
    return call


for _name in POPULATION:        # Library.population_cost(desc, pop, stream) ... Library.adj_population_period(desc, pq, stream)
    setattr(Library, _name[len("hbvx_"):], _population_method(_name))
Library.population_fdc = _population_method("hbvx_population_fdc", PopFdc)       # (desc, pf, stream)
Library.population_events = _population_method("hbvx_population_events", PopEvents)     # (desc, pe, stream)
Library.population_ensemble = _population_method("hbvx_population_ensemble", PopEns)    # (desc, pe, stream)
