"""ctypes binding of libivs.so (the C ABI in include/ivs.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C iv_interpolation_amd/csrc``.
There is NO CPU fallback: if the shared object is missing or no HIP device is visible the
product path raises ``EngineUnavailable``.
"""
from __future__ import annotations

import ctypes as C
import os

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libivs.so")

LINEAR, CUBIC, CUBICSPLINE, SLINEAR = 0, 1, 2, 3
ST_OK, ST_TOO_FEW_KNOTS, ST_BAD_SHAPE, ST_ILL_CONDITIONED = 0, 1, 2, 4
SM_OK, SM_NO_CROSSING, SM_AMBIGUOUS, SM_DEAD = 0, 1, 2, 4      # IVS_SM_*: per-target flags of the smile points
SM_MAX_TARGETS = 16
AR_CALENDAR, AR_BUTTERFLY, AR_NO_STENCIL, AR_DEAD = 1, 2, 4, 8    # IVS_AR_*: per-node flags of the arbitrage report
# IVS_MM_*: per-row flags of the model-free moments, NO_BRACKET on the index only
MM_ONE_SIDED, MM_TRUNCATED, MM_HOLES, MM_DEAD, MM_NO_BRACKET = 1, 2, 4, 8, 16
MM_MAX_HORIZONS = 8
# IVS_SV_*: per-row flags of the SVI slices
SV_BOUND, SV_EDGE, SV_HOLES, SV_DEAD, SV_BUTTERFLY, SV_DEGENERATE = 1, 2, 4, 8, 16, 32
SV_MAX_ROUNDS = 24
# IVS_DS_*: flags of the risk-neutral distribution; NO_BRACKET / AMBIGUOUS per target, TAILS per row, DEAD on both
DS_NO_BRACKET, DS_AMBIGUOUS, DS_TAILS, DS_DEAD = 1, 2, 4, 8
DS_MAX_PROBS, DS_MAX_LEVELS = 16, 16
# IVS_SC_*: per-pair flags of the SVI calendar report; IVS_SE_*: per-query flags of the SVI surface evaluation
SC_CALENDAR, SC_WING_LEFT, SC_WING_RIGHT, SC_DEAD, SC_LAST, SC_UNORDERED = 1, 2, 4, 8, 16, 32
SE_SHORT, SE_LONG, SE_NEG_FWD, SE_DEAD, SE_NEG_G, SE_UNORDERED = 1, 2, 4, 8, 16, 32
ST_MAX_TENORS, SC_MAX_ROWS_PER_WAVE = 64, 32
# IVS_SB_*: per-cell flags of the scenario grid of a book, one bit per dynamic
SB_NEG_VOL_SS, SB_NEG_VOL_SM = 1, 2
RK_MAX_SHOCKS, RK_MAX_GRID = 64, 1024
# IVS_HS_*: per-scenario flags of the historical simulation
HS_ABSENT, HS_VOID_PAIR, HS_NEG_VOL = 1, 2, 4
HS_MAX_WINDOW, HS_MAX_LEVELS = 1024, 8
HA_MAX_TAIL, HA_MAX_GROUPS = 64, 16
# IVS_HG_*: per-candidate flags of the minimum-variance hedge; CHOSEN is informative, the others block a candidate
HG_DEAD, HG_NEG_VOL, HG_FLAT, HG_SPENT, HG_CHOSEN = 1, 2, 4, 8, 16
HG_MAX_INST, HG_MAX_ROUNDS = 64, 8
HG_CALL, HG_PUT, HG_UNDERLYING = 0, 1, 2                         # inst_kind
WI_MAX_RUNGS = 16                                                # sizes per candidate of the what-if ladder
BOOT_MAX_REP, BOOT_MAX_BLOCK, BOOT_MAX_CI = 1024, 1024, 8        # replicates, block length and interval probabilities of the bootstrap
HW_NO_VOL, HW_BAD_WEIGHT = 8, 16                                 # IVS_HW_*: the bits the weighted tail adds to IVS_HS_*
HW_MAX_SPAN = 1024                                               # returns per running vol of the spot
# IVS_SS_*: per-row flags of the SSVI surface; IVS_SF_*: its per-snapshot flags
SS_RAISED, SS_HOLES, SS_DEAD, SS_BUTTERFLY = 1, 4, 8, 16
SF_EDGE_RHO, SF_EDGE_GAMMA, SF_EDGE_ETA_LOW, SF_SURF_DEAD, SF_AT_BOUND, SF_UNORDERED = 1, 2, 4, 8, 16, 32
SS_MAX_ROUNDS, SS_MAX_NODES = 32, 3072
# IVS_IV_*: per-option flags of the implied-vol solver (the pricer knows DEAD only)
IV_ITM, IV_BELOW, IV_ABOVE, IV_DEAD, IV_EDGE = 1, 2, 4, 8, 16
FLAG_FORCE_GENERIC = 1
FLAG_ONE_PASS = 2          # IVS_FLAG_ONE_PASS: skip the row-pass kernels (testing / A-B timing)


def flag_map_groups(n: int) -> int:
    """IVS_FLAG_MAP_GROUPS(n): tuning override of the 64x16 kernel's surface -> workgroup mapping (0 = default)."""
    return (int(n) & 0xff) << 8

ABI_VERSION = 5

# pandas method names (reference core.py:61 forwards self.method) -> engine codes
NEAREST, ZERO, PCHIP, AKIMA, FROM_DERIVATIVES = 4, 5, 6, 7, 8
QUADRATIC = 9
BARYCENTRIC, KROGH = 10, 11
PAD, BFILL = 12, 13        # pandas' fill methods, which Series.interpolate still executes (pad_or_backfill)
POLY_MAX_KNOTS = 32
METHOD_CODES = {"linear": LINEAR, "index": LINEAR, "values": LINEAR,
                "cubic": CUBIC, "cubicspline": CUBICSPLINE, "slinear": SLINEAR,
                "nearest": NEAREST, "zero": ZERO, "pchip": PCHIP, "akima": AKIMA,
                "from_derivatives": FROM_DERIVATIVES, "piecewise_polynomial": FROM_DERIVATIVES, "quadratic": QUADRATIC,
                "barycentric": BARYCENTRIC, "krogh": KROGH,
                "pad": PAD, "ffill": PAD, "bfill": BFILL, "backfill": BFILL}


def method_code(name) -> int:
    """Engine code of a pandas method name, or KeyError.  pandas matches the FILL methods case-insensitively
    (`method.lower() in fillna_methods`, verified against the reference: 'PAD', 'Backfill' work) and every other name
    exactly ('Linear' raises -> None)."""
    if name in METHOD_CODES:
        return METHOD_CODES[name]
    if isinstance(name, str) and name.lower() in ("pad", "ffill", "bfill", "backfill"):
        return METHOD_CODES[name.lower()]
    raise KeyError(name)


class EngineUnavailable(RuntimeError):
    """libivs.so missing / not loadable / no MI355X visible.  Never swallowed by the host code."""


class EngineError(RuntimeError):
    """A C-ABI call returned a negative code."""


_p = C.c_void_p
_i64, _i32, _sz = C.c_int64, C.c_int32, C.c_size_t



class FrameArgs(C.Structure):
    """ivs_frame_args of include/ivs.h (field for field)."""
    _fields_ = [("src_pos", _p), ("src_off", _p), ("q_off", _p),
                ("n_series", _i64), ("total_src", _i64), ("total_queries", _i64),
                ("yk", _p), ("yk_stride", _i64), ("n_channels", _i32), ("method", _i32),
                ("chan_out", _p), ("chan_stride", _i64), ("status", _p),
                ("valid", _p), ("valid_stride", _i64), ("n_valid", _i32),
                ("fsrc", _p), ("fsrc_stride", _i64), ("f_rows", _p), ("n_f", _i32), ("f_out", _p), ("f_stride", _i64),
                ("csrc", _p), ("csrc_stride", _i64), ("c_rows", _p), ("n_c", _i32), ("c_out", _p), ("c_stride", _i64),
                ("idx_rows", _p), ("n_idx", _i32), ("idx_out", _p), ("idx_stride", _i64),
                ("first_ns", _p), ("needs", _p), ("sym_col", _i32), ("date_ns", _p), ("keep", _p),
                ("g_strike", _i32), ("g_rate", _i32), ("g_put", _i32), ("strike_src", _p), ("rate_src", _p), ("put_src", _p),
                ("ch_iv", _i32), ("ch_underlying", _i32), ("ch_ttm", _i32), ("greeks", _p), ("greeks_stride", _i64)]


class SnapshotArgs(C.Structure):
    """ivs_snapshot_args of include/ivs.h (field for field)."""
    _fields_ = [("date_ns", _p), ("iv", _p), ("underlying", _p), ("n_rows", _i64),
                ("row_off", _p), ("n_contracts", _i64),
                ("cells", _p), ("strike", _p), ("expiry_ns", _p), ("nT", _i32), ("nK", _i32),
                ("t0_ns", _i64), ("n_snapshots", _i64),
                ("moneyness", _p), ("mK", _i32), ("kq_empty", C.c_double),
                ("sigma", _p), ("T", _p), ("spot", _p), ("quotes", _p), ("Kq", _p)]


class SmileArgs(C.Structure):
    """ivs_smile_args of include/ivs.h (field for field)."""
    _fields_ = [("vol", _p), ("Kq", _p), ("kq_stride", _i64), ("Tq", _p), ("tq_stride", _i64),
                ("spot", _p), ("rate", C.c_double), ("z", C.POINTER(C.c_double)),
                ("mK", _i32), ("mT", _i32), ("nD", _i32), ("B", _i64),
                ("q_vol", _p), ("q_strike", _p), ("q_flags", _p), ("rows_per_wave", _i32)]


class ArbitrageArgs(C.Structure):
    """ivs_arbitrage_args of include/ivs.h (field for field)."""
    _fields_ = [("vol", _p), ("Kq", _p), ("kq_stride", _i64), ("Tq", _p), ("tq_stride", _i64),
                ("spot", _p), ("rate", C.c_double), ("mK", _i32), ("mT", _i32), ("B", _i64),
                ("flags", _p), ("counts", _p), ("worst", _p), ("local_vol", _p), ("density", _p)]


class MomentsArgs(C.Structure):
    """ivs_moments_args of include/ivs.h (field for field)."""
    _fields_ = [("vol", _p), ("Kq", _p), ("kq_stride", _i64), ("Tq", _p), ("tq_stride", _i64),
                ("spot", _p), ("rate", C.c_double), ("min_mass", C.c_double),
                ("horizons", C.POINTER(C.c_double)), ("nH", _i32), ("mK", _i32), ("mT", _i32), ("B", _i64),
                ("raw", _p), ("stats", _p), ("mass", _p), ("flags", _p), ("index", _p), ("index_flags", _p),
                ("snapshots_per_wg", _i32)]


class SviArgs(C.Structure):
    """ivs_svi_args of include/ivs.h (field for field)."""
    _fields_ = [("vol", _p), ("Kq", _p), ("kq_stride", _i64), ("Tq", _p), ("tq_stride", _i64),
                ("spot", _p), ("rate", C.c_double), ("mK", _i32), ("mT", _i32), ("B", _i64), ("rounds", _i32),
                ("params", _p), ("fit", _p), ("flags", _p), ("fitted", _p), ("rows_per_wg", _i32)]


class DistributionArgs(C.Structure):
    """ivs_distribution_args of include/ivs.h (field for field)."""
    _fields_ = [("params", _p), ("Tq", _p), ("tq_stride", _i64), ("spot", _p), ("rate", C.c_double), ("max_tail", C.c_double),
                ("probs", C.POINTER(C.c_double)), ("nP", _i32), ("levels", C.POINTER(C.c_double)), ("nL", _i32),
                ("mT", _i32), ("B", _i64),
                ("q_x", _p), ("q_strike", _p), ("q_flags", _p), ("p_below", _p), ("p_above", _p), ("tails", _p), ("flags", _p),
                ("rows_per_wave", _i32)]


class CalendarArgs(C.Structure):
    """ivs_calendar_args of include/ivs.h (field for field)."""
    _fields_ = [("params", _p), ("Tq", _p), ("tq_stride", _i64), ("spot", _p), ("mT", _i32), ("B", _i64),
                ("d_min", _p), ("x_min", _p), ("d_atm", _p), ("x_cross", _p), ("n_cross", _p), ("flags", _p),
                ("rows_per_wave", _i32)]


class EvalArgs(C.Structure):
    """ivs_eval_args of include/ivs.h (field for field)."""
    _fields_ = [("params", _p), ("Tq", _p), ("tq_stride", _i64), ("spot", _p), ("rate", C.c_double),
                ("u", _p), ("tau", _p), ("q_stride", _i64), ("strike_mode", _i32), ("mT", _i32), ("Q", _i64), ("B", _i64),
                ("w", _p), ("vol", _p), ("call", _p), ("put", _p), ("fwd_var", _p), ("g", _p), ("local_vol", _p), ("flags", _p)]


class GreeksArgs(C.Structure):
    """ivs_greeks_args of include/ivs.h (field for field)."""
    _fields_ = [("params", _p), ("Tq", _p), ("tq_stride", _i64), ("spot", _p), ("rate", C.c_double),
                ("u", _p), ("tau", _p), ("q_stride", _i64), ("is_put", _p), ("strike_mode", _i32), ("mT", _i32), ("Q", _i64), ("B", _i64),
                ("price", _p), ("delta_ss", _p), ("delta_sm", _p), ("gamma_ss", _p), ("gamma_sm", _p), ("vega", _p), ("theta", _p),
                ("flags", _p)]


class BookArgs(C.Structure):
    """ivs_book_args of include/ivs.h (field for field)."""
    _fields_ = [("params", _p), ("Tq", _p), ("tq_stride", _i64), ("spot", _p), ("rate", C.c_double),
                ("u", _p), ("tau", _p), ("q_stride", _i64), ("is_put", _p), ("qty", _p), ("strike_mode", _i32), ("mT", _i32),
                ("Q", _i64), ("B", _i64),
                ("spot_shocks", C.POINTER(C.c_double)), ("nA", _i32), ("vol_shocks", C.POINTER(C.c_double)), ("nV", _i32),
                ("net", _p), ("n_dead", _p), ("pnl_ss", _p), ("pnl_sm", _p), ("cell_flags", _p), ("cells_per_wg", _i32)]


class ExplainArgs(C.Structure):
    """ivs_explain_args of include/ivs.h (field for field)."""
    _fields_ = [("params", _p), ("Tq", _p), ("tq_stride", _i64), ("spot", _p), ("rate", C.c_double),
                ("u", _p), ("tau", _p), ("q_stride", _i64), ("is_put", _p), ("qty", _p), ("strike_mode", _i32), ("mT", _i32),
                ("Q", _i64), ("B", _i64), ("lag", _i32),
                ("actual", _p), ("theta_pnl", _p), ("delta_ss", _p), ("gamma_ss", _p), ("vega_ss", _p), ("resid_ss", _p),
                ("delta_sm", _p), ("gamma_sm", _p), ("vega_sm", _p), ("resid_sm", _p),
                ("net", _p), ("n_dead", _p), ("flags", _p)]


class HsimArgs(C.Structure):
    """ivs_hsim_args of include/ivs.h (field for field)."""
    _fields_ = [("params", _p), ("Tq", _p), ("tq_stride", _i64), ("spot", _p), ("rate", C.c_double),
                ("u", _p), ("tau", _p), ("q_stride", _i64), ("is_put", _p), ("qty", _p), ("strike_mode", _i32), ("mT", _i32),
                ("Q", _i64), ("B", _i64), ("lag", _i32), ("window", _i32),
                ("tail_probs", C.POINTER(C.c_double)), ("nL", _i32), ("min_scen", _i32), ("scen_per_wg", _i32), ("stages", _i32),
                ("pnl", _p), ("scen_flags", _p), ("var", _p), ("es", _p), ("n_valid", _p), ("n_dead", _p), ("worst", _p),
                ("value", _p)]


class HsimAttribArgs(C.Structure):
    """ivs_hsim_attrib_args of include/ivs.h (field for field)."""
    _fields_ = [("params", _p), ("Tq", _p), ("tq_stride", _i64), ("spot", _p), ("rate", C.c_double),
                ("u", _p), ("tau", _p), ("q_stride", _i64), ("is_put", _p), ("qty", _p), ("strike_mode", _i32), ("mT", _i32),
                ("Q", _i64), ("B", _i64), ("lag", _i32), ("window", _i32),
                ("tail_probs", C.POINTER(C.c_double)), ("nL", _i32), ("min_scen", _i32),
                ("pnl", _p), ("scen_flags", _p), ("group", _p), ("nG", _i32),
                ("ces", _p), ("cvar", _p), ("ces_group", _p), ("cvar_group", _p), ("n_tail", _p), ("order", _p)]


class HedgeArgs(C.Structure):
    """ivs_hedge_args of include/ivs.h (field for field)."""
    _fields_ = [("params", _p), ("Tq", _p), ("tq_stride", _i64), ("spot", _p), ("rate", C.c_double),
                ("inst_u", _p), ("inst_tau", _p), ("inst_stride", _i64), ("inst_kind", _p), ("strike_mode", _i32),
                ("mT", _i32), ("nH", _i32), ("B", _i64), ("lag", _i32), ("window", _i32),
                ("tail_probs", C.POINTER(C.c_double)), ("nL", _i32), ("min_scen", _i32), ("rounds", _i32), ("n_forced", _i32),
                ("tol", C.c_double), ("min_gain", C.c_double), ("stages", _i32), ("scen_per_wg", _i32),
                ("pnl", _p), ("scen_flags", _p), ("inst_pnl", _p), ("inst_flags", _p), ("pick", _p), ("ss", _p), ("n_rounds", _p),
                ("hedge", _p), ("pnl_hedged", _p), ("var_h", _p), ("es_h", _p), ("worst_h", _p), ("n_scen", _p),
                ("solo_qty", _p), ("solo_left", _p), ("inst_value", _p)]


class WhatIfArgs(C.Structure):
    """ivs_whatif_args of include/ivs.h (field for field)."""
    _fields_ = [("params", _p), ("Tq", _p), ("tq_stride", _i64), ("spot", _p), ("rate", C.c_double),
                ("inst_u", _p), ("inst_tau", _p), ("inst_stride", _i64), ("inst_kind", _p), ("strike_mode", _i32),
                ("mT", _i32), ("nH", _i32), ("B", _i64), ("lag", _i32), ("window", _i32),
                ("tail_probs", C.POINTER(C.c_double)), ("nL", _i32), ("min_scen", _i32), ("nQ", _i32),
                ("size", _p), ("size_stride", _i64), ("stages", _i32), ("scen_per_wg", _i32),
                ("pnl", _p), ("scen_flags", _p), ("inst_pnl", _p), ("inst_value", _p), ("trade_flags", _p),
                ("var_w", _p), ("es_w", _p), ("worst_w", _p), ("best", _p), ("var0", _p), ("es0", _p), ("worst0", _p), ("n_scen", _p)]


class BootstrapArgs(C.Structure):
    """ivs_bootstrap_args of include/ivs.h (field for field)."""
    _fields_ = [("pnl", _p), ("scen_flags", _p), ("B", _i64), ("window", _i32), ("nL", _i32),
                ("tail_probs", C.POINTER(C.c_double)), ("min_scen", _i32), ("n_rep", _i32), ("block", _i32), ("nC", _i32),
                ("seed", C.c_uint64), ("ci_probs", C.POINTER(C.c_double)),
                ("var0", _p), ("es0", _p), ("n_scen", _p), ("mean", _p), ("variance", _p), ("quant", _p), ("rep", _p)]


class WeightedArgs(C.Structure):
    """ivs_hsim_weighted_args of include/ivs.h (field for field)."""
    _fields_ = [("pnl", _p), ("scen_flags", _p), ("B", _i64), ("window", _i32), ("lag", _i32), ("nL", _i32), ("min_scen", _i32),
                ("tail_probs", C.POINTER(C.c_double)), ("weight", _p), ("spot", _p), ("vol_weight", _p),
                ("vol_span", _i32), ("min_returns", _i32), ("scale_cap", C.c_double), ("stages", _i32),
                ("sigma", _p), ("var_w", _p), ("es_w", _p), ("n_valid_w", _p), ("worst_w", _p), ("wsum", _p), ("n_eff", _p),
                ("pnl_w", _p), ("scale", _p), ("flags_w", _p)]


class SsviArgs(C.Structure):
    """ivs_ssvi_args of include/ivs.h (field for field)."""
    _fields_ = [("vol", _p), ("Kq", _p), ("kq_stride", _i64), ("Tq", _p), ("tq_stride", _i64),
                ("spot", _p), ("rate", C.c_double), ("raw", _p), ("theta0", _p),
                ("mK", _i32), ("mT", _i32), ("B", _i64), ("rounds", _i32),
                ("surface", _p), ("theta", _p), ("params", _p), ("fit", _p), ("flags", _p), ("sflags", _p), ("fitted", _p)]


# every symbol include/ivs.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "ivs_version": (C.c_int, []),
    "ivs_last_error": (C.c_char_p, []),
    "ivs_last_kernel": (C.c_char_p, []),
    "ivs_device_count": (C.c_int, []),
    "ivs_interp1d_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "ivs_interp1d_batch_f64": (C.c_int, [_p, _p, _i64, _p, _i64, _i32, _i64, _p, _p, _i64, _p, _i64, _p, _i32,
                                         _p, _sz, _p]),
    "ivs_interp1d_greeks_batch_f64": (C.c_int, [_p, _p, _i64, _p, _i64, _i32, _i64, _p, _p, _i64, _p, _i64, _p, _i32,
                                                _i32, _i32, _i32, _p, _i64, _i32, _i32, _i32, _p, _p, _p, _p, _i64,
                                                _p, _sz, _p]),
    "ivs_ffill_index_batch": (C.c_int, [_p, _p, _p, _i64, _i32, _p, _i64, _i64, _p, _i64, _p]),
    "ivs_gather_rows_f64": (C.c_int, [_p, _i64, _p, _i64, _p, _i32, _i64, _p, _i64, _p]),
    "ivs_gather_rows_i32": (C.c_int, [_p, _i64, _p, _i64, _p, _i32, _i64, _p, _i64, _p]),
    "ivs_frame_rows": (C.c_int, [_p, _i64, _i64, _p, _p, _i64, _i32, _p, _p, _p, _p, _p, _p]),
    "ivs_frame_workspace_bytes": (_sz, [_i64, _i64, _i32]),
    "ivs_frame_columns_f64": (C.c_int, [C.POINTER(FrameArgs), _p, _sz, _p]),
    "ivs_bs_greeks_f64": (C.c_int, [_p, _p, _p, _p, _p, _p, _i32, _i64, _p, _p, _p, _p, _p, _p]),
    "ivs_bs_price_f64": (C.c_int, [_p, _p, _p, _p, _p, _p, _i32, _i64, _p, _p, _p, _p]),
    "ivs_bs_implied_vol_f64": (C.c_int, [_p, _p, _p, _p, _p, _p, _i32, _i32, _i64, _p, _p, _p]),
    "ivs_candle_aggregate_f64": (C.c_int, [_p] * 7 + [_i64, _i64, _i64] + [_p] * 8),
    "ivs_bridge_workspace_bytes": (C.c_size_t, [_i64]),
    "ivs_mt19937_words_u32": (C.c_int, [C.c_uint32, _p, _i64, _p]),
    "ivs_bridge_candles_f64": (C.c_int, [_p, _p, _p, _i64, _i64, _i32, C.c_double, C.c_double, _p, _i64, _p, _p, _p,
                                         _p, C.c_size_t, _p]),
    "ivs_debug_stamps": (C.c_int, [_p, _i64]),
    "ivs_debug_last_grid": (_i64, []),
    "ivs_debug_mode_offset": (_i64, []),
    "ivs_surface_workspace_bytes": (_sz, [_i64, _i32]),
    "ivs_snapshot_assemble_f64": (C.c_int, [C.POINTER(SnapshotArgs), _p, _sz, _p]),
    "ivs_smile_delta_points_f64": (C.c_int, [C.POINTER(SmileArgs), _p, _sz, _p]),
    "ivs_surface_arbitrage_f64": (C.c_int, [C.POINTER(ArbitrageArgs), _p, _sz, _p]),
    "ivs_surface_moments_f64": (C.c_int, [C.POINTER(MomentsArgs), _p, _sz, _p]),
    "ivs_svi_slices_f64": (C.c_int, [C.POINTER(SviArgs), _p, _sz, _p]),
    "ivs_svi_distribution_f64": (C.c_int, [C.POINTER(DistributionArgs), _p, _sz, _p]),
    "ivs_svi_calendar_f64": (C.c_int, [C.POINTER(CalendarArgs), _p, _sz, _p]),
    "ivs_svi_eval_f64": (C.c_int, [C.POINTER(EvalArgs), _p, _sz, _p]),
    "ivs_svi_greeks_f64": (C.c_int, [C.POINTER(GreeksArgs), _p, _sz, _p]),
    "ivs_svi_book_f64": (C.c_int, [C.POINTER(BookArgs), _p, _sz, _p]),
    "ivs_svi_explain_f64": (C.c_int, [C.POINTER(ExplainArgs), _p, _sz, _p]),
    "ivs_svi_hsim_f64": (C.c_int, [C.POINTER(HsimArgs), _p, _sz, _p]),
    "ivs_svi_hsim_attrib_f64": (C.c_int, [C.POINTER(HsimAttribArgs), _p, _sz, _p]),
    "ivs_svi_hedge_f64": (C.c_int, [C.POINTER(HedgeArgs), _p, _sz, _p]),
    "ivs_svi_whatif_f64": (C.c_int, [C.POINTER(WhatIfArgs), _p, _sz, _p]),
    "ivs_hsim_bootstrap_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "ivs_hsim_bootstrap_f64": (C.c_int, [C.POINTER(BootstrapArgs), _p, _sz, _p]),
    "ivs_hsim_weighted_f64": (C.c_int, [C.POINTER(WeightedArgs), _p, _sz, _p]),
    "ivs_ssvi_surface_f64": (C.c_int, [C.POINTER(SsviArgs), _p, _sz, _p]),
    "ivs_surface_batch_f64": (C.c_int, [_p, _p, _i64, _i32, _p, _i64, _i32, _p, _i64, _p, _i64, _i32, _p, _i64, _i32,
                                        _p, _p, _i32, _i32, _p, _sz, _p]),
}

_lib = None


def load():
    """Load libivs.so (no GPU needed for loading).  Raises EngineUnavailable if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineUnavailable(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    # torch-ROCm ships its own libamdhip64; libivs.so must bind to THAT copy, so torch has to be loaded first.  Loading
    # libivs.so (-> /opt/rocm's runtime) before torch leaves two HIP runtimes in the process and torch sees no device.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:
        raise EngineUnavailable(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise EngineUnavailable(
                f"{LIB_PATH} does not export {name}: it was built from an older tree; rebuild it with "
                "`python -c 'import __graft_entry__ as g; g.build()'`") from e
        fn.restype = res
        fn.argtypes = args
    if lib.ivs_version() != ABI_VERSION:
        raise EngineUnavailable(f"libivs.so ABI {lib.ivs_version()} != expected {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        raise EngineError(f"{what} failed ({rc}): {load().ivs_last_error().decode()}")
