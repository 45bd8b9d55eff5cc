"""CPU: the exact return code and the complete ivs_last_error() text of every host-side check of the snapshot-analytics
entry points (the eleven ivs_*_args calls, ivs_bs_price_f64 and ivs_bs_implied_vol_f64), and the precedence between checks
that fire together.  Device pointers are fake non-null values that are never dereferenced: every row fails a check, or is
an empty batch, before any launch.  The small lists the C side reads on the host (z, horizons, probs, levels, shocks) are
real arrays."""
import ctypes as C

import pytest

from iv_interpolation_amd import _lib

P = 64                         # a fake non-null device pointer
OK, EINVAL, ERANGE = 0, -22, -34
INF, NAN = float("inf"), float("nan")


def _arr(*xs):
    return C.cast((C.c_double * len(xs))(*xs), C.POINTER(C.c_double))


Z5 = _arr(-1.28, -0.67, 0.0, 0.67, 1.28)
H2, H_NEG, H_INF = _arr(0.08, 0.25), _arr(0.08, -1.0), _arr(INF, 0.25)
PR3, PR_ONE, PR_NAN = _arr(0.05, 0.5, 0.95), _arr(0.05, 1.0, 0.95), _arr(NAN, 0.5, 0.95)
LV2, LV_ZERO, LV_INF = _arr(0.9, 1.1), _arr(0.0, 1.1), _arr(0.9, INF)
SA2, SA_M1, SA_INF = _arr(-0.1, 0.1), _arr(-0.1, -1.0), _arr(INF, 0.1)
SV2, SV_INF, SV_NAN = _arr(-0.05, 0.05), _arr(-INF, 0.05), _arr(-0.05, NAN)

SURFACE = dict(vol=P, Kq=P, kq_stride=0, Tq=P, tq_stride=0, spot=P, rate=0.01, mK=5, mT=3, B=2)
SLICES = dict(params=P, Tq=P, tq_stride=0, spot=P, mT=3, B=2)
QUERIES = dict(SLICES, rate=0.01, u=P, tau=P, q_stride=0, strike_mode=0, Q=3)

# entry point -> (args struct, a set of arguments that passes every check)
CALLS = {
    "ivs_snapshot_assemble_f64": (_lib.SnapshotArgs, dict(
        date_ns=P, iv=P, underlying=P, n_rows=10, row_off=P, n_contracts=2, cells=P, strike=P, expiry_ns=P, nT=2, nK=3,
        t0_ns=0, n_snapshots=4, moneyness=P, mK=3, kq_empty=1.0, sigma=P, T=P, spot=P, quotes=P, Kq=P)),
    "ivs_smile_delta_points_f64": (_lib.SmileArgs, dict(
        SURFACE, z=Z5, nD=5, q_vol=P, q_strike=P, q_flags=P, rows_per_wave=0)),
    "ivs_surface_arbitrage_f64": (_lib.ArbitrageArgs, dict(
        SURFACE, flags=P, counts=P, worst=P, local_vol=P, density=P)),
    "ivs_surface_moments_f64": (_lib.MomentsArgs, dict(
        SURFACE, min_mass=0.99, horizons=H2, nH=2, raw=P, stats=P, mass=P, flags=P, index=P, index_flags=P,
        snapshots_per_wg=0)),
    "ivs_svi_slices_f64": (_lib.SviArgs, dict(
        SURFACE, rounds=0, params=P, fit=P, flags=P, fitted=P, rows_per_wg=0)),
    "ivs_svi_distribution_f64": (_lib.DistributionArgs, dict(
        SLICES, rate=0.01, max_tail=1e-6, probs=PR3, nP=3, levels=LV2, nL=2, q_x=P, q_strike=P, q_flags=P, p_below=P,
        p_above=P, tails=P, flags=P, rows_per_wave=0)),
    "ivs_svi_calendar_f64": (_lib.CalendarArgs, dict(
        SLICES, d_min=P, x_min=P, d_atm=P, x_cross=P, n_cross=P, flags=P, rows_per_wave=0)),
    "ivs_svi_eval_f64": (_lib.EvalArgs, dict(
        QUERIES, w=P, vol=P, call=P, put=P, fwd_var=P, g=P, local_vol=P, flags=P)),
    "ivs_svi_greeks_f64": (_lib.GreeksArgs, dict(
        QUERIES, is_put=P, price=P, delta_ss=P, delta_sm=P, gamma_ss=P, gamma_sm=P, vega=P, theta=P, flags=P)),
    "ivs_svi_book_f64": (_lib.BookArgs, dict(
        QUERIES, is_put=P, qty=P, spot_shocks=SA2, nA=2, vol_shocks=SV2, nV=2, net=P, n_dead=P, pnl_ss=P, pnl_sm=P,
        cell_flags=P, cells_per_wg=0)),
    "ivs_ssvi_surface_f64": (_lib.SsviArgs, dict(
        SURFACE, raw=P, theta0=None, rounds=0, surface=P, theta=P, params=P, fit=P, flags=P, sflags=P, fitted=P)),
}

ROWS_3 = 0x7fffffff // 3 + 1           # 715827883: the first B whose B x 3 rows no longer fit one launch
ROWS_4 = 0x7fffffff // 4 + 1           # 536870912
ROWS_15 = 0x7fffffff // 15 + 1         # 143165577

# (entry point, what differs from the passing set or None for null args, return code, ivs_last_error())
ARGS_TABLE = [
    # ---- ivs_snapshot_assemble_f64
    ("ivs_snapshot_assemble_f64", None, EINVAL, "ivs_snapshot_assemble_f64: null args"),
    ("ivs_snapshot_assemble_f64", dict(n_rows=-1), EINVAL, "ivs_snapshot_assemble_f64: negative size"),
    ("ivs_snapshot_assemble_f64", dict(n_contracts=-1), EINVAL, "ivs_snapshot_assemble_f64: negative size"),
    ("ivs_snapshot_assemble_f64", dict(nT=-1), EINVAL, "ivs_snapshot_assemble_f64: negative size"),
    ("ivs_snapshot_assemble_f64", dict(nK=-1), EINVAL, "ivs_snapshot_assemble_f64: negative size"),
    ("ivs_snapshot_assemble_f64", dict(n_snapshots=-1), EINVAL, "ivs_snapshot_assemble_f64: negative size"),
    ("ivs_snapshot_assemble_f64", dict(mK=-1), EINVAL, "ivs_snapshot_assemble_f64: negative size"),
    ("ivs_snapshot_assemble_f64", dict(nT=33), ERANGE, "ivs_snapshot_assemble_f64: nT=33 expiries exceed the surface engine's 32"),
    ("ivs_snapshot_assemble_f64", dict(n_snapshots=0), OK, ""),
    ("ivs_snapshot_assemble_f64", dict(nT=0), ERANGE, "ivs_snapshot_assemble_f64: nT=0 x nK=3: empty axis"),
    ("ivs_snapshot_assemble_f64", dict(nK=0), ERANGE, "ivs_snapshot_assemble_f64: nT=2 x nK=0: empty axis"),
    ("ivs_snapshot_assemble_f64", dict(cells=None), EINVAL, "ivs_snapshot_assemble_f64: null pointer"),
    ("ivs_snapshot_assemble_f64", dict(strike=None), EINVAL, "ivs_snapshot_assemble_f64: null pointer"),
    ("ivs_snapshot_assemble_f64", dict(expiry_ns=None), EINVAL, "ivs_snapshot_assemble_f64: null pointer"),
    ("ivs_snapshot_assemble_f64", dict(row_off=None), EINVAL, "ivs_snapshot_assemble_f64: null pointer"),
    ("ivs_snapshot_assemble_f64", dict(sigma=None), EINVAL, "ivs_snapshot_assemble_f64: null pointer"),
    ("ivs_snapshot_assemble_f64", dict(T=None), EINVAL, "ivs_snapshot_assemble_f64: null pointer"),
    ("ivs_snapshot_assemble_f64", dict(spot=None), EINVAL, "ivs_snapshot_assemble_f64: null pointer"),
    ("ivs_snapshot_assemble_f64", dict(quotes=None), EINVAL, "ivs_snapshot_assemble_f64: null pointer"),
    ("ivs_snapshot_assemble_f64", dict(date_ns=None), EINVAL, "ivs_snapshot_assemble_f64: null row columns"),
    ("ivs_snapshot_assemble_f64", dict(iv=None), EINVAL, "ivs_snapshot_assemble_f64: null row columns"),
    ("ivs_snapshot_assemble_f64", dict(underlying=None), EINVAL, "ivs_snapshot_assemble_f64: null row columns"),
    ("ivs_snapshot_assemble_f64", dict(moneyness=None), EINVAL, "ivs_snapshot_assemble_f64: Kq needs moneyness [mK >= 1]"),
    ("ivs_snapshot_assemble_f64", dict(mK=0), EINVAL, "ivs_snapshot_assemble_f64: Kq needs moneyness [mK >= 1]"),
    ("ivs_snapshot_assemble_f64", dict(n_contracts=1 << 31), ERANGE,
     "ivs_snapshot_assemble_f64: 2147483648 contracts / 6 cells exceed the int32 tables"),
    ("ivs_snapshot_assemble_f64", dict(nK=1 << 30), ERANGE,
     "ivs_snapshot_assemble_f64: 2 contracts / 2147483648 cells exceed the int32 tables"),
    ("ivs_snapshot_assemble_f64", dict(n_snapshots=1 << 31), ERANGE,
     "ivs_snapshot_assemble_f64: 2147483648 snapshots exceed one launch"),
    # precedence
    ("ivs_snapshot_assemble_f64", dict(n_rows=-1, nT=33), EINVAL, "ivs_snapshot_assemble_f64: negative size"),
    ("ivs_snapshot_assemble_f64", dict(nT=33, n_snapshots=0), ERANGE, "ivs_snapshot_assemble_f64: nT=33 expiries exceed the surface engine's 32"),
    ("ivs_snapshot_assemble_f64", dict(n_snapshots=0, nT=0, cells=None), OK, ""),
    ("ivs_snapshot_assemble_f64", dict(nK=0, cells=None), ERANGE, "ivs_snapshot_assemble_f64: nT=2 x nK=0: empty axis"),
    ("ivs_snapshot_assemble_f64", dict(sigma=None, iv=None), EINVAL, "ivs_snapshot_assemble_f64: null pointer"),
    ("ivs_snapshot_assemble_f64", dict(iv=None, moneyness=None), EINVAL, "ivs_snapshot_assemble_f64: null row columns"),
    ("ivs_snapshot_assemble_f64", dict(moneyness=None, n_contracts=1 << 31), EINVAL, "ivs_snapshot_assemble_f64: Kq needs moneyness [mK >= 1]"),
    ("ivs_snapshot_assemble_f64", dict(nK=1 << 30, n_snapshots=1 << 31), ERANGE,
     "ivs_snapshot_assemble_f64: 2 contracts / 2147483648 cells exceed the int32 tables"),

    # ---- ivs_smile_delta_points_f64
    ("ivs_smile_delta_points_f64", None, EINVAL, "ivs_smile_delta_points_f64: null args"),
    ("ivs_smile_delta_points_f64", dict(B=-1), EINVAL, "ivs_smile_delta_points_f64: negative size"),
    ("ivs_smile_delta_points_f64", dict(mT=-1), EINVAL, "ivs_smile_delta_points_f64: negative size"),
    ("ivs_smile_delta_points_f64", dict(mK=-1), EINVAL, "ivs_smile_delta_points_f64: negative size"),
    ("ivs_smile_delta_points_f64", dict(kq_stride=-1), EINVAL, "ivs_smile_delta_points_f64: negative size"),
    ("ivs_smile_delta_points_f64", dict(tq_stride=-1), EINVAL, "ivs_smile_delta_points_f64: negative size"),
    ("ivs_smile_delta_points_f64", dict(nD=0), ERANGE, "ivs_smile_delta_points_f64: nD=0 outside [1,16]"),
    ("ivs_smile_delta_points_f64", dict(nD=17), ERANGE, "ivs_smile_delta_points_f64: nD=17 outside [1,16]"),
    ("ivs_smile_delta_points_f64", dict(mK=1), ERANGE, "ivs_smile_delta_points_f64: mK=1 < 2: a bracket needs two nodes"),
    ("ivs_smile_delta_points_f64", dict(rows_per_wave=-1), ERANGE, "ivs_smile_delta_points_f64: rows_per_wave=-1 outside [0,12] for nD=5"),
    ("ivs_smile_delta_points_f64", dict(rows_per_wave=13), ERANGE, "ivs_smile_delta_points_f64: rows_per_wave=13 outside [0,12] for nD=5"),
    ("ivs_smile_delta_points_f64", dict(B=0), OK, ""),
    ("ivs_smile_delta_points_f64", dict(mT=0), OK, ""),
    ("ivs_smile_delta_points_f64", dict(vol=None), EINVAL, "ivs_smile_delta_points_f64: null pointer"),
    ("ivs_smile_delta_points_f64", dict(Kq=None), EINVAL, "ivs_smile_delta_points_f64: null pointer"),
    ("ivs_smile_delta_points_f64", dict(Tq=None), EINVAL, "ivs_smile_delta_points_f64: null pointer"),
    ("ivs_smile_delta_points_f64", dict(spot=None), EINVAL, "ivs_smile_delta_points_f64: null pointer"),
    ("ivs_smile_delta_points_f64", dict(z=None), EINVAL, "ivs_smile_delta_points_f64: null pointer"),
    ("ivs_smile_delta_points_f64", dict(q_vol=None), EINVAL, "ivs_smile_delta_points_f64: null pointer"),
    ("ivs_smile_delta_points_f64", dict(q_strike=None), EINVAL, "ivs_smile_delta_points_f64: null pointer"),
    ("ivs_smile_delta_points_f64", dict(q_flags=None), EINVAL, "ivs_smile_delta_points_f64: null pointer"),
    ("ivs_smile_delta_points_f64", dict(kq_stride=4), EINVAL, "ivs_smile_delta_points_f64: grid stride smaller than the grid"),
    ("ivs_smile_delta_points_f64", dict(tq_stride=2), EINVAL, "ivs_smile_delta_points_f64: grid stride smaller than the grid"),
    ("ivs_smile_delta_points_f64", dict(B=ROWS_3), ERANGE, "ivs_smile_delta_points_f64: 715827883 x 3 rows exceed one launch"),
    # precedence; a stride above the grid's length is accepted here, so it reaches the launch limit
    ("ivs_smile_delta_points_f64", dict(B=-1, nD=0), EINVAL, "ivs_smile_delta_points_f64: negative size"),
    ("ivs_smile_delta_points_f64", dict(nD=17, mK=1), ERANGE, "ivs_smile_delta_points_f64: nD=17 outside [1,16]"),
    ("ivs_smile_delta_points_f64", dict(mK=1, rows_per_wave=13), ERANGE, "ivs_smile_delta_points_f64: mK=1 < 2: a bracket needs two nodes"),
    ("ivs_smile_delta_points_f64", dict(rows_per_wave=13, B=0), ERANGE, "ivs_smile_delta_points_f64: rows_per_wave=13 outside [0,12] for nD=5"),
    ("ivs_smile_delta_points_f64", dict(mT=0, vol=None, kq_stride=4), OK, ""),
    ("ivs_smile_delta_points_f64", dict(z=None, kq_stride=4), EINVAL, "ivs_smile_delta_points_f64: null pointer"),
    ("ivs_smile_delta_points_f64", dict(tq_stride=2, B=ROWS_3), EINVAL, "ivs_smile_delta_points_f64: grid stride smaller than the grid"),
    ("ivs_smile_delta_points_f64", dict(kq_stride=6, tq_stride=4, B=ROWS_3), ERANGE, "ivs_smile_delta_points_f64: 715827883 x 3 rows exceed one launch"),

    # ---- ivs_surface_arbitrage_f64
    ("ivs_surface_arbitrage_f64", None, EINVAL, "ivs_surface_arbitrage_f64: null args"),
    ("ivs_surface_arbitrage_f64", dict(B=-1), EINVAL, "ivs_surface_arbitrage_f64: negative size"),
    ("ivs_surface_arbitrage_f64", dict(mT=-1), EINVAL, "ivs_surface_arbitrage_f64: negative size"),
    ("ivs_surface_arbitrage_f64", dict(mK=-1), EINVAL, "ivs_surface_arbitrage_f64: negative size"),
    ("ivs_surface_arbitrage_f64", dict(kq_stride=-1), EINVAL, "ivs_surface_arbitrage_f64: negative size"),
    ("ivs_surface_arbitrage_f64", dict(tq_stride=-1), EINVAL, "ivs_surface_arbitrage_f64: negative size"),
    ("ivs_surface_arbitrage_f64", dict(mK=2), ERANGE, "ivs_surface_arbitrage_f64: mK=2 < 3: the strike stencil needs three nodes"),
    ("ivs_surface_arbitrage_f64", dict(mT=1), ERANGE, "ivs_surface_arbitrage_f64: mT=1 < 2: the tenor stencil needs two rows"),
    ("ivs_surface_arbitrage_f64", dict(mT=0), ERANGE, "ivs_surface_arbitrage_f64: mT=0 < 2: the tenor stencil needs two rows"),
    ("ivs_surface_arbitrage_f64", dict(B=0), OK, ""),
    ("ivs_surface_arbitrage_f64", dict(vol=None), EINVAL, "ivs_surface_arbitrage_f64: null pointer"),
    ("ivs_surface_arbitrage_f64", dict(Kq=None), EINVAL, "ivs_surface_arbitrage_f64: null pointer"),
    ("ivs_surface_arbitrage_f64", dict(Tq=None), EINVAL, "ivs_surface_arbitrage_f64: null pointer"),
    ("ivs_surface_arbitrage_f64", dict(spot=None), EINVAL, "ivs_surface_arbitrage_f64: null pointer"),
    ("ivs_surface_arbitrage_f64", dict(flags=None), EINVAL, "ivs_surface_arbitrage_f64: null pointer"),
    ("ivs_surface_arbitrage_f64", dict(counts=None), EINVAL, "ivs_surface_arbitrage_f64: null pointer"),
    ("ivs_surface_arbitrage_f64", dict(worst=None), EINVAL, "ivs_surface_arbitrage_f64: null pointer"),
    ("ivs_surface_arbitrage_f64", dict(kq_stride=4), EINVAL, "ivs_surface_arbitrage_f64: grid stride is neither 0 nor the grid's length"),
    ("ivs_surface_arbitrage_f64", dict(kq_stride=6), EINVAL, "ivs_surface_arbitrage_f64: grid stride is neither 0 nor the grid's length"),
    ("ivs_surface_arbitrage_f64", dict(tq_stride=2), EINVAL, "ivs_surface_arbitrage_f64: grid stride is neither 0 nor the grid's length"),
    ("ivs_surface_arbitrage_f64", dict(B=ROWS_3), ERANGE, "ivs_surface_arbitrage_f64: 715827883 x 3 rows exceed one launch"),
    ("ivs_surface_arbitrage_f64", dict(kq_stride=5, tq_stride=3, B=ROWS_3), ERANGE, "ivs_surface_arbitrage_f64: 715827883 x 3 rows exceed one launch"),
    # precedence
    ("ivs_surface_arbitrage_f64", dict(mT=-1, mK=2), EINVAL, "ivs_surface_arbitrage_f64: negative size"),
    ("ivs_surface_arbitrage_f64", dict(mK=2, mT=1), ERANGE, "ivs_surface_arbitrage_f64: mK=2 < 3: the strike stencil needs three nodes"),
    ("ivs_surface_arbitrage_f64", dict(mT=1, B=0), ERANGE, "ivs_surface_arbitrage_f64: mT=1 < 2: the tenor stencil needs two rows"),
    ("ivs_surface_arbitrage_f64", dict(B=0, vol=None, kq_stride=4), OK, ""),
    ("ivs_surface_arbitrage_f64", dict(worst=None, kq_stride=4), EINVAL, "ivs_surface_arbitrage_f64: null pointer"),
    ("ivs_surface_arbitrage_f64", dict(tq_stride=4, B=ROWS_3), EINVAL, "ivs_surface_arbitrage_f64: grid stride is neither 0 nor the grid's length"),

    # ---- ivs_surface_moments_f64
    ("ivs_surface_moments_f64", None, EINVAL, "ivs_surface_moments_f64: null args"),
    ("ivs_surface_moments_f64", dict(B=-1), EINVAL, "ivs_surface_moments_f64: negative size"),
    ("ivs_surface_moments_f64", dict(mT=-1), EINVAL, "ivs_surface_moments_f64: negative size"),
    ("ivs_surface_moments_f64", dict(mK=-1), EINVAL, "ivs_surface_moments_f64: negative size"),
    ("ivs_surface_moments_f64", dict(nH=-1), EINVAL, "ivs_surface_moments_f64: negative size"),
    ("ivs_surface_moments_f64", dict(kq_stride=-1), EINVAL, "ivs_surface_moments_f64: negative size"),
    ("ivs_surface_moments_f64", dict(tq_stride=-1), EINVAL, "ivs_surface_moments_f64: negative size"),
    ("ivs_surface_moments_f64", dict(mK=1), ERANGE, "ivs_surface_moments_f64: mK=1 < 2: a segment needs two nodes"),
    ("ivs_surface_moments_f64", dict(nH=9), ERANGE, "ivs_surface_moments_f64: nH=9 outside [0,8]"),
    ("ivs_surface_moments_f64", dict(snapshots_per_wg=-1), ERANGE, "ivs_surface_moments_f64: snapshots_per_wg=-1 outside [0,4]"),
    ("ivs_surface_moments_f64", dict(snapshots_per_wg=5), ERANGE, "ivs_surface_moments_f64: snapshots_per_wg=5 outside [0,4]"),
    ("ivs_surface_moments_f64", dict(min_mass=1.5), EINVAL, "ivs_surface_moments_f64: min_mass=1.5 outside [0,1]"),
    ("ivs_surface_moments_f64", dict(min_mass=-0.25), EINVAL, "ivs_surface_moments_f64: min_mass=-0.25 outside [0,1]"),
    ("ivs_surface_moments_f64", dict(min_mass=NAN), EINVAL, "ivs_surface_moments_f64: min_mass=nan outside [0,1]"),
    ("ivs_surface_moments_f64", dict(horizons=None), EINVAL, "ivs_surface_moments_f64: null horizons"),
    ("ivs_surface_moments_f64", dict(horizons=H_NEG), EINVAL, "ivs_surface_moments_f64: horizon 1 (-1) is not a finite positive number"),
    ("ivs_surface_moments_f64", dict(horizons=H_INF), EINVAL, "ivs_surface_moments_f64: horizon 0 (inf) is not a finite positive number"),
    ("ivs_surface_moments_f64", dict(B=0), OK, ""),
    ("ivs_surface_moments_f64", dict(mT=0), OK, ""),
    ("ivs_surface_moments_f64", dict(vol=None), EINVAL, "ivs_surface_moments_f64: null pointer"),
    ("ivs_surface_moments_f64", dict(Kq=None), EINVAL, "ivs_surface_moments_f64: null pointer"),
    ("ivs_surface_moments_f64", dict(Tq=None), EINVAL, "ivs_surface_moments_f64: null pointer"),
    ("ivs_surface_moments_f64", dict(spot=None), EINVAL, "ivs_surface_moments_f64: null pointer"),
    ("ivs_surface_moments_f64", dict(raw=None), EINVAL, "ivs_surface_moments_f64: null pointer"),
    ("ivs_surface_moments_f64", dict(stats=None), EINVAL, "ivs_surface_moments_f64: null pointer"),
    ("ivs_surface_moments_f64", dict(mass=None), EINVAL, "ivs_surface_moments_f64: null pointer"),
    ("ivs_surface_moments_f64", dict(flags=None), EINVAL, "ivs_surface_moments_f64: null pointer"),
    ("ivs_surface_moments_f64", dict(index=None), EINVAL, "ivs_surface_moments_f64: null index / index_flags with nH=2"),
    ("ivs_surface_moments_f64", dict(index_flags=None), EINVAL, "ivs_surface_moments_f64: null index / index_flags with nH=2"),
    ("ivs_surface_moments_f64", dict(kq_stride=6), EINVAL, "ivs_surface_moments_f64: grid stride is neither 0 nor the grid's length"),
    ("ivs_surface_moments_f64", dict(tq_stride=2), EINVAL, "ivs_surface_moments_f64: grid stride is neither 0 nor the grid's length"),
    ("ivs_surface_moments_f64", dict(B=ROWS_3), ERANGE, "ivs_surface_moments_f64: 715827883 x 3 rows exceed one launch"),
    ("ivs_surface_moments_f64", dict(mT=513), ERANGE, "ivs_surface_moments_f64: mT=513 > 512 row slots per snapshot"),
    # precedence
    ("ivs_surface_moments_f64", dict(nH=-1, mK=1), EINVAL, "ivs_surface_moments_f64: negative size"),
    ("ivs_surface_moments_f64", dict(mK=1, nH=9), ERANGE, "ivs_surface_moments_f64: mK=1 < 2: a segment needs two nodes"),
    ("ivs_surface_moments_f64", dict(nH=9, snapshots_per_wg=5), ERANGE, "ivs_surface_moments_f64: nH=9 outside [0,8]"),
    ("ivs_surface_moments_f64", dict(snapshots_per_wg=5, min_mass=2.0), ERANGE, "ivs_surface_moments_f64: snapshots_per_wg=5 outside [0,4]"),
    ("ivs_surface_moments_f64", dict(min_mass=2.0, horizons=None), EINVAL, "ivs_surface_moments_f64: min_mass=2 outside [0,1]"),
    ("ivs_surface_moments_f64", dict(horizons=H_NEG, B=0), EINVAL, "ivs_surface_moments_f64: horizon 1 (-1) is not a finite positive number"),
    ("ivs_surface_moments_f64", dict(mT=0, vol=None, index=None), OK, ""),
    ("ivs_surface_moments_f64", dict(nH=0, horizons=None, index=None, index_flags=None, B=0), OK, ""),
    ("ivs_surface_moments_f64", dict(flags=None, index=None), EINVAL, "ivs_surface_moments_f64: null pointer"),
    ("ivs_surface_moments_f64", dict(index=None, kq_stride=6), EINVAL, "ivs_surface_moments_f64: null index / index_flags with nH=2"),
    ("ivs_surface_moments_f64", dict(kq_stride=6, B=ROWS_3), EINVAL, "ivs_surface_moments_f64: grid stride is neither 0 nor the grid's length"),
    ("ivs_surface_moments_f64", dict(mT=513, B=0x7fffffff // 513 + 1), ERANGE, "ivs_surface_moments_f64: 4186128 x 513 rows exceed one launch"),

    # ---- ivs_svi_slices_f64
    ("ivs_svi_slices_f64", None, EINVAL, "ivs_svi_slices_f64: null args"),
    ("ivs_svi_slices_f64", dict(B=-1), EINVAL, "ivs_svi_slices_f64: negative size"),
    ("ivs_svi_slices_f64", dict(mT=-1), EINVAL, "ivs_svi_slices_f64: negative size"),
    ("ivs_svi_slices_f64", dict(mK=-1), EINVAL, "ivs_svi_slices_f64: negative size"),
    ("ivs_svi_slices_f64", dict(kq_stride=-1), EINVAL, "ivs_svi_slices_f64: negative size"),
    ("ivs_svi_slices_f64", dict(tq_stride=-1), EINVAL, "ivs_svi_slices_f64: negative size"),
    ("ivs_svi_slices_f64", dict(mK=4), ERANGE, "ivs_svi_slices_f64: mK=4 < 5: five parameters need five nodes"),
    ("ivs_svi_slices_f64", dict(mK=1025), ERANGE, "ivs_svi_slices_f64: mK=1025 > 1024 nodes of the LDS slot"),
    ("ivs_svi_slices_f64", dict(rounds=-1), ERANGE, "ivs_svi_slices_f64: rounds=-1 outside [0,24]"),
    ("ivs_svi_slices_f64", dict(rounds=25), ERANGE, "ivs_svi_slices_f64: rounds=25 outside [0,24]"),
    ("ivs_svi_slices_f64", dict(rows_per_wg=-1), ERANGE, "ivs_svi_slices_f64: rows_per_wg=-1 outside [0,4]"),
    ("ivs_svi_slices_f64", dict(rows_per_wg=5), ERANGE, "ivs_svi_slices_f64: rows_per_wg=5 outside [0,4]"),
    ("ivs_svi_slices_f64", dict(B=0), OK, ""),
    ("ivs_svi_slices_f64", dict(mT=0), OK, ""),
    ("ivs_svi_slices_f64", dict(vol=None), EINVAL, "ivs_svi_slices_f64: null pointer"),
    ("ivs_svi_slices_f64", dict(Kq=None), EINVAL, "ivs_svi_slices_f64: null pointer"),
    ("ivs_svi_slices_f64", dict(Tq=None), EINVAL, "ivs_svi_slices_f64: null pointer"),
    ("ivs_svi_slices_f64", dict(spot=None), EINVAL, "ivs_svi_slices_f64: null pointer"),
    ("ivs_svi_slices_f64", dict(params=None), EINVAL, "ivs_svi_slices_f64: null pointer"),
    ("ivs_svi_slices_f64", dict(fit=None), EINVAL, "ivs_svi_slices_f64: null pointer"),
    ("ivs_svi_slices_f64", dict(flags=None), EINVAL, "ivs_svi_slices_f64: null pointer"),
    ("ivs_svi_slices_f64", dict(kq_stride=4), EINVAL, "ivs_svi_slices_f64: grid stride is neither 0 nor the grid's length"),
    ("ivs_svi_slices_f64", dict(tq_stride=4), EINVAL, "ivs_svi_slices_f64: grid stride is neither 0 nor the grid's length"),
    ("ivs_svi_slices_f64", dict(B=ROWS_3), ERANGE, "ivs_svi_slices_f64: 715827883 x 3 rows exceed one launch"),
    # precedence
    ("ivs_svi_slices_f64", dict(B=-1, mK=4), EINVAL, "ivs_svi_slices_f64: negative size"),
    ("ivs_svi_slices_f64", dict(mK=4, rounds=25), ERANGE, "ivs_svi_slices_f64: mK=4 < 5: five parameters need five nodes"),
    ("ivs_svi_slices_f64", dict(mK=1025, rounds=25), ERANGE, "ivs_svi_slices_f64: mK=1025 > 1024 nodes of the LDS slot"),
    ("ivs_svi_slices_f64", dict(rounds=25, rows_per_wg=5), ERANGE, "ivs_svi_slices_f64: rounds=25 outside [0,24]"),
    ("ivs_svi_slices_f64", dict(rows_per_wg=5, mT=0), ERANGE, "ivs_svi_slices_f64: rows_per_wg=5 outside [0,4]"),
    ("ivs_svi_slices_f64", dict(B=0, params=None, tq_stride=4), OK, ""),
    ("ivs_svi_slices_f64", dict(params=None, tq_stride=4), EINVAL, "ivs_svi_slices_f64: null pointer"),
    ("ivs_svi_slices_f64", dict(kq_stride=6, B=ROWS_3), EINVAL, "ivs_svi_slices_f64: grid stride is neither 0 nor the grid's length"),

    # ---- ivs_svi_distribution_f64
    ("ivs_svi_distribution_f64", None, EINVAL, "ivs_svi_distribution_f64: null args"),
    ("ivs_svi_distribution_f64", dict(B=-1), EINVAL, "ivs_svi_distribution_f64: negative size"),
    ("ivs_svi_distribution_f64", dict(mT=-1), EINVAL, "ivs_svi_distribution_f64: negative size"),
    ("ivs_svi_distribution_f64", dict(tq_stride=-1), EINVAL, "ivs_svi_distribution_f64: negative size"),
    ("ivs_svi_distribution_f64", dict(nP=0), ERANGE, "ivs_svi_distribution_f64: nP=0 outside [1,16]"),
    ("ivs_svi_distribution_f64", dict(nP=17), ERANGE, "ivs_svi_distribution_f64: nP=17 outside [1,16]"),
    ("ivs_svi_distribution_f64", dict(nL=-1), ERANGE, "ivs_svi_distribution_f64: nL=-1 outside [0,16]"),
    ("ivs_svi_distribution_f64", dict(nL=17), ERANGE, "ivs_svi_distribution_f64: nL=17 outside [0,16]"),
    ("ivs_svi_distribution_f64", dict(rows_per_wave=-1), ERANGE, "ivs_svi_distribution_f64: rows_per_wave=-1 outside [0,21] with nP=3"),
    ("ivs_svi_distribution_f64", dict(rows_per_wave=22), ERANGE, "ivs_svi_distribution_f64: rows_per_wave=22 outside [0,21] with nP=3"),
    ("ivs_svi_distribution_f64", dict(max_tail=2.0), EINVAL, "ivs_svi_distribution_f64: max_tail=2 outside [0,1]"),
    ("ivs_svi_distribution_f64", dict(max_tail=NAN), EINVAL, "ivs_svi_distribution_f64: max_tail=nan outside [0,1]"),
    ("ivs_svi_distribution_f64", dict(probs=None), EINVAL, "ivs_svi_distribution_f64: null probs"),
    ("ivs_svi_distribution_f64", dict(levels=None), EINVAL, "ivs_svi_distribution_f64: null levels"),
    ("ivs_svi_distribution_f64", dict(probs=PR_ONE), EINVAL, "ivs_svi_distribution_f64: probability 1 (1) is not strictly inside (0, 1)"),
    ("ivs_svi_distribution_f64", dict(probs=PR_NAN), EINVAL, "ivs_svi_distribution_f64: probability 0 (nan) is not strictly inside (0, 1)"),
    ("ivs_svi_distribution_f64", dict(levels=LV_ZERO), EINVAL, "ivs_svi_distribution_f64: level 0 (0) is not a finite positive number"),
    ("ivs_svi_distribution_f64", dict(levels=LV_INF), EINVAL, "ivs_svi_distribution_f64: level 1 (inf) is not a finite positive number"),
    ("ivs_svi_distribution_f64", dict(B=0), OK, ""),
    ("ivs_svi_distribution_f64", dict(mT=0), OK, ""),
    ("ivs_svi_distribution_f64", dict(params=None), EINVAL, "ivs_svi_distribution_f64: null pointer"),
    ("ivs_svi_distribution_f64", dict(Tq=None), EINVAL, "ivs_svi_distribution_f64: null pointer"),
    ("ivs_svi_distribution_f64", dict(spot=None), EINVAL, "ivs_svi_distribution_f64: null pointer"),
    ("ivs_svi_distribution_f64", dict(q_x=None), EINVAL, "ivs_svi_distribution_f64: null pointer"),
    ("ivs_svi_distribution_f64", dict(q_strike=None), EINVAL, "ivs_svi_distribution_f64: null pointer"),
    ("ivs_svi_distribution_f64", dict(q_flags=None), EINVAL, "ivs_svi_distribution_f64: null pointer"),
    ("ivs_svi_distribution_f64", dict(tails=None), EINVAL, "ivs_svi_distribution_f64: null pointer"),
    ("ivs_svi_distribution_f64", dict(flags=None), EINVAL, "ivs_svi_distribution_f64: null pointer"),
    ("ivs_svi_distribution_f64", dict(p_below=None), EINVAL, "ivs_svi_distribution_f64: null p_below / p_above with nL=2"),
    ("ivs_svi_distribution_f64", dict(p_above=None), EINVAL, "ivs_svi_distribution_f64: null p_below / p_above with nL=2"),
    ("ivs_svi_distribution_f64", dict(tq_stride=2), EINVAL, "ivs_svi_distribution_f64: grid stride is neither 0 nor the grid's length"),
    ("ivs_svi_distribution_f64", dict(tq_stride=4), EINVAL, "ivs_svi_distribution_f64: grid stride is neither 0 nor the grid's length"),
    ("ivs_svi_distribution_f64", dict(B=ROWS_3), ERANGE, "ivs_svi_distribution_f64: 715827883 x 3 rows exceed one launch"),
    ("ivs_svi_distribution_f64", dict(mT=65, tq_stride=65, B=0x7fffffff // 65 + 1), ERANGE, "ivs_svi_distribution_f64: 33038210 x 65 rows exceed one launch"),
    # precedence
    ("ivs_svi_distribution_f64", dict(mT=-1, nP=0), EINVAL, "ivs_svi_distribution_f64: negative size"),
    ("ivs_svi_distribution_f64", dict(nP=17, nL=17), ERANGE, "ivs_svi_distribution_f64: nP=17 outside [1,16]"),
    ("ivs_svi_distribution_f64", dict(nL=17, rows_per_wave=22), ERANGE, "ivs_svi_distribution_f64: nL=17 outside [0,16]"),
    ("ivs_svi_distribution_f64", dict(rows_per_wave=22, max_tail=2.0), ERANGE, "ivs_svi_distribution_f64: rows_per_wave=22 outside [0,21] with nP=3"),
    ("ivs_svi_distribution_f64", dict(max_tail=2.0, probs=None), EINVAL, "ivs_svi_distribution_f64: max_tail=2 outside [0,1]"),
    ("ivs_svi_distribution_f64", dict(probs=None, levels=None), EINVAL, "ivs_svi_distribution_f64: null probs"),
    ("ivs_svi_distribution_f64", dict(levels=None, probs=PR_ONE), EINVAL, "ivs_svi_distribution_f64: null levels"),
    ("ivs_svi_distribution_f64", dict(probs=PR_ONE, levels=LV_ZERO), EINVAL, "ivs_svi_distribution_f64: probability 1 (1) is not strictly inside (0, 1)"),
    ("ivs_svi_distribution_f64", dict(levels=LV_ZERO, B=0), EINVAL, "ivs_svi_distribution_f64: level 0 (0) is not a finite positive number"),
    ("ivs_svi_distribution_f64", dict(B=0, params=None, p_below=None), OK, ""),
    ("ivs_svi_distribution_f64", dict(nL=0, levels=None, p_below=None, p_above=None, mT=0), OK, ""),
    ("ivs_svi_distribution_f64", dict(flags=None, p_above=None), EINVAL, "ivs_svi_distribution_f64: null pointer"),
    ("ivs_svi_distribution_f64", dict(p_above=None, tq_stride=2), EINVAL, "ivs_svi_distribution_f64: null p_below / p_above with nL=2"),
    ("ivs_svi_distribution_f64", dict(tq_stride=2, B=ROWS_3), EINVAL, "ivs_svi_distribution_f64: grid stride is neither 0 nor the grid's length"),

    # ---- ivs_svi_calendar_f64
    ("ivs_svi_calendar_f64", None, EINVAL, "ivs_svi_calendar_f64: null args"),
    ("ivs_svi_calendar_f64", dict(B=-1), EINVAL, "ivs_svi_calendar_f64: negative size"),
    ("ivs_svi_calendar_f64", dict(mT=-1), EINVAL, "ivs_svi_calendar_f64: negative size"),
    ("ivs_svi_calendar_f64", dict(tq_stride=-1), EINVAL, "ivs_svi_calendar_f64: negative size"),
    ("ivs_svi_calendar_f64", dict(mT=65), ERANGE, "ivs_svi_calendar_f64: mT=65 > 64 tenors of one ballot"),
    ("ivs_svi_calendar_f64", dict(rows_per_wave=-1), ERANGE, "ivs_svi_calendar_f64: rows_per_wave=-1 outside [0,32]"),
    ("ivs_svi_calendar_f64", dict(rows_per_wave=33), ERANGE, "ivs_svi_calendar_f64: rows_per_wave=33 outside [0,32]"),
    ("ivs_svi_calendar_f64", dict(B=0), OK, ""),
    ("ivs_svi_calendar_f64", dict(mT=0), OK, ""),
    ("ivs_svi_calendar_f64", dict(params=None), EINVAL, "ivs_svi_calendar_f64: null pointer"),
    ("ivs_svi_calendar_f64", dict(Tq=None), EINVAL, "ivs_svi_calendar_f64: null pointer"),
    ("ivs_svi_calendar_f64", dict(spot=None), EINVAL, "ivs_svi_calendar_f64: null pointer"),
    ("ivs_svi_calendar_f64", dict(d_min=None), EINVAL, "ivs_svi_calendar_f64: null pointer"),
    ("ivs_svi_calendar_f64", dict(x_min=None), EINVAL, "ivs_svi_calendar_f64: null pointer"),
    ("ivs_svi_calendar_f64", dict(d_atm=None), EINVAL, "ivs_svi_calendar_f64: null pointer"),
    ("ivs_svi_calendar_f64", dict(x_cross=None), EINVAL, "ivs_svi_calendar_f64: null pointer"),
    ("ivs_svi_calendar_f64", dict(n_cross=None), EINVAL, "ivs_svi_calendar_f64: null pointer"),
    ("ivs_svi_calendar_f64", dict(flags=None), EINVAL, "ivs_svi_calendar_f64: null pointer"),
    ("ivs_svi_calendar_f64", dict(tq_stride=2), EINVAL, "ivs_svi_calendar_f64: grid stride is neither 0 nor the grid's length"),
    ("ivs_svi_calendar_f64", dict(tq_stride=4), EINVAL, "ivs_svi_calendar_f64: grid stride is neither 0 nor the grid's length"),
    ("ivs_svi_calendar_f64", dict(B=ROWS_3), ERANGE, "ivs_svi_calendar_f64: 715827883 x 3 rows exceed one launch"),
    # precedence
    ("ivs_svi_calendar_f64", dict(B=-1, mT=65), EINVAL, "ivs_svi_calendar_f64: negative size"),
    ("ivs_svi_calendar_f64", dict(mT=65, rows_per_wave=33), ERANGE, "ivs_svi_calendar_f64: mT=65 > 64 tenors of one ballot"),
    ("ivs_svi_calendar_f64", dict(rows_per_wave=33, B=0), ERANGE, "ivs_svi_calendar_f64: rows_per_wave=33 outside [0,32]"),
    ("ivs_svi_calendar_f64", dict(mT=0, params=None, tq_stride=2), OK, ""),
    ("ivs_svi_calendar_f64", dict(n_cross=None, tq_stride=2), EINVAL, "ivs_svi_calendar_f64: null pointer"),
    ("ivs_svi_calendar_f64", dict(tq_stride=2, B=ROWS_3), EINVAL, "ivs_svi_calendar_f64: grid stride is neither 0 nor the grid's length"),

    # ---- ivs_svi_eval_f64
    ("ivs_svi_eval_f64", None, EINVAL, "ivs_svi_eval_f64: null args"),
    ("ivs_svi_eval_f64", dict(B=-1), EINVAL, "ivs_svi_eval_f64: negative size"),
    ("ivs_svi_eval_f64", dict(mT=-1), EINVAL, "ivs_svi_eval_f64: negative size"),
    ("ivs_svi_eval_f64", dict(Q=-1), EINVAL, "ivs_svi_eval_f64: negative size"),
    ("ivs_svi_eval_f64", dict(tq_stride=-1), EINVAL, "ivs_svi_eval_f64: negative size"),
    ("ivs_svi_eval_f64", dict(q_stride=-1), EINVAL, "ivs_svi_eval_f64: negative size"),
    ("ivs_svi_eval_f64", dict(strike_mode=2), EINVAL, "ivs_svi_eval_f64: strike_mode=2 is neither 0 nor 1"),
    ("ivs_svi_eval_f64", dict(strike_mode=-1), EINVAL, "ivs_svi_eval_f64: strike_mode=-1 is neither 0 nor 1"),
    ("ivs_svi_eval_f64", dict(mT=65), ERANGE, "ivs_svi_eval_f64: mT=65 > 64 tenors of one snapshot"),
    ("ivs_svi_eval_f64", dict(B=0), OK, ""),
    ("ivs_svi_eval_f64", dict(mT=0), OK, ""),
    ("ivs_svi_eval_f64", dict(Q=0), OK, ""),
    ("ivs_svi_eval_f64", dict(params=None), EINVAL, "ivs_svi_eval_f64: null pointer"),
    ("ivs_svi_eval_f64", dict(Tq=None), EINVAL, "ivs_svi_eval_f64: null pointer"),
    ("ivs_svi_eval_f64", dict(spot=None), EINVAL, "ivs_svi_eval_f64: null pointer"),
    ("ivs_svi_eval_f64", dict(u=None), EINVAL, "ivs_svi_eval_f64: null pointer"),
    ("ivs_svi_eval_f64", dict(tau=None), EINVAL, "ivs_svi_eval_f64: null pointer"),
    ("ivs_svi_eval_f64", dict(flags=None), EINVAL, "ivs_svi_eval_f64: null pointer"),
    ("ivs_svi_eval_f64", dict(tq_stride=2), EINVAL, "ivs_svi_eval_f64: grid or query stride is neither 0 nor the full length"),
    ("ivs_svi_eval_f64", dict(q_stride=4), EINVAL, "ivs_svi_eval_f64: grid or query stride is neither 0 nor the full length"),
    ("ivs_svi_eval_f64", dict(B=ROWS_3, Q=1), ERANGE, "ivs_svi_eval_f64: 715827883 x 3 rows exceed one launch"),
    ("ivs_svi_eval_f64", dict(B=ROWS_3, mT=1), ERANGE, "ivs_svi_eval_f64: 715827883 x 3 queries exceed one launch"),
    # precedence
    ("ivs_svi_eval_f64", dict(Q=-1, strike_mode=2), EINVAL, "ivs_svi_eval_f64: negative size"),
    ("ivs_svi_eval_f64", dict(strike_mode=2, mT=65), EINVAL, "ivs_svi_eval_f64: strike_mode=2 is neither 0 nor 1"),
    ("ivs_svi_eval_f64", dict(mT=65, Q=0), ERANGE, "ivs_svi_eval_f64: mT=65 > 64 tenors of one snapshot"),
    ("ivs_svi_eval_f64", dict(Q=0, params=None, tq_stride=2), OK, ""),
    ("ivs_svi_eval_f64", dict(flags=None, q_stride=4), EINVAL, "ivs_svi_eval_f64: null pointer"),
    ("ivs_svi_eval_f64", dict(q_stride=4, B=ROWS_3), EINVAL, "ivs_svi_eval_f64: grid or query stride is neither 0 nor the full length"),
    ("ivs_svi_eval_f64", dict(B=ROWS_3), ERANGE, "ivs_svi_eval_f64: 715827883 x 3 rows exceed one launch"),

    # ---- ivs_svi_greeks_f64
    ("ivs_svi_greeks_f64", None, EINVAL, "ivs_svi_greeks_f64: null args"),
    ("ivs_svi_greeks_f64", dict(B=-1), EINVAL, "ivs_svi_greeks_f64: negative size"),
    ("ivs_svi_greeks_f64", dict(mT=-1), EINVAL, "ivs_svi_greeks_f64: negative size"),
    ("ivs_svi_greeks_f64", dict(Q=-1), EINVAL, "ivs_svi_greeks_f64: negative size"),
    ("ivs_svi_greeks_f64", dict(tq_stride=-1), EINVAL, "ivs_svi_greeks_f64: negative size"),
    ("ivs_svi_greeks_f64", dict(q_stride=-1), EINVAL, "ivs_svi_greeks_f64: negative size"),
    ("ivs_svi_greeks_f64", dict(strike_mode=2), EINVAL, "ivs_svi_greeks_f64: strike_mode=2 is neither 0 nor 1"),
    ("ivs_svi_greeks_f64", dict(mT=65), ERANGE, "ivs_svi_greeks_f64: mT=65 > 64 tenors of one snapshot"),
    ("ivs_svi_greeks_f64", dict(B=0), OK, ""),
    ("ivs_svi_greeks_f64", dict(mT=0), OK, ""),
    ("ivs_svi_greeks_f64", dict(Q=0), OK, ""),
    ("ivs_svi_greeks_f64", dict(params=None), EINVAL, "ivs_svi_greeks_f64: null pointer"),
    ("ivs_svi_greeks_f64", dict(Tq=None), EINVAL, "ivs_svi_greeks_f64: null pointer"),
    ("ivs_svi_greeks_f64", dict(spot=None), EINVAL, "ivs_svi_greeks_f64: null pointer"),
    ("ivs_svi_greeks_f64", dict(u=None), EINVAL, "ivs_svi_greeks_f64: null pointer"),
    ("ivs_svi_greeks_f64", dict(tau=None), EINVAL, "ivs_svi_greeks_f64: null pointer"),
    ("ivs_svi_greeks_f64", dict(flags=None), EINVAL, "ivs_svi_greeks_f64: null pointer"),
    ("ivs_svi_greeks_f64", dict(tq_stride=4), EINVAL, "ivs_svi_greeks_f64: grid or query stride is neither 0 nor the full length"),
    ("ivs_svi_greeks_f64", dict(q_stride=2), EINVAL, "ivs_svi_greeks_f64: grid or query stride is neither 0 nor the full length"),
    ("ivs_svi_greeks_f64", dict(B=ROWS_3, Q=1), ERANGE, "ivs_svi_greeks_f64: 715827883 x 3 rows exceed one launch"),
    ("ivs_svi_greeks_f64", dict(B=ROWS_3, mT=1), ERANGE, "ivs_svi_greeks_f64: 715827883 x 3 options exceed one launch"),
    # precedence
    ("ivs_svi_greeks_f64", dict(B=-1, strike_mode=2), EINVAL, "ivs_svi_greeks_f64: negative size"),
    ("ivs_svi_greeks_f64", dict(strike_mode=2, mT=65), EINVAL, "ivs_svi_greeks_f64: strike_mode=2 is neither 0 nor 1"),
    ("ivs_svi_greeks_f64", dict(mT=65, B=0), ERANGE, "ivs_svi_greeks_f64: mT=65 > 64 tenors of one snapshot"),
    ("ivs_svi_greeks_f64", dict(mT=0, u=None, q_stride=2), OK, ""),
    ("ivs_svi_greeks_f64", dict(tau=None, tq_stride=4), EINVAL, "ivs_svi_greeks_f64: null pointer"),
    ("ivs_svi_greeks_f64", dict(tq_stride=4, B=ROWS_3), EINVAL, "ivs_svi_greeks_f64: grid or query stride is neither 0 nor the full length"),
    ("ivs_svi_greeks_f64", dict(B=ROWS_3), ERANGE, "ivs_svi_greeks_f64: 715827883 x 3 rows exceed one launch"),

    # ---- ivs_svi_book_f64
    ("ivs_svi_book_f64", None, EINVAL, "ivs_svi_book_f64: null args"),
    ("ivs_svi_book_f64", dict(B=-1), EINVAL, "ivs_svi_book_f64: negative size"),
    ("ivs_svi_book_f64", dict(mT=-1), EINVAL, "ivs_svi_book_f64: negative size"),
    ("ivs_svi_book_f64", dict(Q=-1), EINVAL, "ivs_svi_book_f64: negative size"),
    ("ivs_svi_book_f64", dict(nA=-1), EINVAL, "ivs_svi_book_f64: negative size"),
    ("ivs_svi_book_f64", dict(nV=-1), EINVAL, "ivs_svi_book_f64: negative size"),
    ("ivs_svi_book_f64", dict(tq_stride=-1), EINVAL, "ivs_svi_book_f64: negative size"),
    ("ivs_svi_book_f64", dict(q_stride=-1), EINVAL, "ivs_svi_book_f64: negative size"),
    ("ivs_svi_book_f64", dict(strike_mode=2), EINVAL, "ivs_svi_book_f64: strike_mode=2 is neither 0 nor 1"),
    ("ivs_svi_book_f64", dict(mT=65), ERANGE, "ivs_svi_book_f64: mT=65 > 64 tenors of one snapshot"),
    ("ivs_svi_book_f64", dict(nA=65), ERANGE, "ivs_svi_book_f64: nA=65 or nV=2 > 64 shocks per axis"),
    ("ivs_svi_book_f64", dict(nV=65), ERANGE, "ivs_svi_book_f64: nA=2 or nV=65 > 64 shocks per axis"),
    ("ivs_svi_book_f64", dict(nA=64, nV=17), ERANGE, "ivs_svi_book_f64: nA*nV=1088 > 1024 cells"),
    ("ivs_svi_book_f64", dict(cells_per_wg=-1), ERANGE, "ivs_svi_book_f64: cells_per_wg=-1 outside [0,256]"),
    ("ivs_svi_book_f64", dict(cells_per_wg=257), ERANGE, "ivs_svi_book_f64: cells_per_wg=257 outside [0,256]"),
    ("ivs_svi_book_f64", dict(spot_shocks=None), EINVAL, "ivs_svi_book_f64: null shocks"),
    ("ivs_svi_book_f64", dict(vol_shocks=None), EINVAL, "ivs_svi_book_f64: null shocks"),
    ("ivs_svi_book_f64", dict(spot_shocks=SA_M1), ERANGE, "ivs_svi_book_f64: spot shock 1 (-1) is not a finite number above -1"),
    ("ivs_svi_book_f64", dict(spot_shocks=SA_INF), ERANGE, "ivs_svi_book_f64: spot shock 0 (inf) is not a finite number above -1"),
    ("ivs_svi_book_f64", dict(vol_shocks=SV_INF), ERANGE, "ivs_svi_book_f64: vol shock 0 (-inf) is not finite"),
    ("ivs_svi_book_f64", dict(vol_shocks=SV_NAN), ERANGE, "ivs_svi_book_f64: vol shock 1 (nan) is not finite"),
    ("ivs_svi_book_f64", dict(B=0), OK, ""),
    ("ivs_svi_book_f64", dict(mT=0), OK, ""),
    ("ivs_svi_book_f64", dict(Q=0), OK, ""),
    ("ivs_svi_book_f64", dict(params=None), EINVAL, "ivs_svi_book_f64: null pointer"),
    ("ivs_svi_book_f64", dict(Tq=None), EINVAL, "ivs_svi_book_f64: null pointer"),
    ("ivs_svi_book_f64", dict(spot=None), EINVAL, "ivs_svi_book_f64: null pointer"),
    ("ivs_svi_book_f64", dict(u=None), EINVAL, "ivs_svi_book_f64: null pointer"),
    ("ivs_svi_book_f64", dict(tau=None), EINVAL, "ivs_svi_book_f64: null pointer"),
    ("ivs_svi_book_f64", dict(qty=None), EINVAL, "ivs_svi_book_f64: null pointer"),
    ("ivs_svi_book_f64", dict(net=None), EINVAL, "ivs_svi_book_f64: null pointer"),
    ("ivs_svi_book_f64", dict(n_dead=None), EINVAL, "ivs_svi_book_f64: null pointer"),
    ("ivs_svi_book_f64", dict(cell_flags=None), EINVAL, "ivs_svi_book_f64: null pointer (cell_flags)"),
    ("ivs_svi_book_f64", dict(tq_stride=2), EINVAL, "ivs_svi_book_f64: grid or query stride is neither 0 nor the full length"),
    ("ivs_svi_book_f64", dict(q_stride=4), EINVAL, "ivs_svi_book_f64: grid or query stride is neither 0 nor the full length"),
    ("ivs_svi_book_f64", dict(B=ROWS_3, Q=1), ERANGE, "ivs_svi_book_f64: 715827883 x 3 rows exceed one launch"),
    ("ivs_svi_book_f64", dict(B=ROWS_3, mT=1), ERANGE, "ivs_svi_book_f64: 715827883 x 3 options exceed one launch"),
    ("ivs_svi_book_f64", dict(B=ROWS_4, mT=1, Q=1), ERANGE, "ivs_svi_book_f64: 536870912 x 4 cells exceed one launch"),
    # precedence
    ("ivs_svi_book_f64", dict(nA=-1, strike_mode=2), EINVAL, "ivs_svi_book_f64: negative size"),
    ("ivs_svi_book_f64", dict(strike_mode=2, mT=65), EINVAL, "ivs_svi_book_f64: strike_mode=2 is neither 0 nor 1"),
    ("ivs_svi_book_f64", dict(mT=65, nA=65), ERANGE, "ivs_svi_book_f64: mT=65 > 64 tenors of one snapshot"),
    ("ivs_svi_book_f64", dict(nA=65, nV=17), ERANGE, "ivs_svi_book_f64: nA=65 or nV=17 > 64 shocks per axis"),
    ("ivs_svi_book_f64", dict(nA=64, nV=17, cells_per_wg=257), ERANGE, "ivs_svi_book_f64: nA*nV=1088 > 1024 cells"),
    ("ivs_svi_book_f64", dict(cells_per_wg=257, spot_shocks=None), ERANGE, "ivs_svi_book_f64: cells_per_wg=257 outside [0,256]"),
    ("ivs_svi_book_f64", dict(vol_shocks=None, spot_shocks=SA_M1), EINVAL, "ivs_svi_book_f64: null shocks"),
    ("ivs_svi_book_f64", dict(spot_shocks=SA_M1, vol_shocks=SV_NAN), ERANGE, "ivs_svi_book_f64: spot shock 1 (-1) is not a finite number above -1"),
    ("ivs_svi_book_f64", dict(vol_shocks=SV_NAN, Q=0), ERANGE, "ivs_svi_book_f64: vol shock 1 (nan) is not finite"),
    ("ivs_svi_book_f64", dict(nA=0, spot_shocks=None, vol_shocks=SV_NAN, B=0), OK, ""),
    ("ivs_svi_book_f64", dict(B=0, params=None, cell_flags=None), OK, ""),
    ("ivs_svi_book_f64", dict(n_dead=None, cell_flags=None), EINVAL, "ivs_svi_book_f64: null pointer"),
    ("ivs_svi_book_f64", dict(cell_flags=None, tq_stride=2), EINVAL, "ivs_svi_book_f64: null pointer (cell_flags)"),
    ("ivs_svi_book_f64", dict(tq_stride=2, B=ROWS_3), EINVAL, "ivs_svi_book_f64: grid or query stride is neither 0 nor the full length"),
    ("ivs_svi_book_f64", dict(B=ROWS_3), ERANGE, "ivs_svi_book_f64: 715827883 x 3 rows exceed one launch"),
    ("ivs_svi_book_f64", dict(B=ROWS_3, mT=1, Q=4), ERANGE, "ivs_svi_book_f64: 715827883 x 4 options exceed one launch"),

    # ---- ivs_ssvi_surface_f64
    ("ivs_ssvi_surface_f64", None, EINVAL, "ivs_ssvi_surface_f64: null args"),
    ("ivs_ssvi_surface_f64", dict(B=-1), EINVAL, "ivs_ssvi_surface_f64: negative size"),
    ("ivs_ssvi_surface_f64", dict(mT=-1), EINVAL, "ivs_ssvi_surface_f64: negative size"),
    ("ivs_ssvi_surface_f64", dict(mK=-1), EINVAL, "ivs_ssvi_surface_f64: negative size"),
    ("ivs_ssvi_surface_f64", dict(kq_stride=-1), EINVAL, "ivs_ssvi_surface_f64: negative size"),
    ("ivs_ssvi_surface_f64", dict(tq_stride=-1), EINVAL, "ivs_ssvi_surface_f64: negative size"),
    ("ivs_ssvi_surface_f64", dict(theta0=P), EINVAL, "ivs_ssvi_surface_f64: exactly one of raw and theta0 must be given"),
    ("ivs_ssvi_surface_f64", dict(raw=None), EINVAL, "ivs_ssvi_surface_f64: exactly one of raw and theta0 must be given"),
    ("ivs_ssvi_surface_f64", dict(mT=65), ERANGE, "ivs_ssvi_surface_f64: mT=65 > 64 tenors of one ballot"),
    ("ivs_ssvi_surface_f64", dict(mK=0), ERANGE, "ivs_ssvi_surface_f64: mK=0 < 1"),
    ("ivs_ssvi_surface_f64", dict(mT=7, mK=439), ERANGE, "ivs_ssvi_surface_f64: mT*mK=3073 > 3072 nodes of the LDS"),
    ("ivs_ssvi_surface_f64", dict(rounds=-1), ERANGE, "ivs_ssvi_surface_f64: rounds=-1 outside [0,32]"),
    ("ivs_ssvi_surface_f64", dict(rounds=33), ERANGE, "ivs_ssvi_surface_f64: rounds=33 outside [0,32]"),
    ("ivs_ssvi_surface_f64", dict(B=0), OK, ""),
    ("ivs_ssvi_surface_f64", dict(mT=0), OK, ""),
    ("ivs_ssvi_surface_f64", dict(raw=None, theta0=P, B=0), OK, ""),
    ("ivs_ssvi_surface_f64", dict(vol=None), EINVAL, "ivs_ssvi_surface_f64: null pointer"),
    ("ivs_ssvi_surface_f64", dict(Kq=None), EINVAL, "ivs_ssvi_surface_f64: null pointer"),
    ("ivs_ssvi_surface_f64", dict(Tq=None), EINVAL, "ivs_ssvi_surface_f64: null pointer"),
    ("ivs_ssvi_surface_f64", dict(spot=None), EINVAL, "ivs_ssvi_surface_f64: null pointer"),
    ("ivs_ssvi_surface_f64", dict(surface=None), EINVAL, "ivs_ssvi_surface_f64: null pointer"),
    ("ivs_ssvi_surface_f64", dict(theta=None), EINVAL, "ivs_ssvi_surface_f64: null pointer"),
    ("ivs_ssvi_surface_f64", dict(params=None), EINVAL, "ivs_ssvi_surface_f64: null pointer"),
    ("ivs_ssvi_surface_f64", dict(fit=None), EINVAL, "ivs_ssvi_surface_f64: null pointer"),
    ("ivs_ssvi_surface_f64", dict(flags=None), EINVAL, "ivs_ssvi_surface_f64: null pointer"),
    ("ivs_ssvi_surface_f64", dict(sflags=None), EINVAL, "ivs_ssvi_surface_f64: null pointer"),
    ("ivs_ssvi_surface_f64", dict(kq_stride=6), EINVAL, "ivs_ssvi_surface_f64: grid stride is neither 0 nor the grid's length"),
    ("ivs_ssvi_surface_f64", dict(tq_stride=2), EINVAL, "ivs_ssvi_surface_f64: grid stride is neither 0 nor the grid's length"),
    ("ivs_ssvi_surface_f64", dict(B=ROWS_15), ERANGE, "ivs_ssvi_surface_f64: 143165577 x 3 x 5 nodes exceed one launch"),
    # precedence
    ("ivs_ssvi_surface_f64", dict(mK=-1, theta0=P), EINVAL, "ivs_ssvi_surface_f64: negative size"),
    ("ivs_ssvi_surface_f64", dict(raw=None, mT=65), EINVAL, "ivs_ssvi_surface_f64: exactly one of raw and theta0 must be given"),
    ("ivs_ssvi_surface_f64", dict(theta0=P, B=0), EINVAL, "ivs_ssvi_surface_f64: exactly one of raw and theta0 must be given"),
    ("ivs_ssvi_surface_f64", dict(mT=65, mK=0), ERANGE, "ivs_ssvi_surface_f64: mT=65 > 64 tenors of one ballot"),
    ("ivs_ssvi_surface_f64", dict(mK=0, rounds=33), ERANGE, "ivs_ssvi_surface_f64: mK=0 < 1"),
    ("ivs_ssvi_surface_f64", dict(mT=7, mK=439, rounds=33), ERANGE, "ivs_ssvi_surface_f64: mT*mK=3073 > 3072 nodes of the LDS"),
    ("ivs_ssvi_surface_f64", dict(rounds=33, B=0), ERANGE, "ivs_ssvi_surface_f64: rounds=33 outside [0,32]"),
    ("ivs_ssvi_surface_f64", dict(mT=0, vol=None, kq_stride=6), OK, ""),
    ("ivs_ssvi_surface_f64", dict(sflags=None, kq_stride=6), EINVAL, "ivs_ssvi_surface_f64: null pointer"),
    ("ivs_ssvi_surface_f64", dict(tq_stride=2, B=ROWS_15), EINVAL, "ivs_ssvi_surface_f64: grid stride is neither 0 nor the grid's length"),
]


def _row_id(row):
    fn, diff = row[0], row[1]
    return fn + "-" + ("null" if diff is None else ",".join(f"{k}={'arr' if isinstance(v, C._Pointer) else v}" for k, v in diff.items()))


@pytest.mark.parametrize("fn,diff,rc,message", ARGS_TABLE, ids=[_row_id(r) for r in ARGS_TABLE])
def test_args_entry_point(fn, diff, rc, message):
    lib = _lib.load()
    if diff is None:
        a = None
    else:
        cls, base = CALLS[fn]
        a = cls()
        for k, v in dict(base, **diff).items():
            setattr(a, k, v)
    assert getattr(lib, fn)(a, None, 0, None) == rc
    assert lib.ivs_last_error() == message.encode()
    assert lib.ivs_last_kernel() == b""                    # nothing was launched


def test_table_covers_every_args_entry_point():
    assert {r[0] for r in ARGS_TABLE} == set(CALLS) and len(CALLS) == 11


# ivs_bs_price_f64(S, K, T, r, sigma, is_put, default_is_put, n, price, vega, flags, stream)
PRICE_TABLE = [
    (dict(n=-1), EINVAL, "ivs_bs_price_f64: negative size n=-1"),
    (dict(n=1 << 31), ERANGE, "ivs_bs_price_f64: n=2147483648 options exceed one launch"),
    (dict(n=0), OK, ""),
    (dict(S=None), EINVAL, "ivs_bs_price_f64: null pointer"),
    (dict(K=None), EINVAL, "ivs_bs_price_f64: null pointer"),
    (dict(T=None), EINVAL, "ivs_bs_price_f64: null pointer"),
    (dict(r=None), EINVAL, "ivs_bs_price_f64: null pointer"),
    (dict(sigma=None), EINVAL, "ivs_bs_price_f64: null pointer"),
    (dict(price=None), EINVAL, "ivs_bs_price_f64: null pointer"),
    # precedence
    (dict(n=-1, S=None), EINVAL, "ivs_bs_price_f64: negative size n=-1"),
    (dict(n=1 << 31, price=None), ERANGE, "ivs_bs_price_f64: n=2147483648 options exceed one launch"),
    (dict(n=0, S=None, price=None), OK, ""),
]


@pytest.mark.parametrize("diff,rc,message", PRICE_TABLE, ids=[str(r[0]) for r in PRICE_TABLE])
def test_bs_price(diff, rc, message):
    lib = _lib.load()
    a = dict(dict(S=P, K=P, T=P, r=P, sigma=P, is_put=P, n=8, price=P, vega=P, flags=P), **diff)
    got = lib.ivs_bs_price_f64(a["S"], a["K"], a["T"], a["r"], a["sigma"], a["is_put"], 0, a["n"], a["price"], a["vega"],
                               a["flags"], None)
    assert got == rc
    assert lib.ivs_last_error() == message.encode()
    assert lib.ivs_last_kernel() == b""


# ivs_bs_implied_vol_f64(price, S, K, T, r, is_put, default_is_put, price_mode, n, vol, flags, stream)
IMPLIED_TABLE = [
    (dict(n=-1), EINVAL, "ivs_bs_implied_vol_f64: negative size n=-1"),
    (dict(price_mode=2), EINVAL, "ivs_bs_implied_vol_f64: price_mode=2 is neither 0 nor 1"),
    (dict(price_mode=-1), EINVAL, "ivs_bs_implied_vol_f64: price_mode=-1 is neither 0 nor 1"),
    (dict(n=1 << 31), ERANGE, "ivs_bs_implied_vol_f64: n=2147483648 options exceed one launch"),
    (dict(n=0), OK, ""),
    (dict(price=None), EINVAL, "ivs_bs_implied_vol_f64: null pointer"),
    (dict(S=None), EINVAL, "ivs_bs_implied_vol_f64: null pointer"),
    (dict(K=None), EINVAL, "ivs_bs_implied_vol_f64: null pointer"),
    (dict(T=None), EINVAL, "ivs_bs_implied_vol_f64: null pointer"),
    (dict(r=None), EINVAL, "ivs_bs_implied_vol_f64: null pointer"),
    (dict(vol=None), EINVAL, "ivs_bs_implied_vol_f64: null pointer"),
    (dict(flags=None), EINVAL, "ivs_bs_implied_vol_f64: null pointer"),
    # precedence
    (dict(n=-1, price_mode=2), EINVAL, "ivs_bs_implied_vol_f64: negative size n=-1"),
    (dict(price_mode=2, n=1 << 31), EINVAL, "ivs_bs_implied_vol_f64: price_mode=2 is neither 0 nor 1"),
    (dict(price_mode=2, n=0), EINVAL, "ivs_bs_implied_vol_f64: price_mode=2 is neither 0 nor 1"),
    (dict(n=1 << 31, vol=None), ERANGE, "ivs_bs_implied_vol_f64: n=2147483648 options exceed one launch"),
    (dict(n=0, price=None, flags=None), OK, ""),
]


@pytest.mark.parametrize("diff,rc,message", IMPLIED_TABLE, ids=[str(r[0]) for r in IMPLIED_TABLE])
def test_bs_implied_vol(diff, rc, message):
    lib = _lib.load()
    a = dict(dict(price=P, S=P, K=P, T=P, r=P, is_put=P, price_mode=0, n=8, vol=P, flags=P), **diff)
    got = lib.ivs_bs_implied_vol_f64(a["price"], a["S"], a["K"], a["T"], a["r"], a["is_put"], 0, a["price_mode"], a["n"],
                                     a["vol"], a["flags"], None)
    assert got == rc
    assert lib.ivs_last_error() == message.encode()
    assert lib.ivs_last_kernel() == b""
