"""Hand-built micro cases of rules H0-H9, the seeded generators of the GPU shapes and the tolerances.
TEST INFRASTRUCTURE ONLY.  A case is a dict(params [B,mT,5], Tq, spot [B], rate, u, tau ([Q] or [B,Q]), strike_mode, is_put [Q] or
None, qty [Q], lag, window, tail_probs, min_scen); a micro case also carries what must come out, worked out by hand from the
rules: `scen_flags` [B,window], `n_valid` and `n_dead` [B].  The constants R_CPU below have their measured source in
profiles/hsim/errlog.txt."""
import numpy as np

import cal_cases as CC
import explain_cases as XC

NAN, INF = float("nan"), float("inf")
EPS, TINY = CC.EPS, CC.TINY
ABSENT, VOID, NEG = 1, 2, 4
VALUE_KEYS = ("pnl", "var", "es", "value")
GOOD, LATER, DEADROW, TAU = CC.GOOD, CC.LATER, CC.DEADROW, CC.TAU
MINUTE = XC.MINUTE

# R_CPU: the largest |fp64 restatement - the same rules in mpmath at 50 digits| over the inputs the GPU tests use on which mpmath
# stays affordable (MICRO and MP_SHAPES), in units of eps x the value's scale (hsim_ref's scale_<key>: for a scenario P&L the
# summed units of its two prices per option, P' propagated through S', x' and all three vols of H2, plus eps x L x the sum of
# their magnitudes, L the depth of rule B5; for a VaR the largest scenario unit of its row, an order statistic being 1-Lipschitz
# in the row's sup norm; for an ES that plus two roundings of the mean; for value as section 17's net).  Measured by
# test_hsim.test_rounding_level (errlog.txt) and recorded here a third higher, rounded up.  The GPU tests allow C_GPU x R_CPU,
# the project's standing margin for the device's erfc / exp / log / sqrt / division.
# Measured: pnl 0.0507, var 0.0386, es 0.0386 (each the larger of the books' figure and that of the books of one option alone, which
# no sum averages out), value 0.0228.  The scales count every rounding of a term generously, so the figures stay well below 1.
R_CPU = {"pnl": 0.068, "var": 0.052, "es": 0.052, "value": 0.031}
C_GPU = 8.0
# the pure-spot history against section 17's sticky-moneyness cell: S (1 + a) with a = S_b / S_a - 1 against S (S_b / S_a).  Measured
# by test_hsim.test_pure_spot_history_is_the_sticky_moneyness_cell in units of eps x sum |qty| S (errlog.txt): 0, on every scenario.
# For a quotient between 1/2 and 2 the subtraction q - 1 is exact (Sterbenz) and 1 + (q - 1) gives q back, so the two spots carry
# the same bits; the margin of one unit is for quotients outside that range, which these paths do not have.
SPOT_ONLY_UNITS = 1.0


def tolerances(ref, factor):
    with np.errstate(all="ignore"):
        return {k: factor[k] * EPS * ref["scale_" + k] + TINY for k in VALUE_KEYS}


def units(got, ref, keys=VALUE_KEYS):
    """|got - ref| of every compared value in the units of its tolerance (the additive term taken off first)."""
    one, zero = tolerances(ref, {k: 1.0 for k in VALUE_KEYS}), tolerances(ref, {k: 0.0 for k in VALUE_KEYS})
    out = {}
    with np.errstate(all="ignore"):
        for k in keys:
            if got.get(k) is None:
                continue
            d = np.abs(np.asarray(got[k], np.float64) - ref[k])
            out[k] = np.where(d <= zero[k], 0.0, (d - zero[k]) / (one[k] - zero[k]))
    return out


# ------------------------------------------------------------------ micro cases
def _case(params, Tq, spot, u, tau, qty, scen_flags, n_valid, n_dead, is_put=None, lag=1, window=None, tail_probs=(0.5,), min_scen=1,
          rate=0.03, strike_mode=0):
    params = np.asarray(params, np.float64)
    B = params.shape[0]
    fl = np.asarray(scen_flags, np.int32)
    return dict(params=params, Tq=np.asarray(Tq, np.float64), spot=np.broadcast_to(np.asarray(spot, np.float64), (B,)).copy(), rate=rate,
                u=np.asarray(u, np.float64), tau=np.asarray(tau, np.float64), strike_mode=strike_mode,
                is_put=None if is_put is None else np.asarray(is_put, np.uint8), qty=np.asarray(qty, np.float64), lag=lag,
                window=fl.shape[1] if window is None else window, tail_probs=tuple(tail_probs), min_scen=min_scen, scen_flags=fl,
                n_valid=np.asarray(n_valid, np.int32), n_dead=np.asarray(n_dead, np.int32))


def moved(k, rows=(GOOD, LATER)):
    """The two slices moved a little, differently for every k: a by 0.4 % x k, b by 0.2 % x k, m by 0.0003 x k."""
    return [(r[0] * (1 + 0.004 * k), r[1] * (1 + 0.002 * k), r[2], r[3] + 0.0003 * k, r[4]) for r in rows]


def scaled(f, rows=(GOOD, LATER)):
    """a and b of every slice times f: W times f, to the bit when f is a power of two."""
    return [(r[0] * f, r[1] * f, r[2], r[3], r[4]) for r in rows]


_T2 = [TAU, 2 * TAU]
_UN = [TAU, TAU]                          # equal tenors: UNORDERED
_U5 = [0.8, 0.95, 1.0, 1.1, 1.3]
_T5 = [0.5 * TAU, 1.2 * TAU, 1.5 * TAU, 1.8 * TAU, 2.5 * TAU]
_PUT5, _QTY5 = [1, 0, 1, 0, 0], [1.0, -2.0, 0.5, -0.25, 3.0]
_S4 = [100.0, 100.3, 99.8, 100.1]
_V4 = [[1, 1, 1], [2, 1, 1], [2, 2, 1], [0, 2, 2]]           # snapshot 1 is bad: it voids itself and the pairs (0,1), (1,2)
_P4 = [moved(0), moved(1), moved(2), moved(3)]


def _neg_w_slice():
    """A live slice (T1: a + b sigma sqrt(1 - rho^2) > 0 as computed) whose computed w at x = 0 is negative: a is the negative of
    the next number below the vertex term, so the true minimum of w is one ulp above 0 and the rounding of T3's own sum decides
    the sign; m is scanned in steps of 1e-9 round the value that puts the vertex at x = 0 until it comes out negative.  x = 0 is
    reached without a rounding (K == S', rate 0), and T3 is additions, products and a square root: the same bits everywhere."""
    b, rho, sig = 0.25, -0.8863, 0.3
    vertex = b * sig * np.sqrt(1.0 - rho * rho)
    a = -np.nextafter(vertex, 0.0)
    assert a + b * sig * np.sqrt(1.0 - rho * rho) > 0.0
    for i in range(4000):
        m = rho * sig / np.sqrt(1.0 - rho * rho) + i * 1e-9
        dx = 0.0 - m
        if a + b * (rho * dx + np.sqrt(dx * dx + sig * sig)) < 0.0:
            return (float(a), b, rho, float(m), sig)
    raise AssertionError("no negative w next to the vertex")


_NEGROW = _neg_w_slice()

MICRO = {
    # H6: snapshots 0 and 1 carry the same bits: scenario (0,1) is +0.0 for p = 1 (s = 0) and for p = 2 (s = 1)
    "same_pair": _case([moved(0), moved(0), moved(3)], _T2, [100.0, 100.0, 100.4], _U5, _T5, _QTY5, [[1, 1], [0, 1], [0, 0]], [0, 1, 2], [0, 0, 0],
                       is_put=_PUT5),
    # H1: every void cause at the start of a pair, at its end and at p itself (snapshot 1 is the bad one)
    "bad_spot_nan": _case(_P4, _T2, [100.0, NAN, 99.8, 100.1], _U5, _T5, _QTY5, _V4, [0, 0, 0, 1], [0, 5, 0, 0], is_put=_PUT5),
    "bad_spot_zero": _case(_P4, _T2, [100.0, 0.0, 99.8, 100.1], _U5, _T5, _QTY5, _V4, [0, 0, 0, 1], [0, 5, 0, 0]),
    "bad_spot_inf": _case(_P4, _T2, [100.0, INF, 99.8, 100.1], _U5, _T5, _QTY5, _V4, [0, 0, 0, 1], [0, 5, 0, 0]),
    "no_live_slice": _case([moved(0), [DEADROW, DEADROW], moved(2), moved(3)], _T2, _S4, _U5, _T5, _QTY5, _V4, [0, 0, 0, 1], [0, 5, 0, 0], is_put=_PUT5),
    "unordered": _case(_P4, [_T2, _UN, _T2, _T2], _S4, _U5, _T5, _QTY5, _V4, [0, 0, 0, 1], [0, 5, 0, 0]),
    # H5: sigma' < 0: the start of the pair has 16 x the variance of its end and of today
    "neg_vol": _case([scaled(16.0), moved(0), moved(1)], _T2, [100.0, 100.2, 100.1], _U5, _T5, _QTY5, [[1, 1], [4, 1], [0, 4]], [0, 0, 1], [0, 0, 0]),
    # H5: sigma' == 0 exactly: the start has 4 x the variance (twice the vol, to the bit) of its end, which is today: s + (s - 2 s)
    "zero_vol": _case([scaled(4.0), scaled(1.0)], _T2, [100.0, 100.0], _U5, _T5, _QTY5, [[1], [4]], [0, 0], [0, 0], is_put=_PUT5),
    # H5: a historic W < 0 (a live slice whose computed w is negative next to its vertex): sqrt gives NaN, !(sigma' > 0) catches it
    "neg_hist_w": _case([[_NEGROW], [GOOD], [GOOD]], [TAU], [100.0, 100.0, 100.0], [100.0], [TAU], [1.0], [[1, 1], [4, 1], [0, 4]],
                        [0, 0, 1], [0, 0, 0], rate=0.0, strike_mode=1),
    # E2 across the pair: LONG and SHORT at the historic ends while today brackets the option, and the reverse
    "hist_long_short": _case(_P4[:3], [[0.5 * TAU, TAU], [0.5 * TAU, TAU], [0.3 * TAU, 3 * TAU]], _S4[:3], [0.9, 1.0, 1.1], [1.5 * TAU, 0.4 * TAU, 2 * TAU],
                             [1.0, -1.0, 2.0], [[1, 1], [0, 1], [0, 0]], [0, 1, 2], [0, 0, 0], is_put=[0, 1, 0]),
    "today_long_short": _case(_P4[:3], [[0.3 * TAU, 3 * TAU], [0.3 * TAU, 3 * TAU], [0.5 * TAU, TAU]], _S4[:3], [0.9, 1.0, 1.1], [1.5 * TAU, 0.4 * TAU, 2 * TAU],
                              [1.0, -1.0, 2.0], [[1, 1], [0, 1], [0, 0]], [0, 1, 2], [0, 0, 0], is_put=[0, 1, 0]),
    # G0 / E1: dead options (bad strike, bad expiry), a zero quantity (live), quantities that are not finite (dead)
    "dead_options": _case(_P4[:3], _T2, _S4[:3], [1.0, NAN, 0.0, -1.0, INF, 1.0, 1.0, 1.0, 1.0, 1.0, 1.05], [0.3, 0.3, 0.3, 0.3, 0.3, NAN, 0.0, -0.1, INF, 0.3, 0.3],
                          [1.0] * 11, [[1, 1], [0, 1], [0, 0]], [0, 1, 2], [8, 8, 8]),
    "quantities": _case(_P4[:3], _T2, _S4[:3], _U5, _T5, [0.0, NAN, 1.0, INF, -0.0], [[1, 1], [0, 1], [0, 0]], [0, 1, 2], [2, 2, 2], is_put=_PUT5),
    "one_option": _case(_P4, _T2, _S4, [1.05], [1.5 * TAU], [-3.0], [[1, 1, 1], [0, 1, 1], [0, 0, 1], [0, 0, 0]], [0, 1, 2, 3], [0] * 4, is_put=[1]),
    # window = 1, and a window longer than B
    "window_one": _case(_P4, _T2, _S4, _U5, _T5, _QTY5, [[1], [0], [0], [0]], [0, 1, 1, 1], [0] * 4, is_put=_PUT5),
    "window_long": _case(_P4, _T2, _S4, _U5, _T5, _QTY5, [[1] * 9, [0] + [1] * 8, [0, 0] + [1] * 7, [0, 0, 0] + [1] * 6], [0, 1, 2, 3], [0] * 4),
    # B <= lag: every scenario ABSENT
    "b_le_lag": _case(_P4[:2], _T2, _S4[:2], _U5, _T5, _QTY5, [[1, 1, 1]] * 2, [0, 0], [0, 0], lag=2),
    "lag_two": _case(_P4, _T2, _S4, _U5, _T5, _QTY5, [[1, 1], [1, 1], [0, 1], [0, 0]], [0, 0, 1, 2], [0] * 4, lag=2, is_put=_PUT5),
    # n < min_scen: NaN in var and es, worst still given
    "too_few": _case(_P4, _T2, _S4, _U5, _T5, _QTY5, [[1, 1, 1], [0, 1, 1], [0, 0, 1], [0, 0, 0]], [0, 1, 2, 3], [0] * 4, min_scen=3, tail_probs=(0.5, 0.9)),
}

# H7 on rows given directly (hsim_ref.tail on the CPU, the tail kernel alone on the GPU): each is (pnl row, flags row, tail_probs,
# min_scen, var, es, n_valid, worst), worked out by hand
_R10 = [5.0, -3.0, 2.0, -7.0, 0.5, 9.0, -1.0, 4.0, -2.0, 1.0]               # ascending: -7 -3 -2 -1 0.5 1 2 4 5 9
ROWS = {
    # m = floor(n tp): 10 x 0.3 = 3.0000000000000004 -> 3; 10 x 0.29999999999999993 -> 2; 10 x 0.7 = 7.000000000000001 -> 7;
    # 10 x 0.6999999999999999 -> 6; 10 x 0.05 -> max(1, 0) = 1
    "m_round": (_R10, [0] * 10, (0.3, 0.29999999999999993, 0.7, 0.6999999999999999, 0.05), 1, [2.0, 3.0, -2.0, -1.0, 7.0],
                [4.0, 5.0, 9.5 / 7.0, 11.5 / 6.0, 7.0], 10, 3),
    # ties rank by the lower s, and -0.0 ties with +0.0: ranks are s = 1 (-0.0), 2 (+0.0), 4 (-0.0), then 0 and 3
    "ties": ([1.0, -0.0, 0.0, 1.0, -0.0], [0] * 5, (0.2, 0.5, 0.99), 1, [0.0, 0.0, -1.0], [0.0, 0.0, -0.25], 5, 1),
    # flagged scenarios and NaN are not ranked
    "flagged": ([NAN, -1.0, NAN, 3.0, NAN, -5.0], [2, 0, 4, 0, 1, 0], (0.5,), 3, [5.0], [5.0], 3, 5),
    "too_few": ([NAN, -1.0, NAN, 3.0], [2, 0, 4, 0], (0.5,), 3, [NAN], [NAN], 2, 1),
    "none": ([NAN, NAN], [2, 1], (0.5, 0.1), 1, [NAN, NAN], [NAN, NAN], 0, -1),
}


# ------------------------------------------------------------------ generated batches
LEVELS8 = (0.5, 0.25, 0.2, 0.1, 0.05, 0.025, 0.01, 0.001)


def _walk(r, B):
    w = np.cumsum(r.normal(size=B))
    return w / max(1.0, np.abs(w).max())


def path(B, mT, Q, lag, window, nL, seed, per=False, min_scen=3):
    """One chain observed every minute on a smooth but wandering path, in the manner of explain_cases.path: snapshot b is
    snapshot 0 with the spot moved by up to 1 %, a of every slice by up to 2 %, b by up to 1 % and m by up to 0.002, each along a
    seeded random walk of its own.  per: strikes are absolute and the expiries come a minute closer per snapshot (u, tau [B,Q],
    Tq [B,mT]); otherwise one shared list of moneyness and expiries."""
    c = XC.batch(1, mT, Q, 1, seed, False)
    r = np.random.default_rng(seed + 17)
    P = np.repeat(c["params"], B, axis=0)
    P[:, :, 0] *= 1.0 + 0.02 * _walk(r, B)[:, None]
    P[:, :, 1] *= 1.0 + 0.01 * _walk(r, B)[:, None]
    P[:, :, 3] += 0.002 * _walk(r, B)[:, None]
    spot = c["spot"][0] * (1.0 + 0.01 * _walk(r, B))
    out = dict(c, params=P, spot=spot, lag=lag, window=window, tail_probs=LEVELS8[:nL], min_scen=min_scen)
    if per:
        n = np.arange(B, dtype=np.float64)[:, None]
        out.update(u=np.tile(c["u"] * c["spot"][0], (B, 1)), tau=np.ascontiguousarray(1.003 * c["tau"][None, :] - MINUTE * n), strike_mode=1,
                   Tq=np.tile(np.asarray(c["Tq"]), (B, 1)), rate=0.03)
    return out


def unordered(B, mT, Q, lag, window, nL, seed, per=True, min_scen=3):
    """explain_cases.batch with per-snapshot tenors at mT = 64: every snapshot UNORDERED, every existing scenario VOID_PAIR."""
    c = XC.batch(B, mT, Q, lag, seed, True)
    return dict(c, window=window, tail_probs=LEVELS8[:nL], min_scen=min_scen)


# B in {1, 2, 3, 9, 70}, lag in {1, 2}, window in {1, 2, 4, 63, 64, 65, 257}, mT in {1, 2, 16, 64}, Q in {1, 2, 63, 64, 65, 255, 256, 257,
# 1025}, nL in {0, 1, 2, 8}: every value at least once.  A workgroup takes its run of scenarios 256 at a time; the last shape
# (B = 260, window 257) is the smallest with an existing scenario in a second sub-run, and the bit tests force runs of 257, 256
# and 100 on it.  mpmath stays affordable on MP_SHAPES.
SHAPES = [dict(B=1, mT=1, Q=1, lag=1, window=1, nL=0, seed=1900),
          dict(B=2, mT=2, Q=1025, lag=1, window=2, nL=1, seed=1901, per=True),
          dict(B=3, mT=16, Q=257, lag=2, window=4, nL=2, seed=1902),
          dict(B=9, mT=16, Q=65, lag=1, window=63, nL=8, seed=1903, per=True),
          dict(B=70, mT=16, Q=63, lag=1, window=65, nL=2, seed=1904),
          dict(B=3, mT=64, Q=64, lag=2, window=64, nL=1, seed=1905),
          dict(B=9, mT=2, Q=256, lag=2, window=257, nL=2, seed=1906),
          dict(B=70, mT=1, Q=2, lag=2, window=64, nL=2, seed=1907, per=True),
          dict(B=9, mT=64, Q=255, lag=1, window=4, nL=1, seed=1908),
          dict(B=260, mT=2, Q=2, lag=1, window=257, nL=1, seed=1909)]
UNORDERED_SHAPES = (5,)
MP_SHAPES = (0, 1, 2, 3, 6)
STREAM_SHAPE = dict(B=70, mT=16, Q=257, lag=1, window=64, nL=2, seed=1991, per=True)


def make(n):
    s = STREAM_SHAPE if n == "stream" else SHAPES[n]
    return unordered(**s) if n in UNORDERED_SHAPES else path(**s)


def shape_id(s):
    return f"B{s['B']}-mT{s['mT']}-Q{s['Q']}-lag{s['lag']}-w{s['window']}-L{s['nL']}-{'p' if s.get('per') else 's'}"
