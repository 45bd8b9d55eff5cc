"""Hand-built micro cases, one per rule and flag of T1-T4, C1-C6 and E1-E6, the seeded generators of the
GPU shapes and the tolerances.  TEST INFRASTRUCTURE ONLY.  A calendar case is a dict(params [B,mT,5], Tq, spot); an evaluation
case carries besides rate, u, tau, strike_mode.  A micro case also carries what must come out, worked out by hand from the
rules: `flags` and, where the case is about them, `n_cross` and `cells`.  The constants R_CPU below have their measured source
in profiles/svi_surface/errlog.txt."""
import numpy as np
import pandas as pd

import dist_cases as DC

NAN, INF = float("nan"), float("inf")
CALENDAR, WING_LEFT, WING_RIGHT, DEAD, LAST, UNORDERED = 1, 2, 4, 8, 16, 32
SHORT, LONG, NEG_FWD, Q_DEAD, NEG_G, Q_UNORDERED = 1, 2, 4, 8, 16, 32
EPS = DC.EPS
GOOD, TAU = DC.GOOD, DC.TAU

# R_CPU: the largest |fp64 restatement - the same rules in mpmath at 50 digits| over every input the GPU tests use (MICRO_CAL,
# MICRO_EVAL, SHAPES with their queries and every 8th snapshot of the chain with the restatement's own SVI fit), in units of eps
# x the rule's scale (tolerances_* below).  Measured by test_svi_surface.test_rounding_level (errlog.txt) and recorded here
# rounded up: "d" covers d_min, d_atm and x_min (0.361, on d_atm), x_cross 0.228, "w" covers w, vol and fwd_var (0.298, on w),
# "price" call and put (0.126), "lv" g and local_vol (0.438, on g).  The scales count every rounding of a term generously, so the
# figures stay below 1.
# The GPU tests allow C_GPU x R_CPU, the project's standing margin for FMA contraction and the device's erfc / exp / log / sqrt
# / division.
R_CPU = {"d": 0.37, "x_cross": 0.23, "w": 0.30, "price": 0.13, "lv": 0.44}
C_GPU = 8.0
BISECTION_WIDTH = 4.0 * 2.0 ** -52       # of the cell: where 52 halvings stop, either side of the sign change
TINY = float(np.finfo(np.float64).tiny)  # below the normal range a price has no relative precision left
CAL_UNIT = {"d_min": "d", "x_min": "d", "d_atm": "d", "x_cross": "x_cross"}
EVAL_UNIT = {"w": "w", "vol": "w", "fwd_var": "w", "call": "price", "put": "price", "g": "lv", "local_vol": "lv"}


def tolerances_calendar(ref, factor):
    """Absolute tolerances of the calendar values of `ref` (a restatement) at `factor` units: factor x eps x the scale of
    DESIGN.md section 14.  d_min, d_atm: the terms the two w are summed from at the point, plus |w'| times the placement of
    the grid point; x_min: |x| times the relative error of s0; x_cross: d's scale at the crossing over |d'| plus the point's
    own placement, plus 4 x 2^-52 of the cell."""
    with np.errstate(all="ignore"):
        return {"d_min": factor["d"] * EPS * ref["scale_min"], "d_atm": factor["d"] * EPS * ref["scale_atm"],
                "x_min": factor["d"] * EPS * ref["scale_x"],
                "x_cross": factor["x_cross"] * EPS * (ref["cross_scale"] / np.abs(ref["cross_slope"]) + ref["cross_xrel"])
                + BISECTION_WIDTH * ref["width"]}


def tolerances_eval(ref, factor):
    """Absolute tolerances of the evaluation's values: factor x eps x scale_<key> of the restatement, plus the smallest normal
    number for the prices."""
    with np.errstate(all="ignore"):
        return {k: factor[EVAL_UNIT[k]] * EPS * ref["scale_" + k] + (TINY if EVAL_UNIT[k] == "price" else 0.0) for k in EVAL_UNIT}


def units(got, ref, tol_fn, unit):
    """|got - ref| of every compared value in the units of its tolerance: the factor at which it would just pass (the additive
    terms taken off first).  NaN where both are NaN."""
    one, zero = tol_fn(ref, {k: 1.0 for k in R_CPU}), tol_fn(ref, {k: 0.0 for k in R_CPU})
    out = {}
    with np.errstate(all="ignore"):
        for k in unit:
            if got.get(k) is None:
                continue
            d = np.abs(np.asarray(got[k], np.float64) - ref[k])
            out[k] = np.where(d <= zero[k], 0.0, (d - zero[k]) / (one[k] - zero[k]))
    return out


# ------------------------------------------------------------------ calendar micro cases
LATER = (0.008, 0.1, -0.4, 0.03, 0.12)                     # above GOOD everywhere, steeper wings
BELOW = (0.006, 0.03, -0.4, 0.03, 0.12)                    # flatter wings and a lower vertex: d < 0 at every point
BEYOND = (0.008, 0.0499, -0.4, 0.03, 0.12)                 # above GOOD on the grid, wings a hair flatter: crosses beyond it
EARLY2 = (0.002, 0.08, -0.4, 0.03, 0.12)                   # with TWICE as the later slice: d < 0 in both wings, > 0 between
TWICE = (0.008, 0.05, -0.4, 0.03, 0.12)
ONCE = (0.0045, 0.05, -0.3, 0.06, 0.12)                    # the left wing slope falls from 0.07 to 0.065, the right one rises
DEADROW = (NAN,) * 5
ALL = CALENDAR | WING_LEFT | WING_RIGHT


def _cal(params, Tq, flags, spot=100.0, **more):
    params = np.asarray(params, np.float64)
    if params.ndim == 2:
        params = params[None]
    B, mT, _ = params.shape
    return dict(params=params, Tq=np.asarray(Tq, np.float64), spot=np.broadcast_to(np.asarray(spot, np.float64), (B,)).copy(),
                flags=np.asarray(flags, np.int32).reshape(B, mT), **more)


_T2 = [TAU, 2 * TAU]
# T1 with every cause of dist_cases.DEAD_CAUSES as row 0 of its own snapshot and LATER at twice the tenor as row 1: a bad spot
# kills both rows, anything else row 0 alone (row 1 is then the last live row); the three live causes pair with row 1
_DC_FLAGS = [[DEAD, DEAD] if not (np.isfinite(s) and s > 0) else ([DEAD, LAST] if n not in DC._LIVE else [-1, LAST]) for n, _, s, _ in DC.DEAD_CAUSES]
MICRO_CAL = {
    "clean": _cal([GOOD, LATER], _T2, [0, LAST], n_cross=[[0, 0]], index=36, d_min=9.50e-3),
    "below_everywhere": _cal([GOOD, BELOW], _T2, [ALL, LAST], n_cross=[[0, 0]]),
    "beyond_the_grid": _cal([GOOD, BEYOND], _T2, [WING_LEFT | WING_RIGHT, LAST], n_cross=[[0, 0]], d_min=3.86e-3),
    "two_crossings": _cal([EARLY2, TWICE], _T2, [ALL, LAST], n_cross=[[2, 0]], cells=(26, 48)),
    "one_crossing": _cal([GOOD, ONCE], _T2, [CALENDAR | WING_LEFT, LAST], n_cross=[[1, 0]], cells=(9, 9)),
    "identical": _cal([GOOD, GOOD], _T2, [0, LAST], n_cross=[[0, 0]], index=0, d_min=0.0),
    # T4: the pair skips a dead row, whose tenor (out of order, even) plays no part
    "dead_between": _cal([GOOD, DEADROW, LATER], [TAU, 0.1 * TAU, 2 * TAU], [0, DEAD, LAST], n_cross=[[0, 0, 0]], index=36, d_min=9.50e-3),
    "single_live": _cal([[GOOD, DEADROW, DEADROW], [DEADROW, GOOD, DEADROW], [DEADROW, DEADROW, DEADROW]], [TAU, 2 * TAU, 3 * TAU],
                        [[LAST, DEAD, DEAD], [DEAD, LAST, DEAD], [DEAD, DEAD, DEAD]]),
    "one_row": _cal([[GOOD]], [TAU], [LAST]),
    # T2: equal tenors, descending tenors, and a snapshot of the same batch in order
    "unordered": _cal([[GOOD, LATER, LATER], [GOOD, DEADROW, LATER], [GOOD, LATER, DEADROW]],
                      [[TAU, 2 * TAU, 2 * TAU], [2 * TAU, 3 * TAU, TAU], [TAU, 2 * TAU, 0.5 * TAU]],
                      [[UNORDERED] * 3, [UNORDERED] * 3, [0, LAST, DEAD]]),
    "dead_causes": _cal([[p, LATER] for _, p, _, _ in DC.DEAD_CAUSES], [[t, 2 * TAU] for _, _, _, t in DC.DEAD_CAUSES], _DC_FLAGS,
                        spot=[s for _, _, s, _ in DC.DEAD_CAUSES], state_only=True),
}

# ------------------------------------------------------------------ evaluation micro cases
FLAT_T = (0.25, 0.5, 1.0)
KINK = DC.KINK


def _ev(params, Tq, u, tau, flags, rate=0.0, strike_mode=0, spot=100.0):
    params = np.asarray(params, np.float64)
    if params.ndim == 2:
        params = params[None]
    B = params.shape[0]
    return dict(params=params, Tq=np.asarray(Tq, np.float64), spot=np.broadcast_to(np.asarray(spot, np.float64), (B,)).copy(), rate=rate,
                u=np.asarray(u, np.float64), tau=np.asarray(tau, np.float64), strike_mode=strike_mode,
                flags=np.broadcast_to(np.asarray(flags, np.int32), (B, np.shape(u)[-1])).copy())


MICRO_EVAL = {
    # b = 0 and a = 0.04 tau: 20 % vol at every strike and expiry; before the first slice, on a slice, between slices, on the
    # last slice (no row above it: LONG) and beyond it
    "flat": _ev([(0.04 * t, 0.0, 0.0, 0.0, 0.1) for t in FLAT_T], FLAT_T, [0.9, 1.0, 1.1, 0.8, 1.25, 1.0], [0.1, 0.25, 0.3, 0.7, 1.0, 2.0],
                [SHORT, 0, 0, 0, LONG, LONG], rate=0.03),
    # E3 / E5: between GOOD and a slice that lies below it everywhere the forward variance is negative
    "inside_a_calendar_pair": _ev([GOOD, BELOW], _T2, [0.8, 1.0, 1.3], [0.3, 0.3, 0.45], [NEG_FWD] * 3),
    # E5: next to the kink of dist_cases.KINK (and of twice that slice above it) Durrleman's g is negative; at the kink it is not
    "kink": _ev([KINK, tuple(2 * v if q < 2 else v for q, v in enumerate(KINK))], _T2, [np.exp(0.01), np.exp(-0.01), 1.0], [0.3, 0.4, 0.3],
                [NEG_G, NEG_G, 0]),
    # E1: every dead query, then a snapshot without a live slice, as strikes
    "dead_queries": _ev([[GOOD, LATER], [DEADROW, DEADROW]], _T2, [100.0, NAN, 0.0, -90.0, INF, 100.0, 100.0, 100.0, 100.0],
                        [0.3, 0.3, 0.3, 0.3, 0.3, NAN, 0.0, -0.3, INF], [[0] + [Q_DEAD] * 8, [Q_DEAD] * 9], strike_mode=1),
    "unordered": _ev([[GOOD, LATER], [GOOD, LATER]], [[TAU, 2 * TAU], [2 * TAU, TAU]], [1.0, NAN], [0.3, 0.3], [[0, Q_DEAD], [Q_UNORDERED] * 2]),
    "single_slice": _ev([[GOOD]], [TAU], [0.9, 1.0, 1.1], [0.1, TAU, 0.4], [SHORT, LONG, LONG], rate=0.03),
}


# ------------------------------------------------------------------ generated batches
def queries(c, Q, seed, per_q, strike_mode):
    """Q queries for the batch `c`: expiries from half the first tenor to 1.15 x the last (SHORT and LONG occur), strikes
    within +- 2 standard deviations at 50 % vol; every 7th query from the 3rd sits exactly on a tenor of the grid, every 13th
    from the 5th is dead by one cause of E1 in turn."""
    r = np.random.default_rng(seed)
    B = len(c["spot"])
    Tq = np.asarray(c["Tq"])
    shape = (B, Q) if per_q else (Q,)
    tq = r.uniform(0.5 * Tq.min(), 1.15 * Tq.max(), shape)
    flat_t = Tq.reshape(-1)
    for n, q in enumerate(range(2, Q, 7)):
        tq[..., q] = Tq[..., (3 * n) % Tq.shape[-1]] if (per_q and Tq.ndim == 2) else flat_t[(3 * n) % len(flat_t)]
    u = np.exp(r.uniform(-1.0, 1.0, shape) * np.sqrt(tq))
    if strike_mode == 1:
        u = u * (c["spot"][:, None] if per_q else c["spot"][0])
    causes = [("u", NAN), ("u", 0.0), ("u", -1.0), ("u", INF), ("t", NAN), ("t", 0.0), ("t", -0.1), ("t", INF)]
    for n, q in enumerate(range(4, Q, 13)):
        which, v = causes[n % len(causes)]
        (u if which == "u" else tq)[..., q] = v
    return dict(c, u=np.ascontiguousarray(u), tau=np.ascontiguousarray(tq), strike_mode=strike_mode)


def batch(B, mT, Q, seed, per):
    """dist_cases.batch (its planted dead rows included) with queries: shared tenors, one shared list of moneyness queries and
    rate 0, or per-snapshot tenors (jittered by 10 %: out of order at mT = 64), per-snapshot strike queries and rate 0.03."""
    c = DC.batch(B, mT, 1, 0, seed, per_tq=per, rate=0.03 if per else 0.0)
    c = {k: c[k] for k in ("params", "Tq", "spot", "rate")}
    return queries(c, Q, seed + 3, per, 1 if per else 0)


# (B, mT) of the issue, each with shared and per-snapshot inputs; Q runs through {1, 63, 64, 65, 257} so that every value meets
# a ragged last block or none, one block and two
SHAPES = []
for n_, (B_, mT_) in enumerate(((1, 1), (1, 2), (4, 3), (2, 13), (3, 16), (2, 64))):
    for q_, per_ in enumerate((False, True)):
        SHAPES.append(dict(B=B_, mT=mT_, Q=(63, 64, 65, 257, 1)[(2 * n_ + q_) % 5], seed=1400 + 2 * n_ + q_, per=per_))
STREAM_SHAPE = dict(B=64, mT=16, Q=257, seed=1490, per=True)


def shape_id(s):
    return f"B{s['B']}-mT{s['mT']}-Q{s['Q']}-{'p' if s['per'] else 's'}"


def chain_book(res):
    """A book of 12 options round the first underlying's spot, expiring 4 to 25 days after the first snapshot, and one that
    has expired."""
    spot = res[0].spot
    t0, s = res[0].dates[0], float((spot.cpu().numpy() if hasattr(spot, "cpu") else np.asarray(spot))[0])
    days = [4, 9, 9, 12, 12, 15, 15, 18, 21, 25, 10, -1]
    return pd.DataFrame({"strike": s * np.array([1.0, 0.9, 1.1, 0.8, 1.2, 0.95, 1.05, 1.0, 0.9, 1.1, 1.0, 1.0]),
                         "expiry": [t0 + pd.Timedelta(days=d) for d in days]})
