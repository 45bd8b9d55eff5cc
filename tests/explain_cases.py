"""Hand-built micro cases of rules X0-X9, the seeded generators of the GPU shapes and the tolerances.
TEST INFRASTRUCTURE ONLY.  A case is a dict(params [B,mT,5], Tq, spot [B], rate, u, tau ([Q] or [B,Q]), strike_mode, is_put [Q] or
None, qty [Q], lag); a micro case also carries what must come out, worked out by hand from the rules: `flags` [P,Q] and `n_dead`
[P].  The constants R_CPU below have their measured source in profiles/explain/errlog.txt."""
import numpy as np

import cal_cases as CC
import dist_cases as DC

NAN, INF = float("nan"), float("inf")
EPS, TINY = CC.EPS, CC.TINY
SHORT, LONG, NEG_FWD, DEAD, UNORDERED = 1, 2, 4, 8, 32
KEYS = ("actual", "theta_pnl", "delta_ss", "gamma_ss", "vega_ss", "resid_ss", "delta_sm", "gamma_sm", "vega_sm", "resid_sm")
VALUE_KEYS = KEYS + ("net",)
GOOD, LATER, DEADROW, TAU = CC.GOOD, CC.LATER, CC.DEADROW, CC.TAU
MINUTE = 1.0 / 525600.0

# R_CPU: the largest |fp64 restatement - the same rules in mpmath at 50 digits| over every input the GPU tests use (MICRO, SHAPES,
# STREAM_SHAPE and the chain's book with the restatement's own SVI fit), in units of eps x the value's scale (explain_ref's
# scale_<key>: first-order propagation through the rule's own terms; for a remainder the summed units of its five operands plus
# eps x their magnitudes; for a net figure the summed units of its terms plus eps x (L + 1) x the sum of their magnitudes, L the
# depth of rule B5).  Measured by test_explain.test_rounding_level (errlog.txt) and recorded here a third higher, rounded up.
# The GPU tests allow C_GPU x R_CPU, the project's standing margin for the device's erfc / exp / log / sqrt / division.
# Measured: actual 0.0648, theta_pnl 0.206, delta_ss 0.307, gamma_ss 0.238, vega_ss 0.216, resid_ss 0.0641, delta_sm 0.297,
# gamma_sm 0.230, vega_sm 0.221, resid_sm 0.0643, net 0.0975 (the chain's book).  The scales count every rounding of a term
# generously, so the figures stay below 1; a cancelling difference (actual, the remainders) carries the units of both prices.
R_CPU = {"actual": 0.087, "theta_pnl": 0.28, "delta_ss": 0.41, "gamma_ss": 0.32, "vega_ss": 0.29, "resid_ss": 0.086,
         "delta_sm": 0.40, "gamma_sm": 0.31, "vega_sm": 0.30, "resid_sm": 0.086, "net": 0.13}
C_GPU = 8.0


def tolerances(ref, factor):
    """Absolute tolerances of the values of `ref` (a restatement) at `factor` units: factor x eps x the value's scale, plus the
    smallest normal number (an underflowed value has no relative precision left)."""
    with np.errstate(all="ignore"):
        return {k: factor[k] * EPS * ref["scale_" + k] + TINY for k in VALUE_KEYS}


def units(got, ref, keys=VALUE_KEYS):
    """|got - ref| of every compared value in the units of its tolerance (the additive term taken off first).  NaN where both
    are NaN."""
    one, zero = tolerances(ref, {k: 1.0 for k in R_CPU}), tolerances(ref, {k: 0.0 for k in R_CPU})
    out = {}
    with np.errstate(all="ignore"):
        for k in keys:
            if got.get(k) is None:
                continue
            d = np.abs(np.asarray(got[k], np.float64) - ref[k])
            out[k] = np.where(d <= zero[k], 0.0, (d - zero[k]) / (one[k] - zero[k]))
    return out


def F(a=0, b=0, c=0):
    """X5: the bits of the placements (a), (b), (c)."""
    return a | (b << 8) | (c << 16)


# ------------------------------------------------------------------ micro cases
def _case(params, Tq, spot, u, tau, qty, flags, n_dead, is_put=None, lag=1, rate=0.03, strike_mode=0):
    params = np.asarray(params, np.float64)
    B = params.shape[0]
    qty = np.asarray(qty, np.float64)
    P = max(B - lag, 0)
    return dict(params=params, Tq=np.asarray(Tq, np.float64), spot=np.broadcast_to(np.asarray(spot, np.float64), (B,)).copy(), rate=rate,
                u=np.asarray(u, np.float64), tau=np.asarray(tau, np.float64), strike_mode=strike_mode,
                is_put=None if is_put is None else np.asarray(is_put, np.uint8), qty=qty, lag=lag,
                flags=np.broadcast_to(np.asarray(flags, np.int32), (P, len(qty))).copy(), n_dead=np.asarray(n_dead, np.int32).reshape(P))


_T2 = [TAU, 2 * TAU]
_PAIR = [[GOOD, LATER]] * 2
_MOVED = [[GOOD, LATER], [tuple(v * (1.01 if q < 2 else 1.0) for q, v in enumerate(GOOD)), tuple(v * (1.02 if q < 2 else 1.0) for q, v in enumerate(LATER))]]
_U5 = [0.8, 0.95, 1.0, 1.1, 1.3]
_T5 = [0.5 * TAU, 1.2 * TAU, 1.5 * TAU, 1.8 * TAU, 2.5 * TAU]
_F5 = [F(SHORT, SHORT, SHORT), 0, 0, 0, F(LONG, LONG, LONG)]
_PUT5, _QTY5 = [1, 0, 1, 0, 0], [1.0, -2.0, 0.5, -0.25, 3.0]
_BAD = [NAN, 0.0, -1.0, INF]
_ALL = F(DEAD, DEAD, DEAD)
_UN = [TAU, TAU]                          # equal tenors: UNORDERED
MICRO = {
    # X8: two ends with the same bits, the expiries one shared list (dt = 0): +0.0 everywhere
    "same_ends": _case(_PAIR, _T2, 100.0, _U5, _T5, _QTY5, _F5, [0], is_put=_PUT5),
    # X8, first corollary: the same surface and spot one minute later
    "time_step": _case(_PAIR, _T2, 100.0, [_U5, _U5], [_T5, [t - MINUTE for t in _T5]], _QTY5, _F5, [0], is_put=_PUT5),
    # X8, second corollary: the same surface and expiries, the spot 0.4 % higher
    "spot_step": _case(_PAIR, _T2, [100.0, 100.4], _U5, _T5, _QTY5, _F5, [0], is_put=_PUT5),
    # everything moves at once: spot, both slices and a minute of time
    "full_step": _case(_MOVED, _T2, [100.0, 99.7], [_U5, _U5], [_T5, [t - MINUTE for t in _T5]], _QTY5, _F5, [0], is_put=_PUT5),
    # X2: every dead cause of an option: a bad strike kills all three placements, a bad expiry at end 0 kills (a), at end 1 (b)
    # and (c); u of end 1 is not read
    "dead_options": _case(_PAIR, _T2, [100.0, 100.5], [[100.0] + _BAD + [100.0] * 8, [NAN] * 13],
                          [[0.3] * 5 + _BAD + [0.3] * 4, [0.3] * 9 + _BAD], [1.0] * 13, [0] + [_ALL] * 4 + [F(DEAD)] * 4 + [F(0, DEAD, DEAD)] * 4, [12],
                          strike_mode=1),
    # X2: a bad spot or no live slice at one end makes the pair degenerate: pairs (0,1) bad S1, (1,2) bad S0, (2,3) end 1 without
    # a slice, (3,4) end 0 without one
    "dead_ends": _case([[GOOD, LATER], [GOOD, LATER], [GOOD, LATER], [DEADROW, DEADROW], [GOOD, LATER]], _T2, [100.0, NAN, 100.0, 100.0, 100.0],
                       [100.0, 95.0], [0.3, 0.4], [1.0, 2.0], [[F(0, DEAD, 0)] * 2, [F(DEAD, 0, DEAD)] * 2, [F(0, DEAD, 0)] * 2, [F(DEAD, 0, DEAD)] * 2],
                       [2, 2, 2, 2], strike_mode=1),
    # T2: UNORDERED at end 1, at both ends, at end 0
    "unordered": _case([[GOOD, LATER]] * 4, [_T2, _UN, _UN, _T2], 100.0, [1.0, 1.1], [0.3, 0.4], [1.0, 1.0],
                       [[F(0, UNORDERED, 0)] * 2, [F(UNORDERED, UNORDERED, UNORDERED)] * 2, [F(UNORDERED, 0, UNORDERED)] * 2], [2, 2, 2]),
    # E2 across the pair: LONG at (a) and bracketed at (c), the reverse, bracketed at (a) and SHORT at (c), the reverse, and an
    # option that expires inside the pair
    "brackets": _case(_PAIR, _T2, [100.0, 100.2], [[1.0] * 5, [1.0] * 5],
                      [[2.05 * TAU, 1.95 * TAU, 1.02 * TAU, 0.98 * TAU, 0.5 * MINUTE], [1.95 * TAU, 2.05 * TAU, 0.98 * TAU, 1.02 * TAU, -0.5 * MINUTE]],
                      [1.0] * 5, [F(LONG), F(0, LONG, LONG), F(0, SHORT, SHORT), F(SHORT), F(SHORT, DEAD, DEAD)], [1], is_put=[0, 1, 0, 1, 0]),
    # G0: a quantity of zero is live and adds +-0; one that is not finite kills the option
    "quantities": _case(_MOVED, _T2, [100.0, 100.3], _U5, _T5, [0.0, NAN, 1.0, INF, -0.0], _F5, [2], is_put=_PUT5),
    "one_option": _case(_MOVED, _T2, [100.0, 99.5], [1.05], [1.5 * TAU], [-3.0], [0], [0], is_put=[1]),
    # lag = B - 1: one pair, snapshot 0 against snapshot 2
    "lag_two": _case([_MOVED[0], _PAIR[0], _MOVED[1]], _T2, [100.0, 250.0, 100.3], _U5, _T5, _QTY5, _F5, [0], is_put=_PUT5, lag=2),
}


# ------------------------------------------------------------------ generated batches
def book(c, seed, puts):
    """Sides and quantities for the batch `c`: signed quantities up to 10 in size, every 61st from the 9th not finite, every 19th
    from the 3rd zero."""
    r = np.random.default_rng(seed)
    Q = np.asarray(c["u"]).shape[-1]
    qty = np.round(r.uniform(-10.0, 10.0, Q), 2)
    qty[8::61] = (NAN, INF, -INF)[seed % 3]
    qty[2::19] = 0.0
    return dict(c, is_put=(r.random(Q) < 0.5).astype(np.uint8) if puts else None, qty=qty)


def batch(B, mT, Q, lag, seed, per, puts=True):
    """cal_cases.batch with the spots of one chain (within 2 % of the first snapshot's, so that a strike of end 0 is a strike
    of end 1) and a book.  The snapshots' slices are independent draws: the remainder is large, every placement is exercised."""
    c = DC.batch(B, mT, 1, 0, seed, per_tq=per, rate=0.03 if per else 0.0)
    c = {k: c[k] for k in ("params", "Tq", "spot", "rate")}
    c["spot"] = c["spot"][0] * (1.0 + np.random.default_rng(seed + 11).uniform(-0.02, 0.02, B))
    c = CC.queries(c, Q, seed + 3, per, 1 if per else 0)
    return dict(book(c, seed + 5, puts), lag=lag)


def path(B, mT, Q, lag, seed, h=1.0):
    """One chain observed every minute: snapshot b is snapshot 0 moved by b x h x (dS, dparams, dt): the spot by 0.05 %, a and b
    of every slice by 0.1 % and 0.05 %, m by 0.0002, the expiries by one minute.  Strikes are absolute."""
    c = batch(1, mT, Q, 1, seed, False)
    n = np.arange(B, dtype=np.float64)[:, None] * h
    P = np.repeat(c["params"], B, axis=0)
    P[:, :, 0] *= 1.0 + 0.001 * n
    P[:, :, 1] *= 1.0 + 0.0005 * n
    P[:, :, 3] += 0.0002 * n
    spot = c["spot"][0] * (1.0 + 0.0005 * n[:, 0])
    u = np.tile(c["u"] * c["spot"][0], (B, 1))
    tau = 1.003 * c["tau"][None, :] - MINUTE * n          # off the tenors: an expiry that crosses one meets the kink of E3 (MICRO["brackets"])
    return dict(c, params=P, spot=spot, u=u, tau=np.ascontiguousarray(tau), strike_mode=1, lag=lag)


# B in {2, 3, 65}, lag in {1, 2, B - 1}, mT in {1, 2, 16, 64}, Q in {1, 63, 64, 65, 255, 256, 257, 1025} (one ragged pass, a filled
# wavefront, one over, a filled pass, one over, five passes); shared and per-snapshot inputs (per-snapshot tenors at mT = 64 are
# out of order: UNORDERED), moneyness and strikes, is_put NULL and given.  mT <= 2 goes with B <= 3: dist_cases.batch plants a dead
# row in every 11th, which with one slice per snapshot would leave a fifth of the pairs at B = 65 degenerate.  The sizes are
# kept where the same rules in mpmath stay affordable.
SHAPES = [dict(B=2, mT=1, Q=1, lag=1, seed=1800, per=False, puts=False),
          dict(B=2, mT=2, Q=1025, lag=1, seed=1801, per=True),
          dict(B=3, mT=16, Q=257, lag=2, seed=1802, per=False),
          dict(B=3, mT=16, Q=65, lag=1, seed=1803, per=True, puts=False),
          dict(B=65, mT=16, Q=63, lag=1, seed=1804, per=False),
          dict(B=3, mT=64, Q=64, lag=2, seed=1805, per=True),
          dict(B=3, mT=2, Q=256, lag=1, seed=1806, per=True),
          dict(B=2, mT=16, Q=255, lag=1, seed=1807, per=False),
          dict(B=65, mT=16, Q=2, lag=64, seed=1808, per=True),
          dict(B=3, mT=64, Q=63, lag=1, seed=1809, per=False),
          dict(B=3, mT=1, Q=64, lag=2, seed=1810, per=True)]
PATH_SHAPE = dict(B=9, mT=16, Q=65, lag=1, seed=1850)      # what the workload looks like: small moves, cancelling differences
STREAM_SHAPE = dict(B=65, mT=16, Q=257, lag=1, seed=1891, per=True)
UNORDERED_SHAPES = (5,)                   # per-snapshot tenors at mT = 64: every snapshot UNORDERED, so the conditions on live options do not apply


def shape_id(s):
    return f"B{s['B']}-mT{s['mT']}-Q{s['Q']}-lag{s['lag']}-{'p' if s['per'] else 's'}"
