"""Hand-built micro cases of rules G0-G6 and B1-B5, the seeded generators of the GPU shapes and the
tolerances.  TEST INFRASTRUCTURE ONLY.  A case is an evaluation case of cal_cases (params, Tq, spot, rate, u, tau, strike_mode)
plus is_put [Q] or None, qty [Q], spot_shocks and vol_shocks; a micro case also carries what must come out, worked out by hand
from the rules: `flags` [B,Q], `n_dead` [B] and `cell_flags` [B,nA,nV].  The constants R_CPU below have their measured source in
profiles/risk/errlog.txt."""
import numpy as np

import cal_cases as CC

NAN, INF = float("nan"), float("inf")
EPS, TINY = CC.EPS, CC.TINY
SHORT, LONG, NEG_FWD, Q_DEAD, Q_UNORDERED = 1, 2, 4, 8, 32
NEG_VOL_SS, NEG_VOL_SM = 1, 2
GREEK_KEYS = ("price", "delta_ss", "delta_sm", "gamma_ss", "gamma_sm", "vega", "theta")
VALUE_KEYS = GREEK_KEYS + ("net", "pnl_ss", "pnl_sm")
DEFAULT_SPOT_SHOCKS = (-0.20, -0.15, -0.10, -0.05, 0.0, 0.05, 0.10, 0.15, 0.20)
DEFAULT_VOL_SHOCKS = (-0.10, -0.05, 0.0, 0.05, 0.10)

# R_CPU: the largest |fp64 restatement - the same rules in mpmath at 50 digits| over every input the GPU tests use (MICRO, SHAPES,
# STREAM_SHAPE and the chain's book with the restatement's own SVI fit), in units of eps x the value's scale (first-order
# propagation through the rule's own terms, risk_ref.restate_*; for a sum over the book the summed units of its terms plus
# eps x L x the sum of their magnitudes, L the depth of rule B5).  Measured by test_risk.test_rounding_level (errlog.txt) and
# recorded here with a margin.  The scales count every rounding of a term generously, so the figures stay below 1.
# The GPU tests allow C_GPU x R_CPU, the project's standing margin for the device's erfc / exp / log / sqrt / division.
# Measured: price 0.0948, delta_ss 0.379, delta_sm 0.371, gamma_ss 0.342, gamma_sm 0.327, vega 0.360, theta 0.302 (each on the
# B64-mT16-Q63 batch or the stream shape), net 0.110 (the chain's book), pnl_ss 0.0209 and pnl_sm 0.0221 (the 32 x 32 grid): the
# unit of a sum counts L roundings of the whole book per cell, which a sum in the same order never spends.  The worst of some
# thousand values moves when another host's exp / log / erfc change last bits of intermediates (section 16 saw +- 0.3 of a
# unit on figures near 1), so each figure is recorded a third higher, rounded up.
R_CPU = {"price": 0.13, "delta_ss": 0.51, "delta_sm": 0.50, "gamma_ss": 0.46, "gamma_sm": 0.44, "vega": 0.48, "theta": 0.41,
         "net": 0.15, "pnl_ss": 0.028, "pnl_sm": 0.030}
C_GPU = 8.0


def tolerances_greeks(ref, factor):
    """Absolute tolerances of the Greeks of `ref` (a restatement) at `factor` units: factor x eps x the value's scale, plus the
    smallest normal number (an underflowed value has no relative precision left)."""
    with np.errstate(all="ignore"):
        return {k: factor[k] * EPS * ref["scale_" + k] + TINY for k in GREEK_KEYS}


def tolerances_book(ref, factor):
    with np.errstate(all="ignore"):
        return {k: factor[k] * EPS * ref["scale_" + k] + TINY for k in ("net", "pnl_ss", "pnl_sm")}


def units(got, ref, tol_fn, keys):
    """|got - ref| of every compared value in the units of its tolerance: the factor at which it would just pass (the additive
    term taken off first).  NaN where both are NaN."""
    one, zero = tol_fn(ref, {k: 1.0 for k in R_CPU}), tol_fn(ref, {k: 0.0 for k in R_CPU})
    out = {}
    with np.errstate(all="ignore"):
        for k in keys:
            if got.get(k) is None:
                continue
            d = np.abs(np.asarray(got[k], np.float64) - ref[k])
            out[k] = np.where(d <= zero[k], 0.0, (d - zero[k]) / (one[k] - zero[k]))
    return out


# ------------------------------------------------------------------ micro cases
def _risk(ev, is_put, qty, spot_shocks=DEFAULT_SPOT_SHOCKS, vol_shocks=DEFAULT_VOL_SHOCKS, n_dead=None, cell_flags=0, flags=None):
    c = {k: ev[k] for k in ("params", "Tq", "spot", "rate", "u", "tau", "strike_mode")}
    B, Q = ev["flags"].shape
    c.update(is_put=None if is_put is None else np.asarray(is_put, np.uint8), qty=np.asarray(qty, np.float64),
             spot_shocks=tuple(spot_shocks), vol_shocks=tuple(vol_shocks),
             flags=ev["flags"].copy() if flags is None else np.asarray(flags, np.int32).reshape(B, Q),
             n_dead=np.asarray(n_dead, np.int32).reshape(B),
             cell_flags=np.broadcast_to(np.asarray(cell_flags, np.int32), (B, len(spot_shocks), len(vol_shocks))).copy())
    return c


_E = CC.MICRO_EVAL
_FLAT1 = CC._ev([(0.04 * t, 0.0, 0.0, 0.0, 0.1) for t in CC.FLAT_T], CC.FLAT_T, [1.05], [0.3], [0], rate=0.03)
MICRO = {
    # b = 0: 20 % vol everywhere; the sticky-moneyness Greeks are the sticky-strike ones and both are Black-Scholes'
    "flat": _risk(_E["flat"], [0, 1, 0, 1, 0, 1], [1.0, -2.0, 3.0, 0.5, -1.5, 2.0], n_dead=[0]),
    # E1: every dead cause of a query (8 of the 9 options), then a snapshot without a live slice: all NaN, n_dead = Q
    "dead_queries": _risk(_E["dead_queries"], [0, 1] * 4 + [0], [1.0] * 9, n_dead=[8, 9]),
    "unordered": _risk(_E["unordered"], None, [1.0, 1.0], n_dead=[1, 2]),
    "short_long": _risk(_E["single_slice"], [1, 0, 1], [1.0, 1.0, -1.0], n_dead=[0]),
    "calendar_pair": _risk(_E["inside_a_calendar_pair"], [0, 1, 0], [1.0, 2.0, 3.0], n_dead=[0]),     # NEG_FWD, theta still formed
    "one_option": _risk(_FLAT1, [1], [-3.0], n_dead=[0]),
    # a quantity of zero: live, adds +-0 to every sum; with it alone every sum is +0.0
    "qty_zero": _risk(_E["flat"], [0, 1, 0, 1, 0, 1], [0.0, 1.0, 0.0, -1.0, 0.0, 0.0], n_dead=[0]),
    "qty_all_zero": _risk(_FLAT1, None, [0.0], n_dead=[0]),
    # G0: a quantity that is not finite kills the option (its flags stay those of E1-E3)
    "qty_nan": _risk(_E["flat"], [0, 1, 0, 1, 0, 1], [1.0, NAN, 1.0, INF, -INF, 2.0], n_dead=[3]),
    # B3: vol 0.2 with shocks of -0.25 (below zero), -0.2 (exactly zero: sqrt(0.04 t / t) is 0.2 to the bit) and -0.1
    "neg_vol": _risk(_FLAT1, [0], [1.0], spot_shocks=(-0.1, 0.0), vol_shocks=(-0.25, -0.2, -0.1), n_dead=[0],
                     cell_flags=[[[3, 3, 0]] * 2]),
    # B4 on a skewed pair of slices, calls and puts, both signs of quantity
    "zero_cell": _risk(CC._ev([CC.GOOD, CC.LATER], CC._T2, [0.8, 0.95, 1.0, 1.1, 1.3], [0.2, 0.3, 0.3, 0.4, 0.6], [SHORT, 0, 0, 0, LONG], rate=0.03),
                       [1, 0, 1, 0, 0], [1.0, -2.0, 0.5, -0.25, 3.0], spot_shocks=(-0.1, 0.0, 0.1), vol_shocks=(0.0, 0.02), n_dead=[0]),
    # nA nV == 0: net and n_dead alone
    "no_grid": _risk(_E["flat"], None, [1.0] * 6, spot_shocks=(), vol_shocks=DEFAULT_VOL_SHOCKS, n_dead=[0]),
}


# ------------------------------------------------------------------ generated batches
def book(c, seed, puts, spot_shocks, vol_shocks):
    """Sides, quantities and a scenario grid for the evaluation batch `c`: signed quantities up to 10 in size, every 61st from
    the 9th not finite, every 19th from the 3rd zero."""
    r = np.random.default_rng(seed)
    Q = np.asarray(c["u"]).shape[-1]
    qty = np.round(r.uniform(-10.0, 10.0, Q), 2)
    qty[8::61] = (NAN, INF, -INF)[seed % 3]
    qty[2::19] = 0.0
    return dict(c, is_put=(r.random(Q) < 0.5).astype(np.uint8) if puts else None, qty=qty, spot_shocks=tuple(spot_shocks), vol_shocks=tuple(vol_shocks))


def make_grid(nA, nV):
    """An nA x nV grid inside +-20 % of spot and -3 ... +5 points of vol, the zero shock on each axis that has three or more."""
    a = np.linspace(-0.2, 0.2, nA) if nA > 1 else np.array([0.07])
    v = np.linspace(-0.03, 0.05, nV) if nV > 1 else np.array([0.02])
    if nA >= 3:
        a[nA // 2] = 0.0
    if nV >= 3:
        v[nV // 2] = 0.0
    return tuple(float(z) for z in a), tuple(float(z) for z in v)


# B in {1, 3, 64}, mT in {1, 2, 16, 64}, Q in {1, 63, 64, 65, 255, 256, 257, 1025} (one ragged pass, a filled wavefront, one over,
# a filled pass, one over, five passes), the grids 1x1, 1x5, 9x1, 9x5, 33x31 (four runs of cells, the last ragged) and 32x32 (the
# limit); shared and per-snapshot inputs (per-snapshot tenors at mT = 64 are out of order: UNORDERED), moneyness and strikes,
# is_put NULL and given.  The sizes are kept where the same rules in mpmath stay affordable: Q x cells is what counts.
SHAPES = [dict(B=1, mT=1, Q=1, seed=1700, per=False, puts=False, grid=(1, 1)),
          dict(B=1, mT=2, Q=1025, seed=1701, per=True, puts=True, grid=(1, 5)),
          dict(B=3, mT=16, Q=257, seed=1702, per=False, puts=True, grid=(9, 1)),
          dict(B=3, mT=16, Q=65, seed=1703, per=True, puts=False, grid=(9, 5)),
          dict(B=64, mT=16, Q=63, seed=1704, per=False, puts=True, grid=(1, 1)),
          dict(B=1, mT=64, Q=2, seed=1705, per=False, puts=True, grid=(33, 31)),
          dict(B=1, mT=2, Q=3, seed=1706, per=True, puts=True, grid=(32, 32)),
          dict(B=3, mT=2, Q=256, seed=1707, per=True, puts=True, grid=(1, 5)),
          dict(B=1, mT=16, Q=255, seed=1708, per=False, puts=False, grid=(9, 5)),
          dict(B=1, mT=1, Q=64, seed=1709, per=True, puts=True, grid=(9, 5)),
          dict(B=3, mT=64, Q=63, seed=1710, per=True, puts=True, grid=(1, 5))]
STREAM_SHAPE = dict(B=64, mT=16, Q=257, seed=1791, per=True, puts=True, grid=(9, 5))
UNORDERED_SHAPES = (10,)                  # per-snapshot tenors at mT = 64: every snapshot UNORDERED, so the conditions on live options do not apply


def batch(B, mT, Q, seed, per, puts, grid):
    a, v = make_grid(*grid)
    return book(CC.batch(B, mT, Q, seed, per), seed + 5, puts, a, v)


def shape_id(s):
    return f"B{s['B']}-mT{s['mT']}-Q{s['Q']}-{s['grid'][0]}x{s['grid'][1]}-{'p' if s['per'] else 's'}"


def chain_book(res):
    """cal_cases.chain_book (12 options round the first underlying's spot, the last one expired) with sides and quantities."""
    b = CC.chain_book(res)
    b["callput"] = ["c", "P", "call", "put", "C", "p", "c", "p", "c", "p", "c", "p"]
    b["quantity"] = [1.0, -2.0, 3.0, 1.5, -1.0, 2.0, -0.5, 4.0, 1.0, -3.0, NAN, 1.0]
    return b
