"""Hand-built micro cases, one per rule and flag of P1-P8, the seeded generators of the GPU shapes and
the tolerances.  TEST INFRASTRUCTURE ONLY.  A case is a dict(params [B,mT,5], Tq, spot, rate, probs, levels, max_tail); a
micro case carries besides what must come out, worked out by hand from the rules: `flags` [B,mT] and `q_flags` [B,mT,nP].
The constant R_CPU below has its measured source in profiles/distribution/errlog.txt."""
import numpy as np

import svi_cases as SC

NAN, INF = float("nan"), float("inf")
NO_BRACKET, AMBIGUOUS, TAILS, DEAD = 1, 2, 4, 8
EPS = float(np.finfo(np.float64).eps)
DEFAULT_PROBS = (0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99)
DEFAULT_LEVELS = (0.8, 0.9, 1.0, 1.1, 1.2)

# R_CPU: the largest |fp64 restatement - the same rules in mpmath at 50 digits| over every input the GPU tests use (MICRO,
# SHAPES with their level lists, STREAM_SHAPE's first rows and the chain with the restatement's own SVI fit), in units of
# eps x the rule's scale (tolerances() below).  Measured by test_distribution.test_rounding_level (errlog.txt): 1.49 for L /
# U / the tails / the level probabilities, 1.65 for q_x, 0.36 for q_strike (each on the Lee-bound micro slice; the generated
# batches stay below 1.0, 0.62 and 0.09); recorded here rounded up.  The GPU tests allow
# C_GPU x R_CPU, the project's standing margin for FMA contraction and the device's erfc / exp / log / sqrt / division.
R_CPU = {"prob": 1.5, "q_x": 1.7, "q_strike": 0.4}
C_GPU = 8.0
BISECTION_WIDTH = 4.0 * 2.0 ** -52       # of the bracket: where 52 halvings stop, either side of the sign change
STRIKE_EPS = 4.0                         # exp, the product with F and F's own exp: a few eps relative
TINY = float(np.finfo(np.float64).tiny)  # below the normal range a probability has no relative precision left


def tolerances(ref, c, factor):
    """Absolute tolerances of every output of `ref` (a restatement of `c`) at `factor` units: factor x eps x the scale of
    DESIGN.md section 13.  L, U and the tails: Phi (1 + d2^2) + phi |theta'| (1 + d2^2) + (|x| / theta) phi at the point;
    plus the smallest normal number (an underflowed tail has no relative precision); q_x: that scale at the root over
    |L'(x*)|, plus 4 x 2^-52 of the bracket's width; q_strike: F e^x* times q_x's, plus a few eps relative.  `factor` is a dict with the keys of R_CPU."""
    with np.errstate(all="ignore"):
        qx = factor["q_x"] * EPS * ref["q_scale"] / np.abs(ref["q_dens"]) + BISECTION_WIDTH * ref["width"]
        strike = np.abs(ref["q_strike"])
        qk = strike * (factor["q_strike"] * EPS * ref["q_scale"] / np.abs(ref["q_dens"]) + BISECTION_WIDTH * ref["width"] + STRIKE_EPS * EPS)
        t = {"q_x": qx, "q_strike": qk, "tails": factor["prob"] * EPS * ref["tail_scale"] + TINY}
        if len(c["levels"]):
            t["p_below"], t["p_above"] = factor["prob"] * EPS * ref["below_scale"] + TINY, factor["prob"] * EPS * ref["above_scale"] + TINY
    return t


def units(got, ref, c):
    """|got - ref| of every compared output in the units of tolerances(): the factor at which the output would just pass
    (the additive terms of q_x and q_strike taken off first).  NaN where both are NaN."""
    one = tolerances(ref, c, {k: 1.0 for k in R_CPU})
    zero = tolerances(ref, c, {k: 0.0 for k in R_CPU})
    out = {}
    with np.errstate(all="ignore"):
        for k in one:
            d = np.abs(np.asarray(got[k], np.float64) - ref[k])
            out[k] = np.where(d <= zero[k], 0.0, (d - zero[k]) / (one[k] - zero[k]))
    return out


UNIT_KEY = {"q_x": "q_x", "q_strike": "q_strike", "tails": "prob", "p_below": "prob", "p_above": "prob"}


def _case(params, Tq, spot, flags, q_flags, rate=0.0, probs=DEFAULT_PROBS, levels=DEFAULT_LEVELS, max_tail=1e-6):
    params = np.asarray(params, np.float64)
    if params.ndim == 2:
        params = params[None]
    B, mT, _ = params.shape
    flags = np.asarray(flags, np.int32).reshape(B, mT)
    q_flags = np.broadcast_to(np.asarray(q_flags, np.int32), (B, mT, len(probs))).copy()
    return dict(params=params, Tq=np.asarray(Tq, np.float64), spot=np.asarray(spot, np.float64), rate=rate, probs=tuple(probs),
                levels=tuple(levels), max_tail=max_tail, flags=flags, q_flags=q_flags)


GOOD = (0.004, 0.05, -0.4, 0.03, 0.12)                     # a, b, rho, m, sigma: a smile well inside every condition of P1
TAU = 0.25


def _with(**cells):
    p = list(GOOD)
    for k, v in cells.items():
        p["a b rho m sigma".split().index(k)] = v
    return p


# P1, one snapshot per cause (mT = 1, a tenor per snapshot): name, parameters, spot, tenor
DEAD_CAUSES = [
    ("control", GOOD, 100.0, TAU),
    ("spot nan", GOOD, NAN, TAU), ("spot zero", GOOD, 0.0, TAU), ("spot negative", GOOD, -100.0, TAU), ("spot inf", GOOD, INF, TAU),
    ("tenor nan", GOOD, 100.0, NAN), ("tenor zero", GOOD, 100.0, 0.0), ("tenor negative", GOOD, 100.0, -TAU), ("tenor inf", GOOD, 100.0, INF),
    ("a nan", _with(a=NAN), 100.0, TAU), ("b nan", _with(b=NAN), 100.0, TAU), ("rho nan", _with(rho=NAN), 100.0, TAU),
    ("m nan", _with(m=NAN), 100.0, TAU), ("sigma nan", _with(sigma=NAN), 100.0, TAU),
    ("a inf", _with(a=INF), 100.0, TAU), ("b inf", _with(b=INF), 100.0, TAU), ("m -inf", _with(m=-INF), 100.0, TAU), ("sigma inf", _with(sigma=INF), 100.0, TAU),
    ("b negative", _with(b=-0.05), 100.0, TAU), ("rho above 1", _with(rho=1.0 + 2.0 ** -52), 100.0, TAU), ("rho below -1", _with(rho=-1.5), 100.0, TAU),
    ("sigma zero", _with(sigma=0.0), 100.0, TAU), ("sigma negative", _with(sigma=-0.12), 100.0, TAU),
    # w_min = a + b sigma sqrt(1 - rho^2): exactly 0 (rho = 0, a = -b sigma = -0.25 x 0.5, exact in fp64) and below 0
    ("w_min zero", (-0.125, 0.25, 0.0, 0.0, 0.5), 100.0, TAU), ("w_min negative", _with(a=-0.01), 100.0, TAU),
    ("a dead row of the fit", (NAN,) * 5, 100.0, TAU),
    # the borders that are still live: b = 0 (flat), |rho| = 1 with a > 0
    ("rho is 1", _with(rho=1.0), 100.0, TAU), ("rho is -1", _with(rho=-1.0), 100.0, TAU),
]
_LIVE = {"control", "rho is 1", "rho is -1"}

# P5 / P8 on the issue's Lee-bound slice: the right wing's slope b (1 + rho) = 1.9 and the kink sigma = 0.01 push L up to 2.7
# just right of the forward, from where it FALLS to 1: the CDF is not monotone, but every level in (0, 1) is crossed upward
# once, so no target is AMBIGUOUS (the issue expected some); U(x_63) = -5.4e-6, beyond max_tail = 1e-6: TAILS.
LEE = (4e-4, 1.0, 0.9, 0.0, 0.01)
# P5: a symmetric V (rho = 0) with a sharp kink (sigma = 0.001): theta' jumps from -b/(2 theta) to +b/(2 theta) across the
# kink, so L falls below 0 on its left (to -0.2), jumps to 1.2 and falls back below 1 before it rises to 1 again.  The levels
# 0.02 and 0.98 are each crossed upward twice (AMBIGUOUS), 0.5 once; both tails (7.4e-5, 1.4e-5) exceed max_tail: TAILS.
KINK = (4e-4, 0.1, 0.0, 0.0, 0.001)
# P5: L(x_0) = 2.8e-15 on the Lee slice and L rises from there: a target of 1e-15 has h >= 0 at every grid point.  FAT is a
# smooth slice with a monotone CDF whose right wing (slope 0.38) leaves U(x_63) = 6.1e-10 beyond the grid: the target
# 1 - 1e-10 has h = 1e-10 - U < 0 at every grid point.  Both tails of FAT stay below max_tail: no TAILS.
FAT = (0.001, 0.2, 0.9, 0.0, 0.1)

MICRO = {
    "dead_causes": _case([[p] for _, p, _, _ in DEAD_CAUSES], [[t] for _, _, _, t in DEAD_CAUSES], [s for _, _, s, _ in DEAD_CAUSES],
                         [[0 if n in _LIVE else DEAD] for n, _, _, _ in DEAD_CAUSES],
                         [[[0 if n in _LIVE else DEAD]] for n, _, _, _ in DEAD_CAUSES]),
    # P2 / P6: b = 0 is Black-Scholes at total vol theta = 0.2: x = theta inv_cdf(p) - theta^2 / 2, in closed form
    "flat_smile": _case([[(0.04, 0.0, 0.0, 0.0, 0.1)]], [TAU], [100.0], [0], 0, rate=0.03),
    "lee_bound_kink": _case([[LEE]], [TAU], [100.0], [TAILS], 0),
    "symmetric_kink": _case([[KINK]], [TAU], [100.0], [TAILS], [AMBIGUOUS, 0, AMBIGUOUS], probs=(0.02, 0.5, 0.98)),
    "beyond_the_grid": _case([[LEE, FAT]], [TAU, 2 * TAU], [100.0], [TAILS, 0], [[[NO_BRACKET, 0, 0], [0, 0, NO_BRACKET]]],
                             probs=(1e-15, 0.5, 1.0 - 1e-10), levels=()),
    # P8: max_tail = 0 flags every row whose grid leaves anything out; max_tail = 1 none (here the Lee slice's 5.4e-6)
    "max_tail_zero": _case([[LEE, GOOD]], [TAU, TAU], [100.0], [TAILS, TAILS], 0, max_tail=0.0),
    "max_tail_one": _case([[LEE, GOOD]], [TAU, TAU], [100.0], [0, 0], 0, max_tail=1.0),
}


def probs_for(nP):
    """1: the median; 5 and 7: the cone; 16: log-spaced from 1e-6 to 1 - 1e-6."""
    if nP == 1:
        return (0.5,)
    if nP == 5:
        return (0.01, 0.25, 0.5, 0.75, 0.99)
    if nP == 7:
        return DEFAULT_PROBS
    lo = np.geomspace(1e-6, 0.4, nP // 2)
    return tuple(lo) + tuple(1.0 - lo[::-1]) + ((0.5,) if nP % 2 else ())


def levels_for(nL):
    return tuple(np.linspace(0.8, 1.2, nL)) if nL != 16 else tuple(np.geomspace(0.5, 2.0, 16))


def batch(B, mT, nP, nL, seed, per_tq=False, rate=0.0, dead_every=11):
    """Parameters of svi_cases.batch (rows well inside every condition), every `dead_every`-th row from the 6th on overwritten
    by a DEAD cause in turn (none when the batch has fewer than 10 rows); shared tenors, or per snapshot (jittered by 10 %)."""
    c, gen = SC.batch(B, mT, 9, seed, per_kq=True, holes=0.0, rate=rate)
    params = np.ascontiguousarray(gen["params"], np.float64).copy()
    spot, Tq = c["spot"].copy(), c["Tq"]
    r = np.random.default_rng(seed + 7)
    if per_tq:
        Tq = Tq[None, :] * r.uniform(0.9, 1.1, (B, mT))
    causes = [q for n, q, s, t in DEAD_CAUSES if n not in _LIVE and s == 100.0 and t == TAU]
    flat = params.reshape(-1, 5)
    if len(flat) >= 10:
        for n, row in enumerate(range(5, len(flat), dead_every)):
            flat[row] = causes[n % len(causes)]
    return dict(params=params, Tq=np.ascontiguousarray(Tq), spot=spot, rate=rate, probs=probs_for(nP), levels=levels_for(nL),
                max_tail=1e-6)


# (B, mT, nP, nL): one row, one lane; 6 rows: a ragged last wavefront at 12 rows per wave; exactly 12 rows: one filled
# wavefront; 26 rows: 12 + 12 + 2; 15 rows at 4 per wave, ragged; the bench's row shape; 64 rows in one wavefront.  Each with
# shared tenors at rate 0 and per-snapshot tenors at rate 0.03.
SHAPES = []
for n_, (B_, mT_, nP_, nL_) in enumerate(((1, 1, 1, 5), (3, 2, 5, 0), (4, 3, 5, 16), (2, 13, 5, 5), (5, 3, 16, 5), (3, 16, 7, 5), (64, 1, 1, 16))):
    for q_, per_ in enumerate((False, True)):
        SHAPES.append(dict(B=B_, mT=mT_, nP=nP_, nL=nL_, seed=1300 + 2 * n_ + q_, per_tq=per_, rate=0.03 if per_ else 0.0))
STREAM_SHAPE = dict(B=64, mT=16, nP=7, nL=5, seed=1390, per_tq=True, rate=0.03)


def shape_id(s):
    return f"B{s['B']}-mT{s['mT']}-nP{s['nP']}-nL{s['nL']}-{'t' if s['per_tq'] else 's'}-r{s['rate']}"
