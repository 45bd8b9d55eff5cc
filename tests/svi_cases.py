"""Hand-built micro cases, one per rule and flag of V1-V8, and the seeded generators of the GPU
shapes.  TEST INFRASTRUCTURE ONLY.  A case is a dict(vol [B,mT,mK], Kq, Tq, spot, rate); a micro case carries besides what
must come out, worked out by hand from the rules: `flags` [B,mT], and `free` [B,mT], the bits the rules leave to rounding
(compared nowhere).  Every tolerance constant below has its measured source in profiles/svi/errlog.txt."""
import numpy as np

NAN, INF = float("nan"), float("inf")
BOUND, EDGE, HOLES, DEAD, BUTTERFLY, DEGENERATE = 1, 2, 4, 8, 16, 32
EPS = float(np.finfo(np.float64).eps)

# Recovery of noiseless SVI rows by the restatement at 16 rounds, over every exact row of SHAPES: the largest |fitted vol -
# generating vol| at a node and the largest |parameter - generating parameter| were 7.8e-11 and 1.5e-9 (errlog.txt); the
# test allows 8 x.
RECOVERY = {"vol": 8 * 7.8e-11, "params": 8 * 1.5e-9}

# Quality of the noisy rows against the best of a bounded multi-start scipy.optimize.least_squares: the worst SSE / SSE_scipy
# - 1 over QUALITY_ROWS noisy rows was 7.8e-15 (errlog.txt): the generating parameters are one of the starts, so the two are
# roundings of one optimum.  The test allows 4 x that, but no less than 1e-10: least_squares stops at xtol = ftol = 1e-15
# relative, its Jacobian is a finite-difference one (relative step 1.5e-8), and another SciPy or BLAS build lands within the
# square of that step of the optimum, not on the same rounding.
QUALITY_MARGIN = max(4 * 7.8e-15, 1e-10)
QUALITY_ROWS = 24

# R_CPU[rounds]: the largest |restatement - twin| over every input the GPU tests run at that number of rounds (MICRO, SHAPES,
# LDS_SHAPE and the chain at 16; SHAPES at 4) and TWIN_SEEDS, on the stable rows: rmse_w relative to rmse_w + RMSE_FLOOR w_max
# (the last grid step, 1e-9 of the domain, leaves an exact row a residual of that order, which is no signal), fitted vols and
# the two vol statistics absolute, m and ln sigma in final grid steps, g_min absolute.  Measured (errlog.txt), recorded here
# rounded up: 4.81e-7, 1.19e-9, 25.0 and 5.70e-9 at 16 rounds (the steps and the vols come from the chain, whose sigma sits
# at its lower border); 7.40e-12, 1.50e-15, 0 and 1.12e-14 at 4 rounds, where every twin run ends on the restatement's own grid
# point: there the same-grid-point bound of the GPU test stands in for the step figure.  The GPU tests allow C_GPU x R_CPU.
R_CPU = {16: {"rmse_w": 4.9e-7, "vol": 1.2e-9, "steps": 25.0, "g_min": 5.8e-9},
         4: {"rmse_w": 7.5e-12, "vol": 1.6e-15, "steps": 0.0, "g_min": 1.2e-14}}
RMSE_FLOOR = 1e-9
C_GPU = 8.0
TWIN_SEEDS = (1, 2, 3)
UNSTABLE_STEPS = 100.0       # twin runs further apart than this in m or ln sigma have flipped basins
UNSTABLE_SHARE = 0.02


def svi_w(x, a, b, rho, m, sigma):
    return a + b * (rho * (x - m) + np.sqrt((x - m) ** 2 + sigma ** 2))


def _case(vol, Kq, Tq, spot, flags, free=0, rate=0.0):
    vol = np.asarray(vol, np.float64)
    if vol.ndim == 2:
        vol = vol[None]
    B, mT, _ = vol.shape
    flags = np.asarray(flags, np.int32).reshape(B, mT)
    return dict(vol=vol, Kq=np.asarray(Kq, np.float64), Tq=np.asarray(Tq, np.float64), spot=np.asarray(spot, np.float64),
                rate=rate, flags=flags, free=np.broadcast_to(np.asarray(free, np.int32), flags.shape).copy())


# 9 strikes round the spot 100, one tenor of 0.25 years; the smile of the micro cases in x = ln(k / 100)
K9 = 100.0 * np.exp(np.linspace(-0.4, 0.4, 9))
X9 = np.log(K9 / 100.0)
TAU = 0.25
P9 = (0.004, 0.05, -0.4, 0.03, 0.12)                       # a, b, rho, m, sigma: well inside every constraint


def _vol(w):
    return np.sqrt(np.asarray(w, np.float64) / TAU)[None, :]


def _with(a, **cells):
    a = np.array(a, np.float64)
    for key, v in cells.items():
        a[0, int(key[1:])] = v
    return a


_SVI9 = _vol(svi_w(X9, *P9))
MICRO = {
    # V1: 4 valid nodes of 9 (every kind of invalid vol, and one invalid strike under a good vol)
    "four_valid_nodes": _case(_with(_SVI9, c0=NAN, c2=0.0, c4=-0.3, c6=INF), np.where(np.arange(9) == 8, NAN, K9), [TAU], [100.0], [DEAD]),
    # V1: valid strikes that do not ascend strictly (descending pair 3, 4; equal pair in snapshot 1)
    "descending_strikes": _case([_SVI9, _SVI9], [np.where(np.arange(9) == 3, K9[4] + 1.0, K9), np.where(np.arange(9) == 3, K9[4], K9)],
                                [TAU], [100.0, 100.0], [[DEAD], [DEAD]]),
    # V1: a hole between valid nodes is skipped and flagged; the fit through the other 8 nodes is the generating curve
    "a_hole": _case(_with(_SVI9, c3=NAN), K9, [TAU], [100.0], [HOLES]),
    # V4: a straight-line skew is the limit sigma -> 0, m -> beyond the last node of the left wing rho = -1: the search ends
    # in the corner (m = last x, lowest sigma), the linear problem on the edge d = -c
    "straight_line_skew": _case(_vol(0.02 - 0.02 * X9), K9, [TAU], [100.0], [BOUND | EDGE]),
    # V5: on a flat row every candidate fits exactly with b = 0, and the first of equals is the lower corner of the domain;
    # the unconstrained solution sits ON the vertex c = d = 0, so BOUND is rounding's to decide
    "flat_row": _case(_vol(np.full(9, 0.0625)), K9, [TAU], [100.0], [EDGE], free=BOUND),
    # V1: no spot, no tenor, a negative tenor: DEAD whatever the row holds
    "spot_nan": _case([_SVI9, _SVI9, _SVI9], K9, [[TAU], [NAN], [-TAU]], [NAN, 100.0, 100.0], [[DEAD], [DEAD], [DEAD]]),
    # V1: exactly 5 valid nodes are enough (a smile through 5 nodes, the other 4 holes outside and between)
    "five_nodes": _case(_with(_SVI9, c0=NAN, c3=NAN, c5=NAN, c8=NAN), K9, [TAU], [100.0], [HOLES]),
    # V7: a sharp V cannot be fitted without a kink: g < 0 next to it
    "v_shape": _case(_vol(0.002 + 0.3 * np.abs(X9)), K9, [TAU], [100.0], [BUTTERFLY]),
}
# the rows of MICRO that the twin runs may move by more than UNSTABLE_STEPS (all their candidates tie at rounding level)
MICRO_UNSTABLE = {"flat_row"}


def batch(B, mT, mK, seed, per_kq=True, holes=0.1, rate=0.0, noise=0.002, exact_every=4):
    """Raw-SVI smiles: per row its own (a, b, rho, m, sigma), well inside the constraints, on strikes S exp(x) with x
    spread evenly over +- 2.5 standard deviations of the row's tenor at vol 0.5 ... of the LONGEST tenor when the grid is
    shared (jittered per snapshot when it is per snapshot).  Row r = b mT + j is exact when r % exact_every == 0, else
    it carries normal vol noise of `noise` (20 bp).  holes: the share of nodes made invalid (NaN / 0 / negative / inf).
    Returns the case and `gen` = dict(params [B,mT,5], exact [B,mT] bool, clean [B,mT,mK] the generating vols)."""
    r = np.random.default_rng(seed)
    spot = r.uniform(50.0, 30000.0, B)
    Tq = np.geomspace(5.0 / 365.0, 90.0 / 365.0, mT) if mT > 1 else np.array([30.0 / 365.0])
    half = 2.5 * 0.5 * np.sqrt(Tq[-1])
    x = np.linspace(-half, half, mK)
    if per_kq:
        xs = x[None, :] + r.uniform(-0.2, 0.2, (B, mK)) * (2 * half / (mK - 1))
        Kq = spot[:, None] * np.exp(xs)
    else:
        spot = spot[0] * np.exp(r.uniform(-0.05, 0.05, B))               # one shared grid: the spots stay near it
        Kq = spot[0] * np.exp(x)
        xs = np.log(Kq[None, :] / spot[:, None])
    xx = xs[:, None, :] - rate * Tq[None, :, None]
    w0 = (r.uniform(0.4, 0.6, (B, mT, 1)) ** 2) * Tq[None, :, None]     # the level: vols of 40 .. 60 %
    sig = r.uniform(0.25, 0.5, (B, mT, 1)) * half
    m = r.uniform(-0.15, 0.15, (B, mT, 1)) * half
    rho = r.uniform(-0.6, 0.2, (B, mT, 1))
    b = r.uniform(0.3, 0.8, (B, mT, 1)) * w0 / half
    a = w0 * r.uniform(0.3, 0.6, (B, mT, 1))
    clean = np.sqrt(svi_w(xx, a, b, rho, m, sig) / Tq[None, :, None])
    exact = (np.arange(B * mT).reshape(B, mT) % exact_every) == 0
    vol = np.where(exact[:, :, None], clean, clean + r.normal(0.0, noise, clean.shape))
    assert vol.min() > 0.1 and vol.max() < 3.0
    if holes > 0:
        bad = r.random(vol.shape) < holes
        vol = np.where(bad, r.choice([NAN, 0.0, -0.4, INF], vol.shape), vol)
    case = dict(vol=np.ascontiguousarray(vol), Kq=np.ascontiguousarray(Kq), Tq=np.ascontiguousarray(Tq), spot=spot, rate=rate)
    gen = dict(params=np.concatenate([a, b, rho, m, sig], axis=-1), exact=exact, clean=clean)
    return case, gen


# (B, mT, mK): the smallest legal row; a few short rows; one chunk; one node into the second chunk; two chunks and a bit (the
# carried strike of the ascending check, holes at chunk edges); the bench's row shape; and a batch of many workgroups, used
# once, by the stream test (bitwise against itself, no restatement).  Each with shared and per-snapshot strike grids.
SHAPES = []
for n_, (B_, mT_, mK_) in enumerate(((1, 1, 5), (3, 2, 7), (5, 3, 64), (5, 3, 65), (2, 2, 130), (3, 16, 64))):
    for q_, per_ in enumerate((False, True)):
        SHAPES.append(dict(B=B_, mT=mT_, mK=mK_, seed=900 + 2 * n_ + q_, per_kq=per_, rate=0.03 if per_ else 0.0,
                           holes=0.1 if mK_ >= 7 else 0.0))
STREAM_SHAPE = dict(B=64, mT=16, mK=64, seed=990, per_kq=True, rate=0.03)
# the longest row the call takes: with rows_per_wg = 4 the workgroup asks for the whole 64 KiB of LDS, and its last slot is
# used by no row (5 rows: the second workgroup holds one)
LDS_SHAPE = dict(B=1, mT=5, mK=1024, seed=995, per_kq=False, rate=0.0)


def shape_id(s):
    return f"B{s['B']}-mT{s['mT']}-mK{s['mK']}-{'k' if s['per_kq'] else 's'}-r{s['rate']}"


# The end-to-end chain of the GPU test (snapshot_cases.big_chain: a put / call offset of 3 vol points leaves a step at the
# forward, so sigma runs to its lower border on most rows), on the tenors of the sibling stages' chain tests, at the default
# rounds.
CHAIN = dict(n_und=2, nT=4, nK=24, minutes=40, seed=4)
CHAIN_MONEYNESS = np.linspace(0.72, 1.28, 64)
CHAIN_TENORS = np.linspace(8.0, 20.0, 6) / 365.0
CHAIN_RATE = 0.01
