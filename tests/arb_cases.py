"""Hand-built micro surfaces, one per rule A1-A5, the closed-form anchors and the generators of the
dense synthetic surfaces.  TEST INFRASTRUCTURE ONLY.  A micro case is a dict(vol [B,mT,mK], Kq, Tq, spot, rate) plus what
must come out, worked out by hand from the rules: `flags` [B,mT,mK] and `counts` [B,4]."""
import itertools

import numpy as np

NAN, INF = float("nan"), float("inf")
CAL, BFLY, NOST, DEAD = 1, 2, 4, 8
EPS = float(np.finfo(np.float64).eps)

# Rounding level of the float64 restatement against the same rules in np.longdouble, in units of eps x scale: the largest
# ratio over every input the GPU tests use (GPU_SHAPES, BIG, ROUGH, WHOLE below) was 1.76 (N) and 1.40 (g), recorded here
# rounded up (test_arbitrage.py::test_rounding_level asserts that it stays below R_CPU).  The GPU tests allow C = 8 x R_CPU.
R_CPU = 2.0
C_GPU = 8.0 * R_CPU


def _case(vol, Kq, Tq, spot, flags, counts, rate=0.0):
    vol = np.asarray(vol, np.float64)
    if vol.ndim == 2:
        vol = vol[None]
    return dict(vol=vol, Kq=np.asarray(Kq, np.float64), Tq=np.asarray(Tq, np.float64), spot=np.asarray(spot, np.float64),
                rate=rate, flags=np.asarray(flags, np.int32).reshape(vol.shape), counts=np.asarray(counts, np.int32).reshape(-1, 4))


K5 = [80.0, 90.0, 100.0, 110.0, 120.0]
K7 = [70.0, 80.0, 90.0, 100.0, 110.0, 120.0, 130.0]
EDGE5, ROW5 = [NOST] * 5, [NOST, 0, 0, 0, NOST]


def _flat(mT, mK, sigma=0.5):
    return np.full((mT, mK), sigma)


def _with(a, **cells):
    a = np.array(a, np.float64)
    for key, v in cells.items():
        j, i = (int(c) for c in key[1:].split("_"))
        a[j, i] = v
    return a


CASES = {
    # A3/A4 on the plainest input: the first and the last strike have no strike stencil, everything else is clean
    "flat": _case(_flat(3, 5), K5, [0.1, 0.2, 0.3], [100.0], [ROW5] * 3, [9, 0, 0, 9]),
    # A5 calendar: w = 0.025, 0.010, 0.075, 0.100 at tau = 0.1 .. 0.4.  Row 0 differences forward INTO the dip (< 0); row 1,
    # the dip itself, takes the central difference of rows 0 and 2 (> 0, equal spacing: its own w has weight 0); rows 2, 3 > 0
    "calendar_dip": _case(_with(_flat(4, 5), c1_0=0.2236, c1_1=0.2236, c1_2=0.2236, c1_3=0.2236, c1_4=0.2236), K5,
                          [0.1, 0.2, 0.3, 0.4], [100.0], [[NOST, CAL, CAL, CAL, NOST], ROW5, ROW5, ROW5], [12, 3, 0, 9]),
    # A5 calendar on unequal spacing: tau = 0.1, 0.2, 0.21, 0.4 and a dip in row 2 (w = 0.025, 0.05, 0.04, 0.1).  Row 1's
    # 3-point weights are -0.909, -90, +90.9: 90.9 * 0.04 - 90 * 0.05 - 0.909 * 0.025 = -0.89 < 0; row 2's are -95, +94.7,
    # +0.263: -95 * 0.05 + 94.7 * 0.04 + 0.263 * 0.1 = -0.93 < 0; row 3 differences backward (0.1 - 0.04 > 0); row 0 forward
    "calendar_dip_unequal": _case(_with(_flat(4, 5), c2_0=0.43644, c2_1=0.43644, c2_2=0.43644, c2_3=0.43644, c2_4=0.43644), K5,
                                  [0.1, 0.2, 0.21, 0.4], [100.0],
                                  [ROW5, [NOST, CAL, CAL, CAL, NOST], [NOST, CAL, CAL, CAL, NOST], ROW5], [12, 6, 0, 6]),
    # A5 butterfly: one node sticks out of a flat smile (w0 = 0.049 between 0.025 and 0.025: w'' = -4.8, g = -1.4); at its
    # strike neighbours w'' > 0 and g > 0; N stays > 0 in both rows (0.075 - 0.049 over 0.2)
    "butterfly_kink": _case(_with(_flat(2, 7), c0_3=0.7), K7, [0.1, 0.3], [100.0],
                            [[NOST, 0, 0, BFLY, 0, 0, NOST], [NOST, 0, 0, 0, 0, 0, NOST]], [10, 0, 1, 9]),
    # A1/A3/A4: a NaN hole is DEAD and takes the stencil of its two strike and its two tenor neighbours
    "nan_hole": _case(_with(_flat(3, 5), c1_2=NAN), K5, [0.1, 0.2, 0.3], [100.0],
                      [[NOST, 0, NOST, 0, NOST], [NOST, NOST, DEAD, NOST, NOST], [NOST, 0, NOST, 0, NOST]], [4, 0, 0, 4]),
    # A1: every kind of invalid vol (0, negative, inf); each is DEAD and its strike neighbour loses the stencil, but an
    # edge node that is valid (flag 4) still serves as a TENOR neighbour
    "bad_values": _case(_with(_flat(3, 5), c0_0=0.0, c1_0=-0.5, c2_4=INF), K5, [0.1, 0.2, 0.3], [100.0],
                        [[DEAD, NOST, 0, 0, NOST], [DEAD, NOST, 0, 0, NOST], [NOST, 0, 0, NOST, DEAD]], [6, 0, 0, 6]),
    # A1: an invalid strike kills its column and the stencil of both neighbouring columns
    "bad_strike": _case(_flat(2, 7), [70.0, 80.0, 90.0, -100.0, 110.0, 120.0, 130.0], [0.1, 0.3], [100.0],
                        [[NOST, 0, NOST, DEAD, NOST, 0, NOST]] * 2, [4, 0, 0, 4]),
    # A1/A4: dead rows.  Snapshot 0 has no spot: all DEAD, counts 0, worst NaN.  The tenor 0.0 kills row 1 everywhere: row 0
    # then has no tenor neighbour at all (NO_STENCIL), row 2 falls back to the 2-point difference towards row 3
    "dead_rows": _case(np.full((3, 4, 5), 0.5), K5, [0.1, 0.0, 0.3, 0.4], [NAN, 100.0, 100.0],
                       [[[DEAD] * 5] * 4] + [[EDGE5, [DEAD] * 5, ROW5, ROW5]] * 2, [[0, 0, 0, 0], [6, 0, 0, 6], [6, 0, 0, 6]]),
    # A3: a strike pair that does not increase (equal in snapshot 0, decreasing in snapshot 1) takes the stencil of both
    # of its nodes: the spacing between them is not > 0
    "non_increasing_strikes": _case(np.full((2, 2, 7), 0.5), [[80.0, 90.0, 90.0, 110.0, 120.0, 130.0, 140.0],
                                                              [80.0, 100.0, 90.0, 110.0, 120.0, 130.0, 140.0]], [0.1, 0.3],
                                    [100.0, 100.0], [[[NOST, NOST, NOST, 0, 0, 0, NOST]] * 2] * 2, [[6, 0, 0, 6]] * 2),
    # A4: tenors 0.2, 0.1, 0.3, 0.3.  Row 0 has no neighbour below and 0.1 is not above 0.2: no stencil.  Row 1 looks up only
    # (0.2 is not below 0.1), row 2 looks down only (0.3 is not above 0.3), row 3 has nothing below 0.3 and nothing above
    "tenor_two_point": _case(_flat(4, 5), K5, [0.2, 0.1, 0.3, 0.3], [100.0], [EDGE5, ROW5, ROW5, EDGE5], [6, 0, 0, 6]),
    # A4 with two rows only: each differences towards the other
    "two_rows": _case(_flat(2, 5), K5, [0.1, 0.3], [100.0], [ROW5, ROW5], [6, 0, 0, 6], rate=0.03),
}


def shared_and_spelled():
    """The same three surfaces once with shared grids and once with the grids spelled out per snapshot."""
    c = smooth(3, 3, 5, 11, per_kq=False, per_tq=False)
    return c, dict(c, Kq=np.tile(c["Kq"], (3, 1)), Tq=np.tile(c["Tq"], (3, 1)))


def flat_surface(sigma, S, rate, mK=67, Tq=(1 / 365, 7 / 365, 0.04, 0.25)):
    Tq = np.asarray(Tq, np.float64)
    Kq = S * np.exp(np.linspace(-0.5, 0.5, mK))
    return dict(vol=np.full((1, len(Tq), mK), sigma), Kq=Kq, Tq=Tq, spot=np.array([S]), rate=rate)


def parabola_surface(a, b, c, S, rate=0.03, mK=41, Tq=(0.02, 0.05, 0.11, 0.25, 0.4)):
    """w = tau (a + b x + c x^2), x = ln(k / S): every stencil of rules A3 / A4 is exact on it."""
    Tq = np.asarray(Tq, np.float64)
    Kq = S * np.exp(np.linspace(-0.4, 0.4, mK) + 0.003 * np.sin(np.arange(mK)))        # uneven spacing
    x = np.log(Kq / S)
    vol = np.sqrt(a + b * x + c * x * x)[None, None, :] * np.ones((1, len(Tq), 1))
    return dict(vol=vol, Kq=Kq, Tq=Tq, spot=np.array([S]), rate=rate, abc=(a, b, c))


def smooth(B, mT, mK, seed, per_kq=True, per_tq=False, holes=0.0, rate=0.0, noise=0.0, width=0.5):
    """Skewed parabolas in log-moneyness x = ln(k / S): sigma(x) = s0 + a x + c x^2, between 0.3 and 0.9 over |x| <= width
    without clipping; s0, a, c per snapshot with a small drift from tenor to tenor; tenors from 1/365 to 0.25 years; strikes
    S exp(x) with x evenly spaced (jittered per snapshot when the grid is per snapshot).  holes: the share of nodes made
    invalid (NaN / 0 / negative / inf vols).  noise: relative noise on every vol (0 = none; > 0 kinks the smiles, so
    butterfly and calendar flags appear)."""
    r = np.random.default_rng(seed)
    spot = r.uniform(50.0, 30000.0, B)
    x = np.linspace(-width, width, mK)
    if per_kq:
        xs = x[None, :] + r.uniform(-0.2, 0.2, (B, mK)) * (2 * width / (mK - 1))
        Kq = spot[:, None] * np.exp(xs)
    else:
        spot = spot[0] * np.exp(r.uniform(-0.05, 0.05, B))               # one shared grid: the spots stay near it
        Kq = spot[0] * np.exp(x)
        xs = np.log(Kq[None, :] / spot[:, None])
    if per_tq:
        Tq = np.sort(r.uniform(1.0 / 365.0, 0.25, (B, mT)), axis=1)
    else:
        Tq = np.geomspace(1.0 / 365.0, 0.25, mT)
    s0 = r.uniform(0.4, 0.6, (B, 1, 1)) + r.uniform(-0.01, 0.01, (B, mT, 1))
    a = r.uniform(-0.15, 0.05, (B, 1, 1)) + r.uniform(-0.01, 0.01, (B, mT, 1))
    c = r.uniform(0.0, 0.25, (B, 1, 1)) + r.uniform(0.0, 0.02, (B, mT, 1))
    xx = xs[:, None, :]
    vol = s0 + a * xx + c * xx * xx
    if noise > 0:
        vol = vol * (1.0 + noise * r.standard_normal(vol.shape))
    assert vol.min() > 0.3 - 4 * noise and vol.max() < 0.9 + 4 * noise
    if holes > 0:
        bad = r.random(vol.shape) < holes
        vol = np.where(bad, r.choice([NAN, 0.0, -0.4, INF], vol.shape), vol)
    return dict(vol=np.ascontiguousarray(vol), Kq=np.ascontiguousarray(Kq), Tq=np.ascontiguousarray(Tq), spot=spot, rate=rate)


# every mK around the 64-strike chunk x every mT around the strip lengths x every B around the snapshots-per-workgroup
# packing; grids shared / per snapshot, the rate and the holes alternate over the list (holes only where the surface is
# large enough for 90 % of its interior to stay evaluated)
GPU_SHAPES = []
for n, (mK, mT, B) in enumerate(itertools.product((3, 5, 63, 64, 65, 130), (2, 3, 16, 17), (1, 7, 33))):
    GPU_SHAPES.append(dict(B=B, mT=mT, mK=mK, seed=500 + n, per_kq=bool(n & 1), per_tq=bool((n >> 1) & 1),
                           rate=0.03 if (n // 3) & 1 else 0.0, holes=0.01 if (n % 5 == 2 and B * mT * mK >= 2000) else 0.0))
BIG = dict(B=512, mT=16, mK=64, seed=499, per_kq=True, per_tq=False, rate=0.03, holes=0.01)
ROUGH = dict(B=33, mT=16, mK=65, seed=498, per_kq=True, per_tq=True, rate=0.03, noise=0.03)
# enough snapshots for whole-snapshot strips (one wavefront per snapshot) on any device up to 256 CUs
WHOLE = dict(B=4200, mT=16, mK=3, seed=497, per_kq=True, per_tq=False, rate=0.03)


def shape_id(s):
    return f"B{s['B']}-mT{s['mT']}-mK{s['mK']}-{'k' if s['per_kq'] else 's'}{'t' if s['per_tq'] else 's'}-r{s['rate']}-h{s['holes']}"
