"""Hand-built micro cases, one per rule and flag of M1-M7, the flat-surface anchor and the seeded
generators of the GPU shapes.  TEST INFRASTRUCTURE ONLY.  A micro case is a dict(vol [B,mT,mK], Kq, Tq, spot, rate,
horizons, min_mass) plus what must come out, worked out by hand from the rules: `flags` [B,mT] and `index_flags` [B,nH]."""
import numpy as np

NAN, INF = float("nan"), float("inf")
ONE, TRUNC, HOLES, DEAD, NOBR = 1, 2, 4, 8, 16
EPS = float(np.finfo(np.float64).eps)

# Rounding level of the float64 restatement against the same rules in mpmath at 50 digits, in units of eps x raw_scale: the
# largest ratio over every input the GPU tests use (MICRO, EDGE and SHAPES below) was 0.30 (L), 0.24 (V), 0.28 (W) and
# 0.34 (X), recorded here rounded up (test_moments.py::test_rounding_level asserts that it stays below R_CPU).  The GPU
# tests allow C = 8 x R_CPU.
R_CPU = 0.5
C_GPU = 8.0 * R_CPU

# Flat-surface anchor (vol 0.6, rate 0.01, log-uniform grid over +-8 standard deviations), measured on the restatement
# with 64 nodes at tau = 2/365, 30/365, 1: L / w - 1, |skew|, |kurt - 3|.  The test holds each to its figure plus 20 %.
ANCHOR_TAUS = (2.0 / 365.0, 30.0 / 365.0, 1.0)
ANCHOR_L = (0.009950, 0.010173, 0.012851)
ANCHOR_SKEW = (0.001758, 0.006827, 0.032856)
ANCHOR_KURT = (0.066402, 0.064601, 0.031644)


def _case(vol, Kq, Tq, spot, flags, index_flags, rate=0.0, horizons=(30.0 / 365.0,), min_mass=0.99):
    vol = np.asarray(vol, np.float64)
    if vol.ndim == 2:
        vol = vol[None]
    B, mT, _ = vol.shape
    return dict(vol=vol, Kq=np.asarray(Kq, np.float64), Tq=np.asarray(Tq, np.float64), spot=np.asarray(spot, np.float64),
                rate=rate, horizons=tuple(horizons), min_mass=min_mass, flags=np.asarray(flags, np.int32).reshape(B, mT),
                index_flags=np.asarray(index_flags, np.int32).reshape(B, len(horizons)))


# 41 strikes from 40 to 250 around the spot 100: at vol 0.5 and tenors of 20 / 40 days they cover all but 1e-12 of the
# lognormal mass; K9 (80 .. 120) covers far less than 99 % of it
KW = np.concatenate([np.linspace(40.0, 100.0, 21), np.linspace(105.0, 250.0, 20)])
K9 = np.linspace(80.0, 120.0, 9)
T2 = [20.0 / 365.0, 40.0 / 365.0]


def _flat(mT, mK, sigma=0.5):
    return np.full((mT, mK), sigma)


def _with(a, **cells):
    a = np.array(a, np.float64)
    for key, v in cells.items():
        j, i = (int(c) for c in key[1:].split("_"))
        a[j, i] = v
    return a


MICRO = {
    # M4: rate 0, so F = spot = 100 = node 20 exactly: no split, not one-sided; wide grid: clean rows and a clean index
    "forward_on_a_node": _case(_flat(2, 41), KW, T2, [100.0], [0, 0], [0]),
    # M4: F = 102 lies strictly between the nodes 100 and 105: the segment is split there
    "forward_between_nodes": _case(_flat(2, 41), KW, T2, [102.0], [0, 0], [0]),
    # M1 / M4: the node at 100 is a hole in row 0 (NaN) and in row 1 (vol 0): 97 and 105 pair up across it and F = 101
    # splits that segment
    "forward_across_a_hole": _case(_with(_flat(2, 41), c0_20=NAN, c1_20=0.0), KW, T2, [101.0], [HOLES, HOLES], [HOLES]),
    # M4: F below the first / above the last valid strike: ONE_SIDED, and the narrow grid is TRUNCATED as well
    "forward_below_the_grid": _case(_flat(2, 9), K9, T2, [75.0], [ONE | TRUNC] * 2, [ONE | TRUNC]),
    "forward_above_the_grid": _case(_flat(2, 9), K9, T2, [125.0], [ONE | TRUNC] * 2, [ONE | TRUNC]),
    # M4: F equal to the first valid strike is inside the range: no split, not one-sided
    "forward_on_the_first_node": _case(_flat(2, 9), K9, T2, [80.0], [TRUNC] * 2, [TRUNC]),
    # M1: one valid node in row 0, none in row 1 (all kinds of invalid vol), snapshot 1 has no spot, snapshot 2 a zero tenor
    "too_few_nodes": _case([_with(np.full((2, 9), NAN), c0_4=0.5, c1_0=0.0, c1_1=-0.5, c1_2=INF), _flat(2, 9), _flat(2, 9)],
                           K9, [[20.0 / 365.0, 40.0 / 365.0]] * 2 + [[0.0, 40.0 / 365.0]], [100.0, NAN, 100.0],
                           [[DEAD, DEAD], [DEAD, DEAD], [DEAD, TRUNC]], [[NOBR], [NOBR], [NOBR]]),
    # M1: valid strikes equal (snapshot 0) or descending (snapshot 1) kill the rows; in snapshot 2 the offending strike sits
    # under a hole of row 0 only, so row 0 lives (HOLES) and row 1 is dead
    "non_ascending_strikes": _case([_flat(2, 9), _flat(2, 9), _with(_flat(2, 9), c0_3=NAN)],
                                   [[80, 85, 90, 90, 100, 105, 110, 115, 120], [80, 85, 95, 90, 100, 105, 110, 115, 120],
                                    [80, 85, 90, 89, 100, 105, 110, 115, 120]], T2, [100.0] * 3,
                                   [[DEAD, DEAD], [DEAD, DEAD], [HOLES | TRUNC, DEAD]], [[NOBR]] * 3),
    # M7: the dead row 1 (tenor 25 days, no valid vol) is skipped: rows 0 and 2 (20 and 40 days) bracket 30 days; HOLES of
    # row 2 reaches the index through the OR
    "dead_row_between_live_rows": _case(_with(np.vstack([_flat(1, 41), np.full((1, 41), NAN), _flat(1, 41)]), c2_5=NAN), KW,
                                        [20.0 / 365.0, 25.0 / 365.0, 40.0 / 365.0], [100.0], [0, DEAD, HOLES], [HOLES]),
    # M7: horizons on the first, a middle and the last tenor, and one inside
    "horizon_on_a_tenor": _case(_flat(3, 41), KW, [20.0 / 365.0, 30.0 / 365.0, 40.0 / 365.0], [100.0], [0, 0, 0], [0, 0, 0, 0],
                                horizons=(20.0 / 365.0, 30.0 / 365.0, 40.0 / 365.0, 33.0 / 365.0)),
    # M7: horizons below and above every tenor, tenors that do not ascend (40, 20 days: no pair with tau_j < tau_j')
    "horizon_outside_the_tenors": _case([_flat(2, 41), _flat(2, 41)], KW, [T2, T2[::-1]], [100.0, 100.0], [[0, 0], [0, 0]],
                                        [[NOBR, NOBR, 0], [NOBR, NOBR, NOBR]], horizons=(10.0 / 365.0, 50.0 / 365.0, 30.0 / 365.0)),
    # M6: min_mass = 0 switches TRUNCATED off on the narrow grid; the default flags it
    "min_mass_zero": _case(_flat(2, 9), K9, T2, [100.0], [0, 0], [0], min_mass=0.0),
    "min_mass_default": _case(_flat(2, 9), K9, T2, [100.0], [TRUNC, TRUNC], [TRUNC]),
    # rate != 0 moves the forward off the spot: F = 100 exp(0.05 tau) lies between 100 and 105
    "rate_moves_the_forward": _case(_flat(2, 41), KW, T2, [100.0], [0, 0], [0], rate=0.05),
}


def flat_anchor(n, tau, sigma=0.6, rate=0.01, S=100.0, width=8.0):
    """n log-uniform strikes over +- width standard deviations around the forward."""
    sd = sigma * np.sqrt(tau)
    F = S * np.exp(rate * tau)
    Kq = F * np.exp(np.linspace(-width * sd, width * sd, n))
    return dict(vol=np.full((1, 1, n), sigma), Kq=Kq, Tq=np.array([tau]), spot=np.array([S]), rate=rate, horizons=(), min_mass=0.99)


def smooth(B, mT, mK, seed, per_kq=True, per_tq=False, holes=0.1, rate=0.0, width=4.0, horizons=(30.0 / 365.0,), min_mass=0.99):
    """Skewed smiles sigma(x) = s0 + a x + c x^2 in x = ln(k / S) between about 0.2 and 1.1, s0, a, c per snapshot with a
    small drift from tenor to tenor; tenors from 5 to 90 days; strikes S exp(x) with x spread evenly over +- width standard
    deviations of the LONGEST tenor at vol 0.5 (jittered per snapshot when the grid is per snapshot), so short tenors see a
    wide grid and long ones a truncated one.  holes: the share of nodes made invalid (NaN / 0 / negative / inf vols)."""
    r = np.random.default_rng(seed)
    spot = r.uniform(50.0, 30000.0, B)
    if per_tq:
        Tq = np.sort(r.uniform(5.0 / 365.0, 90.0 / 365.0, (B, mT)), axis=1)
    else:
        Tq = np.geomspace(5.0 / 365.0, 90.0 / 365.0, mT) if mT > 1 else np.array([30.0 / 365.0])
    half = width * 0.5 * np.sqrt(90.0 / 365.0) * (0.35 if mK < 8 else 1.0)
    x = np.linspace(-half, half, mK)
    if per_kq:
        xs = x[None, :] + r.uniform(-0.2, 0.2, (B, mK)) * (2 * half / max(mK - 1, 1))
        Kq = spot[:, None] * np.exp(xs)
    else:
        spot = spot[0] * np.exp(r.uniform(-0.05, 0.05, B))               # one shared grid: the spots stay near it
        Kq = spot[0] * np.exp(x)
        xs = np.log(Kq[None, :] / spot[:, None])
    s0 = r.uniform(0.4, 0.6, (B, 1, 1)) + r.uniform(-0.01, 0.01, (B, mT, 1))
    a = r.uniform(-0.15, 0.05, (B, 1, 1)) + r.uniform(-0.01, 0.01, (B, mT, 1))
    c = r.uniform(0.0, 0.25, (B, 1, 1)) + r.uniform(0.0, 0.02, (B, mT, 1))
    xx = xs[:, None, :]
    vol = s0 + a * xx + c * xx * xx
    assert vol.min() > 0.15 and vol.max() < 1.2
    if holes > 0 and mK > 3:
        bad = r.random(vol.shape) < holes
        vol = np.where(bad, r.choice([NAN, 0.0, -0.4, INF], vol.shape), vol)
    return dict(vol=np.ascontiguousarray(vol), Kq=np.ascontiguousarray(Kq), Tq=np.ascontiguousarray(Tq), spot=spot, rate=rate,
                horizons=tuple(horizons), min_mass=min_mass)


# (B, mT, mK): the smallest legal row; one short of a chunk's worth of anything; one chunk; one node and two chunks and a
# bit into the chunk carry; a batch of more than one workgroup per snapshot count.  Each with shared and per-snapshot grids
# and rate 0 and 0.03 (the largest with per-snapshot grids and rate 0.03 only: its restatement in mpmath is the slow one).
SHAPES = []
for n, (B, mT, mK) in enumerate(((1, 1, 2), (1, 2, 3), (3, 16, 64), (5, 3, 65), (2, 4, 130), (64, 16, 64))):
    for q, (per, rate) in enumerate(((False, 0.0), (True, 0.03), (True, 0.0), (False, 0.03))):
        if B == 64 and q != 1:
            continue
        SHAPES.append(dict(B=B, mT=mT, mK=mK, seed=700 + 4 * n + q, per_kq=per, per_tq=per and mT > 1, rate=rate,
                           holes=0.1 if mK > 3 else 0.0,
                           horizons=(30.0 / 365.0,) if B != 5 else (7.0 / 365.0, 30.0 / 365.0, 60.0 / 365.0)))


def shape_id(s):
    return f"B{s['B']}-mT{s['mT']}-mK{s['mK']}-{'k' if s['per_kq'] else 's'}{'t' if s['per_tq'] else 's'}-r{s['rate']}"


def _edge(spot, holes=(), rate=0.0):
    """mK = 130 strikes 70, 70.5, .. 134.5 (node 63 = 101.5, node 64 = 102), two tenors, flat vol 0.5 with a mild smile."""
    Kq = 70.0 + 0.5 * np.arange(130)
    vol = 0.5 + 0.1 * np.log(Kq / 100.0) ** 2 * np.ones((1, 2, 1))
    for i in holes:
        vol[0, :, i] = NAN
    return dict(vol=vol, Kq=Kq, Tq=np.array(T2), spot=np.array([spot]), rate=rate, horizons=(30.0 / 365.0,), min_mass=0.99)


# rule M4 at the chunk edge of a 130-strike row: the straddling segment is the one carried from chunk 0 into chunk 1
EDGE = {
    "between_63_and_64": (_edge(101.75), 0),
    "hole_at_63": (_edge(101.75, holes=(63,)), HOLES),                # 62 (101.0) and 64 (102.0) bracket F across the edge
    "hole_at_64": (_edge(101.75, holes=(64,)), HOLES),                # 63 (101.5) and 65 (102.5) bracket F
    "holes_at_63_and_64": (_edge(101.75, holes=(63, 64)), HOLES),     # 62 and 65 bracket F
    "forward_on_node_64": (_edge(102.0), 0),                          # first node of chunk 1: no split
    "forward_on_node_63": (_edge(101.5), 0),                          # last node of chunk 0: no split
    "chunk_1_all_holes_but_last": (_edge(120.0, holes=tuple(range(64, 129))), HOLES),   # 63 pairs with 129 across chunk 1
    "between_63_and_64_with_rate": (_edge(101.7, rate=0.03), 0),
}
