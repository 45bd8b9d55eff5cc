"""Hand-built micro smiles, one per rule D2-D5, and the generator of the dense synthetic smiles.
TEST INFRASTRUCTURE ONLY.  A case is a dict(vol [B,mT,mK], Kq, Tq, spot, deltas, rate) plus what must come out:
`flags` [B,mT,nD] and, where it matters, `bracket` = {(b, j, t): (ia, ib)} node indices of the bracket."""
import numpy as np

NAN, INF = float("nan"), float("inf")
OK, NO_CROSSING, AMBIGUOUS, DEAD = 0, 1, 2, 4
DEFAULT = (-0.10, -0.25, 0.5, 0.25, 0.10)
# 16 targets: seven deltas on both sides, ATM and one more call
WIDE16 = (-0.05, -0.10, -0.15, -0.20, -0.25, -0.30, -0.40, 0.5, 0.45, 0.40, 0.30, 0.25, 0.20, 0.15, 0.10, 0.05)


def _case(vol, Kq, Tq, spot, deltas, flags, rate=0.0, bracket=None):
    vol = np.asarray(vol, np.float64)
    if vol.ndim == 1:
        vol = vol[None, None, :]
    elif vol.ndim == 2:
        vol = vol[None, :, :]
    return dict(vol=vol, Kq=np.asarray(Kq, np.float64), Tq=np.asarray(Tq, np.float64), spot=np.asarray(spot, np.float64),
                deltas=tuple(deltas), rate=rate, flags=np.asarray(flags, np.int32).reshape(vol.shape[0], vol.shape[1], -1),
                bracket=bracket or {})


K5 = [80.0, 90.0, 100.0, 110.0, 120.0]
# sigma sqrt(tau) = 0.1 at sigma 0.5, tau 0.04: the ATM strike of a flat smile is 100 exp(0.005), inside (100, 110)
CASES = {
    # D4/D5 on the plainest input: flat smile, the ATM bracket is (2, 3)
    "atm_flat": _case([0.5] * 5, K5, [0.04], [100.0], (0.5,), [OK], bracket={(0, 0, 0): (2, 3)}),
    # D2: an invalid node in the middle is skipped, the bracket spans it
    "gap_middle": _case([0.5, 0.5, 0.5, NAN, 0.5], K5, [0.04], [100.0], (0.5,), [OK], bracket={(0, 0, 0): (2, 4)}),
    # D2: every kind of invalid node (vol 0, negative, inf, NaN; strike 0 / negative) at both ends and between
    "gap_ends": _case([0.0, 0.5, 0.5, -0.5, 0.5, 0.5, INF], [70.0, 80.0, 100.0, 102.0, 110.0, 0.0, 130.0], [0.04], [100.0], (0.5,),
                      [OK], bracket={(0, 0, 0): (2, 4)}),
    "gap_bad_strikes": _case([0.5] * 5, [-80.0, 90.0, 100.0, NAN, 120.0], [0.04], [100.0], (0.5, -0.25), [OK, OK],
                             bracket={(0, 0, 0): (2, 4), (0, 0, 1): (1, 2)}),
    # D2: dead rows -- spot (NaN, 0, negative, inf), tenor (0, NaN, negative, inf), fewer than two valid nodes
    "dead_spot": _case(np.full((4, 1, 5), 0.5), K5, [0.04], [NAN, 0.0, -100.0, INF], DEFAULT, np.full((4, 1, 5), DEAD)),
    "dead_tenor": _case(np.full((1, 5, 5), 0.5), K5, [0.0, NAN, -0.04, INF, 0.04], [100.0], (0.5,), [DEAD, DEAD, DEAD, DEAD, OK]),
    "dead_nodes": _case([[NAN, 0.5, NAN, 0.0, -1.0], [NAN] * 5, [0.5, NAN, NAN, NAN, 0.5]], K5, [0.04, 0.04, 0.04], [100.0], (0.5,),
                        [DEAD, DEAD, OK], bracket={(0, 2, 0): (0, 4)}),
    # D4: no crossing -- every strike above the target (h < 0 everywhere), every strike below it (h >= 0 everywhere)
    "no_crossing_left": _case([0.5] * 5, K5, [0.04], [50.0], DEFAULT, [NO_CROSSING] * 5),
    "no_crossing_right": _case([0.5] * 5, K5, [0.04], [200.0], DEFAULT, [NO_CROSSING] * 5),
    # D4: an UPWARD crossing alone is no bracket (h < 0 then h >= 0: the vols make d1 rise with the strike)
    "upward_only": _case([0.05, 3.0], [101.0, 102.0], [0.04], [100.0], (0.25,), [NO_CROSSING]),
    # D4: two downward crossings -- h at the -0.16 target is +, -, +, - : brackets (0,1) and (2,3), the first is used
    "ambiguous": _case([0.5, 1.5, 0.15, 0.5], [80.0, 90.0, 95.0, 110.0], [0.04], [100.0], (-0.16,), [AMBIGUOUS],
                       bracket={(0, 0, 0): (0, 1)}),
    # D3: a put delta d means the call delta 1 + d -- both targets give the same numbers
    "put_call_mapping": _case([0.6, 0.55, 0.5, 0.52, 0.56], K5, [0.04], [100.0], (-0.25, 0.75), [OK, OK],
                              bracket={(0, 0, 0): (1, 2), (0, 0, 1): (1, 2)}),
    # the default targets on a skewed smile with a rate: five different brackets in strike order
    "default_targets": _case([0.62, 0.55, 0.50, 0.47, 0.46, 0.47, 0.50, 0.55, 0.62],
                             [70.0, 80.0, 90.0, 95.0, 100.0, 105.0, 110.0, 120.0, 130.0], [0.04], [100.0], DEFAULT, [OK] * 5, rate=0.03),
}


def per_snapshot_pair():
    """The same three smiles once with shared grids and once with the grids spelled out per snapshot (D1)."""
    vol = np.array([[[0.6, 0.55, 0.5, 0.52, 0.56], [0.5, 0.5, 0.5, 0.5, 0.5]]] * 3)
    Kq, Tq, spot = np.array(K5), np.array([0.02, 0.04]), np.array([100.0, 100.0, 100.0])
    shared = dict(vol=vol, Kq=Kq, Tq=Tq, spot=spot, deltas=DEFAULT, rate=0.0)
    spelled = dict(shared, Kq=np.tile(Kq, (3, 1)), Tq=np.tile(Tq, (3, 1)))
    return shared, spelled


def dense(B, mT, mK, seed, per_kq=True, per_tq=False, holes=0.0, width=1.2):
    """Skewed parabolas in log-moneyness x = ln(k / S): sigma(x) = s0 + a x + c x^2 clipped to [0.3, 0.9], tenors from
    1/365 to 0.25 years, strikes S exp(x) with x evenly spaced over [-width, width] (jittered per snapshot when the grid
    is per snapshot).  holes: the share of nodes made invalid (NaN / 0 / negative / inf vols)."""
    r = np.random.default_rng(seed)
    spot = r.uniform(50.0, 30000.0, B)
    x = np.linspace(-width, width, mK)
    if per_kq:
        jit = r.uniform(-0.2, 0.2, (B, mK)) * (2 * width / max(mK - 1, 1))
        xs = x[None, :] + jit
        Kq = spot[:, None] * np.exp(xs)
    else:
        spot = spot[0] * np.exp(r.uniform(-0.05, 0.05, B))               # one shared grid: the spots stay near it
        Kq = spot[0] * np.exp(x)
        xs = np.log(Kq[None, :] / spot[:, None])
    if per_tq:
        Tq = np.sort(r.uniform(1.0 / 365.0, 0.25, (B, mT)), axis=1)
        tau = Tq
    else:
        Tq = np.geomspace(1.0 / 365.0, 0.25, mT) if mT > 1 else np.array([0.04])
        tau = np.broadcast_to(Tq, (B, mT))
    s0 = r.uniform(0.35, 0.7, (B, mT, 1))
    a = r.uniform(-0.15, 0.05, (B, mT, 1))
    c = r.uniform(0.0, 0.25, (B, mT, 1))
    vol = np.clip(s0 + a * xs[:, None, :] + c * xs[:, None, :] ** 2, 0.3, 0.9) + 0.0 * tau[:, :, None]
    if holes > 0:
        bad = r.random(vol.shape) < holes
        vol = np.where(bad, r.choice([NAN, 0.0, -0.4, INF], vol.shape), vol)
    return dict(vol=np.ascontiguousarray(vol), Kq=np.ascontiguousarray(Kq), Tq=np.ascontiguousarray(Tq), spot=spot, rate=0.0)


def edge_63_64(span_gap: bool):
    """130 nodes, flat smile, the ATM root between nodes 63 and 64: the bracket sits exactly on the edge of the first
    64-node chunk.  span_gap: nodes 62..66 are invalid, so the bracket (61, 67) reaches across the edge."""
    mK, sigma, tau = 130, 0.5, 0.04
    K = 100.0 * np.exp(np.linspace(-0.6, 0.6, mK))
    spot = np.sqrt(K[63] * K[64]) * np.exp(-0.5 * sigma * sigma * tau)     # d1 = 0 at the geometric middle of the two
    vol = np.full((1, 1, mK), sigma)
    if span_gap:
        vol[0, 0, 62:67] = [NAN, 0.0, NAN, -1.0, INF]
    return dict(vol=vol, Kq=K, Tq=np.array([tau]), spot=np.array([spot]), deltas=DEFAULT, rate=0.0,
                bracket={(0, 0, 2): (61, 67) if span_gap else (63, 64)})
