"""Hand-built micro cases, one per rule and flag of J1-J8, and the seeded generators of the GPU
shapes.  TEST INFRASTRUCTURE ONLY.  A case is a dict(vol [B,mT,mK], Kq, Tq, spot, rate, and theta0 [B,mT] or raw [B,mT,5]); a
micro case carries besides what must come out, worked out by hand from the rules: `flags` [B,mT] and `sflags` [B] (with
`sfree` [B], the surface bits the rules leave to the search).  Every tolerance constant below has its measured source in
profiles/ssvi/errlog.txt."""
import numpy as np

NAN, INF = float("nan"), float("inf")
RAISED, HOLES, DEAD, BUTTERFLY = 1, 4, 8, 16
EDGE_RHO, EDGE_GAMMA, EDGE_ETA_LOW, SURF_DEAD, AT_BOUND, UNORDERED = 1, 2, 4, 8, 16, 32
EPS = float(np.finfo(np.float64).eps)
S_MIN = -6.931471805599453

# R_CPU[rounds]: the largest |restatement - twin| over every input the GPU tests run (MICRO and SHAPES, at 20 and at 4
# rounds) and TWIN_SEEDS, on the stable snapshots: rho, gamma and s in final grid steps (gamma only where it is identified),
# theta in eps, rmse relative to rmse + RMSE_FLOOR, the fitted vols and the two vol statistics absolute, g_min absolute.
# Measured (profiles/ssvi/errlog.txt), recorded here rounded up: steps 0, theta 0, rmse 8.69e-8, vol 1.11e-15, g_min 0 at 20
# rounds; 0, 0, 7.52e-14, 8.9e-16, 0 at 4.  The GPU tests allow C_GPU x R_CPU.  Every twin run ends on the restatement's own
# grid point, bit for bit, and so with its very slices: the twin says nothing about what another arithmetic does to a grid
# point or to a slice of given parameters.  Three floors from the number format stand in there (never narrower than C_GPU x
# R_CPU): SAME_POINT, the same grid point within 4 eps of the domain's width (lo + i h is rounded differently with a fused
# multiply-add); VOL_EPS x eps x the snapshot's largest fitted vol (phi = eta exp(-gamma L) with |gamma L| up to 6, x = a
# logarithm and a product, the sum of J4: each a few eps relative on w_fit, halved by the square root); G_EPS x eps x g_scale, the
# magnitude of the terms g_min is summed from (x, w' and w_fit carry those few eps each, and g cancels between its terms).
R_CPU = {20: {"steps": 0.0, "theta": 0.0, "rmse": 8.7e-8, "vol": 1.2e-15, "g_min": 0.0},
         4: {"steps": 0.0, "theta": 0.0, "rmse": 7.6e-14, "vol": 9.0e-16, "g_min": 0.0}}
VOL_EPS, G_EPS = 16.0, 32.0
RMSE_FLOOR = 1e-9
C_GPU = 8.0
TWIN_SEEDS = (1, 2, 3)
UNSTABLE_STEPS = 100.0       # twin runs further apart than this in rho, gamma or s have flipped basins
UNSTABLE_SHARE = 0.02
SAME_POINT = 4 * EPS         # rounds = 4: the same grid point, within this share of the domain's width

# Recovery of noiseless SSVI surfaces by the restatement at 20 rounds over the exact snapshots of SHAPES with an identified
# gamma: the largest |(rho, gamma, s) - generating| was 7.4e-3, 1.19e-1, 1.11e-1 and the largest relative rmse 1.65e-1
# (errlog.txt): a box of J7 shrinks to 2/5 whether or not the optimum is still inside, and on these surfaces (theta over a
# factor of 50, strikes to +- 1 in log-moneyness) gamma and s trade off along a narrow curved valley that the early, coarse
# rounds step out of.  The 1e-7 of the sketch that preceded the rules is not reached.  The test allows 8 x the figures.
RECOVERY = {"point": 8 * np.array([7.4e-3, 1.19e-1, 1.11e-1]), "rmse": 8 * 1.65e-1}
# Quality against the best of several bounded scipy.optimize.least_squares starts on the same objective with theta fixed,
# the generating point and the search's own end among the starts: the worst SSE / SSE_scipy - 1 over the noisy snapshots of
# two shapes was 0.416 (errlog.txt; the other snapshot reached 1.2e-12).  The test allows 8 x.
QUALITY_MARGIN = 8 * 0.416
DOMAIN_WIDTH = np.array([2.0 * (1.0 - 2.0 ** -10), 1.0, -S_MIN])                       # rho, gamma, s


def ssvi_w(x, th, rho, phi):
    return 0.5 * th * (1.0 + rho * phi * x + np.sqrt((phi * x + rho) ** 2 + (1.0 - rho * rho)))


def eta_max(th, rho, gam):
    A = 1.0 + abs(rho)
    e = th ** -gam
    return float(np.min(np.minimum(4.0 / (th * e * A), 2.0 / (np.sqrt(th) * e * np.sqrt(A)))))


def raw_of(th, rho, phi):
    """J8: the raw-SVI form (a, b, rho, m, sigma) of SSVI slices."""
    omr = 1.0 - rho * rho
    return np.stack([th * omr / 2.0, th * phi / 2.0, rho + 0.0 * th, -rho / phi, np.sqrt(omr) / phi], axis=-1)


# ---- micro cases: 9 strikes round the spot 100, 3 tenors
K9 = 100.0 * np.exp(np.linspace(-0.4, 0.4, 9))
X9 = np.log(K9 / 100.0)
T3 = np.array([0.1, 0.25, 0.5])
TH3 = np.array([0.02, 0.05, 0.1])
GEN = dict(rho=-0.4, gam=0.4, s=np.log(0.5))


def _surface(th, tq, rho, gam, s, x=X9):
    """vol [mT, mK] of the SSVI surface (rho, gam, s) on theta th; eta_max is taken over th's running maximum."""
    thm = np.maximum.accumulate(th)
    eta = np.exp(s) * eta_max(thm, rho, gam)
    phi = eta * thm ** -gam
    return np.sqrt(ssvi_w(x[None, :], thm[:, None], rho, phi[:, None]) / tq[:, None])


def _case(vol, Tq, spot, theta0, flags, sflags, sfree=0, Kq=K9, raw=None, rate=0.0):
    vol = np.asarray(vol, np.float64)
    if vol.ndim == 2:
        vol = vol[None]
    B, mT, _ = vol.shape
    c = dict(vol=vol, Kq=np.asarray(Kq, np.float64), Tq=np.asarray(Tq, np.float64), spot=np.asarray(spot, np.float64).reshape(B),
             rate=rate, flags=np.asarray(flags, np.int32).reshape(B, mT), sflags=np.asarray(sflags, np.int32).reshape(B),
             sfree=np.broadcast_to(np.asarray(sfree, np.int32), (B,)).copy())
    if raw is None:
        c["theta0"] = np.asarray(theta0, np.float64).reshape(B, mT)
    else:
        c["raw"] = np.asarray(raw, np.float64).reshape(B, mT, 5)
    return c


def _cells(a, cells):
    a = np.array(a, np.float64)
    for (j, i), v in cells.items():
        a[j, i] = v
    return a


_V3 = _surface(TH3, T3, **GEN)
_FOUR = np.full((3, 9), NAN)
_FOUR[0, 1], _FOUR[0, 4], _FOUR[1, 2], _FOUR[2, 7] = _V3[0, 1], _V3[0, 4], _V3[1, 2], _V3[2, 7]
_TH_DOWN = np.array([0.02, 0.05, 0.04])
_PHI3 = np.exp(GEN["s"]) * eta_max(TH3, GEN["rho"], GEN["gam"]) * TH3 ** -GEN["gam"]
_RAW3 = raw_of(TH3, GEN["rho"], _PHI3)
MICRO = {
    # J1: a dead row in the middle (NaN tenor): the other two are fitted, the dead one is DEAD alone
    "dead_row_in_the_middle": _case(_V3, [0.1, NAN, 0.5], [100.0], TH3, [0, DEAD, 0], [0]),
    # J1: 4 valid nodes on the whole snapshot
    "four_valid_nodes": _case(_FOUR, T3, [100.0], TH3, [DEAD, DEAD, DEAD], [SURF_DEAD]),
    # J1 / T2: live tenors out of order (and, snapshot 1, equal)
    "out_of_order_tenors": _case([_V3, _V3], [[0.1, 0.5, 0.25], [0.1, 0.25, 0.25]], [100.0, 100.0], [TH3, TH3],
                                 [[DEAD] * 3, [DEAD] * 3], [UNORDERED, UNORDERED]),
    # J3: a decreasing theta0: the last row is raised to its neighbour's theta and repeats its slice bit for bit
    "decreasing_theta0": _case(_surface(_TH_DOWN, T3, **GEN), T3, [100.0], _TH_DOWN, [0, 0, RAISED], [0]),
    # J8: a row with theta0 but no valid node: real theta and params, NaN fit
    "row_without_nodes": _case(_cells(_V3, {(1, i): NAN for i in range(9)}), T3, [100.0], TH3, [0, 0, 0], [0]),
    # J1: a NaN spot (snapshot 0) next to a good snapshot
    "nan_spot": _case([_V3, _V3], T3, [NAN, 100.0], [TH3, TH3], [[DEAD] * 3, [0, 0, 0]], [SURF_DEAD, 0]),
    # J1: `raw` with a dead slice (sigma = 0): the row is DEAD, the other two carry theta0 = w(0)
    "raw_with_a_dead_slice": _case(_V3, T3, [100.0], None, [0, DEAD, 0], [0], raw=_cells(_RAW3, {(1, 4): 0.0})),
    # J5: a surface generated at s = 0 has its optimum ON the border with a zero gradient there.  A box of J7 leaves out its
    # own centre, so rho and gamma end a little off the generating point and s gives way by about 1e-4 to make up for it:
    # whether the final s is within 2^-20 of the border is the search's to decide (measured: it is not).  The by-hand case is
    # therefore the surface generated BEYOND the bound, at s = ln 1.25, whose constrained optimum sits on the border firmly
    "generated_at_the_bound": _case(_surface(TH3, T3, -0.4, 0.4, 0.0), T3, [100.0], TH3, [0, 0, 0], [0], sfree=AT_BOUND),
    "at_the_bound": _case(_surface(TH3, T3, -0.4, 0.4, np.log(1.25)), T3, [100.0], TH3, [0, 0, 0], [AT_BOUND]),
    # V1: a hole between valid nodes is skipped and flagged
    "a_hole": _case(_cells(_V3, {(0, 3): NAN, (2, 0): 0.0}), T3, [100.0], TH3, [HOLES, 0, 0], [0]),
}


def batch(B, mT, mK, seed, per_kq=True, per_tq=False, holes=0.1, rate=0.0, noise=0.002, exact_every=2, use_raw=False):
    """SSVI surfaces: per snapshot its own (rho, gamma, s) well inside the domain and an increasing theta on geometric
    tenors; snapshot b is exact when b % exact_every == 0, else its vols carry normal noise of `noise` (20 bp).  With
    mT >= 3 one row per snapshot gets a theta0 below its neighbour's (RAISED), and about 3 % of the rows a NaN theta0 (DEAD).
    holes: the share of nodes made invalid.  use_raw: theta0 travels as raw slices (the generating ones; a dead one for a
    NaN theta0).  Returns the case and gen = dict(point [B,3] (rho, gamma, s), eta [B], exact [B], theta [B,mT])."""
    r = np.random.default_rng(seed)
    spot = r.uniform(50.0, 30000.0, B)
    Tq = np.geomspace(7.0 / 365.0, 1.0, mT) if mT > 1 else np.array([30.0 / 365.0])
    if per_tq:
        Tq = Tq[None, :] * (1.0 + r.uniform(-0.2, 0.2, (B, mT)) * (min(0.5 * (Tq[1] / Tq[0] - 1.0), 0.5) if mT > 1 else 0.5))
    TT = np.broadcast_to(Tq, (B, mT))
    half = 2.0 * 0.5 * np.sqrt(TT.max())
    x = np.linspace(-half, half, mK) if mK > 1 else np.zeros(1)
    if per_kq:
        xs = x[None, :] + r.uniform(-0.2, 0.2, (B, mK)) * (2 * half / max(mK - 1, 1))
        Kq = spot[:, None] * np.exp(xs)
    else:
        spot = spot[0] * np.exp(r.uniform(-0.05, 0.05, B))
        Kq = spot[0] * np.exp(x)
        xs = np.log(Kq[None, :] / spot[:, None])
    xx = xs[:, None, :] - rate * TT[:, :, None]
    th = (r.uniform(0.4, 0.6, (B, 1)) ** 2) * TT * np.cumprod(r.uniform(1.0, 1.05, (B, mT)), axis=1)
    th0 = th.copy()
    if mT >= 3:
        j = r.integers(1, mT, B)
        th0[np.arange(B), j] = 0.9 * th0[np.arange(B), j - 1]
    dead = r.random((B, mT)) < 0.03 if mT >= 13 else np.zeros((B, mT), bool)
    th0 = np.where(dead, NAN, th0)
    point = np.stack([r.uniform(-0.7, 0.3, B), r.uniform(0.2, 0.7, B), np.log(r.uniform(0.2, 0.9, B))], axis=1)
    eta, clean, thm = np.zeros(B), np.zeros((B, mT, mK)), np.zeros((B, mT))
    for b in range(B):
        lv = ~dead[b]
        t = np.full(mT, NAN)
        t[lv] = np.maximum.accumulate(th0[b][lv])
        thm[b] = t
        eta[b] = np.exp(point[b, 2]) * eta_max(t[lv], point[b, 0], point[b, 1])
        phi = eta[b] * t ** -point[b, 1]
        clean[b] = np.sqrt(ssvi_w(xx[b], t[:, None], point[b, 0], phi[:, None]) / TT[b][:, None])
    exact = (np.arange(B) % exact_every) == 0
    vol = np.where(exact[:, None, None], clean, clean + r.normal(0.0, noise, clean.shape))
    vol = np.where(dead[:, :, None], 0.5, vol)                                         # a dead row still holds quotes
    assert np.nanmin(vol) > 0.05 and np.nanmax(vol) < 20.0
    if holes > 0:
        bad = r.random(vol.shape) < holes
        vol = np.where(bad, r.choice([NAN, 0.0, -0.4, INF], vol.shape), vol)
    case = dict(vol=np.ascontiguousarray(vol), Kq=np.ascontiguousarray(Kq), Tq=np.ascontiguousarray(Tq), spot=spot, rate=rate)
    if use_raw:
        # a raw slice whose w(0) is the wanted theta0: the SSVI form at phi = 1 (w(0) = theta exactly up to rounding is not
        # needed: theta0 is DEFINED as w(0) of the slice)
        raw = raw_of(np.where(dead, 1.0, th0), -0.3, 1.0 + 0.0 * th0)
        raw[dead] = NAN
        case["raw"] = np.ascontiguousarray(raw)
    else:
        case["theta0"] = np.ascontiguousarray(th0)
    return case, dict(point=point, eta=eta, exact=exact, theta=thm)


# (B, mT, mK) over B in {1, 3}, mT in {1, 2, 13, 16, 64}, mK in {5, 63, 64, 65, 130}, mT mK <= 3072 (mK <= 48 at mT = 64): the
# smallest snapshot; two rows of one chunk less one; 13 rows of one chunk and one node (dead rows, a raised row); the bench's
# shape; two chunks and a bit; the ballot's 64 tenors.  Shared and per-snapshot grids, theta0 and raw, rate 0 and 0.03.
SHAPES = [
    dict(B=1, mT=1, mK=5, seed=1500, per_kq=False, per_tq=False, rate=0.0, holes=0.0, use_raw=False),
    dict(B=3, mT=2, mK=63, seed=1501, per_kq=True, per_tq=True, rate=0.03, holes=0.1, use_raw=True),
    dict(B=3, mT=13, mK=65, seed=1502, per_kq=False, per_tq=True, rate=0.0, holes=0.1, use_raw=False),
    dict(B=3, mT=16, mK=64, seed=1503, per_kq=True, per_tq=False, rate=0.03, holes=0.1, use_raw=True),
    dict(B=1, mT=2, mK=130, seed=1504, per_kq=False, per_tq=False, rate=0.03, holes=0.1, use_raw=False),
    dict(B=3, mT=64, mK=5, seed=1505, per_kq=True, per_tq=False, rate=0.0, holes=0.0, use_raw=False),
    dict(B=1, mT=64, mK=48, seed=1506, per_kq=False, per_tq=True, rate=0.03, holes=0.1, use_raw=True),
]
STREAM_SHAPE = dict(B=24, mT=16, mK=64, seed=1590, per_kq=True, per_tq=False, rate=0.03, holes=0.1, use_raw=False)


def shape_id(s):
    return (f"B{s['B']}-mT{s['mT']}-mK{s['mK']}-{'k' if s['per_kq'] else 's'}{'t' if s['per_tq'] else 's'}-r{s['rate']}-"
            f"{'raw' if s['use_raw'] else 'th0'}")


def case_args(c):
    return dict(vol=c["vol"], Kq=c["Kq"], Tq=c["Tq"], spot=c["spot"], rate=c["rate"], raw=c.get("raw"), theta0=c.get("theta0"))


def point_of(got, ref):
    """(rho, gamma, s) [B,3] of outputs that carry none (the kernel's): s = ln(eta / eta_max) with J5 on the outputs' own rho,
    gamma and theta (a few eps, against a final step of 4e-8)."""
    import ssvi_ref as R
    if "point" in got:
        return got["point"]
    su, th = got["surface"], got["theta"]
    pt = np.full((su.shape[0], 3), np.nan)
    for b in range(su.shape[0]):
        t = th[b][np.isfinite(th[b])]
        if np.isfinite(su[b, 0]) and len(t):
            em = R.eta_max(np.array([su[b, 0]]), np.array([su[b, 2]]), t, np.log(t), np.sqrt(t))[0]
            pt[b] = su[b, 0], su[b, 2], np.log(su[b, 1] / em)
    return pt


def units(got, ref):
    """Distances of `got` (the kernel, or a twin run) from the restatement `ref` in the units of R_CPU: steps [B] (the
    largest of rho, gamma, s in final grid steps; gamma only where it is identified), theta, rmse, vol, g_min (the largest
    over a snapshot, [B]); NaN where the restatement has no value.  Both must carry `fitted`."""
    B = ref["surface"].shape[0]
    d = np.abs(point_of(got, ref) - ref["point"]) / ref["step"]
    d[~ref["identified"], 1] = 0.0
    with np.errstate(all="ignore"):
        mx = lambda a: np.nanmax(np.where(np.isnan(a), -1.0, a).reshape(B, -1), axis=1)  # noqa: E731
        u = {"steps": np.max(d, axis=1),
             "theta": mx(np.abs(got["theta"] - ref["theta"]) / (EPS * ref["theta"])),
             "rmse": np.abs(got["surface"][:, 3] - ref["surface"][:, 3]) / (ref["surface"][:, 3] + RMSE_FLOOR),
             "vol": np.maximum(mx(np.abs(got["fitted"] - ref["fitted"])), mx(np.abs(got["fit"][..., :2] - ref["fit"][..., :2]))),
             "g_min": mx(np.abs(got["fit"][..., 2] - ref["fit"][..., 2]))}
        u["point_eps"] = np.max(np.abs(point_of(got, ref) - ref["point"]) / (EPS * DOMAIN_WIDTH) * np.where(ref["identified"][:, None], 1.0, [1.0, 0.0, 1.0]), axis=1)
    dead = np.isnan(ref["surface"][:, 0])
    return {k: np.where(dead, np.nan, v) for k, v in u.items()}


def tolerances(ref, rounds):
    """What the GPU tests allow per snapshot [B], in the units of `units`: C_GPU x R_CPU, or the format's floor where wider."""
    B = ref["surface"].shape[0]
    r = R_CPU[rounds]
    with np.errstate(all="ignore"):
        mx = lambda a: np.nanmax(np.where(np.isnan(a), 0.0, a).reshape(B, -1), axis=1)  # noqa: E731
        return {"steps": np.full(B, C_GPU * r["steps"]), "theta": np.full(B, C_GPU * r["theta"]), "rmse": np.full(B, C_GPU * r["rmse"]),
                "vol": np.maximum(C_GPU * r["vol"], VOL_EPS * EPS * mx(ref["fitted"])),
                "g_min": np.maximum(C_GPU * r["g_min"], G_EPS * EPS * mx(ref["g_scale"]))}
