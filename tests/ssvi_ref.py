"""Independent restatement of the SSVI rules J1-J8.  TEST INFRASTRUCTURE ONLY.

Shares no code with iv_interpolation_amd: a snapshot is one flat array of its valid nodes in (tenor, node) order, the 216
candidates of a round are one NumPy axis, and the sum over the nodes runs in plain ascending order (a cumulative sum); there
are no lanes, no chunks and no butterflies.

    restate(vol, Kq, Tq, spot, rate=0.0, raw=None, theta0=None, rounds=0, fitted=True, margins=False) -> dict
        surface [B,4] (rho, eta, gamma, rmse), theta [B,mT], params [B,mT,5], fit [B,mT,3], flags [B,mT] int32, sflags [B]
        int32, fitted [B,mT,mK] (None with fitted=False), and for the tests point [B,3] = (rho, gamma, s) as the search left
        them, step [B,3] = the last round's grid steps, n [B], sse [B], identified [B] (more than one distinct theta: gamma is
        not identified otherwise, see below), g_scale [B,mT] (the magnitude of the terms g_min is summed from)
        margins=True asserts the conditions of the generated batches
    twin(case, seed, rounds) -> restate(...) of the case with vol x (1 + 2^-52 xi), xi standard normal: the stand-in for
        another arithmetic (FMA contraction, another log / exp / sqrt)
    theta0_of_raw(raw, Tq, spot) -> rule J1's theta0 from raw slices
    RefBackend() -> cal_ref.RefBackend (every earlier stage restated) plus ssvi

With a single distinct theta among the live rows phi = exp(s) min(4 / (theta A), 2 / (sqrt(theta A))) whatever gamma is: e_j
cancels between J4 and J5, every gamma ties up to rounding, and gamma and eta are then compared only through the slices."""
import numpy as np

import cal_ref
import dist_ref as DR

RAISED, HOLES, DEAD, BUTTERFLY = 1, 4, 8, 16                                          # IVS_SS_*
EDGE_RHO, EDGE_GAMMA, EDGE_ETA_LOW, SURF_DEAD, AT_BOUND, UNORDERED = 1, 2, 4, 8, 16, 32   # IVS_SF_*
DEFAULT_ROUNDS = 20
EDGE_BAND = 2.0 ** -20
RHO_MAX = 1.0 - 2.0 ** -10
S_MIN = -6.931471805599453                                                             # ln 2^-10
DOM_LO = np.array([-RHO_MAX, 0.0, S_MIN])                                               # rho, gamma, s
DOM_HI = np.array([RHO_MAX, 1.0, 0.0])
_C = np.arange(216)
_IDX = np.stack([_C % 6, (_C // 6) % 6, _C // 36])                                      # candidate 36 i_s + 6 i_gamma + i_rho


def _pos(a):
    return np.isfinite(a) & (a > 0)


def _asc(t):
    """Plain left-to-right sum along the last axis."""
    return np.cumsum(t, axis=-1)[..., -1] if t.shape[-1] else np.zeros(t.shape[:-1])


def theta0_of_raw(raw, Tq, spot):
    P = np.asarray(raw, np.float64)
    B, mT, _ = P.shape
    S = np.broadcast_to(np.asarray(spot, np.float64).reshape(B, 1), (B, mT))
    tau = np.broadcast_to(np.asarray(Tq, np.float64), (B, mT))
    a, b, rho, m, sig = (P[..., q] for q in range(5))
    with np.errstate(all="ignore"):
        dx = 0.0 - m
        w0 = a + b * (rho * dx + np.sqrt(dx * dx + sig * sig))                         # T3 at x = 0
    return np.where(DR.live_rows(P, S, tau), w0, np.nan)


def model(th, phi, rho, x):
    """J4."""
    px = phi * x
    t = px + rho
    return 0.5 * th * (1.0 + rho * px + np.sqrt(t * t + (1.0 - rho * rho)))


def eta_max(rho, gam, th, L, q):
    """J5 for candidates rho, gam [C] on the live rows th, L, q [nl], in tenor order."""
    A = 1.0 + np.abs(rho)
    sA = np.sqrt(A)
    emax = np.full(rho.shape, np.inf)
    for l in range(len(th)):
        e = np.exp(-gam * L[l])
        emax = np.minimum(emax, np.minimum(4.0 / (th[l] * e * A), 2.0 / (q[l] * e * sA)))
    return emax


def objective(rho, gam, s, th, L, q, inv, row, x, w):
    """J4-J6 for candidates [C]: eta [C] and SSE [C] over the nodes x, w [n] whose live row is row [n]."""
    eta = np.exp(s) * eta_max(rho, gam, th, L, q)
    phi = eta[:, None] * np.exp(-gam[:, None] * L[None, :])                            # [C, nl]
    wf = model(th[row][None, :], phi[:, row], rho[:, None], x[None, :])
    r = (wf - w[None, :]) * inv[row][None, :]
    return eta, _asc(r * r)


def search(th, L, q, inv, row, x, w, rounds):
    """J7.  Returns the final point (rho, gamma, s), eta, SSE and the last round's steps."""
    lo, hi = DOM_LO.copy(), DOM_HI.copy()
    for _ in range(rounds):
        h = (hi - lo) / 5.0
        p = lo[:, None] + np.arange(6)[None, :] * h[:, None]
        p[:, 5] = hi
        rho, gam, s = (p[a][_IDX[a]] for a in range(3))
        eta, sse = objective(rho, gam, s, th, L, q, inv, row, x, w)
        best = int(np.argmin(np.where(np.isnan(sse), np.inf, sse)))                   # the first of equals
        pt = np.array([rho[best], gam[best], s[best]])
        lo, hi = np.maximum(DOM_LO, pt - h), np.minimum(DOM_HI, pt + h)
    return pt, eta[best], sse[best], h


def restate(vol, Kq, Tq, spot, rate=0.0, raw=None, theta0=None, rounds=0, fitted=True, margins=False):
    assert (raw is None) != (theta0 is None)
    vol = np.asarray(vol, np.float64)
    B, mT, mK = vol.shape
    assert mT <= 64 and mT * mK <= 3072
    K = np.broadcast_to(np.asarray(Kq, np.float64), (B, mK))
    T = np.broadcast_to(np.asarray(Tq, np.float64), (B, mT))
    S = np.asarray(spot, np.float64).reshape(B)
    TH0 = np.asarray(theta0, np.float64).reshape(B, mT) if raw is None else theta0_of_raw(raw, T, S)
    rounds = DEFAULT_ROUNDS if rounds == 0 else int(rounds)
    surface, theta = np.full((B, 4), np.nan), np.full((B, mT), np.nan)
    params, fit = np.full((B, mT, 5), np.nan), np.full((B, mT, 3), np.nan)
    flags, sflags = np.full((B, mT), DEAD, np.int32), np.zeros(B, np.int32)
    fit_vol = np.full((B, mT, mK), np.nan)
    point, step = np.full((B, 3), np.nan), np.full((B, 3), np.nan)
    n_, sse_ = np.zeros(B, np.int64), np.full(B, np.nan)
    identified = np.zeros(B, bool)
    g_scale = np.full((B, mT), np.nan)                                                 # the magnitude of g's terms, for the tests
    with np.errstate(all="ignore"):
        for b in range(B):
            live = _pos(S[b]) & _pos(T[b]) & _pos(TH0[b])                              # J1
            valid = _pos(K[b])[None, :] & _pos(vol[b]) & live[:, None]
            rows = np.flatnonzero(live)
            n = int(valid.sum())
            if len(rows) == 0 or n < 5:
                sflags[b] |= SURF_DEAD
            if (np.diff(T[b][rows]) <= 0).any() or np.isnan(np.diff(T[b][rows])).any():
                sflags[b] |= UNORDERED
            if sflags[b]:
                continue
            th = np.maximum.accumulate(TH0[b][rows])                                   # J3
            L, q, inv = np.log(th), np.sqrt(th), 1.0 / th
            xs, ws, rw = [], [], []
            for l, j in enumerate(rows):                                               # J2, (tenor, node) order
                i = np.flatnonzero(valid[j])
                xs.append(np.log(K[b][i] / S[b]) - rate * T[b, j])
                ws.append(vol[b, j][i] * vol[b, j][i] * T[b, j])
                rw.append(np.full(len(i), l))
            x, w, row = np.concatenate(xs), np.concatenate(ws), np.concatenate(rw).astype(int)
            pt, eta, sse, h = search(th, L, q, inv, row, x, w, rounds)
            rho, gam, s = pt
            point[b], step[b], n_[b], sse_[b] = pt, h, n, sse
            identified[b] = len(np.unique(th)) > 1
            surface[b] = rho, eta, gam, np.sqrt(sse / n)
            band = (DOM_HI - DOM_LO) * EDGE_BAND                                       # J8
            if rho - DOM_LO[0] <= band[0] or DOM_HI[0] - rho <= band[0]:
                sflags[b] |= EDGE_RHO
            if gam - DOM_LO[1] <= band[1] or DOM_HI[1] - gam <= band[1]:
                sflags[b] |= EDGE_GAMMA
            if s - DOM_LO[2] <= band[2]:
                sflags[b] |= EDGE_ETA_LOW
            if DOM_HI[2] - s <= band[2]:
                sflags[b] |= AT_BOUND
            omr = 1.0 - rho * rho
            for l, j in enumerate(rows):
                phi = eta * np.exp(-gam * L[l])
                pa, pb, pm, psig = th[l] * omr / 2.0, th[l] * phi / 2.0, -rho / phi, np.sqrt(omr) / phi
                theta[b, j] = th[l]
                params[b, j] = pa, pb, rho, pm, psig
                fl = (RAISED if th[l] > TH0[b, j] else 0)
                i = np.flatnonzero(valid[j])
                if len(i) and i[-1] - i[0] + 1 > len(i):
                    fl |= HOLES
                kp = _pos(K[b])
                xa = np.log(K[b] / S[b]) - rate * T[b, j]
                wf = model(th[l], phi, rho, xa)
                vf = np.sqrt(np.maximum(wf, 0.0) / T[b, j])
                fit_vol[b, j] = np.where(kp, vf, np.nan)
                if len(i):
                    e = vf[i] - vol[b, j][i]
                    dx = xa[i] - pm
                    r = np.sqrt(dx * dx + psig * psig)
                    w1 = pb * (rho + dx / r)
                    w2 = pb * psig * psig / (r * r * r)
                    u = 1.0 - xa[i] * w1 / (2.0 * wf[i])
                    g = u * u - (w1 * w1 / 4.0) * (1.0 / wf[i] + 0.25) + w2 / 2.0
                    fit[b, j] = np.sqrt(_asc(e * e) / len(i)), np.max(np.abs(e)), np.min(g)
                    a_ = xa[i] * w1 / (2.0 * wf[i])
                    g_scale[b, j] = np.max(u * u + (w1 * w1 / 4.0) * (1.0 / wf[i] + 0.25) + w2 / 2.0 + 2.0 * np.abs(u * a_))
                    if np.min(g) < 0.0:
                        fl |= BUTTERFLY
                flags[b, j] = fl
    out = {"surface": surface, "theta": theta, "params": params, "fit": fit, "flags": flags, "sflags": sflags,
           "fitted": fit_vol if fitted else None, "point": point, "step": step, "n": n_, "sse": sse_, "identified": identified,
           "theta0": TH0, "g_scale": g_scale}
    if margins:
        check_margins(out)
    return out


def check_margins(r):
    """The conditions of the generated batches: gamma* <= 0.95, adjacent unraised theta at least 1e-9
    apart relatively, at least 90 % of the rows live, at least one RAISED row with mT >= 13."""
    fl, th = r["flags"], r["theta"]
    B, mT = fl.shape
    lv = fl != DEAD
    assert lv.mean() >= 0.9, f"only {lv.mean():.3f} of the rows are live: the generator is at fault"
    ok = (r["sflags"] & (SURF_DEAD | UNORDERED)) == 0
    assert (r["surface"][ok, 2] <= 0.95).all(), r["surface"][ok, 2].max()
    for b in np.flatnonzero(ok):
        j = np.flatnonzero(lv[b])
        d = np.diff(th[b][j])
        un = (fl[b][j][1:] & RAISED) == 0
        assert (d[un] >= 1e-9 * th[b][j][1:][un]).all(), (b, d[un].min())
    if mT >= 13:
        assert (fl[lv] & RAISED).any(), "no RAISED row"


def twin(case, seed, rounds=0):
    """The restatement on vol x (1 + 2^-52 xi), xi standard normal."""
    xi = np.random.default_rng(seed).standard_normal(case["vol"].shape)
    with np.errstate(all="ignore"):
        vol = case["vol"] * (1.0 + 2.0 ** -52 * xi)
    return restate(vol, case["Kq"], case["Tq"], case["spot"], case["rate"], raw=case.get("raw"), theta0=case.get("theta0"),
                   rounds=rounds)


class RefBackend(cal_ref.RefBackend):
    """CPU stand-in for snapshots.HipBackend with the SSVI fit restated."""

    def ssvi(self, vol, Kq, Tq, spot, rate, raw, theta0, rounds, fitted):
        r = restate(vol, Kq, Tq, spot, rate, raw=raw, theta0=theta0, rounds=rounds, fitted=fitted)
        return {k: r[k] for k in ("surface", "theta", "params", "fit", "flags", "sflags", "fitted")}
