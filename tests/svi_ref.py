"""Independent restatement of the SVI rules V1-V8.  TEST INFRASTRUCTURE ONLY.

Shares no code with iv_interpolation_amd: a row is one whole array of its valid nodes, the 64 candidates of a round are one
NumPy vector, the 27 active sets of rule V4 one more axis, and every sum over the nodes runs in plain ascending order (a
cumulative sum); there are no lanes, no chunks and no butterflies.  Up to 64 rows are searched at once to spare NumPy's
call overhead: a shorter row is padded with masked nodes, which trail in every sum as exact zeros and change no bit.

    restate(vol, Kq, Tq, spot, rate=0.0, rounds=0, fitted=True, margins=False) -> dict
        params [B,mT,5] (a, b, rho, m, sigma), fit [B,mT,4] (rmse_w, rmse_vol, max_vol_err, g_min), flags [B,mT] int32,
        fitted [B,mT,mK] (None with fitted=False), and for the tests u [B,mT] = ln sigma as the search left it, step [B,mT,2]
        = the last round's grid step in m and u, width [B,mT,2] = the width of the domain in m and u, sse [B,mT], n [B,mT],
        wmax [B,mT]
        margins=True asserts that >= 90 % of the rows are not DEAD
    twin(case, seed)  -> restate(...) of the case with vol x (1 + 2^-52 xi), xi standard normal: the stand-in for another
        arithmetic (FMA contraction, another log / exp / sqrt)
    inner(x, w, m, sigma) -> the 27 solutions of rule V4 for given candidates (the brute-force test ranks them)
    RefBackend()  -> mm_ref.RefBackend plus svi
"""
import numpy as np

import mm_ref

BOUND, EDGE, HOLES, DEAD, BUTTERFLY, DEGENERATE = 1, 2, 4, 8, 16, 32
DEFAULT_ROUNDS = 16

# V4: set s = 9 ia + icd.  ia: a free, a = 0, a = w_max.  icd: interior, d = c, d = -c, c + d = 2 sigma, c - d = 2 sigma, then
# the vertices (c, d) = (0, 0), (sigma, sigma), (2 sigma, 0), (sigma, -sigma).  In p = (c - d) / 2, q = (c + d) / 2 the prism
# is the box 0 <= a <= w_max, 0 <= p, q <= sigma, so a set is one state per variable: 0 free, 1 at 0, 2 at its upper bound.
_PQ = ((0, 0), (1, 0), (0, 1), (0, 2), (2, 0), (1, 1), (1, 2), (2, 2), (2, 1))
STATES = np.array([(ia,) + _PQ[icd] for ia in range(3) for icd in range(9)])          # [27, 3]


def _pos(a):
    return np.isfinite(a) & (a > 0)


def _asc(terms):
    """Plain left-to-right sum along the last axis."""
    acc = np.array(terms[..., 0], np.float64)
    for i in range(1, terms.shape[-1]):
        acc = acc + terms[..., i]
    return acc


def inner(x, w, m, sigma, mask=None):
    """Rule V4 for candidates m, sigma [..., C] on the nodes x, w [..., n] (leading axes = rows; mask [..., n] marks the nodes
    of a row shorter than n, which then trail as exact zeros in every sum): returns theta [..., 27, C, 3] = (a, p, q) of every
    active set, feasible [..., 27, C], E [..., 27, C], and y, z [..., C, n]."""
    mask = np.ones(x.shape) if mask is None else mask
    n = mask.sum(axis=-1)[..., None]                                                 # [..., 1]
    mk = mask[..., None, :]
    inv = 1.0 / sigma
    y = (x[..., None, :] - m[..., :, None]) * inv[..., :, None] * mk
    z = np.sqrt(y * y + 1.0) * mk
    wn = w[..., None, :]
    Sy, Sz, Syy, Syz = _asc(y), _asc(z), _asc(y * y), _asc(y * z)
    Swy, Swz, Sw = _asc(wn * y), _asc(wn * z), _asc(w)[..., None]
    wmax = w.max(axis=-1)[..., None]
    # the Gram matrix of (1, y, z) in the basis (1, z - y, z + y) of (a, p, q); z^2 - y^2 = 1
    nn = n + 0.0 * Sy
    H = {(0, 0): nn, (0, 1): Sz - Sy, (0, 2): Sz + Sy, (1, 1): (2.0 * Syy + n) - 2.0 * Syz, (2, 2): (2.0 * Syy + n) + 2.0 * Syz,
         (1, 2): nn}
    g = [Sw + 0.0 * Sy, Swz - Swy, Swz + Swy]
    hi = [wmax + 0.0 * sigma, sigma, sigma]
    ex = lambda a: a[..., None, :]  # noqa: E731                                      [..., C] -> [..., 1, C]
    Hs = lambda i, j: ex(H[(min(i, j), max(i, j))])  # noqa: E731
    fixed = [STATES[:, i:i + 1] != 0 for i in range(3)]                              # [27, 1]
    val = [np.where(STATES[:, i:i + 1] == 2, ex(hi[i]), 0.0) for i in range(3)]      # [..., 27, C]
    # fixed variable k: row and column k of the system become the unit row, its right-hand side the bound
    A = {}
    for i in range(3):
        for j in range(i, 3):
            A[(i, j)] = np.where(fixed[i] | fixed[j], 1.0 if i == j else 0.0, Hs(i, j))
    b = []
    for i in range(3):
        r = ex(g[i]) + 0.0 * val[0]
        for j in range(3):
            if j != i:
                r = r - np.where(fixed[j], Hs(i, j) * val[j], 0.0)
        b.append(np.where(fixed[i], val[i], r))
    # LDL^T in the order a, p, q
    d0 = A[(0, 0)]
    l10, l20 = A[(0, 1)] / d0, A[(0, 2)] / d0
    d1 = A[(1, 1)] - l10 * A[(0, 1)]
    t21 = A[(1, 2)] - l20 * A[(0, 1)]
    l21 = t21 / d1
    d2 = A[(2, 2)] - l20 * A[(0, 2)] - l21 * t21
    y1 = b[1] - l10 * b[0]
    y2 = b[2] - l20 * b[0] - l21 * y1
    t2 = y2 / d2
    t1 = y1 / d1 - l21 * t2
    t0 = b[0] / d0 - l10 * t1 - l20 * t2
    th = [np.where(fixed[i], val[i], t) for i, t in enumerate((t0, t1, t2))]
    feas = np.ones(th[0].shape, bool)
    for i in range(3):
        feas &= fixed[i] | ((th[i] >= 0.0) & (th[i] <= ex(hi[i])))
    dl = [th[i] - th[i][..., 0:1, :] for i in range(3)]                              # set 0 is the unconstrained solution
    E = (Hs(0, 0) * dl[0] * dl[0] + Hs(1, 1) * dl[1] * dl[1] + Hs(2, 2) * dl[2] * dl[2]
         + 2.0 * (Hs(0, 1) * dl[0] * dl[1] + Hs(0, 2) * dl[0] * dl[2] + Hs(1, 2) * dl[1] * dl[2]))
    return np.stack(th, axis=-1), feas, E, y, z


def candidates(x, w, m, sigma, mask=None):
    """Rule V4 for candidates m, sigma [..., C]: the winning set's (a, d, c), its number and its direct-residual SSE."""
    th, feas, E, y, z = inner(x, w, m, sigma, mask)
    mask = np.ones(x.shape) if mask is None else mask
    best = np.full(m.shape, np.inf)
    a = (_asc(w) / mask.sum(axis=-1))[..., None] + 0.0 * m                            # the fallback: set 5, the flat line
    p, q = 0.0 * m, 0.0 * m
    win = np.full(m.shape, 5)
    for s in range(27):
        Es, fs = E[..., s, :], feas[..., s, :]
        take = fs & (Es < best)
        best = np.where(take, Es, best)
        a, p, q = np.where(take, th[..., s, :, 0], a), np.where(take, th[..., s, :, 1], p), np.where(take, th[..., s, :, 2], q)
        win = np.where(take, s, win)
    c, d = p + q, q - p
    res = (a[..., None] + d[..., None] * y + c[..., None] * z - w[..., None, :]) * mask[..., None, :]
    return a, d, c, win, _asc(res * res)


EDGE_BAND = 2.0 ** -20
_IM, _IU = np.arange(64) % 8, np.arange(64) // 8                                      # candidate 8 i_u + i_m


def grid(lo, hi):
    """p_i = lo + i step, p_7 = hi itself; lo, hi [R] -> p [R, 8], step [R]."""
    step = (hi - lo) / 7.0
    p = lo[:, None] + np.arange(8) * step[:, None]
    p[:, 7] = hi
    return p, step


def search(xs, ws, rounds):
    """Rule V5 on a list of rows (x, w) at once: the rows are padded to one length with masked nodes.  Returns per row
    a, d, c, win, sse, m, u, sigma, the last steps (hm, hu) and the domains."""
    R_, N = len(xs), max(len(x) for x in xs)
    x, w, mask = np.zeros((R_, N)), np.zeros((R_, N)), np.zeros((R_, N))
    for r, (xr, wr) in enumerate(zip(xs, ws)):
        x[r, :len(xr)], w[r, :len(xr)], mask[r, :len(xr)] = xr, wr, 1.0
        x[r, len(xr):] = xr[-1]
    x0, x1 = np.array([xr[0] for xr in xs]), np.array([xr[-1] for xr in xs])
    X = x1 - x0
    u0, u1 = np.log(X / 256.0), np.log(4.0 * X)
    mlo, mhi, ulo, uhi = x0, x1, u0, u1
    rows = np.arange(R_)
    for _ in range(rounds):
        (pm, hm), (pu, hu) = grid(mlo, mhi), grid(ulo, uhi)
        m, u = pm[:, _IM], pu[:, _IU]
        sig = np.exp(u)
        a, d, c, win, sse = candidates(x, w, m, sig, mask)
        best = np.argmin(np.where(np.isnan(sse), np.inf, sse), axis=1)               # the first of equals
        ms, us = m[rows, best], u[rows, best]
        mlo, mhi = np.maximum(x0, ms - hm), np.minimum(x1, ms + hm)
        ulo, uhi = np.maximum(u0, us - hu), np.minimum(u1, us + hu)
    pick = lambda t: t[rows, best]  # noqa: E731
    return dict(a=pick(a), d=pick(d), c=pick(c), win=pick(win), sse=pick(sse), m=ms, u=us, sigma=pick(sig), hm=hm, hu=hu,
                x0=x0, x1=x1, u0=u0, u1=u1)


def prepare(k, s, S, tau, rate):
    """V1 / V2 for one row: None for a DEAD row, else (idx, x, w, flags)."""
    if not (_pos(S) and _pos(tau)):
        return None
    idx = np.flatnonzero(_pos(k) & _pos(s))
    if len(idx) < 5 or not np.all(np.diff(k[idx]) > 0):
        return None
    flags = HOLES if idx[-1] - idx[0] + 1 > len(idx) else 0
    return idx, np.log(k[idx] / S) - rate * tau, s[idx] * s[idx] * tau, flags


def finish(f, r, x, w, s, tau, flags):
    """V6 / V7 for row r of the search result f."""
    a, d, c, win, sse, sig, ms, us = (f[k][r] for k in ("a", "d", "c", "win", "sse", "sigma", "m", "u"))
    n = len(x)
    b = c / sig
    rho = d / c if c != 0.0 else 0.0
    if win != 0:
        flags |= BOUND
    X, U = f["x1"][r] - f["x0"][r], f["u1"][r] - f["u0"][r]
    if ms - f["x0"][r] <= X * EDGE_BAND or f["x1"][r] - ms <= X * EDGE_BAND or us - f["u0"][r] <= U * EDGE_BAND or f["u1"][r] - us <= U * EDGE_BAND:
        flags |= EDGE
    dx = x - ms
    rr = np.sqrt(dx * dx + sig * sig)
    wf = a + b * (rho * dx + rr)
    vf = np.sqrt(np.maximum(wf, 0.0) / tau)
    e = vf - s
    w1 = b * (rho + dx / rr)
    w2 = b * sig * sig / (rr * rr * rr)
    t = 1.0 - x * w1 / (2.0 * wf)
    g = t * t - (w1 * w1 / 4.0) * (1.0 / wf + 0.25) + w2 / 2.0
    gmin = np.min(g)
    if (wf <= 0.0).any():
        flags |= DEGENERATE
        gmin = np.nan
    if gmin < 0.0:
        flags |= BUTTERFLY
    fit = (np.sqrt(sse / n), np.sqrt(_asc(e * e) / n), np.max(np.abs(e)), gmin)
    return dict(params=(a, b, rho, ms, sig), fit=fit, flags=flags, u=us, step=(f["hm"][r], f["hu"][r]), width=(X, U), sse=sse, n=n,
                wmax=w.max())


BLOCK = 64          # rows searched at once: bounds the [rows, 27, 64] and [rows, 64, n] temporaries


def restate(vol, Kq, Tq, spot, rate=0.0, rounds=0, fitted=True, margins=False):
    vol = np.asarray(vol, np.float64)
    B, mT, mK = vol.shape
    K = np.broadcast_to(np.asarray(Kq, np.float64), (B, mK))
    T = np.broadcast_to(np.asarray(Tq, np.float64), (B, mT))
    S = np.asarray(spot, np.float64).reshape(B)
    rounds = DEFAULT_ROUNDS if rounds == 0 else int(rounds)
    params, fit = np.full((B, mT, 5), np.nan), np.full((B, mT, 4), np.nan)
    flags = np.full((B, mT), DEAD, np.int32)
    fit_vol = np.full((B, mT, mK), np.nan)
    u, sse, wmax = np.full((B, mT), np.nan), np.full((B, mT), np.nan), np.full((B, mT), np.nan)
    step, width = np.full((B, mT, 2), np.nan), np.full((B, mT, 2), np.nan)
    n = np.zeros((B, mT), np.int32)
    with np.errstate(all="ignore"):
        live = []
        for b in range(B):
            for j in range(mT):
                pr = prepare(K[b], vol[b, j], S[b], T[b, j], rate)
                if pr is not None:
                    live.append((b, j) + pr)
        for at in range(0, len(live), BLOCK):
            blk = live[at:at + BLOCK]
            f = search([t[3] for t in blk], [t[4] for t in blk], rounds)
            for q, (b, j, idx, x, w, fl) in enumerate(blk):
                r = finish(f, q, x, w, vol[b, j][idx], T[b, j], fl)
                params[b, j], fit[b, j], flags[b, j], u[b, j], sse[b, j], n[b, j] = r["params"], r["fit"], r["flags"], r["u"], r["sse"], r["n"]
                step[b, j], width[b, j], wmax[b, j] = r["step"], r["width"], r["wmax"]
                a_, b_, rho, m, sig = r["params"]
                kp = _pos(K[b])                                                      # V8: every node with a strike
                dx = np.log(K[b][kp] / S[b]) - rate * T[b, j] - m
                wf = a_ + b_ * (rho * dx + np.sqrt(dx * dx + sig * sig))
                fit_vol[b, j, kp] = np.sqrt(np.maximum(wf, 0.0) / T[b, j])
    if margins:
        ok = flags != DEAD
        assert ok.mean() >= 0.9, f"only {ok.mean():.3f} of the rows are not DEAD: the generator is at fault"
    return {"params": params, "fit": fit, "flags": flags, "fitted": fit_vol if fitted else None, "u": u, "step": step,
            "width": width, "sse": sse, "n": n, "wmax": wmax}


def twin(case, seed, rounds=0):
    """The restatement on vol x (1 + 2^-52 xi), xi standard normal."""
    xi = np.random.default_rng(seed).standard_normal(case["vol"].shape)
    with np.errstate(all="ignore"):
        vol = case["vol"] * (1.0 + 2.0 ** -52 * xi)
    return restate(vol, case["Kq"], case["Tq"], case["spot"], case["rate"], rounds)


class RefBackend(mm_ref.RefBackend):
    """CPU stand-in for snapshots.HipBackend with the SVI fit restated."""

    def svi(self, vol, Kq, Tq, spot, rate, rounds, fitted):
        r = restate(vol, Kq, Tq, spot, rate, rounds, fitted)
        return {k: r[k] for k in ("params", "fit", "flags", "fitted")}
