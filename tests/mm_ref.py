"""Independent restatement of the moment rules M1-M7.  TEST INFRASTRUCTURE ONLY.

Shares no code with iv_interpolation_amd: a row is one whole array of its valid nodes, the forward node of rule M4 is put in
with np.insert, and every sum runs in plain ascending order (a cumulative sum); there are no lanes and no chunks.  The
arithmetic is selectable: float64 (NumPy, scipy.special) or mpmath at 50 digits on the same float64 inputs (the
rounding-level test).

    restate(vol, Kq, Tq, spot, rate=0.0, horizons=(30/365,), min_mass=0.99, exact=False, margins=False) -> dict
        raw [B,mT,4] (L, V, W, X), stats [B,mT,4] (mf_vol, bkm_vol, skew, kurt), mass [B,mT], flags [B,mT] int32,
        index [B,nH], index_flags [B,nH] int32, and for the tolerances raw_scale [B,mT,4] (see below), d2_first, d2_last
        [B,mT] (the two arguments of `mass`)
        margins=True asserts L >= 1e-9 raw_scale[0] and var >= 1e-9 var_scale in every row that is not DEAD, mass at least
        1e-6 away from min_mass, and that >= 90 % of the rows are not DEAD
    tolerances(ref, C, eps)  -> dict of absolute tolerances for raw, stats, mass, index (rules of the GPU test)
    RefBackend()  -> arb_ref.RefBackend plus moments

raw_scale: the sum of the absolute values of the trapezoid terms, in which each Phi inside Q counts (1 + d^2) times (erfc
carries eps d^2 from its exponential) and the x-dependent factor, taken term by term in absolute value, counts
(1 + |x| / sqrt(w)) times (the rounding of the log reaches d through x / sqrt(w)).  The forward node of M4 counts as it
is (its erf has no cancellation).  exact=True leaves raw_scale NaN: the rounding-level test takes it from the float64 run.
"""
import numpy as np

import arb_ref

ONE_SIDED, TRUNCATED, HOLES, DEAD, NO_BRACKET = 1, 2, 4, 8, 16
MARGIN = 1e-9
MASS_MARGIN = 1e-6


class _F64:
    """float64 arithmetic: NumPy and scipy.special."""
    def __init__(self):
        from scipy import special
        self.erf, self.erfc = special.erf, special.erfc
        self.log, self.exp, self.sqrt = np.log, np.exp, np.sqrt
        self.num = np.float64

    def arr(self, a):
        return np.asarray(a, np.float64)


class _MP:
    """mpmath at 50 digits on object arrays."""
    def __init__(self):
        import mpmath
        self.mp = mpmath.mp.clone()
        self.mp.dps = 50
        for name in ("erf", "erfc", "log", "exp", "sqrt"):
            setattr(self, name, np.frompyfunc(getattr(self.mp, name), 1, 1))
        self.num = self.mp.mpf

    def arr(self, a):
        a = np.asarray(a, np.float64)
        out = np.empty(a.shape, object)
        out.ravel()[:] = [self.mp.mpf(float(v)) for v in a.ravel()]
        return out if a.ndim else out[()]


def _pos(a):
    return np.isfinite(a) & (a > 0)


def _ascending_sum(terms):
    """Plain left-to-right sum along the last axis."""
    return np.cumsum(terms, axis=-1)[..., -1]


def _g(x, absolute=False):
    """Rule M5's x-dependent factors of L, V, W, X; absolute=True: every term of each polynomial in absolute value."""
    one = x * 0 + 1
    if absolute:
        x = abs(x)
        return [2 * one, 2 * (1 + x), 6 * x + 3 * x * x, 12 * x * x + 4 * x * x * x]
    return [2 * one, 2 * (1 - x), 6 * x - 3 * x * x, 12 * x * x - 4 * x * x * x]


def _row(k, s, S, tau, rate, min_mass, A, scales=True):
    """One row (M1-M6).  k, s float64 arrays, S, tau float64.  Returns None for a DEAD row, else
    (raw[4], stats[4], mass, flags, raw_scale[4], var_scale, d2_first, d2_last) in A's arithmetic."""
    if not (_pos(S) and _pos(tau)):
        return None
    valid = _pos(k) & _pos(s)
    idx = np.flatnonzero(valid)
    if len(idx) < 2 or not np.all(np.diff(k[idx]) > 0):                # M1
        return None
    flags = HOLES if idx[-1] - idx[0] + 1 > len(idx) else 0
    half = A.num(1) / 2
    kk, ss, Sx, tx, r = A.arr(k[idx]), A.arr(s[idx]), A.arr(S), A.arr(tau), A.arr(rate)
    # M2
    w = ss * ss * tx
    sq = A.sqrt(w)
    x = A.log(kk / Sx) - r * tx
    F = Sx * A.exp(r * tx)
    d2 = -x / sq - half * sq
    d1 = d2 + sq
    rt2 = A.sqrt(A.num(2))
    Phi = lambda z: half * A.erfc(-z / rt2)  # noqa: E731
    # M3
    put = kk < F
    a2, a1 = np.where(put, -d2, d2), np.where(put, -d1, d1)
    P2, P1 = Phi(a2), Phi(a1)
    Q = np.where(put, kk * P2 - F * P1, F * P1 - kk * P2)
    Qs = kk * P2 * (1 + a2 * a2) + F * P1 * (1 + a1 * a1) if scales else None
    k2 = kk * kk
    f = [g * Q / k2 for g in _g(x)]
    fs = [g * (1 + abs(x) / sq) * Qs / k2 for g in _g(x, absolute=True)] if scales else [kk * float("nan")] * 4
    kn = kk
    # M4
    if F < kk[0] or F > kk[-1]:
        flags |= ONE_SIDED
    else:
        a = int(np.flatnonzero(kk < F)[-1]) if (kk < F).any() else -1
        if a >= 0 and a + 1 < len(kk) and kk[a + 1] > F:
            sF = ss[a] + (ss[a + 1] - ss[a]) * (F - kk[a]) / (kk[a + 1] - kk[a])
            QF = F * A.erf(A.sqrt(sF * sF * tx) / (2 * rt2))
            fF = [2 * QF / (F * F), 2 * QF / (F * F), A.num(0), A.num(0)]
            kn = np.insert(kn, a + 1, F)
            f = [np.insert(f[m], a + 1, fF[m]) for m in range(4)]
            fs = [np.insert(fs[m], a + 1, fF[m]) for m in range(4)]
    # M5
    dk = kn[1:] - kn[:-1]
    raw = [_ascending_sum(half * (f[m][:-1] + f[m][1:]) * dk) for m in range(4)]
    scale = [_ascending_sum(half * (fs[m][:-1] + fs[m][1:]) * dk) for m in range(4)]
    # M6
    L, V, W, X = raw
    mu = -V / 2 - W / 6 - X / 24
    var = V - mu * mu
    if not (L > 0 and var > 0):
        return None
    mu_scale = scale[1] / 2 + scale[2] / 6 + scale[3] / 24
    var_scale = scale[1] + 2 * abs(mu) * mu_scale
    stats = [A.sqrt(L / tx), A.sqrt(var / tx), (W - 3 * mu * V + 2 * mu ** 3) / (var * A.sqrt(var)),
             (X - 4 * mu * W + 6 * mu * mu * V - 3 * mu ** 4) / (var * var)]
    mass = 1 - Phi(-d2[0]) - Phi(d2[-1])
    if mass < min_mass:
        flags |= TRUNCATED
    return raw, stats, mass, flags, scale, var_scale, d2[0], d2[-1]


def index_of(L, tau, flags, horizons):
    """Rule M7 for one snapshot: L, tau, flags [mT] -> (index [nH], index_flags [nH])."""
    ix, fx = np.full(len(horizons), np.nan), np.full(len(horizons), NO_BRACKET, np.int32)
    rows = [j for j in range(len(L)) if not flags[j] & DEAD]
    for t, h in enumerate(horizons):
        for j, jn in zip(rows[:-1], rows[1:]):
            if tau[j] <= h <= tau[jn] and tau[j] < tau[jn]:
                Lh = L[j] + (L[jn] - L[j]) * (h - tau[j]) / (tau[jn] - tau[j])
                ix[t], fx[t] = 100.0 * np.sqrt(Lh / h), flags[j] | flags[jn]
                break
    return ix, fx


def restate(vol, Kq, Tq, spot, rate=0.0, horizons=(30.0 / 365.0,), min_mass=0.99, exact=False, margins=False):
    A = _MP() if exact else _F64()
    vol = np.asarray(vol, np.float64)
    B, mT, mK = vol.shape
    K = np.broadcast_to(np.asarray(Kq, np.float64), (B, mK))
    T = np.broadcast_to(np.asarray(Tq, np.float64), (B, mT))
    S = np.asarray(spot, np.float64).reshape(B)
    hz = [float(h) for h in horizons]
    dt = object if exact else np.float64
    raw, stats, scale = (np.full((B, mT, 4), np.nan, dt) for _ in range(3))
    mass, var_scale, d2f, d2l = (np.full((B, mT), np.nan, dt) for _ in range(4))
    flags = np.full((B, mT), DEAD, np.int32)
    with np.errstate(all="ignore"):
        for b in range(B):
            for j in range(mT):
                r = _row(K[b], vol[b, j], S[b], T[b, j], rate, min_mass, A, scales=not exact)
                if r is not None:
                    raw[b, j], stats[b, j], mass[b, j], flags[b, j], scale[b, j], var_scale[b, j], d2f[b, j], d2l[b, j] = r
        index, index_flags = np.full((B, len(hz)), np.nan), np.full((B, len(hz)), NO_BRACKET, np.int32)
        Lf = raw[:, :, 0].astype(np.float64)
        for b in range(B):
            index[b], index_flags[b] = index_of(Lf[b], T[b], flags[b], hz)
    out = {"raw": raw, "stats": stats, "mass": mass, "flags": flags, "index": index, "index_flags": index_flags,
           "raw_scale": scale, "var_scale": var_scale, "d2_first": d2f, "d2_last": d2l}
    if margins:
        ok = flags != DEAD
        assert ok.mean() >= 0.9, f"only {ok.mean():.3f} of the rows are not DEAD: the generator is at fault"
        assert np.all(raw[ok][:, 0] >= MARGIN * scale[ok][:, 0]), "a row has L within 1e-9 of 0: the generator is at fault"
        var = raw[ok][:, 1] - (raw[ok][:, 1] / 2 + raw[ok][:, 2] / 6 + raw[ok][:, 3] / 24) ** 2
        assert np.all(var >= MARGIN * var_scale[ok]), "a row has var within 1e-9 of 0: the generator is at fault"
        if min_mass > 0:
            assert np.all(np.abs(mass[ok] - min_mass) >= MASS_MARGIN), "a row's mass sits on min_mass: the generator is at fault"
    return out


def stats_of(raw, tau):
    """Rule M6 in NumPy on given raw moments [..., 4] and tenors [...]."""
    L, V, W, X = (raw[..., m] for m in range(4))
    mu = -V / 2 - W / 6 - X / 24
    var = V - mu * mu
    return np.stack([np.sqrt(L / tau), np.sqrt(var / tau), (W - 3 * mu * V + 2 * mu ** 3) / (var * np.sqrt(var)),
                     (X - 4 * mu * W + 6 * mu * mu * V - 3 * mu ** 4) / (var * var)], axis=-1)


def tolerances(ref, Tq, horizons, C, eps):
    """Absolute tolerances of the GPU test.  raw: C eps raw_scale.  stats and index: the raw tolerances carried through the
    formulas of M6 / M7 -- every term of a numerator or denominator contributes |term| x the relative tolerances of its
    factors -- plus C eps of the result for the formula's own arithmetic.  mass: C eps (1 + d2^2) per Phi."""
    from scipy import special
    raw, sc = ref["raw"], ref["raw_scale"]
    B, mT, _ = raw.shape
    T = np.broadcast_to(np.asarray(Tq, np.float64), (B, mT))
    with np.errstate(all="ignore"):
        t = C * eps * sc
        tL, tV, tW, tX = (t[..., m] for m in range(4))
        L, V, W, X = (raw[..., m] for m in range(4))
        mu = -V / 2 - W / 6 - X / 24
        var = V - mu * mu
        tmu = tV / 2 + tW / 6 + tX / 24
        tvar = tV + 2 * np.abs(mu) * tmu
        st = ref["stats"]
        t_mf = st[..., 0] * (0.5 * tL / L + C * eps)
        t_bkm = st[..., 1] * (0.5 * tvar / var + C * eps)
        num3 = tW + 3 * (np.abs(V) * tmu + np.abs(mu) * tV) + 6 * mu * mu * tmu
        abs3 = np.abs(W) + 3 * np.abs(mu * V) + 2 * np.abs(mu) ** 3
        t_skew = (num3 + C * eps * abs3) / var ** 1.5 + np.abs(st[..., 2]) * (1.5 * tvar / var + C * eps)
        num4 = tX + 4 * (np.abs(W) * tmu + np.abs(mu) * tW) + 6 * (2 * np.abs(mu * V) * tmu + mu * mu * tV) + 12 * np.abs(mu) ** 3 * tmu
        abs4 = np.abs(X) + 4 * np.abs(mu * W) + 6 * mu * mu * np.abs(V) + 3 * mu ** 4
        t_kurt = (num4 + C * eps * abs4) / var ** 2 + np.abs(st[..., 3]) * (2 * tvar / var + C * eps)
        Phi = lambda z: 0.5 * special.erfc(-z / np.sqrt(2.0))  # noqa: E731
        d2f, d2l = ref["d2_first"], ref["d2_last"]
        t_mass = C * eps * (1 + Phi(-d2f) * (1 + d2f ** 2) + Phi(d2l) * (1 + d2l ** 2))
        hz = [float(h) for h in horizons]
        t_ix = np.full((B, len(hz)), np.nan)
        for b in range(B):
            rows = [j for j in range(mT) if not ref["flags"][b, j] & DEAD]
            for q, h in enumerate(hz):
                for j, jn in zip(rows[:-1], rows[1:]):
                    if T[b, j] <= h <= T[b, jn] and T[b, j] < T[b, jn]:
                        u = (h - T[b, j]) / (T[b, jn] - T[b, j])
                        Lh = L[b, j] + (L[b, jn] - L[b, j]) * u
                        tLh = (1 - u) * tL[b, j] + u * tL[b, jn] + C * eps * (np.abs(L[b, j]) + np.abs(L[b, jn]))
                        t_ix[b, q] = ref["index"][b, q] * (0.5 * tLh / Lh + C * eps)
                        break
    return {"raw": t, "stats": np.stack([t_mf, t_bkm, t_skew, t_kurt], axis=-1), "mass": t_mass, "index": t_ix}


class RefBackend(arb_ref.RefBackend):
    """CPU stand-in for snapshots.HipBackend with the moments restated."""

    def moments(self, vol, Kq, Tq, spot, rate, horizons, min_mass):
        r = restate(vol, Kq, Tq, spot, rate, horizons, min_mass)
        return {k: r[k] for k in ("raw", "stats", "mass", "flags", "index", "index_flags")}
