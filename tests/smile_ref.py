"""Independent NumPy restatement of the smile rules D1-D6.  TEST INFRASTRUCTURE ONLY.

Shares no code with iv_interpolation_amd: a row's valid nodes are COMPRESSED into their own arrays (so neighbours are
adjacent and no "previous valid node" bookkeeping exists), the brackets are found row by row in a Python loop, and the 52
bisection steps then run on all brackets at once as NumPy array operations.

    restate(vol, Kq, Tq, spot, deltas, rate=0.0, monotone=False) -> dict(vol, strike, flags, ia, ib)
    closed_form_flat(S, sigma, tau, z, rate)                        -> strike of a flat smile (the anchor of the restatement)
    RefBackend()                                                    -> snapshot_ref.RefBackend plus smile_points
"""
from statistics import NormalDist

import numpy as np

import snapshot_ref

OK, NO_CROSSING, AMBIGUOUS, DEAD = 0, 1, 2, 4
STEPS = 52


def z_of(delta):
    """D3: the standard-normal quantile of the call delta a signed target means."""
    d = float(delta)
    if 0.0 < d < 1.0:
        return NormalDist().inv_cdf(d)
    if -1.0 < d < 0.0:
        return NormalDist().inv_cdf(1.0 + d)
    raise ValueError(f"bad target delta {delta!r}")


def call_delta(delta):
    d = float(delta)
    return d if d > 0 else 1.0 + d


def d1_of(S, k, s, r, tau):
    """D1, the expression of bs_greeks_one."""
    return (np.log(S / k) + (r + 0.5 * s * s) * tau) / (s * np.sqrt(tau))


def closed_form_flat(S, sigma, tau, z, rate=0.0):
    return S * np.exp(-z * sigma * np.sqrt(tau) + (rate + 0.5 * sigma * sigma) * tau)


def restate(vol, Kq, Tq, spot, deltas, rate=0.0, monotone=False):
    """Rules D1-D6.  vol [B,mT,mK]; Kq [mK] or [B,mK]; Tq [mT] or [B,mT]; spot [B].  Returns host arrays vol, strike
    (float64), flags (int32) of shape [B,mT,nD] and ia, ib (int64, -1 = no bracket): the node indices of the bracket.
    monotone=True asserts that h decreases strictly along every bracket's chord (9 samples)."""
    vol = np.asarray(vol, np.float64)
    B, mT, mK = vol.shape
    Kq = np.broadcast_to(np.asarray(Kq, np.float64), (B, mK))
    Tq = np.broadcast_to(np.asarray(Tq, np.float64), (B, mT))
    spot = np.asarray(spot, np.float64).reshape(B)
    z = np.array([z_of(d) for d in deltas], np.float64)
    nD = len(z)
    q_vol = np.full((B, mT, nD), np.nan)
    q_strike = np.full((B, mT, nD), np.nan)
    flags = np.full((B, mT, nD), DEAD, np.int32)
    ia = np.full((B, mT, nD), -1, np.int64)
    ib = np.full((B, mT, nD), -1, np.int64)
    with np.errstate(all="ignore"):
        for b in range(B):
            S = spot[b]
            if not (np.isfinite(S) and S > 0):
                continue                                                     # D2: dead row
            k_all = Kq[b]
            k_ok = np.isfinite(k_all) & (k_all > 0)
            for j in range(mT):
                tau = Tq[b, j]
                if not (np.isfinite(tau) and tau > 0):
                    continue
                s_all = vol[b, j]
                idx = np.flatnonzero(k_ok & np.isfinite(s_all) & (s_all > 0))   # D2: the valid nodes, in strike order
                if len(idx) < 2:
                    continue
                d1 = d1_of(S, k_all[idx], s_all[idx], rate, tau)
                h = d1[None, :] - z[:, None]                                  # [nD, valid nodes]
                cross = (h[:, :-1] >= 0) & (h[:, 1:] < 0)                     # D4
                n = cross.sum(1)
                first = cross.argmax(1)
                flags[b, j] = np.where(n == 0, NO_CROSSING, np.where(n > 1, AMBIGUOUS, OK))
                hit = n > 0
                ia[b, j, hit] = idx[first[hit]]
                ib[b, j, hit] = idx[first[hit] + 1]
        # D5 on every bracket at once
        bb, jj, tt = np.nonzero(ia >= 0)
        if len(bb):
            S, tau, zz = spot[bb], Tq[bb, jj], z[tt]
            ka, kb = Kq[bb, ia[bb, jj, tt]], Kq[bb, ib[bb, jj, tt]]
            sa, sb = vol[bb, jj, ia[bb, jj, tt]], vol[bb, jj, ib[bb, jj, tt]]

            def h_at(w):
                return d1_of(S, ka + w * (kb - ka), sa + w * (sb - sa), rate, tau) - zz
            if monotone:
                hs = np.stack([h_at(np.full(len(bb), w)) for w in np.linspace(0.0, 1.0, 9)])
                assert np.all(np.diff(hs, axis=0) < 0), "h is not monotone inside a bracket: the generator is at fault"
            lo, hi = np.zeros(len(bb)), np.ones(len(bb))
            for _ in range(STEPS):
                mid = 0.5 * (lo + hi)
                up = h_at(mid) >= 0
                lo = np.where(up, mid, lo)
                hi = np.where(up, hi, mid)
            w = 0.5 * (lo + hi)
            q_strike[bb, jj, tt] = ka + w * (kb - ka)
            q_vol[bb, jj, tt] = sa + w * (sb - sa)
    return {"vol": q_vol, "strike": q_strike, "flags": flags, "ia": ia, "ib": ib}


def delta_of(strike, vol, Tq, spot, rate=0.0):
    """Call delta norm_cdf(d1) of restated points [B,mT,nD] (math.erfc through NumPy's vectorize)."""
    import math
    B, mT, nD = strike.shape
    Tq = np.broadcast_to(np.asarray(Tq, np.float64), (B, mT))
    with np.errstate(all="ignore"):
        d1 = d1_of(np.asarray(spot, np.float64).reshape(B, 1, 1), strike, vol, rate, Tq[:, :, None])
    erfc = np.vectorize(lambda x: math.erfc(x) if x == x else math.nan, otypes=[np.float64])
    return 0.5 * erfc(-d1 * 0.70710678118654752440)


class RefBackend(snapshot_ref.RefBackend):
    """CPU stand-in for snapshots.HipBackend with the smile points restated."""

    def smile_points(self, vol, Kq, Tq, spot, deltas, rate):
        r = restate(vol, Kq, Tq, spot, deltas, rate)
        return {"vol": r["vol"], "strike": r["strike"], "flags": r["flags"]}
