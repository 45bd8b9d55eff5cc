"""Independent NumPy restatement of the arbitrage rules A1-A7.  TEST INFRASTRUCTURE ONLY.

Shares no code with iv_interpolation_amd: the whole batch is one [B, mT, mK] array and every neighbour is a shifted copy of
it (NaN / False shifted in at the borders), so there are no lanes, chunks or strips.  `dtype` selects the arithmetic: the
inputs are always float64 values; np.longdouble gives the same rules at higher precision (the rounding-level test).

    restate(vol, Kq, Tq, spot, rate=0.0, dtype=np.float64, margins=False) -> dict
        flags [B,mT,mK] int32, counts [B,4] int32, worst [B,2], local_vol, density, and per node N, g, d2, evaluated and
        the rounding scales w1_scale, w2_scale, wt_scale, N_scale, g_scale (sums of the absolute values of the terms)
        margins=True asserts |N| >= 1e-9 N_scale and |g| >= 1e-9 g_scale at every evaluated node and that >= 90 % of the
        interior nodes (strike index 1 .. mK-2) are evaluated
    RefBackend()  -> smile_ref.RefBackend plus arbitrage
"""
import numpy as np

import smile_ref

CALENDAR, BUTTERFLY, NO_STENCIL, DEAD = 1, 2, 4, 8
MARGIN = 1e-9


def _pos(a):
    return np.isfinite(a) & (a > 0)


def _shift(a, d, axis, fill):
    """b[..., n, ...] = a[..., n + d, ...] along `axis`, `fill` where n + d falls outside."""
    out = np.full(a.shape, fill, a.dtype)
    n = a.shape[axis]
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    if d > 0:
        src[axis], dst[axis] = slice(d, n), slice(0, n - d)
    else:
        src[axis], dst[axis] = slice(0, n + d), slice(-d, n)
    out[tuple(dst)] = a[tuple(src)]
    return out


def _d1_weights(hm, hp):
    return -hp / (hm * (hm + hp)), (hp - hm) / (hm * hp), hm / (hp * (hm + hp))


def restate(vol, Kq, Tq, spot, rate=0.0, dtype=np.float64, margins=False):
    f = dtype
    vol = np.asarray(vol, np.float64)
    B, mT, mK = vol.shape
    K = np.broadcast_to(np.asarray(Kq, np.float64), (B, mK)).astype(f)
    T = np.broadcast_to(np.asarray(Tq, np.float64), (B, mT)).astype(f)
    S = np.asarray(spot, np.float64).reshape(B).astype(f)
    s = vol.astype(f)
    r = f(rate)
    nan = f(np.nan)
    with np.errstate(all="ignore"):
        # A1
        live = _pos(S)[:, None] & _pos(T)                                   # [B, mT]
        valid = live[:, :, None] & _pos(K)[:, None, :] & _pos(s)
        # A2
        tau = T[:, :, None]
        w = s * s * tau
        gap = np.log1p((K[:, 1:] - K[:, :-1]) / K[:, :-1])                  # [B, mK-1]: spacing to the right of node i
        hp = np.concatenate([gap, np.full((B, 1), nan, f)], axis=1)[:, None, :]
        hm = np.concatenate([np.full((B, 1), nan, f), gap], axis=1)[:, None, :]
        y = np.log(K / S[:, None])[:, None, :] - r * tau
        # A3
        wl, wr = _shift(w, -1, 2, nan), _shift(w, 1, 2, nan)
        k_ok = _shift(valid, -1, 2, False) & _shift(valid, 1, 2, False) & (hm > 0) & (hp > 0)
        am, a0, ap = _d1_weights(hm, hp)
        bm, b0, bp = 2 / (hm * (hm + hp)), -2 / (hm * hp), 2 / (hp * (hm + hp))
        w1 = am * wl + a0 * w + ap * wr
        w2 = bm * wl + b0 * w + bp * wr
        w1_scale = np.abs(am * wl) + np.abs(a0 * w) + np.abs(ap * wr)
        w2_scale = np.abs(bm * wl) + np.abs(b0 * w) + np.abs(bp * wr)
        # A4
        t_up, t_dn = _shift(tau, 1, 1, nan), _shift(tau, -1, 1, nan)
        w_up, w_dn = _shift(w, 1, 1, nan), _shift(w, -1, 1, nan)
        up = _shift(valid, 1, 1, False) & (t_up > tau)
        dn = _shift(valid, -1, 1, False) & (t_dn < tau)
        dm, dp = tau - t_dn, t_up - tau
        cm, c0, cp = _d1_weights(dm, dp)
        both = cm * w_dn + c0 * w + cp * w_up
        both_scale = np.abs(cm * w_dn) + np.abs(c0 * w) + np.abs(cp * w_up)
        fwd, fwd_scale = (w_up - w) / dp, (np.abs(w_up) + np.abs(w)) / np.abs(dp)
        bwd, bwd_scale = (w_dn - w) / (t_dn - tau), (np.abs(w_dn) + np.abs(w)) / np.abs(t_dn - tau)
        wt = np.where(up & dn, both, np.where(up, fwd, bwd))
        wt_scale = np.where(up & dn, both_scale, np.where(up, fwd_scale, bwd_scale))
        ev = valid & k_ok & (up | dn)
        # A5
        N = wt + r * w1
        yw = y / w
        q = -f(0.25) - 1 / w + yw * yw
        g = 1 - yw * w1 + f(0.25) * q * (w1 * w1) + f(0.5) * w2
        N_scale = wt_scale + abs(r) * w1_scale
        g_scale = 1 + np.abs(yw) * w1_scale + f(0.5) * np.abs(q) * np.abs(w1) * w1_scale + f(0.5) * w2_scale
        cal, bfly = ev & (N < 0), ev & (g < 0)
        # A6
        lv = np.where(ev & (N >= 0) & (g > 0), np.sqrt(N / g), nan)
        sq = np.sqrt(w)
        d2 = -y / sq - f(0.5) * sq
        den = np.where(ev, g * np.exp(-f(0.5) * (d2 * d2)) / (K[:, None, :] * np.sqrt(f(6.283185307179586) * w)), nan)
        flags = np.where(~valid, DEAD, np.where(~ev, NO_STENCIL, cal * CALENDAR + bfly * BUTTERFLY)).astype(np.int32)
        # A7
        counts = np.stack([ev.sum((1, 2)), cal.sum((1, 2)), bfly.sum((1, 2)), np.isfinite(lv).sum((1, 2))], axis=1).astype(np.int32)
        inf = f(np.inf)
        worst = np.stack([np.fmin.reduce(np.where(ev, N, inf).reshape(B, -1), axis=1),
                          np.fmin.reduce(np.where(ev, g, inf).reshape(B, -1), axis=1)], axis=1)
        worst = np.where((counts[:, 0] > 0)[:, None], worst, nan)
    out = {"flags": flags, "counts": counts, "worst": worst, "local_vol": lv, "density": den, "N": np.where(ev, N, nan),
           "g": np.where(ev, g, nan), "d2": d2, "evaluated": ev, "w1_scale": w1_scale, "w2_scale": w2_scale,
           "wt_scale": wt_scale, "N_scale": N_scale, "g_scale": g_scale}
    if margins:
        assert np.all(np.abs(N[ev]) >= MARGIN * N_scale[ev]), "an evaluated node has N within 1e-9 of 0: the generator is at fault"
        assert np.all(np.abs(g[ev]) >= MARGIN * g_scale[ev]), "an evaluated node has g within 1e-9 of 0: the generator is at fault"
        share = ev[:, :, 1:-1].mean()
        assert share >= 0.9, f"only {share:.3f} of the interior nodes are evaluated: the generator is at fault"
    return out


class RefBackend(smile_ref.RefBackend):
    """CPU stand-in for snapshots.HipBackend with the arbitrage report restated."""

    def arbitrage(self, vol, Kq, Tq, spot, rate):
        r = restate(vol, Kq, Tq, spot, rate)
        return {k: r[k] for k in ("flags", "counts", "worst", "local_vol", "density")}
