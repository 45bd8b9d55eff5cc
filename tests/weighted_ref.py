"""NumPy restatement of rules W0-W9: age-weighted, volatility-scaled historical-simulation VaR and expected
shortfall.  TEST INFRASTRUCTURE ONLY: written from the rules on top of hsim_ref.tail's ordering (a stable argsort: ties to the lower s,
-0.0 == +0.0) and risk_ref.b5_sum (W5: the order of the sums); it shares no code with the kernels.  The definition is this
repository's own: there is no reference counterpart.  W3-W8 are a fixed sequence of IEEE operations under a total order, so the
kernel has to reproduce them to the bit once both are given the same sigma; sigma itself ends in a square root, which the device
computes within 1 ulp.  `walk` is W7 as the rule reads, one rank at a time, for the tables by hand; `weighted` forms the same sums
with serial accumulations."""
import numpy as np

import boot_ref as BR
import risk_ref as R

NO_VOL, BAD_WEIGHT = 8, 16                                                           # IVS_HW_*
MAX_SPAN = 1024
OUT_KEYS = ("var_w", "es_w", "n_valid_w", "worst_w", "wsum", "n_eff", "pnl_w", "scale", "flags_w", "sigma")
TAIL_KEYS = OUT_KEYS[:-1]


def _fpos(x):
    with np.errstate(invalid="ignore"):
        return np.isfinite(x) & (x > 0)


def age_weights(window, decay):
    """w_0 = 1.0, w_{s+1} = w_s x decay: the repeated multiplication engine.age_weights makes."""
    w, x = np.empty(int(window)), np.float64(1.0)
    for s in range(int(window)):
        w[s] = x
        x = x * np.float64(decay)
    return w


def returns(spot):
    """W1: r [B] (r[0] unused) and its validity."""
    spot = np.asarray(spot, np.float64)
    r, ok = np.full(len(spot), np.nan), np.zeros(len(spot), bool)
    with np.errstate(all="ignore"):
        r[1:] = spot[1:] / spot[:-1] - 1.0
    ok[1:] = _fpos(spot[1:]) & _fpos(spot[:-1]) & np.isfinite(r[1:])
    return r, ok


def ewma_sigma(spot, vol_weight, min_returns):
    """W2: sigma [B].  The terms in ascending k, serially from +0.0; a term left out leaves both sums as they are."""
    a = np.asarray(vol_weight, np.float64)
    r, ok = returns(spot)
    B = len(r)
    num, den, cnt, bad = np.zeros(B), np.zeros(B), np.zeros(B, np.int64), np.zeros(B, bool)
    j = np.arange(B)
    with np.errstate(all="ignore"):
        for k in range(min(len(a), B)):
            i = j - k
            take = (i >= 1) & ok[np.maximum(i, 0)]
            rr = r[np.maximum(i, 0)]
            num = np.where(take, num + a[k] * (rr * rr), num)
            den = np.where(take, den + a[k], den)
            cnt += take
            bad |= take & (not (np.isfinite(a[k]) and a[k] >= 0))
        q = num / den
        good = (cnt >= int(min_returns)) & ~bad & _fpos(q)
        return np.where(good, np.sqrt(q), np.nan)


def walk(z, w, tp, W):
    """W7 as the rule reads on one row's ranked z and w (rank order): (var_w, es_w, whether a rank reached the target)."""
    n = len(z)
    with np.errstate(all="ignore"):
        target = np.float64(tp) * np.float64(W)
        cum, s, star, reached = np.float64(0.0), np.float64(0.0), n - 1, False
        for rho in range(n):
            nxt = cum + w[rho]
            if nxt >= target:
                star, reached = rho, True
                break
            s = s + w[rho] * z[rho]
            cum = nxt
        s = s + (target - cum) * z[star]
        return np.float64(0.0) - z[star], np.float64(0.0) - s / target, reached


def _tail(z, w, tp, W):
    """W7 with serial accumulations in the place of the loop: the same operations in the same order."""
    n = len(z)
    with np.errstate(all="ignore"):
        target = np.float64(tp) * np.float64(W)
        cum = np.add.accumulate(np.concatenate([[0.0], w]))                                  # cum[k]: the weight below rank k
        hit = np.flatnonzero(cum[1:] >= target)
        reached = len(hit) > 0
        star = int(hit[0]) if reached else n - 1
        upto = star if reached else n
        s = np.add.accumulate(np.concatenate([[0.0], w[:upto] * z[:upto]]))[-1]
        s = s + (target - cum[upto]) * z[star]
        return np.float64(0.0) - z[star], np.float64(0.0) - s / target, reached


def weighted(pnl, scen_flags, spot=None, lag=1, tail_probs=(0.05, 0.01), min_scen=20, weight=None, vol_span=0, vol_weight=None,
             min_returns=20, scale_cap=3.0, stages=0, sigma=None):
    """Rules W0-W9.  Returns the outputs of OUT_KEYS (sigma None with vol_span == 0; at stages 1 sigma alone), and for the tests
    active [B], reached [B,nL] and ranked [B,window]."""
    pnl, fl = np.asarray(pnl, np.float64), np.asarray(scen_flags, np.int32)
    B, window = pnl.shape
    tp = np.asarray(tail_probs, np.float64).reshape(-1)
    nL, M = len(tp), int(vol_span)
    assert 1 <= window <= 1024 and lag >= 1 and nL <= 8 and min_scen >= 1 and 0 <= M <= MAX_SPAN and stages in (0, 1, 2)
    assert ((tp > 0) & (tp < 1)).all()
    if M > 0:
        assert 1 <= min_returns <= M and np.isfinite(scale_cap) and scale_cap >= 1
        if stages != 2:
            vw = np.asarray(vol_weight, np.float64)
            assert vw.shape == (M,) and len(spot) == B
            sigma = ewma_sigma(spot, vw, min_returns)
        sigma = np.asarray(sigma, np.float64)
    else:
        sigma = None
    if stages == 1:
        return dict(sigma=sigma)
    w = np.ones(window) if weight is None else np.asarray(weight, np.float64)
    assert w.shape == (window,)
    c, cap_lo = np.float64(scale_cap), np.float64(1.0) / np.float64(scale_cap)
    s = np.arange(window)
    with np.errstate(invalid="ignore"):
        w_ok = np.isfinite(w) & (w >= 0)
    out = dict(var_w=np.full((B, nL), np.nan), es_w=np.full((B, nL), np.nan), n_valid_w=np.zeros(B, np.int32), worst_w=np.full(B, -1, np.int32),
               wsum=np.zeros(B), n_eff=np.full(B, np.nan), pnl_w=np.full((B, window), np.nan), scale=np.full((B, window), np.nan),
               flags_w=np.zeros((B, window), np.int32), sigma=sigma, active=np.zeros(B, bool), reached=np.ones((B, nL), bool),
               ranked=np.zeros((B, window), bool))
    for p in range(B):
        v = pnl[p]
        bits = np.where(w_ok, 0, BAD_WEIGHT).astype(np.int32)
        with np.errstate(all="ignore"):
            if M > 0:                                                                        # W3
                j = p - int(lag) - s
                sj = np.where(j >= 0, sigma[np.maximum(j, 0)], np.nan)
                formed = (j >= 0) & _fpos(sigma[p]) & _fpos(sj)
                f = np.where(formed, np.minimum(np.maximum(sigma[p] / sj, cap_lo), c), np.nan)
                z = np.where(formed, v * f, v)
                bits |= np.where(formed, 0, NO_VOL).astype(np.int32)
            else:
                f, z = np.ones(window), v
            ranked = (fl[p] == 0) & (bits == 0) & ~np.isnan(z)                               # W4
            Wm = R.b5_sum(np.where(ranked, w, 0.0))                                          # W5
            W2 = R.b5_sum(np.where(ranked, w * w, 0.0))
            out["n_eff"][p] = (Wm * Wm) / W2 if W2 > 0 else np.nan
        idx = np.flatnonzero(ranked)
        n = len(idx)
        order = idx[np.argsort(z[idx], kind="stable")]                                       # -0.0 == +0.0: the lower s first
        out["flags_w"][p], out["scale"][p], out["pnl_w"][p], out["ranked"][p] = fl[p] | bits, f, np.where(ranked, z, np.nan), ranked
        out["n_valid_w"][p], out["wsum"][p] = n, Wm
        if n:
            out["worst_w"][p] = order[0]
        out["active"][p] = n >= min_scen and n > 0 and bool(np.isfinite(Wm)) and Wm > 0     # W6
        if out["active"][p]:
            for l, t in enumerate(tp):
                out["var_w"][p, l], out["es_w"][p, l], out["reached"][p, l] = _tail(z[order], w[order], t, Wm)
    return out


class RefBackend(BR.RefBackend):
    """CPU stand-in for a device backend with the weighted tail restated."""

    def weighted(self, pnl, scen_flags, spot, lag, tail_probs, min_scen, weight, vol_span, vol_weight, min_returns, scale_cap):
        r = weighted(pnl, scen_flags, spot, lag, tail_probs, min_scen, weight, vol_span, vol_weight, min_returns, scale_cap)
        return {k: r[k] for k in OUT_KEYS}
