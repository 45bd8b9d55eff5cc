"""NumPy restatement of rules T1-T4, C1-C6 and E1-E6: the calendar report between raw SVI slices and
the surface at any (strike, expiry).  TEST INFRASTRUCTURE ONLY: written from the rules, array-wise, with math.erfc as Phi; it
shares no code with the kernels.  Both restatements also return what the tolerances of the tests are built from (the error
scale of every value they compare, in units of eps) and, with margins=True, assert the conditions under which flags and NaN
patterns of two arithmetics must be equal.  `exact_calendar` / `exact_eval` are the same rules in mpmath."""
import numpy as np

import dist_ref as DR

CALENDAR, WING_LEFT, WING_RIGHT, DEAD, LAST, UNORDERED = 1, 2, 4, 8, 16, 32          # IVS_SC_*
SHORT, LONG, NEG_FWD, Q_DEAD, NEG_G, Q_UNORDERED = 1, 2, 4, 8, 16, 32                # IVS_SE_*
STEPS = 52
_T = np.arange(64) - 31.5
Y = _T * (1.0 + _T * _T / 1024.0) / 8.0                    # C1, exact in fp64
CAL_KEYS = ("d_min", "x_min", "d_atm", "x_cross", "n_cross", "flags")
EVAL_KEYS = ("w", "vol", "call", "put", "fwd_var", "g", "local_vol")
Phi, phi = DR.Phi, DR.phi


def curve(P, x, xerr=0.0):
    """T3 at x (broadcast against the rows of P [..., 5]): w, w', w'' and their error scales sw, sw1, sw2 in units of eps:
    the magnitudes of the terms each value is summed from, a few roundings each, plus the next derivative times `xerr`, the
    error of x itself in units of eps."""
    a, b, rho, m, sig = (P[..., q] for q in range(5))
    with np.errstate(all="ignore"):
        dx = x - m
        r = np.sqrt(dx * dx + sig * sig)
        w = a + b * (rho * dx + r)
        w1 = b * (rho + dx / r)
        w2 = b * sig * sig / (r * r * r)
        w3 = -3.0 * b * sig * sig * dx / r ** 5
        sw = np.abs(a) + 3.0 * b * (np.abs(rho * dx) + r) + np.abs(w1) * xerr
        sw1 = 3.0 * b * (np.abs(rho) + np.abs(dx) / r) + np.abs(w2) * xerr
        sw2 = 6.0 * np.abs(w2) + np.abs(w3) * xerr
    return dict(w=w, w1=w1, w2=w2, sw=sw, sw1=sw1, sw2=sw2)


def structure(params, Tq, spot):
    """T1, T2, T4: live [B,mT], unordered [B], nxt [B,mT] (the lowest live row above j, -1 = none)."""
    P = np.asarray(params, np.float64)
    B, mT, _ = P.shape
    assert mT <= 64
    S = np.broadcast_to(np.asarray(spot, np.float64).reshape(B, 1), (B, mT))
    tau = np.broadcast_to(np.asarray(Tq, np.float64), (B, mT))
    live = DR.live_rows(P, S, tau)
    nxt = np.full((B, mT), -1)
    unordered = np.zeros(B, bool)
    for b in range(B):
        last = -1
        for j in range(mT - 1, -1, -1):
            nxt[b, j] = last
            if live[b, j]:
                if last >= 0 and not tau[b, last] > tau[b, j]:
                    unordered[b] = True
                last = j
    return P, S, tau, live, unordered, nxt


def restate_calendar(params, Tq, spot, margins=False):
    """Rules T1-T4, C1-C6 on params [B,mT,5], Tq [mT] or [B,mT], spot [B].  Returns the kernel's outputs (CAL_KEYS) and, for
    the tests: live, pair [B,mT] (rows with a pair), nxt, index (of the minimum among the 66 points), cells [B,mT,2] (-1 =
    none), s0, d66 / x66 [B,mT,66], scale_min / scale_atm / scale_x (error scales of d_min, d_atm, x_min in units of eps),
    cross_scale / cross_slope / width [B,mT,2] (error scale of d and d' at the crossing, the cell's width), gap (second
    smallest d minus the smallest) and w0 = w_j'(0)."""
    P, S, tau, live, unordered, nxt = structure(params, Tq, spot)
    B, mT, _ = P.shape
    pair = live & (nxt >= 0) & ~unordered[:, None]
    jp = np.maximum(nxt, 0)
    Pl = np.where(pair[..., None], P, np.nan)
    Ph = np.where(pair[..., None], np.take_along_axis(P, jp[..., None], axis=1), np.nan)
    with np.errstate(all="ignore"):
        c0l, c0h = curve(Pl, 0.0), curve(Ph, 0.0)
        top = np.maximum(c0l["w"], c0h["w"])
        s0 = np.sqrt(top)                                                     # C1
        xrel = np.maximum(c0l["sw"], c0h["sw"]) / (2.0 * top) + 2.0           # relative error of s0 and of s0 y, in eps
        xg = s0[..., None] * Y
        x66 = np.concatenate([xg, Pl[..., 3:4], Ph[..., 3:4]], axis=-1)       # C2: the grid, m_j, m_j'
        xerr = np.concatenate([np.abs(xg) * xrel[..., None], np.zeros((B, mT, 2))], axis=-1)
        cl, ch = curve(Pl[:, :, None, :], x66, xerr), curve(Ph[:, :, None, :], x66, xerr)
        d66 = ch["w"] - cl["w"]
        s66 = ch["sw"] + cl["sw"] + np.abs(d66)
        key = np.where(np.isnan(d66), np.inf, d66)
        index = key.argmin(axis=-1)                                           # ties: the lowest index
        pick = lambda a: np.take_along_axis(a, index[..., None], axis=-1)[..., 0]   # noqa: E731
        d_min, x_min = pick(d66), pick(x66)
        d_atm = c0h["w"] - c0l["w"]
        neg = d66[..., :64] < 0                                               # C3
        cell = neg[..., :-1] != neg[..., 1:]
        n_cross = np.where(pair, cell.sum(axis=-1), 0).astype(np.int32)
        first, last = cell.argmax(axis=-1), 62 - cell[..., ::-1].argmax(axis=-1)
        cells = np.where((n_cross > 0)[..., None], np.stack([first, last], axis=-1), -1)
        i0 = np.maximum(cells, 0)
        sign = np.take_along_axis(neg, i0, axis=-1)
        lo, hi = s0[..., None] * Y[i0], s0[..., None] * Y[i0 + 1]
        width = hi - lo
        Plc, Phc = Pl[:, :, None, :], Ph[:, :, None, :]
        for _ in range(STEPS):                                                # C4
            mid = 0.5 * (lo + hi)
            same = ((curve(Phc, mid)["w"] - curve(Plc, mid)["w"]) < 0) == sign
            lo, hi = np.where(same, mid, lo), np.where(same, hi, mid)
        x_cross = np.where(cells >= 0, 0.5 * (lo + hi), np.nan)
        xe = np.abs(x_cross) * xrel[..., None]
        rl, rh = curve(Plc, x_cross, xe), curve(Phc, x_cross, xe)
        bl, rl_, bh, rh_ = Pl[..., 1], Pl[..., 2], Ph[..., 1], Ph[..., 2]
        wl = bh * (1.0 - rh_) < bl * (1.0 - rl_)                              # C5
        wr = bh * (1.0 + rh_) < bl * (1.0 + rl_)
        flags = np.where(d_min < 0, CALENDAR, 0) | np.where(wl, WING_LEFT, 0) | np.where(wr, WING_RIGHT, 0)
        flags = np.where(pair, flags, np.where(live, LAST, DEAD))
        flags = np.where(unordered[:, None], UNORDERED, flags).astype(np.int32)
        srt = np.sort(key, axis=-1)
        gap = srt[..., 1] - srt[..., 0]
    out = dict(d_min=d_min, x_min=x_min, d_atm=d_atm, x_cross=x_cross, n_cross=n_cross, flags=flags,
               live=live, pair=pair, nxt=nxt, unordered=unordered, index=np.where(pair, index, -1), cells=cells, s0=s0, d66=d66, x66=x66,
               scale_min=pick(s66), scale_atm=c0h["sw"] + c0l["sw"] + np.abs(d_atm), scale_x=np.abs(x_min) * xrel,
               cross_scale=rl["sw"] + rh["sw"], cross_slope=rh["w1"] - rl["w1"], cross_xrel=np.abs(x_cross) * xrel[..., None],
               width=np.where(cells >= 0, width, np.nan), gap=gap, w0=c0h["w"],
               wing=np.stack([bh * (1.0 - rh_) - bl * (1.0 - rl_), bh * (1.0 + rh_) - bl * (1.0 + rl_)], axis=-1),
               wing_scale=np.maximum(bh, bl))
    if margins:
        check_calendar_margins(out)
    return out


def check_calendar_margins(r):
    """The conditions for generated batches: no comparison of the rules sits on a threshold, and the batch is neither mostly
    NaN nor all one verdict."""
    live, pair = r["live"], r["pair"]
    mT = live.shape[1]
    assert live.mean() >= 0.9, f"only {live.mean():.0%} of the rows are live"
    if not pair.any():
        return
    floor = 1e-9 * r["w0"][pair]
    assert (np.abs(r["d66"][pair]) >= floor[:, None]).all(), "a point of the difference sits on 0"
    assert (r["gap"][pair] >= floor).all(), "two points tie for the minimum"
    assert (np.abs(r["wing"][pair]) >= 1e-9 * r["wing_scale"][pair][:, None]).all(), "two wing slopes tie"
    if mT >= 13:
        share = ((r["flags"][pair] & CALENDAR) != 0).mean()
        assert 0.1 <= share <= 0.9, f"{share:.0%} of the live pairs are flagged CALENDAR"


def restate_eval(params, Tq, spot, rate, u, tau_q, strike_mode=0, margins=False):
    """Rules T1-T3, E1-E6 on params [B,mT,5], Tq [mT] or [B,mT], spot [B], queries u, tau_q [Q] or [B,Q].  Returns the kernel's
    outputs (EVAL_KEYS and flags, each [B,Q]) and, for the tests: lo, hi [B,Q] (-1 = none), x, lam and scale_<key>, the error
    scale of every value in units of eps."""
    P, S, tau, live, unordered, _ = structure(params, Tq, spot)
    B, mT, _ = P.shape
    u = np.asarray(u, np.float64)
    Q = u.shape[-1]
    u, tq = np.broadcast_to(u, (B, Q)), np.broadcast_to(np.asarray(tau_q, np.float64), (B, Q))
    Sq = S[:, :1]
    with np.errstate(all="ignore"):
        tl = np.where(live, tau, np.nan)[:, None, :]                          # a dead row is picked by no comparison
        le, gt = tl <= tq[..., None], tl > tq[..., None]                      # E2
        lo = np.where(le.any(axis=-1), mT - 1 - le[..., ::-1].argmax(axis=-1), -1)
        hi = np.where(gt.any(axis=-1), gt.argmax(axis=-1), -1)
        pos = lambda v: np.isfinite(v) & (v > 0)                              # noqa: E731
        ok = pos(u) & pos(tq) & pos(Sq) & live.any(axis=1)[:, None] & ~unordered[:, None]      # E1
        lo, hi = np.where(ok, lo, -1), np.where(ok, hi, -1)
        both, short, long_ = (lo >= 0) & (hi >= 0), ok & (lo < 0), ok & (hi < 0)
        K = Sq * u if strike_mode == 0 else u
        rt = rate * tq
        F, D = Sq * np.exp(rt), np.exp(-rt)
        lk = np.log(K / Sq)
        x = np.where(ok, lk - rt, np.nan)
        xs = 2.0 + np.abs(lk) + 2.0 * np.abs(rt)                              # the error of x in units of eps
        one = np.where(lo >= 0, lo, np.maximum(hi, 0))                        # the only slice under SHORT / LONG
        ia, ic = np.where(both, lo, one), np.where(both, hi, one)
        gather = lambda a, i: a[np.arange(B)[:, None], i]                     # noqa: E731
        ca, cc = curve(gather(P, ia), x, xs), curve(gather(P, ic), x, xs)
        ta, tc = gather(tau, ia), gather(tau, ic)
        dt = tc - ta
        lam = np.where(both, (tq - ta) / dt, 0.0)                             # E3
        sc = tq / ta
        val, scale = {}, {}
        for k, sk in (("w", "sw"), ("w1", "sw1"), ("w2", "sw2")):
            val[k] = np.where(both, ca[k] + (cc[k] - ca[k]) * lam, ca[k] * sc)
            scale[k] = np.where(both, ca[sk] * (1.0 + lam) + cc[sk] * lam + 5.0 * np.abs(cc[k] - ca[k]) * lam, ca[sk] * sc + np.abs(val[k])) + np.abs(val[k])
        W, W1, W2 = (np.where(ok, val[k], np.nan) for k in ("w", "w1", "w2"))
        SW, SW1, SW2 = scale["w"], scale["w1"], scale["w2"]
        V = np.where(ok, np.where(both, (cc["w"] - ca["w"]) / dt, ca["w"] / ta), np.nan)
        SV = np.where(both, (ca["sw"] + cc["sw"]) / dt, ca["sw"] / ta) + 3.0 * np.abs(V)
        th = np.sqrt(W)                                                       # E4
        d1 = -x / th + 0.5 * th
        d2 = d1 - th
        vol = np.sqrt(W / tq)
        call = D * (F * Phi(d1) - K * Phi(d2))
        put = D * (K * Phi(-d2) - F * Phi(-d1))
        dth = SW / (2.0 * th) + th
        dd1 = xs / th + np.abs(x) / (th * th) * dth + np.abs(x) / th + 0.5 * dth + np.abs(d1)
        dd2 = dd1 + dth + np.abs(d2)
        fF = 3.0 + 2.0 * np.abs(rt)
        s_phi = lambda d, dd: (2.0 + fF) * Phi(d) + phi(d) * dd               # noqa: E731
        S_call = D * (F * s_phi(d1, dd1) + K * s_phi(d2, dd2)) + np.abs(call) * fF
        S_put = D * (F * s_phi(-d1, dd1) + K * s_phi(-d2, dd2)) + np.abs(put) * fF
        t = x * W1 / (2.0 * W)                                                # E5
        h = 1.0 - t
        A, c1, c2, Cq = h * h, W1 * W1 / 4.0, 1.0 / W + 0.25, W2 / 2.0
        g = A - c1 * c2 + Cq
        dtt = 4.0 * np.abs(t) + (xs * np.abs(W1) + np.abs(x) * SW1) / (2.0 * W) + np.abs(t) * SW / W
        Sg = 2.0 * np.abs(h) * (dtt + np.abs(h)) + A + (np.abs(W1) * SW1 / 2.0 + 2.0 * c1) * c2 + c1 * (SW / (W * W) + 2.0 * c2) + c1 * c2 \
            + SW2 / 2.0 + A + c1 * c2 + np.abs(Cq)
        fine = ok & ~(V < 0) & ~(g <= 0)
        lv = np.where(fine, np.sqrt(V / g), np.nan)
        S_lv = lv * (SV / (2.0 * np.abs(V)) + Sg / (2.0 * np.abs(g)) + 2.0)
        flags = np.where(short, SHORT, 0) | np.where(long_, LONG, 0) | np.where(ok & (V < 0), NEG_FWD, 0) | np.where(ok & (g <= 0), NEG_G, 0)
        flags = np.where(ok, flags, Q_DEAD)
        flags = np.where(unordered[:, None], Q_UNORDERED, flags).astype(np.int32)
    nan = lambda a: np.where(ok, a, np.nan)                                   # noqa: E731
    out = dict(w=W, vol=nan(vol), call=nan(call), put=nan(put), fwd_var=V, g=nan(g), local_vol=lv, flags=flags,
               ok=ok, lo=lo, hi=hi, x=x, lam=lam, K=K, F=F, D=D, d1=d1, d2=d2, live=live, unordered=unordered,
               scale_w=SW, scale_vol=vol * (SW / (2.0 * W) + 2.0), scale_call=S_call, scale_put=S_put, scale_fwd_var=SV, scale_g=Sg,
               scale_local_vol=S_lv, v_floor=(np.abs(ca["w"]) + np.abs(cc["w"])) / np.where(both, dt, ta), g_floor=A + c1 * c2 + np.abs(Cq))
    if margins:
        check_eval_margins(out)
    return out


def check_eval_margins(r):
    ok = r["ok"]
    assert r["live"].mean() >= 0.9, f"only {r['live'].mean():.0%} of the rows are live"
    if ok.any():
        assert (np.abs(r["fwd_var"][ok]) >= 1e-9 * r["v_floor"][ok]).all(), "a forward variance sits on 0"
        assert (np.abs(r["g"][ok]) >= 1e-9 * r["g_floor"][ok]).all(), "a g sits on 0"


class RefBackend(DR.RefBackend):
    """CPU stand-in for snapshots.HipBackend with the calendar report and the evaluation restated."""

    def calendar(self, params, Tq, spot):
        r = restate_calendar(params, Tq, spot)
        return {k: r[k] for k in CAL_KEYS}

    def evaluate(self, params, Tq, spot, rate, u, tau, strike_mode):
        r = restate_eval(params, Tq, spot, rate, u, tau, strike_mode)
        return {k: r[k] for k in EVAL_KEYS + ("flags",)}


# ------------------------------------------------------------------ the same rules in mpmath
def _mp_curve(mp, p5, x):
    a, b, rho, m, sig = p5
    dx = x - m
    r = mp.sqrt(dx * dx + sig * sig)
    return a + b * (rho * dx + r), b * (rho + dx / r), b * sig * sig / (r * r * r)


def exact_calendar(c, ref, dps=50):
    """d_min (at the restatement's index), x_min, d_atm and x_cross (the root of d in the restatement's cell, to 1e-40) of
    every pair of `ref` in mpmath at `dps` digits, rounded to fp64 at the end.  A cell whose sign change mpmath does not see is
    rounding's and is left NaN."""
    import mpmath as mp
    P = np.asarray(c["params"], np.float64)
    out = {k: np.full(np.shape(ref[k]), np.nan) for k in ("d_min", "x_min", "d_atm", "x_cross")}
    with mp.workdps(dps):
        f = mp.mpf
        for b, j in zip(*np.nonzero(ref["pair"])):
            lo5, hi5 = [f(float(v)) for v in P[b, j]], [f(float(v)) for v in P[b, ref["nxt"][b, j]]]
            d = lambda x: _mp_curve(mp, hi5, x)[0] - _mp_curve(mp, lo5, x)[0]     # noqa: E731
            s0 = mp.sqrt(max(_mp_curve(mp, lo5, f(0))[0], _mp_curve(mp, hi5, f(0))[0]))
            i = int(ref["index"][b, j])
            x = s0 * f(float(Y[i])) if i < 64 else (lo5[3] if i == 64 else hi5[3])
            out["d_min"][b, j], out["x_min"][b, j], out["d_atm"][b, j] = float(d(x)), float(x), float(d(f(0)))
            for q in range(2):
                i = int(ref["cells"][b, j, q])
                if i < 0:
                    continue
                lo, hi = s0 * f(float(Y[i])), s0 * f(float(Y[i + 1]))
                if not (d(lo) < 0) != (d(hi) < 0):
                    continue
                out["x_cross"][b, j, q] = float(mp.findroot(d, (lo, hi), solver="anderson", tol=1e-40, maxsteps=200))
    return out


def exact_eval(c, ref, dps=50):
    """Every value of every live query of `ref` in mpmath at `dps` digits, with the restatement's bracket (lo, hi) and its
    verdicts on V and g; rounded to fp64 at the end."""
    import mpmath as mp
    P = np.asarray(c["params"], np.float64)
    B, mT, _ = P.shape
    tau = np.broadcast_to(np.asarray(c["Tq"], np.float64), (B, mT))
    Q = np.asarray(c["u"]).shape[-1]
    uq, tq = np.broadcast_to(np.asarray(c["u"], np.float64), (B, Q)), np.broadcast_to(np.asarray(c["tau"], np.float64), (B, Q))
    out = {k: np.full((B, Q), np.nan) for k in EVAL_KEYS}
    with mp.workdps(dps):
        f = mp.mpf
        sqrt2 = mp.sqrt(2)
        Phi_ = lambda z: mp.erfc(-z / sqrt2) / 2                                 # noqa: E731
        for b, q in zip(*np.nonzero(ref["ok"])):
            S, t, rate = f(float(c["spot"][b])), f(float(tq[b, q])), f(float(c["rate"]))
            K = S * f(float(uq[b, q])) if c["strike_mode"] == 0 else f(float(uq[b, q]))
            F, D, x = S * mp.exp(rate * t), mp.exp(-rate * t), mp.log(K / S) - rate * t
            lo, hi = int(ref["lo"][b, q]), int(ref["hi"][b, q])
            if lo >= 0 and hi >= 0:
                ta, tc = f(float(tau[b, lo])), f(float(tau[b, hi]))
                wa, wc = _mp_curve(mp, [f(float(v)) for v in P[b, lo]], x), _mp_curve(mp, [f(float(v)) for v in P[b, hi]], x)
                lam = (t - ta) / (tc - ta)
                W, W1, W2 = (wa[k] + (wc[k] - wa[k]) * lam for k in range(3))
                V = (wc[0] - wa[0]) / (tc - ta)
            else:
                i = lo if lo >= 0 else hi
                ta = f(float(tau[b, i]))
                wa = _mp_curve(mp, [f(float(v)) for v in P[b, i]], x)
                W, W1, W2 = (wa[k] * t / ta for k in range(3))
                V = wa[0] / ta
            th = mp.sqrt(W)
            d1 = -x / th + th / 2
            d2 = d1 - th
            g = (1 - x * W1 / (2 * W)) ** 2 - (W1 * W1 / 4) * (1 / W + f(1) / 4) + W2 / 2
            out["w"][b, q], out["vol"][b, q], out["fwd_var"][b, q], out["g"][b, q] = float(W), float(mp.sqrt(W / t)), float(V), float(g)
            out["call"][b, q] = float(D * (F * Phi_(d1) - K * Phi_(d2)))
            out["put"][b, q] = float(D * (K * Phi_(-d2) - F * Phi_(-d1)))
            if np.isfinite(ref["local_vol"][b, q]) and V >= 0 and g > 0:
                out["local_vol"][b, q] = float(mp.sqrt(V / g))
    return out
