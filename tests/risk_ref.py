"""NumPy restatement of rules G0-G6 and B1-B5: smile-aware Greeks per option, net Greeks and the
scenario P&L grid of a book per snapshot.  TEST INFRASTRUCTURE ONLY: written from the rules, array-wise, with math.erfc as Phi;
it shares no code with the kernels.  The definition is this repository's own: there is no reference counterpart.  Both
restatements also return the error scale of every value they compare, in units of eps (first-order propagation through the
rule's own terms), and, with margins=True, assert the conditions under which flags and NaN patterns of two arithmetics must be
equal.  `exact_greeks` / `exact_book` are the same rules in mpmath."""
import numpy as np

import cal_ref as CR

SHORT, LONG, NEG_FWD, Q_DEAD, NEG_G, Q_UNORDERED = 1, 2, 4, 8, 16, 32                # IVS_SE_*
NEG_VOL_SS, NEG_VOL_SM = 1, 2                                                        # IVS_SB_*
GREEK_KEYS = ("price", "delta_ss", "delta_sm", "gamma_ss", "gamma_sm", "vega", "theta")
NET_KEYS = GREEK_KEYS + ("gross",)
BOOK_KEYS = ("net", "n_dead", "pnl_ss", "pnl_sm", "cell_flags")
PASS = 256                                                                           # options per pass of rule B5
Phi, phi = CR.Phi, CR.phi


def depth(Q):
    """L of rule B5: six levels of the butterfly, two across the wavefronts, one per pass of 256 options."""
    return 8 + max(1, -(-int(Q) // PASS))


def b5_sum(terms):
    """Rule B5 along the last axis (the options): per pass of 256 the xor butterfly 32, 16, 8, 4, 2, 1 inside each group of 64,
    the four groups as (s0 + s1) + (s2 + s3), the passes in turn from +0.0.  Absent lanes add +0.0."""
    t = np.asarray(terms, np.float64)
    Q = t.shape[-1]
    n = max(1, -(-Q // PASS))
    pad = np.zeros(t.shape[:-1] + (n * PASS,))
    pad[..., :Q] = t
    v = pad.reshape(t.shape[:-1] + (n, 4, 64))
    with np.errstate(all="ignore"):
        for s in (32, 16, 8, 4, 2, 1):
            v = v[..., :s] + v[..., s:2 * s]
        w = (v[..., 0, 0] + v[..., 1, 0]) + (v[..., 2, 0] + v[..., 3, 0])
        tot = np.zeros(t.shape[:-1])
        for k in range(n):
            tot = tot + w[..., k]
    return tot


def _pos(v):
    return np.isfinite(v) & (v > 0)


def locate(params, Tq, spot, rate, u, tau_q, strike_mode):
    """Rules T1-T3, E1-E3: where every option sits.  Everything [B,Q]."""
    P, S, tau, live, unordered, _ = CR.structure(params, Tq, spot)
    B, mT, _ = P.shape
    u = np.asarray(u, np.float64)
    Q = u.shape[-1]
    u, tq = np.broadcast_to(u, (B, Q)), np.broadcast_to(np.asarray(tau_q, np.float64), (B, Q))
    Sq = np.broadcast_to(S[:, :1], (B, Q))
    with np.errstate(all="ignore"):
        tl = np.where(live, tau, np.nan)[:, None, :]
        le, gt = tl <= tq[..., None], tl > tq[..., None]
        lo = np.where(le.any(axis=-1), mT - 1 - le[..., ::-1].argmax(axis=-1), -1)
        hi = np.where(gt.any(axis=-1), gt.argmax(axis=-1), -1)
        ok = _pos(u) & _pos(tq) & _pos(Sq) & live.any(axis=1)[:, None] & ~unordered[:, None]
        lo, hi = np.where(ok, lo, -1), np.where(ok, hi, -1)
        both, short, long_ = (lo >= 0) & (hi >= 0), ok & (lo < 0), ok & (hi < 0)
        K = Sq * u if strike_mode == 0 else u
        rt = rate * tq
        D = np.exp(-rt)
        lk = np.log(K / Sq)
        x = np.where(ok, lk - rt, np.nan)
        xs = 2.0 + np.abs(lk) + 2.0 * np.abs(rt)
        one = np.where(lo >= 0, lo, np.maximum(hi, 0))
        ia, ic = np.where(both, lo, one), np.where(both, hi, one)
        gather = lambda a, i: a[np.arange(B)[:, None], i]                     # noqa: E731
        Pa, Pc, ta, tc = gather(P, ia), gather(P, ic), gather(tau, ia), gather(tau, ic)
        lam = np.where(both, (tq - ta) / (tc - ta), tq / ta)
        flags = np.where(short, SHORT, 0) | np.where(long_, LONG, 0)
        flags = np.where(ok, flags, Q_DEAD)
        flags = np.where(unordered[:, None], Q_UNORDERED, flags).astype(np.int32)
    return dict(ok=ok, both=both, lo=lo, hi=hi, K=K, rt=rt, D=D, x=x, xs=xs, Pa=Pa, Pc=Pc, ta=ta, tc=tc, lam=lam, S=Sq, tq=tq, flags=flags,
                live=live, unordered=unordered, degenerate=unordered | ~live.any(axis=1), B=B, Q=Q)


def surface(L, x, xs, derivs=False):
    """Rule E3 at x (broadcast against the options, extra trailing axes allowed): W and its scale, with derivs=True also W',
    W'', V and theirs."""
    ex = (Ellipsis,) + (None,) * (np.ndim(x) - 2)
    Pa, Pc = L["Pa"][(slice(None), slice(None)) + (None,) * (np.ndim(x) - 2)], L["Pc"][(slice(None), slice(None)) + (None,) * (np.ndim(x) - 2)]
    both, lam, ta, tc = L["both"][ex], L["lam"][ex], L["ta"][ex], L["tc"][ex]
    with np.errstate(all="ignore"):
        ca, cc = CR.curve(Pa, x, xs), CR.curve(Pc, x, xs)
        out = {}
        for k, sk in (("w", "sw"), ("w1", "sw1"), ("w2", "sw2")):
            val = np.where(both, ca[k] + (cc[k] - ca[k]) * lam, ca[k] * lam)
            out[k] = val
            out[sk] = np.where(both, ca[sk] * (1.0 + lam) + cc[sk] * lam + 5.0 * np.abs(cc[k] - ca[k]) * lam, ca[sk] * lam + np.abs(val)) + np.abs(val)
            if not derivs:
                break
        if derivs:
            dt = tc - ta
            out["v"] = np.where(both, (cc["w"] - ca["w"]) / dt, ca["w"] / ta)
            out["sv"] = np.where(both, (ca["sw"] + cc["sw"]) / dt, ca["sw"] / ta) + 3.0 * np.abs(out["v"])
            out["v_floor"] = (np.abs(ca["w"]) + np.abs(cc["w"])) / np.where(both, dt, ta)
    return out


def sigma(L, x, xs):
    """sqrt(W / tau) at x with a placement's bracket and weight, and its scale: the one function of rules X8 and H2."""
    s = surface(L, x, xs)
    with np.errstate(all="ignore"):
        sig = np.sqrt(s["w"] / L["tq"])
        return sig, sig * (s["sw"] / (2.0 * s["w"]) + 2.0)


def price(S, fS, KD, fKD, x, xs, th, dth, put):
    """Rule G1 at (S, x, theta) and its scale; fS, fKD: the relative errors of S and K D, dth: the error of theta, in eps."""
    with np.errstate(all="ignore"):
        d1 = -x / th + 0.5 * th
        d2 = d1 - th
        dd1 = xs / th + np.abs(x) / (th * th) * dth + np.abs(x) / th + 0.5 * dth + np.abs(d1)
        dd2 = dd1 + dth + np.abs(d2)
        call = S * Phi(d1) - KD * Phi(d2)
        putv = KD * Phi(-d2) - S * Phi(-d1)
        s_phi = lambda d, dd, f: (3.0 + f) * Phi(d) + phi(d) * dd             # noqa: E731
        s_call = S * s_phi(d1, dd1, fS) + KD * s_phi(d2, dd2, fKD) + np.abs(call)
        s_put = S * s_phi(-d1, dd1, fS) + KD * s_phi(-d2, dd2, fKD) + np.abs(putv)
    return np.where(put, putv, call), np.where(put, s_put, s_call), (d1, d2, dd1, dd2)


def _side(is_put, Q):
    return np.zeros(Q, bool) if is_put is None else np.asarray(is_put).astype(bool)


def restate_greeks(params, Tq, spot, rate, u, tau_q, is_put=None, strike_mode=0, margins=False):
    """Rules G0-G6.  Returns the kernel's outputs (GREEK_KEYS and flags, each [B,Q]) and scale_<key>."""
    L = locate(params, Tq, spot, rate, u, tau_q, strike_mode)
    ok, x, xs, S, K, D, rt, tq = (L[k] for k in ("ok", "x", "xs", "S", "K", "D", "rt", "tq"))
    put = np.broadcast_to(_side(is_put, L["Q"]), ok.shape)
    s = surface(L, x, xs, derivs=True)
    with np.errstate(all="ignore"):
        W, W1, W2, V = (np.where(ok, s[k], np.nan) for k in ("w", "w1", "w2", "v"))
        SW, SW1, SW2, SV = s["sw"], s["sw1"], s["sw2"], s["sv"]
        th = np.sqrt(W)
        dth = SW / (2.0 * th) + th
        th1 = W1 / (2.0 * th)
        dth1 = SW1 / (2.0 * th) + np.abs(th1) * dth / th + 2.0 * np.abs(th1)
        A, Bq = W2 / (2.0 * th), W1 * W1 / (4.0 * th * th * th)
        th2 = A - Bq
        dth2 = SW2 / (2.0 * th) + np.abs(A) * dth / th + 2.0 * np.abs(A) + np.abs(W1) * SW1 / (2.0 * th ** 3) + 3.0 * Bq * dth / th + 4.0 * Bq + np.abs(th2)
        KD = K * D
        fKD = 4.0 + 2.0 * np.abs(rt)
        pr, s_pr, (d1, d2, dd1, dd2) = price(S, 0.0, KD, fKD, x, xs, th, dth, put)
        dss = np.where(put, -Phi(-d1), Phi(d1))
        s_dss = 2.0 * np.abs(dss) + phi(d1) * dd1
        pdf = phi(d1)
        dpdf = pdf * (np.abs(d1) * dd1 + d1 * d1 + 3.0)
        dsm = dss - pdf * th1
        s_dsm = s_dss + dpdf * np.abs(th1) + pdf * dth1 + np.abs(pdf * th1) + np.abs(dsm)
        gss = pdf / (S * th)
        s_gss = gss * (dpdf / pdf + dth / th + 3.0)
        c = x / (th * th) + 0.5
        d1x = -1.0 / th + c * th1
        dd1x = dth / (th * th) + 1.0 / th + (xs / (th * th) + 2.0 * np.abs(x) * dth / th ** 3 + 3.0 * np.abs(x) / (th * th) + 0.5) * np.abs(th1) \
            + np.abs(c) * dth1 + np.abs(c * th1) + np.abs(d1x)
        d2x = d1x - th1
        dd2x = dd1x + dth1 + np.abs(d2x)
        t3 = d1 * d1x * th1
        G = -d2x - t3 + th2 - th1
        dG = dd2x + dd1 * np.abs(d1x * th1) + np.abs(d1 * th1) * dd1x + np.abs(d1 * d1x) * dth1 + 3.0 * np.abs(t3) + dth2 + dth1 \
            + 3.0 * (np.abs(d2x) + np.abs(t3) + np.abs(th2) + np.abs(th1))
        gsm = pdf * G / S
        s_gsm = (dpdf * np.abs(G) + pdf * dG) / S + 3.0 * np.abs(gsm)
        vega = S * pdf * np.sqrt(tq)
        s_vega = vega * (dpdf / pdf + 3.0)
        exx = KD / S
        n2 = np.where(put, Phi(-d2), Phi(d2))
        T1 = np.where(put, -1.0, 1.0) * rate * exx * n2
        e_T1 = np.abs(rate * exx) * ((5.0 + fKD) * n2 + phi(d2) * dd2)
        M = V - rate * W1
        dM = SV + np.abs(rate) * SW1 + np.abs(V) + 2.0 * np.abs(rate * W1) + np.abs(M)
        T2 = pdf * M / (2.0 * th)
        e_T2 = (dpdf * np.abs(M) + pdf * dM) / (2.0 * th) + np.abs(T2) * (dth / th + 3.0)
        theta = -S * (T1 + T2)
        s_theta = S * (e_T1 + e_T2 + np.abs(T1) + np.abs(T2)) + 2.0 * np.abs(theta)
        flags = (L["flags"] | np.where(ok & (V < 0), NEG_FWD, 0)).astype(np.int32)
    nan = lambda a: np.where(ok, a, np.nan)                                   # noqa: E731
    vals = dict(price=pr, delta_ss=dss, delta_sm=dsm, gamma_ss=gss, gamma_sm=gsm, vega=vega, theta=theta)
    scales = dict(price=s_pr, delta_ss=s_dss, delta_sm=s_dsm, gamma_ss=s_gss, gamma_sm=s_gsm, vega=s_vega, theta=s_theta)
    out = {k: nan(v) for k, v in vals.items()}
    out.update({"scale_" + k: nan(v) for k, v in scales.items()})
    out.update(flags=flags, ok=ok, put=put, fwd_var=V, v_floor=s["v_floor"], W=W, W1=W1, W2=W2, SW=SW, loc=L, live_rows=L["live"])
    if margins:
        check_greeks_margins(out)
    return out


def check_greeks_margins(r):
    ok = r["ok"]
    assert ok.mean() >= 0.9 or ok.size < 10, f"only {ok.mean():.0%} of the options are live"
    if ok.any():
        assert (np.abs(r["fwd_var"][ok]) >= 1e-9 * r["v_floor"][ok]).all(), "a forward variance sits on 0"


def restate_book(params, Tq, spot, rate, u, tau_q, qty, spot_shocks, vol_shocks, is_put=None, strike_mode=0, margins=False):
    """Rules B1-B5.  Returns net [B,8], n_dead [B], pnl_ss / pnl_sm / cell_flags [B,nA,nV] and the units scale_net,
    scale_pnl_ss, scale_pnl_sm (in eps), min_vol (the smallest shocked vol of a live option over both dynamics)."""
    g = restate_greeks(params, Tq, spot, rate, u, tau_q, is_put, strike_mode)
    L = g["loc"]
    B, Q = L["B"], L["Q"]
    qty = np.asarray(qty, np.float64)
    a, v = np.asarray(spot_shocks, np.float64), np.asarray(vol_shocks, np.float64)
    nA, nV = len(a), len(v)
    live = g["ok"] & np.isfinite(qty)[None, :]
    Ldepth = depth(Q)
    q_ = np.where(live, np.broadcast_to(qty, (B, Q)), 0.0)
    aq = np.abs(q_)
    deg = L["degenerate"] & (Q > 0)          # a book without options is worth 0 whatever the snapshot
    with np.errstate(all="ignore"):
        net, s_net = np.zeros((B, 8)), np.zeros((B, 8))
        for n, k in enumerate(NET_KEYS):
            val = g["price" if k == "gross" else k]
            w = aq if k == "gross" else q_
            term = np.where(live, w * np.where(live, val, 0.0), 0.0)
            net[:, n] = b5_sum(term)
            unit = np.where(live, aq * g["scale_" + ("price" if k == "gross" else k)], 0.0)
            s_net[:, n] = unit.sum(axis=1) + (Ldepth + 1.0) * np.abs(term).sum(axis=1)
        net[deg] = np.nan
        n_dead = np.where(deg, Q, (~live).sum(axis=1)).astype(np.int32)

        S, K, D, rt, tq, x, xs = (L[k] for k in ("S", "K", "D", "rt", "tq", "x", "xs"))
        put = g["put"]
        KD, fKD = K * D, 4.0 + 2.0 * np.abs(rt)
        sqt = np.sqrt(tq)
        W0 = surface(L, x, xs)
        sig0 = np.sqrt(W0["w"] / tq)
        dsig0 = sig0 * (W0["sw"] / (2.0 * W0["w"]) + 2.0)
        shocks = np.concatenate([[0.0], a])                                   # state 0: the base, through the cells' own code
        S1 = S[..., None] * (1.0 + shocks)                                    # [B,Q,1+nA]
        lk1 = np.log(K[..., None] / S1)
        x1 = lk1 - rt[..., None]
        xs1 = 4.0 + np.abs(lk1) + 2.0 * np.abs(rt[..., None])
        W1s = surface(L, x1, xs1)
        sig1 = np.sqrt(W1s["w"] / tq[..., None])
        dsig1 = sig1 * (W1s["sw"] / (2.0 * W1s["w"]) + 2.0)
        vv = np.concatenate([[0.0], v])

        def cells(sig, dsig):
            """Prices and scales at every (state, vol shock): [B,Q,1+nA,1+nV]."""
            sg = sig[..., None] + vv
            th = sg * sqt[..., None, None]
            dth = (dsig[..., None] + np.abs(sg)) * sqt[..., None, None] + 2.0 * np.abs(th)
            e4 = lambda z: z[..., None, None]                                 # noqa: E731
            pr, sc, _ = price(S1[..., None], 2.0, e4(KD), e4(fKD), x1[..., None], xs1[..., None], th, dth, e4(put))
            return pr, sc, sg

        out = {}
        min_vol = np.inf
        for name, sig, dsig in (("ss", np.broadcast_to(sig0[..., None], sig1.shape), np.broadcast_to(dsig0[..., None], sig1.shape)),
                                ("sm", sig1, dsig1)):
            pr, sc, sg = cells(sig, dsig)
            base, sbase = pr[:, :, 0, 0], sc[:, :, 0, 0]
            P1, sP1, sg1 = pr[:, :, 1:, 1:], sc[:, :, 1:, 1:], sg[:, :, 1:, 1:]
            lv = live[..., None, None]
            term = np.where(lv, q_[..., None, None] * (P1 - base[..., None, None]), 0.0)           # [B,Q,nA,nV]
            tot = b5_sum(np.moveaxis(term, 1, -1))                            # [B,nA,nV]
            neg = (lv & (sg1 <= 0.0)).any(axis=1)
            unit = np.where(lv, aq[..., None, None] * (sP1 + sbase[..., None, None] + np.abs(P1 - base[..., None, None])), 0.0).sum(axis=1) \
                + Ldepth * np.where(lv, aq[..., None, None] * (np.abs(P1) + np.abs(base[..., None, None])), 0.0).sum(axis=1)
            tot = np.where(neg | deg[:, None, None], np.nan, tot)
            out["pnl_" + name], out["neg_" + name], out["scale_pnl_" + name] = tot, neg, unit
            out["base_" + name] = base
            if live.any() and nA * nV:
                min_vol = min(min_vol, float(np.nanmin(np.where(lv, np.abs(sg1), np.inf))))
        cell_flags = (np.where(out["neg_ss"], NEG_VOL_SS, 0) | np.where(out["neg_sm"], NEG_VOL_SM, 0)).astype(np.int32)
    res = dict(net=net, n_dead=n_dead, pnl_ss=out["pnl_ss"], pnl_sm=out["pnl_sm"], cell_flags=cell_flags, scale_net=s_net,
               scale_pnl_ss=out["scale_pnl_ss"], scale_pnl_sm=out["scale_pnl_sm"], live=live, min_vol=min_vol, greeks=g, degenerate=deg,
               base_ss=out["base_ss"], base_sm=out["base_sm"])
    if margins:
        check_greeks_margins(g)
        assert live.mean() >= 0.9 or live.size < 10, f"only {live.mean():.0%} of the options are live"
        assert not cell_flags.any(), "a cell is NEG_VOL"
        assert min_vol >= 1e-9, "a shocked vol sits on 0"
    return res


class RefBackend(CR.RefBackend):
    """CPU stand-in for snapshots.HipBackend with the Greeks and the book restated."""

    def greeks(self, params, Tq, spot, rate, u, tau, is_put, strike_mode):
        r = restate_greeks(params, Tq, spot, rate, u, tau, is_put, strike_mode)
        return {k: r[k] for k in GREEK_KEYS + ("flags",)}

    def book(self, params, Tq, spot, rate, u, tau, qty, spot_shocks, vol_shocks, is_put, strike_mode):
        r = restate_book(params, Tq, spot, rate, u, tau, qty, spot_shocks, vol_shocks, is_put, strike_mode)
        return {k: r[k] for k in BOOK_KEYS}


# ------------------------------------------------------------------ the same rules in mpmath
def _mp_point(mp, c, L, b, q):
    f = mp.mpf
    P = np.asarray(c["params"], np.float64)
    S, t, rate = f(float(c["spot"][b])), f(float(L["tq"][b, q])), f(float(c["rate"]))
    K = f(float(L["K"][b, q])) if c["strike_mode"] == 1 else S * f(float(np.broadcast_to(c["u"], L["ok"].shape)[b, q]))
    lo, hi = int(L["lo"][b, q]), int(L["hi"][b, q])
    tau = np.broadcast_to(np.asarray(c["Tq"], np.float64), P.shape[:2])
    if lo >= 0 and hi >= 0:
        ta, tc = f(float(tau[b, lo])), f(float(tau[b, hi]))
        pa, pc = [f(float(z)) for z in P[b, lo]], [f(float(z)) for z in P[b, hi]]
        lam = (t - ta) / (tc - ta)

        def W(x, n=1):
            wa, wc = CR._mp_curve(mp, pa, x), CR._mp_curve(mp, pc, x)
            return [wa[k] + (wc[k] - wa[k]) * lam for k in range(n)] + [(wc[0] - wa[0]) / (tc - ta)]
    else:
        i = lo if lo >= 0 else hi
        ta = f(float(tau[b, i]))
        pa = [f(float(z)) for z in P[b, i]]

        def W(x, n=1):
            wa = CR._mp_curve(mp, pa, x)
            return [wa[k] * t / ta for k in range(n)] + [wa[0] / ta]
    return S, K, t, rate, W


def _mp_price(mp, S, KD, x, th, put):
    sqrt2 = mp.sqrt(2)
    N = lambda z: mp.erfc(-z / sqrt2) / 2                                     # noqa: E731
    d1 = -x / th + th / 2
    d2 = d1 - th
    return KD * N(-d2) - S * N(-d1) if put else S * N(d1) - KD * N(d2)


def exact_greeks(c, ref, dps=50):
    """Every value of every live option of `ref` in mpmath at `dps` digits, with the restatement's bracket; rounded to fp64."""
    import mpmath as mp
    L = ref["loc"]
    out = {k: np.full(ref["ok"].shape, np.nan) for k in GREEK_KEYS}
    with mp.workdps(dps):
        sqrt2, s2pi = mp.sqrt(2), mp.sqrt(2 * mp.pi)
        N = lambda z: mp.erfc(-z / sqrt2) / 2                                 # noqa: E731
        n_ = lambda z: mp.exp(-z * z / 2) / s2pi                              # noqa: E731
        for b, q in zip(*np.nonzero(ref["ok"])):
            S, K, t, rate, Wf = _mp_point(mp, c, L, b, q)
            put = bool(ref["put"][b, q])
            D = mp.exp(-rate * t)
            x = mp.log(K / S) - rate * t
            W, W1, W2, V = Wf(x, 3)
            th = mp.sqrt(W)
            th1 = W1 / (2 * th)
            th2 = W2 / (2 * th) - W1 * W1 / (4 * th ** 3)
            d1 = -x / th + th / 2
            d2 = d1 - th
            d1x = -1 / th + (x / th ** 2 + mp.mpf(1) / 2) * th1
            d2x = d1x - th1
            dss = -N(-d1) if put else N(d1)
            pdf = n_(d1)
            carry = -rate * (K * D / S) * N(-d2) if put else rate * (K * D / S) * N(d2)
            vals = (_mp_price(mp, S, K * D, x, th, put), dss, dss - pdf * th1, pdf / (S * th),
                    pdf * (-d2x - d1 * d1x * th1 + th2 - th1) / S, S * pdf * mp.sqrt(t), -S * (carry + pdf * (V - rate * W1) / (2 * th)))
            for k, val in zip(GREEK_KEYS, vals):
                out[k][b, q] = float(val)
    return out


def exact_book(c, ref, dps=50):
    """net, pnl_ss and pnl_sm of `ref` in mpmath at `dps` digits (exact sums over the restatement's live options), rounded to
    fp64 at the end; NaN where the restatement has NaN."""
    import mpmath as mp
    L = ref["greeks"]["loc"]
    B, Q = L["B"], L["Q"]
    a, v = [float(z) for z in c["spot_shocks"]], [float(z) for z in c["vol_shocks"]]
    nA, nV = len(a), len(v)
    ex_g = exact_greeks(c, ref["greeks"], dps)
    out = dict(net=np.full((B, 8), np.nan), pnl_ss=np.full((B, nA, nV), np.nan), pnl_sm=np.full((B, nA, nV), np.nan))
    qty = np.asarray(c["qty"], np.float64)
    with mp.workdps(dps):
        f = mp.mpf
        for b in range(B):
            if ref["degenerate"][b]:
                continue
            lv = np.flatnonzero(ref["live"][b])
            for n, k in enumerate(NET_KEYS):
                col = ex_g["price" if k == "gross" else k][b]
                out["net"][b, n] = float(mp.fsum(f(abs(float(qty[q])) if k == "gross" else float(qty[q])) * f(float(col[q])) for q in lv))
            # the net figures above start from values already rounded to fp64: half an eps of each, well inside one unit
            tot = {d: [[f(0)] * nV for _ in range(nA)] for d in ("ss", "sm")}
            for q in lv:
                S, K, t, rate, Wf = _mp_point(mp, c, L, b, q)
                put = bool(ref["greeks"]["put"][b, q])
                KD = K * mp.exp(-rate * t)
                x = mp.log(K / S) - rate * t
                sig0 = mp.sqrt(Wf(x)[0] / t)
                P0 = _mp_price(mp, S, KD, x, sig0 * mp.sqrt(t), put)
                w = f(float(qty[q]))
                for i in range(nA):
                    S1 = S * (1 + f(a[i]))
                    x1 = mp.log(K / S1) - rate * t
                    sig1 = mp.sqrt(Wf(x1)[0] / t)
                    for k in range(nV):
                        tot["ss"][i][k] += w * (_mp_price(mp, S1, KD, x1, (sig0 + f(v[k])) * mp.sqrt(t), put) - P0)
                        tot["sm"][i][k] += w * (_mp_price(mp, S1, KD, x1, (sig1 + f(v[k])) * mp.sqrt(t), put) - P0)
            for d in ("ss", "sm"):
                for i in range(nA):
                    for k in range(nV):
                        if not np.isnan(ref["pnl_" + d][b, i, k]):
                            out["pnl_" + d][b, i, k] = float(tot[d][i][k])
    return out
