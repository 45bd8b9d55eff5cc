"""NumPy restatement of rules X0-X9: the P&L of a book between snapshot p and snapshot p + lag, split
into theta, delta, gamma, vega and a remainder under sticky strike and under sticky moneyness.  TEST INFRASTRUCTURE ONLY: written
from the rules on top of risk_ref.restate_greeks (placements (a) and (b)), risk_ref.locate / surface (placement (c) and the three
vols) and risk_ref.b5_sum; it shares no code with the kernels.  The definition is this repository's own: there is no reference
counterpart.  The restatement also returns the error scale of every value it compares, in units of eps (first-order propagation
through the rule's own terms).  `exact_explain` is the same rules in mpmath."""
import numpy as np

import risk_ref as R

KEYS = ("actual", "theta_pnl", "delta_ss", "gamma_ss", "vega_ss", "resid_ss", "delta_sm", "gamma_sm", "vega_sm", "resid_sm")
NET_KEYS = KEYS + ("value", "gross")
OUT_KEYS = KEYS + ("flags", "net", "n_dead")
SHORT, LONG, NEG_FWD, Q_DEAD, Q_UNORDERED = R.SHORT, R.LONG, R.NEG_FWD, R.Q_DEAD, R.Q_UNORDERED


def pair_inputs(params, Tq, spot, u, tau, lag):
    """X0: the two ends of every pair.  Returns P and, per end e in (0, 1), params_e [P,mT,5], Tq_e, spot_e [P], and u0, tau0,
    tau1 ([Q] when shared, [P,Q] otherwise)."""
    params, Tq, spot = np.asarray(params, np.float64), np.asarray(Tq, np.float64), np.asarray(spot, np.float64)
    u, tau = np.asarray(u, np.float64), np.asarray(tau, np.float64)
    B = params.shape[0]
    P = max(B - int(lag), 0)
    i0, i1 = np.arange(P), np.arange(P) + int(lag)
    pick = lambda a, i: a[i] if a.ndim == 2 else a                            # noqa: E731
    return dict(P=P, params0=params[i0], params1=params[i1], Tq0=pick(Tq, i0), Tq1=pick(Tq, i1), spot0=spot[i0], spot1=spot[i1],
                u0=pick(u, i0), tau0=pick(tau, i0), tau1=pick(tau, i1))


def restate_explain(params, Tq, spot, rate, u, tau, qty, lag=1, is_put=None, strike_mode=0, margins=False):
    """Rules X0-X9.  Returns the ten values [P,Q], flags [P,Q], net [P,12], n_dead [P], scale_<key> of every value and
    scale_net (in eps), and for the tests: live, degenerate, a / b (the restated Greeks of the two ends), K, dS, dt, sig1,
    sig_ss, sig_sm."""
    E = pair_inputs(params, Tq, spot, u, tau, lag)
    P = E["P"]
    qty = np.asarray(qty, np.float64)
    Q = qty.shape[0]
    if P == 0:
        out = {k: np.zeros((0, Q)) for k in KEYS}
        out.update({"scale_" + k: np.zeros((0, Q)) for k in KEYS})
        out.update(flags=np.zeros((0, Q), np.int32), net=np.zeros((0, 12)), scale_net=np.zeros((0, 12)), n_dead=np.zeros(0, np.int32),
                   live=np.zeros((0, Q), bool), degenerate=np.zeros(0, bool), P=0)
        return out
    S0, S1 = E["spot0"], E["spot1"]
    with np.errstate(all="ignore"):
        u0 = np.broadcast_to(E["u0"], (P, Q))
        K = S0[:, None] * u0 if strike_mode == 0 else u0                      # X0
        t0, t1 = np.broadcast_to(E["tau0"], (P, Q)), np.broadcast_to(E["tau1"], (P, Q))
        a = R.restate_greeks(E["params0"], E["Tq0"], S0, rate, E["u0"], E["tau0"], is_put, strike_mode)       # X1 (a)
        b = R.restate_greeks(E["params1"], E["Tq1"], S1, rate, K, t1, is_put, 1)                              # X1 (b)
        La, Lb = a["loc"], b["loc"]
        Lc = R.locate(E["params0"], E["Tq0"], S0, rate, K, t1, 1)                                             # X1 (c)
        sig1, dsig1 = R.sigma(Lb, Lb["x"], Lb["xs"])
        sig_ss, dsig_ss = R.sigma(Lc, Lc["x"], Lc["xs"])
        sig_sm, dsig_sm = R.sigma(Lc, Lb["x"], Lb["xs"])
        live = a["ok"] & b["ok"] & Lc["ok"] & np.isfinite(qty)[None, :]       # X2
        deg = (La["degenerate"] | Lb["degenerate"]) & (Q > 0)
        flags = (a["flags"] | (Lb["flags"] << 8) | (Lc["flags"] << 16)).astype(np.int32)        # X5
        dS = (S1 - S0)[:, None]
        dS2 = dS * dS
        dt = t0 - t1
        v, s = {}, {}
        v["actual"] = b["price"] - a["price"]                                 # X3
        s["actual"] = b["scale_price"] + a["scale_price"] + np.abs(v["actual"])
        v["theta_pnl"] = a["theta"] * dt + 0.0
        s["theta_pnl"] = a["scale_theta"] * np.abs(dt) + 3.0 * np.abs(v["theta_pnl"])
        for d, sg0, dsg0 in (("ss", sig_ss, dsig_ss), ("sm", sig_sm, dsig_sm)):
            v["delta_" + d] = a["delta_" + d] * dS + 0.0
            s["delta_" + d] = a["scale_delta_" + d] * np.abs(dS) + 3.0 * np.abs(v["delta_" + d])
            v["gamma_" + d] = (0.5 * a["gamma_" + d]) * dS2 + 0.0
            s["gamma_" + d] = a["scale_gamma_" + d] * 0.5 * dS2 + 4.0 * np.abs(v["gamma_" + d])
            dsg = sig1 - sg0
            v["vega_" + d] = a["vega"] * dsg + 0.0
            s["vega_" + d] = a["scale_vega"] * np.abs(dsg) + a["vega"] * (dsig1 + dsg0 + np.abs(dsg)) + 2.0 * np.abs(v["vega_" + d])
            ops = ("actual", "theta_pnl", "delta_" + d, "gamma_" + d, "vega_" + d)
            v["resid_" + d] = v["actual"] - (((v["theta_pnl"] + v["delta_" + d]) + v["gamma_" + d]) + v["vega_" + d])       # X4
            s["resid_" + d] = sum(s[k] for k in ops) + sum(np.abs(v[k]) for k in ops)
        out = {k: np.where(live, v[k], np.nan) for k in KEYS}
        out.update({"scale_" + k: np.where(live, s[k], np.nan) for k in KEYS})
        q_ = np.where(live, np.broadcast_to(qty, (P, Q)), 0.0)                # X6
        aq = np.abs(q_)
        Ld = R.depth(Q)
        net, s_net = np.zeros((P, 12)), np.zeros((P, 12))
        for n, k in enumerate(NET_KEYS):
            val = a["price"] if k in ("value", "gross") else v[k]
            unit = a["scale_price"] if k in ("value", "gross") else s[k]
            w = aq if k == "gross" else q_
            term = np.where(live, w * np.where(live, val, 0.0), 0.0)
            net[:, n] = R.b5_sum(term)                                        # X7
            s_net[:, n] = np.where(live, aq * unit, 0.0).sum(axis=1) + (Ld + 1.0) * np.abs(term).sum(axis=1)
        net[deg] = np.nan
        n_dead = np.where(deg, Q, (~live).sum(axis=1)).astype(np.int32)
    out.update(flags=flags, net=net, scale_net=s_net, n_dead=n_dead, live=live, degenerate=deg, a=a, b=b, Lc=Lc, K=K, dS=dS, dt=dt, sig1=sig1,
               sig_ss=sig_ss, sig_sm=sig_sm, P=P, ends=E, t1=t1)
    if margins:
        check_margins(out)
    return out


def check_margins(r):
    """The conditions on a generated batch: at least 90 % of the options live in at least 90 % of the pairs, the forward variance
    of (a) off zero by section 14's margin, and a positive time left for every live option."""
    live = r["live"]
    if live.size == 0:
        return
    share = live.mean(axis=1)
    assert (share >= 0.9).mean() >= 0.9 or live.shape[1] < 10, f"only {(share >= 0.9).mean():.0%} of the pairs have 90 % of the options live"
    if live.any():
        assert (np.abs(r["a"]["fwd_var"][live]) >= 1e-9 * r["a"]["v_floor"][live]).all(), "a forward variance sits on 0"
        assert (r["t1"][live] > 0).all(), "a live option has no time left at end 1"


class RefBackend(R.RefBackend):
    """CPU stand-in for snapshots.HipBackend with the explain restated."""

    def explain(self, params, Tq, spot, rate, u, tau, qty, lag, is_put, strike_mode):
        r = restate_explain(params, Tq, spot, rate, u, tau, qty, lag, is_put, strike_mode)
        return {k: r[k] for k in OUT_KEYS}


# ------------------------------------------------------------------ the same rules in mpmath
def exact_explain(ref, rate, qty, strike_mode, dps=50):
    """The ten values of every live option of `ref` and net[0..11] in mpmath at `dps` digits with the restatement's brackets
    (exact sums over the restatement's live options), rounded to fp64 at the end; NaN where the restatement has NaN."""
    import mpmath as mp
    E, a, b, Lc = ref["ends"], ref["a"], ref["b"], ref["Lc"]
    P, Q = ref["live"].shape
    qty = np.asarray(qty, np.float64)
    out = {k: np.full((P, Q), np.nan) for k in KEYS}
    out["net"] = np.full((P, 12), np.nan)
    ca = dict(params=E["params0"], Tq=E["Tq0"], spot=E["spot0"], rate=rate, u=E["u0"], strike_mode=strike_mode)
    cb = dict(params=E["params1"], Tq=E["Tq1"], spot=E["spot1"], rate=rate, u=ref["K"], strike_mode=1)
    cc = dict(params=E["params0"], Tq=E["Tq0"], spot=E["spot0"], rate=rate, u=ref["K"], strike_mode=1)
    with mp.workdps(dps):
        f = mp.mpf
        sqrt2, s2pi = mp.sqrt(2), mp.sqrt(2 * mp.pi)
        N = lambda z: mp.erfc(-z / sqrt2) / 2                                 # noqa: E731
        n_ = lambda z: mp.exp(-z * z / 2) / s2pi                              # noqa: E731
        for p in range(P):
            tot = [f(0)] * 12
            for q in np.flatnonzero(ref["live"][p]):
                S0, K, t0, r, Wa = R._mp_point(mp, ca, a["loc"], p, q)        # K = S0 u, not rounded
                S1, _, t1, _, Wb = R._mp_point(mp, cb, b["loc"], p, q)
                _, _, _, _, Wc = R._mp_point(mp, cc, Lc, p, q)
                put = bool(a["put"][p, q])
                D0, x0 = mp.exp(-r * t0), mp.log(K / S0) - r * t0
                W, W1, W2, V = Wa(x0, 3)
                th = mp.sqrt(W)
                th1 = W1 / (2 * th)
                th2 = W2 / (2 * th) - W1 * W1 / (4 * th ** 3)
                d1 = -x0 / th + th / 2
                d2 = d1 - th
                d1x = -1 / th + (x0 / th ** 2 + f(1) / 2) * th1
                d2x = d1x - th1
                pdf = n_(d1)
                dss = -N(-d1) if put else N(d1)
                dsm = dss - pdf * th1
                gss = pdf / (S0 * th)
                gsm = pdf * (-d2x - d1 * d1x * th1 + th2 - th1) / S0
                vega = S0 * pdf * mp.sqrt(t0)
                carry = -r * (K * D0 / S0) * N(-d2) if put else r * (K * D0 / S0) * N(d2)
                theta = -S0 * (carry + pdf * (V - r * W1) / (2 * th))
                P0 = R._mp_price(mp, S0, K * D0, x0, th, put)
                x1 = mp.log(K / S1) - r * t1
                P1 = R._mp_price(mp, S1, K * mp.exp(-r * t1), x1, mp.sqrt(Wb(x1)[0]), put)
                sg1 = mp.sqrt(Wb(x1)[0] / t1)
                sg_ss = mp.sqrt(Wc(mp.log(K / S0) - r * t1)[0] / t1)
                sg_sm = mp.sqrt(Wc(x1)[0] / t1)
                dS, dt = S1 - S0, t0 - t1
                act, thp = P1 - P0, theta * dt
                vals = [act, thp]
                for dl, gm, sg in ((dss, gss, sg_ss), (dsm, gsm, sg_sm)):
                    t = [dl * dS, gm * dS * dS / 2, vega * (sg1 - sg)]
                    vals += t + [act - (thp + t[0] + t[1] + t[2])]
                for k, val in zip(KEYS, vals):
                    out[k][p, q] = float(val)
                w = f(float(qty[q]))
                for n, val in enumerate(vals + [P0]):
                    tot[n] += w * val
                tot[11] += abs(w) * P0
            if not ref["degenerate"][p]:
                out["net"][p] = [float(z) for z in tot]
    return out
