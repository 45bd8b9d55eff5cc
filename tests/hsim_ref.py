"""NumPy restatement of rules H0-H9: historical-simulation VaR and expected shortfall of a book per
snapshot.  TEST INFRASTRUCTURE ONLY: written from the rules on top of risk_ref.restate_greeks (today's placement and H8),
risk_ref.locate / surface / price (the three vols of H2 and the two prices) and risk_ref.b5_sum; it shares no code with the
kernels.  The definition is this repository's own: there is no reference counterpart.  The restatement also returns the error
scale of every value it compares, in units of eps (first-order propagation through the rule's own terms).  `exact_hsim` is the
same rules in mpmath."""
import numpy as np

import risk_ref as R

ABSENT, VOID_PAIR, NEG_VOL = 1, 2, 4                                                 # IVS_HS_*
OUT_KEYS = ("pnl", "scen_flags", "var", "es", "n_valid", "n_dead", "worst", "value")
VALUE_KEYS = ("pnl", "var", "es", "value")
_CHUNK = 4_000_000                                                                   # rows x Q x mT of one locate


def exists(B, lag, window):
    """H0: n_p [B] and the mask [B,window] of the scenarios that exist."""
    n_p = np.clip(np.arange(B) - int(lag) + 1, 0, int(window))
    return n_p, np.arange(int(window))[None, :] < n_p[:, None]


def tail(pnl, scen_flags, tail_probs, min_scen):
    """H7 on rows of scenario P&Ls: var, es [B,nL], n_valid, worst [B].  Ranked: no flag and a P&L that is a number."""
    pnl, fl = np.asarray(pnl, np.float64), np.asarray(scen_flags)
    B = pnl.shape[0]
    tp = np.asarray(tail_probs, np.float64)
    var, es = np.full((B, len(tp)), np.nan), np.full((B, len(tp)), np.nan)
    n_valid, worst = np.zeros(B, np.int32), np.full(B, -1, np.int32)
    for p in range(B):
        idx = np.flatnonzero((fl[p] == 0) & ~np.isnan(pnl[p]))
        n = len(idx)
        n_valid[p] = n
        if n == 0:
            continue
        order = idx[np.argsort(pnl[p, idx], kind="stable")]               # -0.0 == +0.0: the lower s first
        worst[p] = order[0]
        if n < min_scen:
            continue
        srt = pnl[p, order]
        run = np.add.accumulate(np.concatenate([[0.0], srt]))[1:]         # serially from +0.0
        for l, t in enumerate(tp):
            m = max(1, int(np.floor(np.float64(n) * t)))
            var[p, l] = 0.0 - srt[m - 1]
            es[p, l] = 0.0 - run[m - 1] / np.float64(m)
    return var, es, n_valid, worst


def _rows(L, idx):
    B = L["B"]
    return {k: (v[idx] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B else v) for k, v in L.items()} | {"B": len(idx)}


def restate_hsim(params, Tq, spot, rate, u, tau, qty, lag=1, window=256, tail_probs=(0.05, 0.01), min_scen=20, is_put=None,
                 strike_mode=0, margins=False, keep=False):
    """Rules H0-H9.  Returns pnl, scen_flags [B,window], var, es [B,nL], n_valid, n_dead, worst [B], value [B,2], the units
    scale_pnl, scale_var, scale_es, scale_value (in eps) and for the tests: live, degenerate, min_vol (the smallest |sigma'| of a
    live option in a scenario without VOID_PAIR), with keep=True also `chunks` (the placements of every existing scenario)."""
    params, Tq, spot = np.asarray(params, np.float64), np.asarray(Tq, np.float64), np.asarray(spot, np.float64)
    qty = np.asarray(qty, np.float64)
    B, mT = params.shape[:2]
    Q = qty.shape[0]
    lag, window = int(lag), int(window)
    g = R.restate_greeks(params, Tq, spot, rate, u, tau, is_put, strike_mode)                  # today's placement (E1-E3), P0
    L = g["loc"]
    live = g["ok"] & np.isfinite(qty)[None, :]
    deg = L["degenerate"] & (Q > 0)
    q_ = np.where(live, np.broadcast_to(qty, (B, Q)), 0.0)
    aq = np.abs(q_)
    Ld = R.depth(Q)
    n_p, ex = exists(B, lag, window)
    Tq2 = np.broadcast_to(Tq, (B, mT))
    with np.errstate(all="ignore"):
        value, s_value = np.zeros((B, 2)), np.zeros((B, 2))                                    # H8
        for n, w in enumerate((q_, aq)):
            term = np.where(live, w * np.where(live, g["price"], 0.0), 0.0)
            value[:, n] = R.b5_sum(term)
            s_value[:, n] = np.where(live, aq * g["scale_price"], 0.0).sum(axis=1) + (Ld + 1.0) * np.abs(term).sum(axis=1)
        value[deg] = np.nan
        n_dead = np.where(deg, Q, (~live).sum(axis=1)).astype(np.int32)

        pnl, s_pnl = np.full((B, window), np.nan), np.full((B, window), np.nan)
        flags = np.where(ex, 0, ABSENT).astype(np.int32)
        pp, ss = np.nonzero(ex)
        min_vol, chunks = np.inf, []
        terms = np.full((B, window, Q), np.nan) if keep else None             # the single-option books: option q alone
        s_terms = np.full((B, window, Q), np.nan) if keep else None
        step = max(1, _CHUNK // max(1, Q * max(mT, 1)))
        for c0 in range(0, len(pp), step):
            p_, s_ = pp[c0:c0 + step], ss[c0:c0 + step]
            ja = p_ - lag - s_                                                                 # H0
            jb = ja + lag
            Lp = _rows(L, p_)
            K, tq, rt, S, put = Lp["K"], Lp["tq"], Lp["rt"], Lp["S"], g["put"][p_]
            lv = live[p_]
            La = R.locate(params[ja], Tq2[ja], spot[ja], rate, K, tq, 1)
            Lb = R.locate(params[jb], Tq2[jb], spot[jb], rate, K, tq, 1)
            void = (La["degenerate"] | Lb["degenerate"] | ~R._pos(spot[ja]) | ~R._pos(spot[jb]) | L["degenerate"][p_]) & (Q > 0)            # H1
            KD, fKD, sqt = K * Lp["D"], 4.0 + 2.0 * np.abs(rt), np.sqrt(tq)

            def priced(ratio, fS, ends):
                """H2 / H3: the price at the spot quotient `ratio`, with the pair's vol change or with +0.0; its scale; sigma'."""
                S1 = S * ratio
                lk = np.log(K / S1)
                x1 = lk - rt
                xs1 = 3.0 + fS + np.abs(lk) + 2.0 * np.abs(rt)
                sg, dsg = R.sigma(Lp, x1, xs1)
                if ends:
                    sb, dsb = R.sigma(Lb, x1, xs1)
                    sa, dsa = R.sigma(La, x1, xs1)
                    d = sb - sa
                    sg = sg + d
                    dsg = dsg + dsb + dsa + np.abs(d) + np.abs(sg)
                else:
                    sg = sg + 0.0
                th = sg * sqt
                dth = (dsg + np.abs(sg)) * sqt + 2.0 * np.abs(th)
                pr, sc, _ = R.price(S1, fS, KD, fKD, x1, xs1, th, dth, put)
                return pr, sc, sg

            base, s_base, _ = priced(1.0, 1.0, False)                                          # H3
            ratio = (spot[jb] / spot[ja])[:, None]                                             # H1: the quotient first
            pr, s_pr, sg = priced(ratio, 2.0, True)
            term = np.where(lv, q_[p_] * (pr - base), 0.0)                                     # H4
            tot = R.b5_sum(term)
            unit = np.where(lv, aq[p_] * (s_pr + s_base + np.abs(pr - base)), 0.0).sum(axis=1) \
                + Ld * np.where(lv, aq[p_] * (np.abs(pr) + np.abs(base)), 0.0).sum(axis=1)
            neg = (lv & ~(sg > 0.0)).any(axis=1)                                               # H5
            f = np.where(void, VOID_PAIR, np.where(neg, NEG_VOL, 0)).astype(np.int32)
            flags[p_, s_] = f
            pnl[p_, s_] = np.where(f != 0, np.nan, tot)
            s_pnl[p_, s_] = np.where(f != 0, np.nan, unit)
            ok_rows = lv & ~void[:, None]
            if ok_rows.any():
                min_vol = min(min_vol, float(np.nanmin(np.where(ok_rows, np.abs(sg), np.inf))))
            if keep:
                one = np.where(lv, aq[p_] * (s_pr + s_base + np.abs(pr - base)) + Ld * aq[p_] * (np.abs(pr) + np.abs(base)), np.nan)
                terms[p_, s_] = np.where(lv & (f == 0)[:, None], term, np.nan)
                s_terms[p_, s_] = np.where(lv & (f == 0)[:, None], one, np.nan)
                chunks.append(dict(p=p_, s=s_, ja=ja, jb=jb, Lp=Lp, La=La, Lb=Lb, void=void, sg=sg))
        var, es, n_valid, worst = tail(pnl, flags, tail_probs, min_scen)
        row_unit = np.where(np.isnan(pnl), 0.0, np.nan_to_num(s_pnl)).max(axis=1, initial=0.0)  # 1-Lipschitz in the row's sup norm
        s_var = np.where(np.isnan(var), np.nan, row_unit[:, None])
        s_es = np.where(np.isnan(es), np.nan, row_unit[:, None] + np.abs(es) * 2.0)
    out = dict(pnl=pnl, scen_flags=flags, var=var, es=es, n_valid=n_valid, n_dead=n_dead, worst=worst, value=value, scale_pnl=s_pnl,
               scale_var=s_var, scale_es=s_es, scale_value=s_value, live=live, degenerate=deg, min_vol=min_vol, greeks=g, n_p=n_p,
               exists=ex, chunks=chunks, terms=terms, scale_terms=s_terms, tail_probs=np.asarray(tail_probs, np.float64), min_scen=min_scen)
    if margins:
        check_margins(out)
    return out


def boundary_gaps(r):
    """For every snapshot and level with a VaR: (gap, allowance) of the two valid P&Ls of ranks m - 1 and m (the tail boundary),
    and of ranks 0 and 1 (the one `worst` rests on).  Lists of pairs."""
    pairs = []
    for p in range(r["pnl"].shape[0]):
        idx = np.flatnonzero((r["scen_flags"][p] == 0) & ~np.isnan(r["pnl"][p]))
        n = len(idx)
        if n < 2:
            continue
        order = idx[np.argsort(r["pnl"][p, idx], kind="stable")]
        v, sc = r["pnl"][p, order], r["scale_pnl"][p, order]
        cuts = {1}
        if n >= r["min_scen"]:
            cuts |= {max(1, int(np.floor(np.float64(n) * t))) for t in r["tail_probs"]}
        for m in cuts:
            if m < n:
                pairs.append((p, m, v[m] - v[m - 1], sc[m] + sc[m - 1]))
    return pairs


def check_margins(r, factor=1.0, unordered=False):
    """The conditions on a generated batch (the UNORDERED shape is exempt from the first two): at least 90 % of the options live;
    at least 90 % of the existing scenarios valid in at least 90 % of the snapshots with n_p > 0; every sigma' at least 1e-9 from
    0; the forward variance off zero by section 14's margin; and no two valid P&Ls that straddle a tail boundary closer than the
    sum of their allowances (`factor` x eps x their units)."""
    live, g = r["live"], r["greeks"]
    if not unordered:
        assert live.mean() >= 0.9 or live.size < 10, f"only {live.mean():.0%} of the options are live"
        has = r["n_p"] > 0
        if has.any():
            share = r["n_valid"][has] / r["n_p"][has]
            assert (share >= 0.9).mean() >= 0.9, f"only {(share >= 0.9).mean():.0%} of the snapshots have 90 % of their scenarios valid"
    assert r["min_vol"] >= 1e-9, "a scenario vol sits on 0"
    ok = g["ok"]
    if ok.any():
        assert (np.abs(g["fwd_var"][ok]) >= 1e-9 * g["v_floor"][ok]).all(), "a forward variance sits on 0"
    eps = float(np.finfo(np.float64).eps)
    for p, m, gap, allow in boundary_gaps(r):
        assert gap > factor * eps * allow, f"snapshot {p}: the P&Ls of ranks {m - 1} and {m} are {gap:.3e} apart, allowance {factor * eps * allow:.3e}"


class RefBackend(R.RefBackend):
    """CPU stand-in for snapshots.HipBackend with the explain and the historical simulation restated."""

    def explain(self, params, Tq, spot, rate, u, tau, qty, lag, is_put, strike_mode):
        import explain_ref as XR
        r = XR.restate_explain(params, Tq, spot, rate, u, tau, qty, lag, is_put, strike_mode)
        return {k: r[k] for k in XR.OUT_KEYS}

    def hsim(self, params, Tq, spot, rate, u, tau, qty, lag, window, tail_probs, min_scen, is_put, strike_mode):
        r = restate_hsim(params, Tq, spot, rate, u, tau, qty, lag, window, tail_probs, min_scen, is_put, strike_mode)
        return {k: r[k] for k in OUT_KEYS}


# ------------------------------------------------------------------ the same rules in mpmath
def exact_hsim(c, ref, dps=50):
    """pnl, var, es, value and terms (the P&L of every single-option book) of `ref` (restate_hsim(..., keep=True) of the case `c`) in mpmath at `dps` digits with the
    restatement's brackets and live options (exact sums), rounded to fp64 at the end; NaN where the restatement has NaN."""
    import mpmath as mp
    params, spot = np.asarray(c["params"], np.float64), np.asarray(c["spot"], np.float64)
    B, mT = params.shape[:2]
    Tq2 = np.broadcast_to(np.asarray(c["Tq"], np.float64), (B, mT))
    qty = np.asarray(c["qty"], np.float64)
    g = ref["greeks"]
    pnl = np.full(ref["pnl"].shape, np.nan)
    terms = np.full(ref["terms"].shape, np.nan)
    value = np.full((B, 2), np.nan)
    ex_g = R.exact_greeks(dict(c), g, dps)
    with mp.workdps(dps):
        f = mp.mpf
        for b in range(B):
            if not ref["degenerate"][b]:
                lv = np.flatnonzero(ref["live"][b])
                value[b, 0] = float(mp.fsum(f(float(qty[q])) * f(float(ex_g["price"][b, q])) for q in lv))
                value[b, 1] = float(mp.fsum(f(abs(float(qty[q]))) * f(float(ex_g["price"][b, q])) for q in lv))
        for ch in ref["chunks"]:
            cp = dict(params=params[ch["p"]], Tq=Tq2[ch["p"]], spot=spot[ch["p"]], rate=c["rate"], u=ch["Lp"]["K"], strike_mode=1)
            ca = dict(cp, params=params[ch["ja"]], Tq=Tq2[ch["ja"]], spot=spot[ch["ja"]])
            cb = dict(cp, params=params[ch["jb"]], Tq=Tq2[ch["jb"]], spot=spot[ch["jb"]])
            if c["strike_mode"] == 0:                         # K = S u, not rounded
                cp = dict(cp, u=np.broadcast_to(c["u"], ref["live"].shape)[ch["p"]], strike_mode=0)
            for n, (p, s) in enumerate(zip(ch["p"], ch["s"])):
                if np.isnan(ref["pnl"][p, s]):
                    continue
                tot = f(0)
                for q in np.flatnonzero(ref["live"][p]):
                    S, K, t, r, Wp = R._mp_point(mp, cp, ch["Lp"], n, q)
                    Sa, _, _, _, Wa = R._mp_point(mp, dict(ca, u=None), ch["La"], n, q)
                    Sb, _, _, _, Wb = R._mp_point(mp, dict(cb, u=None), ch["Lb"], n, q)
                    put = bool(g["put"][p, q])
                    KD = K * mp.exp(-r * t)
                    x0 = mp.log(K / S) - r * t
                    P0 = R._mp_price(mp, S, KD, x0, mp.sqrt(Wp(x0)[0]), put)
                    S1 = S * (Sb / Sa)
                    x1 = mp.log(K / S1) - r * t
                    sg = mp.sqrt(Wp(x1)[0] / t) + (mp.sqrt(Wb(x1)[0] / t) - mp.sqrt(Wa(x1)[0] / t))
                    one = f(float(qty[q])) * (R._mp_price(mp, S1, KD, x1, sg * mp.sqrt(t), put) - P0)
                    terms[p, s, q] = float(one)
                    tot += one
                pnl[p, s] = float(tot)
    var, es, _, _ = tail(pnl, ref["scen_flags"], ref["tail_probs"], ref["min_scen"])
    return dict(pnl=pnl, var=var, es=es, value=value, terms=terms)
