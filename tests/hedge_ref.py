"""NumPy restatement of rules M0-M11: the minimum-variance hedge of a book over its historical scenarios.
TEST INFRASTRUCTURE ONLY: written from the rules on top of hsim_ref.restate_hsim(keep=True) (the single-option rows of M2) and
hsim_ref.tail (H7); it shares no code with the kernels.  The definition is this repository's own: there is no reference
counterpart.

Every value of the selection (M3-M10) comes with its unit in eps: the first-order propagation of the rounding of every operation
of the rule through the operations after it, the rows x and y taken as exact (the device tests of stage 2 feed both sides the same
rows).  A product z = x y carries |x| dy + |y| dx + |z|, a difference dx + dy + |z|, a quotient dx / |y| + |z| dy / |y| + |z|, and a
serial sum of n terms the terms' own units plus n x the sum of their magnitudes.  The Gram-Schmidt steps divide by nu_k, so the units
grow with the collinearity of the picked set; that growth is the bound.  `exact_hedge` is the same rules in mpmath with the
restatement's picks taken as given."""
import numpy as np

import attrib_ref as AR
import hsim_ref as H

DEAD, NEG_VOL, FLAT, SPENT, CHOSEN = 1, 2, 4, 8, 16                                  # IVS_HG_*
CALL, PUT, UNDERLYING = 0, 1, 2
MAX_INST, MAX_ROUNDS = 64, 8
OUT_KEYS = ("inst_pnl", "inst_flags", "pick", "ss", "n_rounds", "hedge", "pnl_hedged", "var_h", "es_h", "worst_h", "n_scen", "solo_qty",
            "solo_left", "inst_value")
VALUE_KEYS = ("ss", "hedge", "pnl_hedged", "var_h", "es_h", "solo_qty", "solo_left")


# ------------------------------------------------------------------ values with their units
def _mul(x, dx, y, dy):
    z = x * y
    return z, np.abs(x) * dy + np.abs(y) * dx + np.abs(z)


def _sub(x, dx, y, dy):
    z = x - y
    return z, dx + dy + np.abs(z)


def _add(x, dx, y, dy):
    z = x + y
    return z, dx + dy + np.abs(z)


def _div(x, dx, y, dy):
    z = x / y
    return z, dx / np.abs(y) + np.abs(z) * dy / np.abs(y) + np.abs(z)


def ssum(t):
    """The sum convention: along axis 0 in ascending order, serially from +0.0."""
    t = np.asarray(t, np.float64)
    return np.add.accumulate(np.concatenate([np.zeros((1,) + t.shape[1:]), t]), axis=0)[-1]


def _dot(x, dx, y, dy):
    t, dt = _mul(x, dx, y, dy)
    return ssum(t), dt.sum(axis=0) + t.shape[0] * np.abs(t).sum(axis=0)


# ------------------------------------------------------------------ M2
def inst_rows(params, Tq, spot, rate, inst_u, inst_tau, inst_kind, lag, window, strike_mode):
    """M2: x [B,window,nH], its unit, dead [B,nH], value [B,nH] and its unit (section 17's price: NOT H3's bits)."""
    params, spot = np.asarray(params, np.float64), np.asarray(spot, np.float64)
    kind = np.asarray(inst_kind, np.uint8)
    nH = kind.shape[0]
    B = params.shape[0]
    und = kind == UNDERLYING
    u = np.where(und, np.nan, np.asarray(inst_u, np.float64))
    tau = np.where(und, np.nan, np.asarray(inst_tau, np.float64))
    put = (kind == PUT).astype(np.uint8)

    def run(cols):
        return H.restate_hsim(params, Tq, spot, rate, u[..., cols], tau[..., cols], np.ones(len(cols)), lag, window, (), 1, put[cols],
                              strike_mode, keep=True)
    r = run(np.arange(nH))
    x, sx = r["terms"].copy(), r["scale_terms"].copy()
    if (r["scen_flags"] == H.NEG_VOL).any():                 # the flag of the joint book hides the others: each candidate alone
        for h in np.flatnonzero(~und):
            rh = run(np.array([h]))
            x[:, :, h], sx[:, :, h] = rh["terms"][:, :, 0], rh["scale_terms"][:, :, 0]
    dead = ~r["live"]
    value, s_value = np.where(r["live"], r["greeks"]["price"], np.nan), np.where(r["live"], r["greeks"]["scale_price"], np.nan)
    void = (r["scen_flags"] & (H.ABSENT | H.VOID_PAIR)) != 0
    with np.errstate(all="ignore"):
        for h in np.flatnonzero(und):
            p_, s_ = np.nonzero(~void)
            ja = p_ - lag - s_
            S1 = spot[p_] * (spot[ja + lag] / spot[ja])
            S0 = spot[p_] * 1.0
            x[:, :, h], sx[:, :, h] = np.nan, np.nan
            x[p_, s_, h] = S1 - S0
            sx[p_, s_, h] = 2.0 * np.abs(S1) + np.abs(S1 - S0)
            dead[:, h] = r["degenerate"]
            value[:, h] = np.where(r["degenerate"], np.nan, spot * 1.0)
            s_value[:, h] = 0.0
    return dict(inst_pnl=x, scale_inst_pnl=sx, dead=dead, inst_value=value, scale_inst_value=s_value, hsim=r)


# ------------------------------------------------------------------ M3-M9 on the ranked rows of one snapshot
def pursue(x, y, dead, K, n_forced, tol, min_gain, active):
    """x [n,nH], y [n]: the ranked scenarios in ascending s.  Returns a dict of the snapshot's outputs, their units and `cond`:
    what the conditions of hedge_cases need (the gains' margins, the tested ratios, every nu)."""
    n, nH = x.shape
    zx, zy = np.zeros_like(x), np.zeros_like(y)
    nan = np.nan
    with np.errstate(all="ignore"):
        g0, dg0 = _dot(x, zx, x, zx)
        a0, da0 = _dot(x, zx, y[:, None], zy[:, None])
        E0, dE0 = _dot(y, zy, y, zy)
        bad = np.isnan(x).any(axis=0) if n else np.zeros(nH, bool)
        fl = np.where(dead, DEAD, 0) | np.where(bad, NEG_VOL, 0) | np.where(~(g0 > 0.0), FLAT, 0)
        usable = fl == 0
        out = dict(pick=np.full(K, -1, np.int32), ss=np.full(K + 1, nan), scale_ss=np.full(K + 1, nan), n_rounds=0,
                   hedge=np.full(nH, nan), scale_hedge=np.full(nH, nan), solo_qty=np.full(nH, nan), solo_left=np.full(nH, nan),
                   scale_solo_qty=np.full(nH, nan), scale_solo_left=np.full(nH, nan), q={}, cond=dict(gains=[], ratios=[], nu=[]),
                   steps=[])
        if not active:
            out["inst_flags"] = fl.astype(np.int32)
            return out
        sq, dsq = _div(a0, da0, g0, dg0)                                                   # M11: the solo figures
        gn, dgn = _div(*_mul(a0, da0, a0, da0), g0, dg0)
        sl_, dsl = _div(*_sub(E0, dE0, gn, dgn), E0, dE0)
        out["solo_qty"], out["scale_solo_qty"] = np.where(usable, 0.0 - sq, nan), np.where(usable, dsq, nan)
        out["solo_left"], out["scale_solo_left"] = np.where(usable, sl_, nan), np.where(usable, dsl, nan)

        e, de = y.copy(), zy.copy()
        g, dg, a, da, E, dE = g0.copy(), dg0.copy(), a0.copy(), da0.copy(), E0, dE0
        chosen, spent = np.zeros(nH, bool), np.zeros(nH, bool)
        steps = []                                                                         # the non-empty rounds
        out["ss"][0], out["scale_ss"][0] = E0, dE0
        stop = False
        for k in range(K):
            c = -1
            if not stop:
                elig = usable & ~chosen & ~spent                                           # M5
                thr = tol * g0
                out["cond"]["ratios"] += [float(v) for v in (g / thr)[elig]] if tol > 0 else []
                gone = elig & ~(g > thr)
                spent |= gone
                elig &= ~gone
                if k < n_forced:                                                           # M6
                    c = k if elig[k] else -1
                else:
                    gain, dgain = _div(*_mul(a, da, a, da), g, dg)
                    val = np.where(elig & ~np.isnan(gain), gain, -np.inf)
                    c0 = int(np.argmax(val))                                               # the first of the largest: the lower h
                    floor = min_gain * E
                    if val[c0] > floor:
                        c = c0
                        if min_gain > 0:
                            out["cond"]["ratios"].append(float(val[c0] / floor))
                        rest = np.where(np.arange(nH) == c0, -np.inf, val)
                        c1 = int(np.argmax(rest))
                        if rest[c1] > -np.inf:
                            out["cond"]["gains"].append((k, float(val[c0] - rest[c1]), float(dgain[c0] + dgain[c1])))
                    else:
                        stop = True
                        if min_gain > 0 and val[c0] > -np.inf and floor > 0:
                            out["cond"]["ratios"].append(float(val[c0] / floor))
            if c >= 0:                                                                     # M7
                v, dv = x[:, c].copy(), zy.copy()
                R = {}
                for st in steps:
                    r_, dr = _div(st["p"][c], st["dp"][c], st["nu"], st["dnu"])
                    v, dv = _sub(v, dv, *_mul(r_, dr, st["v"], st["dv"]))
                    R[st["k"]] = (r_, dr)
                nu, dnu = _dot(v, dv, v, dv)
                out["cond"]["nu"].append(float(nu))
                if not nu > 0.0:
                    spent[c] = True
                    c = -1
                else:                                                                      # M8
                    t, dt = _div(*_dot(v, dv, e, de), nu, dnu)
                    e, de = _sub(e, de, *_mul(t, dt, v, dv))
                    E, dE = _dot(e, de, e, de)
                    p, dp = _dot(x, zx, v[:, None], dv[:, None])
                    a, da = _dot(x, zx, e[:, None], de[:, None])
                    g, dg = _sub(g, dg, *_div(*_mul(p, dp, p, dp), nu, dnu))
                    chosen[c] = True
                    steps.append(dict(k=k, c=c, v=v, dv=dv, nu=nu, dnu=dnu, t=t, dt=dt, p=p, dp=dp, R=R))
            out["pick"][k] = c
            out["ss"][k + 1], out["scale_ss"][k + 1] = E, dE
        tau = {st["k"]: (st["t"], st["dt"]) for st in steps}                               # M9
        out["hedge"][:], out["scale_hedge"][:] = 0.0, 0.0
        for st in reversed(steps):
            tk, dtk = tau[st["k"]]
            out["q"][st["k"]] = (st["c"], 0.0 - tk, dtk)
            out["hedge"][st["c"]], out["scale_hedge"][st["c"]] = 0.0 - tk, dtk
            for j, (r_, dr) in st["R"].items():
                tau[j] = _sub(*tau[j], *_mul(tk, dtk, r_, dr))
        out["n_rounds"] = len(steps)
        out["inst_flags"] = (fl | np.where(spent, SPENT, 0) | np.where(chosen, CHOSEN, 0)).astype(np.int32)
        out["steps"], out["resid"] = steps, e
    return out


def hedged_row(y, x, picks):
    """M10 on the ranked rows: y + sum over the picks (c, q, dq) in round order of q x_c, from y; and its unit."""
    r, dr = y.copy(), np.zeros_like(y)
    with np.errstate(all="ignore"):
        for c, q, dq in picks:
            r, dr = _add(r, dr, *_mul(q, dq, x[:, c], 0.0))
    return r, dr


def select(inst_pnl, dead, pnl, scen_flags, lag, tail_probs, min_scen, rounds, n_forced, tol, min_gain):
    """M1, M3-M11 on rows given: stage 2."""
    x, pnl, fl = np.asarray(inst_pnl, np.float64), np.asarray(pnl, np.float64), np.asarray(scen_flags)
    B, W, nH = x.shape
    K = int(rounds)
    assert 1 <= nH <= MAX_INST and 1 <= K <= MAX_ROUNDS and 0 <= n_forced <= min(K, nH) and 0 <= tol < 1 and min_gain >= 0
    n_p, _ = H.exists(B, lag, W)
    out = dict(inst_flags=np.zeros((B, nH), np.int32), pick=np.full((B, K), -1, np.int32), ss=np.full((B, K + 1), np.nan),
               n_rounds=np.zeros(B, np.int32), hedge=np.full((B, nH), np.nan), pnl_hedged=np.full((B, W), np.nan),
               solo_qty=np.full((B, nH), np.nan), solo_left=np.full((B, nH), np.nan))
    unit = {k: np.full(out[k].shape, np.nan) for k in ("ss", "hedge", "pnl_hedged", "solo_qty", "solo_left")}
    cond, resid, active = [], [], np.zeros(B, bool)
    for p in range(B):
        idx = np.flatnonzero((fl[p] == 0) & ~np.isnan(pnl[p]) & (np.arange(W) < n_p[p]))      # M1
        active[p] = len(idx) >= min_scen and len(idx) > 0
        r = pursue(x[p, idx], pnl[p, idx], dead[p], K, n_forced, tol, min_gain, active[p])
        for k in ("inst_flags", "pick", "ss", "n_rounds", "hedge", "solo_qty", "solo_left"):
            out[k][p] = r[k]
        for k in ("ss", "hedge", "solo_qty", "solo_left"):
            unit[k][p] = r["scale_" + k]
        picks = [r["q"][k] for k in sorted(r["q"])]
        out["pnl_hedged"][p, idx], unit["pnl_hedged"][p, idx] = hedged_row(pnl[p, idx], x[p, idx], picks)
        cond.append(r["cond"])
        resid.append((idx, r.get("resid"), r["steps"]))
    var, es, n_scen, worst = H.tail(out["pnl_hedged"], fl, tail_probs, min_scen)
    with np.errstate(all="ignore"):
        row_unit = np.nan_to_num(unit["pnl_hedged"]).max(axis=1, initial=0.0)              # 1-Lipschitz in the row's sup norm
        unit["var_h"] = np.where(np.isnan(var), np.nan, row_unit[:, None])
        unit["es_h"] = np.where(np.isnan(es), np.nan, row_unit[:, None] + np.abs(es) * 2.0)
    out.update(inst_pnl=x, var_h=var, es_h=es, worst_h=worst, n_scen=n_scen, cond=cond, resid=resid, active=active, n_p=n_p,
               tail_probs=np.asarray(tail_probs, np.float64), min_scen=min_scen)
    out.update({"scale_" + k: v for k, v in unit.items()})
    return out


def restate_hedge(params, Tq, spot, rate, inst_u, inst_tau, inst_kind, pnl, scen_flags, lag=1, window=256, tail_probs=(0.05, 0.01),
                  min_scen=20, rounds=4, n_forced=0, tol=1e-6, min_gain=1e-4, strike_mode=0, inst_pnl=None, rows=None):
    """Rules M0-M11.  inst_pnl: the rows stage 2 selects on (None: the restatement's own).  rows: inst_rows(...) of the same
    inputs, when the caller has it already.  Returns the outputs, scale_<key> of the values (in eps) and `rows`."""
    rows = rows if rows is not None else inst_rows(params, Tq, spot, rate, inst_u, inst_tau, inst_kind, lag, window, strike_mode)
    x = rows["inst_pnl"] if inst_pnl is None else np.asarray(inst_pnl, np.float64)
    out = select(x, rows["dead"], pnl, scen_flags, lag, tail_probs, min_scen, rounds, n_forced, tol, min_gain)
    out.update(inst_pnl=x, scale_inst_pnl=rows["scale_inst_pnl"], inst_value=rows["inst_value"], rows=rows)
    return out


def hedged_margins(r, factor=1.0):
    """hsim_ref's boundary margins on the hedged row, with its own units."""
    eps = float(np.finfo(np.float64).eps)
    view = dict(pnl=r["pnl_hedged"], scale_pnl=r["scale_pnl_hedged"], scen_flags=np.where(np.isnan(r["pnl_hedged"]), 1, 0),
                min_scen=r["min_scen"], tail_probs=r["tail_probs"])
    for p, m, gap, allow in H.boundary_gaps(view):
        assert gap > factor * eps * allow, f"snapshot {p}: the hedged P&Ls of ranks {m - 1} and {m} are {gap:.3e} apart, allowance {factor * eps * allow:.3e}"


class RefBackend(AR.RefBackend):
    """CPU stand-in for a device backend with the hedge restated."""

    def hedge(self, params, Tq, spot, rate, inst_u, inst_tau, inst_kind, pnl, scen_flags, lag, window, tail_probs, min_scen, rounds,
              n_forced, tol, min_gain, strike_mode):
        r = restate_hedge(params, Tq, spot, rate, inst_u, inst_tau, inst_kind, pnl, scen_flags, lag, window, tail_probs, min_scen, rounds,
                          n_forced, tol, min_gain, strike_mode)
        return {k: r[k] for k in OUT_KEYS}


# ------------------------------------------------------------------ the same rules in mpmath
def exact_hedge(ref, pnl, dps=50):
    """ss, hedge, pnl_hedged, solo_qty and solo_left of `ref` (select / restate_hedge on the rows ref['inst_pnl'] and `pnl`) in mpmath
    at `dps` digits with the restatement's ranked sets, usable candidates and picks taken as given, rounded to fp64 at the end;
    NaN where the restatement has NaN.  var_h and es_h follow by H7 on the exact hedged row with the restatement's flags."""
    import mpmath as mp
    x, pnl = ref["inst_pnl"], np.asarray(pnl, np.float64)
    B, W, nH = x.shape
    out = {k: np.full(ref[k].shape, np.nan) for k in ("ss", "hedge", "pnl_hedged", "solo_qty", "solo_left")}
    with mp.workdps(dps):
        f = mp.mpf
        for p in range(B):
            idx, _, steps = ref["resid"][p]
            if not ref["active"][p]:
                out["pnl_hedged"][p, idx] = pnl[p, idx]
                continue
            y = [f(float(v)) for v in pnl[p, idx]]
            col = lambda h: [f(float(v)) for v in x[p, idx, h]]                         # noqa: E731
            dot = lambda u, v: mp.fsum(a * b for a, b in zip(u, v))                    # noqa: E731
            E0 = dot(y, y)
            out["ss"][p, 0] = float(E0)
            for h in range(nH):
                if not np.isnan(ref["solo_qty"][p, h]):
                    xh = col(h)
                    a, g = dot(xh, y), dot(xh, xh)
                    out["solo_qty"][p, h] = float(-a / g)
                    out["solo_left"][p, h] = float((E0 - a * a / g) / E0)
            e, V, NU, T, C = list(y), [], [], [], []
            E, kk = E0, 0
            for k in range(ref["pick"].shape[1]):
                if kk < len(steps) and steps[kk]["k"] == k:
                    c = steps[kk]["c"]
                    xc = col(c)
                    v = list(xc)
                    for vj, nuj in zip(V, NU):
                        r_ = dot(xc, vj) / nuj
                        v = [a - r_ * b for a, b in zip(v, vj)]
                    nu = dot(v, v)
                    t = dot(v, e) / nu
                    e = [a - t * b for a, b in zip(e, v)]
                    E = dot(e, e)
                    V.append(v); NU.append(nu); T.append(t); C.append(c)
                    kk += 1
                out["ss"][p, k + 1] = float(E)
            tau = list(T)                                                               # M9
            q = [f(0)] * len(T)
            for k in range(len(T) - 1, -1, -1):
                q[k] = -tau[k]
                xk = col(C[k])
                for j in range(k):
                    tau[j] = tau[j] - tau[k] * (dot(xk, V[j]) / NU[j])
            out["hedge"][p] = 0.0
            row = list(y)
            for k, c in enumerate(C):
                out["hedge"][p, c] = float(q[k])
                row = [a + q[k] * b for a, b in zip(row, col(c))]
            out["pnl_hedged"][p, idx] = [float(v) for v in row]
    var, es, _, _ = H.tail(out["pnl_hedged"], np.where(np.isnan(ref["pnl_hedged"]), 1, 0), ref["tail_probs"], ref["min_scen"])
    out.update(var_h=var, es_h=es)
    return out
