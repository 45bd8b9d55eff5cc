"""NumPy restatement of rules W0-W9: the what-if VaR and expected shortfall of a book per candidate trade
and size.  TEST INFRASTRUCTURE ONLY: written from the rules on top of hedge_ref.inst_rows (W2: the rows of M2) and hsim_ref.tail (W5,
W6: H7); it shares no code with the kernels.  The definition is this repository's own: there is no reference counterpart.

Every value comes with two units in eps.  scale_<key> is the ladder's own: the rows x and y taken as exact, z = y + q x carries the
rounding of the product and of the sum, |q x| + |z|; an order statistic is 1-Lipschitz in the sup norm of its row, so var_w carries
the largest of them over the row, and es_w that plus the sum of the magnitudes of the m smallest (the m roundings of the serial sum,
over m) plus |es| (the quotient).  rows_<key>
is what the rows bring in when they are not exact: unit(y) + |q| unit(x), again the largest over the row.  `exact_whatif` is the same
rules in mpmath on the rows given."""
import numpy as np

import hedge_ref as G
import hsim_ref as H

NEG_VOL = G.NEG_VOL
MAX_RUNGS = 16
OUT_KEYS = ("inst_pnl", "inst_value", "trade_flags", "var_w", "es_w", "worst_w", "best", "var0", "es0", "worst0", "n_scen")
VALUE_KEYS = ("var_w", "es_w", "var0", "es0")
INT_KEYS = ("trade_flags", "worst_w", "best", "worst0", "n_scen")
STAGE2_KEYS = tuple(k for k in OUT_KEYS if k not in ("inst_pnl", "inst_value"))


def ranked_set(pnl, scen_flags, lag):
    """W1: the mask [B,window] of the ranked scenarios."""
    pnl, fl = np.asarray(pnl, np.float64), np.asarray(scen_flags)
    B, W = pnl.shape
    n_p, _ = H.exists(B, lag, W)
    return (fl == 0) & ~np.isnan(pnl) & (np.arange(W)[None, :] < n_p[:, None])


def sizes(size, B, nH):
    """The ladder as [B,nH,nQ]."""
    size = np.asarray(size, np.float64)
    assert size.ndim in (2, 3) and size.shape[-2] == nH and 1 <= size.shape[-1] <= MAX_RUNGS
    return np.broadcast_to(size, (B,) + size.shape[-2:])


def best_rung(es, live):
    """W7: [B,nH,nL] from es [B,nH,nQ,nL] and live [B,nH,nQ]: the smallest es that is a number, ties to the lower rung."""
    ok = live[..., None] & ~np.isnan(es)
    key = np.where(ok, es, np.inf)
    j = np.argmin(key, axis=2)                                                             # the first of the smallest
    hit = np.take_along_axis(ok, j[:, :, None, :], axis=2)[:, :, 0, :]
    j = np.where(hit, j, np.argmax(ok, axis=2))                                            # every es that counts is +inf
    return np.where(ok.any(axis=2), j, -1).astype(np.int32)


def tail_mass(z, n, tp):
    """The sum of the magnitudes of the m smallest of every row of z [..., W] (NaN: not ranked) at every level: [..., nL]; n: the
    rows' counts, broadcast against z's leading axes.  It is what the m roundings of the serial sum, over m, are counted at."""
    run = np.nancumsum(np.abs(np.sort(z, axis=-1)), axis=-1)                                # NaN sorts last
    n = np.broadcast_to(n, z.shape[:-1])
    m = np.maximum(1, np.floor(n.astype(np.float64)[..., None] * tp).astype(np.int64))     # one IEEE product, as H7 forms it
    return np.take_along_axis(run, np.minimum(m, z.shape[-1]) - 1, axis=-1)


def ladder(inst_pnl, pnl, scen_flags, size, lag, tail_probs, min_scen, unit_x=None, unit_y=None):
    """W1, W3-W7 on rows given: stage 2.  unit_x, unit_y: the units of the rows in eps (None: exact)."""
    x, y = np.asarray(inst_pnl, np.float64), np.asarray(pnl, np.float64)
    B, W, nH = x.shape
    q = sizes(size, B, nH)
    nQ = q.shape[-1]
    tp = np.asarray(tail_probs, np.float64)
    nL = len(tp)
    assert 1 <= nH <= G.MAX_INST and nL <= 8 and min_scen >= 1
    ranked = ranked_set(y, scen_flags, lag)
    n = ranked.sum(axis=1)
    active = (n >= min_scen) & (n > 0)
    ux = np.zeros_like(x) if unit_x is None else np.nan_to_num(np.asarray(unit_x, np.float64))
    uy = np.zeros_like(y) if unit_y is None else np.nan_to_num(np.asarray(unit_y, np.float64))
    with np.errstate(all="ignore"):
        yr = np.where(ranked, y, np.nan)
        var0, es0, n_scen, worst0 = H.tail(yr, np.where(ranked, 0, 1), tp, min_scen)           # W6
        bad = (ranked[:, :, None] & np.isnan(x)).any(axis=1)                                   # W3
        xr = np.where(ranked[:, :, None], x, 0.0).transpose(0, 2, 1)                           # [B,nH,W]
        prod = q[..., None] * xr[:, :, None, :]                                                # W4: rounded, then added
        z = yr[:, None, None, :] + prod
        live = ~bad[:, :, None] & active[:, None, None] & np.isfinite(q)
        live &= ~(np.isnan(z) & ranked[:, None, None, :]).any(axis=-1)                         # inf - inf, 0 x inf: no order
        z = np.where(live[..., None], z, np.nan)
        own = np.where(np.isnan(z), 0.0, np.abs(prod) + np.abs(z))
        rows = np.where(np.isnan(z), 0.0, uy[:, None, None, :] + np.abs(q)[..., None] * ux.transpose(0, 2, 1)[:, :, None, :])
        v, e, _, w = H.tail(z.reshape(-1, W), np.isnan(z).reshape(-1, W).astype(np.int32), tp, 1)       # W5: n is the row's own
        var_w, es_w, worst_w = v.reshape(B, nH, nQ, nL), e.reshape(B, nH, nQ, nL), w.reshape(B, nH, nQ).astype(np.int32)
        nanl = lambda a, ref: np.where(np.isnan(ref), np.nan, a)                               # noqa: E731
        s_var = nanl(np.broadcast_to(own.max(axis=-1)[..., None], var_w.shape), var_w)
        s_es = nanl(own.max(axis=-1)[..., None] + tail_mass(z, n[:, None, None], tp) + np.abs(es_w), es_w)
        r_w = nanl(np.broadcast_to(rows.max(axis=-1)[..., None], var_w.shape), var_w)
        r_0 = nanl(np.broadcast_to(np.where(ranked, uy, 0.0).max(axis=1, initial=0.0)[:, None], var0.shape), var0)
    return dict(trade_flags=np.where(bad, NEG_VOL, 0).astype(np.int32), var_w=var_w, es_w=es_w, worst_w=worst_w, best=best_rung(es_w, live),
                var0=var0, es0=es0, worst0=worst0, n_scen=n_scen, scale_var_w=s_var, scale_es_w=s_es, rows_var_w=r_w, rows_es_w=r_w,
                scale_var0=nanl(np.zeros_like(var0), var0), scale_es0=nanl(tail_mass(yr, n, tp) + np.abs(es0), es0), rows_var0=r_0, rows_es0=r_0,
                live=live, active=active, ranked=ranked, z=z, unit_z=own, rows_z=rows, size=q, inst_pnl=x, tail_probs=tp, min_scen=min_scen)


def restate_whatif(params, Tq, spot, rate, inst_u, inst_tau, inst_kind, pnl, scen_flags, size, lag=1, window=256, tail_probs=(0.05, 0.01),
                   min_scen=20, strike_mode=0, inst_pnl=None, rows=None, unit_y=None):
    """Rules W0-W9.  inst_pnl: the rows the ladder is formed on (None: the restatement's own, with their units).  rows:
    hedge_ref.inst_rows(...) of the same inputs, when the caller has it.  unit_y: the unit of pnl (hsim_ref's scale_pnl)."""
    rows = rows if rows is not None else G.inst_rows(params, Tq, spot, rate, inst_u, inst_tau, inst_kind, lag, window, strike_mode)
    own = inst_pnl is None
    out = ladder(rows["inst_pnl"] if own else inst_pnl, pnl, scen_flags, size, lag, tail_probs, min_scen,
                 rows["scale_inst_pnl"] if own else None, unit_y)
    out.update(scale_inst_pnl=rows["scale_inst_pnl"], inst_value=rows["inst_value"], rows=rows)
    return out


def boundary_gaps(r):
    """hsim_ref.check_margins' logic on every live row z: for the boundaries m - 1 | m of every level and 0 | 1, (where, m, gap, the
    two values' own units, the two values' row units)."""
    out = []
    B, nH, nQ, W = r["z"].shape
    for p, h, j in zip(*np.nonzero(r["live"])):
        z = r["z"][p, h, j]
        idx = np.flatnonzero(~np.isnan(z))
        n = len(idx)
        if n < 2:
            continue
        order = idx[np.argsort(z[idx], kind="stable")]
        cuts = {1} | {max(1, int(np.floor(np.float64(n) * t))) for t in r["tail_probs"]}
        for m in cuts:
            if m < n:
                a, b = order[m - 1], order[m]
                out.append(((p, h, j), m, z[b] - z[a], r["unit_z"][p, h, j, a] + r["unit_z"][p, h, j, b],
                            r["rows_z"][p, h, j, a] + r["rows_z"][p, h, j, b]))
    return out


def best_gaps(r):
    """For every (p, h, l) with two live rungs: (where, second-best es - best es, their own units, their row units)."""
    out = []
    es = r["es_w"]
    B, nH, nQ, nL = es.shape
    for p, h, l in zip(*np.nonzero(r["best"] >= 0)):
        e = es[p, h, :, l]
        ok = np.flatnonzero(r["live"][p, h] & ~np.isnan(e))
        if len(ok) < 2:
            continue
        o = ok[np.argsort(e[ok], kind="stable")]
        out.append(((p, h, l), e[o[1]] - e[o[0]], r["scale_es_w"][p, h, o[0], l] + r["scale_es_w"][p, h, o[1], l],
                    r["rows_es_w"][p, h, o[0], l] + r["rows_es_w"][p, h, o[1], l]))
    return out


class RefBackend(G.RefBackend):
    """CPU stand-in for a device backend with the what-if ladder restated."""

    def whatif(self, params, Tq, spot, rate, inst_u, inst_tau, inst_kind, pnl, scen_flags, size, lag, window, tail_probs, min_scen,
               strike_mode, inst_pnl=None):
        r = restate_whatif(params, Tq, spot, rate, inst_u, inst_tau, inst_kind, pnl, scen_flags, size, lag, window, tail_probs, min_scen,
                           strike_mode, inst_pnl=inst_pnl)
        return {k: r[k] for k in OUT_KEYS}


# ------------------------------------------------------------------ the same rules in mpmath
def exact_whatif(ref, pnl, dps=50):
    """var_w, es_w, var0 and es0 of `ref` (ladder / restate_whatif on the rows ref['inst_pnl'] and `pnl`) in mpmath at `dps` digits
    with the restatement's ranked sets and live rungs taken as given: z, its order, the sum of the m smallest and the quotient are
    exact, rounded to fp64 at the end; NaN where the restatement has NaN."""
    import mpmath as mp
    x, pnl, q = ref["inst_pnl"], np.asarray(pnl, np.float64), ref["size"]
    tp, min_scen = ref["tail_probs"], ref["min_scen"]
    out = {k: np.full(ref[k].shape, np.nan) for k in VALUE_KEYS}
    with mp.workdps(dps):
        f = mp.mpf

        def tail(row, n, var, es):
            srt = sorted(row)
            for l, t in enumerate(tp):
                m = max(1, int(np.floor(np.float64(n) * t)))
                var[l], es[l] = float(-srt[m - 1]), float(-mp.fsum(srt[:m]) / m)

        for p in np.flatnonzero(ref["active"]):
            idx = np.flatnonzero(ref["ranked"][p])
            y = [f(float(v)) for v in pnl[p, idx]]
            tail(y, len(idx), out["var0"][p], out["es0"][p])
            for h, j in zip(*np.nonzero(ref["live"][p])):
                qq = f(float(q[p, h, j]))
                tail([a + qq * f(float(b)) for a, b in zip(y, x[p, idx, h])], len(idx), out["var_w"][p, h, j], out["es_w"][p, h, j])
    return out
