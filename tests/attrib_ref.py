"""NumPy restatement of rules A0-A8: the VaR and expected shortfall of a book attributed to its options
and to groups of them.  TEST INFRASTRUCTURE ONLY: built from hsim_ref.restate_hsim(keep=True)'s `terms` and `scale_terms` (the
P&L of every single-option book and its unit) and risk_ref.b5_sum; it shares no code with the kernels.  The definition is this
repository's own: there is no reference counterpart.  Every compared value comes with its unit in eps, derived from the rule's own
operations: a term's unit is scale_terms; a component ES is m serial additions and one division; a group sum has depth L."""
import numpy as np

import hsim_ref as H
import risk_ref as R

OUT_KEYS = ("ces", "cvar", "ces_group", "cvar_group", "n_tail", "order")
VALUE_KEYS = ("ces", "cvar", "ces_group", "cvar_group")
MAX_TAIL, MAX_GROUPS = 64, 16


def rank(pnl, scen_flags, n_p):
    """A1 on one row: the s of every rank, ascending, ties (and -0.0 against +0.0) by the lower s."""
    pnl = np.asarray(pnl, np.float64)
    idx = np.flatnonzero((np.asarray(scen_flags) == 0) & ~np.isnan(pnl) & (np.arange(len(pnl)) < n_p))
    return idx[np.argsort(pnl[idx], kind="stable")]


def tails(n, tail_probs, min_scen):
    """m_l of H7 for n ranked scenarios, 0 for an inactive level."""
    if n < min_scen or n == 0:
        return [0] * len(tail_probs)
    return [max(1, int(np.floor(np.float64(n) * np.float64(t)))) for t in tail_probs]


def allocate(terms, s_terms, live, degenerate, pnl, scen_flags, n_p, tail_probs, min_scen, group, nG):
    """A1-A6 on given terms [B,window,Q] (NaN where the option is dead or the scenario flagged) and the rows to rank."""
    B, W, Q = terms.shape
    nL = len(tail_probs)
    group = np.zeros(Q, np.int32) if group is None else np.asarray(group, np.int32)
    member = [(group == g) for g in range(nG)]
    out = dict(ces=np.full((B, nL, Q), np.nan), cvar=np.full((B, nL, Q), np.nan), ces_group=np.full((B, nL, nG), np.nan),
               cvar_group=np.full((B, nL, nG), np.nan), n_tail=np.zeros((B, nL), np.int32), order=np.full((B, W), -1, np.int32))
    unit = {k: np.full(out[k].shape, np.nan) for k in VALUE_KEYS}
    out["members"] = np.stack([(live & member[g][None, :]).sum(axis=1) for g in range(nG)], axis=1).astype(np.int32)   # [B, nG] live members
    Ld = R.depth(Q)
    with np.errstate(all="ignore"):
        for p in range(B):
            od = rank(pnl[p], scen_flags[p], n_p[p])
            out["order"][p, :len(od)] = od
            if degenerate[p]:
                continue
            ms = tails(len(od), tail_probs, min_scen)
            out["n_tail"][p] = ms
            M = max(ms, default=0)
            if M == 0:
                continue
            lv = live[p]
            t = np.where(lv[None, :], terms[p, od[:M]], 0.0)                                   # [M, Q]
            u = np.where(lv[None, :], s_terms[p, od[:M]], 0.0)
            G = np.stack([R.b5_sum(np.where((member[g] & lv)[None, :], t, 0.0)) for g in range(nG)], axis=1)      # [M, nG]
            # the unit of a group's sum is that of a scenario P&L in hsim_ref: the members' own units (each carries its share of
            # the depth-L roundings)
            uG = np.stack([np.where((member[g] & lv)[None, :], u, 0.0).sum(axis=1) for g in range(nG)], axis=1)
            run_t = np.add.accumulate(np.concatenate([np.zeros((1, Q)), t]), axis=0)[1:]       # serially from +0.0
            run_G = np.add.accumulate(np.concatenate([np.zeros((1, nG)), G]), axis=0)[1:]
            for l, m in enumerate(ms):
                if m == 0:
                    continue
                fm = np.float64(m)
                ces = 0.0 - run_t[m - 1] / fm
                out["ces"][p, l] = np.where(lv, ces, np.nan)
                out["cvar"][p, l] = np.where(lv, 0.0 - t[m - 1], np.nan)
                # m serial additions, each rounding a partial sum bounded by the sum of magnitudes; one division
                unit["ces"][p, l] = np.where(lv, (u[:m].sum(axis=0) + m * np.abs(t[:m]).sum(axis=0)) / fm + 2.0 * np.abs(ces), np.nan)
                unit["cvar"][p, l] = np.where(lv, u[m - 1], np.nan)
                ceg = 0.0 - run_G[m - 1] / fm
                out["ces_group"][p, l] = ceg
                out["cvar_group"][p, l] = 0.0 - G[m - 1]
                unit["ces_group"][p, l] = (uG[:m].sum(axis=0) + m * np.abs(G[:m]).sum(axis=0)) / fm + 2.0 * np.abs(ceg)
                unit["cvar_group"][p, l] = uG[m - 1]
    out.update({"scale_" + k: v for k, v in unit.items()})
    return out


def restate_attrib(params, Tq, spot, rate, u, tau, qty, lag=1, window=256, tail_probs=(0.05, 0.01), min_scen=20, is_put=None,
                   strike_mode=0, group=None, nG=1, pnl=None, scen_flags=None, hsim=None):
    """Rules A0-A8.  pnl, scen_flags: the rows to rank (None: the restatement's own).  hsim: restate_hsim(keep=True) of the same
    inputs, when the caller has it already.  Returns the six outputs, scale_<key> of the four values (in eps) and `hsim`."""
    r = hsim if hsim is not None else H.restate_hsim(params, Tq, spot, rate, u, tau, qty, lag, window, tail_probs, min_scen, is_put,
                                                      strike_mode, keep=True)
    assert 1 <= nG <= MAX_GROUPS
    for t in tail_probs:
        assert max(1, int(np.floor(np.float64(window) * np.float64(t)))) <= MAX_TAIL, "A7"
    pnl = r["pnl"] if pnl is None else np.asarray(pnl, np.float64)
    scen_flags = r["scen_flags"] if scen_flags is None else np.asarray(scen_flags)
    out = allocate(r["terms"], r["scale_terms"], r["live"], r["degenerate"], pnl, scen_flags, r["n_p"], tail_probs, min_scen, group, nG)
    out["hsim"] = r
    return out


class RefBackend(H.RefBackend):
    """CPU stand-in for snapshots.HipBackend with the attribution restated."""

    def hsim_attrib(self, params, Tq, spot, rate, u, tau, qty, pnl, scen_flags, group, n_groups, lag, window, tail_probs, min_scen, is_put,
                    strike_mode):
        r = restate_attrib(params, Tq, spot, rate, u, tau, qty, lag, window, tail_probs, min_scen, is_put, strike_mode, group, n_groups,
                           pnl, scen_flags)
        return {k: r[k] for k in OUT_KEYS}


def exact_attrib(ref, exact_terms, tail_probs, group, nG):
    """The four values from hsim_ref.exact_hsim's `terms` with the restatement's ranks, tails and live options, summed in mpmath
    (exact sums), rounded to fp64 at the end; NaN where the restatement has NaN."""
    import mpmath as mp
    r = ref["hsim"]
    B, W, Q = exact_terms.shape
    group = np.zeros(Q, np.int32) if group is None else np.asarray(group, np.int32)
    out = {k: np.full(ref[k].shape, np.nan) for k in VALUE_KEYS}
    with mp.workdps(50):
        f = mp.mpf
        for p in range(B):
            for l, m in enumerate(ref["n_tail"][p]):
                if m == 0:
                    continue
                od = ref["order"][p, :m]
                lv = np.flatnonzero(r["live"][p])
                for q in lv:
                    out["ces"][p, l, q] = float(-mp.fsum(f(float(exact_terms[p, s, q])) for s in od) / m)
                    out["cvar"][p, l, q] = -exact_terms[p, od[m - 1], q]
                for g in range(nG):
                    mem = [q for q in lv if group[q] == g]
                    out["ces_group"][p, l, g] = float(-mp.fsum(f(float(exact_terms[p, s, q])) for s in od for q in mem) / m)
                    out["cvar_group"][p, l, g] = float(-mp.fsum(f(float(exact_terms[p, od[m - 1], q])) for q in mem))
    return out
