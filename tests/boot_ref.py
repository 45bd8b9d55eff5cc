"""NumPy restatement of rules C0-C9: bootstrap standard errors and intervals for a book's VaR and expected
shortfall.  TEST INFRASTRUCTURE ONLY: written from the rules on top of hsim_ref.tail (C1: H7 on the row, var0 / es0 / n_scen) and
risk_ref.b5_sum (C6: the order of the sums); it shares no code with the kernel.  The definition is this repository's own: there is no
reference counterpart.  C1-C7 are a fixed sequence of IEEE and integer operations under a total order, so the kernel has to
reproduce every output to the bit; there are no units here.  `walk` is C5 as the rule reads, one rank at a time, for the tables by hand;
`bootstrap` forms the same sums array-wise (a rank that adds nothing adds a zero, which changes no bit of a sum that started at +0.0
and holds finite terms)."""
import numpy as np

import hsim_ref as H
import risk_ref as R
import whatif_ref as W

MAX_REP, MAX_BLOCK, MAX_CI = 1024, 1024, 8
OUT_KEYS = ("var0", "es0", "n_scen", "mean", "variance", "quant", "rep")
M64 = (1 << 64) - 1


def words(seed, r, i, n):
    """C3: the block starts b(r, i) for arrays r, i (broadcast), as int64 in [0, n).  uint64 arithmetic wraps."""
    with np.errstate(over="ignore"):
        c = (np.asarray(r, np.uint64) << np.uint64(32)) | np.asarray(i, np.uint64)
        z = np.uint64(int(seed) & M64) + (c + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        u = z >> np.uint64(32)
        return ((u * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def word_by_hand(seed, r, i, n):
    """C3 on Python integers: the check of `words`."""
    c = (r << 32) | i
    z = (seed + (c + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return ((z >> 32) * n) >> 32


def positions(n, block, seed, n_rep):
    """C4: the time positions [n_rep, n] every replicate draws."""
    Lp = min(int(block), n)
    nb = -(-n // Lp)
    b = words(seed, np.arange(n_rep)[:, None], np.arange(nb)[None, :], n)                     # [R, nb]
    pos = (b[:, :, None] + np.arange(Lp)[None, None, :]) % n
    return pos.reshape(n_rep, nb * Lp)[:, :n]


def ranked(pnl_row, flag_row):
    """C1 on one row: (v in rank order, rho [n]: the rank of time position k)."""
    idx = np.flatnonzero((np.asarray(flag_row) == 0) & ~np.isnan(pnl_row))
    order = np.argsort(pnl_row[idx], kind="stable")                                         # -0.0 == +0.0: the lower s first
    rho = np.empty(len(idx), np.int64)
    rho[order] = np.arange(len(idx))
    return pnl_row[idx][order], rho


def walk(counts, v, m):
    """C5 as the rule reads, on one replicate's counts: (var*, es*)."""
    s, taken, last = np.float64(0.0), 0, None
    for rk, c in enumerate(counts):
        if c > 0:
            k = min(int(c), m - taken)
            s = s + np.float64(k) * v[rk]
            taken += k
            last = v[rk]
            if taken == m:
                break
    return np.float64(0.0) - last, np.float64(0.0) - s / np.float64(m)


def summaries(x, ci):
    """C6 on x [..., R]: mean, variance [...], quant [..., nC]."""
    n_rep = x.shape[-1]
    with np.errstate(all="ignore"):
        mean = R.b5_sum(x) / np.float64(n_rep)
        d = x - mean[..., None]
        variance = R.b5_sum(d * d) / np.float64(n_rep - 1) if n_rep > 1 else np.full(mean.shape, np.nan)
    srt = np.sort(x, axis=-1)
    quant = np.stack([srt[..., min(n_rep - 1, int(np.floor(np.float64(n_rep) * np.float64(c))))] for c in ci], axis=-1) if len(ci) \
        else np.zeros(x.shape[:-1] + (0,))
    return mean, variance, quant


def bootstrap(pnl, scen_flags, tail_probs, min_scen, n_rep, block, seed, ci_probs):
    """Rules C0-C9.  Returns var0, es0 [B,nL], n_scen int32 [B], mean, variance [B,2,nL], quant [B,2,nL,nC], rep [B,R,2,nL], and for the
    tests active [B] and counts (a list per row of [R,n] arrays, None for a row that is not active)."""
    pnl, fl = np.asarray(pnl, np.float64), np.asarray(scen_flags)
    B, window = pnl.shape
    tp, ci = np.asarray(tail_probs, np.float64).reshape(-1), np.asarray(ci_probs, np.float64).reshape(-1)
    nL, nC = len(tp), len(ci)
    assert 1 <= window <= 1024 and nL <= 8 and nC <= MAX_CI and min_scen >= 1 and 1 <= n_rep <= MAX_REP and 1 <= block <= MAX_BLOCK
    assert ((tp > 0) & (tp < 1)).all() and ((ci > 0) & (ci < 1)).all() and 0 <= seed <= M64
    var0, es0, n_scen, _ = H.tail(pnl, fl, tp, min_scen)                                     # C1
    rep = np.full((B, n_rep, 2, nL), np.nan)
    mean, variance, quant = np.full((B, 2, nL), np.nan), np.full((B, 2, nL), np.nan), np.full((B, 2, nL, nC), np.nan)
    active, counts = np.zeros(B, bool), [None] * B
    for p in range(B):
        v, rho = ranked(pnl[p], fl[p])
        n = len(v)
        active[p] = n >= min_scen and n > 0 and bool(np.isfinite(v).all())                  # C2
        if not active[p]:
            continue
        drawn = rho[positions(n, block, seed, n_rep)]                                        # [R, n] ranks
        cnt = np.zeros((n_rep, n), np.int64)
        np.add.at(cnt, (np.arange(n_rep)[:, None], drawn), 1)
        counts[p] = cnt
        before = np.cumsum(cnt, axis=1) - cnt
        for l, t in enumerate(tp):
            m = max(1, int(np.floor(np.float64(n) * t)))                                    # one IEEE product, as H7
            k = np.clip(m - before, 0, cnt)
            top = int((k > 0).any(axis=0).nonzero()[0].max()) + 1                           # no replicate walks past this rank
            terms = k[:, :top].astype(np.float64) * v[None, :top]                            # the product is rounded ...
            s = np.add.accumulate(np.concatenate([np.zeros((n_rep, 1)), terms], axis=1), axis=1)[:, -1]        # ... then the sum, serially from +0.0
            star = (np.cumsum(cnt, axis=1) >= m).argmax(axis=1)
            rep[p, :, 0, l] = 0.0 - v[star]
            rep[p, :, 1, l] = 0.0 - s / np.float64(m)
        if nL:
            x = rep[p].transpose(1, 2, 0)                                                    # [2, nL, R]
            mean[p], variance[p], quant[p] = summaries(x, ci)
    return dict(var0=var0, es0=es0, n_scen=n_scen, mean=mean, variance=variance, quant=quant, rep=rep, active=active, counts=counts)


class RefBackend(W.RefBackend):
    """CPU stand-in for a device backend with the bootstrap restated."""

    def bootstrap(self, pnl, scen_flags, tail_probs, min_scen, n_rep, block, seed, ci_probs, want_rep=False):
        r = bootstrap(pnl, scen_flags, tail_probs, min_scen, n_rep, block, seed, ci_probs)
        out = {k: r[k] for k in OUT_KEYS}
        with np.errstate(all="ignore"):
            out["se"] = np.sqrt(out["variance"])
        if not want_rep:
            out["rep"] = None
        return out
