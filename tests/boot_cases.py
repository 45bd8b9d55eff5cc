"""The cases of rules C0-C9.  TEST INFRASTRUCTURE ONLY.  A generated case is a batch of rows of seeded
Student-t(4) P&Ls with flags and NaNs sprinkled in (and garbage under the flags), or `clean` rows where every scenario is ranked, so
that a block length given relative to n is exact.  A table (TABLES) is a row of integers where every operation is exact.  There are
no tolerances: the rules are a fixed sequence of IEEE and integer operations, and every comparison is to the bit."""
import numpy as np

NAN, INF = float("nan"), float("inf")
TP8 = (0.05, 0.01, 0.5, 0.25, 0.1, 0.9, 0.3, 0.7)
CI8 = (0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 0.999)

# B in {1, 3, 70}, window in {1, 2, 63, 64, 65, 256, 257, 1024}, R in {1, 2, 255, 256, 257, 1024}, L in {1, 2, 7, n - 1, n, n + 1, 1024},
# nL in {0, 1, 2, 8}, nC in {0, 1, 8}: every value at least once.  R = 255, 256, 257 and 1024 are one pass of C6 short of full, one full,
# one and a single term, and four; windows 63..65 and 256, 257 sit on either side of a wavefront's and of the workgroup's width.
CASES = {
    "w1": dict(B=1, window=1, R=1, L=1, nL=1, nC=1, min_scen=1, clean=True, seed=2300),
    "w2": dict(B=3, window=2, R=2, L=2, nL=2, nC=0, min_scen=1, clean=True, seed=2301),                  # L = n
    "w63": dict(B=3, window=63, R=255, L=7, nL=8, nC=8, min_scen=20, seed=2302),
    "w64": dict(B=70, window=64, R=256, L=63, nL=2, nC=1, min_scen=20, clean=True, seed=2303),           # L = n - 1
    "w65": dict(B=3, window=65, R=257, L=66, nL=1, nC=8, min_scen=20, clean=True, seed=2304),            # L = n + 1
    "w256": dict(B=3, window=256, R=1024, L=1, nL=2, nC=2, min_scen=20, seed=2305),                      # the defaults, four passes
    "w257": dict(B=1, window=257, R=2, L=1024, nL=0, nC=1, min_scen=20, seed=2306),                      # no level: n_scen alone
    "w1024": dict(B=3, window=1024, R=256, L=2, nL=2, nC=1, min_scen=20, seed=2307),
    "w1024_l7": dict(B=1, window=1024, R=2, L=7, nL=8, nC=1, min_scen=1000, seed=2308),                  # n < min_scen on a long row
}
DEFAULT_TP = (0.05, 0.01)


def rows(B, window, seed, clean=False):
    """pnl [B,window] and scen_flags [B,window]: Student-t(4); unless clean, 6 % of the scenarios flagged (with a number, a NaN or an
    infinity under the flag) and 3 % NaN without a flag."""
    r = np.random.default_rng(seed)
    pnl = r.standard_t(4, (B, window))
    fl = np.zeros((B, window), np.int32)
    if not clean:
        flagged = r.random((B, window)) < 0.06
        fl[flagged] = r.choice([1, 2, 4], int(flagged.sum()))                                # IVS_HS_*
        junk = r.choice([NAN, INF, -1e300, 7.0], (B, window))
        pnl = np.where(flagged, junk, pnl)
        pnl[(r.random((B, window)) < 0.03) & ~flagged] = NAN
    return pnl, fl


def make(name):
    s = dict(CASES[name])
    pnl, fl = rows(s["B"], s["window"], s["seed"], s.get("clean", False))
    nL, nC = s["nL"], s["nC"]
    tp = TP8[:nL] if nL != 2 else DEFAULT_TP
    ci = CI8[:nC] if nC != 2 else (0.05, 0.95)
    return dict(pnl=pnl, scen_flags=fl, tail_probs=tuple(tp), min_scen=s["min_scen"], n_rep=s["R"], block=s["L"], seed=s["seed"] * 7919 + 1,
                ci_probs=tuple(ci))


# ------------------------------------------------------------------ tables by hand: integer rows
def table(pnl, tail_probs=(0.5,), min_scen=1, n_rep=3, block=1, seed=23, ci_probs=(0.5,), scen_flags=None, want=None):
    pnl = np.atleast_2d(np.asarray(pnl, np.float64))
    fl = np.zeros(pnl.shape, np.int32) if scen_flags is None else np.atleast_2d(np.asarray(scen_flags, np.int32))
    return dict(pnl=pnl, scen_flags=fl, tail_probs=tuple(tail_probs), min_scen=min_scen, n_rep=n_rep, block=block, seed=seed,
                ci_probs=tuple(ci_probs), want=want or {})


def _tie_row(n, a, b, c, at, low):
    y = ((np.arange(n) * a) % b - c).astype(np.float64)
    y[at] = low
    return y


# The words of "four": seed 23, n = 4, L = 2, so two blocks per replicate.  b(r, i) = (u n) >> 32:
#   r = 0: 3, 2     r = 1: 1, 2     r = 2: 3, 3
# The row 3, -1, 2, -4 has v = -4, -1, 2, 3 and rho = 3, 1, 2, 0.  m = max(1, floor(4 x 0.5)) = 2.
#   r = 0: positions 3, 0 | 2, 3 (block 0 wraps past n - 1): ranks 0, 3, 2, 0, counts 2, 0, 1, 1: sum = 2 x -4, var* = 4, es* = 4
#   r = 1: positions 1, 2 | 2, 3: ranks 1, 2, 2, 0, counts 1, 1, 2, 0: sum = -4 + -1, var* = 1, es* = 2.5
#   r = 2: positions 3, 0 | 3, 0: counts 2, 0, 0, 2: var* = 4, es* = 4
# mean = 3 and 3.5; variance = (1 + 4 + 1) / 2 = 3 and (0.25 + 1 + 0.25) / 2 = 0.75; the median (i = min(2, floor(1.5)) = 1) is 4 and 4
FOUR_WORDS = [[3, 2], [1, 2], [3, 3]]
TABLES = {
    "four": table([3, -1, 2, -4], block=2,
                  want=dict(rep=[[[4.0], [4.0]], [[1.0], [2.5]], [[4.0], [4.0]]], mean=[[3.0], [3.5]], variance=[[3.0], [0.75]], quant=[[[4.0]], [[4.0]]],
                            var0=[1.0], es0=[2.5], n_scen=4)),
    # a row that rises with s at L = ceil(n / 2): two blocks, which often coincide, and then no rank below about n / 2 is drawn
    "rising": table(np.arange(64) - 20, tail_probs=(0.05, 0.25), n_rep=64, block=32, ci_probs=(0.05, 0.95)),
    # duplicated values: n = 6, m = 3 and max(1, floor(1.2)) = 1
    "dup": table([1, 1, 1, 1, 0, 0], tail_probs=(0.5, 0.2), n_rep=16, block=2),
    # -0.0 against +0.0: equal, the lower s first; every figure that is zero is +0.0
    "zeros": table([-0.0, 0.0, -0.0, 0.0, 1, 1], tail_probs=(0.5, 0.2), n_rep=16),
    # the smallest values tie across position 256 (the second pass of the ranking) and across the ends of the longest row
    "tie_257": table(_tie_row(257, 37, 11, 5, [255, 256], -6.0), tail_probs=(0.05, 0.01), n_rep=8, block=3, want=dict(var0=[5.0, 6.0], n_scen=257)),
    "tie_1024": table(_tie_row(1024, 37, 23, 11, [3, 255, 256, 1023], -12.0), tail_probs=(0.01, 0.3), n_rep=4, block=1024, want=dict(n_scen=1024)),
    # n x tp just under and just over an integer: n = 10, m = 3, 2, 7, 6 and max(1, 0) = 1
    "m_round": table([3, -1, 4, -1, 5, -9, 2, -6, 5, -3], tail_probs=(0.3, 0.29999999999999993, 0.7, 0.6999999999999999, 0.05), n_rep=16, block=4,
                     want=dict(var0=[3.0, 6.0, -3.0, -2.0, 9.0])),          # L' = 4 does not divide n = 10: blocks of 4, 4 and 2
    # n < min_scen: not active, NaN everywhere; n_scen stays
    "too_few": table([-2, 2, -4, 4], min_scen=5, want=dict(var0=[NAN], es0=[NAN], n_scen=4, mean=[[NAN], [NAN]], variance=[[NAN], [NAN]], quant=[[[NAN]], [[NAN]]])),
    # an infinite ranked value: not active (C2), yet var0 and es0 are H7's
    "infinite": table([-2, 2, -INF, 4], want=dict(var0=[2.0], es0=[INF], n_scen=4, mean=[[NAN], [NAN]], variance=[[NAN], [NAN]])),
    # a NaN and garbage under a flag do not matter: the two rows rank the same five scenarios
    "garbage": table([[5, NAN, -3, 1e300, 2, -7, 0, INF], [5, -INF, -3, NAN, 2, -7, 0, -1]], scen_flags=[[0, 4, 0, 2, 0, 0, 0, 1], [0, 1, 0, 0, 0, 0, 0, 2]],
                     tail_probs=(0.4,), n_rep=16, block=2, want=dict(n_scen=[5, 5], var0=[[3.0], [3.0]])),
    # R = 1: the variance is NaN, every quantile is the one value
    "one_rep": table([3, -1, 2, -4], n_rep=1, want=dict(variance=[[NAN], [NAN]])),
}
