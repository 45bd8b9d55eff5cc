"""The cases of rules W0-W9 and their tolerances.  TEST INFRASTRUCTURE ONLY.  A generated case is a case of
hedge_cases.generated (a book, its chain and nH candidates) with a ladder: `mult` [nQ] (one ladder for all snapshots) or [B,nQ] (a
ladder per snapshot), multiples of a size per candidate that `with_sizes` takes from the restated rows, so that a rung moves the
book's row by about its own magnitude.  A table (TABLES) is stage 2 alone on integer rows, every operation exact, worked out by
hand.  The micro cases are hedge_cases.MICRO with a ladder.  R_CPU has its measured source in profiles/whatif/errlog.txt."""
import numpy as np

import hedge_cases as GC
import hsim_cases as HC
import whatif_ref as W

EPS, TINY, NAN, INF = GC.EPS, GC.TINY, float("nan"), float("inf")
CALL, PUT, UND = GC.CALL, GC.PUT, GC.UND
NEG_VOL = 2
VALUE_KEYS, INT_KEYS = W.VALUE_KEYS, W.INT_KEYS

# R_CPU: the largest |fp64 restatement - the same rules in mpmath at 50 digits on the same rows, the restatement's ranked sets and
# live rungs taken as given| over the tables, the micro cases and the generated cases of MP_CASES, in units of eps x the value's own
# scale (whatif_ref's scale_<key>: z carries the rounding of q x and of the sum, an order statistic the largest of them over its
# row, es that plus the magnitudes of its tail and itself).  Measured by test_whatif.test_rounding_level (profiles/whatif/errlog.txt) and recorded here a
# third higher, rounded up.  var0 is an element of the row itself: its error is exactly 0.
# Measured: var_w 0.5965, es_w 0.2853, var0 0, es0 0.1481.
R_CPU = {"var_w": 0.796, "es_w": 0.381, "var0": 0.0, "es0": 0.198}
R_TERM = GC.R_TERM                                           # inst_pnl is a term of section 19 ...
R_ROW = HC.R_CPU["pnl"]                                      # ... and pnl its row
C_GPU = HC.C_GPU


def allowance(ref, k, factor=1.0):
    """What a value computed on rows of its own may differ from the restatement by: factor x (R_CPU x its own unit + the rows' unit at
    the rows' own level), in eps, plus the additive term.  The rows' level is the larger of section 19's row and term."""
    return factor * EPS * (R_CPU[k] * ref["scale_" + k] + max(R_ROW, R_TERM) * ref["rows_" + k]) + TINY


def ratios(got, ref, factor=1.0, keys=VALUE_KEYS):
    """|got - ref| over its allowance, per key."""
    out = {}
    with np.errstate(all="ignore"):
        for k in keys:
            d = np.abs(np.asarray(got[k], np.float64) - ref[k])
            out[k] = np.where(d == 0.0, 0.0, d / allowance(ref, k, factor))
    return out


# ------------------------------------------------------------------ generated cases
# B in {1, 2, 3, 9, 70, 260}, lag in {1, 2}, window in {1, 2, 4, 63, 64, 65, 257, 1024}, mT in {1, 2, 16}, nH in {1, 2, 3, 63, 64}, nQ
# in {1, 2, 15, 16}, nL in {0, 1, 2, 8}, shared and per-snapshot ladders, kinds 0, 1 and 2: every value at least once.  A window
# holds no more scenarios than the snapshots before it, so the windows of 257 and 1024 are full only in the tables; here they set
# the launch geometry (five and sixteen registers per lane) on the scenarios there are.
CASES = {
    "one": dict(B=1, mT=1, Q=1, lag=1, window=1, nL=0, nH=1, nQ=1, seed=2200, min_scen=1),
    "two_per": dict(B=2, mT=2, Q=2, lag=1, window=2, nL=1, nH=2, nQ=2, seed=2201, per=True, min_scen=1, per_ladder=True),
    "three_lag2": dict(B=3, mT=16, Q=2, lag=2, window=4, nL=2, nH=3, nQ=15, seed=2202, min_scen=1, kinds=[PUT, UND, CALL]),
    "nine_63": dict(B=9, mT=16, Q=65, lag=1, window=63, nL=8, nH=63, nQ=2, seed=2203, per=True, per_ladder=True),
    "nine_65": dict(B=9, mT=2, Q=3, lag=1, window=65, nL=1, nH=64, nQ=1, seed=2204),
    "seventy": dict(B=70, mT=16, Q=63, lag=1, window=64, nL=2, nH=3, nQ=16, seed=2205, min_scen=20),
    "second_word": dict(B=260, mT=2, Q=2, lag=1, window=257, nL=1, nH=2, nQ=2, seed=2206, min_scen=20),
    "sixteen_regs": dict(B=3, mT=1, Q=2, lag=1, window=1024, nL=2, nH=2, nQ=2, seed=2207, min_scen=1),
}
CHAIN = ("three_lag2", "nine_63", "nine_65", "seventy", "second_word")    # value cases on the device's own rows: they meet the conditions
MP_CASES = ("two_per", "three_lag2", "nine_63", "seventy")
WIDE = dict(B=70, mT=2, Q=2, lag=1, window=64, nL=2, nH=64, nQ=16, seed=2208, min_scen=20)         # W8 and the stream test


def make(name):
    s = dict(WIDE if name == "wide" else CASES[name])
    nQ, per_ladder = s.pop("nQ"), s.pop("per_ladder", False)
    c = GC.generated(rounds=1, **s)
    r = np.random.default_rng(s["seed"] + 47)
    B = c["params"].shape[0]
    mult = np.sort(r.uniform(-1.5, 3.0, (B, nQ) if per_ladder else (nQ,)), axis=-1)
    return dict(c, mult=mult)


def with_sizes(c, pnl, inst_pnl):
    """The case with `size` [nH,nQ] or [B,nH,nQ]: mult x sqrt(sum pnl^2 / sum x_h^2) over the entries that are numbers, 1.0 for a
    candidate without one."""
    with np.errstate(all="ignore"):
        g = np.sqrt(np.nansum(np.square(pnl)) / np.nansum(np.square(inst_pnl), axis=(0, 1)))
    g = np.where(np.isfinite(g) & (g > 0.0), g, 1.0)
    m = c["mult"]
    size = g[:, None] * m[None, :] if m.ndim == 1 else g[None, :, None] * m[:, None, :]
    return dict(c, size=np.ascontiguousarray(size))


def check_conditions(r, factor=C_GPU):
    """What this file promises of a value case that runs on the device's own rows, for the restatement alone: no two z of a row that
    straddle a tail boundary (ranks m - 1 | m and 0 | 1) closer than the sum of their allowances, the best and the second-best ES of
    every (p, h, l) further apart than theirs, and at least 90 % of the (p, h) of the active snapshots usable."""
    level = max(R_ROW, R_TERM)
    for where, m, gap, own, rows in W.boundary_gaps(r):
        allow = factor * EPS * (own + level * rows)
        assert gap > allow, f"{where}: the z of ranks {m - 1} and {m} are {gap:.3e} apart, allowance {allow:.3e}"
    for where, gap, own, rows in W.best_gaps(r):
        allow = factor * EPS * (R_CPU["es_w"] * own + level * rows)
        assert gap > allow, f"{where}: the best and the second-best ES are {gap:.3e} apart, allowance {allow:.3e}"
    act = r["active"]
    if act.any():
        usable = (r["trade_flags"][act] == 0).mean()
        assert usable >= 0.9, f"only {usable:.0%} of the candidates of the active snapshots are usable"


# ------------------------------------------------------------------ micro cases: hedge_cases.MICRO through both stages
MICRO_LADDER = (0.0, 1.0, -0.5)
MICRO = {k: dict(v, size=np.tile(np.asarray(MICRO_LADDER), (len(v["inst_kind"]), 1))) for k, v in GC.MICRO.items()}


# ------------------------------------------------------------------ tables by hand: stage 2 on integer rows given directly
def table(y, x, size, tail_probs=(0.5,), min_scen=1, scen_flags=None, want=None):
    """hedge_cases.table's layout (one snapshot p = n behind n void ones) with a ladder `size` [nH][nQ]; want: {key: value at p}."""
    x = np.asarray(x, np.float64)
    t = GC.table(y, x, None, None, None, None, min_scen=min_scen, tail_probs=tail_probs, scen_flags=scen_flags)
    return dict(t, size=np.asarray(size, np.float64), want=want or {})


def _rows(n, a, b, c, d):
    s = np.arange(n)
    return ((s * a) % b - c).astype(np.float64), ((s * d) % 13 - 6).astype(np.float64)


_X = [[1, -1, 0], [-1, 1, 1], [2, -2, 1], [-2, 2, -1]]      # column 1 is the negation of column 0
_Y257, _X257 = _rows(257, 37, 11, 5, 101)
_Y1024, _X1024 = _rows(1024, 37, 23, 11, 101)
_Y257[[255, 256]] = -6.0                                     # the two smallest tie across the 256 boundary ...
_X257[[255, 256]] = 1.0
_Y1024[[3, 255, 256, 1023]] = -12.0                          # ... and here across the first and the last of sixteen registers
_X1024[[3, 255, 256, 1023]] = 2.0
TABLES = {
    # the book is -2 x candidate 0: q = 2 leaves nothing (var = es = +0.0, every scenario ties: the lowest s is the worst) and is the
    # best rung; q = 0 is the book itself; q = 1 halves it; q = 3 is the candidate alone.  m = max(1, floor(4 x 0.5)) = 2.  Candidate 1
    # is candidate 0 negated and its ladder too: the same rows, the same bits
    "minus_two": table([-2, 2, -4, 4], _X, [[0, 1, 2, 3], [-0.0, -1, -2, -3], [0.5, 1, 1.5, 2]],
                       want=dict(var_w0=[2.0, 1.0, 0.0, 1.0], es_w0=[3.0, 1.5, 0.0, 1.5], worst_w0=[2, 2, 0, 3], best0=2, var0=2.0, es0=3.0, worst0=2,
                                 n_scen=4, trade_flags=[0, 0, 0])),
    # a flagged scenario (s = 1) and a NaN P&L (s = 3) are not ranked (n = 3, m = max(1, floor(1.5)) = 1): candidate 1 is NaN in the ranked s = 2 (flagged, every rung
    # dead), candidate 2 only where nothing is ranked (usable; what it holds there is not read)
    "nan_columns": table([-2, 9, -2, NAN, -4], [[1, 1, 1], [5, NAN, NAN], [1, NAN, 1], [7, 0, NAN], [2, -1, 2]], [[0, 2], [0, 2], [0, 2]],
                         scen_flags=[0, HC.NEG, 0, 0, 0],
                         want=dict(trade_flags=[0, NEG_VOL, 0], var_w0=[4.0, 0.0], es_w0=[4.0, 0.0], worst_w0=[4, 0], worst_w1=[-1, -1], best1=-1,
                                   var_w2=[4.0, 0.0], n_scen=3, worst0=4, var0=4.0)),
    # a size that is not finite: that rung alone is dead
    "bad_size": table([-2, 2, -4, 4], _X, [[1, NAN, INF, 2], [-INF, 0, 1, NAN], [NAN, NAN, NAN, NAN]],
                      want=dict(var_w0=[1.0, NAN, NAN, 0.0], worst_w0=[2, -1, -1, 0], best0=3, best2=-1, trade_flags=[0, 0, 0])),
    # n < min_scen: inactive.  Every rung is dead, the base figures NaN; n_scen, worst0 and the flags stay as defined
    "too_few": table([-2, 2, -4, 4], _X, [[0, 1], [0, 1], [0, 1]], min_scen=5,
                     want=dict(var_w0=[NAN, NAN], es_w0=[NAN, NAN], worst_w0=[-1, -1], best0=-1, var0=NAN, es0=NAN, worst0=2, n_scen=4, trade_flags=[0, 0, 0])),
    # duplicated z: q = 1 makes every scenario 1; n = 6, m = 3 and max(1, floor(1.2)) = 1
    "ties_dup": table([1, 1, 1, 1, 0, 0], [[0], [0], [0], [0], [1], [1]], [[1, 0]], tail_probs=(0.5, 0.2),
                      want=dict(var_w0=[[-1.0, -1.0], [-1.0, 0.0]], es_w0=[[-1.0, -1.0], [-1.0 / 3.0, 0.0]], worst_w0=[0, 4])),
    # -0.0 against +0.0: equal, the lower s first.  Candidate 0 is an all-zero column (H6 in every scenario): q = -1 makes every product
    # -0.0, so z keeps the zeros' signs; candidate 1 under q = 0.0 and -0.0
    "ties_zero": table([-0.0, 0.0, -0.0, 0.0], [[0, 1], [0, -1], [0, 1], [0, -1]], [[-1, 1], [0.0, -0.0]],
                       want=dict(var_w0=[0.0, 0.0], es_w0=[0.0, 0.0], worst_w0=[0, 0], var_w1=[0.0, 0.0], worst_w1=[0, 0], best0=0, trade_flags=[0, 0])),
    # n x tp just under and just over an integer (section 19's m_round): n = 10, m = 3, 2, 7, 6 and max(1, 0) = 1
    "m_round": table([3, -1, 4, -1, 5, -9, 2, -6, 5, -3], [[1], [2], [-1], [0], [3], [1], [-2], [2], [0], [1]], [[0, 1, -1]],
                     tail_probs=(0.3, 0.29999999999999993, 0.7, 0.6999999999999999, 0.05),
                     want=dict(var_w0=[[3.0, 6.0, -3.0, -2.0, 9.0], [2.0, 4.0, -3.0, -1.0, 8.0], [4.0, 8.0, -2.0, -2.0, 10.0]])),
    # a row that needs a fifth register per lane, and the longest there is
    "row_257": table(_Y257, _X257[:, None], [[0, 1, -1, 5]], tail_probs=(0.05, 0.5), want=dict(worst0=255, var0=[5.0, 0.0], n_scen=257)),
    "row_1024": table(_Y1024, _X1024[:, None], [[0, -3]], tail_probs=(0.01, 0.3), want=dict(worst0=3, n_scen=1024)),
}
