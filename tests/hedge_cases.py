"""The cases of rules M0-M11 and their tolerances.  TEST INFRASTRUCTURE ONLY.  A case is a case of hsim_cases
(the book whose row is hedged) with the candidates `inst_u`, `inst_tau` ([nH] or [B,nH], read under the case's strike_mode),
`inst_kind` (uint8 [nH]) and the settings `rounds`, `n_forced`, `tol`, `min_gain`.  A table (TABLES) is stage 2 alone: rows given
directly, worked out by hand.  The constants R_CPU below have their measured source in profiles/hedge/errlog.txt."""
import numpy as np

import hsim_cases as HC

EPS, TINY, NAN = HC.EPS, HC.TINY, float("nan")
CALL, PUT, UND = 0, 1, 2
DEAD, NEG_VOL, FLAT, SPENT, CHOSEN = 1, 2, 4, 8, 16
VALUE_KEYS = ("ss", "hedge", "pnl_hedged", "var_h", "es_h", "solo_qty", "solo_left")
INT_KEYS = ("inst_flags", "pick", "n_rounds", "worst_h", "n_scen")

# R_CPU: the largest |fp64 restatement - the same rules in mpmath at 50 digits, the restatement's picks taken as given| over the
# tables and the generated cases on which mpmath stays affordable (MP_CASES), in units of eps x the value's scale (hedge_ref's
# scale_<key>: the first-order propagation of every rounding of M3-M10 through the operations after it, the rows taken as exact).
# Measured by test_hedge.test_rounding_level (profiles/hedge/errlog.txt) and recorded here a third higher, rounded up.  The GPU
# tests allow hsim_cases.C_GPU x R_CPU.  The scales count every rounding of a serial sum at the sum of the magnitudes, so the
# figures stay well below 1.
# Measured: ss 0.1661, hedge 0.1329, pnl_hedged 0.1340, var_h 0.0537, es_h 0.0276, solo_qty 0.1461, solo_left 0.1394 (the shallow
# cases set them: one or two rounds on a few scenarios, where the unit is small; the quantities and the hedged row of the forced set of eight stay below 1e-5 of their units).
R_CPU = {"ss": 0.222, "hedge": 0.178, "pnl_hedged": 0.179, "var_h": 0.072, "es_h": 0.037, "solo_qty": 0.195, "solo_left": 0.186}
R_TERM = HC.R_CPU["pnl"]                                     # inst_pnl is a term of section 19
C_GPU = HC.C_GPU


def units(got, ref, keys=VALUE_KEYS):
    """|got - ref| of every compared value in units of eps x its scale (the additive term taken off first)."""
    out = {}
    with np.errstate(all="ignore"):
        for k in keys:
            if got.get(k) is None:
                continue
            d = np.abs(np.asarray(got[k], np.float64) - ref[k])
            out[k] = np.where(d <= TINY, 0.0, (d - TINY) / (EPS * ref["scale_" + k]))
    return out


def allowance_ratios(got, ref, factor=1.0, keys=VALUE_KEYS):
    return {k: v / (factor * (R_TERM if k == "inst_pnl" else R_CPU[k])) for k, v in units(got, ref, keys).items()}


# ------------------------------------------------------------------ generated cases
def _slice_walks(c, seed):
    """An independent walk per slice on top of hsim_cases.path's four: a of slice t by up to 2 %, b by up to 1 %, m by up to 0.002."""
    r = np.random.default_rng(seed + 23)
    P = c["params"].copy()
    B, mT = P.shape[:2]
    for t in range(mT):
        P[:, t, 0] *= 1.0 + 0.02 * HC._walk(r, B)
        P[:, t, 1] *= 1.0 + 0.01 * HC._walk(r, B)
        P[:, t, 3] += 0.002 * HC._walk(r, B)
    return dict(c, params=P)


def candidates(c, nH, seed, kinds=None, spread=0):
    """nH candidates on the case's chain: moneyness 0.9 .. 1.1, expiries inside the tenors, calls and puts, the underlying first
    when there is room for more than one (kinds: the list to use instead).  spread: the first `spread` candidates expire just
    behind every other tenor, so that with a walk per slice each answers to a slice of its own and a forced set of them is no
    more collinear than the common delta makes it."""
    r = np.random.default_rng(seed + 31)
    B = c["params"].shape[0]
    tq = np.asarray(c["Tq"], np.float64).reshape(-1, c["params"].shape[1])[0]
    m = r.uniform(0.9, 1.1, nH)
    t = r.uniform(0.7 * tq.min(), 1.1 * tq.max(), nH)
    if spread:
        t[:spread] = 1.003 * tq[(1 + 2 * np.arange(spread)) % len(tq)]
    kind = r.integers(0, 2, nH).astype(np.uint8)
    if nH > 1:
        kind[0] = UND
    if kinds is not None:
        kind = np.asarray(kinds, np.uint8)
    if c["strike_mode"] == 1:                                # absolute strikes, the expiries a minute closer per snapshot
        n = np.arange(B, dtype=np.float64)[:, None]
        u, tau = np.tile(m * c["spot"][0], (B, 1)), np.ascontiguousarray(t[None, :] - HC.MINUTE * n)
    else:
        u, tau = m, t
    return dict(inst_u=u, inst_tau=tau, inst_kind=kind)


def generated(B, mT, Q, lag, window, nL, nH, rounds, seed, n_forced=0, per=False, indep=True, tol=1e-6, min_gain=1e-4, min_scen=3, kinds=None, spread=0):
    c = HC.path(B, mT, Q, lag, window, nL, seed, per, min_scen)
    if indep:
        c = _slice_walks(c, seed)
    return dict(c, **candidates(c, nH, seed, kinds, spread), rounds=rounds, n_forced=n_forced, tol=tol, min_gain=min_gain)


# B in {1, 2, 3, 9, 40, 70, 260}, lag in {1, 2}, window in {1, 2, 4, 63, 64, 65, 257}, mT in {1, 2, 16, 64}, nH in {1, 2, 3, 63, 64}, K in
# {1, 2, 8}, shared and per-snapshot candidates, kinds 0, 1 and 2: every value at least once.  Greedy value cases have K <= 2; the
# K = 8 value case forces its picks; `collinear` keeps hsim_cases.path's four walks alone.  260 / 257 is the smallest shape with a
# scenario in a second word of 256.  With a single ranked scenario every candidate explains the whole row and all gains tie, and with
# no more scenarios than picks the hedged row is rounding noise whose ranks tie: B <= 3 can give no more than two scenarios, so those
# cases are inactive by min_scen = 2 (they test stage 1, the flags and the inactive pattern), and the cases of 4 and 8 rounds ask for
# 20 scenarios.
CASES = {
    "one": dict(B=1, mT=1, Q=1, lag=1, window=1, nL=0, nH=1, rounds=1, seed=2100),
    "two_per": dict(B=2, mT=2, Q=2, lag=1, window=2, nL=1, nH=2, rounds=2, seed=2101, per=True, min_scen=2),
    "three_lag2": dict(B=3, mT=16, Q=2, lag=2, window=4, nL=2, nH=3, rounds=2, seed=2102, min_scen=2, kinds=[PUT, UND, CALL]),
    "nine_63": dict(B=9, mT=16, Q=65, lag=1, window=63, nL=8, nH=63, rounds=2, seed=2103, per=True),
    "forced8": dict(B=40, mT=16, Q=63, lag=1, window=65, nL=1, nH=64, rounds=8, n_forced=8, seed=2104, min_scen=20, spread=8),
    "collinear": dict(B=70, mT=16, Q=63, lag=1, window=64, nL=2, nH=3, rounds=2, seed=2105, indep=False),
    "wide_tenors": dict(B=9, mT=64, Q=2, lag=2, window=4, nL=1, nH=2, rounds=1, seed=2106, min_scen=2),
    "und_alone": dict(B=9, mT=2, Q=63, lag=1, window=63, nL=1, nH=1, rounds=1, seed=2107, kinds=[UND]),
    "second_word": dict(B=260, mT=2, Q=2, lag=1, window=257, nL=1, nH=2, rounds=2, seed=2108),
}
MP_CASES = ("one", "two_per", "three_lag2", "nine_63", "wide_tenors", "und_alone")
DEEP = dict(B=260, mT=2, Q=2, lag=1, window=257, nL=1, nH=64, rounds=8, seed=2110, min_scen=20)       # deep greedy: invariants and bits only
STREAM = dict(B=70, mT=16, Q=63, lag=1, window=64, nL=2, nH=64, rounds=4, seed=2111, per=True, min_scen=20)


def make(name):
    s = DEEP if name == "deep" else STREAM if name == "stream" else CASES[name]
    return generated(**s)


# ------------------------------------------------------------------ micro cases on chains of hsim_cases.MICRO: both stages
def micro(name, inst_u, inst_tau, inst_kind, pnl, flags, want_flags, want_pick, rounds=2, min_gain=0.0, **more):
    """A chain of hsim_cases.MICRO with candidates of its own and a book's row given directly (pnl, scen_flags [B,window]: what is
    ranked is chosen here, whatever the chain's own book would give); `want`: inst_flags [B,nH] and pick [B,rounds] by hand."""
    m = HC.MICRO[name]
    return dict(m, inst_u=np.asarray(inst_u, np.float64), inst_tau=np.asarray(inst_tau, np.float64), inst_kind=np.asarray(inst_kind, np.uint8),
                pnl=np.asarray(pnl, np.float64), row_flags=np.asarray(flags, np.int32), rounds=rounds, n_forced=0, tol=1e-6, min_gain=min_gain,
                tail_probs=(0.5,), min_scen=1, want=dict(inst_flags=want_flags, pick=want_pick), **more)        # None: a row not worked out by hand


_T = 1.5 * HC.TAU
_ALL = DEAD | NEG_VOL | FLAT
MICRO = {
    # a dead candidate (bad strike), one with sigma' < 0 in a ranked scenario (the start of the pair (0, 1) has 16 x the variance) and
    # the underlying.  p = 1 ranks that scenario: the option is NEG_VOL | FLAT, the underlying picked; p = 2 ranks it as s = 1 too
    "dead_and_neg_vol": micro("neg_vol", [NAN, 1.0, 1.0], [0.3, _T, 1.0], [CALL, CALL, UND], [[NAN, NAN], [1.0, NAN], [-2.0, 0.5]],
                              [[1, 1], [0, 1], [0, 0]], [[DEAD | FLAT, FLAT, FLAT], [_ALL, NEG_VOL | FLAT, CHOSEN], [_ALL, NEG_VOL | FLAT, CHOSEN]],
                              [[-1, -1], [2, -1], [2, -1]]),
    # H6: snapshots 0 and 1 carry the same bits, so the pair (0, 1) gives every candidate exactly +0.0, the underlying too: at p = 1 it
    # is the only scenario and all three are FLAT; at p = 2 it is s = 1 beside a scenario that moves
    "h6_pair": micro("same_pair", [0.95, 1.05, 1.0], [_T, 0.6 * HC.TAU, 1.0], [CALL, PUT, UND], [[NAN, NAN], [1.0, NAN], [-2.0, 0.5]],
                     [[1, 1], [0, 1], [0, 0]], [[FLAT, FLAT, FLAT], [FLAT, FLAT, FLAT], None], [[-1, -1], [-1, -1], None]),
    # a snapshot whose spot is NaN (no live slice) and one whose tenors are out of order: degenerate, the underlying is DEAD there,
    # every scenario that touches it is void, inst_value NaN
    "dead_snapshot": micro("bad_spot_nan", [1.0, 1.0], [_T, 1.0], [CALL, UND], [[NAN] * 3, [NAN] * 3, [NAN] * 3, [0.7, NAN, NAN]],
                           [[1, 1, 1], [2, 1, 1], [2, 2, 1], [0, 2, 2]], [[FLAT, FLAT], [DEAD | FLAT, DEAD | FLAT], [FLAT, FLAT], None],
                           [[-1, -1]] * 3 + [None], dead_at=1),
    "unordered_snapshot": micro("unordered", [1.0, 1.0], [_T, 1.0], [CALL, UND], [[NAN] * 3, [NAN] * 3, [NAN] * 3, [0.7, NAN, NAN]],
                                [[1, 1, 1], [2, 1, 1], [2, 2, 1], [0, 2, 2]], [[FLAT, FLAT], [DEAD | FLAT, DEAD | FLAT], [FLAT, FLAT], None],
                                [[-1, -1]] * 3 + [None], dead_at=1),
}


# ------------------------------------------------------------------ tables by hand: stage 2 on rows given directly
def table(y, x, picks, hedge, ss, flags, rounds=2, n_forced=0, tol=1e-6, min_gain=1e-4, min_scen=1, tail_probs=(0.5,), scen_flags=None):
    """One snapshot p = n (so that all n scenarios exist at lag 1) behind n void ones.  y [n], x [n][nH]; what must come out for
    it: picks [rounds], hedge [nH], ss [rounds+1] or None, flags [nH].  The chain under it (two good slices, every candidate a live
    call) only says that no candidate is dead."""
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    n, nH = x.shape
    B = n + 1
    pnl, fl = np.full((B, n), NAN), np.full((B, n), HC.VOID, np.int32)
    pnl[n], fl[n] = y, (0 if scen_flags is None else scen_flags)
    X = np.full((B, n, nH), NAN)
    X[n] = x
    chain = dict(params=np.tile(np.asarray([HC.GOOD, HC.LATER], np.float64), (B, 1, 1)), Tq=np.asarray([HC.TAU, 2 * HC.TAU]), spot=np.full(B, 100.0),
                 rate=0.03, strike_mode=0, inst_u=np.linspace(0.95, 1.05, nH), inst_tau=np.full(nH, 1.5 * HC.TAU), inst_kind=np.zeros(nH, np.uint8))
    return dict(chain, pnl=pnl, scen_flags=fl, inst_pnl=X, lag=1, window=n, rounds=rounds, n_forced=n_forced, tol=tol, min_gain=min_gain,
                min_scen=min_scen, tail_probs=tuple(tail_probs), nH=nH, want=dict(pick=picks, hedge=hedge, ss=ss, inst_flags=flags))


_X2 = [[1, 0], [0, 1], [1, 1], [2, -1]]                      # integer rows: every operation below is exact
TABLES = {
    # the book is -2 x candidate 0: one round removes everything, the quantity to add is 2
    "minus_two": table([-2, 0, -2, -4], _X2, [0, -1], [2.0, 0.0], [24.0, 0.0, 0.0], [CHOSEN, 0]),
    # y = 3 x0 - x1: round 0 picks 0 (gain 19^2 / 6 against 6^2 / 3), round 1 picks 1; the pair reproduces y (t_0 = 19 / 6 is rounded)
    "both": table([3, -1, 2, 7], _X2, [0, 1], [-3.0, 1.0], None, [CHOSEN, CHOSEN], min_gain=0.0),
    # the same candidate twice: the second has g_1 = 0 after the first pick and is SPENT, never picked
    "twice": table([1, 2, 3, 5], [[1, 1], [0, 0], [1, 1], [2, 2]], [0, -1], None, None, [CHOSEN, SPENT], min_gain=0.0),
    # a FLAT candidate (every scenario an H6 pair: +0.0) and one that is NaN in a ranked scenario
    "flat_nan": table([1, 2, 3, 5], [[0, 1, 1], [0, NAN, 0], [0, 1, 1], [0, 2, 2]], [2, -1], None, None, [FLAT, NEG_VOL | FLAT, CHOSEN]),
    # forced on a FLAT candidate: round 0 is empty, the greedy rounds go on
    "forced_flat": table([1, 2, 3, 5], [[0, 1], [0, 0], [0, 1], [0, 2]], [-1, 1, -1], None, None, [FLAT, CHOSEN], rounds=3, n_forced=1),
    # min_gain stops: candidate 0 explains a quarter of y's sum of squares, below the half that is asked
    "min_gain": table([0, 0, 0, 5], [[1], [1], [1], [1]], [-1, -1], [0.0], [25.0, 25.0, 25.0], [0], min_gain=0.5),
    # n < min_scen: inactive
    "too_few": table([1, 2, 3, 5], _X2, [-1, -1], [NAN, NAN], [NAN, NAN, NAN], [0, 0], min_scen=5),
    # a flagged scenario and a NaN P&L are not ranked: the NaN of candidate 1 there does not count
    "unranked": table([-2, 9, -2, NAN, -4], [[1, 0], [5, NAN], [1, NAN], [7, NAN], [2, -1]], [0, -1], [2.0, 0.0], [24.0, 0.0, 0.0],
                      [CHOSEN, NEG_VOL | FLAT], scen_flags=[0, HC.NEG, 0, 0, 0]),
}
