"""The cases of rules W0-W9.  TEST INFRASTRUCTURE ONLY.  A generated case is a batch of rows drawn as
boot_cases draws them (seeded Student-t(4), 6 % of the scenarios flagged with a number, a NaN or an infinity underneath, 3 % NaN) with
a positive random-walk spot.  A table (TABLES) is a row where every operation is exact or short enough to follow by hand.  There are
no tolerances but one: sigma ends in a square root (1 ulp on the device); everything after it is compared to the bit."""
import numpy as np

import boot_cases as BC

NAN, INF = float("nan"), float("inf")
TP8 = (0.05, 0.01, 0.5, 0.25, 0.1, 0.3, 0.2, 0.4)        # every level <= 0.5: the target is reached before the ranks run out
DEFAULT_TP = (0.05, 0.01)

# B in {1, 3, 70}, window in {1, 2, 63, 64, 65, 256, 257, 1024}, lag in {1, 2, 5}, M in {0, 1, 2, 64, 65, 1024}, decay in {1.0, 0.99, 0.94, 0.5},
# nL in {0, 1, 2, 8}: every value at least once.  Windows 63..65 and 256, 257 sit on either side of a wavefront's and of the workgroup's
# width (a second pass of W5 with one term).  decay 0.5 runs into the subnormals inside a window of 1024 (w_1023 = 2^-1023) and its
# squares underflow to 0 from s = 538 on; decay 0.25 (an extra case) reaches 0 itself at s = 538: zero weights on ranked scenarios.
# decay None is weight = NULL.  With M > 0 and B = 70 the rows p < 20 + lag have fewer than min_scen scenarios with a vol: not active.
CASES = {
    "w1": dict(B=1, window=1, lag=1, M=0, decay=1.0, nL=1, min_scen=1, seed=2400),
    "w2": dict(B=3, window=2, lag=2, M=1, decay=0.5, nL=2, min_scen=1, seed=2401),
    "w63": dict(B=70, window=63, lag=5, M=2, decay=0.94, nL=8, min_scen=20, seed=2402),
    "w64": dict(B=70, window=64, lag=1, M=64, decay=0.99, nL=2, min_scen=20, seed=2403),
    "w65": dict(B=70, window=65, lag=2, M=65, decay=None, nL=1, min_scen=20, seed=2404, min_returns=20),
    "w256": dict(B=70, window=256, lag=1, M=0, decay=0.99, nL=2, min_scen=20, seed=2405),                # the defaults
    "w257": dict(B=3, window=257, lag=1, M=1024, decay=0.94, nL=0, min_scen=1, seed=2406),              # no level
    "w1024": dict(B=3, window=1024, lag=1, M=0, decay=0.5, nL=2, min_scen=20, seed=2407),
    "w1024_zero": dict(B=1, window=1024, lag=1, M=0, decay=0.25, nL=8, min_scen=1000, seed=2408),       # n < min_scen on a long row
    "w1024_vol": dict(B=70, window=1024, lag=5, M=1024, decay=0.99, nL=2, min_scen=20, seed=2409, cap=1.25),
}


def spot_walk(B, seed):
    r = np.random.default_rng(seed + 100000)
    return 100.0 * np.cumprod(1.0 + 0.01 * r.standard_normal(B))


def age_weights(window, decay):
    w, x = np.empty(window), np.float64(1.0)
    for s in range(window):
        w[s] = x
        x = x * np.float64(decay)
    return w


def make(name):
    s = dict(CASES[name])
    pnl, fl = BC.rows(s["B"], s["window"], s["seed"])
    nL, M = s["nL"], s["M"]
    tp = TP8[:nL] if nL != 2 else DEFAULT_TP
    return dict(pnl=pnl, scen_flags=fl, spot=spot_walk(s["B"], s["seed"]), lag=s["lag"], tail_probs=tuple(tp), min_scen=s["min_scen"],
                weight=None if s["decay"] is None else age_weights(s["window"], s["decay"]), vol_span=M,
                vol_weight=age_weights(M, 0.94) if M else None, min_returns=s.get("min_returns", 1), scale_cap=s.get("cap", 3.0))


# ------------------------------------------------------------------ tables by hand
def table(pnl, tail_probs=(0.5,), min_scen=1, weight=None, scen_flags=None, spot=None, lag=1, vol_span=0, vol_weight=None, min_returns=1,
          scale_cap=3.0, want=None):
    pnl = np.atleast_2d(np.asarray(pnl, np.float64))
    fl = np.zeros(pnl.shape, np.int32) if scen_flags is None else np.atleast_2d(np.asarray(scen_flags, np.int32))
    return dict(pnl=pnl, scen_flags=fl, spot=None if spot is None else np.asarray(spot, np.float64), lag=lag, tail_probs=tuple(tail_probs),
                min_scen=min_scen, weight=None if weight is None else np.asarray(weight, np.float64), vol_span=vol_span,
                vol_weight=None if vol_weight is None else np.asarray(vol_weight, np.float64), min_returns=min_returns, scale_cap=scale_cap,
                want=want or {})


def _grid(B, window, seed):
    """Small integers, no two equal in a row: every product with a power of two is exact."""
    r = np.random.default_rng(seed)
    return np.stack([r.permutation(4 * window)[:window] - 2.0 * window for _ in range(B)])


G7, G6 = 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6
GROW7 = G7 ** np.arange(8)                               # 49 bits at most: every spot, quotient and difference is exact
STEPS = np.cumprod([1.0, G7, G7, G7, G6, G6, G6, G7])    # 47 bits at most; sigma = nan, a, a, a, 2a, 2a, 2a, a with a = 2^-7 at M = 1
_A, _H = 2.0 ** -7, 0.5


def _steps_scale(lo, hi):
    """f[p][s] = sigma[p] / sigma[p - 1 - s] of STEPS at lag 1, window 6, held inside [lo, hi]; NaN where p - 1 - s < 1."""
    n = NAN
    return [[n] * 6, [n] * 6, [1, n, n, n, n, n], [1, 1, n, n, n, n], [hi, hi, hi, n, n, n], [1, hi, hi, hi, n, n], [1, 1, hi, hi, hi, n],
            [lo, lo, lo, 1, 1, 1]]


_M10 = [3, -1, 4, -1, 5, -9, 2, -6, 5, -3]               # sorted: -9, -6, -3, -1, -1, 2, 3, 4, 5, 5
_T_UNDER, _T_OVER = 0.29999999999999993, 0.30000000000000004        # x 10: 2.9999999999999996 and 3.0000000000000004; 0.3 x 10 is 3.0
TABLES = {
    # weights 1.0, n = 8, tp = 0.25: H7 takes m = 2 ranks, var = 6, es = (9 + 6) / 2.  W7: target = 2.0; rank 0: next = 1 < 2, sum = -9,
    # cum = 1; rank 1: next = 2 >= 2: sum = -9 + (2 - 1) x -6 = -15; var = 6, es = 15 / 2: H7's operations
    "h7_n8": table([3, -1, 4, -1.5, 5, -9, 2, -6], tail_probs=(0.25,),
                   want=dict(var_w=[6.0], es_w=[7.5], n_valid_w=8, worst_w=5, wsum=8.0, n_eff=8.0)),
    # n x tp at, just under and just over 3: the target is reached at rank 2 (next = 3 >= 3.0 and >= 2.99...96: NOT H7, whose m would be 2)
    # and at rank 3 (3 < 3.00...04, then 4)
    "m_round": table(_M10, tail_probs=(0.3, _T_UNDER, _T_OVER),
                     want=dict(var_w=[3.0, 3.0, 1.0], es_w=[(15.0 + 1.0 * 3.0) / 3.0, (15.0 + (_T_UNDER * 10.0 - 2.0) * 3.0) / (_T_UNDER * 10.0),
                                                            (18.0 + (_T_OVER * 10.0 - 3.0) * 1.0) / (_T_OVER * 10.0)])),
    # a fractional boundary: z by age -4, 2, -1, 3 with w 1, 1/2, 1/4, 1/4: W = 2, W2 = 1.375.  In rank order z = -4, -1, 2, 3, w = 1, 1/4, 1/2, 1/4.
    #   tp 0.5: target 1: rank 0 reaches it: sum = 1 x -4: var 4, es 4
    #   tp 0.75: target 1.5: sum = -4, cum = 1; sum = -4.25, cum = 1.25; rank 2: next = 1.75: sum = -4.25 + 0.25 x 2 = -3.75: var -2, es 2.5
    #   tp 0.25: target 0.5: rank 0: sum = 0.5 x -4: var 4, es 4
    "fraction": table([-4, 2, -1, 3], tail_probs=(0.5, 0.75, 0.25), weight=[1, 0.5, 0.25, 0.25],
                      want=dict(var_w=[4.0, -2.0, 4.0], es_w=[4.0, 2.5, 4.0], wsum=2.0, n_eff=4.0 / 1.375, worst_w=0, n_valid_w=4)),
    # the smallest values tie across position 256 (the second pass) and across the ends of the longest row.  tie_257: ranks 0, 1 are the
    # two -6 (s = 255 first), ranks 2..25 the 24 values -5: target 12.85 is reached at rank 12 and 2.57 at rank 2, both -5 (H7: 5 and 6)
    "tie_257": table(BC._tie_row(257, 37, 11, 5, [255, 256], -6.0), tail_probs=(0.05, 0.01), want=dict(var_w=[5.0, 5.0], worst_w=255, n_valid_w=257)),
    # four -12, then 45 values -11: target 10.24 is reached at rank 10
    "tie_1024": table(BC._tie_row(1024, 37, 23, 11, [3, 255, 256, 1023], -12.0), tail_probs=(0.01, 0.3), want=dict(worst_w=3, n_valid_w=1024, wsum=1024.0)),
    # -0.0 against +0.0: equal, the lower s first; target 3 is reached at rank 2, a -0.0: the sum stays +0.0 and var = 0.0 - -0.0 = +0.0
    "zeros": table([-0.0, 0.0, -0.0, 0.0, 1, 1], tail_probs=(0.5, 0.2), want=dict(var_w=[0.0, 0.0], es_w=[0.0, 0.0], worst_w=0)),
    # a zero weight at rank 0: it is ranked and the worst, adds 0 x -5 = -0.0 to +0.0 and no mass.  target 1.5: sum = 1, cum = 1; rank 2: 1 + 0.5 x 2
    "zero_first": table([-5, 1, 2, 3], weight=[0, 1, 1, 1], want=dict(var_w=[-2.0], es_w=[-2.0 / 1.5], worst_w=0, n_valid_w=4, wsum=3.0, n_eff=3.0)),
    # a NaN, an infinite and a negative weight: the bit on that scenario of every row, and it is not ranked.  Left: 1, 2, 3 (row 0), target 1.5
    "bad_weights": table([[1, -9, -8, -7, 2, 3], [7, 1, 1, 1, 9, 8]], weight=[1, NAN, INF, -1, 1, 1],
                         want=dict(flags_w=[[0, 16, 16, 16, 0, 0]] * 2, n_valid_w=[3, 3], var_w=[[-2.0], [-8.0]], es_w=[[-2.0 / 1.5], [-(7.0 + 0.5 * 8.0) / 1.5]],
                                   pnl_w=[[1, NAN, NAN, NAN, 2, 3], [7, NAN, NAN, NAN, 9, 8]], wsum=[3.0, 3.0])),
    # a flag and the new bits side by side; garbage under the flag does not matter
    "flag_and_bit": table([[5, INF, -3, 2], [5, NAN, -3, 2]], scen_flags=[[0, 4, 0, 0]] * 2, weight=[1, -1, 1, 1],
                          want=dict(flags_w=[[0, 20, 0, 0]] * 2, n_valid_w=[3, 3], var_w=[[-2.0]] * 2)),
    # n < min_scen: not active, NaN; the counts and masses stay
    "too_few": table([-2, 2, -4, 4], min_scen=5, want=dict(var_w=[NAN], es_w=[NAN], n_valid_w=4, worst_w=2, wsum=4.0, n_eff=4.0)),
    # W = 0: not active, and n_eff is NaN
    "no_mass": table([1, 2, 3], weight=[0, 0, 0], want=dict(var_w=[NAN], es_w=[NAN], n_valid_w=3, worst_w=0, wsum=0.0, n_eff=NAN)),
    # no ranked scenario at all
    "nothing": table([NAN, 1, 2], scen_flags=[0, 1, 2], want=dict(var_w=[NAN], n_valid_w=0, worst_w=-1, wsum=0.0, n_eff=NAN)),
    # a spot that grows by exactly 1 + 2^-7 per snapshot: r = 2^-7 and r r = 2^-14 exactly, so num = 2^-14 den whatever the a_k and every
    # sigma is 2^-7; f = 1.0 and pnl_w carries pnl's bits.  Scenario s of p starts at p - 1 - s, which has a vol from 1 on.
    "grow7": table(_grid(8, 4, 11), spot=GROW7, vol_span=3, vol_weight=[1.0, 0.94, 0.94 * 0.94], tail_probs=(0.5, 0.25),
                   want=dict(sigma=[NAN] + [_A] * 7,
                             scale=[[1.0 if p - 1 - s >= 1 else NAN for s in range(4)] for p in range(8)],
                             flags_w=[[0 if p - 1 - s >= 1 else 8 for s in range(4)] for p in range(8)],
                             n_valid_w=[0, 0, 1, 2, 3, 4, 4, 4])),
    # three such steps, three of 1 + 2^-6, one more of 1 + 2^-7, at M = 1: f is 1/2, 1 or 2 exactly; and held inside [1 / 1.5, 1.5]
    "steps": table(_grid(8, 6, 12), spot=STEPS, vol_span=1, vol_weight=[0.75], tail_probs=(0.5,),
                   want=dict(sigma=[NAN, _A, _A, _A, 2 * _A, 2 * _A, 2 * _A, _A], scale=_steps_scale(_H, 2.0))),
    "steps_cap": table(_grid(8, 6, 12), spot=STEPS, vol_span=1, vol_weight=[0.75], tail_probs=(0.5,), scale_cap=1.5,
                       want=dict(scale=_steps_scale(1.0 / 1.5, 1.5))),
    # a NaN, a zero and an infinite spot inside the span of M = 3: the returns 2, 3, 5, 6, 7, 8 are invalid; a sigma needs one of its three
    "bad_spot": table(_grid(10, 3, 13), spot=[100, 101, NAN, 102, 103, 0, 104, INF, 105, 106], vol_span=3, vol_weight=[1, 1, 1], tail_probs=(0.5,),
                      want=dict(sigma_finite=[0, 1, 1, 1, 1, 1, 1, 0, 0, 1])),
    # fewer than min_returns = 3 terms: no sigma before snapshot 3; at lag 2 scenario s of p has a vol iff p >= 3 and p - 2 - s >= 3
    "few_returns": table(_grid(8, 4, 14), spot=100.0 + np.arange(8.0) ** 2, lag=2, vol_span=4, vol_weight=[1, 0.5, 0.25, 0.125], min_returns=3,
                         tail_probs=(0.5,), want=dict(sigma_finite=[0, 0, 0, 1, 1, 1, 1, 1],
                                                      flags_w=[[0 if p >= 3 and p - 2 - s >= 3 else 8 for s in range(4)] for p in range(8)])),
    # an a_k that is not finite and >= 0 spoils the sigmas whose sum it takes part in: a_1 is used from snapshot 2 on
    "bad_vol_weight": table(_grid(5, 2, 15), spot=[100, 101, 103, 102, 104], vol_span=2, vol_weight=[1, -1], tail_probs=(0.5,),
                            want=dict(sigma_finite=[0, 1, 0, 0, 0])),
}


def check_want(name, t, got):
    """The hand-made values of a table against `got` (host arrays by output)."""
    for k, v in t["want"].items():
        if k == "sigma_finite":
            assert np.isfinite(got["sigma"]).tolist() == [bool(x) for x in v], (name, k)
            continue
        g = np.asarray(got[k])
        g = g[0] if np.ndim(v) < g.ndim else g
        assert np.array_equal(g, np.asarray(v, g.dtype).reshape(g.shape), equal_nan=True), (name, k, g, v)
