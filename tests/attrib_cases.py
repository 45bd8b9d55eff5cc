"""The cases of rules A0-A8 and their tolerances.  TEST INFRASTRUCTURE ONLY.  A case is a case of
hsim_cases (micro table or seeded path) with the tail probabilities of its own and two more entries: `group` (int32 [Q] or None =
every option in group 0) and `nG`.  The constants R_CPU below have their measured source in profiles/attrib/errlog.txt."""
import numpy as np

import hsim_cases as HC

EPS, TINY = HC.EPS, HC.TINY
VALUE_KEYS = ("ces", "cvar", "ces_group", "cvar_group")

# R_CPU: the largest |fp64 restatement - the same rules in mpmath at 50 digits| over the micro tables and the generated shapes on
# which mpmath stays affordable (MP_CASES), in units of eps x the value's scale (attrib_ref's scale_<key>).  A component VaR is one
# term: its unit is hsim_ref's scale_terms and its R_CPU is hsim_cases.R_CPU["pnl"], which books of one option set.  The unit of a
# component ES is the mean of its m terms' units plus the m roundings of the serial sum (each bounded by eps x the sum of the
# terms' magnitudes) over m, plus two roundings of the quotient; a group's figures are the same with the B5 sum of its members in
# place of a term, whose unit is the sum of the members' units (each carries its depth-L share, as a scenario P&L's does).
# Measured by test_attrib.test_rounding_level (errlog.txt) and recorded here a third higher, rounded up.  The GPU tests allow
# hsim_cases.C_GPU x R_CPU, the project's standing margin for the device's erfc / exp / log / sqrt / division.
# Measured: ces 0.0422, cvar 0.0422, ces_group 0.0178, cvar_group 0.0178; a third higher 0.057, 0.057, 0.024, 0.024.  A component
# VaR is a term, so its constant is R_TERM.  The other three take the figure above, except where the value IS a smaller thing:
# with m = 1 a component ES is one term (R_TERM), a group with at most one live member is that member (its cvar_group a term,
# its ces_group that option's component ES), and no value may be held to less than what it reduces to.  `constants` has the table.
R_TERM = HC.R_CPU["pnl"]
R_CPU = {"ces": 0.057, "cvar": R_TERM, "ces_group": 0.024, "cvar_group": 0.024}
C_GPU = HC.C_GPU


def constants(ref):
    """R_CPU of every compared value, in the value's shape: [B,nL,Q] for ces and cvar, [B,nL,nG] for the group figures."""
    one = (ref["n_tail"] == 1)[:, :, None]                                               # m = 1: a tail of one scenario
    solo = (ref["members"] <= 1)[:, None, :]                                             # a group of at most one live option
    ces = np.where(one, R_TERM, R_CPU["ces"])
    return {"ces": np.broadcast_to(ces, ref["ces"].shape), "cvar": np.full(ref["cvar"].shape, R_TERM),
            "cvar_group": np.broadcast_to(np.where(solo, R_TERM, R_CPU["cvar_group"]), ref["cvar_group"].shape),
            "ces_group": np.where(solo, ces, R_CPU["ces_group"])}


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
    """units() over factor x the value's own constant: at most 1 where the value is inside its allowance."""
    k_ = constants(ref)
    return {k: v / (factor * k_[k]) for k, v in units(got, ref, keys).items()}


def with_groups(c, group, nG, **more):
    return dict(c, group=None if group is None else np.asarray(group, np.int32), nG=nG, **more)


# ------------------------------------------------------------------ micro cases: hsim_cases.MICRO with groups, and tables by hand
M = HC.MICRO
MICRO = {
    # a one-option book: ces == es and cvar == var to the bit
    "one_option": with_groups(M["one_option"], None, 1, tail_probs=(0.5, 0.9, 0.3)),
    # H6's pair in the tail: snapshot 1's only scenario is the pair with the same bits: +0.0 everywhere
    "same_pair": with_groups(M["same_pair"], [0, 1, 0, 1, 5], 2),
    # dead options (bad strike, bad expiry) and quantities that are not finite: NaN in ces and cvar, no part in a group
    "dead_options": with_groups(M["dead_options"], [0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2], 3),
    "quantities": with_groups(M["quantities"], [0, 1, 0, 1, 0], 2),
    # group ids outside 0..nG-1 (and negative): in no group
    "group_range": with_groups(M["lag_two"], [0, 2, -1, 1, 16], 2),
    # a group without a live member (group 1 holds the two dead quantities alone; group 2 nobody): +0.0
    "empty_group": with_groups(M["quantities"], [0, 1, 0, 1, 0], 3),
    # n < min_scen at snapshots 1 and 2, active at 3
    "too_few": with_groups(M["too_few"], [0, 0, 1, 1, 1], 2),
    # flagged scenarios: void pairs round the bad snapshot, NEG_VOL
    "bad_spot_nan": with_groups(M["bad_spot_nan"], None, 1),
    "neg_vol": with_groups(M["neg_vol"], [0, 1, 2, 3, 4], 5),
    "window_long": with_groups(M["window_long"], [3, 2, 1, 0, 0], 4, tail_probs=(0.5, 0.9, 0.1)),
    "b_le_lag": with_groups(M["b_le_lag"], None, 1),
    "hist_long_short": with_groups(M["hist_long_short"], [1, 0, 1], 2),
}

# A1 on rows given directly with ties and zeros of both signs: (pnl row, flags row, n_p, order)
ROWS = {
    "ties": ([1.0, -0.0, 0.0, 1.0, -0.0], [0] * 5, 5, [1, 2, 4, 0, 3]),
    "flagged": ([HC.NAN, -1.0, HC.NAN, 3.0, HC.NAN, -5.0], [2, 0, 4, 0, 1, 0], 6, [5, 1, 3]),
    "foreign": ([4.0, -1.0, 2.0, -3.0], [0, 0, 0, 0], 2, [1, 0]),            # s >= n_p is never ranked, whatever the row says
    "none": ([HC.NAN, HC.NAN], [2, 1], 2, []),
}


# ------------------------------------------------------------------ generated batches
def _path(B, mT, Q, lag, window, seed, levels, group, nG, per=False, min_scen=3, gen=HC.path):
    c = gen(B, mT, Q, lag, window, len(levels), seed, per, min_scen)
    g = None if group is None else np.asarray(group(np.arange(Q), Q), np.int32)
    return dict(c, tail_probs=tuple(levels), group=g, nG=nG)


CASES = {
    # M up to 16; sixteen groups dealt round the options, every 17th option in none
    "B70-Q63-w65": lambda: _path(70, 16, 63, 1, 65, 2004, (0.25, 0.05), lambda q, Q: q % 17, 16),
    # nL = 8; two groups by side
    "B9-Q65-w63-L8": lambda: _path(9, 16, 65, 1, 63, 2003, HC.LEVELS8, lambda q, Q: q % 2, 2, per=True),
    # M reaches exactly 64 = the cap; one group: the bit link to var and es
    "B260-Q2-w257": lambda: _path(260, 2, 2, 1, 257, 2009, (0.25, 0.01), None, 1),
    # five passes, lag 2; sixteen contiguous groups, as expiries are in a listed book
    "B9-Q1025-w257": lambda: _path(9, 2, 1025, 2, 257, 2006, (0.2, 0.05), lambda q, Q: q * 16 // Q, 16, per=True),
    # min_scen = 1, the smallest B > lag
    "B3-Q257-w4": lambda: _path(3, 16, 257, 2, 4, 2002, (0.5,), lambda q, Q: (q // 64) % 2, 2, min_scen=1),
    # two passes with an odd M = 3: the last rank of a pass and rank 0 of the next share a pair of slice buffers
    "B16-Q300-w16": lambda: _path(16, 4, 300, 1, 16, 2010, (0.25, 0.1), lambda q, Q: q % 3, 3),
    # the UNORDERED shape: NaN pattern only
    "B3-Q64-w64-unordered": lambda: _path(3, 64, 64, 2, 64, 1905, HC.LEVELS8[:1], None, 1, per=True, gen=HC.unordered),
}
UNORDERED = ("B3-Q64-w64-unordered",)
MARGINS = ("B70-Q63-w65", "B9-Q65-w63-L8", "B260-Q2-w257", "B9-Q1025-w257")      # those that pass hsim_ref.check_margins as generated
MP_CASES = ("B9-Q65-w63-L8", "B3-Q257-w4")                                      # mpmath stays affordable on these
STREAM_CASE = "B70-Q63-w65"


def make(name):
    return CASES[name]()
