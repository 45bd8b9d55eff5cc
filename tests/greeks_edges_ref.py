"""The error unit and the assertions of the Greeks edge tests, shared by the GPU tests, the fixture generator and the
wrong-variant check.  TEST INFRASTRUCTURE ONLY (NumPy; the exact values come from tests/golden/greeks_edges.npz).

Error of point p and Greek g in units of float64 epsilon of a scale s:  u = |got - exact| / (2^-52 s), with
  s = max(|exact|, 2^-970)  for gamma, vega, rho and the call delta (the floor turns a denormal or flushed result into an
                            absolute error of at most one smallest normal number),
  s = 1                     for the put delta (formed as cdf - 1: absolute accuracy is all the formula has),
  s = (|common| + |r K exp(-rT) cdf(+-d2)|) / 365, floored like the others, for theta (its two terms cancel for puts).
Points are grouped by the exact d1 (|d1| < 8, 8..37, > 37); per (group, option type, Greek) the fixture stores the float64
oracle's own worst error U_oracle, and code under test must stay within 4 U_oracle + 4: it runs the same float64
statements, differing only in the last-ulp rounding of log / exp / erfc / sqrt / divide and in FMA contraction, all of
which the same condition factor amplifies; the oracle is at most 2 ulp off in the benign groups, hence the + 4."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import greeks_oracle as G  # noqa: E402

GREEKS = ("delta", "gamma", "theta", "vega", "rho")
TYPES = ("call", "put")
GROUPS = ("|d1|<8", "8<=|d1|<=37", "|d1|>37")
EPS = 2.0 ** -52
FLOOR = 2.0 ** -970
FACTOR, SLACK = 4.0, 4.0


def group_of(d1):
    a = np.abs(np.asarray(d1, np.float64))
    return np.where(a < 8.0, 0, np.where(a <= 37.0, 1, 2))


def scales(exact, theta_scale, put):
    """exact: dict greek -> float64 [n]; returns dict greek -> the scale s of the module docstring"""
    s = {k: np.maximum(np.abs(exact[k]), FLOOR) for k in GREEKS}
    if put:
        s["delta"] = np.ones_like(exact["delta"])
    s["theta"] = np.maximum(theta_scale, FLOOR)
    return s


def units(got, exact, theta_scale, put):
    """dict greek -> u [n] (inf where `got` is not finite)"""
    s = scales(exact, theta_scale, put)
    with np.errstate(all="ignore"):
        return {k: np.where(np.isfinite(got[k]), np.abs(got[k] - exact[k]) / (EPS * s[k]), np.inf) for k in GREEKS}


def fixture_exact(fx, typ):
    t = TYPES.index(typ)
    return {k: fx["exact"][t, j] for j, k in enumerate(GREEKS)}, fx["theta_scale"][t]


def max_units(got_by_type, fx):
    """U [group, type, greek] = max u over the fixture's points; got_by_type: {"call": dict, "put": dict} over all points"""
    grp = group_of(fx["d1"])
    U = np.zeros((len(GROUPS), 2, len(GREEKS)))
    for t, typ in enumerate(TYPES):
        exact, ts = fixture_exact(fx, typ)
        u = units(got_by_type[typ], exact, ts, typ == "put")
        for j, k in enumerate(GREEKS):
            for gi in range(len(GROUPS)):
                m = grp == gi
                U[gi, t, j] = u[k][m].max() if m.any() else 0.0
    return U


def fixture_violations(got_by_type, fx):
    """The assertions of the exact-fixture test as a list of messages (empty = pass), and the measured U."""
    bad = []
    for typ in TYPES:
        exact, _ = fixture_exact(fx, typ)
        for k in GREEKS:
            g = np.asarray(got_by_type[typ][k])
            if not np.isfinite(g).all():
                bad.append(f"{typ} {k}: {np.count_nonzero(~np.isfinite(g))} NaN / inf values")
            # a value whose exact counterpart rounds to 0 (below the denormals) has no sign to compare: the unit bounds it
            both = (g != 0) & (exact[k] != 0) & np.isfinite(g)
            wrong = both & (np.signbit(g) != np.signbit(exact[k]))
            if wrong.any():
                bad.append(f"{typ} {k}: wrong sign at {np.flatnonzero(wrong)[:5].tolist()}")
    U = max_units(got_by_type, fx)
    over = U > FACTOR * fx["U_oracle"] + SLACK
    for gi, t, j in zip(*np.nonzero(over)):
        bad.append(f"{GROUPS[gi]} {TYPES[t]} {GREEKS[j]}: U = {U[gi, t, j]:.4g} > 4 * {fx['U_oracle'][gi, t, j]:.4g} + 4")
    return bad, U


def theta_scale_f64(S, K, T, r, sigma, put):
    """theta's scale from the oracle's own float64 terms (for inputs that have no exact fixture)"""
    with np.errstate(all="ignore"):
        sq = np.sqrt(T)
        d1 = (np.log(S / K) + (r + 0.5 * sigma ** 2) * T) / (sigma * sq)
        d2 = d1 - sigma * sq
        common = -S * G.norm_pdf(d1) * sigma / (2 * sq)
        other = r * K * np.exp(-r * T) * G.norm_cdf(-d2 if put else d2)
        return (np.abs(common) + np.abs(other)) / 365


def degenerate_violations(got, ref, theta_scale, put, U_benign):
    """Out-of-domain inputs against the float64 oracle: the same NaN positions, the same infinities with sign, zeros where
    the oracle has zeros, finite values within 4 U + 4 of the oracle's with U of the |d1| < 8 group [greek]."""
    bad = []
    fin = {k: np.isfinite(np.asarray(ref[k])) & np.isfinite(np.asarray(got[k])) for k in GREEKS}
    with np.errstate(all="ignore"):                      # cells that are not finite are compared by pattern, not by value
        u = units({k: np.where(fin[k], got[k], 0.0) for k in GREEKS}, {k: np.where(fin[k], ref[k], 0.0) for k in GREEKS},
                  np.where(np.isfinite(theta_scale), theta_scale, 0.0), put)
    for j, k in enumerate(GREEKS):
        g, e = np.asarray(got[k]), np.asarray(ref[k])
        if not np.array_equal(np.isnan(g), np.isnan(e)):
            bad.append(f"{k}: NaN pattern differs at rows {np.flatnonzero(np.isnan(g) != np.isnan(e)).tolist()}")
            continue
        inf_g, inf_e = np.isinf(g), np.isinf(e)
        if not (np.array_equal(inf_g, inf_e) and np.array_equal(np.signbit(g[inf_g]), np.signbit(e[inf_e]))):
            bad.append(f"{k}: infinities differ at rows {np.flatnonzero((inf_g != inf_e) | (inf_g & (g != e))).tolist()}")
            continue
        z = (e == 0) & (g != 0)
        if z.any():
            bad.append(f"{k}: nonzero where the oracle has zero at rows {np.flatnonzero(z).tolist()}")
        over = fin[k] & (u[k] > FACTOR * U_benign[j] + SLACK)
        if over.any():
            bad.append(f"{k}: {u[k][over].max():.4g} units off the oracle at rows {np.flatnonzero(over).tolist()}")
    return bad


# ---- deliberate mistakes, applied to a copy of the oracle: the fixture must tell each of them from the right code
_erf = np.vectorize(math.erf, otypes=[np.float64])


def wrong_greeks(S, K, T, r, sigma, is_put, mistake):
    """oracle/greeks_oracle.calculate_greeks restated with ONE mistake: 'one_minus_erf' (1 - erf(z) in place of erfc(z) in
    the cdf), 'no_rate_in_d1', 'put_delta_sign'; mistake=None is the right code."""
    S, K, T, r, sigma = [np.asarray(a, np.float64) for a in (S, K, T, r, sigma)]
    is_put = np.broadcast_to(np.asarray(is_put, bool), S.shape)
    if mistake == "one_minus_erf":
        cdf = lambda x: 0.5 * (1.0 - _erf(-np.asarray(x, np.float64) / math.sqrt(2.0)))      # noqa: E731
    else:
        cdf = G.norm_cdf
    with np.errstate(all="ignore"):
        sq = np.sqrt(T)
        drift = 0.5 * sigma ** 2 if mistake == "no_rate_in_d1" else r + 0.5 * sigma ** 2
        d1 = (np.log(S / K) + drift * T) / (sigma * sq)
        d2 = d1 - sigma * sq
        disc = r * K * np.exp(-r * T)
        common = -S * G.norm_pdf(d1) * sigma / (2 * sq)
        put_delta = 1 - cdf(d1) if mistake == "put_delta_sign" else cdf(d1) - 1
        delta = np.where(is_put, put_delta, cdf(d1))
        theta = np.where(is_put, (common + disc * cdf(-d2)) / 365, (common - disc * cdf(d2)) / 365)
        gamma = G.norm_pdf(d1) / (S * sigma * sq)
        vega = S * G.norm_pdf(d1) * sq / 100
        rho = K * T * np.exp(-r * T) * np.where(is_put, cdf(-d2), cdf(d2)) / 100
    return {"delta": delta, "gamma": gamma, "theta": theta, "vega": vega, "rho": rho}
