#!/usr/bin/env python3
"""Exact vectors for the Greeks kernel in the regimes where float64 itself struggles (wings, underflow tails, expiries
of minutes, vols of basis points, at the money, other price scales): the five formulas of oracle/greeks_oracle.py
restated in mpmath at 80 digits, evaluated on the float64 inputs of tests/greeks_edges_cases.py taken exactly.
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_greeks_edges.py
Writes greeks_edges.npz: inputs, regime index, exact d1 / d2, exact values rounded to float64 (exact[type, greek, point]),
theta's scale (theta_scale[type, point]) and U_oracle[group, type, greek], the worst error of the float64 oracle in the
unit of tests/greeks_edges_ref.py."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
import greeks_edges_cases as C  # noqa: E402
import greeks_edges_ref as R  # noqa: E402
import greeks_oracle as G  # noqa: E402

DIGITS = 80


def exact_point(S, K, T, r, sigma):
    """One option exactly: (d1, d2, {type: [delta, gamma, theta, vega, rho]}, {type: theta scale}) as mpf"""
    import mpmath as mp
    S, K, T, r, sigma = (mp.mpf(float(x)) for x in (S, K, T, r, sigma))      # the float64 inputs, exactly
    cdf = lambda x: mp.erfc(-x / mp.sqrt(2)) / 2                              # noqa: E731
    pdf = lambda x: mp.exp(-x * x / 2) / mp.sqrt(2 * mp.pi)                   # noqa: E731
    sq = mp.sqrt(T)
    d1 = (mp.log(S / K) + (r + sigma ** 2 / 2) * T) / (sigma * sq)
    d2 = d1 - sigma * sq
    disc = r * K * mp.exp(-r * T)
    common = -S * pdf(d1) * sigma / (2 * sq)
    gamma = pdf(d1) / (S * sigma * sq)
    vega = S * pdf(d1) * sq / 100
    out, scale = {}, {}
    for typ in R.TYPES:
        put = typ == "put"
        c2 = cdf(-d2) if put else cdf(d2)
        delta = -cdf(-d1) if put else cdf(d1)          # cdf(d1) - 1 without the cancellation (80 digits end near 1e-80)
        theta = (common + disc * c2) / 365 if put else (common - disc * c2) / 365
        rho = K * T * mp.exp(-r * T) * c2 / 100
        out[typ] = [delta, gamma, theta, vega, rho]
        scale[typ] = (abs(common) + abs(disc * c2)) / 365
    return d1, d2, out, scale


def build(n_per_regime):
    """The fixture's arrays for n_per_regime points per regime (everything but U_oracle)."""
    import mpmath as mp
    cols = [[] for _ in range(5)]
    regime = []
    for ri, name in enumerate(C.REGIMES):
        for j, a in enumerate(C.regime_inputs(name, n_per_regime)):
            cols[j].append(a)
        regime.append(np.full(n_per_regime, ri, np.int8))
    S, K, T, r, sigma = (np.concatenate(c) for c in cols)
    n = S.size
    fx = {"S": S, "K": K, "T": T, "r": r, "sigma": sigma, "regime": np.concatenate(regime),
          "d1": np.empty(n), "d2": np.empty(n), "exact": np.empty((2, 5, n)), "theta_scale": np.empty((2, n))}
    with mp.workdps(DIGITS):
        for i in range(n):
            d1, d2, out, scale = exact_point(S[i], K[i], T[i], r[i], sigma[i])
            fx["d1"][i], fx["d2"][i] = float(d1), float(d2)
            for t, typ in enumerate(R.TYPES):
                fx["exact"][t, :, i] = [float(v) for v in out[typ]]
                fx["theta_scale"][t, i] = float(scale[typ])
    return fx


def oracle_units(fx):
    with np.errstate(all="ignore"):
        got = {typ: G.calculate_greeks(fx["S"], fx["K"], fx["T"], fx["r"], fx["sigma"], typ == "put") for typ in R.TYPES}
    return R.max_units(got, fx)


if __name__ == "__main__":
    fx = build(C.N_PER_REGIME)
    w = fx["regime"] == C.REGIMES.index("wings")
    assert (np.abs(fx["d1"][w]) >= 8).all() and (np.abs(fx["d1"][w]) <= 37).all(), "wings must stay inside 8 <= |d1| <= 37"
    fx["U_oracle"] = oracle_units(fx)
    fx["regimes"] = np.array(C.REGIMES)
    path = os.path.join(HERE, "greeks_edges.npz")
    np.savez_compressed(path, **fx)
    grp = R.group_of(fx["d1"])
    print("greeks edges golden:", fx["S"].size, "points x 2 option types,", os.path.getsize(path), "bytes")
    for ri, name in enumerate(C.REGIMES):
        m = fx["regime"] == ri
        print(f"  {name:9s} |d1| {np.abs(fx['d1'][m]).min():9.3g} .. {np.abs(fx['d1'][m]).max():9.3g}   groups {np.bincount(grp[m], minlength=3).tolist()}")
    for gi, gname in enumerate(R.GROUPS):
        for t, typ in enumerate(R.TYPES):
            print(f"  U_oracle {gname:12s} {typ:4s} " + " ".join(f"{k}={fx['U_oracle'][gi, t, j]:.4g}" for j, k in enumerate(R.GREEKS)))
