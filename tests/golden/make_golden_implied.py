#!/usr/bin/env python3
"""Exact vectors for the Black-Scholes pricer and the implied-vol solver: the seven regimes of
tests/iv_cases.py, 64 seeded points each, priced and inverted in mpmath at 50 digits on the float64 inputs taken exactly
(tests/iv_ref.py exact_price / exact_implied).
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_implied.py
Writes implied_vol.npz, per regime `<regime>.<field>`: the inputs S, K, T, r, sigma, is_put; price = the exact price of the
float64 sigma rounded to float64 (the solver's input and the pricer's expected output); vol_exact = the exact vol of that
float64 price; unit_vol and unit_price = the error units U of every point; flags = what the solver must report; and d1, t1,
t2, vega, ds_dx, the pieces of unit_vol at the exact solution."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import iv_cases as C  # noqa: E402
import iv_ref as R  # noqa: E402


def check(reg, p):
    """What the issue fixes for every generated point: off the thresholds of V4, never on a border of the search."""
    put = p["is_put"] != 0
    KD = p["K"] * np.exp(-p["r"] * p["T"])
    itm = p["flags"] == C.ITM
    intrinsic = np.where(put, np.maximum(KD - p["S"], 0.0), np.maximum(p["S"] - KD, 0.0))
    upper = np.where(put, KD, p["S"])
    tv = np.where(itm, p["price"] - intrinsic, p["price"])
    p_scale = np.where(itm, p["price"] + p["S"] + KD, p["price"])
    assert len(p["S"]) == C.POINTS and (p["price"] > C.MIN_PRICE).all(), reg
    assert (tv >= C.MARGIN * p_scale).all() and (upper - p["price"] >= C.MARGIN * upper).all(), reg
    got = R.restate_implied(p["price"], p["S"], p["K"], p["T"], p["r"], p["is_put"])
    assert (got["flags"] == p["flags"]).all() and not (got["flags"] & C.EDGE).any() and np.isfinite(got["vol"]).all(), reg
    x_over_s = (np.log(p["S"] / p["K"]) + p["r"] * p["T"]) / (p["sigma"] * np.sqrt(p["T"]))
    assert (np.abs(x_over_s) <= C.REGIMES[reg]["d"] * (1 + 1e-9)).all(), reg
    return got


if __name__ == "__main__":
    out = {}
    for reg in C.REGIMES:
        p = C.generate(reg)
        got = check(reg, p)
        ratio = np.abs(got["vol"] - p["vol_exact"]) / p["unit_vol"]
        print(f"  {reg:9s} itm {int((p['flags'] == C.ITM).sum()):2d}  puts {int(p['is_put'].sum()):2d}  price {p['price'].min():.3g} .. {p['price'].max():.3g}"
              f"  restatement / U max {ratio.max():.3f}")
        out.update({f"{reg}.{k}": v for k, v in p.items()})
    path = os.path.join(HERE, "implied_vol.npz")
    np.savez_compressed(path, **out)
    print("implied vol golden:", C.POINTS * len(C.REGIMES), "points,", os.path.getsize(path), "bytes")
