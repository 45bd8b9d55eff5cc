"""The inputs of the implied-vol tests: the seeded generators of the seven regimes of
tests/golden/implied_vol.npz, the hand-built micro cases, one per rule and flag of V1-V7, and the tolerances.  TEST
INFRASTRUCTURE ONLY.  The constants R_CPU below have their measured source in profiles/implied/errlog.txt."""
import numpy as np

import iv_ref as R

NAN, INF = float("nan"), float("inf")
ITM, BELOW, ABOVE, DEAD, EDGE = R.ITM, R.BELOW, R.ABOVE, R.DEAD, R.EDGE
EPS = R.EPS
POINTS = 64                                # per regime
MIN_PRICE = 1e-300                         # only points whose float64 price is above this
MARGIN = 2.0 ** -30                        # every generated point stays this far (relative) off the thresholds of V4

# regime -> sigma range, T range (years), largest |d| = |x| / s, share of in-the-money points, seed
REGIMES = {
    "core_otm": dict(sigma=(0.05, 3.0), T=(1.0 / 365.0, 2.0), d=4.0, itm=0.0, seed=1601),
    "core_itm": dict(sigma=(0.05, 3.0), T=(1.0 / 365.0, 2.0), d=4.0, itm=1.0, seed=1602),
    "near_atm": dict(sigma=(0.05, 3.0), T=(1.0 / 365.0, 2.0), d=0.01, itm=0.5, seed=1603),
    "short": dict(sigma=(0.1, 2.0), T=(1e-6, 1e-4), d=6.0, itm=0.0, seed=1604),
    "wings": dict(sigma=(0.05, 3.0), T=(1.0 / 365.0, 2.0), d=36.0, itm=0.0, seed=1605),
    "tinyvol": dict(sigma=(1e-4, 1e-2), T=(1.0 / 365.0, 1.0), d=8.0, itm=0.3, seed=1606),
    "bigvol": dict(sigma=(3.0, 8.0), T=(0.25, 1.0), d=3.0, itm=0.3, seed=1607),
}
RATES = (0.0, 0.03, -0.01)
FIELDS = ("S", "K", "T", "r", "sigma", "is_put", "price", "vol_exact", "unit_vol", "unit_price", "flags", "d1", "t1", "t2",
          "vega", "ds_dx")

# R_CPU: the largest |fp64 restatement - mpmath at 50 digits| / U over the 64 points of a regime, U the unit of the issue
# computed in mpmath at the exact solution (iv_ref.exact_implied / exact_price).  Measured by
# test_implied.test_restatement_against_the_fixture (profiles/implied/errlog.txt).  The worst of 64 points is a noisy figure:
# it moved by up to 0.3 (core_otm 0.74 -> 0.50, wings 0.85 -> 1.15) when nothing but last bits of the inputs changed (the
# generator's exp / log replaced by mpmath's), and another host's exp / log / erfc changes last bits of intermediates in the
# same way.  Recorded here: the measured figure + 0.3, rounded up to one decimal.  The GPU tests allow C_GPU x R_CPU, the
# project's standing margin for FMA contraction and the device's erfc / exp / log / sqrt / division.
# Measured: vol 0.496, 0.329, 0.418, 0.996, 1.146, 1.029, 0.635; price 0.597, 0.240, 0.283, 0.816, 1.074, 1.094, 0.366.
R_CPU = {"core_otm": 0.8, "core_itm": 0.7, "near_atm": 0.8, "short": 1.3, "wings": 1.5, "tinyvol": 1.4, "bigvol": 1.0}
R_CPU_PRICE = {"core_otm": 0.9, "core_itm": 0.6, "near_atm": 0.6, "short": 1.2, "wings": 1.4, "tinyvol": 1.4, "bigvol": 0.7}
R_CPU_LIMIT = 4.0                          # no regime's recorded R_CPU for the vol may exceed this
C_GPU = 8.0


def generate(regime, count=POINTS):
    """The first `count` accepted points of a regime: dict of float64 arrays (FIELDS).  A candidate is drawn from the seeded
    stream, priced in mpmath at its float64 inputs, and kept when its float64 price is above MIN_PRICE and stays MARGIN off the
    bounds of V4; the kept point is then inverted in mpmath.  Everything between the generator's uniform doubles and the
    float64 inputs is mpmath too, so that no host's exp or log decides a last bit of the file."""
    mp = R._mp()
    g = REGIMES[regime]
    rng = np.random.default_rng(g["seed"])
    log_uniform = lambda u, lo, hi: float(mp.exp(mp.log(lo) + mp.mpf(u) * (mp.log(hi) - mp.log(lo))))   # noqa: E731
    rows = []
    while len(rows) < count:
        u = [float(v) for v in rng.random(6)]
        sigma, T = log_uniform(u[0], *g["sigma"]), log_uniform(u[1], *g["T"])
        d = (2.0 * u[2] - 1.0) * g["d"]
        S = log_uniform(u[3], 1.0, 1e5)
        r = RATES[int(rng.integers(0, 3))]
        itm = bool(u[4] < g["itm"])
        s = float(mp.mpf(sigma) * mp.sqrt(T))
        K = float(mp.mpf(S) * mp.exp(mp.mpf(r) * T - mp.mpf(d) * s))
        put = (d > 0) != itm                                                  # x = d s > 0: the put is out of the money
        e = R.exact_price(S, K, T, r, sigma, put)
        P = float(e["price"])
        KD = float(mp.mpf(K) * mp.exp(-mp.mpf(r) * T))
        intrinsic = max(KD - S, 0.0) if put else max(S - KD, 0.0)
        upper = KD if put else S
        tv, p_scale = (P - intrinsic, P + S + KD) if itm else (P, P)
        if not (P > MIN_PRICE and tv >= MARGIN * p_scale and upper - P >= MARGIN * upper):
            continue
        v = R.exact_implied(P, S, K, T, r, put, s)
        assert v["itm"] == itm
        rows.append((S, K, T, r, sigma, float(put), P, float(v["vol"]), v["unit"], e["unit"], float(ITM if itm else 0),
                     v["d1"], v["t1"], v["t2"], v["vega"], v["ds_dx"]))
    a = np.array(rows, np.float64)
    return {k: np.ascontiguousarray(a[:, i]) for i, k in enumerate(FIELDS)}


def load_fixture(path):
    """tests/golden/implied_vol.npz -> {regime: dict of arrays}."""
    z = np.load(path)
    return {reg: {k: z[f"{reg}.{k}"] for k in FIELDS} for reg in REGIMES}


def joined(fix, regimes=None):
    """The regimes of a fixture one after the other: dict of arrays plus `regime`, the index of every point's regime."""
    regimes = list(regimes or REGIMES)
    out = {k: np.concatenate([fix[reg][k] for reg in regimes]) for k in FIELDS}
    out["regime"] = np.concatenate([np.full(len(fix[reg]["S"]), i) for i, reg in enumerate(regimes)])
    return out


# ------------------------------------------------------------------ micro cases (r = 0: every bound is an exact number)
def _micro(price, S, K, T, put, flags, vol, r=0.0, mode=0):
    return dict(price=price, S=S, K=K, T=T, r=r, is_put=put, price_mode=mode, flags=flags, vol=vol)


KNOWN = dict(S=25000.0, K=25500.0, T=0.05, r=0.01, sigma=0.6)
MICRO = {
    "itm_call_at_intrinsic": _micro(20.0, 100.0, 80.0, 0.5, 0, BELOW | ITM, 0.0),
    "itm_call_one_ulp_under": _micro(float(np.nextafter(20.0, 0.0)), 100.0, 80.0, 0.5, 0, BELOW | ITM, NAN),
    "itm_put_at_intrinsic": _micro(20.0, 80.0, 100.0, 0.5, 1, BELOW | ITM, 0.0),
    "otm_call_worth_nothing": _micro(0.0, 100.0, 120.0, 0.5, 0, BELOW, 0.0),
    "call_at_upper": _micro(100.0, 100.0, 120.0, 0.5, 0, ABOVE, NAN),
    "call_over_upper": _micro(101.0, 100.0, 120.0, 0.5, 0, ABOVE, NAN),
    "put_at_upper": _micro(90.0, 100.0, 90.0, 0.5, 1, ABOVE, NAN),
    "itm_call_at_upper": _micro(100.0, 100.0, 80.0, 0.5, 0, ABOVE | ITM, NAN),
    "mode1_whole_underlying": _micro(1.0, 100.0, 120.0, 0.5, 0, ABOVE, NAN, mode=1),
    "atm_under_the_lower_border": _micro(100.0 * 1e-14, 100.0, 100.0, 0.25, 0, EDGE, 2.0 ** -40 / 0.5),
    "atm_put_under_the_lower_border": _micro(100.0 * 1e-14, 100.0, 100.0, 0.25, 1, EDGE, 2.0 ** -40 / 0.5),
}
_LIVE = dict(price=2.5, S=100.0, K=110.0, T=0.5, r=0.01)
DEAD_CAUSES = [(k, v) for k in ("price", "S", "K", "T", "r") for v in (NAN, INF, -INF)]
DEAD_CAUSES += [("price", -1.0), ("S", 0.0), ("S", -100.0), ("K", 0.0), ("K", -110.0), ("T", 0.0), ("T", -0.5)]


def dead_batch():
    """One option per cause of V1 (both sides), dict of arrays; every one must come out NaN with DEAD alone."""
    rows = []
    for put in (0.0, 1.0):
        for k, v in DEAD_CAUSES:
            c = dict(_LIVE, is_put=put)
            c[k] = v
            rows.append(c)
    return {k: np.array([c[k] for c in rows], np.float64) for k in ("price", "S", "K", "T", "r", "is_put")}


def micro_batch():
    """The micro cases of one price_mode each: {mode: (names, dict of arrays)}."""
    out = {}
    for mode in (0, 1):
        names = [n for n, c in MICRO.items() if c["price_mode"] == mode]
        out[mode] = (names, {k: np.array([MICRO[n][k] for n in names], np.float64)
                             for k in ("price", "S", "K", "T", "r", "is_put", "flags", "vol")})
    return out


def check_micro(solve):
    """The micro cases through solve(price, S, K, T, r, is_put, price_mode) -> dict(vol, flags)."""
    for mode, (names, c) in micro_batch().items():
        got = solve(c["price"], c["S"], c["K"], c["T"], c["r"], c["is_put"], mode)
        for i, n in enumerate(names):
            assert int(got["flags"][i]) == int(c["flags"][i]), (n, int(got["flags"][i]))
            assert np.array_equal(got["vol"][i:i + 1], c["vol"][i:i + 1], equal_nan=True), (n, got["vol"][i])
    d = dead_batch()
    for mode in (0, 1):
        got = solve(d["price"], d["S"], d["K"], d["T"], d["r"], d["is_put"], mode)
        assert (got["flags"] == DEAD).all() and np.isnan(got["vol"]).all()


def check_known(price, solve):
    """SURVEY.md section 8f's option: priced, then inverted, for both sides."""
    k = KNOWN
    exact = {0: 1120.4215468331388, 1: 1607.6747338019552}                    # mpmath at 50 digits, rounded
    for put in (0, 1):
        one = lambda v: np.array([v], np.float64)                             # noqa: E731
        p = price(one(k["S"]), one(k["K"]), one(k["T"]), one(k["r"]), one(k["sigma"]), one(put))
        e = R.exact_price(k["S"], k["K"], k["T"], k["r"], k["sigma"], put)
        assert p["flags"][0] == 0 and abs(p["price"][0] - exact[put]) <= C_GPU * max(R_CPU_PRICE.values()) * e["unit"]
        s = k["sigma"] * np.sqrt(k["T"])
        d1 = (np.log(k["S"] / k["K"]) + k["r"] * k["T"]) / s + 0.5 * s
        assert abs(p["vega"][0] - k["S"] * np.exp(-0.5 * d1 * d1) / np.sqrt(2 * np.pi) * np.sqrt(k["T"])) <= 1e-12 * p["vega"][0]
        v = solve(p["price"], one(k["S"]), one(k["K"]), one(k["T"]), one(k["r"]), one(put), 0)
        u = R.exact_implied(p["price"][0], k["S"], k["K"], k["T"], k["r"], put, k["sigma"] * np.sqrt(k["T"]))
        assert v["flags"][0] == (ITM if put else 0)                        # K above the forward: the put is in the money
        assert abs(v["vol"][0] - float(u["vol"])) <= C_GPU * max(R_CPU.values()) * u["unit"]
        assert abs(v["vol"][0] - k["sigma"]) <= 1e-12


def tiled(fix, n):
    """The fixture's points, all regimes joined, repeated to n options: dict of arrays and the index of every option's point."""
    j = joined(fix)
    idx = np.arange(n) % len(j["S"])
    return {k: np.ascontiguousarray(j[k][idx]) for k in FIELDS}, idx
