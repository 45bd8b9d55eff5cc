"""Rules V1-V8 of DESIGN.md section 16 (Black-Scholes pricer and price -> implied vol), restated twice.  TEST INFRASTRUCTURE
ONLY.  restate_price / restate_implied: NumPy float64 with scipy.special.erfc, statement by statement what the kernels of
csrc/ivs_implied.hpp do.  exact_price / exact_implied: the same rules in mpmath at 50 digits on the float64 inputs taken as
exact numbers; exact_implied also returns what the error unit of the issue is built from."""
import numpy as np

ITM, BELOW, ABOVE, DEAD, EDGE = 1, 2, 4, 8, 16
EPS = 2.0 ** -52
T_LO, T_HI, STEPS = -40.0, 6.0, 64
NAN = float("nan")


def _phi_cdf(z):
    from scipy.special import erfc
    return 0.5 * erfc(-z * 0.70710678118654752440)


def _b(h, em, ep, s):
    q, hs = h / s, 0.5 * s
    return em * _phi_cdf(-q + hs) - ep * _phi_cdf(-q - hs)


def _arrays(*a):
    return [np.ascontiguousarray(v, np.float64).ravel() for v in np.broadcast_arrays(*[np.asarray(x, np.float64) for x in a])]


def restate_price(S, K, T, r, sigma, is_put):
    """dict(price, vega, flags) by rules V1 and V8."""
    S, K, T, r, sigma, put = _arrays(S, K, T, r, sigma, np.asarray(is_put, np.float64))
    put = put != 0
    with np.errstate(all="ignore"):
        live = np.isfinite(S) & np.isfinite(K) & np.isfinite(T) & np.isfinite(r) & np.isfinite(sigma) & (S > 0) & (K > 0) & (T > 0) & (sigma > 0)
        sq = np.sqrt(T)
        KD = K * np.exp(-r * T)
        x = np.log(S / K) + r * T
        s = sigma * sq
        d1 = x / s + 0.5 * s
        d2 = d1 - s
        v = np.where(put, KD * _phi_cdf(-d2) - S * _phi_cdf(-d1), S * _phi_cdf(d1) - KD * _phi_cdf(d2))
        vega = S * (np.exp(-d1 * d1 * 0.5) * 0.39894228040143267794) * sq
    return {"price": np.where(live, v, NAN), "vega": np.where(live, vega, NAN), "flags": np.where(live, 0, DEAD).astype(np.int32)}


def restate_implied(price, S, K, T, r, is_put, price_mode=0):
    """dict(vol, flags) by rules V1-V7."""
    price, S, K, T, r, put = _arrays(price, S, K, T, r, np.asarray(is_put, np.float64))
    put = put != 0
    with np.errstate(all="ignore"):
        live = np.isfinite(price) & np.isfinite(S) & np.isfinite(K) & np.isfinite(T) & np.isfinite(r) & (S > 0) & (K > 0) & (T > 0) & (price >= 0)
        P = price * S if price_mode else price
        KD = K * np.exp(-r * T)
        x = np.log(S / K) + r * T
        h = np.abs(x)
        itm = np.where(put, x < 0, x > 0)
        gap = np.where(put, KD - S, S - KD)
        intrinsic, upper = np.where(gap > 0, gap, 0.0), np.where(put, KD, S)
        tv = np.where(itm, P - intrinsic, P)
        beta = tv / np.sqrt(S * KD)
        em, ep = np.exp(-0.5 * h), np.exp(0.5 * h)
        at_lo = _b(h, em, ep, np.exp2(T_LO)) >= beta
        at_hi = _b(h, em, ep, np.exp2(T_HI)) < beta
        lo, hi = np.full(len(P), T_LO), np.full(len(P), T_HI)
        for _ in range(STEPS):
            mid = 0.5 * (lo + hi)
            below = _b(h, em, ep, np.exp2(mid)) < beta
            lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
        t = np.where(at_lo, T_LO, np.where(at_hi, T_HI, 0.5 * (lo + hi)))
        v = np.exp2(t) / np.sqrt(T)
        side = np.where(itm, ITM, 0)
        f = side | np.where(at_lo | at_hi, EDGE, 0)
        above, under, equal = P >= upper, P < intrinsic, P == intrinsic
        v = np.where(above | under, NAN, np.where(equal, 0.0, v))
        f = np.where(above, side | ABOVE, np.where(under | equal, side | BELOW, f))
    return {"vol": np.where(live, v, NAN), "flags": np.where(live, f, DEAD).astype(np.int32)}


# ------------------------------------------------------------------ the same in mpmath
def _mp():
    import mpmath
    mpmath.mp.dps = 50
    return mpmath.mp


def _terms(mp, S, KD, x, s, otm_put):
    """d1 and the two terms of one side's price at total vol s (call unless otm_put)."""
    d1 = x / s + s / 2
    d2 = d1 - s
    N = lambda z: mp.erfc(-z / mp.sqrt(2)) / 2                                # noqa: E731
    if otm_put:
        return d1, KD * N(-d2), S * N(-d1)
    return d1, S * N(d1), KD * N(d2)


def exact_price(S, K, T, r, sigma, is_put):
    """One option at 50 digits: dict(price, unit): the price as an mpf and the pricer's error unit (a float)."""
    mp = _mp()
    S, K, T, r, sigma = (mp.mpf(float(v)) for v in (S, K, T, r, sigma))
    KD = K * mp.exp(-r * T)
    x = mp.log(S / K) + r * T
    s = sigma * mp.sqrt(T)
    d1, t1, t2 = _terms(mp, S, KD, x, s, bool(is_put))
    vega = S * mp.npdf(d1) * mp.sqrt(T)
    unit = EPS * ((t1 + t2) * (2 + d1 * d1 / 2 + abs(mp.log(S / K)) + abs(r * T)) + vega * sigma)
    return {"price": t1 - t2, "unit": float(unit)}


def exact_implied(P, S, K, T, r, is_put, s0):
    """One live option strictly between its bounds, at 50 digits: the root of log(price(s) / tv) from the start s0 (a total
    vol), and dict(vol, unit, d1, t1, t2, vega, ds_dx, itm)."""
    mp = _mp()
    P, S, K, T, r = (mp.mpf(float(v)) for v in (P, S, K, T, r))
    KD = K * mp.exp(-r * T)
    x = mp.log(S / K) + r * T
    itm = (x < 0) if is_put else (x > 0)
    intrinsic = max(KD - S, mp.mpf(0)) if is_put else max(S - KD, mp.mpf(0))
    tv = P - intrinsic if itm else P
    otm_put = not (x < 0)                                                     # the side the equation is solved on

    def g(s):
        _, t1, t2 = _terms(mp, S, KD, x, s, otm_put)
        return mp.log((t1 - t2) / tv)

    def dg(s):
        d1, t1, t2 = _terms(mp, S, KD, x, s, otm_put)
        return S * mp.npdf(d1) / (t1 - t2)

    s = mp.findroot(g, mp.mpf(float(s0)), solver="newton", df=dg, tol=mp.mpf(10) ** -80, maxsteps=200, verify=False)
    assert s > 0 and abs(g(s)) < mp.mpf(10) ** -40, (float(s), float(g(s)))
    d1, t1, t2 = _terms(mp, S, KD, x, s, otm_put)
    sq = mp.sqrt(T)
    sigma, vega = s / sq, S * mp.npdf(d1) * sq
    ds_dx = (t1 + t2) / (2 * vega)
    p_scale = P + S + KD if itm else P
    unit = EPS * (sigma + (p_scale + (t1 + t2) * (1 + d1 * d1 / 2)) / vega + ds_dx * (1 + abs(mp.log(S / K)) + abs(r * T)))
    return {"vol": sigma, "unit": float(unit), "d1": float(d1), "t1": float(t1), "t2": float(t2), "vega": float(vega),
            "ds_dx": float(ds_dx), "itm": bool(itm)}


def unit_from_restatement(vol, P, S, K, T, r, is_put):
    """The vol's error unit evaluated in float64 at a solution `vol` (arrays): what a test uses where no exact solution is at
    hand.  Returns (unit, vega)."""
    from scipy.special import erfc
    vol, P, S, K, T, r, put = _arrays(vol, P, S, K, T, r, np.asarray(is_put, np.float64))
    put = put != 0
    with np.errstate(all="ignore"):
        KD = K * np.exp(-r * T)
        x = np.log(S / K) + r * T
        sq = np.sqrt(T)
        s = vol * sq
        d1 = x / s + 0.5 * s
        d2 = d1 - s
        N = lambda z: 0.5 * erfc(-z * 0.70710678118654752440)                 # noqa: E731
        t1 = np.where(x < 0, S * N(d1), KD * N(-d2))
        t2 = np.where(x < 0, KD * N(d2), S * N(-d1))
        vega = S * np.exp(-0.5 * d1 * d1) * 0.39894228040143267794 * sq
        itm = np.where(put, x < 0, x > 0)
        p_scale = np.where(itm, P + S + KD, P)
        unit = EPS * (vol + (p_scale + (t1 + t2) * (1 + d1 * d1 / 2)) / vega + (t1 + t2) / (2 * vega) * (1 + np.abs(np.log(S / K)) + np.abs(r * T)))
    return unit, vega


class RefBackend:
    """The restatement behind the backend interface of iv_interpolation_amd.implied (host arrays in, host arrays out)."""

    def price(self, S, K, T, r, sigma, is_put, default_is_put=False):
        put = np.full(len(np.atleast_1d(S)), float(bool(default_is_put))) if is_put is None else is_put
        return restate_price(S, K, T, r, sigma, put)

    def implied_vol(self, price, S, K, T, r, is_put, default_is_put=False, price_mode=0):
        put = np.full(len(np.atleast_1d(S)), float(bool(default_is_put))) if is_put is None else is_put
        return restate_implied(price, S, K, T, r, put, price_mode)
