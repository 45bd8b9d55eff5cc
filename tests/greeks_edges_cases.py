"""Edge inputs for the Black-Scholes Greeks kernel.  TEST INPUTS ONLY (NumPy, no reference values).

``regime_inputs`` draws the float64 points of tests/golden/greeks_edges.npz (make_golden_greeks_edges.py evaluates them
exactly); the first k points of a regime do not depend on how many are drawn.  ``DEGENERATE`` is the hand-written table
of inputs outside the formula's domain, for which the float64 oracle's own NumPy behaviour is the specification."""
import numpy as np

SEED = 20240611
REGIMES = ("mid", "wings", "underflow", "short", "lowvol", "highvol", "atm", "units")
N_PER_REGIME = 192


def regime_inputs(name, n=N_PER_REGIME):
    """(S, K, T, r, sigma) float64 [n] of one regime."""
    u = np.random.default_rng([SEED, REGIMES.index(name)]).random((n, 8))     # filled row by row: a prefix is a prefix
    lin = lambda c, lo, hi: lo + (hi - lo) * u[:, c]                          # noqa: E731
    geo = lambda c, lo, hi: np.exp(np.log(lo) + (np.log(hi) - np.log(lo)) * u[:, c])   # noqa: E731
    i = np.arange(n)
    S = lin(0, 20000.0, 30000.0)
    r = lin(3, 0.0, 0.05)
    if name == "mid":
        K, T, sg = S * lin(1, 0.7, 1.3), lin(2, 1 / 365, 1.5), lin(4, 0.05, 3.0)
    elif name == "wings":                         # K/S chosen so that 8 <= |d1| <= 37
        T, sg = lin(2, 1 / 365, 0.1), lin(4, 0.05, 0.3)
        d1 = np.where(u[:, 5] < 0.5, -1.0, 1.0) * lin(1, 8.5, 36.5)
        K = S * np.exp(-(d1 * sg * np.sqrt(T) - (r + 0.5 * sg * sg) * T))
    elif name == "underflow":
        K, T, sg = S * geo(1, 0.3, 3.0), lin(2, 1 / 365, 0.1), lin(4, 0.05, 0.3)
    elif name == "short":
        K, T, sg = S * lin(1, 0.98, 1.02), geo(2, 1e-6, 1 / 365), lin(4, 0.05, 3.0)
    elif name == "lowvol":
        K, T, sg = S * lin(1, 0.995, 1.005), lin(2, 0.01, 1.0), geo(4, 1e-4, 0.02)
    elif name == "highvol":
        K, T, sg = S * lin(1, 0.7, 1.3), lin(2, 0.5, 3.0), lin(4, 3.0, 20.0)
    elif name == "atm":                           # K = S exactly, or S (1 +- 2^-40 .. 2^-20); r = 0 exactly, or -0.02 .. 0.5
        T, sg = lin(2, 1 / 365, 1.5), lin(4, 0.05, 3.0)
        K = np.where(i % 3 == 0, S, S * (1.0 + np.where(u[:, 5] < 0.5, -1.0, 1.0) * 2.0 ** -lin(1, 20.0, 40.0)))
        r = np.where((i // 3) % 3 == 0, 0.0, lin(3, -0.02, 0.5))
    elif name == "units":
        S = geo(0, 1e-3, 1e7)
        K, T, sg = S * lin(1, 0.7, 1.3), lin(2, 1 / 365, 1.5), lin(4, 0.05, 3.0)
    else:
        raise KeyError(name)
    return tuple(np.ascontiguousarray(a, np.float64) for a in (S, K, T, r, sg))


NAN, INF = np.nan, np.inf
_B = (25000.0, 25500.0, 0.05, 0.01, 0.6)          # S, K, T, r, sigma of a benign option


def _row(**kw):
    d = dict(zip(("S", "K", "T", "r", "sigma"), _B)); d.update(kw)
    return tuple(float(d[k]) for k in ("S", "K", "T", "r", "sigma"))


DEGENERATE = [
    _row(),
    # T = 0, -1, inf: out of, in and at the money
    _row(T=0.0), _row(T=0.0, K=24500.0), _row(T=0.0, K=25000.0), _row(T=0.0, K=25000.0, r=0.0), _row(T=-0.0),
    _row(T=-1.0), _row(T=-1.0, K=24500.0), _row(T=INF), _row(T=INF, K=24500.0), _row(T=INF, r=0.0), _row(T=INF, r=-0.01),
    _row(T=5e-324), _row(T=5e-324, K=24500.0), _row(T=1e-300, K=25000.0, r=0.0),
    # sigma = 0 with the numerator of d1 positive, negative and exactly zero; negative, infinite and denormal sigma
    _row(sigma=0.0, K=24500.0), _row(sigma=0.0), _row(sigma=0.0, K=25000.0, r=0.0), _row(sigma=0.0, K=25000.0),
    _row(sigma=-0.0, K=24500.0), _row(sigma=-0.2), _row(sigma=-0.2, K=24500.0), _row(sigma=INF), _row(sigma=INF, K=24500.0),
    _row(sigma=-INF), _row(sigma=5e-324), _row(sigma=5e-324, K=24500.0), _row(sigma=0.0, T=0.0), _row(sigma=0.0, T=0.0, K=25000.0, r=0.0),
    _row(sigma=INF, T=0.0), _row(sigma=0.0, T=INF), _row(sigma=1e200, T=1e200),
    # S = 0, K = 0, negative prices
    _row(S=0.0), _row(K=0.0), _row(S=0.0, K=0.0), _row(S=-25000.0), _row(K=-25500.0), _row(S=-25000.0, K=-25500.0),
    _row(S=-0.0), _row(K=-0.0), _row(S=5e-324), _row(K=5e-324), _row(S=1e308, K=1e-308), _row(S=1e-308, K=1e308),
    # NaN and infinities in each input
    _row(S=NAN), _row(K=NAN), _row(T=NAN), _row(r=NAN), _row(sigma=NAN),
    _row(S=INF), _row(K=INF), _row(S=INF, K=INF), _row(r=INF), _row(r=-INF), _row(r=INF, T=0.0), _row(S=-INF),
    # the rate: zero, negative, large
    _row(r=0.0), _row(r=-0.0), _row(r=-0.5), _row(r=1e4), _row(r=-1e4),
]


def degenerate_inputs():
    """(S, K, T, r, sigma) float64 [len(DEGENERATE)]"""
    a = np.asarray(DEGENERATE, np.float64)
    return tuple(np.ascontiguousarray(a[:, j]) for j in range(5))
