"""Case table of tests/test_bridge_edges.py: every input of the bridge / MT19937 edge tests, built deterministically.

A batch is a dict: price, volume (float64 [n]), off (int64 [S+1], CSR rows of the symbols).  Group numbers follow the
docstring of test_bridge_edges.py.  Nothing here touches the device or the oracle."""
import functools
from fractions import Fraction

import numpy as np

DRAWS = {0: 5, 1: 2, 2: 0, 3: 1, 4: 4}          # doubles drawn by the candle builder per valid row (bridge_uniforms)
BAD_PRICES = (np.nan, -1.0, 0.0, -np.inf)       # what the reference skips: NaN or <= 0
CHUNK_LENS = (63, 64, 65, 127, 128, 129)        # around the 64-row chunks of bridge_candles_kernel
GRID_S = 8 * 256 + 173                           # symbols of group 1 on a 256-CU part: one full grid trip and 173 more
SEED = 20240607


def _walk(r, n, p0=2000.0, sd=5e-4):
    return p0 * np.exp(np.cumsum(r.normal(0, sd, n)))


def _holes(r, price, volume):
    """Holes the reference reacts to: price NaN / <= 0 (row skipped), volume NaN / 0 / negative (volume drawn)."""
    n = len(price)
    price[r.random(n) < 0.05] = np.nan
    price[r.random(n) < 0.01] = -1.0
    price[r.random(n) < 0.005] = 0.0
    volume[r.random(n) < 0.2] = np.nan
    volume[r.random(n) < 0.1] = 0.0
    volume[r.random(n) < 0.02] = -3.0
    return price, volume


def _batch(r, lens, holes=True):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(off[-1])
    price, volume = _walk(r, n), r.uniform(0, 30, n).round(4)
    if holes:
        _holes(r, price, volume)
    return {"price": price, "volume": volume, "off": off}


# ---------------------------------------------------------------- 1: more symbols than wavefronts in the grid
@functools.lru_cache(maxsize=None)
def grid_batch(S=GRID_S):
    r = np.random.default_rng(101)
    lens = r.integers(0, 41, S)
    ninth = np.arange(0, S, 9)
    lens[ninth] = np.array(CHUNK_LENS)[np.arange(len(ninth)) % len(CHUNK_LENS)]
    lens[::17] = 0
    return _batch(r, lens)


# ---------------------------------------------------------------- 2: more than 256 scan blocks
SCAN_ROWS = 256 * 1024 + 1500
SCAN_LONG = 100_000


@functools.lru_cache(maxsize=None)
def scan_batch():
    r = np.random.default_rng(102)
    S = 40
    rest = SCAN_ROWS - SCAN_LONG
    cuts = np.sort(r.choice(np.arange(1, rest), S - 3, replace=False))
    lens = list(np.diff(np.concatenate([[0], cuts, [rest]])))             # S - 2 symbols, none empty
    lens.insert(7, SCAN_LONG)
    lens.insert(20, 0)
    return _batch(r, np.array(lens, np.int64))


def words_consumed(batch, strategy):
    """Sum over the valid rows of 2 * draws(strategy) + 2 * [volume missing] (uniform strategies)."""
    p, v = batch["price"], batch["volume"]
    ok = ~(np.isnan(p) | (p <= 0))
    miss = np.isnan(v) | (v <= 0)
    return int(2 * DRAWS[strategy] * ok.sum() + 2 * (ok & miss).sum())


# ---------------------------------------------------------------- 3: chunk boundaries and holes inside a symbol's chain
CHAIN_LENS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193)
CHAIN_PATTERNS = ("none", "chunk1_invalid", "last_only", "first_only", "first_at_63", "every_other")


def chain_invalid(pattern, n):
    """Rows of an n-row symbol made invalid by the pattern."""
    i = np.arange(n)
    return {"none": np.zeros(n, bool), "chunk1_invalid": (i >= 64) & (i < 128), "last_only": i < n - 1, "first_only": i > 0,
            "first_at_63": i < 63, "every_other": i % 2 == 1}[pattern]


@functools.lru_cache(maxsize=None)
def chain_batch():
    r = np.random.default_rng(103)
    lens = np.array([n for _ in CHAIN_PATTERNS for n in CHAIN_LENS], np.int64)
    b = _batch(r, lens, holes=False)
    v = b["volume"]
    v[r.random(len(v)) < 0.3] = np.nan
    v[r.random(len(v)) < 0.1] = 0.0
    k = 0
    for s, pat in enumerate(pat for pat in CHAIN_PATTERNS for _ in CHAIN_LENS):
        a, e = int(b["off"][s]), int(b["off"][s + 1])
        for j in np.flatnonzero(chain_invalid(pat, e - a)):
            b["price"][a + j] = BAD_PRICES[k % len(BAD_PRICES)]; k += 1
    b["pattern"] = [pat for pat in CHAIN_PATTERNS for _ in CHAIN_LENS]
    return b


# ---------------------------------------------------------------- 4: trend_following, three chained calls on one stream
TREND_CALL1_ROWS = 20_480 + 37


@functools.lru_cache(maxsize=None)
def trend_calls(pending):
    """[call 1, call 2, call 3].  Call 1 has an odd number of valid rows when ``pending`` (the polar method then leaves a
    cached deviate), an even one otherwise, and 63 valid rows in its first 64-row group either way.  Call 2 has no valid
    row.  The first valid row of call 3 has no volume, so it draws an exponential right behind the deviate it takes."""
    r = np.random.default_rng(104)
    c1 = _batch(r, np.array([700, 0, 3000, 64, 9000, 1, TREND_CALL1_ROWS - 12765], np.int64))
    p, v = c1["price"], c1["volume"]
    p[:64] = _walk(r, 64); p[10] = np.nan
    p[-2:] = (1990.0, 1991.0); v[-2:] = (np.nan, 2.5)
    ok = ~(np.isnan(p) | (p <= 0))
    if (int(ok.sum()) % 2 == 1) != bool(pending):
        p[-1] = np.nan
    n2 = 130
    c2 = {"price": np.array([BAD_PRICES[i % len(BAD_PRICES)] for i in range(n2)]), "volume": r.uniform(0, 30, n2).round(4),
          "off": np.array([0, 64, 64, n2], np.int64)}
    c2["volume"][::3] = np.nan
    c3 = _batch(r, np.array([100, 129, 71], np.int64))
    c3["price"][:3] = (np.nan, 0.0, 2003.25); c3["volume"][:3] = (1.0, np.nan, np.nan)
    return [c1, c2, c3]


# ---------------------------------------------------------------- 5: the word buffer at exact fit
@functools.lru_cache(maxsize=None)
def fit_batch():
    r = np.random.default_rng(105)
    lens = r.integers(0, 200, 30); lens[3] = 0; lens[11] = 257
    b = _batch(r, lens)
    b["price"][-1] = 2001.5; b["volume"][-1] = np.nan          # the last row is valid and draws: the stream ends on a draw
    return b


def acc_capacity(rows):
    """bridge_acc_capacity (ivs_bridge.hpp): doubles of the stream whose acceptance flag fits in the workspace."""
    return rows * 6 + 8192


# ---------------------------------------------------------------- 6: rounding table (Python's round is the reference)
ROUND_DIGITS = (4, 6)
VOLUME_EDGE_CELLS = (np.inf, 0.0, -0.0, -5.0, np.nan, 1e-7, 4.5e-7, 9.1e9)       # beside ordinary prices


def product_residual_sign(x, p10):
    """Sign of x * p10 - fl(x * p10), exactly."""
    e = Fraction(x) * Fraction(p10) - Fraction(float(np.float64(x) * np.float64(p10)))
    return (e > 0) - (e < 0)


@functools.lru_cache(maxsize=None)
def rounding_table(nd):
    """dict kind -> float64 array of positive doubles to be rounded to nd digits.
    tie_pos / tie_neg / tie_zero: doubles nearest to (2 m + 1) / (2 p10) whose float product with p10 is exactly m + 0.5,
    by the sign of the exact residual (zero: true ties), even and odd m in each; near_tie: neighbours of those whose
    product is one ulp off m + 0.5; small: around half a unit of the last digit, and the smallest denormal; cross: log-spaced
    through 2^53 / p10 (a quarter to four times); big: 1e15, 1e300, 1e305."""
    p10 = 10 ** nd
    r = np.random.default_rng(600 + nd)
    per = 60                                                # per (sign, parity of m)
    got = {(s, par): [] for s in (1, -1) for par in (0, 1)}
    near = []
    ms = np.unique(np.floor(np.exp(r.uniform(np.log(10), np.log(4e8 if nd == 4 else 4e9), 6000))).astype(np.int64))
    r.shuffle(ms)
    for m in ms:
        m = int(m)
        x = (2 * m + 1) / (2 * p10)                         # int / int: correctly rounded
        if x * p10 != m + 0.5:
            continue
        s = product_residual_sign(x, p10)
        if s and len(got[(s, m % 2)]) < per:
            got[(s, m % 2)].append(x)
            if len(near) < 120:
                for y in (np.nextafter(x, np.inf), np.nextafter(x, 0.0)):
                    if abs(float(y) * p10 - (m + 0.5)) == np.spacing(m + 0.5):
                        near.append(float(y))
    den = 32 if nd == 4 else 128                            # (2 m + 1) / (2 p10) is a double only as odd / den
    ties = [(2 * k + 1) / den for k in (0, 1, 2, 3, 4, 5, 6, 7, 50, 51, 1000, 1001, 40000, 40001)]
    half = 0.5 / p10
    lo = 2.0 ** 53 / p10
    return {"tie_pos": np.array(got[(1, 0)] + got[(1, 1)]), "tie_neg": np.array(got[(-1, 0)] + got[(-1, 1)]),
            "tie_zero": np.array(ties), "near_tie": np.array(near),
            "small": np.array([half * 0.99998, half, half * 1.00002, float(f"4.9999e-{nd + 1}"), float(f"5e-{nd + 1}"),
                               float(f"5.0001e-{nd + 1}"), 5e-324]),
            "cross": np.concatenate([np.exp(np.linspace(np.log(lo / 4), np.log(lo * 4), 200)),
                                     [np.nextafter(lo, 0.0), lo, np.nextafter(lo, np.inf)]]),
            "big": np.array([1e15, 1e300, 1e305])}


def rounding_values(nd):
    return np.concatenate(list(rounding_table(nd).values()))


@functools.lru_cache(maxsize=None)
def rounding_batch():
    """simple_spread rounds open = price to 4 digits and a passed-through volume to 6: the 4-digit table as prices, the
    6-digit table as volumes, the shorter padded with ordinary cells; then the volume edge cells beside ordinary prices."""
    p4, v6 = rounding_values(4), rounding_values(6)
    n = max(len(p4), len(v6))
    m = len(VOLUME_EDGE_CELLS)
    price = np.concatenate([p4, 100.0 + 0.37 * np.arange(n - len(p4) + m)])
    volume = np.concatenate([v6, 1.2345 + 0.01 * np.arange(n - len(v6)), VOLUME_EDGE_CELLS])
    return {"price": price, "volume": volume, "off": np.array([0, 300, 300, n - 1, n + m], np.int64)}


# ---------------------------------------------------------------- 7: spread_simulation parameters
SPREAD_PCTS = (0.0004, 0.002, 0.05)
VOL_FACTORS = (0.5, 1.5, 3.0)


@functools.lru_cache(maxsize=None)
def param_batch():
    r = np.random.default_rng(107)
    lens = np.array([500, 0, 64, 936, 1, 499], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(off[-1])
    price, volume = _walk(r, n, sd=1e-4), r.uniform(0, 30, n).round(4)      # small steps: the trend bias stays below the spread
    price[r.random(n) < 0.02] = np.nan
    volume[r.random(n) < 0.2] = np.nan
    return {"price": price, "volume": volume, "off": off}


# ---------------------------------------------------------------- 8: the generator
MT_SEEDS = (0, 1, 2 ** 31, 2 ** 32 - 1)
MT_LENGTHS = (1, 2, 623, 624, 625, 1247, 1248, 1249)
MT_LONG = (987654321, 8_000_000)                   # (seed, words): 12 821 regenerations of the double-buffered state
MT_BAD_SEEDS = (-1, 2 ** 32)


# ---------------------------------------------------------------- 9: converter frames
@functools.lru_cache(maxsize=None)
def converter_batches():
    r = np.random.default_rng(109)
    out = []
    for n in (3000, 3100, 2900):
        b = _batch(r, np.array([n], np.int64))
        b["price"][0] = 2000.0
        out.append(b)
    return out
