"""Tiny deterministic edge cases for N-minute candle aggregation, packed as the device call takes them.  TEST INPUTS ONLY.

CASES maps a name to dict(ts int64 ns [n], cols = [open, high, low, close, volume] float64 [n], series_off int64 [S+1],
freq minutes).  Rows of a series are sorted by timestamp with a stable sort, so duplicate timestamps keep their order."""
import numpy as np

MIN = 60_000_000_000
T0 = 27_960_480 * MIN                 # 2023-03-01 00:00 UTC, a multiple of one day
NAN, INF = np.nan, np.inf
CASES = {}


def _plain(n, k=0):
    """benign OHLCV cells for n rows, distinct per row and per series k"""
    i = np.arange(n, dtype=np.float64)
    o = 100.0 + k + 0.25 * ((7 * i + 3 * k) % 23)
    return [o, o + 1.5 + 0.125 * (i % 3), o - 1.25 - 0.125 * (i % 5), o + 0.5 - 0.0625 * (i % 7), 1.0 + (i % 9) + 0.1 * k]


def _add(name, series, freq=5):
    """series: list of (ts_ns, cols or None); None = _plain cells"""
    ts_l, cols_l, off = [], [], [0]
    for k, (ts, cols) in enumerate(series):
        ts = np.asarray(ts, np.int64)
        cols = _plain(ts.size, k) if cols is None else [np.asarray(c, np.float64) for c in cols]
        assert all(c.size == ts.size for c in cols) and len(cols) == 5
        order = np.argsort(ts, kind="stable")
        ts_l.append(ts[order]); cols_l.append([c[order] for c in cols]); off.append(off[-1] + ts.size)
    assert name not in CASES
    CASES[name] = {"ts": np.concatenate(ts_l), "cols": [np.concatenate([c[j] for c in cols_l]) for j in range(5)],
                   "series_off": np.asarray(off, np.int64), "freq": freq}


def _minutes(a, b):
    return T0 + np.arange(a, b, dtype=np.int64) * MIN


# ---- series boundaries: the last rows of one series and the first rows of the next share a bucket number
def _shared(first_len):
    e = first_len - 1                               # last minute of series 0
    b0 = e // 5 * 5                                 # its bucket: series 1 starts inside it
    s1 = _minutes(b0, b0 + 9)
    last1 = b0 + 8
    s2 = _minutes(last1, last1 + 1)                 # one row, in the bucket of series 1's last rows
    s3 = _minutes(last1 // 5 * 5 + 1, last1 // 5 * 5 + 11)
    return [(_minutes(0, first_len), None), (s1, None), (s2, None), (s3, None)]


_add("shared_bucket", _shared(8))
_add("shared_bucket_boundary_at_row_255", _shared(255))
_add("shared_bucket_boundary_at_row_256", _shared(256))
_add("shared_bucket_boundary_at_row_257", _shared(257))
_add("same_timestamps_three_series", [(_minutes(3, 14), None)] * 3)

# ---- block boundaries (256 rows per block)
_add("bucket_rows_254_258", [(_minutes(1, 301), None)])                   # row i = minute i + 1: rows 254..258 = minutes 255..259
_add("one_bucket_three_blocks", [(_minutes(0, 600), None)], freq=1440)
for _n in (1, 255, 256, 257):
    _add(f"n_rows_{_n}", [(_minutes(2, 2 + _n), None)])

# ---- timestamps
_add("pre_1970_minutes", [(np.arange(-7, 3, dtype=np.int64) * MIN, None)])
_add("pre_1970_edges", [(np.array([-10 * MIN - 1, -10 * MIN, -5 * MIN - 1, -5 * MIN, -5 * MIN + 1, -1, 0, 1], np.int64), None)])
_add("off_grid_seconds", [(_minutes(0, 23) + (np.arange(23, dtype=np.int64) * 17_123_456_789) % MIN, None),
                          (-40 * MIN + np.arange(23, dtype=np.int64) * (MIN + 7_000_000_001), None)])
_add("duplicate_timestamps", [(T0 + np.array([0, 0, 1, 1, 1, 4, 5, 5, 5, 9, 9, 10], np.int64) * MIN, None)])

# ---- cells
for _j, _name in enumerate(("open", "high", "low", "close", "volume")):
    _c = _plain(15)
    _c[_j][5:10] = NAN                                                  # the middle bucket of this column is all NaN
    _add(f"all_nan_bucket_{_name}", [(_minutes(0, 15), _c)])
_c = _plain(10)
_c[0][:5] = [NAN, NAN, 3, 4, NAN]; _c[3][:5] = [1, NAN, 3, NAN, NAN]
_c[1][:5] = [NAN, 5, NAN, 7, NAN]; _c[2][:5] = [NAN, 5, NAN, 3, NAN]
_c[0][5:] = [NAN, 1, 2, 3, 4]; _c[3][5:] = [1, 2, 3, 4, NAN]
_add("nan_first_and_last_cells", [(_minutes(0, 10), _c)])
for _sgn, _name in ((1.0, "pos"), (-1.0, "neg")):
    _c = _plain(15)
    for _j in range(4):
        _c[_j][1] = _sgn * INF                                          # inside a bucket
        _c[_j][5] = _sgn * INF; _c[_j][9] = -_sgn * INF                 # first and last cell, both signs
        _c[_j][10] = NAN; _c[_j][11] = _sgn * INF; _c[_j][14] = NAN     # next to NaN cells
    _add(f"inf_cells_{_name}", [(_minutes(0, 15), _c)])
_z = [[NAN, -0.0, 0.0, NAN, -1.0], [NAN, 0.0, -0.0, NAN, -1.0], [-0.0, 0.0, -0.0, 0.0, -0.0], [0.0, -0.0, 0.0, -0.0, 0.0]]
_c = _plain(20)
for _j in range(4):
    _c[_j][:] = np.concatenate(_z)
_c[2][:] = -_c[2]                                                        # low: the same orders around +1
_add("signed_zero_orders", [(_minutes(0, 20), _c)])

# ---- volume
_v = [[1, INF, 2, 3, 4], [1, -INF, 2, 3, 4], [1, INF, -INF, 2, 3], [1e308, 1e308, 2, 3, 4], [-1e308, -1e308, 2, 3, 4],
      [1e16, 1, -1e16, 1, 1], [1, 1e100, 1, -1e100, 1], [0.1, 0.2, 0.3, 0.4, 0.5], [NAN] * 5, [NAN, INF, NAN, 1, NAN]]
_c = _plain(5 * len(_v)); _c[4] = np.concatenate(_v).astype(np.float64)
_add("volume_inf_overflow_kahan", [(_minutes(0, 5 * len(_v)), _c)])
_c = _plain(120); _c[4][:60] = 0.1; _c[4][60:] = np.where(np.arange(60) % 2 == 0, 1e16, 1.0) * np.where(np.arange(60) % 4 < 2, 1, -1)
_add("volume_kahan_hour", [(_minutes(0, 120), _c)], freq=60)
