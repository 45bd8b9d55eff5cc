"""CPU oracle for N-minute candle aggregation.  TEST INFRASTRUCTURE ONLY.

Restates reference ``src/candle_reconstruction/core.py:36-106`` (CandleReconstructor.reconstruct_symbol_candles):
sort by timestamp (:59), floor to the target frequency (:69), groupby-agg open=first / high=max / low=min /
close=last / volume=sum (:72-79; pandas' first/last/max/min/sum skip NaN, sum of nothing = 0), keep only groups
with at least N member rows (:86-88).  Pinned by tests/golden/candles.npz (real reference outputs)."""
import numpy as np

MINUTE_NS = 60_000_000_000


def _kahan_nansum(x):
    """pandas' groupby sum (pandas/_libs/groupby.pyx group_sum): Kahan summation in row order, NaN skipped; a
    compensation that has become NaN (inf - inf after an infinite cell) is reset to 0, so [1, inf, 2] sums to inf."""
    s = 0.0; comp = 0.0
    with np.errstate(all="ignore"):
        for val in np.asarray(x, np.float64):
            if val == val:
                y = val - comp
                t = s + y
                comp = t - s - y
                if comp != comp:
                    comp = 0.0
                s = t
    return float(s)


def _first_extreme(x, greater):
    """pandas' groupby max / min: sequential over the non-NaN cells, a later cell replaces the running one only when it
    is strictly greater / smaller, so of -0.0 and 0.0 the FIRST is kept (np.nanmax would not say which)."""
    best = np.nan
    for val in np.asarray(x, np.float64):
        if val == val and (best != best or (val > best if greater else val < best)):
            best = val
    return float(best)


def aggregate(ts_ns, o, h, l, c, v, freq_minutes, min_rows=None):
    """One symbol.  ts_ns int64 (any order), OHLCV float64.  Returns dict of arrays (bucket start ns, o, h, l, c, v)
    or None when there are fewer than freq_minutes rows (:63-66).  min_rows (default freq_minutes, the reference's
    rule) is the number of member rows a group needs to be kept; 1 keeps every group."""
    ts_ns = np.asarray(ts_ns, np.int64)
    min_rows = freq_minutes if min_rows is None else min_rows
    if ts_ns.size == 0 or ts_ns.size < min_rows:
        return None
    order = np.argsort(ts_ns, kind="stable")
    ts = ts_ns[order]
    cols = [np.asarray(a, np.float64)[order] for a in (o, h, l, c, v)]
    f = freq_minutes * MINUTE_NS
    bucket = (ts // f) * f                                     # dt.floor(f'{N}min')
    starts = np.flatnonzero(np.r_[True, bucket[1:] != bucket[:-1]])
    ends = np.r_[starts[1:], ts.size]
    out = {k: [] for k in ("timestamp", "open", "high", "low", "close", "volume", "count")}
    for a, b in zip(starts, ends):
        if b - a < min_rows:                                   # incomplete group (:86-88), counts rows incl. NaN cells
            continue
        oo, hh, ll, cc, vv = [x[a:b] for x in cols]
        first = oo[~np.isnan(oo)]; last = cc[~np.isnan(cc)]
        out["timestamp"].append(bucket[a])
        out["open"].append(first[0] if first.size else np.nan)
        out["high"].append(_first_extreme(hh, True))
        out["low"].append(_first_extreme(ll, False))
        out["close"].append(last[-1] if last.size else np.nan)
        out["volume"].append(_kahan_nansum(vv))
        out["count"].append(b - a)
    return {k: np.asarray(x, np.int64 if k in ("timestamp", "count") else np.float64) for k, x in out.items()}
