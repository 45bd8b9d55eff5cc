"""Plain references for N-minute candle aggregation.  TEST INFRASTRUCTURE ONLY.

``pandas_reference`` is the operation itself, the groupby-agg the reference executes per symbol.  ``packed_model`` is a
row-by-row Python restatement of the packed multi-series operation (the layout of ivs_candle_aggregate_f64) whose
switches turn single rules off: with every switch on it must equal pandas on every case of candle_cases.py, with one
off it must not -- that is how the case table shows it can tell a wrong kernel from a right one."""
import numpy as np
import pandas as pd

MINUTE_NS = 60_000_000_000
COLS = ("open", "high", "low", "close", "volume")


def pandas_reference(ts_ns, cols, freq_minutes):
    """One symbol, rows in their packed order (sorted by timestamp).  Returns dict(timestamp int64 ns, open, high, low,
    close, volume float64, count int64) with one entry per bucket."""
    df = pd.DataFrame({"timestamp": pd.to_datetime(np.asarray(ts_ns, np.int64)), **dict(zip(COLS, cols))})
    grp = df.groupby(df["timestamp"].dt.floor(f"{freq_minutes}min"))
    agg = grp.agg(open=("open", "first"), high=("high", "max"), low=("low", "min"), close=("close", "last"),
                  volume=("volume", "sum"))
    out = {k: agg[k].to_numpy(np.float64) for k in COLS}
    out["timestamp"] = pd.DatetimeIndex(agg.index).as_unit("ns").asi8
    out["count"] = grp.size().to_numpy(np.int64)
    return out


def reference_case(case, min_rows):
    """pandas_reference per series of a packed case, buckets with at least min_rows rows, concatenated in series order."""
    off = case["series_off"]
    parts = []
    for a, b in zip(off[:-1], off[1:]):
        r = pandas_reference(case["ts"][a:b], [c[a:b] for c in case["cols"]], case["freq"])
        keep = r["count"] >= min_rows
        parts.append({k: v[keep] for k, v in r.items()})
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def sparse_to_buckets(out, min_rows):
    """The sparse per-row result (out_ts, o, h, l, c, v, count) -> the same dict layout as reference_case.  Only rows with
    count >= min_rows are read: the other rows of the OHLCV outputs are left unwritten by the ABI."""
    cnt = np.asarray(out[6])
    keep = np.flatnonzero(cnt >= max(1, min_rows))
    res = {k: np.asarray(out[1 + i])[keep] for i, k in enumerate(COLS)}
    res["timestamp"] = np.asarray(out[0])[keep]
    res["count"] = cnt[keep].astype(np.int64)
    return res


def mismatches(got, ref):
    """Bit-for-bit comparison of two bucket dicts: timestamps, counts, and the five columns with NaN == NaN and the sign
    of zero compared.  Returns one message per differing key (empty = equal)."""
    bad = [f"{k}: got {got[k].tolist()}, want {ref[k].tolist()}" for k in ("timestamp", "count") if not np.array_equal(got[k], ref[k])]
    if bad:
        return bad
    for k in COLS:
        g, r = got[k], ref[k]
        same = ((g == r) & (np.signbit(g) == np.signbit(r))) | ((g != g) & (r != r))
        if not same.all():
            i = np.flatnonzero(~same)
            bad.append(f"{k}: buckets {i.tolist()} got {g[i].tolist()}, want {r[i].tolist()}")
    return bad


def packed_model(ts, cols, series_off, freq_minutes, series_check=True, floor=True, kahan=True, comp_reset=True):
    """The packed operation row by row: row i heads a bucket when it is the first row of its series or its bucket number
    differs from row i-1's; the head reduces rows i.. while they stay inside the series and the bucket.  Returns the
    sparse layout (out_ts, o, h, l, c, v, count).  The keyword switches drop one rule each (see the module docstring)."""
    ts = np.asarray(ts, np.int64)
    n = ts.size
    f = freq_minutes * MINUTE_NS
    if floor:
        bucket = ts // f
    else:                                        # truncating division, as C's a / b
        bucket = np.where(ts < 0, -((-ts) // f), ts // f)
    out_ts = np.zeros(n, np.int64); outs = [np.full(n, np.nan) for _ in range(5)]; cnt = np.zeros(n, np.int32)
    o, h, l, c, v = [np.asarray(x, np.float64) for x in cols]
    starts = set(int(a) for a in series_off[:-1])
    end_of = np.repeat(np.asarray(series_off[1:], np.int64), np.diff(series_off))
    with np.errstate(all="ignore"):
        for i in range(n):
            head = i == 0 or bucket[i - 1] != bucket[i] or (series_check and i in starts)
            if not head:
                continue
            op = hi = lo = cl = np.nan; s = 0.0; comp = 0.0; j = i
            while j < end_of[i] and bucket[j] == bucket[i]:
                if op != op and o[j] == o[j]: op = o[j]
                if h[j] == h[j] and not (hi >= h[j]): hi = h[j]
                if l[j] == l[j] and not (lo <= l[j]): lo = l[j]
                if c[j] == c[j]: cl = c[j]
                if v[j] == v[j]:
                    if kahan:
                        y = v[j] - comp; t = s + y; comp = t - s - y
                        if comp_reset and comp != comp: comp = 0.0
                        s = t
                    else:
                        s = s + v[j]
                j += 1
            out_ts[i] = bucket[i] * f; cnt[i] = j - i
            for k, val in enumerate((op, hi, lo, cl, s)):
                outs[k][i] = val
    return [out_ts, *outs, cnt]
