"""Candle aggregation: oracle vs the real reference's golden outputs (CPU), HIP kernel vs both (GPU, bit-exact)."""
import os
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import candles_oracle as CO  # noqa: E402
import candle_ref as CR  # noqa: E402
from candle_cases import CASES as EDGE  # noqa: E402
from golden_io import GOLDEN  # noqa: E402

g = np.load(os.path.join(GOLDEN, "candles.npz"))
CASES = [(str(n), str(f)) for n, f in zip(g["names"], g["freqs"])]
KEYS = ("open", "high", "low", "close", "volume")


def _minutes(f):
    return int(f[:-3]) if f.endswith("min") else int(f[:-1])


@pytest.mark.parametrize("name,freq", CASES)
def test_oracle_against_reference_golden(name, freq):
    r = CO.aggregate(*[g[f"{name}/{k}"] for k in ("ts", "o", "h", "l", "c", "v")], _minutes(freq))
    if bool(g[f"{name}/none"]):
        assert r is None
        return
    assert np.array_equal(r["timestamp"], g[f"{name}/out_ts"])
    for k in KEYS:
        assert np.array_equal(r[k], g[f"{name}/out_{k}"], equal_nan=True), k     # bit-exact incl. Kahan volume


def test_known_answer_survey_8f():
    r = CO.aggregate(g["kat/ts"], g["kat/o"], g["kat/h"], g["kat/l"], g["kat/c"], g["kat/v"], 5)
    assert [tuple(r[k][i] for k in KEYS) for i in range(2)] == [(100, 106, 99, 105, 10), (105, 111, 104, 110, 35)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,freq", CASES)
def test_hip_candles_against_reference_golden(name, freq):
    from iv_interpolation_amd.candles import CandleReconstructor
    df = pd.DataFrame({"symbol": "btc-20mar23-25000-c", "timestamp": pd.to_datetime(g[f"{name}/ts"]),
                       **{c: g[f"{name}/{k}"] for c, k in zip(KEYS, "ohlcv")}})
    out = CandleReconstructor(freq).reconstruct_symbol_candles(df)
    if bool(g[f"{name}/none"]):
        assert out is None
        return
    assert list(out.columns) == ["symbol", "timestamp", "open", "high", "low", "close", "volume", "frequency", "source_candles", "created_at"]
    assert np.array_equal(out["timestamp"].to_numpy().astype("datetime64[ns]").astype(np.int64), g[f"{name}/out_ts"])
    for k in KEYS:
        assert np.array_equal(out[k].to_numpy(), g[f"{name}/out_{k}"], equal_nan=True), k


@pytest.mark.gpu
def test_hip_candles_batch_vs_oracle():
    from iv_interpolation_amd.candles import CandleReconstructor
    r = np.random.default_rng(3)
    frames = []
    for s in range(50):
        n = int(r.integers(3, 3000))
        ts = pd.Timestamp("2023-03-01") + pd.to_timedelta(np.sort(r.choice(4000, n, replace=False)), unit="min")
        o = r.uniform(90, 110, n); frames.append(pd.DataFrame({"symbol": f"s{s}", "timestamp": ts, "open": o, "high": o + 1, "low": o - 1,
                                                                "close": o + r.normal(0, .3, n), "volume": r.uniform(0, 9, n)}))
    outs = CandleReconstructor("5min").reconstruct_batch(frames)
    for f, o in zip(frames, outs):
        ref = CO.aggregate(f["timestamp"].to_numpy().astype("datetime64[ns]").astype(np.int64), f["open"], f["high"], f["low"], f["close"], f["volume"], 5)
        if ref is None:
            assert o is None
            continue
        assert np.array_equal(o["timestamp"].to_numpy().astype("datetime64[ns]").astype(np.int64), ref["timestamp"])
        for k in KEYS:
            assert np.array_equal(o[k].to_numpy(), ref[k], equal_nan=True)


# ---- edge cases (candle_cases.py) against the operation itself in pandas (candle_ref.py): bit for bit, the sign of zero
# included; every bucket (count >= 1) and the reference's rule for complete groups (count >= N)
def _oracle_case(case, min_rows):
    """candles_oracle.aggregate per series of a packed case, in the bucket layout of candle_ref.reference_case"""
    off = case["series_off"]
    keys = ("timestamp", "count") + CR.COLS
    parts = {k: [] for k in keys}
    for a, b in zip(off[:-1], off[1:]):
        r = CO.aggregate(case["ts"][a:b], *[c[a:b] for c in case["cols"]], case["freq"], min_rows=min_rows)
        if r is None:                                       # fewer rows than min_rows: no bucket can be complete
            continue
        for k in keys:
            parts[k].append(r[k])
    return {k: np.concatenate(v) if v else np.zeros(0, np.int64 if k in ("timestamp", "count") else np.float64)
            for k, v in parts.items()}


@pytest.mark.parametrize("name", list(EDGE))
def test_oracle_equals_pandas_on_edge_cases(name):
    case = EDGE[name]
    for min_rows in (1, case["freq"]):
        assert CR.mismatches(_oracle_case(case, min_rows), CR.reference_case(case, min_rows)) == [], (name, min_rows)


@pytest.mark.parametrize("name", list(EDGE))
def test_packed_model_equals_pandas_on_edge_cases(name):
    """The row-by-row restatement of the packed operation with every rule on: the baseline of the wrong-variant check."""
    case = EDGE[name]
    out = CR.packed_model(case["ts"], case["cols"], case["series_off"], case["freq"])
    for min_rows in (1, case["freq"]):
        assert CR.mismatches(CR.sparse_to_buckets(out, min_rows), CR.reference_case(case, min_rows)) == [], (name, min_rows)


@pytest.mark.parametrize("rule", ["series_check", "floor", "kahan", "comp_reset"])
def test_edge_cases_separate_a_wrong_candle_kernel(rule):
    """Each rule switched off in the packed model (no series check at the head, truncating division for the bucket, a
    naive sum, no reset of a NaN compensation) must be caught by at least one case under the GPU test's comparison."""
    caught = []
    for name, case in EDGE.items():
        out = CR.packed_model(case["ts"], case["cols"], case["series_off"], case["freq"], **{rule: False})
        if any(CR.mismatches(CR.sparse_to_buckets(out, m), CR.reference_case(case, m)) for m in (1, case["freq"])):
            caught.append(name)
    assert caught, rule


def test_pre_1970_buckets_floor_towards_minus_infinity():
    r = CR.reference_case(EDGE["pre_1970_minutes"], 1)
    assert list(r["timestamp"] // (5 * CR.MINUTE_NS)) == [-2, -1, 0] and list(r["count"]) == [2, 5, 3]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EDGE))
def test_hip_candles_equal_pandas_on_edge_cases(name):
    import torch
    from iv_interpolation_amd import engine
    case = EDGE[name]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    out = engine.candle_aggregate(dev(case["ts"]), *[dev(c) for c in case["cols"]], dev(case["series_off"]), case["freq"])
    out = [t.cpu().numpy() for t in out]
    assert out[6].sum() == case["ts"].size                   # every row belongs to exactly one bucket
    for min_rows in (1, case["freq"]):
        assert CR.mismatches(CR.sparse_to_buckets(out, min_rows), CR.reference_case(case, min_rows)) == [], (name, min_rows)


# ---- host-side API of the reference's module kept by the drop-in (core.py:108-300); expectations below were read off
# the REAL reference run on the same frames (known answers, data only)
def _kat_frame():
    ts = pd.date_range("2023-03-01 09:00", periods=12, freq="1min")
    o = 100 + np.arange(12.0)
    return pd.DataFrame({"symbol": "s", "timestamp": ts, "open": o, "high": o + 2, "low": o - 1, "close": o + 1,
                         "volume": np.arange(12.0)})


def test_validate_and_stats_known_answers():
    from oracle_backend import OracleCandleBackend
    from iv_interpolation_amd.candles import CandleReconstructor
    df = _kat_frame()
    r = CandleReconstructor("5min", backend=OracleCandleBackend())
    assert r.validate_candle_data(df) is True
    assert r.validate_candle_data(df.assign(high=df.low - 1)) is False          # high < low
    assert r.validate_candle_data(df.assign(volume=-1.0)) is False              # negative volume
    assert r.validate_candle_data(df.assign(open=np.nan)) is False              # nulls in a critical column
    assert r.validate_candle_data(df.iloc[:0]) is False
    assert r.validate_candle_data(df.drop(columns=["high"])) is False           # any exception -> False
    out = r.reconstruct_symbol_candles(df)
    st = r.get_reconstruction_stats(df, out)
    assert st["original_candles"] == 12 and st["reconstructed_candles"] == 2 and st["compression_ratio"] == 6.0
    assert st["original_timespan"] == pd.Timedelta(minutes=11) and st["reconstructed_timespan"] == pd.Timedelta(minutes=5)
    assert st["coverage_ratio"] == pytest.approx(0.45454545454545453, abs=0)
    assert st["total_volume_original"] == 66.0 and st["total_volume_reconstructed"] == 45.0
    assert st["volume_preservation"] == pytest.approx(0.31818181818181823, abs=1e-16)
    assert r.get_reconstruction_stats(df.iloc[:0], out) == {} and r.get_reconstruction_stats(df, out.iloc[:0]) == {}


def test_symbol_column_rules_like_the_reference_agg():
    from oracle_backend import OracleCandleBackend
    from iv_interpolation_amd.candles import CandleReconstructor
    df = _kat_frame()
    r = CandleReconstructor("5min", backend=OracleCandleBackend())
    assert r.reconstruct_symbol_candles(df.drop(columns=["symbol"])) is None   # agg({'symbol': 'first'}) raises -> None
    d2 = df.copy(); d2["symbol"] = [None, "a", "a", "a", "a", "b", "b", None, "b", "b", "c", "c"]
    out = r.reconstruct_symbol_candles(d2)
    assert list(out["symbol"]) == ["a", "b"] and list(out["open"]) == [100.0, 105.0] and list(out["volume"]) == [10.0, 35.0]
    bad = df.copy(); bad["open"] = "not a number"
    assert r.reconstruct_symbol_candles(bad) is None                             # documented: non-numeric OHLCV -> None


def test_multi_symbol_reconstructor_on_the_frame_store(tmp_path):
    from types import SimpleNamespace
    from oracle_backend import OracleCandleBackend
    from iv_interpolation_amd.candles import MultiSymbolCandleReconstructor
    from iv_interpolation_amd.frame_store import FrameStore
    from candle_reconstruction.core import MultiSymbolCandleReconstructor as Shim      # reference main.py:28 import path
    assert Shim is MultiSymbolCandleReconstructor
    store = FrameStore(str(tmp_path))
    good = _kat_frame(); good["symbol"] = "good"
    short = _kat_frame().iloc[:3].copy(); short["symbol"] = "short"
    broken = _kat_frame(); broken["symbol"] = "broken"; broken["high"] = broken["low"] - 5
    for name, f in (("good", good), ("short", short), ("broken", broken)):
        store.write_table("minute_candles", name, f)
    cfg = SimpleNamespace(candle_reconstruction=SimpleNamespace(target_frequency="5min"))
    m = MultiSymbolCandleReconstructor(store, cfg, backend=OracleCandleBackend())
    assert m.get_symbols_with_minute_data() == ["broken", "good", "short"]
    assert m.get_symbols_with_minute_data("2030-01-01", "2030-01-02") == []
    res = {r["symbol"]: r for r in m.process_symbols(["good", "short", "broken", "missing"])}
    assert res["good"]["status"] == "success" and res["good"]["input_candles"] == 12 and res["good"]["output_candles"] == 2
    assert res["good"]["stats"]["compression_ratio"] == 6.0
    assert res["short"] == {"symbol": "short", "status": "skipped", "reason": "Reconstruction failed"}
    assert res["broken"] == {"symbol": "broken", "status": "error", "error": "Invalid input candle data"}
    assert res["missing"] == {"symbol": "missing", "status": "skipped", "reason": "No minute data found"}
    assert m.process_symbol("good")["status"] == "success"                         # upsert: still two rows afterwards
    saved = store.read_table("reconstructed_candles", "good")
    assert len(saved) == 2 and list(saved["open"]) == [100.0, 105.0]
