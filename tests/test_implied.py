"""CPU: rules V1-V8 of DESIGN.md section 16 (Black-Scholes pricer, price -> implied vol) on the NumPy restatement
(tests/iv_ref.py) against tests/golden/implied_vol.npz, the fixture's own regeneration from mpmath, the micro cases, the host
layers (ImpliedVolatility, complete_pipeline --task implied) through an injected NumPy backend, and the ABI table.

The rounding test prints the largest |restatement - exact| / U per regime; with IVS_IV_ERRLOG=<file> set the figures are
appended to that file as well (a recorded run belongs in profiles/implied/errlog.txt)."""
import ctypes as C
import os

import numpy as np
import pytest

import iv_cases as IC
import iv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "implied_vol.npz")


def log(name, **figures):
    line = name + ": " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items())
    print(line)
    path = os.environ.get("IVS_IV_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.fixture(scope="module")
def fix():
    return IC.load_fixture(FIXTURE)


def test_restatement_against_the_fixture(fix):
    """R_CPU measured, printed and held: per regime under the figure recorded in iv_cases.py, which is itself at most 4."""
    assert set(IC.R_CPU) == set(IC.REGIMES) == set(IC.R_CPU_PRICE) and max(IC.R_CPU.values()) <= IC.R_CPU_LIMIT
    worst = {}
    for reg, p in fix.items():
        assert len(p["S"]) == IC.POINTS and (p["price"] > IC.MIN_PRICE).all()
        got = R.restate_implied(p["price"], p["S"], p["K"], p["T"], p["r"], p["is_put"])
        assert np.array_equal(got["flags"], p["flags"].astype(np.int32)) and np.isfinite(got["vol"]).all(), reg
        rv = float((np.abs(got["vol"] - p["vol_exact"]) / p["unit_vol"]).max())
        pr = R.restate_price(p["S"], p["K"], p["T"], p["r"], p["sigma"], p["is_put"])
        assert (pr["flags"] == 0).all()
        rp = float((np.abs(pr["price"] - p["price"]) / p["unit_price"]).max())
        log(f"cpu[{reg}]", vol_units=rv, R_CPU=IC.R_CPU[reg], price_units=rp, R_CPU_PRICE=IC.R_CPU_PRICE[reg])
        worst[reg] = (rv, rp)
    for reg, (rv, rp) in worst.items():
        assert rv <= IC.R_CPU[reg], (reg, rv)
        assert rp <= IC.R_CPU_PRICE[reg], (reg, rp)


def test_fixture_regenerates_from_mpmath(fix):
    """The first 8 points of every regime, generated, priced and inverted again in mpmath, equal the file bit for bit."""
    import mpmath  # noqa: F401  (a missing mpmath fails the test)
    for reg, p in fix.items():
        again = IC.generate(reg, 8)
        for k in IC.FIELDS:
            assert np.array_equal(again[k], p[k][:8]), (reg, k)


def test_fixture_keeps_off_the_thresholds(fix):
    for reg, p in fix.items():
        put, itm = p["is_put"] != 0, p["flags"] == IC.ITM
        KD = p["K"] * np.exp(-p["r"] * p["T"])
        intrinsic = np.where(put, np.maximum(KD - p["S"], 0.0), np.maximum(p["S"] - KD, 0.0))
        upper = np.where(put, KD, p["S"])
        tv = np.where(itm, p["price"] - intrinsic, p["price"])
        scale = np.where(itm, p["price"] + p["S"] + KD, p["price"])
        assert (tv >= IC.MARGIN * scale).all() and (upper - p["price"] >= IC.MARGIN * upper).all(), reg
        d = (np.log(p["S"] / p["K"]) + p["r"] * p["T"]) / (p["sigma"] * np.sqrt(p["T"]))
        g = IC.REGIMES[reg]
        assert (np.abs(d) <= g["d"] * (1 + 1e-9)).all() and set(np.unique(p["r"])) <= set(IC.RATES), reg
        assert (p["sigma"] >= g["sigma"][0]).all() and (p["sigma"] <= g["sigma"][1]).all() and (p["T"] >= g["T"][0]).all() and (p["T"] <= g["T"][1]).all()
        want_itm = {0.0: 0, 1.0: IC.POINTS}.get(g["itm"])
        assert want_itm is None or int(itm.sum()) == want_itm, reg
        assert ((np.where(put, d < 0, d > 0)) == itm).all(), reg


def test_micro_cases_on_the_restatement():
    IC.check_micro(R.restate_implied)
    IC.check_known(R.restate_price, R.restate_implied)


def test_pricer_dead_inputs_on_the_restatement():
    live = dict(S=100.0, K=110.0, T=0.5, r=0.01, sigma=0.4)
    for k in live:
        for bad in (IC.NAN, IC.INF, -IC.INF) + (() if k == "r" else (0.0, -1.0)):
            c = dict(live)
            c[k] = bad
            got = R.restate_price(c["S"], c["K"], c["T"], c["r"], c["sigma"], 0.0)
            assert got["flags"][0] == IC.DEAD and np.isnan(got["price"][0]) and np.isnan(got["vega"][0]), (k, bad)
    assert R.restate_price(100.0, 110.0, 0.5, -0.01, 0.4, 1.0)["flags"][0] == 0


def test_price_modes_agree_on_the_restatement(fix):
    j = IC.joined(fix)
    a = R.restate_implied(j["price"], j["S"], j["K"], j["T"], j["r"], j["is_put"], 0)
    b = R.restate_implied(j["price"] / j["S"], j["S"], j["K"], j["T"], j["r"], j["is_put"], 1)
    assert np.array_equal(a["flags"], b["flags"])
    # the division and the multiplication each round the price once more: one more unit on top of the restatement's own
    assert (np.abs(a["vol"] - b["vol"]) <= (2 * max(IC.R_CPU.values()) + 2) * j["unit_vol"]).all()


def test_implied_volatility_argument_handling():
    from iv_interpolation_amd import ImpliedVolatility as IV
    from iv_interpolation_amd import _lib, implied
    be = R.RefBackend()
    k = IC.KNOWN
    p = IV.price(k["S"], k["K"], k["T"], k["r"], k["sigma"], "call", backend=be)
    assert set(p) == {"price", "vega", "flags"} and np.ndim(p["price"]) == 0 and abs(p["price"] - 1120.4215468331388) < 1e-9
    v = IV.implied_vol(p["price"], k["S"], k["K"], k["T"], k["r"], backend=be)
    assert set(v) == {"vol", "flags"} and np.ndim(v["vol"]) == 0 and abs(v["vol"] - 0.6) < 1e-12 and v["flags"] == 0
    # broadcasting: strikes along one axis, sides by option_type, the mark convention by price_mode
    K = np.array([[24000.0, 25500.0, 27000.0]])
    T = np.array([[0.05], [0.5]])
    pp = IV.price(k["S"], K, T, k["r"], k["sigma"], "put", backend=be)
    assert pp["price"].shape == (2, 3) and pp["flags"].dtype == np.int32
    vv = IV.implied_vol(pp["price"] / k["S"], k["S"], K, T, k["r"], "put", price_mode="underlying", backend=be)
    assert vv["vol"].shape == (2, 3) and np.allclose(vv["vol"], 0.6, rtol=0, atol=1e-11)
    assert ((vv["flags"] & _lib.IV_ITM) != 0).tolist() == [[False, True, True]] * 2    # K above the forward
    assert np.array_equal(IV.implied_vol(pp["price"], k["S"], K, T, k["r"], "p", price_mode=0, backend=be)["vol"],
                          IV.implied_vol(pp["price"], k["S"], K, T, k["r"], "put", price_mode="quote", backend=be)["vol"])
    for bad in ("spot", 2, None, True):
        with pytest.raises(ValueError, match="price_mode"):
            IV.implied_vol(1.0, 2.0, 2.0, 1.0, 0.0, price_mode=bad, backend=be)
    with pytest.raises(ValueError, match="option_type"):
        IV.price(1.0, 1.0, 1.0, 0.0, 0.2, "straddle", backend=be)
    with pytest.raises(ValueError):                                           # shapes that do not broadcast
        IV.price(np.ones(3), np.ones(2), 1.0, 0.0, 0.2, backend=be)
    c = implied.count_flags(np.array([0, 1, 3, 4, 8, 17, 16], np.int32))
    assert c == {"solved_rows": 2, "itm_rows": 3, "below_rows": 1, "above_rows": 1, "dead_rows": 1, "edge_rows": 2}
    assert (_lib.IV_ITM, _lib.IV_BELOW, _lib.IV_ABOVE, _lib.IV_DEAD, _lib.IV_EDGE) == (R.ITM, R.BELOW, R.ABOVE, R.DEAD, R.EDGE)


def test_implied_task_end_to_end(tmp_path):
    """--task implied on frame_store's synthetic chain: every stored row with a mark goes through the solver in price_mode
    "underlying" with its own rate, expiry, strike, side and underlying price."""
    import complete_pipeline as cp
    from iv_interpolation_amd.frame_store import FrameStore, synthetic_chain
    store = FrameStore(str(tmp_path))
    frames = synthetic_chain("btc", expiry_days=(2, 9), strikes=(24000.0, 25000.0, 26000.0), n_hours=4, seed=3)
    frames += synthetic_chain("eth", expiry_days=(9,), strikes=(25000.0,), n_hours=3, seed=4)
    frames[0] = frames[0].copy()
    frames[0].loc[frames[0].index[1], "mark_price"] = np.nan                   # a row without a mark is left out
    frames[1] = frames[1].copy()
    frames[1]["mark_price"] = frames[1]["mark_price"].astype(np.float64)
    frames[1].loc[frames[1].index[0], "mark_price"] = 1.5                      # more than the underlying: ABOVE
    for f in frames:
        store.write_output(f["symbol"].iloc[0], f, 1)
    assert cp.main(["--task", "implied", "--data-dir", str(tmp_path)], implied_backend=R.RefBackend()) == 0
    assert sorted(store.symbols("iv_implied")) == ["btc", "eth"]
    n_rows = 0
    for und in ("btc", "eth"):
        out = store.read_table("iv_implied", und)
        assert list(out.columns) == ["symbol", "date", "iv", "iv_from_mark", "iv_diff", "flags"]
        src = pd_concat([store.read_output(s) for s in store.symbols("interpolated_trading_tickers") if s.startswith(und)])
        src = src[src["mark_price"].notna()]
        assert len(out) == len(src) and out["symbol"].tolist() == src["symbol"].tolist()
        ref = R.restate_implied(src["mark_price"], src["underlying_price"], src["strike"], src["time_to_maturity"],
                                src["interest_rate"], (src["callput"] == "p").to_numpy(np.float64), 1)
        assert np.array_equal(out["flags"].to_numpy(np.int32), ref["flags"])
        assert np.allclose(out["iv_from_mark"].to_numpy(), ref["vol"], rtol=1e-12, atol=0, equal_nan=True)
        assert np.allclose(out["iv_diff"].to_numpy(), ref["vol"] - src["iv"].to_numpy(), rtol=1e-9, atol=1e-12, equal_nan=True)
        n_rows += len(out)
    pipe = cp.CompleteOptimizedPipeline(cp.get_config(), data_dir=str(tmp_path), implied_backend=R.RefBackend())
    res = pipe.run_implied()
    assert res["success"] and res["underlyings"] == 2 and res["rows"] == n_rows == sum(len(f) for f in frames) - 1
    assert res["above_rows"] == 1 and res["dead_rows"] == 0 and res["solved_rows"] + res["below_rows"] + res["above_rows"] + res["edge_rows"] == n_rows
    assert res["solved_rows"] > n_rows // 2
    empty = cp.CompleteOptimizedPipeline(cp.get_config(), data_dir=str(tmp_path / "none"), implied_backend=R.RefBackend())
    assert empty.run_implied()["success"] is False
    with pytest.raises(SystemExit):
        cp.main(["--task", "vols", "--data-dir", str(tmp_path)])


def pd_concat(frames):
    import pandas as pd
    return pd.concat(frames, ignore_index=True)


def test_abi_table():
    """The two symbols exist in libivs.so with the documented argument counts, and refuse bad arguments before any launch
    (fake non-null pointers are never dereferenced)."""
    import re
    from iv_interpolation_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ivs.h")).read(), flags=re.S)
    for name, n_args in (("ivs_bs_price_f64", 12), ("ivs_bs_implied_vol_f64", 12)):
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == n_args
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(decl.split(",")) == n_args, name
    assert lib.ivs_version() == _lib.ABI_VERSION == 5
    for k, v in (("ITM", 1), ("BELOW", 2), ("ABOVE", 4), ("DEAD", 8), ("EDGE", 16)):
        assert re.search(r"IVS_IV_" + k + r"\s*=\s*" + str(v) + r"\b", src), k
    P = C.c_void_p(64)
    iv = lambda **kw: lib.ivs_bs_implied_vol_f64(kw.get("price", P), P, P, P, P, None, 0, kw.get("mode", 0), kw.get("n", 10),  # noqa: E731
                                                 kw.get("vol", P), kw.get("flags", P), None)
    assert iv(vol=None) == -22 and b"ivs_bs_implied_vol_f64: null pointer" in lib.ivs_last_error()
    assert iv(flags=None) == -22 and iv(price=None) == -22
    assert iv(n=-1) == -22 and b"negative size" in lib.ivs_last_error()
    assert iv(mode=2) == -22 and b"price_mode=2" in lib.ivs_last_error()
    assert iv(mode=-1) == -22
    assert iv(n=1 << 31) == -34 and b"exceed one launch" in lib.ivs_last_error()
    assert iv(n=0) == 0 and iv(n=0, vol=None) == 0 and lib.ivs_last_error() == b""
    pr = lambda **kw: lib.ivs_bs_price_f64(P, P, P, P, kw.get("sigma", P), None, 0, kw.get("n", 10), kw.get("price", P), None, None, None)  # noqa: E731
    assert pr(price=None) == -22 and b"ivs_bs_price_f64: null pointer" in lib.ivs_last_error()
    assert pr(sigma=None) == -22 and pr(n=-1) == -22 and pr(n=1 << 31) == -34 and pr(n=0) == 0
