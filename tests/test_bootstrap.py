"""CPU: rules C0-C9 on the NumPy restatement (tests/boot_ref.py): the tables by hand, the consequences of the
rules, the host-side checks and the C refusals (which need the library but no device), and the host layers (builder, frame, pipeline
task) with the restatement as the backend.  The device tests are in test_bootstrap_gpu.py."""
import ctypes
import math

import numpy as np
import pytest

import boot_cases as BC
import boot_ref as BR
import hsim_ref as H

KEYS = BR.OUT_KEYS


def same_bits(a, b, keys, what):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), (k, what)
        if x.dtype.kind == "f":
            assert np.array_equal(np.signbit(np.nan_to_num(x)), np.signbit(np.nan_to_num(y))), (k, what)


def run(t, **over):
    t = {**t, **over}
    return BR.bootstrap(t["pnl"], t["scen_flags"], t["tail_probs"], t["min_scen"], t["n_rep"], t["block"], t["seed"], t["ci_probs"])


_cache = {}


def table(name):
    if name not in _cache:
        _cache[name] = run(BC.TABLES[name])
    return _cache[name]


# ------------------------------------------------------------------ the tables
def test_the_words_of_the_first_table():
    got = BR.words(23, np.arange(3)[:, None], np.arange(2)[None, :], 4)
    assert got.tolist() == BC.FOUR_WORDS == [[BR.word_by_hand(23, r, i, 4) for i in range(2)] for r in range(3)]
    assert BR.positions(4, 2, 23, 3).tolist() == [[3, 0, 2, 3], [1, 2, 2, 3], [3, 0, 3, 0]]          # r = 0 and 2 wrap past n - 1
    big = BR.words(2 ** 64 - 1, np.array([0, 1023]), np.array([1023, 0]), 1024)                      # the sum wraps mod 2^64
    assert big.tolist() == [BR.word_by_hand(2 ** 64 - 1, 0, 1023, 1024), BR.word_by_hand(2 ** 64 - 1, 1023, 0, 1024)]
    u = BR.words(5, np.arange(64)[:, None], np.arange(64)[None, :], 1000)
    assert u.min() >= 0 and u.max() < 1000 and len(np.unique(u)) > 900


@pytest.mark.parametrize("name", sorted(BC.TABLES))
def test_tables_by_hand(name):
    t, r = BC.TABLES[name], table(name)
    for k, v in t["want"].items():
        g = np.asarray(r[k])[0] if np.ndim(v) < np.ndim(r[k]) else np.asarray(r[k])
        assert np.array_equal(g, np.asarray(v, g.dtype).reshape(g.shape), equal_nan=True), (name, k, g, v)
    tp = np.asarray(t["tail_probs"])
    for p in range(t["pnl"].shape[0]):                       # C5 as the rule reads, one rank at a time
        if not r["active"][p]:
            assert np.isnan(r["rep"][p]).all() and np.isnan(r["mean"][p]).all() and np.isnan(r["quant"][p]).all()
            continue
        v, rho = BR.ranked(t["pnl"][p], t["scen_flags"][p])
        n = len(v)
        assert (r["counts"][p].sum(axis=1) == n).all()
        for rr in range(t["n_rep"]):
            for l in range(len(tp)):
                m = max(1, int(np.floor(np.float64(n) * tp[l])))
                var, es = BR.walk(r["counts"][p][rr], v, m)
                assert var.tobytes() == r["rep"][p, rr, 0, l].tobytes() and es.tobytes() == r["rep"][p, rr, 1, l].tobytes(), (name, rr, l)


def test_the_deep_walk_and_the_wrapping_block():
    t, r = BC.TABLES["rising"], table("rising")
    lowest = (r["counts"][0] > 0).argmax(axis=1)                                                     # the lowest rank each replicate drew
    assert lowest.max() >= 16 and lowest.min() == 0, lowest                                          # m = 3 and 16: walks that start deep in the row
    pos = BR.positions(64, 32, t["seed"], t["n_rep"])
    assert (np.diff(pos[:, :32], axis=1) < 0).any()                                                  # a block that wraps past n - 1
    assert (r["rep"][0, :, 0, 0] <= 20.0 - lowest).all()                                             # v = rank - 20: the walk ends at or past the lowest rank
    m = BR.positions(10, 4, 23, 16)                          # L' = 4 does not divide n = 10: the last block is cut to two draws
    assert m.shape == (16, 10) and ((m[:, 9] - m[:, 8]) % 10 == 1).all()


def test_zeros_keep_their_sign_out():
    r = table("zeros")
    for k in ("rep", "mean", "quant", "var0", "es0"):
        assert not np.signbit(r[k][r[k] == 0.0]).any(), k
    assert (r["rep"][0, :, 0, 0] == 0.0).any()


def test_garbage_under_a_flag_does_not_matter():
    r = table("garbage")
    same_bits({k: r[k][0] for k in KEYS}, {k: r[k][1] for k in KEYS}, KEYS, "two rows with the same ranked scenarios")


# ------------------------------------------------------------------ the consequences of the rules
@pytest.fixture(scope="module")
def base():
    c = BC.make("w256")
    return c, run(c)


def test_var0_es0_are_h7(base):
    for name in ("w63", "w256", "w1024_l7"):
        c = BC.make(name)
        r = run(c, n_rep=2)
        var, es, n_valid, _ = H.tail(c["pnl"], c["scen_flags"], c["tail_probs"], c["min_scen"])
        same_bits(r, dict(var0=var, es0=es, n_scen=n_valid), ("var0", "es0", "n_scen"), name)
    c = BC.make("w1024_l7")
    assert not run(c, n_rep=2)["active"].any()


def test_a_block_as_long_as_the_row_is_the_sample():
    """L >= n: every replicate is a rotation of the sample, so rep and quant carry the bits of var0 / es0."""
    for name, L in (("w64", 64), ("w64", 1024), ("w63", 1024)):
        c = BC.make(name)
        r = run(c, block=L, n_rep=5)
        act = r["active"]
        assert act.any()
        for k, own in enumerate(("var0", "es0")):
            want = np.broadcast_to(r[own][:, None, :], r["rep"][:, :, k, :].shape)
            same_bits(dict(v=r["rep"][:, :, k, :][act]), dict(v=want[act]), ("v",), (name, own))
            same_bits(dict(v=r["quant"][:, k][act]), dict(v=np.broadcast_to(r[own][:, :, None], r["quant"][:, k].shape)[act]), ("v",), (name, own))
        assert (r["variance"][act] <= (1e-15 * r["mean"][act]) ** 2).all()                           # the mean of five equal values is rounded


def test_es_is_at_least_var(base):
    c, r = base
    assert r["active"].all() and (r["rep"][:, :, 1, :] >= r["rep"][:, :, 0, :]).all()
    assert (r["variance"] > 0.0).all() and (r["quant"][..., 0] <= r["quant"][..., 1]).all()


def test_a_row_times_two(base):
    c, r = base
    d = run(c, pnl=c["pnl"] * 2.0)
    for k in ("var0", "es0", "mean", "quant", "rep"):
        same_bits(d, {k: r[k] * 2.0}, (k,), "times 2")
    same_bits(d, dict(variance=r["variance"] * 4.0), ("variance",), "times 4")


def test_prefix_property(base):
    c, r = base
    assert c["n_rep"] == 1024
    for n_rep in (1, 2):
        same_bits(run(c, n_rep=n_rep), dict(rep=r["rep"][:, :n_rep]), ("rep",), n_rep)


def test_a_row_alone_and_elsewhere():
    c = BC.make("w64")
    r = run(c)
    for p in (0, 37, 69):
        one = run(c, pnl=c["pnl"][p:p + 1], scen_flags=c["scen_flags"][p:p + 1])
        same_bits({k: one[k][0] for k in KEYS}, {k: r[k][p] for k in KEYS}, KEYS, p)
    perm = np.random.default_rng(1).permutation(70)
    moved = run(c, pnl=c["pnl"][perm], scen_flags=c["scen_flags"][perm])
    same_bits(moved, {k: r[k][perm] for k in KEYS}, KEYS, "permuted rows")
    one_level = run(c, tail_probs=c["tail_probs"][1:], ci_probs=())
    same_bits(one_level, dict(rep=r["rep"][..., 1:], mean=r["mean"][..., 1:], variance=r["variance"][..., 1:]), ("rep", "mean", "variance"), "one level")
    assert one_level["quant"].shape == (70, 2, 1, 0)


def test_the_cases_cover_the_shapes():
    s = BC.CASES.values()
    assert {c["B"] for c in s} == {1, 3, 70} and {c["window"] for c in s} == {1, 2, 63, 64, 65, 256, 257, 1024}
    assert {c["R"] for c in s} == {1, 2, 255, 256, 257, 1024} and {c["nL"] for c in s} == {0, 1, 2, 8} and {c["nC"] for c in s} == {0, 1, 8, 2}
    rel = {c["L"] - c["window"] for c in s if c.get("clean")}
    assert {-1, 0, 1} <= rel and {1, 2, 7, 1024} <= {c["L"] for c in s}
    for name in BC.CASES:
        c = BC.make(name)
        r = run(c)
        assert r["rep"].shape == (c["pnl"].shape[0], c["n_rep"], 2, len(c["tail_probs"]))
        if not BC.CASES[name].get("clean") and name != "w1024_l7":
            assert (r["n_scen"] < c["pnl"].shape[1]).any() or c["pnl"].shape[1] < 8


def test_statistical_sanity():
    """The bootstrap standard deviation of the 5 % VaR of 256 standard normals against the asymptotic sqrt(p (1 - p) / n) / phi(z_p):
    a check against gross errors (a wrong n, an off-by-one in m), not a measurement.  On the restatement only."""
    p, n = 0.05, 256
    z = -1.6448536269514722
    asym = math.sqrt(p * (1 - p) / n) / (math.exp(-0.5 * z * z) / math.sqrt(2 * math.pi))
    assert abs(asym - 0.132) < 5e-4
    ratios = []
    for i in range(12):
        row = np.random.default_rng(100 + i).standard_normal((1, n))
        r = BR.bootstrap(row, np.zeros((1, n), np.int32), (p,), 20, 1024, 1, i, ())
        ratios.append(float(np.sqrt(r["variance"][0, 0, 0])) / asym)
    mean = float(np.mean(ratios))
    print(f"bootstrap sd / asymptotic: mean {mean:.3f}, rows {min(ratios):.2f}..{max(ratios):.2f}")
    assert 0.75 <= mean <= 1.25, (mean, ratios)


# ------------------------------------------------------------------ argument checks: no device
def test_bootstrap_settings():
    from iv_interpolation_amd import _lib, engine
    assert engine.bootstrap_settings(256, (0.05, 0.01), 20, 512, 1, 0, (0.05, 0.95)) == (256, [0.05, 0.01], 20, 512, 1, 0, [0.05, 0.95])
    assert _lib.BOOT_MAX_REP == 1024 and engine.bootstrap_settings(1, (), 1, 1024, 1024, 2 ** 64 - 1, ())[5] == 2 ** 64 - 1
    bad = [dict(window=0), dict(window=1025), dict(tail_probs=(1.0,)), dict(tail_probs=(0.1,) * 9), dict(min_scen=0), dict(n_rep=0), dict(n_rep=1025),
           dict(n_rep=2.5), dict(block=0), dict(block=1025), dict(seed=-1), dict(seed=2 ** 64), dict(seed=0.5), dict(ci_probs=(0.0,)), dict(ci_probs=(1.0,)),
           dict(ci_probs=(float("nan"),)), dict(ci_probs=(0.5,) * 9)]
    for b in bad:
        kw = dict(window=256, tail_probs=(0.05,), min_scen=20, n_rep=512, block=1, seed=0, ci_probs=(0.05, 0.95))
        kw.update(b)
        with pytest.raises(ValueError):
            engine.bootstrap_settings(**kw)


def _dbl(*xs):
    a = (ctypes.c_double * max(len(xs), 1))(*xs)
    return ctypes.cast(a, ctypes.POINTER(ctypes.c_double))


def _args(**over):
    """A call that passes every check but names buffers that do not exist: it must be refused before any of them is touched."""
    from iv_interpolation_amd import _lib
    a = _lib.BootstrapArgs()
    for k, t in _lib.BootstrapArgs._fields_:
        if t is ctypes.c_void_p:
            setattr(a, k, 0x1000)
    a.tail_probs, a.nL, a.ci_probs, a.nC = _dbl(0.05, 0.01), 2, _dbl(0.05, 0.95), 2
    a.B, a.window, a.min_scen, a.n_rep, a.block, a.seed = 100, 256, 20, 512, 1, 7
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_c_refusals_touch_nothing():
    from iv_interpolation_amd import _lib
    lib = _lib.load()                                        # a library that is missing or lacks the entry point fails here
    EINVAL, ERANGE = -22, -34
    assert lib.ivs_version() == 5
    assert lib.ivs_hsim_bootstrap_f64(None, None, 0, None) == EINVAL
    table = [(EINVAL, dict(B=-1)), (EINVAL, dict(nL=-1)), (EINVAL, dict(nC=-1)), (ERANGE, dict(window=0)), (ERANGE, dict(window=1025)), (ERANGE, dict(nL=9)),
             (EINVAL, dict(tail_probs=None)), (ERANGE, dict(tail_probs=_dbl(0.05, 1.0))), (ERANGE, dict(tail_probs=_dbl(float("nan"), 0.5))),
             (ERANGE, dict(min_scen=0)), (ERANGE, dict(n_rep=0)), (ERANGE, dict(n_rep=1025)), (ERANGE, dict(block=0)), (ERANGE, dict(block=1025)),
             (ERANGE, dict(nC=9)), (EINVAL, dict(ci_probs=None)), (ERANGE, dict(ci_probs=_dbl(0.0, 0.5))), (ERANGE, dict(ci_probs=_dbl(0.5, float("inf")))),
             (ERANGE, dict(B=2 ** 31 // 256 + 1)), (ERANGE, dict(B=2 ** 31 // (1024 * 2 * 2) + 1, window=1, n_rep=1024)),
             (ERANGE, dict(B=2 ** 31 // (2 * 8 * 8) + 1, window=1, n_rep=1, nL=8, nC=8, tail_probs=_dbl(*[0.1] * 8), ci_probs=_dbl(*[0.5] * 8))),
             (EINVAL, dict(pnl=None)), (EINVAL, dict(scen_flags=None)), (EINVAL, dict(n_scen=None)), (EINVAL, dict(var0=None)), (EINVAL, dict(es0=None)),
             (EINVAL, dict(mean=None)), (EINVAL, dict(variance=None)), (EINVAL, dict(quant=None))]
    for want, over in table:
        a = _args(**over)
        rc = lib.ivs_hsim_bootstrap_f64(ctypes.byref(a), None, 0, None)
        assert rc == want, (over, rc, lib.ivs_last_error())
        assert lib.ivs_last_error() and lib.ivs_last_kernel() == b""
    need = lib.ivs_hsim_bootstrap_workspace_bytes(100, 512, 2)
    assert need == 100 * 512 * 2 * 2 * 8 and lib.ivs_hsim_bootstrap_workspace_bytes(100, 512, 0) == 0
    assert lib.ivs_hsim_bootstrap_workspace_bytes(0, 512, 2) == 0 and lib.ivs_hsim_bootstrap_workspace_bytes(2 ** 40, 1024, 8) == 0
    for ws, nbytes in ((None, 0), (None, need), (0x1000, need - 1), (0x1000, 0)):                    # no rep: the workspace has to hold the replicates
        assert lib.ivs_hsim_bootstrap_f64(ctypes.byref(_args(rep=None)), ws, nbytes, None) == EINVAL, (ws, nbytes)
        assert b"workspace" in lib.ivs_last_error() and lib.ivs_last_kernel() == b""
    # the limits come before the zero-size return, and an empty call is a no-op on buffers that do not exist
    assert lib.ivs_hsim_bootstrap_f64(ctypes.byref(_args(B=0)), None, 0, None) == 0
    assert lib.ivs_hsim_bootstrap_f64(ctypes.byref(_args(B=0, rep=None, pnl=None)), None, 0, None) == 0
    assert lib.ivs_hsim_bootstrap_f64(ctypes.byref(_args(B=0, n_rep=1025)), None, 0, None) == ERANGE


# ------------------------------------------------------------------ host layers with the restatement as the backend
HOUR = 60
KW = dict(rate=0.01, lag=HOUR, window=8, tail_probs=(0.5, 0.25), min_scenarios=1)


def _built():
    import pandas as pd
    from iv_interpolation_amd.snapshots import SnapshotSurfaceBuilder
    from iv_interpolation_amd.frame_store import synthetic_chain
    chain = synthetic_chain("btc", expiry_days=(0.5, 3), strikes=tuple(np.linspace(17000.0, 34000.0, 12)), n_hours=5, seed=5)
    b = SnapshotSurfaceBuilder(backend=BR.RefBackend(), moneyness=np.linspace(0.72, 1.28, 24), tenors=np.array([1.0, 2.0, 2.8]) / 365)
    res = b.build(chain)
    svi = b.svi(res, rate=0.01, rounds=6)
    t0 = res[0].dates[0]
    bk = pd.DataFrame({"symbol": list("abc"), "strike": [20000.0, 25000.0, 30000.0], "expiry": [t0 + pd.Timedelta(days=d) for d in (1.5, 2.5, 5.0)],
                       "callput": ["c", "P", "call"], "quantity": [2.0, -1.0, 0.5]})
    return b, res, svi, bk


def test_builder_report_and_frame():
    from iv_interpolation_amd.snapshots import BootstrapReport, confidence_frame
    b, res, svi, bk = _built()
    var = b.var(res, bk, svi, **KW)
    reps = b.var_confidence(var, n_rep=16, seed=3, ci=(0.1, 0.5, 0.9))
    assert len(reps) == 1 and isinstance(reps[0], BootstrapReport)
    p = reps[0]
    assert p.block == HOUR and p.n_rep == 16 and p.seed == 3 and list(p.ci) == [0.1, 0.5, 0.9] and p.var is var[0].var      # block=None: the lag
    ref = BR.bootstrap(var[0].pnl, var[0].scen_flags, (0.5, 0.25), 1, 16, HOUR, 3, (0.1, 0.5, 0.9))
    for k in ("var0", "es0", "n_scen", "mean", "variance", "quant"):
        assert np.array_equal(getattr(p, k), ref[k], equal_nan=True), k
    assert np.array_equal(p.se, np.sqrt(ref["variance"]), equal_nan=True)
    assert np.array_equal(p.var0, var[0].var, equal_nan=True) and np.array_equal(p.n_scen, var[0].n_valid)
    one = b.var_confidence(var, n_rep=16, block=1, seed=3)[0]
    assert one.block == 1 and list(one.ci) == [0.05, 0.95] and np.isfinite(one.se).any()
    r = res[0]
    keep = np.flatnonzero(np.asarray(r.quotes) > 0)
    f = confidence_frame(reps, res)
    assert list(f.columns) == ["underlying", "date", "n_valid"] + [f"{s}_{tp}{e}" for tp in ("0.5", "0.25") for s in ("var", "es") for e in ("", "_se", "_lo", "_hi")]
    assert len(f) == len(keep) and (f["date"] == r.dates[keep]).all() and (f["n_valid"] == np.asarray(var[0].n_valid)[keep]).all()
    assert np.array_equal(f["var_0.5"], np.asarray(var[0].var)[keep, 0], equal_nan=True)
    assert np.array_equal(f["es_0.25_se"], np.sqrt(ref["variance"])[keep, 1, 1], equal_nan=True)
    assert np.array_equal(f["es_0.25_lo"], ref["quant"][keep, 1, 1, 0], equal_nan=True) and np.array_equal(f["var_0.5_hi"], ref["quant"][keep, 0, 0, 2], equal_nan=True)
    assert len(confidence_frame([], [])) == 0
    for kw in (dict(n_rep=0), dict(n_rep=1025), dict(block=0), dict(seed=-1), dict(ci=(1.5,))):
        with pytest.raises(ValueError):
            b.var_confidence(var, **kw)


def test_varci_task_end_to_end(tmp_path):
    import complete_pipeline as cp
    from iv_interpolation_amd.frame_store import FrameStore, synthetic_chain
    store = FrameStore(str(tmp_path))
    chain = synthetic_chain("btc", expiry_days=(20, 45), strikes=tuple(np.linspace(17000.0, 34000.0, 6)), n_hours=4, seed=5)
    for f in chain:
        store.write_output(f["symbol"].iloc[0], f, 1)
    argv = ["--task", "varci", "--replicates", "32", "--seed", "4", "--ci", "0.1,0.9", "--lag", "60", "--window", "121", "--levels", "0.5,0.25",
            "--min-scenarios", "1", "--data-dir", str(tmp_path)]
    assert cp.main(argv, surface_backend=BR.RefBackend()) == 0
    out, var = store.read_table("iv_var_ci", "btc"), store.read_table("iv_var", "btc")
    assert list(out.columns)[:3] == ["underlying", "date", "n_valid"] and len(out) == len(var) > 0
    assert np.array_equal(out["var_0.5"], var["var_0.5"], equal_nan=True) and np.array_equal(out["es_0.25"], var["es_0.25"], equal_nan=True)
    ok = np.isfinite(out["var_0.5"].to_numpy())
    assert ok.any() and (out["var_0.5_lo"][ok] <= out["var_0.5_hi"][ok]).all() and (out["var_0.5_se"][ok] >= 0).all()
    pipe = cp.CompleteOptimizedPipeline(cp.get_config(), data_dir=str(tmp_path), surface_backend=BR.RefBackend())
    kw = dict(lag=60, window=121, levels=(0.5, 0.25), min_scenarios=1)
    res = pipe.run_varci(replicates=32, seed=4, ci=(0.1, 0.9), **kw)
    assert res["success"] and res["ci_rows"] == len(out) and set(res) == set(pipe.run_var(**kw)) | {"ci_rows", "median_rel_se"}
    assert len(res["median_rel_se"]) == 2 and all(np.isfinite(x) and x >= 0 for x in res["median_rel_se"])
    again = store.read_table("iv_var_ci", "btc")
    assert np.array_equal(again["var_0.5_se"], out["var_0.5_se"], equal_nan=True)                    # block=None is the lag, as the command line's default
    other = pipe.run_varci(replicates=32, seed=5, block=1, ci=(0.1, 0.9), **kw)
    assert other["success"] and not np.array_equal(store.read_table("iv_var_ci", "btc")["var_0.5_se"], out["var_0.5_se"], equal_nan=True)
    assert "n_rep" in pipe.run_varci(replicates=0)["error"] and "block" in pipe.run_varci(block=2000)["error"]
    assert "interval" in pipe.run_varci(ci=(0.0,))["error"] and "window" in pipe.run_varci(window=0)["error"]
