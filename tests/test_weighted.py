"""CPU: rules W0-W9 on the NumPy restatement (tests/weighted_ref.py): the tables by hand, the consequences of
the rules, the host-side checks and the C refusals (which need the library but no device), and the host layers (builder, frame,
pipeline task) with the restatement as the backend.  The device tests are in test_weighted_gpu.py."""
import ctypes
import math

import numpy as np
import pytest

import hsim_ref as H
from iv_interpolation_amd.engine import age_weights, weighted_settings  # noqa: F401  (without the feature the module fails here)
import weighted_cases as WC
import weighted_ref as WR

KEYS = WR.OUT_KEYS
ARGS = ("pnl", "scen_flags", "spot", "lag", "tail_probs", "min_scen", "weight", "vol_span", "vol_weight", "min_returns", "scale_cap")


def same_bits(a, b, keys, what):
    for k in keys:
        if a[k] is None and b[k] is None:
            continue
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), (k, what)
        if x.dtype.kind == "f":
            assert np.array_equal(np.signbit(np.nan_to_num(x)), np.signbit(np.nan_to_num(y))), (k, what)


def run(t, **over):
    t = {**t, **over}
    return WR.weighted(*[t[k] for k in ARGS], **{k: t[k] for k in ("stages", "sigma") if k in t})


_cache = {}


def case(name):
    if name not in _cache:
        c = WC.TABLES[name] if name in WC.TABLES else WC.make(name)
        _cache[name] = (c, run(c))
    return _cache[name]


# ------------------------------------------------------------------ the tables
@pytest.mark.parametrize("name", sorted(WC.TABLES))
def test_tables_by_hand(name):
    t, r = case(name)
    WC.check_want(name, t, r)
    w = np.ones(t["pnl"].shape[1]) if t["weight"] is None else t["weight"]
    for p in range(t["pnl"].shape[0]):                       # W7 as the rule reads, one rank at a time
        if not r["active"][p]:
            assert np.isnan(r["var_w"][p]).all() and np.isnan(r["es_w"][p]).all()
            continue
        idx = np.flatnonzero(r["ranked"][p])
        order = idx[np.argsort(r["pnl_w"][p, idx], kind="stable")]
        for l, tp in enumerate(t["tail_probs"]):
            var, es, reached = WR.walk(r["pnl_w"][p, order], w[order], tp, r["wsum"][p])
            assert reached and var.tobytes() == r["var_w"][p, l].tobytes() and es.tobytes() == r["es_w"][p, l].tobytes(), (name, p, l)


def test_zero_signs_and_exact_scales():
    t, r = case("zeros")
    assert not np.signbit(r["var_w"]).any() and not np.signbit(r["es_w"]).any()
    assert np.signbit(r["pnl_w"][0]).tolist() == [True, False, True, False, False, False]
    t, r = case("grow7")
    keep = r["ranked"]
    assert keep.sum() == 18 and r["pnl_w"][keep].tobytes() == t["pnl"][keep].tobytes()       # f = 1.0: pnl's bits
    t, r = case("steps")
    assert set(r["scale"][np.isfinite(r["scale"])].tolist()) == {0.5, 1.0, 2.0}
    t, r = case("steps_cap")
    assert set(r["scale"][np.isfinite(r["scale"])].tolist()) == {1.0 / 1.5, 1.0, 1.5}


def test_walk_without_a_rank_that_reaches_the_target():
    """W7's last resort, which rounding alone can cause: rho* = n - 1, whose w z was added once, and the remainder of the target on top."""
    z, w = np.array([-3.0, -1.0, 2.0]), np.array([1.0, 1.0, 1.0])
    var, es, reached = WR.walk(z, w, 0.5, 8.0)               # a W that the weights do not add up to: target 4 > 3
    assert not reached and var == -2.0 and es == -((-3.0 - 1.0 + 2.0) + (4.0 - 3.0) * 2.0) / 4.0
    assert WR._tail(z, w, 0.5, 8.0) == (var, es, False)


# ------------------------------------------------------------------ consequences of the rules
@pytest.mark.parametrize("name", sorted(WC.CASES))
def test_generated_cases_meet_their_conditions(name):
    c, r = case(name)
    assert r["reached"][r["active"]].all(), "a row runs out of ranks before its target"
    assert max(c["tail_probs"], default=0.0) <= 0.5
    w = np.ones(c["pnl"].shape[1]) if c["weight"] is None else c["weight"]
    for p in np.flatnonzero(r["active"]):                    # the one-rank-at-a-time reading agrees
        idx = np.flatnonzero(r["ranked"][p])
        order = idx[np.argsort(r["pnl_w"][p, idx], kind="stable")]
        for l, tp in enumerate(c["tail_probs"]):
            var, es, _ = WR.walk(r["pnl_w"][p, order], w[order], tp, r["wsum"][p])
            assert var.tobytes() == r["var_w"][p, l].tobytes() and es.tobytes() == r["es_w"][p, l].tobytes(), (name, p, l)
    if c["vol_span"] > 0 and c["min_returns"] == 1:
        B, window = c["pnl"].shape
        j = np.arange(B)[:, None] - c["lag"] - np.arange(window)[None, :]
        no_vol = (r["flags_w"] & WR.NO_VOL) != 0
        assert np.isfinite(r["sigma"][1:]).all() and np.isnan(r["sigma"][0])
        rows = np.arange(B)[:, None] >= 1
        assert np.array_equal(no_vol & (j >= 0) & rows, (j == 0) & rows)     # the scenario that starts at snapshot 0 has no vol behind it
        assert no_vol[j < 0].all() and no_vol[0].all()
    if name == "w1024_zero":
        assert (c["weight"][r["ranked"][0]] == 0.0).sum() > 400
    if name == "w1024":
        assert c["weight"][-1] == 2.0 ** -1023 and (c["weight"] > 0).all()


def test_some_case_is_active_at_every_size():
    active = {name: case(name)[1]["active"] for name in WC.CASES}
    assert all(active[n].any() for n in ("w1", "w63", "w64", "w65", "w256", "w1024", "w1024_vol"))
    assert not active["w1024_zero"].any() and not active["w64"].all()


@pytest.mark.parametrize("n,tps", [(200, (0.5, 0.25, 0.05, 0.01)), (8, (0.25, 0.5)), (64, (0.25, 0.125))])
def test_unit_weights_with_an_integer_tail_are_h7_to_the_bit(n, tps):
    r = np.random.default_rng(24)
    pnl = r.standard_t(4, (5, n))
    fl = np.zeros((5, n), np.int32)
    for tp in tps:
        assert np.float64(n) * np.float64(tp) == round(n * tp)
    var, es, n_valid, worst = H.tail(pnl, fl, tps, 1)
    got = WR.weighted(pnl, fl, tail_probs=tps, min_scen=1)
    same_bits(got, dict(var_w=var, es_w=es, n_valid_w=n_valid, worst_w=worst), ("var_w", "es_w", "n_valid_w", "worst_w"), n)
    same_bits(got, WR.weighted(pnl, fl, tail_probs=tps, min_scen=1, weight=WR.age_weights(n, 1.0)), WR.TAIL_KEYS, "decay 1.0")


def test_a_row_times_two_gives_twice_the_figures():
    c, r = case("w256")
    twice = run(c, pnl=c["pnl"] * 2.0)
    same_bits(twice, dict(var_w=r["var_w"] * 2.0, es_w=r["es_w"] * 2.0), ("var_w", "es_w"), "x 2")
    same_bits(twice, r, ("n_valid_w", "worst_w", "wsum", "n_eff", "flags_w"), "x 2")
    c, r = case("w64")                                       # and through the scaling: f is the same, z doubles
    twice = run(c, pnl=c["pnl"] * 2.0)
    same_bits(twice, dict(var_w=r["var_w"] * 2.0, es_w=r["es_w"] * 2.0, scale=r["scale"]), ("var_w", "es_w", "scale"), "x 2, scaled")


def test_decay_one_is_no_weight():
    from iv_interpolation_amd import engine
    c, r = case("w65")
    assert c["weight"] is None
    w = engine.age_weights(65, 1.0)
    assert w.dtype == np.float64 and (w == 1.0).all()
    same_bits(run(c, weight=w), r, KEYS, "decay 1.0")
    for decay in (0.99, 0.94, 0.5):
        assert engine.age_weights(300, decay).tobytes() == WR.age_weights(300, decay).tobytes() == WC.age_weights(300, decay).tobytes()
    assert engine.age_weights(3, 0.5).tolist() == [1.0, 0.5, 0.25]
    for bad in (0.0, 1.5, -0.1, float("nan")):
        with pytest.raises(ValueError):
            engine.age_weights(8, bad)
    with pytest.raises(ValueError):
        engine.age_weights(0, 0.9)


def test_a_row_alone_and_a_level_alone():
    c, r = case("w256")                                      # M = 0: the row is all a row's outputs depend on
    for p in (0, 37, 69):
        one = run(c, pnl=c["pnl"][p:p + 1], scen_flags=c["scen_flags"][p:p + 1])
        same_bits({k: one[k][0] for k in WR.TAIL_KEYS}, {k: r[k][p] for k in WR.TAIL_KEYS}, WR.TAIL_KEYS, ("alone", p))
    lone = run(c, tail_probs=c["tail_probs"][1:])
    same_bits(lone, dict(var_w=r["var_w"][:, 1:], es_w=r["es_w"][:, 1:]), ("var_w", "es_w"), "one level of two")
    c, r = case("w64")                                       # M = 64: stage 2 on the sigmas of stage 1 is stage 0
    sig = run(c, stages=1)
    assert set(sig) == {"sigma"}
    same_bits(run(c, stages=2, sigma=sig["sigma"]), r, KEYS, "stages 1 then 2")


def test_rows_that_differ_only_under_a_flag_agree():
    t, r = case("flag_and_bit")
    keys = [k for k in WR.TAIL_KEYS if k != "pnl_w"]
    same_bits({k: r[k][0] for k in keys}, {k: r[k][1] for k in keys}, keys, "garbage under a flag")
    assert np.isnan(r["pnl_w"][:, 1]).all()


def test_recent_turbulence_raises_the_weighted_var():
    """A direction, not a band: a row whose recent half is its old half times 3; at decay 0.94 the recent half carries nearly all the mass,
    so the weighted VaR lies above the plain one."""
    r = np.random.default_rng(2424)
    old = r.standard_t(4, 128)
    pnl = np.concatenate([old * 3.0, old])[None, :]          # age 0..127: the recent, violent half
    fl = np.zeros(pnl.shape, np.int32)
    plain = H.tail(pnl, fl, (0.05, 0.01), 20)[0]
    got = WR.weighted(pnl, fl, weight=WR.age_weights(256, 0.94))
    assert (got["var_w"] > plain).all() and got["n_eff"][0] < 40


# ------------------------------------------------------------------ host checks and C refusals
def test_weighted_settings():
    from iv_interpolation_amd import engine
    assert engine.weighted_settings(256, 1, (0.05, 0.01), 20) == (256, 1, [0.05, 0.01], 20, 0, 20, 3.0, 0)
    assert engine.weighted_settings(256, 2, (0.05,), 20, 64, 20, 2, 2) == (256, 2, [0.05], 20, 64, 20, 2.0, 2)
    assert engine.weighted_settings(8, 1, (), 1, 0, 99, 0.5)[4] == 0     # without scaling min_returns and scale_cap are not read
    for bad in (dict(window=0), dict(window=1025), dict(lag=0), dict(tail_probs=(1.0,)), dict(tail_probs=(0.1,) * 9), dict(min_scen=0),
                dict(vol_span=-1), dict(vol_span=1025), dict(vol_span=1.5), dict(vol_span=8, min_returns=0), dict(vol_span=8, min_returns=9),
                dict(vol_span=8, min_returns=2, scale_cap=0.99), dict(vol_span=8, min_returns=2, scale_cap=math.inf),
                dict(vol_span=8, min_returns=2, scale_cap=math.nan), dict(stages=3), dict(stages=-1)):
        kw = dict(window=256, lag=1, tail_probs=(0.05,), min_scen=20, vol_span=0, min_returns=20, scale_cap=3.0, stages=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            engine.weighted_settings(**kw)


def _dbl(*xs):
    a = (ctypes.c_double * max(len(xs), 1))(*xs)
    return ctypes.cast(a, ctypes.POINTER(ctypes.c_double))


def _args(**over):
    """A call that passes every check but names buffers that do not exist: it must be refused before any of them is touched."""
    from iv_interpolation_amd import _lib
    a = _lib.WeightedArgs()
    for k, t in _lib.WeightedArgs._fields_:
        if t is ctypes.c_void_p:
            setattr(a, k, 0x1000)
    a.tail_probs, a.nL = _dbl(0.05, 0.01), 2
    a.B, a.window, a.lag, a.min_scen, a.vol_span, a.min_returns, a.scale_cap, a.stages = 100, 256, 1, 20, 64, 20, 3.0, 0
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_c_refusals_touch_nothing():
    from iv_interpolation_amd import _lib
    lib = _lib.load()                                        # a library that is missing or lacks the entry point fails here
    EINVAL, ERANGE = -22, -34
    assert lib.ivs_version() == 5 and (_lib.HW_NO_VOL, _lib.HW_BAD_WEIGHT, _lib.HW_MAX_SPAN) == (8, 16, 1024)
    assert lib.ivs_hsim_weighted_f64(None, None, 0, None) == EINVAL
    table = [(EINVAL, dict(B=-1)), (EINVAL, dict(nL=-1)), (ERANGE, dict(window=0)), (ERANGE, dict(window=1025)), (ERANGE, dict(lag=0)), (ERANGE, dict(nL=9)),
             (EINVAL, dict(tail_probs=None)), (ERANGE, dict(tail_probs=_dbl(0.05, 1.0))), (ERANGE, dict(tail_probs=_dbl(float("nan"), 0.5))),
             (ERANGE, dict(min_scen=0)), (ERANGE, dict(vol_span=-1)), (ERANGE, dict(vol_span=1025)), (ERANGE, dict(min_returns=0)),
             (ERANGE, dict(min_returns=65)), (ERANGE, dict(scale_cap=0.5)), (ERANGE, dict(scale_cap=float("inf"))), (ERANGE, dict(scale_cap=float("nan"))),
             (ERANGE, dict(stages=3)), (ERANGE, dict(stages=-1)), (ERANGE, dict(B=2 ** 31 // 256 + 1)),
             (EINVAL, dict(pnl=None)), (EINVAL, dict(scen_flags=None)), (EINVAL, dict(flags_w=None)), (EINVAL, dict(n_valid_w=None)), (EINVAL, dict(worst_w=None)),
             (EINVAL, dict(wsum=None)), (EINVAL, dict(n_eff=None)), (EINVAL, dict(var_w=None)), (EINVAL, dict(es_w=None)), (EINVAL, dict(sigma=None)),
             (EINVAL, dict(spot=None)), (EINVAL, dict(vol_weight=None)), (EINVAL, dict(stages=2, sigma=None)), (EINVAL, dict(stages=1, spot=None)),
             (EINVAL, dict(stages=1, sigma=None))]
    for want, over in table:
        a = _args(**over)
        rc = lib.ivs_hsim_weighted_f64(ctypes.byref(a), None, 0, None)
        assert rc == want, (over, rc, lib.ivs_last_error())
        assert lib.ivs_last_error() and lib.ivs_last_kernel() == b""
    # the limits come before the zero-size return, and an empty call is a no-op on buffers that do not exist
    assert lib.ivs_hsim_weighted_f64(ctypes.byref(_args(B=0)), None, 0, None) == 0
    assert lib.ivs_hsim_weighted_f64(ctypes.byref(_args(B=0, pnl=None, sigma=None)), None, 0, None) == 0
    assert lib.ivs_hsim_weighted_f64(ctypes.byref(_args(B=0, vol_span=1025)), None, 0, None) == ERANGE
    assert lib.ivs_hsim_weighted_f64(ctypes.byref(_args(B=0, vol_span=0, min_returns=0, scale_cap=0.0)), None, 0, None) == 0       # not read without scaling
    assert lib.ivs_hsim_weighted_f64(ctypes.byref(_args(vol_span=0, stages=1, pnl=None, sigma=None)), None, 0, None) == 0        # nothing to do
    assert lib.ivs_last_kernel() == b""


# ------------------------------------------------------------------ host layers with the restatement as the backend
LAG = 2
KW = dict(rate=0.01, lag=LAG, window=8, tail_probs=(0.5, 0.25), min_scenarios=1)


def _built():
    """A minute chain: the running vol needs the spot of consecutive snapshots (on an hourly chain the snapshots between two quotes
    have no spot, so no return is valid and every scenario is NO_VOL: test_varw_task_end_to_end has that)."""
    import pandas as pd
    import snapshot_cases as SNC
    from iv_interpolation_amd.snapshots import SnapshotSurfaceBuilder
    b = SnapshotSurfaceBuilder(backend=WR.RefBackend(), moneyness=np.linspace(0.8, 1.2, 12), tenors=np.array([10.0, 20.0, 30.0]) / 365)
    res = b.build(SNC.big_chain(n_und=1, nT=5, nK=12, minutes=24, unlisted=0.0))
    svi = b.svi(res, rate=0.01, rounds=6)
    t0 = res[0].dates[0]
    bk = pd.DataFrame({"symbol": list("abc"), "strike": [22000.0, 25000.0, 28000.0], "expiry": [t0 + pd.Timedelta(days=d) for d in (12.0, 18.0, 25.0)],
                       "callput": ["c", "P", "call"], "quantity": [2.0, -1.0, 0.5]})
    return b, res, svi, bk


def test_builder_report_and_frame():
    from iv_interpolation_amd.snapshots import WeightedVarReport, weighted_var_frame
    b, res, svi, bk = _built()
    var = b.var(res, bk, svi, **KW)
    reps = b.var_weighted(res, var, decay=0.9, vol_span=6, vol_decay=0.9, min_returns=3, scale_cap=2.0)
    assert len(reps) == 1 and isinstance(reps[0], WeightedVarReport)
    p, h = reps[0], var[0]
    assert (p.decay, p.vol_span, p.vol_decay, p.min_returns, p.scale_cap, p.lag, p.window) == (0.9, 6, 0.9, 3, 2.0, LAG, 8) and p.var is h.var
    ref = WR.weighted(h.pnl, h.scen_flags, np.asarray(res[0].spot), LAG, (0.5, 0.25), 1, WR.age_weights(8, 0.9), 6, WR.age_weights(6, 0.9), 3, 2.0)
    for k in KEYS:
        assert np.array_equal(getattr(p, k), ref[k], equal_nan=True), k
    assert np.isfinite(p.var_w).sum() >= 20 and np.isfinite(p.sigma).sum() >= 20 and (np.asarray(p.scale)[np.isfinite(p.scale)] != 1.0).any()
    plain = b.var_weighted(res, var, decay=1.0)[0]           # the defaults but for the decay: no scaling, unit weights
    assert plain.sigma is None and plain.vol_span == 0
    assert np.array_equal(plain.n_valid_w, h.n_valid) and np.array_equal(plain.worst_w, h.worst) and np.array_equal(plain.pnl_w, h.pnl, equal_nan=True)
    r = res[0]
    keep = np.flatnonzero(np.asarray(r.quotes) > 0)
    f = weighted_var_frame(reps, res)
    assert list(f.columns) == ["underlying", "date", "n_valid", "n_eff", "sigma"] + [f"{s}_{tp}" for tp in ("0.5", "0.25") for s in ("var", "es", "varw", "esw")]
    assert len(f) == len(keep) and (f["date"] == r.dates[keep]).all() and (f["n_valid"] == ref["n_valid_w"][keep]).all()
    assert np.array_equal(f["var_0.5"], np.asarray(h.var)[keep, 0], equal_nan=True) and np.array_equal(f["esw_0.25"], ref["es_w"][keep, 1], equal_nan=True)
    assert np.array_equal(f["varw_0.5"], ref["var_w"][keep, 0], equal_nan=True) and np.array_equal(f["sigma"], ref["sigma"][keep], equal_nan=True)
    assert np.isnan(weighted_var_frame([plain], res)["sigma"]).all() and len(weighted_var_frame([], [])) == 0
    for kw in (dict(decay=0.0), dict(decay=1.5), dict(vol_span=-1), dict(vol_span=2000), dict(vol_span=8, min_returns=9), dict(vol_span=8, min_returns=2, scale_cap=0.5),
               dict(vol_span=8, min_returns=2, vol_decay=0.0)):
        with pytest.raises(ValueError):
            b.var_weighted(res, var, **kw)


def test_kupiec_by_hand():
    import complete_pipeline as cp
    # N = 100, x = 5, tp = 0.05: the observed rate is the level: LR = 0
    assert cp.kupiec_lr(100, 5, 0.05) == pytest.approx(0.0, abs=1e-12)
    # N = 100, x = 10, tp = 0.05: -2 [90 ln 0.95 + 10 ln 0.05 - 90 ln 0.9 - 10 ln 0.1] = -2 [90 ln(0.95 / 0.9) + 10 ln 0.5] = 4.13077...
    assert cp.kupiec_lr(100, 10, 0.05) == pytest.approx(-2.0 * (90.0 * math.log(0.95 / 0.9) + 10.0 * math.log(0.5)), rel=1e-12)
    assert cp.kupiec_lr(100, 10, 0.05) == pytest.approx(4.1308, abs=1e-3) and cp.kupiec_lr(100, 10, 0.05) > 3.84     # beyond chi2_1's 5 % point
    # 0 ln 0 = 0: x = 0 gives -2 N ln(1 - tp), x = N gives -2 N ln tp
    assert cp.kupiec_lr(50, 0, 0.01) == pytest.approx(-2.0 * 50.0 * math.log(0.99), rel=1e-12)
    assert cp.kupiec_lr(4, 4, 0.25) == pytest.approx(-2.0 * 4.0 * math.log(0.25), rel=1e-12)
    assert math.isnan(cp.kupiec_lr(0, 0, 0.05))


def test_varw_task_end_to_end(tmp_path):
    import complete_pipeline as cp
    from iv_interpolation_amd.frame_store import FrameStore, synthetic_chain
    store = FrameStore(str(tmp_path))
    chain = synthetic_chain("btc", expiry_days=(20, 45), strikes=tuple(np.linspace(17000.0, 34000.0, 6)), n_hours=4, seed=5)
    for f in chain:
        store.write_output(f["symbol"].iloc[0], f, 1)
    argv = ["--task", "varw", "--decay", "0.97", "--lag", "60", "--window", "121",
            "--levels", "0.5,0.25", "--min-scenarios", "1", "--data-dir", str(tmp_path)]
    assert cp.main(argv, surface_backend=WR.RefBackend()) == 0
    out, var = store.read_table("iv_var_w", "btc"), store.read_table("iv_var", "btc")
    assert list(out.columns)[:5] == ["underlying", "date", "n_valid", "n_eff", "sigma"] and len(out) == len(var) > 0
    assert np.array_equal(out["var_0.5"], var["var_0.5"], equal_nan=True) and np.array_equal(out["es_0.25"], var["es_0.25"], equal_nan=True)
    assert np.isfinite(out["varw_0.5"]).any() and np.isnan(out["sigma"]).all()
    pipe = cp.CompleteOptimizedPipeline(cp.get_config(), data_dir=str(tmp_path), surface_backend=WR.RefBackend())
    kw = dict(lag=60, window=121, levels=(0.5, 0.25), min_scenarios=1)
    plain = pipe.run_var(**kw)
    res = pipe.run_varw(decay=0.97, **kw)
    assert res["success"] and res["w_rows"] == len(out) and set(res) == set(plain) | {"w_rows", "backtest_w", "kupiec"}
    for k in plain:                                          # run_var's keys, equal to a plain run_var's
        if k != "duration":
            assert res[k] == plain[k] or (k == "backtest" and str(res[k]) == str(plain[k])), k
    assert [b["tp"] for b in res["backtest_w"]] == [0.5, 0.25] and all(set(b) == {"tp", "eligible", "exceedances", "exceedance_rate"} for b in res["backtest_w"])
    assert all(0 <= b["exceedances"] <= b["eligible"] for b in res["backtest_w"]) and any(b["eligible"] > 0 for b in res["backtest_w"])
    for k, plain_b, w_b in zip(res["kupiec"], res["backtest"], res["backtest_w"]):
        assert set(k) == {"tp", "plain", "weighted"}
        for got, b in ((k["plain"], plain_b), (k["weighted"], w_b)):
            want = cp.kupiec_lr(b["eligible"], b["exceedances"], b["tp"])
            assert (math.isnan(got) and math.isnan(want)) or got == want
    assert np.array_equal(store.read_table("iv_var_w", "btc")["varw_0.5"], out["varw_0.5"], equal_nan=True)
    assert np.array_equal(out["n_valid"], var["n_valid"])   # no scaling: the ranked set is the plain one
    hourly = pipe.run_varw(decay=0.97, vol_span=8, vol_decay=0.9, scale_cap=2.0, **kw)       # (min_returns: min(20, 8)) an hourly chain on the minute grid: no two
    again = store.read_table("iv_var_w", "btc")                                             # consecutive spots, no return, no vol
    assert hourly["success"] and np.isnan(again["sigma"]).all() and (again["n_valid"] == 0).all() and np.isnan(again["varw_0.5"]).all()
    assert all(b["eligible"] == 0 for b in hourly["backtest_w"]) and all(math.isnan(k["weighted"]) for k in hourly["kupiec"])
    assert "decay" in pipe.run_varw(decay=0.0)["error"] and "vol_span" in pipe.run_varw(vol_span=-1)["error"]
    assert "scale_cap" in pipe.run_varw(vol_span=30, scale_cap=0.5)["error"] and "window" in pipe.run_varw(window=0)["error"]
