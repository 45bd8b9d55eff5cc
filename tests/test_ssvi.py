"""CPU: the restatement of the SSVI rules J1-J8 (tests/ssvi_ref.py) against the rules' own consequences: the hand-built micro
cases, its sensitivity to one unit in the last place of the input (R_CPU, the unit of error of the GPU tests), the recovery of
noiseless surfaces, the quality of the search against a bounded least-squares solver, the raw-SVI identity and freedom from
calendar and butterfly arbitrage through the project's own checks (tests/cal_ref.py).

Every test prints its figures; with IVS_SSVI_ERRLOG=<file> set they are appended to that file (a recorded run belongs in
profiles/ssvi/errlog.txt)."""
import os

import numpy as np
import pytest

import cal_ref
import ssvi_cases as C
import ssvi_ref as R

ROUNDS = (20, 4)


def log(name, **figures):
    line = name + ": " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items())
    print(line)
    path = os.environ.get("IVS_SSVI_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


_cache = {}


def generated(n):
    """Case, generator record and restatement (20 rounds, margins asserted) of SHAPES[n], computed once, read-only."""
    if n not in _cache:
        c, g = C.batch(**C.SHAPES[n])
        r = R.restate(**C.case_args(c), margins=C.SHAPES[n]["mT"] >= 2)
        for a in list(c.values()) + list(g.values()) + list(r.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[n] = (c, g, r)
    return _cache[n]


def inputs():
    for name in sorted(C.MICRO):
        yield "micro:" + name, C.MICRO[name]
    for n, s in enumerate(C.SHAPES):
        yield C.shape_id(s), generated(n)[0]


@pytest.mark.parametrize("name", sorted(C.MICRO))
def test_micro(name):
    c = C.MICRO[name]
    r = R.restate(**C.case_args(c))
    assert np.array_equal(r["flags"], c["flags"]), r["flags"]
    assert np.array_equal(r["sflags"] & ~c["sfree"], c["sflags"]), r["sflags"]
    dead = r["flags"] == C.DEAD
    for k in ("theta", "params", "fit", "fitted"):
        v = r[k].reshape(dead.shape + (-1,))
        assert np.isnan(v[dead]).all(), k
    assert np.isfinite(r["theta"][~dead]).all() and np.isfinite(r["params"][~dead]).all()
    sd = (r["sflags"] & (C.SURF_DEAD | C.UNORDERED)) != 0
    assert np.isnan(r["surface"][sd]).all() and np.isfinite(r["surface"][~sd]).all() and dead[sd].all()
    if name == "decreasing_theta0":
        assert np.array_equal(r["params"][0, 2], r["params"][0, 1]) and r["theta"][0, 2] == r["theta"][0, 1] == 0.05
    if name == "row_without_nodes":
        assert np.isnan(r["fit"][0, 1]).all() and np.isfinite(r["fit"][0, [0, 2]]).all() and np.isfinite(r["fitted"][0, 1]).all()
    if name == "raw_with_a_dead_slice":
        assert np.allclose(r["theta"][0, [0, 2]], C.TH3[[0, 2]], rtol=1e-14)
    if name == "at_the_bound":
        assert r["point"][0, 2] == 0.0


def test_twin_sensitivity():
    """R_CPU: the restatement against itself on vol x (1 + 2^-52 xi), over every input of the GPU tests."""
    for rounds in ROUNDS:
        worst = {k: 0.0 for k in C.R_CPU[rounds]}
        unstable = fitted = 0
        for name, c in inputs():
            ref = R.restate(**C.case_args(c), rounds=rounds)
            for seed in C.TWIN_SEEDS:
                tw = R.twin(c, seed, rounds)
                assert np.array_equal(tw["flags"] & ~C.BUTTERFLY, ref["flags"] & ~C.BUTTERFLY), name
                u = C.units(tw, ref)
                live = np.isfinite(u["steps"])
                bad = live & (u["steps"] > C.UNSTABLE_STEPS)
                unstable += int(bad.sum())
                fitted += int(live.sum())
                for k in worst:
                    v = u[k][live & ~bad]
                    if len(v):
                        worst[k] = max(worst[k], float(np.max(v)))
        log(f"twin[rounds={rounds}]", **worst, unstable=unstable, fitted=fitted)
        assert unstable == 0, "the generated inputs must have no unstable snapshot in the restatement alone"
        for k, v in worst.items():
            assert v <= C.R_CPU[rounds][k], (rounds, k, v)


def test_recovery_of_noiseless_surfaces():
    worst, rm = np.zeros(3), 0.0
    for n, s in enumerate(C.SHAPES):
        c, g, r = generated(n)
        ex = g["exact"] & r["identified"]
        if ex.any():
            worst = np.maximum(worst, np.abs(r["point"][ex] - g["point"][ex]).max(axis=0))
            rm = max(rm, float(r["surface"][ex, 3].max()))
    log("recovery", rho=float(worst[0]), gamma=float(worst[1]), s=float(worst[2]), rmse=rm)
    assert (worst <= C.RECOVERY["point"]).all() and rm <= C.RECOVERY["rmse"]


def _nodes(c, r, b):
    """theta, row index, x, w of snapshot b as rule J2 lays them out."""
    K = np.broadcast_to(c["Kq"], (c["vol"].shape[0], c["vol"].shape[2]))[b]
    T = np.broadcast_to(c["Tq"], c["vol"].shape[:2])[b]
    rows = np.flatnonzero(r["flags"][b] != C.DEAD)
    xs, ws, rw = [], [], []
    for l, j in enumerate(rows):
        v = c["vol"][b, j]
        with np.errstate(all="ignore"):
            i = np.flatnonzero(np.isfinite(v) & (v > 0) & np.isfinite(K) & (K > 0))
        xs.append(np.log(K[i] / c["spot"][b]) - c["rate"] * T[j])
        ws.append(v[i] ** 2 * T[j])
        rw.append(np.full(len(i), l))
    return r["theta"][b][rows], np.concatenate(rw), np.concatenate(xs), np.concatenate(ws)


def test_quality_against_least_squares():
    """The same objective (theta fixed) through scipy.optimize.least_squares from several starts, the generating point
    among them: the SSE ratio is recorded, and bounded by what was measured."""
    from scipy.optimize import least_squares
    worst = 0.0
    for n in (2, 3):
        c, g, r = generated(n)
        for b in np.flatnonzero(~g["exact"]):
            th, row, x, w = _nodes(c, r, b)
            L, q, inv = np.log(th), np.sqrt(th), 1.0 / th

            def res(p):
                eta = np.exp(p[2]) * R.eta_max(p[0:1], p[1:2], th, L, q)[0]
                return (R.model(th[row], eta * np.exp(-p[1] * L[row]), p[0], x) - w) * inv[row]

            best = np.inf
            for start in (g["point"][b], r["point"][b], np.array([0.0, 0.5, -1.0]), np.array([-0.5, 0.3, -0.3])):
                s = least_squares(res, np.clip(start, R.DOM_LO, R.DOM_HI), bounds=(R.DOM_LO, R.DOM_HI), xtol=1e-15, ftol=1e-15, gtol=1e-15)
                best = min(best, 2.0 * s.cost)
            ratio = float(r["sse"][b] / best - 1.0)
            log(f"quality[{C.shape_id(C.SHAPES[n])}, b={b}]", sse=float(r["sse"][b]), sse_scipy=float(best), excess=ratio)
            worst = max(worst, ratio)
    log("quality", worst_excess=worst)
    assert worst <= C.QUALITY_MARGIN


def test_raw_form_identity():
    """w from `params` through T3 equals J4 to a few eps of the terms."""
    worst = 0.0
    for n in range(len(C.SHAPES)):
        c, g, r = generated(n)
        x = np.linspace(-1.5, 1.5, 41)
        P, su, th = r["params"], r["surface"], r["theta"]
        phi = su[:, 1, None] * th ** -su[:, 2, None]
        with np.errstate(all="ignore"):
            wj = R.model(th[..., None], phi[..., None], su[:, 0, None, None], x)
            cv = cal_ref.curve(P[:, :, None, :], x)
            u = np.abs(cv["w"] - wj) / (C.EPS * cv["sw"])
        assert np.array_equal(np.isnan(u[..., 0]), r["flags"] == C.DEAD)
        worst = max(worst, float(np.nanmax(u)))
    log("raw_form_identity", eps_of_the_terms=worst)
    assert worst <= 8.0


def test_arbitrage_freedom_through_the_projects_checks():
    """No CALENDAR, WING_LEFT or WING_RIGHT on any live pair (cal_ref.restate_calendar on the fitted params), g_min >= 0 on
    every live row; a RAISED row repeats its neighbour's bits (d = 0 exactly)."""
    pairs = raised = 0
    for n, s in enumerate(C.SHAPES):
        c, g, r = generated(n)
        cal = cal_ref.restate_calendar(r["params"], c["Tq"], c["spot"])
        bad = cal["flags"] & (cal_ref.CALENDAR | cal_ref.WING_LEFT | cal_ref.WING_RIGHT)
        assert not bad[cal["pair"]].any(), (C.shape_id(s), np.argwhere(bad & cal["pair"]))
        assert np.array_equal(cal["live"], r["flags"] != C.DEAD)
        assert not (cal["flags"] & cal_ref.UNORDERED).any()
        gm = r["fit"][..., 2]
        assert (gm[np.isfinite(gm)] >= 0).all() and not (r["flags"] & C.BUTTERFLY).any()
        for b, j in np.argwhere((r["flags"] != C.DEAD) & ((r["flags"] & C.RAISED) != 0)):
            prev = max(q for q in range(j) if r["flags"][b, q] != C.DEAD)
            assert np.array_equal(r["params"][b, j], r["params"][b, prev]) and cal["d_min"][b, prev] == 0.0
            raised += 1
        pairs += int(cal["pair"].sum())
    log("arbitrage_freedom", pairs=pairs, raised=raised)
    assert pairs > 200 and raised >= 4


# ------------------------------------------------------------------ host layers with the restatement as the backend
def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _built():
    from iv_interpolation_amd.snapshots import SnapshotSurfaceBuilder
    from iv_interpolation_amd.frame_store import synthetic_chain
    chain = synthetic_chain("btc", expiry_days=(0.5, 3), strikes=tuple(np.linspace(17000.0, 34000.0, 12)), n_hours=3, seed=5)
    b = SnapshotSurfaceBuilder(backend=R.RefBackend(), moneyness=np.linspace(0.72, 1.28, 24), tenors=np.array([1.0, 2.0, 2.8]) / 365)
    return b, b.build(chain)


def test_ssvi_report_frames_and_downstream_stages():
    from iv_interpolation_amd.snapshots import calendar_frame, ssvi_frame, ssvi_slices_frame
    b, res = _built()
    fits = b.svi(res, rate=0.01)
    reps = b.ssvi(res, fits, rate=0.01, rounds=6, fitted=True)
    assert len(reps) == len(res) == 1
    s, r = reps[0], res[0]
    assert s.underlying == "btc" and s.dates.equals(r.dates) and same(s.tenors, r.tenors) and s.rate == 0.01 and s.rounds == 6
    ref = R.restate(r.out, r.Kq, r.tenors, r.spot, 0.01, raw=fits[0].params, rounds=6)
    for k in ("surface", "theta", "params", "fit", "flags", "sflags", "fitted"):
        assert same(getattr(s, k), ref[k]), k
    own = b.ssvi(res, rate=0.01, rounds=6)[0]                                 # runs svi itself
    assert own.fitted is None and same(own.params, s.params)
    keep = np.flatnonzero(np.asarray(r.quotes) > 0)
    live = ref["flags"][keep] != R.DEAD
    assert len(keep) == 3 and live.any() and (np.delete(ref["sflags"], keep) & R.SURF_DEAD).all()

    f = ssvi_frame(reps, res)
    cols = ["underlying", "date", "spot", "rho", "eta", "gamma", "rmse", "live_rows", "raised_rows", "sflags"]
    assert list(f.columns) == cols and len(f) == 3 and list(f["date"]) == list(r.dates[keep])
    assert same(f["rho"].to_numpy(), ref["surface"][keep, 0]) and same(f["live_rows"].to_numpy(), live.sum(axis=1))
    assert same(f["raised_rows"].to_numpy(), (live & (ref["flags"][keep] & R.RAISED != 0)).sum(axis=1))
    assert same(f["sflags"].to_numpy(), ref["sflags"][keep])
    g = ssvi_slices_frame(reps, res)
    cols2 = ["underlying", "date", "spot", "tenor", "theta", "a", "b", "rho", "m", "sigma", "rmse_vol", "max_vol_err", "g_min", "flags"]
    assert list(g.columns) == cols2 and len(g) == int(live.sum())
    assert same(g["theta"].to_numpy(), ref["theta"][keep][live]) and same(g["sigma"].to_numpy(), ref["params"][keep][live][:, 4])
    assert same(g["g_min"].to_numpy(), ref["fit"][keep][live][:, 2]) and same(g["flags"].to_numpy(), ref["flags"][keep][live])
    assert list(ssvi_frame([], []).columns) == cols and list(ssvi_slices_frame([], []).columns) == cols2

    # an SsviReport goes wherever an SviReport does
    cal = b.calendar(res, reps)
    cf = np.asarray(cal[0].flags)[keep]
    assert not (cf & (cal_ref.CALENDAR | cal_ref.WING_LEFT | cal_ref.WING_RIGHT | cal_ref.UNORDERED)).any()
    assert same(cf == cal_ref.DEAD, ~live) and len(calendar_frame(cal, res)) == int(live.sum()) - 3
    assert np.asarray(b.distribution(res, reps, rate=0.01)[0].q_strike).shape[:2] == ref["flags"].shape
    for bad in (-1, 33, 2.5):
        with pytest.raises(ValueError, match="rounds"):
            b.ssvi(res, rounds=bad)


def test_ssvi_task_end_to_end(tmp_path):
    import complete_pipeline as cp
    from iv_interpolation_amd.frame_store import FrameStore
    from iv_interpolation_amd.frame_store import synthetic_chain
    store = FrameStore(str(tmp_path))
    for f in synthetic_chain("btc", expiry_days=(20, 45), strikes=tuple(np.linspace(17000.0, 34000.0, 6)), n_hours=3, seed=5):
        store.write_output(f["symbol"].iloc[0], f, 1)
    assert cp.main(["--task", "ssvi", "--data-dir", str(tmp_path)], surface_backend=R.RefBackend()) == 0
    assert store.read_table("iv_svi", "btc") is None and store.read_table("iv_calendar", "btc") is None
    out = store.read_table("iv_ssvi", "btc")
    assert list(out.columns) == ["underlying", "date", "spot", "tenor", "theta", "a", "b", "rho", "m", "sigma", "rmse_vol", "max_vol_err",
                                 "g_min", "flags", "eta", "gamma", "rmse", "sflags"]
    assert len(out) and (out["flags"] & R.DEAD == 0).all() and out["gamma"].between(0, 1).all()
    assert (out.groupby("date")["theta"].apply(lambda t: (np.diff(t.to_numpy()) >= 0).all())).all()
    pipe = cp.CompleteOptimizedPipeline(cp.get_config(), data_dir=str(tmp_path), surface_backend=R.RefBackend())
    res = pipe.run_ssvi()
    assert res["success"] and res["underlyings"] == 1 and res["rows"] == len(out) and res["ssvi_surfaces"] == out["date"].nunique()
    assert res["raised_rows"] == int((out["flags"] & R.RAISED != 0).sum())
    assert set(res) == set(pipe.run_svi()) | {"ssvi_surfaces", "raised_rows"}


# ------------------------------------------------------------------ C ABI validation, no device needed
def test_abi_validation_needs_no_gpu():
    import ctypes
    from iv_interpolation_amd import _lib
    lib = _lib.load()

    def call(**kw):
        a = _lib.SsviArgs()
        for k in ("vol", "Kq", "Tq", "spot", "raw", "surface", "theta", "params", "fit", "flags", "sflags"):
            setattr(a, k, 64)                                                 # fake non-null pointers: never dereferenced
        a.mK, a.mT, a.B = 64, 16, 1
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.ivs_ssvi_surface_f64(ctypes.byref(a), None, 0, None)

    assert lib.ivs_ssvi_surface_f64(None, None, 0, None) == -22
    assert call(theta0=64) == -22 and b"exactly one" in lib.ivs_last_error() and call(raw=None) == -22
    assert call(B=-1) == -22 and call(kq_stride=-1) == -22 and call(kq_stride=5) == -22 and call(tq_stride=15) == -22
    for k in ("vol", "Kq", "Tq", "spot", "surface", "theta", "params", "fit", "flags", "sflags"):
        assert call(**{k: None}) == -22 and b"null pointer" in lib.ivs_last_error(), k
    assert call(mT=65, mK=1) == -34 and call(mK=0) == -34 and call(mT=64, mK=49) == -34 and b"LDS" in lib.ivs_last_error()
    assert call(rounds=33) == -34 and call(rounds=-1) == -34 and call(B=(1 << 31) // 1024 + 1) == -34
    assert call(B=0) == 0 and call(mT=0) == 0 and call(B=0, vol=None) == 0
