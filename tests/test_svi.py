"""CPU: raw SVI slices with a butterfly check (rules V1-V9).  The restatement (tests/svi_ref.py) is
checked on one hand-built micro case per rule and flag, its inner solve against brute force, its recovery of noiseless rows
and its quality against scipy's least squares on noisy ones; its sensitivity to one unit in the last place of the input (the
twin runs) is held below the recorded R_CPU the GPU tests build on; the host layers (builder, frame, pipeline task) run with
the restatement injected as their backend; the C ABI's argument validation runs without a device.  The kernel itself is
checked in test_svi_gpu.py.

Every measuring test prints its figures; with IVS_SV_ERRLOG=<file> set they are appended to that file as well (a recorded run
belongs in profiles/svi/errlog.txt)."""
import ctypes as C
import os

import numpy as np
import pytest

import svi_cases as SC
import svi_ref as R
from iv_interpolation_amd import _lib, synth
from iv_interpolation_amd.frame_store import FrameStore, synthetic_chain
from iv_interpolation_amd.snapshots import SnapshotSurfaceBuilder, svi_frame

M, TQ = synth.query_grids(64, 16)


def log(name, **figures):
    line = name + ": " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items())
    print(line)
    path = os.environ.get("IVS_SV_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def restate(c, **kw):
    return R.restate(c["vol"], c["Kq"], c["Tq"], c["spot"], c["rate"], **kw)


# ------------------------------------------------------------------ one case per rule and flag
@pytest.mark.parametrize("name", sorted(SC.MICRO))
def test_micro_case(name):
    c = SC.MICRO[name]
    r = restate(c)
    assert r["flags"].dtype == np.int32 and same(r["flags"] & ~c["free"], c["flags"]), r["flags"]
    dead = c["flags"] == R.DEAD
    for k in ("params", "fit", "fitted"):
        assert same(np.isnan(r[k]).all(axis=-1), dead), k                     # V1: NaN in every value of a DEAD row
    assert not np.isnan(r["params"][~dead]).any() and not np.isnan(r["fit"][~dead]).any()
    kpos = np.broadcast_to((np.isfinite(c["Kq"]) & (c["Kq"] > 0)).reshape(-1, 1, c["vol"].shape[2]), c["vol"].shape)
    assert same(np.isnan(r["fitted"]), dead[:, :, None] | ~kpos)               # V8: every node with a strike, holes filled


def test_micro_case_values():
    """What the hand-built rows are about, beyond their flags."""
    r = restate(SC.MICRO["a_hole"])
    assert np.abs(r["params"][0, 0] - SC.P9).max() < SC.RECOVERY["params"]                # the 8 other nodes carry the curve
    assert abs(r["fitted"][0, 0, 3] - SC._SVI9[0, 3]) < SC.RECOVERY["vol"]                 # ... and the hole is filled
    r = restate(SC.MICRO["five_nodes"])
    assert np.abs(r["fitted"][0, 0] - SC._SVI9[0]).max() < 1e-6 and r["n"][0, 0] == 5
    r = restate(SC.MICRO["straight_line_skew"])
    a, b, rho, m, sig = r["params"][0, 0]
    assert rho == -1.0 and m == SC.X9[-1] and abs(np.log(sig) - np.log((SC.X9[-1] - SC.X9[0]) / 256.0)) < 1e-15
    assert r["fit"][0, 0, 2] < 5e-4                                                      # a line, to half a vol point per mille
    r = restate(SC.MICRO["flat_row"])
    a, b, rho, m, sig = r["params"][0, 0]
    assert (a, b, rho, m) == (0.0625, 0.0, 0.0, SC.X9[0]) and r["fit"][0, 0, 0] == 0.0 and r["fit"][0, 0, 3] == 1.0
    assert r["u"][0, 0] == np.log((SC.X9[-1] - SC.X9[0]) / 256.0) and sig == np.exp(r["u"][0, 0])   # the lower sigma border itself
    r = restate(SC.MICRO["v_shape"])
    assert r["fit"][0, 0, 3] < -0.1 and abs(r["params"][0, 0, 3]) < 1e-6                   # the kink sits at x = 0


def test_rounds_argument():
    c = SC.MICRO["a_hole"]
    r16, r0, r4 = restate(c, rounds=16), restate(c, rounds=0), restate(c, rounds=4)
    assert same(r16["params"], r0["params"])                                             # 0 = the default 16
    assert np.allclose(r4["step"] / r4["width"], (2.0 / 7.0) ** 3 / 7.0, rtol=1e-12)       # V5: a round shrinks the box to 2/7
    assert np.abs(r4["params"][0, 0] - SC.P9).max() > np.abs(r16["params"][0, 0] - SC.P9).max()


# ------------------------------------------------------------------ V4 against brute force
def test_inner_solve_against_brute_force():
    """For each of the 27 sets the direct-residual SSE ranks as the excess E does (SSE = SSE_unconstrained + E), the
    solution satisfies its active constraints exactly, and the winner is the feasible set of the smallest SSE: no feasible
    point of a fine sampling of the prism does better."""
    rng = np.random.default_rng(5)
    x = np.linspace(-0.3, 0.3, 9)
    for trial in range(6):
        w = 0.02 + 0.05 * rng.random() * np.abs(x - 0.1 * rng.normal()) + 0.004 * rng.normal(size=9) * (trial % 3)
        w = np.abs(w) + 1e-4
        m, sig = rng.uniform(-0.3, 0.3, 4), np.exp(rng.uniform(np.log(0.6 / 256), np.log(2.4), 4))
        th, feas, E, y, z = R.inner(x, w, m, sig)
        a, p, q = th[..., 0], th[..., 1], th[..., 2]
        res = a[..., None] + (q - p)[..., None] * y[None] + (p + q)[..., None] * z[None] - w
        sse = (res * res).sum(axis=-1)                                        # [27, 4]
        assert np.allclose(sse, sse[0:1] + E, rtol=1e-9, atol=1e-18)
        for s, (sa, sp, sq) in enumerate(R.STATES):
            for t, st, hi in ((a, sa, w.max() + 0 * sig), (p, sp, sig), (q, sq, sig)):
                if st:
                    assert same(t[s], hi if st == 2 else 0 * hi)
        A, D, Cc, win, best = R.candidates(x, w, m, sig)
        for cnd in range(4):
            ok = np.flatnonzero(feas[:, cnd])
            assert len(ok) and win[cnd] == ok[np.argmin(E[ok, cnd])] and abs(best[cnd] - sse[win[cnd], cnd]) <= 1e-12 * best[cnd] + 1e-30
            ga, gp, gq = np.meshgrid(np.linspace(0, w.max(), 21), np.linspace(0, sig[cnd], 21), np.linspace(0, sig[cnd], 21), indexing="ij")
            rs = ga[..., None] + (gq - gp)[..., None] * y[cnd] + (gp + gq)[..., None] * z[cnd] - w
            assert (rs * rs).sum(axis=-1).min() >= best[cnd] * (1 - 1e-12)


# ------------------------------------------------------------------ recovery, quality, sensitivity
_cache = {}


def case(n, rounds=0):
    """Inputs, generator record and restatement of one generated batch, computed once and shared (read-only)."""
    if (n, rounds) not in _cache:
        c, gen = SC.batch(**SC.SHAPES[n])
        _cache[(n, rounds)] = (c, gen, restate(c, rounds=rounds, margins=True))
    return _cache[(n, rounds)]


def test_recovery_of_noiseless_rows():
    worst_v = worst_p = 0.0
    rows = 0
    for n in range(len(SC.SHAPES)):
        c, gen, r = case(n)
        ex = gen["exact"] & (r["flags"] != R.DEAD)
        rows += int(ex.sum())
        assert (r["flags"][ex] & ~R.HOLES == 0).all()                                    # the generating curve is interior
        with np.errstate(invalid="ignore"):
            worst_v = max(worst_v, float(np.nanmax(np.abs(r["fitted"] - gen["clean"])[ex])))
        worst_p = max(worst_p, float(np.abs(r["params"] - gen["params"])[ex].max()))
    log("recovery", rows=rows, vol=worst_v, params=worst_p)
    assert rows >= 20 and worst_v <= SC.RECOVERY["vol"] and worst_p <= SC.RECOVERY["params"]


def noisy_rows():
    out = []
    for n in range(len(SC.SHAPES)):
        if SC.SHAPES[n]["mK"] < 64:
            continue
        c, gen, r = case(n)
        B, mT, mK = c["vol"].shape
        for b in range(B):
            for j in range(mT):
                if not gen["exact"][b, j] and r["flags"][b, j] != R.DEAD and len(out) < SC.QUALITY_ROWS:
                    K = np.broadcast_to(c["Kq"], (B, mK))[b]
                    v = c["vol"][b, j]
                    ok = np.isfinite(v) & (v > 0)
                    x = np.log(K[ok] / c["spot"][b]) - c["rate"] * c["Tq"][j]
                    out.append((x, v[ok] ** 2 * c["Tq"][j], gen["params"][b, j], r["sse"][b, j]))
    return out


def test_quality_against_scipy_least_squares():
    """The restatement's SSE <= (1 + margin) x the best of 16 bounded least_squares starts (the generating parameters, and
    15 seeded draws from the search domain) on 24 noisy rows."""
    optimize = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(12)
    worst, rows = -1.0, noisy_rows()
    assert len(rows) == SC.QUALITY_ROWS
    for x, w, gen, sse in rows:
        X = x[-1] - x[0]
        lo = np.array([0.0, 0.0, -1.0, x[0], X / 256.0])
        hi = np.array([w.max(), 2.0, 1.0, x[-1], 4.0 * X])
        starts = [gen] + [lo + (hi - lo) * rng.random(5) * np.array([1, 0.1, 1, 1, 0.25]) for _ in range(15)]
        best = min(optimize.least_squares(lambda t: SC.svi_w(x, *t) - w, np.clip(s0, lo, hi), bounds=(lo, hi), xtol=1e-15, ftol=1e-15,
                                          gtol=1e-15, x_scale=np.array([w.max(), w.max(), 1.0, X, X])).cost * 2.0 for s0 in starts)
        worst = max(worst, sse / best - 1.0)
    log("quality", rows=len(rows), worst_excess=float(worst))
    assert worst <= SC.QUALITY_MARGIN


def gpu_inputs():
    """Every input the GPU tests compare with the restatement, by name (the end-to-end chain is measured in its own test)."""
    for name in sorted(SC.MICRO):
        yield f"micro[{name}]", SC.MICRO[name], name in SC.MICRO_UNSTABLE
    for s in SC.SHAPES:
        yield f"shape[{SC.shape_id(s)}]", SC.batch(**s)[0], False
    yield "lds", SC.batch(**SC.LDS_SHAPE)[0], False


def distances(a, b):
    """|a - b| of two runs in the quantities the GPU tests compare, per row (NaN in DEAD rows)."""
    with np.errstate(all="ignore"):
        steps = np.fmax(np.abs(a["params"][..., 3] - b["params"][..., 3]) / a["step"][..., 0], np.abs(a["u"] - b["u"]) / a["step"][..., 1])
        rmse = np.abs(a["fit"][..., 0] - b["fit"][..., 0]) / (a["fit"][..., 0] + SC.RMSE_FLOOR * a["wmax"])
        vol = np.fmax(np.nanmax(np.abs(a["fitted"] - b["fitted"]), axis=-1), np.abs(a["fit"][..., 1:3] - b["fit"][..., 1:3]).max(axis=-1))
        g = np.abs(a["fit"][..., 3] - b["fit"][..., 3])
    return {"steps": steps, "rmse_w": rmse, "vol": vol, "g_min": g}


@pytest.mark.parametrize("rounds", (0, 4))
def test_twin_sensitivity(rounds):
    """R_CPU: over every input of the GPU tests and three seeds, on the rows whose twin runs stay within UNSTABLE_STEPS final
    grid steps of the restatement, the distances stay below the recorded R_CPU; the unstable share stays below
    UNSTABLE_SHARE per case (the one flat micro row aside, which is unstable by construction); and the flags of the stable
    rows do not move."""
    worst = {k: 0.0 for k in SC.R_CPU[16]}
    unstable_rows = 0
    for name, c, expect_unstable in gpu_inputs():
        if rounds == 4 and not name.startswith("shape"):
            continue                                                            # the GPU tests run 4 rounds on SHAPES only
        r = restate(c, rounds=rounds)
        live = r["flags"] != R.DEAD
        if not live.any():
            continue
        unstable = np.zeros(live.shape, bool)
        runs = [(R.twin(c, seed, rounds)) for seed in SC.TWIN_SEEDS]
        ds = [distances(r, t) for t in runs]
        for d in ds:
            unstable |= live & ~(d["steps"] <= SC.UNSTABLE_STEPS)
        if expect_unstable:
            assert unstable.sum() <= 1
        else:
            assert unstable.sum() <= SC.UNSTABLE_SHARE * live.sum(), (name, int(unstable.sum()), int(live.sum()))
        unstable_rows += int(unstable.sum())
        ok = live & ~unstable
        for t, d in zip(runs, ds):
            assert same(t["flags"][ok], r["flags"][ok]) and same(t["flags"] & (R.DEAD | R.HOLES), r["flags"] & (R.DEAD | R.HOLES)), name
            for k in worst:
                if ok.any() and np.isfinite(d[k][ok]).any():
                    worst[k] = max(worst[k], float(np.nanmax(d[k][ok])))
    log(f"twin[rounds={rounds or 16}]", unstable_rows=unstable_rows, **worst)
    for k in worst:
        assert worst[k] <= SC.R_CPU[rounds or 16][k], (k, worst[k])


def test_twin_sensitivity_of_the_chain():
    """The end-to-end chain of the GPU test (surfaces from the CPU backend here) at the default rounds: most rows end with
    sigma at its lower border, the twin runs wander along it by some twenty final steps, and no row is unstable, no flag
    moves (EDGE is a band of 2^-20 of the domain, not the border's bits) and the distances stay below R_CPU."""
    import snapshot_cases as SNC
    b = SnapshotSurfaceBuilder(moneyness=SC.CHAIN_MONEYNESS, tenors=SC.CHAIN_TENORS, backend=R.RefBackend())
    worst = {k: 0.0 for k in SC.R_CPU[16]}
    edge = rows = 0
    for r in b.build(SNC.big_chain(**SC.CHAIN)):
        c = dict(vol=np.asarray(r.out), Kq=np.asarray(r.Kq), Tq=SC.CHAIN_TENORS, spot=np.asarray(r.spot), rate=SC.CHAIN_RATE)
        ref = restate(c, margins=True)
        edge, rows = edge + int((ref["flags"] & R.EDGE != 0).sum()), rows + ref["flags"].size
        for seed in SC.TWIN_SEEDS:
            t = R.twin(c, seed)
            d = distances(ref, t)
            assert (d["steps"] <= SC.UNSTABLE_STEPS).all() and same(t["flags"], ref["flags"])
            worst = {k: max(worst[k], float(np.nanmax(d[k]))) for k in worst}
    log("twin[chain, rounds=16]", rows=rows, edge_rows=edge, **worst)
    assert edge >= rows // 2
    for k in worst:
        assert worst[k] <= SC.R_CPU[16][k], (k, worst[k])


def test_generators_stay_inside_the_margins():
    """>= 90 % of the rows of every generated batch are not DEAD (asserted by the restatement), a quarter of the rows is
    exact, holes occur, and both grid forms are there."""
    seen = 0
    for n, s in enumerate(SC.SHAPES):
        c, gen, r = case(n)
        assert gen["exact"].reshape(-1)[::4].all() and gen["exact"].sum() == (gen["exact"].size + 3) // 4
        assert (c["Kq"].ndim == 2) == s["per_kq"]
        seen |= int(np.bitwise_or.reduce(r["flags"].reshape(-1)))
    assert seen & R.HOLES
    c, _ = SC.batch(**SC.STREAM_SHAPE)
    assert c["vol"].shape == (64, 16, 64)


# ------------------------------------------------------------------ host layers with the restatement as the backend
def _built():
    chain = synthetic_chain("btc", expiry_days=(0.5, 3), strikes=tuple(np.linspace(17000.0, 34000.0, 12)), n_hours=3, seed=5)
    b = SnapshotSurfaceBuilder(backend=R.RefBackend(), moneyness=np.linspace(0.72, 1.28, 24), tenors=np.array([1.0, 2.0, 2.8]) / 365)
    return b, b.build(chain)


def test_svi_report_and_frame():
    b, res = _built()
    reps = b.svi(res, rate=0.01, rounds=6, fitted=True)
    assert len(reps) == len(res) == 1
    v, r = reps[0], res[0]
    assert v.underlying == "btc" and v.dates.equals(r.dates) and same(v.tenors, r.tenors) and same(v.moneyness, r.moneyness)
    assert v.rate == 0.01 and v.rounds == 6
    ref = R.restate(r.out, r.Kq, r.tenors, r.spot, 0.01, 6)
    for k in ("params", "fit", "flags", "fitted"):
        assert same(getattr(v, k), ref[k]), k
    assert b.svi(res)[0].fitted is None and b.svi(res)[0].rounds == 0
    keep = np.flatnonzero(np.asarray(r.quotes) > 0)
    assert len(keep) == 3 and (ref["flags"][keep] != R.DEAD).all()
    assert (np.delete(ref["flags"], keep, axis=0) == R.DEAD).all()                # minutes without quotes: NaN surfaces

    f = svi_frame(reps, res)
    cols = ["underlying", "date", "spot", "tenor", "a", "b", "rho", "m", "sigma", "rmse_vol", "max_vol_err", "g_min", "flags"]
    assert list(f.columns) == cols
    assert [str(t) for t in f.dtypes] == ["object", str(f["date"].dtype)] + ["float64"] * 10 + ["int32"]
    assert len(f) == len(keep) * 3 and list(f["date"][::3]) == list(r.dates[keep]) and same(f["tenor"].to_numpy(), np.tile(r.tenors, 3))
    assert same(f["spot"].to_numpy(), np.repeat(np.asarray(r.spot)[keep], 3))
    for q, k in enumerate(("a", "b", "rho", "m", "sigma")):
        assert same(f[k].to_numpy(), ref["params"][keep, :, q].reshape(-1)), k
    for q, k in ((1, "rmse_vol"), (2, "max_vol_err"), (3, "g_min")):
        assert same(f[k].to_numpy(), ref["fit"][keep, :, q].reshape(-1)), k
    assert same(f["flags"].to_numpy(), ref["flags"][keep].reshape(-1))
    assert len(svi_frame([], [])) == 0 and list(svi_frame([], []).columns) == cols
    for bad in (-1, 25, 2.5):
        with pytest.raises(ValueError, match="rounds"):
            b.svi(res, rounds=bad)


def test_svi_task_end_to_end(tmp_path):
    import complete_pipeline as cp
    import snapshot_ref
    store = FrameStore(str(tmp_path))
    # three hourly quotes per contract stand in for the interpolation task's output: 121 minute snapshots, 3 with quotes
    for f in synthetic_chain("btc", expiry_days=(20, 45), strikes=tuple(np.linspace(17000.0, 34000.0, 6)), n_hours=3, seed=5):
        store.write_output(f["symbol"].iloc[0], f, 1)
    assert cp.main(["--task", "svi", "--data-dir", str(tmp_path)], surface_backend=R.RefBackend()) == 0
    assert store.read_table("iv_surfaces", "btc") is None and store.read_table("iv_volindex", "btc") is None
    out = store.read_table("iv_svi", "btc")
    assert list(out.columns) == ["underlying", "date", "spot", "tenor", "a", "b", "rho", "m", "sigma", "rmse_vol", "max_vol_err",
                                 "g_min", "flags"]
    frames = [store.read_output(s) for s in store.symbols("interpolated_trading_tickers")]
    ref, _ = snapshot_ref.restate(frames, M, TQ)
    r = ref["btc"]
    live = np.flatnonzero(r["quotes"] > 0)
    v = R.restate(r["out"], r["Kq"], TQ, r["spot"], 0.0)
    assert len(live) == 3 and len(out) == len(live) * len(TQ)
    assert np.allclose(out["sigma"].to_numpy(), v["params"][live, :, 4].reshape(-1), rtol=1e-9, equal_nan=True)
    assert same(out["flags"].to_numpy().astype(np.int32), v["flags"][live].reshape(-1))
    fl = v["flags"][live].reshape(-1)
    pipe = cp.CompleteOptimizedPipeline(cp.get_config(), data_dir=str(tmp_path), surface_backend=R.RefBackend())
    res = pipe.run_svi()
    assert res["success"] and res["underlyings"] == 1 and res["rows"] == len(out)
    assert res["fitted_rows"] == int((fl != R.DEAD).sum()) and res["butterfly_rows"] == int(((fl & R.BUTTERFLY) != 0).sum())
    assert set(res) == set(pipe.run_smiles()) | {"fitted_rows", "butterfly_rows"}


# ------------------------------------------------------------------ C ABI validation, no device needed
def _args(**kw):
    P = 64
    a = _lib.SviArgs()
    a.vol, a.Kq, a.Tq, a.spot = (kw.get(k, P) for k in ("vol", "Kq", "Tq", "spot"))
    a.kq_stride, a.tq_stride, a.rate = kw.get("kq_stride", 0), kw.get("tq_stride", 0), 0.0
    a.mK, a.mT, a.B, a.rounds = kw.get("mK", 64), kw.get("mT", 16), kw.get("B", 1), kw.get("rounds", 0)
    a.params, a.fit, a.flags, a.fitted = (kw.get(k, P) for k in ("params", "fit", "flags", "fitted"))
    a.rows_per_wg = kw.get("rpw", 0)
    return a


def test_abi_validation_codes_without_gpu():
    """Host-side validation returns errno-style codes before any launch (the fake pointers are never dereferenced)."""
    lib = _lib.load()
    assert _lib.ABI_VERSION == 5 == lib.ivs_version()                                           # the symbol is additive
    assert hasattr(lib, "ivs_svi_slices_f64") and "ivs_svi_slices_f64" in _lib.SIGNATURES
    call = lambda **kw: lib.ivs_svi_slices_f64(C.byref(_args(**kw)), None, 0, None)   # noqa: E731
    assert lib.ivs_svi_slices_f64(None, None, 0, None) == -22 and b"null args" in lib.ivs_last_error()
    for k in ("vol", "Kq", "Tq", "spot", "params", "fit", "flags"):
        assert call(**{k: None}) == -22 and b"null pointer" in lib.ivs_last_error(), k
    assert call(B=-1) == -22 and call(mT=-1) == -22 and call(mK=-1) == -22 and call(kq_stride=-1) == -22 and call(tq_stride=-1) == -22
    assert b"negative" in lib.ivs_last_error()
    for bad in (63, 65, 1, 128):
        assert call(kq_stride=bad) == -22 and b"stride" in lib.ivs_last_error(), bad
    for bad in (15, 17, 1, 64):
        assert call(tq_stride=bad) == -22 and b"stride" in lib.ivs_last_error(), bad
    assert call(kq_stride=64, tq_stride=16, B=0) == 0
    assert call(mK=4) == -34 and b"mK=4" in lib.ivs_last_error() and call(mK=0) == -34           # IVS_ERANGE
    assert call(mK=1025) == -34 and b"mK=1025" in lib.ivs_last_error() and b"LDS" in lib.ivs_last_error()
    assert call(rounds=25) == -34 and b"rounds=25" in lib.ivs_last_error() and call(rounds=-1) == -34
    assert call(rpw=5) == -34 and b"rows_per_wg=5" in lib.ivs_last_error() and call(rpw=-1) == -34
    assert call(B=1 << 27, mT=16) == -34 and b"134217728 x 16 rows" in lib.ivs_last_error()     # B * mT = 2^31
    assert call(B=1 << 40, mT=2) == -34
    assert call(B=0) == 0 and call(mT=0) == 0 and call(B=0, vol=None, flags=None) == 0 and lib.ivs_last_error() == b""   # a no-op
    assert call(B=0, mK=4) == -34                                                               # the shape is checked first
    assert (_lib.SV_BOUND, _lib.SV_EDGE, _lib.SV_HOLES, _lib.SV_DEAD, _lib.SV_BUTTERFLY, _lib.SV_DEGENERATE) == \
        (R.BOUND, R.EDGE, R.HOLES, R.DEAD, R.BUTTERFLY, R.DEGENERATE) == (1, 2, 4, 8, 16, 32)
    assert C.sizeof(_lib.SviArgs) == 120


def test_stale_library_is_reported(monkeypatch):
    """A libivs.so without the new symbol raises EngineUnavailable with a message that says to rebuild."""
    class Old:
        def __getattr__(self, name):
            if name == "ivs_svi_slices_f64":
                raise AttributeError(name)
            return lambda *a: _lib.ABI_VERSION
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.C, "CDLL", lambda path: Old())
    with pytest.raises(_lib.EngineUnavailable, match="ivs_svi_slices_f64.*rebuild"):
        _lib.load()
