"""CPU: model-free variance, skew, kurtosis and the vol index (rules M1-M8).  The restatement
(tests/mm_ref.py) is anchored against the closed forms of a flat surface, checked on one hand-built micro case per rule and
flag, and its own rounding level against mpmath at 50 digits is held below the recorded R_CPU; the generators are held to
the margins the GPU tests rely on; the host layers (builder, frames, pipeline task) run with the restatement injected as
their backend; the C ABI's argument validation runs without a device.  The kernel itself is checked in
test_moments_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import mm_cases as MC
import mm_ref as R
from iv_interpolation_amd import _lib, synth
from iv_interpolation_amd.frame_store import FrameStore, synthetic_chain
from iv_interpolation_amd.snapshots import SnapshotSurfaceBuilder, moments_frame, volindex_frame

M, TQ = synth.query_grids(64, 16)
EPS = MC.EPS


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def restate(c, **kw):
    return R.restate(c["vol"], c["Kq"], c["Tq"], c["spot"], c["rate"], c["horizons"], c["min_mass"], **kw)


# ------------------------------------------------------------------ the closed forms of a flat surface
@pytest.mark.parametrize("n", range(3))
def test_anchor_flat_surface(n):
    """Flat vol sigma: L = var = w = sigma^2 tau, skew = 0, kurt = 3.  The trapezoid is second order: going from 64 to 127
    nodes (half the spacing) cuts |L / w - 1| by a factor in [3.5, 4.5]; the 64-node errors stay within the recorded
    figures plus 20 %."""
    tau = MC.ANCHOR_TAUS[n]
    w = 0.6 * 0.6 * tau
    r64, r127 = restate(MC.flat_anchor(64, tau)), restate(MC.flat_anchor(127, tau))
    assert r64["flags"][0, 0] == 0 and r127["flags"][0, 0] == 0
    e64, e127 = r64["raw"][0, 0, 0] / w - 1.0, r127["raw"][0, 0, 0] / w - 1.0
    skew, kurt = r64["stats"][0, 0, 2], r64["stats"][0, 0, 3]
    print(f"anchor tau={tau:.5f}: L/w-1 = {e64:.6f} (64), {e127:.6f} (127), ratio {e64 / e127:.3f}; skew {skew:.6f}, kurt-3 {kurt - 3:.6f}; "
          f"mf_vol {r64['stats'][0, 0, 0]:.6f}, bkm_vol {r64['stats'][0, 0, 1]:.6f}, mass {r64['mass'][0, 0]:.15f}")
    assert 3.5 <= abs(e64) / abs(e127) <= 4.5
    assert abs(e64) <= 1.2 * MC.ANCHOR_L[n] and abs(skew) <= 1.2 * MC.ANCHOR_SKEW[n] and abs(kurt - 3.0) <= 1.2 * MC.ANCHOR_KURT[n]
    assert abs(r64["stats"][0, 0, 0] / 0.6 - 1.0) <= 1.2 * MC.ANCHOR_L[n]            # mf_vol = sigma (1 + e)^(1/2)
    assert 1.0 - r64["mass"][0, 0] < 1e-14                                          # +-8 standard deviations


def test_default_grid_truncation():
    """What DESIGN.md section 11 says about the default 0.72-1.28 moneyness grid: a flat 60 % surface (rate 0.01) keeps
    L / w = 1.006 at 2 days, 0.968 at 30 days and 0.561 at one year, and says so through `mass` and TRUNCATED."""
    taus = np.array([2.0 / 365.0, 30.0 / 365.0, 1.0])
    r = R.restate(np.full((1, 3, 64), 0.6), 100.0 * M, taus, [100.0], 0.01, ())
    ratio = r["raw"][0, :, 0] / (0.36 * taus)
    print("default grid, flat 60 %: L/w", ratio, "mass", r["mass"][0], "flags", r["flags"][0])
    assert np.allclose(ratio, [1.006, 0.968, 0.561], atol=5e-4)
    assert r["flags"][0].tolist() == [0, R.TRUNCATED, R.TRUNCATED]


# ------------------------------------------------------------------ one case per rule and flag
@pytest.mark.parametrize("name", sorted(MC.MICRO))
def test_micro_case(name):
    c = MC.MICRO[name]
    r = restate(c)
    assert same(r["flags"], c["flags"]) and r["flags"].dtype == np.int32, r["flags"]
    assert same(r["index_flags"], c["index_flags"]) and r["index_flags"].dtype == np.int32, r["index_flags"]
    dead = c["flags"] == R.DEAD
    for k in ("raw", "stats"):
        assert same(np.isnan(r[k]), np.broadcast_to(dead[:, :, None], r[k].shape)), k     # M1: NaN exactly in the DEAD rows
    assert same(np.isnan(r["mass"]), dead)
    assert same(np.isnan(r["index"]), c["index_flags"] == R.NO_BRACKET)
    live = ~dead
    assert (r["raw"][live][:, 0] > 0).all() and (r["stats"][live][:, :2] > 0).all()
    assert same(r["stats"][live], R.stats_of(r["raw"][live], np.broadcast_to(c["Tq"], dead.shape)[live]))


def test_forward_node_rules():
    """M4 by construction: with the forward on a node nothing is inserted, so the row equals the plain trapezoid; with it
    between two nodes the split row equals the plain trapezoid over the nodes plus the forward node."""
    from scipy import special
    c = MC.MICRO["forward_between_nodes"]
    k, tau, F = c["Kq"], c["Tq"][0], 102.0
    kn = np.insert(k, 21, F)
    x = np.log(kn / F)
    sq = 0.5 * np.sqrt(tau)
    d2 = -x / sq - sq / 2
    Phi = lambda z: 0.5 * special.erfc(-z / np.sqrt(2.0))  # noqa: E731
    Q = np.where(kn < F, kn * Phi(-d2) - F * Phi(-d2 - sq), F * Phi(d2 + sq) - kn * Phi(d2))
    assert abs(Q[21] / (F * special.erf(sq / (2 * np.sqrt(2.0)))) - 1) < 1e-13           # put = call at the forward
    f = 2 * Q / kn ** 2
    L = np.sum(0.5 * (f[1:] + f[:-1]) * np.diff(kn))
    assert abs(restate(c)["raw"][0, 0, 0] / L - 1) < 1e-13
    # the hole case pairs 97 with 105 and splits that segment
    c = MC.MICRO["forward_across_a_hole"]
    keep = np.arange(41) != 20
    d = dict(c, vol=c["vol"][:, :, keep], Kq=c["Kq"][keep])
    a, b = restate(c), restate(d)
    assert same(a["raw"], b["raw"]) and same(a["index"], b["index"]) and (b["flags"] == 0).all()


def test_index_rules():
    """M7 on the micro cases: a horizon on a tenor returns that row's own mf_vol, one inside interpolates L linearly."""
    c = MC.MICRO["horizon_on_a_tenor"]
    r = restate(c)
    L, t = r["raw"][0, :, 0], c["Tq"]
    assert np.allclose(r["index"][0, :3], 100.0 * r["stats"][0, :, 0], rtol=1e-14)
    Lh = L[1] + (L[2] - L[1]) * (33.0 / 365.0 - t[1]) / (t[2] - t[1])
    assert r["index"][0, 3] == 100.0 * np.sqrt(Lh / (33.0 / 365.0))
    c = MC.MICRO["dead_row_between_live_rows"]
    r = restate(c)
    L, t = r["raw"][0, :, 0], c["Tq"]
    Lh = L[0] + (L[2] - L[0]) * (30.0 / 365.0 - t[0]) / (t[2] - t[0])
    assert r["index"][0, 0] == 100.0 * np.sqrt(Lh / (30.0 / 365.0))


def test_shared_and_per_snapshot_grids_agree():
    c = MC.smooth(3, 3, 9, 11, per_kq=False, per_tq=False)
    a, b = restate(c), restate(dict(c, Kq=np.tile(c["Kq"], (3, 1)), Tq=np.tile(c["Tq"], (3, 1))))
    for k in ("raw", "stats", "mass", "flags", "index", "index_flags"):
        assert same(a[k], b[k]), k


# ------------------------------------------------------------------ what the GPU tests rely on
def gpu_inputs():
    """Every input the GPU tests send to the kernel."""
    for name in sorted(MC.MICRO):
        yield f"micro[{name}]", MC.MICRO[name]
    for name in sorted(MC.EDGE):
        yield f"edge[{name}]", MC.EDGE[name][0]
    for s in MC.SHAPES:
        yield f"shape[{MC.shape_id(s)}]", MC.smooth(**s)


def test_generators_stay_inside_the_margins():
    """Asserted by the restatement: in every row that is not DEAD, L and var >= 1e-9 x their scale and mass at least 1e-6
    away from min_mass; >= 90 % of the rows are not DEAD.  The shapes carry HOLES and TRUNCATED rows (ONE_SIDED and DEAD are
    the micro cases' business); the chunk-edge cases keep the forward inside the strikes and a finite index."""
    seen = 0
    for s in MC.SHAPES:
        r = restate(MC.smooth(**s), margins=True)
        seen |= int(np.bitwise_or.reduce(r["flags"].reshape(-1))) | int(np.bitwise_or.reduce(r["index_flags"].reshape(-1)))
    assert seen & R.TRUNCATED and seen & R.HOLES
    for name, (c, holes) in MC.EDGE.items():
        r = restate(c, margins=True)
        assert ((r["flags"] & R.HOLES) == holes).all() and not (r["flags"] & (R.DEAD | R.ONE_SIDED)).any(), name
        assert np.isfinite(r["index"]).all(), name


def test_rounding_level():
    """r = max |float64 - mpmath (50 digits)| / (eps raw_scale) over the exact inputs the GPU tests use stays below the
    recorded R_CPU (the GPU tolerance is 8 R_CPU eps raw_scale); flags agree."""
    worst = np.zeros(4)
    for name, c in gpu_inputs():
        a, b = restate(c), restate(c, exact=True)
        assert same(a["flags"], b["flags"]) and same(a["index_flags"], b["index_flags"]), name
        ok = a["flags"] != R.DEAD
        if ok.any():
            err = np.abs(a["raw"][ok] - b["raw"][ok]) / (EPS * a["raw_scale"][ok])
            worst = np.maximum(worst, err.max(axis=0).astype(np.float64))
    print("rounding level: L {:.3f}, V {:.3f}, W {:.3f}, X {:.3f} (R_CPU = {})".format(*worst, MC.R_CPU))
    assert worst.max() <= MC.R_CPU, worst


# ------------------------------------------------------------------ host layers with the restatement as the backend
def _built():
    chain = synthetic_chain("btc", expiry_days=(0.5, 3), strikes=tuple(np.linspace(17000.0, 34000.0, 12)), n_hours=3, seed=5)
    b = SnapshotSurfaceBuilder(backend=R.RefBackend(), moneyness=np.linspace(0.72, 1.28, 24), tenors=np.array([1.0, 2.0, 2.8]) / 365)
    return b, b.build(chain)


def test_moment_report_and_frames():
    b, res = _built()
    hz = (1.5 / 365, 2.5 / 365, 30 / 365)
    reps = b.moments(res, rate=0.01, horizons=hz, min_mass=0.9)
    assert len(reps) == len(res) == 1
    m, r = reps[0], res[0]
    assert m.underlying == "btc" and m.dates.equals(r.dates) and same(m.tenors, r.tenors) and same(m.horizons, hz)
    assert m.rate == 0.01 and m.min_mass == 0.9
    ref = R.restate(r.out, r.Kq, r.tenors, r.spot, 0.01, hz, 0.9)
    for k in ("raw", "stats", "mass", "flags", "index", "index_flags"):
        assert same(getattr(m, k), ref[k]), k
    keep = np.flatnonzero(np.asarray(r.quotes) > 0)
    assert len(keep) == 3 and (ref["flags"][keep] != R.DEAD).all() and np.isfinite(ref["index"][keep, :2]).all()
    assert (ref["index_flags"][keep, 2] == R.NO_BRACKET).all()                    # 30 days lies beyond these tenors
    assert (np.delete(ref["flags"], keep, axis=0) == R.DEAD).all()                # minutes without quotes: NaN surfaces

    f = moments_frame(reps, res)
    assert list(f.columns) == ["underlying", "date", "spot", "tenor", "mf_vol", "bkm_vol", "skew", "kurt", "mass", "flags"]
    assert [str(t) for t in f.dtypes] == ["object", str(f["date"].dtype)] + ["float64"] * 7 + ["int32"]
    assert len(f) == len(keep) * 3 and list(f["date"][::3]) == list(r.dates[keep]) and same(f["tenor"].to_numpy(), np.tile(r.tenors, 3))
    assert same(f["spot"].to_numpy(), np.repeat(np.asarray(r.spot)[keep], 3))
    for q, k in enumerate(("mf_vol", "bkm_vol", "skew", "kurt")):
        assert same(f[k].to_numpy(), ref["stats"][keep, :, q].reshape(-1)), k
    assert same(f["mass"].to_numpy(), ref["mass"][keep].reshape(-1)) and same(f["flags"].to_numpy(), ref["flags"][keep].reshape(-1))

    v = volindex_frame(reps, res)
    assert list(v.columns) == ["underlying", "date", "spot", "vix_1.5d", "flags_1.5d", "vix_2.5d", "flags_2.5d", "vix_30d", "flags_30d"]
    assert [str(t) for t in v.dtypes] == ["object", str(v["date"].dtype), "float64"] + ["float64", "int32"] * 3
    assert len(v) == len(keep) and list(v["date"]) == list(r.dates[keep])
    for q, d in enumerate(("1.5", "2.5", "30")):
        assert same(v[f"vix_{d}d"].to_numpy(), ref["index"][keep, q]) and same(v[f"flags_{d}d"].to_numpy(), ref["index_flags"][keep, q])
    assert len(moments_frame([], [])) == 0 and list(moments_frame([], []).columns) == list(f.columns)
    assert len(volindex_frame([], [])) == 0 and list(volindex_frame([], []).columns) == ["underlying", "date", "spot"]
    assert list(volindex_frame(b.moments(res), res).columns) == ["underlying", "date", "spot", "vix_30d", "flags_30d"]   # the default
    other = b.moments(res, horizons=(7 / 365,))
    with pytest.raises(ValueError, match="different horizon lists"):
        volindex_frame(reps + other, res + res)


def test_builder_rejects_bad_options():
    b, res = _built()
    for bad in ((), (0.0,), (-1.0,), (float("nan"),), (float("inf"),), tuple([0.1] * 9)):
        with pytest.raises(ValueError, match="horizons"):
            b.moments(res, horizons=bad)
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="min_mass"):
            b.moments(res, min_mass=bad)


def test_volindex_task_end_to_end(tmp_path):
    import complete_pipeline as cp
    import snapshot_ref
    from oracle_backend import OracleBackend
    store = FrameStore(str(tmp_path))
    for f in synthetic_chain("btc", expiry_days=(20, 45), strikes=tuple(np.linspace(17000.0, 34000.0, 6)), n_hours=12, seed=5):
        store.write_source(f["symbol"].iloc[0], f)
    assert cp.main(["--task", "interpolation", "--data-dir", str(tmp_path)], backend=OracleBackend()) == 0
    assert cp.main(["--task", "volindex", "--data-dir", str(tmp_path)], surface_backend=R.RefBackend()) == 0
    assert store.read_table("iv_surfaces", "btc") is None and store.read_table("iv_arbitrage", "btc") is None
    out = store.read_table("iv_volindex", "btc")
    assert list(out.columns) == ["underlying", "date", "spot", "vix_30d", "flags_30d"]
    frames = [store.read_output(s) for s in store.symbols("interpolated_trading_tickers")]
    ref, _ = snapshot_ref.restate(frames, M, TQ)
    r = ref["btc"]
    live = np.flatnonzero(r["quotes"] > 0)
    m = R.restate(r["out"], r["Kq"], TQ, r["spot"], 0.0)
    assert len(out) == len(live) == 661
    assert np.allclose(out["vix_30d"].to_numpy(), m["index"][live, 0], rtol=1e-9, equal_nan=True)
    assert same(out["flags_30d"].to_numpy().astype(np.int32), m["index_flags"][live, 0])
    finite = int(np.isfinite(m["index"][live, 0]).sum())
    assert finite > 600                                                          # the chain's expiries bracket 30 days
    pipe = cp.CompleteOptimizedPipeline(cp.get_config(), data_dir=str(tmp_path), surface_backend=R.RefBackend())
    res = pipe.run_volindex()
    assert res["success"] and res["underlyings"] == 1 and res["rows"] == len(out) and res["indexed_snapshots"] == finite
    assert set(res) == set(pipe.run_smiles()) | {"indexed_snapshots"}


# ------------------------------------------------------------------ C ABI validation, no device needed
def _args(**kw):
    P = 64
    a = _lib.MomentsArgs()
    a.vol, a.Kq, a.Tq, a.spot = (kw.get(k, P) for k in ("vol", "Kq", "Tq", "spot"))
    a.kq_stride, a.tq_stride, a.rate, a.min_mass = kw.get("kq_stride", 0), kw.get("tq_stride", 0), 0.0, kw.get("min_mass", 0.99)
    hz = kw.get("horizons", (30.0 / 365.0,))
    a._keep = (C.c_double * max(len(hz), 1))(*hz)
    a.horizons = None if kw.get("null_horizons") else C.cast(a._keep, C.POINTER(C.c_double))
    a.nH = kw.get("nH", len(hz))
    a.mK, a.mT, a.B = kw.get("mK", 64), kw.get("mT", 16), kw.get("B", 1)
    a.raw, a.stats, a.mass, a.flags = (kw.get(k, P) for k in ("raw", "stats", "mass", "flags"))
    a.index, a.index_flags = kw.get("index", P), kw.get("index_flags", P)
    a.snapshots_per_wg = kw.get("spw", 0)
    return a


def test_abi_validation_codes_without_gpu():
    """Host-side validation returns errno-style codes before any launch (the fake pointers are never dereferenced)."""
    lib = _lib.load()
    assert _lib.ABI_VERSION == 5 == lib.ivs_version()                                           # the symbol is additive
    assert hasattr(lib, "ivs_surface_moments_f64") and "ivs_surface_moments_f64" in _lib.SIGNATURES
    call = lambda **kw: lib.ivs_surface_moments_f64(C.byref(_args(**kw)), None, 0, None)   # noqa: E731
    assert lib.ivs_surface_moments_f64(None, None, 0, None) == -22 and b"null args" in lib.ivs_last_error()
    for k in ("vol", "Kq", "Tq", "spot", "raw", "stats", "mass", "flags"):
        assert call(**{k: None}) == -22 and b"null pointer" in lib.ivs_last_error(), k
    for k in ("index", "index_flags"):
        assert call(**{k: None}) == -22 and b"null index" in lib.ivs_last_error(), k
    assert call(nH=0, horizons=(), index=None, index_flags=None, B=0) == 0                      # no M7: both may be NULL
    assert call(null_horizons=True) == -22 and b"null horizons" in lib.ivs_last_error()
    assert call(B=-1) == -22 and call(mT=-1) == -22 and call(mK=-1) == -22 and call(kq_stride=-1) == -22 and call(tq_stride=-1) == -22
    assert call(nH=-1) == -22 and b"negative" in lib.ivs_last_error()
    for bad in (63, 65, 1, 128):
        assert call(kq_stride=bad) == -22 and b"stride" in lib.ivs_last_error(), bad
    for bad in (15, 17, 1, 64):
        assert call(tq_stride=bad) == -22 and b"stride" in lib.ivs_last_error(), bad
    assert call(kq_stride=64, tq_stride=16, B=0) == 0
    for bad in (-0.01, 1.01, float("nan"), float("inf")):
        assert call(min_mass=bad) == -22 and b"min_mass" in lib.ivs_last_error(), bad
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(horizons=(0.1, bad)) == -22 and b"horizon 1" in lib.ivs_last_error(), bad
    assert call(mK=1) == -34 and b"mK=1" in lib.ivs_last_error() and call(mK=0) == -34           # IVS_ERANGE
    assert call(B=1 << 27, mT=16) == -34 and b"134217728 x 16 rows" in lib.ivs_last_error()     # B * mT = 2^31
    assert call(B=1 << 40, mT=2) == -34
    assert call(horizons=tuple([0.1] * 9)) == -34 and b"nH=9" in lib.ivs_last_error()
    assert call(spw=5) == -34 and b"snapshots_per_wg=5" in lib.ivs_last_error() and call(spw=-1) == -34
    assert call(mT=513) == -34 and b"mT=513" in lib.ivs_last_error()                            # the LDS row slots
    assert call(B=0) == 0 and call(mT=0) == 0 and call(B=0, vol=None, flags=None) == 0 and lib.ivs_last_error() == b""   # a no-op
    assert call(B=0, mK=1) == -34                                                               # the shape is checked first
    assert (_lib.MM_ONE_SIDED, _lib.MM_TRUNCATED, _lib.MM_HOLES, _lib.MM_DEAD, _lib.MM_NO_BRACKET) == \
        (R.ONE_SIDED, R.TRUNCATED, R.HOLES, R.DEAD, R.NO_BRACKET) == (1, 2, 4, 8, 16)
    assert C.sizeof(_lib.MomentsArgs) == 152


def test_stale_library_is_reported(tmp_path, monkeypatch):
    """A libivs.so without the new symbol raises EngineUnavailable with a message that says to rebuild."""
    class Old:
        def __getattr__(self, name):
            if name == "ivs_surface_moments_f64":
                raise AttributeError(name)
            return lambda *a: _lib.ABI_VERSION
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.C, "CDLL", lambda path: Old())
    with pytest.raises(_lib.EngineUnavailable, match="ivs_surface_moments_f64.*rebuild"):
        _lib.load()
