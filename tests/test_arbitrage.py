"""CPU: static-arbitrage report, Dupire local vol and density (rules A1-A8).  The restatement
(tests/arb_ref.py) is checked on one hand-built micro case per rule and anchored against two closed forms; its own rounding
level against np.longdouble is held below the recorded R_CPU; the host layers (builder, frames, pipeline task) run with the
restatement injected as their backend; the C ABI's argument validation runs without a device.  The kernel itself is
checked in test_arbitrage_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import arb_cases as AC
import arb_ref as R
from iv_interpolation_amd import _lib, synth
from iv_interpolation_amd.frame_store import FrameStore, synthetic_chain
from iv_interpolation_amd.snapshots import SnapshotSurfaceBuilder, arbitrage_frame, local_vol_frame

M, TQ = synth.query_grids(64, 16)
EPS = AC.EPS
LD = np.longdouble
HAS_LD = np.finfo(LD).eps < np.finfo(np.float64).eps


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def restate(c, **kw):
    return R.restate(c["vol"], c["Kq"], c["Tq"], c["spot"], c.get("rate", 0.0), **kw)


@pytest.mark.parametrize("name", sorted(AC.CASES))
def test_micro_case(name):
    c = AC.CASES[name]
    r = restate(c)
    assert same(r["flags"], c["flags"]) and r["flags"].dtype == np.int32, r["flags"]
    assert same(r["counts"], c["counts"]) and r["counts"].dtype == np.int32, r["counts"]
    ev = (c["flags"] & (R.DEAD | R.NO_STENCIL)) == 0
    assert same(r["evaluated"], ev)
    assert same(np.isnan(r["density"]), ~ev)                                            # A6: NaN exactly where not evaluated
    assert same(np.isnan(r["local_vol"]), ~(ev & ((c["flags"] & R.CALENDAR) == 0) & ((c["flags"] & R.BUTTERFLY) == 0)))
    assert same(np.sign(r["density"][ev]), np.where(c["flags"][ev] & R.BUTTERFLY, -1.0, 1.0))   # negative where g is
    for b in range(len(c["counts"])):                                                   # A7: the minima, NaN without nodes
        if c["counts"][b, 0] == 0:
            assert np.isnan(r["worst"][b]).all()
        else:
            assert r["worst"][b, 0] == np.nanmin(r["N"][b]) and r["worst"][b, 1] == np.nanmin(r["g"][b])
            assert (r["worst"][b, 0] < 0) == (c["counts"][b, 1] > 0) and (r["worst"][b, 1] < 0) == (c["counts"][b, 2] > 0)


def test_shared_and_per_snapshot_grids_agree():
    shared, spelled = AC.shared_and_spelled()
    a, b = restate(shared), restate(spelled)
    for k in ("flags", "counts", "worst", "local_vol", "density"):
        assert same(a[k], b[k]), k
    assert a["counts"][:, 0].min() > 0


def _exact(dtype):
    return dtype if HAS_LD else np.float64


def _anchor(r, c, N, g, lv, den):
    """The restatement against exact N, g, local vol and density at every evaluated node, within 8 eps scale."""
    ev = r["evaluated"]
    assert ev[:, :, 1:-1].all() and not ev[:, :, 0].any() and not ev[:, :, -1].any()
    tol_N, tol_g = 8 * EPS * r["N_scale"], 8 * EPS * r["g_scale"]
    eN = np.abs(r["N"] - N)[ev] / (EPS * r["N_scale"][ev])
    eg = np.abs(r["g"] - g)[ev] / (EPS * r["g_scale"][ev])
    tol_lv = lv * (0.5 * (tol_N / np.abs(N) + tol_g / np.abs(g)) + 8 * EPS)
    tol_den = np.abs(den) * (tol_g / np.abs(g) + 8 * EPS * (1 + r["d2"] ** 2))
    elv, eden = (np.abs(r["local_vol"] - lv) / tol_lv)[ev], (np.abs(r["density"] - den) / tol_den)[ev]
    print(f"anchor: N {eN.max():.2f} g {eg.max():.2f} eps*scale; local vol {float(elv.max()):.2f} density {float(eden.max()):.2f} of the tolerance")
    assert eN.max() <= 8 and eg.max() <= 8 and elv.max() <= 1 and eden.max() <= 1
    assert (r["flags"][ev] == 0).all()


@pytest.mark.parametrize("sigma,S,rate", [(0.5, 100.0, 0.0), (0.31, 27123.4, 0.03), (0.9, 0.41, 0.0), (0.65, 1800.0, -0.01)])
def test_anchor_flat_surface(sigma, S, rate):
    """Flat surface: g = 1, N = sigma^2, local vol = sigma, lognormal density."""
    c = AC.flat_surface(sigma, S, rate)
    r = restate(c)
    f = _exact(LD)
    k, tau = c["Kq"].astype(f)[None, None, :], c["Tq"].astype(f)[None, :, None]
    w = f(sigma) * f(sigma) * tau
    d2 = -(np.log(k / f(S)) - f(rate) * tau) / np.sqrt(w) - np.sqrt(w) / 2
    den = np.exp(-d2 * d2 / 2) / (k * np.sqrt(2 * f(np.pi) * w))
    one = np.ones(r["N"].shape)
    _anchor(r, c, (f(sigma) * f(sigma) * one).astype(np.float64), one, sigma * one, den.astype(np.float64))


@pytest.mark.parametrize("a,b,c,S", [(0.25, -0.1, 0.3, 100.0), (0.09, 0.05, 0.02, 31000.0), (0.5, -0.3, 1.0, 2.5)])
def test_anchor_parabola_in_log_strike(a, b, c, S):
    """w = tau (a + b x + c x^2), x = ln(k / S), rate 0.03: both stencils are exact, so w' = tau (b + 2 c x), w'' = 2 c tau,
    the tenor derivative is a + b x + c x^2 and N, g, local vol and density follow in closed form."""
    cs = AC.parabola_surface(a, b, c, S)
    r = restate(cs)
    f = _exact(LD)
    rate = f(cs["rate"])
    k, tau = cs["Kq"].astype(f)[None, None, :], cs["Tq"].astype(f)[None, :, None]
    x = np.log(k / f(S))
    p = f(a) + f(b) * x + f(c) * x * x
    w, w1, w2 = tau * p, tau * (f(b) + 2 * f(c) * x), 2 * f(c) * tau
    y = x - rate * tau
    N = p + rate * w1
    g = 1 - y / w * w1 + (-f(0.25) - 1 / w + y * y / (w * w)) * w1 * w1 / 4 + w2 / 2
    assert (N > 0).all() and (g > 0).all()
    d2 = -y / np.sqrt(w) - np.sqrt(w) / 2
    den = g * np.exp(-d2 * d2 / 2) / (k * np.sqrt(2 * f(np.pi) * w))
    _anchor(r, cs, N.astype(np.float64), g.astype(np.float64), np.sqrt(N / g).astype(np.float64), den.astype(np.float64))


def test_generators_stay_inside_the_margins():
    """What the GPU tests rely on (asserted by the restatement): |N| and |g| >= 1e-9 scale at every evaluated node and
    >= 90 % of the interior nodes evaluated; the rough surfaces carry both kinds of flag, the smooth ones do not kink."""
    for s in AC.GPU_SHAPES[::7] + [AC.ROUGH]:
        restate(AC.smooth(**s), margins=True)
    rough = restate(AC.smooth(**AC.ROUGH))["counts"].sum(0)
    assert rough[1] > 1000 and rough[2] > 1000 and rough[3] > 1000
    assert restate(AC.smooth(**AC.GPU_SHAPES[40]))["counts"][:, 2].sum() == 0


@pytest.mark.skipif(not HAS_LD, reason="np.longdouble has no extra precision here")
def test_rounding_level():
    """r = max |float64 - longdouble| / (eps scale) for N and g over the exact inputs the GPU tests use stays below the
    recorded R_CPU (the GPU tolerance is 8 R_CPU eps scale)."""
    worst = [0.0, 0.0]
    for s in AC.GPU_SHAPES + [AC.BIG, AC.ROUGH, AC.WHOLE]:
        c = AC.smooth(**s)
        a, b = restate(c), restate(c, dtype=LD)
        assert same(a["flags"], b["flags"]) and same(a["counts"], b["counts"])
        ev = a["evaluated"]
        if ev.any():
            worst[0] = max(worst[0], float(np.max(np.abs(a["N"][ev] - b["N"][ev]) / (EPS * b["N_scale"][ev]))))
            worst[1] = max(worst[1], float(np.max(np.abs(a["g"][ev] - b["g"][ev]) / (EPS * b["g_scale"][ev]))))
    print(f"rounding level: N {worst[0]:.3f}, g {worst[1]:.3f} (R_CPU = {AC.R_CPU})")
    assert max(worst) <= AC.R_CPU, worst


# ------------------------------------------------------------------ host layers with the restatement as the backend
def _built():
    chain = synthetic_chain("btc", expiry_days=(0.5, 3), strikes=tuple(np.linspace(17000.0, 34000.0, 12)), n_hours=3, seed=5)
    b = SnapshotSurfaceBuilder(backend=R.RefBackend(), moneyness=np.linspace(0.72, 1.28, 24), tenors=np.array([1.0, 2.0, 2.8]) / 365)
    return b, b.build(chain)


def test_arbitrage_report_and_frames():
    b, res = _built()
    reps = b.arbitrage(res, rate=0.01)
    assert len(reps) == len(res) == 1
    a, r = reps[0], res[0]
    assert a.underlying == "btc" and a.dates.equals(r.dates) and same(a.tenors, r.tenors) and same(a.moneyness, r.moneyness)
    assert a.rate == 0.01
    ref = R.restate(r.out, r.Kq, r.tenors, r.spot, 0.01)
    for k in ("flags", "counts", "worst", "local_vol", "density"):
        assert same(getattr(a, k), ref[k]), k
    keep = np.flatnonzero(np.asarray(r.quotes) > 0)
    assert len(keep) == 3 and ref["counts"][keep, 0].min() > 0
    assert (np.delete(ref["flags"], keep, axis=0) == R.DEAD).all()            # minutes without quotes: NaN surfaces

    s = arbitrage_frame(reps, res)
    assert list(s.columns) == ["underlying", "date", "spot", "evaluated", "calendar", "butterfly", "local_vol_nodes",
                               "min_numerator", "min_density_factor", "arbitrage_free"]
    assert [str(t) for t in s.dtypes] == ["object", str(s["date"].dtype), "float64", "int32", "int32", "int32", "int32", "float64",
                                          "float64", "bool"]
    assert len(s) == len(keep) and list(s["date"]) == list(r.dates[keep])
    assert same(s[["evaluated", "calendar", "butterfly", "local_vol_nodes"]].to_numpy(), ref["counts"][keep])
    assert same(s["min_numerator"].to_numpy(), ref["worst"][keep, 0]) and same(s["min_density_factor"].to_numpy(), ref["worst"][keep, 1])
    c = ref["counts"][keep]
    assert same(s["arbitrage_free"].to_numpy(), (c[:, 0] > 0) & (c[:, 1] == 0) & (c[:, 2] == 0))

    df = local_vol_frame(reps, res)
    assert list(df.columns) == ["underlying", "date", "spot", "tenor", "moneyness", "iv", "local_vol", "density", "flags"]
    assert str(df["flags"].dtype) == "int32" and len(df) == len(keep) * 3 * 24
    base = b.to_frame(res)
    for k in ("underlying", "date", "spot", "tenor", "moneyness", "iv"):                # to_frame's rows, in its order
        assert df[k].equals(base[k]), k
    assert same(df["local_vol"].to_numpy(), ref["local_vol"][keep].reshape(-1))
    assert same(df["density"].to_numpy(), ref["density"][keep].reshape(-1))
    assert same(df["flags"].to_numpy(), ref["flags"][keep].reshape(-1))
    assert len(arbitrage_frame([], [])) == 0 and len(local_vol_frame([], [])) == 0
    assert list(arbitrage_frame([], []).columns) == list(s.columns) and list(local_vol_frame([], []).columns) == list(df.columns)


def test_arbitrage_frame_verdict():
    """A8 on doctored counts: free needs evaluated > 0 and neither kind of violation."""
    b, res = _built()
    rep = b.arbitrage(res)[0]
    keep = np.flatnonzero(np.asarray(res[0].quotes) > 0)
    counts = np.array(rep.counts)
    counts[keep[0]] = [5, 0, 0, 5]
    counts[keep[1]] = [0, 0, 0, 0]
    counts[keep[2]] = [9, 0, 1, 8]
    rep.counts = counts
    assert list(arbitrage_frame([rep], res)["arbitrage_free"]) == [True, False, False]
    counts[keep[2]] = [9, 2, 0, 7]
    assert list(arbitrage_frame([rep], res)["arbitrage_free"]) == [True, False, False]


def test_arbitrage_task_end_to_end(tmp_path):
    import complete_pipeline as cp
    import snapshot_ref
    from oracle_backend import OracleBackend
    store = FrameStore(str(tmp_path))
    for f in synthetic_chain("btc", expiry_days=(0.5, 3), strikes=tuple(np.linspace(17000.0, 34000.0, 6)), n_hours=12, seed=5):
        store.write_source(f["symbol"].iloc[0], f)
    assert cp.main(["--task", "interpolation", "--data-dir", str(tmp_path)], backend=OracleBackend()) == 0
    assert cp.main(["--task", "arbitrage", "--data-dir", str(tmp_path)], surface_backend=R.RefBackend()) == 0
    assert store.read_table("iv_surfaces", "btc") is None and store.read_table("iv_smiles", "btc") is None
    out = store.read_table("iv_arbitrage", "btc")
    assert list(out.columns) == ["underlying", "date", "spot", "evaluated", "calendar", "butterfly", "local_vol_nodes",
                                 "min_numerator", "min_density_factor", "arbitrage_free"]
    frames = [store.read_output(s) for s in store.symbols("interpolated_trading_tickers")]
    ref, _ = snapshot_ref.restate(frames, M, TQ)
    r = ref["btc"]
    live = np.flatnonzero(r["quotes"] > 0)
    a = R.restate(r["out"], r["Kq"], TQ, r["spot"], 0.0)
    assert len(out) == len(live) == 661
    assert same(out[["evaluated", "calendar", "butterfly", "local_vol_nodes"]].to_numpy(), a["counts"][live])
    assert np.allclose(out["min_numerator"].to_numpy(), a["worst"][live, 0], rtol=1e-9, equal_nan=True)
    free = (a["counts"][live, 0] > 0) & (a["counts"][live, 1] == 0) & (a["counts"][live, 2] == 0)
    assert same(out["arbitrage_free"].to_numpy().astype(bool), free)
    pipe = cp.CompleteOptimizedPipeline(cp.get_config(), data_dir=str(tmp_path), surface_backend=R.RefBackend())
    res = pipe.run_arbitrage()
    assert res["success"] and res["underlyings"] == 1 and res["rows"] == len(out)
    assert res["arbitrage_free_snapshots"] == int(free.sum())


# ------------------------------------------------------------------ C ABI validation, no device needed
def _args(**kw):
    P = 64
    a = _lib.ArbitrageArgs()
    a.vol, a.Kq, a.Tq, a.spot = (kw.get(k, P) for k in ("vol", "Kq", "Tq", "spot"))
    a.kq_stride, a.tq_stride, a.rate = kw.get("kq_stride", 0), kw.get("tq_stride", 0), 0.0
    a.mK, a.mT, a.B = kw.get("mK", 64), kw.get("mT", 16), kw.get("B", 1)
    a.flags, a.counts, a.worst = (kw.get(k, P) for k in ("flags", "counts", "worst"))
    a.local_vol, a.density = kw.get("local_vol", P), kw.get("density", P)
    return a


def test_abi_validation_codes_without_gpu():
    """Host-side validation returns errno-style codes before any launch (the fake pointers are never dereferenced)."""
    lib = _lib.load()
    assert _lib.ABI_VERSION == 5 == lib.ivs_version()                                           # the symbol is additive
    call = lambda **kw: lib.ivs_surface_arbitrage_f64(C.byref(_args(**kw)), None, 0, None)   # noqa: E731
    assert lib.ivs_surface_arbitrage_f64(None, None, 0, None) == -22 and b"null args" in lib.ivs_last_error()
    for k in ("vol", "Kq", "Tq", "spot", "flags", "counts", "worst"):
        assert call(**{k: None}) == -22 and b"null pointer" in lib.ivs_last_error(), k
    assert call(B=-1) == -22 and call(mT=-1) == -22 and call(mK=-1) == -22 and call(kq_stride=-1) == -22 and call(tq_stride=-1) == -22
    assert b"negative" in lib.ivs_last_error()
    for bad in (63, 65, 1, 128):
        assert call(kq_stride=bad) == -22 and b"stride" in lib.ivs_last_error(), bad
    for bad in (15, 17, 1, 64):
        assert call(tq_stride=bad) == -22 and b"stride" in lib.ivs_last_error(), bad
    assert call(mK=2) == -34 and b"mK=2" in lib.ivs_last_error() and call(mK=0) == -34           # IVS_ERANGE
    assert call(mT=1) == -34 and b"mT=1" in lib.ivs_last_error() and call(mT=0) == -34
    assert call(B=1 << 27, mT=16) == -34 and b"134217728 x 16 rows" in lib.ivs_last_error()     # B * mT = 2^31
    assert call(B=1 << 40, mT=2) == -34
    assert call(B=0) == 0 and call(B=0, vol=None, flags=None) == 0 and lib.ivs_last_error() == b""   # empty: a no-op
    assert call(B=0, mK=2) == -34                                                               # the shape is checked first
    assert (_lib.AR_CALENDAR, _lib.AR_BUTTERFLY, _lib.AR_NO_STENCIL, _lib.AR_DEAD) == (R.CALENDAR, R.BUTTERFLY, R.NO_STENCIL, R.DEAD) == (1, 2, 4, 8)


def test_stale_library_is_reported(tmp_path, monkeypatch):
    """A libivs.so without the new symbol raises EngineUnavailable with a message that says to rebuild."""
    class Old:
        def __getattr__(self, name):
            if name == "ivs_surface_arbitrage_f64":
                raise AttributeError(name)
            return lambda *a: _lib.ABI_VERSION
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.C, "CDLL", lambda path: Old())
    with pytest.raises(_lib.EngineUnavailable, match="ivs_surface_arbitrage_f64.*rebuild"):
        _lib.load()
