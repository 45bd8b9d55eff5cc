"""GPU: surface_moments_kernel (ivs_surface_moments_f64) against the restatement of rules M1-M7 (tests/mm_ref.py): equal
flags and NaN pattern; raw within C eps raw_scale with C = 8 R_CPU (tests/mm_cases.py; DESIGN.md section 11 has the
reasoning); stats and index within rules M6 / M7 applied in NumPy to the restatement's raw moments, the raw tolerances
carried through the formulas; mass within C eps (1 + d2^2) per Phi.

Every test prints its largest error / tolerance ratios; with IVS_MM_ERRLOG=<file> set the figures are appended to that file
as well (a recorded run belongs in profiles/moments/errlog.txt)."""
import ctypes
import os

import numpy as np
import pytest

import mm_cases as MC
import mm_ref as R

pytestmark = pytest.mark.gpu
EPS, C = MC.EPS, MC.C_GPU
SENT_F, SENT_I = -7.25, -77          # no output of the rules: flags >= 0; no moment, statistic, mass or index ever hits -7.25
KEYS = ("raw", "stats", "mass", "flags", "index", "index_flags")


def log(name, **figures):
    line = name + ": " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items())
    print(line)
    path = os.environ.get("IVS_MM_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def host(t):
    return None if t is None else t.cpu().numpy()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()


def sentinels(B, mT, nH):
    import torch
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")  # noqa: E731
    return {"raw": full((B, mT, 4), SENT_F, torch.float64), "stats": full((B, mT, 4), SENT_F, torch.float64),
            "mass": full((B, mT), SENT_F, torch.float64), "flags": full((B, mT), SENT_I, torch.int32),
            "index": full((B, nH), SENT_F, torch.float64), "index_flags": full((B, nH), SENT_I, torch.int32)}


def run(c, stream=None, spw=0, horizons=None):
    """One call with every output pre-filled with a sentinel; asserts that every element was overwritten."""
    import torch
    from iv_interpolation_amd import engine
    B, mT, _ = c["vol"].shape
    hz = c["horizons"] if horizons is None else horizons
    out = sentinels(B, mT, len(hz))
    if not hz:
        out.pop("index"), out.pop("index_flags")
    q = engine.surface_moments(dev(c["vol"]), dev(c["Kq"]), dev(c["Tq"]), dev(c["spot"]), c["rate"], horizons=hz,
                               min_mass=c["min_mass"], out=out, stream=stream, snapshots_per_wg=spw)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    assert engine.last_kernel() == "surface_moments_kernel"
    got = {k: host(v) for k, v in q.items()}
    for k, v in got.items():
        if v is not None:
            assert not (v == (SENT_I if v.dtype == np.int32 else SENT_F)).any(), f"{k}: an element was not written"
    return got


def reference(c, margins=False):
    return R.restate(c["vol"], c["Kq"], c["Tq"], c["spot"], c["rate"], c["horizons"], c["min_mass"], margins=margins)


def compare(name, got, ref, c):
    """Flags and NaN patterns equal; values within the tolerances of the module docstring."""
    tol = R.tolerances(ref, c["Tq"], c["horizons"], C, EPS)
    assert got["flags"].dtype == np.int32
    fig = {}
    with np.errstate(all="ignore"):
        for k in ("raw", "stats", "mass") + (("index",) if c["horizons"] else ()):
            e = np.abs(got[k] - ref[k]) / tol[k]
            if k in ("raw", "stats"):
                for m, nm in enumerate(("L", "V", "W", "X") if k == "raw" else ("mf_vol", "bkm_vol", "skew", "kurt")):
                    fig[nm] = float(np.nanmax(e[..., m])) if np.isfinite(e[..., m]).any() else 0.0
            else:
                fig[k] = float(np.nanmax(e)) if np.isfinite(e).any() else 0.0
    live = ref["flags"] != R.DEAD
    log(name, **fig, rows=int(live.size), live=int(live.sum()), flagged=int((ref["flags"][live] != 0).sum()),
        no_bracket=int((ref["index_flags"] == R.NO_BRACKET).sum()))
    assert np.array_equal(got["flags"], ref["flags"]), (name, got["flags"][:2], ref["flags"][:2])
    for k in ("raw", "stats", "mass"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (name, k)
    if c["horizons"]:
        assert got["index_flags"].dtype == np.int32 and np.array_equal(got["index_flags"], ref["index_flags"]), name
        assert np.array_equal(np.isnan(got["index"]), np.isnan(ref["index"])), name
    assert all(v <= 1.0 for v in fig.values()), (name, fig)


_cache = {}


def case(n):
    """Inputs and restatement of one generated batch, computed once and shared (read-only)."""
    if n not in _cache:
        c = MC.smooth(**MC.SHAPES[n])
        ref = reference(c, margins=True)
        for a in list(c.values()) + list(ref.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[n] = (c, ref)
    return _cache[n]


def shape_index(B, mT, mK, per_kq):
    return next(n for n, s in enumerate(MC.SHAPES) if (s["B"], s["mT"], s["mK"], s["per_kq"]) == (B, mT, mK, per_kq))


@pytest.mark.parametrize("name", sorted(MC.MICRO))
def test_micro_case(name):
    c = MC.MICRO[name]
    got = run(c)
    assert np.array_equal(got["flags"], c["flags"]), got["flags"]
    assert np.array_equal(got["index_flags"], c["index_flags"]), got["index_flags"]
    compare(f"micro[{name}]", got, reference(c), c)


@pytest.mark.parametrize("n", range(len(MC.SHAPES)), ids=[MC.shape_id(s) for s in MC.SHAPES])
def test_shapes(n):
    c, ref = case(n)
    compare(f"shape[{MC.shape_id(MC.SHAPES[n])}]", run(c), ref, c)


@pytest.mark.parametrize("name", sorted(MC.EDGE))
def test_forward_node_at_the_chunk_edge(name):
    """mK = 130: the segment that straddles the forward is the one carried from the first 64-strike chunk into the second
    (or, with the forward on node 63 / 64, no segment at all)."""
    c, holes = MC.EDGE[name]
    ref = reference(c, margins=True)
    assert ((ref["flags"] & R.HOLES) == holes).all()
    compare(f"edge[{name}]", run(c), ref, c)


def test_partition_independence():
    """B = 5 snapshots with snapshots_per_wg = 1, 2, 4 and 0: identical bits (5 is a multiple of none of them, so the last
    workgroup is partly empty)."""
    n = shape_index(5, 3, 65, True)
    c, ref = case(n)
    base = run(c, spw=0)
    compare("partition[spw=0]", base, ref, c)
    for spw in (1, 2, 4):
        got = run(c, spw=spw)
        for k in KEYS:
            assert np.array_equal(base[k], got[k], equal_nan=True), (k, spw)


def test_shared_and_per_snapshot_grids_agree_bitwise():
    c, ref = case(shape_index(3, 16, 64, False))
    spelled = dict(c, Kq=np.tile(c["Kq"], (3, 1)), Tq=np.tile(c["Tq"], (3, 1)))
    a, b = run(c), run(spelled)
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_explicit_stream_then_immediate_reallocation():
    """The call runs on an explicit stream while another stream is current; its inputs are temporaries that die when the
    call returns, and tensors of the same sizes are allocated and filled on the current stream at once.  The allocator must
    not hand the inputs' blocks out while the kernel still reads them (record_stream), so the results are the usual bits."""
    import torch
    from iv_interpolation_amd import engine
    c, ref = case(shape_index(64, 16, 64, True))
    base = run(c)
    on_stream = run(c, stream=torch.cuda.Stream())
    for k in KEYS:
        assert np.array_equal(base[k], on_stream[k], equal_nan=True), k
    s = torch.cuda.Stream()
    with torch.cuda.stream(torch.cuda.Stream()):
        q = engine.surface_moments(dev(c["vol"]), dev(c["Kq"]), dev(c["Tq"]), dev(c["spot"]), c["rate"], horizons=c["horizons"],
                                   stream=s)
        junk = [torch.full(c["vol"].shape, 3.0, dtype=torch.float64, device="cuda") for _ in range(4)]
        junk += [torch.full(x.shape, 3.0, dtype=torch.float64, device="cuda") for x in (c["Kq"], c["Tq"], c["spot"])]
        s.synchronize()
        torch.cuda.synchronize()
    for k in KEYS:
        assert np.array_equal(host(q[k]), base[k], equal_nan=True), k
    del junk


def test_horizon_counts():
    """nH == 0: no M7, the call returns no index and a buffer passed through the C ABI keeps its sentinel; nH == 8: every
    horizon of every snapshot is written and agrees with the restatement."""
    import torch
    from iv_interpolation_amd import _lib, engine
    c, ref = case(shape_index(3, 16, 64, False))                                       # shared grids: tenors 5 .. 90 days
    none = run(c, horizons=())
    assert none["index"] is None and none["index_flags"] is None
    for k in ("raw", "stats", "mass", "flags"):
        assert np.array_equal(none[k], run(c)[k], equal_nan=True), k
    B, mT, mK = c["vol"].shape
    out = sentinels(B, mT, 8)
    vol, Kq, Tq, spot = dev(c["vol"]), dev(c["Kq"]), dev(c["Tq"]), dev(c["spot"])
    a = _lib.MomentsArgs()
    a.vol, a.Kq, a.kq_stride, a.Tq, a.tq_stride, a.spot = vol.data_ptr(), Kq.data_ptr(), 0, Tq.data_ptr(), 0, spot.data_ptr()
    a.rate, a.min_mass, a.horizons, a.nH = c["rate"], c["min_mass"], ctypes.POINTER(ctypes.c_double)(), 0
    a.mK, a.mT, a.B = mK, mT, B
    a.raw, a.stats, a.mass, a.flags = (out[k].data_ptr() for k in ("raw", "stats", "mass", "flags"))
    a.index, a.index_flags = out["index"].data_ptr(), out["index_flags"].data_ptr()
    _lib.check(_lib.load().ivs_surface_moments_f64(a, None, 0, torch.cuda.current_stream().cuda_stream), "ivs_surface_moments_f64")
    torch.cuda.synchronize()
    assert (host(out["index"]) == SENT_F).all() and (host(out["index_flags"]) == SENT_I).all(), "index was touched with nH == 0"
    assert np.array_equal(host(out["raw"]), none["raw"], equal_nan=True)
    hz = tuple(d / 365.0 for d in (3.0, 7.0, 14.0, 30.0, 45.0, 60.0, 89.0, 120.0))     # 3 and 120 days lie outside the tenors
    c8 = dict(c, horizons=hz)
    ref8 = reference(c8)
    assert (ref8["index_flags"][:, [0, 7]] == R.NO_BRACKET).all() and np.isfinite(ref8["index"][:, 1:7]).all()
    compare("horizons[8]", run(c8), ref8, c8)
    with pytest.raises(ValueError, match="horizons"):
        engine.surface_moments(vol, Kq, Tq, spot, horizons=tuple([0.1] * 9))


def test_shape_and_dtype_checks():
    import torch
    from iv_interpolation_amd import _lib, engine
    c, _ = case(shape_index(3, 16, 64, True))
    v, k, t, s = dev(c["vol"]), dev(c["Kq"]), dev(c["Tq"]), dev(c["spot"])
    with pytest.raises(ValueError):
        engine.surface_moments(v[0], k, t, s)
    with pytest.raises(ValueError):
        engine.surface_moments(v, k[..., :-1], t, s)
    with pytest.raises(ValueError):
        engine.surface_moments(v, k, t, torch.cat([s, s]))
    with pytest.raises(TypeError):
        engine.surface_moments(v.float(), k, t, s)
    with pytest.raises(ValueError):
        engine.surface_moments(v, k, t, s, out={"flags": torch.empty(v.shape[:2], dtype=torch.float64, device="cuda")})
    with pytest.raises(ValueError, match="min_mass"):
        engine.surface_moments(v, k, t, s, min_mass=1.5)
    with pytest.raises(ValueError, match="horizons"):
        engine.surface_moments(v, k, t, s, horizons=(0.0,))
    with pytest.raises(_lib.EngineError, match="mK=1"):
        engine.surface_moments(v[:, :, :1].contiguous(), k[..., :1].contiguous(), t, s)
    with pytest.raises(_lib.EngineError, match="snapshots_per_wg=5"):
        engine.surface_moments(v, k, t, s, snapshots_per_wg=5)


def test_builder_and_frames_on_a_wide_chain():
    """End to end: the chain of the arbitrage GPU test through build() and moments() on the device, against the
    restatement applied to the host copy of `out`."""
    import snapshot_cases as SC
    from iv_interpolation_amd.snapshots import HipBackend, SnapshotSurfaceBuilder, moments_frame, volindex_frame
    frame = SC.big_chain(n_und=2, nT=4, nK=24, minutes=40, seed=4)
    mny, ten = np.linspace(0.72, 1.28, 64), np.linspace(8.0, 20.0, 6) / 365.0
    hz = (10.0 / 365.0, 15.0 / 365.0, 30.0 / 365.0)
    b = SnapshotSurfaceBuilder(moneyness=mny, tenors=ten, backend=HipBackend())
    res = b.build(frame)
    reps = b.moments(res, rate=0.01, horizons=hz, min_mass=0.9)
    assert [m.underlying for m in reps] == ["btc", "eth"]
    for m, r in zip(reps, res):
        c = dict(vol=host(r.out), Kq=host(r.Kq), Tq=ten, spot=host(r.spot), rate=0.01, horizons=hz, min_mass=0.9)
        ref = reference(c, margins=True)
        assert np.isfinite(ref["index"][:, :2]).all() and (ref["index_flags"][:, 2] == R.NO_BRACKET).all()
        compare(f"builder[{m.underlying}]", {k: host(getattr(m, k)) for k in KEYS}, ref, c)
    f, v = moments_frame(reps, res), volindex_frame(reps, res)
    assert len(f) == 80 * 6 and len(v) == 80 and set(v["underlying"]) == {"btc", "eth"}
    assert list(v.columns) == ["underlying", "date", "spot", "vix_10d", "flags_10d", "vix_15d", "flags_15d", "vix_30d", "flags_30d"]
    assert v["vix_10d"].between(5.0, 300.0).all() and v["vix_30d"].isna().all() and (f["flags"] != R.DEAD).all()
