"""GPU: surface_arbitrage_kernel (ivs_surface_arbitrage_f64) against the NumPy restatement of rules A1-A7
(tests/arb_ref.py): equal flags and counts, equal NaN pattern, and N, g, worst, local vol and density within
C eps scale with C = 8 R_CPU (tests/arb_cases.py; DESIGN.md section 10 has the reasoning).  N and g are not outputs of
the kernel: they are held through `worst` (their minima) and through local vol = sqrt(N / g) and density = g x lognormal.

Every test prints its largest error / tolerance ratios; with IVS_ARB_ERRLOG=<file> set the figures are appended to that
file as well (a recorded run belongs in profiles/arbitrage/errlog.txt)."""
import os

import numpy as np
import pytest

import arb_cases as AC
import arb_ref as R

pytestmark = pytest.mark.gpu
EPS, C = AC.EPS, AC.C_GPU
SENT_F, SENT_I = -7.25, -77          # no output of the rules: local vol >= 0, flags / counts >= 0; density and worst never hit it


def log(name, **figures):
    line = name + ": " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items())
    print(line)
    path = os.environ.get("IVS_ARB_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def host(t):
    return None if t is None else t.cpu().numpy()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()


def run(c, local_vol=True, density=True, stream=None, raw=False):
    """One call with every output pre-filled with a sentinel; asserts that every element was overwritten."""
    import torch
    from iv_interpolation_amd import engine
    B, mT, mK = c["vol"].shape
    out = {"flags": torch.full((B, mT, mK), SENT_I, dtype=torch.int32, device="cuda"),
           "counts": torch.full((B, 4), SENT_I, dtype=torch.int32, device="cuda"),
           "worst": torch.full((B, 2), SENT_F, dtype=torch.float64, device="cuda"),
           "local_vol": torch.full((B, mT, mK), SENT_F, dtype=torch.float64, device="cuda"),
           "density": torch.full((B, mT, mK), SENT_F, dtype=torch.float64, device="cuda")}
    q = engine.surface_arbitrage(dev(c["vol"]), dev(c["Kq"]), dev(c["Tq"]), dev(c["spot"]), c.get("rate", 0.0),
                                 local_vol=local_vol, density=density, out=out, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    got = {k: host(v) for k, v in q.items()}
    for k, v in got.items():
        if v is not None:
            assert not (v == (SENT_I if v.dtype == np.int32 else SENT_F)).any(), f"{k}: an element was not written"
    if not local_vol:
        assert (host(out["local_vol"]) == SENT_F).all(), "local_vol was written although it was not requested"
    if not density:
        assert (host(out["density"]) == SENT_F).all(), "density was written although it was not requested"
    return (got, out) if raw else got


def compare(name, got, ref):
    """Flags, counts and NaN patterns equal; values within the tolerances of the module docstring."""
    ev = ref["evaluated"]
    assert got["flags"].dtype == np.int32 and got["counts"].dtype == np.int32
    flags_ok, counts_ok = np.array_equal(got["flags"], ref["flags"]), np.array_equal(got["counts"], ref["counts"])
    with np.errstate(all="ignore"):
        tol_N, tol_g = C * EPS * ref["N_scale"], C * EPS * ref["g_scale"]
        lv, den = ref["local_vol"], ref["density"]
        tol_lv = lv * (0.5 * (tol_N / np.abs(ref["N"]) + tol_g / np.abs(ref["g"])) + C * EPS)
        tol_den = np.abs(den) * (tol_g / np.abs(ref["g"]) + C * EPS * (1 + ref["d2"] ** 2))
        fig = {}
        for k, tol in (("local_vol", tol_lv), ("density", tol_den)):
            if got.get(k) is not None:
                e = np.abs(got[k] - ref[k]) / tol
                fig[k] = float(np.nanmax(e)) if np.isfinite(e).any() else 0.0
        # worst: the restatement's minimum sits at some node; the device's minimum may sit at another one whose value is
        # within its own tolerance of it, so the bound is the largest tolerance among the nodes that could be the minimum
        B = ev.shape[0]
        fig["worst_N"] = fig["worst_g"] = 0.0
        for q, (key, tol) in enumerate((("N", tol_N), ("g", tol_g))):
            for b in range(B):
                if ref["counts"][b, 0] == 0:
                    continue
                v, t = ref[key][b][ev[b]], tol[b][ev[b]]
                near = v - t <= ref["worst"][b, q] + t[np.argmin(v)]
                fig["worst_" + key] = max(fig["worst_" + key], float(abs(got["worst"][b, q] - ref["worst"][b, q]) / t[near].max()))
    log(name, **fig, evaluated=int(ev.sum()), nodes=int(ev.size), calendar=int(ref["counts"][:, 1].sum()),
        butterfly=int(ref["counts"][:, 2].sum()))
    assert flags_ok, name
    assert counts_ok, (name, got["counts"][:4], ref["counts"][:4])
    assert np.array_equal(np.isnan(got["worst"]), np.isnan(ref["worst"])), name
    for k in ("local_vol", "density"):
        if got.get(k) is not None:
            assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (name, k)
    assert all(v <= 1.0 for v in fig.values()), (name, fig)


_cache = {}


def case(key, spec):
    """Inputs and restatement of one generated surface batch, computed once and shared (read-only)."""
    if key not in _cache:
        c = AC.smooth(**spec)
        ref = R.restate(c["vol"], c["Kq"], c["Tq"], c["spot"], c["rate"], margins=True)
        for a in list(c.values()) + list(ref.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = (c, ref)
    return _cache[key]


@pytest.mark.parametrize("name", sorted(AC.CASES))
def test_micro_case(name):
    c = AC.CASES[name]
    got = run(c)
    assert np.array_equal(got["flags"], c["flags"]), got["flags"]
    assert np.array_equal(got["counts"], c["counts"]), got["counts"]
    compare(f"micro[{name}]", got, R.restate(c["vol"], c["Kq"], c["Tq"], c["spot"], c["rate"]))


def test_shared_and_per_snapshot_grids_agree_bitwise():
    shared, spelled = AC.shared_and_spelled()
    a, b = run(shared), run(spelled)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    compare("shared_vs_per_snapshot", a, R.restate(shared["vol"], shared["Kq"], shared["Tq"], shared["spot"], shared["rate"], margins=True))


@pytest.mark.parametrize("n", range(len(AC.GPU_SHAPES)), ids=[AC.shape_id(s) for s in AC.GPU_SHAPES])
def test_shapes(n):
    c, ref = case(n, AC.GPU_SHAPES[n])
    compare(f"shape[{AC.shape_id(AC.GPU_SHAPES[n])}]", run(c), ref)


def test_rough_surfaces_carry_every_flag():
    """3 % noise kinks the smiles: thousands of CALENDAR and BUTTERFLY nodes, NaN local vols next to finite ones."""
    c, ref = case("rough", AC.ROUGH)
    assert ref["counts"][:, 1].sum() > 1000 and ref["counts"][:, 2].sum() > 1000 and (ref["flags"] == 3).any()
    compare("rough[33-16-65]", run(c), ref)


def test_big_batch_is_reproducible_and_outputs_are_optional():
    """512 surfaces of 16 x 64: two calls give identical bits; with local_vol / density left out the flags and the report
    are the same bits and the buffer left out keeps its sentinel (checked inside run)."""
    c, ref = case("big", AC.BIG)
    a = run(c)
    compare("big[512-16-64]", a, ref)
    b = run(c)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    for lv, den in ((False, True), (True, False), (False, False)):
        part = run(c, local_vol=lv, density=den)
        assert (part["local_vol"] is None) == (not lv) and (part["density"] is None) == (not den)
        for k in a:
            if part[k] is not None:
                assert np.array_equal(a[k], part[k], equal_nan=True), (k, lv, den)


def test_whole_snapshot_strips_and_partition_independence():
    """4200 narrow snapshots: enough for one wavefront to walk all 16 rows of a snapshot.  The same snapshots sent seven at
    a time are cut into strips of four rows instead: the bits must not depend on the cut."""
    c, ref = case("whole", AC.WHOLE)
    got = run(c)
    compare("whole[4200-16-3]", got, ref)
    few = run({k: (v[:7] if isinstance(v, np.ndarray) and v.shape[:1] == (4200,) else v) for k, v in c.items()})
    for k in got:
        assert np.array_equal(got[k][:7], few[k], equal_nan=True), k


def test_explicit_stream_then_immediate_reallocation():
    """The call runs on an explicit stream while another stream is current; its inputs are temporaries that die when the
    call returns, and tensors of the same sizes are allocated and filled on the current stream at once.  The allocator must
    not hand the inputs' blocks out while the kernel still reads them (record_stream), so the results are the usual bits."""
    import torch
    from iv_interpolation_amd import engine
    c, ref = case("big", AC.BIG)
    base = run(c)
    s = torch.cuda.Stream()
    with torch.cuda.stream(torch.cuda.Stream()):
        q = engine.surface_arbitrage(dev(c["vol"]), dev(c["Kq"]), dev(c["Tq"]), dev(c["spot"]), c["rate"], stream=s)
        junk = [torch.full(c["vol"].shape, 3.0, dtype=torch.float64, device="cuda") for _ in range(4)]
        junk += [torch.full(x.shape, 3.0, dtype=torch.float64, device="cuda") for x in (c["Kq"], c["Tq"], c["spot"])]
        s.synchronize()
        torch.cuda.synchronize()
    assert engine.last_kernel() == "surface_arbitrage_kernel"
    for k in base:
        assert np.array_equal(host(q[k]), base[k], equal_nan=True), k
    del junk


def test_shape_and_dtype_checks():
    import torch
    from iv_interpolation_amd import _lib, engine
    c, _ = case(0, AC.GPU_SHAPES[0])
    v, k, t, s = dev(c["vol"]), dev(c["Kq"]), dev(c["Tq"]), dev(c["spot"])
    with pytest.raises(ValueError):
        engine.surface_arbitrage(v[0], k, t, s)
    with pytest.raises(ValueError):
        engine.surface_arbitrage(v, k[..., :-1], t, s)
    with pytest.raises(ValueError):
        engine.surface_arbitrage(v, k, t, torch.cat([s, s]))
    with pytest.raises(TypeError):
        engine.surface_arbitrage(v.float(), k, t, s)
    with pytest.raises(ValueError):
        engine.surface_arbitrage(v, k, t, s, out={"flags": torch.empty(v.shape, dtype=torch.float64, device="cuda")})
    with pytest.raises(_lib.EngineError, match="mT=1"):
        engine.surface_arbitrage(v[:, :1].contiguous(), k, t[..., :1].contiguous(), s)


def test_builder_and_frames_on_a_wide_chain():
    """End to end: a chain through build() and arbitrage() on the device, against the restatement applied to the host
    copy of `out`; the linear surfaces of a noisy chain do violate, which is what the report is for."""
    import snapshot_cases as SC
    from iv_interpolation_amd.snapshots import HipBackend, SnapshotSurfaceBuilder, arbitrage_frame, local_vol_frame
    frame = SC.big_chain(n_und=2, nT=4, nK=24, minutes=40, seed=4)
    mny, ten = np.linspace(0.72, 1.28, 64), np.linspace(8.0, 20.0, 6) / 365.0
    b = SnapshotSurfaceBuilder(moneyness=mny, tenors=ten, backend=HipBackend())
    res = b.build(frame)
    reps = b.arbitrage(res, rate=0.01)
    assert [a.underlying for a in reps] == ["btc", "eth"]
    for a, r in zip(reps, res):
        ref = R.restate(host(r.out), host(r.Kq), ten, host(r.spot), 0.01)
        assert ref["evaluated"][:, :, 1:-1].mean() >= 0.9
        near = ((np.abs(ref["N"]) < R.MARGIN * ref["N_scale"]) | (np.abs(ref["g"]) < R.MARGIN * ref["g_scale"])).sum()
        assert near == 0, "a node of this chain sits on a flag threshold: pick another seed"
        compare(f"builder[{a.underlying}]", {k: host(getattr(a, k)) for k in ("flags", "counts", "worst", "local_vol", "density")}, ref)
    s, lv = arbitrage_frame(reps, res), local_vol_frame(reps, res)
    assert len(s) == 80 and len(lv) == 80 * 6 * 64 and set(s["underlying"]) == {"btc", "eth"}
    assert s["evaluated"].min() > 0 and lv["flags"].isin([0, 1, 2, 3, 4, 8]).all()
