"""GPU: svi_distribution_kernel (ivs_svi_distribution_f64) against the restatement of rules P1-P8 (tests/dist_ref.py).

Flags and every NaN pattern equal the restatement's everywhere (the generated batches keep every comparison of the rules off
its threshold: dist_ref.check_margins).  The values agree within C_GPU x R_CPU units of eps x the rule's own scale
(dist_cases.tolerances; DESIGN.md section 13 has the reasoning): R_CPU is the restatement's distance from the same rules in
mpmath at 50 digits, measured by test_distribution.test_rounding_level.

Every test prints its largest error / tolerance ratios; with IVS_DS_ERRLOG=<file> set the figures are appended to that file
as well (a recorded run belongs in profiles/distribution/errlog_gpu.txt; errlog.txt there holds the CPU run)."""
import os

import numpy as np
import pytest

import dist_cases as DC
import dist_ref as R

pytestmark = pytest.mark.gpu
SENT_F, SENT_I = -7.25e9, -77        # no output of the rules: flags >= 0; no probability, ln(K/F) or strike ever hits -7.25e9
KEYS = ("q_x", "q_strike", "q_flags", "p_below", "p_above", "tails", "flags")
GPU_FACTOR = {k: DC.C_GPU * v for k, v in DC.R_CPU.items()}


def log(name, **figures):
    line = name + ": " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items())
    print(line)
    path = os.environ.get("IVS_DS_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def host(t):
    return None if t is None else t.cpu().numpy()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()


def sentinels(B, mT, nP, nL):
    import torch
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")  # noqa: E731
    out = {"q_x": full((B, mT, nP), SENT_F, torch.float64), "q_strike": full((B, mT, nP), SENT_F, torch.float64),
           "q_flags": full((B, mT, nP), SENT_I, torch.int32), "tails": full((B, mT, 2), SENT_F, torch.float64),
           "flags": full((B, mT), SENT_I, torch.int32)}
    if nL:
        out["p_below"], out["p_above"] = full((B, mT, nL), SENT_F, torch.float64), full((B, mT, nL), SENT_F, torch.float64)
    return out


def run(c, stream=None, rpw=0, params=None):
    """One call with every output pre-filled with a sentinel; asserts that every element was overwritten."""
    import torch
    from iv_interpolation_amd import engine
    B, mT, _ = c["params"].shape
    out = sentinels(B, mT, len(c["probs"]), len(c["levels"]))
    q = engine.svi_distribution(dev(c["params"]) if params is None else params, dev(c["Tq"]), dev(c["spot"]), c["rate"],
                                probs=c["probs"], levels=c["levels"], max_tail=c["max_tail"], out=out, stream=stream, rows_per_wave=rpw)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    assert engine.last_kernel() == "svi_distribution_kernel"
    got = {k: host(v) for k, v in q.items()}
    assert set(got) == set(KEYS)
    for k, v in got.items():
        if v is not None:
            assert not (v == (SENT_I if v.dtype == np.int32 else SENT_F)).any(), f"{k}: an element was not written"
    assert (got["p_below"] is None) == (len(c["levels"]) == 0) == (got["p_above"] is None)
    return got


def reference(c, margins=False):
    return R.restate(c["params"], c["Tq"], c["spot"], c["rate"], c["probs"], c["levels"], c["max_tail"], margins=margins)


def compare(name, got, ref, c):
    assert got["flags"].dtype == np.int32 and got["q_flags"].dtype == np.int32
    u = DC.units(got, ref, c)
    fig = {k: (float(np.nanmax(v)) / GPU_FACTOR[DC.UNIT_KEY[k]] if np.isfinite(v).any() else 0.0) for k, v in u.items()}
    log(name, **fig, rows=int(ref["live"].size), live=int(ref["live"].sum()), bracketed=int((ref["bracket"] >= 0).sum()),
        targets=int(ref["bracket"].size))
    assert np.array_equal(got["flags"], ref["flags"]), (name, got["flags"], ref["flags"])
    assert np.array_equal(got["q_flags"], ref["q_flags"]), (name, got["q_flags"], ref["q_flags"])
    for k in u:
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (name, k)
    assert all(v <= 1.0 for v in fig.values()), (name, fig)


def same_bits(a, b, what):
    for k in KEYS:
        if a[k] is None:
            assert b[k] is None, (k, what)
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), (k, what)


_cache = {}


def case(n):
    """Inputs and restatement of one generated batch, computed once and shared (read-only)."""
    if n not in _cache:
        c = DC.batch(**DC.SHAPES[n])
        ref = reference(c, margins=True)
        for a in list(c.values()) + list(ref.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[n] = (c, ref)
    return _cache[n]


def shape_index(B, mT, nP, per_tq):
    return next(n for n, s in enumerate(DC.SHAPES) if (s["B"], s["mT"], s["nP"], s["per_tq"]) == (B, mT, nP, per_tq))


@pytest.mark.parametrize("name", sorted(DC.MICRO))
def test_micro_case(name):
    c = DC.MICRO[name]
    got = run(c)
    assert np.array_equal(got["flags"], c["flags"]), got["flags"]
    assert np.array_equal(got["q_flags"], c["q_flags"]), got["q_flags"]
    compare(f"micro[{name}]", got, reference(c), c)


@pytest.mark.parametrize("n", range(len(DC.SHAPES)), ids=[DC.shape_id(s) for s in DC.SHAPES])
def test_shapes(n):
    """Every (B, mT) x nP of the table, with nL = 0 (NULL level outputs), 5 and 16, shared tenors at rate 0 and per-snapshot
    tenors at rate 0.03."""
    c, ref = case(n)
    compare(f"shape[{DC.shape_id(DC.SHAPES[n])}]", run(c), ref, c)


@pytest.mark.parametrize("B,mT,nP", [(3, 2, 5), (4, 3, 5), (2, 13, 5), (5, 3, 16), (3, 16, 7), (64, 1, 1)])
def test_partition_independence(B, mT, nP):
    """rows_per_wave forced to 1, to every other legal value and left at 0: identical bits.  The launcher picks 1 on batches
    this small, so the forced values are what runs (4, 3, 5) as one filled wavefront of 12 rows, (2, 13, 5) as 12 + 12 + 2."""
    c, ref = case(shape_index(B, mT, nP, True))
    base = run(c, rpw=0)
    compare(f"partition[B{B}-mT{mT}-nP{nP}, rpw=0]", base, ref, c)
    for rpw in range(1, 64 // nP + 1):
        same_bits(base, run(c, rpw=rpw), rpw)


def test_shared_and_per_snapshot_tenors_agree_bitwise():
    c, _ = case(shape_index(3, 16, 7, False))
    same_bits(run(c), run(dict(c, Tq=np.tile(c["Tq"], (3, 1)))), "tq")


def test_levels_left_out():
    """nL = 0 through the C ABI with buffers lying next to the call's outputs: NULL p_below / p_above, neither is touched, and
    the other outputs keep the bits of a call with levels."""
    import ctypes
    import torch
    from iv_interpolation_amd import _lib
    c, _ = case(shape_index(3, 16, 7, False))
    full, none = run(c), run(dict(c, levels=()))
    assert none["p_below"] is None and none["p_above"] is None
    for k in ("q_x", "q_strike", "q_flags", "tails", "flags"):
        assert np.array_equal(none[k], full[k], equal_nan=True), k
    B, mT, _ = c["params"].shape
    nP = len(c["probs"])
    out = sentinels(B, mT, nP, 5)
    params, Tq, spot = dev(c["params"]), dev(c["Tq"]), dev(c["spot"])
    pbuf = (ctypes.c_double * nP)(*c["probs"])
    a = _lib.DistributionArgs()
    a.params, a.Tq, a.tq_stride, a.spot, a.rate, a.max_tail = params.data_ptr(), Tq.data_ptr(), 0, spot.data_ptr(), c["rate"], c["max_tail"]
    a.probs, a.nP, a.nL, a.mT, a.B = ctypes.cast(pbuf, ctypes.POINTER(ctypes.c_double)), nP, 0, mT, B
    a.q_x, a.q_strike, a.q_flags = out["q_x"].data_ptr(), out["q_strike"].data_ptr(), out["q_flags"].data_ptr()
    a.tails, a.flags = out["tails"].data_ptr(), out["flags"].data_ptr()
    _lib.check(_lib.load().ivs_svi_distribution_f64(a, None, 0, torch.cuda.current_stream().cuda_stream), "ivs_svi_distribution_f64")
    torch.cuda.synchronize()
    assert (host(out["p_below"]) == SENT_F).all() and (host(out["p_above"]) == SENT_F).all()
    for k in ("q_x", "q_strike", "q_flags", "tails", "flags"):
        assert np.array_equal(host(out[k]), full[k], equal_nan=True), k


def test_explicit_stream_then_immediate_reallocation():
    """The call runs on an explicit stream while another stream is current; its inputs are temporaries that die when the
    call returns, and tensors of the same sizes are allocated and filled on the current stream at once.  The allocator must
    not hand the inputs' blocks out while the kernel still reads them (record_stream), so the results are the usual bits."""
    import torch
    from iv_interpolation_amd import engine
    c = DC.batch(**DC.STREAM_SHAPE)
    base = run(c)
    assert (base["flags"] & R.DEAD == 0).mean() >= 0.9
    same_bits(base, run(c, stream=torch.cuda.Stream()), "stream")
    s = torch.cuda.Stream()
    with torch.cuda.stream(torch.cuda.Stream()):
        q = engine.svi_distribution(dev(c["params"]), dev(c["Tq"]), dev(c["spot"]), c["rate"], probs=c["probs"], levels=c["levels"],
                                    max_tail=c["max_tail"], stream=s)
        junk = [torch.full(x.shape, 3.0, dtype=torch.float64, device="cuda") for x in (c["params"], c["Tq"], c["spot"]) for _ in range(3)]
        s.synchronize()
        torch.cuda.synchronize()
    same_bits(base, {k: host(v) for k, v in q.items()}, "reallocation")
    del junk


def test_shape_and_dtype_checks():
    import torch
    from iv_interpolation_amd import _lib, engine
    c, _ = case(shape_index(3, 16, 7, True))
    p, t, s = dev(c["params"]), dev(c["Tq"]), dev(c["spot"])
    with pytest.raises(ValueError):
        engine.svi_distribution(p[0], t, s)
    with pytest.raises(ValueError):
        engine.svi_distribution(p[..., :4].contiguous(), t, s)
    with pytest.raises(ValueError):
        engine.svi_distribution(p, t[..., :-1], s)
    with pytest.raises(ValueError):
        engine.svi_distribution(p, t, torch.cat([s, s]))
    with pytest.raises(TypeError):
        engine.svi_distribution(p.float(), t, s)
    with pytest.raises(ValueError):
        engine.svi_distribution(p, t, s, out={"flags": torch.empty(p.shape[:2], dtype=torch.float64, device="cuda")})
    with pytest.raises(ValueError, match="probabilities"):
        engine.svi_distribution(p, t, s, probs=(0.5, 1.0))
    with pytest.raises(ValueError, match="levels"):
        engine.svi_distribution(p, t, s, levels=(0.0,))
    with pytest.raises(ValueError, match="max_tail"):
        engine.svi_distribution(p, t, s, max_tail=2.0)
    with pytest.raises(_lib.EngineError, match="rows_per_wave=10"):
        engine.svi_distribution(p, t, s, rows_per_wave=10)


def test_builder_and_frame_on_a_wide_chain():
    """End to end: the chain of the SVI GPU test through build(), svi() and distribution() on the device.  The restatement is
    fed the kernel's own `params` copied back, so the late-round ties of the fit play no part."""
    import svi_cases as SC
    import snapshot_cases as SNC
    from iv_interpolation_amd.snapshots import HipBackend, SnapshotSurfaceBuilder, distribution_frame
    ten = SC.CHAIN_TENORS
    b = SnapshotSurfaceBuilder(moneyness=SC.CHAIN_MONEYNESS, tenors=ten, backend=HipBackend())
    res = b.build(SNC.big_chain(**SC.CHAIN))
    fits = b.svi(res, rate=SC.CHAIN_RATE)
    reps = b.distribution(res, fits, rate=SC.CHAIN_RATE)
    assert [d.underlying for d in reps] == ["btc", "eth"]
    for d, v, r in zip(reps, fits, res):
        c = dict(params=host(v.params), Tq=ten, spot=host(r.spot), rate=SC.CHAIN_RATE, probs=DC.DEFAULT_PROBS, levels=DC.DEFAULT_LEVELS,
                 max_tail=1e-6)
        ref = reference(c, margins=True)
        compare(f"builder[{d.underlying}]", {k: host(getattr(d, k)) for k in KEYS}, ref, c)
    own = b.distribution(res, rate=SC.CHAIN_RATE)                             # runs svi itself: the same bits
    for d, o in zip(reps, own):
        same_bits({k: host(getattr(d, k)) for k in KEYS}, {k: host(getattr(o, k)) for k in KEYS}, "own svi")
    f = distribution_frame(reps, res)
    assert len(f) == 80 * len(ten) and set(f["underlying"]) == {"btc", "eth"}
    assert list(f.columns) == ["underlying", "date", "spot", "tenor", "forward"] + [f"q_{p}" for p in (1, 5, 25, 50, 75, 95, 99)] + \
        [f"below_{u}" for u in (80, 90, 100, 110, 120)] + ["tail_lo", "tail_hi", "flags"]
    assert (f["flags"] & R.DEAD == 0).all() and (f["q_5"] < f["q_50"]).all() and (f["q_50"] < f["q_95"]).all()
    assert f["below_100"].between(0.3, 0.7).all() and (f["forward"] >= f["spot"]).all()
