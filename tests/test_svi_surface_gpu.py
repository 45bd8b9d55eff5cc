"""GPU: svi_calendar_kernel (ivs_svi_calendar_f64) and svi_eval_kernel (ivs_svi_eval_f64) against the restatement of rules
T1-T4, C1-C6 and E1-E6 (tests/cal_ref.py).

Flags, n_cross and every NaN pattern equal the restatement's everywhere (the generated batches keep every comparison of the
rules off its threshold: cal_ref.check_*_margins).  The values agree within C_GPU x R_CPU units of eps x the rule's own scale
(cal_cases.tolerances_*; DESIGN.md section 14 has the reasoning): R_CPU is the restatement's distance from the same rules in
mpmath at 50 digits, measured by test_svi_surface.test_rounding_level.

Every test prints its largest error / tolerance ratios; with IVS_SS_ERRLOG=<file> set the figures are appended to that file
as well (a recorded run belongs in profiles/svi_surface/errlog_gpu.txt; errlog.txt there holds the CPU run)."""
import ctypes
import os

import numpy as np
import pytest

import cal_cases as CC
import cal_ref as R

pytestmark = pytest.mark.gpu
SENT_F, SENT_I = -7.25e9, -77        # no output of the rules: flags and counts >= 0; no value ever hits -7.25e9
GUARD = 67                           # elements of guard tail behind every output
GPU_FACTOR = {k: CC.C_GPU * v for k, v in CC.R_CPU.items()}
EVAL_ALL = R.EVAL_KEYS + ("flags",)


def log(name, **figures):
    line = name + ": " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items())
    print(line)
    path = os.environ.get("IVS_SS_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def host(t):
    return None if t is None else t.cpu().numpy()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()


def guarded(shapes):
    """One flat sentinel-filled buffer per output, GUARD elements longer than the output; the output is its head."""
    import torch
    flat, out = {}, {}
    for k, (shape, dt) in shapes.items():
        n = int(np.prod(shape))
        flat[k] = torch.full((n + GUARD,), SENT_I if dt == torch.int32 else SENT_F, dtype=dt, device="cuda")
        out[k] = flat[k][:n].view(shape)
    return flat, out


def check_written(flat, out, keys):
    got = {}
    for k in keys:
        v, tail = host(out[k]), host(flat[k])[out[k].numel():]
        sent = SENT_I if v.dtype == np.int32 else SENT_F
        assert not (v == sent).any(), f"{k}: an element was not written"
        assert (tail == sent).all(), f"{k}: the guard tail was touched"
        got[k] = v
    return got


def run_cal(c, stream=None, rpw=0):
    """One calendar call with every output pre-filled with a sentinel and followed by a guard tail."""
    import torch
    from iv_interpolation_amd import engine
    B, mT, _ = c["params"].shape
    f64, i32 = torch.float64, torch.int32
    flat, out = guarded({"d_min": ((B, mT), f64), "x_min": ((B, mT), f64), "d_atm": ((B, mT), f64), "x_cross": ((B, mT, 2), f64),
                         "n_cross": ((B, mT), i32), "flags": ((B, mT), i32)})
    q = engine.svi_calendar(dev(c["params"]), dev(c["Tq"]), dev(c["spot"]), out=out, stream=stream, rows_per_wave=rpw)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    assert engine.last_kernel() == "svi_calendar_kernel" and set(q) == set(R.CAL_KEYS)
    return check_written(flat, out, R.CAL_KEYS)


def run_eval(c, stream=None, want=R.EVAL_KEYS):
    import torch
    from iv_interpolation_amd import engine
    B, Q = c["params"].shape[0], c["u"].shape[-1]
    shapes = {k: ((B, Q), torch.float64) for k in R.EVAL_KEYS}
    shapes["flags"] = ((B, Q), torch.int32)
    flat, out = guarded(shapes)
    q = engine.svi_eval(dev(c["params"]), dev(c["Tq"]), dev(c["spot"]), c["rate"], dev(c["u"]), dev(c["tau"]), strike_mode=c["strike_mode"],
                        want=want, out={k: out[k] for k in tuple(want) + ("flags",)}, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    assert engine.last_kernel() == "svi_eval_kernel" and set(q) == set(EVAL_ALL)
    for k in R.EVAL_KEYS:
        if k not in want:                                                    # left out: None, and its buffer untouched
            assert q[k] is None and (host(flat[k]) == SENT_F).all(), k
    got = check_written(flat, out, tuple(want) + ("flags",))
    got.update({k: None for k in R.EVAL_KEYS if k not in want})
    return got


def ref_cal(c, margins=False):
    return R.restate_calendar(c["params"], c["Tq"], c["spot"], margins=margins)


def ref_eval(c, margins=False):
    return R.restate_eval(c["params"], c["Tq"], c["spot"], c["rate"], c["u"], c["tau"], c["strike_mode"], margins=margins)


def compare_cal(name, got, ref):
    assert got["flags"].dtype == np.int32 and got["n_cross"].dtype == np.int32
    u = CC.units(got, ref, CC.tolerances_calendar, CC.CAL_UNIT)
    fig = {k: (float(np.nanmax(v)) / GPU_FACTOR[CC.CAL_UNIT[k]] if np.isfinite(v).any() else 0.0) for k, v in u.items()}
    log(name, **fig, rows=int(ref["live"].size), pairs=int(ref["pair"].sum()), crossings=int(ref["n_cross"].sum()))
    assert np.array_equal(got["flags"], ref["flags"]), (name, got["flags"], ref["flags"])
    assert np.array_equal(got["n_cross"], ref["n_cross"]), (name, got["n_cross"], ref["n_cross"])
    for k in u:
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (name, k)
    assert all(v <= 1.0 for v in fig.values()), (name, fig)


def compare_eval(name, got, ref):
    assert got["flags"].dtype == np.int32
    u = CC.units(got, ref, CC.tolerances_eval, CC.EVAL_UNIT)
    fig = {k: (float(np.nanmax(v)) / GPU_FACTOR[CC.EVAL_UNIT[k]] if np.isfinite(v).any() else 0.0) for k, v in u.items()}
    log(name, **fig, queries=int(ref["ok"].size), live=int(ref["ok"].sum()))
    assert np.array_equal(got["flags"], ref["flags"]), (name, got["flags"], ref["flags"])
    for k in u:
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (name, k)
    assert all(v <= 1.0 for v in fig.values()), (name, fig)


def same_bits(a, b, keys, what):
    for k in keys:
        if a[k] is None:
            assert b[k] is None, (k, what)
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), (k, what)


_cache = {}


def case(n):
    """Inputs and restatements of one generated batch, computed once and shared (read-only)."""
    if n not in _cache:
        c = CC.batch(**CC.SHAPES[n])
        rc, re_ = ref_cal(c, margins=True), ref_eval(c, margins=True)
        for a in list(c.values()) + list(rc.values()) + list(re_.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[n] = (c, rc, re_)
    return _cache[n]


def shape_index(B, mT, per):
    return next(n for n, s in enumerate(CC.SHAPES) if (s["B"], s["mT"], s["per"]) == (B, mT, per))


@pytest.mark.parametrize("name", sorted(CC.MICRO_CAL))
def test_micro_calendar(name):
    c = CC.MICRO_CAL[name]
    got = run_cal(c)
    state = CC.DEAD | CC.LAST | CC.UNORDERED
    assert np.array_equal(got["flags"] & state, np.where(c["flags"] < 0, 0, c["flags"]) & state), got["flags"]
    if not c.get("state_only"):
        assert np.array_equal(got["flags"], c["flags"]), got["flags"]
    if "n_cross" in c:
        assert np.array_equal(got["n_cross"], c["n_cross"])
    if name == "identical":
        assert got["d_min"][0, 0] == 0.0 and got["d_atm"][0, 0] == 0.0
    compare_cal(f"micro_cal[{name}]", got, ref_cal(c))


@pytest.mark.parametrize("name", sorted(CC.MICRO_EVAL))
def test_micro_eval(name):
    c = CC.MICRO_EVAL[name]
    got = run_eval(c)
    assert np.array_equal(got["flags"], c["flags"]), got["flags"]
    compare_eval(f"micro_eval[{name}]", got, ref_eval(c))


@pytest.mark.parametrize("n", range(len(CC.SHAPES)), ids=[CC.shape_id(s) for s in CC.SHAPES])
def test_shapes(n):
    """Every (B, mT) of the table with Q in {1, 63, 64, 65, 257}: shared tenors and queries at rate 0 with moneyness levels,
    per-snapshot tenors and queries at rate 0.03 with strikes; at mT = 64 the jittered tenors are out of order."""
    c, rc, re_ = case(n)
    compare_cal(f"cal[{CC.shape_id(CC.SHAPES[n])}]", run_cal(c), rc)
    compare_eval(f"eval[{CC.shape_id(CC.SHAPES[n])}]", run_eval(c), re_)


@pytest.mark.parametrize("B,mT", [(1, 2), (4, 3), (2, 13), (3, 16), (2, 64)])
def test_partition_independence(B, mT):
    """rows_per_wave forced to every legal value and left at 0: identical bits.  With 32 rows per wave the wavefronts of
    (2, 13) and (3, 16) span snapshots and (2, 64) starts one in the middle of a snapshot."""
    c, rc, _ = case(shape_index(B, mT, False))
    base = run_cal(c, rpw=0)
    compare_cal(f"partition[B{B}-mT{mT}, rpw=0]", base, rc)
    for rpw in range(1, 33):
        same_bits(base, run_cal(c, rpw=rpw), R.CAL_KEYS, rpw)


def test_shared_and_per_snapshot_inputs_agree_bitwise():
    c, _, _ = case(shape_index(3, 16, False))
    B = 3
    wide = dict(c, Tq=np.tile(c["Tq"], (B, 1)), u=np.tile(c["u"], (B, 1)), tau=np.tile(c["tau"], (B, 1)))
    same_bits(run_cal(c), run_cal(wide), R.CAL_KEYS, "tq")
    same_bits(run_eval(c), run_eval(wide), EVAL_ALL, "tq and queries")


def test_strike_modes_agree_bitwise():
    c, _, re_ = case(shape_index(3, 16, False))
    shape = re_["w"].shape
    k = dict(c, u=c["spot"][:, None] * np.broadcast_to(c["u"], shape), tau=np.broadcast_to(c["tau"], shape), strike_mode=1)
    same_bits(run_eval(c), run_eval(k), EVAL_ALL, "strike mode")


def test_optional_outputs_left_out():
    """NULL value outputs are neither written nor needed: `call` alone, nothing but the flags, and all but one keep the bits of
    the full call."""
    c, _, _ = case(shape_index(3, 16, True))
    full = run_eval(c)
    for want in (("call",), (), ("w", "vol", "put", "fwd_var", "g", "local_vol")):
        part = run_eval(c, want=want)
        same_bits({k: full[k] for k in tuple(want) + ("flags",)}, part, tuple(want) + ("flags",), want)


def test_explicit_stream_then_immediate_reallocation():
    """The calls run on an explicit stream while another stream is current; their inputs are temporaries that die when the
    call returns, and tensors of the same sizes are allocated and filled on the current stream at once (record_stream)."""
    import torch
    from iv_interpolation_amd import engine
    c = CC.batch(**CC.STREAM_SHAPE)
    base_c, base_e = run_cal(c), run_eval(c)
    assert (base_c["flags"] & R.DEAD == 0).mean() >= 0.9
    same_bits(base_c, run_cal(c, stream=torch.cuda.Stream()), R.CAL_KEYS, "stream")
    same_bits(base_e, run_eval(c, stream=torch.cuda.Stream()), EVAL_ALL, "stream")
    s = torch.cuda.Stream()
    with torch.cuda.stream(torch.cuda.Stream()):
        qc = engine.svi_calendar(dev(c["params"]), dev(c["Tq"]), dev(c["spot"]), stream=s)
        qe = engine.svi_eval(dev(c["params"]), dev(c["Tq"]), dev(c["spot"]), c["rate"], dev(c["u"]), dev(c["tau"]), strike_mode=1, stream=s)
        junk = [torch.full(x.shape, 3.0, dtype=torch.float64, device="cuda") for x in (c["params"], c["Tq"], c["spot"], c["u"], c["tau"]) for _ in range(3)]
        s.synchronize()
        torch.cuda.synchronize()
    same_bits(base_c, {k: host(v) for k, v in qc.items()}, R.CAL_KEYS, "reallocation")
    same_bits(base_e, {k: host(v) for k, v in qe.items()}, EVAL_ALL, "reallocation")
    del junk


def test_abi_error_table():
    import torch
    from iv_interpolation_amd import _lib, engine
    c, _, _ = case(shape_index(3, 16, True))
    p, t, s, u, tq = dev(c["params"]), dev(c["Tq"]), dev(c["spot"]), dev(c["u"]), dev(c["tau"])
    for bad in (lambda: engine.svi_calendar(p[0], t, s), lambda: engine.svi_calendar(p[..., :4].contiguous(), t, s),
                lambda: engine.svi_calendar(p, t[..., :-1], s), lambda: engine.svi_calendar(p, t, torch.cat([s, s])),
                lambda: engine.svi_calendar(p, t, s, out={"flags": torch.empty(p.shape[:2], dtype=torch.float64, device="cuda")}),
                lambda: engine.svi_calendar(torch.zeros((1, 65, 5), dtype=torch.float64, device="cuda"), torch.ones(65, dtype=torch.float64, device="cuda"), s[:1]),
                lambda: engine.svi_eval(p, t, s, 0.0, u, tq[:, :-1]), lambda: engine.svi_eval(p, t, s, 0.0, u[:2], tq[:2]),
                lambda: engine.svi_eval(p, t, s, 0.0, u, tq, strike_mode=3), lambda: engine.svi_eval(p, t, s, 0.0, u, tq, want=("delta",)),
                lambda: engine.svi_eval(p, t, s, 0.0, u, tq, out={"call": torch.empty(u.shape, dtype=torch.float32, device="cuda")})):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        engine.svi_calendar(p.float(), t, s)
    with pytest.raises(TypeError):
        engine.svi_eval(p, t, s, 0.0, u.float(), tq)
    with pytest.raises(_lib.EngineError, match="rows_per_wave=33"):
        engine.svi_calendar(p, t, s, rows_per_wave=33)
    lib = _lib.load()
    a = _lib.EvalArgs()
    a.params, a.Tq, a.tq_stride, a.spot, a.u, a.tau, a.q_stride = p.data_ptr(), t.data_ptr(), 16, s.data_ptr(), u.data_ptr(), tq.data_ptr(), 7
    a.mT, a.Q, a.B = 16, u.shape[1], 3
    flags = torch.full(u.shape, SENT_I, dtype=torch.int32, device="cuda")
    a.flags = flags.data_ptr()
    assert lib.ivs_svi_eval_f64(ctypes.byref(a), None, 0, None) == -22 and b"stride" in lib.ivs_last_error()
    a.q_stride, a.strike_mode = u.shape[1], 2
    assert lib.ivs_svi_eval_f64(ctypes.byref(a), None, 0, None) == -22 and b"strike_mode" in lib.ivs_last_error()
    a.strike_mode, a.flags = 1, None
    assert lib.ivs_svi_eval_f64(ctypes.byref(a), None, 0, None) == -22 and b"null pointer" in lib.ivs_last_error()
    torch.cuda.synchronize()
    assert (host(flags) == SENT_I).all()                                      # a refused call launches nothing
    assert engine.svi_eval(p, t, s, 0.0, u[:, :0].contiguous(), tq[:, :0].contiguous())["flags"].shape == (3, 0)   # Q == 0: a no-op


def test_builder_and_frames_on_a_wide_chain():
    """End to end: the chain of the SVI GPU test through build(), svi(), calendar() and price() on the device.  The
    restatement is fed the kernel's own `params` copied back, so the late-round ties of the fit play no part."""
    import svi_cases as SC
    import snapshot_cases as SNC
    from iv_interpolation_amd.snapshots import HipBackend, SnapshotSurfaceBuilder, calendar_frame, price_frame
    ten = SC.CHAIN_TENORS
    b = SnapshotSurfaceBuilder(moneyness=SC.CHAIN_MONEYNESS, tenors=ten, backend=HipBackend())
    res = b.build(SNC.big_chain(**SC.CHAIN))
    fits = b.svi(res, rate=SC.CHAIN_RATE)
    cals = b.calendar(res, fits)
    book = CC.chain_book(res)
    marks = b.price(res, book, fits, rate=SC.CHAIN_RATE)
    assert [d.underlying for d in cals] == ["btc", "eth"] == [d.underlying for d in marks]
    for cl, mk, v, r in zip(cals, marks, fits, res):
        c = dict(params=host(v.params), Tq=ten, spot=host(r.spot), rate=SC.CHAIN_RATE,
                 u=np.ascontiguousarray(np.broadcast_to(mk.strikes, mk.tau.shape)), tau=mk.tau, strike_mode=1)
        compare_cal(f"builder_cal[{cl.underlying}]", {k: host(getattr(cl, k)) for k in R.CAL_KEYS}, ref_cal(c, margins=True))
        compare_eval(f"builder_eval[{mk.underlying}]", {k: host(getattr(mk, k)) for k in EVAL_ALL}, ref_eval(c, margins=True))
    own = b.calendar(res, rate=SC.CHAIN_RATE)                                 # runs svi itself: the same bits
    for d, o in zip(cals, own):
        same_bits({k: host(getattr(d, k)) for k in R.CAL_KEYS}, {k: host(getattr(o, k)) for k in R.CAL_KEYS}, R.CAL_KEYS, "own svi")
    f = calendar_frame(cals, res)
    assert len(f) == 80 * (len(ten) - 1) and set(f["underlying"]) == {"btc", "eth"} and (f["next_tenor"] > f["tenor"]).all()
    g = price_frame(marks, res)
    assert len(g) == 80 * len(book) and (g["flags"][11::12] == R.Q_DEAD).all() and (g["flags"][:11] & R.Q_DEAD == 0).all()
    near = g[(g["flags"] & R.Q_DEAD == 0) & (g["underlying"] == "btc")]      # the book's strikes lie round btc's spot
    assert (near["call"] > 0).all() and (near["put"] > 0).all() and near["vol"].between(0.05, 3.0).all()
