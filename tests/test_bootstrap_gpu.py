"""GPU: hsim_bootstrap_kernel behind ivs_hsim_bootstrap_f64 against the restatement of rules C0-C9 (tests/boot_ref.py).

C1-C7 are a fixed sequence of IEEE and integer operations under a total order, so every output must equal the restatement's TO THE
BIT: integers, NaN patterns and the signs of zeros included.  There is no value allowance anywhere in this file, the chain on the
device's own rows included: the restatement is applied on the host to the rows the device wrote."""
import ctypes

import numpy as np
import pytest

import boot_cases as BC
import boot_ref as BR
import hsim_cases as HC

pytestmark = pytest.mark.gpu
SENT_F, SENT_I = -7.25e9, -77        # no output of the rules: counts >= 0; no value of a case hits -7.25e9
GUARD = 67                           # elements of guard tail behind every output
KEYS = BR.OUT_KEYS
_cache = {}


def host(t):
    return None if t is None else t.cpu().numpy()


def dev(a, dtype=np.float64):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, dtype, order="C")).cuda()


def shapes_of(c):
    import torch
    B = np.shape(c["pnl"])[0]
    nL, nC, R = len(c["tail_probs"]), len(c["ci_probs"]), c["n_rep"]
    f, i = torch.float64, torch.int32
    return dict(var0=((B, nL), f), es0=((B, nL), f), n_scen=((B,), i), mean=((B, 2, nL), f), variance=((B, 2, nL), f), quant=((B, 2, nL, nC), f),
                rep=((B, R, 2, nL), f))


def guarded(shapes):
    """One flat sentinel-filled buffer per output, GUARD elements longer than the output; the output is its head."""
    import torch
    flat, out = {}, {}
    for k, (shape, dt) in shapes.items():
        n = int(np.prod(shape))
        flat[k] = torch.full((n + GUARD,), SENT_I if dt == torch.int32 else SENT_F, dtype=dt, device="cuda")
        out[k] = flat[k][:n].view(shape)
    return flat, out


def sentinel(t):
    import torch
    return SENT_I if t.dtype == torch.int32 else SENT_F


def run(c, pnl=None, scen_flags=None, abi=False, want_rep=True, stream=None, **over):
    """The call through engine.hsim_bootstrap, or (abi) through the C entry point itself, into sentinel-filled outputs with guard tails;
    without rep the replicates go through a workspace (guarded too when the test makes it).  Returns host arrays, se included."""
    import torch
    from iv_interpolation_amd import _lib, engine
    c = {**c, **over}
    pnl = c["pnl"] if pnl is None else pnl
    scen_flags = c["scen_flags"] if scen_flags is None else scen_flags
    pnl = pnl if torch.is_tensor(pnl) else dev(pnl)
    scen_flags = scen_flags if torch.is_tensor(scen_flags) else dev(scen_flags, np.int32)
    flat, out = guarded(shapes_of(dict(c, pnl=pnl)))
    B, window = pnl.shape
    tp, ci = list(c["tail_probs"]), list(c["ci_probs"])
    se = None
    if abi:
        lib = _lib.load()
        a = _lib.BootstrapArgs()
        a.pnl, a.scen_flags, a.B, a.window = pnl.data_ptr(), scen_flags.data_ptr(), B, window
        a.tail_probs = ctypes.cast((ctypes.c_double * max(len(tp), 1))(*tp), ctypes.POINTER(ctypes.c_double))
        a.ci_probs = ctypes.cast((ctypes.c_double * max(len(ci), 1))(*ci), ctypes.POINTER(ctypes.c_double))
        a.nL, a.nC, a.min_scen, a.n_rep, a.block, a.seed = len(tp), len(ci), c["min_scen"], c["n_rep"], c["block"], c["seed"]
        for k in KEYS:
            setattr(a, k, out[k].data_ptr() if (k != "rep" or want_rep) else None)
        need = lib.ivs_hsim_bootstrap_workspace_bytes(B, c["n_rep"], len(tp))
        assert need == B * c["n_rep"] * 2 * len(tp) * 8
        ws = None if want_rep else torch.full((need // 8 + GUARD,), SENT_F, dtype=torch.float64, device="cuda")
        rc = lib.ivs_hsim_bootstrap_f64(ctypes.byref(a), None if ws is None else ws.data_ptr(), 0 if ws is None else need, None)
        assert rc == 0, lib.ivs_last_error()
        assert lib.ivs_last_kernel() == b"hsim_bootstrap_kernel"
        torch.cuda.synchronize()
        if ws is not None:
            assert (host(ws)[need // 8:] == SENT_F).all(), "the workspace's guard tail was touched"
    else:
        q = engine.hsim_bootstrap(pnl, scen_flags, tp, c["min_scen"], c["n_rep"], c["block"], c["seed"], ci, want_rep=want_rep,
                                  out={k: out[k] for k in KEYS if k != "rep" or want_rep}, stream=stream)
        assert engine.last_kernel() == "hsim_bootstrap_kernel" and set(q) == set(engine.BOOTSTRAP_OUTPUTS)
        assert (q["rep"] is None) == (not want_rep) and all(q[k] is out[k] for k in KEYS if k != "rep")
        se = q["se"]
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    got = {}
    for k in KEYS:
        v, tail = host(out[k]), host(flat[k])[out[k].numel():]
        assert (tail == sentinel(flat[k])).all(), f"{k}: the guard tail was touched"
        if k == "rep" and not want_rep:
            assert (v == SENT_F).all(), "rep: left out, yet written"
            got[k] = None
        else:
            assert not (v == sentinel(flat[k])).any(), f"{k}: an element was not written"
            got[k] = v
    if se is not None:
        got["se"] = host(se)
        assert np.array_equal(got["se"], host(torch.sqrt(out["variance"])), equal_nan=True)
        with np.errstate(all="ignore"):
            assert np.array_equal(got["se"], np.sqrt(got["variance"]), equal_nan=True)
    return got


def ref_of(c, **over):
    c = {**c, **over}
    return BR.bootstrap(c["pnl"], c["scen_flags"], c["tail_probs"], c["min_scen"], c["n_rep"], c["block"], c["seed"], c["ci_probs"])


def case(name):
    if name not in _cache:
        c = BC.TABLES[name] if name in BC.TABLES else BC.make(name)
        _cache[name] = (c, ref_of(c))
    return _cache[name]


def same_bits(a, b, keys, what):
    for k in keys:
        if a[k] is None or b[k] is None:
            continue
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype or x.dtype.kind == y.dtype.kind == "i", (k, what, x.dtype, y.dtype)
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), (k, what)
        if x.dtype.kind == "f":
            assert np.array_equal(np.signbit(np.nan_to_num(x)), np.signbit(np.nan_to_num(y))), (k, what)     # a zero's sign too


# ------------------------------------------------------------------ the restatement's bits
@pytest.mark.parametrize("name", sorted(BC.CASES))
def test_generated_bits(name):
    c, r = case(name)
    for abi in (False, True):
        for want_rep in (True, False):
            got = run(c, abi=abi, want_rep=want_rep)
            same_bits(got, r, KEYS, (name, abi, want_rep))
            assert got["n_scen"].dtype == np.int32


@pytest.mark.parametrize("name", sorted(BC.TABLES))
def test_tables_by_hand(name):
    t, r = case(name)
    for abi, want_rep in ((False, True), (True, False)):
        got = run(t, abi=abi, want_rep=want_rep)
        same_bits(got, r, KEYS, (name, abi))
        for k, v in t["want"].items():                       # the hand-made values themselves
            if got[k] is None:
                continue
            g = got[k][0] if np.ndim(v) < np.ndim(got[k]) else got[k]
            assert np.array_equal(g, np.asarray(v, g.dtype).reshape(g.shape), equal_nan=True), (name, k, g, v)


def _hsim_stage2(pnl, scen_flags, tail_probs, min_scen):
    """The device's own H7 on rows given: svi_hsim(stages=2) with a book that is not read."""
    import torch
    from iv_interpolation_amd import engine
    B, window = pnl.shape
    one = torch.ones(1, dtype=torch.float64, device="cuda")
    q = engine.svi_hsim(torch.zeros(B, 1, 5, dtype=torch.float64, device="cuda"), one, torch.ones(B, dtype=torch.float64, device="cuda"), 0.0, one, one, one,
                        lag=1, window=window, tail_probs=tail_probs, min_scen=min_scen, stages=2, out=dict(pnl=pnl, scen_flags=scen_flags))
    torch.cuda.synchronize()
    return dict(var0=host(q["var"]), es0=host(q["es"]), n_scen=host(q["n_valid"]))


@pytest.mark.parametrize("name", ["w63", "w256", "w1024", "w1024_l7", "tie_257", "infinite", "too_few", "garbage"])
def test_var0_es0_n_scen_are_the_tail_kernels(name):
    c, r = case(name)
    pnl, fl = dev(c["pnl"]), dev(c["scen_flags"], np.int32)
    got = run(c, pnl, fl, n_rep=2)
    same_bits(got, _hsim_stage2(pnl, fl, c["tail_probs"], c["min_scen"]), ("var0", "es0", "n_scen"), name)


def test_chain_on_the_device_rows():
    """hsim_cases' B = 70, window 65 shape through svi_hsim on the device, then the bootstrap on the rows the device wrote: the
    restatement on those rows, to the bit, and var0 / es0 / n_scen are that call's var / es / n_valid."""
    import torch
    from iv_interpolation_amd import engine
    h = HC.make(4)
    q = engine.svi_hsim(dev(h["params"]), dev(h["Tq"]), dev(h["spot"]), h["rate"], dev(h["u"]), dev(h["tau"]), dev(h["qty"]), lag=h["lag"],
                        window=h["window"], tail_probs=h["tail_probs"], min_scen=h["min_scen"], is_put=dev(h["is_put"], np.uint8),
                        strike_mode=h["strike_mode"])
    torch.cuda.synchronize()
    c = dict(tail_probs=tuple(h["tail_probs"]), min_scen=h["min_scen"], n_rep=64, block=2, seed=99, ci_probs=(0.05, 0.5, 0.95))
    got = run(c, q["pnl"], q["scen_flags"])
    r = ref_of(dict(c, pnl=host(q["pnl"]), scen_flags=host(q["scen_flags"])))
    assert r["active"].sum() >= 40 and not r["active"].all()
    same_bits(got, r, KEYS, "the restatement on the device's rows")
    same_bits(got, dict(var0=host(q["var"]), es0=host(q["es"]), n_scen=host(q["n_valid"])), ("var0", "es0", "n_scen"), "section 19's own")
    same_bits(got, run(c, q["pnl"], q["scen_flags"]), KEYS + ("se",), "two runs")


# ------------------------------------------------------------------ C8
def test_a_row_does_not_depend_on_the_launch():
    c, r = case("w64")
    full = run(c)
    for p in (0, 37, 69):
        one = run(c, c["pnl"][p:p + 1], c["scen_flags"][p:p + 1])
        same_bits({k: v[0] for k, v in one.items()}, {k: v[p] for k, v in full.items()}, KEYS, ("alone", p))
    c, r = case("w256")
    assert c["n_rep"] == 1024
    two = run(c, n_rep=2)
    same_bits(two, dict(rep=r["rep"][:, :2]), ("rep",), "R = 1024 against R = 2")
    same_bits(two, ref_of(c, n_rep=2), KEYS, "R = 2")
    same_bits(run(c), run(c), KEYS + ("se",), "two runs")
    lone = run(c, tail_probs=c["tail_probs"][1:], ci_probs=c["ci_probs"][:1])
    same_bits(lone, {k: r[k][..., 1:] for k in ("rep", "mean", "variance")}, ("rep", "mean", "variance"), "one level of two")
    same_bits(lone, dict(quant=r["quant"][:, :, 1:, :1]), ("quant",), "one quantile of two")


# ------------------------------------------------------------------ housekeeping
def test_null_rep_no_level_no_quantile():
    c, r = case("w63")
    a, b = run(c, want_rep=True), run(c, want_rep=False)
    assert b["rep"] is None
    same_bits(a, b, KEYS + ("se",), "NULL rep")
    for over in (dict(tail_probs=()), dict(ci_probs=()), dict(tail_probs=(), ci_probs=())):
        for abi in (False, True):
            got = run(c, abi=abi, **over)
            same_bits(got, ref_of(c, **over), KEYS, over)
            assert got["quant"].size == 0 and got["n_scen"].tolist() == r["n_scen"].tolist()


def test_explicit_stream_then_immediate_reallocation():
    import torch
    from iv_interpolation_amd import engine
    c, r = case("w256")
    pnl, fl = dev(np.tile(c["pnl"], (24, 1))), dev(np.tile(c["scen_flags"], (24, 1)), np.int32)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    out = engine.hsim_bootstrap(pnl, fl, c["tail_probs"], c["min_scen"], c["n_rep"], c["block"], c["seed"], c["ci_probs"], stream=s)
    junk = [torch.full((72, 1024, 2, 2), 3.0, dtype=torch.float64, device="cuda") for _ in range(4)]      # takes the workspace if it was freed too early
    s.synchronize()
    torch.cuda.synchronize()
    for k in ("var0", "es0", "n_scen", "mean", "variance", "quant"):
        same_bits({k: host(out[k])}, {k: np.tile(r[k], (24,) + (1,) * (r[k].ndim - 1))}, (k,), "explicit stream")
    assert out["rep"] is None and np.array_equal(host(out["se"]), np.sqrt(host(out["variance"])))
    del junk


def test_refused_calls_leave_the_device_buffers_alone():
    import torch
    from iv_interpolation_amd import _lib, engine
    c, r = case("w63")
    flat, out = guarded(shapes_of(c))
    pnl, fl = dev(c["pnl"]), dev(c["scen_flags"], np.int32)
    B, window = pnl.shape
    lib = _lib.load()
    need = lib.ivs_hsim_bootstrap_workspace_bytes(B, c["n_rep"], len(c["tail_probs"]))
    ws = torch.full((need // 8,), SENT_F, dtype=torch.float64, device="cuda")
    keep = []

    def dbl(xs):
        keep.append((ctypes.c_double * max(len(xs), 1))(*xs))
        return ctypes.cast(keep[-1], ctypes.POINTER(ctypes.c_double))
    for over, want in ((dict(window=1025), -34), (dict(window=0), -34), (dict(nL=9), -34), (dict(min_scen=0), -34), (dict(n_rep=0), -34), (dict(n_rep=1025), -34),
                       (dict(block=0), -34), (dict(block=1025), -34), (dict(nC=9), -34), (dict(ci_probs=dbl([0.5, 1.0] * 4)), -34),
                       (dict(tail_probs=dbl([0.0] * 8)), -34), (dict(B=2 ** 31 // (c["n_rep"] * 16) + 1), -34), (dict(nL=-1), -22), (dict(pnl=0), -22),
                       (dict(scen_flags=0), -22), (dict(quant=0), -22), (dict(mean=0), -22), (dict(n_scen=0), -22), (dict(ci_probs=None), -22),
                       (dict(rep=0, ws_bytes=need - 8), -22), (dict(rep=0, ws=None), -22)):
        over = dict(over)
        a = _lib.BootstrapArgs()
        a.pnl, a.scen_flags, a.B, a.window = pnl.data_ptr(), fl.data_ptr(), B, window
        a.tail_probs, a.ci_probs = dbl(c["tail_probs"]), dbl(c["ci_probs"])
        a.nL, a.nC, a.min_scen, a.n_rep, a.block, a.seed = len(c["tail_probs"]), len(c["ci_probs"]), c["min_scen"], c["n_rep"], c["block"], c["seed"]
        for k in KEYS:
            setattr(a, k, out[k].data_ptr())
        w, nbytes = over.pop("ws", ws), over.pop("ws_bytes", need)
        for k, v in over.items():
            setattr(a, k, v)
        rc = lib.ivs_hsim_bootstrap_f64(ctypes.byref(a), None if w is None else w.data_ptr(), nbytes if w is not None else 0, None)
        assert rc == want, (over, lib.ivs_last_error())
        assert lib.ivs_last_kernel() == b""
    with pytest.raises(ValueError, match="one shape"):
        engine.hsim_bootstrap(pnl, fl[:2], out=out)
    with pytest.raises(ValueError, match="n_rep"):
        engine.hsim_bootstrap(pnl, fl, n_rep=1025, out=out)
    with pytest.raises(ValueError, match="no output"):
        engine.hsim_bootstrap(pnl, fl, out=dict(out, se=out["mean"]))
    with pytest.raises(TypeError):
        engine.hsim_bootstrap(pnl, fl.to(torch.int64), out=out)
    torch.cuda.synchronize()
    for k, v in {**flat, "ws": ws}.items():
        assert (host(v) == sentinel(v)).all(), k
    empty = engine.hsim_bootstrap(pnl[:0], fl[:0])                                                   # B = 0: a no-op
    assert empty["mean"].shape == (0, 2, 2) and empty["se"].shape == (0, 2, 2) and engine.last_kernel() == ""


def test_builder_var_confidence_on_a_wide_chain():
    """End to end: build(), svi(), var() and var_confidence() on the device with the defaults: every figure is the restatement on
    the report's own rows, the base is the VarReport's to the bit, and the frame carries them."""
    import risk_cases as RC
    import svi_cases as SC
    import snapshot_cases as SNC
    from iv_interpolation_amd.snapshots import HipBackend, SnapshotSurfaceBuilder, confidence_frame
    b = SnapshotSurfaceBuilder(moneyness=SC.CHAIN_MONEYNESS, tenors=SC.CHAIN_TENORS, backend=HipBackend())
    res = b.build(SNC.big_chain(**SC.CHAIN))
    fits = b.svi(res, rate=SC.CHAIN_RATE)
    bk = RC.chain_book(res)
    var = b.var(res, bk, fits, rate=SC.CHAIN_RATE)
    reps = b.var_confidence(var)
    assert [d.underlying for d in reps] == ["btc", "eth"]
    for rp, v in zip(reps, var):
        assert (rp.n_rep, rp.block, rp.seed, list(rp.ci)) == (512, 1, 0, [0.05, 0.95])
        ref = BR.bootstrap(host(v.pnl), host(v.scen_flags), (0.05, 0.01), 20, 512, 1, 0, (0.05, 0.95))
        same_bits({k: host(getattr(rp, k)) for k in KEYS if k != "rep"}, ref, [k for k in KEYS if k != "rep"], "the report")
        same_bits(dict(a=host(rp.var0), b=host(rp.es0), c=host(rp.n_scen)), dict(a=host(v.var), b=host(v.es), c=host(v.n_valid)), ("a", "b", "c"), "C1")
        assert np.array_equal(host(rp.se), np.sqrt(ref["variance"]), equal_nan=True)
    f = confidence_frame(reps, res)
    assert len(f) > 0 and set(f["underlying"]) == {"btc", "eth"} and "es_0.01_hi" in f.columns
    ok = np.isfinite(f["var_0.05"].to_numpy())
    assert (f["var_0.05_lo"][ok] <= f["var_0.05_hi"][ok]).all() and (f["var_0.05_se"][ok] >= 0).all()
