"""GPU: svi_hsim_attrib_kernel (ivs_svi_hsim_attrib_f64) against the restatement of rules A0-A8 (tests/attrib_ref.py).

Value tests feed the kernel the RESTATEMENT's pnl and scen_flags, so that both sides rank the same rows: order, n_tail and every
NaN pattern must be equal, the values agree within C_GPU x R_CPU units of eps x the value's own scale (attrib_cases.constants;
DESIGN.md section 20 has the reasoning).  Chain tests feed it section 19's own device output and compare bits only: with one
group the group figures are var and es, the B5 sum of cvar on the host is var, order is the stable argsort of the device's pnl.

Every test prints its largest error / tolerance ratios; with IVS_ATTRIB_ERRLOG=<file> set the figures are appended to that file as
well (a recorded run belongs in profiles/attrib/errlog_gpu.txt; errlog.txt there holds the CPU run)."""
import ctypes
import os

import numpy as np
import pytest

import attrib_cases as AC
import attrib_ref as A
import hsim_cases as HC
import risk_ref as R

pytestmark = pytest.mark.gpu
SENT_F, SENT_I = -7.25e9, -77        # no output of the rules: counts and ranks >= -1; no value ever hits -7.25e9
GUARD = 67                           # elements of guard tail behind every output
INT_KEYS = ("n_tail", "order")
OPTIONAL = ("ces", "cvar", "ces_group", "cvar_group", "order")


def log(name, **figures):
    line = name + ": " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items())
    print(line)
    path = os.environ.get("IVS_ATTRIB_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def host(t):
    return None if t is None else t.cpu().numpy()


def dev(a, dtype=np.float64):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, dtype, order="C")).cuda()      # a copy: the cached cases are read-only


def shapes_of(c):
    import torch
    B, w, nL, Q, nG = c["params"].shape[0], c["window"], len(c["tail_probs"]), len(c["qty"]), c["nG"]
    f, i = torch.float64, torch.int32
    return dict(ces=((B, nL, Q), f), cvar=((B, nL, Q), f), ces_group=((B, nL, nG), f), cvar_group=((B, nL, nG), f), n_tail=((B, nL), i),
                order=((B, w), i))


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


def inputs(c):
    return dict(params=dev(c["params"]), Tq=dev(c["Tq"]), spot=dev(c["spot"]), u=dev(c["u"]), tau=dev(c["tau"]), qty=dev(c["qty"]),
                is_put=dev(c["is_put"], np.uint8), group=dev(c["group"], np.int32))


def hsim_on_device(c):
    """Section 19's own call on the case: device tensors."""
    import torch
    from iv_interpolation_amd import engine
    t = inputs(c)
    q = engine.svi_hsim(t["params"], t["Tq"], t["spot"], c["rate"], t["u"], t["tau"], t["qty"], lag=c["lag"], window=c["window"], tail_probs=c["tail_probs"],
                        min_scen=c["min_scen"], is_put=t["is_put"], strike_mode=c["strike_mode"])
    torch.cuda.synchronize()
    return q


def run(c, pnl, scen_flags, stream=None, want=OPTIONAL, abi=False):
    """The call through engine.svi_hsim_attrib, or (abi) through the C entry point itself, into sentinel-filled outputs.  pnl,
    scen_flags: host arrays or device tensors."""
    import torch
    from iv_interpolation_amd import _lib, engine
    flat, out = guarded(shapes_of(c))
    keys = tuple(k for k in A.OUT_KEYS if k in want or k == "n_tail")
    t = inputs(c)
    pnl = pnl if torch.is_tensor(pnl) else dev(pnl)
    scen_flags = scen_flags if torch.is_tensor(scen_flags) else dev(scen_flags, np.int32)
    if abi:
        a = _lib.HsimAttribArgs()
        B, mT = c["params"].shape[:2]
        Q = len(c["qty"])
        for k, v in t.items():
            setattr(a, k, 0 if v is None else v.data_ptr())
        a.pnl, a.scen_flags = pnl.data_ptr(), scen_flags.data_ptr()
        a.tq_stride, a.q_stride, a.rate = (mT if np.ndim(c["Tq"]) == 2 else 0), (Q if np.ndim(c["u"]) == 2 else 0), c["rate"]
        a.strike_mode, a.mT, a.Q, a.B, a.lag, a.window, a.nG = c["strike_mode"], mT, Q, B, c["lag"], c["window"], c["nG"]
        tp = list(c["tail_probs"])
        a.tail_probs, a.nL, a.min_scen = ctypes.cast((ctypes.c_double * max(len(tp), 1))(*tp), ctypes.POINTER(ctypes.c_double)), len(tp), c["min_scen"]
        for k in keys:
            setattr(a, k, out[k].data_ptr())
        lib = _lib.load()
        assert lib.ivs_svi_hsim_attrib_f64(ctypes.byref(a), None, 0, None) == 0, lib.ivs_last_error()
        assert lib.ivs_last_kernel() == b"svi_hsim_attrib_kernel"
    else:
        q = engine.svi_hsim_attrib(t["params"], t["Tq"], t["spot"], c["rate"], t["u"], t["tau"], t["qty"], pnl, scen_flags, group=t["group"], n_groups=c["nG"],
                                   lag=c["lag"], window=c["window"], tail_probs=c["tail_probs"], min_scen=c["min_scen"], is_put=t["is_put"],
                                   strike_mode=c["strike_mode"], want=tuple(k for k in want), out={k: out[k] for k in keys}, stream=stream)
        assert engine.last_kernel() == "svi_hsim_attrib_kernel" and set(q) == set(A.OUT_KEYS)
        assert all((q[k] is None) == (k not in keys) for k in A.OUT_KEYS)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    for k in A.OUT_KEYS:
        if k not in keys:
            assert (host(flat[k]) == (SENT_I if flat[k].dtype == torch.int32 else SENT_F)).all(), k      # left out: its buffer untouched
    got = check_written(flat, out, keys)
    for k in A.OUT_KEYS:
        got.setdefault(k, None)
    return got


def ref_of(c):
    return A.restate_attrib(c["params"], c["Tq"], c["spot"], c["rate"], c["u"], c["tau"], c["qty"], c["lag"], c["window"], c["tail_probs"],
                            c["min_scen"], c["is_put"], c["strike_mode"], c["group"], c["nG"])


def compare(name, got, ref):
    for k in INT_KEYS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), (name, k, got[k], ref[k])
    u = AC.allowance_ratios(got, ref, AC.C_GPU)
    fig = {k: (float(np.nanmax(v)) if np.isfinite(v).any() else 0.0) for k, v in u.items()}
    log(name, **fig, tails=int(ref["n_tail"].sum()), options=int(ref["hsim"]["live"].size))
    for k in u:
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (name, k)
    assert all(v <= 1.0 for v in fig.values()), (name, fig)


def same_bits(a, b, keys, what):
    for k in keys:
        if a[k] is None or b[k] is None:
            continue
        assert np.array_equal(a[k], b[k], equal_nan=True), (k, what)
        assert np.array_equal(np.signbit(np.nan_to_num(a[k])), np.signbit(np.nan_to_num(b[k]))), (k, what)     # a zero's sign too


def plus_zero(a):
    a = np.asarray(a)
    return bool((a == 0.0).all() and not np.signbit(a).any())


_cache = {}


def case(name):
    """Inputs and restatement of one generated batch, computed once and shared (read-only)."""
    if name not in _cache:
        c = AC.make(name)
        r = ref_of(c)
        for a in list(c.values()) + list(r.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = (c, r)
    return _cache[name]


def value_run(c, r, **kw):
    return run(c, r["hsim"]["pnl"], r["hsim"]["scen_flags"], **kw)


# ------------------------------------------------------------------ value tests: the restatement's rows
@pytest.mark.parametrize("name", sorted(AC.MICRO))
def test_micro(name):
    c = AC.MICRO[name]
    r = ref_of(c)
    g = value_run(c, r)
    compare(f"micro[{name}]", g, r)
    same_bits(g, value_run(c, r, abi=True), A.OUT_KEYS, "C ABI")


@pytest.mark.parametrize("name", list(AC.CASES))
def test_cases(name):
    c, r = case(name)
    g = value_run(c, r)
    compare(f"case[{name}]", g, r)
    if name in AC.UNORDERED:
        assert all(np.isnan(g[k]).all() for k in AC.VALUE_KEYS) and (g["n_tail"] == 0).all() and (g["order"] == -1).all()
    same_bits(g, value_run(c, r, abi=True), A.OUT_KEYS, "C ABI")


def test_micro_patterns_on_the_device():
    """The one-option book, H6's pair in the tail, zero quantities and a group without a live member, to the bit."""
    c = AC.MICRO["one_option"]
    h = {k: host(v) for k, v in hsim_on_device(c).items()}
    g = run(c, h["pnl"], h["scen_flags"])
    for k, v in (("cvar", "var"), ("ces", "es")):
        same_bits({k: g[k][:, :, 0], k + "_group": g[k + "_group"][:, :, 0]}, {k: h[v], k + "_group": h[v]}, (k, k + "_group"), "one option")
    c = AC.MICRO["same_pair"]
    g = value_run(c, ref_of(c))
    assert all(plus_zero(g[k][1]) for k in AC.VALUE_KEYS) and (g["cvar"][2] != 0.0).any()
    c = AC.MICRO["empty_group"]
    g = value_run(c, ref_of(c))
    on = g["n_tail"][:, 0] > 0
    assert on.any() and plus_zero(g["ces_group"][on][:, :, 1:]) and plus_zero(g["cvar_group"][on][:, :, 1:]) and plus_zero(g["ces"][on][:, :, [0, 4]])
    assert np.isnan(g["ces"][on][:, :, [1, 3]]).all()


@pytest.mark.parametrize("name", sorted(AC.ROWS))
def test_a1_rows_given_directly(name):
    """The ranking alone on rows by hand: ties with -0.0 against +0.0, flags, NaN, and entries past n_p that no call of section 19
    writes as valid."""
    pnl, fl, n_p, order = AC.ROWS[name]
    c, _ = case("B9-Q65-w63-L8")                                                         # snapshot 8 has eight scenarios: lag 9 - n_p fits the row
    w = len(pnl)
    cc = dict(c, window=w, lag=9 - n_p, tail_probs=(0.5,), min_scen=1)
    rows = np.full((9, w), np.nan)
    rows[8] = pnl
    flags = np.full((9, w), HC.ABSENT, np.int32)
    flags[8] = fl
    g = run(cc, rows, flags)
    assert list(g["order"][8]) == order + [-1] * (w - len(order)) and (g["order"][:8] == -1).all()
    assert g["n_tail"][8, 0] == (max(1, len(order) // 2) if order else 0) and (g["n_tail"][:8] == 0).all()


# ------------------------------------------------------------------ chain tests: section 19's own device output, bits only
@pytest.mark.parametrize("name", ["B70-Q63-w65", "B9-Q65-w63-L8", "B260-Q2-w257", "B9-Q1025-w257", "B3-Q257-w4"])
def test_chain_from_the_device_rows(name):
    c, _ = case(name)
    q = hsim_on_device(c)
    h = {k: host(v) for k, v in q.items()}
    one = run(dict(c, group=None, nG=1), q["pnl"], q["scen_flags"])
    assert np.array_equal(one["cvar_group"][:, :, 0], h["var"], equal_nan=True) and np.array_equal(np.signbit(one["cvar_group"][:, :, 0]), np.signbit(h["var"]))
    assert np.array_equal(one["ces_group"][:, :, 0], h["es"], equal_nan=True) and np.array_equal(np.signbit(one["ces_group"][:, :, 0]), np.signbit(h["es"]))
    n_p = np.clip(np.arange(len(c["spot"])) - c["lag"] + 1, 0, c["window"])
    for p in range(len(n_p)):
        od = A.rank(h["pnl"][p], h["scen_flags"][p], n_p[p])
        assert list(one["order"][p, :len(od)]) == list(od) and (one["order"][p, len(od):] == -1).all() and len(od) == h["n_valid"][p], p
        assert list(one["n_tail"][p]) == A.tails(len(od), c["tail_probs"], c["min_scen"])
    on = one["n_tail"] > 0
    for p, l in zip(*np.nonzero(on)):
        cv = one["cvar"][p, l]                                                           # NaN = a dead option: +0.0 in its lane
        tot = 0.0 - R.b5_sum(np.where(np.isnan(cv), 0.0, 0.0 - cv))
        assert tot == h["var"][p, l] and np.signbit(tot) == np.signbit(h["var"][p, l]), (p, l)
    g = run(c, q["pnl"], q["scen_flags"])                                                # the case's own groups: per-option figures unchanged
    same_bits(g, one, ("ces", "cvar", "n_tail", "order"), "grouping")
    same_bits(g, run(c, q["pnl"], q["scen_flags"]), A.OUT_KEYS, "second run")


def test_same_bits_for_a_snapshot_alone_and_with_null_outputs():
    c, _ = case("B70-Q63-w65")
    q = hsim_on_device(c)
    base = run(c, q["pnl"], q["scen_flags"])
    rows = np.arange(4, 70)                                                              # snapshot 69: its 65 scenarios reach back to snapshot 4
    pick = lambda a: a[rows] if np.ndim(a) == 2 and a.shape[0] == 70 else a    # noqa: E731
    alone_c = dict(c, params=c["params"][rows], spot=c["spot"][rows], Tq=pick(c["Tq"]), u=pick(c["u"]), tau=pick(c["tau"]))
    qa = hsim_on_device(alone_c)
    assert np.array_equal(host(qa["pnl"])[-1], host(q["pnl"])[-1])
    alone = run(alone_c, qa["pnl"], qa["scen_flags"])
    for k in A.OUT_KEYS:
        assert np.array_equal(alone[k][-1], base[k][-1], equal_nan=True), k
    for want in (("ces",), ("cvar_group", "order"), ("ces_group",), ()):
        part = run(c, q["pnl"], q["scen_flags"], want=want)
        same_bits(base, part, A.OUT_KEYS, want)
        same_bits(base, run(c, q["pnl"], q["scen_flags"], want=want, abi=True), A.OUT_KEYS, want)


def test_null_group_outputs_on_more_than_one_pass_and_an_odd_tail():
    """Without group outputs the kernel drops the butterflies and their traffic, not the barrier that ends a pass: Q = 300 is two
    passes and M = 3 makes the last rank of a pass read the pair of slice buffers that rank 0 of the next pass stages into.  Also
    five passes (Q = 1025).  The bits of the per-option outputs must be those of the full call, and the values inside the allowance."""
    for name in ("B16-Q300-w16", "B9-Q1025-w257"):
        c, r = case(name)
        if name == "B16-Q300-w16":
            assert len(c["qty"]) > 256 and r["n_tail"].max() == 3
        base = value_run(c, r)
        for want in (("ces", "cvar"), ("cvar",), ("ces", "order")):
            for abi in (False, True):
                part = value_run(c, r, want=want, abi=abi)
                assert part["ces_group"] is None and part["cvar_group"] is None
                same_bits(base, part, A.OUT_KEYS, (name, want, abi))
        compare(f"null groups[{name}]", dict(value_run(c, r, want=("ces", "cvar", "order")), ces_group=None, cvar_group=None), r)


def test_empty_inputs_through_the_wrapper():
    """A8: the C call writes nothing with Q == 0 or mT == 0; the wrapper defines the result."""
    import torch
    from iv_interpolation_amd import engine
    c, r = case("B9-Q65-w63-L8")
    t = inputs(c)
    B, w, nL = 9, c["window"], 8
    kw = dict(lag=1, window=w, tail_probs=c["tail_probs"], min_scen=c["min_scen"], strike_mode=1, n_groups=2)
    n_p = np.clip(np.arange(B), 0, w)
    for stream in (None, torch.cuda.Stream()):
        e = dict(c, qty=c["qty"][:0])
        h = engine.svi_hsim(t["params"], t["Tq"], t["spot"], c["rate"], t["u"][:, :0].contiguous(), t["tau"][:, :0].contiguous(), t["qty"][:0].contiguous(),
                            lag=1, window=w, tail_probs=c["tail_probs"], min_scen=c["min_scen"], strike_mode=1)
        flat, out = guarded(shapes_of(e))
        engine.svi_hsim_attrib(t["params"], t["Tq"], t["spot"], c["rate"], t["u"][:, :0].contiguous(), t["tau"][:, :0].contiguous(), t["qty"][:0].contiguous(),
                               h["pnl"], h["scen_flags"], out=out, stream=stream, **kw)
        torch.cuda.synchronize()
        g = check_written(flat, out, ("ces_group", "cvar_group", "n_tail", "order"))
        ok = n_p >= c["min_scen"]
        assert np.array_equal(g["n_tail"], np.array([A.tails(n, c["tail_probs"], c["min_scen"]) for n in n_p]))
        assert plus_zero(g["ces_group"][ok]) and plus_zero(g["cvar_group"][ok]) and np.isnan(g["ces_group"][~ok]).all()
        assert np.array_equal(g["order"], np.where(np.arange(w)[None, :] < n_p[:, None], np.arange(w)[None, :], -1))
        flat, out = guarded(shapes_of(c))
        h = engine.svi_hsim(t["params"][:, :0].contiguous(), t["Tq"][:, :0].contiguous(), t["spot"], c["rate"], t["u"], t["tau"], t["qty"], lag=1, window=w,
                            tail_probs=c["tail_probs"], min_scen=c["min_scen"], strike_mode=1)
        engine.svi_hsim_attrib(t["params"][:, :0].contiguous(), t["Tq"][:, :0].contiguous(), t["spot"], c["rate"], t["u"], t["tau"], t["qty"], h["pnl"],
                               h["scen_flags"], out=out, stream=stream, **kw)
        torch.cuda.synchronize()
        g = check_written(flat, out, A.OUT_KEYS)
        assert all(np.isnan(g[k]).all() for k in AC.VALUE_KEYS) and (g["n_tail"] == 0).all() and (g["order"] == -1).all()


def test_explicit_stream_then_immediate_reallocation():
    import torch
    from iv_interpolation_amd import engine
    c, r = case(AC.STREAM_CASE)
    base = value_run(c, r)
    same_bits(base, value_run(c, r, stream=torch.cuda.Stream()), A.OUT_KEYS, "stream")
    s = torch.cuda.Stream()
    with torch.cuda.stream(torch.cuda.Stream()):
        t = inputs(c)
        pnl, fl = dev(r["hsim"]["pnl"]), dev(r["hsim"]["scen_flags"], np.int32)
        torch.cuda.current_stream().synchronize()
        q = engine.svi_hsim_attrib(t["params"], t["Tq"], t["spot"], c["rate"], t["u"], t["tau"], t["qty"], pnl, fl, group=t["group"], n_groups=c["nG"], lag=c["lag"],
                                   window=c["window"], tail_probs=c["tail_probs"], min_scen=c["min_scen"], is_put=t["is_put"], strike_mode=c["strike_mode"], stream=s)
        del t, pnl, fl
        junk = [torch.full(x.shape, 3.0, dtype=torch.float64, device="cuda") for x in (c["params"], c["Tq"], c["spot"], c["u"], c["tau"], c["qty"], r["hsim"]["pnl"]) for _ in range(3)]
        s.synchronize()
        torch.cuda.synchronize()
    same_bits(base, {k: host(v) for k, v in q.items()}, A.OUT_KEYS, "reallocation")
    del junk


def test_abi_error_table():
    import torch
    from iv_interpolation_amd import _lib, engine
    c, r = case("B9-Q65-w63-L8")
    t = inputs(c)
    p, tq_, s, u, tau, qty = (t[k] for k in ("params", "Tq", "spot", "u", "tau", "qty"))
    pnl, fl = dev(r["hsim"]["pnl"]), dev(r["hsim"]["scen_flags"], np.int32)
    kw = dict(window=63, tail_probs=(0.5,), min_scen=1, strike_mode=1)
    f = lambda *a, **k: (lambda: engine.svi_hsim_attrib(*a, **{**kw, **k}))   # noqa: E731
    for bad in (f(p[0], tq_, s, 0.0, u, tau, qty, pnl, fl), f(p, tq_, s, 0.0, u, tau, qty[:-1], pnl, fl), f(p, tq_, s, 0.0, u, tau, qty, pnl[:, :-1], fl),
                f(p, tq_, s, 0.0, u, tau, qty, pnl, fl[:-1]), f(p, tq_, s, 0.0, u, tau, qty, pnl, fl, group=t["group"][:-1]), f(p, tq_, s, 0.0, u, tau, qty, pnl, fl, n_groups=17),
                f(p, tq_, s, 0.0, u, tau, qty, pnl, fl, n_groups=0), f(p, tq_, s, 0.0, u, tau, qty, pnl, fl, lag=0), f(p, tq_, s, 0.0, u, tau, qty, pnl, fl, tail_probs=(1.0,)),
                f(p, tq_, s, 0.0, u, tau, qty, dev(np.zeros((9, 260))), dev(np.zeros((9, 260)), np.int32), window=260, tail_probs=(0.25,)),
                f(p, tq_, s, 0.0, u, tau, qty, pnl, fl, want=("var",)), f(p, tq_, s, 0.0, u, tau, qty, pnl, fl, out={"ces": torch.empty((9, 1, 64), dtype=torch.float64, device="cuda")}),
                f(p, tq_, s, 0.0, u, tau, qty, pnl, fl, out={"order": torch.empty((9, 63), dtype=torch.int64, device="cuda")})):
        with pytest.raises(ValueError):
            bad()
    for bad in (f(p, tq_, s, 0.0, u, tau, qty, pnl.float(), fl), f(p, tq_, s, 0.0, u, tau, qty, pnl, fl.long()), f(p, tq_, s, 0.0, u, tau, qty, pnl, fl, group=t["group"].long())):
        with pytest.raises(TypeError):
            bad()
    lib = _lib.load()
    B, Q, w = 9, u.shape[1], 63
    cc = dict(c, tail_probs=c["tail_probs"])
    bufs = {k: torch.full(shape, SENT_I if dt == torch.int32 else SENT_F, dtype=dt, device="cuda") for k, (shape, dt) in shapes_of(cc).items()}
    a = _lib.HsimAttribArgs()
    a.params, a.Tq, a.tq_stride, a.spot, a.u, a.tau, a.q_stride, a.qty = p.data_ptr(), tq_.data_ptr(), 16, s.data_ptr(), u.data_ptr(), tau.data_ptr(), Q, qty.data_ptr()
    a.mT, a.Q, a.B, a.strike_mode, a.lag, a.window, a.min_scen, a.nG = 16, Q, B, 1, 1, w, c["min_scen"], 2
    a.pnl, a.scen_flags, a.group = pnl.data_ptr(), fl.data_ptr(), t["group"].data_ptr()
    tp = (ctypes.c_double * 8)(*c["tail_probs"])
    a.tail_probs, a.nL = ctypes.cast(tp, ctypes.POINTER(ctypes.c_double)), 8
    for k, v in bufs.items():
        setattr(a, k, v.data_ptr())
    call = lambda: lib.ivs_svi_hsim_attrib_f64(ctypes.byref(a), None, 0, None)       # noqa: E731
    for field, bad, good, code, word in (("lag", 0, 1, -34, b"lag=0"), ("q_stride", 7, Q, -22, b"stride"), ("strike_mode", 2, 1, -22, b"strike_mode"),
                                         ("mT", 65, 16, -34, b"mT=65"), ("Q", -1, Q, -22, b"negative"), ("window", 0, w, -34, b"window=0"),
                                         ("window", 1025, w, -34, b"window=1025"), ("nL", 9, 8, -34, b"nL=9"), ("min_scen", 0, c["min_scen"], -34, b"min_scen=0"),
                                         ("nG", 0, 2, -34, b"nG=0"), ("nG", 17, 2, -34, b"nG=17"), ("window", 130, w, -34, b"tail of 65 > 64")):
        setattr(a, field, bad)
        assert call() == code and word in lib.ivs_last_error() and lib.ivs_last_kernel() == b"", (field, lib.ivs_last_error())
        setattr(a, field, good)
    tp[3] = 1.0
    assert call() == -34 and b"tail probability 3" in lib.ivs_last_error()
    tp[3] = c["tail_probs"][3]
    for k in ("pnl", "scen_flags", "n_tail", "qty", "params"):
        keep = getattr(a, k)
        setattr(a, k, None)
        assert call() == -22 and b"null pointer" in lib.ivs_last_error() and lib.ivs_last_kernel() == b"", k
        setattr(a, k, keep)
    assert lib.ivs_svi_hsim_attrib_f64(None, None, 0, None) == -22
    torch.cuda.synchronize()
    for k, buf in bufs.items():                                              # a refused call launches nothing and touches no buffer
        assert (host(buf) == (SENT_I if buf.dtype == torch.int32 else SENT_F)).all(), k
    assert call() == 0 and lib.ivs_last_kernel() == b"svi_hsim_attrib_kernel"   # and the same struct, accepted, writes everything
    torch.cuda.synchronize()
    for k, buf in bufs.items():
        assert not (host(buf) == (SENT_I if buf.dtype == torch.int32 else SENT_F)).any(), k
    assert np.array_equal(host(bufs["order"]), r["order"]) and np.array_equal(host(bufs["n_tail"]), r["n_tail"])


def test_builder_and_frame_on_a_wide_chain():
    """End to end: the chain of the SVI GPU test through build(), svi(), var() and var_attribution() on the device: the groups add
    up to the VarReport's figures, and with one group they are its bits."""
    import risk_cases as RC
    import svi_cases as SC
    import snapshot_cases as SNC
    from iv_interpolation_amd.snapshots import HipBackend, SnapshotSurfaceBuilder, var_attribution_frame
    b = SnapshotSurfaceBuilder(moneyness=SC.CHAIN_MONEYNESS, tenors=SC.CHAIN_TENORS, backend=HipBackend())
    res = b.build(SNC.big_chain(**SC.CHAIN))
    fits = b.svi(res, rate=SC.CHAIN_RATE)
    bk = RC.chain_book(res)
    kw = dict(rate=SC.CHAIN_RATE, window=16, tail_probs=(0.5, 0.1), min_scenarios=2)
    var = b.var(res, bk, fits, **kw)
    reps = b.var_attribution(res, bk, var, fits, group_by="side", **kw)
    assert [d.underlying for d in reps] == ["btc", "eth"]
    for rp, v, fit, r in zip(reps, var, fits, res):
        es, vr, n_tail = host(v.es), host(v.var), host(rp.n_tail)
        on = n_tail > 0
        assert np.array_equal(on, ~np.isnan(vr)) and on.any() and rp.labels == ["call", "put"]
        ceg, cvg = host(rp.ces_group), host(rp.cvar_group)
        assert np.allclose(ceg.sum(axis=2)[on], es[on], rtol=1e-9, atol=1e-9) and np.allclose(cvg.sum(axis=2)[on], vr[on], rtol=1e-9, atol=1e-9)
        assert np.allclose(np.nansum(host(rp.ces), axis=2)[on], es[on], rtol=1e-9, atol=1e-9)
        u = np.ascontiguousarray(np.broadcast_to(rp.strikes, v.tau.shape))
        one = HipBackend().hsim_attrib(fit.params, r.tenors, r.spot, SC.CHAIN_RATE, u, v.tau, rp.quantity, v.pnl, v.scen_flags,
                                       np.zeros(len(rp.quantity), np.int32), 1, 1, 16, [0.5, 0.1], 2, rp.is_put, 1)
        assert np.array_equal(host(one["cvar_group"])[:, :, 0], vr, equal_nan=True) and np.array_equal(host(one["ces_group"])[:, :, 0], es, equal_nan=True)
    f = var_attribution_frame(reps, res)
    quoted = sum(int((host(r.quotes) > 0).sum()) for r in res)
    assert quoted > 0 and len(f) == quoted * 2 * 2 and set(f["underlying"]) == {"btc", "eth"} and set(f["group"]) == {"call", "put"}
    ok = f["n_tail"] > 0
    assert ok.any() and f["var_start"][ok].notna().all() and np.isfinite(f["ces_share"][ok]).all()
