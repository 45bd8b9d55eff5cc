"""GPU: svi_hsim_kernel and hsim_tail_kernel (ivs_svi_hsim_f64) against the restatement of rules H0-H9 (tests/hsim_ref.py).

Flags, n_valid, n_dead, worst and every NaN pattern equal the restatement's everywhere (the generated batches keep the comparisons
of the rules off their thresholds: hsim_ref.check_margins).  The values agree within C_GPU x R_CPU units of eps x the value's own
scale (hsim_cases.tolerances; DESIGN.md section 19 has the reasoning): R_CPU is the restatement's distance from the same rules in
mpmath at 50 digits, measured by test_hsim.test_rounding_level.  var, es, worst and n_valid are also, to the bit, rule H7
restated on the host and applied to the kernel's own pnl and scen_flags.

Every test prints its largest error / tolerance ratios; with IVS_HSIM_ERRLOG=<file> set the figures are appended to that file as
well (a recorded run belongs in profiles/hsim/errlog_gpu.txt; errlog.txt there holds the CPU run)."""
import ctypes
import os

import numpy as np
import pytest

import hsim_cases as HC
import hsim_ref as H
import risk_ref as R

pytestmark = pytest.mark.gpu
SENT_F, SENT_I = -7.25e9, -77        # no output of the rules: flags and counts >= -1; no value ever hits -7.25e9
GUARD = 67                           # elements of guard tail behind every output
GPU_FACTOR = {k: HC.C_GPU * v for k, v in HC.R_CPU.items()}
INT_KEYS = ("scen_flags", "n_valid", "n_dead", "worst")


def log(name, **figures):
    line = name + ": " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items())
    print(line)
    path = os.environ.get("IVS_HSIM_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def host(t):
    return None if t is None else t.cpu().numpy()


def dev(a, dtype=np.float64):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def shapes_of(c):
    import torch
    B, w, nL = c["params"].shape[0], c["window"], len(c["tail_probs"])
    f, i = torch.float64, torch.int32
    return dict(pnl=((B, w), f), scen_flags=((B, w), i), var=((B, nL), f), es=((B, nL), f), n_valid=((B,), i), n_dead=((B,), i), worst=((B,), i),
                value=((B, 2), f))


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


def run(c, stream=None, value=True, scen_per_wg=0, abi=False):
    """The call through engine.svi_hsim, or (abi) through the C entry point itself, into sentinel-filled outputs."""
    import torch
    from iv_interpolation_amd import _lib, engine
    flat, out = guarded(shapes_of(c))
    keys = tuple(k for k in H.OUT_KEYS if value or k != "value")
    t = dict(params=dev(c["params"]), Tq=dev(c["Tq"]), spot=dev(c["spot"]), u=dev(c["u"]), tau=dev(c["tau"]), qty=dev(c["qty"]), is_put=dev(c["is_put"], np.uint8))
    if abi:
        a = _lib.HsimArgs()
        B, mT = c["params"].shape[:2]
        Q = len(c["qty"])
        for k, v in t.items():
            setattr(a, k, 0 if v is None else v.data_ptr())
        a.tq_stride, a.q_stride, a.rate = (mT if np.ndim(c["Tq"]) == 2 else 0), (Q if np.ndim(c["u"]) == 2 else 0), c["rate"]
        a.strike_mode, a.mT, a.Q, a.B, a.lag, a.window = c["strike_mode"], mT, Q, B, c["lag"], c["window"]
        tp = list(c["tail_probs"])
        a.tail_probs, a.nL, a.min_scen, a.scen_per_wg = ctypes.cast((ctypes.c_double * max(len(tp), 1))(*tp), ctypes.POINTER(ctypes.c_double)), len(tp), c["min_scen"], scen_per_wg
        for k in keys:
            setattr(a, k, out[k].data_ptr())
        lib = _lib.load()
        assert lib.ivs_svi_hsim_f64(ctypes.byref(a), None, 0, None) == 0, lib.ivs_last_error()
        assert lib.ivs_last_kernel() == b"hsim_tail_kernel"
    else:
        q = engine.svi_hsim(t["params"], t["Tq"], t["spot"], c["rate"], t["u"], t["tau"], t["qty"], lag=c["lag"], window=c["window"], tail_probs=c["tail_probs"],
                            min_scen=c["min_scen"], is_put=t["is_put"], strike_mode=c["strike_mode"], value=value, out={k: out[k] for k in keys}, stream=stream,
                            scen_per_wg=scen_per_wg)
        assert engine.last_kernel() == "hsim_tail_kernel" and set(q) == set(H.OUT_KEYS)
        assert value or q["value"] is None
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    if not value:
        assert (host(flat["value"]) == SENT_F).all()                         # left out: its buffer untouched
    keys = tuple(k for k in keys if len(c["tail_probs"]) or k not in ("var", "es"))
    got = check_written(flat, out, keys)
    for k in H.OUT_KEYS:
        got.setdefault(k, None if k == "value" and not value else host(out[k]))
    return got


def ref_of(c, margins=False, unordered=False):
    r = H.restate_hsim(c["params"], c["Tq"], c["spot"], c["rate"], c["u"], c["tau"], c["qty"], c["lag"], c["window"], c["tail_probs"], c["min_scen"],
                       c["is_put"], c["strike_mode"])
    if margins:
        H.check_margins(r, factor=GPU_FACTOR["pnl"], unordered=unordered)
    return r


def compare(name, got, ref, c):
    for k in INT_KEYS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), (name, k, got[k], ref[k])
    u = HC.units(got, ref)
    fig = {k: (float(np.nanmax(v)) / GPU_FACTOR[k] if np.isfinite(v).any() else 0.0) for k, v in u.items()}
    log(name, **fig, scenarios=int(ref["exists"].sum()), valid=int(ref["n_valid"].sum()), options=int(ref["live"].size))
    for k in u:
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (name, k)
    assert all(v <= 1.0 for v in fig.values()), (name, fig)
    h7_on_own_rows(name, got, c)


def h7_on_own_rows(name, got, c):
    """var, es, worst and n_valid are rule H7 on the kernel's own pnl and scen_flags: the same bits."""
    var, es, n_valid, worst = H.tail(got["pnl"], got["scen_flags"], c["tail_probs"], c["min_scen"])
    assert np.array_equal(got["n_valid"], n_valid) and np.array_equal(got["worst"], worst), name
    for k, v in (("var", var), ("es", es)):
        assert np.array_equal(got[k], v, equal_nan=True) and np.array_equal(np.signbit(got[k]), np.signbit(v)), (name, k)


def same_bits(a, b, keys, what):
    for k in keys:
        if a[k] is None:
            assert b[k] is None, (k, what)
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), (k, what)


def plus_zero(a):
    a = np.asarray(a)
    return bool((a == 0.0).all() and not np.signbit(a).any())


_cache = {}


def case(n):
    """Inputs and restatement of one generated batch, computed once and shared (read-only)."""
    if n not in _cache:
        c = HC.make(n)
        r = ref_of(c, margins=True, unordered=n in HC.UNORDERED_SHAPES)
        for a in list(c.values()) + list(r.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[n] = (c, r)
    return _cache[n]


def rows_of(c, rows, **more):
    """The snapshots `rows` of `c` as a batch of their own."""
    B = len(c["spot"])
    pick = lambda a: a[rows] if np.ndim(a) == 2 and a.shape[0] == B else a    # noqa: E731
    return dict(c, params=c["params"][rows], spot=c["spot"][rows], Tq=pick(c["Tq"]), u=pick(c["u"]), tau=pick(c["tau"]), **more)


@pytest.mark.parametrize("name", sorted(HC.MICRO))
def test_micro(name):
    c = HC.MICRO[name]
    g = run(c)
    assert np.array_equal(g["scen_flags"], c["scen_flags"]) and np.array_equal(g["n_valid"], c["n_valid"]) and np.array_equal(g["n_dead"], c["n_dead"])
    compare(f"micro[{name}]", g, ref_of(c), c)
    same_bits(g, run(c, abi=True), H.OUT_KEYS, "C ABI")


@pytest.mark.parametrize("n", range(len(HC.SHAPES)), ids=[HC.shape_id(s) for s in HC.SHAPES])
def test_shapes(n):
    c, r = case(n)
    g = run(c)
    compare(f"shape[{HC.shape_id(HC.SHAPES[n])}]", g, r, c)
    if n % 2:
        same_bits(g, run(c, abi=True), H.OUT_KEYS, "C ABI")


@pytest.mark.parametrize("name", sorted(HC.ROWS))
def test_h7_rows_through_the_tail_kernel_alone(name):
    """stages = 2: the order statistics of rows given directly: m round an integer, ties with -0.0 against +0.0, flags, too few."""
    import torch
    from iv_interpolation_amd import engine
    pnl, fl, tp, min_scen, var, es, n_valid, worst = HC.ROWS[name]
    c, _ = case(0)                                                           # B = 1: the inputs are not read by the tail kernel
    out = dict(pnl=dev([pnl]), scen_flags=dev([fl], np.int32))
    q = engine.svi_hsim(dev(c["params"]), dev(c["Tq"]), dev(c["spot"]), 0.0, dev(c["u"]), dev(c["tau"]), dev(c["qty"]), window=len(pnl), tail_probs=tp,
                        min_scen=min_scen, out=out, stages=2)
    torch.cuda.synchronize()
    g = {k: host(q[k])[0] for k in ("var", "es", "n_valid", "worst")}
    assert np.array_equal(g["var"], var, equal_nan=True) and np.array_equal(g["es"], es, equal_nan=True) and g["n_valid"] == n_valid and g["worst"] == worst
    assert np.array_equal(np.signbit(g["var"]), np.signbit(np.asarray(var))) and np.array_equal(np.signbit(g["es"]), np.signbit(np.asarray(es)))
    assert np.array_equal(host(q["pnl"])[0], pnl, equal_nan=True)            # read, not written


def test_wide_rows_through_the_tail_kernel_alone():
    """window 257 and 1024 with ties, zeros of both signs and flagged entries, against H7 on the host."""
    import torch
    from iv_interpolation_amd import engine
    c, _ = case(0)
    rng = np.random.default_rng(1950)
    for w in (257, 1024):
        pnl = np.round(rng.normal(size=(1, w)), 1)                           # many ties
        pnl[0, ::17] = -0.0
        fl = np.where(rng.random((1, w)) < 0.1, rng.integers(1, 8, (1, w)), 0).astype(np.int32)
        pnl[0, 5::29] = np.nan
        q = engine.svi_hsim(dev(c["params"]), dev(c["Tq"]), dev(c["spot"]), 0.0, dev(c["u"]), dev(c["tau"]), dev(c["qty"]), window=w, tail_probs=HC.LEVELS8,
                            min_scen=20, out=dict(pnl=dev(pnl), scen_flags=dev(fl, np.int32)), stages=2)
        torch.cuda.synchronize()
        h7_on_own_rows(f"wide[{w}]", dict({k: host(v) for k, v in q.items()}, pnl=pnl, scen_flags=fl), dict(tail_probs=HC.LEVELS8, min_scen=20))


def test_same_bits_across_runs_splits_batches_and_windows():
    """H4: two runs; every scen_per_wg; a scenario inside B = 70 against the three-snapshot call on p and the pair's ends alone;
    window 4 against the first four of window 65."""
    c, _ = case(4)                                                           # B = 70, lag 1, window 65
    base = run(c)
    same_bits(base, run(c), H.OUT_KEYS, "second run")
    for spw in (1, 2, 7, 64, 65):
        same_bits(base, run(c, scen_per_wg=spw), H.OUT_KEYS, f"scen_per_wg {spw}")
    for p, s in ((69, 5), (33, 32), (12, 0), (69, 64)):
        ja, jb = p - 1 - s, p - s
        rows = [ja, jb, p] if jb != p else [ja, p]
        alone = run(rows_of(c, rows, window=2))
        assert np.array_equal(alone["pnl"][-1, len(rows) - 2], base["pnl"][p, s]) and alone["scen_flags"][-1, len(rows) - 2] == 0, (p, s)
        assert np.array_equal(alone["value"][-1], base["value"][p])
    short = run(dict(c, window=4))
    assert np.array_equal(short["pnl"], base["pnl"][:, :4], equal_nan=True) and np.array_equal(short["scen_flags"], base["scen_flags"][:, :4])
    c7, _ = case(7)                                                          # lag 2: both ends staged afresh
    b7 = run(c7)
    for spw in (1, 7, 64):
        same_bits(b7, run(c7, scen_per_wg=spw), H.OUT_KEYS, f"lag 2, scen_per_wg {spw}")
    alone = run(rows_of(c7, [10, 12, 40], lag=1, window=2))                  # scenario (10, 12) of snapshot 40: s = 28 at lag 2
    assert np.array_equal(alone["pnl"][2, 1], b7["pnl"][40, 28])
    c9, _ = case(9)                                                          # window 257 at B = 260: a run of 257 is two sub-runs of a workgroup
    b9 = run(c9)
    assert (b9["scen_flags"][258:, 256] == 0).all() and (b9["scen_flags"][:257, 256] == HC.ABSENT).all()
    for spw in (257, 256, 100, 1):
        same_bits(b9, run(c9, scen_per_wg=spw), H.OUT_KEYS, f"window 257, scen_per_wg {spw}")


def test_h6_identical_ends_give_plus_zero():
    g = run(HC.MICRO["same_pair"])
    assert plus_zero(g["pnl"][1, 0]) and plus_zero(g["pnl"][2, 1]) and g["pnl"][2, 0] != 0.0 and plus_zero(g["var"][1]) and plus_zero(g["es"][1])
    c, _ = case(3)                                                           # a generated batch with one pair duplicated
    twin = dict(c, params=c["params"].copy(), spot=c["spot"].copy(), Tq=c["Tq"].copy())
    twin["params"][4], twin["spot"][4], twin["Tq"][4] = twin["params"][3], twin["spot"][3], twin["Tq"][3]
    g = run(twin)
    for p in range(4, 9):
        assert plus_zero(g["pnl"][p, p - 4]), p
    assert (g["pnl"][5:, 0] != 0.0).all()
    for spw in (1, 7):
        same_bits(g, run(twin, scen_per_wg=spw), H.OUT_KEYS, spw)


def test_value_is_the_b5_sum_of_the_greeks_calls_price():
    import torch
    from iv_interpolation_amd import engine
    for n in (1, 3, 6):
        c, r = case(n)
        g = run(c)
        q = engine.svi_greeks(dev(c["params"]), dev(c["Tq"]), dev(c["spot"]), c["rate"], dev(c["u"]), dev(c["tau"]), is_put=dev(c["is_put"], np.uint8),
                              strike_mode=c["strike_mode"], want=("price",))
        torch.cuda.synchronize()
        price = np.nan_to_num(host(q["price"]))
        qty = np.where(np.isfinite(c["qty"]), c["qty"], 0.0)[None, :]
        assert np.array_equal(R.b5_sum(np.where(r["live"], qty * price, 0.0)), g["value"][:, 0]), n
        assert np.array_equal(R.b5_sum(np.where(r["live"], np.abs(qty) * price, 0.0)), g["value"][:, 1]), n
        assert np.array_equal(g["n_dead"], (~r["live"]).sum(axis=1))


def test_books_of_one_option():
    """Every 9th option of a batch alone at its own quantity: the scenario P&L is that option's term, nothing averaged out."""
    c, _ = case(3)
    worst = 0.0
    for q in range(0, len(c["qty"]), 9):
        solo = dict(c, qty=np.where(np.arange(len(c["qty"])) == q, c["qty"], 0.0))
        g, r = run(solo), ref_of(solo)
        for k in INT_KEYS:
            assert np.array_equal(g[k], r[k]), (q, k)
        u = HC.units(g, r, ("pnl", "var", "es"))
        for k, v in u.items():
            if np.isfinite(v).any():
                worst = max(worst, float(np.nanmax(v)) / GPU_FACTOR[k])
    log("one-option books", worst=worst)
    assert worst <= 1.0


def test_null_value_leaves_the_rest_unchanged():
    c, _ = case(3)
    keys = tuple(k for k in H.OUT_KEYS if k != "value")
    same_bits(run(c), run(c, value=False), keys, "value left out")
    same_bits(run(c), run(c, value=False, abi=True), keys, "value NULL through the C ABI")


def test_empty_inputs_through_the_wrapper():
    """H9: the C call writes nothing with Q == 0 or mT == 0; the wrapper defines the result.  B <= lag is not empty."""
    import torch
    from iv_interpolation_amd import engine
    c, _ = case(3)
    p, t, s, u, tq, qty = (dev(c[k]) for k in ("params", "Tq", "spot", "u", "tau", "qty"))
    B, Q, w = 9, u.shape[1], c["window"]
    n_p, ex = H.exists(B, 1, w)
    kw = dict(lag=1, window=w, tail_probs=c["tail_probs"], min_scen=c["min_scen"], strike_mode=1)
    for stream in (None, torch.cuda.Stream()):
        flat, out = guarded(shapes_of(c))
        engine.svi_hsim(p, t, s, c["rate"], u[:, :0].contiguous(), tq[:, :0].contiguous(), qty[:0].contiguous(), out=out, stream=stream, **kw)
        torch.cuda.synchronize()
        g = check_written(flat, out, H.OUT_KEYS)
        assert plus_zero(g["pnl"][ex]) and np.isnan(g["pnl"][~ex]).all() and np.array_equal(g["scen_flags"], np.where(ex, 0, HC.ABSENT))
        ok = n_p >= c["min_scen"]
        assert plus_zero(g["var"][ok]) and plus_zero(g["es"][ok]) and np.isnan(g["var"][~ok]).all() and np.isnan(g["es"][~ok]).all()
        assert np.array_equal(g["n_valid"], n_p) and np.array_equal(g["worst"], np.where(n_p > 0, 0, -1)) and plus_zero(g["value"]) and (g["n_dead"] == 0).all()
        flat, out = guarded(shapes_of(c))
        engine.svi_hsim(p[:, :0].contiguous(), t[:, :0].contiguous(), s, c["rate"], u, tq, qty, out=out, stream=stream, **kw)
        torch.cuda.synchronize()
        g = check_written(flat, out, H.OUT_KEYS)
        assert np.isnan(g["pnl"]).all() and np.array_equal(g["scen_flags"], np.where(ex, HC.VOID, HC.ABSENT)) and np.isnan(g["var"]).all() and np.isnan(g["es"]).all()
        assert (g["n_valid"] == 0).all() and (g["worst"] == -1).all() and np.isnan(g["value"]).all() and (g["n_dead"] == Q).all()
    g = run(dict(c, lag=9, window=5))                                        # B <= lag: launched, every scenario ABSENT
    assert (g["scen_flags"] == HC.ABSENT).all() and np.isnan(g["pnl"]).all() and (g["n_valid"] == 0).all() and np.isfinite(g["value"]).all()


def test_explicit_stream_then_immediate_reallocation():
    import torch
    from iv_interpolation_amd import engine
    c, r = case("stream")
    base = run(c)
    compare("stream", base, r, c)
    same_bits(base, run(c, stream=torch.cuda.Stream()), H.OUT_KEYS, "stream")
    s = torch.cuda.Stream()
    with torch.cuda.stream(torch.cuda.Stream()):
        q = engine.svi_hsim(dev(c["params"]), dev(c["Tq"]), dev(c["spot"]), c["rate"], dev(c["u"]), dev(c["tau"]), dev(c["qty"]), lag=c["lag"], window=c["window"],
                            tail_probs=c["tail_probs"], min_scen=c["min_scen"], is_put=dev(c["is_put"], np.uint8), strike_mode=c["strike_mode"], stream=s)
        junk = [torch.full(x.shape, 3.0, dtype=torch.float64, device="cuda") for x in (c["params"], c["Tq"], c["spot"], c["u"], c["tau"], c["qty"]) for _ in range(3)]
        s.synchronize()
        torch.cuda.synchronize()
    same_bits(base, {k: host(v) for k, v in q.items()}, H.OUT_KEYS, "reallocation")
    del junk


def test_abi_error_table():
    import torch
    from iv_interpolation_amd import _lib, engine
    c, _ = case(3)
    p, t, s, u, tq, qty = (dev(c[k]) for k in ("params", "Tq", "spot", "u", "tau", "qty"))
    side = dev(np.zeros(u.shape[1]), np.uint8)
    f = lambda *a, **k: (lambda: engine.svi_hsim(*a, **k))                    # noqa: E731
    for bad in (f(p[0], t, s, 0.0, u, tq, qty), f(p, t, s, 0.0, u, tq[:, :-1], qty), f(p, t, s, 0.0, u, tq, qty, strike_mode=2), f(p, t, s, 0.0, u, tq, qty[:-1]),
                f(p, t, s, 0.0, u, tq, qty, is_put=side[:-1]), f(p, t, s, 0.0, u, tq, qty, lag=0), f(p, t, s, 0.0, u, tq, qty, lag=1.5),
                f(p, t, s, 0.0, u, tq, qty, window=0), f(p, t, s, 0.0, u, tq, qty, window=1025), f(p, t, s, 0.0, u, tq, qty, tail_probs=(0.0,)),
                f(p, t, s, 0.0, u, tq, qty, tail_probs=(0.5,) * 9), f(p, t, s, 0.0, u, tq, qty, min_scen=0), f(p, t, s, 0.0, u, tq, qty, window=4, scen_per_wg=5),
                f(p, t, s, 0.0, u, tq, qty, stages=3), f(p, t, s, 0.0, u, tq, qty, out={"pnl": torch.empty((9, 8), dtype=torch.float64, device="cuda")}),
                f(p, t, s, 0.0, u, tq, qty, out={"worst": torch.empty(9, dtype=torch.int64, device="cuda")})):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        engine.svi_hsim(p, t, s, 0.0, u.float(), tq, qty)
    lib = _lib.load()
    B, Q, w = 9, u.shape[1], 4
    bufs = {k: torch.full(shape, SENT_I if dt == torch.int32 else SENT_F, dtype=dt, device="cuda") for k, (shape, dt) in shapes_of(dict(c, window=w)).items()}
    a = _lib.HsimArgs()
    a.params, a.Tq, a.tq_stride, a.spot, a.u, a.tau, a.q_stride, a.qty = p.data_ptr(), t.data_ptr(), 16, s.data_ptr(), u.data_ptr(), tq.data_ptr(), Q, qty.data_ptr()
    a.mT, a.Q, a.B, a.strike_mode, a.lag, a.window, a.min_scen = 16, Q, B, 1, 1, w, 1
    tp = (ctypes.c_double * 8)(*c["tail_probs"])
    a.tail_probs, a.nL = ctypes.cast(tp, ctypes.POINTER(ctypes.c_double)), 8
    for k, v in bufs.items():
        setattr(a, k, v.data_ptr())
    call = lambda: lib.ivs_svi_hsim_f64(ctypes.byref(a), None, 0, None)       # noqa: E731
    for field, bad, good, code, word in (("lag", 0, 1, -34, b"lag=0"), ("q_stride", 7, Q, -22, b"stride"), ("strike_mode", 2, 1, -22, b"strike_mode"),
                                         ("mT", 65, 16, -34, b"mT=65"), ("Q", -1, Q, -22, b"negative"), ("window", 0, w, -34, b"window=0"),
                                         ("window", 1025, w, -34, b"window=1025"), ("nL", 9, 8, -34, b"nL=9"), ("min_scen", 0, 1, -34, b"min_scen=0"),
                                         ("scen_per_wg", 5, 0, -34, b"scen_per_wg=5"), ("stages", -1, 0, -34, b"stages=-1")):
        setattr(a, field, bad)
        assert call() == code and word in lib.ivs_last_error() and lib.ivs_last_kernel() == b"", (field, lib.ivs_last_error())
        setattr(a, field, good)
    tp[3] = 1.0
    assert call() == -34 and b"tail probability 3" in lib.ivs_last_error()
    tp[3] = c["tail_probs"][3]
    for k in ("pnl", "scen_flags", "var", "es", "n_valid", "n_dead", "worst", "qty"):
        keep = getattr(a, k)
        setattr(a, k, None)
        assert call() == -22 and b"null pointer" in lib.ivs_last_error() and lib.ivs_last_kernel() == b"", k
        setattr(a, k, keep)
    assert lib.ivs_svi_hsim_f64(None, None, 0, None) == -22
    torch.cuda.synchronize()
    for k, buf in bufs.items():                                              # a refused call launches nothing and touches no buffer
        assert (host(buf) == (SENT_I if buf.dtype == torch.int32 else SENT_F)).all(), k
    assert call() == 0 and lib.ivs_last_kernel() == b"hsim_tail_kernel"      # and the same struct, accepted, writes everything
    torch.cuda.synchronize()
    for k, buf in bufs.items():
        assert not (host(buf) == (SENT_I if buf.dtype == torch.int32 else SENT_F)).any(), k


def test_builder_and_frame_on_a_wide_chain():
    """End to end: the chain of the SVI GPU test through build(), svi() and var() on the device.  The restatement is fed the
    kernel's own `params` copied back, so the late-round ties of the fit play no part."""
    import risk_cases as RC
    import svi_cases as SC
    import snapshot_cases as SNC
    from iv_interpolation_amd.snapshots import HipBackend, SnapshotSurfaceBuilder, var_frame
    ten = SC.CHAIN_TENORS
    b = SnapshotSurfaceBuilder(moneyness=SC.CHAIN_MONEYNESS, tenors=ten, backend=HipBackend())
    res = b.build(SNC.big_chain(**SC.CHAIN))
    fits = b.svi(res, rate=SC.CHAIN_RATE)
    bk = RC.chain_book(res)
    reps = b.var(res, bk, fits, rate=SC.CHAIN_RATE, window=16, tail_probs=(0.5, 0.1), min_scenarios=2)
    assert [d.underlying for d in reps] == ["btc", "eth"]
    for rp, v, r in zip(reps, fits, res):
        c = dict(params=host(v.params), Tq=ten, spot=host(r.spot), rate=SC.CHAIN_RATE, u=np.ascontiguousarray(np.broadcast_to(rp.strikes, rp.tau.shape)),
                 tau=rp.tau, strike_mode=1, is_put=rp.is_put, qty=rp.quantity, lag=1, window=16, tail_probs=(0.5, 0.1), min_scen=2)
        got = {k: host(getattr(rp, k)) for k in H.OUT_KEYS}
        ref = ref_of(c)
        h7_on_own_rows(f"builder[{rp.underlying}]", got, c)
        for k in ("scen_flags", "n_dead"):
            assert np.array_equal(got[k], ref[k]), k
        u = HC.units(got, ref, ("pnl", "value"))
        fig = {k: float(np.nanmax(v)) / GPU_FACTOR[k] if np.isfinite(v).any() else 0.0 for k, v in u.items()}
        log(f"builder[{rp.underlying}]", **fig)
        assert all(v <= 1.0 for v in fig.values()), fig
    f = var_frame(reps, res)
    quoted = sum(int((host(r.quotes) > 0).sum()) for r in res)
    assert quoted > 0 and len(f) == quoted and set(f["underlying"]) == {"btc", "eth"} and list(f.columns)[4:8] == ["var_0.5", "es_0.5", "var_0.1", "es_0.1"]
    btc = f[f["underlying"] == "btc"]
    assert (btc["n_dead"] == 2).all() and (btc["gross"] > 0).all()           # the expired option and the NaN quantity
    ok = btc["var_0.1"].notna()
    assert ok.any() and (btc["var_0.5"][ok] <= btc["var_0.1"][ok]).all() and (btc["var_0.1"][ok] <= btc["es_0.1"][ok]).all()
