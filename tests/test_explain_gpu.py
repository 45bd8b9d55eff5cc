"""GPU: svi_explain_kernel (ivs_svi_explain_f64) against the restatement of rules X0-X9 (tests/explain_ref.py).

Flags, n_dead and every NaN pattern equal the restatement's everywhere (the generated batches keep the comparisons of the rules
off their thresholds: explain_ref's margins).  The values agree within C_GPU x R_CPU units of eps x the value's own scale
(explain_cases.tolerances; DESIGN.md section 18 has the reasoning): R_CPU is the restatement's distance from the same rules in
mpmath at 50 digits, measured by test_explain.test_rounding_level.

Every test prints its largest error / tolerance ratios; with IVS_EXPLAIN_ERRLOG=<file> set the figures are appended to that file
as well (a recorded run belongs in profiles/explain/errlog_gpu.txt; errlog.txt there holds the CPU run)."""
import ctypes
import os

import numpy as np
import pytest

import explain_cases as XC
import explain_ref as X
import risk_ref as R

pytestmark = pytest.mark.gpu
SENT_F, SENT_I = -7.25e9, -77        # no output of the rules: flags and counts >= 0; no value ever hits -7.25e9
GUARD = 67                           # elements of guard tail behind every output
GPU_FACTOR = {k: XC.C_GPU * v for k, v in XC.R_CPU.items()}
INT_KEYS = ("flags", "n_dead")


def log(name, **figures):
    line = name + ": " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items())
    print(line)
    path = os.environ.get("IVS_EXPLAIN_ERRLOG")
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
    B, Q = c["params"].shape[0], len(c["qty"])
    P = max(B - c["lag"], 0)
    s = {k: ((P, Q), torch.float64) for k in X.KEYS}
    s.update(flags=((P, Q), torch.int32), net=((P, 12), torch.float64), n_dead=((P,), torch.int32))
    return s


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


def run(c, stream=None, want=X.KEYS):
    import torch
    from iv_interpolation_amd import engine
    flat, out = guarded(shapes_of(c))
    keys = tuple(want) + ("flags", "net", "n_dead")
    q = engine.svi_explain(dev(c["params"]), dev(c["Tq"]), dev(c["spot"]), c["rate"], dev(c["u"]), dev(c["tau"]), dev(c["qty"]), lag=c["lag"],
                           is_put=dev(c["is_put"], np.uint8), strike_mode=c["strike_mode"], want=want, out={k: out[k] for k in keys}, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    assert engine.last_kernel() == "svi_explain_kernel" and set(q) == set(X.OUT_KEYS)
    for k in X.KEYS:
        if k not in want:                                                    # left out: None, and its buffer untouched
            assert q[k] is None and (host(flat[k]) == SENT_F).all(), k
    got = check_written(flat, out, keys)
    got.update({k: None for k in X.KEYS if k not in want})
    return got


def ref_of(c, margins=False):
    return X.restate_explain(c["params"], c["Tq"], c["spot"], c["rate"], c["u"], c["tau"], c["qty"], c["lag"], c["is_put"], c["strike_mode"], margins=margins)


def compare(name, got, ref):
    assert got["flags"].dtype == np.int32 and got["n_dead"].dtype == np.int32
    u = XC.units(got, ref)
    fig = {k: (float(np.nanmax(v)) / GPU_FACTOR[k] if np.isfinite(v).any() else 0.0) for k, v in u.items()}
    log(name, **fig, options=int(ref["live"].size), live=int(ref["live"].sum()))
    assert np.array_equal(got["flags"], ref["flags"]), (name, got["flags"], ref["flags"])
    assert np.array_equal(got["n_dead"], ref["n_dead"]), (name, got["n_dead"], ref["n_dead"])
    for k in u:
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (name, k)
    assert all(v <= 1.0 for v in fig.values()), (name, fig)


def same_bits(a, b, keys, what):
    for k in keys:
        if a[k] is None:
            assert b[k] is None, (k, what)
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), (k, what)


def plus_zero(a):
    return bool((a == 0.0).all() and not np.signbit(a).any())


_cache = {}


def case(n):
    """Inputs and restatement of one generated batch (n = "path": the smooth path), computed once and shared (read-only)."""
    if n not in _cache:
        c = XC.path(**XC.PATH_SHAPE) if n == "path" else XC.batch(**XC.SHAPES[n])
        r = ref_of(c, margins=n not in XC.UNORDERED_SHAPES)
        for a in list(c.values()) + list(r.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[n] = (c, r)
    return _cache[n]


def pair_of(c, p):
    """The pair p of `c` as a batch of its own two snapshots."""
    rows = [p, p + c["lag"]]
    pick = lambda a: a[rows] if a.ndim == 2 else a                            # noqa: E731
    return dict(c, params=c["params"][rows], Tq=pick(c["Tq"]), spot=c["spot"][rows], u=pick(c["u"]), tau=pick(c["tau"]), lag=1)


@pytest.mark.parametrize("name", sorted(XC.MICRO))
def test_micro(name):
    c = XC.MICRO[name]
    g = run(c)
    assert np.array_equal(g["flags"], c["flags"]) and np.array_equal(g["n_dead"], c["n_dead"]), (g["flags"], g["n_dead"])
    compare(f"micro[{name}]", g, ref_of(c))


@pytest.mark.parametrize("n", range(len(XC.SHAPES)), ids=[XC.shape_id(s) for s in XC.SHAPES])
def test_shapes(n):
    c, r = case(n)
    compare(f"shape[{XC.shape_id(XC.SHAPES[n])}]", run(c), r)


def test_smooth_path():
    c, r = case("path")
    compare("path", run(c), r)


def test_x8_same_ends_give_plus_zero_and_both_corollaries():
    g = run(XC.MICRO["same_ends"])
    for k in X.KEYS:
        assert plus_zero(g[k]), k
    assert plus_zero(g["net"][:, :10]) and (g["net"][:, 11] > 0).all() and (g["n_dead"] == 0).all()
    c, _ = case(3)                                                           # a generated batch whose end 1 is made a copy of end 0
    twin = pair_of(c, 0)
    twin = dict(twin, params=twin["params"][[0, 0]], Tq=twin["Tq"][[0, 0]], spot=twin["spot"][[0, 0]], u=twin["u"][[0, 0]], tau=twin["tau"][[0, 0]])
    g, r = run(twin), ref_of(twin)
    assert r["live"].sum() > 50
    for k in X.KEYS:
        assert plus_zero(g[k][r["live"]]) and np.isnan(g[k][~r["live"]]).all(), k
    assert plus_zero(g["net"][:, :10])
    t = run(XC.MICRO["time_step"])                                           # a pure time step
    for k in ("delta_ss", "gamma_ss", "vega_ss", "delta_sm", "gamma_sm", "vega_sm"):
        assert (t[k] == 0.0).all(), k
    assert (t["theta_pnl"] != 0.0).all() and np.array_equal(t["resid_ss"], t["resid_sm"])
    late = dict(twin, tau=np.stack([twin["tau"][0], twin["tau"][0] - XC.MINUTE]))
    t, r = run(late), ref_of(late)
    for k in ("delta_ss", "gamma_ss", "vega_ss", "delta_sm", "gamma_sm", "vega_sm"):
        assert (t[k][r["live"]] == 0.0).all(), k
    s = run(XC.MICRO["spot_step"])                                           # a pure spot step
    assert (s["vega_sm"] == 0.0).all() and (s["vega_ss"] != 0.0).any() and (s["theta_pnl"] == 0.0).all()
    moved = dict(twin, spot=twin["spot"] * np.array([1.0, 1.003]))
    s, r = run(moved), ref_of(moved)
    assert (s["vega_sm"][r["live"]] == 0.0).all() and (s["delta_sm"][r["live"]] != 0.0).any()


def test_net_is_the_b5_sum_of_the_kernels_own_values():
    for n in (1, 2, 4, "path"):
        c, r = case(n)
        g = run(c)
        live = r["live"]
        qty = np.where(np.isfinite(c["qty"]), c["qty"], 0.0)[None, :]
        for k_, k in enumerate(X.KEYS):
            term = np.where(live, qty * np.nan_to_num(g[k]), 0.0)
            assert np.array_equal(R.b5_sum(term), g["net"][:, k_]), (n, k)    # the same terms in the order of X7: the same bits
        assert np.array_equal(g["n_dead"], (~live).sum(axis=1))


def test_same_bits_across_runs_batches_and_lags():
    """Two runs give identical bits; a pair computed alone equals the same pair inside B = 65; lag 2 equals the two-snapshot call
    on the pair's own ends."""
    c, _ = case(4)                                                           # B = 65
    base = run(c)
    same_bits(base, run(c), X.OUT_KEYS, "second run")
    for p in (0, 31, 63):
        same_bits({k: base[k][p:p + 1] for k in X.OUT_KEYS}, run(pair_of(c, p)), X.OUT_KEYS, f"pair {p} alone")
    for n in (2, 5, 10):                                                     # lag 2 at B = 3, shared and per-snapshot inputs
        c, _ = case(n)
        same_bits(run(c), run(pair_of(c, 0)), X.OUT_KEYS, f"lag 2 of shape {n}")
    c, _ = case(8)                                                           # lag = B - 1 = 64
    same_bits(run(c), run(pair_of(c, 0)), X.OUT_KEYS, "lag 64")


def test_p0_and_flags_are_the_greeks_calls():
    """net[10] is the B5 sum of qty x svi_greeks' price of the pair's first snapshot: P0 is that price to the bit; bits 0-7 of the
    flags are that call's flags."""
    import torch
    from iv_interpolation_amd import engine
    for n in (3, "path"):
        c, r = case(n)
        g = run(c)
        q = engine.svi_greeks(dev(c["params"]), dev(c["Tq"]), dev(c["spot"]), c["rate"], dev(c["u"]), dev(c["tau"]), is_put=dev(c["is_put"], np.uint8),
                              strike_mode=c["strike_mode"], want=("price",))
        torch.cuda.synchronize()
        P = r["P"]
        price, fl = host(q["price"])[:P], host(q["flags"])[:P]
        assert np.array_equal(g["flags"] & 0xff, fl)
        qty = np.where(np.isfinite(c["qty"]), c["qty"], 0.0)[None, :]
        term = np.where(r["live"], qty * np.nan_to_num(price), 0.0)
        assert np.array_equal(R.b5_sum(term), g["net"][:, 10]) and np.array_equal(R.b5_sum(np.abs(qty) * np.where(r["live"], np.nan_to_num(price), 0.0)), g["net"][:, 11])
        for q_ in range(0, len(c["qty"]), 9):                                # a book of option q_ alone at quantity 1: net[10] is its P0 itself
            solo = run(dict(c, qty=np.where(np.arange(len(c["qty"])) == q_, 1.0, 0.0)), want=())
            assert np.array_equal(solo["net"][:, 10], np.where(r["a"]["ok"][:, q_] & r["b"]["ok"][:, q_] & r["Lc"]["ok"][:, q_], price[:, q_], 0.0)), (n, q_)
        # and per option: P1 of pair p is P0 of pair p + lag wherever the contract is the same (the path's absolute strikes)
        if n == "path":
            p1 = g["actual"] + price
            both = r["live"][:-1] & r["live"][1:]
            tol = XC.tolerances(r, GPU_FACTOR)["actual"]
            assert (np.abs(p1[:-1] - price[1:P])[both] <= tol[:-1][both]).all()


def test_optional_outputs_left_out():
    c, _ = case(3)
    full = run(c)
    for want in (("actual",), (), ("resid_ss", "resid_sm"), ("theta_pnl", "delta_sm", "gamma_sm", "vega_sm"), X.KEYS[:5]):
        part = run(c, want=want)
        keys = tuple(want) + ("flags", "net", "n_dead")
        same_bits({k: full[k] for k in keys}, part, keys, want)


def test_empty_inputs_through_the_wrapper():
    """X9: the C call writes nothing with Q == 0, mT == 0 or B <= lag; the wrapper defines the result."""
    import torch
    from iv_interpolation_amd import engine
    c, _ = case(3)
    p, t, s, u, tq, qty = (dev(c[k]) for k in ("params", "Tq", "spot", "u", "tau", "qty"))
    Q = u.shape[1]
    for stream in (None, torch.cuda.Stream()):
        flat, out = guarded(shapes_of(dict(c, qty=c["qty"][:0])))
        q = engine.svi_explain(p, t, s, c["rate"], u[:, :0].contiguous(), tq[:, :0].contiguous(), qty[:0].contiguous(), strike_mode=1, out=out, stream=stream)
        torch.cuda.synchronize()
        got = check_written(flat, out, ("net", "n_dead"))
        assert plus_zero(got["net"]) and (got["n_dead"] == 0).all() and set(q) == set(X.OUT_KEYS) and q["actual"].shape == (2, 0)
        flat, out = guarded(shapes_of(c))
        engine.svi_explain(p[:, :0].contiguous(), t[:, :0].contiguous(), s, c["rate"], u, tq, qty, strike_mode=1, want=("actual", "resid_sm"),
                           out={k: v for k, v in out.items() if k in ("actual", "resid_sm", "flags", "net", "n_dead")}, stream=stream)
        torch.cuda.synchronize()
        got = check_written(flat, out, ("actual", "resid_sm", "flags", "net", "n_dead"))
        assert np.isnan(got["net"]).all() and np.isnan(got["actual"]).all() and np.isnan(got["resid_sm"]).all() and (got["n_dead"] == Q).all()
        assert (got["flags"] == XC.F(XC.DEAD, XC.DEAD, XC.DEAD)).all() and (host(flat["theta_pnl"]) == SENT_F).all()
        for lag in (3, 7):                                                   # B <= lag: no pair
            q = engine.svi_explain(p, t, s, c["rate"], u, tq, qty, lag=lag, strike_mode=1, stream=stream)
            torch.cuda.synchronize()
            assert q["net"].shape == (0, 12) and q["n_dead"].shape == (0,) and q["flags"].shape == (0, Q) and q["actual"].shape == (0, Q)


def test_explicit_stream_then_immediate_reallocation():
    import torch
    from iv_interpolation_amd import engine
    c = XC.batch(**XC.STREAM_SHAPE)
    r = ref_of(c, margins=True)
    base = run(c)
    compare("stream", base, r)
    same_bits(base, run(c, stream=torch.cuda.Stream()), X.OUT_KEYS, "stream")
    s = torch.cuda.Stream()
    with torch.cuda.stream(torch.cuda.Stream()):
        q = engine.svi_explain(dev(c["params"]), dev(c["Tq"]), dev(c["spot"]), c["rate"], dev(c["u"]), dev(c["tau"]), dev(c["qty"]), lag=c["lag"],
                               is_put=dev(c["is_put"], np.uint8), strike_mode=1, stream=s)
        junk = [torch.full(x.shape, 3.0, dtype=torch.float64, device="cuda") for x in (c["params"], c["Tq"], c["spot"], c["u"], c["tau"], c["qty"]) for _ in range(3)]
        s.synchronize()
        torch.cuda.synchronize()
    same_bits(base, {k: host(v) for k, v in q.items()}, X.OUT_KEYS, "reallocation")
    del junk


def test_abi_error_table():
    import torch
    from iv_interpolation_amd import _lib, engine
    c, _ = case(3)
    p, t, s, u, tq, qty = (dev(c[k]) for k in ("params", "Tq", "spot", "u", "tau", "qty"))
    side = dev(np.zeros(u.shape[1]), np.uint8)
    for bad in (lambda: engine.svi_explain(p[0], t, s, 0.0, u, tq, qty), lambda: engine.svi_explain(p, t, s, 0.0, u, tq[:, :-1], qty),
                lambda: engine.svi_explain(p, t, s, 0.0, u, tq, qty, strike_mode=2), lambda: engine.svi_explain(p, t, s, 0.0, u, tq, qty, want=("vanna",)),
                lambda: engine.svi_explain(p, t, s, 0.0, u, tq, qty[:-1]), lambda: engine.svi_explain(p, t, s, 0.0, u, tq, qty, is_put=side[:-1]),
                lambda: engine.svi_explain(p, t, s, 0.0, u, tq, qty, lag=0), lambda: engine.svi_explain(p, t, s, 0.0, u, tq, qty, lag=1.5),
                lambda: engine.svi_explain(p, t, s, 0.0, u, tq, qty, out={"net": torch.empty((2, 8), dtype=torch.float64, device="cuda")}),
                lambda: engine.svi_explain(p, t, s, 0.0, u, tq, qty, out={"n_dead": torch.empty(2, dtype=torch.int64, device="cuda")})):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        engine.svi_explain(p, t, s, 0.0, u.float(), tq, qty)
    with pytest.raises(TypeError):
        engine.svi_explain(p, t, s, 0.0, u, tq, qty, is_put=side.double())
    lib = _lib.load()
    Q = u.shape[1]
    net = torch.full((2, 12), SENT_F, dtype=torch.float64, device="cuda")
    nd = torch.full((2,), SENT_I, dtype=torch.int32, device="cuda")
    fl = torch.full((2, Q), SENT_I, dtype=torch.int32, device="cuda")
    act = torch.full((2, Q), SENT_F, dtype=torch.float64, device="cuda")
    a = _lib.ExplainArgs()
    a.params, a.Tq, a.tq_stride, a.spot, a.u, a.tau, a.q_stride, a.qty = p.data_ptr(), t.data_ptr(), 16, s.data_ptr(), u.data_ptr(), tq.data_ptr(), Q, qty.data_ptr()
    a.mT, a.Q, a.B, a.strike_mode, a.lag = 16, Q, 3, 1, 1
    a.net, a.n_dead, a.flags, a.actual = net.data_ptr(), nd.data_ptr(), fl.data_ptr(), act.data_ptr()
    call = lambda: lib.ivs_svi_explain_f64(ctypes.byref(a), None, 0, None)   # noqa: E731
    a.lag = 0
    assert call() == -34 and b"lag=0" in lib.ivs_last_error() and lib.ivs_last_kernel() == b""
    a.lag, a.q_stride = 1, 7
    assert call() == -22 and b"stride" in lib.ivs_last_error()
    a.q_stride, a.strike_mode = Q, 2
    assert call() == -22 and b"strike_mode" in lib.ivs_last_error()
    a.strike_mode, a.mT = 1, 65
    assert call() == -34 and b"mT=65" in lib.ivs_last_error()
    a.mT, a.Q = 16, -1
    assert call() == -22 and b"negative" in lib.ivs_last_error()
    a.Q = Q
    for k in ("net", "n_dead", "flags"):
        keep = getattr(a, k)
        setattr(a, k, None)
        assert call() == -22 and b"null pointer" in lib.ivs_last_error() and lib.ivs_last_kernel() == b"", k
        setattr(a, k, keep)
    assert lib.ivs_svi_explain_f64(None, None, 0, None) == -22
    a.lag = 3                                                                # B <= lag: a no-op
    assert call() == 0 and lib.ivs_last_kernel() == b""
    torch.cuda.synchronize()
    for buf, sent in ((net, SENT_F), (nd, SENT_I), (fl, SENT_I), (act, SENT_F)):                       # a refused call launches nothing
        assert (host(buf) == sent).all()
    a.lag = 1                                                                # and the same struct, accepted, writes everything
    assert call() == 0 and lib.ivs_last_kernel() == b"svi_explain_kernel"
    torch.cuda.synchronize()
    assert not (host(net) == SENT_F).any() and not (host(nd) == SENT_I).any() and not (host(fl) == SENT_I).any() and not (host(act) == SENT_F).any()


def test_builder_and_frames_on_a_wide_chain():
    """End to end: the chain of the SVI GPU test through build(), svi() and explain() on the device.  The restatement is fed the
    kernel's own `params` copied back, so the late-round ties of the fit play no part."""
    import risk_cases as RC
    import svi_cases as SC
    import snapshot_cases as SNC
    from iv_interpolation_amd.snapshots import HipBackend, SnapshotSurfaceBuilder, explain_frame, explain_options_frame
    ten = SC.CHAIN_TENORS
    b = SnapshotSurfaceBuilder(moneyness=SC.CHAIN_MONEYNESS, tenors=ten, backend=HipBackend())
    res = b.build(SNC.big_chain(**SC.CHAIN))
    fits = b.svi(res, rate=SC.CHAIN_RATE)
    bk = RC.chain_book(res)
    reps = b.explain(res, bk, fits, rate=SC.CHAIN_RATE)
    assert [d.underlying for d in reps] == ["btc", "eth"]
    for rp, v, r in zip(reps, fits, res):
        c = dict(params=host(v.params), Tq=ten, spot=host(r.spot), rate=SC.CHAIN_RATE, u=np.ascontiguousarray(np.broadcast_to(rp.strikes, rp.tau.shape)),
                 tau=rp.tau, strike_mode=1, is_put=rp.is_put, qty=rp.quantity, lag=1)
        got = {k: host(rp.values[k]) for k in X.KEYS}
        got.update(flags=host(rp.flags), net=host(rp.net), n_dead=host(rp.n_dead))
        compare(f"builder[{rp.underlying}]", got, ref_of(c))
    f, o = explain_frame(reps, res), explain_options_frame(reps, res)
    quoted = [host(r.quotes) > 0 for r in res]
    pairs = sum(int((q[:-1] & q[1:]).sum()) for q in quoted)
    assert pairs > 0 and len(f) == pairs and len(o) == pairs * len(bk) and set(f["underlying"]) == {"btc", "eth"}
    btc = f[f["underlying"] == "btc"]
    assert (btc["n_dead"] == 2).all() and (btc["gross"] > 0).all()          # the expired option and the NaN quantity
    for d in ("ss", "sm"):
        total = btc["theta_pnl"] + btc["delta_" + d] + btc["gamma_" + d] + btc["vega_" + d] + btc["resid_" + d]
        assert np.allclose(total, btc["actual"], rtol=0, atol=1e-9 * btc["gross"].max())
