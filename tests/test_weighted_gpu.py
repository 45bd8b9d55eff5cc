"""GPU: spot_ewma_kernel and hsim_wtail_kernel behind ivs_hsim_weighted_f64 against the restatement of rules W0-W9 (tests/weighted_ref.py).

W3-W8 are a fixed sequence of IEEE operations under a total order, so once the restatement is fed the device's own sigma every
output must equal it TO THE BIT: integers, NaN patterns and the signs of zeros included.  sigma itself ends in a square root, for which
the HIP math documentation gives 1 ulp; the division before it is correctly rounded, so sigma is held to the restatement within 1 ulp
(and to its NaN pattern exactly).  With IVS_WEIGHTED_ERRLOG set, the count of sigmas that differ at all is appended to that file."""
import ctypes
import os

import numpy as np
import pytest

import hsim_cases as HC
import weighted_cases as WC
import weighted_ref as WR

pytestmark = pytest.mark.gpu
SENT_F, SENT_I = -7.25e9, -77        # no output of the rules: counts and flags >= -1; no value of a case hits -7.25e9
GUARD = 67                           # elements of guard tail behind every output
KEYS, TAIL = WR.OUT_KEYS, WR.TAIL_KEYS
ARGS = ("pnl", "scen_flags", "spot", "lag", "tail_probs", "min_scen", "weight", "vol_span", "vol_weight", "min_returns", "scale_cap")
_cache = {}


def host(t):
    return None if t is None else t.cpu().numpy()


def dev(a, dtype=np.float64):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, dtype, order="C")).cuda()


def shapes_of(B, window, nL):
    import torch
    f, i = torch.float64, torch.int32
    return dict(var_w=((B, nL), f), es_w=((B, nL), f), n_valid_w=((B,), i), worst_w=((B,), i), wsum=((B,), f), n_eff=((B,), f),
                pnl_w=((B, window), f), scale=((B, window), f), flags_w=((B, window), i), sigma=((B,), f))


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


def run(c, pnl=None, scen_flags=None, abi=False, stages=0, sigma=None, want=("pnl_w", "scale"), stream=None, **over):
    """The call through engine.hsim_weighted, or (abi) through the C entry point itself, into sentinel-filled outputs with guard tails.
    sigma: the input of stages 2 (a host array).  Returns host arrays; an output the call does not make is None."""
    import torch
    from iv_interpolation_amd import _lib, engine
    c = {**c, **over}
    pnl = dev(c["pnl"] if pnl is None else pnl) if not torch.is_tensor(pnl) else pnl
    scen_flags = dev(c["scen_flags"] if scen_flags is None else scen_flags, np.int32) if not torch.is_tensor(scen_flags) else scen_flags
    B, window = pnl.shape
    tp, M = list(c["tail_probs"]), c["vol_span"]
    flat, out = guarded(shapes_of(B, window, len(tp)))
    if stages == 2 and M > 0:
        out["sigma"].copy_(dev(sigma))
    made = {k: (k == "sigma" and M > 0) if stages == 1 else (k != "sigma" or M > 0) and (k not in ("pnl_w", "scale") or k in want) for k in KEYS}
    spot, weight, vol_weight = (dev(c[k]) if c[k] is not None and (k == "weight" or M > 0) else None for k in ("spot", "weight", "vol_weight"))
    kernel = "spot_ewma_kernel" if stages == 1 else "hsim_wtail_kernel"
    if M == 0 and stages == 1:
        kernel = ""
    if abi:
        lib = _lib.load()
        a = _lib.WeightedArgs()
        a.pnl, a.scen_flags, a.B, a.window, a.lag = pnl.data_ptr(), scen_flags.data_ptr(), B, window, c["lag"]
        a.tail_probs = ctypes.cast((ctypes.c_double * max(len(tp), 1))(*tp), ctypes.POINTER(ctypes.c_double))
        a.nL, a.min_scen, a.vol_span, a.min_returns, a.scale_cap, a.stages = len(tp), c["min_scen"], M, c["min_returns"], c["scale_cap"], stages
        a.weight, a.spot, a.vol_weight = (None if t is None else t.data_ptr() for t in (weight, spot, vol_weight))
        for k in KEYS:
            setattr(a, k, out[k].data_ptr() if made[k] else None)
        rc = lib.ivs_hsim_weighted_f64(ctypes.byref(a), None, 0, None)
        assert rc == 0, lib.ivs_last_error()
        assert lib.ivs_last_kernel() == kernel.encode()
    else:
        q = engine.hsim_weighted(pnl, scen_flags, spot, lag=c["lag"], tail_probs=tp, min_scen=c["min_scen"], weight=weight, vol_span=M, vol_weight=vol_weight,
                                 min_returns=c["min_returns"], scale_cap=c["scale_cap"], stages=stages, want=want,
                                 out={k: out[k] for k in KEYS if made[k]}, stream=stream)
        assert engine.last_kernel() == kernel and set(q) == set(engine.WEIGHTED_OUTPUTS)
        assert all((q[k] is out[k]) if made[k] else q[k] is None for k in KEYS)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    got = {}
    for k in KEYS:
        v, tail = host(out[k]), host(flat[k])[out[k].numel():]
        assert (tail == sentinel(flat[k])).all(), f"{k}: the guard tail was touched"
        if not made[k]:
            assert (v == sentinel(flat[k])).all(), f"{k}: left out, yet written"
            got[k] = None
        else:
            assert not (v == sentinel(flat[k])).any(), f"{k}: an element was not written"
            got[k] = v
    return got


def ref_of(c, **over):
    c = {**c, **over}
    return WR.weighted(*[c[k] for k in ARGS], **{k: c[k] for k in ("stages", "sigma") if k in c})


def case(name):
    if name not in _cache:
        c = WC.TABLES[name] if name in WC.TABLES else WC.make(name)
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


def sigma_within_one_ulp(got, ref, what):
    """The device's sigma against the restatement's: the same NaN pattern, and within 1 ulp where it is a number.  Logs the count of
    values that differ at all."""
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, "NaN pattern")
    ok = ~np.isnan(ref)
    differ = int((got[ok] != ref[ok]).sum())
    path = os.environ.get("IVS_WEIGHTED_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(f"{what}: {differ} of {int(ok.sum())} sigmas differ from the restatement\n")
    assert (np.abs(got[ok] - ref[ok]) <= np.spacing(ref[ok])).all(), (what, differ)


def check(c, r, name, abi):
    """Stage 0 (sigma read back, the restatement fed with it), stage 1 and stage 2 of one case."""
    got = run(c, abi=abi)
    if c["vol_span"] > 0:
        sigma_within_one_ulp(got["sigma"], r["sigma"], f"{name} ({'C ABI' if abi else 'wrapper'})")
        fed = ref_of(c, stages=2, sigma=got["sigma"])
        same_bits(got, fed, KEYS, (name, abi, "stage 0 on the device's sigma"))
        first = run(c, abi=abi, stages=1)
        same_bits(first, got, ("sigma",), (name, abi, "stage 1"))
        same_bits(run(c, abi=abi, stages=2, sigma=got["sigma"]), got, KEYS, (name, abi, "stage 2"))
        same_bits(run(c, abi=abi, stages=2, sigma=r["sigma"]), r, KEYS, (name, abi, "stage 2 on the restatement's sigma"))
    else:
        assert got["sigma"] is None
        same_bits(got, r, TAIL, (name, abi))
    assert got["n_valid_w"].dtype == got["worst_w"].dtype == got["flags_w"].dtype == np.int32
    return got


# ------------------------------------------------------------------ the restatement's bits
@pytest.mark.parametrize("name", sorted(WC.CASES))
def test_generated_bits(name):
    c, r = case(name)
    for abi in (False, True):
        check(c, r, name, abi)


@pytest.mark.parametrize("name", sorted(WC.TABLES))
def test_tables_by_hand(name):
    t, r = case(name)
    for abi in (False, True):
        WC.check_want(name, t, check(t, r, name, abi))          # the hand-made values themselves


def _hsim_stage2(pnl, scen_flags, tail_probs, min_scen):
    """The device's own H7 on rows given: svi_hsim(stages=2) with a book that is not read."""
    import torch
    from iv_interpolation_amd import engine
    B, window = pnl.shape
    one = torch.ones(1, dtype=torch.float64, device="cuda")
    q = engine.svi_hsim(torch.zeros(B, 1, 5, dtype=torch.float64, device="cuda"), one, torch.ones(B, dtype=torch.float64, device="cuda"), 0.0, one, one, one,
                        lag=1, window=window, tail_probs=tail_probs, min_scen=min_scen, stages=2, out=dict(pnl=pnl, scen_flags=scen_flags))
    torch.cuda.synchronize()
    return {k: host(q[k]) for k in ("var", "es", "n_valid", "worst")}


@pytest.mark.parametrize("name", ["w63", "w256", "w1024", "w1024_zero", "tie_257", "tie_1024", "too_few", "nothing"])
def test_n_valid_is_the_tail_kernels(name):
    c, r = case(name)
    pnl, fl = dev(c["pnl"]), dev(c["scen_flags"], np.int32)
    got = run(c, pnl, fl, weight=None, vol_span=0)
    h = _hsim_stage2(pnl, fl, c["tail_probs"], c["min_scen"])
    same_bits(got, dict(n_valid_w=h["n_valid"], worst_w=h["worst"]), ("n_valid_w", "worst_w"), name)


def test_unit_weights_with_an_integer_tail_are_the_tail_kernels_bits():
    r = np.random.default_rng(24)
    pnl, fl = dev(r.standard_t(4, (5, 200))), dev(np.zeros((5, 200)), np.int32)
    tps = (0.5, 0.25, 0.05, 0.01)
    c = dict(WC.table(np.zeros((5, 200)), tail_probs=tps))
    got = run(c, pnl, fl)
    h = _hsim_stage2(pnl, fl, tps, 1)
    same_bits(got, dict(var_w=h["var"], es_w=h["es"], n_valid_w=h["n_valid"], worst_w=h["worst"]), ("var_w", "es_w", "n_valid_w", "worst_w"), "H7")


def test_chain_on_the_device_rows():
    """hsim_cases' B = 70, window 65 shape through svi_hsim on the device, then the weighted tail on the rows the device wrote, with the
    chain's own spot: the restatement on those rows and the device's sigma, to the bit; the rows feed the bootstrap unchanged."""
    import torch
    from iv_interpolation_amd import engine
    h = HC.make(4)
    q = engine.svi_hsim(dev(h["params"]), dev(h["Tq"]), dev(h["spot"]), h["rate"], dev(h["u"]), dev(h["tau"]), dev(h["qty"]), lag=h["lag"],
                        window=h["window"], tail_probs=h["tail_probs"], min_scen=h["min_scen"], is_put=dev(h["is_put"], np.uint8),
                        strike_mode=h["strike_mode"])
    torch.cuda.synchronize()
    c = dict(pnl=host(q["pnl"]), scen_flags=host(q["scen_flags"]), spot=np.asarray(h["spot"], np.float64), lag=h["lag"], tail_probs=tuple(h["tail_probs"]),
             min_scen=h["min_scen"], weight=WC.age_weights(h["window"], 0.97), vol_span=16, vol_weight=WC.age_weights(16, 0.94), min_returns=4, scale_cap=3.0)
    got = run(c, q["pnl"], q["scen_flags"])
    sigma_within_one_ulp(got["sigma"], WR.ewma_sigma(c["spot"], c["vol_weight"], 4), "chain")
    r = ref_of(c, stages=2, sigma=got["sigma"])
    assert r["active"].sum() >= 30 and not r["active"].all()
    same_bits(got, r, KEYS, "the restatement on the device's rows")
    same_bits(got, run(c, q["pnl"], q["scen_flags"]), KEYS, "two runs")
    plain = run(c, q["pnl"], q["scen_flags"], weight=None, vol_span=0)
    same_bits(plain, dict(n_valid_w=host(q["n_valid"]), worst_w=host(q["worst"])), ("n_valid_w", "worst_w"), "section 19's own")
    boot = engine.hsim_bootstrap(dev(got["pnl_w"]), dev(got["flags_w"], np.int32), h["tail_probs"], h["min_scen"], n_rep=16)      # a row in section 19's sense
    torch.cuda.synchronize()
    assert np.array_equal(host(boot["n_scen"]), got["n_valid_w"])


# ------------------------------------------------------------------ W9
def test_a_row_does_not_depend_on_the_launch():
    c, r = case("w256")                                      # M = 0: the row alone
    full = run(c)
    for p in (0, 37, 69):
        one = run(c, c["pnl"][p:p + 1], c["scen_flags"][p:p + 1])
        same_bits({k: v[0] for k, v in one.items() if v is not None}, {k: v[p] for k, v in full.items() if v is not None}, TAIL, ("alone", p))
    lone = run(c, tail_probs=c["tail_probs"][1:])
    same_bits(lone, dict(var_w=full["var_w"][:, 1:], es_w=full["es_w"][:, 1:]), ("var_w", "es_w"), "one level of two")
    same_bits(lone, full, ("n_valid_w", "worst_w", "wsum", "n_eff", "pnl_w", "scale", "flags_w"), "one level of two")
    same_bits(run(c), full, TAIL, "two runs")
    c, r = case("w64")                                       # M = 64: a row with the sigmas it reads, the others' rows zeroed
    full = run(c)
    for p in (30, 69):
        pnl = np.zeros_like(c["pnl"])
        pnl[p] = c["pnl"][p]
        one = run(c, pnl, c["scen_flags"], stages=2, sigma=full["sigma"])
        same_bits({k: one[k][p] for k in TAIL}, {k: full[k][p] for k in TAIL}, TAIL, ("the other rows zeroed", p))
    same_bits(run(c), full, KEYS, "two runs, scaled")


# ------------------------------------------------------------------ housekeeping
def test_null_outputs_and_no_level():
    c, r = case("w63")
    full = run(c)
    for want in ((), ("pnl_w",), ("scale",)):
        for abi in (False, True):
            got = run(c, abi=abi, want=want)
            assert all((got[k] is None) == (k not in want) for k in ("pnl_w", "scale"))
            same_bits(got, full, KEYS, ("NULL outputs", want, abi))
    for abi in (False, True):
        got = run(c, abi=abi, tail_probs=())
        assert got["var_w"].shape == (70, 0) and got["es_w"].size == 0
        same_bits(got, full, ("n_valid_w", "worst_w", "wsum", "n_eff", "pnl_w", "scale", "flags_w", "sigma"), ("nL = 0", abi))


def test_explicit_stream_then_immediate_reallocation():
    import torch
    from iv_interpolation_amd import engine
    c, r = case("w64")
    reps = 40
    pnl, fl = dev(np.tile(c["pnl"], (reps, 1))), dev(np.tile(c["scen_flags"], (reps, 1)), np.int32)
    w = dev(c["weight"])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    out = engine.hsim_weighted(pnl, fl, lag=c["lag"], tail_probs=c["tail_probs"], min_scen=c["min_scen"], weight=w, stream=s)
    junk = [torch.full((reps * 70, 64), 3.0, dtype=torch.float64, device="cuda") for _ in range(4)]      # takes an output if it was freed too early
    s.synchronize()
    torch.cuda.synchronize()
    ref = ref_of(c, vol_span=0)
    for k in TAIL:
        same_bits({k: host(out[k])}, {k: np.tile(ref[k], (reps,) + (1,) * (ref[k].ndim - 1))}, (k,), "explicit stream")
    assert out["sigma"] is None
    del junk


def test_refused_calls_leave_the_device_buffers_alone():
    import torch
    from iv_interpolation_amd import _lib, engine
    c, r = case("w64")
    B, window = c["pnl"].shape
    flat, out = guarded(shapes_of(B, window, len(c["tail_probs"])))
    pnl, fl, spot, w, vw = dev(c["pnl"]), dev(c["scen_flags"], np.int32), dev(c["spot"]), dev(c["weight"]), dev(c["vol_weight"])
    lib = _lib.load()
    keep = []

    def dbl(xs):
        keep.append((ctypes.c_double * max(len(xs), 1))(*xs))
        return ctypes.cast(keep[-1], ctypes.POINTER(ctypes.c_double))
    for over, want in ((dict(window=1025), -34), (dict(window=0), -34), (dict(lag=0), -34), (dict(nL=9), -34), (dict(min_scen=0), -34), (dict(vol_span=1025), -34),
                       (dict(vol_span=-1), -34), (dict(min_returns=0), -34), (dict(min_returns=65), -34), (dict(scale_cap=0.999), -34),
                       (dict(scale_cap=float("inf")), -34), (dict(stages=3), -34), (dict(tail_probs=dbl([0.0] * 8)), -34), (dict(B=2 ** 31 // 64 + 1), -34),
                       (dict(nL=-1), -22), (dict(B=-1), -22), (dict(pnl=0), -22), (dict(scen_flags=0), -22), (dict(flags_w=0), -22), (dict(wsum=0), -22),
                       (dict(n_eff=0), -22), (dict(n_valid_w=0), -22), (dict(worst_w=0), -22), (dict(var_w=0), -22), (dict(es_w=0), -22), (dict(sigma=0), -22),
                       (dict(spot=0), -22), (dict(vol_weight=0), -22), (dict(tail_probs=None), -22), (dict(stages=2, sigma=0), -22)):
        a = _lib.WeightedArgs()
        a.pnl, a.scen_flags, a.B, a.window, a.lag = pnl.data_ptr(), fl.data_ptr(), B, window, c["lag"]
        a.tail_probs, a.nL, a.min_scen = dbl(c["tail_probs"]), len(c["tail_probs"]), c["min_scen"]
        a.weight, a.spot, a.vol_weight = w.data_ptr(), spot.data_ptr(), vw.data_ptr()
        a.vol_span, a.min_returns, a.scale_cap, a.stages = c["vol_span"], c["min_returns"], c["scale_cap"], 0
        for k in KEYS:
            setattr(a, k, out[k].data_ptr())
        for k, v in over.items():
            setattr(a, k, v)
        rc = lib.ivs_hsim_weighted_f64(ctypes.byref(a), None, 0, None)
        assert rc == want, (over, lib.ivs_last_error())
        assert lib.ivs_last_kernel() == b""
    with pytest.raises(ValueError, match="one shape"):
        engine.hsim_weighted(pnl, fl[:2], out=out)
    with pytest.raises(ValueError, match="vol_span"):
        engine.hsim_weighted(pnl, fl, vol_span=1025, out=out)
    with pytest.raises(ValueError, match="needs spot"):
        engine.hsim_weighted(pnl, fl, vol_span=8, min_returns=2, out=out)
    with pytest.raises(ValueError, match="must be given"):
        engine.hsim_weighted(pnl, fl, vol_span=8, min_returns=2, stages=2)
    with pytest.raises(ValueError, match=r"\[window\]"):
        engine.hsim_weighted(pnl, fl, weight=w[:5], out=out)
    with pytest.raises(ValueError, match="want"):
        engine.hsim_weighted(pnl, fl, want=("sigma",), out=out)
    with pytest.raises(TypeError):
        engine.hsim_weighted(pnl, fl.to(torch.int64), out=out)
    torch.cuda.synchronize()
    for k, v in flat.items():
        assert (host(v) == sentinel(v)).all(), k
    empty = engine.hsim_weighted(pnl[:0], fl[:0])                                                    # B = 0: a no-op
    assert empty["var_w"].shape == (0, 2) and empty["flags_w"].shape == (0, 64) and engine.last_kernel() == ""


def test_builder_var_weighted_on_a_wide_chain():
    """End to end: build(), svi(), var() and var_weighted() on the device with the defaults, and with the scaling on: every figure is
    the restatement on the report's own rows and sigma, and the frame carries them."""
    import risk_cases as RC
    import svi_cases as SC
    import snapshot_cases as SNC
    from iv_interpolation_amd.snapshots import HipBackend, SnapshotSurfaceBuilder, weighted_var_frame
    b = SnapshotSurfaceBuilder(moneyness=SC.CHAIN_MONEYNESS, tenors=SC.CHAIN_TENORS, backend=HipBackend())
    res = b.build(SNC.big_chain(**SC.CHAIN))
    fits = b.svi(res, rate=SC.CHAIN_RATE)
    bk = RC.chain_book(res)
    var = b.var(res, bk, fits, rate=SC.CHAIN_RATE)
    for kw in (dict(), dict(vol_span=64, min_returns=4)):
        reps = b.var_weighted(res, var, **kw)
        assert [d.underlying for d in reps] == ["btc", "eth"]
        for rp, v, rs in zip(reps, var, res):
            M = kw.get("vol_span", 0)
            assert (rp.decay, rp.vol_span, rp.vol_decay, rp.min_returns, rp.scale_cap) == (0.99, M, 0.94, kw.get("min_returns", 20), 3.0)
            spot = host(rs.spot)
            if M:
                sigma_within_one_ulp(host(rp.sigma), WR.ewma_sigma(spot, WR.age_weights(M, 0.94), rp.min_returns), "builder " + rp.underlying)
            else:
                assert rp.sigma is None
            ref = WR.weighted(host(v.pnl), host(v.scen_flags), spot, v.lag, (0.05, 0.01), 20, WR.age_weights(v.window, 0.99), M,
                              None, rp.min_returns, 3.0, stages=2, sigma=None if rp.sigma is None else host(rp.sigma))
            same_bits({k: host(getattr(rp, k)) for k in TAIL}, ref, TAIL, "the report")
            assert ref["active"].any()
        f = weighted_var_frame(reps, res)
        assert len(f) > 0 and set(f["underlying"]) == {"btc", "eth"} and "esw_0.01" in f.columns
        assert np.isfinite(f["varw_0.05"]).any() and (f["n_eff"][np.isfinite(f["varw_0.05"])] > 1).all()
