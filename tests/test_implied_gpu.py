"""GPU: bs_price_kernel (ivs_bs_price_f64) and bs_implied_vol_kernel (ivs_bs_implied_vol_f64) against
tests/golden/implied_vol.npz, the exact vectors of rules V1-V8 from mpmath.

Flags and NaN patterns equal the fixture's everywhere (its generator keeps every point 2^-30 off the thresholds of V4).  A vol
agrees with the exact vol of its float64 price within C_GPU x R_CPU[regime] units U of the point, a price with the exact price
within C_GPU x R_CPU_PRICE[regime] of its own unit; U is stored in the file, R_CPU is the restatement's distance measured by
test_implied.test_restatement_against_the_fixture (iv_cases.py).

Every test prints its largest error / tolerance ratios; with IVS_IV_ERRLOG=<file> set the figures are appended to that file
as well (a recorded run belongs in profiles/implied/errlog_gpu.txt; errlog.txt there holds the CPU run)."""
import ctypes
import os

import numpy as np
import pytest

import iv_cases as IC
import iv_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT_F, SENT_I = -7.25e9, -77        # no output of the rules: flags >= 0; no vol, price or vega is negative
GUARD = 67                           # elements of guard tail behind every output
TINY = float(np.finfo(np.float64).tiny)
REGS = list(IC.REGIMES)
IN_KEYS = ("S", "K", "T", "r")


def log(name, **figures):
    line = name + ": " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items())
    print(line)
    path = os.environ.get("IVS_IV_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def host(t):
    return None if t is None else t.cpu().numpy()


def dev(a, dtype=np.float64):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()       # a copy: the shared inputs are read-only


def guarded(n, spec):
    """One flat sentinel-filled buffer per output, GUARD elements longer than the output; the output is its head."""
    import torch
    flat = {k: torch.full((n + GUARD,), SENT_I if dt == torch.int32 else SENT_F, dtype=dt, device="cuda") for k, dt in spec.items()}
    return flat, {k: v[:n] for k, v in flat.items()}


def check_written(flat, out, keys):
    got = {}
    for k in keys:
        v, tail = host(out[k]), host(flat[k])[out[k].numel():]
        sent = SENT_I if v.dtype == np.int32 else SENT_F
        assert not (v == sent).any(), f"{k}: an element was not written"
        assert (tail == sent).all(), f"{k}: the guard tail was touched"
        got[k] = v
    return got


def run_iv(c, mode=0, stream=None, default=None):
    """One solver call with both outputs pre-filled with a sentinel and followed by a guard tail.  default: None passes
    c["is_put"] as an array, True / False passes no array and default_is_put."""
    import torch
    from iv_interpolation_amd import engine
    n = len(c["S"])
    flat, out = guarded(n, {"vol": torch.float64, "flags": torch.int32})
    put = dev(c["is_put"], np.uint8) if default is None else None
    q = engine.bs_implied_vol(dev(c["price"]), *[dev(c[k]) for k in IN_KEYS], is_put=put, default_is_put=bool(default),
                              price_mode=mode, out=out, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    assert engine.last_kernel() == "bs_implied_vol_kernel" and set(q) == {"vol", "flags"}
    return check_written(flat, out, ("vol", "flags"))


def run_price(c, stream=None, default=None, vega=True, flags=True):
    import torch
    from iv_interpolation_amd import engine
    n = len(c["S"])
    flat, out = guarded(n, {"price": torch.float64, "vega": torch.float64, "flags": torch.int32})
    put = dev(c["is_put"], np.uint8) if default is None else None
    keys = ("price",) + (("vega",) if vega else ()) + (("flags",) if flags else ())
    q = engine.bs_price(*[dev(c[k]) for k in IN_KEYS], dev(c["sigma"]), is_put=put, default_is_put=bool(default), want_vega=vega,
                        want_flags=flags, out={k: out[k] for k in keys}, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    assert engine.last_kernel() == "bs_price_kernel" and set(q) == {"price", "vega", "flags"}
    for k in ("vega", "flags"):
        if k not in keys:                                                    # left out: None, and its buffer untouched
            assert q[k] is None and (host(flat[k]) == (SENT_I if k == "flags" else SENT_F)).all(), k
    got = check_written(flat, out, keys)
    got.update({k: None for k in ("vega", "flags") if k not in keys})
    return got


def same_bits(a, b, keys, what):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), (k, what)


_cache = {}


def fixture():
    """The file, its regimes joined, and the kernels' results on all 448 points in one call; computed once, read-only."""
    if not _cache:
        fix = IC.load_fixture(os.path.join(ROOT, "tests", "golden", "implied_vol.npz"))
        j = IC.joined(fix)
        for a in list(j.values()) + [a for p in fix.values() for a in p.values()]:
            a.setflags(write=False)
        _cache.update(fix=fix, j=j, iv=run_iv(j), price=run_price(j))
    return _cache["fix"], _cache["j"], _cache["iv"], _cache["price"]


def compare_iv(name, got, p):
    """got against the exact vols of the points p, regime by regime (p carries `regime`, or is one regime named `name`)."""
    assert got["flags"].dtype == np.int32 and got["vol"].dtype == np.float64
    assert np.array_equal(got["flags"], p["flags"].astype(np.int32)), (name, got["flags"])
    assert np.isfinite(got["vol"]).all(), name                                # the fixture's NaN pattern: none
    ratio = np.abs(got["vol"] - p["vol_exact"]) / p["unit_vol"]
    reg = p["regime"] if "regime" in p else np.full(len(ratio), REGS.index(name))
    fig = {REGS[i]: float(ratio[reg == i].max()) / (IC.C_GPU * IC.R_CPU[REGS[i]]) for i in np.unique(reg)}
    log(f"implied[{name}]", **fig, options=len(ratio))
    assert all(v <= 1.0 for v in fig.values()), (name, fig)


def test_fixture_in_one_call_then_each_regime_alone():
    fix, j, iv, _ = fixture()
    assert len(j["S"]) == 448
    compare_iv("all", iv, j)
    for i, reg in enumerate(REGS):
        alone = run_iv(fix[reg])
        compare_iv(reg, alone, fix[reg])
        same_bits({k: v[j["regime"] == i] for k, v in iv.items()}, alone, ("vol", "flags"), reg)


def vega_unit(p):
    """eps x vega x (2 + |d1| x the error of d1 in its own units): phi(d1) is known to |d1| times d1's error, d1 = x / s + s / 2
    carries x's rounding (a logarithm and a product) over s and its own two roundings; one more for the products."""
    s = p["sigma"] * np.sqrt(p["T"])
    x = np.log(p["S"] / p["K"]) + p["r"] * p["T"]
    d1 = x / s + 0.5 * s
    vega = p["S"] * np.exp(-0.5 * d1 * d1) / np.sqrt(2 * np.pi) * np.sqrt(p["T"])
    dd1 = (np.abs(np.log(p["S"] / p["K"])) + np.abs(p["r"] * p["T"])) / s + np.abs(x) / s + 0.5 * s + np.abs(d1)
    return vega, IC.EPS * vega * (2.0 + np.abs(d1) * dd1) + TINY


def test_pricer_against_the_exact_prices():
    fix, j, _, pr = fixture()
    assert (pr["flags"] == 0).all() and np.isfinite(pr["price"]).all() and np.isfinite(pr["vega"]).all()
    ratio = np.abs(pr["price"] - j["price"]) / j["unit_price"]
    fig = {reg: float(ratio[j["regime"] == i].max()) / (IC.C_GPU * IC.R_CPU_PRICE[reg]) for i, reg in enumerate(REGS)}
    vega, unit = vega_unit(j)
    fig["vega"] = float((np.abs(pr["vega"] - vega) / unit).max()) / IC.C_GPU
    log("price[all]", **fig, options=len(ratio))
    assert all(v <= 1.0 for v in fig.values()), fig
    # vega and flags left out: their buffers stay untouched (run_price) and the price bits do not change
    for vg, fl in ((False, True), (True, False), (False, False)):
        part = run_price(j, vega=vg, flags=fl)
        same_bits(pr, part, [k for k in ("price", "vega", "flags") if part[k] is not None], (vg, fl))
    # through the raw ABI with both NULL
    import torch
    from iv_interpolation_amd import _lib
    lib = _lib.load()
    ins = [dev(j[k]) for k in IN_KEYS + ("sigma",)]
    put = dev(j["is_put"], np.uint8)
    flat, out = guarded(len(j["S"]), {"price": torch.float64})
    assert lib.ivs_bs_price_f64(*[t.data_ptr() for t in ins], put.data_ptr(), 0, len(j["S"]), out["price"].data_ptr(), None, None, None) == 0
    torch.cuda.synchronize()
    assert lib.ivs_last_kernel() == b"bs_price_kernel"
    same_bits(pr, check_written(flat, out, ("price",)), ("price",), "raw")


def test_pricer_dead_inputs():
    live = dict(S=100.0, K=110.0, T=0.5, r=0.01, sigma=0.4)
    rows = []
    for k in live:
        for bad in (IC.NAN, IC.INF, -IC.INF) + (() if k == "r" else (0.0, -1.0)):
            rows.append(dict(live, **{k: bad}))
    rows.append(live)
    c = {k: np.array([r_[k] for r_ in rows]) for k in live}
    for put in (0.0, 1.0):
        c["is_put"] = np.full(len(rows), put)
        got = run_price(c)
        assert (got["flags"][:-1] == IC.DEAD).all() and np.isnan(got["price"][:-1]).all() and np.isnan(got["vega"][:-1]).all()
        assert got["flags"][-1] == 0 and got["price"][-1] > 0 and got["vega"][-1] > 0


def gpu_solve(price, S, K, T, r, is_put, mode):
    return run_iv(dict(price=price, S=S, K=K, T=T, r=r, is_put=is_put), mode=mode)


def gpu_price(S, K, T, r, sigma, is_put):
    return run_price(dict(S=S, K=K, T=T, r=r, sigma=sigma, is_put=is_put))


def test_micro_cases():
    IC.check_micro(gpu_solve)


def test_known_answer_priced_then_inverted():
    IC.check_known(gpu_price, gpu_solve)


def grid_cap():
    """Blocks at which the launch stops growing and the kernels start to stride (capped_blocks: 16 per CU)."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 16


def geometry_sizes():
    return [1, 63, 64, 65, 255, 256, 257, "wrap"]


@pytest.mark.parametrize("n", geometry_sizes())
def test_launch_geometry(n):
    """The fixture's points tiled into n options: every copy of a point has the bits it has in the 448-point call, wherever
    it stands; is_put as an array and as default_is_put give the same bits."""
    fix, j, iv, pr = fixture()
    if n == "wrap":
        n = grid_cap() * 256 + 1                                             # one option past a full stride of the capped grid
        assert n < 4_000_000
    c, idx = IC.tiled(fix, n)
    got = run_iv(c)
    same_bits({k: v[idx] for k, v in iv.items()}, got, ("vol", "flags"), n)
    gp = run_price(c)
    same_bits({k: v[idx] for k, v in pr.items()}, gp, ("price", "vega", "flags"), n)
    for put in (False, True):                                                # one side only, the side passed as the default
        pick = np.flatnonzero((j["is_put"] != 0) == put)
        sub_idx = pick[np.arange(min(n, 100_003)) % len(pick)]
        sub = {k: np.ascontiguousarray(j[k][sub_idx]) for k in IC.FIELDS}
        same_bits({k: v[sub_idx] for k, v in iv.items()}, run_iv(sub, default=put), ("vol", "flags"), (n, put))
        same_bits({k: v[sub_idx] for k, v in pr.items()}, run_price(sub, default=put), ("price", "vega", "flags"), (n, put))


def test_price_modes_agree():
    """price_mode 1 on price / S against mode 0 on price.  The division and the product each round the price once more, and a
    vol moves by at most eps P / Vega <= U per rounding of its price; each result is within C_GPU x R_CPU x U of the exact vol
    of its own price."""
    _, j, iv, _ = fixture()
    c = dict(j)
    c["price"] = j["price"] / j["S"]
    got = run_iv(c, mode=1)
    assert np.array_equal(got["flags"], iv["flags"])
    rc = np.array([IC.R_CPU[REGS[i]] for i in j["regime"]])
    ratio = np.abs(got["vol"] - iv["vol"]) / ((2.0 * IC.C_GPU * rc + 2.0) * j["unit_vol"])
    log("modes", worst=float(ratio.max()), differing=int((got["vol"] != iv["vol"]).sum()))
    assert (ratio <= 1.0).all()
    ratio1 = np.abs(got["vol"] - j["vol_exact"]) / ((IC.C_GPU * rc + 2.0) * j["unit_vol"])
    assert (ratio1 <= 1.0).all()


def test_round_trip_through_the_product():
    """surface -> price() -> vol -> the same surface: the chain of the SVI surface test through build(), svi() and price(),
    then the call and the put of every live query back through the solver with the query's tau, the snapshot's spot and the
    rate.  The tolerance is the vol's unit evaluated with the restatement at the point, times C_GPU x the largest R_CPU, plus
    the price's own tolerance (cal_cases) over vega.  Where that tolerance of the price reaches the time value or the upper
    bound, the price says nothing about the vol (deep in or out of the money: eth against a book round btc's spot) and the
    point is only counted."""
    import cal_cases as CC
    import cal_ref as CR
    import snapshot_cases as SNC
    import svi_cases as SC
    from iv_interpolation_amd.snapshots import HipBackend, SnapshotSurfaceBuilder
    ten = SC.CHAIN_TENORS
    b = SnapshotSurfaceBuilder(moneyness=SC.CHAIN_MONEYNESS, tenors=ten, backend=HipBackend())
    res = b.build(SNC.big_chain(**SC.CHAIN))
    fits = b.svi(res, rate=SC.CHAIN_RATE)
    marks = b.price(res, CC.chain_book(res), fits, rate=SC.CHAIN_RATE)
    factor = {k: CC.C_GPU * v for k, v in CC.R_CPU.items()}
    r_max = max(IC.R_CPU.values())
    for mk, v, r in zip(marks, fits, res):
        fl = host(mk.flags)
        live = (fl & CC.Q_DEAD) == 0
        spot = host(r.spot)
        S = np.broadcast_to(spot[:, None], fl.shape)[live]
        K = np.broadcast_to(mk.strikes, fl.shape)[live]
        tau, vol = mk.tau[live], host(mk.vol)[live]
        rate = np.full(len(S), SC.CHAIN_RATE)
        ref = CR.restate_eval(host(v.params), ten, spot, SC.CHAIN_RATE, np.ascontiguousarray(np.broadcast_to(mk.strikes, fl.shape)), mk.tau, 1)
        tol_p = CC.tolerances_eval(ref, factor)
        KD = K * np.exp(-rate * tau)
        for side, put in (("call", 0.0), ("put", 1.0)):
            P = host(getattr(mk, side))[live]
            got = run_iv(dict(price=P, S=S, K=K, T=tau, r=rate, is_put=np.full(len(S), put)))
            with np.errstate(all="ignore"):
                unit, vega = R.unit_from_restatement(vol, P, S, K, tau, rate, put)
                tp = tol_p[side][live]
                tol = IC.C_GPU * r_max * unit + tp / vega
                intrinsic = np.maximum(KD - S, 0.0) if put else np.maximum(S - KD, 0.0)
                told = np.isfinite(tol) & (P - intrinsic > tp) & ((KD if put else S) - P > tp)
                ratio = np.abs(got["vol"] - vol) / tol
            log(f"round_trip[{mk.underlying},{side}]", worst=float(ratio[told].max()) if told.any() else 0.0, live=int(live.sum()), told=int(told.sum()))
            assert np.isfinite(got["vol"][told]).all() and (ratio[told] <= 1.0).all(), (mk.underlying, side)
            assert ((got["flags"][told] & ~IC.ITM) == 0).all()
            if mk.underlying == "btc":                                       # the book lies round btc's spot: every query counts
                assert told.all() and told.sum() >= 400


def test_explicit_stream_then_immediate_reallocation():
    """The calls run on an explicit stream while another stream is current; their inputs are temporaries that die when the
    call returns, and tensors of the same sizes are allocated and filled on the current stream at once (record_stream)."""
    import torch
    from iv_interpolation_amd import engine
    fix, j, _, _ = fixture()
    c, idx = IC.tiled(fix, 50_021)
    base_v, base_p = run_iv(c), run_price(c)
    same_bits(base_v, run_iv(c, stream=torch.cuda.Stream()), ("vol", "flags"), "stream")
    same_bits(base_p, run_price(c, stream=torch.cuda.Stream()), ("price", "vega", "flags"), "stream")
    s = torch.cuda.Stream()
    with torch.cuda.stream(torch.cuda.Stream()):
        qv = engine.bs_implied_vol(dev(c["price"]), *[dev(c[k]) for k in IN_KEYS], is_put=dev(c["is_put"], np.uint8), stream=s)
        qp = engine.bs_price(*[dev(c[k]) for k in IN_KEYS], dev(c["sigma"]), is_put=dev(c["is_put"], np.uint8), want_vega=True, stream=s)
        junk = [torch.full((len(idx),), 3.0, dtype=torch.float64, device="cuda") for _ in range(16)]
        junk += [torch.full((len(idx),), 1, dtype=torch.uint8, device="cuda") for _ in range(4)]
        s.synchronize()
        torch.cuda.synchronize()
    same_bits(base_v, {k: host(t) for k, t in qv.items()}, ("vol", "flags"), "reallocation")
    same_bits(base_p, {k: host(t) for k, t in qp.items()}, ("price", "vega", "flags"), "reallocation")
    del junk


def test_error_table():
    import torch
    from iv_interpolation_amd import _lib, engine
    _, j, iv, _ = fixture()
    n = 100
    p, S, K, T, r, sg = (dev(j[k][:n]) for k in ("price", "S", "K", "T", "r", "sigma"))
    put = dev(j["is_put"][:n], np.uint8)
    f32 = torch.float32
    for bad in (lambda: engine.bs_implied_vol(p[:-1], S, K, T, r), lambda: engine.bs_implied_vol(p, S, K, T[:5], r),
                lambda: engine.bs_implied_vol(p, S, K, T, r, is_put=put[:-1]), lambda: engine.bs_implied_vol(p, S, K, T, r, price_mode=2),
                lambda: engine.bs_implied_vol(p, S, K, T, r, price_mode=-1),
                lambda: engine.bs_implied_vol(p, S, K, T, r, out={"vol": torch.empty(n, dtype=f32, device="cuda")}),
                lambda: engine.bs_implied_vol(p, S, K, T, r, out={"flags": torch.empty(n + 1, dtype=torch.int32, device="cuda")}),
                lambda: engine.bs_price(S, K, T, r, sg[:-1]), lambda: engine.bs_price(S, K, T, r, sg, is_put=put[:3]),
                lambda: engine.bs_price(S, K, T, r, sg, out={"price": torch.empty(n, dtype=f32, device="cuda")})):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: engine.bs_implied_vol(p.float(), S, K, T, r), lambda: engine.bs_implied_vol(p, S, K, T, r.cpu()),
                lambda: engine.bs_price(S, K, T, r, sg.float()), lambda: engine.bs_price(S.to(torch.int64), K, T, r, sg)):
        with pytest.raises(TypeError):
            bad()
    lib = _lib.load()
    flat, out = guarded(n, {"vol": torch.float64, "flags": torch.int32, "price": torch.float64})
    ptr = lambda t: t.data_ptr()                                              # noqa: E731
    iv_call = lambda vol, n_, mode: lib.ivs_bs_implied_vol_f64(ptr(p), ptr(S), ptr(K), ptr(T), ptr(r), ptr(put), 0, mode, n_, vol, ptr(out["flags"]), None)  # noqa: E731
    assert iv_call(None, n, 0) == -22 and b"null pointer" in lib.ivs_last_error() and lib.ivs_last_kernel() == b""
    assert iv_call(ptr(out["vol"]), -1, 0) == -22 and b"negative size" in lib.ivs_last_error()
    assert iv_call(ptr(out["vol"]), n, 2) == -22 and b"price_mode=2" in lib.ivs_last_error()
    assert iv_call(ptr(out["vol"]), 1 << 31, 0) == -34 and b"exceed one launch" in lib.ivs_last_error()
    assert iv_call(ptr(out["vol"]), 0, 0) == 0 and lib.ivs_last_error() == b""                    # n == 0: a no-op
    pr_call = lambda price, n_: lib.ivs_bs_price_f64(ptr(S), ptr(K), ptr(T), ptr(r), ptr(sg), None, 0, n_, price, None, None, None)  # noqa: E731
    assert pr_call(None, n) == -22 and b"null pointer" in lib.ivs_last_error()
    assert pr_call(ptr(out["price"]), -1) == -22 and pr_call(ptr(out["price"]), 1 << 31) == -34 and pr_call(ptr(out["price"]), 0) == 0
    torch.cuda.synchronize()
    for k, t in flat.items():                                                 # a refused call launches nothing
        assert (host(t) == (SENT_I if t.dtype == torch.int32 else SENT_F)).all(), k
    empty = engine.bs_implied_vol(p[:0], S[:0], K[:0], T[:0], r[:0])
    assert empty["vol"].shape == (0,) and empty["flags"].shape == (0,) and engine.bs_price(S[:0], K[:0], T[:0], r[:0], sg[:0])["price"].shape == (0,)
    assert iv_call(ptr(out["vol"]), n, 1) == 0                                # and the same arguments, accepted, do launch
    torch.cuda.synchronize()
    assert lib.ivs_last_kernel() == b"bs_implied_vol_kernel" and not (host(out["flags"]) == SENT_I).any()


def test_implied_volatility_on_the_device():
    """ImpliedVolatility with scalars, arrays and CUDA tensors."""
    import torch
    from iv_interpolation_amd import ImpliedVolatility as IV
    k = IC.KNOWN
    p = IV.price(k["S"], k["K"], k["T"], k["r"], k["sigma"], "put")
    assert np.ndim(p["price"]) == 0 and abs(p["price"] - 1607.6747338019552) < 1e-9
    v = IV.implied_vol(p["price"] / k["S"], k["S"], k["K"], k["T"], k["r"], "put", price_mode="underlying")
    assert abs(v["vol"] - 0.6) < 1e-12 and v["flags"] == IC.ITM
    Ks = np.array([24000.0, 25500.0, 27000.0])
    pa = IV.price(k["S"], Ks, k["T"], k["r"], k["sigma"])
    t = [torch.full((3,), float(k[n]), dtype=torch.float64, device="cuda") for n in ("S", "T", "r")]
    pt = IV.price(t[0], dev(Ks), t[1], t[2], torch.full((3,), 0.6, dtype=torch.float64, device="cuda"))
    assert pt["price"].is_cuda and np.array_equal(host(pt["price"]), pa["price"]) and np.array_equal(host(pt["vega"]), pa["vega"])
    vt = IV.implied_vol(pt["price"], t[0], dev(Ks), t[1], t[2])
    assert vt["vol"].is_cuda and np.allclose(host(vt["vol"]), 0.6, rtol=0, atol=1e-11)
