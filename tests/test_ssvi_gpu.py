"""GPU: ssvi_surface_kernel (ivs_ssvi_surface_f64) against the restatement of rules J1-J8 (tests/ssvi_ref.py).

Flags, sflags and every NaN pattern equal the restatement's; the values agree within ssvi_cases.tolerances: C_GPU x R_CPU, the
restatement's own sensitivity to one unit in the last place of the input (test_ssvi.test_twin_sensitivity), or the number
format's floor where that is wider (DESIGN.md section 15 has the reasoning).  A snapshot that ends more than UNSTABLE_STEPS
final steps from the restatement is unstable: it is left out of the value and EDGE comparisons, not of the rest, and at most
UNSTABLE_SHARE of a case's fitted snapshots may be.

Every test prints its largest error / tolerance ratios; with IVS_SSVI_ERRLOG=<file> set the figures are appended to that file
(a recorded run belongs in profiles/ssvi/errlog_gpu.txt; errlog.txt there holds the CPU run)."""
import ctypes
import os

import numpy as np
import pytest

import ssvi_cases as C
import ssvi_ref as R

pytestmark = pytest.mark.gpu
SENT_F, SENT_I = -7.25e9, -77        # no output of the rules: flags >= 0; no value ever hits -7.25e9
GUARD = 67                           # elements of guard tail behind every output
KEYS = ("surface", "theta", "params", "fit", "flags", "sflags")
EDGES = C.EDGE_RHO | C.EDGE_GAMMA | C.EDGE_ETA_LOW | C.AT_BOUND


def log(name, **figures):
    line = name + ": " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items())
    print(line)
    path = os.environ.get("IVS_SSVI_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def host(t):
    return None if t is None else t.cpu().numpy()


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, np.float64, order="C")).cuda()   # a copy: the shared cases are read-only


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


def run(c, rounds=0, fitted=True, stream=None):
    """One call with every output pre-filled with a sentinel and followed by a guard tail."""
    import torch
    from iv_interpolation_amd import engine
    B, mT, mK = c["vol"].shape
    f64, i32 = torch.float64, torch.int32
    flat, out = guarded({"surface": ((B, 4), f64), "theta": ((B, mT), f64), "params": ((B, mT, 5), f64), "fit": ((B, mT, 3), f64),
                         "flags": ((B, mT), i32), "sflags": ((B,), i32), "fitted": ((B, mT, mK), f64)})
    q = engine.ssvi_surface(dev(c["vol"]), dev(c["Kq"]), dev(c["Tq"]), dev(c["spot"]), c["rate"], raw=dev(c.get("raw")),
                            theta0=dev(c.get("theta0")), rounds=rounds, fitted=fitted,
                            out={k: v for k, v in out.items() if fitted or k != "fitted"}, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    assert engine.last_kernel() == "ssvi_surface_kernel" and set(q) == set(KEYS) | {"fitted"}
    got = check_written(flat, out, KEYS + (("fitted",) if fitted else ()))
    if not fitted:
        assert q["fitted"] is None and (host(flat["fitted"]) == SENT_F).all(), "fitted=False touched the buffer"
        got["fitted"] = None
    return got


def compare(name, got, ref, rounds):
    rounds = R.DEFAULT_ROUNDS if rounds == 0 else rounds
    assert got["flags"].dtype == np.int32 and got["sflags"].dtype == np.int32
    u, tol = C.units(got, ref), C.tolerances(ref, rounds)
    live = np.isfinite(u["steps"])
    same = u["point_eps"] <= C.SAME_POINT / C.EPS
    unstable = live & ~same & (u["steps"] > C.UNSTABLE_STEPS)
    keep = live & ~unstable
    fig = {}
    for k in tol:
        with np.errstate(all="ignore"):
            ratio = np.where(tol[k] > 0, u[k] / tol[k], np.where(u[k] > 0, np.inf, 0.0))
        if k == "steps":
            ratio = np.where(same, 0.0, ratio)
        fig[k] = float(np.max(ratio[keep])) if keep.any() else 0.0
    log(name, **fig, point_eps=float(np.max(u["point_eps"][keep])) if keep.any() else 0.0, fitted=int(live.sum()), unstable=int(unstable.sum()))
    assert np.array_equal(got["flags"] & ~C.BUTTERFLY, ref["flags"] & ~C.BUTTERFLY), (name, got["flags"], ref["flags"])
    assert not (got["flags"][got["flags"] != C.DEAD] & C.BUTTERFLY).any(), (name, "BUTTERFLY")
    assert np.array_equal(got["sflags"] & ~EDGES, ref["sflags"] & ~EDGES), (name, got["sflags"], ref["sflags"])
    assert np.array_equal((got["sflags"] & EDGES)[keep], (ref["sflags"] & EDGES)[keep]), (name, got["sflags"], ref["sflags"])
    for k in ("surface", "theta", "params", "fit", "fitted"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (name, k)
    assert unstable.sum() <= C.UNSTABLE_SHARE * max(int(live.sum()), 1), (name, "unstable", int(unstable.sum()))
    assert all(v <= 1.0 for v in fig.values()), (name, fig)


def same_bits(a, b, keys, what):
    for k in keys:
        if a[k] is None:
            assert b[k] is None, (k, what)
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), (k, what)


_cache = {}


def case(n, rounds=0):
    """Inputs and restatement of one generated batch, computed once and shared (read-only)."""
    if (n, rounds) not in _cache:
        c, _ = C.batch(**C.SHAPES[n])
        r = R.restate(**C.case_args(c), rounds=rounds, margins=C.SHAPES[n]["mT"] >= 2 and rounds == 0)
        for a in list(c.values()) + list(r.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[(n, rounds)] = (c, r)
    return _cache[(n, rounds)]


def shape_index(B, mT, mK):
    return next(n for n, s in enumerate(C.SHAPES) if (s["B"], s["mT"], s["mK"]) == (B, mT, mK))


@pytest.mark.parametrize("name", sorted(C.MICRO))
def test_micro(name):
    c = C.MICRO[name]
    got = run(c)
    assert np.array_equal(got["flags"], c["flags"]), got["flags"]
    assert np.array_equal(got["sflags"] & ~c["sfree"], c["sflags"]), got["sflags"]
    if name == "decreasing_theta0":
        assert np.array_equal(got["params"][0, 2], got["params"][0, 1]) and got["theta"][0, 2] == got["theta"][0, 1] == 0.05
    if name == "row_without_nodes":
        assert np.isnan(got["fit"][0, 1]).all() and np.isfinite(got["params"][0, 1]).all() and np.isfinite(got["fitted"][0, 1]).all()
    compare(f"micro[{name}]", got, R.restate(**C.case_args(c)), 0)


@pytest.mark.parametrize("n", range(len(C.SHAPES)), ids=[C.shape_id(s) for s in C.SHAPES])
def test_shapes(n):
    """B in {1, 3}, mT in {1, 2, 13, 16, 64}, mK in {5, 63, 64, 65, 130, 48}: shared and per-snapshot grids, theta0 and raw,
    rate 0 and 0.03, 10 % missing nodes, dead and raised rows."""
    c, r = case(n)
    compare(f"shape[{C.shape_id(C.SHAPES[n])}]", run(c), r, 0)


@pytest.mark.parametrize("n", range(len(C.SHAPES)), ids=[C.shape_id(s) for s in C.SHAPES])
def test_four_rounds_end_on_the_restatements_grid_point(n):
    """rounds = 4 pins the round logic: the same grid point, within 4 eps of the domain's width."""
    c, r = case(n, 4)
    got = run(c, rounds=4)
    u = C.units(got, r)
    live = np.isfinite(u["point_eps"])
    log(f"four_rounds[{C.shape_id(C.SHAPES[n])}]", point_eps=float(np.max(u["point_eps"][live])) if live.any() else 0.0)
    assert (u["point_eps"][live] <= C.SAME_POINT / C.EPS).all(), u["point_eps"]
    compare(f"four_rounds_values[{C.shape_id(C.SHAPES[n])}]", got, r, 4)


def test_shared_and_per_snapshot_grids_agree_bitwise():
    c, _ = case(shape_index(3, 13, 65))                                       # shared Kq, per-snapshot Tq
    wide = dict(c, Kq=np.tile(c["Kq"], (3, 1)))
    same_bits(run(c), run(wide), KEYS + ("fitted",), "kq")
    c, _ = case(shape_index(3, 64, 5))                                        # per-snapshot Kq, shared Tq
    wide = dict(c, Tq=np.tile(c["Tq"], (3, 1)))
    same_bits(run(c), run(wide), KEYS + ("fitted",), "tq")


def test_raw_and_the_equivalent_theta0_agree_bitwise():
    for n in (shape_index(3, 16, 64), shape_index(3, 2, 63)):
        c, _ = case(n)
        th0 = R.theta0_of_raw(c["raw"], c["Tq"], c["spot"])
        alt = {k: v for k, v in c.items() if k != "raw"}
        alt["theta0"] = th0
        same_bits(run(c), run(alt), KEYS + ("fitted",), "raw against theta0")
    m = C.MICRO["raw_with_a_dead_slice"]
    alt = {k: v for k, v in m.items() if k != "raw"}
    alt["theta0"] = R.theta0_of_raw(m["raw"], m["Tq"], m["spot"])
    same_bits(run(m), run(alt), KEYS + ("fitted",), "micro raw against theta0")


def test_fitted_left_out():
    """fitted=False leaves its buffer untouched, and the other outputs keep their bits."""
    c, _ = case(shape_index(3, 16, 64))
    same_bits(run(c), run(c, fitted=False), KEYS, "fitted=False")


def test_explicit_stream_then_immediate_reallocation():
    """The call runs on an explicit stream while another stream is current; its inputs are temporaries that die when the call
    returns, and tensors of the same sizes are allocated and filled on the current stream at once (record_stream)."""
    import torch
    from iv_interpolation_amd import engine
    c, _ = C.batch(**C.STREAM_SHAPE)
    base = run(c, rounds=6)
    assert (base["flags"] != C.DEAD).mean() >= 0.9
    same_bits(base, run(c, rounds=6, stream=torch.cuda.Stream()), KEYS + ("fitted",), "stream")
    s = torch.cuda.Stream()
    with torch.cuda.stream(torch.cuda.Stream()):
        q = engine.ssvi_surface(dev(c["vol"]), dev(c["Kq"]), dev(c["Tq"]), dev(c["spot"]), c["rate"], theta0=dev(c["theta0"]), rounds=6,
                                fitted=True, stream=s)
        junk = [torch.full(x.shape, 3.0, dtype=torch.float64, device="cuda") for x in (c["vol"], c["Kq"], c["Tq"], c["spot"], c["theta0"]) for _ in range(3)]
        s.synchronize()
        torch.cuda.synchronize()
    same_bits(base, {k: host(v) for k, v in q.items()}, KEYS + ("fitted",), "reallocation")
    del junk


def test_abi_error_table():
    import torch
    from iv_interpolation_amd import _lib, engine
    c, _ = case(shape_index(3, 16, 64))
    v, k, t, s, raw = dev(c["vol"]), dev(c["Kq"]), dev(c["Tq"]), dev(c["spot"]), dev(c["raw"])
    th0 = raw[..., 0].contiguous()
    z = lambda *shape: torch.ones(shape, dtype=torch.float64, device="cuda")   # noqa: E731
    for bad in (lambda: engine.ssvi_surface(v[0], k, t, s, raw=raw), lambda: engine.ssvi_surface(v, k[:, :-1], t, s, raw=raw),
                lambda: engine.ssvi_surface(v, k, t[:-1], s, raw=raw), lambda: engine.ssvi_surface(v, k, t, torch.cat([s, s]), raw=raw),
                lambda: engine.ssvi_surface(v, k, t, s), lambda: engine.ssvi_surface(v, k, t, s, raw=raw, theta0=th0),
                lambda: engine.ssvi_surface(v, k, t, s, raw=raw[..., :4]), lambda: engine.ssvi_surface(v, k, t, s, theta0=th0[:, :-1]),
                lambda: engine.ssvi_surface(v, k, t, s, raw=raw, rounds=33), lambda: engine.ssvi_surface(v, k, t, s, raw=raw, rounds=-1),
                lambda: engine.ssvi_surface(z(1, 65, 2), z(2), z(65), z(1), theta0=z(1, 65)),
                lambda: engine.ssvi_surface(z(1, 64, 49), z(49), z(64), z(1), theta0=z(1, 64)),
                lambda: engine.ssvi_surface(v, k, t, s, raw=raw, out={"sflags": torch.empty(3, dtype=torch.float64, device="cuda")})):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        engine.ssvi_surface(v.float(), k, t, s, raw=raw)
    with pytest.raises(TypeError):
        engine.ssvi_surface(v, k, t, s, theta0=th0.float())
    lib = _lib.load()
    B, mT, mK = v.shape
    f64, i32 = torch.float64, torch.int32
    flat, out = guarded({"surface": ((B, 4), f64), "theta": ((B, mT), f64), "params": ((B, mT, 5), f64), "fit": ((B, mT, 3), f64),
                         "flags": ((B, mT), i32), "sflags": ((B,), i32), "fitted": ((B, mT, mK), f64)})

    def args(**kw):
        a = _lib.SsviArgs()
        a.vol, a.Kq, a.kq_stride, a.Tq, a.tq_stride, a.spot, a.rate = v.data_ptr(), k.data_ptr(), mK, t.data_ptr(), 0, s.data_ptr(), 0.03
        a.raw, a.theta0, a.mK, a.mT, a.B, a.rounds = raw.data_ptr(), None, mK, mT, B, 0
        for key in out:
            setattr(a, key, out[key].data_ptr())
        for key, val in kw.items():
            setattr(a, key, val)
        return a

    call = lambda **kw: lib.ivs_ssvi_surface_f64(ctypes.byref(args(**kw)), None, 0, None)   # noqa: E731
    EINVAL, ERANGE = -22, -34
    assert lib.ivs_ssvi_surface_f64(None, None, 0, None) == EINVAL and b"null args" in lib.ivs_last_error()
    for key in ("vol", "Kq", "Tq", "spot", "surface", "theta", "params", "fit", "flags", "sflags"):
        assert call(**{key: None}) == EINVAL and b"null pointer" in lib.ivs_last_error(), key
    assert call(theta0=th0.data_ptr()) == EINVAL and b"exactly one" in lib.ivs_last_error()
    assert call(raw=None) == EINVAL and b"exactly one" in lib.ivs_last_error()
    assert call(B=-1) == EINVAL and call(mT=-1) == EINVAL and call(mK=-1) == EINVAL and b"negative" in lib.ivs_last_error()
    assert call(kq_stride=7) == EINVAL and b"stride" in lib.ivs_last_error()
    assert call(tq_stride=3) == EINVAL and call(tq_stride=-1) == EINVAL
    assert call(mT=65, mK=1, kq_stride=1) == ERANGE and b"mT=65" in lib.ivs_last_error()
    assert call(mK=0, kq_stride=0) == ERANGE and b"mK=0" in lib.ivs_last_error()
    assert call(mT=64, mK=49, kq_stride=49) == ERANGE and b"LDS" in lib.ivs_last_error()
    assert call(rounds=33) == ERANGE and call(rounds=-1) == ERANGE and b"rounds" in lib.ivs_last_error()
    assert call(B=(1 << 31) // (mT * mK) + 1) == ERANGE and b"exceed" in lib.ivs_last_error()
    assert call(B=0) == 0 and call(mT=0) == 0                                  # a no-op
    torch.cuda.synchronize()
    for key, f in flat.items():                                               # a refused call launches nothing
        assert (host(f) == (SENT_I if f.dtype == i32 else SENT_F)).all(), key
    assert call() == 0                                                        # ... and the table's own arguments are good
    torch.cuda.synchronize()
    check_written(flat, out, KEYS + ("fitted",))


def test_builder_and_frames_on_a_wide_chain():
    """End to end on the wide chain of the SVI GPU test: build -> svi -> ssvi, then calendar, distribution and price on the
    SSVI params: no pair of any snapshot is CALENDAR, prices are positive near the money, the frames have their rows."""
    import cal_cases as CC
    import svi_cases as SC
    import snapshot_cases as SNC
    from iv_interpolation_amd import _lib
    from iv_interpolation_amd.snapshots import (HipBackend, SnapshotSurfaceBuilder, calendar_frame, distribution_frame, price_frame,
                                                ssvi_frame, ssvi_slices_frame)
    ten = SC.CHAIN_TENORS
    b = SnapshotSurfaceBuilder(moneyness=SC.CHAIN_MONEYNESS, tenors=ten, backend=HipBackend())
    res = b.build(SNC.big_chain(**SC.CHAIN))
    fits = b.svi(res, rate=SC.CHAIN_RATE)
    surf = b.ssvi(res, fits, rate=SC.CHAIN_RATE, fitted=True)
    own = b.ssvi(res, rate=SC.CHAIN_RATE)                                     # runs svi itself: the same bits
    assert [d.underlying for d in surf] == ["btc", "eth"]
    for d, o in zip(surf, own):
        same_bits({k: host(getattr(d, k)) for k in KEYS}, {k: host(getattr(o, k)) for k in KEYS}, KEYS, "own svi")
        assert o.fitted is None and d.fitted.shape == (40, len(ten), 64)
    cals = b.calendar(res, surf)
    dist = b.distribution(res, surf, rate=SC.CHAIN_RATE)
    book = CC.chain_book(res)
    marks = b.price(res, book, surf, rate=SC.CHAIN_RATE)
    n_live = 0
    for d, cl in zip(surf, cals):
        fl, sf, cf = host(d.flags), host(d.sflags), host(cl.flags)
        assert (sf & (_lib.SF_SURF_DEAD | _lib.SF_UNORDERED) == 0).all() and (fl & _lib.SS_BUTTERFLY == 0).all()
        assert np.array_equal(cf == _lib.SC_DEAD, fl == _lib.SS_DEAD)           # every live SSVI row is live downstream (P1)
        assert (cf & (_lib.SC_CALENDAR | _lib.SC_WING_LEFT | _lib.SC_WING_RIGHT | _lib.SC_UNORDERED) == 0).all(), d.underlying
        n_live += int((fl != _lib.SS_DEAD).sum())
    log("chain", live_rows=n_live, raised=int(sum((host(d.flags) & _lib.SS_RAISED != 0).sum() for d in surf)),
        rmse_max=float(max(np.nanmax(host(d.surface)[:, 3]) for d in surf)))
    f = ssvi_frame(surf, res)
    assert len(f) == 80 and set(f["underlying"]) == {"btc", "eth"} and f["live_rows"].between(1, len(ten)).all() and f["rho"].between(-1, 1).all()
    g = ssvi_slices_frame(surf, res)
    assert len(g) == n_live == int(f["live_rows"].sum()) and (g["theta"] > 0).all() and (g["sigma"] > 0).all()
    assert len(calendar_frame(cals, res)) == n_live - 80                         # one pair per live row but the last
    assert len(distribution_frame(dist, res)) == 80 * len(ten)
    p = price_frame(marks, res)
    assert len(p) == 80 * len(book)
    near = p[(p["flags"] & _lib.SE_DEAD == 0) & (p["underlying"] == "btc")]   # the book's strikes lie round btc's spot
    assert len(near) and (near["call"] > 0).all() and (near["put"] > 0).all() and near["vol"].between(0.05, 3.0).all()
