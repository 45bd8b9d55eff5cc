"""GPU: svi_inst_pnl_kernel and hedge_pursuit_kernel (ivs_svi_hedge_f64) against the restatement of rules M0-M11 (tests/hedge_ref.py).

Stage 1 value tests compare inst_pnl with the restatement within the term allowance of section 19 (C_GPU x hsim_cases.R_CPU["pnl"]
units of eps x the term's scale), patterns equal, and a column with the device's own section 19 call on the one-option book.
Stage 2 value tests feed the kernel the RESTATEMENT's inst_pnl, pnl and scen_flags, so that both sides see the same rows: pick,
n_rounds, the flags and every NaN pattern must be equal, the values agree within C_GPU x R_CPU units of eps x the value's own scale
(hedge_cases.R_CPU; DESIGN.md section 21 has the reasoning).  Chain tests run on the device's own rows and compare bits only.  The
deep greedy run is checked by its invariants.

Every test prints its largest error / allowance ratios; with IVS_HEDGE_ERRLOG=<file> set the figures are appended to that file as
well (a recorded run belongs in profiles/hedge/errlog_gpu.txt; errlog.txt there holds the CPU run)."""
import ctypes
import os

import numpy as np
import pytest

import hedge_cases as GC
import hedge_ref as G
import hsim_ref as H

pytestmark = pytest.mark.gpu
SENT_F, SENT_I = -7.25e9, -77        # no output of the rules: picks and counts >= -1, flags >= 0; no value ever hits -7.25e9
GUARD = 67                           # elements of guard tail behind every output
STAGE1 = ("inst_pnl", "inst_value")
OPTIONAL = ("solo_qty", "solo_left", "inst_value")
EPS = GC.EPS
_cache = {}


def log(name, **figures):
    line = name + ": " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items())
    print(line)
    path = os.environ.get("IVS_HEDGE_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def host(t):
    return None if t is None else t.cpu().numpy()


def dev(a, dtype=np.float64):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, dtype, order="C")).cuda()


def shapes_of(c, B=None):
    import torch
    B = c["params"].shape[0] if B is None else B
    w, nL, nH, K = c["window"], len(c["tail_probs"]), len(c["inst_kind"]), c["rounds"]
    f, i = torch.float64, torch.int32
    return dict(inst_pnl=((B, w, nH), f), inst_flags=((B, nH), i), pick=((B, K), i), ss=((B, K + 1), f), n_rounds=((B,), i), hedge=((B, nH), f),
                pnl_hedged=((B, w), f), var_h=((B, nL), f), es_h=((B, nL), f), worst_h=((B,), i), n_scen=((B,), i), solo_qty=((B, nH), f),
                solo_left=((B, nH), f), inst_value=((B, nH), f))


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


def book_on_device(c):
    """Section 19's own call on the case's book: device tensors."""
    import torch
    from iv_interpolation_amd import engine
    q = engine.svi_hsim(dev(c["params"]), dev(c["Tq"]), dev(c["spot"]), c["rate"], dev(c["u"]), dev(c["tau"]), dev(c["qty"]), lag=c["lag"],
                        window=c["window"], tail_probs=c["tail_probs"], min_scen=c["min_scen"], is_put=dev(c["is_put"], np.uint8),
                        strike_mode=c["strike_mode"])
    torch.cuda.synchronize()
    return q


def run(c, pnl, scen_flags, stages=0, inst_pnl=None, want=OPTIONAL, abi=False, stream=None, **over):
    """The call through engine.svi_hedge, or (abi) through the C entry point itself, into sentinel-filled outputs.  pnl, scen_flags,
    inst_pnl (the input of stages = 2): host arrays or device tensors."""
    import torch
    from iv_interpolation_amd import _lib, engine
    c = dict(c, **over)
    flat, out = guarded(shapes_of(c))
    if inst_pnl is not None:
        out["inst_pnl"].copy_(inst_pnl if torch.is_tensor(inst_pnl) else dev(inst_pnl))
    keys = tuple(k for k in G.OUT_KEYS if (k in STAGE1) == (stages == 1) or stages == 0)
    keys = tuple(k for k in keys if k not in OPTIONAL or k in want)
    t = dict(params=dev(c["params"]), Tq=dev(c["Tq"]), spot=dev(c["spot"]), inst_u=dev(c["inst_u"]), inst_tau=dev(c["inst_tau"]),
             inst_kind=dev(c["inst_kind"], np.uint8))
    pnl = pnl if torch.is_tensor(pnl) else dev(pnl)
    scen_flags = scen_flags if torch.is_tensor(scen_flags) else dev(scen_flags, np.int32)
    if abi:
        a = _lib.HedgeArgs()
        B, mT = c["params"].shape[:2]
        nH = len(c["inst_kind"])
        for k, v in t.items():
            setattr(a, k, v.data_ptr())
        a.pnl, a.scen_flags = pnl.data_ptr(), scen_flags.data_ptr()
        a.tq_stride, a.inst_stride, a.rate = (mT if np.ndim(c["Tq"]) == 2 else 0), (nH if np.ndim(c["inst_u"]) == 2 else 0), c["rate"]
        a.strike_mode, a.mT, a.nH, a.B, a.lag, a.window = c["strike_mode"], mT, nH, B, c["lag"], c["window"]
        tp = list(c["tail_probs"])
        a.tail_probs, a.nL, a.min_scen = ctypes.cast((ctypes.c_double * max(len(tp), 1))(*tp), ctypes.POINTER(ctypes.c_double)), len(tp), c["min_scen"]
        a.rounds, a.n_forced, a.tol, a.min_gain, a.stages = c["rounds"], c["n_forced"], c["tol"], c["min_gain"], stages
        for k in set(keys) | {"inst_pnl"}:
            setattr(a, k, out[k].data_ptr())
        lib = _lib.load()
        assert lib.ivs_svi_hedge_f64(ctypes.byref(a), None, 0, None) == 0, lib.ivs_last_error()
        assert lib.ivs_last_kernel() == (b"svi_inst_pnl_kernel" if stages == 1 else b"hsim_tail_kernel")
    else:
        q = engine.svi_hedge(t["params"], t["Tq"], t["spot"], c["rate"], t["inst_u"], t["inst_tau"], t["inst_kind"], pnl, scen_flags, lag=c["lag"],
                             window=c["window"], tail_probs=c["tail_probs"], min_scen=c["min_scen"], rounds=c["rounds"], n_forced=c["n_forced"],
                             tol=c["tol"], min_gain=c["min_gain"], strike_mode=c["strike_mode"], want=tuple(k for k in OPTIONAL if k in want),
                             out={k: out[k] for k in set(keys) | {"inst_pnl"}}, stream=stream, stages=stages)
        assert engine.last_kernel() == ("svi_inst_pnl_kernel" if stages == 1 else "hsim_tail_kernel") and set(q) == set(G.OUT_KEYS)
        assert all((q[k] is None) == (k not in keys and k != "inst_pnl") for k in G.OUT_KEYS)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    got = {}
    for k in G.OUT_KEYS:
        v, tail = host(out[k]), host(flat[k])[out[k].numel():]
        assert (tail == sentinel(flat[k])).all(), f"{k}: the guard tail was touched"
        if k in keys:
            assert not (v == sentinel(flat[k])).any(), f"{k}: an element was not written"
            got[k] = v
        elif k == "inst_pnl":
            got[k] = v                                       # the input of stage 2
        else:
            assert (v == sentinel(flat[k])).all(), f"{k}: left out, yet written"
            got[k] = None
    return got


def case(name):
    """(case, section 19 restated on its book, the hedge restated on those rows)."""
    if name not in _cache:
        c = GC.make(name)
        h = H.restate_hsim(c["params"], c["Tq"], c["spot"], c["rate"], c["u"], c["tau"], c["qty"], c["lag"], c["window"], c["tail_probs"],
                           c["min_scen"], c["is_put"], c["strike_mode"])
        r = G.restate_hedge(c["params"], c["Tq"], c["spot"], c["rate"], c["inst_u"], c["inst_tau"], c["inst_kind"], h["pnl"], h["scen_flags"],
                            c["lag"], c["window"], c["tail_probs"], c["min_scen"], c["rounds"], c["n_forced"], c["tol"], c["min_gain"],
                            c["strike_mode"])
        _cache[name] = (c, h, r)
    return _cache[name]


def compare(name, got, ref, keys=GC.VALUE_KEYS, ints=GC.INT_KEYS):
    for k in ints:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), (name, k, got[k], ref[k])
    u = GC.allowance_ratios(got, ref, GC.C_GPU, keys)
    fig = {k: (float(np.nanmax(v)) if np.isfinite(v).any() else 0.0) for k, v in u.items()}
    log(name, **fig)
    for k in u:
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (name, k)
    assert all(v <= 1.0 for v in fig.values()), (name, fig)


def same_bits(a, b, keys, what):
    for k in keys:
        if a[k] is None or b[k] is None:
            continue
        assert np.array_equal(a[k], b[k], equal_nan=True), (k, what)
        assert np.array_equal(np.signbit(np.nan_to_num(a[k])), np.signbit(np.nan_to_num(b[k]))), (k, what)     # a zero's sign too


# ------------------------------------------------------------------ stage 1
@pytest.mark.parametrize("name", sorted(GC.CASES))
def test_stage1_values(name):
    c, h, r = case(name)
    got = run(c, h["pnl"], h["scen_flags"], stages=1, abi=name in ("three_lag2", "nine_63"))
    compare("stage1 " + name, got, r, keys=("inst_pnl",), ints=())
    und = c["inst_kind"] == GC.UND
    assert np.array_equal(np.isnan(got["inst_value"]), r["rows"]["dead"])
    assert np.array_equal(got["inst_value"][:, und], np.where(r["rows"]["dead"], np.nan, c["spot"][:, None])[:, und], equal_nan=True)
    if und.any():                                            # the underlying's row is three IEEE operations on the spots: the bits
        same_bits(dict(x=got["inst_pnl"][:, :, und]), dict(x=r["inst_pnl"][:, :, und]), ("x",), name)


def test_stage1_column_is_the_one_option_book_of_section_19():
    """M2's link: on the device too, a candidate option's column is section 19's row of the book of that contract at quantity 1.0."""
    from iv_interpolation_amd import engine
    c, h, r = case("nine_63")
    got = run(c, h["pnl"], h["scen_flags"], stages=1, want=())
    for hh in np.flatnonzero((c["inst_kind"] != GC.UND) & ~r["rows"]["dead"].any(axis=0))[[0, 17, -1]]:
        q = engine.svi_hsim(dev(c["params"]), dev(c["Tq"]), dev(c["spot"]), c["rate"], dev(c["inst_u"][:, hh:hh + 1]), dev(c["inst_tau"][:, hh:hh + 1]),
                            dev([1.0]), lag=c["lag"], window=c["window"], tail_probs=(), min_scen=1,
                            is_put=dev([int(c["inst_kind"][hh] == GC.PUT)], np.uint8), strike_mode=c["strike_mode"], value=False)
        assert np.array_equal(host(q["pnl"]) + 0.0, got["inst_pnl"][:, :, hh] + 0.0, equal_nan=True), hh


def test_stage1_same_bits_for_every_run_length():
    c, h, r = case("second_word")
    base = run(c, h["pnl"], h["scen_flags"], stages=1)
    from iv_interpolation_amd import engine
    for spw in (1, 100, 256, 257):
        out = engine.svi_hedge(dev(c["params"]), dev(c["Tq"]), dev(c["spot"]), c["rate"], dev(c["inst_u"]), dev(c["inst_tau"]),
                               dev(c["inst_kind"], np.uint8), dev(h["pnl"]), dev(h["scen_flags"], np.int32), lag=c["lag"], window=c["window"],
                               tail_probs=c["tail_probs"], min_scen=c["min_scen"], rounds=c["rounds"], strike_mode=c["strike_mode"], stages=1,
                               scen_per_wg=spw)
        same_bits(dict(x=host(out["inst_pnl"]), v=host(out["inst_value"])), dict(x=base["inst_pnl"], v=base["inst_value"]), ("x", "v"), spw)


# ------------------------------------------------------------------ stage 2 on the restatement's rows
@pytest.mark.parametrize("name", sorted(GC.CASES))
def test_stage2_values(name):
    c, h, r = case(name)
    got = run(c, h["pnl"], h["scen_flags"], stages=2, inst_pnl=r["inst_pnl"], abi=name in ("collinear", "wide_tenors"))
    compare("stage2 " + name, got, r)
    assert got["inst_value"] is None


@pytest.mark.parametrize("name", sorted(GC.TABLES))
def test_stage2_tables_by_hand(name):
    t = GC.TABLES[name]
    r = G.select(t["inst_pnl"], np.zeros((t["inst_pnl"].shape[0], t["nH"]), bool), t["pnl"], t["scen_flags"], t["lag"], t["tail_probs"],
                 t["min_scen"], t["rounds"], t["n_forced"], t["tol"], t["min_gain"])
    got = run(t, t["pnl"], t["scen_flags"], stages=2, inst_pnl=t["inst_pnl"])
    compare("table " + name, got, r)
    p, w = t["window"], t["want"]
    assert list(got["pick"][p]) == list(w["pick"]) and list(got["inst_flags"][p]) == list(w["inst_flags"])
    if name in ("minus_two", "min_gain", "unranked"):        # integer rows, every operation exact
        assert np.array_equal(got["hedge"][p], w["hedge"]) and np.array_equal(got["ss"][p], w["ss"])


@pytest.mark.parametrize("name", sorted(GC.MICRO))
def test_micro_cases(name):
    """hedge_cases.MICRO through both stages on the device: a dead candidate and one with a scenario vol that is not positive, H6
    pairs (exactly +0.0 for options and the underlying), a snapshot without a live slice and an UNORDERED one (the underlying DEAD
    there).  Flags, picks and patterns are the restatement's and the hand-made ones; the values are compared on the restatement's rows."""
    c = GC.MICRO[name]
    r = G.restate_hedge(c["params"], c["Tq"], c["spot"], c["rate"], c["inst_u"], c["inst_tau"], c["inst_kind"], c["pnl"], c["row_flags"], c["lag"],
                        c["window"], c["tail_probs"], c["min_scen"], c["rounds"], c["n_forced"], c["tol"], c["min_gain"], c["strike_mode"])
    got = run(c, c["pnl"], c["row_flags"])
    compare("micro stage1 " + name, got, r, keys=("inst_pnl",), ints=("inst_flags", "pick", "n_rounds"))
    assert np.array_equal(np.isnan(got["inst_value"]), r["rows"]["dead"])
    for p, (fl, pk) in enumerate(zip(c["want"]["inst_flags"], c["want"]["pick"])):
        if fl is not None:
            assert list(got["inst_flags"][p]) == fl and list(got["pick"][p]) == pk, p
    if name == "h6_pair":
        for z in (got["inst_pnl"][1, 0], got["inst_pnl"][2, 1]):
            assert (z == 0.0).all() and not np.signbit(z).any()
    compare("micro stage2 " + name, run(c, c["pnl"], c["row_flags"], stages=2, inst_pnl=r["inst_pnl"]), r)


# ------------------------------------------------------------------ the chain on the device's own rows: bits
def m10(y, x, pick, hedge):
    """M10 restated on the kernel's own outputs."""
    out = np.full(y.shape, np.nan)
    for p in range(y.shape[0]):
        ok = ~np.isnan(y[p])
        row = y[p].copy()
        for c in pick[p]:
            if c >= 0:
                row = row + hedge[p, c] * x[p, :, c]
        out[p, ok] = row[ok]
    return out


@pytest.mark.parametrize("name", ["forced8", "collinear", "second_word", "deep", "stream"])
def test_chain_on_the_device_rows(name):
    c = GC.make(name)
    q = book_on_device(c)
    a = run(c, q["pnl"], q["scen_flags"])
    keys = tuple(k for k in G.OUT_KEYS)
    same_bits(a, run(c, q["pnl"], q["scen_flags"]), keys, "two runs")
    one = run(c, q["pnl"], q["scen_flags"], stages=1)
    two = run(c, q["pnl"], q["scen_flags"], stages=2, inst_pnl=one["inst_pnl"])
    same_bits(a, dict(two, inst_value=one["inst_value"]), keys, "stages 0 against 1 then 2")
    pnl, fl = host(q["pnl"]), host(q["scen_flags"])
    n_p, _ = H.exists(pnl.shape[0], c["lag"], c["window"])
    ranked = (fl == 0) & ~np.isnan(pnl) & (np.arange(c["window"])[None, :] < n_p[:, None])
    same_bits(dict(r=a["pnl_hedged"]), dict(r=m10(np.where(ranked, pnl, np.nan), a["inst_pnl"], a["pick"], a["hedge"])), ("r",), "M10")
    var, es, n, worst = H.tail(a["pnl_hedged"], fl, c["tail_probs"], c["min_scen"])
    same_bits(a, dict(var_h=var, es_h=es, worst_h=worst, n_scen=n), ("var_h", "es_h", "worst_h", "n_scen"), "H7 on the hedged row")
    # every round empty: section 19's bits
    z = run(c, q["pnl"], q["scen_flags"], stages=2, inst_pnl=one["inst_pnl"], min_gain=0.999e9, n_forced=0)
    assert (z["pick"] == -1).all() and (z["n_rounds"] == 0).all()
    same_bits(z, dict(var_h=host(q["var"]), es_h=host(q["es"]), worst_h=host(q["worst"]), n_scen=host(q["n_valid"]), pnl_hedged=pnl),
              ("var_h", "es_h", "worst_h", "n_scen", "pnl_hedged"), "every round empty")
    # invariants, on every snapshot: distinct picks, ss not increasing, the hedged row orthogonal to every pick, each within the
    # units of the restatement forced through the device's picks on the device's rows
    worst_fig = dict(orth=0.0, mono=0.0)
    for p in range(pnl.shape[0]):
        picks = [int(v) for v in a["pick"][p] if v >= 0]
        assert len(set(picks)) == len(picks) == a["n_rounds"][p]
        if not picks:
            continue
        idx = np.flatnonzero(ranked[p])
        x, y = a["inst_pnl"][p, idx], pnl[p, idx]
        f = G.pursue(x[:, picks], y, np.zeros(len(picks), bool), len(picks), len(picks), 0.0, 0.0, True)
        row, drow = G.hedged_row(y, x[:, picks], [f["q"][k] for k in sorted(f["q"])])
        for j in range(len(picks)):
            v, dv = G._dot(x[:, picks[j]], 0.0, a["pnl_hedged"][p, idx], drow)
            worst_fig["orth"] = max(worst_fig["orth"], abs(float(v)) / (EPS * float(dv)))
        ss, ds = a["ss"][p], f["scale_ss"]
        nz = [0] + [k + 1 for k in range(c["rounds"]) if a["pick"][p, k] >= 0]
        for i in range(len(nz) - 1):
            worst_fig["mono"] = max(worst_fig["mono"], float((ss[nz[i + 1]] - ss[nz[i]]) / (EPS * (ds[i] + ds[i + 1]) + GC.TINY)))
        assert all(ss[k + 1] == ss[k] for k in range(c["rounds"]) if a["pick"][p, k] < 0)
    log("chain " + name, **worst_fig, rounds=int(a["n_rounds"].sum()))
    assert worst_fig["orth"] <= 1.0 and worst_fig["mono"] <= 1.0, worst_fig


def test_a_snapshot_against_a_call_on_its_own_rows():
    c = GC.make("collinear")
    p = c["params"].shape[0] - 1
    lo = max(0, p - c["window"] - c["lag"] + 1)
    q = book_on_device(c)
    a = run(c, q["pnl"], q["scen_flags"])
    sub = {k: (np.asarray(c[k])[lo:] if k in ("params", "spot") else c[k]) for k in c}
    qs = book_on_device(sub)
    b = run(sub, qs["pnl"], qs["scen_flags"])
    same_bits({k: v[p] for k, v in a.items()}, {k: v[p - lo] for k, v in b.items()}, G.OUT_KEYS, "a snapshot alone")


# ------------------------------------------------------------------ housekeeping
def test_null_optional_outputs():
    c, h, r = case("nine_63")
    a = run(c, h["pnl"], h["scen_flags"])
    b = run(c, h["pnl"], h["scen_flags"], want=())
    assert b["solo_qty"] is None and b["solo_left"] is None and b["inst_value"] is None
    same_bits(a, b, G.OUT_KEYS, "NULL optional outputs")


def test_the_largest_rows_fit_the_workgroup():
    """window 1024 and 8 rounds: 72 KB of rows per workgroup."""
    c = GC.generated(B=6, mT=2, Q=2, lag=1, window=1024, nL=1, nH=3, rounds=8, seed=2120, min_scen=1, n_forced=3)
    h = H.restate_hsim(c["params"], c["Tq"], c["spot"], c["rate"], c["u"], c["tau"], c["qty"], c["lag"], c["window"], c["tail_probs"], c["min_scen"],
                       c["is_put"], c["strike_mode"])
    r = G.restate_hedge(c["params"], c["Tq"], c["spot"], c["rate"], c["inst_u"], c["inst_tau"], c["inst_kind"], h["pnl"], h["scen_flags"], c["lag"],
                        c["window"], c["tail_probs"], c["min_scen"], c["rounds"], c["n_forced"], c["tol"], c["min_gain"], c["strike_mode"])
    got = run(c, h["pnl"], h["scen_flags"], stages=2, inst_pnl=r["inst_pnl"])
    for k in ("pick", "n_rounds", "inst_flags"):
        assert np.array_equal(got[k], r[k]), k
    same_bits(dict(r=got["pnl_hedged"][:, 8:]), dict(r=r["pnl_hedged"][:, 8:]), ("r",), "absent scenarios")


def test_explicit_stream_then_immediate_reallocation():
    import torch
    c = GC.make("stream")
    q = book_on_device(c)
    base = run(c, q["pnl"], q["scen_flags"])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    from iv_interpolation_amd import engine
    args = (dev(c["params"]), dev(c["Tq"]), dev(c["spot"]), c["rate"], dev(c["inst_u"]), dev(c["inst_tau"]), dev(c["inst_kind"], np.uint8))
    kw = dict(lag=c["lag"], window=c["window"], tail_probs=c["tail_probs"], min_scen=c["min_scen"], rounds=c["rounds"], n_forced=c["n_forced"],
              tol=c["tol"], min_gain=c["min_gain"], strike_mode=c["strike_mode"], stream=s)
    out = engine.svi_hedge(*args, q["pnl"], q["scen_flags"], **kw)
    junk = [torch.full((c["params"].shape[0], c["window"], 64), 3.0, dtype=torch.float64, device="cuda") for _ in range(4)]      # takes any block freed too early
    s.synchronize()
    torch.cuda.synchronize()
    same_bits({k: host(v) for k, v in out.items()}, base, G.OUT_KEYS, "explicit stream")
    del junk


def test_refused_calls_leave_the_device_buffers_alone():
    from iv_interpolation_amd import _lib, engine
    c, h, r = case("three_lag2")
    flat, out = guarded(shapes_of(c))
    t = dict(params=dev(c["params"]), Tq=dev(c["Tq"]), spot=dev(c["spot"]), inst_u=dev(c["inst_u"]), inst_tau=dev(c["inst_tau"]),
             inst_kind=dev(c["inst_kind"], np.uint8), pnl=dev(h["pnl"]), scen_flags=dev(h["scen_flags"], np.int32))
    lib = _lib.load()
    for over, want in ((dict(rounds=9), -34), (dict(n_forced=3), -34), (dict(tol=1.0), -34), (dict(stages=3), -34), (dict(window=1025), -34),
                       (dict(inst_kind=0), -22), (dict(pick=0), -22), (dict(inst_stride=2), -22)):
        a = _lib.HedgeArgs()
        for k, v in {**t, **out}.items():
            setattr(a, k, v.data_ptr())
        B, mT = c["params"].shape[:2]
        a.tq_stride, a.inst_stride, a.rate, a.strike_mode, a.mT, a.nH, a.B = 0, 0, c["rate"], c["strike_mode"], mT, 3, B
        tp = (ctypes.c_double * 2)(*c["tail_probs"])
        a.tail_probs, a.nL = ctypes.cast(tp, ctypes.POINTER(ctypes.c_double)), 2
        a.lag, a.window, a.min_scen, a.rounds, a.n_forced, a.tol, a.min_gain, a.stages = c["lag"], c["window"], c["min_scen"], 2, 0, 1e-6, 1e-4, 0
        for k, v in over.items():
            setattr(a, k, v)
        assert lib.ivs_svi_hedge_f64(ctypes.byref(a), None, 0, None) == want, (over, lib.ivs_last_error())
        assert lib.ivs_last_kernel() == b""
    import torch
    torch.cuda.synchronize()
    for k, v in flat.items():
        assert (host(v) == sentinel(v)).all(), k
    with pytest.raises(ValueError, match="stages = 2"):
        engine.svi_hedge(t["params"], t["Tq"], t["spot"], c["rate"], t["inst_u"], t["inst_tau"], t["inst_kind"], t["pnl"], t["scen_flags"], lag=c["lag"],
                         window=c["window"], stages=2)
    with pytest.raises(ValueError, match="mT = 0"):          # no slice: refused by the wrapper, nothing launched
        engine.svi_hedge(t["params"][:, :0], t["Tq"][:0], t["spot"], c["rate"], t["inst_u"], t["inst_tau"], t["inst_kind"], t["pnl"], t["scen_flags"],
                         lag=c["lag"], window=c["window"], out=out)
    torch.cuda.synchronize()
    for k, v in flat.items():
        assert (host(v) == sentinel(v)).all(), k


def test_builder_and_frame_on_a_wide_chain():
    """End to end: the chain of the SVI GPU test through build(), svi(), var() and hedge() on the device with the default
    instruments: the hedged row is M10 on the report's own quantities, its tail H7 on that row, no round adds variance, and with
    every round empty the hedged figures are the VarReport's bits."""
    import risk_cases as RC
    import svi_cases as SC
    import snapshot_cases as SNC
    from iv_interpolation_amd.snapshots import HipBackend, SnapshotSurfaceBuilder, hedge_frame
    b = SnapshotSurfaceBuilder(moneyness=SC.CHAIN_MONEYNESS, tenors=SC.CHAIN_TENORS, backend=HipBackend())
    res = b.build(SNC.big_chain(**SC.CHAIN))
    fits = b.svi(res, rate=SC.CHAIN_RATE)
    bk = RC.chain_book(res)
    kw = dict(rate=SC.CHAIN_RATE, window=16, tail_probs=(0.5, 0.1), min_scenarios=6)
    var = b.var(res, bk, fits, **kw)
    reps = b.hedge(res, bk, None, var, fits, rounds=2, **kw)
    assert [d.underlying for d in reps] == ["btc", "eth"]
    for rp, v in zip(reps, var):
        assert rp.labels[0] == "underlying" and rp.kind[0] == 2 and (rp.kind[1:] == 0).all() and 1 < len(rp.labels) <= 64
        pnl, fl, pick, ss = host(v.pnl), host(v.scen_flags), host(rp.pick), host(rp.ss)
        n_p, _ = H.exists(pnl.shape[0], 1, 16)
        ranked = (fl == 0) & ~np.isnan(pnl) & (np.arange(16)[None, :] < n_p[:, None])
        same_bits(dict(r=host(rp.pnl_hedged)), dict(r=m10(np.where(ranked, pnl, np.nan), host(rp.inst_pnl), pick, host(rp.hedge))), ("r",), "M10")
        vh, eh, n, worst = H.tail(host(rp.pnl_hedged), fl, (0.5, 0.1), 6)
        same_bits(dict(var_h=host(rp.var_h), es_h=host(rp.es_h), worst_h=host(rp.worst_h)), dict(var_h=vh, es_h=eh, worst_h=worst), ("var_h", "es_h", "worst_h"), "H7")
        done = host(rp.n_rounds) > 0
        assert done.any() and (ss[done, -1] < ss[done, 0]).all() and np.array_equal(np.isnan(ss[:, 0]), ~(ranked.sum(axis=1) >= 6))
    none = b.hedge(res, bk, None, var, fits, rounds=2, min_gain=0.999e9, **kw)
    for rp, v in zip(none, var):
        same_bits(dict(a=host(rp.var_h), b=host(rp.es_h), c=host(rp.worst_h)), dict(a=host(v.var), b=host(v.es), c=host(v.worst)), ("a", "b", "c"), "empty")
    f = hedge_frame(reps, res)
    assert len(f) > 0 and set(f["underlying"]) == {"btc", "eth"} and f["left"].between(0.0, 1.0).all() and set(f["round"]) <= {0, 1}
