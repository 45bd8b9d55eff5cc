"""CPU: the SVI term structure (rules T1-T4, C1-C6, E1-E6).  The restatement (tests/cal_ref.py) is
checked on one hand-built micro case per rule and flag, against the closed form of a flat surface, put-call parity, the slice
itself at lambda = 0 and the distribution restatement's CDF by a finite difference of its call price; its rounding level
against the same rules in mpmath at 50 digits is held below the recorded R_CPU the GPU tests build on; the host layers (builder,
frames, pipeline task) run with the restatement injected as their backend; header, ctypes structs and bindings are compared
field for field, and the C ABI's argument validation runs without a device.  The kernels themselves are checked in
test_svi_surface_gpu.py.

Every measuring test prints its figures; with IVS_SS_ERRLOG=<file> set they are appended to that file as well (a recorded run
belongs in profiles/svi_surface/errlog.txt)."""
import ctypes as C
import os
import re

import numpy as np
import pandas as pd
import pytest

import cal_cases as CC
import cal_ref as R
import dist_ref as DR
from iv_interpolation_amd import _lib, engine, synth
from iv_interpolation_amd.frame_store import FrameStore, synthetic_chain
from iv_interpolation_amd.snapshots import YEAR_NS, CalendarReport, PriceReport, SnapshotSurfaceBuilder, calendar_frame, price_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, TQ = synth.query_grids(64, 16)
EPS = CC.EPS


def log(name, **figures):
    line = name + ": " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items())
    print(line)
    path = os.environ.get("IVS_SS_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def cal(c, **kw):
    return R.restate_calendar(c["params"], c["Tq"], c["spot"], **kw)


def ev(c, **kw):
    return R.restate_eval(c["params"], c["Tq"], c["spot"], c["rate"], c["u"], c["tau"], c["strike_mode"], **kw)


_cache = {}


def case(n):
    """Inputs and both restatements of one generated batch, computed once and shared (read-only)."""
    if n not in _cache:
        c = CC.batch(**CC.SHAPES[n])
        _cache[n] = (c, cal(c, margins=True), ev(c, margins=True))
    return _cache[n]


# ------------------------------------------------------------------ one case per rule and flag
@pytest.mark.parametrize("name", sorted(CC.MICRO_CAL))
def test_micro_calendar(name):
    c = CC.MICRO_CAL[name]
    r = cal(c)
    assert r["flags"].dtype == np.int32 and r["n_cross"].dtype == np.int32
    state = CC.DEAD | CC.LAST | CC.UNORDERED
    assert same(r["flags"] & state, np.where(c["flags"] < 0, 0, c["flags"]) & state), r["flags"]
    if not c.get("state_only"):
        assert same(r["flags"], c["flags"]), r["flags"]
    no_pair = (r["flags"] & state) != 0
    assert same(no_pair, ~r["pair"]) and (r["n_cross"][no_pair] == 0).all()
    for k in ("d_min", "x_min", "d_atm"):
        assert same(np.isnan(r[k]), no_pair), k
    assert same(np.isnan(r["x_cross"]), np.broadcast_to((r["n_cross"] == 0)[..., None], r["x_cross"].shape))
    if "n_cross" in c:
        assert same(r["n_cross"], c["n_cross"])
    if "cells" in c:
        assert tuple(r["cells"][0, 0]) == c["cells"]
        lo, hi = r["s0"][0, 0] * R.Y[list(c["cells"])], r["s0"][0, 0] * R.Y[np.array(c["cells"]) + 1]
        assert ((lo < r["x_cross"][0, 0]) & (r["x_cross"][0, 0] < hi)).all()
    if "index" in c:
        assert r["index"][0, 0] == c["index"]
    if "d_min" in c:
        assert r["d_min"][0, 0] == pytest.approx(c["d_min"], rel=2e-3, abs=0.0)


def test_micro_calendar_values():
    """What the hand-built pairs are about, beyond their flags."""
    r = cal(CC.MICRO_CAL["below_everywhere"])
    assert (r["d66"][0, 0] < 0).all()
    r = cal(CC.MICRO_CAL["beyond_the_grid"])
    assert (r["d66"][0, 0] > 0).all() and r["d_min"][0, 0] > 0
    r = cal(CC.MICRO_CAL["two_crossings"])
    assert r["x_cross"][0, 0, 0] < 0 < r["x_cross"][0, 0, 1] and r["d_atm"][0, 0] > 0
    for x in r["x_cross"][0, 0]:                                              # the located crossings are roots of d
        p = CC.MICRO_CAL["two_crossings"]["params"][0]
        assert abs(R.curve(p[1], x)["w"] - R.curve(p[0], x)["w"]) < 1e-15
    r = cal(CC.MICRO_CAL["one_crossing"])
    assert r["x_cross"][0, 0, 0] == r["x_cross"][0, 0, 1] < 0
    r = cal(CC.MICRO_CAL["identical"])
    assert (r["d66"][0, 0] == 0).all() and r["d_min"][0, 0] == 0 and r["x_min"][0, 0] == r["s0"][0, 0] * R.Y[0]
    a, b = cal(CC.MICRO_CAL["clean"]), cal(CC.MICRO_CAL["dead_between"])
    for k in R.CAL_KEYS:                                                      # T4: the pair (0, 2) is the pair (0, 1) of the clean case
        assert same(a[k][0, 0], b[k][0, 0]), k
    r = cal(CC.MICRO_CAL["dead_causes"])
    import dist_cases as DC
    live = np.array([n in DC._LIVE for n, _, _, _ in DC.DEAD_CAUSES])
    assert same(r["pair"][:, 0], live) and same(r["live"][:, 0], live)


def test_grid():
    """C1: 64 points, exact in fp64, spacing 0.125 at the centre up to the cubic term, span +- 7.75, odd about 0."""
    from fractions import Fraction
    t = [Fraction(2 * i - 63, 2) for i in range(64)]
    assert [Fraction(float(y)) for y in R.Y] == [x * (1 + x * x / 1024) / 8 for x in t]
    assert same(R.Y, -R.Y[::-1]) and R.Y[32] - R.Y[31] == 0.125 * (1 + 1 / 4096) and round(R.Y[63], 2) == 7.75
    assert (np.diff(R.Y) > 0).all()


@pytest.mark.parametrize("name", sorted(CC.MICRO_EVAL))
def test_micro_eval(name):
    c = CC.MICRO_EVAL[name]
    r = ev(c)
    assert r["flags"].dtype == np.int32
    assert same(r["flags"], c["flags"]), r["flags"]
    off = (c["flags"] & (CC.Q_DEAD | CC.Q_UNORDERED)) != 0
    for k in ("w", "vol", "call", "put", "fwd_var", "g"):
        assert same(np.isnan(r[k]), off), k
    assert same(np.isnan(r["local_vol"]), off | ((c["flags"] & (CC.NEG_FWD | CC.NEG_G)) != 0))


def test_flat_surface():
    """b = 0, a = 0.04 tau: vol and local vol are 0.2 to rounding at every query, g is exactly 1, the forward variance 0.04,
    and call - put = D (F - K)."""
    c = CC.MICRO_EVAL["flat"]
    r = ev(c)
    tol = CC.tolerances_eval(r, CC.R_CPU)
    assert (np.abs(r["vol"] - 0.2) <= tol["vol"] + 4 * EPS).all() and (np.abs(r["local_vol"] - 0.2) <= tol["local_vol"] + 4 * EPS).all()
    assert (r["g"] == 1.0).all() and (np.abs(r["fwd_var"] - 0.04) <= tol["fwd_var"]).all()
    par = r["D"] * (r["F"] - r["K"])
    assert (np.abs(r["call"] - r["put"] - par) <= tol["call"] + tol["put"]).all()


def test_put_call_parity():
    """call - put = D (F - K) within the two prices' tolerances at the recorded rounding level, on every generated batch."""
    worst = 0.0
    for n in range(len(CC.SHAPES)):
        c, _, r = case(n)
        tol = CC.tolerances_eval(r, CC.R_CPU)
        ok = r["ok"]
        if ok.any():
            with np.errstate(invalid="ignore"):
                u = np.abs(r["call"] - r["put"] - r["D"] * (r["F"] - r["K"])) / (tol["call"] + tol["put"] + 4 * EPS * r["D"] * (r["F"] + r["K"]))
            worst = max(worst, float(np.nanmax(u[ok])))
    log("put_call_parity", worst_over_tolerance=worst)
    assert worst <= 1.0


def test_a_query_on_a_slice_is_that_slice():
    """E2 / E3: tau_q equal to a tenor gives lambda = 0 and the slice's own w, bit for bit."""
    n_on = 0
    for n in range(len(CC.SHAPES)):
        c, _, r = case(n)
        B, mT, _ = c["params"].shape
        tau = np.broadcast_to(c["Tq"], (B, mT))
        tq = np.broadcast_to(c["tau"], r["w"].shape)
        for b, q in zip(*np.nonzero(r["ok"] & (r["lo"] >= 0))):
            lo = r["lo"][b, q]
            if tau[b, lo] == tq[b, q]:
                assert r["w"][b, q] == R.curve(c["params"][b, lo], r["x"][b, q])["w"] and (r["hi"][b, q] < 0 or r["lam"][b, q] == 0.0)
                n_on += 1
    assert n_on >= 50


def test_prices_against_the_distribution_restatement():
    """At lambda = 0 a central difference of `call` in ln K reproduces dist_ref's L = 1 + dC/dK of the undiscounted call on a
    unit forward.  Step 1e-6 in x; the bound per point as in section 13: each normalised price is two terms of at most 1
    rounded to a few eps, so the quotient carries 4 eps / step, times 1 / K; the truncation is step^2 / 6 times the third
    derivative of C in x, of the order phi / s0^2 < 1e3 for s0 > 0.02."""
    step, worst, worst_abs, points = 1e-6, 0.0, 0.0, 0
    for n in (4, 7, 9):
        c, _, _ = case(n)
        B, mT, _ = c["params"].shape
        tau = np.broadcast_to(c["Tq"], (B, mT))
        live = DR.live_rows(c["params"], c["spot"][:, None], tau)
        for b in range(B):
            j = int(np.flatnonzero(live[b])[1])                              # a slice with one below and one above
            p5, S, t = c["params"][b, j], c["spot"][b], tau[b, j]
            s0 = np.sqrt(R.curve(p5, 0.0)["w"])
            assert s0 > 0.02
            x = s0 * DR.Y[28:36]                                              # +- 0.6 s0 on section 13's grid
            F = S * np.exp(c["rate"] * t)
            norm = lambda xx: (lambda r: r["call"][0] / (r["D"][0] * r["F"][0]))(  # noqa: E731
                R.restate_eval(c["params"][b:b + 1], tau[b:b + 1], c["spot"][b:b + 1], c["rate"], F * np.exp(xx), np.full(len(xx), t), 1))
            fd = 1.0 + (norm(x + step) - norm(x - step)) / (2 * step) / np.exp(x)
            L = DR.terms(p5, x)["L"]
            bound = 4 * EPS / step / np.exp(x) + step * step / 6 * 1e3 / np.exp(x)
            worst, worst_abs, points = max(worst, float(np.max(np.abs(fd - L) / bound))), max(worst_abs, float(np.max(np.abs(fd - L)))), points + len(x)
    log("finite_difference", step=step, points=points, worst_abs=worst_abs, worst_over_bound=worst)
    assert worst <= 1.0 and points >= 64


def test_strike_modes_agree():
    """K = S u as a moneyness level and as a strike: the same bits."""
    for n in (2, 8):
        c, _, r = case(n)
        assert c["strike_mode"] == 0
        k = ev(dict(c, u=c["spot"][:, None] * np.broadcast_to(c["u"], r["w"].shape), tau=np.broadcast_to(c["tau"], r["w"].shape), strike_mode=1))
        for key in R.EVAL_KEYS + ("flags",):
            assert same(r[key], k[key]), key


def test_generators_stay_inside_the_margins():
    """The conditions of the generated batches hold (asserted by the restatements with margins=True); the shapes, query counts
    and both input forms are there; the jittered tenors of mT = 64 are out of order and nothing else is; every flag of the
    evaluation occurs."""
    seen = 0
    for n, s in enumerate(CC.SHAPES):
        c, rc, re_ = case(n)
        assert (c["Tq"].ndim == 2) == s["per"] == (c["u"].ndim == 2) and c["strike_mode"] == int(s["per"]) and c["u"].shape[-1] == s["Q"]
        assert rc["unordered"].all() == (s["mT"] == 64 and s["per"]) == bool(rc["unordered"].any())
        seen |= int(np.bitwise_or.reduce(re_["flags"].ravel()))
        if s["mT"] >= 13 and not rc["unordered"].any():
            assert (rc["n_cross"] > 0).any() and ((rc["flags"] & (CC.WING_LEFT | CC.WING_RIGHT)) != 0).any()
    assert seen == CC.SHORT | CC.LONG | CC.NEG_FWD | CC.Q_DEAD | CC.Q_UNORDERED          # NEG_G is the kink's micro case
    assert {(s["B"], s["mT"]) for s in CC.SHAPES} == {(1, 1), (1, 2), (4, 3), (2, 13), (3, 16), (2, 64)}
    assert {s["Q"] for s in CC.SHAPES} == {1, 63, 64, 65, 257}


# ------------------------------------------------------------------ the rounding level the GPU tests build on
def chain_cases():
    """The end-to-end chain of the GPU test with the restatement's own SVI fit (the GPU test feeds the kernel's), every 8th
    snapshot, with the book of that test."""
    import snapshot_cases as SNC
    import svi_cases as SC
    b = SnapshotSurfaceBuilder(moneyness=SC.CHAIN_MONEYNESS, tenors=SC.CHAIN_TENORS, backend=R.RefBackend())
    res = b.build(SNC.big_chain(**SC.CHAIN))
    fits = b.svi(res, rate=SC.CHAIN_RATE)
    for r, v, p in zip(res, fits, b.price(res, CC.chain_book(res), fits, rate=SC.CHAIN_RATE)):
        yield r.underlying, dict(params=np.asarray(v.params)[::8], Tq=SC.CHAIN_TENORS, spot=np.asarray(r.spot)[::8], rate=SC.CHAIN_RATE,
                                 u=np.ascontiguousarray(np.broadcast_to(p.strikes, p.tau.shape)[::8]), tau=p.tau[::8], strike_mode=1)


def gpu_inputs():
    for name in sorted(CC.MICRO_CAL):
        yield f"micro_cal[{name}]", CC.MICRO_CAL[name]
    for name in sorted(CC.MICRO_EVAL):
        yield f"micro_eval[{name}]", CC.MICRO_EVAL[name]
    for s in CC.SHAPES:
        yield f"shape[{CC.shape_id(s)}]", CC.batch(**s)
    c = CC.batch(**CC.STREAM_SHAPE)
    yield "stream[first 2 snapshots]", {k: (v[:2] if isinstance(v, np.ndarray) and v.ndim and len(v) == 64 else v) for k, v in c.items()}
    for u, c in chain_cases():
        yield f"chain[{u}, every 8th snapshot]", c


def test_rounding_level():
    """R_CPU: |restatement - the same rules in mpmath at 50 digits| in units of eps x the rule's scale, over every input of
    the GPU tests, stays below the recorded constants."""
    import mpmath  # noqa: F401  (a missing library fails the test: R_CPU holds every GPU tolerance)
    worst = {k: 0.0 for k in CC.R_CPU}
    compared = 0
    for name, c in gpu_inputs():
        rc = cal(c)
        parts = [(CC.units(R.exact_calendar(c, rc), rc, CC.tolerances_calendar, CC.CAL_UNIT), CC.CAL_UNIT)]
        if "u" in c:
            re_ = ev(c)
            e = R.exact_eval(c, re_)
            for k in R.EVAL_KEYS:
                assert same(np.isnan(e[k]), np.isnan(re_[k])), (name, k)       # mpmath agrees on every verdict
            parts.append((CC.units(e, re_, CC.tolerances_eval, CC.EVAL_UNIT), CC.EVAL_UNIT))
        fig = {}
        for u, unit in parts:
            for k, v in u.items():
                if np.isfinite(v).any():
                    fig[k] = float(np.nanmax(v))
                    worst[unit[k]] = max(worst[unit[k]], fig[k])
                    compared += int(np.isfinite(v).sum())
        log(f"rounding[{name}]", rows=int(rc["live"].size), pairs=int(rc["pair"].sum()), **fig)
    log("rounding[all]", compared=compared, **worst)
    assert compared > 5000
    for k in worst:
        assert worst[k] <= CC.R_CPU[k], (k, worst[k])


# ------------------------------------------------------------------ host layers with the restatement as the backend
def _built():
    chain = synthetic_chain("btc", expiry_days=(0.5, 3), strikes=tuple(np.linspace(17000.0, 34000.0, 12)), n_hours=3, seed=5)
    b = SnapshotSurfaceBuilder(backend=R.RefBackend(), moneyness=np.linspace(0.72, 1.28, 24), tenors=np.array([1.0, 2.0, 2.8]) / 365)
    return b, b.build(chain)


def test_calendar_report_and_frame():
    b, res = _built()
    svi = b.svi(res, rate=0.01, rounds=6)
    reps = b.calendar(res, svi)
    assert len(reps) == 1 and isinstance(reps[0], CalendarReport)
    c, r = reps[0], res[0]
    assert c.underlying == "btc" and c.dates.equals(r.dates) and same(c.tenors, r.tenors)
    ref = R.restate_calendar(svi[0].params, r.tenors, r.spot)
    for k in R.CAL_KEYS:
        assert same(getattr(c, k), ref[k]), k
    own = b.calendar(res, rate=0.01, rounds=6)[0]                             # runs svi itself
    assert same(own.d_min, c.d_min) and same(own.flags, c.flags)
    with pytest.raises(ValueError, match="SVI reports"):
        b.calendar(res, svi_reports=[])
    keep = np.flatnonzero(np.asarray(r.quotes) > 0)
    f = calendar_frame(reps, res)
    cols = ["underlying", "date", "spot", "tenor", "next_tenor", "d_min", "x_min", "d_atm", "n_cross", "x_first", "x_last", "flags"]
    assert list(f.columns) == cols and f["flags"].dtype == np.int32 and f["n_cross"].dtype == np.int32
    s, j = np.nonzero(ref["pair"][keep])
    assert len(f) == len(s) == 2 * len(keep) and len(keep) == 3
    assert same(f["tenor"].to_numpy(), r.tenors[j]) and same(f["next_tenor"].to_numpy(), r.tenors[ref["nxt"][keep][s, j]])
    assert list(f["date"]) == list(r.dates[keep][s]) and same(f["spot"].to_numpy(), np.asarray(r.spot)[keep][s])
    for k in ("d_min", "x_min", "d_atm", "n_cross", "flags"):
        assert same(f[k].to_numpy(), ref[k][keep][s, j]), k
    assert same(f["x_first"].to_numpy(), ref["x_cross"][keep][s, j, 0]) and same(f["x_last"].to_numpy(), ref["x_cross"][keep][s, j, 1])
    assert len(calendar_frame([], [])) == 0 and list(calendar_frame([], []).columns) == cols


def test_calendar_frame_skips_dead_rows_and_unordered_snapshots():
    c = CC.MICRO_CAL["unordered"]
    r = cal(c)
    rep = CalendarReport("x", pd.DatetimeIndex(["2024-01-01", "2024-01-02", "2024-01-03"]), np.array([0.25, 0.5, 0.75]),
                         *(r[k] for k in R.CAL_KEYS))

    class Snap:
        quotes, spot = np.array([3, 3, 3], np.int32), c["spot"]
    f = calendar_frame([rep], [Snap()])
    assert len(f) == 1 and f["tenor"][0] == 0.25 and f["next_tenor"][0] == 0.5 and f["date"][0] == pd.Timestamp("2024-01-03")
    c = CC.MICRO_CAL["dead_between"]
    r = cal(c)
    rep = CalendarReport("x", pd.DatetimeIndex(["2024-01-01"]), np.array([0.25, 0.3, 0.5]), *(r[k] for k in R.CAL_KEYS))

    class One:
        quotes, spot = np.array([3], np.int32), c["spot"]
    f = calendar_frame([rep], [One()])
    assert len(f) == 1 and f["tenor"][0] == 0.25 and f["next_tenor"][0] == 0.5                # the pair skips the dead row


def test_price_report_and_frame():
    b, res = _built()
    svi = b.svi(res, rate=0.01, rounds=6)
    r = res[0]
    t0 = r.dates[0]
    book = pd.DataFrame({"strike": [20000.0, 25000.0, 30000.0, 25000.0], "expiry": [t0 + pd.Timedelta(days=d) for d in (1.5, 2.5, 5.0, -1.0)],
                         "label": list("abcd")})
    reps = b.price(res, book, svi, rate=0.01)
    assert len(reps) == 1 and isinstance(reps[0], PriceReport)
    p = reps[0]
    tau = (p.expiries.as_unit("ns").asi8[None, :] - r.dates.as_unit("ns").asi8[:, None]) / YEAR_NS
    assert same(p.tau, tau) and same(p.strikes, book["strike"]) and p.rate == 0.01 and p.tau.shape == (len(r.dates), 4)
    ref = R.restate_eval(svi[0].params, r.tenors, r.spot, 0.01, np.broadcast_to(p.strikes, tau.shape), tau, 1)
    for k in R.EVAL_KEYS + ("flags",):
        assert same(getattr(p, k), ref[k]), k
    keep = np.flatnonzero(np.asarray(r.quotes) > 0)
    assert (ref["flags"][keep, 3] == CC.Q_DEAD).all() and (ref["flags"][keep, :3] & CC.Q_DEAD == 0).all()   # the expired option
    assert (ref["flags"][keep, 2] & CC.LONG != 0).all()
    f = price_frame(reps, res)
    cols = ["underlying", "date", "spot", "strike", "expiry", "tau", "w", "vol", "call", "put", "fwd_var", "g", "local_vol", "flags"]
    assert list(f.columns) == cols and len(f) == 4 * len(keep) and f["flags"].dtype == np.int32
    assert same(f["strike"].to_numpy(), np.tile(p.strikes, len(keep))) and list(f["expiry"][:4]) == list(book["expiry"])
    assert list(f["date"][::4]) == list(r.dates[keep]) and same(f["tau"].to_numpy(), tau[keep].reshape(-1))
    for k in R.EVAL_KEYS + ("flags",):
        assert same(f[k].to_numpy(), ref[k][keep].reshape(-1)), k
    own = b.price(res, book, rate=0.01, rounds=6)[0]                          # runs svi itself
    assert same(own.call, p.call) and same(own.flags, p.flags)
    with pytest.raises(KeyError):
        b.price(res, book[["strike"]], svi)
    with pytest.raises(ValueError, match="SVI reports"):
        b.price(res, book, svi_reports=[])
    assert len(price_frame([], [])) == 0 and list(price_frame([], []).columns) == cols


def test_calendar_task_end_to_end(tmp_path):
    import complete_pipeline as cp
    import snapshot_ref
    import svi_ref
    store = FrameStore(str(tmp_path))
    for f in synthetic_chain("btc", expiry_days=(20, 45), strikes=tuple(np.linspace(17000.0, 34000.0, 6)), n_hours=3, seed=5):
        store.write_output(f["symbol"].iloc[0], f, 1)
    assert cp.main(["--task", "calendar", "--data-dir", str(tmp_path)], surface_backend=R.RefBackend()) == 0
    assert store.read_table("iv_surfaces", "btc") is None and store.read_table("iv_svi", "btc") is None
    out = store.read_table("iv_calendar", "btc")
    assert list(out.columns) == ["underlying", "date", "spot", "tenor", "next_tenor", "d_min", "x_min", "d_atm", "n_cross", "x_first", "x_last", "flags"]
    frames = [store.read_output(s) for s in store.symbols("interpolated_trading_tickers")]
    ref, _ = snapshot_ref.restate(frames, M, TQ)
    r = ref["btc"]
    live = np.flatnonzero(r["quotes"] > 0)
    v = svi_ref.restate(r["out"], r["Kq"], TQ, r["spot"], 0.0)
    d = R.restate_calendar(v["params"], TQ, r["spot"])
    s, j = np.nonzero(d["pair"][live])
    assert len(live) == 3 and len(out) == len(s) > 0
    assert np.allclose(out["d_min"].to_numpy(), d["d_min"][live][s, j], rtol=1e-9, atol=1e-15)
    assert same(out["flags"].to_numpy().astype(np.int32), d["flags"][live][s, j])
    pipe = cp.CompleteOptimizedPipeline(cp.get_config(), data_dir=str(tmp_path), surface_backend=R.RefBackend())
    res = pipe.run_calendar()
    fl = d["flags"][live][s, j]
    assert res["success"] and res["underlyings"] == 1 and res["rows"] == len(out)
    assert res["calendar_pairs"] == int(((fl & CC.CALENDAR) != 0).sum()) and res["wing_pairs"] == int(((fl & (CC.WING_LEFT | CC.WING_RIGHT)) != 0).sum())
    assert set(res) == set(pipe.run_svi()) | {"calendar_pairs", "wing_pairs"}
    assert res["fitted_rows"] == pipe.run_svi()["fitted_rows"]


# ------------------------------------------------------------------ header, structs and bindings, field for field
CTYPE = {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}


def header_fields(struct):
    src = open(os.path.join(ROOT, "include", "ivs.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.fullmatch(r"(const\s+)?(\w+)\s*(\*?)\s*(\w+)", decl)
        assert m, decl
        fields.append((m.group(4), "pointer" if m.group(3) else CTYPE[m.group(2)]))
    return src, fields


@pytest.mark.parametrize("struct,bound,fn", [("ivs_calendar_args", _lib.CalendarArgs, "ivs_svi_calendar_f64"), ("ivs_eval_args", _lib.EvalArgs, "ivs_svi_eval_f64")])
def test_header_struct_and_binding_agree(struct, bound, fn):
    src, fields = header_fields(struct)
    assert [n for n, _ in fields] == [n for n, _ in bound._fields_]
    for (name, want), (_, have) in zip(fields, bound._fields_):
        assert have is (C.c_void_p if want == "pointer" else want), name
    assert re.search(r"int\s+%s\(const %s\*[^,]*,\s*void\*[^,]*,\s*size_t[^,]*,\s*void\*[^)]*\);" % (fn, struct), src)
    res, args = _lib.SIGNATURES[fn]
    assert res is C.c_int and args == [C.POINTER(bound), C.c_void_p, C.c_size_t, C.c_void_p]


def test_header_enums_and_abi_version():
    src = open(os.path.join(ROOT, "include", "ivs.h")).read()
    sc = {k: int(v) for k, v in re.findall(r"(IVS_SC_\w+)\s*=\s*(\d+)", src)}
    se = {k: int(v) for k, v in re.findall(r"(IVS_SE_\w+)\s*=\s*(\d+)", src)}
    assert sc == {"IVS_SC_CALENDAR": 1, "IVS_SC_WING_LEFT": 2, "IVS_SC_WING_RIGHT": 4, "IVS_SC_DEAD": 8, "IVS_SC_LAST": 16, "IVS_SC_UNORDERED": 32}
    assert se == {"IVS_SE_SHORT": 1, "IVS_SE_LONG": 2, "IVS_SE_NEG_FWD": 4, "IVS_SE_DEAD": 8, "IVS_SE_NEG_G": 16, "IVS_SE_UNORDERED": 32}
    assert (_lib.SC_CALENDAR, _lib.SC_WING_LEFT, _lib.SC_WING_RIGHT, _lib.SC_DEAD, _lib.SC_LAST, _lib.SC_UNORDERED) == \
        (R.CALENDAR, R.WING_LEFT, R.WING_RIGHT, R.DEAD, R.LAST, R.UNORDERED) == (1, 2, 4, 8, 16, 32)
    assert (_lib.SE_SHORT, _lib.SE_LONG, _lib.SE_NEG_FWD, _lib.SE_DEAD, _lib.SE_NEG_G, _lib.SE_UNORDERED) == \
        (R.SHORT, R.LONG, R.NEG_FWD, R.Q_DEAD, R.NEG_G, R.Q_UNORDERED) == (1, 2, 4, 8, 16, 32)
    assert re.search(r"#define\s+IVS_ABI_VERSION\s+5\b", src) and engine.EVAL_OUTPUTS == R.EVAL_KEYS


# ------------------------------------------------------------------ C ABI validation, no device needed
def _cal_args(**kw):
    P = 64
    a = _lib.CalendarArgs()
    for k in ("params", "Tq", "spot", "d_min", "x_min", "d_atm", "x_cross", "n_cross", "flags"):
        setattr(a, k, kw.get(k, P))
    a.tq_stride, a.mT, a.B, a.rows_per_wave = kw.get("tq_stride", 0), kw.get("mT", 16), kw.get("B", 1), kw.get("rpw", 0)
    return a


def _eval_args(**kw):
    P = 64
    a = _lib.EvalArgs()
    for k in ("params", "Tq", "spot", "u", "tau", "flags") + R.EVAL_KEYS:
        setattr(a, k, kw.get(k, P))
    a.tq_stride, a.q_stride, a.rate, a.strike_mode = kw.get("tq_stride", 0), kw.get("q_stride", 0), 0.0, kw.get("strike_mode", 0)
    a.mT, a.Q, a.B = kw.get("mT", 16), kw.get("Q", 100), kw.get("B", 1)
    return a


def test_abi_validation_codes_without_gpu():
    """Host-side validation returns errno-style codes before any launch (the fake pointers are never dereferenced)."""
    lib = _lib.load()
    assert _lib.ABI_VERSION == 5 == lib.ivs_version()                                           # the symbols are additive
    cal_fn, ev_fn = lib.ivs_svi_calendar_f64, lib.ivs_svi_eval_f64
    ccall = lambda **kw: cal_fn(C.byref(_cal_args(**kw)), None, 0, None)       # noqa: E731
    ecall = lambda **kw: ev_fn(C.byref(_eval_args(**kw)), None, 0, None)       # noqa: E731
    assert cal_fn(None, None, 0, None) == -22 and b"null args" in lib.ivs_last_error()
    assert ev_fn(None, None, 0, None) == -22 and b"null args" in lib.ivs_last_error()
    for k in ("params", "Tq", "spot", "d_min", "x_min", "d_atm", "x_cross", "n_cross", "flags"):
        assert ccall(**{k: None}) == -22 and b"null pointer" in lib.ivs_last_error(), k
    for k in ("params", "Tq", "spot", "u", "tau", "flags"):
        assert ecall(**{k: None}) == -22 and b"null pointer" in lib.ivs_last_error(), k
    assert ccall(B=-1) == -22 and ccall(mT=-1) == -22 and ccall(tq_stride=-1) == -22 and b"negative" in lib.ivs_last_error()
    assert ecall(B=-1) == -22 and ecall(mT=-1) == -22 and ecall(Q=-1) == -22 and ecall(tq_stride=-1) == -22 and ecall(q_stride=-1) == -22
    for bad in (15, 17, 1, 64):
        assert ccall(tq_stride=bad) == -22 and b"stride" in lib.ivs_last_error(), bad
        assert ecall(tq_stride=bad) == -22 and b"stride" in lib.ivs_last_error(), bad
    for bad in (99, 101, 1, 16):
        assert ecall(q_stride=bad) == -22 and b"stride" in lib.ivs_last_error(), bad
    assert ccall(tq_stride=16, B=0) == 0 and ecall(tq_stride=16, q_stride=100, B=0) == 0
    for bad in (-1, 2, 7):
        assert ecall(strike_mode=bad) == -22 and b"strike_mode" in lib.ivs_last_error(), bad
    assert ecall(strike_mode=1, B=0) == 0
    assert ccall(mT=65) == -34 and b"mT=65" in lib.ivs_last_error() and ecall(mT=65) == -34 and b"mT=65" in lib.ivs_last_error()     # IVS_ERANGE
    assert ccall(mT=64, B=0) == 0 and ecall(mT=64, B=0) == 0
    assert ccall(rpw=33) == -34 and b"rows_per_wave=33" in lib.ivs_last_error() and ccall(rpw=-1) == -34 and ccall(rpw=32, B=0) == 0
    assert ccall(B=1 << 27, mT=16) == -34 and b"134217728 x 16 rows" in lib.ivs_last_error() and ccall(B=1 << 40, mT=2) == -34
    assert ecall(B=1 << 27, mT=16) == -34 and ecall(B=1 << 21, Q=1 << 10) == -34 and b"2097152 x 1024 queries" in lib.ivs_last_error()
    assert ecall(B=1 << 40, Q=2, mT=1) == -34
    for kw in (dict(B=0), dict(mT=0), dict(B=0, params=None, flags=None)):                      # a no-op
        assert ccall(**kw) == 0 and ecall(**kw) == 0 and lib.ivs_last_error() == b""
    assert ecall(Q=0) == 0 and ecall(Q=0, u=None, tau=None, flags=None) == 0
    assert C.sizeof(_lib.CalendarArgs) == 104 and C.sizeof(_lib.EvalArgs) == 152


def test_host_value_errors():
    assert engine.EVAL_OUTPUTS == ("w", "vol", "call", "put", "fwd_var", "g", "local_vol")
    for fn, args in ((engine.svi_eval, (None,) * 6),):
        with pytest.raises(ValueError, match="strike_mode"):
            fn(*args, strike_mode=2)
        with pytest.raises(ValueError, match="want"):
            fn(*args, want=("w", "delta"))


@pytest.mark.parametrize("symbol", ["ivs_svi_calendar_f64", "ivs_svi_eval_f64"])
def test_stale_library_is_reported(monkeypatch, symbol):
    """A libivs.so without the new symbols raises EngineUnavailable with a message that says to rebuild."""
    class Old:
        def __getattr__(self, name):
            if name == symbol:
                raise AttributeError(name)
            return lambda *a: _lib.ABI_VERSION
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.C, "CDLL", lambda path: Old())
    with pytest.raises(_lib.EngineUnavailable, match=symbol + ".*rebuild"):
        _lib.load()
