"""CPU: the risk-neutral distribution off raw SVI slices (rules P1-P9).  The restatement
(tests/dist_ref.py) is checked on one hand-built micro case per rule and flag, against the closed form of a flat smile,
against L + U = 1 and a finite difference of its own call price, and for ascending quantiles; its rounding level against the
same rules in mpmath at 50 digits is held below the recorded R_CPU the GPU tests build on; the host layers (builder, frame,
pipeline task) run with the restatement injected as their backend; header, ctypes struct and binding are compared field for
field, and the C ABI's argument validation runs without a device.  The kernel itself is checked in test_distribution_gpu.py.

Every measuring test prints its figures; with IVS_DS_ERRLOG=<file> set they are appended to that file as well (a recorded run
belongs in profiles/distribution/errlog.txt)."""
import ctypes as C
import os
import re
from statistics import NormalDist

import numpy as np
import pytest

import dist_cases as DC
import dist_ref as R
from iv_interpolation_amd import _lib, engine, synth
from iv_interpolation_amd.frame_store import FrameStore, synthetic_chain
from iv_interpolation_amd.snapshots import DistributionReport, SnapshotSurfaceBuilder, distribution_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, TQ = synth.query_grids(64, 16)
EPS = DC.EPS


def log(name, **figures):
    line = name + ": " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items())
    print(line)
    path = os.environ.get("IVS_DS_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def restate(c, **kw):
    return R.restate(c["params"], c["Tq"], c["spot"], c["rate"], c["probs"], c["levels"], c["max_tail"], **kw)


_cache = {}


def case(n):
    """Inputs and restatement of one generated batch, computed once and shared (read-only)."""
    if n not in _cache:
        c = DC.batch(**DC.SHAPES[n])
        _cache[n] = (c, restate(c, margins=True))
    return _cache[n]


# ------------------------------------------------------------------ one case per rule and flag
@pytest.mark.parametrize("name", sorted(DC.MICRO))
def test_micro_case(name):
    c = DC.MICRO[name]
    r = restate(c)
    assert r["flags"].dtype == np.int32 and r["q_flags"].dtype == np.int32
    assert same(r["flags"], c["flags"]), r["flags"]
    assert same(r["q_flags"], c["q_flags"]), r["q_flags"]
    dead = c["flags"] == R.DEAD
    assert same(dead, ~r["live"]) and same((c["q_flags"] == R.DEAD).all(axis=-1), dead)
    for k in ("q_x", "q_strike"):                                              # NaN exactly where no bracket was used
        assert same(np.isnan(r[k]), (c["q_flags"] & (R.DEAD | R.NO_BRACKET)) != 0), k
    assert same(np.isnan(r["tails"]).all(axis=-1), dead) and same(np.isnan(r["tails"]).any(axis=-1), dead)
    if len(c["levels"]):
        for k in ("p_below", "p_above"):
            assert same(np.isnan(r[k]), np.broadcast_to(dead[..., None], r[k].shape)), k
    else:
        assert r["p_below"] is None and r["p_above"] is None


def test_micro_case_values():
    """What the hand-built rows are about, beyond their flags."""
    r = restate(DC.MICRO["lee_bound_kink"])
    assert (np.diff(r["grid_L"][0, 0]) < 0).sum() > 20 and r["grid_L"].max() > 2.5       # the CDF overshoots and falls back
    assert (r["count"] == 1).all() and -6e-6 < r["tails"][0, 0, 1] < -5e-6 and 0 < r["tails"][0, 0, 0] < 1e-14
    r = restate(DC.MICRO["symmetric_kink"])
    assert same(r["count"][0, 0], [2, 1, 2]) and r["grid_L"].min() < -0.15 and r["grid_L"].max() > 1.15
    assert (np.abs(r["tails"]) > 1e-5).all()
    r = restate(DC.MICRO["beyond_the_grid"])
    assert r["tails"][0, 0, 0] > 1e-15 and (np.diff(r["grid_L"][0, 0, :30]) >= 0).all()   # p = 1e-15 lies below L(x_0)
    assert r["tails"][0, 1, 1] > 1e-10 and (np.diff(r["grid_L"][0, 1]) >= 0).all()         # 1 - p = 1e-10 lies below U(x_63)
    c = DC.MICRO["max_tail_zero"]
    assert (restate(c)["tails"] != 0).all()
    assert same(restate(dict(c, max_tail=1.0))["flags"], DC.MICRO["max_tail_one"]["flags"])


def test_scan_grid():
    """P4: 64 points, exact in fp64, spacing 0.125 (1 + 1/256) at the centre, span +- 64.98, odd about 0."""
    from fractions import Fraction
    j = [Fraction(2 * i - 63, 2) for i in range(64)]
    assert [Fraction(float(y)) for y in R.Y] == [x * (1 + x * x / 64) / 8 for x in j]
    assert same(R.Y, -R.Y[::-1]) and R.Y[32] - R.Y[31] == 0.125 * (1 + 1 / 256) and round(R.Y[63], 2) == 64.98
    assert (np.diff(R.Y) > 0).all()


def test_flat_smile_closed_form():
    """b = 0: x = theta inv_cdf(p) - theta^2 / 2 and K = F e^x, for every default probability; the level probabilities are
    Phi((log u - r tau) / theta + theta / 2).  The restatement may be off by its recorded rounding level; the closed form
    itself by a few eps of theta inv_cdf(p)."""
    c = DC.MICRO["flat_smile"]
    r = restate(c)
    th, inv = 0.2, NormalDist().inv_cdf
    x = np.array([th * inv(p) - th * th / 2 for p in c["probs"]])
    tol = DC.tolerances(r, c, DC.R_CPU)
    worst = float(np.max(np.abs(r["q_x"][0, 0] - x) / (tol["q_x"][0, 0] + 4 * EPS * np.abs(x) + 4 * EPS * th)))
    F = 100.0 * np.exp(0.03 * DC.TAU)
    worst_k = float(np.max(np.abs(r["q_strike"][0, 0] - F * np.exp(x)) / (tol["q_strike"][0, 0] + 8 * EPS * F * np.exp(x))))
    xl = np.log(np.array(c["levels"])) - 0.03 * DC.TAU
    below = np.array([NormalDist().cdf(v / th + th / 2) for v in xl])
    worst_l = float(np.max(np.abs(r["p_below"][0, 0] - below) / (tol["p_below"][0, 0] + 4 * EPS)))
    log("flat_smile", q_x=worst, q_strike=worst_k, p_below=worst_l)
    assert worst <= 1.0 and worst_k <= 1.0 and worst_l <= 1.0
    assert r["q_x"][0, 0, 3] == pytest.approx(-0.02, abs=1e-15)                # the median sits at -theta^2 / 2


def test_lower_and_upper_form_add_up_to_one():
    """U = 1 - L: each form is a rounding of its own terms, so the sum is 1 within the two scales."""
    worst = 0.0
    for n in range(len(DC.SHAPES)):
        c, r = case(n)
        t = R.terms(np.where(r["live"][..., None], c["params"], np.nan)[:, :, None, :], r["s0"][..., None] * R.Y)
        with np.errstate(invalid="ignore"):
            u = np.abs(t["L"] + t["U"] - 1.0) / (EPS * (t["scale_L"] + t["scale_U"]) + EPS)
        worst = max(worst, float(np.nanmax(u)))
    log("L_plus_U", worst_units=worst)
    assert worst <= DC.R_CPU["prob"]


def test_lower_form_against_a_difference_of_the_call_price():
    """L = 1 + dC/dK of the undiscounted call on a unit forward, C = Phi(d1) - e^x Phi(d2): a central difference in x at step
    1e-6, divided by K = e^x.  The bound per point: each price is two terms of at most 1 rounded to a few eps, so the
    difference quotient carries 4 eps / step, times 1 / K; its truncation is step^2 / 6 times the third derivative of C in x,
    of the order phi / s0^2 < 1e3 for s0 > 0.02 (the shortest tenor of the batches, 5 days at 40 % vol, has s0 = 0.047)."""
    step = 1e-6
    worst = worst_abs = 0.0
    for n in range(len(DC.SHAPES)):
        c, r = case(n)
        assert np.nanmin(r["s0"]) > 0.02
        P = np.where(r["live"][..., None], c["params"], np.nan)[:, :, None, :]
        x = r["s0"][..., None] * R.Y[16:48]                                   # the central half of the grid, +- 6.3 s0
        with np.errstate(invalid="ignore"):
            fd = 1.0 + (R.call_price(P, x + step) - R.call_price(P, x - step)) / (2 * step) / np.exp(x)
            err = np.abs(R.terms(P, x)["L"] - fd)
            bound = 4 * EPS / step / np.exp(x) + step * step / 6 * 1e3 / np.exp(x)
            worst, worst_abs = max(worst, float(np.nanmax(err / bound))), max(worst_abs, float(np.nanmax(err)))
    log("finite_difference", step=step, worst_abs=worst_abs, worst_over_bound=worst)
    assert worst <= 1.0


def test_quantiles_ascend_with_the_probability():
    """On rows whose CDF is monotone on the grid the quantiles are strictly ascending in p (the probability lists of the
    generated batches ascend), and every one lies inside its bracket."""
    rows = 0
    for n in range(len(DC.SHAPES)):
        c, r = case(n)
        mono = r["live"] & (np.diff(r["grid_L"], axis=-1) >= 0).all(axis=-1)
        assert same(mono, r["live"])                                          # every generated live row is monotone
        assert (r["count"][r["live"]] == 1).all()
        rows += int(mono.sum())
        if len(c["probs"]) > 1:
            assert (np.diff(r["q_x"][mono], axis=-1) > 0).all() and (np.diff(r["q_strike"][mono], axis=-1) > 0).all()
        i = r["bracket"][mono]
        lo, hi = r["s0"][mono][:, None] * R.Y[i], r["s0"][mono][:, None] * R.Y[i + 1]
        assert ((lo <= r["q_x"][mono]) & (r["q_x"][mono] <= hi)).all()
    assert rows >= 150


def test_generators_stay_inside_the_margins():
    """The conditions of the generated batches hold (asserted by the restatement with margins=True), DEAD rows occur in every
    batch of ten rows or more, both tenor forms are there, and the shapes are the ones the packing can go wrong at."""
    for n, s in enumerate(DC.SHAPES):
        c, r = case(n)
        assert (c["Tq"].ndim == 2) == s["per_tq"] and len(c["probs"]) == s["nP"] and len(c["levels"]) == s["nL"]
        assert ((~r["live"]).sum() > 0) == (s["B"] * s["mT"] >= 10)
    assert {(s["B"], s["mT"], s["nP"]) for s in DC.SHAPES} == {(1, 1, 1), (3, 2, 5), (4, 3, 5), (2, 13, 5), (5, 3, 16), (3, 16, 7), (64, 1, 1)}
    assert {s["nL"] for s in DC.SHAPES} == {0, 5, 16}
    for nP in (1, 5, 7, 16):
        p = DC.probs_for(nP)
        assert len(p) == nP and all(0.0 < q < 1.0 for q in p) and list(p) == sorted(p)
    assert min(DC.probs_for(16)) == 1e-6 and max(DC.probs_for(16)) == 1.0 - 1e-6


# ------------------------------------------------------------------ the rounding level the GPU tests build on
def chain_case():
    """The end-to-end chain of the GPU test with the restatement's own SVI fit (the GPU test feeds the kernel's)."""
    import snapshot_cases as SNC
    import svi_cases as SC
    b = SnapshotSurfaceBuilder(moneyness=SC.CHAIN_MONEYNESS, tenors=SC.CHAIN_TENORS, backend=R.RefBackend())
    res = b.build(SNC.big_chain(**SC.CHAIN))
    for r, v in zip(res, b.svi(res, rate=SC.CHAIN_RATE)):
        yield r.underlying, dict(params=np.asarray(v.params)[::8], Tq=SC.CHAIN_TENORS, spot=np.asarray(r.spot)[::8], rate=SC.CHAIN_RATE,
                                 probs=DC.DEFAULT_PROBS, levels=DC.DEFAULT_LEVELS, max_tail=1e-6)


def gpu_inputs():
    for name in sorted(DC.MICRO):
        yield f"micro[{name}]", DC.MICRO[name]
    for s in DC.SHAPES:
        yield f"shape[{DC.shape_id(s)}]", DC.batch(**s)
    c = DC.batch(**DC.STREAM_SHAPE)
    yield "stream[first 4 snapshots]", dict(c, params=c["params"][:4], Tq=c["Tq"][:4], spot=c["spot"][:4])
    for u, c in chain_case():
        yield f"chain[{u}, every 8th snapshot]", c


def test_rounding_level():
    """R_CPU: |restatement - the same rules in mpmath at 50 digits| in units of eps x the rule's scale, over every input of
    the GPU tests, stays below the recorded constants."""
    import mpmath  # noqa: F401  (a missing library fails the test: R_CPU holds every GPU tolerance)
    worst = {k: 0.0 for k in DC.R_CPU}
    compared = 0
    for name, c in gpu_inputs():
        r = restate(c)
        e = R.exact(c, r)
        u = DC.units(r, {**r, **e}, c)
        for k, v in u.items():
            assert same(np.isnan(e[k]), np.isnan(np.asarray(r[k], np.float64))), (name, k)   # mpmath agrees on every bracket
            if np.isfinite(v).any():
                worst[DC.UNIT_KEY[k]] = max(worst[DC.UNIT_KEY[k]], float(np.nanmax(v)))
                compared += int(np.isfinite(v).sum())
        log(f"rounding[{name}]", rows=int(r["live"].size), live=int(r["live"].sum()),
            **{k: (float(np.nanmax(v)) if np.isfinite(v).any() else 0.0) for k, v in u.items()})
    log("rounding[all]", compared=compared, **worst)
    assert compared > 5000
    for k in worst:
        assert worst[k] <= DC.R_CPU[k], (k, worst[k])


# ------------------------------------------------------------------ host layers with the restatement as the backend
def _built():
    chain = synthetic_chain("btc", expiry_days=(0.5, 3), strikes=tuple(np.linspace(17000.0, 34000.0, 12)), n_hours=3, seed=5)
    b = SnapshotSurfaceBuilder(backend=R.RefBackend(), moneyness=np.linspace(0.72, 1.28, 24), tenors=np.array([1.0, 2.0, 2.8]) / 365)
    return b, b.build(chain)


def test_host_value_errors():
    b, res = _built()
    for bad in ((), (0.0,), (1.0,), (0.5, -0.1), (0.5, float("nan")), tuple([0.5] * 17)):
        with pytest.raises(ValueError):
            b.distribution(res, probs=bad)
        with pytest.raises(ValueError):
            engine.distribution_targets(bad, DC.DEFAULT_LEVELS)
    for bad in ((0.0,), (-1.0,), (float("inf"),), (float("nan"),), tuple([1.0] * 17)):
        with pytest.raises(ValueError):
            b.distribution(res, levels=bad)
        with pytest.raises(ValueError):
            engine.distribution_targets(DC.DEFAULT_PROBS, bad)
    for bad in (-1e-9, 1.5, float("nan")):
        with pytest.raises(ValueError, match="max_tail"):
            b.distribution(res, max_tail=bad)
    with pytest.raises(ValueError, match="SVI reports"):
        b.distribution(res, svi_reports=[])
    assert engine.distribution_targets((0.5,), ()) == ([0.5], [])
    assert engine.DEFAULT_PROBS == DC.DEFAULT_PROBS == R.DEFAULT_PROBS and engine.DEFAULT_LEVELS == DC.DEFAULT_LEVELS == R.DEFAULT_LEVELS


def test_distribution_report_and_frame():
    b, res = _built()
    svi = b.svi(res, rate=0.01, rounds=6)
    reps = b.distribution(res, svi, rate=0.01, probs=(0.95, 0.05, 0.5), levels=(1.1, 0.9), max_tail=1e-9)
    assert len(reps) == len(res) == 1 and isinstance(reps[0], DistributionReport)
    d, r = reps[0], res[0]
    assert d.underlying == "btc" and d.dates.equals(r.dates) and same(d.tenors, r.tenors)
    assert d.rate == 0.01 and d.max_tail == 1e-9 and same(d.probs, [0.95, 0.05, 0.5]) and same(d.levels, [1.1, 0.9])
    ref = R.restate(svi[0].params, r.tenors, r.spot, 0.01, (0.95, 0.05, 0.5), (1.1, 0.9), 1e-9)
    for k in ("q_x", "q_strike", "q_flags", "p_below", "p_above", "tails", "flags"):
        assert same(getattr(d, k), ref[k]), k
    own = b.distribution(res, rate=0.01, rounds=6, probs=(0.95, 0.05, 0.5), levels=(1.1, 0.9), max_tail=1e-9)[0]   # runs svi itself
    assert same(own.q_x, d.q_x) and same(own.flags, d.flags)
    dflt = b.distribution(res)[0]
    assert same(dflt.probs, DC.DEFAULT_PROBS) and same(dflt.levels, DC.DEFAULT_LEVELS) and dflt.max_tail == 1e-6
    none = b.distribution(res, levels=())[0]
    assert none.p_below is None and none.p_above is None and len(none.levels) == 0
    keep = np.flatnonzero(np.asarray(r.quotes) > 0)
    assert len(keep) == 3 and ref["live"][keep].all() and not np.delete(ref["live"], keep, axis=0).any()

    f = distribution_frame(reps, res)
    cols = ["underlying", "date", "spot", "tenor", "forward", "q_95", "q_5", "q_50", "below_110", "below_90", "tail_lo", "tail_hi", "flags"]
    assert list(f.columns) == cols
    assert [str(t) for t in f.dtypes] == ["object", str(f["date"].dtype)] + ["float64"] * 10 + ["int32"]
    assert len(f) == len(keep) * 3 and list(f["date"][::3]) == list(r.dates[keep]) and same(f["tenor"].to_numpy(), np.tile(r.tenors, 3))
    spot = np.repeat(np.asarray(r.spot)[keep], 3)
    assert same(f["spot"].to_numpy(), spot) and same(f["forward"].to_numpy(), spot * np.exp(0.01 * np.tile(r.tenors, 3)))
    for t, k in enumerate(("q_95", "q_5", "q_50")):
        assert same(f[k].to_numpy(), ref["q_strike"][keep, :, t].reshape(-1)), k
    for t, k in enumerate(("below_110", "below_90")):
        assert same(f[k].to_numpy(), ref["p_below"][keep, :, t].reshape(-1)), k
    assert same(f["tail_lo"].to_numpy(), ref["tails"][keep, :, 0].reshape(-1)) and same(f["tail_hi"].to_numpy(), ref["tails"][keep, :, 1].reshape(-1))
    assert same(f["flags"].to_numpy(), (ref["flags"][keep] | np.bitwise_or.reduce(ref["q_flags"][keep], axis=-1)).reshape(-1))
    assert (f["q_5"] < f["q_50"]).all() and (f["q_50"] < f["q_95"]).all() and (f["below_90"] < f["below_110"]).all()
    f0 = distribution_frame(b.distribution(res, levels=()), res)
    assert list(f0.columns) == ["underlying", "date", "spot", "tenor", "forward"] + [f"q_{p}" for p in (1, 5, 25, 50, 75, 95, 99)] + \
        ["tail_lo", "tail_hi", "flags"]
    assert len(distribution_frame([], [])) == 0
    assert list(distribution_frame([], []).columns) == ["underlying", "date", "spot", "tenor", "forward", "tail_lo", "tail_hi", "flags"]
    with pytest.raises(ValueError, match="different"):
        distribution_frame([reps[0], dflt], [r, r])
    for kw in (dict(probs=(0.5, 0.5)), dict(levels=(0.9, 0.9)), dict(probs=(0.25, 0.25 + 1e-12))):   # one label for two columns
        with pytest.raises(ValueError, match="share a column name"):
            distribution_frame(b.distribution(res, svi, **kw), res)


def test_frame_flags_or_the_target_flags():
    """P9: `flags` is the row flag OR-ed with the OR of its target flags."""
    import pandas as pd
    c = DC.MICRO["symmetric_kink"]
    r = restate(c)
    rep = DistributionReport("x", pd.DatetimeIndex(["2024-01-01"]), c["Tq"], np.asarray(c["probs"]), np.asarray(c["levels"]), 0.0, 1e-6,
                             r["q_x"], r["q_strike"], r["q_flags"], r["p_below"], r["p_above"], r["tails"], r["flags"])

    class Snap:
        quotes, spot = np.array([3], np.int32), c["spot"]
    f = distribution_frame([rep], [Snap()])
    assert list(f["flags"]) == [R.TAILS | R.AMBIGUOUS] and f["flags"].dtype == np.int32


def test_distribution_task_end_to_end(tmp_path):
    import complete_pipeline as cp
    import snapshot_ref
    import svi_ref
    store = FrameStore(str(tmp_path))
    # three hourly quotes per contract stand in for the interpolation task's output: 121 minute snapshots, 3 with quotes
    for f in synthetic_chain("btc", expiry_days=(20, 45), strikes=tuple(np.linspace(17000.0, 34000.0, 6)), n_hours=3, seed=5):
        store.write_output(f["symbol"].iloc[0], f, 1)
    assert cp.main(["--task", "distribution", "--data-dir", str(tmp_path)], surface_backend=R.RefBackend()) == 0
    assert store.read_table("iv_surfaces", "btc") is None and store.read_table("iv_svi", "btc") is None
    out = store.read_table("iv_distribution", "btc")
    assert list(out.columns) == ["underlying", "date", "spot", "tenor", "forward"] + [f"q_{p}" for p in (1, 5, 25, 50, 75, 95, 99)] + \
        [f"below_{u}" for u in (80, 90, 100, 110, 120)] + ["tail_lo", "tail_hi", "flags"]
    frames = [store.read_output(s) for s in store.symbols("interpolated_trading_tickers")]
    ref, _ = snapshot_ref.restate(frames, M, TQ)
    r = ref["btc"]
    live = np.flatnonzero(r["quotes"] > 0)
    v = svi_ref.restate(r["out"], r["Kq"], TQ, r["spot"], 0.0)
    d = R.restate(v["params"], TQ, r["spot"], 0.0)
    assert len(live) == 3 and len(out) == len(live) * len(TQ)
    assert np.allclose(out["q_50"].to_numpy(), d["q_strike"][live, :, 3].reshape(-1), rtol=1e-12, equal_nan=True)
    assert np.allclose(out["below_90"].to_numpy(), d["p_below"][live, :, 1].reshape(-1), rtol=1e-9, atol=1e-15, equal_nan=True)
    fl = (d["flags"][live] | np.bitwise_or.reduce(d["q_flags"][live], axis=-1)).reshape(-1)
    assert same(out["flags"].to_numpy().astype(np.int32), fl)
    pipe = cp.CompleteOptimizedPipeline(cp.get_config(), data_dir=str(tmp_path), surface_backend=R.RefBackend())
    res = pipe.run_distribution()
    assert res["success"] and res["underlyings"] == 1 and res["rows"] == len(out)
    assert res["live_rows"] == int((fl & R.DEAD == 0).sum()) and res["ambiguous_rows"] == int(((fl & R.AMBIGUOUS) != 0).sum())
    assert set(res) == set(pipe.run_smiles()) | {"live_rows", "ambiguous_rows"}


# ------------------------------------------------------------------ header, struct and binding, field for field
CTYPE = {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}


def header_fields():
    src = open(os.path.join(ROOT, "include", "ivs.h")).read()
    body = re.search(r"typedef struct ivs_distribution_args \{(.*?)\} ivs_distribution_args;", src, flags=re.S).group(1)
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


def test_header_struct_and_binding_agree():
    src, fields = header_fields()
    bound = _lib.DistributionArgs._fields_
    assert [n for n, _ in fields] == [n for n, _ in bound]
    for (name, want), (_, have) in zip(fields, bound):
        if want == "pointer":
            assert have in (C.c_void_p, C.POINTER(C.c_double)), name
            assert (have is not C.c_void_p) == (name in ("probs", "levels")), name           # the host arrays are typed
        else:
            assert have is want, name
    assert [n for n, _ in fields] == ["params", "Tq", "tq_stride", "spot", "rate", "max_tail", "probs", "nP", "levels", "nL", "mT", "B",
                                      "q_x", "q_strike", "q_flags", "p_below", "p_above", "tails", "flags", "rows_per_wave"]
    assert re.search(r"int\s+ivs_svi_distribution_f64\(const ivs_distribution_args\*[^,]*,\s*void\*[^,]*,\s*size_t[^,]*,\s*void\*[^)]*\);", src)
    res, args = _lib.SIGNATURES["ivs_svi_distribution_f64"]
    assert res is C.c_int and args == [C.POINTER(_lib.DistributionArgs), C.c_void_p, C.c_size_t, C.c_void_p]
    enum = dict(re.findall(r"(IVS_DS_\w+)\s*=\s*(\d+)", src))
    assert {k: int(v) for k, v in enum.items()} == {"IVS_DS_NO_BRACKET": 1, "IVS_DS_AMBIGUOUS": 2, "IVS_DS_TAILS": 4, "IVS_DS_DEAD": 8}
    assert (_lib.DS_NO_BRACKET, _lib.DS_AMBIGUOUS, _lib.DS_TAILS, _lib.DS_DEAD) == (R.NO_BRACKET, R.AMBIGUOUS, R.TAILS, R.DEAD) == (1, 2, 4, 8)
    assert re.search(r"#define\s+IVS_ABI_VERSION\s+5\b", src) and "ivs_svi_distribution_f64 call on this thread" in src


# ------------------------------------------------------------------ C ABI validation, no device needed
def _args(**kw):
    P = 64
    a = _lib.DistributionArgs()
    a.params, a.Tq, a.spot = (kw.get(k, P) for k in ("params", "Tq", "spot"))
    a.tq_stride, a.rate, a.max_tail = kw.get("tq_stride", 0), 0.0, kw.get("max_tail", 1e-6)
    probs, levels = kw.get("probs", DC.DEFAULT_PROBS), kw.get("levels", DC.DEFAULT_LEVELS)
    a.nP, a.nL = kw.get("nP", 0 if probs is None else len(probs)), kw.get("nL", 0 if levels is None else len(levels))
    keep = []
    for name, v in (("probs", probs), ("levels", levels)):
        if v is not None:
            buf = (C.c_double * max(len(v), 1))(*v)
            keep.append(buf)
            setattr(a, name, C.cast(buf, C.POINTER(C.c_double)))
    a.mT, a.B = kw.get("mT", 16), kw.get("B", 1)
    a.q_x, a.q_strike, a.q_flags, a.p_below, a.p_above, a.tails, a.flags = (
        kw.get(k, P) for k in ("q_x", "q_strike", "q_flags", "p_below", "p_above", "tails", "flags"))
    a.rows_per_wave = kw.get("rpw", 0)
    a._keep = keep
    return a


def test_abi_validation_codes_without_gpu():
    """Host-side validation returns errno-style codes before any launch (the fake pointers are never dereferenced)."""
    lib = _lib.load()
    assert _lib.ABI_VERSION == 5 == lib.ivs_version()                                           # the symbol is additive
    assert hasattr(lib, "ivs_svi_distribution_f64")
    fn = lib.ivs_svi_distribution_f64

    def call(**kw):
        a = _args(**kw)
        return fn(C.byref(a), None, 0, None)
    assert fn(None, None, 0, None) == -22 and b"null args" in lib.ivs_last_error()
    for k in ("params", "Tq", "spot", "q_x", "q_strike", "q_flags", "tails", "flags", "p_below", "p_above"):
        assert call(**{k: None}) == -22 and b"null p" in lib.ivs_last_error(), k
    assert call(probs=None, nP=7) == -22 and b"null probs" in lib.ivs_last_error()
    assert call(levels=None, nL=5) == -22 and b"null levels" in lib.ivs_last_error()
    assert call(B=-1) == -22 and call(mT=-1) == -22 and call(tq_stride=-1) == -22 and b"negative" in lib.ivs_last_error()
    for bad in (15, 17, 1, 64):
        assert call(tq_stride=bad) == -22 and b"stride" in lib.ivs_last_error(), bad
    assert call(tq_stride=16, B=0) == 0
    for bad in (0.0, 1.0, -0.5, 1.5, float("nan"), float("inf")):
        assert call(probs=(0.5, bad)) == -22 and b"probability 1" in lib.ivs_last_error(), bad
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(levels=(1.0, 1.1, bad)) == -22 and b"level 2" in lib.ivs_last_error(), bad
    for bad in (-1e-9, 1.0000001, float("nan")):
        assert call(max_tail=bad) == -22 and b"max_tail" in lib.ivs_last_error(), bad
    assert call(max_tail=0.0, B=0) == 0 and call(max_tail=1.0, B=0) == 0
    assert call(probs=(), nP=0) == -34 and b"nP=0" in lib.ivs_last_error() and call(probs=(0.5,) * 17) == -34      # IVS_ERANGE
    assert call(levels=(1.0,) * 17) == -34 and b"nL=17" in lib.ivs_last_error() and call(nL=-1) == -34
    assert call(rpw=10) == -34 and b"rows_per_wave=10" in lib.ivs_last_error() and call(rpw=-1) == -34           # 64 // 7 = 9
    assert call(rpw=9, B=0) == 0 and call(probs=(0.5,), rpw=64, B=0) == 0 and call(probs=(0.5,), rpw=65) == -34
    assert call(probs=(0.5,) * 16, rpw=4, B=0) == 0 and call(probs=(0.5,) * 16, rpw=5) == -34
    assert call(B=1 << 27, mT=16) == -34 and b"134217728 x 16 rows" in lib.ivs_last_error()     # B * mT = 2^31
    assert call(B=1 << 40, mT=2) == -34
    assert call(B=0) == 0 and call(mT=0) == 0 and call(B=0, params=None, flags=None) == 0 and lib.ivs_last_error() == b""   # a no-op
    assert call(levels=(), p_below=None, p_above=None, B=0) == 0
    assert call(B=0, probs=(2.0,)) == -22                                                       # the targets are checked first
    assert C.sizeof(_lib.DistributionArgs) == 152


def test_stale_library_is_reported(monkeypatch):
    """A libivs.so without the new symbol raises EngineUnavailable with a message that says to rebuild."""
    class Old:
        def __getattr__(self, name):
            if name == "ivs_svi_distribution_f64":
                raise AttributeError(name)
            return lambda *a: _lib.ABI_VERSION
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.C, "CDLL", lambda path: Old())
    with pytest.raises(_lib.EngineUnavailable, match="ivs_svi_distribution_f64.*rebuild"):
        _lib.load()
