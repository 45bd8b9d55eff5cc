"""GPU: smile_delta_kernel (ivs_smile_delta_points_f64) against the NumPy restatement of rules D1-D6 (tests/smile_ref.py):
equal flags, equal NaN pattern, q_vol / q_strike at rtol 1e-13 / atol 1e-14 (DESIGN.md section 9 has the estimate).

Every test prints its largest error; with IVS_SMILES_ERRLOG=<file> set the figures are appended to that file as well
(a recorded run belongs in profiles/smiles/errlog.txt)."""
import os

import numpy as np
import pytest

import smile_cases as SM
import smile_ref as R
from iv_interpolation_amd import synth
from iv_interpolation_amd.frame_store import FrameStore, synthetic_chain
from iv_interpolation_amd.snapshots import HipBackend, SnapshotSurfaceBuilder, smile_summary

pytestmark = pytest.mark.gpu
M, TQ = synth.query_grids(64, 16)
RTOL, ATOL = 1e-13, 1e-14
TARGETS = {1: (0.5,), 5: SM.DEFAULT, 16: SM.WIDE16}


def log(name, **figures):
    line = name + ": " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items())
    print(line)
    path = os.environ.get("IVS_SMILES_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def host(t):
    return t.cpu().numpy()


def run(c, deltas=None, stream=None, out=None, rows_per_wave=0):
    import torch
    from iv_interpolation_amd import engine
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()    # noqa: E731
    q = engine.smile_delta_points(d(c["vol"]), d(c["Kq"]), d(c["Tq"]), d(c["spot"]), deltas or c["deltas"], c.get("rate", 0.0),
                                  stream=stream, out=out, rows_per_wave=rows_per_wave)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return {k: host(v) for k, v in q.items()}


def rel_err(a, b):
    with np.errstate(all="ignore"):
        e = np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    return float(np.nanmax(e)) if np.isfinite(e).any() else 0.0


def compare(name, got, ref):
    assert got["flags"].dtype == np.int32 and got["flags"].shape == ref["flags"].shape
    ev, ek = rel_err(got["vol"], ref["vol"]), rel_err(got["strike"], ref["strike"])
    log(name, max_rel_vol=ev, max_rel_strike=ek, elements=int(ref["flags"].size))
    assert np.array_equal(got["flags"], ref["flags"]), name
    for k in ("vol", "strike"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (name, k)
        assert np.allclose(got[k], ref[k], rtol=RTOL, atol=ATOL, equal_nan=True), (name, k, ev, ek)


@pytest.mark.parametrize("name", sorted(SM.CASES))
def test_micro_case(name):
    c = SM.CASES[name]
    got = run(c)
    assert np.array_equal(got["flags"], c["flags"]), got["flags"]
    compare(f"micro[{name}]", got, R.restate(c["vol"], c["Kq"], c["Tq"], c["spot"], c["deltas"], c["rate"]))
    if name == "put_call_mapping":
        assert np.array_equal(got["vol"][..., 0], got["vol"][..., 1]) and np.array_equal(got["strike"][..., 0], got["strike"][..., 1])


def test_shared_and_per_snapshot_grids_agree_bitwise():
    shared, spelled = SM.per_snapshot_pair()
    a, b = run(shared), run(spelled)
    for k in ("vol", "strike", "flags"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    compare("shared_vs_per_snapshot", a, R.restate(shared["vol"], shared["Kq"], shared["Tq"], shared["spot"], shared["deltas"]))


@pytest.mark.parametrize("span_gap", [False, True])
def test_bracket_on_the_chunk_edge(span_gap):
    c = SM.edge_63_64(span_gap)
    ref = R.restate(c["vol"], c["Kq"], c["Tq"], c["spot"], c["deltas"], monotone=True)
    assert (ref["ia"][0, 0, 2], ref["ib"][0, 0, 2]) == c["bracket"][(0, 0, 2)]
    compare(f"edge_63_64[gap={span_gap}]", run(c), ref)


# (B, mT, mK, nD, per-snapshot Kq, per-snapshot Tq, share of invalid nodes): every mK around the 64-node chunk, both mT,
# every B (1000 x 16 rows put several rows on one wavefront, with a ragged last one) and every nD
DENSE = [(1, 1, 2, 1, False, False, 0.0), (3, 16, 3, 5, True, False, 0.0), (3, 1, 63, 16, False, True, 0.0),
         (1, 16, 64, 5, False, False, 0.0), (3, 16, 65, 16, True, True, 0.1), (3, 16, 130, 5, True, False, 0.1),
         (1000, 16, 64, 5, True, False, 0.0), (1000, 1, 65, 16, False, True, 0.1), (1000, 16, 130, 1, True, True, 0.0),
         (1000, 16, 64, 16, True, False, 0.05)]
_dense_cache = {}


def dense_case(i):
    """Inputs and restatement of DENSE[i], computed once and shared (read-only) by the tests below."""
    if i not in _dense_cache:
        B, mT, mK, nD, pk, pt, holes = DENSE[i]
        c = SM.dense(B, mT, mK, 100 + i, per_kq=pk, per_tq=pt, holes=holes)
        c["deltas"] = TARGETS[nD]
        ref = R.restate(c["vol"], c["Kq"], c["Tq"], c["spot"], c["deltas"], monotone=True)
        for a in list(c.values()) + list(ref.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _dense_cache[i] = (c, ref)
    return _dense_cache[i]


@pytest.mark.parametrize("i", range(len(DENSE)), ids=[f"B{c[0]}-mT{c[1]}-mK{c[2]}-nD{c[3]}" for c in DENSE])
def test_dense_smiles(i):
    c, ref = dense_case(i)
    share = float((ref["flags"] != R.NO_CROSSING).mean())
    assert share >= 0.9 and not (ref["flags"] == R.DEAD).any(), share         # the comparison below is not vacuous
    got = run(c)
    compare(f"dense[{'-'.join(str(x) for x in DENSE[i])}] crossing_share={share:.3f}", got, ref)


# (dense case, rows per wavefront): the packing the launcher picks for large batches -- 64 // nD rows share a wavefront, so
# 64 / 60 / 64 lanes invert side by side for nD = 1 / 5 / 16 -- forced on small batches, with row counts that leave the last
# wavefront ragged (1, 16, 16000 rows by 64 or 12; 16000 by 3) and ones that fill it exactly; 1 = one row per wavefront
PACKED = [(0, 64), (8, 64), (8, 7), (1, 12), (3, 12), (5, 12), (6, 12), (6, 1), (6, 5), (2, 4), (4, 4), (7, 4), (9, 4), (9, 3),
          (9, 1)]


@pytest.mark.parametrize("i,rpw", PACKED, ids=[f"case{i}-rows{DENSE[i][0] * DENSE[i][1]}-nD{DENSE[i][3]}-rpw{g}" for i, g in PACKED])
def test_rows_per_wave_packing(i, rpw):
    """Every packing gives the restatement's numbers -- and the default launch's, bit for bit."""
    c, ref = dense_case(i)
    got = run(c, rows_per_wave=rpw)
    compare(f"packed[{'-'.join(str(x) for x in DENSE[i])}] rows_per_wave={rpw}", got, ref)
    base = run(c)
    for k in ("vol", "strike", "flags"):
        assert np.array_equal(got[k], base[k], equal_nan=True), k


def test_large_batch_reaches_full_packing_by_itself():
    """20 801 rows x 16 targets: above 4 x 16 x CUs rows the launcher itself packs 4 rows per wavefront (every lane inverts), and
    20 801 is not a multiple of 4, so the last wavefront is ragged."""
    c = SM.dense(20801, 1, 8, 31, per_kq=True, per_tq=False, holes=0.05)
    ref = R.restate(c["vol"], c["Kq"], c["Tq"], c["spot"], SM.WIDE16, monotone=True)
    assert float((ref["flags"] != R.NO_CROSSING).mean()) >= 0.9
    got = run(c, deltas=SM.WIDE16)
    compare("large_batch[20801-1-8-16]", got, ref)
    one = run(c, deltas=SM.WIDE16, rows_per_wave=1)
    for k in ("vol", "strike", "flags"):
        assert np.array_equal(got[k], one[k], equal_nan=True), k


def test_rows_per_wave_out_of_range():
    from iv_interpolation_amd import _lib
    c, _ = dense_case(3)
    for bad in (13, 64, -1):
        with pytest.raises(_lib.EngineError, match="rows_per_wave"):
            run(c, rows_per_wave=bad)


def test_narrow_grid_mixes_crossings_and_misses():
    """A strike grid too narrow for the wings at the long tenors: NO_CROSSING next to OK inside one batch (the NaN pattern
    and the flags carry the check; the dense cases above never miss)."""
    c = SM.dense(3, 16, 64, 77, per_kq=True, per_tq=False, width=0.15)
    ref = R.restate(c["vol"], c["Kq"], c["Tq"], c["spot"], SM.WIDE16, monotone=True)
    miss = float((ref["flags"] == R.NO_CROSSING).mean())
    assert 0.05 < miss < 0.95, miss
    compare(f"narrow_grid no_crossing_share={miss:.3f}", run(c, deltas=SM.WIDE16), ref)


@pytest.mark.parametrize("i", [3, 6])
def test_returned_points_have_the_target_delta(i):
    """engine.bs_greeks on the returned (strike, vol) gives the target call delta.  Margin: 10 x the worst error of the
    restatement's own points pushed through norm_cdf(d1) on the host -- which absorbs erfc."""
    import torch
    from iv_interpolation_amd import engine
    c, ref = dense_case(i)
    target = np.array([R.call_delta(d) for d in c["deltas"]])[None, None, :]
    own = float(np.nanmax(np.abs(R.delta_of(ref["strike"], ref["vol"], c["Tq"], c["spot"]) - target)))
    got = run(c)
    B, mT, nD = got["vol"].shape
    ok = ~np.isnan(got["vol"])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()    # noqa: E731
    S = np.broadcast_to(c["spot"][:, None, None], (B, mT, nD))[ok]
    T = np.broadcast_to(np.broadcast_to(c["Tq"], (B, mT))[:, :, None], (B, mT, nD))[ok]
    g = engine.bs_greeks(d(S), d(got["strike"][ok]), d(T), d(np.zeros(S.shape)), d(got["vol"][ok]))
    torch.cuda.synchronize()
    err = float(np.max(np.abs(host(g["delta"]) - np.broadcast_to(target, (B, mT, nD))[ok])))
    log(f"delta_consistency[{'-'.join(str(x) for x in DENSE[i])}]", restatement_own=own, margin=10 * own, device=err)
    assert ok.any() and err <= 10 * own


def test_non_default_stream_and_preallocated_outputs():
    import torch
    from iv_interpolation_amd import engine
    c, ref = dense_case(5)
    base = run(c)
    s = torch.cuda.Stream()
    B, mT, nD = ref["flags"].shape
    out = {"vol": torch.empty((B, mT, nD), dtype=torch.float64, device="cuda"),
           "strike": torch.empty((B, mT, nD), dtype=torch.float64, device="cuda"),
           "flags": torch.empty((B, mT, nD), dtype=torch.int32, device="cuda")}
    with torch.cuda.stream(torch.cuda.Stream()):                      # current stream differs from the call's stream too
        got = run(c, stream=s, out=out)
    assert engine.last_kernel() == "smile_delta_kernel"
    for k in ("vol", "strike", "flags"):
        assert np.array_equal(got[k], base[k], equal_nan=True), k
        assert np.array_equal(host(out[k]), base[k], equal_nan=True), k
    with pytest.raises(ValueError):
        engine.smile_delta_points(out["vol"], out["vol"][0, 0], out["vol"][0, :, 0], out["vol"][:, 0, 0], (1.0,))
    with pytest.raises(ValueError):
        run(c, out={"flags": out["vol"]})


def test_builder_smiles_on_a_wide_chain():
    """End to end: a chain with wide strikes and short tenors through build() and smiles(), against the restatement
    applied to the host copy of `out`."""
    import snapshot_cases as SC
    frame = SC.big_chain(n_und=2, nT=4, nK=24, minutes=40, seed=4)
    mny, ten = np.linspace(0.72, 1.28, 64), np.linspace(8.0, 20.0, 6) / 365.0
    b = SnapshotSurfaceBuilder(moneyness=mny, tenors=ten, backend=HipBackend())
    res = b.build(frame)
    qs = b.smiles(res)
    assert [q.underlying for q in qs] == ["btc", "eth"]
    for q, r in zip(qs, res):
        ref = R.restate(host(r.out), host(r.Kq), ten, host(r.spot), SM.DEFAULT)
        share = float((ref["flags"] == R.OK).mean())
        assert share >= 0.9, share
        compare(f"builder[{q.underlying}] ok_share={share:.3f}", {k: host(getattr(q, k)) for k in ("vol", "strike", "flags")}, ref)
        assert host(q.vol).shape == (40, 6, 5)


def test_smiles_task_on_gpu(tmp_path):
    import complete_pipeline as cp
    import snapshot_ref
    store = FrameStore(str(tmp_path))
    for f in synthetic_chain("btc", expiry_days=(0.5, 3, 10), strikes=tuple(np.linspace(17000.0, 34000.0, 12)), n_hours=12,
                             seed=9, missing=0.2):
        store.write_source(f["symbol"].iloc[0], f)
    assert cp.main(["--task", "interpolation", "--data-dir", str(tmp_path)]) == 0
    assert cp.main(["--task", "smiles", "--data-dir", str(tmp_path)]) == 0
    out = store.read_table("iv_smiles", "btc")
    frames = [store.read_output(s) for s in store.symbols("interpolated_trading_tickers")]
    ref, _ = snapshot_ref.restate(frames, M, TQ)
    r = ref["btc"]
    live = np.flatnonzero(r["quotes"] > 0)
    q = R.restate(r["out"], r["Kq"], TQ, r["spot"], SM.DEFAULT)
    v = q["vol"][live].reshape(-1, 5)
    assert len(out) == len(v) and len(live) == 661 and np.isfinite(v[:, 2]).mean() > 0.5
    exp = {"atm": v[:, 2], "rr_10": v[:, 4] - v[:, 0], "bf_10": 0.5 * (v[:, 4] + v[:, 0]) - v[:, 2],
           "rr_25": v[:, 3] - v[:, 1], "bf_25": 0.5 * (v[:, 3] + v[:, 1]) - v[:, 2]}
    worst = 0.0
    for k, e in exp.items():
        a = out[k].to_numpy()
        worst = max(worst, float(np.nanmax(np.abs(a - e))) if np.isfinite(e).any() else 0.0)
        assert np.array_equal(np.isnan(a), np.isnan(e)), k
        assert np.allclose(a, e, rtol=RTOL, atol=ATOL, equal_nan=True), k
    log("task_smiles", max_abs_summary_error=worst, rows=len(out))
