"""CPU: delta-quoted smile points (rules D1-D7).  The restatement (tests/smile_ref.py) is anchored
against the closed form of a flat smile and checked on one hand-built micro case per rule; the host layers (builder,
frames, summary, pipeline task) run with the restatement injected as their backend; the C ABI's argument validation runs
without a device.  The kernel itself is checked in test_smiles_gpu.py."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

import smile_cases as SM
import smile_ref as R
from iv_interpolation_amd import _lib, engine, snapshots, synth
from iv_interpolation_amd.frame_store import FrameStore, synthetic_chain
from iv_interpolation_amd.snapshots import SnapshotSurfaceBuilder, smile_frame, smile_summary

M, TQ = synth.query_grids(64, 16)


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def restate(c, **kw):
    return R.restate(c["vol"], c["Kq"], c["Tq"], c["spot"], c["deltas"], c.get("rate", 0.0), **kw)


def test_restatement_matches_the_closed_form_of_a_flat_smile():
    """Flat smile -> flat chord: strike = S exp(-z sigma sqrt(tau) + (r + sigma^2 / 2) tau), vol = sigma, at the
    project's inside-hull class rtol 1e-13 / atol 1e-14."""
    worst = 0.0
    for S, sigma, rate in ((100.0, 0.5, 0.0), (27123.4, 0.31, 0.03), (0.41, 0.9, 0.0), (1800.0, 0.65, -0.01)):
        Tq = np.array([1 / 365, 7 / 365, 0.04, 0.25])
        Kq = S * np.exp(np.linspace(-1.3, 1.3, 67))
        vol = np.full((1, len(Tq), len(Kq)), sigma)
        r = R.restate(vol, Kq, Tq, [S], SM.DEFAULT, rate, monotone=True)
        assert (r["flags"] == R.OK).all()
        z = np.array([R.z_of(d) for d in SM.DEFAULT])
        exp = R.closed_form_flat(S, sigma, Tq[:, None], z[None, :], rate)[None]
        assert np.allclose(r["strike"], exp, rtol=1e-13, atol=1e-14), np.max(np.abs(r["strike"] / exp - 1))
        assert np.allclose(r["vol"], sigma, rtol=1e-13, atol=1e-14)
        worst = max(worst, float(np.max(np.abs(r["strike"] / exp - 1))))
    print(f"restatement vs closed form: max rel strike error {worst:.3e}")


@pytest.mark.parametrize("name", sorted(SM.CASES))
def test_micro_case(name):
    c = SM.CASES[name]
    r = restate(c)
    assert same(r["flags"], c["flags"]) and r["flags"].dtype == np.int32, r["flags"]
    for key, pair in c["bracket"].items():
        assert (r["ia"][key], r["ib"][key]) == pair, (key, r["ia"][key], r["ib"][key])
    hit = (c["flags"] == R.OK) | (c["flags"] == R.AMBIGUOUS)
    assert same(np.isnan(r["vol"]), ~hit) and same(np.isnan(r["strike"]), ~hit)        # D4: NaN exactly without a bracket
    for (b, j, t), (ia, ib) in c["bracket"].items():                                    # D5: the point lies on the chord
        Kq = np.broadcast_to(c["Kq"], (c["vol"].shape[0], c["vol"].shape[2]))
        assert Kq[b, ia] <= r["strike"][b, j, t] <= Kq[b, ib]
        lo, hi = sorted((c["vol"][b, j, ia], c["vol"][b, j, ib]))
        assert lo <= r["vol"][b, j, t] <= hi


def test_put_and_call_targets_of_one_delta_agree():
    r = restate(SM.CASES["put_call_mapping"])
    assert same(r["vol"][..., 0], r["vol"][..., 1]) and same(r["strike"][..., 0], r["strike"][..., 1])
    assert R.z_of(-0.25) == R.z_of(0.75) and R.z_of(0.5) == 0.0
    assert engine.delta_targets((-0.25, 0.75, 0.5)) == [R.z_of(-0.25), R.z_of(0.75), 0.0]


def test_gaps_change_the_chord_not_the_rule():
    """atm_flat and its gapped twins are flat, so they agree to rounding although their brackets differ."""
    a = restate(SM.CASES["atm_flat"])["strike"].ravel()[0]
    for n in ("gap_middle", "gap_ends", "gap_bad_strikes"):
        assert abs(restate(SM.CASES[n])["strike"].ravel()[0] / a - 1) < 1e-13
    assert abs(a / R.closed_form_flat(100.0, 0.5, 0.04, 0.0) - 1) < 1e-13


def test_shared_and_per_snapshot_grids_agree():
    shared, spelled = SM.per_snapshot_pair()
    a, b = restate(shared), restate(spelled)
    for k in ("vol", "strike", "flags"):
        assert same(a[k], b[k])
    assert (a["flags"] == R.OK).all()


def test_edge_cases_bracket_on_the_chunk_edge():
    for gap, pair in ((False, (63, 64)), (True, (61, 67))):
        c = SM.edge_63_64(gap)
        r = restate(c, monotone=True)
        assert (r["ia"][0, 0, 2], r["ib"][0, 0, 2]) == pair and (r["flags"] == R.OK).all()


def test_dense_generator_crosses_and_is_monotone():
    """What the GPU tests rely on: h is monotone inside every bracket (asserted by the restatement) and at least 90 % of
    the (row, target) pairs have a crossing."""
    for (B, mT, mK, deltas, pk, pt, holes) in ((3, 16, 65, SM.WIDE16, True, True, 0.1), (40, 16, 64, SM.DEFAULT, True, False, 0.0),
                                               (3, 1, 63, SM.WIDE16, False, True, 0.0), (1, 1, 2, (0.5,), False, False, 0.0)):
        d = SM.dense(B, mT, mK, 5, per_kq=pk, per_tq=pt, holes=holes)
        r = R.restate(d["vol"], d["Kq"], d["Tq"], d["spot"], deltas, monotone=True)
        assert (r["flags"] != R.NO_CROSSING).mean() >= 0.9 and not (r["flags"] == R.DEAD).any()


# ------------------------------------------------------------------ host layers with the restatement as the backend
def _chain():
    return synthetic_chain("btc", expiry_days=(0.5, 3), strikes=tuple(np.linspace(17000.0, 34000.0, 12)), n_hours=3, seed=5)


def _built():
    b = SnapshotSurfaceBuilder(backend=R.RefBackend(), moneyness=np.linspace(0.72, 1.28, 24), tenors=np.array([1.0, 2.0, 2.8]) / 365)
    res = b.build(_chain())
    return b, res


def test_bad_deltas_raise():
    b, res = _built()
    for bad in ((0.0,), (1.0,), (-1.0,), (1.5,), (float("nan"),), (), tuple([0.5] * 17)):
        with pytest.raises(ValueError):
            b.smiles(res, deltas=bad)
        with pytest.raises(ValueError):
            engine.delta_targets(bad)
    assert snapshots.DEFAULT_DELTAS is engine.DEFAULT_DELTAS and engine.DEFAULT_DELTAS == SM.DEFAULT


def test_smiles_frame_and_summary():
    b, res = _built()
    qs = b.smiles(res)
    assert len(qs) == len(res) == 1
    q, r = qs[0], res[0]
    assert q.underlying == "btc" and q.dates.equals(r.dates) and same(q.tenors, r.tenors) and same(q.deltas, SM.DEFAULT)
    ref = R.restate(r.out, r.Kq, r.tenors, r.spot, SM.DEFAULT)
    for k in ("vol", "strike", "flags"):
        assert same(getattr(q, k), ref[k]) and np.asarray(getattr(q, k)).shape == (len(r.dates), 3, 5)
    keep = np.flatnonzero(np.asarray(r.quotes) > 0)                           # the hourly quotes: minutes in between are empty
    assert len(keep) == 3 and (np.asarray(q.flags)[keep] == R.OK).mean() > 0.5
    assert (np.delete(np.asarray(q.flags), keep, axis=0) == R.DEAD).all()

    df = smile_frame(qs, res)
    assert list(df.columns) == ["underlying", "date", "spot", "tenor", "delta", "strike", "iv", "flags"]
    assert [str(t) for t in df.dtypes] == ["object", str(df["date"].dtype), "float64", "float64", "float64", "float64", "float64", "int32"]
    assert len(df) == len(keep) * 3 * 5
    assert same(df["iv"].to_numpy(), np.asarray(q.vol)[keep].reshape(-1))
    assert same(df["strike"].to_numpy(), np.asarray(q.strike)[keep].reshape(-1))
    assert same(df["delta"].to_numpy()[:5], SM.DEFAULT) and same(df["tenor"].to_numpy()[:15], np.repeat(r.tenors, 5))
    key = df[["underlying", "date", "tenor"]]
    assert key.equals(key.sort_values(list(key.columns), kind="stable"))
    assert sorted(df["date"].unique()) == sorted(r.dates[keep])

    s = smile_summary(qs, res)
    assert list(s.columns) == ["underlying", "date", "spot", "tenor", "atm", "rr_10", "bf_10", "rr_25", "bf_25"]
    v = np.asarray(q.vol)[keep].reshape(-1, 5)                                # columns -0.10, -0.25, 0.5, 0.25, 0.10
    assert len(s) == len(v)
    assert same(s["atm"].to_numpy(), v[:, 2])
    assert same(s["rr_25"].to_numpy(), v[:, 3] - v[:, 1]) and same(s["bf_25"].to_numpy(), 0.5 * (v[:, 3] + v[:, 1]) - v[:, 2])
    assert same(s["rr_10"].to_numpy(), v[:, 4] - v[:, 0]) and same(s["bf_10"].to_numpy(), 0.5 * (v[:, 4] + v[:, 0]) - v[:, 2])
    assert np.isfinite(s["rr_25"].to_numpy()).any()


def test_summary_nan_propagation_and_one_sided_targets():
    b, res = _built()
    qs = b.smiles(res, deltas=(-0.25, 0.5, 0.25, 0.10))
    q = qs[0]
    vol = np.array(q.vol, np.float64)
    keep = np.flatnonzero(np.asarray(res[0].quotes) > 0)
    row = keep[0]
    vol[row, 0, :] = [0.6, np.nan, 0.5, 0.4]                                  # ATM missing
    vol[row, 1, :] = [np.nan, 0.5, 0.5, 0.4]                                  # the put wing missing
    vol[row, 2, :] = [0.6, 0.5, 0.45, np.nan]                                 # only the one-sided 10d call missing
    q.vol = vol
    s = smile_summary(qs, res)
    assert list(s.columns) == ["underlying", "date", "spot", "tenor", "atm", "rr_25", "bf_25"]    # 0.10 has no put side
    first = s[s["date"] == res[0].dates[row]].sort_values("tenor")
    assert np.isnan(first["atm"].iloc[0]) and np.isnan(first["bf_25"].iloc[0]) and first["rr_25"].iloc[0] == 0.5 - 0.6
    assert np.isnan(first["rr_25"].iloc[1]) and np.isnan(first["bf_25"].iloc[1]) and first["atm"].iloc[1] == 0.5
    assert first["rr_25"].iloc[2] == 0.45 - 0.6 and first["bf_25"].iloc[2] == 0.5 * (0.45 + 0.6) - 0.5
    s2 = smile_summary(b.smiles(res, deltas=(0.25, -0.25)), res)              # no ATM asked: atm and bf are NaN, rr is not
    assert s2["atm"].isna().all() and s2["bf_25"].isna().all() and s2["rr_25"].notna().any()
    assert len(smile_frame([], [])) == 0 and len(smile_summary([], [])) == 0
    s3 = smile_summary(b.smiles(res, deltas=(-0.5, 0.5, 0.25, -0.25)), res)  # -0.5 is the ATM call delta too: no rr_50 / bf_50
    assert list(s3.columns) == ["underlying", "date", "spot", "tenor", "atm", "rr_25", "bf_25"]
    with pytest.raises(ValueError, match="target lists"):
        smile_summary(b.smiles(res) + b.smiles(res, deltas=(0.5,)), res + res)


def test_smiles_task_end_to_end(tmp_path):
    import complete_pipeline as cp
    import snapshot_ref
    from oracle_backend import OracleBackend
    store = FrameStore(str(tmp_path))
    for f in synthetic_chain("btc", expiry_days=(0.5, 3), strikes=tuple(np.linspace(17000.0, 34000.0, 6)), n_hours=12, seed=5):
        store.write_source(f["symbol"].iloc[0], f)
    assert cp.main(["--task", "interpolation", "--data-dir", str(tmp_path)], backend=OracleBackend()) == 0
    assert cp.main(["--task", "smiles", "--data-dir", str(tmp_path)], surface_backend=R.RefBackend()) == 0
    assert store.read_table("iv_surfaces", "btc") is None                      # the smiles task writes its own table only
    out = store.read_table("iv_smiles", "btc")
    assert list(out.columns) == ["underlying", "date", "spot", "tenor", "atm", "rr_10", "bf_10", "rr_25", "bf_25"]
    frames = [store.read_output(s) for s in store.symbols("interpolated_trading_tickers")]
    ref, _ = snapshot_ref.restate(frames, M, TQ)
    r = ref["btc"]
    live = np.flatnonzero(r["quotes"] > 0)
    q = R.restate(r["out"], r["Kq"], TQ, r["spot"], SM.DEFAULT)
    v = q["vol"][live].reshape(-1, 5)
    assert len(out) == len(v) == len(live) * len(TQ) and len(live) == 661
    tol = dict(rtol=1e-13, atol=1e-14, equal_nan=True)
    assert np.allclose(out["atm"].to_numpy(), v[:, 2], **tol) and np.isfinite(v[:, 2]).any()
    assert np.allclose(out["rr_25"].to_numpy(), v[:, 3] - v[:, 1], **tol)
    assert np.allclose(out["bf_10"].to_numpy(), 0.5 * (v[:, 4] + v[:, 0]) - v[:, 2], **tol)
    pipe = cp.CompleteOptimizedPipeline(cp.get_config(), data_dir=str(tmp_path), surface_backend=R.RefBackend())
    res = pipe.run_smiles()
    assert res["success"] and res["underlyings"] == 1 and res["rows"] == len(out)


# ------------------------------------------------------------------ C ABI validation, no device needed
def _args(**kw):
    P = 64
    z = (C.c_double * 16)(*([0.0] * 16))
    a = _lib.SmileArgs()
    a.vol, a.Kq, a.Tq, a.spot = (kw.get(k, P) for k in ("vol", "Kq", "Tq", "spot"))
    a.kq_stride, a.tq_stride, a.rate = kw.get("kq_stride", 0), kw.get("tq_stride", 0), 0.0
    a.z = None if kw.get("z_null") else C.cast(z, C.POINTER(C.c_double))
    a.mK, a.mT, a.nD, a.B = kw.get("mK", 64), kw.get("mT", 16), kw.get("nD", 5), kw.get("B", 1)
    a.q_vol, a.q_strike, a.q_flags = (kw.get(k, P) for k in ("q_vol", "q_strike", "q_flags"))
    a.rows_per_wave = kw.get("rows_per_wave", 0)
    a._keep = z
    return a


def test_abi_validation_codes_without_gpu():
    """Host-side validation returns errno-style codes before any launch (the fake pointers are never dereferenced)."""
    lib = _lib.load()
    assert _lib.ABI_VERSION == 5 == lib.ivs_version()
    call = lambda **kw: lib.ivs_smile_delta_points_f64(C.byref(_args(**kw)), None, 0, None)   # noqa: E731
    assert lib.ivs_smile_delta_points_f64(None, None, 0, None) == -22 and b"null args" in lib.ivs_last_error()
    for k in ("vol", "Kq", "Tq", "spot", "q_vol", "q_strike", "q_flags"):
        assert call(**{k: None}) == -22 and b"null pointer" in lib.ivs_last_error(), k
    assert call(z_null=True) == -22
    assert call(nD=0) == -34 and call(nD=17) == -34 and b"nD=17" in lib.ivs_last_error()        # IVS_ERANGE
    assert call(mK=1) == -34 and b"mK=1" in lib.ivs_last_error() and call(mK=0) == -34
    assert call(B=0) == 0 and call(mT=0) == 0 and call(B=0, vol=None) == 0                      # empty: a no-op
    assert call(B=-1) == -22 and call(mT=-1) == -22 and call(kq_stride=-1) == -22
    assert call(kq_stride=63) == -22 and call(tq_stride=15) == -22 and b"stride" in lib.ivs_last_error()
    assert call(B=1 << 27, mT=16) == -34 and b"rows" in lib.ivs_last_error()                    # B * mT = 2^31
    assert call(B=1 << 40, mT=1) == -34
    assert call(rows_per_wave=13) == -34 and b"rows_per_wave=13" in lib.ivs_last_error()       # 64 // 5 = 12 at most
    assert call(rows_per_wave=-1) == -34 and call(nD=16, rows_per_wave=5) == -34
    assert call(B=0, rows_per_wave=12) == 0 and call(B=0, nD=1, rows_per_wave=64) == 0
    assert (_lib.SM_OK, _lib.SM_NO_CROSSING, _lib.SM_AMBIGUOUS, _lib.SM_DEAD) == (R.OK, R.NO_CROSSING, R.AMBIGUOUS, R.DEAD) == (0, 1, 2, 4)
