"""CPU: rules H0-H9 on the restatement tests/hsim_ref.py: the micro tables worked out by hand, the checks
of meaning against independent formulas, the restatement's rounding level against the same rules in mpmath (R_CPU), the
conditions of the generated batches, and the host layers (builder, frame, pipeline task, argument checks, C refusals) with the
restatement as the backend.

With IVS_HSIM_ERRLOG=<file> set the measured figures are appended to that file (a recorded run belongs in
profiles/hsim/errlog.txt)."""
import os

import numpy as np
import pandas as pd
import pytest

import cal_ref as CR
import hsim_cases as HC
import hsim_ref as H
import risk_ref as R
from iv_interpolation_amd.frame_store import FrameStore, synthetic_chain
from iv_interpolation_amd.snapshots import SnapshotSurfaceBuilder, VarReport, var_frame, var_level_columns

EPS = HC.EPS


def log(name, **figures):
    line = name + ": " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items())
    print(line)
    path = os.environ.get("IVS_HSIM_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def hsim(c, **kw):
    return H.restate_hsim(c["params"], c["Tq"], c["spot"], c["rate"], c["u"], c["tau"], c["qty"], c["lag"], c["window"], c["tail_probs"],
                          c["min_scen"], c["is_put"], c["strike_mode"], **kw)


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def plus_zero(a):
    a = np.asarray(a)
    return bool((a == 0.0).all() and not np.signbit(a).any())


# ------------------------------------------------------------------ micro tables
@pytest.mark.parametrize("name", sorted(HC.MICRO))
def test_micro(name):
    c = HC.MICRO[name]
    r = hsim(c)
    assert same(r["scen_flags"], c["scen_flags"]) and same(r["n_valid"], c["n_valid"]) and same(r["n_dead"], c["n_dead"])
    assert same(np.isnan(r["pnl"]), c["scen_flags"] != 0)                     # H5: a flag, and only a flag, gives NaN
    n_p, ex = H.exists(len(c["spot"]), c["lag"], c["window"])
    assert same(c["scen_flags"] == HC.ABSENT, ~ex)                            # H0
    few = c["n_valid"] < c["min_scen"]
    assert np.isnan(r["var"][few]).all() and np.isnan(r["es"][few]).all() and np.isfinite(r["var"][~few]).all()
    assert same(r["worst"] < 0, c["n_valid"] == 0)
    deg = c["n_dead"] == len(c["qty"])
    today_ok = ~deg & (np.arange(len(deg)) > 0 if name == "neg_hist_w" else True)   # that case's snapshot 0 has W < 0 today as well
    assert np.isnan(r["value"][deg]).all() and np.isfinite(r["value"][today_ok]).all()


def test_h6_identical_ends_give_plus_zero():
    r = hsim(HC.MICRO["same_pair"])
    assert plus_zero(r["pnl"][1, 0]) and plus_zero(r["pnl"][2, 1]) and r["pnl"][2, 0] != 0.0
    assert plus_zero(r["var"][1]) and plus_zero(r["es"][1])                   # H7: a zero is +0.0
    c = HC.make(3)                                                           # a generated batch with one pair duplicated
    twin = dict(c, params=c["params"].copy(), spot=c["spot"].copy(), Tq=c["Tq"].copy())
    twin["params"][4], twin["spot"][4], twin["Tq"][4] = twin["params"][3], twin["spot"][3], twin["Tq"][3]
    r = hsim(twin)
    for p in range(4, 9):
        assert plus_zero(r["pnl"][p, p - 4]), p                              # the pair (3, 4) is scenario s = p - 4 of snapshot p
    assert (r["pnl"][5:, 0] != 0.0).all()


@pytest.mark.parametrize("name", sorted(HC.ROWS))
def test_h7_rows(name):
    """m at n tp just under and just over an integer, ties with -0.0 against +0.0, flagged scenarios, n < min_scen."""
    pnl, fl, tp, min_scen, var, es, n_valid, worst = HC.ROWS[name]
    g = H.tail(np.array([pnl]), np.array([fl]), tp, min_scen)
    assert same(g[0][0], var) and same(g[1][0], es) and g[2][0] == n_valid and g[3][0] == worst
    assert same(np.signbit(g[0][0]), np.signbit(np.asarray(var))) and same(np.signbit(g[1][0]), np.signbit(np.asarray(es)))


def test_window_and_lag():
    """H0 and H4: a scenario's bits depend on p, the pair and the book alone: not on the window, the batch or the lag's route."""
    c = HC.make(3)                                                           # B = 9, lag 1, window 63
    full = hsim(c)
    for w in (1, 4, 8, 9):
        r = hsim(dict(c, window=w))
        assert same(r["pnl"], full["pnl"][:, :w]) and same(r["scen_flags"], full["scen_flags"][:, :w])
    assert (full["scen_flags"][:, 8:] == HC.ABSENT).all() and same(full["n_valid"], np.arange(9))
    two = hsim(dict(c, lag=2))
    rows = [3, 5, 8]                                                         # start, end, today: scenario (3, 5) of snapshot 8 is s = 3 at lag 2
    pick = lambda a: a[rows] if a.ndim == 2 and a.shape[0] == 9 else a        # noqa: E731
    alone = hsim(dict(c, lag=1, window=2, params=c["params"][rows], spot=c["spot"][rows], Tq=pick(c["Tq"]), u=pick(c["u"]), tau=pick(c["tau"])))
    assert same(alone["pnl"][2, 1], two["pnl"][8, 3]) and same(alone["value"][2], two["value"][8])


# ------------------------------------------------------------------ checks of meaning
def _bs(S, K, D, sig, tau, put):
    d1 = (np.log(S / (K * D)) + 0.5 * sig * sig * tau) / (sig * np.sqrt(tau))
    d2 = d1 - sig * np.sqrt(tau)
    return K * D * CR.Phi(-d2) - S * CR.Phi(-d1) if put else S * CR.Phi(d1) - K * D * CR.Phi(d2)


def test_a_scenario_against_the_surface_evaluation_rerun_at_the_moved_spot():
    """pnl[p][s] from cal_ref.restate_eval (the section 14 restatement, another code path) run on the three snapshots' slices at
    the spot S', and the textbook Black-Scholes formula at sigma'."""
    c = HC.make(3)
    r = hsim(c)
    worst = 0.0
    for p, s in ((8, 0), (8, 7), (5, 2), (1, 0)):
        ja, jb = p - 1 - s, p - s
        S1 = c["spot"][p] * (c["spot"][jb] / c["spot"][ja])
        K, tau = c["u"][p], c["tau"][p]
        vol = lambda b, S: CR.restate_eval(c["params"][b:b + 1], c["Tq"][b:b + 1], np.array([S]), c["rate"], K[None], tau[None], 1)["vol"][0]  # noqa: E731
        sg = vol(p, S1) + (vol(jb, S1) - vol(ja, S1))
        sg0 = vol(p, c["spot"][p])
        lv = r["live"][p]
        D = np.exp(-c["rate"] * tau)
        with np.errstate(all="ignore"):
            put = c["is_put"].astype(bool)
            new = np.where(put, _bs(S1, K, D, sg, tau, True), _bs(S1, K, D, sg, tau, False))
            old = np.where(put, _bs(c["spot"][p], K, D, sg0, tau, True), _bs(c["spot"][p], K, D, sg0, tau, False))
        total = float(np.sum(np.where(lv, c["qty"] * (new - old), 0.0)))
        # the textbook d1 is rounded differently from G1's -x/theta + theta/2: allow 64 units of the restatement's own scale
        err = abs(total - r["pnl"][p, s]) / (EPS * r["scale_pnl"][p, s])
        worst = max(worst, err)
        assert err <= 64.0, (p, s, total, r["pnl"][p, s])
    log("meaning[eval+bs]", units=worst)


def _spot_only(c):
    """The batch `c` with the slices, tenors and expiries of snapshot 0 throughout: only the spot moves."""
    B = len(c["spot"])
    return dict(c, params=np.repeat(c["params"][:1], B, axis=0), Tq=c["Tq"][0] if np.ndim(c["Tq"]) == 2 else c["Tq"],
                u=c["u"][0] if np.ndim(c["u"]) == 2 else c["u"], tau=c["tau"][0] if np.ndim(c["tau"]) == 2 else c["tau"])


def test_pure_spot_history_is_the_sticky_moneyness_cell():
    """Identical slices throughout: sigma_b - sigma_a is +0.0 and the scenario is section 17's sticky-moneyness cell with
    a = S_b / S_a - 1 and v = 0, up to S (1 + a) against S (S_b / S_a): two roundings of a number near 1, which a price turns into
    at most |delta| S x 2 eps <= S x 2 eps per option.  Measured in units of eps x sum |qty| S and asserted at SPOT_ONLY_UNITS."""
    c = _spot_only(HC.make(3))
    r = hsim(c)
    worst = 0.0
    for p in (3, 8):
        S = c["spot"]
        a = np.array([S[p - s] / S[p - 1 - s] - 1.0 for s in range(p)])
        bk = R.restate_book(c["params"][p:p + 1], c["Tq"], S[p:p + 1], c["rate"], c["u"], c["tau"], c["qty"], a, [0.0], c["is_put"], c["strike_mode"])
        unit = EPS * float(np.sum(np.abs(np.where(r["live"][p], c["qty"], 0.0)))) * S[p]
        err = np.abs(r["pnl"][p, :p] - bk["pnl_sm"][0, :, 0]) / unit
        worst = max(worst, float(err.max()))
        assert same(np.isnan(r["pnl"][p, :p]), np.isnan(bk["pnl_sm"][0, :, 0]))
    log("meaning[spot-only vs sticky-moneyness cell]", units=worst)
    assert worst <= HC.SPOT_ONLY_UNITS, worst


def test_var_of_a_long_call_is_the_pnl_at_the_mth_worst_return():
    """One long call, spot-only scenarios with distinct returns: the P&L is increasing in the return, so VaR is minus the P&L of
    the m-th smallest return and worst is that return's scenario."""
    c = _spot_only(HC.make(4))                                               # B = 70
    c = dict(c, u=np.array([1.02]), tau=np.array([float(np.asarray(c["Tq"]).reshape(-1)[3])]), qty=np.array([1.0]), is_put=np.array([0], np.uint8), strike_mode=0,
             tail_probs=(0.05, 0.25, 0.5), min_scen=10, window=65)
    r = hsim(c)
    S = c["spot"]
    for p in (20, 69):
        n = min(p, 65)
        ret = np.array([S[p - s] / S[p - 1 - s] for s in range(n)])
        order = np.argsort(ret, kind="stable")
        assert len(np.unique(ret)) == n and r["n_valid"][p] == n and r["worst"][p] == order[0]
        for l, tp in enumerate(c["tail_probs"]):
            m = max(1, int(np.floor(n * tp)))
            assert r["var"][p, l] == 0.0 - r["pnl"][p, order[m - 1]]
            assert r["es"][p, l] == pytest.approx(-np.mean(r["pnl"][p, order[:m]]), rel=1e-12)


def test_var_is_at_most_es_and_both_fall_with_the_tail_probability():
    for n in (3, 4, 6, 7):
        r = hsim(HC.make(n))
        ok = ~np.isnan(r["var"][:, 0])
        assert ok.any() and (r["var"][ok] <= r["es"][ok]).all()
        tp = np.asarray(r["tail_probs"])
        order = np.argsort(tp)
        assert (np.diff(r["var"][ok][:, order], axis=1) <= 0).all() and (np.diff(r["es"][ok][:, order], axis=1) <= 0).all()


def test_an_empty_book_and_a_batch_without_slices():
    """H9 as the restatement has it: without options every existing scenario, VaR, ES and value is +0.0."""
    c = HC.make(3)
    r = hsim(dict(c, u=c["u"][:, :0], tau=c["tau"][:, :0], qty=c["qty"][:0], is_put=c["is_put"][:0]))
    ex = r["exists"]
    assert plus_zero(r["pnl"][ex]) and np.isnan(r["pnl"][~ex]).all() and (r["scen_flags"][ex] == 0).all() and plus_zero(r["value"]) and (r["n_dead"] == 0).all()
    ok = r["n_valid"] >= c["min_scen"]
    assert plus_zero(r["var"][ok]) and plus_zero(r["es"][ok]) and np.isnan(r["var"][~ok]).all() and same(r["worst"], np.where(r["n_valid"] > 0, 0, -1))


# ------------------------------------------------------------------ the restatement's own rounding level
def test_rounding_level():
    """R_CPU: the restatement against the same rules in mpmath at 50 digits over the micro tables and the small generated shapes
    the GPU tests use, in the units of hsim_cases.tolerances; the scenario P&Ls of the books, and of every book of one of their
    options alone (the GPU tests run some of those)."""
    import mpmath  # noqa: F401  (a host without it must not pass this test by skipping it)
    worst = {k: 0.0 for k in HC.VALUE_KEYS}
    compared = 0
    # neg_hist_w is left out: the sign of its W is decided by the rounding of fp64 itself, which is what that case is about
    inputs = [(f"micro[{k}]", c) for k, c in sorted(HC.MICRO.items()) if k != "neg_hist_w"] + [(HC.shape_id(HC.SHAPES[n]), HC.make(n)) for n in HC.MP_SHAPES]
    for name, c in inputs:
        r = hsim(c, keep=True)
        ex = H.exact_hsim(c, r)
        u = HC.units(ex, r)
        fig = {}
        for k, v in u.items():
            assert same(np.isnan(ex[k]), np.isnan(r[k])), (name, k)
            fig[k] = float(np.nanmax(v)) if np.isfinite(v).any() else 0.0
            worst[k] = max(worst[k], fig[k])
            compared += int(np.isfinite(v).sum())
        with np.errstate(all="ignore"):                                      # the books of one option each: scenario P&L = its own term
            solo = np.abs(ex["terms"] - r["terms"]) / (EPS * r["scale_terms"] + HC.TINY)
        assert same(np.isnan(ex["terms"]), np.isnan(r["terms"])), name
        if np.isfinite(solo).any():
            fig["pnl_one_option"] = float(np.nanmax(solo))
            worst["pnl"] = max(worst["pnl"], fig["pnl_one_option"])
            compared += int(np.isfinite(solo).sum())
            for q in range(0, solo.shape[2], 3):                             # and their VaR and ES, in the unit of H7: the row's largest
                if not r["live"][:, q].any():
                    continue
                fl = np.where(np.isnan(r["terms"][:, :, q]), np.maximum(r["scen_flags"], H.VOID_PAIR), r["scen_flags"])
                a, b = H.tail(r["terms"][:, :, q], fl, c["tail_probs"], c["min_scen"]), H.tail(ex["terms"][:, :, q], fl, c["tail_probs"], c["min_scen"])
                unit = EPS * np.nan_to_num(r["scale_terms"][:, :, q]).max(axis=1)[:, None] + HC.TINY
                for k, i in (("var", 0), ("es", 1)):
                    if np.isfinite(a[i]).any():
                        d = float(np.nanmax(np.abs(a[i] - b[i]) / (unit + (2.0 * EPS * np.abs(a[i]) if k == "es" else 0.0))))
                        fig[k + "_one_option"] = max(fig.get(k + "_one_option", 0.0), d)
                        worst[k] = max(worst[k], d)
        log(f"rounding[{name}]", options=int(r["live"].size), live=int(r["live"].sum()), scenarios=int((r["scen_flags"] == 0).sum()), **fig)
    log("rounding[all]", compared=compared, **worst)
    assert compared > 10000
    for k in worst:
        assert worst[k] <= HC.R_CPU[k], (k, worst[k])


def test_generated_batches_meet_their_conditions():
    """The conditions of the generated batches hold for the restatement alone (hsim_ref.check_margins): live options, valid
    scenarios, sigma' off zero, |V| off zero, and no two valid P&Ls that straddle a tail boundary (or the first rank, on which
    `worst` rests) closer than the sum of their GPU allowances."""
    factor = HC.C_GPU * HC.R_CPU["pnl"]
    for n in list(range(len(HC.SHAPES))) + ["stream"]:
        c = HC.make(n)
        r = hsim(c)
        H.check_margins(r, factor=factor, unordered=n in HC.UNORDERED_SHAPES)
        S = c["spot"]
        assert S.max() / S.min() <= 1.02 * 1.02
        if n in HC.UNORDERED_SHAPES:
            assert r["degenerate"].all() and (r["scen_flags"][r["exists"]] == HC.VOID).all() and (r["n_valid"] == 0).all() and np.isnan(r["value"]).all()


# ------------------------------------------------------------------ host layers with the restatement as the backend
HOUR = 60                                 # the synthetic chain is quoted hourly, the snapshots are per minute


def _built():
    chain = synthetic_chain("btc", expiry_days=(0.5, 3), strikes=tuple(np.linspace(17000.0, 34000.0, 12)), n_hours=3, seed=5)
    b = SnapshotSurfaceBuilder(backend=H.RefBackend(), moneyness=np.linspace(0.72, 1.28, 24), tenors=np.array([1.0, 2.0, 2.8]) / 365)
    res = b.build(chain)
    svi = b.svi(res, rate=0.01, rounds=6)
    t0 = res[0].dates[0]
    bk = pd.DataFrame({"strike": [20000.0, 25000.0, 30000.0, 25000.0, 26000.0], "expiry": [t0 + pd.Timedelta(days=d) for d in (1.5, 2.5, 5.0, -1.0, 2.0)],
                       "callput": ["c", "P", "call", "p", "put"], "quantity": [2.0, -1.0, 0.5, 1.0, float("nan")]})
    return b, res, svi, bk


def test_var_report_and_frame():
    b, res, svi, bk = _built()
    reps = b.var(res, bk, svi, rate=0.01, lag=HOUR, window=4, tail_probs=(0.5, 0.25), min_scenarios=1)
    assert len(reps) == 1 and isinstance(reps[0], VarReport)
    p, r = reps[0], res[0]
    B = len(r.dates)
    assert p.lag == HOUR and p.window == 4 and list(p.dates) == list(r.dates) and p.tau.shape == (B, 5) and same(p.tail_probs, [0.5, 0.25])
    c = dict(params=svi[0].params, Tq=r.tenors, spot=r.spot, rate=0.01, u=np.broadcast_to(p.strikes, p.tau.shape), tau=p.tau, strike_mode=1,
             is_put=p.is_put, qty=p.quantity, lag=HOUR, window=4, tail_probs=(0.5, 0.25), min_scen=1)
    ref = hsim(c)
    for k in H.OUT_KEYS:
        assert same(getattr(p, k), ref[k]), k
    keep = np.flatnonzero(np.asarray(r.quotes) > 0)
    f = var_frame(reps, res)
    cols = ["underlying", "date", "spot", "n_valid"] + var_level_columns((0.5, 0.25)) + ["worst_pnl", "worst_start", "value", "gross", "n_dead"]
    assert list(f.columns) == cols and cols[4:8] == ["var_0.5", "es_0.5", "var_0.25", "es_0.25"] and len(f) == len(keep) == 3
    assert list(f["date"]) == list(r.dates[keep]) and f["n_dead"].dtype == np.int32 and (f["n_dead"] == 2).all()
    assert same(f["var_0.25"].to_numpy(), ref["var"][keep, 1]) and same(f["es_0.5"].to_numpy(), ref["es"][keep, 0]) and same(f["gross"].to_numpy(), ref["value"][keep, 1])
    w = ref["worst"][keep]
    assert (w[1:] >= 0).all() and w[0] == -1 and np.isnan(f["worst_pnl"][0]) and pd.isna(f["worst_start"][0])
    for i in (1, 2):
        assert f["worst_pnl"][i] == ref["pnl"][keep[i], w[i]] and f["worst_start"][i] == r.dates[keep[i] - HOUR - w[i]]
    # the scenarios between two quoted hours start at snapshots without quotes: their pairs are void, the hourly ones are valid
    assert same(f["n_valid"].to_numpy(), ref["n_valid"][keep]) and len(var_frame([], [])) == 0
    own = b.var(res, bk, rate=0.01, rounds=6, lag=HOUR, window=4, tail_probs=(0.5, 0.25), min_scenarios=1)[0]       # runs svi itself
    assert same(own.pnl, ref["pnl"])


def test_argument_checks():
    from iv_interpolation_amd import engine
    b, res, svi, bk = _built()
    for col in ("strike", "expiry", "callput", "quantity"):
        with pytest.raises(KeyError):
            b.var(res, bk.drop(columns=col), svi)
    with pytest.raises(ValueError, match="callput"):
        b.var(res, bk.assign(callput="x"), svi)
    with pytest.raises(ValueError, match="SVI reports"):
        b.var(res, bk, svi_reports=[])
    for kw, word in ((dict(lag=0), "lag"), (dict(lag=1.5), "lag"), (dict(window=0), "window"), (dict(window=1025), "window"), (dict(min_scenarios=0), "min_scen"),
                     (dict(tail_probs=(0.0,)), "tail"), (dict(tail_probs=(1.0,)), "tail"), (dict(tail_probs=(float("nan"),)), "tail"),
                     (dict(tail_probs=(0.1,) * 9), "tail")):
        with pytest.raises(ValueError, match=word):
            b.var(res, bk, svi, **kw)
    assert engine.hsim_settings(2, 7, (0.5,), 3, 7) == (2, 7, [0.5], 3, 7) and engine.HSIM_OUTPUTS == H.OUT_KEYS
    with pytest.raises(ValueError, match="scen_per_wg"):
        engine.hsim_settings(1, 4, (), 1, 5)


def test_var_task_end_to_end(tmp_path):
    import complete_pipeline as cp
    store = FrameStore(str(tmp_path))
    chain = synthetic_chain("btc", expiry_days=(20, 45), strikes=tuple(np.linspace(17000.0, 34000.0, 6)), n_hours=4, seed=5)
    for f in chain:
        store.write_output(f["symbol"].iloc[0], f, 1)
    argv = ["--task", "var", "--lag", "60", "--window", "121", "--levels", "0.5,0.25", "--min-scenarios", "1", "--data-dir", str(tmp_path)]
    assert cp.main(argv, surface_backend=H.RefBackend()) == 0
    out = store.read_table("iv_var", "btc")
    assert list(out.columns)[:8] == ["underlying", "date", "spot", "n_valid", "var_0.5", "es_0.5", "var_0.25", "es_0.25"] and len(out) == 4
    assert list(out["n_valid"]) == [0, 1, 2, 3] and (out["n_dead"] == 0).all() and same(out["gross"].to_numpy(), out["value"].to_numpy())
    pipe = cp.CompleteOptimizedPipeline(cp.get_config(), data_dir=str(tmp_path), surface_backend=H.RefBackend())
    res = pipe.run_var(lag=HOUR, window=121, levels=(0.5, 0.25), min_scenarios=1)
    assert res["success"] and res["var_rows"] == 4 and res["dead_options"] == 0
    assert set(res) == set(pipe.run_svi()) | {"var_rows", "dead_options", "backtest"}
    realised = store.read_table("iv_explain", "btc")
    assert realised is None                                                  # the back-test writes no table of its own
    bt = res["backtest"]
    assert [b_["tp"] for b_ in bt] == [0.5, 0.25]
    ex = pipe.run_explain(lag=HOUR) and store.read_table("iv_explain", "btc")
    both = out.merge(ex[["start", "actual"]], left_on="date", right_on="start")
    for b_, col in zip(bt, ("var_0.5", "var_0.25")):
        ok = np.isfinite(both[col]) & np.isfinite(both["actual"])
        assert b_["eligible"] == int(ok.sum()) == 2 and b_["exceedances"] == int((ok & (both["actual"] < -both[col])).sum())
        assert b_["exceedance_rate"] == b_["exceedances"] / b_["eligible"]
    assert "window" in pipe.run_var(window=0)["error"] and "tail" in pipe.run_var(levels=(1.5,))["error"]
    assert cp.main(["--task", "var", "--lag", "500", "--data-dir", str(tmp_path)], surface_backend=H.RefBackend()) == 0     # every scenario ABSENT: rows all the same
    late = store.read_table("iv_var", "btc")
    assert (late["n_valid"] == 0).all() and late["var_0.05"].isna().all() and list(late.columns)[4:8] == ["var_0.05", "es_0.05", "var_0.01", "es_0.01"]


# ------------------------------------------------------------------ header, struct and binding, field for field
def test_header_struct_and_binding_agree():
    import ctypes as C
    import re
    from test_risk import _header_fields
    from iv_interpolation_amd import _lib
    scalar = {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}
    src, fields = _header_fields("ivs_hsim_args")
    assert [n for n, _, _ in fields] == [n for n, _ in _lib.HsimArgs._fields_]
    for (name, ctype, ptr), (_, have) in zip(fields, _lib.HsimArgs._fields_):
        assert have is ((C.POINTER(C.c_double) if name == "tail_probs" else C.c_void_p) if ptr else scalar[ctype]), name
    assert re.search(r"int\s+ivs_svi_hsim_f64\(const ivs_hsim_args\*[^,]*,\s*void\*[^,]*,\s*size_t[^,]*,\s*void\*[^)]*\);", src)
    res, args = _lib.SIGNATURES["ivs_svi_hsim_f64"]
    assert res is C.c_int and args == [C.POINTER(_lib.HsimArgs), C.c_void_p, C.c_size_t, C.c_void_p]
    assert re.search(r"#define\s+IVS_ABI_VERSION\s+5\b", src) and _lib.ABI_VERSION == 5
    for name, v in (("ABSENT", 1), ("VOID_PAIR", 2), ("NEG_VOL", 4)):
        assert re.search(r"IVS_HS_%s\s*=\s*%d\b" % (name, v), src) and getattr(_lib, "HS_" + name) == v == getattr(H, name)


def test_c_abi_refusals_need_no_device():
    """Every refusal of the entry point comes before anything touches the device: the pointers here are fakes."""
    import ctypes as C
    from iv_interpolation_amd import _lib
    lib = _lib.load()
    fn = lib.ivs_svi_hsim_f64
    ptrs = ("params", "Tq", "spot", "u", "tau", "qty", "pnl", "scen_flags", "var", "es", "n_valid", "n_dead", "worst")
    ints = dict(tq_stride=0, q_stride=0, mT=16, Q=8, B=3, strike_mode=0, lag=1, window=4, min_scen=1, scen_per_wg=0, stages=0)

    def args(tp=(0.05, 0.01), **kw):
        a = _lib.HsimArgs()
        for k in ptrs:
            setattr(a, k, kw.get(k, 64))
        for k, v in ints.items():
            setattr(a, k, kw.get(k, v))
        a.nL = kw["nL"] if "nL" in kw else len(tp)
        a.tail_probs = C.cast((C.c_double * max(len(tp), 1))(*tp), C.POINTER(C.c_double)) if tp is not None else None
        return a

    EINVAL, ERANGE = -22, -34
    assert fn(None, None, 0, None) == EINVAL and b"null args" in lib.ivs_last_error()
    table = [(dict(Q=-1), EINVAL, b"negative"), (dict(B=-1), EINVAL, b"negative"), (dict(nL=-1), EINVAL, b"negative"), (dict(strike_mode=2), EINVAL, b"strike_mode"),
             (dict(mT=65), ERANGE, b"mT=65"), (dict(lag=0), ERANGE, b"lag=0"), (dict(window=0), ERANGE, b"window=0"), (dict(window=1025), ERANGE, b"window=1025"),
             (dict(nL=9, tp=(0.1,) * 9), ERANGE, b"nL=9"), (dict(tp=(0.05, 0.0)), ERANGE, b"tail probability 1"), (dict(tp=(1.0,)), ERANGE, b"tail probability 0"),
             (dict(tp=(float("nan"),)), ERANGE, b"tail probability"), (dict(tp=(float("inf"),)), ERANGE, b"tail probability"), (dict(tp=None, nL=1), EINVAL, b"null tail"),
             (dict(min_scen=0), ERANGE, b"min_scen=0"), (dict(scen_per_wg=-1), ERANGE, b"scen_per_wg=-1"), (dict(scen_per_wg=5), ERANGE, b"scen_per_wg=5"),
             (dict(stages=3), ERANGE, b"stages=3"), (dict(q_stride=7), EINVAL, b"stride"), (dict(tq_stride=3), EINVAL, b"stride"),
             (dict(B=2 ** 31, Q=1), ERANGE, b"exceed"), (dict(B=2 ** 20, Q=2 ** 11), ERANGE, b"exceed"), (dict(B=2 ** 21, Q=1, mT=1, window=1024), ERANGE, b"scenarios exceed"),
             (dict(lag=0, B=0), ERANGE, b"lag=0"), (dict(window=0, Q=0), ERANGE, b"window=0"), (dict(tp=(2.0,), mT=0), ERANGE, b"tail probability")]
    table += [({k: None}, EINVAL, b"null pointer") for k in ptrs]
    for kw, code, word in table:
        assert fn(C.byref(args(**kw)), None, 0, None) == code and word in lib.ivs_last_error() and lib.ivs_last_kernel() == b"", (kw, lib.ivs_last_error())
    for kw in (dict(Q=0), dict(B=0), dict(mT=0)):                                                                              # H9: no-ops
        assert fn(C.byref(args(**kw)), None, 0, None) == 0 and lib.ivs_last_kernel() == b"", kw
