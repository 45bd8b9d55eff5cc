"""CPU: rules A0-A8 on the restatement tests/attrib_ref.py: the micro tables worked out by hand, the
additivity and bit links of the allocation, the restatement's rounding level against the same rules in mpmath (R_CPU), the
conditions of the generated batches, and the host layers (builder, frame, pipeline task, argument checks, C refusals) with the
restatement as the backend.

With IVS_ATTRIB_ERRLOG=<file> set the measured figures are appended to that file (a recorded run belongs in
profiles/attrib/errlog.txt)."""
import os

import numpy as np
import pandas as pd
import pytest

import attrib_cases as AC
import attrib_ref as A
import hsim_cases as HC
import hsim_ref as H
import risk_ref as R
from iv_interpolation_amd.frame_store import FrameStore, synthetic_chain
from iv_interpolation_amd.snapshots import SnapshotSurfaceBuilder, VarAttributionReport, top_contributors, var_attribution_frame

EPS = AC.EPS


def log(name, **figures):
    line = name + ": " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items())
    print(line)
    path = os.environ.get("IVS_ATTRIB_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def attrib(c, **kw):
    return A.restate_attrib(c["params"], c["Tq"], c["spot"], c["rate"], c["u"], c["tau"], c["qty"], c["lag"], c["window"], c["tail_probs"],
                            c["min_scen"], c["is_put"], c["strike_mode"], c["group"], c["nG"], **kw)


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return same(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def plus_zero(a):
    a = np.asarray(a)
    return bool((a == 0.0).all() and not np.signbit(a).any())


_cache = {}


def case(name):
    """Inputs and restatement of one generated batch, computed once and shared (read-only)."""
    if name not in _cache:
        c = AC.make(name)
        r = attrib(c)
        for a in list(c.values()) + list(r.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = (c, r)
    return _cache[name]


# ------------------------------------------------------------------ micro tables
@pytest.mark.parametrize("name", sorted(AC.MICRO))
def test_micro(name):
    """The NaN pattern of A6, n_tail and order by hand from the case's own scen_flags and n_valid, and the additivity of A3-A5."""
    c = AC.MICRO[name]
    r = attrib(c)
    h = r["hsim"]
    B, Q, nL = len(c["spot"]), len(c["qty"]), len(c["tail_probs"])
    assert same(h["scen_flags"], c["scen_flags"]) and same(h["n_valid"], c["n_valid"])
    active = (c["n_valid"] >= c["min_scen"]) & (c["n_valid"] > 0)
    for p in range(B):
        n = int(c["n_valid"][p])
        m = [max(1, int(np.floor(n * t))) if active[p] else 0 for t in c["tail_probs"]]
        assert list(r["n_tail"][p]) == m, (p, m)
        assert (r["order"][p, :n] >= 0).all() and (r["order"][p, n:] == -1).all() and sorted(r["order"][p, :n]) == list(np.flatnonzero(c["scen_flags"][p] == 0))
        assert (np.diff(h["pnl"][p, r["order"][p, :n]]) >= 0).all()
        for l in range(nL):
            on = m[l] > 0
            for k in ("ces", "cvar"):
                assert same(np.isnan(r[k][p, l]), ~(h["live"][p] & on)), (k, p, l)          # a dead option, an inactive level
            for k in ("ces_group", "cvar_group"):
                assert np.isnan(r[k][p, l]).all() == (not on) and np.isnan(r[k][p, l]).any() == (not on), (k, p, l)
            if on:                                                                      # A4 adds up to the bit, A3 within its unit
                assert same_bits(0.0 - R.b5_sum(np.where(h["live"][p], 0.0 - r["cvar"][p, l], 0.0)), h["var"][p, l]), (p, l)
                tot = np.nansum(r["ces"][p, l])
                assert abs(tot - h["es"][p, l]) <= 4.0 * EPS * np.nansum(r["scale_ces"][p, l]) + HC.TINY, (p, l)


def test_one_option_book_is_var_and_es_to_the_bit():
    c = AC.MICRO["one_option"]
    r = attrib(c)
    h = r["hsim"]
    assert np.isfinite(h["var"][1:]).all()
    for k, v in (("cvar", "var"), ("ces", "es")):
        assert same_bits(r[k][:, :, 0], h[v]) and same_bits(r[k + "_group"][:, :, 0], h[v]), k


def test_h6_pair_in_the_tail_gives_plus_zero():
    c = AC.MICRO["same_pair"]
    r = attrib(c)
    assert list(r["order"][1]) == [0, -1] and r["n_tail"][1, 0] == 1                      # snapshot 1: the identical pair alone
    for k in AC.VALUE_KEYS:
        assert plus_zero(r[k][1]), k
    assert (r["cvar"][2] != 0.0).any()


def test_dead_options_quantities_and_groups():
    c = AC.MICRO["quantities"]                                                           # quantities 0, NaN, 1, inf, -0: options 1 and 3 dead
    r = attrib(c)
    on = r["n_tail"][:, 0] > 0
    assert on.any() and np.isnan(r["ces"][on][:, :, [1, 3]]).all() and np.isfinite(r["ces"][on][:, :, [0, 2, 4]]).all()
    assert plus_zero(r["ces"][on][:, :, [0, 4]]) and plus_zero(r["cvar"][on][:, :, [0, 4]])      # a zero quantity of either sign: +0.0
    assert plus_zero(r["ces_group"][on][:, :, 1]) and plus_zero(r["cvar_group"][on][:, :, 1])    # group 1 = the dead ones alone
    e = attrib(AC.MICRO["empty_group"])
    assert plus_zero(e["ces_group"][on][:, :, 1:]) and same_bits(e["ces_group"][:, :, 0], r["ces_group"][:, :, 0])
    g = attrib(AC.MICRO["group_range"])                                                  # options 2 and 4 are in no group
    h = g["hsim"]
    on = g["n_tail"][:, 0] > 0
    assert on.any()
    for p in np.flatnonzero(on):
        t = 0.0 - g["cvar"][p, 0]
        assert same_bits(g["cvar_group"][p, 0, 0], 0.0 - R.b5_sum(np.where(np.arange(5) == 0, t, 0.0)))
        assert same_bits(g["cvar_group"][p, 0, 1], 0.0 - R.b5_sum(np.where(np.arange(5) == 3, t, 0.0)))
        assert g["cvar_group"][p, 0].sum() != h["var"][p, 0]


def test_too_few_and_flagged():
    r = attrib(AC.MICRO["too_few"])                                                      # min_scen 3: n = 0, 1, 2, 3
    assert list(r["n_tail"][:, 0]) == [0, 0, 0, 1] and list(r["n_tail"][:, 1]) == [0, 0, 0, 2]
    for k in AC.VALUE_KEYS:
        assert np.isnan(r[k][:3]).all() and np.isfinite(r[k][3]).all(), k
    assert list(r["order"][2]) == sorted(r["order"][2][:2], key=lambda s: r["hsim"]["pnl"][2, s]) + [-1]
    b = attrib(AC.MICRO["bad_spot_nan"])                                                 # snapshot 3 alone has a valid scenario: s = 0
    assert list(b["order"][3]) == [0, -1, -1] and (b["order"][:3] == -1).all() and list(b["n_tail"][:, 0]) == [0, 0, 0, 1]
    assert np.isnan(b["ces"][1]).all() and np.isnan(b["ces_group"][1]).all()             # the degenerate snapshot


@pytest.mark.parametrize("name", sorted(AC.ROWS))
def test_a1_rows(name):
    pnl, fl, n_p, order = AC.ROWS[name]
    assert list(A.rank(pnl, fl, n_p)) == order


# ------------------------------------------------------------------ the generated batches
def test_generated_batches_meet_their_conditions():
    """hsim_ref.check_margins on the shapes that pass it as generated; an active level in every case but the UNORDERED one; the
    B = 260 case reaches the cap; B3-Q257-w4 has an active row with min_scen = 1 and none with 3; and every m in {1, 2, 63, 64},
    nG in {1, 2, 16} and Q in {1, 2, 63, 65, 257, 1025} occurs."""
    factor = HC.C_GPU * HC.R_CPU["pnl"]
    ms, nGs, Qs = set(), set(), set()
    for name in AC.CASES:
        c, r = case(name)
        h = r["hsim"]
        if name in AC.MARGINS:
            H.check_margins(h, factor=factor)
        if name in AC.UNORDERED:
            assert h["degenerate"].all() and (r["n_tail"] == 0).all() and (r["order"] == -1).all()
            assert all(np.isnan(r[k]).all() for k in AC.VALUE_KEYS)
        else:
            assert (r["n_tail"] > 0).any(), name
        ms |= set(r["n_tail"].ravel().tolist())
        nGs.add(c["nG"])
        Qs.add(len(c["qty"]))
    for name, c in AC.MICRO.items():
        nGs.add(c["nG"])
        Qs.add(len(c["qty"]))
    assert case("B260-Q2-w257")[1]["n_tail"].max() == A.MAX_TAIL == 64
    c3 = AC.make("B3-Q257-w4")
    assert c3["min_scen"] == 1 and (case("B3-Q257-w4")[1]["n_tail"] > 0).any() and (attrib(dict(c3, min_scen=3))["n_tail"] == 0).all()
    assert {1, 2, 63, 64} <= ms and {1, 2, 16} <= nGs and {1, 2, 63, 65, 257, 1025} <= Qs, (ms, nGs, Qs)


@pytest.mark.parametrize("name", [n for n in AC.CASES if n not in AC.UNORDERED])
def test_additivity_and_links(name):
    """b5_sum of the live options' cvar == var to the bit; the sums of ces over the options and of ces_group over the groups that
    cover the book are es within the derived unit; with one group the group figures are var and es to the bit."""
    c, r = case(name)
    h = r["hsim"]
    lv = h["live"]
    on = r["n_tail"] > 0
    one = r if c["nG"] == 1 and c["group"] is None else attrib(dict(c, group=None, nG=1), hsim=h)
    assert same_bits(one["cvar_group"][:, :, 0], h["var"]) and same_bits(one["ces_group"][:, :, 0], h["es"])
    assert same(np.isnan(h["var"]), ~on)
    worst = 0.0
    for p, l in zip(*np.nonzero(on)):
        assert same_bits(0.0 - R.b5_sum(np.where(lv[p], 0.0 - r["cvar"][p, l], 0.0)), h["var"][p, l]), (p, l)
        unit = EPS * (np.nansum(r["scale_ces"][p, l]) + h["scale_es"][p, l] + 2.0 * len(lv[p]) * abs(h["es"][p, l])) + HC.TINY
        worst = max(worst, abs(np.nansum(r["ces"][p, l]) - h["es"][p, l]) / unit)
        unit = EPS * (one["scale_ces_group"][p, l, 0] + r["scale_ces_group"][p, l].sum() + 2.0 * c["nG"] * abs(h["es"][p, l])) + HC.TINY
        covered = c["group"] is None or ((c["group"] >= 0) & (c["group"] < c["nG"]))
        if np.all(covered | ~lv[p]):
            worst = max(worst, abs(r["ces_group"][p, l].sum() - h["es"][p, l]) / unit)
    log(f"additivity[{name}]", worst=float(worst), levels=int(on.sum()))
    assert worst <= 1.0


def test_ces_does_not_depend_on_the_grouping_or_on_b():
    c, r = case("B70-Q63-w65")
    other = attrib(dict(c, group=(np.arange(63) % 3).astype(np.int32), nG=3), hsim=r["hsim"])
    for k in ("ces", "cvar", "n_tail", "order"):
        assert same_bits(other[k], r[k]), k
    rows = np.arange(4, 70)                                                              # snapshot 69 of B = 70 against the call on its own rows
    pick = lambda a: a[rows] if np.ndim(a) == 2 and a.shape[0] == 70 else a    # noqa: E731
    alone = attrib(dict(c, params=c["params"][rows], spot=c["spot"][rows], Tq=pick(c["Tq"]), u=pick(c["u"]), tau=pick(c["tau"])))
    for k in AC.VALUE_KEYS + ("n_tail", "order"):
        assert same_bits(alone[k][-1], r[k][-1]), k


def test_rounding_level():
    """R_CPU: the restatement against the same rules in mpmath at 50 digits over the micro tables and the generated shapes on
    which mpmath stays affordable, each value in units of its own constant (attrib_cases.constants): every figure must stay at or below 1."""
    import mpmath  # noqa: F401  (a host without it must not pass this test by skipping it)
    worst, measured = {k: 0.0 for k in AC.VALUE_KEYS}, {k: 0.0 for k in AC.VALUE_KEYS}
    compared = 0
    inputs = [(f"micro[{k}]", c) for k, c in sorted(AC.MICRO.items())] + [(n, AC.make(n)) for n in AC.MP_CASES]
    for name, c in inputs:
        r = attrib(c)
        ex = A.exact_attrib(r, H.exact_hsim(c, r["hsim"])["terms"], c["tail_probs"], c["group"], c["nG"])
        raw, u = AC.units(ex, r), AC.allowance_ratios(ex, r)                             # in eps x scale; over the value's own constant
        fig = {}
        for k, v in u.items():
            assert same(np.isnan(ex[k]), np.isnan(r[k])), (name, k)
            fig[k] = float(np.nanmax(raw[k])) if np.isfinite(v).any() else 0.0
            measured[k] = max(measured[k], fig[k])
            worst[k] = max(worst[k], float(np.nanmax(v)) if np.isfinite(v).any() else 0.0)
            compared += int(np.isfinite(v).sum())
        log(f"rounding[{name}]", options=int(r["hsim"]["live"].size), tails=int(r["n_tail"].sum()), **fig)
    log("rounding[all]", compared=compared, **measured)                                  # R_CPU is this, a third higher
    log("rounding[all] over the constants", **worst)
    assert compared > 3000
    for k in worst:
        assert worst[k] <= 1.0, (k, worst[k])


# ------------------------------------------------------------------ host layers with the restatement as the backend
HOUR = 60


def _built():
    chain = synthetic_chain("btc", expiry_days=(0.5, 3), strikes=tuple(np.linspace(17000.0, 34000.0, 12)), n_hours=3, seed=5)
    b = SnapshotSurfaceBuilder(backend=A.RefBackend(), moneyness=np.linspace(0.72, 1.28, 24), tenors=np.array([1.0, 2.0, 2.8]) / 365)
    res = b.build(chain)
    svi = b.svi(res, rate=0.01, rounds=6)
    t0 = res[0].dates[0]
    bk = pd.DataFrame({"symbol": list("abcde"), "strike": [20000.0, 25000.0, 30000.0, 25000.0, 26000.0],
                       "expiry": [t0 + pd.Timedelta(days=d) for d in (1.5, 2.5, 5.0, -1.0, 1.5)],
                       "callput": ["c", "P", "call", "p", "put"], "quantity": [2.0, -1.0, 0.5, 1.0, float("nan")]})
    return b, res, svi, bk


KW = dict(rate=0.01, lag=HOUR, window=4, tail_probs=(0.5, 0.25), min_scenarios=1)


def test_report_and_frame():
    b, res, svi, bk = _built()
    var = b.var(res, bk, svi, **KW)
    reps = b.var_attribution(res, bk, var, svi, **KW)
    assert len(reps) == 1 and isinstance(reps[0], VarAttributionReport)
    p, r = reps[0], res[0]
    exp = sorted(set(bk["expiry"]))
    assert p.labels == [str(e) for e in exp] and list(p.group) == [exp.index(e) for e in bk["expiry"]] and p.var is var[0].var
    c = dict(params=svi[0].params, Tq=r.tenors, spot=r.spot, rate=0.01, u=np.broadcast_to(p.strikes, var[0].tau.shape), tau=var[0].tau, strike_mode=1,
             is_put=p.is_put, qty=p.quantity, lag=HOUR, window=4, tail_probs=(0.5, 0.25), min_scen=1, group=p.group, nG=len(exp))
    ref = attrib(c)
    for k in A.OUT_KEYS:
        assert same(getattr(p, k), ref[k]), k
    own = b.var_attribution(res, bk, rounds=6, **KW)[0]                                  # runs svi and var itself
    assert same(own.ces, ref["ces"]) and same(own.es, var[0].es)
    keep = np.flatnonzero(np.asarray(r.quotes) > 0)
    f = var_attribution_frame(reps, res)
    assert list(f.columns) == ["underlying", "date", "level", "group", "ces", "cvar", "ces_share", "n_tail", "var_start"]
    assert len(f) == len(keep) * 2 * len(exp) and f["n_tail"].dtype == np.int32 and len(var_attribution_frame([], [])) == 0
    i = 0
    for n in keep:
        for l, tp in enumerate((0.5, 0.25)):
            for g, lab in enumerate(p.labels):
                row = f.iloc[i]
                i += 1
                assert row["date"] == r.dates[n] and row["level"] == tp and row["group"] == lab and row["n_tail"] == ref["n_tail"][n, l]
                assert same(row["ces"], ref["ces_group"][n, l, g]) and same(row["cvar"], ref["cvar_group"][n, l, g])
                m = ref["n_tail"][n, l]
                if m:
                    assert row["ces_share"] == ref["ces_group"][n, l, g] / var[0].es[n, l]
                    assert row["var_start"] == r.dates[n - HOUR - ref["order"][n, m - 1]]
                else:
                    assert np.isnan(row["ces_share"]) and pd.isna(row["var_start"])
    assert (f["n_tail"] > 0).any() and (f["n_tail"] == 0).any()
    side = b.var_attribution(res, bk, var, svi, group_by="side", **KW)[0]
    assert side.labels == ["call", "put"] and list(side.group) == [0, 1, 0, 1, 1] and same(side.ces, ref["ces"])
    lab = b.var_attribution(res, bk, var, svi, groups=pd.Series({"a": "x", "b": "y", "c": "x", "e": "y"}), **KW)[0]
    assert lab.labels == ["x", "y"] and list(lab.group) == [0, 1, 0, -1, 1]
    top = top_contributors(reps, res, count=3)
    assert len(top) == 3 and list(top.columns)[:2] == ["underlying", "option"] and top["mean_abs_share"].is_monotonic_decreasing
    on = ref["n_tail"][keep, 0] > 0
    with np.errstate(all="ignore"):
        share = np.abs(ref["ces"][keep, 0][on] / var[0].es[keep, 0][on][:, None])
        share = np.where(np.isnan(share).all(axis=0), np.nan, np.nansum(share, axis=0) / np.maximum((~np.isnan(share)).sum(axis=0), 1))
    assert top["option"][0] == int(np.nanargmax(share)) and np.isclose(top["mean_abs_share"][0], np.nanmax(share), rtol=1e-14)


def test_many_expiries_fold_into_later():
    t0 = pd.Timestamp("2024-01-01")
    e = pd.DatetimeIndex([t0 + pd.Timedelta(days=d) for d in [5, 3, 1, 20, 19, 18, 17, 16, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6]] + [pd.NaT])
    ids, labels = SnapshotSurfaceBuilder._groups(pd.DataFrame(), e, np.zeros(19, bool), "expiry", None)
    assert len(labels) == 16 and labels[-1] == "later" and labels[0] == str(t0 + pd.Timedelta(days=1))
    assert list(ids) == [2, 1, 0, 15, 15, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, -1]
    ids, labels = SnapshotSurfaceBuilder._groups(pd.DataFrame(), e[:16], np.zeros(16, bool), "expiry", None)
    assert len(labels) == 16 and "later" not in labels and sorted(ids) == list(range(16))


def test_argument_checks():
    from iv_interpolation_amd import engine
    b, res, svi, bk = _built()
    for col in ("strike", "expiry", "callput", "quantity"):
        with pytest.raises(KeyError):
            b.var_attribution(res, bk.drop(columns=col), None, svi)
    with pytest.raises(KeyError):
        b.var_attribution(res, bk.drop(columns="symbol"), None, svi, groups=pd.Series({"a": "x"}), **KW)
    for kw, word in ((dict(lag=0), "lag"), (dict(window=1025), "window"), (dict(min_scenarios=0), "min_scen"), (dict(tail_probs=(1.0,)), "tail"),
                     (dict(tail_probs=(0.1,) * 9), "tail"), (dict(window=260, tail_probs=(0.25,)), "64"), (dict(window=1024, tail_probs=(0.05, 0.07)), "64"),
                     (dict(group_by="strike"), "group_by"), (dict(groups=pd.Series({c: c for c in "abcde"} | {"z": "q"}).iloc[:0]), "labels")):
        with pytest.raises(ValueError, match=word):
            b.var_attribution(res, bk, None, svi, **{**KW, **kw})
    with pytest.raises(ValueError, match="VaR reports"):
        b.var_attribution(res, bk, [], svi, **KW)
    with pytest.raises(ValueError, match="other settings"):
        b.var_attribution(res, bk, b.var(res, bk, svi, **{**KW, "window": 5}), svi, **KW)
    assert engine.attrib_settings(2, 1024, (0.05, 0.0625), 3, 16) == (2, 1024, [0.05, 0.0625], 3, 16) and engine.ATTRIB_OUTPUTS == A.OUT_KEYS
    assert engine.attrib_settings(1, 259, (0.25,), 1)[1] == 259                          # floor(64.75) = 64: the cap itself
    for n in (0, 17, 1.5):
        with pytest.raises(ValueError, match="n_groups"):
            engine.attrib_settings(1, 4, (0.5,), 1, n)


def test_varattrib_task_end_to_end(tmp_path):
    import complete_pipeline as cp
    store = FrameStore(str(tmp_path))
    chain = synthetic_chain("btc", expiry_days=(20, 45), strikes=tuple(np.linspace(17000.0, 34000.0, 6)), n_hours=4, seed=5)
    for f in chain:
        store.write_output(f["symbol"].iloc[0], f, 1)
    argv = ["--task", "varattrib", "--lag", "60", "--window", "121", "--levels", "0.5,0.25", "--min-scenarios", "1", "--data-dir", str(tmp_path)]
    assert cp.main(argv, surface_backend=A.RefBackend()) == 0
    out, var = store.read_table("iv_var_attrib", "btc"), store.read_table("iv_var", "btc")
    assert list(out.columns) == ["underlying", "date", "level", "group", "ces", "cvar", "ces_share", "n_tail", "var_start"]
    assert len(var) == 4 and len(out) == 4 * 2 * 2 and out["group"].nunique() == 2
    for (d, lv), part in out.groupby(["date", "level"]):
        v = var[var["date"] == d].iloc[0]
        if part["n_tail"].iloc[0]:
            assert np.isclose(part["ces"].sum(), v[f"es_{lv:g}"], rtol=1e-12, atol=1e-12) and np.isclose(part["cvar"].sum(), v[f"var_{lv:g}"], rtol=1e-12, atol=1e-12)
        else:
            assert part["ces"].isna().all() and np.isnan(v[f"var_{lv:g}"])
    pipe = cp.CompleteOptimizedPipeline(cp.get_config(), data_dir=str(tmp_path), surface_backend=A.RefBackend())
    res = pipe.run_varattrib(lag=HOUR, window=121, levels=(0.5, 0.25), min_scenarios=1, group_by="side")
    assert res["success"] and res["attrib_rows"] == 16 and set(res) == set(pipe.run_var(lag=HOUR, window=121, levels=(0.5, 0.25), min_scenarios=1)) | {"attrib_rows", "top_contributors"}
    top = res["top_contributors"]
    assert 0 < len(top) <= 10 and {"symbol", "mean_abs_share", "group"} <= set(top[0]) and top[0]["mean_abs_share"] >= top[-1]["mean_abs_share"]
    assert set(store.read_table("iv_var_attrib", "btc")["group"]) == {"call", "put"}
    assert "64" in pipe.run_varattrib(window=1024, levels=(0.1,))["error"] and "group_by" in pipe.run_varattrib(group_by="x")["error"]
    assert "window" in pipe.run_varattrib(window=0)["error"]


# ------------------------------------------------------------------ header, struct and binding, field for field
def test_header_struct_and_binding_agree():
    import ctypes as C
    import re
    from test_risk import _header_fields
    from iv_interpolation_amd import _lib
    scalar = {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}
    src, fields = _header_fields("ivs_hsim_attrib_args")
    assert [n for n, _, _ in fields] == [n for n, _ in _lib.HsimAttribArgs._fields_]
    for (name, ctype, ptr), (_, have) in zip(fields, _lib.HsimAttribArgs._fields_):
        assert have is ((C.POINTER(C.c_double) if name == "tail_probs" else C.c_void_p) if ptr else scalar[ctype]), name
    assert re.search(r"int\s+ivs_svi_hsim_attrib_f64\(const ivs_hsim_attrib_args\*[^,]*,\s*void\*[^,]*,\s*size_t[^,]*,\s*void\*[^)]*\);", src)
    res, args = _lib.SIGNATURES["ivs_svi_hsim_attrib_f64"]
    assert res is C.c_int and args == [C.POINTER(_lib.HsimAttribArgs), C.c_void_p, C.c_size_t, C.c_void_p]
    assert re.search(r"#define\s+IVS_ABI_VERSION\s+5\b", src) and _lib.ABI_VERSION == 5
    assert (_lib.HA_MAX_TAIL, _lib.HA_MAX_GROUPS) == (A.MAX_TAIL, A.MAX_GROUPS) == (64, 16)


def test_c_abi_refusals_need_no_device():
    """Every refusal of the entry point comes before anything touches the device: the pointers here are fakes."""
    import ctypes as C
    from iv_interpolation_amd import _lib
    lib = _lib.load()
    fn = lib.ivs_svi_hsim_attrib_f64
    ptrs = ("params", "Tq", "spot", "u", "tau", "qty", "pnl", "scen_flags", "n_tail")
    ints = dict(tq_stride=0, q_stride=0, mT=16, Q=8, B=3, strike_mode=0, lag=1, window=4, min_scen=1, nG=1)

    def args(tp=(0.05, 0.01), **kw):
        a = _lib.HsimAttribArgs()
        for k in ptrs + ("ces", "cvar", "ces_group", "cvar_group", "order", "group"):
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
             (dict(tp=(float("nan"),)), ERANGE, b"tail probability"), (dict(tp=None, nL=1), EINVAL, b"null tail"), (dict(min_scen=0), ERANGE, b"min_scen=0"),
             (dict(nG=0), ERANGE, b"nG=0"), (dict(nG=17), ERANGE, b"nG=17"), (dict(nG=-1), ERANGE, b"nG=-1"),
             (dict(window=260, tp=(0.05, 0.25)), ERANGE, b"tail of 65 > 64"), (dict(window=1024, tp=(0.0635,)), ERANGE, b"tail of 65 > 64"),
             (dict(q_stride=7), EINVAL, b"stride"), (dict(tq_stride=3), EINVAL, b"stride"),
             (dict(B=2 ** 31, Q=1), ERANGE, b"exceed"), (dict(B=2 ** 20, Q=2 ** 11), ERANGE, b"exceed"), (dict(B=2 ** 21, Q=1, mT=1, window=1024, tp=(0.05,)), ERANGE, b"scenarios exceed"),
             (dict(lag=0, B=0), ERANGE, b"lag=0"), (dict(nG=17, Q=0), ERANGE, b"nG=17"), (dict(window=1024, tp=(0.5,), mT=0), ERANGE, b"tail of 512")]
    table += [({k: None}, EINVAL, b"null pointer") for k in ptrs]
    for kw, code, word in table:
        assert fn(C.byref(args(**kw)), None, 0, None) == code and word in lib.ivs_last_error() and lib.ivs_last_kernel() == b"", (kw, lib.ivs_last_error())
    for kw in (dict(Q=0), dict(B=0), dict(mT=0), dict(window=259, tp=(0.25,), B=0), dict(window=1024, tp=(0.0625,), Q=0)):     # A8: no-ops; 64 is allowed
        assert fn(C.byref(args(**kw)), None, 0, None) == 0 and lib.ivs_last_kernel() == b"", kw
