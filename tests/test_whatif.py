"""CPU: the restatement of rules W0-W9 (tests/whatif_ref.py) against the tables worked out by hand, the consequences of the rules
(the q = 0 rung, the one-round link to section 21, negation, es >= var, convexity in q), W8, the same rules in mpmath, the
conditions every generated value case must meet, the host-side argument checks and the refusals of the C entry point, which need
no device; and the builder, the frame and the pipeline task with the restatement as the backend.

test_rounding_level prints the largest error of every output in its unit; with IVS_WHATIF_ERRLOG=<file> set the figures are appended
to that file (a recorded run belongs in profiles/whatif/errlog.txt)."""
import ctypes
import os

import numpy as np
import pytest

import hedge_ref as G
import hsim_ref as H
import whatif_cases as WC
import whatif_ref as W

EPS = WC.EPS
_cache = {}


def log(name, **figures):
    line = name + ": " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items())
    print(line)
    path = os.environ.get("IVS_WHATIF_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def case(name):
    """(case with its sizes, section 19 restated on its book, the ladder restated on the restated rows)."""
    if name not in _cache:
        c = WC.make(name)
        h = H.restate_hsim(c["params"], c["Tq"], c["spot"], c["rate"], c["u"], c["tau"], c["qty"], c["lag"], c["window"], c["tail_probs"],
                           c["min_scen"], c["is_put"], c["strike_mode"])
        rows = G.inst_rows(c["params"], c["Tq"], c["spot"], c["rate"], c["inst_u"], c["inst_tau"], c["inst_kind"], c["lag"], c["window"], c["strike_mode"])
        c = WC.with_sizes(c, h["pnl"], rows["inst_pnl"])
        _cache[name] = (c, h, restate(c, h, rows=rows))
    return _cache[name]


def restate(c, h, size=None, **kw):
    return W.restate_whatif(c["params"], c["Tq"], c["spot"], c["rate"], c["inst_u"], c["inst_tau"], c["inst_kind"], h["pnl"], h["scen_flags"],
                            c["size"] if size is None else size, c["lag"], c["window"], c["tail_probs"], c["min_scen"], c["strike_mode"],
                            unit_y=h["scale_pnl"], **kw)


def table_ref(t, **over):
    t = dict(t, **over)
    return W.ladder(t["inst_pnl"], t["pnl"], t["scen_flags"], t["size"], t["lag"], t["tail_probs"], t["min_scen"])


def same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), what
    if a.dtype.kind == "f":
        assert np.array_equal(np.signbit(np.nan_to_num(a)), np.signbit(np.nan_to_num(b))), what      # a zero's sign too


def check_want(name, r, p, want):
    """want: {key or key + candidate: the value at snapshot p (of that candidate)}, exact."""
    for k, v in want.items():
        key, h = (k[:-1], int(k[-1])) if k[-1].isdigit() and k[:-1] in r else (k, None)
        got = r[key][p] if h is None else r[key][p, h]
        v = np.asarray(v, np.asarray(got).dtype)
        want_v = v.reshape(np.shape(got)) if v.size == np.size(got) else np.broadcast_to(v, np.shape(got))
        same_bits(got, want_v, (name, k, got, v))


@pytest.mark.parametrize("name", sorted(WC.TABLES))
def test_tables_by_hand(name):
    t = WC.TABLES[name]
    r = table_ref(t)
    p = t["window"]
    check_want(name, r, p, t["want"])
    assert (r["worst_w"][:p] == -1).all() and (r["best"][:p] == -1).all() and (r["n_scen"][:p] == 0).all() and (r["trade_flags"][:p] == 0).all()
    assert np.isnan(r["var_w"][:p]).all() and np.isnan(r["var0"][:p]).all()          # nothing ranked: inactive, and no flag without a scenario
    if name == "minus_two":                                  # x and -x under q and -q: the same rows
        for k in ("var_w", "es_w", "worst_w", "best"):
            same_bits(r[k][p, 0], r[k][p, 1], k)
        same_bits(r["var_w"][p, 0, 0], r["var0"][p], "q = 0")


@pytest.mark.parametrize("name", sorted(WC.MICRO))
def test_micro_cases(name):
    """hedge_cases.MICRO with a ladder: W3's bit is M3's (a dead candidate, one with a scenario vol that is not positive, degenerate
    snapshots), the flagged candidates' rungs are dead, and the q = 0 rung of every other is the book itself."""
    c = WC.MICRO[name]
    h = dict(pnl=c["pnl"], scen_flags=c["row_flags"], scale_pnl=None)
    r = restate(c, h)
    g = G.restate_hedge(c["params"], c["Tq"], c["spot"], c["rate"], c["inst_u"], c["inst_tau"], c["inst_kind"], c["pnl"], c["row_flags"], c["lag"],
                        c["window"], c["tail_probs"], c["min_scen"], c["rounds"], c["n_forced"], c["tol"], c["min_gain"], c["strike_mode"])
    assert np.array_equal(r["trade_flags"], g["inst_flags"] & G.NEG_VOL)
    dead = (r["trade_flags"] != 0) | ~r["active"][:, None]
    assert (r["worst_w"][dead] == -1).all() and np.isnan(r["es_w"][dead]).all() and (r["best"][dead] == -1).all()
    assert np.array_equal(r["live"], np.broadcast_to(~dead[:, :, None], r["live"].shape))
    B, nH = dead.shape
    for p, hh in zip(*np.nonzero(~dead)):
        same_bits(r["var_w"][p, hh, 0], r["var0"][p], "q = 0")
        same_bits(r["es_w"][p, hh, 0], r["es0"][p], "q = 0")
        assert r["worst_w"][p, hh, 0] == r["worst0"][p]
    var, es, n, worst = H.tail(c["pnl"], np.where(r["ranked"], 0, 1), c["tail_probs"], c["min_scen"])
    for a, b in ((r["var0"], var), (r["es0"], es), (r["n_scen"], n), (r["worst0"], worst)):
        same_bits(a, b, "W6")
    if name == "dead_and_neg_vol":
        assert list(r["trade_flags"][1]) == [2, 2, 0] and r["best"][2, 2, 0] >= 0


# ------------------------------------------------------------------ the consequences of the rules
def test_zero_rung_carries_the_books_own_bits():
    c, h, r = case("seventy")
    size = np.array(c["size"])
    size[:, 3], size[:, 9] = 0.0, -0.0
    z = restate(c, h, size, rows=r["rows"])
    live = z["live"][:, :, 3]
    assert live.sum() > 100
    for j in (3, 9):
        for k, b in (("var_w", "var0"), ("es_w", "es0")):
            same_bits(z[k][:, :, j][live], np.broadcast_to(z[b][:, None], z[k][:, :, j].shape)[live], (k, j))
        assert np.array_equal(z["worst_w"][:, :, j][live], np.broadcast_to(z["worst0"][:, None], live.shape)[live])
    for k, b in (("var0", "var"), ("es0", "es"), ("worst0", "worst"), ("n_scen", "n_valid")):      # W6: section 19's own
        same_bits(z[k], h[b], k)


@pytest.mark.parametrize("n_forced", [0, 1])
def test_one_round_of_section_21_is_a_rung(n_forced):
    """With one non-empty round the hedged row of M10 is y + q x_c from y: the rung at q = hedge[p][c] is that row, and H7 on it is
    the same."""
    c, h, r = case("seventy")
    g = G.restate_hedge(c["params"], c["Tq"], c["spot"], c["rate"], c["inst_u"], c["inst_tau"], c["inst_kind"], h["pnl"], h["scen_flags"], c["lag"],
                        c["window"], c["tail_probs"], c["min_scen"], 1, n_forced, 1e-6, 0.0, c["strike_mode"], rows=r["rows"])
    z = restate(c, h, g["hedge"][:, :, None], rows=r["rows"])
    done = np.flatnonzero(g["pick"][:, 0] >= 0)
    assert len(done) >= 40
    for p in done:
        cc = g["pick"][p, 0]
        same_bits(z["var_w"][p, cc, 0], g["var_h"][p], p)
        same_bits(z["es_w"][p, cc, 0], g["es_h"][p], p)
        assert z["worst_w"][p, cc, 0] == g["worst_h"][p] and z["n_scen"][p] == g["n_scen"][p]
    assert np.isnan(z["var_w"][~g["active"]]).all()          # hedge is NaN there: the rungs are dead


def test_negation_es_above_var_and_convexity():
    c, h, r = case("seventy")
    neg = W.ladder(-r["inst_pnl"], h["pnl"], h["scen_flags"], -np.asarray(c["size"]), c["lag"], c["tail_probs"], c["min_scen"])
    for k in ("var_w", "es_w", "worst_w", "best", "trade_flags"):
        same_bits(neg[k], r[k], k)
    live = r["live"]
    assert live.sum() > 1000
    with np.errstate(invalid="ignore"):
        assert (r["es_w"][live] >= r["var_w"][live]).all() and (r["es0"][r["active"]] >= r["var0"][r["active"]]).all()
    # convexity: the mean of the m smallest is a minimum of linear functions of q, so a middle rung lies on or below the chord of its
    # neighbours, up to the three allowances; the chord is formed in extended precision
    q = np.broadcast_to(r["size"][..., None], r["es_w"].shape).astype(np.longdouble)
    es, sc = r["es_w"].astype(np.longdouble), r["scale_es_w"]
    ok = (live[:, :, :-2] & live[:, :, 1:-1] & live[:, :, 2:])[..., None] & np.ones(es.shape[-1], bool)
    lam = (q[:, :, 1:-1] - q[:, :, :-2]) / (q[:, :, 2:] - q[:, :, :-2])
    chord = es[:, :, :-2] + lam * (es[:, :, 2:] - es[:, :, :-2])
    allow = WC.R_CPU["es_w"] * EPS * (sc[:, :, :-2] + sc[:, :, 1:-1] + sc[:, :, 2:])
    over = (es[:, :, 1:-1] - chord)[ok] / allow[ok]
    log("convexity: (es - chord) over the three allowances", worst=float(over.max()), rungs=int(ok.sum()))
    assert ok.sum() > 1000 and over.max() <= 1.0


def test_a_rung_does_not_depend_on_the_others():
    """W8: one rung of one candidate recomputed alone, and a snapshot on a batch of its own history alone."""
    c, h, r = case("nine_63")
    size = W.sizes(c["size"], 9, 63)
    for p, hh, j in ((8, 62, 1), (5, 0, 0), (8, 17, 1)):
        one = W.ladder(r["inst_pnl"][:, :, hh:hh + 1], h["pnl"], h["scen_flags"], size[:, hh:hh + 1, j:j + 1], c["lag"], c["tail_probs"], c["min_scen"])
        for k in ("var_w", "es_w", "worst_w"):
            same_bits(one[k][p, 0, 0], r[k][p, hh, j], (k, p, hh, j))
    perm = np.random.default_rng(5).permutation(63)
    mixed = W.ladder(r["inst_pnl"][:, :, perm], h["pnl"], h["scen_flags"], size[:, perm], c["lag"], c["tail_probs"], c["min_scen"])
    for k in ("var_w", "es_w", "worst_w", "best", "trade_flags"):
        same_bits(mixed[k], r[k][:, perm], k)


# ------------------------------------------------------------------ tolerances and conditions
def test_rounding_level():
    """R_CPU of whatif_cases: the restatement against the same rules in mpmath on the same rows, in the restatement's own units."""
    worst = {k: 0.0 for k in WC.VALUE_KEYS}
    refs = [(n, case(n)[2], case(n)[1]["pnl"]) for n in WC.MP_CASES] + [(n, table_ref(t), t["pnl"]) for n, t in sorted(WC.TABLES.items()) if n != "row_1024"]
    refs += [("micro " + n, restate(c, dict(pnl=c["pnl"], scen_flags=c["row_flags"], scale_pnl=None)), c["pnl"]) for n, c in sorted(WC.MICRO.items())]
    for name, ref, pnl in refs:
        ex = W.exact_whatif(ref, pnl)
        fig = {}
        with np.errstate(all="ignore"):
            for k in WC.VALUE_KEYS:
                assert np.array_equal(np.isnan(ex[k]), np.isnan(ref[k])), (name, k)
                d = np.abs(ex[k] - ref[k])
                u = np.where(d <= WC.TINY, 0.0, (d - WC.TINY) / (EPS * ref["scale_" + k]))
                fig[k] = float(np.nanmax(u)) if np.isfinite(u).any() else 0.0
                assert not np.isinf(u).any(), (name, k)      # a difference where the unit is 0
                worst[k] = max(worst[k], fig[k])
        log("rounding " + name, **fig)
    log("rounding level", **worst)
    for k, v in worst.items():
        assert v <= WC.R_CPU[k], (k, v, WC.R_CPU[k])
        assert v >= 0.5 * WC.R_CPU[k] or v == 0.0, f"R_CPU[{k}] = {WC.R_CPU[k]} is more than twice the measured {v}: record the measurement"


@pytest.mark.parametrize("name", WC.CHAIN)
def test_generated_cases_meet_their_conditions(name):
    """What whatif_cases promises of the value cases that run on the device's own rows, for the restatement alone; and no (p, h, j, l)
    of them is left out of the comparison: every rung of a usable candidate of an active snapshot is live."""
    c, h, r = case(name)
    H.check_margins(dict(h, tail_probs=np.asarray(c["tail_probs"]), min_scen=c["min_scen"]))
    WC.check_conditions(r)
    usable = (r["trade_flags"] == 0) & r["active"][:, None]
    assert np.array_equal(r["live"], np.broadcast_to(usable[:, :, None], r["live"].shape))
    assert not np.isnan(r["es_w"][r["live"]]).any() and (r["best"][usable] >= 0).all()


def test_the_cases_cover_the_shapes():
    s = list(WC.CASES.values()) + [WC.WIDE]
    for key, want in (("B", {1, 2, 3, 9, 70, 260}), ("lag", {1, 2}), ("window", {1, 2, 4, 63, 64, 65, 257, 1024}), ("mT", {1, 2, 16}),
                      ("nH", {1, 2, 3, 63, 64}), ("nQ", {1, 2, 15, 16}), ("nL", {0, 1, 2, 8})):
        assert {d[key] for d in s} >= want, key
    assert {bool(d.get("per_ladder")) for d in s} == {False, True}
    assert set(np.concatenate([WC.make(n)["inst_kind"] for n in ("three_lag2", "nine_63")])) == {0, 1, 2}


# ------------------------------------------------------------------ argument checks: no device
def test_whatif_settings():
    from iv_interpolation_amd import _lib, engine
    assert engine.whatif_settings(1, 256, (0.05, 0.01), 20, 64, 8) == (1, 256, [0.05, 0.01], 20, 8, 0) and _lib.WI_MAX_RUNGS == 16
    bad = [dict(n_inst=0), dict(n_inst=65), dict(n_rungs=0), dict(n_rungs=17), dict(n_rungs=2.5), dict(stages=3), dict(window=1025), dict(lag=0),
           dict(min_scen=0), dict(tail_probs=(1.0,)), dict(tail_probs=(0.1,) * 9)]
    for b in bad:
        kw = dict(lag=1, window=256, tail_probs=(0.05,), min_scen=20, n_inst=64, n_rungs=8, stages=0)
        kw.update(b)
        with pytest.raises(ValueError):
            engine.whatif_settings(**kw)


def _args(**over):
    """A call that passes every check but names buffers that do not exist: it must be refused before any of them is touched."""
    from iv_interpolation_amd import _lib
    a = _lib.WhatIfArgs()
    for k, t in _lib.WhatIfArgs._fields_:
        if t is ctypes.c_void_p:
            setattr(a, k, 0x1000)
    tp = (ctypes.c_double * 2)(0.05, 0.01)
    a.tail_probs, a.nL = ctypes.cast(tp, ctypes.POINTER(ctypes.c_double)), 2
    a.tq_stride, a.inst_stride, a.rate, a.strike_mode, a.mT, a.nH, a.B = 0, 0, 0.0, 0, 16, 64, 100
    a.lag, a.window, a.min_scen, a.nQ, a.size_stride, a.stages, a.scen_per_wg = 1, 256, 20, 8, 0, 0, 0
    for k, v in over.items():
        setattr(a, k, v)
    a._keep = tp
    return a


def test_c_refusals_touch_nothing():
    from iv_interpolation_amd import _lib
    lib = _lib.load()                                        # a library that is missing or lacks the entry point fails here
    EINVAL, ERANGE = -22, -34
    assert lib.ivs_svi_whatif_f64(None, None, 0, None) == EINVAL
    table = [(EINVAL, dict(nL=-1)), (EINVAL, dict(B=-1)), (EINVAL, dict(nH=-1)), (EINVAL, dict(strike_mode=2)), (EINVAL, dict(tq_stride=-1)),
             (ERANGE, dict(mT=65)), (ERANGE, dict(lag=0)), (ERANGE, dict(window=0)), (ERANGE, dict(window=1025)), (ERANGE, dict(nL=9)),
             (EINVAL, dict(tail_probs=None)), (ERANGE, dict(min_scen=0)), (ERANGE, dict(scen_per_wg=257)), (ERANGE, dict(nH=65)),
             (ERANGE, dict(nQ=0)), (ERANGE, dict(nQ=17)), (ERANGE, dict(nQ=-1)), (ERANGE, dict(stages=3)), (ERANGE, dict(stages=-1)),
             (ERANGE, dict(B=2 ** 31 // (256 * 64) + 1)), (ERANGE, dict(B=2 ** 31 // (64 * 16 * 8) + 1, window=1, nQ=16, nL=8, tail_probs=_tp8())),
             (EINVAL, dict(size_stride=7)), (EINVAL, dict(size_stride=-1)), (EINVAL, dict(size_stride=64)),
             (EINVAL, dict(params=None)), (EINVAL, dict(inst_kind=None)), (EINVAL, dict(inst_pnl=None)), (EINVAL, dict(pnl=None)),
             (EINVAL, dict(size=None)), (EINVAL, dict(trade_flags=None)), (EINVAL, dict(var_w=None)), (EINVAL, dict(best=None)),
             (EINVAL, dict(es0=None)), (EINVAL, dict(n_scen=None)), (EINVAL, dict(tq_stride=3)), (EINVAL, dict(inst_stride=7))]
    for want, over in table:
        a = _args(**over)
        rc = lib.ivs_svi_whatif_f64(ctypes.byref(a), None, 0, None)
        assert rc == want, (over, rc, lib.ivs_last_error())
        assert lib.ivs_last_error() and lib.ivs_last_kernel() == b""
    # the limits come before the zero-size return, and an empty call is a no-op on buffers that do not exist
    for over in (dict(B=0), dict(mT=0), dict(nH=0)):
        assert lib.ivs_svi_whatif_f64(ctypes.byref(_args(**over)), None, 0, None) == 0, over
    assert lib.ivs_svi_whatif_f64(ctypes.byref(_args(B=0, nQ=17)), None, 0, None) == ERANGE
    assert lib.ivs_svi_whatif_f64(ctypes.byref(_args(nH=0, size_stride=3)), None, 0, None) == EINVAL


def _tp8():
    tp = (ctypes.c_double * 8)(*[0.1 * (i + 1) for i in range(8)])
    return ctypes.cast(tp, ctypes.POINTER(ctypes.c_double))


# ------------------------------------------------------------------ host layers with the restatement as the backend
HOUR = 60
KW = dict(rate=0.01, lag=HOUR, window=4, tail_probs=(0.5, 0.25), min_scenarios=1)


def _built():
    import pandas as pd
    from iv_interpolation_amd.snapshots import SnapshotSurfaceBuilder
    from iv_interpolation_amd.frame_store import synthetic_chain
    chain = synthetic_chain("btc", expiry_days=(0.5, 3), strikes=tuple(np.linspace(17000.0, 34000.0, 12)), n_hours=3, seed=5)
    b = SnapshotSurfaceBuilder(backend=W.RefBackend(), moneyness=np.linspace(0.72, 1.28, 24), tenors=np.array([1.0, 2.0, 2.8]) / 365)
    res = b.build(chain)
    svi = b.svi(res, rate=0.01, rounds=6)
    t0 = res[0].dates[0]
    bk = pd.DataFrame({"symbol": list("abcde"), "strike": [20000.0, 25000.0, 30000.0, 25000.0, 26000.0],
                       "expiry": [t0 + pd.Timedelta(days=d) for d in (1.5, 2.5, 5.0, -1.0, 1.5)],
                       "callput": ["c", "P", "call", "p", "put"], "quantity": [2.0, -1.0, 0.5, 1.0, float("nan")]})
    inst = pd.DataFrame({"symbol": ["spot", "x", "y"], "strike": [0.0, 24000.0, 27000.0], "expiry": [pd.NaT, t0 + pd.Timedelta(days=2.0), t0 + pd.Timedelta(days=1.2)],
                         "callput": ["underlying", "put", "C"]})
    return b, res, svi, bk, inst


def test_builder_report_and_frame():
    import pandas as pd
    from iv_interpolation_amd.snapshots import WhatIfReport, whatif_frame
    b, res, svi, bk, inst = _built()
    var = b.var(res, bk, svi, **KW)
    ladder = (0.0, 0.5, 1.0, 2.0)
    r = res[0]
    tau = b._tau(pd.DatetimeIndex(inst["expiry"]), r.dates)
    strikes = np.array([np.nan, 24000.0, 27000.0])
    common = (svi[0].params, r.tenors, r.spot, 0.01, np.broadcast_to(strikes, tau.shape), tau, np.array([2, 1, 0], np.uint8), var[0].pnl, var[0].scen_flags)
    # quantities
    reps = b.whatif(res, bk, inst, ladder, "abs", var, svi, **KW)
    assert len(reps) == 1 and isinstance(reps[0], WhatIfReport)
    p = reps[0]
    assert p.labels == ["spot", "x", "y"] and list(p.kind) == [2, 1, 0] and p.var is var[0].var and np.isnan(p.strikes[0]) and p.size_unit == "abs"
    assert np.array_equal(p.size, np.broadcast_to(np.asarray(ladder), (len(r.dates), 3, 4)))
    ref = W.restate_whatif(*common, np.tile(np.asarray(ladder), (3, 1)), HOUR, 4, (0.5, 0.25), 1, 1)
    for k in W.OUT_KEYS:
        assert np.array_equal(getattr(p, k), ref[k], equal_nan=True), k
    assert (p.worst_w[:, :, 0][p.worst_w[:, :, 0] >= 0] == np.broadcast_to(p.worst0[:, None], (len(r.dates), 3))[p.worst_w[:, :, 0] >= 0]).all()
    # multiples of section 21's own size per candidate and snapshot
    solo = b.whatif(res, bk, inst, ladder, "solo", var, svi, **KW)[0]
    g = G.restate_hedge(*common, HOUR, 4, (0.5, 0.25), 1, 1, 0, 1e-6, 1e-4, 1)
    assert np.array_equal(solo.size, g["solo_qty"][:, :, None] * np.asarray(ladder), equal_nan=True)
    ref2 = W.restate_whatif(*common, solo.size, HOUR, 4, (0.5, 0.25), 1, 1)
    for k in W.OUT_KEYS:
        assert np.array_equal(getattr(solo, k), ref2[k], equal_nan=True), k
    dead = np.isnan(g["solo_qty"])
    assert dead.any() and (solo.worst_w[dead] == -1).all() and (solo.worst_w[~dead] >= 0).all()      # a NaN size: no live rung
    own = b.whatif(res, bk, inst, ladder, fit_rounds=6, **KW)[0]                       # runs svi and var itself, the default unit
    assert own.size_unit == "solo" and np.array_equal(own.es_w, ref2["es_w"], equal_nan=True)
    # the frame: the best rung of the top instruments by ES reduction at the first level
    keep = np.flatnonzero(np.asarray(r.quotes) > 0)
    f = whatif_frame([solo], res, top=2)
    assert list(f.columns) == ["underlying", "date", "instrument", "size", "var_0.5", "var_0.5_after", "var_0.5_change", "es_0.5", "es_0.5_after",
                               "es_0.5_change", "var_0.25", "var_0.25_after", "var_0.25_change", "es_0.25", "es_0.25_after", "es_0.25_change",
                               "worst_start", "worst_start_after"]
    assert len(whatif_frame([], [])) == 0 and len(f) > 0
    i = 0
    for n in keep:
        live = np.flatnonzero(ref2["best"][n, :, 0] >= 0)
        gain = {h: ref2["es0"][n, 0] - ref2["es_w"][n, h, ref2["best"][n, h, 0], 0] for h in live}
        for h in sorted(live, key=lambda h: (-gain[h], h))[:2]:
            row, j = f.iloc[i], ref2["best"][n, h, 0]
            i += 1
            assert row["date"] == r.dates[n] and row["instrument"] == solo.labels[h] and row["size"] == solo.size[n, h, j]
            assert row["es_0.5"] == ref2["es0"][n, 0] and row["es_0.5_after"] == ref2["es_w"][n, h, j, 0] and row["var_0.25_after"] == ref2["var_w"][n, h, j, 1]
            assert row["es_0.5_change"] == ref2["es_w"][n, h, j, 0] - ref2["es0"][n, 0]
            assert row["worst_start"] == r.dates[n - HOUR - ref2["worst0"][n]] and row["worst_start_after"] == r.dates[n - HOUR - ref2["worst_w"][n, h, j]]
    assert i == len(f)
    with pytest.raises(ValueError, match="other settings"):
        b.whatif(res, bk, inst, ladder, "abs", b.var(res, bk, svi, **{**KW, "window": 5}), svi, **KW)
    with pytest.raises(ValueError, match="VaR reports"):
        b.whatif(res, bk, inst, ladder, "abs", [], svi, **KW)
    for kw, word in ((dict(sizes=(1.0,) * 17), "rungs"), (dict(sizes=()), "rungs"), (dict(size_unit="lots"), "size_unit"), (dict(window=1025), "window")):
        with pytest.raises(ValueError, match=word):
            b.whatif(res, bk, inst, **{**dict(sizes=ladder), **KW, **kw})
    with pytest.raises(KeyError):
        b.whatif(res, bk, inst.drop(columns="callput"), ladder, "abs", var, svi, **KW)
    with pytest.raises(ValueError, match="callput"):
        b.whatif(res, bk, inst.assign(callput=["underlying", "x", "c"]), ladder, "abs", var, svi, **KW)


def test_default_instruments_and_ladder():
    b, res, svi, book, _ = _built()
    rep = b.whatif(res, book, None, svi_reports=svi, **KW)[0]
    assert rep.labels[0] == "underlying" and list(rep.kind) == [2, 0, 0] and rep.labels[1:] == ["a", "c"]
    assert list(rep.sizes) == [0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 3.0] and rep.es_w.shape == (len(res[0].dates), 3, 8, 2)


def test_whatif_task_end_to_end(tmp_path):
    import pandas as pd
    import complete_pipeline as cp
    from iv_interpolation_amd.frame_store import FrameStore
    from iv_interpolation_amd.frame_store import synthetic_chain
    store = FrameStore(str(tmp_path))
    chain = synthetic_chain("btc", expiry_days=(20, 45), strikes=tuple(np.linspace(17000.0, 34000.0, 6)), n_hours=4, seed=5)
    for f in chain:
        store.write_output(f["symbol"].iloc[0], f, 1)
    argv = ["--task", "whatif", "--sizes", "0.5,1,2", "--top", "2", "--lag", "60", "--window", "121", "--levels", "0.5,0.25", "--min-scenarios", "1",
            "--data-dir", str(tmp_path)]
    assert cp.main(argv, surface_backend=W.RefBackend()) == 0
    out, var = store.read_table("iv_whatif", "btc"), store.read_table("iv_var", "btc")
    assert list(out.columns)[:4] == ["underlying", "date", "instrument", "size"] and len(var) == 4 and 0 < len(out) <= 4 * 2
    assert out.groupby("date").size().max() <= 2 and np.allclose(out["es_0.5_change"], out["es_0.5_after"] - out["es_0.5"])
    pipe = cp.CompleteOptimizedPipeline(cp.get_config(), data_dir=str(tmp_path), surface_backend=W.RefBackend())
    kw = dict(lag=HOUR, window=121, levels=(0.5, 0.25), min_scenarios=1)
    res = pipe.run_whatif(sizes=(0.5, 1, 2), top=2, **kw)
    assert res["success"] and res["whatif_rows"] == len(out) and set(res) == set(pipe.run_var(**kw)) | {"whatif_rows", "median_es_reduction"}
    assert np.isfinite(res["median_es_reduction"])
    listed = sorted(f["symbol"].iloc[0] for f in chain)
    with_file = tmp_path / "trades.csv"
    pd.DataFrame({"symbol": ["underlying", listed[0]]}).to_csv(with_file, index=False)
    res = pipe.run_whatif(trades_file=str(with_file), sizes=(-1.0, 1.0), size_unit="abs", **kw)
    table = store.read_table("iv_whatif", "btc")
    assert res["success"] and set(table["instrument"]) <= {"underlying", listed[0]} and set(table["size"]) <= {-1.0, 1.0}
    pd.DataFrame({"symbol": ["nope"]}).to_csv(with_file, index=False)
    assert "not listed" in pipe.run_whatif(trades_file=str(with_file), **kw)["error"]
    assert "rungs" in pipe.run_whatif(sizes=(1.0,) * 17)["error"] and "window" in pipe.run_whatif(window=0)["error"]
    assert "size_unit" in pipe.run_whatif(size_unit="lots")["error"] and "top" in pipe.run_whatif(top=0)["error"]
    assert pipe.run_hedge(rounds=2, **kw)["success"]         # the hedge task reads its candidates as before
