"""CPU: the restatement of rules G0-G6 and B1-B5 (tests/risk_ref.py) against hand-worked tables, closed forms, finite
differences of the surface evaluation's own prices and the same rules in mpmath; the host layers (builder, frames, pipeline
task) with the restatement injected as the backend.  No GPU.

With IVS_RISK_ERRLOG=<file> set the figures every test prints are appended to that file (a recorded run belongs in
profiles/risk/errlog.txt)."""
import math
import os

import numpy as np
import pandas as pd
import pytest

import cal_ref as CR
import risk_cases as RC
import risk_ref as R
from iv_interpolation_amd.frame_store import FrameStore, synthetic_chain
from iv_interpolation_amd.snapshots import (YEAR_NS, RiskReport, SnapshotSurfaceBuilder, greeks_frame, listed_book, risk_frame,
                                            scenario_frame)

EPS = RC.EPS


def log(name, **figures):
    line = name + ": " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items())
    print(line)
    path = os.environ.get("IVS_RISK_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def greeks(c, **kw):
    return R.restate_greeks(c["params"], c["Tq"], c["spot"], c["rate"], c["u"], c["tau"], c["is_put"], c["strike_mode"], **kw)


def book(c, **kw):
    return R.restate_book(c["params"], c["Tq"], c["spot"], c["rate"], c["u"], c["tau"], c["qty"], c["spot_shocks"], c["vol_shocks"],
                          c["is_put"], c["strike_mode"], **kw)


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def bs(S, K, tau, r, sig, put):
    """Black-Scholes price, delta, gamma, vega and theta per year, written out with math.erfc."""
    N = lambda z: 0.5 * math.erfc(-z / math.sqrt(2.0))                        # noqa: E731
    n = lambda z: math.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)           # noqa: E731
    s = sig * math.sqrt(tau)
    d1 = (math.log(S / K) + r * tau) / s + 0.5 * s
    d2 = d1 - s
    KD = K * math.exp(-r * tau)
    if put:
        return (KD * N(-d2) - S * N(-d1), -N(-d1), n(d1) / (S * s), S * n(d1) * math.sqrt(tau),
                -S * n(d1) * sig / (2.0 * math.sqrt(tau)) + r * KD * N(-d2))
    return (S * N(d1) - KD * N(d2), N(d1), n(d1) / (S * s), S * n(d1) * math.sqrt(tau), -S * n(d1) * sig / (2.0 * math.sqrt(tau)) - r * KD * N(d2))


# ------------------------------------------------------------------ micro tables
@pytest.mark.parametrize("name", sorted(RC.MICRO))
def test_micro(name):
    c = RC.MICRO[name]
    g, b = greeks(c), book(c)
    assert same(g["flags"], c["flags"]), g["flags"]
    assert same(b["n_dead"], c["n_dead"]) and b["n_dead"].dtype == np.int32
    assert same(b["cell_flags"], c["cell_flags"]) and b["cell_flags"].dtype == np.int32
    dead = (g["flags"] & (RC.Q_DEAD | RC.Q_UNORDERED)) != 0
    for k in R.GREEK_KEYS:                                                    # G0: NaN exactly on the dead options
        assert same(np.isnan(g[k]), dead), k
    deg = b["degenerate"]
    assert same(np.isnan(b["net"]), np.broadcast_to(deg[:, None], b["net"].shape))
    for d, bit in (("ss", RC.NEG_VOL_SS), ("sm", RC.NEG_VOL_SM)):             # B3: NaN exactly on degenerate snapshots and NEG_VOL cells
        assert same(np.isnan(b["pnl_" + d]), deg[:, None, None] | ((c["cell_flags"] & bit) != 0)), d


def test_flat_surface_is_black_scholes():
    """b = 0: theta' = theta'' = 0, so the sticky-moneyness Greeks are the sticky-strike ones to the bit, both are Black-Scholes'
    at 20 % vol, and theta is the flat-vol theta (V = 0.04 between the slices and under SHORT / LONG alike)."""
    c = RC.MICRO["flat"]
    g = greeks(c)
    assert same(g["delta_sm"], g["delta_ss"])
    assert np.allclose(g["gamma_sm"], g["gamma_ss"], rtol=8 * EPS, atol=0.0)
    for q in range(6):
        want = bs(100.0, 100.0 * c["u"][q], c["tau"][q], c["rate"], 0.2, bool(c["is_put"][q]))
        got = [g[k][0, q] for k in ("price", "delta_ss", "gamma_ss", "vega", "theta")]
        assert np.allclose(got, want, rtol=1e-12, atol=1e-13), (q, got, want)


def test_put_call_parity():
    c = RC.batch(**RC.SHAPES[3])
    call, put = greeks(dict(c, is_put=None)), greeks(dict(c, is_put=np.ones(c["u"].shape[-1], np.uint8)))
    ok, L = call["ok"], call["loc"]
    assert ok.sum() > 150
    KD = (L["K"] * L["D"])[ok]
    assert np.allclose(call["delta_sm"][ok] - put["delta_sm"][ok], 1.0, rtol=0, atol=64 * EPS)
    assert np.allclose(call["delta_ss"][ok] - put["delta_ss"][ok], 1.0, rtol=0, atol=64 * EPS)
    for k in ("gamma_ss", "gamma_sm", "vega"):
        assert same(call[k], put[k]), k
    assert np.allclose((call["price"] - put["price"])[ok], L["S"][ok] - KD, rtol=0, atol=64 * EPS * L["S"][ok])
    # theta(call) - theta(put) = -rate K D: the difference of the two carries
    scale = call["scale_theta"][ok] + put["scale_theta"][ok]
    assert (np.abs((call["theta"] - put["theta"])[ok] + c["rate"] * KD) <= EPS * scale).all()


def _eval_call(c, spot=None, tau=None):
    r = CR.restate_eval(c["params"], c["Tq"], c["spot"] if spot is None else spot, c["rate"], c["u"], c["tau"] if tau is None else tau, 1)
    return r["call"], r["put"]


def test_central_differences_of_the_surface_prices():
    """G3 and G5 against the surface evaluation's own call and put (rules E1-E4, tests/cal_ref.py) bumped in S at fixed strikes
    (the curve in x stays: sticky moneyness) and in tau.  Step h = 1e-4 relative in S and 1e-5 years in tau: the truncation
    error is h^2/6 of the third derivative (1e-8 times a ratio of derivatives that is large in the wings), the rounding error
    eps x price / h.  Measured on these inputs, relative to the figure itself: 2.6e-7 (delta), 1.7e-7 (gamma), 6.1e-10 (theta);
    the bounds are 1e-6, 1e-6 and 1e-8.  A wrong term of G3 or G5 shows at 1e-3 or more (the last line)."""
    c = dict(RC.MICRO["zero_cell"])
    S = c["spot"]
    c.update(u=S[:, None] * np.asarray(c["u"])[None, :], tau=np.asarray(c["tau"])[None, :], strike_mode=1)
    g = greeks(c)
    put = g["put"]
    pick = lambda cp: np.where(put, cp[1], cp[0])                             # noqa: E731
    h = 1e-4 * S
    up, mid, dn = pick(_eval_call(c, spot=S + h)), pick(_eval_call(c)), pick(_eval_call(c, spot=S - h))
    d_fd, g_fd = (up - dn) / (2 * h), (up - 2 * mid + dn) / (h * h)
    ht = 1e-5
    t_fd = -(pick(_eval_call(c, tau=c["tau"] + ht)) - pick(_eval_call(c, tau=c["tau"] - ht))) / (2 * ht)
    e = {"delta": float(np.max(np.abs(d_fd - g["delta_sm"]) / np.abs(g["delta_sm"]))),
         "gamma": float(np.max(np.abs(g_fd - g["gamma_sm"]) / np.abs(g["gamma_sm"]))),
         "theta": float(np.max(np.abs(t_fd - g["theta"]) / np.abs(g["theta"])))}
    log("central_differences", **e)
    assert e["delta"] <= 1e-6 and e["gamma"] <= 1e-6 and e["theta"] <= 1e-8
    assert np.max(np.abs(g["delta_ss"] - g["delta_sm"])) > 1e-3              # the smile term is there to be seen


def test_a_shocked_cell_is_the_surface_moved_plus_black_scholes():
    """B2 for one-option books: sticky moneyness = the surface evaluated again at spot S' (same strike, same tau) for the vol,
    sticky strike = the base vol; then Black-Scholes at vol + v."""
    c0 = RC.MICRO["zero_cell"]
    S = float(c0["spot"][0])
    for q in range(5):
        K, tau, put, qty = S * c0["u"][q], c0["tau"][q], bool(c0["is_put"][q]), float(c0["qty"][q])
        c = dict(c0, u=np.array([K]), tau=np.array([tau]), strike_mode=1, is_put=np.array([put], np.uint8), qty=np.array([qty]),
                 spot_shocks=(-0.1, 0.05), vol_shocks=(-0.02, 0.03))
        b = book(c)
        vol0 = CR.restate_eval(c["params"], c["Tq"], c["spot"], c["rate"], c["u"], c["tau"], 1)["vol"][0, 0]
        P0 = bs(S, K, tau, c["rate"], vol0, put)[0]
        for i, a in enumerate(c["spot_shocks"]):
            S1 = S * (1.0 + a)
            vol1 = CR.restate_eval(c["params"], c["Tq"], np.array([S1]), c["rate"], c["u"], c["tau"], 1)["vol"][0, 0]
            for k, v in enumerate(c["vol_shocks"]):
                for d, vol in (("ss", vol0), ("sm", vol1)):
                    want = qty * (bs(S1, K, tau, c["rate"], vol + v, put)[0] - P0)
                    assert abs(b["pnl_" + d][0, i, k] - want) <= 1e-11 * S, (q, i, k, d)


def test_small_spot_moves_follow_the_sticky_moneyness_taylor_terms():
    """pnl_sm(a) - qty (delta_sm S a + gamma_sm (S a)^2 / 2) is the third-order remainder: it falls by 8 when a is halved.
    Measured: 3.9e-5 of the book's gross value at |a| = 1e-2 and 4.8e-6 at 5e-3, a ratio of 7.9.  The check is that ratio
    (between 6 and 10: neither a first- nor a second-order term is missing) and a bound of 1e-4 on the remainder itself."""
    c = dict(RC.MICRO["zero_cell"], spot_shocks=(-1e-2, -5e-3, 5e-3, 1e-2), vol_shocks=(0.0,))
    b, g = book(c), greeks(c)
    S = c["spot"][0]
    rem = []
    for i, a in enumerate(c["spot_shocks"]):
        taylor = np.sum(c["qty"] * (g["delta_sm"][0] * S * a + 0.5 * g["gamma_sm"][0] * (S * a) ** 2))
        rem.append(abs(b["pnl_sm"][0, i, 0] - taylor) / b["net"][0, 7])
    log("taylor", a1=float(rem[3]), a_half=float(rem[2]))
    assert max(rem) <= 1e-4 and 6.0 <= rem[3] / rem[2] <= 10.0 and 6.0 <= rem[0] / rem[1] <= 10.0
    ss = abs(b["pnl_ss"][0, 3, 0] - np.sum(c["qty"] * (g["delta_ss"][0] * S * 1e-2 + 0.5 * g["gamma_ss"][0] * (S * 1e-2) ** 2))) / b["net"][0, 7]
    assert ss <= 1e-4


def test_b4_zero_cell_and_b5_order():
    """B4: exactly +0.0 (not -0.0) under both dynamics.  B5: the order is that of a sum in passes of 256."""
    c = RC.MICRO["zero_cell"]
    b = book(c)
    for d in ("ss", "sm"):
        z = b["pnl_" + d][0, 1, 0]
        assert z == 0.0 and not np.signbit(z), d
        assert b["pnl_" + d][0, 1, 1] != 0.0
    b = book(RC.MICRO["qty_all_zero"])
    assert not np.signbit(b["net"]).any() and (b["net"] == 0.0).all() and (b["pnl_sm"] == 0.0).all() and not np.signbit(b["pnl_sm"]).any()
    for s in RC.SHAPES[1:4]:
        cb = RC.batch(**s)
        z = book(cb)
        a, v = np.asarray(cb["spot_shocks"]), np.asarray(cb["vol_shocks"])
        for d in ("ss", "sm"):
            cells = z["pnl_" + d][:, a == 0.0][:, :, v == 0.0]
            assert (cells == 0.0).all() and not np.signbit(cells).any()
    t = np.arange(1.0, 601.0)
    assert R.b5_sum(t) == 600 * 601 / 2 and R.depth(600) == 11 and R.depth(1) == 9 and R.depth(256) == 9 and R.depth(257) == 10
    r = np.random.default_rng(3).standard_normal(700)
    assert abs(R.b5_sum(r) - math.fsum(r)) <= R.depth(700) * EPS * np.abs(r).sum()


def test_book_is_the_sum_of_its_options():
    c = RC.batch(**RC.SHAPES[8])
    b, g = book(c, margins=True), greeks(c)
    live = b["live"]
    q = np.where(live, c["qty"][None, :], 0.0)
    for n, k in enumerate(R.GREEK_KEYS):
        want = np.array([math.fsum(row) for row in np.where(live, q * np.nan_to_num(g[k]), 0.0)])
        assert (np.abs(b["net"][:, n] - want) <= EPS * b["scale_net"][:, n]).all(), k
    assert same(b["n_dead"], (~live).sum(axis=1))
    one = book(dict(c, qty=np.where(np.arange(len(c["qty"])) == 0, c["qty"], 0.0)))      # all but option 0 at quantity zero
    solo = book(dict(c, u=c["u"][..., :1], tau=c["tau"][..., :1], qty=c["qty"][:1], is_put=None))
    assert same(one["pnl_sm"], solo["pnl_sm"]) and same(one["pnl_ss"], solo["pnl_ss"])


# ------------------------------------------------------------------ rounding level
def _inputs():
    yield from (("micro:" + n, c) for n, c in sorted(RC.MICRO.items()))
    yield from ((RC.shape_id(s), RC.batch(**s)) for s in RC.SHAPES)
    s = RC.STREAM_SHAPE
    c = RC.batch(**s)
    yield "stream:" + RC.shape_id(s) + "[::16]", dict(c, params=c["params"][::16], Tq=c["Tq"][::16], spot=c["spot"][::16], u=c["u"][::16], tau=c["tau"][::16])
    b, res, svi, bk = _built()
    rep = b.risk(res, bk, svi, rate=0.01)[0]
    yield "chain", dict(params=np.asarray(svi[0].params), Tq=res[0].tenors, spot=np.asarray(res[0].spot), rate=0.01,
                        u=np.ascontiguousarray(np.broadcast_to(rep.strikes, rep.tau.shape)), tau=rep.tau, strike_mode=1,
                        is_put=rep.is_put.astype(np.uint8), qty=rep.quantity, spot_shocks=tuple(rep.spot_shocks), vol_shocks=tuple(rep.vol_shocks))


def test_rounding_level():
    """R_CPU: the restatement against the same rules in mpmath at 50 digits over every input the GPU tests use (of the stream
    shape every 16th snapshot), in the units of risk_cases.tolerances_*."""
    import mpmath  # noqa: F401  (a host without it must not pass this test by skipping it)
    worst = {k: 0.0 for k in RC.VALUE_KEYS}
    compared = 0
    for name, c in _inputs():
        rb = book(c)
        rg = rb["greeks"]
        eg, eb = R.exact_greeks(c, rg), R.exact_book(c, rb)
        u = RC.units(eg, rg, RC.tolerances_greeks, R.GREEK_KEYS)
        u.update(RC.units(eb, rb, RC.tolerances_book, ("net", "pnl_ss", "pnl_sm")))
        fig = {}
        for k, v in u.items():
            ref = rg[k] if k in rg else rb[k]
            ex = eg[k] if k in eg else eb[k]
            assert same(np.isnan(ex), np.isnan(ref)), (name, k)
            fig[k] = float(np.nanmax(v)) if np.isfinite(v).any() else 0.0
            worst[k] = max(worst[k], fig[k])
            compared += int(np.isfinite(v).sum())
        log(f"rounding[{name}]", options=int(rg["ok"].size), live=int(rb["live"].sum()), **fig)
    log("rounding[all]", compared=compared, **worst)
    assert compared > 20000
    for k in worst:
        assert worst[k] <= RC.R_CPU[k], (k, worst[k])


def test_generated_batches_meet_their_conditions():
    """The off-threshold conditions of the generated batches hold for the restatement alone: >= 90 % of the options live, no
    NEG_VOL cell, every shocked vol 1e-9 off zero, |V| off zero."""
    for n, s in enumerate(RC.SHAPES + [RC.STREAM_SHAPE]):
        b = book(RC.batch(**s), margins=n not in RC.UNORDERED_SHAPES)
        if n in RC.UNORDERED_SHAPES:
            assert b["degenerate"].all() and (b["n_dead"] == s["Q"]).all() and np.isnan(b["pnl_sm"]).all() and not b["cell_flags"].any()


# ------------------------------------------------------------------ host layers with the restatement as the backend
def _built():
    chain = synthetic_chain("btc", expiry_days=(0.5, 3), strikes=tuple(np.linspace(17000.0, 34000.0, 12)), n_hours=3, seed=5)
    b = SnapshotSurfaceBuilder(backend=R.RefBackend(), moneyness=np.linspace(0.72, 1.28, 24), tenors=np.array([1.0, 2.0, 2.8]) / 365)
    res = b.build(chain)
    svi = b.svi(res, rate=0.01, rounds=6)
    t0 = res[0].dates[0]
    bk = pd.DataFrame({"strike": [20000.0, 25000.0, 30000.0, 25000.0, 26000.0], "expiry": [t0 + pd.Timedelta(days=d) for d in (1.5, 2.5, 5.0, -1.0, 2.0)],
                       "callput": ["c", "P", "call", "p", "put"], "quantity": [2.0, -1.0, 0.5, 1.0, float("nan")]})
    return b, res, svi, bk


def test_risk_report_and_frames():
    b, res, svi, bk = _built()
    reps = b.risk(res, bk, svi, rate=0.01)
    assert len(reps) == 1 and isinstance(reps[0], RiskReport)
    p, r = reps[0], res[0]
    tau = (p.expiries.as_unit("ns").asi8[None, :] - r.dates.as_unit("ns").asi8[:, None]) / YEAR_NS
    assert same(p.tau, tau) and same(p.is_put, [False, True, False, True, True]) and same(p.quantity, bk["quantity"])
    assert same(p.spot_shocks, RC.DEFAULT_SPOT_SHOCKS) and same(p.vol_shocks, RC.DEFAULT_VOL_SHOCKS)
    c = dict(params=svi[0].params, Tq=r.tenors, spot=r.spot, rate=0.01, u=np.broadcast_to(p.strikes, tau.shape), tau=tau, strike_mode=1,
             is_put=p.is_put, qty=p.quantity, spot_shocks=p.spot_shocks, vol_shocks=p.vol_shocks)
    rb = book(c)
    for k in R.GREEK_KEYS + ("flags",):
        assert same(p.greeks[k], rb["greeks"][k]), k
    for k in R.BOOK_KEYS:
        assert same(getattr(p, k), rb[k]), k
    keep = np.flatnonzero(np.asarray(r.quotes) > 0)
    assert len(keep) == 3 and (rb["n_dead"][keep] == 2).all()                 # the expired option and the NaN quantity
    f = risk_frame(reps, res)
    cols = ["underlying", "date", "spot"] + list(R.NET_KEYS) + ["n_dead"]
    assert list(f.columns) == cols and len(f) == 3 and f["n_dead"].dtype == np.int32 and list(f["date"]) == list(r.dates[keep])
    for n, k in enumerate(R.NET_KEYS):
        assert same(f[k].to_numpy(), rb["net"][keep, n]), k
    s = scenario_frame(reps, res)
    assert list(s.columns) == ["underlying", "date", "spot", "spot_shock", "vol_shock", "dynamic", "pnl", "flags"] and len(s) == 3 * 45 * 2
    first = s.iloc[:90]
    assert same(first["pnl"].to_numpy()[0::2], rb["pnl_ss"][keep[0]].reshape(-1)) and same(first["pnl"].to_numpy()[1::2], rb["pnl_sm"][keep[0]].reshape(-1))
    assert list(first["dynamic"][:2]) == ["ss", "sm"] and same(first["spot_shock"].to_numpy()[::10], RC.DEFAULT_SPOT_SHOCKS)
    assert same(first["vol_shock"].to_numpy()[:10:2], RC.DEFAULT_VOL_SHOCKS) and s["flags"].dtype == np.int32
    zero = s[(s["spot_shock"] == 0.0) & (s["vol_shock"] == 0.0)]
    assert len(zero) == 6 and (zero["pnl"] == 0.0).all()
    g = greeks_frame(reps, res)
    assert list(g.columns) == ["underlying", "date", "spot", "strike", "expiry", "callput", "quantity", "tau"] + list(R.GREEK_KEYS) + ["flags"]
    assert len(g) == 3 * 5 and list(g["callput"][:5]) == ["c", "p", "c", "p", "p"]
    for k in R.GREEK_KEYS + ("flags",):
        assert same(g[k].to_numpy(), rb["greeks"][k][keep].reshape(-1)), k
    own = b.risk(res, bk, rate=0.01, rounds=6, spot_shocks=(0.0, 0.1), vol_shocks=(0.0,))[0]      # runs svi itself
    assert same(own.net, p.net) and own.pnl_sm.shape == (len(r.dates), 2, 1) and same(own.pnl_sm[:, 1, 0], rb["pnl_sm"][:, 6, 2])
    for f_ in (risk_frame, scenario_frame, greeks_frame):
        assert len(f_([], [])) == 0
    assert list(risk_frame([], []).columns) == cols


def test_argument_checks():
    from iv_interpolation_amd import engine
    b, res, svi, bk = _built()
    for col in ("strike", "expiry", "callput", "quantity"):
        with pytest.raises(KeyError):
            b.risk(res, bk.drop(columns=col), svi)
    with pytest.raises(ValueError, match="callput"):
        b.risk(res, bk.assign(callput="x"), svi)
    with pytest.raises(ValueError, match="SVI reports"):
        b.risk(res, bk, svi_reports=[])
    for a, v in (((-1.0,), (0.0,)), ((float("nan"),), (0.0,)), ((float("inf"),), (0.0,)), ((0.0,), (float("nan"),)), ((0.0,), (float("-inf"),)),
                 ([0.0] * 33, [0.0] * 32), ([0.0] * 65, [0.0]), ([0.0], [0.0] * 65)):
        with pytest.raises(ValueError):
            engine.book_shocks(a, v)
        with pytest.raises(ValueError):
            b.risk(res, bk, svi, spot_shocks=a, vol_shocks=v)
    assert engine.book_shocks([0.0] * 32, [0.0] * 32) == ([0.0] * 32, [0.0] * 32) and engine.book_shocks([0.0] * 33, [0.0] * 31)[0] == [0.0] * 33
    assert engine.DEFAULT_SPOT_SHOCKS == RC.DEFAULT_SPOT_SHOCKS and engine.DEFAULT_VOL_SHOCKS == RC.DEFAULT_VOL_SHOCKS
    assert engine.GREEK_OUTPUTS == R.GREEK_KEYS and engine.NET_COLUMNS == R.NET_KEYS


def test_risk_task_end_to_end(tmp_path):
    import complete_pipeline as cp
    store = FrameStore(str(tmp_path))
    chain = synthetic_chain("btc", expiry_days=(20, 45), strikes=tuple(np.linspace(17000.0, 34000.0, 6)), n_hours=3, seed=5)
    for f in chain:
        store.write_output(f["symbol"].iloc[0], f, 1)
    assert cp.main(["--task", "risk", "--data-dir", str(tmp_path)], surface_backend=R.RefBackend()) == 0
    assert store.read_table("iv_svi", "btc") is None
    out, scen = store.read_table("iv_risk", "btc"), store.read_table("iv_scenarios", "btc")
    assert list(out.columns) == ["underlying", "date", "spot"] + list(R.NET_KEYS) + ["n_dead"]
    assert len(out) == 3 and len(scen) == 3 * 45 * 2
    listed = listed_book(chain)
    assert len(listed) == len(chain) == 24 and (listed["quantity"] == 1.0).all() and set(listed["callput"]) == {"c", "p"}
    assert (out["n_dead"] == 0).all() and (out["gross"] > 0).all() and same(out["gross"].to_numpy(), out["price"].to_numpy())
    zero = scen[(scen["spot_shock"] == 0.0) & (scen["vol_shock"] == 0.0)]
    assert len(zero) == 6 and (zero["pnl"] == 0.0).all()
    pipe = cp.CompleteOptimizedPipeline(cp.get_config(), data_dir=str(tmp_path), surface_backend=R.RefBackend())
    res = pipe.run_risk()
    assert res["success"] and res["risk_rows"] == 3 and res["scenario_rows"] == 270 and res["dead_options"] == 0
    assert set(res) == set(pipe.run_svi()) | {"risk_rows", "scenario_rows", "dead_options"}
    assert res["fitted_rows"] == pipe.run_svi()["fitted_rows"]
    # --book FILE: two contracts, one short
    path = tmp_path / "book.csv"
    pd.DataFrame({"symbol": [listed["symbol"][0], listed["symbol"][5]], "quantity": [2.0, -1.0]}).to_csv(path, index=False)
    assert cp.main(["--task", "risk", "--book", str(path), "--data-dir", str(tmp_path)], surface_backend=R.RefBackend()) == 0
    held = store.read_table("iv_risk", "btc")
    assert len(held) == 3 and not same(held["price"].to_numpy(), out["price"].to_numpy()) and (held["gross"] >= np.abs(held["price"])).all()
    pd.DataFrame({"symbol": ["btc-1jan30-1-c"], "quantity": [1.0]}).to_csv(path, index=False)
    assert cp.main(["--task", "risk", "--book", str(path), "--data-dir", str(tmp_path)], surface_backend=R.RefBackend()) == 1


def test_risk_task_with_a_book_on_one_of_two_underlyings(tmp_path):
    """An underlying without an option of the book gets no tables; a symbol listed twice and a quantity that is not a number
    are refused."""
    import complete_pipeline as cp
    store = FrameStore(str(tmp_path))
    chains = {u: synthetic_chain(u, expiry_days=(20, 45), strikes=tuple(np.linspace(17000.0, 34000.0, 6)), n_hours=3, seed=5 + n)
              for n, u in enumerate(("btc", "eth"))}
    for chain in chains.values():
        for f in chain:
            store.write_output(f["symbol"].iloc[0], f, 1)
    sym = chains["btc"][0]["symbol"].iloc[0]
    path = tmp_path / "book.csv"
    pd.DataFrame({"symbol": [sym], "quantity": [2.0]}).to_csv(path, index=False)

    class Watch(R.RefBackend):
        books = []

        def book(self, params, Tq, spot, rate, u, tau, qty, *rest):
            self.books.append(np.shape(u))
            return super().book(params, Tq, spot, rate, u, tau, qty, *rest)
    pipe = cp.CompleteOptimizedPipeline(cp.get_config(), data_dir=str(tmp_path), surface_backend=Watch())
    res = pipe.run_risk(str(path))
    assert res["success"] and res["underlyings"] == 2 and res["risk_rows"] == 3 and res["scenario_rows"] == 270
    assert all(shape[-1] == 1 for shape in Watch.books) and len(Watch.books) == 1          # never called with an empty book
    assert store.read_table("iv_risk", "eth") is None and store.read_table("iv_scenarios", "eth") is None
    out = store.read_table("iv_risk", "btc")
    assert len(out) == 3 and (out["n_dead"] == 0).all() and same(out["gross"].to_numpy(), out["price"].to_numpy())
    pd.DataFrame({"symbol": [sym, sym], "quantity": [1.0, 1.0]}).to_csv(path, index=False)
    assert "more than once" in pipe.run_risk(str(path))["error"]
    pd.DataFrame({"symbol": [sym], "quantity": ["many"]}).to_csv(path, index=False)
    assert "not a finite number" in pipe.run_risk(str(path))["error"]


def test_an_empty_book_is_worth_zero():
    """Q == 0: every sum, count and flag is 0, whatever the snapshot."""
    c = RC.MICRO["dead_queries"]                                              # its second snapshot has no live slice
    b = book(dict(c, u=c["u"][:0], tau=c["tau"][:0], qty=c["qty"][:0], is_put=None))
    assert b["net"].shape == (2, 8) and (b["net"] == 0.0).all() and (b["n_dead"] == 0).all()
    assert b["pnl_sm"].shape == (2, 9, 5) and (b["pnl_ss"] == 0.0).all() and (b["pnl_sm"] == 0.0).all() and not b["cell_flags"].any()


# ------------------------------------------------------------------ header, structs and bindings, field for field
def _header_fields(struct):
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ivs.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            m = re.fullmatch(r"(const\s+)?(\w+)\s*(\*?)\s*(\w+)", decl)
            assert m, decl
            fields.append((m.group(4), m.group(2), bool(m.group(3))))
    return src, fields


def test_header_structs_enums_and_bindings_agree():
    import ctypes as C
    import re
    from iv_interpolation_amd import _lib
    scalar = {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}
    for struct, bound, fn in (("ivs_greeks_args", _lib.GreeksArgs, "ivs_svi_greeks_f64"), ("ivs_book_args", _lib.BookArgs, "ivs_svi_book_f64")):
        src, fields = _header_fields(struct)
        assert [n for n, _, _ in fields] == [n for n, _ in bound._fields_]
        for (name, ctype, ptr), (_, have) in zip(fields, bound._fields_):
            if not ptr:
                assert have is scalar[ctype], name
            elif name in ("spot_shocks", "vol_shocks"):                       # host arrays
                assert have is C.POINTER(C.c_double) and ctype == "double", name
            else:
                assert have is C.c_void_p, name
        assert re.search(r"int\s+%s\(const %s\*[^,]*,\s*void\*[^,]*,\s*size_t[^,]*,\s*void\*[^)]*\);" % (fn, struct), src)
        res, args = _lib.SIGNATURES[fn]
        assert res is C.c_int and args == [C.POINTER(bound), C.c_void_p, C.c_size_t, C.c_void_p]
    sb = {k: int(v) for k, v in re.findall(r"(IVS_SB_\w+)\s*=\s*(\d+)", src)}
    assert sb == {"IVS_SB_NEG_VOL_SS": 1, "IVS_SB_NEG_VOL_SM": 2}
    assert (_lib.SB_NEG_VOL_SS, _lib.SB_NEG_VOL_SM) == (R.NEG_VOL_SS, R.NEG_VOL_SM) == (RC.NEG_VOL_SS, RC.NEG_VOL_SM) == (1, 2)
    assert re.search(r"#define\s+IVS_ABI_VERSION\s+5\b", src)


def test_c_abi_refusals_need_no_device():
    """Every refusal of the two entry points comes before anything touches the device: the pointers here are fakes."""
    import ctypes as C
    from iv_interpolation_amd import _lib
    lib = _lib.load()
    P = 64

    def greeks_args(**kw):
        a = _lib.GreeksArgs()
        for k in ("params", "Tq", "spot", "u", "tau", "flags"):
            setattr(a, k, kw.get(k, P))
        a.tq_stride, a.q_stride, a.mT, a.Q, a.B, a.strike_mode = kw.get("tq_stride", 0), kw.get("q_stride", 0), kw.get("mT", 16), kw.get("Q", 8), kw.get("B", 2), kw.get("strike_mode", 0)
        return a

    def book_args(sa=(0.0, 0.1), sv=(0.0,), **kw):
        a = _lib.BookArgs()
        for k in ("params", "Tq", "spot", "u", "tau", "qty", "net", "n_dead", "cell_flags"):
            setattr(a, k, kw.get(k, P))
        a.tq_stride, a.q_stride, a.mT, a.Q, a.B, a.strike_mode = kw.get("tq_stride", 0), kw.get("q_stride", 0), kw.get("mT", 16), kw.get("Q", 8), kw.get("B", 2), kw.get("strike_mode", 0)
        a.nA, a.nV, a.cells_per_wg = kw.get("nA", len(sa)), kw.get("nV", len(sv)), kw.get("cpw", 0)
        keep = ((C.c_double * max(len(sa), 1))(*sa), (C.c_double * max(len(sv), 1))(*sv))
        a.spot_shocks, a.vol_shocks = C.cast(keep[0], C.POINTER(C.c_double)), C.cast(keep[1], C.POINTER(C.c_double))
        return a, keep

    def refused(fn, a, code, word):
        assert fn(C.byref(a), None, 0, None) == code and word in lib.ivs_last_error() and lib.ivs_last_kernel() == b"", (code, word, lib.ivs_last_error())

    EINVAL, ERANGE = -22, -34
    g, b = lib.ivs_svi_greeks_f64, lib.ivs_svi_book_f64
    assert g(None, None, 0, None) == EINVAL and b(None, None, 0, None) == EINVAL
    refused(g, greeks_args(Q=-1), EINVAL, b"negative")
    refused(g, greeks_args(strike_mode=2), EINVAL, b"strike_mode")
    refused(g, greeks_args(mT=65), ERANGE, b"mT=65")
    refused(g, greeks_args(flags=None), EINVAL, b"null pointer")
    refused(g, greeks_args(q_stride=7), EINVAL, b"stride")
    refused(g, greeks_args(B=2 ** 31, Q=1), ERANGE, b"exceed")
    refused(g, greeks_args(B=2 ** 20, Q=2 ** 11), ERANGE, b"exceed")
    assert g(C.byref(greeks_args(Q=0)), None, 0, None) == 0 and g(C.byref(greeks_args(B=0)), None, 0, None) == 0      # no-ops
    for kw, code, word in ((dict(nA=-1), EINVAL, b"negative"), (dict(strike_mode=3), EINVAL, b"strike_mode"), (dict(mT=65), ERANGE, b"mT=65"),
                           (dict(sa=[0.0] * 33, sv=[0.0] * 32), ERANGE, b"cells"), (dict(sa=[0.0] * 65), ERANGE, b"per axis"),
                           (dict(sa=(0.0, -1.0)), ERANGE, b"spot shock 1"), (dict(sa=(float("nan"),)), ERANGE, b"spot shock 0"),
                           (dict(sv=(float("inf"),)), ERANGE, b"vol shock 0"), (dict(cpw=257), ERANGE, b"cells_per_wg"),
                           (dict(cell_flags=None), EINVAL, b"null pointer"), (dict(qty=None), EINVAL, b"null pointer"),
                           (dict(net=None), EINVAL, b"null pointer"), (dict(tq_stride=3), EINVAL, b"stride"),
                           (dict(B=2 ** 31, Q=1), ERANGE, b"exceed"), (dict(B=2 ** 30, Q=1, mT=1), ERANGE, b"cells exceed")):
        a, keep = book_args(**kw)
        refused(b, a, code, word)
    a, keep = book_args(B=0)
    assert b(C.byref(a), None, 0, None) == 0
