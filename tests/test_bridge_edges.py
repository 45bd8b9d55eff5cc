"""The IV -> OHLCV bridge and the MT19937 kernel at the boundaries of their launch geometry, scans, chains and rounding.
Inputs: bridge_edges_cases.py; references, tolerances and the comparison: bridge_edges_ref.py (oracle/bridge_oracle.py
for candles, Python's round for rounding, NumPy's RandomState for the stream).  Groups:
  1 more symbols than the candle kernel's grid       6 the rounding table (ties, near-ties, denormals, across 2^53 / 10^n)
  2 more than 256 scan blocks                        7 spread_simulation parameters (narrow-candle branch on / mixed / off)
  3 chunk boundaries and holes inside a chain        8 the generator: seeds, lengths around the state size, 8 M words
  4 trend_following stream state across three calls  9 the converter class across calls on the device
  5 the word buffer at exact fit
The CPU tests check the table and show that the comparisons reject wrong roundings and a chain that is not reset.
IVS_ERRLOG=<file> appends the largest difference and the share of differing cells of every comparison
(profiles/bridge_edges/errlog.txt is one such run)."""
import numpy as np
import pandas as pd
import pytest

import bridge_edges_cases as C
import bridge_edges_ref as R


# ---------------------------------------------------------------- CPU: the table
def _ok(b):
    return ~(np.isnan(b["price"]) | (b["price"] <= 0))


def _has_holes(b):
    p, v = b["price"], b["volume"]
    return np.isnan(p).any() and (p <= 0).any() and np.isnan(v).any() and (v <= 0).any() and _ok(b).any()


def test_case_table_layout():
    g = C.grid_batch()
    lens = np.diff(g["off"])
    assert len(lens) == C.GRID_S == 2221 and 55_000 <= lens.sum() <= 70_000 and _has_holes(g)
    assert (lens[::17] == 0).all() and lens.max() == 129
    ninth = np.setdiff1d(np.arange(0, C.GRID_S, 9), np.arange(0, C.GRID_S, 17))
    assert all((lens[ninth] == n).sum() >= 30 for n in C.CHUNK_LENS)
    rest = np.setdiff1d(np.arange(C.GRID_S), np.arange(0, C.GRID_S, 9))
    assert lens[rest].max() <= 40 and lens[2048:].sum() > 3000          # the second trip of the grid loop has rows to do
    s = C.scan_batch()
    lens = np.diff(s["off"])
    assert lens.sum() == 256 * 1024 + 1500 and len(lens) == 40 and (lens == 0).sum() == 1 and lens.max() == 100_000
    assert _has_holes(s) and -(-int(lens.sum()) // 1024) > 256
    assert all(0 < C.words_consumed(s, k) < 2 ** 31 for k in (1, 3))
    c = C.chain_batch()
    lens = np.diff(c["off"])
    assert list(lens) == list(C.CHAIN_LENS) * len(C.CHAIN_PATTERNS) and lens.sum() == 6930
    ok = _ok(c)
    for i, (pat, n) in enumerate((pat, n) for pat in C.CHAIN_PATTERNS for n in C.CHAIN_LENS):
        a = int(c["off"][i])
        assert np.array_equal(~ok[a:a + n], C.chain_invalid(pat, n)), (pat, n)
    i = C.CHAIN_PATTERNS.index("chunk1_invalid") * len(C.CHAIN_LENS) + C.CHAIN_LENS.index(193)
    a = int(c["off"][i])
    assert ok[a:a + 64].all() and not ok[a + 64:a + 128].any() and ok[a + 128:a + 193].all()
    i = C.CHAIN_PATTERNS.index("first_at_63") * len(C.CHAIN_LENS) + C.CHAIN_LENS.index(129)
    a = int(c["off"][i])
    assert not ok[a:a + 63].any() and ok[a + 63]
    f = C.fit_batch()
    assert 2500 <= len(f["price"]) <= 3500 and _has_holes(f) and _ok(f)[-1] and np.isnan(f["volume"][-1])
    rb = C.rounding_batch()
    assert _ok(rb).all() and len(rb["price"]) == len(rb["volume"]) == rb["off"][-1] and not np.isinf(rb["price"]).any()
    assert np.array_equal(rb["volume"][-len(C.VOLUME_EDGE_CELLS):], C.VOLUME_EDGE_CELLS, equal_nan=True)
    assert np.isin(C.rounding_values(4), rb["price"]).all() and np.isin(C.rounding_values(6), rb["volume"]).all()
    pb = C.param_batch()
    assert len(pb["price"]) == 2000 and np.isnan(pb["price"]).any() and np.isnan(pb["volume"]).any()
    assert [len(b["price"]) for b in C.converter_batches()] == [3000, 3100, 2900]


@pytest.mark.parametrize("pending", [False, True])
def test_trend_calls_end_in_the_stated_parity(pending):
    c1, c2, c3 = C.trend_calls(pending)
    ok = _ok(c1)
    assert len(ok) >= 20_000 and ok[:64].sum() == 63 and ok.sum() % 2 == int(pending) and _has_holes(c1)
    assert not _ok(c2).any() and len(c2["off"]) == 4
    first = int(np.flatnonzero(_ok(c3))[0])
    assert first > 0 and np.isnan(c3["volume"][first])
    rs = np.random.RandomState(C.SEED)
    R.stream_reference([c1], R.TREND, rs)
    assert rs.get_state()[3] == int(pending)                 # the oracle's generator holds a cached deviate, or not
    assert ok.sum() > 16384      # two valid rows share an attempt of two doubles: the walk refills its 16 384-flag window


def test_stream_helpers_position_a_generator_by_words():
    fresh = np.random.RandomState(C.SEED)
    assert R.same_stream_position(R.state_after(C.SEED, 0, 0, 0.0), fresh)
    fresh.random_sample(7)                                       # 14 words
    assert R.same_stream_position(R.state_after(C.SEED, 14, 0, 0.0), fresh)
    assert not R.same_stream_position(R.state_after(C.SEED, 12, 0, 0.0), fresh)
    assert R.state_after(C.SEED, 14, 1, 0.25).get_state()[3:] == (1, 0.25)


def test_param_cases_take_the_narrow_branch_or_not():
    """On the oracle's outputs.  pct 0.0004 with vol_factor 0.5: spread = 0.0002 base, high - low <= spread (2/3 + 1) plus
    0.3 of the trend bias < 0.0005 base: every candle is narrow.  pct 0.05: spread >= 0.025 base, none is.  A larger
    vol_factor at 0.0004 lets spread reach 0.0012 base: both branches."""
    b = C.param_batch()
    ok = _ok(b)
    for pct in C.SPREAD_PCTS:
        for vf in C.VOL_FACTORS:
            _, out = R.oracle("param", b, 0, base_spread_pct=pct, vol_factor=vf)
            width, floor = (out[1] - out[2])[ok], 0.0005 * b["price"][ok]
            narrow = np.abs(width - floor) <= 1.0e-4 + 1e-9          # high and low are each rounded to 1e-4
            assert (width >= floor - (1.0e-4 + 1e-9)).all()
            if pct == 0.0004 and vf == 0.5:
                assert narrow.all()
            elif pct == 0.0004:
                assert narrow.sum() > 100 and (~narrow).sum() > 100, (pct, vf)
            elif pct == 0.05:
                assert not narrow.any() and (width > 2 * floor).all()


@pytest.mark.parametrize("nd", C.ROUND_DIGITS)
def test_rounding_table_holds_each_kind(nd):
    t, p10 = C.rounding_table(nd), 10 ** nd
    for kind, sign in (("tie_pos", 1), ("tie_neg", -1), ("tie_zero", 0)):
        x = t[kind]
        p = x * p10
        m = np.floor(p)
        assert len(x) >= (5 if sign == 0 else 50) and (p - m == 0.5).all(), kind     # the float product is an exact .5
        assert all(C.product_residual_sign(float(v), p10) == sign for v in x), kind
        assert (m % 2 == 0).sum() >= 5 and (m % 2 == 1).sum() >= 5, kind
    assert 0.03125 in C.rounding_table(4)["tie_zero"]
    x = t["near_tie"]
    p = x * p10
    off = np.abs(p - (np.floor(p) + 0.5))
    assert len(x) >= 50 and (off == np.spacing(p)).all()
    lo = 2.0 ** 53 / p10
    assert (t["cross"] < lo).sum() >= 90 and (t["cross"] >= lo).sum() >= 90
    assert t["cross"].min() <= lo / 3.9 and t["cross"].max() >= lo * 3.9
    assert {5e-324, float(f"5e-{nd + 1}")} <= set(t["small"]) and {1e15, 1e300, 1e305} <= set(t["big"])


@pytest.mark.parametrize("nd", C.ROUND_DIGITS)
def test_rounding_table_accepts_the_shipped_formula_and_rejects_wrong_ones(nd):
    assert len(R.rounding_violations(nd)) == 0
    n_ties = sum(len(C.rounding_table(nd)[k]) for k in ("tie_pos", "tie_neg", "tie_zero"))
    before = R.rounding_violations(nd, threshold=False)                  # the formula before the 2^53 rule
    assert len(before) > 0 and (before >= n_ties).all()                  # ... is right on every tie, wrong beyond 2^53
    big = len(C.rounding_values(nd)) - 1
    assert big in before                                                 # 1e305: the product overflows
    for tie in ("none", "half_away"):
        assert len(R.rounding_violations(nd, tie=tie, threshold=False)) > len(before)
        bad = R.rounding_violations(nd, tie=tie)                         # with the 2^53 rule it is the ties that tell (and the
        assert (bad < n_ties).sum() >= 50, tie                           # products in [2^51, 2^52), half of which end in .5)


@pytest.mark.parametrize("strategy", [0, 2])
def test_chain_that_is_not_reset_fails_groups_1_and_3(strategy):
    for key, b in (("grid", C.grid_batch()), ("chain", C.chain_batch())):
        rv, ro = R.oracle(key, b, strategy)
        assert R.violations(key, ro, rv, rv, ro, b, strategy, log=False) == []
        wv, wo = R.oracle_chain_not_reset(b, strategy)
        bad = R.violations(key, wo, wv, rv, ro, b, strategy, log=False)
        assert bad and all("valid" not in m and "volume" not in m for m in bad), (key, bad)    # only the chained prices


def test_comparison_rejects_single_cell_changes():
    b = C.chain_batch()
    rv, ro = R.oracle("chain", b, 0)
    row = int(np.flatnonzero(rv & ~R.drawn_mask(b))[5])
    for j, delta, caught in ((3, 1e-4, True), (4, 1e-6, True), (5, 1e-12, True), (0, 0.0, False)):
        out = ro.copy(); out[j, row] += delta
        assert bool(R.violations("x", out, rv, rv, ro, b, 0, log=False)) == caught, j
    drawn = int(np.flatnonzero(rv & R.drawn_mask(b))[5])
    out = ro.copy(); out[4, drawn] += 1e-6
    assert R.violations("x", out, rv, rv, ro, b, 0, log=False) == []
    out[4, drawn] += 2e-6
    assert R.violations("x", out, rv, rv, ro, b, 0, log=False)
    v = rv.copy(); v[row] = False
    assert R.violations("x", ro, v, rv, ro, b, 0, log=False)
    _, rt = R.oracle("chain", b, R.TREND)
    out = rt.copy(); out[3, row] += 1.5e-4
    assert R.violations("x", out, rv, rv, rt, b, R.TREND, log=False) == []
    out[3, row] += 1.5e-4
    assert R.violations("x", out, rv, rv, rt, b, R.TREND, log=False)


# ---------------------------------------------------------------- GPU
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def stream():
    """The first 2 M words of the stream of C.SEED on the device (the largest batch consumes 1.4 M)."""
    from iv_interpolation_amd import engine
    return engine.mt19937_words(C.SEED, 2_000_000)


def _run(b, strategy, words, tail=None, **kw):
    """(out [6, n], valid [n], rng_tail [4]) on the host."""
    import torch
    from iv_interpolation_amd import engine
    out, valid, tail = engine.bridge_candles(_dev(b["price"]), _dev(b["volume"]), _dev(b["off"]), strategy, words, tail, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), valid.cpu().numpy(), tail.cpu().numpy()


def _ample(stream, b, strategy):
    from iv_interpolation_amd import engine
    return stream[:engine.bridge_words_bound(len(b["price"]), strategy)]


@pytest.mark.gpu
@pytest.mark.parametrize("strategy", [0, 2, 3])
def test_gpu_more_symbols_than_the_grid(stream, strategy):
    import torch
    S = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 173
    b = C.grid_batch(S)
    out, valid, tail = _run(b, strategy, _ample(stream, b, strategy))
    assert tail[3] == 0
    rv, ro = R.oracle("grid" if S == C.GRID_S else f"grid{S}", b, strategy)
    assert R.violations(f"1 grid S={S} strategy {strategy}", out, valid, rv, ro, b, strategy) == []


@pytest.mark.gpu
@pytest.mark.parametrize("strategy", [1, 3])
def test_gpu_more_than_256_scan_blocks(stream, strategy):
    b = C.scan_batch()
    out, valid, tail = _run(b, strategy, _ample(stream, b, strategy))
    assert tail[3] == 0 and tail[0] == C.words_consumed(b, strategy)
    rv, ro = R.oracle("scan", b, strategy)
    assert R.violations(f"2 scan strategy {strategy}", out, valid, rv, ro, b, strategy) == []


@pytest.mark.gpu
@pytest.mark.parametrize("strategy", [0, 2, 4])
def test_gpu_chunk_boundaries_and_holes_in_the_chain(stream, strategy):
    b = C.chain_batch()
    out, valid, tail = _run(b, strategy, _ample(stream, b, strategy))
    assert tail[3] == 0
    rv, ro = R.oracle("chain", b, strategy)
    bad = R.violations(f"3 chain strategy {strategy}", out, valid, rv, ro, b, strategy)
    assert bad == [], (bad, [(s, b["pattern"][s], int(b["off"][s + 1] - b["off"][s])) for s in range(len(b["pattern"]))
                             if not np.array_equal(out[:, b["off"][s]:b["off"][s + 1]], ro[:, b["off"][s]:b["off"][s + 1]],
                                                   equal_nan=True)][:8])


@pytest.mark.gpu
@pytest.mark.parametrize("pending", [False, True])
def test_gpu_trend_stream_state_across_three_calls(stream, pending):
    """The reference of every call is a RandomState advanced by the words the device reports consumed, holding the cached
    deviate it returned; next to it one generator runs through the three calls untouched by the device, and position, cache
    flag and cached deviate must agree with it.  Cached deviate: sqrt(-2 log(r2) / r2) x1 with the device's log against
    libm's (1 ulp each, halved by the square root, plus division, sqrt and product at half an ulp each): below 4 ulps;
    8 ulps allowed."""
    import torch
    calls = C.trend_calls(pending)
    through = np.random.RandomState(C.SEED)
    pos, tail, bad = 0, np.zeros(4, np.int64), []
    for i, b in enumerate(calls):
        t_in = torch.tensor([0, int(tail[1]), int(tail[2]), 0], dtype=torch.int64).cuda()
        has_in, gauss_in = int(tail[1]), float(np.int64(tail[2]).view(np.float64))
        out, valid, tail = _run(b, R.TREND, _ample(stream[pos:], b, R.TREND), t_in)
        assert tail[3] == 0
        (rv, ro), = R.stream_reference([b], R.TREND, R.state_after(C.SEED, pos, has_in, gauss_in))
        bad += R.violations(f"4 trend pending={int(pending)} call {i + 1}", out, valid, rv, ro, b, R.TREND)
        (tv, to), = R.stream_reference([b], R.TREND, through)
        bad += R.violations(f"4 trend pending={int(pending)} call {i + 1} (one generator)", out, valid, tv, to, b, R.TREND, log=False)
        if i == 0:
            assert tail[1] == int(pending)
        if i == 1:
            assert tail[0] == 0 and tail[1] == has_in and tail[2] == t_in.cpu().numpy()[2]
        pos += int(tail[0])
        st = through.get_state()
        assert tail[1] == st[3] and R.same_stream_position(R.state_after(C.SEED, pos, 0, 0.0), through), i
        if st[3]:
            got = float(np.int64(tail[2]).view(np.float64))
            print(f"call {i + 1}: cached deviate {got!r} against {st[4]!r}")
            assert abs(got - st[4]) <= 8 * np.spacing(abs(st[4])), i
        else:
            assert tail[2] == 0
    assert bad == []


@pytest.mark.gpu
@pytest.mark.parametrize("strategy", [0, 1, 2, 3, 4])
def test_gpu_word_buffer_at_exact_fit(stream, strategy):
    b = C.fit_batch()
    n = len(b["price"])
    ample = _ample(stream, b, strategy)
    out, valid, tail = _run(b, strategy, ample)
    used = int(tail[0])
    assert tail[3] == 0 and 0 < used < ample.numel() - 2
    if strategy != R.TREND:
        assert used == C.words_consumed(b, strategy)
    rv, ro = R.oracle("fit", b, strategy)
    assert R.violations(f"5 fit strategy {strategy}", out, valid, rv, ro, b, strategy) == []
    out2, valid2, tail2 = _run(b, strategy, stream[:used])             # exactly the words consumed suffice
    assert tail2[3] == 0 and np.array_equal(tail2, tail)
    assert np.array_equal(out2.view(np.int64), out.view(np.int64)) and np.array_equal(valid2, valid)
    _, _, tail3 = _run(b, strategy, stream[:used - 2])                 # one double short
    assert tail3[3] == 1
    if strategy == R.TREND:                                            # more words than acceptance flags fit: the clamp
        assert ample.numel() // 2 <= C.acc_capacity(n) and used // 2 <= C.acc_capacity(n)
        out4, valid4, tail4 = _run(b, strategy, stream[:2 * C.acc_capacity(n) + 1001])
        assert np.array_equal(tail4, tail)
        assert np.array_equal(out4.view(np.int64), out.view(np.int64)) and np.array_equal(valid4, valid)


@pytest.mark.gpu
def test_gpu_rounding_table(stream):
    """open = round(price, 4) and the passed-through volume = round(volume, 6) are Python's round of the table itself; high,
    low and close go through the same rounding."""
    b = C.rounding_batch()
    out, valid, tail = _run(b, 3, _ample(stream, b, 3))
    assert tail[3] == 0 and valid.all()
    passed = ~R.drawn_mask(b)
    wrong_open = out[0].view(np.int64) != R.python_round(b["price"], 4).view(np.int64)
    wrong_vol = out[4][passed].view(np.int64) != R.python_round(b["volume"][passed], 6).view(np.int64)
    rv, ro = R.oracle("rounding", b, 3)
    bad = R.violations("6 rounding", out, valid, rv, ro, b, 3)
    n_bad = int(wrong_open.sum() + wrong_vol.sum())
    assert n_bad == 0 and bad == [], (f"{n_bad} of {len(wrong_open) + len(wrong_vol)} table cells differ from Python's round",
                                      [(float(x), float(g)) for x, g in zip(b["price"][wrong_open][:5], out[0][wrong_open][:5])], bad)


@pytest.mark.gpu
@pytest.mark.parametrize("pct", C.SPREAD_PCTS)
@pytest.mark.parametrize("vf", C.VOL_FACTORS)
def test_gpu_spread_simulation_parameters(stream, pct, vf):
    b = C.param_batch()
    out, valid, tail = _run(b, 0, _ample(stream, b, 0), base_spread_pct=pct, vol_factor=vf)
    assert tail[3] == 0
    rv, ro = R.oracle("param", b, 0, base_spread_pct=pct, vol_factor=vf)
    assert R.violations(f"7 spread pct={pct} vol_factor={vf}", out, valid, rv, ro, b, 0) == []


@pytest.mark.gpu
def test_gpu_mt19937_seeds_lengths_and_a_long_stream():
    from iv_interpolation_amd import engine
    for seed in C.MT_SEEDS:
        ref = R.BO.mt19937_words(seed, max(C.MT_LENGTHS))
        for n in C.MT_LENGTHS:
            w = engine.mt19937_words(seed, n).cpu().numpy().view(np.uint32)
            assert w.shape == (n,) and np.array_equal(w, ref[:n]), (seed, n)
    seed, n = C.MT_LONG
    w = engine.mt19937_words(seed, n).cpu().numpy().view(np.uint32)
    ref = R.BO.mt19937_words(seed, n)
    assert np.array_equal(w, ref), int(np.flatnonzero(w != ref)[0])
    for seed in C.MT_BAD_SEEDS:
        with pytest.raises(ValueError):
            engine.mt19937_words(seed, 4)


def _config(strategy):
    import config as cfgmod
    cfg = cfgmod.get_config()
    cfg.data_bridge.conversion_strategy = strategy
    return cfg


@pytest.mark.gpu
@pytest.mark.parametrize("strategy", ["spread_simulation", "trend_following"])
def test_gpu_converter_across_calls(strategy):
    """Three calls of the class on its default (HIP) backend against ONE oracle stream over the three frames; the word
    cache of the backend has to grow for the second frame."""
    from iv_interpolation_amd.bridge import InterpolatedToOHLCVConverter
    code = R.BO.strategy_code(strategy)
    batches = C.converter_batches()
    refs = R.stream_reference(batches, code, np.random.RandomState(C.SEED))
    c = InterpolatedToOHLCVConverter(None, _config(strategy), seed=C.SEED)
    bad, sizes = [], []
    for i, (b, (rv, ro)) in enumerate(zip(batches, refs)):
        n = len(b["price"])
        df = pd.DataFrame({"symbol": [f"SYM{i}"] * n, "timestamp": pd.date_range("2024-01-01", periods=n, freq="1min"),
                           "mark_price": b["price"], "volume": b["volume"]})
        res, = c.convert_frames([df])
        sizes.append(c._backend._words.numel())
        assert res is not None and len(res) == int(rv.sum()), i
        assert np.array_equal(res["timestamp"].to_numpy(), df["timestamp"].to_numpy()[rv])
        out = np.full((6, n), np.nan)
        for j, k in enumerate(R.COLS):
            out[j, rv] = res[k].to_numpy(np.float64)
        bad += R.violations(f"9 converter {strategy} frame {i + 1}", out, rv, rv, ro, b, code)
    assert sizes[1] > sizes[0]
    assert bad == []
