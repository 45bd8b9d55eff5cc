"""Layouts that put every block form of the 1-D kernels and of the fused frame pass under every method.  TEST INPUTS ONLY
(NumPy, importable without a GPU).

``layout_m`` serves the twelve non-polynomial methods, ``layout_p`` 'barycentric' / 'krogh' (at most 32 knots per series, one
series beyond that), ``layout_long`` is the single series of 70 000 knots.  A layout is a dict of ``src_off`` / ``q_off`` [S+1],
``pos`` [n_src] (source positions = output rows within the symbol), ``yk`` [3, n_src] (NaN = no quote), ``tags`` [S].
``fill_columns`` draws the validity rows and forward-filled columns of a frame case (shared with test_gpu_parity.py).

``forms(layout, method)`` mirrors on the host the block-uniform predicates by which interp1d_prepare_kernel,
interp1d_eval_kernel and frame_fused_kernel choose where a block reads its knots from; the constants below are mirrored from
csrc/ivs_interp1d.hpp, csrc/ivs_frame.hpp and include/ivs.h (test_interp1d_forms.py compares them with the headers)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import ivs_oracle as O  # noqa: E402

P1_STAGE = 512          # prepare: valid knots of a (series, channel) whose slope solve runs out of LDS
E1_STAGE = 512          # eval: staged knots per block and channel
E1_ROWS = 1024          # eval: output rows per block
FR_ROWS = 4096          # frame pass: output rows per block
FR_CAP = 208            # frame pass: staged source rows per block
FR_MAXSYM = 64
FR_MAXKNOTS = 65535     # frame pass: source rows of a symbol on the window form
FR_MAXV, FR_MAXC, FR_MAXF, FR_MAXCC = 16, 3, 8, 4
POLY_MAX_KNOTS = 32
WAVE = 64               # knots per scan block of the not-a-knot solve

METHODS = ("linear", "cubic", "cubicspline", "slinear", "nearest", "zero", "pchip", "akima", "from_derivatives", "quadratic",
           "barycentric", "krogh", "pad", "bfill")                                   # in the order of their codes 0..13
POLY = ("barycentric", "krogh")
MIN_KNOTS = {"linear": 0, "cubic": 4, "cubicspline": 2, "slinear": 2, "nearest": 1, "zero": 1, "pchip": 2, "akima": 3,
             "from_derivatives": 2, "quadratic": 3, "barycentric": 1, "krogh": 1, "pad": 0, "bfill": 0}
SOLVED = ("cubic", "cubicspline", "pchip", "akima", "quadratic")                     # methods with a slope / coefficient solve
EXACT = ("linear", "nearest", "zero", "from_derivatives", "pad", "bfill")             # bit-exact against the oracle
SEED = 20250107
SPARSE = np.array([0, 1000, 10000, 11000, 20000])      # 5 knots; gaps beyond two frame-pass blocks: blocks without a source row


# ------------------------------------------------------------------------------------------------ layouts
class _Layout:
    def __init__(self, seed):
        self.r = np.random.default_rng(seed)
        self.pos, self.mask, self.m, self.tags = [], [], [], []

    @property
    def rows(self):
        return int(sum(self.m))

    def add(self, tag, pos, tail=3, nan=None, rows=None):
        """One symbol: source positions `pos`, `tail` output rows behind the last one (or `rows` in all); nan = {channel: bool
        [n] of the knots WITHOUT a quote}."""
        pos = np.asarray(pos, np.int64)
        mask = np.zeros((3, pos.size), bool)
        for c, v in (nan or {}).items():
            mask[c] = v
        self.pos.append(pos); self.mask.append(mask); self.tags.append(tag)
        self.m.append(int(rows) if rows is not None else int(pos[-1]) + 1 + tail)

    def even(self, n, gap, start=0):
        return start + gap * np.arange(n, dtype=np.int64)

    def drawn(self, n, lo, hi):
        g = self.r.integers(lo, hi + 1, n); g[0] = 0
        return np.cumsum(g)

    def some(self, n, frac=0.15):
        return self.r.random(n) < frac

    def tiny_run(self, tag, count):
        """`count` symbols of 1..5 knots, 1..3 rows apart (consecutive positions included), 3..5 rows behind the last knot"""
        for k in range(count):
            n = (1, 2, 3, 1, 2, 4, 1, 2, 5, 1)[k % 10]
            nan = {k % 3: np.arange(n) == 0} if k % 7 == 3 else None             # some lose their first knot in one channel
            self.add(tag, self.drawn(n, 1, 3), tail=3 + k % 3, nan=nan)

    def aligned(self, tag, pos, at):
        """a symbol whose successor starts `at` rows into a frame-pass block"""
        base = int(pos[-1]) + 4
        self.add(tag, pos, rows=base + (at - (self.rows + base)) % FR_ROWS)

    def finish(self):
        sizes = np.array([p.size for p in self.pos])
        src_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        q_off = np.concatenate([[0], np.cumsum(self.m)]).astype(np.int64)
        pos = np.concatenate(self.pos)
        ks = np.repeat(np.arange(sizes.size), sizes)
        t = pos.astype(np.float64)
        # slowly varying curves (iv, underlying, time to maturity) + noise of 1e-3 relative: the splines stay well conditioned
        yk = np.stack([0.6 + 0.15 * np.sin(t / 700.0 + ks), 25000.0 + 400.0 * np.sin(t / 1500.0 + 0.3 * ks), 0.08 + 1e-3 * (ks % 5) - t * 1e-6])
        yk *= 1.0 + 1e-3 * self.r.standard_normal(yk.shape)
        yk[np.concatenate(self.mask, axis=1)] = np.nan
        return {"src_off": src_off, "q_off": q_off, "pos": pos, "yk": yk, "tags": list(self.tags), "sizes": sizes}


@functools.lru_cache(maxsize=None)
def layout_m():
    L = _Layout(SEED)
    n = 64
    idx = np.arange(n)
    L.add("ref", L.even(n, 60))
    L.add("ref_lead", L.even(n, 60), nan={0: idx < 5})                                   # leading NaNs
    L.add("ref_trail", L.even(n, 60), nan={1: idx >= n - 6})                             # trailing NaNs
    L.add("ref_random", L.even(n, 60), nan={2: L.some(n)})                               # ~15 % NaNs
    L.add("ref_no0", L.even(n, 60), nan={0: idx >= 0})                                   # channel 0 without any knot
    L.add("ref_no1", L.even(n, 60), nan={1: idx >= 0})                                   # channel 1 without any knot
    L.add("ref_at3", L.even(n, 60, start=3))                                             # first source row at position 3
    L.add("ref_few", L.even(n, 60), nan={0: idx % 21 != 1, 1: idx % 40 != 7, 2: idx != 30})      # 3 / 2 / 1 valid knots
    g = np.full(n, 60); g[0] = 0; g[[9, 10, 33, 63]] = 1                                 # consecutive positions (duplicate-style)
    L.add("ref_consecutive", np.cumsum(g))
    L.add("long400", L.drawn(420, 25, 40), nan={0: L.some(420), 1: np.arange(420) < 3})  # window form; LDS solve over 7 scan blocks
    L.add("ref", L.even(n, 60))
    L.add("dense1200", L.drawn(1200, 2, 5), nan={0: np.arange(1200) < 5, 1: np.arange(1200) >= 1193, 2: L.some(1200)})     # > 512 valid knots
    for k, cnt in enumerate((280, 290, 270)):                                            # neighbours with n1 + n2 > 512
        L.add("mid%d" % cnt, L.drawn(cnt, 3, 7), nan={k: L.some(cnt, 0.05)})
    for _ in range(2):                                                                   # blocks without a source row, then > 64 symbols in one block
        L.aligned("sparse", SPARSE, at=256)
        L.tiny_run("tiny", 72)
    L.aligned("sparse", SPARSE, at=0)
    L.add("ref", L.even(n, 60))
    return L.finish()


@functools.lru_cache(maxsize=None)
def layout_p():
    L = _Layout(SEED + 1)
    for k in range(9):                                                                   # whole form; one- and two-series eval blocks
        n = (30, 8, 17, 25, 32, 10, 30, 12, 31)[k]
        L.add("hourly", L.even(n, 1800 // n), nan={k % 3: np.arange(n) == 2} if k % 2 else None)
    # (one polynomial through 25+ knots is not continued over missing END knots here: three intervals outside the hull the
    # oracle's own two routes, barycentric and Newton form, differ by more than the bound the tests compare at)
    L.add("hourly_lead", L.even(12, 150), nan={0: np.arange(12) < 3, 2: np.arange(12) >= 10})
    for k in range(20):                                                                  # 7-8 symbols per block: window form through spacing
        L.add("spaced", L.even(30, 22), nan={k % 3: np.isin(np.arange(30), (0, 7 + k))} if k % 4 == 1 else None)
    L.add("too_many", L.even(40, 60), nan={2: np.arange(40) % 2 == 1})                   # 40 / 40 / 20 knots: ill-conditioned, ok
    for _ in range(2):
        L.aligned("sparse", SPARSE, at=256)
        L.tiny_run("tiny", 72)
    L.aligned("sparse", SPARSE, at=0)
    L.add("hourly", L.even(30, 60))
    return L.finish()


def layout_long(dense):
    """one series of 70 000 valid knots: 20..24 rows apart (every block of the frame pass takes the window form) or 1..2 apart"""
    L = _Layout(SEED + (3 if dense else 2))
    L.add("dense" if dense else "window", L.drawn(70000, *((1, 2) if dense else (20, 24))))
    return L.finish()


def fill_columns(r, n_src, S):
    """validity rows, forward-filled f64 / code columns, host-gathered rows, dates, `needs` and the Greek inputs of a frame case"""
    nV = 9
    valid = (r.random((nV, n_src)) > 0.3).astype(np.uint8); valid[4] = 0; valid[5] = 1
    fsrc = r.normal(size=(5, n_src)); f_rows = np.array([1, 2, 3, 4, 5], np.int32)
    csrc = r.integers(0, 50, (2, n_src)).astype(np.int32); c_rows = np.array([0, 6], np.int32)
    host_rows = np.array([7, 8], np.int32)
    first_ns = (r.integers(0, 10**6, S) * 60_000_000_000).astype(np.int64)
    needs = (r.random((S, 3)) < 0.7).astype(np.uint8)
    gvalid = (r.random((3, n_src)) > 0.2).astype(np.uint8)
    ksrc = r.uniform(20000, 30000, n_src); rsrc = r.uniform(0, 0.05, n_src); psrc = r.integers(0, 3, n_src).astype(np.uint8)
    return {"valid": valid, "fsrc": fsrc, "f_rows": f_rows, "csrc": csrc, "c_rows": c_rows, "host_rows": host_rows,
            "first_ns": first_ns, "needs": needs, "gvalid": gvalid, "ksrc": ksrc, "rsrc": rsrc, "psrc": psrc}


def frame_case(layout, seed=SEED + 9):
    S = len(layout["src_off"]) - 1
    return dict(layout, **fill_columns(np.random.default_rng(seed), int(layout["src_off"][-1]), S))


def off_lattice_queries(layout):
    """Explicit queries with the lattice's counts per series (so the eval kernel takes the same forms): rows on a source position
    stay there, the others move off the lattice by a fraction, the last two rows of a series (behind every knot: tail >= 3) go
    below its first and above its last knot."""
    q_off, src_off, pos = layout["q_off"], layout["src_off"], layout["pos"]
    total = int(q_off[-1])
    s = np.repeat(np.arange(len(q_off) - 1), np.diff(q_off))
    row = np.arange(total) - q_off[:-1][s]
    xq = row + 0.05 + 0.9 * ((np.arange(total) * 0.6180339887498949) % 1.0)
    gpos = q_off[:-1][np.repeat(np.arange(len(src_off) - 1), np.diff(src_off))] + pos
    xq[gpos] = pos
    xq[q_off[1:] - 2] = -1.5
    xq[q_off[1:] - 1] = pos[src_off[1:] - 1] + 2.25
    return xq


# ------------------------------------------------------------------------------------------------ the oracle on a layout
def knot_counts(layout, method, C=3):
    """(valid knots [S, C], the count the eval kernels see [S, C]: 0 where a polynomial is refused)"""
    ok = ~np.isnan(layout["yk"][:C])
    cs = np.concatenate([np.zeros((C, 1), np.int64), np.cumsum(ok, axis=1)], axis=1)
    n = (cs[:, layout["src_off"][1:]] - cs[:, layout["src_off"][:-1]]).T
    return n, np.where((n > POLY_MAX_KNOTS) & (method in POLY), 0, n)


def oracle(layout, method, xq=None, yk=None):
    yk = layout["yk"] if yk is None else yk
    return O.interp1d_batch(layout["pos"].astype(np.float64), yk, layout["src_off"], xq, layout["q_off"], O.METHOD_CODES[method])


def merged_reference(layout, method, xq=None, C=3):
    """The oracle's interpolant with the source cell at every row that IS a knot of its channel (the kernels' `out` is the merged
    column of the reference's frame), except in series whose polynomial is refused (> 32 knots: all NaN)."""
    ref, st = oracle(layout, method, xq, layout["yk"][:C])
    S = len(layout["src_off"]) - 1
    ks = np.repeat(np.arange(S), layout["sizes"])
    gpos = layout["q_off"][:-1][ks] + layout["pos"]
    for c in range(C):
        y = layout["yk"][c]
        okk = ~np.isnan(y) & (st[ks, c] != O.ST_ILL_CONDITIONED)
        if xq is not None:
            okk &= xq[gpos] == layout["pos"]
        ref[c, gpos[okk]] = y[okk]
    return ref, st


# ------------------------------------------------------------------------------------------------ block forms
def forms(layout, method, C=3, n_valid=12, n_f=5, n_c=2, greeks=True):
    """The form every block of the three kernels takes:
    prepare [S][C]: 'none' (nothing to solve), 'table' (polynomial weights), 'scan' (not-a-knot, >= 4 knots, wavefront scans in
        LDS), 'thread' (one thread in LDS), 'global' (more than P1_STAGE knots: one thread on the global arrays);
    eval [blocks][C]: (form, n1, n2) with form 'one' / 'two' (staged), 'one_big' / 'two_big' (knots do not fit), 'one_empty' /
        'two_empty' (no knot at all), 'multi' (three or more series);
    frame [blocks]: dict(form = 'whole' | 'window' | 'perrow', why = '' | 'rows' | 'nsym' | 'columns', s_first, s_last)."""
    src_off, q_off, pos = layout["src_off"], layout["q_off"], layout["pos"]
    S, total_q = len(src_off) - 1, int(q_off[-1])
    n, wn = knot_counts(layout, method, C)
    series_of = lambda g: int(np.searchsorted(q_off, g, side="right")) - 1          # noqa: E731

    def prep(base):
        if method in POLY:
            return "table" if 1 <= base <= POLY_MAX_KNOTS else "none"
        if method not in SOLVED or base < MIN_KNOTS[method] or base < 2:
            return "none"
        if base > P1_STAGE:
            return "global"
        return "scan" if method in ("cubic", "cubicspline") and base >= 4 else "thread"
    prepare = [[prep(int(n[s, c])) for c in range(C)] for s in range(S)]

    ev = []
    for g0 in range(0, total_q, E1_ROWS):
        s1, s2 = series_of(g0), series_of(min(g0 + E1_ROWS, total_q) - 1)
        per = []
        for c in range(C):
            n1, n2 = int(wn[s1, c]), int(wn[s2, c]) if s2 == s1 + 1 else 0
            if s2 > s1 + 1:
                per.append(("multi", n1, 0))
            else:
                kind = "one" if s1 == s2 else "two"
                per.append((kind + ("" if 0 < n1 + n2 <= E1_STAGE else "_empty" if n1 + n2 == 0 else "_big"), n1, n2))
        ev.append(per)

    fr = []
    gpos = q_off[:-1][np.repeat(np.arange(S), layout["sizes"])] + pos                # output row of every source row
    for g0 in range(0, total_q, FR_ROWS):
        g_last = min(g0 + FR_ROWS, total_q) - 1
        s1, s2 = series_of(g0), series_of(g_last)
        nsym = min(s2 - s1 + 1, FR_MAXSYM + 1)
        W0, W1 = int(src_off[s1]), int(src_off[s2 + 1])
        whole = W1 - W0 <= FR_CAP
        if not whole:
            for last, s, g in ((0, s1, g0), (1, s2, g_last)):
                a, cnt = int(src_off[s]), int(src_off[s + 1] - src_off[s])
                x0 = int(np.searchsorted(pos[a:a + cnt], g - q_off[s], side="right"))
                wide = cnt > FR_MAXKNOTS
                if last:
                    W1 = a + cnt if wide else a + x0
                else:
                    W0 = a if wide else a + max(x0 - 1, 0)
        columns = n_valid <= FR_MAXV and C <= FR_MAXC and n_f <= FR_MAXF and n_c <= FR_MAXCC and (not greeks or C == 3)
        why = "rows" if W1 - W0 > FR_CAP else "nsym" if nsym > FR_MAXSYM else "" if columns else "columns"
        fr.append({"form": "perrow" if why else "whole" if whole else "window", "why": why, "s_first": s1, "s_last": s2,
                   "src_rows": int(np.count_nonzero((gpos >= g0) & (gpos <= g_last)))})
    return {"prepare": prepare, "eval": ev, "frame": fr}


def describe_row(layout, fm, g, c):
    """series, tag and the block forms of output row g, channel c (for failure messages)"""
    s = int(np.searchsorted(layout["q_off"], g, side="right")) - 1
    e, f = fm["eval"][g // E1_ROWS][c], fm["frame"][g // FR_ROWS]
    return (f"row {g} = series {s} ({layout['tags'][s]}) row {g - int(layout['q_off'][s])}, channel {c}: prepare {fm['prepare'][s][c]}, "
            f"eval block {g // E1_ROWS} {e[0]} (n1={e[1]}, n2={e[2]}), frame block {g // FR_ROWS} {f['form']}{(':' + f['why']) if f['why'] else ''}")
