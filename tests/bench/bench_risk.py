#!/usr/bin/env python3
"""Book risk at the snapshot bench's size: U underlyings x B snapshots x 16 tenors, the generating
parameters of tests/svi_cases.batch, a book of Q options per snapshot (strikes within +- 30 % of spot, expiries from 3 to 100
days, per-snapshot strike and expiry arrays, one shared list of sides and quantities), the default 9 x 5 scenario grid, both
dynamics.  Figures (HIP events round the Python calls, median of `reps` after one warm-up call, with min and max, summed over
the underlyings; every buffer is allocated once before the timing and kept: svi_eval's outputs first, the Greeks' outputs of
the same sizes second, the book's after them, the copy buffers last): the Greeks call with all seven outputs beside svi_eval with
all seven of its own and beside a device copy of the size of its outputs; the book call beside a device copy of the size of
its inputs and outputs.  Prints one JSON line.
    python tests/bench/bench_risk.py [--underlyings 4] [--snapshots 3781] [--book 1024] [--reps 5]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from iv_interpolation_amd import _lib, engine
import svi_cases as SC

ap = argparse.ArgumentParser()
ap.add_argument("--underlyings", type=int, default=4); ap.add_argument("--snapshots", type=int, default=3781)
ap.add_argument("--book", type=int, default=1024); ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rate", type=float, default=0.03)
a = ap.parse_args()
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
nA, nV = len(engine.DEFAULT_SPOT_SHOCKS), len(engine.DEFAULT_VOL_SHOCKS)
calls = []
for n in range(a.underlyings):
    c, gen = SC.batch(a.snapshots, 16, 9, 1000 + n, per_kq=True, holes=0.0, rate=a.rate)
    r = np.random.default_rng(2000 + n)
    u = c["spot"][:, None] * r.uniform(0.7, 1.3, (a.snapshots, a.book))
    tau = r.uniform(3.0 / 365.0, 100.0 / 365.0, (a.snapshots, a.book))
    side, qty = dev((r.random(a.book) < 0.5).astype(np.uint8)), dev(np.round(r.uniform(-10.0, 10.0, a.book), 2))
    params, Tq, spot, u, tau = dev(gen["params"]), dev(c["Tq"]), dev(c["spot"]), dev(u), dev(tau)
    ev = engine.svi_eval(params, Tq, spot, a.rate, u, tau, strike_mode=1)
    gr = engine.svi_greeks(params, Tq, spot, a.rate, u, tau, is_put=side, strike_mode=1)
    bk = engine.svi_book(params, Tq, spot, a.rate, u, tau, qty, is_put=side, strike_mode=1)
    calls.append(dict(ins=(params, Tq, spot), q=(u, tau), side=side, qty=qty, ev=ev, gr=gr, bk=bk))
torch.cuda.synchronize()


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def size(ts):
    return sum(t.numel() * t.element_size() for t in ts if t is not None)


def copier(sizes):
    src = [torch.empty(n, dtype=torch.uint8, device="cuda") for n in sizes]
    dst = [torch.empty_like(s) for s in src]

    def run():
        for s, d in zip(src, dst):
            d.copy_(s)
    return run


def eval_all():
    for c in calls:
        engine.svi_eval(*c["ins"], a.rate, *c["q"], strike_mode=1, out=c["ev"])


def greeks_all():
    for c in calls:
        engine.svi_greeks(*c["ins"], a.rate, *c["q"], is_put=c["side"], strike_mode=1, out=c["gr"])


def book_all():
    for c in calls:
        engine.svi_book(*c["ins"], a.rate, *c["q"], c["qty"], is_put=c["side"], strike_mode=1, out=c["bk"])


options = sum(c["gr"]["flags"].numel() for c in calls)
cells = sum(c["bk"]["cell_flags"].numel() for c in calls)
res = {"underlyings": a.underlyings, "snapshots": a.underlyings * a.snapshots, "book_size": a.book, "options": options, "grid": [nA, nV], "cells": cells,
       "reps": a.reps, "dead_options": sum(int(c["bk"]["n_dead"].sum().item()) for c in calls),
       "neg_vol_cells": sum(int((c["bk"]["cell_flags"] != 0).sum().item()) for c in calls)}
out_bytes = {"ev": [size(c["ev"].values()) for c in calls], "gr": [size(c["gr"].values()) for c in calls],
             "bk": [size(c["bk"].values()) + size(c["ins"]) + size(c["q"]) + size((c["side"], c["qty"])) for c in calls]}
for name, fn, key in (("eval_all", eval_all, "ev"), ("greeks_all", greeks_all, "gr"), ("book", book_all, "bk")):
    ms, lo, hi = events(fn, a.reps)
    kernel = engine.last_kernel()
    cp, _, _ = events(copier(out_bytes[key]), a.reps)
    res[name] = {"kernel": kernel, "ms": ms, "ms_min": lo, "ms_max": hi, "M_options_per_s": options / ms / 1e3, "bytes": sum(out_bytes[key]),
                 "copy_ms": cp, "over_copy": ms / cp}
res["greeks_over_eval"] = res["greeks_all"]["ms"] / res["eval_all"]["ms"]
# one price (two erfc) per option, cell and dynamic
res["book"]["G_erfc_per_s"] = options * nA * nV * 2 * 2 / res["book"]["ms"] / 1e6
print(json.dumps(res))
