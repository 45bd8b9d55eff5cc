#!/usr/bin/env python3
"""P&L explain at the book-risk bench's size: U underlyings x B snapshots x 16 tenors, the generating
parameters of tests/svi_cases.batch, a book of Q options (strikes within +- 30 % of spot, expiries from 3 to 100 days,
per-snapshot strike and expiry arrays, one shared list of sides and quantities), lag 1: B - 1 pairs per underlying.  Figures (HIP
events round the Python calls, median of `reps` after one warm-up call, with min and max, summed over the underlyings; every
buffer is allocated once before the timing and kept): the explain call with all ten outputs beside svi_greeks with all seven of
its own and beside a device copy of the size of the explain's outputs, in the same run.  Prints one JSON line.
    python tests/bench/bench_explain.py [--underlyings 4] [--snapshots 3781] [--book 1024] [--lag 1] [--reps 5]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from iv_interpolation_amd import engine
import svi_cases as SC

ap = argparse.ArgumentParser()
ap.add_argument("--underlyings", type=int, default=4); ap.add_argument("--snapshots", type=int, default=3781)
ap.add_argument("--book", type=int, default=1024); ap.add_argument("--lag", type=int, default=1); ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rate", type=float, default=0.03)
a = ap.parse_args()
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
calls = []
for n in range(a.underlyings):
    c, gen = SC.batch(a.snapshots, 16, 9, 1000 + n, per_kq=True, holes=0.0, rate=a.rate)
    r = np.random.default_rng(2000 + n)
    u = c["spot"][:, None] * r.uniform(0.7, 1.3, (a.snapshots, a.book))
    tau = r.uniform(3.0 / 365.0, 100.0 / 365.0, (a.snapshots, a.book))
    side, qty = dev((r.random(a.book) < 0.5).astype(np.uint8)), dev(np.round(r.uniform(-10.0, 10.0, a.book), 2))
    params, Tq, spot, u, tau = dev(gen["params"]), dev(c["Tq"]), dev(c["spot"]), dev(u), dev(tau)
    gr = engine.svi_greeks(params, Tq, spot, a.rate, u, tau, is_put=side, strike_mode=1)
    ex = engine.svi_explain(params, Tq, spot, a.rate, u, tau, qty, lag=a.lag, is_put=side, strike_mode=1)
    calls.append(dict(ins=(params, Tq, spot), q=(u, tau), side=side, qty=qty, gr=gr, ex=ex))
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


def greeks_all():
    for c in calls:
        engine.svi_greeks(*c["ins"], a.rate, *c["q"], is_put=c["side"], strike_mode=1, out=c["gr"])


def explain_all():
    for c in calls:
        engine.svi_explain(*c["ins"], a.rate, *c["q"], c["qty"], lag=a.lag, is_put=c["side"], strike_mode=1, out=c["ex"])


res = {"underlyings": a.underlyings, "snapshots": a.underlyings * a.snapshots, "book_size": a.book, "lag": a.lag, "reps": a.reps,
       "pairs": sum(c["ex"]["n_dead"].numel() for c in calls), "dead_options": sum(int(c["ex"]["n_dead"].sum().item()) for c in calls)}
for name, fn, key in (("greeks_all", greeks_all, "gr"), ("explain_all", explain_all, "ex")):
    options = sum(c[key]["flags"].numel() for c in calls)
    out_bytes = [size(c[key].values()) for c in calls]
    ms, lo, hi = events(fn, a.reps)
    kernel = engine.last_kernel()
    cp, _, _ = events(copier(out_bytes), a.reps)
    res[name] = {"kernel": kernel, "options": options, "ms": ms, "ms_min": lo, "ms_max": hi, "M_options_per_s": options / ms / 1e3,
                 "ns_per_option": ms * 1e6 / options, "bytes": sum(out_bytes), "copy_ms": cp, "over_copy": ms / cp}
res["explain_over_greeks_per_option"] = res["explain_all"]["ns_per_option"] / res["greeks_all"]["ns_per_option"]
print(json.dumps(res))
