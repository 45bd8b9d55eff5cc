#!/usr/bin/env python3
"""SVI term structure at the snapshot bench's size: U underlyings x B snapshots x 16 tenors, the
generating parameters of tests/svi_cases.batch (every row live; the slices of a snapshot are drawn independently, so many
adjacent pairs cross), tenors from 5 to 90 days.  Three figures (HIP events, median after warm-up, summed over the
underlyings), each beside a device-to-device copy of a buffer of the size of that call's outputs, timed the same way: the
calendar kernel over all pairs; the evaluation kernel for a book of Q options per snapshot (strikes within +- 30 % of spot,
expiries from 3 to 100 days, per-snapshot query arrays) with all seven outputs; the same with `call` only.  The events
bracket the Python calls (tensor checks, the argument struct: a few tens of microseconds per call).  Prints one JSON line.
    python tests/bench/bench_svi_surface.py [--underlyings 4] [--snapshots 3781] [--book 1024] [--reps 5]"""
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
calls = []
for n in range(a.underlyings):
    c, gen = SC.batch(a.snapshots, 16, 9, 1000 + n, per_kq=True, holes=0.0, rate=a.rate)
    r = np.random.default_rng(2000 + n)
    u = c["spot"][:, None] * r.uniform(0.7, 1.3, (a.snapshots, a.book))
    tau = r.uniform(3.0 / 365.0, 100.0 / 365.0, (a.snapshots, a.book))
    params, Tq, spot, u, tau = dev(gen["params"]), dev(c["Tq"]), dev(c["spot"]), dev(u), dev(tau)
    cal = engine.svi_calendar(params, Tq, spot)
    full = engine.svi_eval(params, Tq, spot, a.rate, u, tau, strike_mode=1)
    one = engine.svi_eval(params, Tq, spot, a.rate, u, tau, strike_mode=1, want=("call",))
    calls.append(dict(ins=(params, Tq, spot), q=(u, tau), cal=cal, full=full, one=one))
torch.cuda.synchronize()


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def nbytes(key):
    return [sum(t.numel() * t.element_size() for t in c[key].values() if t is not None) for c in calls]


def copier(key):
    src = [torch.empty(n, dtype=torch.uint8, device="cuda") for n in nbytes(key)]
    dst = [torch.empty_like(s) for s in src]

    def run():
        for s, d in zip(src, dst):
            d.copy_(s)
    return run


def calendar_all():
    for c in calls:
        engine.svi_calendar(*c["ins"], out=c["cal"])


def eval_all(key, want):
    for c in calls:
        engine.svi_eval(*c["ins"], a.rate, *c["q"], strike_mode=1, want=want, out={k: v for k, v in c[key].items() if v is not None})


rows = sum(c["cal"]["flags"].numel() for c in calls)
queries = sum(c["full"]["flags"].numel() for c in calls)
count = lambda key, name, bit: sum(int(((c[key][name] & bit) != 0).sum().item()) for c in calls)   # noqa: E731
res = {"underlyings": a.underlyings, "snapshots": a.underlyings * a.snapshots, "rows": rows, "book": a.book, "queries": queries, "reps": a.reps,
       "pairs": rows - count("cal", "flags", _lib.SC_DEAD | _lib.SC_LAST | _lib.SC_UNORDERED),
       "calendar_pairs": count("cal", "flags", _lib.SC_CALENDAR), "wing_pairs": count("cal", "flags", _lib.SC_WING_LEFT | _lib.SC_WING_RIGHT),
       "crossings": sum(int(c["cal"]["n_cross"].sum().item()) for c in calls),
       "neg_fwd_queries": count("full", "flags", _lib.SE_NEG_FWD), "neg_g_queries": count("full", "flags", _lib.SE_NEG_G),
       "short_or_long_queries": count("full", "flags", _lib.SE_SHORT | _lib.SE_LONG)}
for name, fn, key in (("calendar", calendar_all, "cal"), ("eval_all", lambda: eval_all("full", engine.EVAL_OUTPUTS), "full"),
                      ("eval_call", lambda: eval_all("one", ("call",)), "one")):
    ms, lo, hi = events(fn, a.reps)
    kernel = engine.last_kernel()
    cp, _, _ = events(copier(key), a.reps)
    n = rows if key == "cal" else queries
    res[name] = {"kernel": kernel, "ms": ms, "ms_min": lo, "ms_max": hi, "M_per_s": n / ms / 1e3, "out_bytes": sum(nbytes(key)),
                 "copy_ms": cp, "over_copy": ms / cp, "out_GB_per_s": sum(nbytes(key)) / ms / 1e6}
print(json.dumps(res))
