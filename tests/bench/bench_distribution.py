#!/usr/bin/env python3
"""Risk-neutral distribution off raw SVI slices at the snapshot bench's size: U underlyings x B
snapshots x 16 tenors, the default 7 probabilities and 5 levels.  The parameters are the generating ones of
tests/svi_cases.batch (every row live, well inside the constraints), tenors from 5 to 90 days.  Prints one JSON line: the
kernel (HIP events, median after warm-up, summed over the underlyings), its row rate, and for scale a device-to-device copy
of a tensor of the size of the outputs, timed the same way: the kernel is bound by fp64 arithmetic (64 + 52 nP + nL
evaluations of erfc / exp / sqrt / division per row), not by its bytes.  The events bracket the Python calls (tensor checks,
the argument struct: a few tens of microseconds per call).  --sweep times the call's choice (0) and every legal rows_per_wave in two interleaved passes; its entries compare with one
another, not with the headline figure.
    python tests/bench/bench_distribution.py [--underlyings 4] [--snapshots 3781] [--reps 5] [--sweep]"""
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
ap.add_argument("--reps", type=int, default=5); ap.add_argument("--rate", type=float, default=0.03)
ap.add_argument("--sweep", action="store_true")
a = ap.parse_args()
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
probs, levels = engine.DEFAULT_PROBS, engine.DEFAULT_LEVELS
calls = []
for u in range(a.underlyings):
    c, gen = SC.batch(a.snapshots, 16, 9, 1000 + u, per_kq=True, holes=0.0, rate=a.rate)
    params, Tq, spot = dev(gen["params"]), dev(c["Tq"]), dev(c["spot"])
    out = engine.svi_distribution(params, Tq, spot, a.rate, probs=probs, levels=levels)
    calls.append((params, Tq, spot, out))
torch.cuda.synchronize()
rows = sum(c[3]["flags"].numel() for c in calls)
count = lambda key, bit: sum(int(((c[3][key] & bit) != 0).sum().item()) for c in calls)   # noqa: E731
out_bytes = sum(t.numel() * t.element_size() for c in calls for t in c[3].values())


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def dist_all(rpw=0):
    for params, Tq, spot, out in calls:
        engine.svi_distribution(params, Tq, spot, a.rate, probs=probs, levels=levels, out=out, rows_per_wave=rpw)


src = [torch.empty(sum(t.numel() * t.element_size() for t in c[3].values()), dtype=torch.uint8, device="cuda") for c in calls]
dst = [torch.empty_like(s) for s in src]


def copy_all():
    for s, d in zip(src, dst):
        d.copy_(s)


ms, ms_min, ms_max = events(dist_all, a.reps)
cp_ms, _, _ = events(copy_all, a.reps)
res = {"underlyings": a.underlyings, "snapshots": a.underlyings * a.snapshots, "rows": rows, "probs": len(probs), "levels": len(levels),
       "evaluations_per_row": 64 + 52 * len(probs) + len(levels), "dead_rows": count("flags", _lib.DS_DEAD),
       "tails_rows": count("flags", _lib.DS_TAILS), "no_bracket_targets": count("q_flags", _lib.DS_NO_BRACKET),
       "ambiguous_targets": count("q_flags", _lib.DS_AMBIGUOUS), "kernel": engine.last_kernel(), "reps": a.reps,
       "params_bytes": rows * 40, "out_bytes": out_bytes, "distribution_ms": ms, "distribution_ms_min": ms_min,
       "distribution_ms_max": ms_max, "distribution_Mrows_per_s": rows / ms / 1e3, "copy_ms": cp_ms, "distribution_over_copy": ms / cp_ms}
if a.sweep:
    # two passes over 0 (the call's choice) and every forced value, interleaved, the smaller median of the two: the sweep is for
    # comparing its own entries; the headline figure above is the first thing timed and carries the clock ramp
    order = list(range(0, 64 // len(probs) + 1))
    passes = [{rpw: events(lambda: dist_all(rpw), a.reps)[0] for rpw in seq} for seq in (order, order[::-1])]
    res["sweep_ms"] = {str(rpw): min(p_[rpw] for p_ in passes) for rpw in order}
print(json.dumps(res))
