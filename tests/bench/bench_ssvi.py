#!/usr/bin/env python3
"""SSVI surfaces at the snapshot bench's size: U underlyings x B snapshots of 16 x 64 surfaces.  The
surfaces are the noisy SSVI surfaces of tests/ssvi_cases.batch without holes (every other snapshot exact), theta0 given, the
default 20 rounds, no fitted vols.  Prints one JSON line and writes it to profiles/ssvi/bench_ssvi.json: the kernel (HIP
events, median after warm-up, summed over the underlyings), its snapshot rate, and for scale a device-to-device copy of a
tensor of the size of `vol`, timed the same way: the kernel is bound by fp64 arithmetic (rounds x 216 candidates x one square
root per node), not by its bytes.  The events bracket the Python calls (tensor checks, the argument struct: a few tens of
microseconds per call).
    python tests/bench/bench_ssvi.py [--underlyings 4] [--snapshots 3781] [--reps 5] [--rounds 0] [--out FILE]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from iv_interpolation_amd import _lib, engine
import ssvi_cases as SC

ap = argparse.ArgumentParser()
ap.add_argument("--underlyings", type=int, default=4); ap.add_argument("--snapshots", type=int, default=3781)
ap.add_argument("--reps", type=int, default=5); ap.add_argument("--rate", type=float, default=0.03)
ap.add_argument("--rounds", type=int, default=0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssvi", "bench_ssvi.json"))
a = ap.parse_args()
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
calls = []
for u in range(a.underlyings):
    c, _ = SC.batch(a.snapshots, 16, 64, 2000 + u, per_kq=True, holes=0.0, rate=a.rate)
    vol, Kq, Tq, spot, th0 = dev(c["vol"]), dev(c["Kq"]), dev(c["Tq"]), dev(c["spot"]), dev(c["theta0"])
    out = engine.ssvi_surface(vol, Kq, Tq, spot, a.rate, theta0=th0, rounds=a.rounds)
    calls.append((vol, Kq, Tq, spot, th0, out))
torch.cuda.synchronize()
nodes = sum(c[0].numel() for c in calls)
snaps = sum(c[5]["sflags"].numel() for c in calls)
count = lambda key, bit: sum(int(((c[5][key] & bit) != 0).sum().item()) for c in calls)   # noqa: E731
worst_rmse = max(float(torch.nan_to_num(c[5]["surface"][:, 3], nan=0.0).max().item()) for c in calls)


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def ssvi_all():
    for vol, Kq, Tq, spot, th0, out in calls:
        engine.ssvi_surface(vol, Kq, Tq, spot, a.rate, theta0=th0, rounds=a.rounds, out=out)


copies = [torch.empty_like(c[0]) for c in calls]


def copy_all():
    for c, d in zip(calls, copies):
        d.copy_(c[0])


ms, ms_min, ms_max = events(ssvi_all, a.reps)
cp_ms, _, _ = events(copy_all, a.reps)
rounds = a.rounds or 20
line = json.dumps({"underlyings": a.underlyings, "snapshots": snaps, "nodes": nodes, "rounds": rounds,
                   "dead_surfaces": count("sflags", _lib.SF_SURF_DEAD | _lib.SF_UNORDERED), "dead_rows": count("flags", _lib.SS_DEAD),
                   "raised_rows": count("flags", _lib.SS_RAISED), "butterfly_rows": count("flags", _lib.SS_BUTTERFLY),
                   "at_bound": count("sflags", _lib.SF_AT_BOUND), "worst_rmse": worst_rmse,
                   "kernel": engine.last_kernel(), "reps": a.reps, "vol_bytes": nodes * 8, "ssvi_ms": ms, "ssvi_ms_min": ms_min,
                   "ssvi_ms_max": ms_max, "ssvi_snapshots_per_s": snaps / ms * 1e3,
                   "sqrt_evaluations": 216 * rounds * nodes, "ssvi_Gsqrt_per_s": 216 * rounds * nodes / ms / 1e6,
                   "copy_ms": cp_ms, "ssvi_over_copy": ms / cp_ms})
print(line)
if a.out:
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
