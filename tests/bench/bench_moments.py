#!/usr/bin/env python3
"""Model-free moments and the vol index at the snapshot bench's size: U underlyings x B snapshots of
16 x 64 surfaces.  The surfaces are the skewed synthetic smiles of tests/mm_cases.smooth without holes, tenors from 5 to 90
days, one 30-day horizon.  Prints one JSON line: the kernel (HIP events, median after warm-up, summed over the underlyings),
its algorithmic bytes (8 B read per node; 76 B written per row, 12 B per snapshot) and node rate, and the yardstick -- a
device-to-device copy of a tensor of the size of `vol`, timed the same way.  The events bracket the Python calls (tensor
checks, the argument struct: a few tens of microseconds per call), so a kernel-trace figure (rocprofv3 --kernel-trace
--stats) is the check on the kernel time proper.
    python tests/bench/bench_moments.py [--underlyings 4] [--snapshots 3781] [--reps 21]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from iv_interpolation_amd import _lib, engine
import mm_cases as MC

ap = argparse.ArgumentParser()
ap.add_argument("--underlyings", type=int, default=4); ap.add_argument("--snapshots", type=int, default=3781)
ap.add_argument("--reps", type=int, default=21); ap.add_argument("--rate", type=float, default=0.03)
a = ap.parse_args()
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
calls = []
for u in range(a.underlyings):
    c = MC.smooth(a.snapshots, 16, 64, 1000 + u, per_kq=True, per_tq=False, holes=0.0)
    vol, Kq, Tq, spot = dev(c["vol"]), dev(c["Kq"]), dev(c["Tq"]), dev(c["spot"])
    out = engine.surface_moments(vol, Kq, Tq, spot, a.rate)
    calls.append((vol, Kq, Tq, spot, out))
torch.cuda.synchronize()
nodes = sum(c[0].numel() for c in calls)
rows = sum(c[4]["flags"].numel() for c in calls)
dead = sum(int((c[4]["flags"] == _lib.MM_DEAD).sum().item()) for c in calls)
indexed = sum(int(torch.isfinite(c[4]["index"]).sum().item()) for c in calls)


def events(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def moments_all():
    for vol, Kq, Tq, spot, out in calls:
        engine.surface_moments(vol, Kq, Tq, spot, a.rate, out=out)


copies = [torch.empty_like(c[0]) for c in calls]


def copy_all():
    for c, d in zip(calls, copies):
        d.copy_(c[0])


ms, ms_min, ms_max = events(moments_all, a.reps)
cp_ms, _, _ = events(copy_all, a.reps)
vol_bytes = nodes * 8
algo = vol_bytes + rows * 76 + a.underlyings * a.snapshots * 12
print(json.dumps({"underlyings": a.underlyings, "snapshots": a.underlyings * a.snapshots, "nodes": nodes, "rows": rows,
                  "dead_rows": dead, "indexed_snapshots": indexed, "kernel": engine.last_kernel(), "reps": a.reps,
                  "vol_bytes": vol_bytes, "algo_bytes": algo, "moments_ms": ms, "moments_ms_min": ms_min, "moments_ms_max": ms_max,
                  "moments_Gnodes_per_s": nodes / ms / 1e6, "moments_TBps": algo / ms / 1e9, "copy_ms": cp_ms,
                  "copy_TBps": 2 * vol_bytes / cp_ms / 1e9, "moments_over_copy": ms / cp_ms}))
