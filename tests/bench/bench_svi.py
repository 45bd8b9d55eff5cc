#!/usr/bin/env python3
"""Raw SVI slices at the snapshot bench's size: U underlyings x B snapshots of 16 x 64 surfaces.  The
surfaces are the noisy raw-SVI smiles of tests/svi_cases.batch without holes (a quarter of the rows exact), tenors from 5 to
90 days, the default 16 rounds, no fitted vols.  Prints one JSON line: the kernel (HIP events, median after warm-up, summed
over the underlyings), its row rate, and for scale a device-to-device copy of a tensor of the size of `vol`, timed the same
way: the kernel is bound by fp64 arithmetic (rounds x 64 candidates x (2 n square roots + 27 small solves) per row), not by
its bytes.  The events bracket the Python calls (tensor checks, the argument struct: a few tens of microseconds per call).
    python tests/bench/bench_svi.py [--underlyings 4] [--snapshots 3781] [--reps 5] [--rounds 0]"""
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
ap.add_argument("--rounds", type=int, default=0)
a = ap.parse_args()
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
calls = []
for u in range(a.underlyings):
    c, _ = SC.batch(a.snapshots, 16, 64, 1000 + u, per_kq=True, holes=0.0, rate=a.rate)
    vol, Kq, Tq, spot = dev(c["vol"]), dev(c["Kq"]), dev(c["Tq"]), dev(c["spot"])
    out = engine.svi_slices(vol, Kq, Tq, spot, a.rate, rounds=a.rounds)
    calls.append((vol, Kq, Tq, spot, out))
torch.cuda.synchronize()
nodes = sum(c[0].numel() for c in calls)
rows = sum(c[4]["flags"].numel() for c in calls)
count = lambda bit: sum(int(((c[4]["flags"] & bit) != 0).sum().item()) for c in calls)   # noqa: E731
worst_rmse = max(float(torch.nan_to_num(c[4]["fit"][..., 1], nan=0.0).max().item()) for c in calls)


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def svi_all():
    for vol, Kq, Tq, spot, out in calls:
        engine.svi_slices(vol, Kq, Tq, spot, a.rate, rounds=a.rounds, out=out)


copies = [torch.empty_like(c[0]) for c in calls]


def copy_all():
    for c, d in zip(calls, copies):
        d.copy_(c[0])


ms, ms_min, ms_max = events(svi_all, a.reps)
cp_ms, _, _ = events(copy_all, a.reps)
print(json.dumps({"underlyings": a.underlyings, "snapshots": a.underlyings * a.snapshots, "nodes": nodes, "rows": rows,
                  "rounds": a.rounds or 16, "dead_rows": count(_lib.SV_DEAD), "bound_rows": count(_lib.SV_BOUND),
                  "edge_rows": count(_lib.SV_EDGE), "butterfly_rows": count(_lib.SV_BUTTERFLY), "worst_rmse_vol": worst_rmse,
                  "kernel": engine.last_kernel(), "reps": a.reps, "vol_bytes": nodes * 8, "svi_ms": ms, "svi_ms_min": ms_min,
                  "svi_ms_max": ms_max, "svi_Mrows_per_s": rows / ms / 1e3, "copy_ms": cp_ms, "svi_over_copy": ms / cp_ms}))
