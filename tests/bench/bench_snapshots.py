#!/usr/bin/env python3
"""Per-minute surface snapshots at full size: U underlyings x 12 expiries x 48 strikes x 2 sides x
3781 minutes, ~10 % of the strikes unlisted per expiry, the nearest expiry passing mid-window.  Prints one JSON line:
the assembly kernel (HIP events, median after warm-up, summed over the underlyings), its algorithmic bytes (24 B per
row read: date, iv, underlying_price; 8 B per written cell, T and spot) and their share of 8 TB/s, the surface step's
kernels and time, the host bookkeeping of build() on the long frame, and build() end to end.
    python tests/bench/bench_snapshots.py [--underlyings 4] [--minutes 3781] [--reps 5]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from iv_interpolation_amd import engine
from iv_interpolation_amd.snapshots import HipBackend, SnapshotSurfaceBuilder
import snapshot_cases as SC

ap = argparse.ArgumentParser()
ap.add_argument("--underlyings", type=int, default=4); ap.add_argument("--minutes", type=int, default=3781)
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()
frame = SC.big_chain(n_und=a.underlyings, nT=12, nK=48, minutes=a.minutes, seed=2)


class Recording(HipBackend):
    """HipBackend that keeps the device inputs of every call and the time spent inside the calls (synchronised)."""
    def __init__(self):
        super().__init__(); self.calls = []; self.device_s = 0.0; self.surface_kernels = []

    def assemble(self, *args):
        t = time.perf_counter()
        d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
        up = [d(x) for x in args[:7]]
        out = engine.snapshot_assemble(*up, args[7], args[8], d(args[9]), args[10])
        torch.cuda.synchronize(); self.device_s += time.perf_counter() - t
        self.calls.append((up, args[7], args[8], d(args[9]), args[10], out))
        return out

    def surface_batch(self, *args):
        t = time.perf_counter()
        r = super().surface_batch(*args)
        torch.cuda.synchronize(); self.device_s += time.perf_counter() - t
        self.surface_kernels.append(engine.last_kernel())
        return r


def events(fn, reps):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2]


rec = Recording()
SnapshotSurfaceBuilder(backend=rec).build(frame)                   # warm-up + inputs of every underlying
torch.cuda.synchronize()
rec.calls.clear(); rec.device_s = 0.0; rec.surface_kernels.clear()
t = time.perf_counter()
res = SnapshotSurfaceBuilder(backend=rec).build(frame)
torch.cuda.synchronize()
wall = time.perf_counter() - t
host_ms = (wall - rec.device_s) * 1e3

rows = cells = snaps = 0
for up, t0, B, mny, kqe, out in rec.calls:
    nT, nK = up[6].numel(), up[5].numel()
    rows += up[1].numel(); cells += B * nT * nK; snaps += B


def assemble_all():
    for up, t0, B, mny, kqe, out in rec.calls:
        engine.snapshot_assemble(*up, t0, B, mny, kqe, out=out)


asm_ms = events(assemble_all, a.reps)
nT_all = sum(c[0][6].numel() * c[2] for c in rec.calls)
algo_bytes = 24 * rows + 8 * (cells + nT_all + snaps)
K_dev = [torch.from_numpy(r.strikes).cuda() for r in res]
Tq = torch.from_numpy(res[0].tenors).cuda()
surf_ms = events(lambda: [engine.surface_batch(K, c[5]["T"], c[5]["sigma"], c[5]["Kq"], Tq, "linear")
                          for K, c in zip(K_dev, rec.calls)], a.reps)
e2e = []
for _ in range(3):
    t = time.perf_counter()
    SnapshotSurfaceBuilder().build(frame)
    torch.cuda.synchronize(); e2e.append((time.perf_counter() - t) * 1e3)
print(json.dumps({"underlyings": a.underlyings, "expiries": 12, "strikes": 48, "minutes": a.minutes, "rows": rows,
                  "snapshots": snaps, "cells": cells, "assembly_ms": asm_ms, "assembly_bytes": algo_bytes,
                  "assembly_TBps": algo_bytes / asm_ms / 1e9, "assembly_frac_of_8TBps": algo_bytes / asm_ms / 1e9 / 8.0,
                  "surface_kernels": sorted(set(rec.surface_kernels)), "surface_ms": surf_ms,
                  "host_bookkeeping_ms": host_ms, "build_ms": sorted(e2e)[1]}))
