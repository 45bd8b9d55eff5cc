#!/usr/bin/env python3
"""Delta-quoted smile points at the snapshot bench's size: U underlyings x B snapshots of 16 x 64
surfaces, 5 targets.  The surfaces are synthetic skewed parabolas in log-moneyness (tests/smile_cases.dense), so that every
target has a crossing and every lane of the inversion phase bisects.  Prints one JSON line: the kernel (HIP events, median
after warm-up, summed over the underlyings), its algorithmic bytes (vol, Kq, spot read; the three outputs written) and
their share of 8 TB/s, and the yardstick -- a device-to-device copy of a tensor of the size of `vol`, timed the same way.
The events bracket the Python calls (target conversion, tensor checks, the argument struct: a few tens of microseconds per
call), so a kernel-trace figure (rocprofv3 --kernel-trace --stats) is the check on the kernel time proper.  --sweep times
every forced rows_per_wave next to the launcher's own choice.
    python tests/bench/bench_smiles.py [--underlyings 4] [--snapshots 3781] [--reps 21]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from iv_interpolation_amd import engine
import smile_cases as SM

ap = argparse.ArgumentParser()
ap.add_argument("--underlyings", type=int, default=4); ap.add_argument("--snapshots", type=int, default=3781)
ap.add_argument("--reps", type=int, default=21); ap.add_argument("--targets", type=int, default=5)
ap.add_argument("--sweep", action="store_true", help="also time every forced rows_per_wave (the launcher's choice is the default run)")
a = ap.parse_args()
deltas = {1: (0.5,), 5: SM.DEFAULT, 16: SM.WIDE16}[a.targets]
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
calls = []
for u in range(a.underlyings):
    c = SM.dense(a.snapshots, 16, 64, 1000 + u, per_kq=True, per_tq=False)
    vol, Kq, Tq, spot = dev(c["vol"]), dev(c["Kq"]), dev(c["Tq"]), dev(c["spot"])
    out = engine.smile_delta_points(vol, Kq, Tq, spot, deltas)
    calls.append((vol, Kq, Tq, spot, out))
torch.cuda.synchronize()
crossing = float(np.mean([(o["flags"] != 1).float().mean().item() for *_, o in calls]))


def events(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def smiles_all(rpw=0):
    for vol, Kq, Tq, spot, out in calls:
        engine.smile_delta_points(vol, Kq, Tq, spot, deltas, out=out, rows_per_wave=rpw)


copies = [torch.empty_like(c[0]) for c in calls]


def copy_all():
    for c, d in zip(calls, copies):
        d.copy_(c[0])


ms, ms_min, ms_max = events(smiles_all, a.reps)
cp_ms, _, _ = events(copy_all, a.reps)
nD = len(deltas)
sweep = {}
if a.sweep:
    for rpw in sorted({1, 2, 3, 4, 6, 8, 12, 16, 32, 64} & set(range(1, 64 // nD + 1)) | {64 // nD}):
        sweep[str(rpw)] = events(lambda: smiles_all(rpw), a.reps)[0]
rows = sum(c[0].shape[0] * c[0].shape[1] for c in calls)
vol_bytes = sum(c[0].numel() * 8 for c in calls)
algo = vol_bytes + sum(c[1].numel() * 8 + c[3].numel() * 8 for c in calls) + rows * nD * (8 + 8 + 4)
print(json.dumps({"underlyings": a.underlyings, "snapshots": a.underlyings * a.snapshots, "rows": rows, "targets": nD,
                  "crossing_share": crossing, "kernel": engine.last_kernel(), "smiles_ms": ms, "smiles_ms_min": ms_min,
                  "smiles_ms_max": ms_max, "reps": a.reps, "algo_bytes": algo, "smiles_TBps": algo / ms / 1e9,
                  "smiles_frac_of_8TBps": algo / ms / 1e9 / 8.0, "vol_bytes": vol_bytes, "copy_ms": cp_ms,
                  "copy_TBps": 2 * vol_bytes / cp_ms / 1e9, "smiles_over_copy": ms / cp_ms,
                  "bisections_per_s": rows * nD * crossing / (ms * 1e-3), "ms_by_rows_per_wave": sweep}))
