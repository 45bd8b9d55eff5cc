#!/usr/bin/env python3
"""Static-arbitrage report, local vol and density at the snapshot bench's size: U underlyings x B
snapshots of 16 x 64 surfaces.  The surfaces are the smooth synthetic parabolas of tests/arb_cases.smooth, so nearly every
interior node is evaluated.  Prints one JSON line: the kernel (HIP events, median after warm-up, summed over the
underlyings) with all outputs and with flags + report only, the algorithmic bytes of each (8 B read per node; 4 B flags,
+ 8 B local vol, + 8 B density written) and their share of 8 TB/s, and the yardstick -- a device-to-device copy of a tensor
of the size of `vol`, timed the same way.  The events bracket the Python calls (tensor checks, the argument struct: a few
tens of microseconds per call), so a kernel-trace figure (rocprofv3 --kernel-trace --stats) is the check on the kernel time
proper.
    python tests/bench/bench_arbitrage.py [--underlyings 4] [--snapshots 3781] [--reps 21]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from iv_interpolation_amd import engine
import arb_cases as AC

ap = argparse.ArgumentParser()
ap.add_argument("--underlyings", type=int, default=4); ap.add_argument("--snapshots", type=int, default=3781)
ap.add_argument("--reps", type=int, default=21); ap.add_argument("--rate", type=float, default=0.03)
a = ap.parse_args()
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
calls = []
for u in range(a.underlyings):
    c = AC.smooth(a.snapshots, 16, 64, 1000 + u, per_kq=True, per_tq=False)
    vol, Kq, Tq, spot = dev(c["vol"]), dev(c["Kq"]), dev(c["Tq"]), dev(c["spot"])
    out = engine.surface_arbitrage(vol, Kq, Tq, spot, a.rate)
    calls.append((vol, Kq, Tq, spot, out, {k: out[k] for k in ("flags", "counts", "worst")}))
torch.cuda.synchronize()
nodes = sum(c[0].numel() for c in calls)
evaluated = sum(int(c[4]["counts"][:, 0].sum().item()) for c in calls)


def events(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def arb_all():
    for vol, Kq, Tq, spot, out, _ in calls:
        engine.surface_arbitrage(vol, Kq, Tq, spot, a.rate, out=out)


def arb_report_only():
    for vol, Kq, Tq, spot, _, rep in calls:
        engine.surface_arbitrage(vol, Kq, Tq, spot, a.rate, local_vol=False, density=False, out=rep)


copies = [torch.empty_like(c[0]) for c in calls]


def copy_all():
    for c, d in zip(calls, copies):
        d.copy_(c[0])


ms, ms_min, ms_max = events(arb_all, a.reps)
rp, rp_min, rp_max = events(arb_report_only, a.reps)
cp_ms, _, _ = events(copy_all, a.reps)
vol_bytes = nodes * 8
res = {"underlyings": a.underlyings, "snapshots": a.underlyings * a.snapshots, "nodes": nodes,
       "evaluated_share": evaluated / nodes, "kernel": engine.last_kernel(), "reps": a.reps, "vol_bytes": vol_bytes,
       "copy_ms": cp_ms, "copy_TBps": 2 * vol_bytes / cp_ms / 1e9}
for tag, t, lo, hi, per_node in (("", ms, ms_min, ms_max, 8 + 20), ("_report_only", rp, rp_min, rp_max, 8 + 4)):
    algo = nodes * per_node
    res.update({f"arbitrage_ms{tag}": t, f"arbitrage_ms_min{tag}": lo, f"arbitrage_ms_max{tag}": hi, f"algo_bytes{tag}": algo,
                f"arbitrage_TBps{tag}": algo / t / 1e9, f"arbitrage_frac_of_8TBps{tag}": algo / t / 1e9 / 8.0,
                f"arbitrage_over_copy{tag}": t / cp_ms})
print(json.dumps(res))
