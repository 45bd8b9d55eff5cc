#!/usr/bin/env python3
"""What-if VaR and ES per candidate trade and size on the workload of tests/bench/bench_hsim.py: U underlyings
x B snapshots x 16 tenors, a book of Q options, lag 1, a window of W scenarios and the levels 5 % and 1 %.  The candidates are
bench_hedge.py's (the underlying and the first 63 contracts of the book), the ladder is shared: nQ multiples (0.25 .. 3) of every
candidate's median minimum-variance size over the snapshots.  Figures (HIP events round the Python calls, median of `reps` after one
warm-up call, with min and max, summed over the underlyings; every buffer is allocated once before the timing and kept): stage 2
(whatif_tail_kernel) apart, and in the same run stage 2 of ivs_svi_hsim_f64 on pnl (hsim_tail_kernel: the cost of ranking one row
the old way) and a device copy of inst_pnl.  The yardstick is nH x nQ times the tail kernel's cost per row.  Prints one JSON line;
--out FILE writes it there as well.
    python tests/bench/bench_whatif.py [--underlyings 4] [--snapshots 3781] [--book 1024] [--lag 1] [--window 256] [--inst 64] [--rungs 8]"""
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
ap.add_argument("--book", type=int, default=1024); ap.add_argument("--lag", type=int, default=1); ap.add_argument("--window", type=int, default=256)
ap.add_argument("--inst", type=int, default=64); ap.add_argument("--rungs", type=int, default=8)
ap.add_argument("--reps", type=int, default=5); ap.add_argument("--rate", type=float, default=0.03); ap.add_argument("--out")
a = ap.parse_args()
LEVELS = (0.05, 0.01)
MULT = np.array([0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0, -0.5, -1.0, -2.0, -3.0])[:a.rungs]
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
calls = []
for n in range(a.underlyings):
    c, gen = SC.batch(a.snapshots, 16, 9, 1000 + n, per_kq=True, holes=0.0, rate=a.rate)
    r = np.random.default_rng(2000 + n)
    u = c["spot"][:, None] * r.uniform(0.7, 1.3, (a.snapshots, a.book))
    tau = r.uniform(3.0 / 365.0, 100.0 / 365.0, (a.snapshots, a.book))
    side_h = (r.random(a.book) < 0.5).astype(np.uint8)
    side, qty = dev(side_h), dev(np.round(r.uniform(-10.0, 10.0, a.book), 2))
    kind = side_h[:a.inst].copy()
    kind[0] = 2                                                          # the underlying, then 63 contracts of the book
    iu, it, ik = dev(u[:, :a.inst]), dev(tau[:, :a.inst]), dev(kind)
    params, Tq, spot, u, tau = dev(gen["params"]), dev(c["Tq"]), dev(c["spot"]), dev(u), dev(tau)
    kw = dict(lag=a.lag, window=a.window, tail_probs=LEVELS, strike_mode=1)
    hs = engine.svi_hsim(params, Tq, spot, a.rate, u, tau, qty, is_put=side, **kw)
    hg = engine.svi_hedge(params, Tq, spot, a.rate, iu, it, ik, hs["pnl"], hs["scen_flags"], rounds=1, **kw)
    solo = torch.nan_to_num(torch.nanmedian(hg["solo_qty"], dim=0).values, nan=1.0)
    size = (solo[:, None] * dev(MULT)[None, :]).contiguous()
    wi = engine.svi_whatif(params, Tq, spot, a.rate, iu, it, ik, hs["pnl"], hs["scen_flags"], size, inst_pnl=hg["inst_pnl"], stages=2, **kw)
    print(f"underlying {n}: ready", file=sys.stderr, flush=True)
    calls.append(dict(ins=(params, Tq, spot), inst=(iu, it, ik), kw=kw, hs=hs, wi=wi, size=size, one=size[:, 0].contiguous(),
                      copy=torch.empty_like(wi["inst_pnl"])))
    del hg
torch.cuda.synchronize()


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def ladder():
    for c in calls:
        engine.svi_whatif(*c["ins"], a.rate, *c["inst"], c["hs"]["pnl"], c["hs"]["scen_flags"], c["size"], stages=2,
                          out={k: v for k, v in c["wi"].items() if v is not None}, **c["kw"])


def hsim_tail():
    for c in calls:
        engine.svi_hsim(*c["ins"], a.rate, c["inst"][0], c["inst"][1], c["one"], out=c["hs"], stages=2, value=False, **c["kw"])


def copy():
    for c in calls:
        c["copy"].copy_(c["wi"]["inst_pnl"])


snaps = a.underlyings * a.snapshots
rows = snaps * a.inst * a.rungs
live = int(sum((c["wi"]["worst_w"] >= 0).sum().item() for c in calls))
es0 = torch.cat([c["wi"]["es0"][:, 0] for c in calls])
best = torch.cat([torch.where(c["wi"]["best"][:, :, 0] >= 0, c["wi"]["es_w"][:, :, :, 0].gather(2, c["wi"]["best"][:, :, :1].clamp(min=0).long())[:, :, 0],
                              float("inf")).min(dim=1).values for c in calls])
gain = ((es0 - best) / es0)[torch.isfinite(best) & (es0 > 0)]
res = {"underlyings": a.underlyings, "snapshots": snaps, "book_size": a.book, "lag": a.lag, "window": a.window, "levels": LEVELS,
       "candidates": a.inst, "rungs": a.rungs, "reps": a.reps, "rows": rows, "live_rows": live,
       "inst_pnl_bytes": sum(c["wi"]["inst_pnl"].numel() * 8 for c in calls), "median_es_reduction_of_the_best_trade": float(gain.median().item())}
for key, fn, kernel in (("stage2", ladder, "whatif_tail_kernel"), ("hsim_tail", hsim_tail, "hsim_tail_kernel"), ("copy_inst_pnl", copy, "device copy")):
    ms, lo, hi = events(fn, a.reps)
    res[key] = {"kernel": kernel, "ms": ms, "ms_min": lo, "ms_max": hi}
res["stage2"]["ns_per_row"] = res["stage2"]["ms"] * 1e6 / rows
res["hsim_tail"]["ns_per_row"] = res["hsim_tail"]["ms"] * 1e6 / snaps
res["yardstick_ms"] = res["hsim_tail"]["ms"] * a.inst * a.rungs
res["stage2_over_yardstick"] = res["stage2"]["ms"] / res["yardstick_ms"]
res["stage2_over_copy_ms"] = res["stage2"]["ms"] / res["copy_inst_pnl"]["ms"]
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
