#!/usr/bin/env python3
"""Minimum-variance hedge on the workload of tests/bench/bench_hsim.py: U underlyings x B snapshots x 16
tenors, a book of Q options, lag 1, a window of W scenarios and the levels 5 % and 1 %.  The candidates are the underlying and the
first 63 contracts of the book (calls and puts as the book holds them), K = 4 rounds, all greedy.  Figures (HIP events round the
Python calls, median of `reps` after one warm-up call, with min and max, summed over the underlyings; every buffer is allocated once
before the timing and kept): stage 1 (svi_inst_pnl_kernel) and stage 2 (hedge_pursuit_kernel and the tail) apart, and in the same
run the two yardsticks: the P&L call of ivs_svi_hsim_f64 (stages = 1) and a device copy of inst_pnl.  Prints one JSON line; --out
FILE writes it there as well.
    python tests/bench/bench_hedge.py [--underlyings 4] [--snapshots 3781] [--book 1024] [--lag 1] [--window 256] [--inst 64] [--rounds 4]"""
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
ap.add_argument("--inst", type=int, default=64); ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--reps", type=int, default=5); ap.add_argument("--rate", type=float, default=0.03); ap.add_argument("--out")
a = ap.parse_args()
LEVELS = (0.05, 0.01)
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
    hg = engine.svi_hedge(params, Tq, spot, a.rate, iu, it, ik, hs["pnl"], hs["scen_flags"], rounds=a.rounds, **kw)
    print(f"underlying {n}: ready", file=sys.stderr, flush=True)
    calls.append(dict(ins=(params, Tq, spot), q=(u, tau), qty=qty, side=side, inst=(iu, it, ik), kw=kw, hs=hs, hg=hg, copy=torch.empty_like(hg["inst_pnl"])))
torch.cuda.synchronize()


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def hedge(stages):
    def run():
        for c in calls:
            engine.svi_hedge(*c["ins"], a.rate, *c["inst"], c["hs"]["pnl"], c["hs"]["scen_flags"], rounds=a.rounds, stages=stages,
                             out={k: v for k, v in c["hg"].items() if v is not None}, **c["kw"])
    return run


def hsim_pnl():
    for c in calls:
        engine.svi_hsim(*c["ins"], a.rate, *c["q"], c["qty"], out=c["hs"], stages=1, is_put=c["side"], **c["kw"])


def copy():
    for c in calls:
        c["copy"].copy_(c["hg"]["inst_pnl"])


fl = torch.cat([c["hs"]["scen_flags"].reshape(-1) for c in calls])
existing = int((fl != 1).sum().item())
n_rounds = torch.cat([c["hg"]["n_rounds"] for c in calls])
left = torch.cat([c["hg"]["ss"][:, -1] / c["hg"]["ss"][:, 0] for c in calls])
res = {"underlyings": a.underlyings, "snapshots": a.underlyings * a.snapshots, "book_size": a.book, "lag": a.lag, "window": a.window, "levels": LEVELS,
       "candidates": a.inst, "rounds": a.rounds, "reps": a.reps, "scenarios": existing, "revaluations": existing * a.inst,
       "inst_pnl_bytes": sum(c["hg"]["inst_pnl"].numel() * 8 for c in calls), "rounds_run": int(n_rounds.sum().item()),
       "median_left": float(left[~left.isnan()].median().item())}
for key, fn, kernel in (("stage1", hedge(1), "svi_inst_pnl_kernel"), ("stage2", hedge(2), "hedge_pursuit_kernel + hsim_tail_kernel"),
                        ("pnl_call", hsim_pnl, "svi_hsim_kernel"), ("copy_inst_pnl", copy, "device copy")):
    ms, lo, hi = events(fn, a.reps)
    res[key] = {"kernel": kernel, "ms": ms, "ms_min": lo, "ms_max": hi}
res["stage1"]["ns_per_revaluation"] = res["stage1"]["ms"] * 1e6 / (existing * a.inst)
res["pnl_call"]["ns_per_option_scenario"] = res["pnl_call"]["ms"] * 1e6 / (existing * a.book)
res["stage1_over_pnl_per_revaluation"] = res["stage1"]["ns_per_revaluation"] / res["pnl_call"]["ns_per_option_scenario"]
res["stage1_over_pnl_ms"] = res["stage1"]["ms"] / res["pnl_call"]["ms"]
res["stage2_over_copy_ms"] = res["stage2"]["ms"] / res["copy_inst_pnl"]["ms"]
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
