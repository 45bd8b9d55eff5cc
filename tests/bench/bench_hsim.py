#!/usr/bin/env python3
"""Historical-simulation VaR at the book-risk bench's size: U underlyings x B snapshots x 16 tenors, the
generating parameters of tests/svi_cases.batch, a book of Q options (strikes within +- 30 % of spot, expiries from 3 to 100 days,
per-snapshot strike and expiry arrays, one shared list of sides and quantities), lag 1, a window of W scenarios and two levels.
Figures (HIP events round the Python calls, median of `reps` after one warm-up call, with min and max, summed over the
underlyings; every buffer is allocated once before the timing and kept): the P&L call (stages = 1), the order statistics alone
(stages = 2) beside a device copy of pnl, and svi_book with its default grid in the same run as the yardstick: ns per (option,
scenario) beside its ns per (option, cell, dynamic).  Prints one JSON line; --out FILE writes it there as well.
    python tests/bench/bench_hsim.py [--underlyings 4] [--snapshots 3781] [--book 1024] [--lag 1] [--window 256] [--reps 5]"""
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
ap.add_argument("--reps", type=int, default=5); ap.add_argument("--rate", type=float, default=0.03); ap.add_argument("--scen-per-wg", type=int, default=0)
ap.add_argument("--out")
a = ap.parse_args()
LEVELS = (0.05, 0.01)
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
calls = []
for n in range(a.underlyings):
    c, gen = SC.batch(a.snapshots, 16, 9, 1000 + n, per_kq=True, holes=0.0, rate=a.rate)
    r = np.random.default_rng(2000 + n)
    u = c["spot"][:, None] * r.uniform(0.7, 1.3, (a.snapshots, a.book))
    tau = r.uniform(3.0 / 365.0, 100.0 / 365.0, (a.snapshots, a.book))
    side, qty = dev((r.random(a.book) < 0.5).astype(np.uint8)), dev(np.round(r.uniform(-10.0, 10.0, a.book), 2))
    params, Tq, spot, u, tau = dev(gen["params"]), dev(c["Tq"]), dev(c["spot"]), dev(u), dev(tau)
    bk = engine.svi_book(params, Tq, spot, a.rate, u, tau, qty, is_put=side, strike_mode=1)
    hs = engine.svi_hsim(params, Tq, spot, a.rate, u, tau, qty, lag=a.lag, window=a.window, tail_probs=LEVELS, is_put=side, strike_mode=1)
    calls.append(dict(ins=(params, Tq, spot), q=(u, tau), side=side, qty=qty, bk=bk, hs=hs))
torch.cuda.synchronize()


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def hsim(stages):
    def run():
        for c in calls:
            engine.svi_hsim(*c["ins"], a.rate, *c["q"], c["qty"], lag=a.lag, window=a.window, tail_probs=LEVELS, is_put=c["side"], strike_mode=1, out=c["hs"],
                            stages=stages, scen_per_wg=a.scen_per_wg)
    return run


def book_all():
    for c in calls:
        engine.svi_book(*c["ins"], a.rate, *c["q"], c["qty"], is_put=c["side"], strike_mode=1, out=c["bk"])


def copy_pnl():
    for c, d in zip(calls, spare):
        d.copy_(c["hs"]["pnl"])


spare = [torch.empty_like(c["hs"]["pnl"]) for c in calls]
fl = torch.cat([c["hs"]["scen_flags"].reshape(-1) for c in calls])
existing = int((fl != 1).sum().item())
res = {"underlyings": a.underlyings, "snapshots": a.underlyings * a.snapshots, "book_size": a.book, "lag": a.lag, "window": a.window, "levels": LEVELS,
       "reps": a.reps, "scen_per_wg": a.scen_per_wg, "scenarios": existing, "valid_scenarios": int((fl == 0).sum().item()),
       "void_pair": int((fl == 2).sum().item()), "neg_vol": int((fl == 4).sum().item()), "dead_options": sum(int(c["hs"]["n_dead"].sum().item()) for c in calls)}
ms, lo, hi = events(hsim(1), a.reps)
pairs = existing * a.book
res["pnl_call"] = {"kernel": "svi_hsim_kernel", "option_scenarios": pairs, "ms": ms, "ms_min": lo, "ms_max": hi, "ns_per_option_scenario": ms * 1e6 / pairs,
                   "G_option_scenarios_per_s": pairs / ms / 1e6}
ms, lo, hi = events(hsim(2), a.reps)
cp, _, _ = events(copy_pnl, a.reps)
res["tail_call"] = {"kernel": engine.last_kernel(), "rows": a.underlyings * a.snapshots, "ms": ms, "ms_min": lo, "ms_max": hi,
                    "pnl_bytes": sum(s.numel() * 8 for s in spare), "copy_ms": cp, "over_copy": ms / cp}
ms, lo, hi = events(hsim(0), a.reps)
res["both"] = {"ms": ms, "ms_min": lo, "ms_max": hi}
ms, lo, hi = events(book_all, a.reps)
cells = sum(c["bk"]["cell_flags"].numel() for c in calls) * a.book * 2
res["book_all"] = {"kernel": engine.last_kernel(), "option_cell_dynamics": cells, "ms": ms, "ms_min": lo, "ms_max": hi, "ns_per_option_cell_dynamic": ms * 1e6 / cells}
res["hsim_over_book_per_price"] = res["pnl_call"]["ns_per_option_scenario"] / res["book_all"]["ns_per_option_cell_dynamic"]
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
