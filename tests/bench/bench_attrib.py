#!/usr/bin/env python3
"""VaR attribution on the workload of tests/bench/bench_hsim.py: U underlyings x B snapshots x 16 tenors, a
book of Q options, lag 1, a window of W scenarios and the levels 5 % and 1 %, twelve groups by expiry (equal spans of the
expiries at the first snapshot; the options are not sorted by expiry, so a wavefront holds all twelve groups) and both
per-option outputs.  Figures (HIP events round the Python calls, median of `reps` after one warm-up call, with min and max, summed
over the underlyings; every buffer is allocated once before the timing and kept): the attribution call, the same without the
per-option outputs, the same with one group, and the P&L call of ivs_svi_hsim_f64 (stages = 1) in the same run as the yardstick:
ns per (option, tail scenario) beside its ns per (option, scenario).  Prints one JSON line; --out FILE writes it there as well.
    python tests/bench/bench_attrib.py [--underlyings 4] [--snapshots 3781] [--book 1024] [--lag 1] [--window 256] [--reps 5]"""
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
ap.add_argument("--groups", type=int, default=12); ap.add_argument("--reps", type=int, default=5); ap.add_argument("--rate", type=float, default=0.03)
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
    group = np.minimum(((tau[0] - 3.0 / 365.0) / (97.0 / 365.0) * a.groups).astype(np.int32), a.groups - 1)
    side, qty = dev((r.random(a.book) < 0.5).astype(np.uint8)), dev(np.round(r.uniform(-10.0, 10.0, a.book), 2))
    params, Tq, spot, u, tau = dev(gen["params"]), dev(c["Tq"]), dev(c["spot"]), dev(u), dev(tau)
    kw = dict(lag=a.lag, window=a.window, tail_probs=LEVELS, is_put=side, strike_mode=1)
    hs = engine.svi_hsim(params, Tq, spot, a.rate, u, tau, qty, **kw)
    at = engine.svi_hsim_attrib(params, Tq, spot, a.rate, u, tau, qty, hs["pnl"], hs["scen_flags"], group=dev(group), n_groups=a.groups, **kw)
    one = engine.svi_hsim_attrib(params, Tq, spot, a.rate, u, tau, qty, hs["pnl"], hs["scen_flags"], n_groups=1, want=("ces_group", "cvar_group"), **kw)
    calls.append(dict(ins=(params, Tq, spot), q=(u, tau), qty=qty, kw=kw, hs=hs, at=at, one=one, group=dev(group)))
torch.cuda.synchronize()
for c in calls:                                                          # the bit link, on the bench's own data
    assert torch.equal(c["one"]["cvar_group"][:, :, 0].nan_to_num(1e300), c["hs"]["var"].nan_to_num(1e300))
    assert torch.equal(c["one"]["ces_group"][:, :, 0].nan_to_num(1e300), c["hs"]["es"].nan_to_num(1e300))


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def attrib(want, grouped=True):
    def run():
        for c in calls:
            out = c["at"] if grouped else c["one"]
            engine.svi_hsim_attrib(*c["ins"], a.rate, *c["q"], c["qty"], c["hs"]["pnl"], c["hs"]["scen_flags"], group=c["group"] if grouped else None,
                                   n_groups=a.groups if grouped else 1, want=want, out={k: out[k] for k in want + ("n_tail",)}, **c["kw"])
    return run


def hsim_pnl():
    for c in calls:
        engine.svi_hsim(*c["ins"], a.rate, *c["q"], c["qty"], out=c["hs"], stages=1, **c["kw"])


n_tail = torch.cat([c["at"]["n_tail"] for c in calls])
tail_scen = int(n_tail.max(dim=1).values.sum().item())                   # M per snapshot: the scenarios revalued
fl = torch.cat([c["hs"]["scen_flags"].reshape(-1) for c in calls])
existing = int((fl != 1).sum().item())
res = {"underlyings": a.underlyings, "snapshots": a.underlyings * a.snapshots, "book_size": a.book, "lag": a.lag, "window": a.window, "levels": LEVELS,
       "groups": a.groups, "reps": a.reps, "tail_scenarios": tail_scen, "max_tail": int(n_tail.max().item()), "scenarios": existing,
       "output_bytes": sum(c["at"][k].numel() * 8 for c in calls for k in ("ces", "cvar"))}
full = ("ces", "cvar", "ces_group", "cvar_group", "order")
pairs = tail_scen * a.book
for key, fn in (("attrib_call", attrib(full)), ("groups_only", attrib(("ces_group", "cvar_group", "order"))), ("options_only", attrib(("ces", "cvar"))),
                ("one_group", attrib(("ces_group", "cvar_group"), grouped=False))):
    ms, lo, hi = events(fn, a.reps)
    res[key] = {"kernel": engine.last_kernel(), "option_tail_scenarios": pairs, "ms": ms, "ms_min": lo, "ms_max": hi, "ns_per_option_tail_scenario": ms * 1e6 / pairs}
ms, lo, hi = events(hsim_pnl, a.reps)
res["pnl_call"] = {"kernel": "svi_hsim_kernel", "option_scenarios": existing * a.book, "ms": ms, "ms_min": lo, "ms_max": hi,
                   "ns_per_option_scenario": ms * 1e6 / (existing * a.book)}
res["attrib_over_pnl_per_option_scenario"] = res["attrib_call"]["ns_per_option_tail_scenario"] / res["pnl_call"]["ns_per_option_scenario"]
res["attrib_over_pnl_ms"] = res["attrib_call"]["ms"] / res["pnl_call"]["ms"]
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
