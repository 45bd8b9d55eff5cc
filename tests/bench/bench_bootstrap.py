#!/usr/bin/env python3
"""Bootstrap standard errors and intervals for a book's VaR and ES on the workload of tests/bench/bench_hsim.py:
U underlyings x B snapshots x 16 tenors, a book of Q options, lag 1, a window of W scenarios and the levels 5 % and 1 %.  The rows
are section 19's own (one svi_hsim call per underlying, outside the timing).  Figures (HIP events round the Python calls, median of
`reps` after one warm-up call, with min and max, summed over the underlyings; every buffer, the workspace included, is allocated
once before the timing and kept): the bootstrap at R replicates with ci (0.05, 0.95) and no rep, at block 1 and at block 8, and in
the same run stage 2 of ivs_svi_hsim_f64 on pnl (hsim_tail_kernel: what ranking one resample would cost), a device copy of pnl and a
device copy of the workspace.  The yardstick is R times the tail kernel's time.  Prints one JSON line; --out FILE writes it there
as well.
    python tests/bench/bench_bootstrap.py [--underlyings 4] [--snapshots 3781] [--book 1024] [--lag 1] [--window 256] [--replicates 512]"""
import argparse, ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from iv_interpolation_amd import _lib, engine
import svi_cases as SC

ap = argparse.ArgumentParser()
ap.add_argument("--underlyings", type=int, default=4); ap.add_argument("--snapshots", type=int, default=3781)
ap.add_argument("--book", type=int, default=1024); ap.add_argument("--lag", type=int, default=1); ap.add_argument("--window", type=int, default=256)
ap.add_argument("--replicates", type=int, default=512); ap.add_argument("--blocks", default="1,8")
ap.add_argument("--reps", type=int, default=5); ap.add_argument("--rate", type=float, default=0.03); ap.add_argument("--out")
a = ap.parse_args()
LEVELS, CI = (0.05, 0.01), (0.05, 0.95)
BLOCKS = [int(x) for x in a.blocks.split(",")]
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
lib = _lib.load()
calls = []
for n in range(a.underlyings):
    c, gen = SC.batch(a.snapshots, 16, 9, 1000 + n, per_kq=True, holes=0.0, rate=a.rate)
    r = np.random.default_rng(2000 + n)
    u = c["spot"][:, None] * r.uniform(0.7, 1.3, (a.snapshots, a.book))
    tau = r.uniform(3.0 / 365.0, 100.0 / 365.0, (a.snapshots, a.book))
    side, qty = dev((r.random(a.book) < 0.5).astype(np.uint8)), dev(np.round(r.uniform(-10.0, 10.0, a.book), 2))
    ins = (dev(gen["params"]), dev(c["Tq"]), dev(c["spot"]))
    u, tau = dev(u), dev(tau)
    kw = dict(lag=a.lag, window=a.window, tail_probs=LEVELS, strike_mode=1)
    hs = engine.svi_hsim(*ins, a.rate, u, tau, qty, is_put=side, **kw)
    B = a.snapshots
    out = {k: torch.empty(s, dtype=torch.float64, device="cuda") for k, s in (("var0", (B, 2)), ("es0", (B, 2)), ("mean", (B, 2, 2)), ("variance", (B, 2, 2)),
                                                                               ("quant", (B, 2, 2, 2)))}
    out["n_scen"] = torch.empty(B, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.ivs_hsim_bootstrap_workspace_bytes(B, a.replicates, 2) // 8, dtype=torch.float64, device="cuda")
    args = _lib.BootstrapArgs()
    args.pnl, args.scen_flags, args.B, args.window = hs["pnl"].data_ptr(), hs["scen_flags"].data_ptr(), B, a.window
    args.tail_probs, args.ci_probs = engine._doubles(list(LEVELS)), engine._doubles(list(CI))
    args.nL, args.nC, args.min_scen, args.n_rep, args.seed = 2, 2, 20, a.replicates, 0
    for k, v in out.items():
        setattr(args, k, v.data_ptr())
    calls.append(dict(ins=ins, q=(u[:, :1].contiguous(), tau[:, :1].contiguous(), qty[:1].contiguous()), kw=kw, hs=hs, out=out, ws=ws, args=args,
                      copy_pnl=torch.empty_like(hs["pnl"]), copy_ws=torch.empty_like(ws)))
    print(f"underlying {n}: ready", file=sys.stderr, flush=True)
    del u, tau
torch.cuda.synchronize()


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def bootstrap(block):
    def fn():
        st = torch.cuda.current_stream().cuda_stream
        for c in calls:
            c["args"].block = block
            rc = lib.ivs_hsim_bootstrap_f64(ctypes.byref(c["args"]), c["ws"].data_ptr(), c["ws"].numel() * 8, st)
            assert rc == 0, lib.ivs_last_error()
    return fn


def hsim_tail():
    for c in calls:
        engine.svi_hsim(*c["ins"], a.rate, *c["q"], out=c["hs"], stages=2, value=False, **c["kw"])


def copy_pnl():
    for c in calls:
        c["copy_pnl"].copy_(c["hs"]["pnl"])


def copy_ws():
    for c in calls:
        c["copy_ws"].copy_(c["ws"])


snaps = a.underlyings * a.snapshots
res = {"underlyings": a.underlyings, "snapshots": snaps, "book_size": a.book, "lag": a.lag, "window": a.window, "levels": LEVELS, "ci": CI,
       "replicates": a.replicates, "reps": a.reps, "pnl_bytes": sum(c["hs"]["pnl"].numel() * 8 for c in calls),
       "workspace_bytes": sum(c["ws"].numel() * 8 for c in calls)}
for key, fn, kernel in [(f"bootstrap_L{b}", bootstrap(b), "hsim_bootstrap_kernel") for b in BLOCKS] + [
        ("hsim_tail", hsim_tail, "hsim_tail_kernel"), ("copy_pnl", copy_pnl, "device copy"), ("copy_workspace", copy_ws, "device copy")]:
    ms, lo, hi = events(fn, a.reps)
    res[key] = {"kernel": kernel, "ms": ms, "ms_min": lo, "ms_max": hi}
n_act = int(sum((c["out"]["n_scen"] >= 20).sum().item() for c in calls))
draws = float(sum(c["out"]["n_scen"].double().sum().item() for c in calls)) * a.replicates
se = torch.cat([torch.sqrt(c["out"]["variance"][:, 0, :]) / c["out"]["var0"] for c in calls])
res["active_rows"], res["draws"] = n_act, draws
res["median_rel_se_block"] = BLOCKS[-1]
res["median_rel_se_var"] = [float(torch.nanmedian(se[:, l]).item()) for l in range(2)]
res["yardstick_ms"] = res["hsim_tail"]["ms"] * a.replicates
for b in BLOCKS:
    k = f"bootstrap_L{b}"
    res[k]["ns_per_replicate"] = res[k]["ms"] * 1e6 / (snaps * a.replicates)
    res[k]["ps_per_draw"] = res[k]["ms"] * 1e9 / draws if draws else float("nan")
    res[k]["over_yardstick"] = res[k]["ms"] / res["yardstick_ms"]
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
