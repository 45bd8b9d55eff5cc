#!/usr/bin/env python3
"""Age-weighted, volatility-scaled VaR and ES on the workload of tests/bench/bench_hsim.py: U underlyings x B
snapshots x 16 tenors, a book of Q options, lag 1, a window of W scenarios and the levels 5 % and 1 %.  The rows are section 19's own
(one svi_hsim call per underlying, outside the timing).  Figures (HIP events round the calls, median of `reps` after one warm-up
call, with min and max, summed over the underlyings; every buffer is allocated once before the timing and kept): the weighted call at
M = 0 with decay 0.99 (hsim_wtail_kernel alone), at M = 64 with decay 0.99 and vol decay 0.94 (both launches), its stage 1 alone
(spot_ewma_kernel), and in the same run stage 2 of ivs_svi_hsim_f64 on pnl (hsim_tail_kernel) and a device copy of pnl.  The
yardstick is the tail kernel's time of the same run.  Beside them, per level, the back-test of the plain and of the weighted VaR
against the book's realised P&L over the next lag snapshots (svi_explain's net actual), with Kupiec's likelihood ratio.  Prints one
JSON line; --out FILE writes it there as well.
    python tests/bench/bench_weighted.py [--underlyings 4] [--snapshots 3781] [--book 1024] [--lag 1] [--window 256] [--vol-span 64]"""
import argparse, ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from iv_interpolation_amd import _lib, engine
from complete_pipeline import kupiec_lr
import svi_cases as SC

ap = argparse.ArgumentParser()
ap.add_argument("--underlyings", type=int, default=4); ap.add_argument("--snapshots", type=int, default=3781)
ap.add_argument("--book", type=int, default=1024); ap.add_argument("--lag", type=int, default=1); ap.add_argument("--window", type=int, default=256)
ap.add_argument("--decay", type=float, default=0.99); ap.add_argument("--vol-span", type=int, default=64); ap.add_argument("--vol-decay", type=float, default=0.94)
ap.add_argument("--reps", type=int, default=5); ap.add_argument("--rate", type=float, default=0.03); ap.add_argument("--out")
a = ap.parse_args()
LEVELS = (0.05, 0.01)
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
lib = _lib.load()
weight, vol_weight = dev(engine.age_weights(a.window, a.decay)), dev(engine.age_weights(a.vol_span, a.vol_decay))
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
    actual = engine.svi_explain(*ins, a.rate, u, tau, qty, lag=a.lag, is_put=side, strike_mode=1, want=())["net"][:, 0].clone()
    B = a.snapshots
    f64, i32 = torch.float64, torch.int32
    shapes = dict(var_w=((B, 2), f64), es_w=((B, 2), f64), n_valid_w=((B,), i32), worst_w=((B,), i32), wsum=((B,), f64), n_eff=((B,), f64),
                  pnl_w=((B, a.window), f64), scale=((B, a.window), f64), flags_w=((B, a.window), i32), sigma=((B,), f64))
    out = {k: torch.empty(s, dtype=dt, device="cuda") for k, (s, dt) in shapes.items()}
    args = _lib.WeightedArgs()
    args.pnl, args.scen_flags, args.B, args.window, args.lag = hs["pnl"].data_ptr(), hs["scen_flags"].data_ptr(), B, a.window, a.lag
    args.tail_probs, args.nL, args.min_scen = engine._doubles(list(LEVELS)), 2, 20
    args.weight, args.spot, args.vol_weight = weight.data_ptr(), ins[2].data_ptr(), vol_weight.data_ptr()
    args.min_returns, args.scale_cap = min(20, a.vol_span), 3.0
    for k, v in out.items():
        setattr(args, k, v.data_ptr())
    calls.append(dict(ins=ins, q=(u[:, :1].contiguous(), tau[:, :1].contiguous(), qty[:1].contiguous()), kw=kw, hs=hs, out=out, args=args, actual=actual,
                      copy_pnl=torch.empty_like(hs["pnl"])))
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


def weighted(vol_span, stages):
    def fn():
        st = torch.cuda.current_stream().cuda_stream
        for c in calls:
            c["args"].vol_span, c["args"].stages = vol_span, stages
            rc = lib.ivs_hsim_weighted_f64(ctypes.byref(c["args"]), None, 0, st)
            assert rc == 0, lib.ivs_last_error()
    return fn


def hsim_tail():
    for c in calls:
        engine.svi_hsim(*c["ins"], a.rate, *c["q"], out=c["hs"], stages=2, value=False, **c["kw"])


def copy_pnl():
    for c in calls:
        c["copy_pnl"].copy_(c["hs"]["pnl"])


def backtest(c, var):
    """run_var's rule on one underlying: eligible = a finite VaR and a finite actual P&L of the pair p -> p + lag."""
    elig, exc = [], []
    for l in range(len(LEVELS)):
        v = var[:-a.lag, l] if a.lag else var[:, l]
        ok = torch.isfinite(v) & torch.isfinite(c["actual"])
        elig.append(int(ok.sum().item())); exc.append(int((ok & (c["actual"] < -v)).sum().item()))
    return elig, exc


snaps = a.underlyings * a.snapshots
res = {"underlyings": a.underlyings, "snapshots": snaps, "book_size": a.book, "lag": a.lag, "window": a.window, "levels": LEVELS, "decay": a.decay,
       "vol_span": a.vol_span, "vol_decay": a.vol_decay, "reps": a.reps, "pnl_bytes": sum(c["hs"]["pnl"].numel() * 8 for c in calls)}
tests = {}
for key, fn, kernel in [("weighted_M0", weighted(0, 0), "hsim_wtail_kernel"), (f"weighted_M{a.vol_span}", weighted(a.vol_span, 0), "spot_ewma_kernel + hsim_wtail_kernel"),
                        ("sigma_alone", weighted(a.vol_span, 1), "spot_ewma_kernel"), ("hsim_tail", hsim_tail, "hsim_tail_kernel"), ("copy_pnl", copy_pnl, "device copy")]:
    ms, lo, hi = events(fn, a.reps)
    res[key] = {"kernel": kernel, "ms": ms, "ms_min": lo, "ms_max": hi}
    if key.startswith("weighted_M"):                         # the figures of this setting, while the buffers hold them
        torch.cuda.synchronize()
        tot = [np.zeros(2, np.int64), np.zeros(2, np.int64)]
        for c in calls:
            e, x = backtest(c, c["out"]["var_w"])
            tot[0] += e; tot[1] += x
        tests[key] = tot
        res[key]["median_n_eff"] = float(torch.nanmedian(torch.cat([c["out"]["n_eff"] for c in calls])).item())
        res[key]["active_rows"] = int(sum(torch.isfinite(c["out"]["var_w"][:, 0]).sum().item() for c in calls))
plain = [np.zeros(2, np.int64), np.zeros(2, np.int64)]
for c in calls:
    e, x = backtest(c, c["hs"]["var"])
    plain[0] += e; plain[1] += x
tests["plain"] = plain
for key in ("weighted_M0", f"weighted_M{a.vol_span}"):
    res[key]["over_hsim_tail"] = res[key]["ms"] / res["hsim_tail"]["ms"]
res["sigma_alone"]["over_hsim_tail"] = res["sigma_alone"]["ms"] / res["hsim_tail"]["ms"]
res["kupiec"] = [{"tp": tp, **{k: {"eligible": int(t[0][l]), "exceedances": int(t[1][l]), "lr": kupiec_lr(int(t[0][l]), int(t[1][l]), tp)} for k, t in tests.items()}}
                 for l, tp in enumerate(LEVELS)]
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
