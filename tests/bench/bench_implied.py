#!/usr/bin/env python3
"""Price -> implied vol at the snapshot bench's size: U underlyings x B snapshots x a book of Q options.
Every snapshot has its own spot (a seeded random walk); the book holds Q (strike, expiry, side) round the first spot, expiries
from 4 to 180 days, vols from a skewed smile, and its prices come from engine.bs_price.  Prints one JSON line: the solver
(HIP events, median after warm-up, summed over the underlyings) with min and max, its option rate, the pricer timed the same
way, and for scale a device-to-device copy of the 48 B per option the solver moves (five float64 inputs and the vol): the
kernel is bound by fp64 arithmetic (2 + 64 evaluations of the equation per option, each 2 erfc, 1 exp2 and 1 division), not by
its bytes.  The events bracket the Python calls (tensor checks: a few tens of microseconds per call).
    python tests/bench/bench_implied.py [--underlyings 4] [--snapshots 3781] [--book 1024] [--reps 5]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from iv_interpolation_amd import _lib, engine

ap = argparse.ArgumentParser()
ap.add_argument("--underlyings", type=int, default=4); ap.add_argument("--snapshots", type=int, default=3781)
ap.add_argument("--book", type=int, default=1024); ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rate", type=float, default=0.03)
a = ap.parse_args()
dev = lambda x, dt=np.float64: torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()   # noqa: E731
calls = []
for u in range(a.underlyings):
    rng = np.random.default_rng(1700 + u)
    spot = 25000.0 * np.exp(np.cumsum(rng.normal(0, 5e-4, a.snapshots)))
    m = np.exp(rng.uniform(np.log(0.6), np.log(1.6), a.book))                  # strike / first spot
    T0 = rng.uniform(4.0, 180.0, a.book) / 365.0
    put = (rng.random(a.book) < 0.5).astype(np.uint8)
    k = np.log(m)
    sigma = np.sqrt(0.25 + 0.35 * (-0.4 * k + np.sqrt(k * k + 0.04)))          # a skewed smile, 0.5 at the money
    shape = (a.snapshots, a.book)
    S = np.broadcast_to(spot[:, None], shape)
    K = np.broadcast_to(25000.0 * m, shape)
    T = T0[None, :] - np.arange(a.snapshots)[:, None] / (365.0 * 1440.0)       # a snapshot per minute
    ins = dict(S=dev(S).ravel(), K=dev(K).ravel(), T=dev(T).ravel(), r=torch.full((S.size,), a.rate, dtype=torch.float64, device="cuda"),
               sigma=dev(np.broadcast_to(sigma, shape)).ravel(), put=dev(np.broadcast_to(put, shape), np.uint8).ravel())
    pr = engine.bs_price(ins["S"], ins["K"], ins["T"], ins["r"], ins["sigma"], is_put=ins["put"], want_vega=True)
    iv = engine.bs_implied_vol(pr["price"], ins["S"], ins["K"], ins["T"], ins["r"], is_put=ins["put"])
    calls.append((ins, pr, iv))
torch.cuda.synchronize()
n = sum(c[2]["vol"].numel() for c in calls)
count = lambda bit: sum(int(((c[2]["flags"] & bit) != 0).sum().item()) for c in calls)   # noqa: E731
err = max(float((c[2]["vol"] - c[0]["sigma"]).abs().nan_to_num(0.0).max().item()) for c in calls)


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def implied_all():
    for ins, pr, iv in calls:
        engine.bs_implied_vol(pr["price"], ins["S"], ins["K"], ins["T"], ins["r"], is_put=ins["put"], out=iv)


def price_all():
    for ins, pr, iv in calls:
        engine.bs_price(ins["S"], ins["K"], ins["T"], ins["r"], ins["sigma"], is_put=ins["put"], want_vega=True, out=pr)


src = [torch.empty(c[2]["vol"].numel() * 48, dtype=torch.uint8, device="cuda") for c in calls]
dst = [torch.empty_like(s) for s in src]


def copy_all():
    for s, d in zip(src, dst):
        d.copy_(s)


ms, ms_min, ms_max = events(implied_all, a.reps)
kernel = engine.last_kernel()
pms, pms_min, pms_max = events(price_all, a.reps)
cp_ms, _, _ = events(copy_all, a.reps)
res = {"underlyings": a.underlyings, "snapshots": a.underlyings * a.snapshots, "book": a.book, "options": n,
       "evaluations_per_option": 2 + 64, "erfc_per_option": 2 * (2 + 64), "kernel": kernel, "reps": a.reps,
       "itm_options": count(_lib.IV_ITM), "below_options": count(_lib.IV_BELOW), "above_options": count(_lib.IV_ABOVE),
       "dead_options": count(_lib.IV_DEAD), "edge_options": count(_lib.IV_EDGE), "max_abs_vol_minus_sigma": err,
       "bytes_per_option": 48, "implied_ms": ms, "implied_ms_min": ms_min, "implied_ms_max": ms_max,
       "implied_Moptions_per_s": n / ms / 1e3, "price_ms": pms, "price_ms_min": pms_min, "price_ms_max": pms_max,
       "price_Moptions_per_s": n / pms / 1e3, "copy_ms": cp_ms, "implied_over_copy": ms / cp_ms}
print(json.dumps(res))
