"""Thin device-side wrappers: torch-ROCm tensors are only device buffers and streams here;
all arithmetic happens in the HIP kernels behind the C ABI (include/ivs.h)."""
from __future__ import annotations

from typing import Optional, Tuple

from . import _lib
from ._lib import EngineUnavailable


def _torch():
    import torch
    return torch


def require_device():
    """Return torch, after checking that the HIP library loads and a GPU is visible."""
    lib = _lib.load()
    torch = _torch()
    if not torch.cuda.is_available() or lib.ivs_device_count() < 1:
        raise EngineUnavailable("no MI355X / HIP device visible: the interpolation engine has no CPU fallback")
    return torch


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _stream(torch, stream):
    s = torch.cuda.current_stream() if stream is None else stream
    return s.cuda_stream


def _f64(torch, t, name):
    if t.dtype != torch.float64 or not t.is_cuda:
        raise TypeError(f"{name} must be a CUDA float64 tensor")
    return t.contiguous()


def _hold_for_stream(torch, stream, *tensors):
    """Tensors that were allocated on torch's CURRENT stream (per-call workspaces, contiguous temporaries, outputs) but are
    read or written by kernels launched on an explicit `stream`: tell the caching allocator, so that the block is not
    handed to the next allocation on the current stream while those kernels still run."""
    if stream is None or stream == torch.cuda.current_stream():
        return
    for t in tensors:
        if t is not None and t.is_cuda:
            t.record_stream(stream)


# ---- the host checks and call steps the snapshot-analytics wrappers share

def _tenor_inputs(Tq, spot, B, mT):
    if Tq.dim() not in (1, 2) or Tq.shape[-1] != mT or (Tq.dim() == 2 and Tq.shape[0] != B):
        raise ValueError("Tq must be [mT] or [B, mT]")
    if spot.numel() != B:
        raise ValueError("spot must hold one price per surface")


def _surface_inputs(torch, vol, Kq, Tq, spot):
    """The shared input checks of the stages that read surfaces: vol [B,mT,mK], Kq [mK] or [B,mK], Tq [mT] or [B,mT], spot [B]."""
    vol = _f64(torch, vol, "vol"); Kq = _f64(torch, Kq, "Kq"); Tq = _f64(torch, Tq, "Tq"); spot = _f64(torch, spot, "spot")
    if vol.dim() != 3:
        raise ValueError("vol must be [B, mT, mK]")
    B, mT, mK = vol.shape
    if Kq.dim() not in (1, 2) or Kq.shape[-1] != mK or (Kq.dim() == 2 and Kq.shape[0] != B):
        raise ValueError("Kq must be [mK] or [B, mK]")
    _tenor_inputs(Tq, spot, B, mT)
    return vol, Kq, Tq, spot, B, mT, mK


def _svi_inputs(torch, params, Tq, spot, max_tenors=_lib.ST_MAX_TENORS):
    """The shared input checks of the stages that read SVI slices: params [B,mT,5], Tq [mT] or [B,mT], spot [B], and at most
    max_tenors slices per snapshot (None: no limit)."""
    params = _f64(torch, params, "params"); Tq = _f64(torch, Tq, "Tq"); spot = _f64(torch, spot, "spot")
    if params.dim() != 3 or params.shape[-1] != 5:
        raise ValueError("params must be [B, mT, 5]")
    B, mT, _ = params.shape
    _tenor_inputs(Tq, spot, B, mT)
    if max_tenors is not None and mT > max_tenors:
        raise ValueError(f"mT = {mT}: at most {max_tenors} tenors per snapshot are supported")
    return params, Tq, spot, B, mT


def _surface_fields(a, vol, Kq, Tq, spot, rate):
    """The fields every args struct of a surface stage has: the surfaces, their two grids, the spots and the rate."""
    B, mT, mK = vol.shape
    a.vol, a.Kq, a.kq_stride = _ptr(vol), _ptr(Kq), (0 if Kq.dim() == 1 else mK)
    a.Tq, a.tq_stride, a.spot, a.rate = _ptr(Tq), (0 if Tq.dim() == 1 else mT), _ptr(spot), float(rate)
    a.mK, a.mT, a.B = mK, mT, B
    return a


def _slice_fields(a, params, Tq, spot, rate=None):
    """The fields every args struct of a stage on SVI slices has (the calendar has no rate)."""
    B, mT, _ = params.shape
    a.params, a.Tq, a.tq_stride, a.spot = _ptr(params), _ptr(Tq), (0 if Tq.dim() == 1 else mT), _ptr(spot)
    a.mT, a.B = mT, B
    if rate is not None:
        a.rate = float(rate)
    return a


def _query_fields(a, u, tau, strike_mode):
    Q = u.shape[-1]
    a.u, a.tau, a.q_stride, a.strike_mode, a.Q = _ptr(u), _ptr(tau), (0 if u.dim() == 1 else Q), int(strike_mode), Q


def _doubles(xs):
    """A short host list as the const double* of an args struct (one slot even when empty).  The pointer keeps its array
    alive, and the struct the pointer."""
    import ctypes
    return ctypes.cast((ctypes.c_double * max(len(xs), 1))(*xs), ctypes.POINTER(ctypes.c_double))


def _wanted(want, names):
    want = tuple(want)
    if any(k not in names for k in want):
        raise ValueError(f"want must name outputs among {names}, got {want!r}")
    return want


def _outputs(torch, out, shapes, device, per_option=False):
    """`out` (a dict of preallocated tensors, or None) completed to every key of shapes = {key: (shape, dtype, wanted)}: a
    tensor given is checked, one missing is allocated, one not wanted is None.  per_option: the flat pricers take a tensor
    given in any shape with as many elements."""
    import math
    out = dict(out or {})
    for k, (shape, dt, on) in shapes.items():
        t = out.get(k)
        if not on:
            out[k] = None
        elif t is None:
            out[k] = torch.empty(shape, dtype=dt, device=device)
        else:
            bad_shape = t.numel() != math.prod(shape) if per_option else tuple(t.shape) != shape
            if bad_shape or t.dtype != dt or not t.is_cuda or not t.is_contiguous():
                what = "with one entry per option" if per_option else f"of shape {shape}"
                raise ValueError(f"out[{k!r}] must be a contiguous CUDA {dt} tensor {what}")
    return out


def _call(torch, name, a, stream, *tensors):
    """Run the C entry point `name` on the args struct, keep `tensors` alive for `stream`, raise EngineError on failure."""
    rc = getattr(_lib.load(), name)(a, None, 0, _stream(torch, stream))
    _hold_for_stream(torch, stream, *tensors)
    _lib.check(rc, name)


def validate_ragged(K, sigma, k_off, nK_max: int, n_maturities: int):
    """Optional host-side check of CSR offsets with a readable exception (one small device reduction + one D2H read, i.e. it
    SYNCHRONISES: not for capture).  The kernels do not depend on it: they check every span against nK_max and against the
    total strike count passed through the C ABI and flag offending surfaces with ST_BAD_SHAPE."""
    torch = _torch()
    if k_off.numel() < 1:
        raise ValueError("k_off must hold B+1 offsets")
    span = k_off[1:] - k_off[:-1]
    stats = torch.stack([k_off[0], k_off[-1], span.min() if span.numel() else k_off[0] * 0,
                         span.max() if span.numel() else k_off[0] * 0]).tolist()
    first, last, smin, smax = (int(v) for v in stats)
    if first != 0 or smin < 0:
        raise ValueError("k_off must start at 0 and be non-decreasing")
    if smax > nK_max:
        raise ValueError(f"k_off: a surface has {smax} strikes but nK_max={nK_max}")
    if K.numel() != last or sigma.numel() != n_maturities * last:
        raise ValueError(f"ragged batch: K has {K.numel()} and sigma {sigma.numel()} entries, k_off[-1]={last}, nT={n_maturities}")


def surface_workspace(B: int, ragged: bool, device=None):
    """Device scratch for one surface_batch call (ivs_surface_workspace_bytes): uint8 CUDA tensor, 256-byte aligned."""
    torch = require_device()
    n = _lib.load().ivs_surface_workspace_bytes(int(B), 1 if ragged else 0)
    return torch.empty(n, dtype=torch.uint8, device=device or "cuda")


def surface_batch(K, T, sigma, Kq, Tq, method="linear", *, k_off=None, nK_max: Optional[int] = None,
                  n_maturities: Optional[int] = None, out=None, status=None, stream=None,
                  force_generic: bool = False, workspace=None, map_groups: int = 0, one_pass: bool = False,
                  validate: bool = False):
    """Interpolate a batch of (strike x maturity) surfaces on the current device.

    Uniform: K [B,nK] or [nK] (shared), sigma [B,nT,nK].  Ragged: K flat [total], sigma flat
    [nT*total] (surface b row-major [nT][nK_b]), k_off int64 [B+1], nK_max, n_maturities.
    T [nT] or [B,nT]; Kq [mK] or [B,mK]; Tq [mT] or [B,mT].  Returns (out [B,mT,mK], status [B]).
    `workspace`: uint8 CUDA tensor from surface_workspace() (allocated per call when omitted; pass one to keep the
    call allocation-free, e.g. under hipGraph capture).  Ragged offsets are checked ON THE DEVICE (a surface whose span is
    negative, exceeds nK_max or leaves K gets ST_BAD_SHAPE and is skipped), so the call never synchronises;
    `validate=True` adds validate_ragged()'s host-side check (one D2H read) with a readable exception.
    """
    torch = require_device()
    lib = _lib.load()
    code = _lib.METHOD_CODES[method] if isinstance(method, str) else int(method)
    K = _f64(torch, K, "K"); T = _f64(torch, T, "T"); sigma = _f64(torch, sigma, "sigma")
    Kq = _f64(torch, Kq, "Kq"); Tq = _f64(torch, Tq, "Tq")
    if k_off is None:
        B, nT, nK = sigma.shape
        k_stride = 0 if K.dim() == 1 else nK
        if K.shape[-1] != nK or (K.dim() == 2 and K.shape[0] != B):
            raise ValueError("K shape does not match sigma")
    else:
        if k_off.dtype != torch.int64 or not k_off.is_cuda:
            raise TypeError("k_off must be a CUDA int64 tensor")
        if nK_max is None or n_maturities is None:
            raise ValueError("ragged batches need nK_max and n_maturities")
        k_off = k_off.contiguous()
        B = k_off.numel() - 1; nT = int(n_maturities); nK = int(nK_max)
        if B < 0:
            raise ValueError("k_off must hold B+1 offsets")
        if sigma.numel() != nT * K.numel():
            raise ValueError(f"ragged batch: K has {K.numel()} strikes, sigma {sigma.numel()} quotes, nT={nT}")
        if validate:
            validate_ragged(K, sigma, k_off, nK, nT)
        k_stride = K.numel()       # ragged: the C ABI takes the total strike count here and bounds every span by it
    if T.shape[-1] != nT or (T.dim() == 2 and T.shape[0] != B):
        raise ValueError("T shape does not match sigma")
    t_stride = 0 if T.dim() == 1 else nT
    mK, mT = Kq.shape[-1], Tq.shape[-1]
    if (Kq.dim() == 2 and Kq.shape[0] != B) or (Tq.dim() == 2 and Tq.shape[0] != B):
        raise ValueError("per-surface query grids must have B rows")
    kq_stride = 0 if Kq.dim() == 1 else mK
    tq_stride = 0 if Tq.dim() == 1 else mT
    if out is None:
        out = torch.empty((B, mT, mK), dtype=torch.float64, device=sigma.device)
    if status is None:
        status = torch.empty((B,), dtype=torch.int32, device=sigma.device)
    need = lib.ivs_surface_workspace_bytes(B, 0 if k_off is None else 1)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=sigma.device)
    elif workspace.numel() * workspace.element_size() < need or not workspace.is_cuda:
        raise ValueError(f"workspace too small: {workspace.numel() * workspace.element_size()} < {need} bytes")
    flags = ((_lib.FLAG_FORCE_GENERIC if force_generic else 0) | (_lib.FLAG_ONE_PASS if one_pass else 0)
             | _lib.flag_map_groups(map_groups))
    rc = lib.ivs_surface_batch_f64(_ptr(K), _ptr(k_off), k_stride, nK, _ptr(T), t_stride, nT, _ptr(sigma), B,
                                   _ptr(Kq), kq_stride, mK, _ptr(Tq), tq_stride, mT, _ptr(out), _ptr(status),
                                   code, flags, _ptr(workspace), workspace.numel() * workspace.element_size(),
                                   _stream(torch, stream))
    _hold_for_stream(torch, stream, K, T, sigma, Kq, Tq, k_off, out, status, workspace)
    _lib.check(rc, "ivs_surface_batch_f64")
    return out, status


def snapshot_assemble(date_ns, iv, underlying, row_off, cells, strike, expiry_ns, t0_ns: int, n_snapshots: int,
                      moneyness=None, kq_empty: float = 0.0, *, out=None, stream=None):
    """Per-minute snapshot arrays of ONE underlying from its interpolated chain (ivs_snapshot_assemble_f64; rules S4-S7
    of DESIGN.md section 8).  Rows: date_ns int64, iv / underlying float64 [n_rows], contract after contract (row_off
    int64 [C+1]), date-sorted inside a contract; cells int32 [nT*nK, 2] (call / put contract, -1 = none); strike float64
    [nK]; expiry_ns int64 [nT]; all CUDA tensors.  moneyness float64 [mK] or None switches the Kq output on.
    `out`: optional dict of preallocated outputs (keys sigma [B,nT,nK], T [B,nT], spot [B], quotes int32 [B], Kq [B,mK]).
    Returns dict(sigma, T, spot, quotes, Kq) of device tensors (Kq None without moneyness)."""
    torch = require_device()
    iv = _f64(torch, iv, "iv"); underlying = _f64(torch, underlying, "underlying"); strike = _f64(torch, strike, "strike")
    for t, name, dt in ((date_ns, "date_ns", torch.int64), (row_off, "row_off", torch.int64), (cells, "cells", torch.int32),
                        (expiry_ns, "expiry_ns", torch.int64)):
        if t.dtype != dt or not t.is_cuda:
            raise TypeError(f"{name} must be a CUDA {dt} tensor")
    date_ns, row_off, cells, expiry_ns = date_ns.contiguous(), row_off.contiguous(), cells.contiguous(), expiry_ns.contiguous()
    n = iv.numel()
    if date_ns.numel() != n or underlying.numel() != n:
        raise ValueError("date_ns, iv and underlying must have one entry per row")
    nK, nT, B = strike.numel(), expiry_ns.numel(), int(n_snapshots)
    if cells.numel() != 2 * nT * nK:
        raise ValueError(f"cells must be [nT*nK, 2] = [{nT * nK}, 2]")
    if moneyness is not None:
        moneyness = _f64(torch, moneyness, "moneyness")
    mK = 0 if moneyness is None else moneyness.numel()
    shapes = {"sigma": ((B, nT, nK), torch.float64, True), "T": ((B, nT), torch.float64, True),
              "spot": ((B,), torch.float64, True), "quotes": ((B,), torch.int32, True),
              "Kq": ((B, mK), torch.float64, moneyness is not None)}
    out = _outputs(torch, out, shapes, iv.device)
    a = _lib.SnapshotArgs()
    a.date_ns, a.iv, a.underlying, a.n_rows = _ptr(date_ns), _ptr(iv), _ptr(underlying), n
    a.row_off, a.n_contracts = _ptr(row_off), row_off.numel() - 1
    a.cells, a.strike, a.expiry_ns, a.nT, a.nK = _ptr(cells), _ptr(strike), _ptr(expiry_ns), nT, nK
    a.t0_ns, a.n_snapshots = int(t0_ns), B
    a.moneyness, a.mK, a.kq_empty = _ptr(moneyness), mK, float(kq_empty)
    a.sigma, a.T, a.spot, a.quotes, a.Kq = (_ptr(out[k]) for k in ("sigma", "T", "spot", "quotes", "Kq"))
    _call(torch, "ivs_snapshot_assemble_f64", a, stream, date_ns, iv, underlying, row_off, cells, strike, expiry_ns, moneyness,
          *out.values())
    return out


DEFAULT_DELTAS = (-0.10, -0.25, 0.5, 0.25, 0.10)      # rule D3: 10d put, 25d put, ATM, 25d call, 10d call


def delta_targets(deltas):
    """Rule D3 on the host: signed deltas -> z = inv_cdf(call delta), a put delta d in (-1, 0) meaning the call delta 1 + d.
    Anything outside (-1, 0) and (0, 1), an empty list or more than 16 targets raises ValueError."""
    from statistics import NormalDist
    deltas = [float(d) for d in deltas]
    if not 1 <= len(deltas) <= _lib.SM_MAX_TARGETS:
        raise ValueError(f"{len(deltas)} target deltas: between 1 and {_lib.SM_MAX_TARGETS} are supported")
    inv = NormalDist().inv_cdf
    z = []
    for d in deltas:
        if 0.0 < d < 1.0:
            z.append(inv(d))
        elif -1.0 < d < 0.0:
            z.append(inv(1.0 + d))
        else:
            raise ValueError(f"target delta {d!r} is outside (-1, 0) and (0, 1)")
    return z


def smile_delta_points(vol, Kq, Tq, spot, deltas=DEFAULT_DELTAS, rate: float = 0.0, *, out=None, stream=None,
                       rows_per_wave: int = 0):
    """Delta-quoted smile points of a batch of surfaces (ivs_smile_delta_points_f64; rules D1-D6 of DESIGN.md section 9).
    vol float64 [B,mT,mK] (the `out` of surface_batch); Kq [mK] or [B,mK]; Tq [mT] or [B,mT]; spot [B]; all CUDA tensors.
    deltas: 1..16 signed targets (call deltas in (0,1), put deltas in (-1,0), ATM = 0.5); rate: the scalar r of d1.
    `out`: optional dict of preallocated outputs (keys vol, strike float64 [B,mT,nD], flags int32 [B,mT,nD]).
    rows_per_wave: 0 lets the call choose how many rows share a wavefront; 1..64 // nD forces it (tuning / testing; the
    results are the same bit for bit).
    Returns dict(vol, strike, flags) of device tensors; flags are the _lib.SM_* bits."""
    z = delta_targets(deltas)
    torch = require_device()
    vol, Kq, Tq, spot, B, mT, mK = _surface_inputs(torch, vol, Kq, Tq, spot)
    nD = len(z)
    shapes = {"vol": ((B, mT, nD), torch.float64, True), "strike": ((B, mT, nD), torch.float64, True),
              "flags": ((B, mT, nD), torch.int32, True)}
    out = _outputs(torch, out, shapes, vol.device)
    a = _surface_fields(_lib.SmileArgs(), vol, Kq, Tq, spot, rate)
    a.z, a.nD = _doubles(z), nD
    a.q_vol, a.q_strike, a.q_flags = _ptr(out["vol"]), _ptr(out["strike"]), _ptr(out["flags"])
    a.rows_per_wave = int(rows_per_wave)
    _call(torch, "ivs_smile_delta_points_f64", a, stream, vol, Kq, Tq, spot, *out.values())
    return out


def surface_arbitrage(vol, Kq, Tq, spot, rate: float = 0.0, *, local_vol: bool = True, density: bool = True, out=None,
                      stream=None):
    """Static-arbitrage report, Dupire local vol and risk-neutral density of a batch of surfaces
    (ivs_surface_arbitrage_f64; rules A1-A7 of DESIGN.md section 10).  vol float64 [B,mT,mK] (the `out` of surface_batch);
    Kq [mK] or [B,mK]; Tq [mT] or [B,mT]; spot [B]; all CUDA tensors; mK >= 3, mT >= 2.  rate: the scalar r.
    local_vol / density: False leaves that field out (it is neither computed nor written).
    `out`: optional dict of preallocated outputs (keys flags int32 [B,mT,mK], counts int32 [B,4], worst float64 [B,2],
    local_vol, density float64 [B,mT,mK]).
    Returns dict(flags, counts, worst, local_vol, density) of device tensors (None for a field left out); flags are the
    _lib.AR_* bits, counts = evaluated, calendar, butterfly, finite local-vol nodes, worst = min numerator, min g."""
    torch = require_device()
    vol, Kq, Tq, spot, B, mT, mK = _surface_inputs(torch, vol, Kq, Tq, spot)
    shapes = {"flags": ((B, mT, mK), torch.int32, True), "counts": ((B, 4), torch.int32, True),
              "worst": ((B, 2), torch.float64, True), "local_vol": ((B, mT, mK), torch.float64, bool(local_vol)),
              "density": ((B, mT, mK), torch.float64, bool(density))}
    out = _outputs(torch, out, shapes, vol.device)
    a = _surface_fields(_lib.ArbitrageArgs(), vol, Kq, Tq, spot, rate)
    a.flags, a.counts, a.worst = _ptr(out["flags"]), _ptr(out["counts"]), _ptr(out["worst"])
    a.local_vol, a.density = _ptr(out["local_vol"]), _ptr(out["density"])
    _call(torch, "ivs_surface_arbitrage_f64", a, stream, vol, Kq, Tq, spot, *out.values())
    return {k: out[k] for k in shapes}


def surface_moments(vol, Kq, Tq, spot, rate: float = 0.0, *, horizons=(30.0 / 365.0,), min_mass: float = 0.99, out=None,
                    stream=None, snapshots_per_wg: int = 0):
    """Model-free variance, skew, kurtosis and a constant-maturity vol index of a batch of surfaces
    (ivs_surface_moments_f64; rules M1-M7 of DESIGN.md section 11).  vol float64 [B,mT,mK] (the `out` of surface_batch);
    Kq [mK] or [B,mK]; Tq [mT] or [B,mT]; spot [B]; all CUDA tensors; mK >= 2.  rate: the scalar r of the forward.
    horizons: 0..8 index horizons in years (finite, > 0; ValueError otherwise); min_mass in [0, 1]: the lognormal
    probability the strikes must cover before a row is flagged TRUNCATED (0 = never).
    `out`: optional dict of preallocated outputs (keys raw, stats float64 [B,mT,4], mass float64 [B,mT], flags int32
    [B,mT], index float64 [B,nH], index_flags int32 [B,nH]).
    snapshots_per_wg: 0 lets the call choose how many snapshots share a workgroup; 1..4 forces it (tuning / testing; the
    results are the same bit for bit).
    Returns dict(raw, stats, mass, flags, index, index_flags) of device tensors (index / index_flags None without
    horizons); raw = L, V, W, X; stats = mf_vol, bkm_vol, skew, kurt; flags are the _lib.MM_* bits."""
    import math
    hz = [float(h) for h in horizons]
    if len(hz) > _lib.MM_MAX_HORIZONS:
        raise ValueError(f"{len(hz)} horizons: at most {_lib.MM_MAX_HORIZONS} are supported")
    if any(not (math.isfinite(h) and h > 0.0) for h in hz):
        raise ValueError(f"horizons must be finite and > 0, got {hz!r}")
    if not 0.0 <= float(min_mass) <= 1.0:
        raise ValueError(f"min_mass {min_mass!r} is outside [0, 1]")
    torch = require_device()
    vol, Kq, Tq, spot, B, mT, mK = _surface_inputs(torch, vol, Kq, Tq, spot)
    nH = len(hz)
    shapes = {"raw": ((B, mT, 4), torch.float64, True), "stats": ((B, mT, 4), torch.float64, True),
              "mass": ((B, mT), torch.float64, True), "flags": ((B, mT), torch.int32, True),
              "index": ((B, nH), torch.float64, nH > 0), "index_flags": ((B, nH), torch.int32, nH > 0)}
    out = _outputs(torch, out, shapes, vol.device)
    a = _surface_fields(_lib.MomentsArgs(), vol, Kq, Tq, spot, rate)
    a.min_mass = float(min_mass)
    a.horizons, a.nH = _doubles(hz), nH
    a.raw, a.stats, a.mass, a.flags = _ptr(out["raw"]), _ptr(out["stats"]), _ptr(out["mass"]), _ptr(out["flags"])
    a.index, a.index_flags = _ptr(out["index"]), _ptr(out["index_flags"])
    a.snapshots_per_wg = int(snapshots_per_wg)
    _call(torch, "ivs_surface_moments_f64", a, stream, vol, Kq, Tq, spot, *out.values())
    return {k: out[k] for k in shapes}


def svi_slices(vol, Kq, Tq, spot, rate: float = 0.0, *, rounds: int = 0, fitted: bool = False, out=None, stream=None,
               rows_per_wg: int = 0):
    """Raw SVI slices of a batch of surfaces with a butterfly check (ivs_svi_slices_f64; rules V1-V8 of DESIGN.md section
    12).  vol float64 [B,mT,mK] (the `out` of surface_batch); Kq [mK] or [B,mK]; Tq [mT] or [B,mT]; spot [B]; all CUDA
    tensors; 5 <= mK <= 1024.  rate: the scalar r of the forward.
    rounds: rounds of the 8 x 8 grid search over (m, ln sigma); 0 = the default 16, 1..24 otherwise (ValueError outside).
    fitted: True also returns the fitted vol at every strike (holes filled); False leaves it out (it is neither computed
    nor written).
    `out`: optional dict of preallocated outputs (keys params float64 [B,mT,5], fit float64 [B,mT,4], flags int32 [B,mT],
    fitted float64 [B,mT,mK]).
    rows_per_wg: 0 lets the call choose how many rows share a workgroup; 1..4 forces it (tuning / testing; the results are
    the same bit for bit).
    Returns dict(params, fit, flags, fitted) of device tensors (fitted None when left out); params = a, b, rho, m, sigma;
    fit = rmse_w, rmse_vol, max_vol_err, g_min; flags are the _lib.SV_* bits."""
    if not 0 <= int(rounds) <= _lib.SV_MAX_ROUNDS:
        raise ValueError(f"rounds {rounds!r} is outside [0, {_lib.SV_MAX_ROUNDS}]")
    torch = require_device()
    vol, Kq, Tq, spot, B, mT, mK = _surface_inputs(torch, vol, Kq, Tq, spot)
    shapes = {"params": ((B, mT, 5), torch.float64, True), "fit": ((B, mT, 4), torch.float64, True),
              "flags": ((B, mT), torch.int32, True), "fitted": ((B, mT, mK), torch.float64, bool(fitted))}
    out = _outputs(torch, out, shapes, vol.device)
    a = _surface_fields(_lib.SviArgs(), vol, Kq, Tq, spot, rate)
    a.rounds = int(rounds)
    a.params, a.fit, a.flags, a.fitted = _ptr(out["params"]), _ptr(out["fit"]), _ptr(out["flags"]), _ptr(out["fitted"])
    a.rows_per_wg = int(rows_per_wg)
    _call(torch, "ivs_svi_slices_f64", a, stream, vol, Kq, Tq, spot, *out.values())
    return {k: out[k] for k in shapes}


def ssvi_surface(vol, Kq, Tq, spot, rate: float = 0.0, *, raw=None, theta0=None, rounds: int = 0, fitted: bool = False,
                 out=None, stream=None):
    """Arbitrage-free SSVI surface of every snapshot, fitted jointly across its tenors (ivs_ssvi_surface_f64; rules J1-J8 of
    DESIGN.md section 15).  vol float64 [B,mT,mK] (the `out` of surface_batch); Kq [mK] or [B,mK]; Tq [mT] or [B,mT]; spot [B];
    all CUDA tensors; mT <= 64, mK >= 1, mT * mK <= 3072 (ValueError outside).  rate: the scalar r of the forward.
    raw / theta0: where the ATM total variances come from, exactly one of the two (ValueError otherwise): raw float64
    [B,mT,5] = the `params` of svi_slices, or theta0 float64 [B,mT] itself.
    rounds: rounds of the 6 x 6 x 6 grid search over (rho, gamma, ln(eta / eta_max)); 0 = the default 20, 1..32 otherwise
    (ValueError outside).  fitted: True also returns the fitted vol at every strike; False leaves it out (it is neither
    computed nor written).
    `out`: optional dict of preallocated outputs (keys surface float64 [B,4], theta float64 [B,mT], params float64 [B,mT,5],
    fit float64 [B,mT,3], flags int32 [B,mT], sflags int32 [B], fitted float64 [B,mT,mK]).
    Returns dict(surface, theta, params, fit, flags, sflags, fitted) of device tensors (fitted None when left out); surface =
    rho, eta, gamma, rmse; params = a, b, rho, m, sigma (the layout of svi_slices); fit = rmse_vol, max_vol_err, g_min; flags
    are the _lib.SS_* bits, sflags the _lib.SF_* bits."""
    if not 0 <= int(rounds) <= _lib.SS_MAX_ROUNDS:
        raise ValueError(f"rounds {rounds!r} is outside [0, {_lib.SS_MAX_ROUNDS}]")
    if (raw is None) == (theta0 is None):
        raise ValueError("exactly one of raw and theta0 must be given")
    torch = require_device()
    vol, Kq, Tq, spot, B, mT, mK = _surface_inputs(torch, vol, Kq, Tq, spot)
    if mT > _lib.ST_MAX_TENORS:
        raise ValueError(f"mT = {mT}: at most {_lib.ST_MAX_TENORS} tenors per snapshot are supported")
    if mK < 1 or mT * mK > _lib.SS_MAX_NODES:
        raise ValueError(f"mT x mK = {mT} x {mK}: between 1 and {_lib.SS_MAX_NODES} nodes per snapshot are supported")
    if raw is not None:
        raw = _f64(torch, raw, "raw")
        if tuple(raw.shape) != (B, mT, 5):
            raise ValueError("raw must be [B, mT, 5]")
    else:
        theta0 = _f64(torch, theta0, "theta0")
        if tuple(theta0.shape) != (B, mT):
            raise ValueError("theta0 must be [B, mT]")
    shapes = {"surface": ((B, 4), torch.float64, True), "theta": ((B, mT), torch.float64, True),
              "params": ((B, mT, 5), torch.float64, True), "fit": ((B, mT, 3), torch.float64, True),
              "flags": ((B, mT), torch.int32, True), "sflags": ((B,), torch.int32, True),
              "fitted": ((B, mT, mK), torch.float64, bool(fitted))}
    out = _outputs(torch, out, shapes, vol.device)
    a = _surface_fields(_lib.SsviArgs(), vol, Kq, Tq, spot, rate)
    a.raw, a.theta0, a.rounds = _ptr(raw), _ptr(theta0), int(rounds)
    a.surface, a.theta, a.params, a.fit = _ptr(out["surface"]), _ptr(out["theta"]), _ptr(out["params"]), _ptr(out["fit"])
    a.flags, a.sflags, a.fitted = _ptr(out["flags"]), _ptr(out["sflags"]), _ptr(out["fitted"])
    _call(torch, "ivs_ssvi_surface_f64", a, stream, vol, Kq, Tq, spot, raw, theta0, *out.values())
    return {k: out[k] for k in shapes}


DEFAULT_PROBS = (0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99)      # rule P9: the probability cone
DEFAULT_LEVELS = (0.8, 0.9, 1.0, 1.1, 1.2)                     # ... and the moneyness levels


def distribution_targets(probs, levels, max_tail=1e-6):
    """The host-side checks of DESIGN.md section 13: 1..16 probabilities strictly inside (0, 1), 0..16 finite positive
    moneyness levels, max_tail in [0, 1]; ValueError otherwise.  Returns (probs, levels) as lists of floats."""
    import math
    probs, levels = [float(q) for q in probs], [float(u) for u in levels]
    if not 1 <= len(probs) <= _lib.DS_MAX_PROBS:
        raise ValueError(f"{len(probs)} probabilities: between 1 and {_lib.DS_MAX_PROBS} are supported")
    if len(levels) > _lib.DS_MAX_LEVELS:
        raise ValueError(f"{len(levels)} levels: at most {_lib.DS_MAX_LEVELS} are supported")
    if any(not 0.0 < q < 1.0 for q in probs):
        raise ValueError(f"probabilities must be strictly inside (0, 1), got {probs!r}")
    if any(not (math.isfinite(u) and u > 0.0) for u in levels):
        raise ValueError(f"levels must be finite and > 0, got {levels!r}")
    if not 0.0 <= float(max_tail) <= 1.0:
        raise ValueError(f"max_tail {max_tail!r} is outside [0, 1]")
    return probs, levels


def svi_distribution(params, Tq, spot, rate: float = 0.0, *, probs=DEFAULT_PROBS, levels=DEFAULT_LEVELS,
                     max_tail: float = 1e-6, out=None, stream=None, rows_per_wave: int = 0):
    """Risk-neutral quantiles and probabilities off a batch of raw SVI slices (ivs_svi_distribution_f64; rules P1-P8 of
    DESIGN.md section 13).  params float64 [B,mT,5] (the `params` of svi_slices); Tq [mT] or [B,mT]; spot [B]; all CUDA
    tensors.  rate: the scalar r of the forward.
    probs: 1..16 probabilities strictly inside (0, 1); levels: 0..16 moneyness levels, finite and > 0; max_tail in [0, 1]:
    the share of probability the scan grid may leave out on either side before the row is flagged TAILS (ValueError outside).
    `out`: optional dict of preallocated outputs (keys q_x, q_strike float64 [B,mT,nP], q_flags int32 [B,mT,nP], p_below,
    p_above float64 [B,mT,nL], tails float64 [B,mT,2], flags int32 [B,mT]).
    rows_per_wave: 0 lets the call choose how many rows share a wavefront; 1..64 // nP forces it (tuning / testing; the
    results are the same bit for bit).
    Returns dict(q_x, q_strike, q_flags, p_below, p_above, tails, flags) of device tensors (p_below / p_above None without
    levels); the flags are the _lib.DS_* bits."""
    probs, levels = distribution_targets(probs, levels, max_tail)
    torch = require_device()
    params, Tq, spot, B, mT = _svi_inputs(torch, params, Tq, spot, max_tenors=None)     # the rows are independent: any mT
    nP, nL = len(probs), len(levels)
    shapes = {"q_x": ((B, mT, nP), torch.float64, True), "q_strike": ((B, mT, nP), torch.float64, True),
              "q_flags": ((B, mT, nP), torch.int32, True), "p_below": ((B, mT, nL), torch.float64, nL > 0),
              "p_above": ((B, mT, nL), torch.float64, nL > 0), "tails": ((B, mT, 2), torch.float64, True),
              "flags": ((B, mT), torch.int32, True)}
    out = _outputs(torch, out, shapes, params.device)
    a = _slice_fields(_lib.DistributionArgs(), params, Tq, spot, rate)
    a.max_tail = float(max_tail)
    a.probs, a.nP = _doubles(probs), nP
    a.levels, a.nL = _doubles(levels), nL
    a.q_x, a.q_strike, a.q_flags = _ptr(out["q_x"]), _ptr(out["q_strike"]), _ptr(out["q_flags"])
    a.p_below, a.p_above, a.tails, a.flags = _ptr(out["p_below"]), _ptr(out["p_above"]), _ptr(out["tails"]), _ptr(out["flags"])
    a.rows_per_wave = int(rows_per_wave)
    _call(torch, "ivs_svi_distribution_f64", a, stream, params, Tq, spot, *out.values())
    return {k: out[k] for k in shapes}


def svi_calendar(params, Tq, spot, *, out=None, stream=None, rows_per_wave: int = 0):
    """Calendar report between the raw SVI slices of every snapshot (ivs_svi_calendar_f64; rules T1-T4, C1-C6 of DESIGN.md
    section 14).  params float64 [B,mT,5] (the `params` of svi_slices); Tq [mT] or [B,mT]; spot [B]; all CUDA tensors;
    mT <= 64 (ValueError above).  Entry j describes the pair of row j and the next live row above it.
    `out`: optional dict of preallocated outputs (keys d_min, x_min, d_atm float64 [B,mT], x_cross float64 [B,mT,2], n_cross,
    flags int32 [B,mT]).
    rows_per_wave: 0 lets the call choose how many rows share a wavefront; 1..32 forces it (tuning / testing; the results
    are the same bit for bit).
    Returns dict(d_min, x_min, d_atm, x_cross, n_cross, flags) of device tensors; the flags are the _lib.SC_* bits."""
    torch = require_device()
    params, Tq, spot, B, mT = _svi_inputs(torch, params, Tq, spot)
    shapes = {"d_min": ((B, mT), torch.float64, True), "x_min": ((B, mT), torch.float64, True),
              "d_atm": ((B, mT), torch.float64, True), "x_cross": ((B, mT, 2), torch.float64, True),
              "n_cross": ((B, mT), torch.int32, True), "flags": ((B, mT), torch.int32, True)}
    out = _outputs(torch, out, shapes, params.device)
    a = _slice_fields(_lib.CalendarArgs(), params, Tq, spot)
    a.d_min, a.x_min, a.d_atm, a.x_cross = _ptr(out["d_min"]), _ptr(out["x_min"]), _ptr(out["d_atm"]), _ptr(out["x_cross"])
    a.n_cross, a.flags = _ptr(out["n_cross"]), _ptr(out["flags"])
    a.rows_per_wave = int(rows_per_wave)
    _call(torch, "ivs_svi_calendar_f64", a, stream, params, Tq, spot, *out.values())
    return {k: out[k] for k in shapes}


EVAL_OUTPUTS = ("w", "vol", "call", "put", "fwd_var", "g", "local_vol")


def svi_eval(params, Tq, spot, rate, u, tau, *, strike_mode: int = 0, want=EVAL_OUTPUTS, out=None, stream=None):
    """The surface of the raw SVI slices at any (strike, expiry) (ivs_svi_eval_f64; rules T1-T3, E1-E6 of DESIGN.md section
    14).  params float64 [B,mT,5]; Tq [mT] or [B,mT]; spot [B]; u, tau [Q] (one list for all snapshots) or [B,Q], both of one
    shape; all CUDA tensors; mT <= 64.  rate: the scalar r of the forward and the discount factor.
    strike_mode: 0 = u is a moneyness level (K = spot u), 1 = u is the strike (ValueError otherwise).
    want: which of EVAL_OUTPUTS to compute; one left out is neither computed nor written (None in the result).
    `out`: optional dict of preallocated outputs (float64 [B,Q] per value, flags int32 [B,Q]).
    Returns dict(w, vol, call, put, fwd_var, g, local_vol, flags) of device tensors; the flags are the _lib.SE_* bits."""
    _check_strike_mode(strike_mode)
    want = _wanted(want, EVAL_OUTPUTS)
    return _option_call("ivs_svi_eval_f64", _lib.EvalArgs(), params, Tq, spot, rate, u, tau, strike_mode, out, stream,
                        lambda torch, B, Q: _per_option(torch, (B, Q), EVAL_OUTPUTS, want))[1]


GREEK_OUTPUTS = ("price", "delta_ss", "delta_sm", "gamma_ss", "gamma_sm", "vega", "theta")
BOOK_OUTPUTS = ("pnl_ss", "pnl_sm")
NET_COLUMNS = GREEK_OUTPUTS + ("gross",)                       # the eight slots of a book's `net`
DEFAULT_SPOT_SHOCKS = (-0.20, -0.15, -0.10, -0.05, 0.0, 0.05, 0.10, 0.15, 0.20)
DEFAULT_VOL_SHOCKS = (-0.10, -0.05, 0.0, 0.05, 0.10)


def _option_queries(torch, B, u, tau, is_put, qty=None):
    """The shared checks of the options of svi_greeks / svi_book: u, tau [Q] or [B,Q] of one shape, is_put uint8 / bool [Q] or
    None, qty float64 [Q]."""
    u = _f64(torch, u, "u"); tau = _f64(torch, tau, "tau")
    if u.dim() not in (1, 2) or u.shape != tau.shape or (u.dim() == 2 and u.shape[0] != B):
        raise ValueError("u and tau must both be [Q] or both [B, Q]")
    Q = u.shape[-1]
    if is_put is not None:
        if not is_put.is_cuda or is_put.dtype not in (torch.uint8, torch.bool):
            raise TypeError("is_put must be a CUDA uint8 or bool tensor")
        if tuple(is_put.shape) != (Q,):
            raise ValueError("is_put must be [Q]: one side per option, shared by all snapshots")
        is_put = is_put.to(torch.uint8).contiguous()
    if qty is not None:
        qty = _f64(torch, qty, "qty")
        if tuple(qty.shape) != (Q,):
            raise ValueError("qty must be [Q]: one quantity per option, shared by all snapshots")
    return u, tau, is_put, qty, Q


def _check_strike_mode(strike_mode):
    if strike_mode not in (0, 1):
        raise ValueError(f"strike_mode {strike_mode!r} is neither 0 (moneyness) nor 1 (strike)")


def _per_option(torch, shape, names, want):
    """The shapes (as _outputs takes them) of one float64 value per option and name, those in `want` alone, and the flags."""
    return {**{k: (shape, torch.float64, k in want) for k in names}, "flags": (shape, torch.int32, True)}


def _option_call(name, a, params, Tq, spot, rate, u, tau, strike_mode, out, stream, shapes, is_put=None, qty=None, **fields):
    """The chain svi_eval, svi_greeks, svi_book, svi_explain and svi_hsim share: the input checks, the outputs (shapes(torch, B,
    Q) describes them as _outputs takes them), the args struct `a` filled with the slices, the options, the call's own
    `fields` and the outputs' pointers, and the C call `name`.  Returns torch, the result dict and B, mT, Q."""
    torch = require_device()
    params, Tq, spot, B, mT = _svi_inputs(torch, params, Tq, spot)
    u, tau, is_put, qty, Q = _option_queries(torch, B, u, tau, is_put, qty)
    shapes = shapes(torch, B, Q)
    out = _outputs(torch, out, shapes, params.device)
    _slice_fields(a, params, Tq, spot, rate)
    _query_fields(a, u, tau, strike_mode)
    for k, v in fields.items():
        setattr(a, k, v)
    for k, t in (("is_put", is_put), ("qty", qty), *((k, out[k]) for k in shapes)):
        if t is not None:
            setattr(a, k, _ptr(t))
    _call(torch, name, a, stream, params, Tq, spot, u, tau, is_put, qty, *out.values())
    return torch, {k: out[k] for k in shapes}, B, mT, Q


def _fill(torch, stream, out, values):
    """The C call was a no-op (no slice or no option): the wrapper defines the result and writes it on the caller's stream.
    values: {key: number or tensor}, or a function that forms that dict on the stream; an output not wanted is passed over."""
    with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
        for k, v in (values() if callable(values) else values).items():
            if out[k] is not None:
                out[k].copy_(v) if torch.is_tensor(v) else out[k].fill_(v)


def svi_greeks(params, Tq, spot, rate, u, tau, *, is_put=None, strike_mode: int = 0, want=GREEK_OUTPUTS, out=None, stream=None):
    """Smile-aware Greeks of options on the surface of the raw SVI slices (ivs_svi_greeks_f64; rules G0-G6 of DESIGN.md section
    17).  params, Tq, spot, rate, u, tau, strike_mode as in svi_eval; is_put uint8 / bool [Q] (one side per option, shared by
    all snapshots) or None = all calls.
    want: which of GREEK_OUTPUTS to compute; one left out is neither computed nor written (None in the result).
    `out`: optional dict of preallocated outputs (float64 [B,Q] per value, flags int32 [B,Q]).
    With mT == 0 the C call writes nothing and the wrapper fills NaN and DEAD itself.
    Returns dict(price, delta_ss, delta_sm, gamma_ss, gamma_sm, vega, theta, flags) of device tensors; the flags are the
    _lib.SE_* bits SHORT, LONG, NEG_FWD, DEAD, UNORDERED."""
    _check_strike_mode(strike_mode)
    want = _wanted(want, GREEK_OUTPUTS)
    torch, out, _, mT, _ = _option_call(
        "ivs_svi_greeks_f64", _lib.GreeksArgs(), params, Tq, spot, rate, u, tau, strike_mode, out, stream,
        lambda torch, B, Q: _per_option(torch, (B, Q), GREEK_OUTPUTS, want), is_put)
    if mT == 0:                                              # without a slice every option is dead (E1)
        _fill(torch, stream, out, {**dict.fromkeys(GREEK_OUTPUTS, float("nan")), "flags": _lib.SE_DEAD})
    return out


def book_shocks(spot_shocks, vol_shocks):
    """The host-side checks of a scenario grid: at most 64 shocks per axis and 1024 cells, every spot
    shock finite and > -1, every vol shock finite; ValueError otherwise.  Returns (spot_shocks, vol_shocks) as lists."""
    import math
    a, v = [float(x) for x in spot_shocks], [float(x) for x in vol_shocks]
    if len(a) > _lib.RK_MAX_SHOCKS or len(v) > _lib.RK_MAX_SHOCKS or len(a) * len(v) > _lib.RK_MAX_GRID:
        raise ValueError(f"a {len(a)} x {len(v)} grid: at most {_lib.RK_MAX_SHOCKS} shocks per axis and {_lib.RK_MAX_GRID} cells are supported")
    if any(not (math.isfinite(x) and x > -1.0) for x in a):
        raise ValueError(f"spot shocks must be finite and > -1, got {a!r}")
    if any(not math.isfinite(x) for x in v):
        raise ValueError(f"vol shocks must be finite, got {v!r}")
    return a, v


def svi_book(params, Tq, spot, rate, u, tau, qty, spot_shocks=DEFAULT_SPOT_SHOCKS, vol_shocks=DEFAULT_VOL_SHOCKS, *, is_put=None,
             strike_mode: int = 0, want=BOOK_OUTPUTS, out=None, stream=None, cells_per_wg: int = 0):
    """Net Greeks and the scenario P&L grid of a book of options per snapshot (ivs_svi_book_f64; rules B1-B5 of DESIGN.md
    section 17).  Inputs as in svi_greeks, besides qty float64 [Q] (one quantity per option, shared by all snapshots; an option
    whose quantity is not finite is dead) and the two lists of shocks (book_shocks has their limits).
    want: which of pnl_ss (sticky strike) and pnl_sm (sticky moneyness) to compute.
    `out`: optional dict of preallocated outputs (net float64 [B,8], n_dead int32 [B], pnl_ss / pnl_sm float64 [B,nA,nV],
    cell_flags int32 [B,nA,nV]).
    cells_per_wg: 0 lets the call choose how many cells a workgroup takes; 1..256 forces it (tuning / testing; the results are
    the same bit for bit).
    The C call writes nothing when mT == 0 or Q == 0; the wrapper then fills the result itself: without a slice every snapshot is
    degenerate (NaN, n_dead = Q, cell flags 0), and a book without options has 0 in every sum, count and flag.
    Returns dict(net, n_dead, pnl_ss, pnl_sm, cell_flags) of device tensors; net's columns are NET_COLUMNS, the cell flags the
    _lib.SB_* bits."""
    _check_strike_mode(strike_mode)
    want = _wanted(want, BOOK_OUTPUTS)
    sa, sv = book_shocks(spot_shocks, vol_shocks)
    nA, nV = len(sa), len(sv)

    def shapes(torch, B, Q):
        return {"net": ((B, 8), torch.float64, True), "n_dead": ((B,), torch.int32, True),
                "pnl_ss": ((B, nA, nV), torch.float64, "pnl_ss" in want), "pnl_sm": ((B, nA, nV), torch.float64, "pnl_sm" in want),
                "cell_flags": ((B, nA, nV), torch.int32, True)}
    torch, out, B, mT, Q = _option_call(
        "ivs_svi_book_f64", _lib.BookArgs(), params, Tq, spot, rate, u, tau, strike_mode, out, stream, shapes, is_put, qty,
        spot_shocks=_doubles(sa), nA=nA, vol_shocks=_doubles(sv), nV=nV, cells_per_wg=int(cells_per_wg))
    if B > 0 and (mT == 0 or Q == 0):
        empty = float("nan") if mT == 0 else 0.0             # B1: no live slice -> NaN and n_dead = Q; a book without options is worth 0
        _fill(torch, stream, out, {"net": empty, "n_dead": Q if mT == 0 else 0, "cell_flags": 0, "pnl_ss": empty, "pnl_sm": empty})
    return out


EXPLAIN_OUTPUTS = ("actual", "theta_pnl", "delta_ss", "gamma_ss", "vega_ss", "resid_ss", "delta_sm", "gamma_sm", "vega_sm", "resid_sm")
EXPLAIN_NET_COLUMNS = EXPLAIN_OUTPUTS + ("value", "gross")    # the twelve slots of an explain's `net`


def svi_explain(params, Tq, spot, rate, u, tau, qty, *, lag: int = 1, is_put=None, strike_mode: int = 0, want=EXPLAIN_OUTPUTS,
                out=None, stream=None):
    """P&L explain of a book of options between snapshot p and snapshot p + lag (ivs_svi_explain_f64; rules X0-X9 of
    DESIGN.md section 18): the realised change of every option's price split into theta, delta, gamma, vega and a remainder
    under sticky strike and under sticky moneyness, and the same summed over the book.  Inputs as in svi_book without the
    shocks; lag >= 1 (ValueError otherwise).  There are P = max(B - lag, 0) pairs; the contract (strike, side, quantity) is
    the one of the pair's first snapshot.
    want: which of EXPLAIN_OUTPUTS to write; one left out is None in the result.
    `out`: optional dict of preallocated outputs (float64 [P,Q] per value, flags int32 [P,Q], net float64 [P,12], n_dead int32
    [P]).
    The C call writes nothing when mT == 0 or Q == 0; the wrapper then fills the result itself as svi_book does: without a
    slice every pair is degenerate (NaN, n_dead = Q, every placement DEAD), and a book without options has 0 in every sum and
    count.
    Returns dict(the ten values, flags, net, n_dead) of device tensors; net's columns are EXPLAIN_NET_COLUMNS, the flags the
    _lib.SE_* bits of the three placements in bits 0-7, 8-15 and 16-23."""
    _check_strike_mode(strike_mode)
    if int(lag) != lag or lag < 1:
        raise ValueError(f"lag {lag!r} is not an integer >= 1")
    want = _wanted(want, EXPLAIN_OUTPUTS)

    def shapes(torch, B, Q):
        P = max(B - int(lag), 0)
        return {**_per_option(torch, (P, Q), EXPLAIN_OUTPUTS, want),
                "net": ((P, 12), torch.float64, True), "n_dead": ((P,), torch.int32, True)}
    torch, out, B, mT, Q = _option_call(
        "ivs_svi_explain_f64", _lib.ExplainArgs(), params, Tq, spot, rate, u, tau, strike_mode, out, stream, shapes, is_put, qty,
        lag=int(lag))
    if B > lag and (mT == 0 or Q == 0):
        empty = float("nan") if mT == 0 else 0.0             # X2: no live slice -> NaN and n_dead = Q; a book without options is worth 0
        _fill(torch, stream, out, {**dict.fromkeys(EXPLAIN_OUTPUTS, float("nan")), "net": empty, "n_dead": Q if mT == 0 else 0,
                                   "flags": _lib.SE_DEAD | _lib.SE_DEAD << 8 | _lib.SE_DEAD << 16})
    return out


DEFAULT_TAIL_PROBS = (0.05, 0.01)
HSIM_OUTPUTS = ("pnl", "scen_flags", "var", "es", "n_valid", "n_dead", "worst", "value")


def hsim_settings(lag, window, tail_probs, min_scen, scen_per_wg=0):
    """The host-side checks of a historical simulation: lag an integer >= 1, window 1..1024, at most 8
    tail probabilities, each finite and inside (0, 1), min_scen >= 1, scen_per_wg 0..window; ValueError otherwise.  Returns
    (lag, window, tail_probs as a list, min_scen, scen_per_wg)."""
    import math
    for name, v, lo in (("lag", lag, 1), ("window", window, 1), ("min_scen", min_scen, 1), ("scen_per_wg", scen_per_wg, 0)):
        if int(v) != v or v < lo:
            raise ValueError(f"{name} {v!r} is not an integer >= {lo}")
    if window > _lib.HS_MAX_WINDOW:
        raise ValueError(f"window {window}: at most {_lib.HS_MAX_WINDOW} scenarios per snapshot are supported")
    if scen_per_wg > window:
        raise ValueError(f"scen_per_wg {scen_per_wg} exceeds the window {window}")
    tp = [float(x) for x in tail_probs]
    if len(tp) > _lib.HS_MAX_LEVELS:
        raise ValueError(f"{len(tp)} tail probabilities: at most {_lib.HS_MAX_LEVELS} are supported")
    if any(not (math.isfinite(x) and 0.0 < x < 1.0) for x in tp):
        raise ValueError(f"tail probabilities must be finite and inside (0, 1), got {tp!r}")
    return int(lag), int(window), tp, int(min_scen), int(scen_per_wg)


def svi_hsim(params, Tq, spot, rate, u, tau, qty, *, lag: int = 1, window: int = 256, tail_probs=DEFAULT_TAIL_PROBS, min_scen: int = 20,
             is_put=None, strike_mode: int = 0, value: bool = True, out=None, stream=None, scen_per_wg: int = 0, stages: int = 0):
    """Historical-simulation VaR and expected shortfall of a book of options per snapshot (ivs_svi_hsim_f64; rules H0-H9 of
    DESIGN.md section 19): for snapshot p, scenario s is the past pair of snapshots (p - lag - s, p - s); it moves today's spot by
    the pair's quotient and every option's vol by the pair's change at fixed moneyness and tenor, and the book is revalued on
    the surface.  Inputs as in svi_explain; hsim_settings has the limits of lag, window, tail_probs, min_scen and scen_per_wg.
    value: whether to form the book's value and gross value [B,2] (None in the result otherwise).
    `out`: optional dict of preallocated outputs (pnl float64 [B,window], scen_flags int32 [B,window], var / es float64 [B,nL],
    n_valid / n_dead / worst int32 [B], value float64 [B,2]).
    scen_per_wg: 0 lets the call choose how many scenarios a workgroup takes; 1..window forces it (the same bits).  stages: 0 =
    everything, 1 = pnl, scen_flags, value and n_dead alone, 2 = the order statistics alone from out's pnl and scen_flags.
    The C call writes nothing when mT == 0 or Q == 0; the wrapper then fills the result itself as svi_book does: without a
    slice every snapshot is degenerate (every existing scenario VOID_PAIR and NaN, n_valid 0, n_dead = Q, NaN in var / es /
    value), and a book without options has +0.0 in every existing scenario, VaR, ES and value.
    Returns dict(pnl, scen_flags, var, es, n_valid, n_dead, worst, value) of device tensors; the flags are the _lib.HS_* bits."""
    _check_strike_mode(strike_mode)
    if stages not in (0, 1, 2):
        raise ValueError(f"stages {stages!r} is not 0, 1 or 2")
    lag, window, tp, min_scen, scen_per_wg = hsim_settings(lag, window, tail_probs, min_scen, scen_per_wg)
    nL = len(tp)

    def shapes(torch, B, Q):
        i32, f64 = torch.int32, torch.float64
        return {"pnl": ((B, window), f64, True), "scen_flags": ((B, window), i32, True), "var": ((B, nL), f64, True),
                "es": ((B, nL), f64, True), "n_valid": ((B,), i32, True), "n_dead": ((B,), i32, True), "worst": ((B,), i32, True),
                "value": ((B, 2), f64, bool(value))}
    torch, out, B, mT, Q = _option_call(
        "ivs_svi_hsim_f64", _lib.HsimArgs(), params, Tq, spot, rate, u, tau, strike_mode, out, stream, shapes, is_put, qty,
        lag=lag, window=window, tail_probs=_doubles(tp), nL=nL, min_scen=min_scen, scen_per_wg=scen_per_wg, stages=int(stages))

    def empty():                                             # H9
        nan, device = float("nan"), out["pnl"].device
        n_p = (torch.arange(B, device=device) - lag + 1).clamp(0, window)
        exists = torch.arange(window, device=device)[None, :] < n_p[:, None]
        here = torch.full((), _lib.HS_VOID_PAIR if mT == 0 else 0, dtype=torch.int32, device=device)
        tail = torch.where(((n_p >= min_scen) & (mT > 0))[:, None], 0.0, nan).expand(B, nL)
        return {"scen_flags": torch.where(exists, here, torch.full_like(here, _lib.HS_ABSENT)),
                "pnl": torch.where(exists & (mT > 0), 0.0, nan), "var": tail, "es": tail,
                "n_valid": n_p if mT > 0 else torch.zeros_like(n_p), "worst": torch.where((n_p > 0) & (mT > 0), 0, -1),
                "n_dead": Q if mT == 0 else 0, "value": nan if mT == 0 else 0.0}
    if B > 0 and (mT == 0 or Q == 0):
        _fill(torch, stream, out, empty)
    return out


ATTRIB_OUTPUTS = ("ces", "cvar", "ces_group", "cvar_group", "n_tail", "order")
ATTRIB_OPTIONAL = ("ces", "cvar", "ces_group", "cvar_group", "order")


def attrib_settings(lag, window, tail_probs, min_scen, n_groups=1):
    """The host-side checks of a VaR attribution: those of hsim_settings, 1..16 groups, and rule A7: no
    level's largest tail max(1, floor(window x tp)) may exceed 64 scenarios; ValueError otherwise.  Returns (lag, window,
    tail_probs as a list, min_scen, n_groups)."""
    import math
    lag, window, tp, min_scen, _ = hsim_settings(lag, window, tail_probs, min_scen)
    if int(n_groups) != n_groups or not 1 <= n_groups <= _lib.HA_MAX_GROUPS:
        raise ValueError(f"n_groups {n_groups!r} is not an integer in 1..{_lib.HA_MAX_GROUPS}")
    for x in tp:
        if max(1, math.floor(float(window) * x)) > _lib.HA_MAX_TAIL:
            raise ValueError(f"tail probability {x!r} of a window of {window} is a tail of {math.floor(float(window) * x)} scenarios: "
                             f"at most {_lib.HA_MAX_TAIL} are supported")
    return lag, window, tp, min_scen, int(n_groups)


def svi_hsim_attrib(params, Tq, spot, rate, u, tau, qty, pnl, scen_flags, *, group=None, n_groups: int = 1, lag: int = 1,
                    window: int = 256, tail_probs=DEFAULT_TAIL_PROBS, min_scen: int = 20, is_put=None, strike_mode: int = 0,
                    want=ATTRIB_OPTIONAL, out=None, stream=None):
    """The VaR and expected shortfall of svi_hsim attributed to the options of the book and to groups of them
    (ivs_svi_hsim_attrib_f64; rules A0-A8 of DESIGN.md section 20): component ES of an option is the mean of its own P&L over
    the scenarios of the book's tail, component VaR its P&L in the VaR scenario; summed over the book they give es and var back.
    Inputs as in svi_hsim, plus pnl float64 and scen_flags int32 [B,window] as svi_hsim returned them for the same inputs and
    settings, group int32 [Q] (one list for all snapshots; None = every option in group 0; an id outside 0..n_groups-1 is in no
    group) and n_groups in 1..16.  attrib_settings has the limits.
    want: which of ces, cvar [B,nL,Q], ces_group, cvar_group [B,nL,n_groups] and order [B,window] to compute; one left out is
    neither computed nor written (None in the result).  n_tail int32 [B,nL] (the size of every tail, 0 for an inactive level)
    is always given.  `out`: optional dict of preallocated outputs.
    The C call writes nothing when mT == 0 or Q == 0; the wrapper then fills the result itself: without a slice every snapshot
    is degenerate (NaN everywhere, n_tail 0), and a book without options has +0.0 in the groups of every active level; order and
    n_tail are then formed from pnl and scen_flags by rule A1.
    Returns dict(ces, cvar, ces_group, cvar_group, n_tail, order) of device tensors."""
    _check_strike_mode(strike_mode)
    want = _wanted(want, ATTRIB_OPTIONAL)
    lag, window, tp, min_scen, nG = attrib_settings(lag, window, tail_probs, min_scen, n_groups)
    nL = len(tp)
    torch = require_device()
    B, Q0 = _svi_inputs(torch, params, Tq, spot)[3], u.shape[-1]
    pnl = _f64(torch, pnl, "pnl")
    if not scen_flags.is_cuda or scen_flags.dtype != torch.int32:
        raise TypeError("scen_flags must be a CUDA int32 tensor")
    scen_flags = scen_flags.contiguous()
    if tuple(pnl.shape) != (B, window) or tuple(scen_flags.shape) != (B, window):
        raise ValueError(f"pnl and scen_flags must be [B, window] = {(B, window)}")
    if group is not None:
        if not group.is_cuda or group.dtype != torch.int32:
            raise TypeError("group must be a CUDA int32 tensor")
        if tuple(group.shape) != (Q0,):
            raise ValueError("group must be [Q]: one group id per option, shared by all snapshots")
        group = group.contiguous()

    def shapes(torch, B, Q):
        i32, f64 = torch.int32, torch.float64
        return {"ces": ((B, nL, Q), f64, "ces" in want), "cvar": ((B, nL, Q), f64, "cvar" in want),
                "ces_group": ((B, nL, nG), f64, "ces_group" in want), "cvar_group": ((B, nL, nG), f64, "cvar_group" in want),
                "n_tail": ((B, nL), i32, True), "order": ((B, window), i32, "order" in want)}
    torch, out, B, mT, Q = _option_call(
        "ivs_svi_hsim_attrib_f64", _lib.HsimAttribArgs(), params, Tq, spot, rate, u, tau, strike_mode, out, stream, shapes, is_put, qty,
        lag=lag, window=window, tail_probs=_doubles(tp), nL=nL, min_scen=min_scen, pnl=_ptr(pnl), scen_flags=_ptr(scen_flags),
        group=_ptr(group), nG=nG)
    _hold_for_stream(torch, stream, pnl, scen_flags, group)

    def empty():                                             # A8
        nan, device = float("nan"), pnl.device
        n_p = (torch.arange(B, device=device) - lag + 1).clamp(0, window)
        ranked = (scen_flags == 0) & ~torch.isnan(pnl) & (torch.arange(window, device=device)[None, :] < n_p[:, None]) & (mT > 0)
        n = ranked.sum(dim=1)
        idx = torch.sort(torch.where(ranked, pnl, float("inf")), dim=1, stable=True).indices
        order = torch.where(torch.arange(window, device=device)[None, :] < n[:, None], idx, -1).to(torch.int32)
        m = torch.floor(n.to(torch.float64)[:, None] * torch.tensor(tp, dtype=torch.float64, device=device)[None, :]).clamp(min=1)
        on = ((n >= min_scen) & (n > 0))[:, None].expand(B, nL)
        sums = torch.where(on, 0.0, nan)[:, :, None].expand(B, nL, nG)
        return {"ces": nan, "cvar": nan, "ces_group": sums, "cvar_group": sums, "n_tail": torch.where(on, m, 0.0).to(torch.int32),
                "order": order}
    if B > 0 and (mT == 0 or Q == 0):
        _fill(torch, stream, out, empty)
    return out


HEDGE_OUTPUTS = ("inst_pnl", "inst_flags", "pick", "ss", "n_rounds", "hedge", "pnl_hedged", "var_h", "es_h", "worst_h", "n_scen",
                 "solo_qty", "solo_left", "inst_value")
HEDGE_OPTIONAL = ("solo_qty", "solo_left", "inst_value")


def hedge_settings(lag, window, tail_probs, min_scen, n_inst, rounds=4, n_forced=0, tol=1e-6, min_gain=1e-4, stages=0):
    """The host-side checks of a minimum-variance hedge: those of hsim_settings, 1..64 candidates, 1..8
    rounds, n_forced in 0..min(rounds, candidates), tol finite in [0, 1), min_gain finite and >= 0, stages 0, 1 or 2; ValueError
    otherwise.  Returns (lag, window, tail_probs as a list, min_scen, rounds, n_forced, tol, min_gain, stages)."""
    import math
    lag, window, tp, min_scen, _ = hsim_settings(lag, window, tail_probs, min_scen)
    if int(n_inst) != n_inst or not 1 <= n_inst <= _lib.HG_MAX_INST:
        raise ValueError(f"{n_inst!r} candidate instruments: 1..{_lib.HG_MAX_INST} are supported")
    if int(rounds) != rounds or not 1 <= rounds <= _lib.HG_MAX_ROUNDS:
        raise ValueError(f"rounds {rounds!r} is not an integer in 1..{_lib.HG_MAX_ROUNDS}")
    if int(n_forced) != n_forced or not 0 <= n_forced <= min(rounds, n_inst):
        raise ValueError(f"n_forced {n_forced!r} is not an integer in 0..min(rounds, candidates) = {min(rounds, n_inst)}")
    tol, min_gain = float(tol), float(min_gain)
    if not (math.isfinite(tol) and 0.0 <= tol < 1.0):
        raise ValueError(f"tol {tol!r} is not finite and inside [0, 1)")
    if not (math.isfinite(min_gain) and min_gain >= 0.0):
        raise ValueError(f"min_gain {min_gain!r} is not finite and >= 0")
    if stages not in (0, 1, 2):
        raise ValueError(f"stages {stages!r} is not 0, 1 or 2")
    return lag, window, tp, min_scen, int(rounds), int(n_forced), tol, min_gain, int(stages)


def svi_hedge(params, Tq, spot, rate, inst_u, inst_tau, inst_kind, pnl, scen_flags, *, lag: int = 1, window: int = 256,
              tail_probs=DEFAULT_TAIL_PROBS, min_scen: int = 20, rounds: int = 4, n_forced: int = 0, tol: float = 1e-6,
              min_gain: float = 1e-4, strike_mode: int = 0, want=HEDGE_OPTIONAL, out=None, stream=None, scen_per_wg: int = 0,
              stages: int = 0):
    """Minimum-variance hedge of a book over its historical scenarios (ivs_svi_hedge_f64; rules M0-M11 of DESIGN.md section 21):
    which of the candidate instruments, in which sizes, remove the most of the variance of the book's scenario P&L row in at most
    `rounds` steps of an orthogonal matching pursuit, and the VaR and ES of the hedged book.
    params, Tq, spot, rate, strike_mode, lag, window, tail_probs, min_scen as in svi_hsim; pnl float64 and scen_flags int32
    [B,window] as svi_hsim returned them for the book on the same inputs and settings.  inst_u, inst_tau float64 [nH] or [B,nH]: the
    candidates, read as svi_hsim reads u and tau; inst_kind uint8 [nH]: _lib.HG_CALL, HG_PUT or HG_UNDERLYING (u and tau not read).
    n_forced: the first n_forced rounds take candidates 0, 1, ... in turn ("hedge with exactly these"); the others pick greedily.
    hedge_settings has the limits.
    want: which of solo_qty, solo_left and inst_value [B,nH] to compute; one left out is neither computed nor written (None).
    `out`: optional dict of preallocated outputs; with stages = 2 its inst_pnl [B,window,nH] is the input of the selection.
    stages: 0 = everything, 1 = inst_pnl and inst_value alone, 2 = everything but those, from out's inst_pnl.
    Snapshots without a slice (mT == 0) are refused with ValueError: the C call would be a no-op and nothing can be hedged.
    Returns dict(inst_pnl [B,window,nH], inst_flags int32 [B,nH], pick int32 [B,rounds], ss [B,rounds+1], n_rounds int32 [B], hedge
    [B,nH], pnl_hedged [B,window], var_h, es_h [B,nL], worst_h, n_scen int32 [B], solo_qty, solo_left, inst_value [B,nH]) of device
    tensors; the flags are the _lib.HG_* bits."""
    _check_strike_mode(strike_mode)
    want = _wanted(want, HEDGE_OPTIONAL)
    torch = require_device()
    params, Tq, spot, B, mT = _svi_inputs(torch, params, Tq, spot)
    if mT == 0:
        raise ValueError("mT = 0: there is no slice to revalue a candidate on")
    inst_u, inst_tau, inst_kind, _, nH = _option_queries(torch, B, inst_u, inst_tau, inst_kind)
    if inst_kind is None:
        raise TypeError("inst_kind must be a CUDA uint8 tensor [nH]")
    lag, window, tp, min_scen, K, n_forced, tol, min_gain, stages = hedge_settings(lag, window, tail_probs, min_scen, nH, rounds, n_forced,
                                                                                   tol, min_gain, stages)
    hsim_settings(lag, window, tp, min_scen, scen_per_wg)
    nL = len(tp)
    pnl = _f64(torch, pnl, "pnl")
    if not scen_flags.is_cuda or scen_flags.dtype != torch.int32:
        raise TypeError("scen_flags must be a CUDA int32 tensor")
    scen_flags = scen_flags.contiguous()
    if tuple(pnl.shape) != (B, window) or tuple(scen_flags.shape) != (B, window):
        raise ValueError(f"pnl and scen_flags must be [B, window] = {(B, window)}")
    if stages == 2 and (out is None or out.get("inst_pnl") is None):
        raise ValueError("stages = 2 selects on out['inst_pnl'] as given")
    if B * window * nH >= 2 ** 31:
        raise ValueError(f"{B} x {window} x {nH} candidate scenarios exceed one launch")
    i32, f64 = torch.int32, torch.float64
    one, two = stages != 2, stages != 1
    shapes = {"inst_pnl": ((B, window, nH), f64, True), "inst_flags": ((B, nH), i32, two), "pick": ((B, K), i32, two),
              "ss": ((B, K + 1), f64, two), "n_rounds": ((B,), i32, two), "hedge": ((B, nH), f64, two),
              "pnl_hedged": ((B, window), f64, two), "var_h": ((B, nL), f64, two), "es_h": ((B, nL), f64, two),
              "worst_h": ((B,), i32, two), "n_scen": ((B,), i32, two), "solo_qty": ((B, nH), f64, two and "solo_qty" in want),
              "solo_left": ((B, nH), f64, two and "solo_left" in want), "inst_value": ((B, nH), f64, one and "inst_value" in want)}
    out = _outputs(torch, out, shapes, params.device)
    a = _slice_fields(_lib.HedgeArgs(), params, Tq, spot, rate)
    a.inst_u, a.inst_tau, a.inst_stride, a.inst_kind = _ptr(inst_u), _ptr(inst_tau), (0 if inst_u.dim() == 1 else nH), _ptr(inst_kind)
    a.strike_mode, a.nH, a.lag, a.window, a.tail_probs, a.nL, a.min_scen = int(strike_mode), nH, lag, window, _doubles(tp), nL, min_scen
    a.rounds, a.n_forced, a.tol, a.min_gain, a.stages, a.scen_per_wg = K, n_forced, tol, min_gain, stages, int(scen_per_wg)
    a.pnl, a.scen_flags = _ptr(pnl), _ptr(scen_flags)
    for k in shapes:
        setattr(a, k, _ptr(out[k]))
    _call(torch, "ivs_svi_hedge_f64", a, stream, params, Tq, spot, inst_u, inst_tau, inst_kind, pnl, scen_flags, *out.values())

    return {k: out[k] for k in shapes}


WHATIF_OUTPUTS = ("inst_pnl", "inst_value", "trade_flags", "var_w", "es_w", "worst_w", "best", "var0", "es0", "worst0", "n_scen")
WHATIF_OPTIONAL = ("worst_w", "inst_value")


def whatif_settings(lag, window, tail_probs, min_scen, n_inst, n_rungs, stages=0):
    """The host-side checks of a what-if ladder: those of hsim_settings, 1..64 candidates, 1..16 rungs,
    stages 0, 1 or 2; ValueError otherwise.  Returns (lag, window, tail_probs as a list, min_scen, n_rungs, stages)."""
    lag, window, tp, min_scen, _ = hsim_settings(lag, window, tail_probs, min_scen)
    if int(n_inst) != n_inst or not 1 <= n_inst <= _lib.HG_MAX_INST:
        raise ValueError(f"{n_inst!r} candidate instruments: 1..{_lib.HG_MAX_INST} are supported")
    if int(n_rungs) != n_rungs or not 1 <= n_rungs <= _lib.WI_MAX_RUNGS:
        raise ValueError(f"{n_rungs!r} sizes per candidate: 1..{_lib.WI_MAX_RUNGS} rungs are supported")
    if stages not in (0, 1, 2):
        raise ValueError(f"stages {stages!r} is not 0, 1 or 2")
    return lag, window, tp, min_scen, int(n_rungs), int(stages)


def svi_whatif(params, Tq, spot, rate, inst_u, inst_tau, inst_kind, pnl, scen_flags, size, *, inst_pnl=None, lag: int = 1,
               window: int = 256, tail_probs=DEFAULT_TAIL_PROBS, min_scen: int = 20, strike_mode: int = 0, want=WHATIF_OPTIONAL,
               out=None, stream=None, scen_per_wg: int = 0, stages: int = 0):
    """What-if VaR and expected shortfall of a book per candidate trade and size (ivs_svi_whatif_f64; rules W0-W9 of DESIGN.md
    section 22): what svi_hsim's var and es become when size[.., h, j] units of candidate h are added to the book, for every
    snapshot, candidate and rung in one launch, and the rung with the smallest ES per candidate and level.
    params, Tq, spot, rate, strike_mode, lag, window, tail_probs, min_scen, pnl, scen_flags, inst_u, inst_tau, inst_kind as in
    svi_hedge.  size float64 [nH,nQ] (one ladder for all snapshots) or [B,nH,nQ]: the quantity of candidate h to ADD at rung j; a
    rung whose size is not finite is not live.  whatif_settings has the limits.
    inst_pnl: with stages = 2 the rows [B,window,nH] the ladder is formed on (out['inst_pnl'] serves as well).
    want: which of worst_w [B,nH,nQ] and inst_value [B,nH] to compute; one left out is neither computed nor written (None).
    `out`: optional dict of preallocated outputs.  stages: 0 = everything, 1 = inst_pnl and inst_value alone, 2 = everything but those.
    Snapshots without a slice (mT == 0) are refused with ValueError, as svi_hedge refuses them.
    Returns dict(inst_pnl [B,window,nH], inst_value [B,nH], trade_flags int32 [B,nH], var_w, es_w [B,nH,nQ,nL], worst_w int32
    [B,nH,nQ], best int32 [B,nH,nL], var0, es0 [B,nL], worst0, n_scen int32 [B]) of device tensors; a rung that is not live has
    NaN, NaN and -1."""
    _check_strike_mode(strike_mode)
    want = _wanted(want, WHATIF_OPTIONAL)
    torch = require_device()
    params, Tq, spot, B, mT = _svi_inputs(torch, params, Tq, spot)
    if mT == 0:
        raise ValueError("mT = 0: there is no slice to revalue a candidate on")
    inst_u, inst_tau, inst_kind, _, nH = _option_queries(torch, B, inst_u, inst_tau, inst_kind)
    if inst_kind is None:
        raise TypeError("inst_kind must be a CUDA uint8 tensor [nH]")
    size = _f64(torch, size, "size")
    if size.dim() not in (2, 3) or size.shape[-2] != nH or (size.dim() == 3 and size.shape[0] != B):
        raise ValueError(f"size must be [nH, nQ] or [B, nH, nQ] with nH = {nH}")
    nQ = size.shape[-1]
    lag, window, tp, min_scen, nQ, stages = whatif_settings(lag, window, tail_probs, min_scen, nH, nQ, stages)
    hsim_settings(lag, window, tp, min_scen, scen_per_wg)
    nL = len(tp)
    pnl = _f64(torch, pnl, "pnl")
    if not scen_flags.is_cuda or scen_flags.dtype != torch.int32:
        raise TypeError("scen_flags must be a CUDA int32 tensor")
    scen_flags = scen_flags.contiguous()
    if tuple(pnl.shape) != (B, window) or tuple(scen_flags.shape) != (B, window):
        raise ValueError(f"pnl and scen_flags must be [B, window] = {(B, window)}")
    out = dict(out or {})
    if inst_pnl is not None:
        if out.get("inst_pnl") is not None and out["inst_pnl"] is not inst_pnl:
            raise ValueError("inst_pnl and out['inst_pnl'] are two tensors: give one")
        out["inst_pnl"] = inst_pnl
    if stages == 2 and out.get("inst_pnl") is None:
        raise ValueError("stages = 2 forms the ladder on inst_pnl as given")
    if B * window * nH >= 2 ** 31 or B * nH * nQ * max(nL, 1) >= 2 ** 31:
        raise ValueError(f"{B} snapshots x {nH} candidates x {window} scenarios or x {nQ} rungs x {nL} levels exceed one launch")
    i32, f64 = torch.int32, torch.float64
    one, two = stages != 2, stages != 1
    shapes = {"inst_pnl": ((B, window, nH), f64, True), "inst_value": ((B, nH), f64, one and "inst_value" in want),
              "trade_flags": ((B, nH), i32, two), "var_w": ((B, nH, nQ, nL), f64, two), "es_w": ((B, nH, nQ, nL), f64, two),
              "worst_w": ((B, nH, nQ), i32, two and "worst_w" in want), "best": ((B, nH, nL), i32, two),
              "var0": ((B, nL), f64, two), "es0": ((B, nL), f64, two), "worst0": ((B,), i32, two), "n_scen": ((B,), i32, two)}
    out = _outputs(torch, out, shapes, params.device)
    a = _slice_fields(_lib.WhatIfArgs(), params, Tq, spot, rate)
    a.inst_u, a.inst_tau, a.inst_stride, a.inst_kind = _ptr(inst_u), _ptr(inst_tau), (0 if inst_u.dim() == 1 else nH), _ptr(inst_kind)
    a.strike_mode, a.nH, a.lag, a.window, a.tail_probs, a.nL, a.min_scen = int(strike_mode), nH, lag, window, _doubles(tp), nL, min_scen
    a.nQ, a.size, a.size_stride, a.stages, a.scen_per_wg = nQ, _ptr(size), (0 if size.dim() == 2 else nH * nQ), stages, int(scen_per_wg)
    a.pnl, a.scen_flags = _ptr(pnl), _ptr(scen_flags)
    for k in shapes:
        setattr(a, k, _ptr(out[k]))
    _call(torch, "ivs_svi_whatif_f64", a, stream, params, Tq, spot, inst_u, inst_tau, inst_kind, pnl, scen_flags, size, *out.values())
    return {k: out[k] for k in shapes}


BOOTSTRAP_OUTPUTS = ("var0", "es0", "n_scen", "mean", "variance", "se", "quant", "rep")
DEFAULT_CI_PROBS = (0.05, 0.95)


def bootstrap_settings(window, tail_probs, min_scen, n_rep, block, seed, ci_probs):
    """The host-side checks of a bootstrap: window, tail_probs and min_scen as hsim_settings has them,
    n_rep and block integers in 1..1024, seed an integer in 0..2^64 - 1, at most 8 interval probabilities, each finite and inside
    (0, 1); ValueError otherwise.  Returns (window, tail_probs as a list, min_scen, n_rep, block, seed, ci_probs as a list)."""
    import math
    _, window, tp, min_scen, _ = hsim_settings(1, window, tail_probs, min_scen)
    for name, v, hi in (("n_rep", n_rep, _lib.BOOT_MAX_REP), ("block", block, _lib.BOOT_MAX_BLOCK)):
        if int(v) != v or not 1 <= v <= hi:
            raise ValueError(f"{name} {v!r} is not an integer in 1..{hi}")
    if int(seed) != seed or not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed {seed!r} is not an integer in 0..2^64 - 1")
    ci = [float(x) for x in ci_probs]
    if len(ci) > _lib.BOOT_MAX_CI:
        raise ValueError(f"{len(ci)} interval probabilities: at most {_lib.BOOT_MAX_CI} are supported")
    if any(not (math.isfinite(x) and 0.0 < x < 1.0) for x in ci):
        raise ValueError(f"interval probabilities must be finite and inside (0, 1), got {ci!r}")
    return window, tp, min_scen, int(n_rep), int(block), int(seed), ci


def hsim_bootstrap(pnl, scen_flags, tail_probs=DEFAULT_TAIL_PROBS, min_scen: int = 20, n_rep: int = 512, block: int = 1, seed: int = 0,
                   ci_probs=DEFAULT_CI_PROBS, want_rep: bool = False, out=None, stream=None):
    """Bootstrap standard errors and intervals for the VaR and expected shortfall of rows of scenario P&Ls (ivs_hsim_bootstrap_f64;
    rules C0-C9 of DESIGN.md section 23).  pnl float64 and scen_flags int32 [B, window] as svi_hsim returns them (or svi_hedge's
    pnl_hedged with the same flags).  Every row is ranked once; each of n_rep replicates draws n of its ranked scenarios again, in
    circular blocks of `block` consecutive ones in time order (block = the lag of overlapping scenarios keeps their dependence),
    and takes svi_hsim's VaR and ES of the draw.  bootstrap_settings has the limits.
    want_rep: whether to return the replicate values themselves [B, n_rep, 2, nL] (None otherwise; a workspace of that size is
    then allocated for the call).  `out`: optional dict of preallocated outputs (se is never one: it is formed from variance).
    Returns dict(var0, es0 [B,nL] and n_scen int32 [B]: svi_hsim's var, es and n_valid of the rows; mean, variance, se [B,2,nL] over
    the replicates, statistic 0 = VaR and 1 = ES, se = sqrt(variance); quant [B,2,nL,nC]: the replicates' quantiles at ci_probs;
    rep) of device tensors.  A row with fewer than min_scen ranked scenarios, or an infinite one, has NaN in all but the first three."""
    torch = require_device()
    pnl = _f64(torch, pnl, "pnl")
    if not scen_flags.is_cuda or scen_flags.dtype != torch.int32:
        raise TypeError("scen_flags must be a CUDA int32 tensor")
    scen_flags = scen_flags.contiguous()
    if pnl.dim() != 2 or tuple(scen_flags.shape) != tuple(pnl.shape):
        raise ValueError("pnl and scen_flags must be [B, window], of one shape")
    B, window = pnl.shape
    window, tp, min_scen, n_rep, block, seed, ci = bootstrap_settings(window, tail_probs, min_scen, n_rep, block, seed, ci_probs)
    nL, nC = len(tp), len(ci)
    if B * window >= 2 ** 31 or B * n_rep * 2 * max(nL, 1) >= 2 ** 31 or B * 2 * max(nL, 1) * max(nC, 1) >= 2 ** 31:
        raise ValueError(f"{B} rows x {window} scenarios, x {n_rep} replicates or x {nC} quantiles at {nL} levels exceed one launch")
    if out is not None and "se" in out:
        raise ValueError("se is formed from variance by the wrapper: it is no output of the call")
    i32, f64 = torch.int32, torch.float64
    shapes = {"var0": ((B, nL), f64, True), "es0": ((B, nL), f64, True), "n_scen": ((B,), i32, True), "mean": ((B, 2, nL), f64, True),
              "variance": ((B, 2, nL), f64, True), "quant": ((B, 2, nL, nC), f64, True), "rep": ((B, n_rep, 2, nL), f64, bool(want_rep))}
    out = _outputs(torch, out, shapes, pnl.device)
    lib = _lib.load()
    ws_bytes = 0 if want_rep else int(lib.ivs_hsim_bootstrap_workspace_bytes(B, n_rep, nL))
    ws = torch.empty(ws_bytes // 8, dtype=f64, device=pnl.device) if ws_bytes else None
    a = _lib.BootstrapArgs()
    a.pnl, a.scen_flags, a.B, a.window = _ptr(pnl), _ptr(scen_flags), B, window
    a.tail_probs, a.nL, a.min_scen, a.n_rep, a.block, a.seed, a.ci_probs, a.nC = _doubles(tp), nL, min_scen, n_rep, block, seed, _doubles(ci), nC
    for k in shapes:
        setattr(a, k, _ptr(out[k]))
    rc = lib.ivs_hsim_bootstrap_f64(a, _ptr(ws), ws_bytes, _stream(torch, stream))
    _hold_for_stream(torch, stream, pnl, scen_flags, ws, *out.values())
    _lib.check(rc, "ivs_hsim_bootstrap_f64")
    with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
        se = torch.sqrt(out["variance"])                     # allocated on the stream that writes it
    return {**{k: out[k] for k in shapes}, "se": se}


WEIGHTED_OUTPUTS = ("var_w", "es_w", "n_valid_w", "worst_w", "wsum", "n_eff", "pnl_w", "scale", "flags_w", "sigma")
WEIGHTED_OPTIONAL = ("pnl_w", "scale")


def age_weights(window, decay):
    """The weights of an age-weighted historical simulation as a host float64 array [window]: w_0 = 1.0 and
    w_{s+1} = w_s x decay by repeated multiplication, for a decay in (0, 1].  The same call gives the a_k of the running vol."""
    import math
    import numpy as np
    if int(window) != window or window < 1:
        raise ValueError(f"window {window!r} is not an integer >= 1")
    decay = float(decay)
    if not (math.isfinite(decay) and 0.0 < decay <= 1.0):
        raise ValueError(f"decay {decay!r} is not inside (0, 1]")
    w = np.empty(int(window), np.float64)
    x = np.float64(1.0)
    for s in range(int(window)):
        w[s] = x
        x = x * np.float64(decay)
    return w


def weighted_settings(window, lag, tail_probs, min_scen, vol_span=0, min_returns=20, scale_cap=3.0, stages=0):
    """The host-side checks of a weighted historical simulation: lag, window, tail_probs and min_scen as
    hsim_settings has them, vol_span an integer in 0..1024, and with vol_span > 0 min_returns an integer in 1..vol_span and scale_cap
    finite and >= 1; stages 0, 1 or 2; ValueError otherwise.  Returns (window, lag, tail_probs as a list, min_scen, vol_span,
    min_returns, scale_cap, stages)."""
    import math
    lag, window, tp, min_scen, _ = hsim_settings(lag, window, tail_probs, min_scen)
    if int(vol_span) != vol_span or not 0 <= vol_span <= _lib.HW_MAX_SPAN:
        raise ValueError(f"vol_span {vol_span!r} is not an integer in 0..{_lib.HW_MAX_SPAN}")
    if int(min_returns) != min_returns:
        raise ValueError(f"min_returns {min_returns!r} is not an integer")
    scale_cap = float(scale_cap)
    if vol_span > 0:
        if not 1 <= min_returns <= vol_span:
            raise ValueError(f"min_returns {min_returns!r} is not an integer in 1..{vol_span}, the vol_span")
        if not (math.isfinite(scale_cap) and scale_cap >= 1.0):
            raise ValueError(f"scale_cap {scale_cap!r} is not finite and >= 1")
    if stages not in (0, 1, 2):
        raise ValueError(f"stages {stages!r} is not 0, 1 or 2")
    return window, lag, tp, min_scen, int(vol_span), int(min_returns), scale_cap, int(stages)


def hsim_weighted(pnl, scen_flags, spot=None, *, lag: int = 1, tail_probs=DEFAULT_TAIL_PROBS, min_scen: int = 20, weight=None,
                  vol_span: int = 0, vol_weight=None, min_returns: int = 20, scale_cap: float = 3.0, stages: int = 0, sigma=None,
                  want=WEIGHTED_OPTIONAL, out=None, stream=None):
    """Age-weighted, volatility-scaled VaR and expected shortfall of rows of scenario P&Ls (ivs_hsim_weighted_f64; rules W0-W9 of
    DESIGN.md section 24).  pnl float64 and scen_flags int32 [B, window] as svi_hsim returns them, with that call's lag.  weight
    float64 [window] on the device: the probability weight of a scenario by its age s (None: 1.0 each; age_weights makes the usual
    ones).  vol_span = M > 0 turns the scaling on: spot float64 [B] of the snapshots and vol_weight float64 [M] on the device give the
    running vol sigma [B]; scenario s of snapshot p is multiplied by sigma[p] / sigma[p - lag - s], held inside [1 / scale_cap,
    scale_cap].  weighted_settings has the limits.  stages: 0 = everything, 1 = sigma alone (every other output None), 2 = the tail
    alone on `sigma` as given (float64 [B]; also accepted as out["sigma"]).
    want: which of pnl_w and scale to return (None otherwise).  `out`: optional dict of preallocated outputs.
    Returns dict(var_w, es_w [B,nL]; n_valid_w, worst_w int32 [B]; wsum, n_eff [B]; pnl_w, scale [B,window]; flags_w int32 [B,window]:
    scen_flags with the _lib.HW_* bits; sigma [B], None with vol_span == 0) of device tensors."""
    torch = require_device()
    want = _wanted(want, WEIGHTED_OPTIONAL)
    pnl = _f64(torch, pnl, "pnl")
    if not scen_flags.is_cuda or scen_flags.dtype != torch.int32:
        raise TypeError("scen_flags must be a CUDA int32 tensor")
    scen_flags = scen_flags.contiguous()
    if pnl.dim() != 2 or tuple(scen_flags.shape) != tuple(pnl.shape):
        raise ValueError("pnl and scen_flags must be [B, window], of one shape")
    B, window = pnl.shape
    window, lag, tp, min_scen, M, min_returns, scale_cap, stages = weighted_settings(window, lag, tail_probs, min_scen, vol_span, min_returns,
                                                                                      scale_cap, stages)
    nL = len(tp)
    if B * window >= 2 ** 31:
        raise ValueError(f"{B} rows x {window} scenarios exceed one launch")
    if weight is not None:
        weight = _f64(torch, weight, "weight")
        if tuple(weight.shape) != (window,):
            raise ValueError(f"weight must be [window] = [{window}]")
    if M > 0 and stages != 2:
        if spot is None or vol_weight is None:
            raise ValueError("vol_span > 0 needs spot and vol_weight")
        spot, vol_weight = _f64(torch, spot, "spot"), _f64(torch, vol_weight, "vol_weight")
        if spot.numel() != B or tuple(vol_weight.shape) != (M,):
            raise ValueError(f"spot must hold one price per row and vol_weight must be [vol_span] = [{M}]")
    else:
        spot = vol_weight = None
    out = dict(out or {})
    if sigma is not None:
        if "sigma" in out and out["sigma"] is not sigma:
            raise ValueError("sigma was given twice: as an argument and in out")
        out["sigma"] = sigma
    if M > 0 and stages == 2 and out.get("sigma") is None:
        raise ValueError("stages 2 with vol_span > 0 reads sigma: it must be given")
    tail = stages != 1
    i32, f64 = torch.int32, torch.float64
    shapes = {"var_w": ((B, nL), f64, tail), "es_w": ((B, nL), f64, tail), "n_valid_w": ((B,), i32, tail), "worst_w": ((B,), i32, tail),
              "wsum": ((B,), f64, tail), "n_eff": ((B,), f64, tail), "pnl_w": ((B, window), f64, tail and "pnl_w" in want),
              "scale": ((B, window), f64, tail and "scale" in want), "flags_w": ((B, window), i32, tail), "sigma": ((B,), f64, M > 0)}
    out = _outputs(torch, out, shapes, pnl.device)
    a = _lib.WeightedArgs()
    a.pnl, a.scen_flags, a.B, a.window, a.lag = _ptr(pnl), _ptr(scen_flags), B, window, lag
    a.tail_probs, a.nL, a.min_scen = _doubles(tp), nL, min_scen
    a.weight, a.spot, a.vol_weight = _ptr(weight), _ptr(spot), _ptr(vol_weight)
    a.vol_span, a.min_returns, a.scale_cap, a.stages = M, min_returns, scale_cap, stages
    for k in shapes:
        setattr(a, k, _ptr(out[k]))
    _call(torch, "ivs_hsim_weighted_f64", a, stream, pnl, scen_flags, weight, spot, vol_weight, *out.values())
    return {k: out[k] for k in shapes}


def place_output(run, shape, tries: int = 8, dtype=None, warm: int = 8, timed: int = 3):
    """Pick the output buffer a persistent caller should keep.  On MI355X the same surface kernel on the same inputs runs up
    to 8 % faster or slower depending on WHICH allocation it writes to (stable per buffer, independent of offsets inside
    it).  `run(out)` must launch the call on the current stream with `out` as its output tensor.
    Allocates `tries` candidates (all alive at once: distinct allocations), times `run` on each with HIP events (median of
    `timed` after `warm` untimed launches), returns (best_tensor, [median ms per candidate]); the others are freed."""
    torch = require_device()
    dtype = dtype or torch.float64
    cands = [torch.empty(shape, dtype=dtype, device="cuda") for _ in range(max(1, tries))]
    ms = []
    for o in cands:
        for _ in range(warm):
            run(o)
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(timed)]
        for s_, e_ in evs:
            s_.record(); run(o); e_.record()
        torch.cuda.synchronize()
        ms.append(sorted(s_.elapsed_time(e_) for s_, e_ in evs)[timed // 2])
    best = cands[ms.index(min(ms))]
    del cands
    torch.cuda.empty_cache()
    return best, ms


def last_kernel() -> str:
    return _lib.load().ivs_last_kernel().decode()


def interp1d_batch(xk, yk, knot_off, q_off, total_q: int, method, xq=None, stream=None) -> Tuple[object, object]:
    """CSR batch of 1-D series.  xk [TK], yk [C,TK], knot_off/q_off int64 [S+1] (device).
    Returns (out [C,total_q], status [S,C])."""
    torch = require_device()
    lib = _lib.load()
    code = _lib.METHOD_CODES[method] if isinstance(method, str) else int(method)
    xk = _f64(torch, xk, "xk"); yk = _f64(torch, yk, "yk")
    Cn, TK = yk.shape
    S = knot_off.numel() - 1
    dev = yk.device
    out = torch.empty((Cn, total_q), dtype=torch.float64, device=dev)
    status = torch.zeros((S, Cn), dtype=torch.int32, device=dev)
    wsb = lib.ivs_interp1d_workspace_bytes(TK, S, Cn)
    ws = torch.empty((wsb + 7) // 8, dtype=torch.float64, device=dev)
    rc = lib.ivs_interp1d_batch_f64(_ptr(xk), _ptr(yk), TK, _ptr(knot_off), S, Cn, TK,
                                    _ptr(xq), _ptr(q_off), total_q, _ptr(out), total_q, _ptr(status), code,
                                    _ptr(ws), ws.numel() * 8, _stream(torch, stream))
    _hold_for_stream(torch, stream, xk, yk, out, status, ws)
    _lib.check(rc, "ivs_interp1d_batch_f64")
    return out, status


def interp1d_greeks_batch(xk, yk, knot_off, q_off, total_q: int, method, channels, fidx, rows, strike_src, rate_src,
                          put_src, stream=None):
    """interp1d_batch with the Greeks epilogue (ivs_interp1d_greeks_batch_f64).  channels = (ch_iv, ch_S, ch_T); fidx int32
    [n_cols, total_q] from ffill_index_batch; rows = (row_strike, row_rate, row_callput) inside fidx or -1; *_src = source
    columns (float64, float64, uint8 0/1/2) or None.  Returns (out [C,total_q], status [S,C], greeks [5,total_q])."""
    torch = require_device()
    lib = _lib.load()
    code = _lib.METHOD_CODES[method] if isinstance(method, str) else int(method)
    xk = _f64(torch, xk, "xk"); yk = _f64(torch, yk, "yk")
    Cn, TK = yk.shape
    S = knot_off.numel() - 1
    dev = yk.device
    out = torch.empty((Cn, total_q), dtype=torch.float64, device=dev)
    greeks = torch.empty((5, total_q), dtype=torch.float64, device=dev)
    status = torch.zeros((S, Cn), dtype=torch.int32, device=dev)
    wsb = lib.ivs_interp1d_workspace_bytes(TK, S, Cn)
    ws = torch.empty((wsb + 7) // 8, dtype=torch.float64, device=dev)
    fidx = None if fidx is None else fidx.contiguous()
    rc = lib.ivs_interp1d_greeks_batch_f64(_ptr(xk), _ptr(yk), TK, _ptr(knot_off), S, Cn, TK, None, _ptr(q_off), total_q,
                                           _ptr(out), total_q, _ptr(status), code, int(channels[0]), int(channels[1]),
                                           int(channels[2]), _ptr(fidx), 0 if fidx is None else fidx.shape[1],
                                           int(rows[0]), int(rows[1]), int(rows[2]), _ptr(strike_src), _ptr(rate_src),
                                           _ptr(put_src), _ptr(greeks), total_q, _ptr(ws), ws.numel() * 8,
                                           _stream(torch, stream))
    _hold_for_stream(torch, stream, xk, yk, out, status, greeks, ws, fidx)
    _lib.check(rc, "ivs_interp1d_greeks_batch_f64")
    return out, status, greeks


def ffill_index_batch(src_pos, src_off, valid, q_off, total_q: int, stream=None):
    """valid uint8 [n_cols, total_src] -> int32 [n_cols, total_q] flat source-row index or -1."""
    torch = require_device()
    lib = _lib.load()
    n_cols, TS = valid.shape
    S = src_off.numel() - 1
    idx = torch.empty((n_cols, total_q), dtype=torch.int32, device=valid.device)
    valid = valid.contiguous()
    rc = lib.ivs_ffill_index_batch(_ptr(src_pos), _ptr(src_off), _ptr(valid), TS, n_cols, _ptr(q_off),
                                   S, total_q, _ptr(idx), total_q, _stream(torch, stream))
    _hold_for_stream(torch, stream, valid, idx)
    _lib.check(rc, "ivs_ffill_index_batch")
    return idx


def gather_rows(src, idx, idx_row, stream=None):
    """Columnar egress: out[c][g] = src[c][idx[idx_row[c]][g]] (NaN / -1 where the index is negative).  src float64 or int32
    [n_cols, n_src]; idx int32 [rows, n]; idx_row int32 [n_cols] (device)."""
    torch = require_device()
    lib = _lib.load()
    n_cols, n_src = src.shape
    n = idx.shape[1]
    out = torch.empty((n_cols, n), dtype=src.dtype, device=src.device)
    fn = lib.ivs_gather_rows_f64 if src.dtype == torch.float64 else lib.ivs_gather_rows_i32
    src = src.contiguous()
    rc = fn(_ptr(src), n_src, _ptr(idx), idx.shape[1], _ptr(idx_row), n_cols, n, _ptr(out), n, _stream(torch, stream))
    _hold_for_stream(torch, stream, src, out)
    _lib.check(rc, "ivs_gather_rows")
    return out


def frame_rows(q_off, first_ns, chan, sym_code, status, needs, stream=None):
    """Per output row: timestamp (int64 ns) and the dropna / failed-symbol keep flag (ivs_frame_rows)."""
    torch = require_device()
    lib = _lib.load()
    S = q_off.numel() - 1
    Cn, total_q = chan.shape
    dates = torch.empty(total_q, dtype=torch.int64, device=chan.device)
    keep = torch.empty(total_q, dtype=torch.uint8, device=chan.device)
    status = status.contiguous(); needs = needs.contiguous()
    rc = lib.ivs_frame_rows(_ptr(q_off), S, total_q, _ptr(first_ns), _ptr(chan), total_q, Cn, _ptr(sym_code), _ptr(status),
                            _ptr(needs), _ptr(dates), _ptr(keep), _stream(torch, stream))
    _hold_for_stream(torch, stream, status, needs, dates, keep)
    _lib.check(rc, "ivs_frame_rows")
    return dates, keep


def frame_columns(src_pos, src_off, q_off, total_q: int, yk, method, valid, fsrc, f_rows, csrc, c_rows, idx_rows,
                  first_ns=None, needs=None, sym_col: int = -1, greek=None, stream=None):
    """The long output frame in ONE pass over its rows (ivs_frame_columns_f64): channels on the integer lattice, the
    forward-filled f64 / code columns gathered straight from their source columns, raw gather-index rows for the columns the
    host gathers itself, the date column and the dropna keep flag, optionally the Greeks -- what interp1d_batch +
    ffill_index_batch + gather_rows (x2) + frame_rows do together, without the index arrays in between.

    src_pos int64 [n_src], src_off / q_off int64 [S+1], yk float64 [C, n_src], valid uint8 [V, n_src], fsrc float64
    [nF, n_src], csrc int32 [nC, n_src]; f_rows / c_rows / idx_rows: int32 device tensors naming the validity row of each
    column (or None); first_ns int64 [S] + needs uint8 [S, C] switch the date / keep outputs on; greek = (g_rows (3 ints, -1
    = column absent), strike_src, rate_src, put_src) or None.
    Returns dict(chan [C,total_q], status [S,C], F, C, idx, date_ns, keep, greeks) of device tensors (None where not asked)."""
    torch = require_device()
    lib = _lib.load()
    code = _lib.method_code(method) if isinstance(method, str) else int(method)
    dev = yk.device
    yk = _f64(torch, yk, "yk")
    Cn, n_src = yk.shape
    S = src_off.numel() - 1
    total_q = int(total_q)
    a = _lib.FrameArgs()
    keepalive = []

    def cont(t):
        t = t.contiguous(); keepalive.append(t); return t
    src_pos, src_off, q_off = cont(src_pos), cont(src_off), cont(q_off)
    a.src_pos, a.src_off, a.q_off = _ptr(src_pos), _ptr(src_off), _ptr(q_off)
    a.n_series, a.total_src, a.total_queries = S, n_src, total_q
    a.yk, a.yk_stride, a.n_channels, a.method = _ptr(yk), n_src, Cn, code
    chan = torch.empty((Cn, total_q), dtype=torch.float64, device=dev)
    status = torch.zeros((S, Cn), dtype=torch.int32, device=dev)
    a.chan_out, a.chan_stride, a.status = _ptr(chan), total_q, _ptr(status)
    nV = 0 if valid is None else valid.shape[0]
    if nV:
        valid = cont(valid)
    a.valid, a.valid_stride, a.n_valid = (_ptr(valid) if nV else 0), n_src, nV
    F = Cc = idx = None
    nF = 0 if fsrc is None else fsrc.shape[0]
    if nF:
        fsrc, f_rows = cont(fsrc), cont(f_rows)
        F = torch.empty((nF, total_q), dtype=torch.float64, device=dev)
        a.fsrc, a.fsrc_stride, a.f_rows, a.n_f, a.f_out, a.f_stride = _ptr(fsrc), n_src, _ptr(f_rows), nF, _ptr(F), total_q
    nC = 0 if csrc is None else csrc.shape[0]
    if nC:
        csrc, c_rows = cont(csrc), cont(c_rows)
        Cc = torch.empty((nC, total_q), dtype=torch.int32, device=dev)
        a.csrc, a.csrc_stride, a.c_rows, a.n_c, a.c_out, a.c_stride = _ptr(csrc), n_src, _ptr(c_rows), nC, _ptr(Cc), total_q
    nI = 0 if idx_rows is None else idx_rows.numel()
    if nI:
        idx_rows = cont(idx_rows)
        idx = torch.empty((nI, total_q), dtype=torch.int32, device=dev)
        a.idx_rows, a.n_idx, a.idx_out, a.idx_stride = _ptr(idx_rows), nI, _ptr(idx), total_q
    dates = keep = None
    a.sym_col = int(sym_col)
    if first_ns is not None:
        first_ns, needs = cont(first_ns), cont(needs)
        dates = torch.empty(total_q, dtype=torch.int64, device=dev)
        keep = torch.empty(total_q, dtype=torch.uint8, device=dev)
        a.first_ns, a.needs, a.date_ns, a.keep = _ptr(first_ns), _ptr(needs), _ptr(dates), _ptr(keep)
    greeks = None
    a.g_strike = a.g_rate = a.g_put = -1
    if greek is not None:
        g_rows, ksrc, rsrc, psrc = greek
        ksrc, rsrc, psrc = cont(ksrc), cont(rsrc), cont(psrc)
        greeks = torch.empty((5, total_q), dtype=torch.float64, device=dev)
        a.g_strike, a.g_rate, a.g_put = (int(x) for x in g_rows)
        a.strike_src, a.rate_src, a.put_src = _ptr(ksrc), _ptr(rsrc), _ptr(psrc)
        a.ch_iv, a.ch_underlying, a.ch_ttm = 0, 1, 2
        a.greeks, a.greeks_stride = _ptr(greeks), total_q
    wsb = lib.ivs_frame_workspace_bytes(n_src, S, Cn)
    ws = torch.empty((wsb + 7) // 8, dtype=torch.float64, device=dev)
    rc = lib.ivs_frame_columns_f64(a, _ptr(ws), ws.numel() * 8, _stream(torch, stream))
    _hold_for_stream(torch, stream, ws, chan, status, F, Cc, idx, dates, keep, greeks, *keepalive)
    _lib.check(rc, "ivs_frame_columns_f64")
    return {"chan": chan, "status": status, "F": F, "C": Cc, "idx": idx, "date_ns": dates, "keep": keep, "greeks": greeks}


def bs_greeks(S, K, T, r, sigma, is_put=None, default_is_put: bool = False, stream=None):
    """Black-Scholes Greeks on the device.  All inputs CUDA float64 tensors of one shape (is_put: uint8 or None).
    Returns dict(delta, gamma, theta, vega, rho) of tensors with that shape."""
    torch = require_device()
    lib = _lib.load()
    ins = [_f64(torch, t, n) for t, n in zip((S, K, T, r, sigma), ("S", "K", "T", "r", "sigma"))]
    n = ins[0].numel()
    if any(t.numel() != n for t in ins):
        raise ValueError("all inputs must have the same number of elements")
    if is_put is not None:
        is_put = is_put.to(torch.uint8).contiguous()
    outs = [torch.empty_like(ins[0]) for _ in range(5)]
    rc = lib.ivs_bs_greeks_f64(*[_ptr(t) for t in ins], _ptr(is_put), int(bool(default_is_put)), n,
                               *[_ptr(t) for t in outs], _stream(torch, stream))
    _lib.check(rc, "ivs_bs_greeks_f64")
    return dict(zip(("delta", "gamma", "theta", "vega", "rho"), outs))


def _option_inputs(torch, tensors, names, is_put):
    """The shared input checks of bs_price and bs_implied_vol: CUDA float64 tensors of one size, is_put uint8 / bool or None."""
    ins = [_f64(torch, t, n) for t, n in zip(tensors, names)]
    n = ins[0].numel()
    if any(t.numel() != n for t in ins):
        raise ValueError(f"{', '.join(names)} must have the same number of elements")
    if is_put is not None:
        if not is_put.is_cuda or is_put.numel() != n:
            raise ValueError("is_put must be a CUDA tensor with one entry per option")
        is_put = is_put.to(torch.uint8).contiguous()
    return ins, n, is_put


def bs_price(S, K, T, r, sigma, is_put=None, default_is_put: bool = False, want_vega: bool = False, out=None, stream=None,
             want_flags: bool = True):
    """Black-Scholes prices on the device (ivs_bs_price_f64; rules V1, V8 of DESIGN.md section 16).  All inputs CUDA float64
    tensors of one size (is_put: uint8 / bool or None -> default_is_put for every option).  vega is per unit of vol, not per
    1 % like bs_greeks'.  `out`: optional dict of preallocated outputs (price, vega float64, flags int32).  An output that is
    not wanted is neither computed nor written (None in the result).
    Returns dict(price, vega, flags) of tensors with S's shape; flags is _lib.IV_DEAD or 0."""
    torch = require_device()
    lib = _lib.load()
    ins, n, is_put = _option_inputs(torch, (S, K, T, r, sigma), ("S", "K", "T", "r", "sigma"), is_put)
    shape = tuple(ins[0].shape)
    shapes = {"price": (shape, torch.float64, True), "vega": (shape, torch.float64, bool(want_vega)),
              "flags": (shape, torch.int32, bool(want_flags))}
    out = _outputs(torch, out, shapes, ins[0].device, per_option=True)
    res = {k: out[k] for k in shapes}
    rc = lib.ivs_bs_price_f64(*[_ptr(t) for t in ins], _ptr(is_put), int(bool(default_is_put)), n,
                              _ptr(res["price"]), _ptr(res["vega"]), _ptr(res["flags"]), _stream(torch, stream))
    _hold_for_stream(torch, stream, *ins, is_put, *res.values())
    _lib.check(rc, "ivs_bs_price_f64")
    return res


PRICE_MODES = {"quote": 0, "underlying": 1}


def bs_implied_vol(price, S, K, T, r, is_put=None, default_is_put: bool = False, price_mode: int = 0, out=None, stream=None):
    """Price -> Black-Scholes implied volatility on the device (ivs_bs_implied_vol_f64; rules V1-V7 of DESIGN.md section 16).
    All inputs CUDA float64 tensors of one size (is_put: uint8 / bool or None -> default_is_put for every option).
    price_mode: 0 = `price` is in the units of S and K, 1 = `price` is quoted in units of the underlying (P = price S, as the
    chains' mark_price is); ValueError otherwise.  `out`: optional dict of preallocated outputs (vol float64, flags int32).
    Returns dict(vol, flags) of tensors with price's shape; the flags are the _lib.IV_* bits."""
    if price_mode not in (0, 1):
        raise ValueError(f"price_mode {price_mode!r} is neither 0 (quote) nor 1 (units of the underlying)")
    torch = require_device()
    lib = _lib.load()
    ins, n, is_put = _option_inputs(torch, (price, S, K, T, r), ("price", "S", "K", "T", "r"), is_put)
    shape = tuple(ins[0].shape)
    shapes = {"vol": (shape, torch.float64, True), "flags": (shape, torch.int32, True)}
    out = _outputs(torch, out, shapes, ins[0].device, per_option=True)
    res = {k: out[k] for k in shapes}
    rc = lib.ivs_bs_implied_vol_f64(*[_ptr(t) for t in ins], _ptr(is_put), int(bool(default_is_put)), int(price_mode), n,
                                    _ptr(res["vol"]), _ptr(res["flags"]), _stream(torch, stream))
    _hold_for_stream(torch, stream, *ins, is_put, *res.values())
    _lib.check(rc, "ivs_bs_implied_vol_f64")
    return res


def candle_aggregate(ts_ns, o, h, l, c, v, series_off, freq_minutes: int, stream=None):
    """Sparse N-minute aggregation on the device (see ivs_candle_aggregate_f64).  ts_ns int64, OHLCV float64, series_off
    int64 [S+1]; all CUDA tensors.  Returns (out_ts, open, high, low, close, volume, count) of length n."""
    torch = require_device()
    lib = _lib.load()
    n = ts_ns.numel()
    S = series_off.numel() - 1
    cols = [_f64(torch, t, nm) for t, nm in zip((o, h, l, c, v), "ohlcv")]
    out_ts = torch.empty(n, dtype=torch.int64, device=ts_ns.device)
    outs = [torch.empty(n, dtype=torch.float64, device=ts_ns.device) for _ in range(5)]
    cnt = torch.empty(n, dtype=torch.int32, device=ts_ns.device)
    rc = lib.ivs_candle_aggregate_f64(_ptr(ts_ns.contiguous()), *[_ptr(t) for t in cols], _ptr(series_off), S, n,
                                      int(freq_minutes) * 60_000_000_000, _ptr(out_ts), *[_ptr(t) for t in outs], _ptr(cnt),
                                      _stream(torch, stream))
    _lib.check(rc, "ivs_candle_aggregate_f64")
    return (out_ts, *outs, cnt)


BRIDGE_STRATEGIES = {"spread_simulation": 0, "price_as_midpoint": 1, "trend_following": 2, "simple_spread": 3,
                     "pipeline_inline": 4}


def mt19937_words(seed: int, n_words: int, device=None, stream=None):
    """The first n_words raw 32-bit outputs of ``np.random.seed(seed)`` as an int32 CUDA tensor (bit pattern of uint32)."""
    torch = require_device()
    lib = _lib.load()
    if not 0 <= int(seed) <= 0xFFFFFFFF:
        raise ValueError("Seed must be between 0 and 2**32 - 1")          # numpy's own message
    words = torch.empty(int(n_words), dtype=torch.int32, device=device or "cuda")
    rc = lib.ivs_mt19937_words_u32(int(seed), _ptr(words), int(n_words), _stream(torch, stream))
    _lib.check(rc, "ivs_mt19937_words_u32")
    return words


def bridge_words_bound(total_rows: int, strategy: int) -> int:
    """Words that certainly cover one bridge call: exact upper bound for the uniform strategies; for trend_following
    (rejection sampling) a generous estimate -- the call reports when it was not enough."""
    per_row = {0: 12, 1: 6, 2: 10, 3: 4, 4: 10}[int(strategy)]
    return int(total_rows) * per_row + 4096


def bridge_candles(price, volume, row_off, strategy: int, words, rng_tail=None, base_spread_pct: float = 0.002,
                   vol_factor: float = 1.5, stream=None):
    """IV -> OHLCV candles on the device (see ivs_bridge_candles_f64).  price float64 [n], volume float64 [n] or None,
    row_off int64 [S+1], words int32 [n_words] (from mt19937_words, positioned at this call's first draw), rng_tail
    int64 [4] or None (fresh generator).  Returns (out [6, n], valid uint8 [n], rng_tail)."""
    torch = require_device()
    lib = _lib.load()
    price = _f64(torch, price, "price")
    n = price.numel()
    S = row_off.numel() - 1
    if volume is not None:
        volume = _f64(torch, volume, "volume")
        if volume.numel() != n:
            raise ValueError("price and volume must have the same length")
    if rng_tail is None:
        rng_tail = torch.zeros(4, dtype=torch.int64, device=price.device)
    out = torch.empty((6, n), dtype=torch.float64, device=price.device)
    valid = torch.empty(n, dtype=torch.uint8, device=price.device)
    wsb = lib.ivs_bridge_workspace_bytes(n)
    ws = torch.empty((wsb + 7) // 8, dtype=torch.float64, device=price.device)
    rc = lib.ivs_bridge_candles_f64(_ptr(price), _ptr(volume), _ptr(row_off), S, n, int(strategy), float(base_spread_pct),
                                    float(vol_factor), _ptr(words), words.numel(), _ptr(out), _ptr(valid), _ptr(rng_tail),
                                    _ptr(ws), ws.numel() * 8, _stream(torch, stream))
    _lib.check(rc, "ivs_bridge_candles_f64")
    return out, valid, rng_tail
