"""libivs.so is linked from several translation units (iv_interpolation_amd/csrc/*.hip) that share one per-thread call state
(ivs_host.hpp).  CPU: the library exports the C ABI and nothing else that looks like it, and the error string is one per
thread across the units.  GPU: so is ivs_last_kernel(), with the conventions of the older entry points kept."""
import ctypes as C
import subprocess
import threading

import numpy as np
import pytest

from iv_interpolation_amd import _lib


def test_dynamic_symbols_are_the_c_abi():
    """nm -D --defined-only: the ivs_* names are the signatures' keys exactly, and no other defined dynamic symbol is a
    plain (unmangled) C function -- the host helpers the units share are hidden."""
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    syms = [line.split()[-2:] for line in out.splitlines() if len(line.split()) >= 2]
    assert sorted(n for _, n in syms if n.startswith("ivs_")) == sorted(_lib.SIGNATURES)
    stray = [n for kind, n in syms if kind in "TtWwi" and not n.startswith("_Z") and not n.startswith("ivs_")]
    assert stray == []


def _surface(lib, B):
    return lib.ivs_surface_batch_f64(None, None, 0, 64, None, 0, 16, None, B, None, 0, 64, None, 0, 16, None, None, 0, 0, None, 0, None)


def _svi_eval(lib, args):
    return lib.ivs_svi_eval_f64(C.byref(args) if args is not None else None, None, 0, None)


def _gather(lib, n):
    return lib.ivs_gather_rows_f64(None, 0, None, 0, None, 1, n, None, 0, None)


# (the call that fails on validation, its entry point's name, a zero-size call of ANOTHER unit that returns IVS_OK before any HIP call)
CROSS_UNIT = [
    (lambda lib: _surface(lib, -1), b"ivs_surface_batch_f64", lambda lib: _svi_eval(lib, _lib.EvalArgs())),      # surface -> analytics
    (lambda lib: _svi_eval(lib, None), b"ivs_svi_eval_f64", lambda lib: _gather(lib, 0)),                        # analytics -> frame
    (lambda lib: _gather(lib, -1), b"ivs_gather_rows_f64", lambda lib: _surface(lib, 0)),                        # frame -> surface
]


@pytest.mark.parametrize("fails,name,empty", CROSS_UNIT, ids=["surface-analytics", "analytics-frame", "frame-surface"])
def test_error_string_is_shared_by_the_units(fails, name, empty):
    lib = _lib.load()
    assert fails(lib) == -22 and name in lib.ivs_last_error()
    assert empty(lib) == 0 and lib.ivs_last_error() == b""


def test_error_string_is_per_thread():
    lib = _lib.load()
    assert _gather(lib, -1) == -22 and lib.ivs_last_error() != b""
    seen = []
    t = threading.Thread(target=lambda: seen.append(lib.ivs_last_error()))
    t.start(); t.join()
    assert seen == [b""]
    assert b"ivs_gather_rows_f64" in lib.ivs_last_error()


@pytest.mark.gpu
def test_last_kernel_across_units():
    """One stream, five calls of three units: the analytics and surface entries and ivs_bs_price_f64 name their kernel,
    ivs_bs_greeks_f64 and ivs_gather_rows_f64 leave the name alone (the names are those the single-unit library reported)."""
    import torch
    from iv_interpolation_amd import engine, synth
    d = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()  # noqa: E731
    params = np.tile([0.04, 0.4, -0.3, 0.0, 0.2], (1, 2, 1))
    engine.svi_eval(d(params), d([0.25, 0.5]), d([100.0]), 0.01, d([100.0]), d([0.3]))
    assert engine.last_kernel() == "svi_eval_kernel"
    b = synth.numpy_batch(3, 64, 16)
    Kq, Tq = synth.query_grids(64, 16, nT=16)
    engine.surface_batch(d(b["K"]), d(b["T"]), d(b["sigma"]), d(Kq), d(Tq), "linear")
    assert engine.last_kernel() == "surface_pass_kernel<linear>"
    S, K, T, r, sg = (d(v) for v in ([100.0, 101.0, 99.0], [100.0] * 3, [0.5] * 3, [0.01] * 3, [0.2] * 3))
    engine.bs_greeks(S, K, T, r, sg)
    assert engine.last_kernel() == "surface_pass_kernel<linear>"
    engine.bs_price(S, K, T, r, sg)
    assert engine.last_kernel() == "bs_price_kernel"
    engine.gather_rows(d(np.arange(6.0).reshape(2, 3)), d([[0, 2, -1]], np.int32), d([0, 0], np.int32))
    assert engine.last_kernel() == "bs_price_kernel"
    torch.cuda.synchronize()
