"""GPU: the fixed-shape (64 x 16 quotes) row-pass kernel in its two instantiations -- query strikes shared by the batch
(KQS: `Kq` of shape [mK]) and per surface (`Kq` of shape [B, mK]) -- on the points its compile-time shape touches: idle
output lanes, work-queue claims of 4 surfaces (short, exact, one over, several per workgroup), strike tables kept from
surface to surface, and query strikes on and beyond the end knots (the selects that the fixed shape folds away).
All batches share T and Tq."""
import numpy as np
import pytest

from test_gpu_parity import ATOL, METHODS, RTOL, O, close, dev

pytestmark = pytest.mark.gpu

PASS_METHODS = ["linear", "cubic", "cubicspline", "slinear", "nearest", "zero", "pchip", "akima", "from_derivatives", "quadratic"]


def _call(d, Kq, Tq, method, **kw):
    from iv_interpolation_amd import engine
    out, st = engine.surface_batch(dev(d["K"]), dev(d["T"]), dev(d["sigma"]), dev(Kq), dev(Tq), method, **kw)
    return out.cpu().numpy(), st.cpu().numpy(), engine.last_kernel()


def _both(d, Kq, Tq, method):
    """The batch through both instantiations; returns the shared-grid result after checking that they agree bit for bit."""
    B = d["sigma"].shape[0]
    got, st, kern = _call(d, Kq, Tq, method)
    got2, st2, kern2 = _call(d, np.ascontiguousarray(np.broadcast_to(Kq, (B, Kq.shape[0]))), Tq, method)
    assert kern == kern2 == f"surface_pass_kernel<{method}>", (kern, kern2)
    assert np.array_equal(st, st2)
    assert got.tobytes() == got2.tobytes(), f"{method} B={B} mK={Kq.shape[0]}: Kq [mK] and [B, mK] differ"
    return got, st


@pytest.mark.parametrize("method", PASS_METHODS)
def test_shared_and_per_surface_query_strikes_agree(method):
    """Kq as [mK] and as its copy [B, mK]: bit-equal outputs, for output grids that leave lanes idle (mK 1, 37) and batch
    sizes around one claim of 4 surfaces."""
    from iv_interpolation_amd import synth
    for mK in (1, 37, 64):
        Kq, Tq = synth.query_grids(mK, 16)
        for B in (1, 3, 4, 5, 13):
            d = synth.numpy_batch(B, 64, 16, seed=synth.BASE_SEED + 900 + B)
            _, st = _both(d, Kq, Tq, method)
            assert not st.any()


def _runs_batch():
    """21 surfaces whose strike rows repeat in runs of 1, 2, 5, 5, 2, 1, 5; the second run of 5 (surfaces 8..12) has a
    missing quote in its third surface, which is tagged and redone elsewhere and must leave no tables behind."""
    from iv_interpolation_amd import synth
    runs = (1, 2, 5, 5, 2, 1, 5)
    B = sum(runs)
    d = synth.numpy_batch(B, 64, 16, seed=synth.BASE_SEED + 910)
    first = np.repeat(np.cumsum((0,) + runs[:-1]), runs)
    d["K"] = np.ascontiguousarray(d["K"][first])
    d["sigma"][10, 5, 20] = np.nan
    return d


@pytest.mark.parametrize("method", PASS_METHODS)
def test_kept_strike_tables_equal_one_surface_per_call(method):
    """Runs of equal strike rows, one of them interrupted by a tagged surface, against the same surfaces computed one per
    call (no tables to keep): bit for bit, with shared and with per-surface query strikes."""
    from iv_interpolation_amd import synth
    d = _runs_batch()
    B = d["sigma"].shape[0]
    Kq, Tq = synth.query_grids(64, 16)
    got, st = _both(d, Kq, Tq, method)
    for b in range(B):
        one = {"K": d["K"][b:b + 1], "T": d["T"], "sigma": d["sigma"][b:b + 1]}
        ref, rst, _ = _call(one, Kq, Tq, method)
        assert rst[0] == st[b], (b, rst[0], st[b])
        assert ref[0].tobytes() == got[b].tobytes(), f"{method}: surface {b} differs from its own one-surface call"


def test_more_than_one_claim_per_workgroup():
    """8 x 12 x (number of CUs) + 7 surfaces: every workgroup of the full grid claims several chunks and the last claim
    is short.  A strided sample against the oracle, the whole batch against the one-pass kernel, all statuses 0."""
    import torch
    from iv_interpolation_amd import synth
    B = 8 * 12 * torch.cuda.get_device_properties(0).multi_processor_count + 7
    d = synth.numpy_batch(B, 64, 16, seed=synth.BASE_SEED + 920)
    Kq, Tq = synth.query_grids(64, 16)
    got, st, kern = _call(d, Kq, Tq, "cubic")
    assert kern == "surface_pass_kernel<cubic>", kern
    assert not st.any()
    idx = np.unique(np.concatenate([np.arange(0, B, max(1, B // 500)), [B - 8, B - 7, B - 1]]))
    ref, rst = O.surface_batch(d["K"][idx], d["T"], d["sigma"][idx], Kq, Tq, METHODS["cubic"])
    assert not rst.any()
    close(got[idx], ref, "cubic", f"several claims per workgroup, sample of {idx.size}")
    one, st1, kern1 = _call(d, Kq, Tq, "cubic", one_pass=True)
    assert kern1 == "surface_dense_kernel<cubic>", kern1
    assert not st1.any()
    # test_gpu_parity holds both kernel families to the oracle at RTOL / ATOL and states no wider bound between them
    close(got, one, "cubic", "row-pass against one-pass, whole batch", tol=(RTOL, ATOL))


@pytest.mark.parametrize("method", ["cubic", "linear", "quadratic"])
def test_query_strikes_on_and_beyond_the_end_knots(method):
    """Query strikes below the first knot, equal to it, equal to the last knot and above it, against the oracle: the
    `lane < n` selects and index clamps that the fixed shape removes sat on exactly these lanes."""
    from iv_interpolation_amd import synth
    B = 6
    d = synth.numpy_batch(B, 64, 16, seed=synth.BASE_SEED + 930)
    k0, kl = 0.69, 1.31                                         # common end knots, per-surface interior knots
    d["K"][:, 0] = k0
    d["K"][:, -1] = kl
    assert (np.diff(d["K"], axis=1) > 0).all()
    _, Tq = synth.query_grids(64, 16)
    for mK in (64, 4):
        Kq = np.concatenate([[k0 - 0.01, k0], np.linspace(0.75, 1.25, mK - 4), [kl, kl + 0.01]])
        got, st = _both(d, Kq, Tq, method)
        ref, rst = O.surface_batch(d["K"], d["T"], d["sigma"], Kq, Tq, METHODS[method])
        assert np.array_equal(st, rst)
        close(got, ref, method, f"end knots {method} mK={mK}")
