"""GPU: the row walk of the maturity pass in the fixed-shape (64 x 16 quotes) row-pass kernel.  The instantiation for
query strikes shared by the batch (`Kq` of shape [mK]) walks the output rows with one running 32-bit offset per stream and
loads a row's weights at the use; the one for per-surface query strikes (`Kq` of shape [B, mK]) keeps the two running
pointers and the request one row ahead.  (The methods with slopes -- cubic, cubicspline, quadratic, pchip, akima -- take
the new walk; for the others both instantiations walk the old way and the comparison is the one of
test_rowpass_fixed_shape_gpu.py.)  Every batch goes through both (bit-equal outputs) and against the oracle, on
query maturities that put the rows into the intervals in every pattern a re-indexed walk has to survive.
All batches share T and Tq; ROW_GRIDS is checked against the oracle alone in test_rowpass_row_walk_grids.py (no GPU)."""
import numpy as np
import pytest

from test_gpu_parity import ATOL, METHODS, RTOL, O, close, dev

pytestmark = pytest.mark.gpu

PASS_METHODS = ["linear", "cubic", "cubicspline", "slinear", "nearest", "zero", "pchip", "akima", "from_derivatives", "quadratic"]
HOLDS_RIGHT = ("linear", "cubicspline", "pchip")      # finite right of T[-1]: np.interp's clamp / extrapolation


def tq_grid(counts=(), left=0, right=0, knots=()):
    """Ascending query maturities: `left` rows below T[0], counts[j] rows strictly inside (T[j], T[j+1]), the knots
    T[k] for k in `knots`, `right` rows above T[-1]."""
    from iv_interpolation_amd import synth
    T = synth.tenors(16)
    rows = [T[0] * (0.5 + 0.4 * i / max(left, 1)) for i in range(left)]
    for j, n in enumerate(counts):
        rows += [T[j] + (i + 1) / (n + 1) * (T[j + 1] - T[j]) for i in range(n)]
    rows += [T[k] for k in knots]
    rows += [T[-1] * (1.0 + 0.01 * (i + 1)) for i in range(right)]
    return np.sort(np.asarray(rows, np.float64))


def _counts(d):
    c = [0] * 15
    for j, n in d.items():
        c[j] = n
    return c


# name -> Tq.  mT in 1, 2, 15, 16, 17 and 64
ROW_GRIDS = {
    "all 16 rows in one interval": tq_grid(_counts({7: 16})),
    "all 64 rows in one interval": tq_grid(_counts({10: 64})),
    "one row per interval (15)": tq_grid([1] * 15),
    "1, 2, 3 rows in neighbouring intervals (16)": tq_grid(_counts({2: 1, 3: 2, 4: 3, 5: 1, 6: 2, 7: 3, 8: 1, 9: 2, 10: 1})),
    "3, 2, 1 rows, first and last interval included (17)": tq_grid(_counts({0: 3, 1: 2, 2: 1, 12: 3, 13: 2, 14: 3}), knots=(0, 7, 15)),
    "empty intervals between full ones (16)": tq_grid(_counts({0: 4, 3: 4, 5: 4, 14: 4})),
    "rows left of T[0] (16)": tq_grid(_counts({0: 1, 1: 2, 6: 3, 14: 1}), left=9),
    "rows on knots (16)": tq_grid(knots=range(16)),
    "rows right of T[-1] (16)": tq_grid(_counts({13: 2, 14: 3}), knots=(15,), right=10),
    "left, knots, tails, right (17)": tq_grid(_counts({1: 1, 2: 2, 3: 3, 9: 2, 14: 1}), left=2, knots=(0, 1, 15), right=3),
    "one row inside": tq_grid(_counts({3: 1})),
    "one row on T[0]": tq_grid(knots=(0,)),
    "one row left": tq_grid(left=1),
    "two rows: T[0] and T[-1]": tq_grid(knots=(0, 15)),
    "two rows: left and right": tq_grid(left=1, right=1),
    "64 rows of every kind": tq_grid([1, 2, 3, 0, 4, 1, 0, 0, 5, 2, 3, 1, 6, 2, 7], left=3, knots=range(16), right=8),
}
assert sorted({g.size for g in ROW_GRIDS.values()}) == [1, 2, 15, 16, 17, 64]


def expected_nan_rows(Tq, method):
    """Rows that are NaN by the rules: left of T[0] for every method; right of T[-1] unless the method holds or extrapolates."""
    from iv_interpolation_amd import synth
    T = synth.tenors(16)
    return (Tq < T[0]) | ((Tq > T[-1]) & (method not in HOLDS_RIGHT))


def _call(d, Kq, Tq, method):
    from iv_interpolation_amd import engine
    out, st = engine.surface_batch(dev(d["K"]), dev(d["T"]), dev(d["sigma"]), dev(Kq), dev(Tq), method)
    return out.cpu().numpy(), st.cpu().numpy(), engine.last_kernel()


def _both(d, Kq, Tq, method, what):
    """The batch through the new walk (Kq [mK]) and the old one (Kq [B, mK]): bit-equal, the row-pass kernel both times."""
    B = d["sigma"].shape[0]
    got, st, kern = _call(d, Kq, Tq, method)
    got2, st2, kern2 = _call(d, np.ascontiguousarray(np.broadcast_to(Kq, (B, Kq.shape[0]))), Tq, method)
    assert kern == kern2 == f"surface_pass_kernel<{method}>", (what, kern, kern2)
    assert not st.any() and not st2.any(), what
    assert got.tobytes() == got2.tobytes(), f"{what}: Kq [mK] (new row walk) and [B, mK] (old row walk) differ"
    return got


def _against_oracle(d, Kq, Tq, method, what):
    got = _both(d, Kq, Tq, method, what)
    ref, rst = O.surface_batch(d["K"], d["T"], d["sigma"], Kq, Tq, METHODS[method])
    assert not rst.any(), what
    nan_rows = expected_nan_rows(Tq, method)
    assert np.array_equal(np.isnan(got), np.broadcast_to(nan_rows[None, :, None], got.shape)), f"{what}: NaN rows"
    close(got, ref, method, what, tol=(RTOL, ATOL))


@pytest.mark.parametrize("method", PASS_METHODS)
def test_row_patterns(method):
    """Every grid of ROW_GRIDS, 5 surfaces (one claim of 4 and one of 1), output grids of 37 and 64 strikes in turn."""
    from iv_interpolation_amd import synth
    d = synth.numpy_batch(5, 64, 16, seed=synth.BASE_SEED + 940)
    for i, (name, Tq) in enumerate(ROW_GRIDS.items()):
        Kq, _ = synth.query_grids((37, 64)[i & 1], 16)
        _against_oracle(d, Kq, Tq, method, f"{method}: {name}, mK={Kq.size}")


@pytest.mark.parametrize("method", PASS_METHODS)
def test_idle_lanes_and_claims_of_four(method):
    """mK in 1, 37, 64 (idle output lanes) x B in 1, 3, 4, 5, 13 (around a claim of 4 surfaces) on a 17-row grid with left
    rows, hold rows, odd and even tails and right rows."""
    from iv_interpolation_amd import synth
    Tq = ROW_GRIDS["left, knots, tails, right (17)"]
    for mK in (1, 37, 64):
        Kq, _ = synth.query_grids(mK, 16)
        for B in (1, 3, 4, 5, 13):
            d = synth.numpy_batch(B, 64, 16, seed=synth.BASE_SEED + 950 + B)
            _against_oracle(d, Kq, Tq, method, f"{method}: B={B} mK={mK}")


_BIG = {}


def _big_batch():
    """8 x 12 x (number of CUs) + 7 surfaces, generated once for the module and left unchanged."""
    if not _BIG:
        import torch
        from iv_interpolation_amd import synth
        B = 8 * 12 * torch.cuda.get_device_properties(0).multi_processor_count + 7
        _BIG.update(synth.numpy_batch(B, 64, 16, seed=synth.BASE_SEED + 960))
    return _BIG


@pytest.mark.parametrize("method", ["cubic", "linear", "pchip", "akima", "quadratic"])
def test_several_claims_per_workgroup(method):
    """A batch in which every workgroup of the full grid claims several chunks and the last claim is short.  Both walks
    bit-equal on the whole batch, a strided sample against the oracle."""
    from iv_interpolation_amd import synth
    d = _big_batch()
    B = d["sigma"].shape[0]
    Kq, _ = synth.query_grids(37, 16)
    Tq = ROW_GRIDS["3, 2, 1 rows, first and last interval included (17)"]
    got = _both(d, Kq, Tq, method, f"{method}: several claims per workgroup")
    idx = np.unique(np.concatenate([np.arange(0, B, max(1, B // 300)), [B - 8, B - 7, B - 1]]))
    ref, rst = O.surface_batch(d["K"][idx], d["T"], d["sigma"][idx], Kq, Tq, METHODS[method])
    assert not rst.any()
    close(got[idx], ref, method, f"{method}: several claims per workgroup, sample of {idx.size}", tol=(RTOL, ATOL))
