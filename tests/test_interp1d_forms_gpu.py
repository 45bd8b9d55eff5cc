"""GPU: all 14 methods on every block form of interp1d_prepare_kernel, interp1d_eval_kernel and frame_fused_kernel, against the
oracle, on the layouts of interp1d_forms_cases.py (test_interp1d_forms.py shows without a GPU that they reach every form, that
the splines are well conditioned there and that the oracle obeys the end rules on them).

Bounds: 'linear', 'nearest', 'zero', 'from_derivatives', 'pad', 'bfill' bit-exact; the others rtol 1e-12 / atol 1e-13 (the bound
of test_real1d_golden for these kernels); 'barycentric' / 'krogh' add a share of the curve's largest magnitude by knot count, as
test_polynomial_methods_on_gpu_vs_oracle_and_knot_limit scales it.  Rows that are a knot of their channel hold the source cell
exactly.  IVS_ERRLOG=<file> appends the measured error of every comparison."""
import functools

import numpy as np
import pytest

import interp1d_forms_cases as F
from interp1d_forms_cases import O
from test_gpu_parity import _errlog, dev, fused_equals_separate
from test_interp1d_forms import poly_tol

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-12, 1e-13


def layout_of(method):
    return F.layout_p() if method in F.POLY else F.layout_m()


@functools.lru_cache(maxsize=None)
def queries(method):
    return F.off_lattice_queries(layout_of(method))


@functools.lru_cache(maxsize=None)
def reference(method, explicit=False, C=3):
    if C < 3:                                              # the channels are independent: the first rows of the full reference
        ref, st = reference(method, explicit)
        return ref[:C], st[:, :C]
    ref, st = F.merged_reference(layout_of(method), method, queries(method) if explicit else None, C)
    ref.setflags(write=False); st.setflags(write=False)
    return ref, st


def compare(got, st, ref, rst, lay, method, what, xq=None):
    """status, NaN pattern and values of `got` [C, total_q] against the merged reference; a failure names the series, the channel,
    the block forms (by the host mirror) and the worst row"""
    C = got.shape[0]
    fm = F.forms(lay, method, C=C, greeks=False)
    assert np.array_equal(st, rst), f"{what}: status differs in (series, channel) {np.argwhere(st != rst)[:5].tolist()}"
    n, _ = F.knot_counts(lay, method, C)
    S = len(lay["tags"])
    _errlog(f"{what} {method}", got, ref)
    with np.errstate(invalid="ignore"):
        tol = np.zeros_like(ref) if method in F.EXACT else ATOL + RTOL * np.abs(ref)
    if method in F.POLY:
        for s in range(S):
            sl = slice(int(lay["q_off"][s]), int(lay["q_off"][s + 1]))
            for c in range(C):
                if 0 < n[s, c] <= F.POLY_MAX_KNOTS and np.isfinite(ref[c, sl]).any():
                    tol[c, sl] += poly_tol(n[s, c]) * np.nanmax(np.abs(ref[c, sl]))
    nan_bad = np.isnan(got) != np.isnan(ref)
    if nan_bad.any():
        c, g = np.argwhere(nan_bad)[0]
        raise AssertionError(f"{what}: NaN pattern ({int(nan_bad.sum())} rows), first: got {got[c, g]!r}, expected {ref[c, g]!r} at "
                             + F.describe_row(lay, fm, int(g), int(c)) + ("" if xq is None else f", xq = {xq[g]!r}"))
    with np.errstate(invalid="ignore"):
        over = np.where(np.isnan(ref), 0.0, np.abs(got - ref) - tol)
    if (over > 0).any():
        c, g = np.unravel_index(np.argmax(over), over.shape)
        raise AssertionError(f"{what}: {int((over > 0).sum())} rows beyond the bound, worst |diff| {abs(got[c, g] - ref[c, g]):.3e} "
                             f"(bound {tol[c, g]:.3e}, value {ref[c, g]!r}) at " + F.describe_row(lay, fm, int(g), int(c))
                             + ("" if xq is None else f", xq = {xq[g]!r}"))
    # rows that are a knot of their channel hold the source cell, bit for bit (tolerances above or not)
    ks = np.repeat(np.arange(S), lay["sizes"])
    gpos = lay["q_off"][:-1][ks] + lay["pos"]
    for c in range(C):
        y = lay["yk"][c]
        okk = ~np.isnan(y) & (rst[ks, c] != O.ST_ILL_CONDITIONED)
        assert np.array_equal(got[c, gpos[okk]], y[okk]), f"{what}: knot rows of channel {c} do not hold their source cell"


@pytest.mark.parametrize("method", F.METHODS)
def test_interp1d_batch_on_the_lattice(method):
    import torch
    from iv_interpolation_amd import engine
    lay = layout_of(method)
    out, st = engine.interp1d_batch(dev(lay["pos"].astype(np.float64)), dev(lay["yk"]), dev(lay["src_off"]), dev(lay["q_off"]),
                                    int(lay["q_off"][-1]), method)
    torch.cuda.synchronize()
    ref, rst = reference(method)
    compare(out.cpu().numpy(), st.cpu().numpy(), ref, rst, lay, method, "interp1d lattice")


@pytest.mark.parametrize("method", F.METHODS)
def test_interp1d_batch_with_explicit_queries(method):
    """off-lattice queries, queries exactly on knots, one below the first and one above the last knot of every series; the same
    counts per series as the lattice, so the eval kernel takes the same forms"""
    import torch
    from iv_interpolation_amd import engine
    lay = layout_of(method)
    xq = queries(method)
    on_knot = xq[lay["q_off"][:-1][np.repeat(np.arange(len(lay["tags"])), lay["sizes"])] + lay["pos"]] == lay["pos"]
    assert on_knot.all() and (xq[lay["q_off"][1:] - 2] < 0).all() and (xq[lay["q_off"][1:] - 1] > lay["pos"][lay["src_off"][1:] - 1]).all()
    assert (xq != np.floor(xq)).mean() > 0.9
    out, st = engine.interp1d_batch(dev(lay["pos"].astype(np.float64)), dev(lay["yk"]), dev(lay["src_off"]), dev(lay["q_off"]),
                                    int(lay["q_off"][-1]), method, xq=dev(xq))
    torch.cuda.synchronize()
    ref, rst = reference(method, True)
    got = out.cpu().numpy()
    compare(got, st.cpu().numpy(), ref, rst, lay, method, "interp1d explicit xq", xq)


@pytest.mark.parametrize("variant", ["greeks", "plain", "one_channel"])
@pytest.mark.parametrize("method", F.METHODS)
def test_frame_columns_on_every_form(method, variant):
    """the fused pass bit for bit against the separate calls, and its channels against the oracle at the bounds above: with the
    Greeks epilogue, without it, and with a single channel"""
    lay = layout_of(method)
    C = 1 if variant == "one_channel" else 3
    got = fused_equals_separate(F.frame_case(lay), method, greeks=variant == "greeks", C=C)
    ref, rst = reference(method, False, C)
    # the status is compared inside fused_equals_separate (fused == separate) and by the lattice test (separate == oracle)
    compare(got, rst, ref, rst, lay, method, f"frame_columns {variant}")


@pytest.mark.parametrize("dense", [False, True], ids=["spaced", "dense"])
def test_frame_columns_beyond_65535_knots_in_one_series(dense):
    """One series of 70 000 valid knots, one channel, no Greeks.  20..24 rows apart every block's window holds ~190 source rows,
    but the window form keeps knot ranks and counts in 16 bits: such a symbol has to take the per-row path (before
    FR_MAXKNOTS the count was truncated to 4464 and every row behind that knot was wrong).  1..2 rows apart (per-row path by the
    window's size) is the control.  'linear' bit-exact against np.interp, 'pchip' against the oracle."""
    import torch
    from iv_interpolation_amd import engine
    lay = F.layout_long(dense)
    total_q = int(lay["q_off"][-1])
    x, y = lay["pos"].astype(np.float64), lay["yk"][0]
    for method in ("linear", "pchip"):
        got = engine.frame_columns(dev(lay["pos"]), dev(lay["src_off"]), dev(lay["q_off"]), total_q, dev(lay["yk"][:1]), method,
                                   None, None, None, None, None, None)
        torch.cuda.synchronize()
        g = got["chan"].cpu().numpy()
        assert got["status"].cpu().numpy().tolist() == [[O.ST_OK]]
        if method == "linear":
            ref = np.interp(np.arange(total_q, dtype=np.float64), x, y)[None, :]
            ref[0, lay["pos"]] = y
        else:
            ref, rst = F.merged_reference(lay, method, None, 1)
        compare(g, np.zeros((1, 1), np.int32), ref, np.zeros((1, 1), np.int32), lay, method, f"frame_columns 70000 knots {'dense' if dense else 'spaced'}")
