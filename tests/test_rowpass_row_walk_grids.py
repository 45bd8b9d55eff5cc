"""No GPU: the query-maturity grids of test_rowpass_row_walk_gpu.py against the oracle alone.  Every grid must reach the
row walk (ascending, NaN-free Tq; clean quotes: status 0) and must yield NaN exactly in the rows the rules name -- left of
T[0] for every method, right of T[-1] unless the method holds (linear) or extrapolates (cubicspline, pchip) -- and finite
values everywhere else, so that no case of the GPU tests is vacuous."""
import numpy as np
import pytest

from test_rowpass_row_walk_gpu import METHODS, PASS_METHODS, ROW_GRIDS, O, expected_nan_rows


def test_grids_cover_the_row_patterns():
    from iv_interpolation_amd import synth
    T = synth.tenors(16)
    per_iv = {name: np.histogram(Tq[(Tq >= T[0]) & (Tq < T[-1])], bins=T)[0] for name, Tq in ROW_GRIDS.items()}
    assert any(c.max() == 16 and c.sum() == 16 for c in per_iv.values())                 # all rows in one interval
    assert any((c == 1).all() for c in per_iv.values())                                  # exactly one row per interval
    tails = [c for c in per_iv.values() if {1, 2, 3} <= set(c.tolist())]
    assert any(any(tuple(c[j:j + 3]) in ((1, 2, 3), (3, 2, 1)) for j in range(13)) for c in tails)      # neighbouring odd / even tails
    assert any(any(c[j] >= 4 and c[j + 1] == 0 and c[j + 2:].max() >= 4 for j in range(13)) for c in per_iv.values())   # empty between full
    assert any((Tq < T[0]).sum() > 1 for Tq in ROW_GRIDS.values())
    assert any((Tq > T[-1]).sum() > 1 for Tq in ROW_GRIDS.values())
    assert any(np.isin(T, Tq).all() for Tq in ROW_GRIDS.values())                        # rows on every knot, T[0] and T[-1] included
    for Tq in ROW_GRIDS.values():
        assert (np.diff(Tq) > 0).all() and np.isfinite(Tq).all()


@pytest.mark.parametrize("method", PASS_METHODS)
def test_oracle_nan_rows_are_where_the_rules_say(method):
    from iv_interpolation_amd import synth
    d = synth.numpy_batch(3, 64, 16, seed=synth.BASE_SEED + 940)
    for name, Tq in ROW_GRIDS.items():
        for mK in (1, 37, 64):
            Kq, _ = synth.query_grids(mK, 16)
            ref, st = O.surface_batch(d["K"], d["T"], d["sigma"], Kq, Tq, METHODS[method])
            assert ref.shape == (3, Tq.size, mK) and not st.any(), (name, mK)
            want = np.broadcast_to(expected_nan_rows(Tq, method)[None, :, None], ref.shape)
            assert np.array_equal(np.isnan(ref), want), f"{method}: {name}, mK={mK}"
            assert np.isfinite(ref[~want]).all(), f"{method}: {name}, mK={mK}"
