"""Greeks kernel at the edges of float64: an exact (mpmath) fixture over eight regimes, launch geometry, the scalar option
type, and out-of-domain inputs against the float64 oracle.  The error unit and the 4 U_oracle + 4 rule are stated in
greeks_edges_ref.py; IVS_ERRLOG=<file> appends the measured U_kernel next to U_oracle for every group."""
import importlib.util
import os

import numpy as np
import pytest

import greeks_edges_cases as C
import greeks_edges_ref as R
from golden_io import GOLDEN

G = R.G
PATH = os.path.join(GOLDEN, "greeks_edges.npz")
fx = dict(np.load(PATH))
N = fx["S"].size
INPUTS = ("S", "K", "T", "r", "sigma")


def _oracle_by_type(fn=G.calculate_greeks, **kw):
    with np.errstate(all="ignore"):
        return {typ: fn(*[fx[k] for k in INPUTS], typ == "put", **kw) for typ in R.TYPES}


# ---- CPU: the fixture itself, and that its assertions can tell wrong code from right code
def test_fixture_layout():
    assert os.path.getsize(PATH) < 256 * 1024
    assert list(fx["regimes"]) == list(C.REGIMES) and N == len(C.REGIMES) * C.N_PER_REGIME
    assert np.array_equal(fx["regime"], np.repeat(np.arange(len(C.REGIMES)), C.N_PER_REGIME))
    for ri, name in enumerate(C.REGIMES):                   # the inputs are the case table's, bit for bit
        for k, a in zip(INPUTS, C.regime_inputs(name)):
            assert np.array_equal(fx[k][fx["regime"] == ri], a), (name, k)
    assert np.isfinite(fx["exact"]).all() and np.isfinite(fx["theta_scale"]).all() and np.isfinite(fx["U_oracle"]).all()
    grp = R.group_of(fx["d1"])
    assert all((grp == gi).sum() >= 64 for gi in range(3))  # every group is populated
    wings = fx["regime"] == C.REGIMES.index("wings")
    assert (grp[wings] == 1).all()
    atm = fx["regime"] == C.REGIMES.index("atm")
    assert (fx["K"][atm] == fx["S"][atm]).sum() == C.N_PER_REGIME // 3 and (fx["r"][atm] == 0).sum() >= C.N_PER_REGIME // 3
    assert (fx["r"][atm] < 0).any() and (fx["exact"][:, 1][:, grp == 2] == 0).any()       # a negative rate; gamma underflows to 0


def test_fixture_regenerates_from_mpmath():
    """16 points per regime evaluated again in mpmath must equal the committed file (the GPU test reads only the file)."""
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_golden_greeks_edges", os.path.join(GOLDEN, "make_golden_greeks_edges.py"))
    gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
    k = 16
    part = gen.build(k)
    idx = (np.arange(len(C.REGIMES))[:, None] * C.N_PER_REGIME + np.arange(k)[None, :]).ravel()
    for key in INPUTS + ("d1", "d2", "regime"):
        assert np.array_equal(part[key], fx[key][idx]), key
    assert np.array_equal(part["exact"], fx["exact"][:, :, idx]) and np.array_equal(part["theta_scale"], fx["theta_scale"][:, idx])


def test_oracle_passes_the_fixture_assertions():
    bad, _ = R.fixture_violations(_oracle_by_type(), fx)
    assert bad == []
    bad, _ = R.fixture_violations(_oracle_by_type(R.wrong_greeks, mistake=None), fx)
    assert bad == []


@pytest.mark.parametrize("mistake", ["one_minus_erf", "no_rate_in_d1", "put_delta_sign"])
def test_fixture_separates_wrong_greeks(mistake):
    bad, _ = R.fixture_violations(_oracle_by_type(R.wrong_greeks, mistake=mistake), fx)
    assert bad, mistake


def _degenerate_reference():
    ins = C.degenerate_inputs()
    with np.errstate(all="ignore"):
        return ins, {typ: (G.calculate_greeks(*ins, typ == "put"), R.theta_scale_f64(*ins, typ == "put")) for typ in R.TYPES}


def test_degenerate_table_reaches_every_pattern():
    """The table must hold NaN, +inf, -inf and exact zeros in the oracle's outputs, or it pins nothing."""
    ins, ref = _degenerate_reference()
    assert 50 <= len(C.DEGENERATE) <= 80
    allv = np.concatenate([ref[typ][0][k] for typ in R.TYPES for k in R.GREEKS])
    assert np.isnan(allv).any() and (allv == np.inf).any() and (allv == -np.inf).any() and (allv == 0).any()
    for typ in R.TYPES:                                     # and the comparison accepts the oracle, rejects a wrong put delta
        assert R.degenerate_violations(ref[typ][0], ref[typ][0], ref[typ][1], typ == "put", fx["U_oracle"][0, R.TYPES.index(typ)]) == []
    with np.errstate(all="ignore"):
        wrong = R.wrong_greeks(*ins, True, "put_delta_sign")
    assert R.degenerate_violations(wrong, ref["put"][0], ref["put"][1], True, fx["U_oracle"][0, 1])


# ---- GPU
@pytest.fixture(scope="module")
def single_launch():
    """The whole fixture, calls then puts, with a per-element option type in ONE launch: dict greek -> float64 [2 N]"""
    import torch
    from iv_interpolation_amd import engine
    ins = [torch.from_numpy(np.concatenate([fx[k], fx[k]])).cuda() for k in INPUTS]
    put = torch.from_numpy(np.repeat([0, 1], N).astype(np.uint8)).cuda()
    out = engine.bs_greeks(*ins, is_put=put)
    torch.cuda.synchronize()
    return ins, put, out


def _by_type(out):
    return {typ: {k: v.cpu().numpy()[t * N:(t + 1) * N] for k, v in out.items()} for t, typ in enumerate(R.TYPES)}


@pytest.mark.gpu
def test_hip_greeks_against_exact_fixture(single_launch):
    bad, U = R.fixture_violations(_by_type(single_launch[2]), fx)
    print("\n".join(f"{R.GROUPS[gi]:12s} {typ:4s} {k:5s} U_kernel={U[gi, t, j]:.4g} U_oracle={fx['U_oracle'][gi, t, j]:.4g}"
                    for gi in range(3) for t, typ in enumerate(R.TYPES) for j, k in enumerate(R.GREEKS)))
    path = os.environ.get("IVS_ERRLOG")
    if path:
        with open(path, "a") as f:
            for gi in range(3):
                for t, typ in enumerate(R.TYPES):
                    for j, k in enumerate(R.GREEKS):
                        f.write(f"{U[gi, t, j]:.3e} {fx['U_oracle'][gi, t, j]:.3e} greeks_edges U_kernel U_oracle {R.GROUPS[gi]} {typ} {k}\n")
    assert bad == []


@pytest.mark.gpu
@pytest.mark.parametrize("default_put", [False, True])
def test_hip_greeks_scalar_option_type(single_launch, default_put):
    import torch
    from iv_interpolation_amd import engine
    ins, _, base = single_launch
    sl = slice(N, 2 * N) if default_put else slice(0, N)
    out = engine.bs_greeks(*[t[:N] for t in ins], is_put=None, default_is_put=default_put)
    for k in R.GREEKS:
        assert torch.equal(out[k].view(torch.int64), base[k][sl].view(torch.int64)), k


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, "grid"])
def test_hip_greeks_launch_geometry(single_launch, n):
    """Every element equals, bit for bit, what the same input got in the single launch, whatever block and grid-stride trip it
    lands in ('grid' = 2 x 16 blocks per CU x 256 + 77: a second and a partial third trip), and nothing is written past n."""
    import torch
    from iv_interpolation_amd import _lib
    ins, put, base = single_launch
    if n == "grid":
        n = 2 * 16 * 256 * torch.cuda.get_device_properties(0).multi_processor_count + 77
    idx = torch.arange(n, device="cuda") % (2 * N)
    tiled = [t[idx].contiguous() for t in ins]
    tput = put[idx].contiguous()
    guard = 64
    outs = [torch.full((n + guard,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(5)]
    rc = _lib.load().ivs_bs_greeks_f64(*[t.data_ptr() for t in tiled], tput.data_ptr(), 0, n, *[t.data_ptr() for t in outs],
                                       torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "ivs_bs_greeks_f64")
    torch.cuda.synchronize()
    for k, o in zip(R.GREEKS, outs):
        assert torch.equal(o[:n].view(torch.int64), base[k][idx].view(torch.int64)), k
        assert bool(torch.isnan(o[n:]).all()), k


@pytest.mark.gpu
def test_hip_greeks_degenerate_inputs_follow_the_oracle():
    import torch
    from iv_interpolation_amd import engine
    ins, ref = _degenerate_reference()
    m = len(C.DEGENERATE)
    out = engine.bs_greeks(*[torch.from_numpy(np.concatenate([a, a])).cuda() for a in ins],
                           is_put=torch.from_numpy(np.repeat([0, 1], m).astype(np.uint8)).cuda())
    bad = []
    for t, typ in enumerate(R.TYPES):
        got = {k: v.cpu().numpy()[t * m:(t + 1) * m] for k, v in out.items()}
        bad += [f"{typ} {b}" for b in R.degenerate_violations(got, ref[typ][0], ref[typ][1], typ == "put", fx["U_oracle"][0, t])]
    assert bad == [], "\n".join(bad + [f"row {i}: {row}" for i, row in enumerate(C.DEGENERATE)])
