"""GPU: the preallocated outputs of the snapshot-analytics wrappers (engine._outputs): a tensor of the right shape and dtype
comes back as the very same object, one of the wrong shape or dtype raises ValueError with the exact text, and svi_distribution
takes any number of tenors.  Tiny shapes: B = 2, mT = 3, mK = 5, Q = 3."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
B, MT, MK, Q = 2, 3, 5, 3
SLICE = (0.004, 0.05, -0.4, 0.03, 0.12)          # a, b, rho, m, sigma at tenor 0.1, scaled with the tenor below


def dev(a, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def surface():
    spot = np.array([100.0, 101.0])
    Kq = spot[:, None] * np.array([0.8, 0.9, 1.0, 1.1, 1.2])
    Tq = np.array([0.1, 0.25, 0.5])
    vol = 0.2 + 0.1 * (np.log(Kq / spot[:, None]) ** 2)[:, None, :] + 0.02 * Tq[None, :, None]
    return dev(vol), dev(Kq), dev(Tq), dev(spot)


def slices(mT=MT):
    Tq = 0.1 * np.arange(1, mT + 1)
    params = np.array([[(SLICE[0] * t / 0.1, SLICE[1] * t / 0.1) + SLICE[2:] for t in Tq]] * B)
    return dev(params), dev(Tq), dev(np.array([100.0, 101.0]))


def queries():
    return dev([0.9, 1.0, 1.1]), dev([0.15, 0.3, 0.7])


def chain():
    """One contract (a call at the only strike and expiry) quoted in two successive minutes: B = 2 snapshots, nT = nK = 1.
    The arguments of snapshot_assemble up to n_snapshots."""
    minute = 60 * 10**9
    return (dev([0, minute], np.int64), dev([0.5, 0.6]), dev([100.0, 101.0]), dev([0, 2], np.int64), dev([[0, -1]], np.int32),
            dev([100.0]), dev([10**15], np.int64), 0, B)


def _calls():
    import torch
    from iv_interpolation_amd import engine
    f64, i32 = torch.float64, torch.int32
    s, p, (u, tau) = surface(), slices(), queries()
    # wrapper -> (call taking `out`, an output key, its shape, its dtype)
    return {
        "snapshot_assemble": (lambda out: engine.snapshot_assemble(*chain(), dev([0.9, 1.0, 1.1]), 100.0, out=out), "Kq", (B, 3), f64),
        "smile_delta_points": (lambda out: engine.smile_delta_points(*s, out=out), "strike", (B, MT, 5), f64),
        "surface_arbitrage": (lambda out: engine.surface_arbitrage(*s, out=out), "counts", (B, 4), i32),
        "surface_moments": (lambda out: engine.surface_moments(*s, out=out), "index", (B, 1), f64),
        "svi_slices": (lambda out: engine.svi_slices(*s, fitted=True, out=out), "fitted", (B, MT, MK), f64),
        "ssvi_surface": (lambda out: engine.ssvi_surface(*s, raw=p[0], out=out), "sflags", (B,), i32),
        "svi_distribution": (lambda out: engine.svi_distribution(*p, probs=(0.1, 0.5), levels=(0.9,), out=out), "p_above", (B, MT, 1), f64),
        "svi_calendar": (lambda out: engine.svi_calendar(*p, out=out), "x_cross", (B, MT, 2), f64),
        "svi_eval": (lambda out: engine.svi_eval(*p, 0.01, u, tau, out=out), "flags", (B, Q), i32),
        "bs_price": (lambda out: engine.bs_price(u, u, tau, tau, tau, out=out), "price", (Q,), f64),
        "bs_implied_vol": (lambda out: engine.bs_implied_vol(tau, u, u, tau, tau, out=out), "flags", (Q,), i32),
    }


WRAPPERS = ("snapshot_assemble", "smile_delta_points", "surface_arbitrage", "surface_moments", "svi_slices", "ssvi_surface", "svi_distribution",
            "svi_calendar", "svi_eval", "bs_price", "bs_implied_vol")


@pytest.mark.parametrize("name", WRAPPERS)
def test_preallocated_output_is_checked_and_returned(name):
    import torch
    call, key, shape, dt = _calls()[name]
    other = torch.int32 if dt == torch.float64 else torch.float64
    flat = name.startswith("bs_")                    # the flat pricers take any shape with one entry per option
    text = f"out[{key!r}] must be a contiguous CUDA {dt} tensor " + ("with one entry per option" if flat else f"of shape {shape}")
    bad = [torch.empty(shape[:-1] + (shape[-1] + 1,), dtype=dt, device="cuda"), torch.empty(shape, dtype=other, device="cuda"),
           torch.empty(shape[:-1] + (2 * shape[-1],), dtype=dt, device="cuda")[..., ::2]]       # shape, dtype, not contiguous
    for t in bad:
        with pytest.raises(ValueError) as e:
            call({key: t})
        assert str(e.value) == text
    good = torch.empty(shape, dtype=dt, device="cuda")
    res = call({key: good})
    torch.cuda.synchronize()
    assert res[key] is good
    assert all(v is None or v.is_cuda for v in res.values())


def test_assemble_without_moneyness_has_no_kq():
    """Without moneyness the Kq output is off: None in the result even when `out` holds a Kq entry, which is neither checked nor
    written; the other preallocated entries are used as given."""
    import torch
    from iv_interpolation_amd import engine
    kq = torch.full((7,), -7.25e9, dtype=torch.float32, device="cuda")       # neither the shape nor the dtype of a Kq
    quotes = torch.full((B,), -77, dtype=torch.int32, device="cuda")
    res = engine.snapshot_assemble(*chain(), out={"Kq": kq, "quotes": quotes})
    torch.cuda.synchronize()
    assert set(res) == {"sigma", "T", "spot", "quotes", "Kq"} and res["Kq"] is None and res["quotes"] is quotes
    assert bool((kq == -7.25e9).all()) and quotes.tolist() == [1, 1]
    assert res["sigma"].cpu().tolist() == [[[0.5]], [[0.6]]] and res["spot"].cpu().tolist() == [100.0, 101.0]


def test_distribution_takes_more_than_64_tenors():
    """svi_distribution has never limited mT (neither the wrapper nor ivs_svi_distribution_f64 does: the calendar and the
    evaluation need one ballot of tenors per snapshot, the distribution treats every row on its own).  mT = 65 therefore runs,
    and every row carries the bits it gets in a call of its own snapshot split into 64 tenors and 1."""
    import torch
    from iv_interpolation_amd import engine
    params, Tq, spot = slices(65)
    whole = engine.svi_distribution(params, Tq, spot, 0.01)
    head = engine.svi_distribution(params[:, :64].contiguous(), Tq[:64], spot, 0.01)
    tail = engine.svi_distribution(params[:, 64:].contiguous(), Tq[64:], spot, 0.01)
    torch.cuda.synchronize()
    assert whole["flags"].shape == (B, 65) and int((whole["flags"] & 8).sum()) == 0           # no row is DEAD
    for k, v in whole.items():
        both = torch.cat([head[k], tail[k]], dim=1)
        assert v.shape == both.shape and v.dtype == both.dtype, k
        same = (v == both) | ((v != v) & (both != both))
        assert bool(same.all()), k
