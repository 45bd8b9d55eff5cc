"""References and comparisons of tests/test_bridge_edges.py.

Candles: oracle/bridge_oracle.py (pinned by the real reference's goldens), computed once per case and shared.  The
comparison applies the project's tolerances: open / high / low / close / source_price bit-exact (trend_following prices
atol 2e-4: the polar method's log / sqrt on the device), a drawn volume atol 1.000001e-6 (device log), a passed-through
volume exact, valid and the NaN pattern exact.  Rounding: Python's round, and NumPy restatements of the device's
py_round -- the shipped one and three wrong ones -- with the product's residual taken exactly."""
import functools
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import bridge_oracle as BO  # noqa: E402

import bridge_edges_cases as C  # noqa: E402

COLS = BO.OUT_COLS
TREND = 2
TREND_ATOL = 2.0e-4
DRAWN_VOLUME_ATOL = 1.000001e-6


def drawn_mask(batch):
    """Rows whose volume comes from an exponential draw."""
    v = batch["volume"]
    return np.isnan(v) | (v <= 0)


@functools.lru_cache(maxsize=None)
def _oracle(key, strategy, seed, kw):
    return BO.candles_batch(_BATCHES[key]["price"], _BATCHES[key]["volume"], _BATCHES[key]["off"], strategy, seed, **dict(kw))


_BATCHES = {}


def oracle(key, batch, strategy, seed=C.SEED, **kw):
    """(valid, out[6, n]) of the oracle for a named batch on one stream; computed once, shared, never modified."""
    _BATCHES[key] = batch
    valid, out = _oracle(key, strategy, seed, tuple(sorted(kw.items())))
    valid.setflags(write=False); out.setflags(write=False)
    return valid, out


def oracle_chain_not_reset(batch, strategy, seed=C.SEED):
    """WRONG on purpose: the previous-close chain runs on across symbol boundaries (the stream is unaffected)."""
    return BO.candles_batch(batch["price"], batch["volume"], np.array([0, len(batch["price"])]), strategy, seed)


def stream_reference(batches, strategy, rs, **kw):
    """[(valid, out)] of consecutive calls on the RandomState rs (advanced in place)."""
    res = []
    for b in batches:
        n = len(b["price"])
        valid, out = np.zeros(n, bool), np.full((6, n), np.nan)
        for s in range(len(b["off"]) - 1):
            a, e = int(b["off"][s]), int(b["off"][s + 1])
            v, d = BO.candles(b["price"][a:e], b["volume"][a:e], strategy, rs=rs, **kw)
            valid[a:e] = v
            for j, k in enumerate(COLS):
                out[j, a + np.flatnonzero(v)] = d[k]
        res.append((valid, out))
    return res


def state_after(seed, used_words, has_gauss, gauss):
    """The RandomState of ``seed`` after ``used_words`` 32-bit words, with the given cached normal deviate."""
    rs = np.random.RandomState(seed)
    if used_words:                                   # bytes(0) would still draw one word
        rs.bytes(4 * int(used_words))
    st = rs.get_state()
    rs.set_state((st[0], st[1], st[2], int(has_gauss), float(gauss)))
    return rs


def same_stream_position(a, b):
    """Two RandomStates are at the same word of the same stream.  Right after seeding the state reads position 624 of
    the seed array, after the first draw position k of the first generated block: compare through one more draw."""
    a2, b2 = np.random.RandomState(), np.random.RandomState()
    a2.set_state(a.get_state()); b2.set_state(b.get_state())
    return np.array_equal(a2.bytes(4 * 700), b2.bytes(4 * 700))


def errlog(what, diff_max, share):
    path = os.environ.get("IVS_ERRLOG")
    if path:
        with open(path, "a") as f:
            f.write(f"{diff_max:.3e} {share:.3e} bridge_edges max|diff| share_differing {what}\n")


def violations(what, got_out, got_valid, ref_valid, ref_out, batch, strategy, log=True):
    """List of the comparisons that fail (empty: all hold); appends the measured differences to the error log."""
    bad = []
    got_out, got_valid = np.asarray(got_out), np.asarray(got_valid).astype(bool)
    if not np.array_equal(got_valid, ref_valid):
        bad.append(f"{what}: valid differs on {int((got_valid != ref_valid).sum())} rows")
    if not np.array_equal(np.isnan(got_out), np.isnan(ref_out)):
        bad.append(f"{what}: NaN pattern differs on {int((np.isnan(got_out) != np.isnan(ref_out)).sum())} cells")
    drawn = drawn_mask(batch)
    for j, k in enumerate(COLS):
        g, r = got_out[j], ref_out[j]
        with np.errstate(all="ignore"):
            d = np.abs(g - r)
        d[(g == r) | (np.isnan(g) & np.isnan(r))] = 0.0            # equal infinities; NaN against a number stays NaN below
        differs = ~((g == r) | (np.isnan(g) & np.isnan(r)))
        worst = float(np.nanmax(d)) if d.size else 0.0
        share = float(differs.mean()) if d.size else 0.0
        if log:
            errlog(f"{what} {k}", worst, share)
        if k == "volume":
            if differs[~drawn].any():
                bad.append(f"{what}: passed-through volume differs on {int(differs[~drawn].sum())} rows")
            if not np.allclose(g[drawn], r[drawn], rtol=0, atol=DRAWN_VOLUME_ATOL, equal_nan=True):
                bad.append(f"{what}: drawn volume off by {float(np.nanmax(d[drawn])):.3e}")
        elif strategy == TREND and k != "source_price":
            if not np.allclose(g, r, rtol=0, atol=TREND_ATOL, equal_nan=True):
                bad.append(f"{what}: {k} off by {worst:.3e} (atol {TREND_ATOL})")
        elif differs.any():
            i = int(np.flatnonzero(differs)[0])
            bad.append(f"{what}: {k} differs on {int(differs.sum())} rows, worst {worst:.3e}, first row {i}: "
                       f"price {batch['price'][i]!r} got {g[i]!r} expected {r[i]!r}")
    return bad


# ---------------------------------------------------------------- rounding
def python_round(x, nd):
    return np.array([round(float(v), nd) for v in np.asarray(x, np.float64)])


def device_round(x, nd, tie="residual", threshold=True):
    """NumPy restatement of py_round in csrc/ivs_bridge.hpp.  As shipped: tie='residual', threshold=True.
    threshold=False is the formula before the 2^53 rule (rint(x p10) / p10 whatever the size of the product); tie='none'
    drops the residual correction (rint of the float product alone); tie='half_away' rounds the float product half away
    from zero."""
    x = np.asarray(x, np.float64)
    p10 = np.float64(10.0 ** nd)
    with np.errstate(all="ignore"):
        p = x * p10
        r = np.rint(p)
        t = p - r
        if tie == "half_away":
            r = np.copysign(np.floor(np.abs(p) + 0.5), p)
        elif tie == "residual":
            for i in np.flatnonzero(np.abs(t) == 0.5):
                e = Fraction(float(x[i])) * Fraction(float(p10)) - Fraction(float(p[i]))       # the FMA residual, exactly
                if t[i] == 0.5 and e > 0:
                    r[i] += 1.0
                if t[i] == -0.5 and e < 0:
                    r[i] -= 1.0
        res = r / p10
        keep = (np.abs(x) * p10 < 2.0 ** 53) if threshold else np.isfinite(x)
    return np.where(keep, res, x)


def rounding_violations(nd, **variant):
    """Indices into rounding_values(nd) on which the restatement and Python's round differ in any bit, for x or -x."""
    x = C.rounding_values(nd)
    bad = [np.flatnonzero(device_round(s * x, nd, **variant).view(np.int64) != python_round(s * x, nd).view(np.int64))
           for s in (1.0, -1.0)]
    return np.union1d(*bad)
