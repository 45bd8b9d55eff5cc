"""No GPU: what test_interp1d_forms_gpu.py rests on.  The constants mirrored in interp1d_forms_cases.py equal the headers; its
layouts reach every block form of the prepare, eval and frame kernels under every method (by the host mirror `forms`); the
spline methods are well conditioned on them (so the GPU comparison can be tight); and the oracle's result there obeys the
methods' end rules and reproduces the knots, asserted from the rules and not from the oracle's code."""
import collections
import os
import re

import numpy as np
import pytest

import interp1d_forms_cases as F
from interp1d_forms_cases import O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = {"M": (F.layout_m, [m for m in F.METHODS if m not in F.POLY]), "P": (F.layout_p, list(F.POLY))}
CASES = [(name, m) for name, (_, ms) in LAYOUTS.items() for m in ms]
# poly methods: tolerance relative to the curve's largest magnitude by knot count, as test_polynomial_methods_on_gpu_vs_oracle_
# and_knot_limit scales it (the conditioning of one polynomial through n almost equispaced knots grows like 2^n)
POLY_TOL = ((10, 1e-11), (17, 1e-10), (25, 1e-9), (32, 1e-6))


# 'krogh' at its own knots: the Newton form sums n products of up to n factors (x - x_k); on (almost) equispaced knots the terms
# outgrow the value like 2^n, so the far knots come back to n 2^n eps of the curve's scale (the kernels keep the source cell there)
EPS = np.finfo(np.float64).eps


def poly_tol(n):
    return next(t for k, t in POLY_TOL if n <= k)


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_mirrored_constants_equal_the_headers():
    i1, fr, dev = (_read("iv_interpolation_amd", "csrc", n) for n in ("ivs_interp1d.hpp", "ivs_frame.hpp", "ivs_device.hpp"))
    api = _read("include", "ivs.h")

    def const(text, name):
        m = re.search(r"constexpr int %s = ([^;]+);" % name, text)
        assert m, name
        return m.group(1).strip()
    assert int(const(i1, "P1_STAGE")) == F.P1_STAGE and int(const(i1, "E1_STAGE")) == F.E1_STAGE
    assert const(i1, "E1_ROWS") == "256 * E1_RPT" and 256 * int(const(i1, "E1_RPT")) == F.E1_ROWS
    assert const(fr, "FR_ROWS") == "256 * 2 * FR_UNITS" and 512 * int(const(fr, "FR_UNITS")) == F.FR_ROWS
    assert const(fr, "FR_CAP") == "IVS_FR_CAP" and int(re.search(r"#define IVS_FR_CAP (\d+)", fr).group(1)) == F.FR_CAP
    for name in ("FR_MAXSYM", "FR_MAXKNOTS", "FR_MAXV", "FR_MAXC", "FR_MAXF", "FR_MAXCC"):
        assert int(const(fr, name)) == getattr(F, name), name
    assert int(re.search(r"#define IVS_POLY_MAX_KNOTS (\d+)", api).group(1)) == F.POLY_MAX_KNOTS == O.POLY_MAX_KNOTS
    # method codes (include/ivs.h) and minimum knot counts (method_min_knots' switch; default: 2)
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"IVS_([A-Z_]+?)\s*=\s*(\d+)[, ]\s*/\*", api) if not m.group(1).startswith("ST_")}
    assert [codes[m] for m in F.METHODS] == list(range(14)) and all(O.METHOD_CODES[m] == codes[m] for m in F.METHODS)
    body = re.search(r"int method_min_knots\(int m\) \{(.*?)\n\}", dev, re.S).group(1)
    mins = {}
    for line in body.splitlines():
        r = re.search(r"return (\d+);", line)
        if r and "case" in line:
            mins.update({n.lower(): int(r.group(1)) for n in re.findall(r"IVS_([A-Z_]+)", line)})
    default = int(re.search(r"default: return (\d+);", body).group(1))
    for m in F.METHODS:
        assert mins.get(m, default) == F.MIN_KNOTS[m] == O.min_knots(O.METHOD_CODES[m]), m


def test_layout_m_holds_the_symbols_the_forms_need():
    lay = F.layout_m()
    assert int(lay["q_off"][-1]) <= 250_000
    n, _ = F.knot_counts(lay, "linear")
    by = collections.defaultdict(list)
    for s, t in enumerate(lay["tags"]):
        by[t].append(s)
    gaps = lambda s: np.diff(lay["pos"][lay["src_off"][s]:lay["src_off"][s + 1]])        # noqa: E731
    assert len(by["ref"]) >= 3 and all(lay["sizes"][s] == 64 and (gaps(s) == 60).all() for s in by["ref"])
    s, = by["long400"]; assert 380 <= lay["sizes"][s] <= 440 and gaps(s).min() >= 25 and gaps(s).max() <= 40 and n[s].min() > 4 * F.WAVE
    s, = by["dense1200"]; assert n[s].min() > F.P1_STAGE and gaps(s).max() <= 5
    mids = [s for t in by if t.startswith("mid") for s in by[t]]
    assert len(mids) == 3 and all(260 <= lay["sizes"][s] <= 300 for s in mids) and np.ptp(mids) == 2
    assert all(1 <= lay["sizes"][s] <= 5 and (lay["sizes"][s] == 1 or (1 <= gaps(s).min() and gaps(s).max() <= 3)) for s in by["tiny"])
    assert all(lay["sizes"][s] == 5 and gaps(s).min() >= 1000 for s in by["sparse"])
    yk = lambda t, c: lay["yk"][c, lay["src_off"][by[t][0]]:lay["src_off"][by[t][0] + 1]]      # noqa: E731
    assert np.isnan(yk("ref_lead", 0)[:5]).all() and not np.isnan(yk("ref_lead", 0)[5:]).any()
    assert np.isnan(yk("ref_trail", 1)[-6:]).all() and not np.isnan(yk("ref_trail", 1)[:-6]).any()
    assert 0.05 < np.isnan(yk("long400", 0)).mean() < 0.25 and 0.05 < np.isnan(yk("dense1200", 2)).mean() < 0.25
    assert n[by["ref_no0"][0], 0] == 0 and n[by["ref_no1"][0], 1] == 0
    assert n[by["ref_few"][0]].tolist() == [3, 2, 1]             # below the minimum of cubic / akima, quadratic / the other splines
    assert lay["pos"][lay["src_off"][by["ref_at3"][0]]] == 3
    assert (gaps(by["ref_consecutive"][0]) == 1).sum() >= 3 and any((gaps(s) == 1).any() for s in by["tiny"] if lay["sizes"][s] > 1)
    assert (np.diff(lay["q_off"]) - lay["pos"][lay["src_off"][1:] - 1] - 1 >= 3).all()      # >= 3 rows behind every last source row


@pytest.mark.parametrize("name,method", CASES)
def test_every_form_of_every_kernel_is_reached(name, method):
    lay = LAYOUTS[name][0]()
    fm = F.forms(lay, method)
    prep = collections.Counter(x for row in fm["prepare"] for x in row)
    want = {"cubic": ("scan",), "cubicspline": ("scan", "thread"), "pchip": ("thread",), "akima": ("thread",), "quadratic": ("thread",),
            "barycentric": ("table",), "krogh": ("table",)}.get(method, ())
    for k in want + (("global",) if method in F.SOLVED else ()) + ("none",):
        assert prep[k] >= 2, (k, prep)
    if method in ("cubic", "cubicspline"):              # the scan crosses several 64-knot blocks, and stops short of one
        n, _ = F.knot_counts(lay, method)
        assert ((n > 4 * F.WAVE) & (n <= F.P1_STAGE)).any() and ((n >= 4) & (n < F.WAVE)).any() and (n == F.WAVE).any()
    ev = collections.Counter(b[0][0] if len({e[0] for e in b}) == 1 else "mixed" for b in fm["eval"])
    ev_any = collections.Counter(f for b in fm["eval"] for f in {e[0] for e in b})
    for k in ("one", "two", "multi") + (("one_big", "two_big") if name == "M" else ()):
        assert ev_any[k] >= 2, (k, ev, ev_any)
    if name == "M":                                     # two series staged, one of them without a knot in the channel
        two = [e for b in fm["eval"] for e in b if e[0] == "two"]
        assert any(e[1] == 0 for e in two) and any(e[2] == 0 for e in two)
    fr = collections.Counter((b["form"], b["why"]) for b in fm["frame"])
    for k in (("whole", ""), ("window", ""), ("perrow", "nsym")) + ((("perrow", "rows"),) if name == "M" else ()):
        assert fr[k] >= 2, (k, fr)
    assert sum(1 for b in fm["frame"] if b["src_rows"] == 0) >= 2                       # blocks without a source row inside
    if name == "M":      # the window form as the first, an interior and the last block of one symbol, three in a row at least
        s = lay["tags"].index("long400")
        mine = [b for b in fm["frame"] if b["s_first"] <= s <= b["s_last"]]
        assert len(mine) >= 4 and all(b["form"] == "window" for b in mine)
        assert mine[0]["s_first"] < s and mine[-1]["s_last"] > s and sum(1 for b in mine if b["s_first"] == b["s_last"] == s) >= 2
    else:
        assert (F.knot_counts(lay, method)[0] > F.POLY_MAX_KNOTS).any()


def test_the_long_series_takes_the_window_form_and_its_control_the_per_row_path():
    for dense in (False, True):
        lay = F.layout_long(dense)
        assert lay["sizes"].tolist() == [70000] and not np.isnan(lay["yk"]).any()
        fr = collections.Counter((b["form"], b["why"]) for b in F.forms(lay, "linear", C=1, greeks=False)["frame"])
        # 16-bit ranks: a symbol beyond FR_MAXKNOTS source rows leaves the window form, whatever its spacing
        assert set(fr) == {("perrow", "rows")}, fr
    lay = F.layout_long(False)
    short = {k: (v[:, :60000] if k == "yk" else v[:60000] if k in ("pos",) else v) for k, v in lay.items()}
    short["src_off"] = np.array([0, 60000]); short["sizes"] = np.array([60000]); short["q_off"] = np.array([0, int(short["pos"][-1]) + 4])
    fr = collections.Counter(b["form"] for b in F.forms(short, "linear", C=1, greeks=False)["frame"])
    assert set(fr) == {"window"}, fr                     # the same spacing below the limit: every block on the window form


@pytest.mark.parametrize("method", F.SOLVED)
def test_spline_methods_are_well_conditioned_on_layout_m(method):
    """every knot value moved by one ulp in a random direction moves the oracle's result by less than 1e-13 of the column maximum"""
    lay = F.layout_m()
    ref, st = F.oracle(lay, method)
    r = np.random.default_rng(F.SEED + 5)
    up = r.random(lay["yk"].shape) < 0.5
    moved = np.where(up, np.nextafter(lay["yk"], np.inf), np.nextafter(lay["yk"], -np.inf))
    ref2, st2 = F.oracle(lay, method, yk=moved)
    assert np.array_equal(st, st2) and np.array_equal(np.isnan(ref), np.isnan(ref2))
    for c in range(3):
        shift = np.nanmax(np.abs(ref2[c] - ref[c])) / np.nanmax(np.abs(ref[c]))
        assert shift < 1e-13, (method, c, shift)


def test_polynomial_methods_are_well_conditioned_on_layout_p():
    """'barycentric' and 'krogh' are the same polynomial by two routes; on every series and channel of the layout the oracle's two
    routes agree within the bound the GPU tests compare at (by knot count, of the curve's largest magnitude): what is left for
    the kernels to differ by is theirs"""
    lay = F.layout_p()
    b, _ = F.oracle(lay, "barycentric")
    k, _ = F.oracle(lay, "krogh")
    n, _ = F.knot_counts(lay, "krogh")
    assert np.array_equal(np.isnan(b), np.isnan(k))
    for s in range(len(lay["tags"])):
        sl = slice(int(lay["q_off"][s]), int(lay["q_off"][s + 1]))
        for c in range(3):
            if 0 < n[s, c] <= F.POLY_MAX_KNOTS and np.isfinite(b[c, sl]).any():
                d = np.nanmax(np.abs(b[c, sl] - k[c, sl])) / np.nanmax(np.abs(b[c, sl]))
                assert d <= poly_tol(n[s, c]), (s, lay["tags"][s], c, int(n[s, c]), d)


@pytest.mark.parametrize("name,method", CASES)
def test_oracle_obeys_the_end_rules_and_reproduces_the_knots(name, method):
    lay = LAYOUTS[name][0]()
    ref, st = F.oracle(lay, method)
    n, _ = F.knot_counts(lay, method)
    left_only = method in ("linear", "pad", "cubicspline", "pchip", "barycentric", "krogh")     # NaN left of the first knot only
    for s in range(len(lay["tags"])):
        a, b, qa, qb = lay["src_off"][s], lay["src_off"][s + 1], lay["q_off"][s], lay["q_off"][s + 1]
        rows = np.arange(qb - qa)
        for c in range(3):
            y = lay["yk"][c, a:b]
            xv, yv = lay["pos"][a:b][~np.isnan(y)], y[~np.isnan(y)]
            got = ref[c, qa:qb]
            refused = method in F.POLY and n[s, c] > F.POLY_MAX_KNOTS
            assert st[s, c] == (O.ST_ILL_CONDITIONED if refused else O.ST_TOO_FEW_KNOTS if 0 < n[s, c] < F.MIN_KNOTS[method] else O.ST_OK)
            if n[s, c] == 0 or st[s, c] != O.ST_OK:
                assert np.isnan(got).all(), (s, c)
                continue
            nan = rows > xv[-1] if method == "bfill" else rows < xv[0] if left_only else (rows < xv[0]) | (rows > xv[-1])
            assert np.array_equal(np.isnan(got), nan), (method, s, lay["tags"][s], c)
            scale = np.max(np.abs(yv))
            tol = 0.0 if method in F.EXACT + ("slinear",) else n[s, c] * 2.0 ** n[s, c] * EPS * scale if method == "krogh" else poly_tol(n[s, c]) * scale if method == "barycentric" else 1e-12 * scale
            assert np.max(np.abs(got[xv] - yv)) <= tol, (method, s, lay["tags"][s], c, np.max(np.abs(got[xv] - yv)))
