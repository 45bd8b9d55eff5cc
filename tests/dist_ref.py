"""NumPy restatement of rules P1-P8: the risk-neutral distribution off raw SVI slices.  TEST
INFRASTRUCTURE ONLY: written from the rules, array-wise over all rows, with math.erfc as Phi; it shares no code with the
kernel.  `restate` also returns what the tolerances of the tests are built from (the error scale of every L / U it
compares, the slope of the CDF at every root, the bracket widths) and, with margins=True, asserts the conditions under
which flags and NaN patterns of two arithmetics must be equal."""
import math

import numpy as np

import svi_ref

NO_BRACKET, AMBIGUOUS, TAILS, DEAD = 1, 2, 4, 8
STEPS = 52
DEFAULT_PROBS = (0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99)
DEFAULT_LEVELS = (0.8, 0.9, 1.0, 1.1, 1.2)
_J = np.arange(64) - 31.5
Y = _J * (1.0 + _J * _J / 64.0) / 8.0                      # P4, exact in fp64
_erfc = np.frompyfunc(math.erfc, 1, 1)


def Phi(x):
    return 0.5 * _erfc(-np.asarray(x, np.float64) * 0.70710678118654752440).astype(np.float64)


def phi(x):
    return np.exp(-x * x * 0.5) * 0.39894228040143267794


def terms(P, x):
    """P2 at x (broadcast against the rows of P [..., 5]): dict of w, w1, theta, theta1, d2, L, U, `dens` = dL/dx and
    scale_L / scale_U, the error scale of L and U in units of eps: Phi (1 + d2^2) + phi |theta'| (1 + d2^2) + (|x| / theta) phi
    with Phi = Phi(-d2) for L and Phi(d2) for U."""
    a, b, rho, m, sig = (P[..., q] for q in range(5))
    with np.errstate(all="ignore"):
        dx = x - m
        r = np.sqrt(dx * dx + sig * sig)
        w = a + b * (rho * dx + r)
        w1 = b * (rho + dx / r)
        th = np.sqrt(w)
        th1 = w1 / (2.0 * th)
        d2 = -x / th - 0.5 * th
        pd = phi(d2)
        L, U = Phi(-d2) + pd * th1, Phi(d2) - pd * th1
        g = 1.0 + d2 * d2
        rest = pd * np.abs(th1) * g + np.abs(x) / th * pd
        scale_L, scale_U = Phi(-d2) * g + rest, Phi(d2) * g + rest
        # dL/dx = phi(d2) (theta'' - d2 d2' theta' - d2'), the density in x
        w2 = b * sig * sig / (r * r * r)
        th2 = w2 / (2.0 * th) - w1 * w1 / (4.0 * th * th * th)
        dd2 = -1.0 / th + x * th1 / (th * th) - 0.5 * th1
        dens = pd * (th2 - d2 * dd2 * th1 - dd2)
    return dict(w=w, w1=w1, th=th, th1=th1, d2=d2, L=L, U=U, scale_L=scale_L, scale_U=scale_U, dens=dens)


def h_of(L, U, p):
    """P3."""
    return np.where(p <= 0.5, L - p, (1.0 - p) - U)


def live_rows(P, S, tau):
    """P1."""
    a, b, rho, m, sig = (P[..., q] for q in range(5))
    with np.errstate(all="ignore"):
        ok = np.isfinite(S) & (S > 0) & np.isfinite(tau) & (tau > 0) & np.isfinite(P).all(axis=-1)
        ok &= (b >= 0) & (np.abs(rho) <= 1) & (sig > 0)
        ok &= a + b * sig * np.sqrt(1.0 - rho * rho) > 0
    return ok


def restate(params, Tq, spot, rate=0.0, probs=DEFAULT_PROBS, levels=DEFAULT_LEVELS, max_tail=1e-6, margins=False):
    """Rules P1-P8 on params [B,mT,5], Tq [mT] or [B,mT], spot [B].  Returns the kernel's outputs (q_x, q_strike, q_flags,
    p_below, p_above, tails, flags) and, for the tests: live [B,mT], s0, grid_L / grid_U [B,mT,64], tail_scale [B,mT,2],
    bracket [B,mT,nP] (-1 = none), count, width (of the bracket), q_scale / q_dens (error scale of the target's form and CDF
    slope at the root), below_scale / above_scale [B,mT,nL], forward [B,mT]."""
    P = np.asarray(params, np.float64)
    B, mT, _ = P.shape
    probs, levels = np.asarray(probs, np.float64), np.asarray(levels, np.float64)
    nP, nL = len(probs), len(levels)
    S = np.broadcast_to(np.asarray(spot, np.float64).reshape(B, 1), (B, mT))
    tau = np.broadcast_to(np.asarray(Tq, np.float64), (B, mT))
    live = live_rows(P, S, tau)
    Pl = np.where(live[..., None], P, np.nan)
    with np.errstate(all="ignore"):
        F = S * np.exp(rate * tau)
        s0 = np.sqrt(terms(Pl, 0.0)["w"])                                    # P4
        xg = s0[..., None] * Y
        G = terms(Pl[:, :, None, :], xg)
        h = h_of(G["L"][..., None], G["U"][..., None], probs)                # [B,mT,64,nP]
        cross = (h[:, :, :-1] < 0) & (h[:, :, 1:] >= 0)                      # P5
        count = cross.sum(axis=2)
        first = np.where(count > 0, cross.argmax(axis=2), -1)
        i0 = np.maximum(first, 0)
        lo, hi = s0[..., None] * Y[i0], s0[..., None] * Y[i0 + 1]
        width = hi - lo
        Pt = Pl[:, :, None, :]
        for _ in range(STEPS):                                               # P6
            mid = 0.5 * (lo + hi)
            t = terms(Pt, mid)
            neg = h_of(t["L"], t["U"], probs) < 0
            lo, hi = np.where(neg, mid, lo), np.where(neg, hi, mid)
        xs = 0.5 * (lo + hi)
        found = live[..., None] & (count > 0)
        q_x = np.where(found, xs, np.nan)
        q_strike = np.where(found, F[..., None] * np.exp(xs), np.nan)
        q_flags = np.where(~live[..., None], DEAD, np.where(count == 0, NO_BRACKET, np.where(count > 1, AMBIGUOUS, 0))).astype(np.int32)
        R = terms(Pt, q_x)
        xl = np.log(levels) - (rate * tau)[..., None]                        # P7
        V = terms(Pt, xl)
        tails = np.stack([G["L"][:, :, 0], G["U"][:, :, 63]], axis=-1)       # P8
        flags = np.where(~live, DEAD, np.where((np.abs(tails) > max_tail).any(axis=-1), TAILS, 0)).astype(np.int32)
    out = dict(q_x=q_x, q_strike=q_strike, q_flags=q_flags, p_below=V["L"] if nL else None, p_above=V["U"] if nL else None,
               tails=tails, flags=flags, live=live, s0=s0, grid_L=G["L"], grid_U=G["U"],
               tail_scale=np.stack([G["scale_L"][:, :, 0], G["scale_U"][:, :, 63]], axis=-1),
               bracket=np.where(found, first, -1), count=np.where(live[..., None], count, 0), width=np.where(found, width, np.nan),
               q_scale=np.where(probs <= 0.5, R["scale_L"], R["scale_U"]), q_dens=R["dens"], below_scale=V["scale_L"],
               above_scale=V["scale_U"], forward=F)
    if margins:
        check_margins(out, Pl, probs, max_tail, h)
    return out


def check_margins(r, Pl, probs, max_tail, h):
    """The conditions for generated batches: no comparison of the rules sits on a threshold, and the batch is not mostly
    NaN."""
    live = r["live"]
    assert live.mean() >= 0.9, f"only {live.mean():.0%} of the rows are live"
    assert ((r["count"] > 0)[live]).mean() >= 0.9, "fewer than 90 % of the live rows' targets are bracketed"
    hl = np.abs(h[live])                                                      # [n,64,nP]
    assert (hl >= 1e-9 * np.minimum(probs, 1.0 - probs)).all(), "a grid point sits on a target"
    t = np.abs(r["tails"][live])
    assert ((t >= 10.0 * max_tail) | (t <= 0.1 * max_tail)).all(), "a tail sits on max_tail"
    a, b, rho, m, sig = (Pl[live][..., q] for q in range(5))
    assert (a + b * sig * np.sqrt(1.0 - rho * rho) >= 1e-9 * r["s0"][live] ** 2).all(), "w_min sits on 0"


def call_price(P, x):
    """Undiscounted Black call on a unit forward at strike e^x with the slice's vol: Phi(d1) - e^x Phi(d2)."""
    t = terms(P, x)
    return Phi(t["d2"] + t["th"]) - np.exp(x) * Phi(t["d2"])


class RefBackend(svi_ref.RefBackend):
    """CPU stand-in for snapshots.HipBackend with the distribution restated."""

    def distribution(self, params, Tq, spot, rate, probs, levels, max_tail):
        r = restate(params, Tq, spot, rate, probs, levels, max_tail)
        return {k: r[k] for k in ("q_x", "q_strike", "q_flags", "p_below", "p_above", "tails", "flags")}


def exact(c, ref, dps=50):
    """The same rules in mpmath at `dps` digits on the rows and brackets of `ref` (a restatement of the case `c`): tails,
    p_below, p_above, and q_x / q_strike as the root of h in the restatement's bracket (found by a bracketed secant method to
    1e-40, so the 4 x 2^-52 of the bracket that 52 halvings leave is the tolerance's to cover).  Rounded to fp64 at the end."""
    import mpmath as mp
    with mp.workdps(dps):
        f = mp.mpf
        sqrt2, s2pi = mp.sqrt(2), mp.sqrt(2 * mp.pi)
        Phi_ = lambda z: mp.erfc(-z / sqrt2) / 2                                 # noqa: E731

        def LU(p5, x):
            a, b, rho, m, sig = p5
            dx = x - m
            r = mp.sqrt(dx * dx + sig * sig)
            w = a + b * (rho * dx + r)
            th = mp.sqrt(w)
            th1 = b * (rho + dx / r) / (2 * th)
            d2 = -x / th - th / 2
            t = mp.exp(-d2 * d2 / 2) / s2pi * th1
            return Phi_(-d2) + t, Phi_(d2) - t

        P = np.asarray(c["params"], np.float64)
        B, mT, _ = P.shape
        tau = np.broadcast_to(np.asarray(c["Tq"], np.float64), (B, mT))
        probs, levels = c["probs"], c["levels"]
        out = {k: np.full(np.shape(ref[k]), np.nan) for k in ("q_x", "q_strike", "tails")}
        if len(levels):
            out["p_below"], out["p_above"] = np.full(ref["p_below"].shape, np.nan), np.full(ref["p_below"].shape, np.nan)
        for b in range(B):
            for j in range(mT):
                if not ref["live"][b, j]:
                    continue
                p5 = [f(float(v)) for v in P[b, j]]
                rt = f(c["rate"]) * f(float(tau[b, j]))
                F = f(float(c["spot"][b])) * mp.exp(rt)
                s0 = mp.sqrt(p5[0] + p5[1] * (p5[2] * (0 - p5[3]) + mp.sqrt(p5[3] ** 2 + p5[4] ** 2)))
                out["tails"][b, j] = float(LU(p5, s0 * f(float(Y[0])))[0]), float(LU(p5, s0 * f(float(Y[63])))[1])
                for l, u in enumerate(levels):
                    lo_, up_ = LU(p5, mp.log(f(float(u))) - rt)
                    out["p_below"][b, j, l], out["p_above"][b, j, l] = float(lo_), float(up_)
                for t, p in enumerate(probs):
                    i = int(ref["bracket"][b, j, t])
                    if i < 0:
                        continue
                    pm = f(float(p))
                    h = (lambda x: LU(p5, x)[0] - pm) if p <= 0.5 else (lambda x: (1 - pm) - LU(p5, x)[1])
                    lo, hi = s0 * f(float(Y[i])), s0 * f(float(Y[i + 1]))
                    if not (h(lo) < 0 <= h(hi)):
                        continue                                                     # the bracket is rounding's: not compared
                    x = mp.findroot(h, (lo, hi), solver="anderson", tol=1e-40, maxsteps=200)
                    out["q_x"][b, j, t], out["q_strike"][b, j, t] = float(x), float(F * mp.exp(x))
    return out
