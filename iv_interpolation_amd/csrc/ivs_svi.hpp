// Raw SVI slices off snapshot surfaces with a butterfly check (rules V1-V8): per row (b, j) of vol
// [B][mT][mK] the five parameters (a, b, rho, m, sigma) of w(x) = a + b (rho (x - m) + sqrt((x - m)^2 + sigma^2)) that fit
// the total variances w = s^2 tau at x = ln(k / S) - rate tau of the valid nodes in unweighted least squares, the fit's
// statistics, Durrleman's g on the fitted curve and, optionally, the fitted vol at every strike.
//
// One wavefront per row, `rpw` rows per workgroup of four wavefronts.  In the first phase lane = strike, in 64-strike chunks
// read coalesced: the valid (x, w) pairs are compacted in strike order into the wavefront's LDS slot (ballot and prefix
// popcount); the last valid strike travels to the next chunk as a wave-uniform value for the ascending check.  Then, for a
// fixed number of rounds, lane = candidate: lane 8 i_u + i_m holds the grid point (m, ln sigma) of an 8 x 8 grid on the current
// box, accumulates the six sums of rule V4 over the nodes (every lane reads the same LDS address: a broadcast), solves the 27
// active sets of the inner problem in registers (one loop over the set number, the states of (a, p, q) being wave-uniform),
// sums the winner's residuals in node order and enters a fixed xor butterfly over (SSE, lane).  The winner's grid point and
// the next box are wave-uniform.  After the last round lane = strike again for the statistics and the fitted vols; lane 0
// stores params, fit and flags.  Every loop is bounded by mK, `rounds` or a constant; plain loads and stores, no atomics.
// A result depends neither on `rpw` nor on the wavefront that took the row.
#pragma once
#include "ivs_device.hpp"

namespace ivs {

constexpr int SV_WAVES = 4;          // wavefronts per workgroup
constexpr int SV_MAX_K = 1024;       // nodes per row: 4 slots of 16 B x 1024 fill the 64 KiB a workgroup may ask for
constexpr int SV_MAX_ROUNDS = 24;
constexpr int SV_DEFAULT_ROUNDS = 16;
constexpr double SV_EDGE_BAND = 0x1p-20;   // EDGE: within this share of the domain's width of a border

struct SviParams {
    const double* vol; const double* Kq; const double* Tq; const double* spot;
    int64_t kq_stride, tq_stride;                        // 0 = shared
    double rate;
    int32_t mK, mT, rounds, rpw;
    int64_t rows;                                        // B * mT
    double* params; double* fit; int32_t* flags; double* fitted;   // [rows][5], [rows][4], [rows], [rows][mK] or null
};

// V4: set s = 9 ia + icd; the states of p = (c - d) / 2 and q = (c + d) / 2 (0 free, 1 at 0, 2 at sigma) of icd = interior,
// d = c, d = -c, c + d = 2 sigma, c - d = 2 sigma, (0, 0), (sigma, sigma), (2 sigma, 0), (sigma, -sigma), two bits each
constexpr uint32_t SV_P_STATES = 0u | 1u << 2 | 0u << 4 | 0u << 6 | 2u << 8 | 1u << 10 | 1u << 12 | 2u << 14 | 2u << 16;
constexpr uint32_t SV_Q_STATES = 0u | 0u << 2 | 1u << 4 | 2u << 6 | 0u << 8 | 1u << 10 | 2u << 12 | 2u << 14 | 1u << 16;

struct SviSums { double Sy, Sz, Syy, Syz, Swy, Swz; };
struct SviInner { double a, p, q, sse; int set; };

// V4 for this lane's candidate (m, sigma) on the n nodes of the wavefront's slot
__device__ __forceinline__ SviInner sv_inner(const double2* nodes, int n, double Sw, double wmax, double m, double sigma) {
    const double inv = 1.0 / sigma;
    SviSums t{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < n; ++i) {                                        // node order
        const double2 xw = nodes[i];
        const double y = (xw.x - m) * inv;
        const double z = sqrt(y * y + 1.0);
        t.Sy += y; t.Sz += z; t.Syy += y * y; t.Syz += y * z; t.Swy += xw.y * y; t.Swz += xw.y * z;
    }
    // the Gram matrix of (1, y, z) in the basis (1, z - y, z + y) of (a, p, q); z^2 - y^2 = 1
    const double nn = (double)n;
    const double H01 = t.Sz - t.Sy, H02 = t.Sz + t.Sy;
    const double H11 = (2.0 * t.Syy + nn) - 2.0 * t.Syz, H22 = (2.0 * t.Syy + nn) + 2.0 * t.Syz;
    const double g1 = t.Swz - t.Swy, g2 = t.Swz + t.Swy;
    double ua = 0.0, up = 0.0, uq = 0.0;                                 // the unconstrained solution (set 0)
    double best = __builtin_inf();
    SviInner r{Sw / nn, 0.0, 0.0, 0.0, 5};                               // the fallback: set 5, the flat line
#pragma nounroll
    for (int s = 0; s < 27; ++s) {                                       // s is wave-uniform
        const int ia = s / 9, icd = s - 9 * ia;
        const int sp = (int)((SV_P_STATES >> (2 * icd)) & 3u), sq = (int)((SV_Q_STATES >> (2 * icd)) & 3u);
        const bool fa = ia != 0, fp = sp != 0, fq = sq != 0;
        const double va = ia == 2 ? wmax : 0.0, vp = sp == 2 ? sigma : 0.0, vq = sq == 2 ? sigma : 0.0;
        // a fixed variable's row and column become the unit row, its right-hand side the bound
        const double A00 = fa ? 1.0 : nn, A11 = fp ? 1.0 : H11, A22 = fq ? 1.0 : H22;
        const double A01 = (fa || fp) ? 0.0 : H01, A02 = (fa || fq) ? 0.0 : H02, A12 = (fp || fq) ? 0.0 : nn;
        const double b0 = fa ? va : Sw - (fp ? H01 * vp : 0.0) - (fq ? H02 * vq : 0.0);
        const double b1 = fp ? vp : g1 - (fa ? H01 * va : 0.0) - (fq ? nn * vq : 0.0);
        const double b2 = fq ? vq : g2 - (fa ? H02 * va : 0.0) - (fp ? nn * vp : 0.0);
        // LDL^T in the order a, p, q
        const double l10 = A01 / A00, l20 = A02 / A00;
        const double d1 = A11 - l10 * A01;
        const double t21 = A12 - l20 * A01;
        const double l21 = t21 / d1;
        const double d2 = A22 - l20 * A02 - l21 * t21;
        const double y1 = b1 - l10 * b0;
        const double y2 = b2 - l20 * b0 - l21 * y1;
        double tq = y2 / d2;
        double tp = y1 / d1 - l21 * tq;
        double ta = b0 / A00 - l10 * tp - l20 * tq;
        ta = fa ? va : ta; tp = fp ? vp : tp; tq = fq ? vq : tq;
        if (s == 0) { ua = ta; up = tp; uq = tq; }
        const bool feasible = (fa || (ta >= 0.0 && ta <= wmax)) && (fp || (tp >= 0.0 && tp <= sigma)) &&
                              (fq || (tq >= 0.0 && tq <= sigma));
        const double da = ta - ua, dp = tp - up, dq = tq - uq;
        const double E = nn * da * da + H11 * dp * dp + H22 * dq * dq + 2.0 * (H01 * da * dp + H02 * da * dq + nn * dp * dq);
        if (feasible && E < best) {
            best = E;
            r.a = ta; r.p = tp; r.q = tq; r.set = s;
        }
    }
    const double c = r.p + r.q, d = r.q - r.p;
    double sse = 0.0;
    for (int i = 0; i < n; ++i) {                                        // node order
        const double2 xw = nodes[i];
        const double y = (xw.x - m) * inv;
        const double z = sqrt(y * y + 1.0);
        const double res = r.a + d * y + c * z - xw.y;
        sse += res * res;
    }
    r.sse = sse;
    return r;
}

__global__ __launch_bounds__(SV_WAVES * 64) void svi_slice_kernel(SviParams p) {
    extern __shared__ __align__(16) unsigned char sv_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    double2* nodes = reinterpret_cast<double2*>(sv_lds) + (size_t)wave * p.mK;   // this wavefront's slot: (x, w) [mK]
    const int64_t row = (int64_t)blockIdx.x * p.rpw + wave;
    const bool mine = wave < p.rpw && row < p.rows;                      // uniform over the wavefront
    const int64_t b = mine ? row / p.mT : 0;
    const int j = mine ? (int)(row - b * p.mT) : 0;
    const double S = mine ? p.spot[b] : qnan(), tau = mine ? p.Tq[b * p.tq_stride + j] : qnan();
    const bool live = mine && finite_pos(S) && finite_pos(tau);          // V1
    const double rt = p.rate * tau;
    const double* kr = p.Kq + b * p.kq_stride;
    const double* vr = p.vol + (mine ? row : 0) * p.mK;

    // ---- lane = strike: V1 / V2, the valid (x, w) in strike order into the slot
    int n = 0, ifirst = -1, ilast = -1;
    bool bad = false;
    double klast = 0.0;                                                  // the last valid strike so far (uniform)
    if (live) {
        for (int c0 = 0; c0 < p.mK; c0 += 64) {
            const int i = c0 + lane;
            const bool in = i < p.mK;
            const double k = in ? kr[i] : qnan(), s = in ? vr[i] : qnan();
            const bool valid = finite_pos(k) && finite_pos(s);
            const unsigned long long vm = __ballot(valid);
            const unsigned long long above = vm & ~((2ull << lane) - 1ull);
            const double knext = __shfl(k, above ? __builtin_ctzll(above) : lane);
            bad = bad || (valid && above != 0ull && !(knext > k));
            if (vm) {                                                    // uniform
                const int f = __builtin_ctzll(vm), l = 63 - __builtin_clzll(vm);
                const double kf = __shfl(k, f);
                bad = bad || (n > 0 && !(kf > klast));
                klast = __shfl(k, l);
                if (n == 0) ifirst = c0 + f;
                ilast = c0 + l;
            }
            if (valid) {
                const int at = n + __popcll(vm & ((1ull << lane) - 1ull));   // at < mK: one slot entry per valid node
                nodes[at] = double2{log(k / S) - rt, s * s * tau};
            }
            n += __popcll(vm);
        }
    }
    __syncthreads();                                                     // every wavefront of the workgroup gets here
    const bool dead = !live || n < 5 || __ballot(bad) != 0ull;           // V1; uniform

    double ra = qnan(), rp = qnan(), rq = qnan(), rm = qnan(), ru = qnan(), rsig = qnan(), rsse = qnan();
    int rset = 0;
    int32_t fl = IVS_SV_DEAD;
    if (!dead) {
        // ---- lane = candidate: V4 / V5
        double Sw = 0.0, wmax = 0.0;
        for (int i = 0; i < n; ++i) {                                    // node order, the same in every lane
            const double w = nodes[i].y;
            Sw += w;
            wmax = w > wmax ? w : wmax;
        }
        const double x0 = nodes[0].x, x1 = nodes[n - 1].x, X = x1 - x0;
        const double u0 = log(X / 256.0), u1 = log(4.0 * X);
        double mlo = x0, mhi = x1, ulo = u0, uhi = u1;
        const int im = lane & 7, iu = lane >> 3;
        for (int round = 0; round < p.rounds; ++round) {
            const double hm = (mhi - mlo) / 7.0, hu = (uhi - ulo) / 7.0;
            const double m = im == 7 ? mhi : mlo + im * hm;
            const double u = iu == 7 ? uhi : ulo + iu * hu;
            const double sigma = exp(u);
            const SviInner r = sv_inner(nodes, n, Sw, wmax, m, sigma);
            // the smallest SSE, the lowest lane among equals; a NaN never wins
            double best = r.sse == r.sse ? r.sse : __builtin_inf();
            int who = lane;
            for (int d = 32; d > 0; d >>= 1) {
                const double ob = __shfl_xor(best, d);
                const int ow = __shfl_xor(who, d);
                const bool take = ob < best || (ob == best && ow < who);
                best = take ? ob : best;
                who = take ? ow : who;
            }
            who = __builtin_amdgcn_readfirstlane(who);
            rm = __shfl(m, who); ru = __shfl(u, who);
            if (round == p.rounds - 1) {
                ra = __shfl(r.a, who); rp = __shfl(r.p, who); rq = __shfl(r.q, who); rsse = __shfl(r.sse, who);
                rsig = __shfl(sigma, who); rset = __shfl(r.set, who);
            }
            mlo = rm - hm > x0 ? rm - hm : x0; mhi = rm + hm < x1 ? rm + hm : x1;
            ulo = ru - hu > u0 ? ru - hu : u0; uhi = ru + hu < u1 ? ru + hu : u1;
        }
        // V6: on the border, or within 2^-20 of the domain's width of it (what the last rounds' ties can move is far less)
        const double tm = X * SV_EDGE_BAND, tu = (u1 - u0) * SV_EDGE_BAND;
        fl = (ilast - ifirst + 1 > n ? IVS_SV_HOLES : 0) | (rset != 0 ? IVS_SV_BOUND : 0) |
             ((rm - x0 <= tm || x1 - rm <= tm || ru - u0 <= tu || u1 - ru <= tu) ? IVS_SV_EDGE : 0);
    }
    // V6
    const double rc = rp + rq, rd = rq - rp;
    const double pb = rc / rsig, prho = rc != 0.0 ? rd / rc : 0.0;

    // ---- lane = strike: V7 / V8
    double se2 = 0.0, emax = 0.0, gmin = __builtin_inf();
    bool degenerate = false;
    if (mine) {
        double* fr = p.fitted ? p.fitted + row * p.mK : nullptr;
        for (int c0 = 0; c0 < p.mK; c0 += 64) {
            const int i = c0 + lane;
            if (i >= p.mK) continue;
            if (dead) {
                if (fr) fr[i] = qnan();
                continue;
            }
            const double k = kr[i], s = vr[i];
            const bool kpos = finite_pos(k);
            const double x = log(k / S) - rt;
            const double dx = x - rm;
            const double r = sqrt(dx * dx + rsig * rsig);
            const double wf = ra + pb * (prho * dx + r);
            const double vf = sqrt((wf > 0.0 ? wf : 0.0) / tau);
            if (fr) fr[i] = kpos ? vf : qnan();
            if (kpos && finite_pos(s)) {
                const double e = vf - s;
                se2 += e * e;
                emax = __builtin_fabs(e) > emax ? __builtin_fabs(e) : emax;
                const double w1 = pb * (prho + dx / r);
                const double w2 = pb * rsig * rsig / (r * r * r);
                const double t = 1.0 - x * w1 / (2.0 * wf);
                const double g = t * t - (w1 * w1 / 4.0) * (1.0 / wf + 0.25) + w2 / 2.0;
                gmin = g < gmin ? g : gmin;
                degenerate = degenerate || wf <= 0.0;
            }
        }
    }
    for (int d = 32; d > 0; d >>= 1) {                                   // fixed order: the same bits in every lane
        se2 += __shfl_xor(se2, d);
        const double oe = __shfl_xor(emax, d), og = __shfl_xor(gmin, d);
        emax = oe > emax ? oe : emax;
        gmin = og < gmin ? og : gmin;
    }
    const bool deg = __ballot(degenerate) != 0ull;
    if (mine && lane == 0) {
        double* pr = p.params + row * 5;
        double* ft = p.fit + row * 4;
        if (dead) {
            for (int t = 0; t < 5; ++t) pr[t] = qnan();
            for (int t = 0; t < 4; ++t) ft[t] = qnan();
        } else {
            if (deg) { gmin = qnan(); fl |= IVS_SV_DEGENERATE; }
            if (gmin < 0.0) fl |= IVS_SV_BUTTERFLY;
            pr[0] = ra; pr[1] = pb; pr[2] = prho; pr[3] = rm; pr[4] = rsig;
            ft[0] = sqrt(rsse / (double)n); ft[1] = sqrt(se2 / (double)n); ft[2] = emax; ft[3] = gmin;
        }
        p.flags[row] = fl;
    }
}

}  // namespace ivs
