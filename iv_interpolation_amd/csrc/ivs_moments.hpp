// Model-free variance, skew, kurtosis and a constant-maturity vol index off snapshot surfaces (rules
// M1-M7): per row (b, j) of vol [B][mT][mK] the trapezoid over the strikes of g(x) Q / k^2 for the four contracts L, V,
// W, X (Q = the undiscounted out-of-the-money price, x = ln(k / F)), and per snapshot the index 100 sqrt(L_h / h) at each
// horizon h by linear interpolation of L between the bracketing tenors.
//
// A workgroup of four wavefronts owns `spw` whole consecutive snapshots; its spw * mT rows go round its wavefronts.  In a
// row lane = strike, in 64-strike chunks: every lane forms its node (one log, one sqrt, two erfc), finds its next valid
// lane by a bit scan of the validity ballot above it, fetches that node (k, s, x, Q / k^2) by lane permutes and adds the
// trapezoid of the segment between them to its own four sums.  The last valid node of a chunk travels to the next chunk as
// wave-uniform values; there the chunk's last valid lane, which has no next lane of its own, adds the segment from the
// carried node to the chunk's first valid node, so a row longer than 64 strikes and holes at chunk edges need no second
// read.  The one lane whose segment straddles the forward splits it there (M4).  Each sum is reduced once per row by an xor
// butterfly in a fixed order, so a result depends neither on `spw` nor on the wavefront that took the row.  Lane 0 stores
// the row and leaves (L, tau, flags) in the row's LDS slot; after one barrier the first nH threads interpolate the index
// of each of the workgroup's snapshots.  Plain stores only, no atomics, no scratch.
#pragma once
#include "ivs_device.hpp"
#include "ivs_bs_formulas.hpp"

namespace ivs {

constexpr int MM_WAVES = 4;       // wavefronts per workgroup
constexpr int MM_MAX_SPW = 4;     // snapshots per workgroup (with one row per wavefront a workgroup needs no more)
constexpr int MM_MAX_H = 8;       // horizons per call
constexpr int MM_MAX_T = 512;     // tenor rows per snapshot: MM_MAX_SPW * MM_MAX_T row slots stay below 64 KiB of LDS

struct MomParams {
    const double* vol; const double* Kq; const double* Tq; const double* spot;
    int64_t kq_stride, tq_stride;                        // 0 = shared
    double rate, min_mass;
    double h[MM_MAX_H];
    int32_t mK, mT, nH, spw;
    int64_t B;
    double* raw; double* stats; double* mass; int32_t* flags;   // [B][mT][4] x 2, [B][mT] x 2
    double* index; int32_t* index_flags;                        // [B][nH]
};

struct MomSlot { double L, tau; int32_t flags, pad; };
struct MomNode { double k, s, x, q; };                   // strike, vol, x = ln(k / F), q = Q / k^2

__device__ __forceinline__ MomNode mm_from_lane(const MomNode& n, int src) {
    return MomNode{__shfl(n.k, src), __shfl(n.s, src), __shfl(n.x, src), __shfl(n.q, src)};
}

// M5: the four integrands at a node
__device__ __forceinline__ void mm_f(const MomNode& n, double f[4]) {
    const double x2 = n.x * n.x;
    f[0] = 2.0 * n.q;
    f[1] = 2.0 * (1.0 - n.x) * n.q;
    f[2] = (6.0 * n.x - 3.0 * x2) * n.q;
    f[3] = (12.0 * x2 - 4.0 * (x2 * n.x)) * n.q;
}

// M4 / M5: the trapezoids of the segment a -> b, split at the forward where it lies strictly inside, added to acc
__device__ __forceinline__ void mm_segment(const MomNode& a, const MomNode& b, double F, double tau, double acc[4]) {
    double fa[4], fb[4];
    mm_f(a, fa);
    mm_f(b, fb);
    if (a.k < F && F < b.k) {
        const double sF = a.s + (b.s - a.s) * (F - a.k) / (b.k - a.k);
        const double QF = F * erf(sqrt(sF * sF * tau) * 0.35355339059327376220);   // put = call at x = 0
        const double qF = QF / (F * F);
        const double fF[4] = {2.0 * qF, 2.0 * qF, 0.0, 0.0};
        for (int m = 0; m < 4; ++m)
            acc[m] += 0.5 * (fa[m] + fF[m]) * (F - a.k) + 0.5 * (fF[m] + fb[m]) * (b.k - F);
    } else {
        for (int m = 0; m < 4; ++m) acc[m] += 0.5 * (fa[m] + fb[m]) * (b.k - a.k);
    }
}

__global__ __launch_bounds__(MM_WAVES * 64) void surface_moments_kernel(MomParams p) {
    extern __shared__ __align__(16) unsigned char mm_lds[];
    MomSlot* slot = reinterpret_cast<MomSlot*>(mm_lds);                  // [spw][mT]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t b0 = (int64_t)blockIdx.x * p.spw;
    const int nsnap = (int)((p.B - b0) < p.spw ? (p.B - b0) : p.spw);
    const int nrow = nsnap * p.mT;

    for (int r = wave; r < nrow; r += MM_WAVES) {
        const int ls = r / p.mT, j = r - ls * p.mT;
        const int64_t b = b0 + ls;
        const int64_t row = b * p.mT + j;
        const double S = p.spot[b], tau = p.Tq[b * p.tq_stride + j];
        const bool live = finite_pos(S) && finite_pos(tau);              // M1; uniform over the wavefront
        const double rt = p.rate * tau;
        const double F = S * exp(rt);                                    // M2
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        bool bad = false;                                                // a segment whose strikes do not ascend
        int nvalid = 0, ifirst = -1, ilast = -1;
        MomNode first{qnan(), qnan(), qnan(), qnan()}, carry = first;    // first / last valid node so far (uniform)
        if (live) {
            const double* kr = p.Kq + b * p.kq_stride;
            const double* vr = p.vol + row * p.mK;
            for (int c0 = 0; c0 < p.mK; c0 += 64) {
                const int i = c0 + lane;
                const bool in = i < p.mK;
                const double k = in ? kr[i] : qnan(), s = in ? vr[i] : qnan();
                const bool valid = finite_pos(k) && finite_pos(s);
                // M2, M3
                const double x = log(k / S) - rt;
                const double sq = sqrt(s * s * tau);
                const double d2 = -x / sq - 0.5 * sq, d1 = d2 + sq;
                const bool put = k < F;
                const double P2 = norm_cdf(put ? -d2 : d2), P1 = norm_cdf(put ? -d1 : d1);
                const double Q = put ? k * P2 - F * P1 : F * P1 - k * P2;
                const MomNode me{k, s, x, Q / (k * k)};
                // the segment to the next valid lane of this chunk; the chunk's last valid lane has none here (its segment
                // ends in a later chunk), so it takes the one from the chunks before: carry -> the chunk's first valid lane
                const unsigned long long vm = __ballot(valid);
                const unsigned long long above = vm & ~((2ull << lane) - 1ull);
                const int f = vm ? __builtin_ctzll(vm) : 0, l = vm ? 63 - __builtin_clzll(vm) : 0;   // uniform
                const bool inner = valid && above != 0ull, from_carry = valid && above == 0ull && nvalid > 0;
                const MomNode other = mm_from_lane(me, above ? __builtin_ctzll(above) : f);
                if (inner || from_carry) {
                    const MomNode a = inner ? me : carry;
                    bad = bad || !(other.k > a.k);
                    mm_segment(a, other, F, tau, acc);
                }
                if (vm) {                                                // uniform
                    if (nvalid == 0) {
                        first = mm_from_lane(me, f);
                        ifirst = c0 + f;
                    }
                    carry = mm_from_lane(me, l);
                    ilast = c0 + l;
                    nvalid += __popcll(vm);
                }
            }
        }
        for (int m = 0; m < 4; ++m)                                      // fixed order: the same bits in every lane
            for (int d = 32; d > 0; d >>= 1) acc[m] += __shfl_xor(acc[m], d);
        bool dead = !live || nvalid < 2 || __ballot(bad) != 0ull;        // M1
        // M6
        const double L = acc[0], V = acc[1], W = acc[2], X = acc[3];
        const double mu = -V / 2.0 - W / 6.0 - X / 24.0;
        const double var = V - mu * mu;
        dead = dead || !(L > 0.0 && var > 0.0);
        const double sqf = sqrt(first.s * first.s * tau), sql = sqrt(carry.s * carry.s * tau);
        const double d2f = -first.x / sqf - 0.5 * sqf, d2l = -carry.x / sql - 0.5 * sql;
        const double tails = norm_cdf(lane == 0 ? -d2f : d2l);            // lane 0: below the first strike, lane 1: above the last
        const double mass = 1.0 - __shfl(tails, 0) - __shfl(tails, 1);
        int32_t fl = IVS_MM_DEAD;
        if (!dead)
            fl = ((F < first.k || F > carry.k) ? IVS_MM_ONE_SIDED : 0) | (mass < p.min_mass ? IVS_MM_TRUNCATED : 0) |
                 (ilast - ifirst + 1 > nvalid ? IVS_MM_HOLES : 0);
        if (lane == 0) {
            const double mu2 = mu * mu;
            double* raw = p.raw + row * 4;
            double* st = p.stats + row * 4;
            raw[0] = dead ? qnan() : L; raw[1] = dead ? qnan() : V; raw[2] = dead ? qnan() : W; raw[3] = dead ? qnan() : X;
            st[0] = dead ? qnan() : sqrt(L / tau);
            st[1] = dead ? qnan() : sqrt(var / tau);
            st[2] = dead ? qnan() : (W - 3.0 * mu * V + 2.0 * (mu2 * mu)) / (var * sqrt(var));
            st[3] = dead ? qnan() : (X - 4.0 * mu * W + 6.0 * mu2 * V - 3.0 * (mu2 * mu2)) / (var * var);
            p.mass[row] = dead ? qnan() : mass;
            p.flags[row] = fl;
            slot[r] = MomSlot{dead ? qnan() : L, tau, fl, 0};
        }
    }
    __syncthreads();
    // M7: thread t takes horizon t of each of the workgroup's snapshots
    if ((int)threadIdx.x < p.nH) {
        double h = 0.0;
        for (int t = 0; t < MM_MAX_H; ++t)
            if ((int)threadIdx.x == t) h = p.h[t];
        for (int ls = 0; ls < nsnap; ++ls) {
            const MomSlot* rows = slot + ls * p.mT;
            double ix = qnan(), Lp = 0.0, tp = 0.0;
            int32_t fx = IVS_MM_NO_BRACKET, fp = 0;
            bool have = false, found = false;
            for (int j = 0; j < p.mT && !found; ++j) {
                const MomSlot c = rows[j];
                if (c.flags & IVS_MM_DEAD) continue;
                if (have && tp <= h && h <= c.tau && tp < c.tau) {
                    const double Lh = Lp + (c.L - Lp) * (h - tp) / (c.tau - tp);
                    ix = 100.0 * sqrt(Lh / h);
                    fx = fp | c.flags;
                    found = true;
                }
                Lp = c.L; tp = c.tau; fp = c.flags; have = true;
            }
            const int64_t o = (b0 + ls) * p.nH + threadIdx.x;
            p.index[o] = ix;
            p.index_flags[o] = fx;
        }
    }
}

}  // namespace ivs
