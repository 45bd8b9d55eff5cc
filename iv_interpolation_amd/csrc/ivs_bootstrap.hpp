// Bootstrap standard errors and intervals for a book's VaR and expected shortfall (rules C0-C9): how far
// the order statistics of section 19 move when the row of scenario P&Ls is resampled, by a circular block bootstrap over the
// ranked scenarios in time order.  The call works on rows alone (pnl, scen_flags as a section 19 call wrote them).
//
// hsim_bootstrap_kernel: a workgroup of four wavefronts owns one row.  It stages the row in LDS and ranks it by counting ONCE, as
// hsim_tail_kernel does (C1 is H7, restated here: hsim_tail_kernel stays the code it is), and leaves v[rank] and the rank of
// every time position in LDS.  A replicate's VaR and ES depend only on how often each rank was drawn, so nothing is sorted
// again: the replicates are dealt to the wavefronts (r = wave, wave + 4, ...), and a wavefront clears its own histogram of
// counts, draws (lanes enumerate the n draws; a block's start is hashed once per block into LDS when the blocks are longer than
// one draw), adds into the histogram with integer LDS adds (their result does not depend on their order) and walks the counts
// upward, one lane per level, as hsim_tail_kernel walks its sorted row (C5).  The replicate values go to global memory once
// (rep or the workspace); after a barrier the same workgroup reads them back series by series (statistic x level) and forms the
// summaries of C6: the sums through rk_wave_sum / rk_four (B5), the quantiles by a bitonic sort of the series in LDS.
//
// Contraction is off throughout (B4).  No floating-point atomics.
#pragma once
#include "ivs_hsim.hpp"

namespace ivs {

constexpr int BT_MAX_REP = 1024;       // replicates per row: four passes of C6, a series fits the LDS of the row
constexpr int BT_MAX_BLOCK = 1024;
constexpr int BT_MAX_CI = 8;           // the interval probabilities travel in the kernel's arguments

struct BootParams {
    const double* pnl; const int32_t* scen_flags;        // [B][window]
    int32_t window, nL, min_scen, R, L, nC;
    uint64_t seed;
    double tp[HS_MAX_LEVELS];
    double ci[BT_MAX_CI];
    double* var0; double* es0; int32_t* n_scen;          // [B][nL], [B]
    double* mean; double* variance;                      // [B][2][nL]
    double* quant;                                       // [B][2][nL][nC]
    double* rep;                                         // [B][R][2][nL]: the caller's, or the workspace
};

// C3: the upper word of a splitmix64 finaliser at the counter (r, i)
__device__ __forceinline__ uint32_t bt_word(uint64_t seed, uint32_t r, uint32_t i) {
    const uint64_t c = ((uint64_t)r << 32) | i;
    uint64_t z = seed + (c + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (uint32_t)(z >> 32);
}

// what one wavefront wrote to its own LDS is read by its other lanes: the LDS serves a wavefront's instructions in order, so
// only the compiler has to keep them in place
__device__ __forceinline__ void bt_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// B5 over the replicates: x[ps] is this thread's term of pass ps (r = 256 ps + tid, +0.0 for a missing r).  Every thread returns
// the sum.  Two barriers per pass.
__device__ __forceinline__ double bt_sum(const double (&x)[4], int R, double* part, int wave, int lane) {
#pragma clang fp contract(off)
    double S = 0.0;
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
        if (ps * RK_BLOCK < R) {
            const double w = rk_wave_sum(x[ps]);
            if (lane == 0) part[wave] = w;
            __syncthreads();
            S = S + rk_four([&](int k) { return part[k]; });
            __syncthreads();
        }
    }
    return S;
}

__global__ __launch_bounds__(RK_BLOCK) void hsim_bootstrap_kernel(BootParams p) {
#pragma clang fp contract(off)
    __shared__ double row[HS_MAX_WINDOW];                                // the row, NaN where not ranked; then the block starts; then a series
    __shared__ __attribute__((aligned(16))) double val[HS_MAX_WINDOW];   // v[rank]
    __shared__ uint16_t rho[HS_MAX_WINDOW];                              // the rank of time position k
    __shared__ __attribute__((aligned(16))) uint32_t hist[RK_WAVES][HS_MAX_WINDOW];      // per wavefront: how often each rank was drawn
    __shared__ int32_t cnt[RK_WAVES];
    __shared__ int32_t notfin[RK_WAVES];
    __shared__ double part[RK_WAVES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t b = blockIdx.x;
    const int W = p.window, R = p.R, nL = p.nL, nq = 2 * p.nL;

    // C1: H7's ranked set and order
    int32_t mine = 0;
    bool wild = false;
    for (int s = tid; s - tid < W; s += RK_BLOCK) {                      // whole wavefronts go round together
        const bool in = s < W;
        const double v = in ? p.pnl[b * W + s] : qnan();
        const bool ok = in && p.scen_flags[b * W + s] == 0 && v == v;
        if (in) row[s] = ok ? v : qnan();
        mine += __popcll(__ballot(ok));
        wild = wild || (ok && !(fabs(v) < __builtin_inf()));
    }
    const bool wild_any = __ballot(wild) != 0ull;
    if (lane == 0) { cnt[wave] = mine; notfin[wave] = wild_any ? 1 : 0; }
    __syncthreads();
    const int n = cnt[0] + cnt[1] + cnt[2] + cnt[3];
    const bool finite = (notfin[0] | notfin[1] | notfin[2] | notfin[3]) == 0;
    for (int s = tid; s < W; s += RK_BLOCK) {
        const double v = row[s];
        if (!(v == v)) continue;
        int r = 0, k = 0;
        for (int i = 0; i < W; ++i) {                                    // uniform LDS addresses; -0.0 == +0.0: the lower s first
            const double w = row[i];
            r += (w < v || (w == v && i < s)) ? 1 : 0;
            k += (w == w && i < s) ? 1 : 0;
        }
        val[r] = v;
        rho[k] = (uint16_t)r;
    }
    __syncthreads();
    if (tid == 0) p.n_scen[b] = n;
    int m_l = 0;                                                         // H7's tail of this lane's level
    for (int l = 0; l < nL; ++l) {
        int m = (int)floor((double)n * p.tp[l]);
        m = m < 1 ? 1 : m;
        if (lane == l) m_l = m;
    }
    if (tid < nL) {                                                      // var0, es0: H7 on the row itself
        double var = qnan(), es = qnan();
        if (n >= p.min_scen && n > 0) {
            double sum = 0.0;
            for (int i = 0; i < m_l; ++i) sum = sum + val[i];
            var = 0.0 - val[m_l - 1];
            es = 0.0 - sum / (double)m_l;
        }
        p.var0[b * nL + tid] = var;
        p.es0[b * nL + tid] = es;
    }
    if (nL == 0) return;
    const int64_t rep0 = b * R * nq;                                     // < 2^31 elements in all
    if (!(n >= p.min_scen && n > 0 && finite)) {                         // C2: not active
        for (int i = tid; i < R * nq; i += RK_BLOCK) p.rep[rep0 + i] = qnan();
        for (int i = tid; i < nq; i += RK_BLOCK) { p.mean[b * nq + i] = qnan(); p.variance[b * nq + i] = qnan(); }
        for (int i = tid; i < nq * p.nC; i += RK_BLOCK) p.quant[b * nq * p.nC + i] = qnan();
        return;
    }

    // C3-C5: the replicates of this wavefront
    {
        const int Lp = p.L < n ? p.L : n;                                // >= 1
        const int nb = (n + Lp - 1) / Lp;
        const uint32_t inv = (1u << 20) / (uint32_t)Lp + 1u;             // d / Lp = (d inv) >> 20 for d < 1024
        uint16_t* bs = reinterpret_cast<uint16_t*>(row) + wave * HS_MAX_WINDOW;
        uint32_t* h = hist[wave];
        for (int r = wave; r < R; r += RK_WAVES) {
            for (int i = 4 * lane; i < n; i += 256) *reinterpret_cast<uint4*>(h + i) = make_uint4(0u, 0u, 0u, 0u);      // to a multiple of four: the walk reads fours
            if (Lp > 1)
                for (int i = lane; i < nb; i += 64) bs[i] = (uint16_t)__umulhi(bt_word(p.seed, (uint32_t)r, (uint32_t)i), (uint32_t)n);
            bt_wave_sync();
            for (int d = lane; d < n; d += 64) {                         // C4: draw d is element d - i Lp of block i
                int pos;
                if (Lp == 1) {
                    pos = (int)__umulhi(bt_word(p.seed, (uint32_t)r, (uint32_t)d), (uint32_t)n);
                } else {
                    const int i = (int)(((uint32_t)d * inv) >> 20);
                    pos = (int)bs[i] + (d - i * Lp);                     // < 2 n
                    pos -= pos >= n ? n : 0;
                }
                __hip_atomic_fetch_add(&h[rho[pos]], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            bt_wave_sync();
            if (lane < nL) {                                             // C5: the walk up the ranks, lane = level
                // four ranks per LDS round trip, and no branch: a rank that gives nothing (not drawn, or past m_l) adds +0.0, which
                // changes no bit of a sum that began at +0.0 (such a sum is never -0.0)
                double sum = 0.0, last = 0.0;
                int taken = 0;
                auto step = [&](uint32_t c, double v) {
                    const int left = m_l - taken;
                    const int k = (int)c < left ? (int)c : left;         // >= 0
                    sum = sum + (k > 0 ? (double)k * v : 0.0);
                    taken += k;
                    last = k > 0 ? v : last;
                };
                for (int q = 0; q < n && taken < m_l; q += 4) {
                    const uint4 c = *reinterpret_cast<const uint4*>(h + q);
                    const double2 va = *reinterpret_cast<const double2*>(val + q), vb = *reinterpret_cast<const double2*>(val + q + 2);
                    step(c.x, va.x); step(c.y, va.y); step(c.z, vb.x); step(c.w, vb.y);
                }
                const int64_t at = rep0 + (int64_t)r * nq + lane;
                p.rep[at] = 0.0 - last;
                p.rep[at + nL] = 0.0 - sum / (double)m_l;
            }
            bt_wave_sync();                                              // the walk's reads before the next replicate's clearing
        }
    }
    __syncthreads();                                                     // the replicate values of all four wavefronts are visible

    // C6: series q = statistic x level; thread t holds x_r for r = t, t + 256, ...
    int N = 1;                                                           // the series' length rounded up to a power of two, <= 1024
    while (N < R) N <<= 1;
    for (int q = 0; q < nq; ++q) {
        double x[4];
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
            const int r = ps * RK_BLOCK + tid;
            x[ps] = r < R ? p.rep[rep0 + (int64_t)r * nq + q] : 0.0;
            if (r < R) row[r] = x[ps];
        }
        const double mean = bt_sum(x, R, part, wave, lane) / (double)R;  // its barriers also publish the series in LDS
        double d2[4];
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
            const double d = x[ps] - mean;
            d2[ps] = ps * RK_BLOCK + tid < R ? d * d : 0.0;
        }
        const double ss = bt_sum(d2, R, part, wave, lane);
        if (tid == 0) {
            p.mean[b * nq + q] = mean;
            p.variance[b * nq + q] = R > 1 ? ss / (double)(R - 1) : qnan();
        }
        if (p.nC > 0) {
            // a bitonic sort of the series in LDS, padded with +inf to N, a power of two: log2 N (log2 N + 1) / 2 stages of N / 2
            // compare-exchanges, one barrier each.  The replicate values are never -0.0, so equal values are equal bits and the
            // order among them cannot show.
            for (int j = R + tid; j < N; j += RK_BLOCK) row[j] = __builtin_inf();
            __syncthreads();
            for (int k = 2; k <= N; k <<= 1) {
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int t = tid; t < (N >> 1); t += RK_BLOCK) {
                        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;       // < N
                        const double u = row[lo], w = row[hi];
                        if ((u > w) == ((lo & k) == 0)) { row[lo] = w; row[hi] = u; }
                    }
                    __syncthreads();
                }
            }
            for (int c = 0; c < p.nC; ++c) {
                int i = (int)floor((double)R * p.ci[c]);
                i = i > R - 1 ? R - 1 : i;
                if (tid == 0) p.quant[(b * nq + q) * p.nC + c] = row[i];
            }
        }
        __syncthreads();                                                 // the series is read before the next one overwrites it
    }
}

}  // namespace ivs
