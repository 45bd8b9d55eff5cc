// Attribution of a book's historical-simulation VaR and expected shortfall to its options and to groups of them (DESIGN.md
// section 20, rules A0-A8): the Euler allocation of the tail.  Component ES of an option is the mean of its own P&L over the
// scenarios that make up the book's tail, component VaR its P&L in the VaR scenario; both add up to the book's figures.
//
// svi_hsim_attrib_kernel: one workgroup of four wavefronts per snapshot.  It reads the row of pnl and scen_flags that
// ivs_svi_hsim_f64 wrote, ranks it in LDS by counting as hsim_tail_kernel does (A1) and keeps the rank -> s table of the first
// HA_MAX_TAIL ranks.  H7's tail sets are nested prefixes of that one order, so every level is served by revaluing the book in the
// M = max m_l lowest-ranked scenarios only.  Today's slices are staged once; the options pass through 256 at a time, lane =
// option, the PASSES outside and the ranks inside (section 19's reason: the option's own state is formed once per pass).  Each
// rank's two ends are staged afresh into one of two pairs of slice buffers: inside a pass a pair is overwritten two ranks after
// its last read, so one barrier per rank suffices there, and one more barrier ends every pass, because rank 0 of the next pass
// stages into the pair that the last rank of an odd M has just read.  Tail scenarios are not neighbours, so nothing carries over
// from rank to rank.  The term t(q, r) is svi_hsim_kernel's, through the same device
// functions (rk_locate, rk_sigma, rk_price) in the same order: the same bits (A2).  The per-option running sums per level stay in
// registers.  The per-rank group sums are B5: rk_wave_sum, the four wavefront sums through LDS as (s0 + s1) + (s2 + s3), the
// passes serially in the register of the thread that owns the (rank, group) entry.  Plain vector stores, no atomics, no scratch.
//
// The row (8 KB) is dead once the ranks are known; it lies in the first quarter of the wavefront sums (32 KB).
#pragma once
#include "ivs_hsim.hpp"

namespace ivs {

constexpr int HA_MAX_TAIL = 64;        // A7: ranks revalued per snapshot; the per-rank group sums live in LDS
constexpr int HA_MAX_GROUPS = 16;
constexpr int HA_OWN = HA_MAX_TAIL * HA_MAX_GROUPS / RK_BLOCK;           // (rank, group) entries per thread

struct HsimAttribParams {
    const double* params; const double* Tq; const double* spot;
    const double* u; const double* tau; const uint8_t* is_put; const double* qty;
    int64_t tq_stride, q_stride;                         // 0 = shared
    double rate;
    int32_t mT, strike_mode, lag, window, nL, min_scen, nG;
    int64_t Q;
    double tp[HS_MAX_LEVELS];
    const double* pnl; const int32_t* scen_flags;        // [B][window], as ivs_svi_hsim_f64 wrote them
    const int32_t* group;                                // [Q] or null = every option in group 0
    double* ces; double* cvar;                           // [B][nL][Q], each may be null
    double* ces_group; double* cvar_group;               // [B][nL][nG], each may be null
    int32_t* n_tail;                                     // [B][nL]
    int32_t* order;                                      // [B][window], may be null
};

__global__ __launch_bounds__(RK_BLOCK) void svi_hsim_attrib_kernel(HsimAttribParams p) {
#pragma clang fp contract(off)
    __shared__ double sl[ST_MAX_T * 6];                                  // today's slices
    __shared__ double hist[4][ST_MAX_T * 6];                             // two pairs of ends
    __shared__ double gp[RK_WAVES * HA_MAX_TAIL * HA_MAX_GROUPS];        // wavefront sums per (rank, group); before that the row
    __shared__ int32_t tab[HA_MAX_TAIL];                                 // rank -> s
    __shared__ int32_t mls[HS_MAX_LEVELS];                               // m_l, 0 = inactive
    __shared__ int32_t cnt[RK_WAVES];
    double* row = gp;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t b = blockIdx.x;
    const int64_t np64 = b - p.lag + 1;                                  // H0: the scenarios that exist
    const int n_p = np64 < 0 ? 0 : (np64 > p.window ? p.window : (int)np64);
    const int64_t row0 = b * p.window;
    const double S = p.spot[b];
    st_stage(sl, p.params, p.Tq, p.tq_stride, b, p.mT, S);

    // A1: ranked = no flag, a P&L that is a number and s < n_p (which keeps ja >= 0 below whatever the row holds)
    int32_t mine = 0;
    for (int s = tid; s - tid < p.window; s += RK_BLOCK) {               // whole wavefronts go round together
        const bool in = s < p.window;
        const double v = in ? p.pnl[row0 + s] : qnan();
        const bool ok = in && s < n_p && p.scen_flags[row0 + s] == 0 && v == v;
        if (in) row[s] = ok ? v : qnan();
        mine += __popcll(__ballot(ok));
    }
    if (lane == 0) cnt[wave] = mine;
    if (tid < HA_MAX_TAIL) tab[tid] = 0;
    __syncthreads();
    const int n = __builtin_amdgcn_readfirstlane(cnt[0] + cnt[1] + cnt[2] + cnt[3]);
    const bool active = n >= p.min_scen && n > 0;
    int ml[HS_MAX_LEVELS];
    int M = 0;
#pragma unroll
    for (int l = 0; l < HS_MAX_LEVELS; ++l) {
        int m = 0;
        if (l < p.nL && active) {                                        // H7's m, the same IEEE product
            m = (int)floor((double)n * p.tp[l]);
            m = m < 1 ? 1 : (m > HA_MAX_TAIL ? HA_MAX_TAIL : m);         // A7 keeps it below the cap; the clamp never binds on a checked call
        }
        ml[l] = m;
        M = m > M ? m : M;
        if (tid == l) mls[l] = m;
        if (tid == l && l < p.nL) p.n_tail[b * p.nL + l] = m;
    }
    for (int s = tid; s < p.window; s += RK_BLOCK) {
        const double v = row[s];
        if (!(v == v)) continue;
        int r = 0;
        for (int i = 0; i < p.window; ++i) {                             // uniform LDS addresses; -0.0 == +0.0: the lower s first
            const double w = row[i];
            r += (w < v || (w == v && i < s)) ? 1 : 0;
        }
        if (r < HA_MAX_TAIL) tab[r] = s;
        if (p.order) p.order[row0 + r] = s;
    }
    if (p.order)
        for (int r = n + tid; r < p.window; r += RK_BLOCK) p.order[row0 + r] = -1;
    __syncthreads();                                                     // the row is dead from here: gp takes its place

    const bool groups = p.ces_group || p.cvar_group;
    const int nE = M * p.nG;                                             // entries e = r * nG + g
    double gt[HA_OWN];                                                   // thread t: entries t + 256 k
#pragma unroll
    for (int k = 0; k < HA_OWN; ++k) gt[k] = 0.0;
    bool degenerate = false;
    for (int64_t q0 = 0; q0 < p.Q; q0 += RK_BLOCK) {
        const RkOption opt = rk_option(p, b, q0 + tid);
        const double tq = opt.tau, qty = opt.qty;
        const bool put = opt.put;
        bool unordered, any;
        const RkPoint pt = rk_locate(sl, p.mT, S, opt.u, tq, p.rate, p.strike_mode, unordered, any);
        degenerate = unordered || !any;                                  // the snapshot's: the same in every thread and pass
        const bool live = opt.live(pt.ok);
        int grp = -1;                                                    // A0: outside 0..nG-1 = in no group
        if (opt.valid) {
            const int gq = p.group ? p.group[q0 + tid] : 0;
            grp = gq >= 0 && gq < p.nG ? gq : -1;
        }
        double acc[HS_MAX_LEVELS], cv[HS_MAX_LEVELS];
#pragma unroll
        for (int l = 0; l < HS_MAX_LEVELS; ++l) { acc[l] = 0.0; cv[l] = 0.0; }
        if (M > 0) {
            // H3: the option's own state, as svi_hsim_kernel forms it
            const double KD = pt.K * pt.D;
            const double sqt = sqrt(tq);
            double base;
            {
                const double S1 = S * 1.0;
                const double x1 = log(pt.K / S1) - pt.rt;
                base = rk_price(S1, KD, x1, (rk_sigma(sl, pt, x1, tq) + 0.0) * sqt, put);
            }
            for (int r = 0; r < M; ++r) {
                const int s = tab[r];
                const int64_t ja = b - p.lag - s, jb = ja + p.lag;       // H0; 0 <= ja by s < n_p
                const int ib = 2 * (r & 1), ia = ib + 1;                 // overwritten two ranks after its last read: one barrier
                const double Sa = p.spot[ja], Sb = p.spot[jb];
                st_stage(hist[ia], p.params, p.Tq, p.tq_stride, ja, p.mT, Sa);
                st_stage(hist[ib], p.params, p.Tq, p.tq_stride, jb, p.mT, Sb);
                __syncthreads();
                bool una, anya, unb, anyb;
                const RkPoint eb = rk_locate(hist[ib], p.mT, Sb, pt.K, tq, p.rate, 1, unb, anyb);
                const RkPoint ea = rk_locate(hist[ia], p.mT, Sa, pt.K, tq, p.rate, 1, una, anya);
                const bool vd = una || !anya || unb || !anyb || !finite_pos(Sa) || !finite_pos(Sb) || degenerate;
                double t = qnan();                                       // a void pair is never ranked in a row of section 19
                if (!__builtin_amdgcn_readfirstlane((int)vd)) {
                    const double S1 = S * (Sb / Sa);                     // H1
                    const double x1 = log(pt.K / S1) - pt.rt;
                    const double sg = rk_sigma(sl, pt, x1, tq) + (rk_sigma(hist[ib], eb, x1, tq) - rk_sigma(hist[ia], ea, x1, tq));       // H2
                    const double pr = rk_price(S1, KD, x1, sg * sqt, put);
                    t = qty * (pr - base);                               // A2
                }
#pragma unroll
                for (int l = 0; l < HS_MAX_LEVELS; ++l) {                // A3, A4
                    if (r < ml[l]) acc[l] = acc[l] + t;
                    if (r == ml[l] - 1) cv[l] = t;
                }
                if (groups) {                                            // A5
                    double own = 0.0;                                    // lane g: group g's wavefront sum
                    for (int g = 0; g < p.nG; ++g) {
                        const bool in = live && grp == g;
                        double sum = 0.0;
                        if (__ballot(in) != 0ull) sum = rk_wave_sum(in ? t : 0.0);
                        own = lane == g ? sum : own;
                    }
                    if (lane < p.nG) gp[(wave * HA_MAX_TAIL + r) * HA_MAX_GROUPS + lane] = own;
                }
            }
        }
        // every wavefront is done with the slice buffers (and has written its partials) before the next pass stages rank 0 into
        // pair 0 again: the last rank of a pass reads that pair when M is odd
        __syncthreads();
        if (groups) {
#pragma unroll
            for (int k = 0; k < HA_OWN; ++k) {                           // B5: rk_four, then the passes in turn
                const int e = tid + k * RK_BLOCK;
                if (e < nE) {
                    const int r = e / p.nG, g = e - r * p.nG;
                    gt[k] = gt[k] + rk_four([&](int w) { return gp[(w * HA_MAX_TAIL + r) * HA_MAX_GROUPS + g]; });
                }
            }
            __syncthreads();
        }
        if (opt.valid) {                                                 // A6; consecutive lanes, consecutive elements
#pragma unroll
            for (int l = 0; l < HS_MAX_LEVELS; ++l) {
                if (l < p.nL) {
                    const int64_t at = (b * p.nL + l) * p.Q + q0 + tid;
                    const bool on = ml[l] > 0 && live && !degenerate;
                    if (p.ces) p.ces[at] = on ? 0.0 - acc[l] / (double)ml[l] : qnan();
                    if (p.cvar) p.cvar[at] = on ? 0.0 - cv[l] : qnan();
                }
            }
        }
    }

    if (groups) {                                                        // the sums of every rank, then H7's own operations
#pragma unroll
        for (int k = 0; k < HA_OWN; ++k) {
            const int e = tid + k * RK_BLOCK;
            if (e < nE) gp[e] = gt[k];
        }
        __syncthreads();
        if (tid < p.nL * p.nG) {
            const int l = tid / p.nG, g = tid - l * p.nG;
            const int m = mls[l];
            double cg = qnan(), eg = qnan();
            if (m > 0 && !degenerate) {
                double sum = 0.0;
                for (int i = 0; i < m; ++i) sum = sum + gp[i * p.nG + g];
                cg = 0.0 - gp[(m - 1) * p.nG + g];
                eg = 0.0 - sum / (double)m;
            }
            const int64_t at = (b * p.nL + l) * p.nG + g;
            if (p.cvar_group) p.cvar_group[at] = cg;
            if (p.ces_group) p.ces_group[at] = eg;
        }
    }
}

}  // namespace ivs
