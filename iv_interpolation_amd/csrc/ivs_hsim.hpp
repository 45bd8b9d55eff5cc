// Historical-simulation VaR and expected shortfall of a book per snapshot (rules H0-H9): every past pair
// of snapshots (j, j + lag) is a scenario, applied to today's book with a full revaluation on the surface.  Everything is built
// from the device functions of ivs_risk.hpp (rk_locate, rk_sigma, rk_surface, rk_price, rk_greeks, rk_wave_sum) and, underneath,
// st_stage / st_bracket of ivs_svi_surface.hpp: this file adds the scenario's spot and vol (H1, H2) and the order statistics (H7).
//
// svi_hsim_kernel: a workgroup of four wavefronts owns one snapshot p and a run of scenarios.  Today's slices are staged in LDS
// once.  The options pass through 256 at a time, lane = option, and the PASSES are the outer loop: the option's own state (its
// bracket on p, K, K D, sqrt(tau) and the base price of H3: a log, an exp, two square roots, a curve read and a price) is formed
// once per pass and kept in registers while the scenarios of the run go by.  Each scenario's two ends are staged as it comes
// up, into a ring of four slice buffers so that ONE barrier per scenario suffices (a buffer is overwritten two scenarios after
// its last read).  With lag == 1 the end of scenario s is the start of scenario s - 1: it is then neither staged nor bracketed
// again, the buffer and the option's bracket on it carry over.  A run longer than 256 scenarios is taken 256 at a time (thread t
// owns scenario t of the sub-run).  Rule H4 is B5: an xor butterfly inside each wavefront, the four wavefront sums through LDS
// as (s0 + s1) + (s2 + s3), the passes serially in the register of the thread that owns the scenario.  No atomics.
//
// hsim_tail_kernel: one workgroup per snapshot ranks the row of pnl by counting (H7) and forms VaR and ES per level.
//
// Contraction is off throughout (B4): the base price and a scenario whose pair carries the same bits at both ends are the same
// sequence of IEEE operations on the same operands (H3, H6).
#pragma once
#include "ivs_risk.hpp"

namespace ivs {

constexpr int HS_MAX_WINDOW = 1024;    // scenarios per snapshot: the row of the tail kernel lives in LDS
constexpr int HS_MAX_LEVELS = 8;       // the tail probabilities travel in the kernel's arguments
constexpr int HS_RUN = 256;            // scenarios per sub-run: one per thread

struct HsimParams {
    const double* params; const double* Tq; const double* spot;
    const double* u; const double* tau; const uint8_t* is_put; const double* qty;
    int64_t tq_stride, q_stride;                         // 0 = shared
    double rate;
    int32_t mT, strike_mode, lag, window, spw, nchunk;   // spw = scenarios per workgroup, nchunk = workgroups per snapshot
    int64_t Q;
    double* pnl; int32_t* scen_flags;                    // [B][window]
    double* value; int32_t* n_dead;                      // [B][2] (may be null), [B]
};

struct HsimTailParams {
    const double* pnl; const int32_t* scen_flags;        // [B][window]
    int32_t window, nL, min_scen;
    double tp[HS_MAX_LEVELS];
    double* var; double* es;                             // [B][nL]
    int32_t* n_valid; int32_t* worst;                    // [B]
};

__global__ __launch_bounds__(RK_BLOCK) void svi_hsim_kernel(HsimParams p) {
#pragma clang fp contract(off)
    __shared__ double sl[ST_MAX_T * 6];                                  // today's slices
    __shared__ double hist[4][ST_MAX_T * 6];                             // the ring of the scenarios' ends
    __shared__ double part[RK_WAVES][HS_RUN];                            // wavefront sums per scenario
    __shared__ int32_t pflag[RK_WAVES][HS_RUN];
    __shared__ double vpart[RK_WAVES][2];
    __shared__ int32_t dpart[RK_WAVES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t b = blockIdx.x / p.nchunk;
    const int ch = (int)(blockIdx.x - b * p.nchunk);
    const int s0 = ch * p.spw;
    const int s1 = p.window - s0 < p.spw ? p.window : s0 + p.spw;        // this workgroup's scenarios: s0 <= s < s1
    const int64_t np64 = b - p.lag + 1;                                  // H0: the scenarios that exist
    const int n_p = np64 < 0 ? 0 : (np64 > p.window ? p.window : (int)np64);
    const bool first = ch == 0;                                          // this workgroup also owns value and n_dead
    const bool reuse = p.lag == 1;
    const double S = p.spot[b];
    st_stage(sl, p.params, p.Tq, p.tq_stride, b, p.mT, S);
    __syncthreads();

    for (int c0 = s0; c0 < s1; c0 += HS_RUN) {
        const int nc = s1 - c0 < HS_RUN ? s1 - c0 : HS_RUN;
        const int nce = n_p - c0 < 0 ? 0 : (n_p - c0 < nc ? n_p - c0 : nc);                      // those of the sub-run that exist
        const bool owner = first && c0 == 0;
        double tot = 0.0, vtot = 0.0;                                    // thread t: scenario c0 + t; thread k < 2: value figure k
        int32_t tflag = 0, dead = 0;
        bool degenerate = false;
        for (int64_t q0 = 0; q0 < p.Q; q0 += RK_BLOCK) {
            const RkOption opt = rk_option(p, b, q0 + tid);
            const double tq = opt.tau, qty = opt.qty;
            const bool put = opt.put;
            bool unordered, any;
            const RkPoint pt = rk_locate(sl, p.mT, S, opt.u, tq, p.rate, p.strike_mode, unordered, any);
            degenerate = unordered || !any;                              // the snapshot's: the same in every thread and pass
            const bool live = opt.live(pt.ok);
            if (owner) {                                                 // H8
                rk_dead_part(dpart, wave, lane, opt.valid && !live);
                double o[7];
                o[0] = 0.0;
                if (live && p.value) {
                    double W, W1, W2, V;
                    rk_surface(sl, pt, W, W1, W2, V);
                    rk_greeks(RK_PRICE, S, pt.K, pt.D, pt.x, tq, p.rate, W, W1, W2, V, put, o);
                }
                const double v0 = rk_wave_sum(live ? qty * o[0] : 0.0);
                const double v1 = rk_wave_sum(live ? fabs(qty) * o[0] : 0.0);
                if (lane == 0) { vpart[wave][0] = v0; vpart[wave][1] = v1; }
            }

            // H3: the option's own state; the base goes through the code of a scenario with the quotient 1.0 and the change +0.0
            const double KD = pt.K * pt.D;
            const double sqt = sqrt(tq);
            double base;
            {
                const double S1 = S * 1.0;
                const double x1 = log(pt.K / S1) - pt.rt;
                base = rk_price(S1, KD, x1, (rk_sigma(sl, pt, x1, tq) + 0.0) * sqt, put);
            }
            RkPoint ea;                                                  // the option on the start of the previous scenario
            bool una = false, anya = false;
            for (int c = 0; c < nce; ++c) {
                const int64_t ja = b - p.lag - (c0 + c), jb = ja + p.lag;               // H0
                const int ib = reuse ? c & 3 : 2 * (c & 1);
                const int ia = reuse ? (c + 1) & 3 : ib + 1;
                const double Sa = p.spot[ja], Sb = p.spot[jb];
                st_stage(hist[ia], p.params, p.Tq, p.tq_stride, ja, p.mT, Sa);
                if (!reuse || c == 0) st_stage(hist[ib], p.params, p.Tq, p.tq_stride, jb, p.mT, Sb);
                __syncthreads();
                RkPoint eb;
                bool unb, anyb;
                if (reuse && c > 0) { eb = ea; unb = una; anyb = anya; }
                else eb = rk_locate(hist[ib], p.mT, Sb, pt.K, tq, p.rate, 1, unb, anyb);
                ea = rk_locate(hist[ia], p.mT, Sa, pt.K, tq, p.rate, 1, una, anya);
                // H1: the pair's, the same in every thread
                const bool vd = una || !anya || unb || !anyb || !finite_pos(Sa) || !finite_pos(Sb) || degenerate;
                double sum = 0.0;
                int32_t f = IVS_HS_VOID_PAIR;
                if (!__builtin_amdgcn_readfirstlane((int)vd)) {
                    const double S1 = S * (Sb / Sa);                     // H1: the quotient first
                    const double x1 = log(pt.K / S1) - pt.rt;
                    const double sg = rk_sigma(sl, pt, x1, tq) + (rk_sigma(hist[ib], eb, x1, tq) - rk_sigma(hist[ia], ea, x1, tq));       // H2
                    const double pr = rk_price(S1, KD, x1, sg * sqt, put);
                    sum = rk_wave_sum(live ? qty * (pr - base) : 0.0);
                    f = __ballot(live && !(sg > 0.0)) != 0ull ? IVS_HS_NEG_VOL : 0;              // H5
                }
                if (lane == 0) { part[wave][c] = sum; pflag[wave][c] = f; }
            }
            __syncthreads();
            if (tid < nce) {                                             // B5: rk_four, then the passes in turn
                tot = tot + rk_four([&](int w) { return part[w][tid]; });
                tflag |= rk_four_or([&](int w) { return pflag[w][tid]; });
            }
            if (owner) {
                if (tid < 2) vtot = vtot + rk_four([&](int w) { return vpart[w][tid]; });
                dead += rk_dead_sum(dpart);
            }
            __syncthreads();
        }
        if (tid < nc) {                                                  // H5
            const int64_t at = b * p.window + c0 + tid;
            const int32_t f = tid < nce ? tflag : IVS_HS_ABSENT;
            p.pnl[at] = f != 0 ? qnan() : tot;
            p.scen_flags[at] = f;
        }
        if (owner && tid < 2 && p.value) p.value[b * 2 + tid] = degenerate ? qnan() : vtot;
        if (owner && tid == 0) p.n_dead[b] = degenerate ? (int32_t)p.Q : dead;
    }
}

// H7.  A scenario is ranked when it has no flag and its P&L is a number (sums that overflowed to inf - inf are left out).
__global__ __launch_bounds__(RK_BLOCK) void hsim_tail_kernel(HsimTailParams p) {
#pragma clang fp contract(off)
    __shared__ double row[HS_MAX_WINDOW];                                // 8 KB: the row, NaN where not ranked
    __shared__ double sorted[HS_MAX_WINDOW];
    __shared__ int32_t cnt[RK_WAVES];
    __shared__ int32_t first_s;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t b = blockIdx.x;
    int32_t mine = 0;
    for (int s = tid; s - tid < p.window; s += RK_BLOCK) {               // whole wavefronts go round together
        const bool in = s < p.window;
        const double v = in ? p.pnl[b * p.window + s] : qnan();
        const bool ok = in && p.scen_flags[b * p.window + s] == 0 && v == v;
        if (in) row[s] = ok ? v : qnan();
        mine += __popcll(__ballot(ok));
    }
    if (lane == 0) cnt[wave] = mine;
    if (tid == 0) first_s = -1;
    __syncthreads();
    const int n = cnt[0] + cnt[1] + cnt[2] + cnt[3];
    for (int s = tid; s < p.window; s += RK_BLOCK) {
        const double v = row[s];
        if (!(v == v)) continue;
        int r = 0;
        for (int i = 0; i < p.window; ++i) {                             // uniform LDS addresses; -0.0 == +0.0: the lower s first
            const double w = row[i];
            r += (w < v || (w == v && i < s)) ? 1 : 0;
        }
        sorted[r] = v;
        if (r == 0) first_s = s;
    }
    __syncthreads();
    if (tid == 0) { p.n_valid[b] = n; p.worst[b] = first_s; }
    if (tid < p.nL) {
        double var = qnan(), es = qnan();
        if (n >= p.min_scen && n > 0) {
            int m = (int)floor((double)n * p.tp[tid]);
            m = m < 1 ? 1 : m;
            double sum = 0.0;
            for (int i = 0; i < m; ++i) sum = sum + sorted[i];
            var = 0.0 - sorted[m - 1];
            es = 0.0 - sum / (double)m;
        }
        p.var[b * p.nL + tid] = var;
        p.es[b * p.nL + tid] = es;
    }
}

}  // namespace ivs
