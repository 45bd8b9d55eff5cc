// What-if VaR and expected shortfall of a book per candidate trade and size (rules W0-W9): what the tail
// figures of section 19 become when q units of candidate h are added to the book, for every snapshot p, candidate h and rung j
// of a ladder of sizes.  Stage 1 is svi_inst_pnl_kernel of ivs_hedge.hpp, launched as it is; this file adds the ladder.
//
// whatif_tail_kernel (W1, W3-W7): a WAVEFRONT owns snapshot p and some of its candidates.  It reads the book's row y and forms the
// ranked set once and keeps both in registers, lane = scenario (s = 64 i + lane, i < NW), for every candidate and rung it takes;
// a candidate's column x is read once (lane = scenario again: the column is strided, but it is read once for nQ rungs of
// selection, see section 22) and kept for its rungs.  Per rung the row z = y + q x is formed in registers and the m_max smallest
// of it are taken out ONE AT A TIME in rank order: the smallest value of the wavefront (a minimum per lane, an xor butterfly across
// lanes), then the lowest s that holds it (one compare per register, whose mask is the ballot), which is struck out.  That is H7's
// order (ascending, ties to the lower s, -0.0 == +0.0), and the values come out in the order in which H7 adds them, so the serial
// sum runs alongside.  Nothing is ranked past m_max = max_l m_l: n x m_max / 64 compares per row in the place of the n x n / 64 of
// hsim_tail_kernel.  No LDS, no barrier, no atomics, no scratch.  The four wavefronts of a workgroup share nothing: how many
// candidates a workgroup takes (cpw) changes no bit.
//
// Contraction is off throughout (B4): q x is rounded, then added to y (W4).
#pragma once
#include "ivs_hedge.hpp"

namespace ivs {

constexpr int WI_MAX_RUNGS = 16;
constexpr int WI_WAVES = 4;

struct WhatIfParams {
    const double* pnl; const int32_t* scen_flags;        // [B][window]
    const double* inst_pnl;                              // [B][window][nH]
    const double* size; int64_t size_stride;             // [nH][nQ] (0) or [B][nH][nQ] (nH * nQ)
    int32_t lag, window, nH, nQ, nL, min_scen, cpw, nchunk;              // cpw = candidates per workgroup, nchunk = workgroups per snapshot
    double tp[HS_MAX_LEVELS];
    int32_t* trade_flags;                                // [B][nH]
    double* var_w; double* es_w;                         // [B][nH][nQ][nL]
    int32_t* worst_w;                                    // [B][nH][nQ], may be null
    int32_t* best;                                       // [B][nH][nL]
    double* var0; double* es0;                           // [B][nL]
    int32_t* worst0; int32_t* n_scen;                    // [B]
};

// H7 on the row z, NaN where a scenario is not ranked, by taking the mm smallest out in rank order; z is used up.  m_l: the tail
// of this lane's level, 0 for a lane without one.  The value that comes out is the wavefront's minimum, which equals the element
// struck out and can differ from it in the sign of a zero alone: 0.0 - v and sum + v give the same bits for either zero.
template <int NW>
__device__ __forceinline__ void wi_tail(double (&z)[NW], int lane, int mm, int m_l, double& var, double& es, int& worst) {
#pragma clang fp contract(off)
    double sum = 0.0;
    var = qnan();
    es = qnan();
    worst = -1;
    for (int k = 0; k < mm; ++k) {
        double v = z[0];
#pragma unroll
        for (int i = 1; i < NW; ++i) v = fmin(v, z[i]);                  // NaN (struck out, not ranked) loses to a number
        for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
        v = __shfl(v, 0);                                                // one zero for all lanes
        int fi = 0;
        unsigned long long fm = 0ull;
#pragma unroll
        for (int i = NW - 1; i >= 0; --i) {                              // the lowest s that holds it: the lowest i, then the lowest lane
            const unsigned long long eq = __ballot(z[i] == v);
            if (eq != 0ull) { fi = i; fm = eq; }
        }
        const int fl = __ffsll((long long)fm) - 1;
#pragma unroll
        for (int i = 0; i < NW; ++i)
            if (i == fi && lane == fl) z[i] = qnan();
        if (k == 0) worst = fi * 64 + fl;
        sum = sum + v;
        if (k + 1 == m_l) {
            var = 0.0 - v;
            es = 0.0 - sum / (double)m_l;
        }
    }
}

template <int NW>
__global__ __launch_bounds__(WI_WAVES * 64) void whatif_tail_kernel(WhatIfParams p) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t b = blockIdx.x / p.nchunk;
    const int ch = (int)(blockIdx.x - b * p.nchunk);
    const int W = p.window;
    const int64_t np64 = b - p.lag + 1;                                  // H0
    const int n_p = np64 < 0 ? 0 : (np64 > W ? W : (int)np64);
    const int64_t row0 = b * W;

    double y[NW], z[NW];                                                 // W1: the row and the ranked set, once per wavefront
    unsigned rk = 0;
    int n = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const int s = i * 64 + lane;
        const bool in = s < W && s < n_p;
        const double v = in ? p.pnl[row0 + s] : qnan();
        const bool ok = in && p.scen_flags[row0 + s] == 0 && v == v;
        y[i] = ok ? v : qnan();
        rk |= ok ? 1u << i : 0u;
        n += __popcll(__ballot(ok));
    }
    const bool active = n >= p.min_scen && n > 0;
    int m_l = 0, mm = 1;                                                 // H7's tails: this lane's and the longest
    for (int l = 0; l < p.nL; ++l) {
        int m = (int)floor((double)n * p.tp[l]);
        m = m < 1 ? 1 : m;
        if (lane == l) m_l = m;
        mm = m > mm ? m : mm;
    }
    if (!active) { m_l = 0; mm = 1; }

    if (ch == 0 && wave == 0) {                                          // W6: H7 on y itself
        double var = qnan(), es = qnan();
        int worst = -1;
        if (n > 0) {
#pragma unroll
            for (int i = 0; i < NW; ++i) z[i] = y[i];
            wi_tail<NW>(z, lane, mm, m_l, var, es, worst);
        }
        if (lane < p.nL) { p.var0[b * p.nL + lane] = var; p.es0[b * p.nL + lane] = es; }
        if (lane == 0) { p.worst0[b] = worst; p.n_scen[b] = n; }
    }

    const int h1 = (ch + 1) * p.cpw < p.nH ? (ch + 1) * p.cpw : p.nH;
    for (int h = ch * p.cpw + wave; h < h1; h += WI_WAVES) {
        double x[NW];
        bool nanx = false;
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const bool on = (rk >> i) & 1u;
            x[i] = on ? p.inst_pnl[(row0 + i * 64 + lane) * p.nH + h] : 0.0;
            nanx = nanx || !(x[i] == x[i]);
        }
        const bool bad = __ballot(nanx) != 0ull;                         // W3
        if (lane == 0) p.trade_flags[b * p.nH + h] = bad ? IVS_HG_NEG_VOL : 0;
        const double* qs = p.size + b * p.size_stride + (int64_t)h * p.nQ;
        const int64_t at = (b * p.nH + h) * p.nQ;
        double be = 0.0;                                                 // W7, lane = level
        int bj = -1;
        for (int j = 0; j < p.nQ; ++j) {
            const double q = qs[j];
            bool live = !bad && active && fabs(q) < __builtin_inf();
            if (live) {                                                  // W4
                bool nanz = false;
#pragma unroll
                for (int i = 0; i < NW; ++i) {
                    const bool on = (rk >> i) & 1u;
                    const double t = q * x[i];
                    z[i] = on ? y[i] + t : qnan();
                    nanz = nanz || (on && !(z[i] == z[i]));
                }
                live = __ballot(nanz) == 0ull;                           // a row with inf - inf or 0 x inf in it has no order
            }
            double var = qnan(), es = qnan();
            int worst = -1;
            if (live) wi_tail<NW>(z, lane, mm, m_l, var, es, worst);     // W5
            if (lane < p.nL) {
                p.var_w[(at + j) * p.nL + lane] = var;
                p.es_w[(at + j) * p.nL + lane] = es;
                if (live && es == es && (bj < 0 || es < be)) { be = es; bj = j; }
            }
            if (lane == 0 && p.worst_w) p.worst_w[at + j] = worst;
        }
        if (lane < p.nL) p.best[(b * p.nH + h) * p.nL + lane] = bj;
    }
}

}  // namespace ivs
