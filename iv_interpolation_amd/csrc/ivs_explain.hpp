// P&L explain of a book between snapshots (rules X0-X9): what the book earned from snapshot p to snapshot
// p + lag, per option and summed over the book, split into theta, delta, gamma, vega and a remainder under sticky strike and under
// sticky moneyness.  Everything is built from the device functions of ivs_risk.hpp (rk_locate, rk_surface, rk_W, rk_greeks,
// rk_price, rk_wave_sum) and, underneath, st_stage / st_bracket of ivs_svi_surface.hpp: this file adds no arithmetic of its own
// beyond the ten figures of rules X3 and X4.
//
// svi_explain_kernel: a workgroup of four wavefronts owns one pair.  Both ends' slices are staged in LDS (2 x 64 x 6 doubles) and
// read at uniform addresses; the options pass through 256 at a time, lane = option.  Per option three placements (X1): (a) end 0
// at the option's own tenor, (b) end 1 at the tenor left, (c) end 0's slices at the tenor left.  Rule X7 is B5: an xor butterfly
// inside each wavefront, the four wavefront sums through LDS as (s0 + s1) + (s2 + s3), the passes serially in the register of
// the thread that owns the figure.  No atomics; a pair's bits depend on its two snapshots and on Q alone.
//
// Rule X8: contraction is off throughout, both prices come from rk_price on rk_surface's W and the three vols from rk_sigma, so
// a pair whose two ends carry the same bits yields the same sequence of IEEE operations on the same operands at both ends.
#pragma once
#include "ivs_risk.hpp"

namespace ivs {

constexpr int XP_OUT = 10;             // actual, theta_pnl, delta_ss, gamma_ss, vega_ss, resid_ss, delta_sm, gamma_sm, vega_sm, resid_sm
constexpr int XP_NET = 12;             // the ten, then qty P0 and |qty| P0

struct ExplainParams {
    const double* params; const double* Tq; const double* spot;
    const double* u; const double* tau; const uint8_t* is_put; const double* qty;
    int64_t tq_stride, q_stride;                         // 0 = shared
    double rate;
    int32_t mT, strike_mode, lag;
    int64_t Q;
    double* out[XP_OUT];                                 // [P][Q], each may be null
    double* net; int32_t* n_dead;                        // [P][12], [P]
    int32_t* flags;                                      // [P][Q]
};

__global__ __launch_bounds__(RK_BLOCK) void svi_explain_kernel(ExplainParams p) {
#pragma clang fp contract(off)
    __shared__ double sl[2][ST_MAX_T * 6];
    __shared__ double npart[RK_WAVES][XP_NET];
    __shared__ int32_t dpart[RK_WAVES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t b0 = blockIdx.x, b1 = b0 + p.lag;                      // X0: the pair's two ends
    const double S0 = p.spot[b0], S1 = p.spot[b1];
    st_stage(sl[0], p.params, p.Tq, p.tq_stride, b0, p.mT, S0);
    st_stage(sl[1], p.params, p.Tq, p.tq_stride, b1, p.mT, S1);
    __syncthreads();
    const double dS = S1 - S0;
    const double dS2 = dS * dS;

    double ntot = 0.0;                                                   // thread k < 12: net figure k
    int32_t dead = 0;
    bool degenerate = false;
    for (int64_t q0 = 0; q0 < p.Q; q0 += RK_BLOCK) {
        const int64_t q = q0 + tid;
        // rk_option and RkOption::live spelled out: through them this kernel runs 0.5 % slower (profiles/book_refactor/bench.txt)
        const bool valid = q < p.Q;
        const double u = valid ? p.u[b0 * p.q_stride + q] : qnan();
        const double t0 = valid ? p.tau[b0 * p.q_stride + q] : qnan();
        const double t1 = valid ? p.tau[b1 * p.q_stride + q] : qnan();
        const double qty = valid ? p.qty[q] : 0.0;
        const bool put = valid && p.is_put ? p.is_put[q] != 0 : false;
        const double K = p.strike_mode == 0 ? S0 * u : u;                // X0: end 0's strike, absolute from here on
        bool un0, any0, un1, any1, unc, anyc;
        const RkPoint a = rk_locate(sl[0], p.mT, S0, u, t0, p.rate, p.strike_mode, un0, any0);
        const RkPoint e = rk_locate(sl[1], p.mT, S1, K, t1, p.rate, 1, un1, any1);
        const RkPoint c = rk_locate(sl[0], p.mT, S0, K, t1, p.rate, 1, unc, anyc);
        degenerate = un0 || !any0 || un1 || !any1;                       // the pair's: the same in every thread and pass
        const bool live = valid && a.ok && e.ok && c.ok && qty - qty == 0.0;                   // X2
        rk_dead_part(dpart, wave, lane, valid && !live);

        int32_t fl = a.fl | (e.fl << 8) | (c.fl << 16);                  // X5
        double o[XP_NET];
        for (int k = 0; k < XP_NET; ++k) o[k] = qnan();
        if (a.ok) {
            double W, W1, W2, V;
            rk_surface(sl[0], a, W, W1, W2, V);
            if (V < 0.0) fl |= IVS_SE_NEG_FWD;
            if (live) {
                double g[7];
                rk_greeks(RK_ALL, S0, a.K, a.D, a.x, t0, p.rate, W, W1, W2, V, put, g);
                double We, We1, We2, Ve;
                rk_surface(sl[1], e, We, We1, We2, Ve);
                const double P1 = rk_price(S1, e.K * e.D, e.x, sqrt(We), put);
                const double sg1 = rk_sigma(sl[1], e, e.x, t1);
                const double sg_ss = rk_sigma(sl[0], c, c.x, t1);
                const double sg_sm = rk_sigma(sl[0], c, e.x, t1);         // e.x = log(K / S1) - rate t1: the new moneyness
                const double dt = t0 - t1;
                // X3: a product that is a zero of either sign is written as +0.0
                o[0] = P1 - g[0];
                o[1] = g[6] * dt + 0.0;
                o[2] = g[1] * dS + 0.0;
                o[3] = (0.5 * g[3]) * dS2 + 0.0;
                o[4] = g[5] * (sg1 - sg_ss) + 0.0;
                o[5] = o[0] - (((o[1] + o[2]) + o[3]) + o[4]);            // X4
                o[6] = g[2] * dS + 0.0;
                o[7] = (0.5 * g[4]) * dS2 + 0.0;
                o[8] = g[5] * (sg1 - sg_sm) + 0.0;
                o[9] = o[0] - (((o[1] + o[6]) + o[7]) + o[8]);
                o[10] = g[0];
                o[11] = g[0];
            }
        }
        if (valid) {                                                     // consecutive lanes, consecutive elements
            const int64_t at = b0 * p.Q + q;
            for (int k = 0; k < XP_OUT; ++k)
                if (p.out[k]) p.out[k][at] = o[k];
            p.flags[at] = fl;
        }
        for (int k = 0; k < XP_NET; ++k) {                               // X6, X7
            const double w = k == XP_NET - 1 ? fabs(qty) : qty;
            const double s = rk_wave_sum(live ? w * o[k] : 0.0);
            if (lane == 0) npart[wave][k] = s;
        }
        __syncthreads();
        if (tid < XP_NET) ntot = ntot + rk_four([&](int w) { return npart[w][tid]; });
        dead += rk_dead_sum(dpart);
        __syncthreads();
    }
    if (tid < XP_NET) p.net[b0 * XP_NET + tid] = degenerate ? qnan() : ntot;
    if (tid == 0) p.n_dead[b0] = degenerate ? (int32_t)p.Q : dead;
}

}  // namespace ivs
