// Delta-quoted smile points off snapshot surfaces (rules D1-D6): for every row (b, j) of
// vol [B][mT][mK] and every target z = inv_cdf(call delta), the (strike, vol) on the chord between the first pair of
// neighbouring valid nodes whose d1 - z goes from >= 0 to < 0.
//
// One wavefront owns `group` consecutive rows (group * nD <= 64).  Bracket phase, row after row: lane = node, one
// coalesced read of the row's Kq and vol per 64-node chunk, d1 once per node; a node's partner is the previous valid node
// (the highest set bit of the validity ballot below the lane, or the last valid node carried over from the chunks
// before), so a pair is owned by its upper node and a bracket may span invalid nodes and chunk edges.  Per target one
// ballot of "partner's h >= 0 and own h < 0": its lowest set bit is the first bracket, its popcount adds to the
// crossing count.  Lane g*nD + t keeps the two node indices and the count of (row g, target t).  Inversion phase, once:
// the group's <= 64 (row, target) pairs bisect side by side, one lane each, and consecutive lanes store consecutive
// output elements.  No LDS, no atomics, no scratch; z travels in the kernel arguments.
#pragma once
#include "ivs_device.hpp"

namespace ivs {

constexpr int SM_MAX_D = 16;     // targets per call
constexpr int SM_WAVES = 4;      // wavefronts per workgroup
constexpr int SM_STEPS = 52;     // rule D5: bisection steps

struct SmileParams {
    const double* vol; const double* Kq; const double* Tq; const double* spot;
    int64_t kq_stride, tq_stride;                        // 0 = shared
    double rate;
    double z[SM_MAX_D];
    int32_t mK, mT, nD, group;                           // group = rows per wavefront, group * nD <= 64
    int64_t rows;                                        // B * mT
    double* q_vol; double* q_strike; int32_t* q_flags;   // [rows][nD]
};

// rule D1: bs_greeks_one's d1, spelled the same way (sq = sqrt(tau))
__device__ __forceinline__ double sm_d1(double S, double k, double s, double r, double tau, double sq) {
    return (log(S / k) + (r + 0.5 * s * s) * tau) / (s * sq);
}

__global__ __launch_bounds__(SM_WAVES * 64) void smile_delta_kernel(SmileParams p) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t row0 = ((int64_t)blockIdx.x * SM_WAVES + wave) * p.group;
    if (row0 >= p.rows) return;                                          // the whole wavefront
    const int ng = (int)((p.rows - row0) < p.group ? (p.rows - row0) : p.group);
    const int my_g = lane / p.nD, my_t = lane - my_g * p.nD;             // this lane's slot: row row0 + my_g, target my_t

    double my_z = 0.0;
    for (int t = 0; t < p.nD; ++t)
        if (my_t == t) my_z = p.z[t];
    int32_t ia = 0, ib = 0, cnt = 0;                                     // bracket nodes and crossings of the slot
    bool dead = true;

    for (int g = 0; g < ng; ++g) {
        const int64_t row = row0 + g;
        const int64_t b = row / p.mT;
        const int j = (int)(row - b * p.mT);
        const double S = p.spot[b], tau = p.Tq[b * p.tq_stride + j];
        int nvalid = 0;
        if (finite_pos(S) && finite_pos(tau)) {                          // D2; uniform over the wavefront
            const double sq = sqrt(tau);
            const double* kr = p.Kq + b * p.kq_stride;
            const double* vr = p.vol + row * p.mK;
            int32_t c_idx = -1;                                          // last valid node of the chunks before this one
            double c_d1 = 0.0;
            for (int64_t c0 = 0; c0 < p.mK; c0 += 64) {
                const int64_t i = c0 + lane;
                const bool in = i < p.mK;
                const double k = in ? kr[i] : qnan(), s = in ? vr[i] : qnan();
                const bool valid = finite_pos(k) && finite_pos(s);
                const double d1 = sm_d1(S, k, s, p.rate, tau, sq);
                const unsigned long long vm = __ballot(valid);
                const unsigned long long below = vm & ((1ull << lane) - 1ull);
                const int pl = below ? 63 - __builtin_clzll(below) : 0;
                const double pd_in = __shfl(d1, pl);
                const double pd1 = below ? pd_in : c_d1;
                const int32_t pidx = below ? (int32_t)c0 + pl : c_idx;
                const bool pair = valid && pidx >= 0;
                nvalid += __popcll(vm);
                for (int t = 0; t < p.nD; ++t) {
                    const double z = p.z[t];
                    const unsigned long long cm = __ballot(pair && pd1 - z >= 0.0 && d1 - z < 0.0);   // D4
                    if (cm) {
                        const int fb = __builtin_ctzll(cm);
                        const int32_t a_idx = __shfl(pidx, fb);
                        if (lane == g * p.nD + t) {
                            if (cnt == 0) { ia = a_idx; ib = (int32_t)c0 + fb; }
                            cnt += __popcll(cm);
                        }
                    }
                }
                if (vm) {
                    const int last = 63 - __builtin_clzll(vm);
                    c_d1 = __shfl(d1, last);
                    c_idx = (int32_t)c0 + last;
                }
            }
        }
        if (my_g == g) dead = nvalid < 2;
    }

    if (lane >= ng * p.nD) return;
    double qv = qnan(), qk = qnan();
    int32_t fl = IVS_SM_DEAD;
    if (!dead) {
        fl = cnt == 0 ? IVS_SM_NO_CROSSING : (cnt > 1 ? IVS_SM_AMBIGUOUS : IVS_SM_OK);
        if (cnt > 0) {                                                   // D5
            const int64_t row = row0 + my_g;
            const int64_t b = row / p.mT;
            const int j = (int)(row - b * p.mT);
            const double S = p.spot[b], tau = p.Tq[b * p.tq_stride + j];
            const double sq = sqrt(tau);
            const double* kr = p.Kq + b * p.kq_stride;
            const double* vr = p.vol + row * p.mK;
            const double ka = kr[ia], sa = vr[ia];
            const double dk = kr[ib] - ka, ds = vr[ib] - sa;
            double lo = 0.0, hi = 1.0;
            for (int it = 0; it < SM_STEPS; ++it) {
                const double mid = 0.5 * (lo + hi);
                const double h = sm_d1(S, ka + mid * dk, sa + mid * ds, p.rate, tau, sq) - my_z;
                if (h >= 0.0) lo = mid; else hi = mid;
            }
            const double w = 0.5 * (lo + hi);
            qk = ka + w * dk;
            qv = sa + w * ds;
        }
    }
    const int64_t o = row0 * p.nD + lane;                                // D6: every element, consecutive lanes
    p.q_vol[o] = qv;
    p.q_strike[o] = qk;
    p.q_flags[o] = fl;
}

}  // namespace ivs
