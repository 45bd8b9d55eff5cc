// Age-weighted, volatility-scaled historical-simulation VaR and expected shortfall (rules W0-W9): the row of
// scenario P&Ls of section 19 with a probability per scenario that decays with its age (Boudoukh-Richardson-Whitelaw) and, when
// asked for, every scenario multiplied by today's running vol of the spot over the vol at the scenario's start (Hull-White at the
// P&L level).  The call works on rows alone (pnl, scen_flags as a section 19 call wrote them) and on the snapshots' spot.
//
// spot_ewma_kernel: lane = snapshot, grid-stride.  A lane walks the M returns behind its snapshot serially (W1, W2); the spot it
// read as the later end of one return is the earlier end of the next, and neighbouring lanes read neighbouring spots.  The spots
// are loaded eight terms ahead, so that eight loads are in flight while the lane divides: the walk is a chain of latencies.
//
// hsim_wtail_kernel: a workgroup of four wavefronts owns one row.  It stages the row in LDS, forming f and z on the way (W3; the
// sigma reads run backwards from p - lag), and sums the weights of the ranked scenarios in the same sweep: thread t of pass k holds
// scenario 256 k + t, which is the layout of rule B5, so W5 goes through rk_wave_sum / rk_four.  It ranks by counting as
// hsim_tail_kernel does (W4 is H7 on z, restated here: hsim_tail_kernel stays the code it is) and scatters z and w by rank.  One
// lane per level then walks W7 up the ranks, four ranks per LDS round trip; a rank past the boundary changes nothing through
// selects, so the walk has no divergent exit inside a round trip.
//
// Contraction is off throughout (B4).  No floating-point atomics.
#pragma once
#include "ivs_hsim.hpp"

namespace ivs {

constexpr int HW_MAX_SPAN = 1024;      // returns per running vol
constexpr int HW_AHEAD = 8;            // spots a lane of spot_ewma_kernel loads before it walks them

struct SpotEwmaParams {
    const double* spot; const double* vol_weight;        // [B], [M]
    int64_t B;
    int32_t M, min_returns;
    double* sigma;                                       // [B]
};

struct WTailParams {
    const double* pnl; const int32_t* scen_flags;        // [B][window]
    const double* weight;                                // [window] by age, or null: every weight 1.0
    const double* sigma;                                 // [B], or null: no scaling
    int32_t window, nL, min_scen, lag;
    double cap, cap_lo;
    double tp[HS_MAX_LEVELS];
    double* var_w; double* es_w;                         // [B][nL]
    int32_t* n_valid_w; int32_t* worst_w;                // [B]
    double* wsum; double* n_eff;                         // [B]
    double* pnl_w; double* scale;                        // [B][window], may be null
    int32_t* flags_w;                                    // [B][window]
};

__global__ __launch_bounds__(RK_BLOCK) void spot_ewma_kernel(SpotEwmaParams p) {
#pragma clang fp contract(off)
    for (int64_t j = (int64_t)blockIdx.x * RK_BLOCK + threadIdx.x; j < p.B; j += (int64_t)gridDim.x * RK_BLOCK) {
        double num = 0.0, den = 0.0;
        int32_t cnt = 0;
        bool bad = false;
        double s1 = p.spot[j];
        for (int k0 = 0; k0 < p.M && j - k0 >= 1; k0 += HW_AHEAD) {      // W2: a term with j - k < 1 is left out, and so is every later one
            double s0[HW_AHEAD];                                         // the loads of a run of terms are in flight together
#pragma unroll
            for (int i = 0; i < HW_AHEAD; ++i) {
                const int64_t at = j - (k0 + i) - 1;
                s0[i] = (k0 + i < p.M && at >= 0) ? p.spot[at] : qnan(); // a term past M or before the first return: no spot, so it is left out
            }
#pragma unroll
            for (int i = 0; i < HW_AHEAD; ++i) {
                const double r = s1 / s0[i] - 1.0;                       // W1: the quotient first
                if (finite_pos(s1) && finite_pos(s0[i]) && is_finite(r)) {
                    const double a = p.vol_weight[k0 + i];
                    num = num + a * (r * r);
                    den = den + a;
                    bad = bad || !(a >= 0.0 && a < __builtin_inf());
                    ++cnt;
                }
                s1 = s0[i];
            }
        }
        const double q = num / den;
        p.sigma[j] = (cnt >= p.min_returns && !bad && finite_pos(q)) ? sqrt(q) : qnan();
    }
}

__global__ __launch_bounds__(RK_BLOCK) void hsim_wtail_kernel(WTailParams p) {
#pragma clang fp contract(off)
    __shared__ double row[HS_MAX_WINDOW];                                // z, NaN where not ranked
    __shared__ __attribute__((aligned(16))) double zr[HS_MAX_WINDOW];    // z by rank
    __shared__ __attribute__((aligned(16))) double wr[HS_MAX_WINDOW];    // w by rank
    __shared__ double part[HS_MAX_WINDOW / RK_BLOCK][2][RK_WAVES];       // per pass: the wavefronts' sums of w and of w w
    __shared__ int32_t cnt[RK_WAVES];
    __shared__ int32_t first_s;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t b = blockIdx.x;
    const int W = p.window, nL = p.nL;
    const bool scaled = p.sigma != nullptr;
    const double sig_p = scaled ? p.sigma[b] : 1.0;
    const bool sig_p_ok = finite_pos(sig_p);

    // W3-W5: the row, its new bits, and the masses in the layout of B5
    int32_t mine = 0;
    for (int s = tid, ps = 0; s - tid < W; s += RK_BLOCK, ++ps) {        // whole wavefronts go round together
        const bool in = s < W;
        bool ok = false;
        double w = 0.0;
        if (in) {
            const int64_t at = b * W + s;
            const double v = p.pnl[at];
            const int32_t fl = p.scen_flags[at];
            w = p.weight ? p.weight[s] : 1.0;
            int32_t bits = 0;
            double f = 1.0, z = v;
            if (scaled) {
                const int64_t j = b - p.lag - s;                         // H0: the scenario's start
                const double sig_j = j >= 0 ? p.sigma[j] : qnan();
                if (sig_p_ok && finite_pos(sig_j)) {
                    f = sig_p / sig_j;
                    f = fmin(fmax(f, p.cap_lo), p.cap);                  // both operands are numbers
                    z = v * f;
                } else {
                    bits = IVS_HW_NO_VOL;
                    f = qnan();
                }
            }
            const bool w_ok = w >= 0.0 && w < __builtin_inf();
            bits |= w_ok ? 0 : IVS_HW_BAD_WEIGHT;
            ok = fl == 0 && bits == 0 && z == z;
            row[s] = ok ? z : qnan();
            p.flags_w[at] = fl | bits;
            if (p.pnl_w) p.pnl_w[at] = ok ? z : qnan();
            if (p.scale) p.scale[at] = f;
        }
        mine += __popcll(__ballot(ok));
        const double x = ok ? w : 0.0;
        const double sw = rk_wave_sum(x), sw2 = rk_wave_sum(x * x);
        if (lane == 0) { part[ps][0][wave] = sw; part[ps][1][wave] = sw2; }
    }
    if (lane == 0) cnt[wave] = mine;
    if (tid == 0) first_s = -1;
    __syncthreads();
    const int n = cnt[0] + cnt[1] + cnt[2] + cnt[3];
    double Wm = 0.0, W2 = 0.0;
    for (int ps = 0; ps * RK_BLOCK < W; ++ps) {                          // B5: the passes in turn from +0.0
        Wm = Wm + rk_four([&](int k) { return part[ps][0][k]; });
        W2 = W2 + rk_four([&](int k) { return part[ps][1][k]; });
    }

    // W4: H7's order on z; z and w go to their rank
    for (int s = tid; s < W; s += RK_BLOCK) {
        const double v = row[s];
        if (!(v == v)) continue;
        int r = 0;
        for (int i = 0; i < W; ++i) {                                    // uniform LDS addresses; -0.0 == +0.0: the lower s first
            const double u = row[i];
            r += (u < v || (u == v && i < s)) ? 1 : 0;
        }
        zr[r] = v;
        wr[r] = p.weight ? p.weight[s] : 1.0;
        if (r == 0) first_s = s;
    }
    __syncthreads();
    if (tid == 0) {
        p.n_valid_w[b] = n;
        p.worst_w[b] = first_s;
        p.wsum[b] = Wm;
        p.n_eff[b] = W2 > 0.0 ? (Wm * Wm) / W2 : qnan();
    }
    if (tid < nL) {                                                      // W7: lane = level
        double var = qnan(), es = qnan();
        if (n >= p.min_scen && n > 0 && finite_pos(Wm)) {                // W6
            const double target = p.tp[tid] * Wm;
            double cum = 0.0, sum = 0.0, zs = 0.0;
            bool done = false;
            // a rank at or past the boundary, or past n, leaves cum, sum and zs as they are: selects, no branch
            auto step = [&](int q, double z, double w) {
                const double next = cum + w;
                const bool live = !done && q < n;
                const bool hit = live && next >= target;
                const bool go = live && !hit;
                sum = go ? sum + w * z : sum;
                cum = go ? next : cum;
                zs = live ? z : zs;                                      // the boundary's z, or rank n - 1's when no rank reaches the target
                done = done || hit;
            };
            for (int q = 0; q < n && !done; q += 4) {                    // the arrays hold a multiple of four; past n they hold garbage, which step() ignores
                const double2 za = *reinterpret_cast<const double2*>(zr + q), zb = *reinterpret_cast<const double2*>(zr + q + 2);
                const double2 wa = *reinterpret_cast<const double2*>(wr + q), wb = *reinterpret_cast<const double2*>(wr + q + 2);
                step(q, za.x, wa.x); step(q + 1, za.y, wa.y); step(q + 2, zb.x, wb.x); step(q + 3, zb.y, wb.y);
            }
            sum = sum + (target - cum) * zs;
            var = 0.0 - zs;
            es = 0.0 - sum / target;
        }
        p.var_w[b * nL + tid] = var;
        p.es_w[b * nL + tid] = es;
    }
}

}  // namespace ivs
