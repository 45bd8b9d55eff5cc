// Risk-neutral distribution off the raw SVI slices (rules P1-P8): per row (b, j) of params [B][mT][5]
// the quantiles x* = ln(K / F) of nP probabilities, the probabilities below / above nL moneyness levels and the two tails
// of the scan grid, from the closed-form CDF L(x) = Phi(-d2) + phi(d2) theta'(x) of the slice w(x) = a + b (rho (x - m) +
// sqrt((x - m)^2 + sigma^2)), theta = sqrt(w), d2 = -x / theta - theta / 2.
//
// One wavefront owns `group` consecutive rows (group * nP <= 64).  Scan phase, row after row: lane = grid point of rule P4,
// L and U once per lane; the next lane's pair comes by a lane permute (lane 63 has no pair).  Per target one ballot of "own
// h < 0 and the next lane's h >= 0": its lowest set bit is the bracket, its popcount the crossing count.  Lane g*nP + t keeps
// (index, count) of (row g, target t); lanes 0 and 63 store the tails, lane 0 the row flag, lanes l < nL evaluate the levels.
// Inversion phase, once: the group's <= 64 (row, target) pairs bisect side by side, one lane each, one erfc per step, and
// consecutive lanes store consecutive output elements.  No LDS, no atomics, no scratch; probabilities and levels travel in
// the kernel arguments and are read with uniform indices.  A result depends neither on `group` nor on the wavefront that
// took the row: every value is a function of the row's inputs and the grid index alone.
#pragma once
#include "ivs_device.hpp"
#include "ivs_bs_formulas.hpp"

namespace ivs {

constexpr int DS_MAX_P = 16;     // probabilities per call
constexpr int DS_MAX_L = 16;     // levels per call
constexpr int DS_WAVES = 4;      // wavefronts per workgroup
constexpr int DS_STEPS = 52;     // rule P6: bisection steps

struct DistParams {
    const double* params; const double* Tq; const double* spot;
    int64_t tq_stride;                                   // 0 = shared
    double rate, max_tail;
    double probs[DS_MAX_P];
    double levels[DS_MAX_L];
    int32_t mT, nP, nL, group;                           // group = rows per wavefront, group * nP <= 64
    int64_t rows;                                        // B * mT
    double* q_x; double* q_strike; int32_t* q_flags;     // [rows][nP]
    double* p_below; double* p_above;                    // [rows][nL], null with nL == 0
    double* tails; int32_t* flags;                       // [rows][2], [rows]
};

struct DistRow { double a, b, rho, m, sig; };

// rule P1
__device__ __forceinline__ bool ds_live(const DistRow& r, double S, double tau) {
    if (!(finite_pos(S) && finite_pos(tau) && is_finite(r.a) && is_finite(r.b) && is_finite(r.rho) && is_finite(r.m) &&
          is_finite(r.sig)))
        return false;
    if (!(r.b >= 0.0 && __builtin_fabs(r.rho) <= 1.0 && r.sig > 0.0)) return false;
    return r.a + r.b * r.sig * sqrt(1.0 - r.rho * r.rho) > 0.0;
}

// rule P4: the grid in units of s0, exact in fp64
__device__ __forceinline__ double ds_y(int i) {
    const double j = (double)i - 31.5;
    return j * (1.0 + j * j / 64.0) / 8.0;
}

// rule P4: s0 = sqrt(w(0))
__device__ __forceinline__ double ds_s0(const DistRow& r) {
    const double dx = 0.0 - r.m;
    return sqrt(r.a + r.b * (r.rho * dx + sqrt(dx * dx + r.sig * r.sig)));
}

// rule P2: d2 and t = phi(d2) theta' at x
__device__ __forceinline__ void ds_terms(const DistRow& r, double x, double& d2, double& t) {
    const double dx = x - r.m;
    const double rr = sqrt(dx * dx + r.sig * r.sig);
    const double w = r.a + r.b * (r.rho * dx + rr);
    const double w1 = r.b * (r.rho + dx / rr);
    const double th = sqrt(w);
    const double th1 = w1 / (2.0 * th);
    d2 = -x / th - 0.5 * th;
    t = norm_pdf(d2) * th1;
}

// rule P2: L and U
__device__ __forceinline__ void ds_eval(const DistRow& r, double x, double& L, double& U) {
    double d2, t;
    ds_terms(r, x, d2, t);
    L = norm_cdf(-d2) + t;
    U = norm_cdf(d2) - t;
}

// rule P3 from a pair (L, U)
__device__ __forceinline__ double ds_h(double L, double U, double p) { return p <= 0.5 ? L - p : (1.0 - p) - U; }

// rule P3 at x, the one form the target needs: ds_h(ds_eval) in value; FMA contraction may round the two differently, and
// nothing compares one with the other (the bisection only ever looks at its own h)
__device__ __forceinline__ double ds_h_at(const DistRow& r, double x, double p) {
    double d2, t;
    ds_terms(r, x, d2, t);
    const bool lower = p <= 0.5;
    const double c = norm_cdf(lower ? -d2 : d2);
    return lower ? (c + t) - p : (1.0 - p) - (c - t);
}

__global__ __launch_bounds__(DS_WAVES * 64) void svi_distribution_kernel(DistParams p) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t row0 = ((int64_t)blockIdx.x * DS_WAVES + wave) * p.group;
    if (row0 >= p.rows) return;                                          // the whole wavefront
    const int ng = (int)((p.rows - row0) < p.group ? (p.rows - row0) : p.group);
    const int my_g = lane / p.nP, my_t = lane - my_g * p.nP;             // this lane's slot: row row0 + my_g, target my_t

    double my_p = 0.5, my_lv = 1.0;
    for (int t = 0; t < p.nP; ++t)
        if (my_t == t) my_p = p.probs[t];
    for (int l = 0; l < p.nL; ++l)
        if (lane == l) my_lv = p.levels[l];
    const double my_loglv = log(my_lv);
    const double y = ds_y(lane);
    int32_t idx = 0, cnt = 0;                                            // bracket and crossings of the slot
    bool dead = true;

    for (int g = 0; g < ng; ++g) {
        const int64_t row = row0 + g;
        const int64_t b = row / p.mT;
        const int j = (int)(row - b * p.mT);
        const double S = p.spot[b], tau = p.Tq[b * p.tq_stride + j];
        const double* pr = p.params + row * 5;
        const DistRow r{pr[0], pr[1], pr[2], pr[3], pr[4]};
        const bool live = ds_live(r, S, tau);                            // P1; uniform over the wavefront
        double L = qnan(), U = qnan(), Lv = qnan(), Uv = qnan();
        if (live) {
            ds_eval(r, ds_s0(r) * y, L, U);                              // P4
            if (lane < p.nL) ds_eval(r, my_loglv - p.rate * tau, Lv, Uv);   // P7
        }
        const int nx = lane < 63 ? lane + 1 : 63;
        const double Ln = __shfl(L, nx), Un = __shfl(U, nx);
        for (int t = 0; t < p.nP; ++t) {
            const double pt = p.probs[t];
            const unsigned long long cm = __ballot(lane < 63 && ds_h(L, U, pt) < 0.0 && ds_h(Ln, Un, pt) >= 0.0);   // P5
            if (lane == g * p.nP + t) {
                idx = cm ? __builtin_ctzll(cm) : 0;
                cnt = __popcll(cm);
            }
        }
        if (my_g == g) dead = !live;
        const double t_hi = __shfl(U, 63);
        if (lane == 0) {                                                 // P8
            p.tails[row * 2] = L;
            p.flags[row] = !live ? IVS_DS_DEAD
                                 : ((__builtin_fabs(L) > p.max_tail || __builtin_fabs(t_hi) > p.max_tail) ? IVS_DS_TAILS : 0);
        }
        if (lane == 63) p.tails[row * 2 + 1] = U;
        if (lane < p.nL) {
            p.p_below[row * p.nL + lane] = Lv;
            p.p_above[row * p.nL + lane] = Uv;
        }
    }

    if (lane >= ng * p.nP) return;
    double qx = qnan(), qk = qnan();
    int32_t fl = IVS_DS_DEAD;
    if (!dead) {
        fl = cnt == 0 ? IVS_DS_NO_BRACKET : (cnt > 1 ? IVS_DS_AMBIGUOUS : 0);
        if (cnt > 0) {                                                   // P6
            const int64_t row = row0 + my_g;
            const int64_t b = row / p.mT;
            const int j = (int)(row - b * p.mT);
            const double S = p.spot[b], tau = p.Tq[b * p.tq_stride + j];
            const double* pr = p.params + row * 5;
            const DistRow r{pr[0], pr[1], pr[2], pr[3], pr[4]};
            const double s0 = ds_s0(r);
            double lo = s0 * ds_y(idx), hi = s0 * ds_y(idx + 1);
            for (int it = 0; it < DS_STEPS; ++it) {
                const double mid = 0.5 * (lo + hi);
                if (ds_h_at(r, mid, my_p) < 0.0) lo = mid; else hi = mid;
            }
            qx = 0.5 * (lo + hi);
            qk = S * exp(p.rate * tau) * exp(qx);
        }
    }
    const int64_t o = row0 * p.nP + lane;                                // every element, consecutive lanes
    p.q_x[o] = qx;
    p.q_strike[o] = qk;
    p.q_flags[o] = fl;
}

}  // namespace ivs
