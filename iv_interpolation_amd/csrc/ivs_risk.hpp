// Book risk off the raw SVI slices (rules G0-G6, B1-B5): smile-aware Greeks per option and, over a book
// of options, net Greeks and a scenario P&L grid per snapshot.  Both kernels read params [B][mT][5], the tenors, the spots and
// Q options (u, tau, side) per snapshot, and place an option on the surface as svi_eval_kernel does (rules T1-T3, E1-E3 of
// section 14): the slices are staged by st_stage and the option is bracketed by st_bracket of ivs_svi_surface.hpp, the very
// functions svi_eval_kernel calls.  The arithmetic on the bracket (rk_locate's weight, rk_w012, rk_surface) is this file's own
// on account of rule B4 below.
//
// svi_greeks_kernel: the shape of svi_eval_kernel: a block takes one snapshot and 256 options, lane = option, the snapshot's
// mT x 6 doubles staged in LDS once and read at uniform addresses.  An output left out is skipped with its arithmetic.
//
// svi_book_kernel: a workgroup of four wavefronts owns one snapshot and a run of at most 256 scenario cells (a cell = one
// spot shock x one vol shock; the runs of a snapshot are spread over the grid).  The options pass through it 256 at a time,
// lane = option.  Per option the surface is evaluated once and the sticky-strike vol once, the sticky-moneyness curve once per
// spot shock, two prices per cell and dynamic.  Rule B5: the 256 terms of a cell meet in a fixed order: an xor butterfly
// (32, 16, 8, 4, 2, 1) inside each wavefront, the four wavefront sums through LDS as (s0 + s1) + (s2 + s3), and the sums of
// successive 256-option passes serially in the register of the thread that owns the cell.  No atomics; the order depends on Q
// alone, not on B, the run length or the block that took the cell.
//
// Rule B4: every function below is compiled with floating-point contraction off, so that each of its operations is rounded on
// its own: the base price of an option and the price of a cell with a zero spot shock and a zero vol shock are then the same
// sequence of IEEE operations on the same operands and give the same bits wherever the compiler inlines them.
#pragma once
#include "ivs_svi_surface.hpp"

namespace ivs {

constexpr int RK_BLOCK = 256;          // options per pass / per block of the Greeks kernel
constexpr int RK_WAVES = RK_BLOCK / 64;
constexpr int RK_MAX_CELLS = 256;      // scenario cells per workgroup: one per thread
constexpr int RK_MAX_SHOCKS = 64;      // per axis: the shocks travel in the kernel's arguments
constexpr int RK_MAX_GRID = 1024;      // nA * nV
constexpr int RK_NET = 8;

enum : unsigned { RK_PRICE = 1, RK_DSS = 2, RK_DSM = 4, RK_GSS = 8, RK_GSM = 16, RK_VEGA = 32, RK_THETA = 64, RK_ALL = 127 };

struct RiskParams {
    const double* params; const double* Tq; const double* spot;
    const double* u; const double* tau; const uint8_t* is_put;
    int64_t tq_stride, q_stride;                         // 0 = shared
    double rate;
    int32_t mT, strike_mode, nqb;                        // nqb = blocks per snapshot
    int64_t Q;
    double* out[7];                                      // price, delta_ss, delta_sm, gamma_ss, gamma_sm, vega, theta: [B][Q], each may be null
    int32_t* flags;                                      // [B][Q]
};

struct BookParams {
    const double* params; const double* Tq; const double* spot;
    const double* u; const double* tau; const uint8_t* is_put; const double* qty;
    int64_t tq_stride, q_stride;
    double rate;
    int32_t mT, strike_mode, nA, nV, cpb, nchunk;        // cpb = cells per workgroup, nchunk = workgroups per snapshot
    int64_t Q;
    double a[RK_MAX_SHOCKS], v[RK_MAX_SHOCKS];
    double* net; int32_t* n_dead;                        // [B][8], [B]
    double* pnl_ss; double* pnl_sm; int32_t* cell_flags; // [B][nA][nV]; the two values may be null
};

// where an option sits on the surface: rules E1-E3
struct RkPoint {
    double K, x, rt, D;
    double tl, th_;                                      // tenors of the bracket (SHORT / LONG: tl alone)
    double lam;                                          // E3's weight, or tau / tenor under SHORT / LONG
    int lo, hi;                                          // LDS rows; hi < 0 under SHORT / LONG
    int32_t fl;
    bool ok;
};

// rule T3: w alone
__device__ __forceinline__ double rk_w(const double* r, double x) {
#pragma clang fp contract(off)
    const double dx = x - r[3];
    return r[0] + r[1] * (r[2] * dx + sqrt(dx * dx + r[4] * r[4]));
}

__device__ __forceinline__ void rk_w012(const double* r, double x, double& w, double& w1, double& w2) {
#pragma clang fp contract(off)
    const double dx = x - r[3];
    const double s2 = r[4] * r[4];
    const double rr = sqrt(dx * dx + s2);
    w = r[0] + r[1] * (r[2] * dx + rr);
    w1 = r[1] * (r[2] + dx / rr);
    w2 = r[1] * s2 / (rr * rr * rr);
}

// st_bracket's T2 and E2, then rule E1 and the weight of E3; `unordered` and `any` are the snapshot's
__device__ __forceinline__ RkPoint rk_locate(const double* sl, int mT, double S, double u, double tq, double rate, int strike_mode,
                                             bool& unordered, bool& any) {
#pragma clang fp contract(off)
    RkPoint pt;
    int lo, hi;
    st_bracket(sl, mT, tq, lo, hi, unordered, any);
    pt.ok = !unordered && finite_pos(u) && finite_pos(tq) && finite_pos(S) && any;
    pt.fl = unordered ? IVS_SE_UNORDERED : (pt.ok ? 0 : IVS_SE_DEAD);
    pt.K = pt.x = pt.rt = pt.D = pt.tl = pt.th_ = pt.lam = qnan();
    pt.lo = 0; pt.hi = -1;
    if (pt.ok) {
        pt.K = strike_mode == 0 ? S * u : u;
        pt.rt = rate * tq;
        pt.D = exp(-pt.rt);
        pt.x = log(pt.K / S) - pt.rt;
        if (lo >= 0 && hi >= 0) {
            pt.lo = lo; pt.hi = hi;
            pt.tl = sl[lo * 6 + 5]; pt.th_ = sl[hi * 6 + 5];
            pt.lam = (tq - pt.tl) / (pt.th_ - pt.tl);
        } else {
            pt.lo = lo >= 0 ? lo : hi;
            pt.fl |= lo >= 0 ? IVS_SE_LONG : IVS_SE_SHORT;
            pt.tl = sl[pt.lo * 6 + 5];
            pt.lam = tq / pt.tl;
        }
    }
    return pt;
}

// rule E3: W at x with the option's bracket and weight
__device__ __forceinline__ double rk_W(const double* sl, const RkPoint& pt, double x) {
#pragma clang fp contract(off)
    const double wl = rk_w(sl + pt.lo * 6, x);
    if (pt.hi >= 0) {
        const double wh = rk_w(sl + pt.hi * 6, x);
        return wl + (wh - wl) * pt.lam;
    }
    return wl * pt.lam;
}

// the vol at x with a placement's bracket and weight: every vol of the book, explain (X1) and hsim (H2) kernels comes from here
__device__ __forceinline__ double rk_sigma(const double* sl, const RkPoint& pt, double x, double tq) {
#pragma clang fp contract(off)
    return sqrt(rk_W(sl, pt, x) / tq);
}

// rule E3: W, W', W'' and V at the option's own x
__device__ __forceinline__ void rk_surface(const double* sl, const RkPoint& pt, double& W, double& W1, double& W2, double& V) {
#pragma clang fp contract(off)
    double wl, wl1, wl2;
    rk_w012(sl + pt.lo * 6, pt.x, wl, wl1, wl2);
    if (pt.hi >= 0) {
        double wh, wh1, wh2;
        rk_w012(sl + pt.hi * 6, pt.x, wh, wh1, wh2);
        W = wl + (wh - wl) * pt.lam;
        W1 = wl1 + (wh1 - wl1) * pt.lam;
        W2 = wl2 + (wh2 - wl2) * pt.lam;
        V = (wh - wl) / (pt.th_ - pt.tl);
    } else {
        W = wl * pt.lam; W1 = wl1 * pt.lam; W2 = wl2 * pt.lam;
        V = wl / pt.tl;
    }
}

// norm_cdf and norm_pdf of ivs_device.hpp, the same operations, here with contraction off like everything round them
__device__ __forceinline__ double rk_cdf(double x) {
#pragma clang fp contract(off)
    return 0.5 * erfc(-x * 0.70710678118654752440);
}
__device__ __forceinline__ double rk_pdf(double x) {
#pragma clang fp contract(off)
    return exp(-x * x * 0.5) * 0.39894228040143267794;
}

// rule G1 at (S, x, theta); KD = K D
__device__ __forceinline__ double rk_price(double S, double KD, double x, double th, bool put) {
#pragma clang fp contract(off)
    const double d1 = -x / th + 0.5 * th, d2 = d1 - th;
    return put ? KD * rk_cdf(-d2) - S * rk_cdf(-d1) : S * rk_cdf(d1) - KD * rk_cdf(d2);
}

// rules G0-G5; o[] = price, delta_ss, delta_sm, gamma_ss, gamma_sm, vega, theta.  Only the entries named in `want` are formed.
__device__ __forceinline__ void rk_greeks(unsigned want, double S, double K, double D, double x, double tq, double rate, double W,
                                          double W1, double W2, double V, bool put, double* o) {
#pragma clang fp contract(off)
    const double th = sqrt(W);
    const double d1 = -x / th + 0.5 * th, d2 = d1 - th;
    const double KD = K * D;
    if (want & RK_PRICE) o[0] = rk_price(S, KD, x, th, put);
    double dss = 0.0, pdf = 0.0, th1 = 0.0;
    if (want & (RK_DSS | RK_DSM)) dss = put ? -rk_cdf(-d1) : rk_cdf(d1);
    if (want & (RK_DSM | RK_GSS | RK_GSM | RK_VEGA | RK_THETA)) pdf = rk_pdf(d1);
    if (want & (RK_DSM | RK_GSM)) th1 = W1 / (2.0 * th);
    if (want & RK_DSS) o[1] = dss;
    if (want & RK_DSM) o[2] = dss - pdf * th1;
    if (want & RK_GSS) o[3] = pdf / (S * th);
    if (want & RK_GSM) {
        const double th2 = W2 / (2.0 * th) - W1 * W1 / (4.0 * th * th * th);
        const double d1x = -1.0 / th + (x / (th * th) + 0.5) * th1;
        const double d2x = d1x - th1;
        o[4] = pdf * (-d2x - d1 * d1x * th1 + th2 - th1) / S;
    }
    if (want & RK_VEGA) o[5] = S * pdf * sqrt(tq);
    if (want & RK_THETA) {
        const double ex = KD / S;
        const double carry = put ? -rate * ex * rk_cdf(-d2) : rate * ex * rk_cdf(d2);
        o[6] = -S * (carry + pdf * (V - rate * W1) / (2.0 * th));
    }
}

__global__ __launch_bounds__(RK_BLOCK) void svi_greeks_kernel(RiskParams p) {
    __shared__ double sl[ST_MAX_T * 6];
    const int64_t b = blockIdx.x / p.nqb;
    const int qb = (int)(blockIdx.x - b * p.nqb);
    const double S = p.spot[b];
    st_stage(sl, p.params, p.Tq, p.tq_stride, b, p.mT, S);
    __syncthreads();
    const int64_t q = (int64_t)qb * RK_BLOCK + threadIdx.x;
    if (q >= p.Q) return;
    const double u = p.u[b * p.q_stride + q], tq = p.tau[b * p.q_stride + q];
    const bool put = p.is_put ? p.is_put[q] != 0 : false;
    bool unordered, any;
    const RkPoint pt = rk_locate(sl, p.mT, S, u, tq, p.rate, p.strike_mode, unordered, any);
    unsigned want = 0;
    for (int k = 0; k < 7; ++k) want |= p.out[k] ? 1u << k : 0u;
    double o[7];
    for (int k = 0; k < 7; ++k) o[k] = qnan();
    int32_t fl = pt.fl;
    if (pt.ok) {
        double W, W1, W2, V;
        rk_surface(sl, pt, W, W1, W2, V);
        if (V < 0.0) fl |= IVS_SE_NEG_FWD;
        rk_greeks(want, S, pt.K, pt.D, pt.x, tq, p.rate, W, W1, W2, V, put, o);
    }
    const int64_t at = b * p.Q + q;                                      // consecutive lanes, consecutive elements
    for (int k = 0; k < 7; ++k)
        if (p.out[k]) p.out[k][at] = o[k];
    p.flags[at] = fl;
}

// rule B5, first level: the sum over the 64 lanes of a wavefront, the same bits in every lane
__device__ __forceinline__ double rk_wave_sum(double v) {
#pragma clang fp contract(off)
    for (int s = 32; s > 0; s >>= 1) v = v + __shfl_xor(v, s);
    return v;
}

// rule B5, second level: what the four wavefronts left in LDS, s(w) = wavefront w's entry, as (s0 + s1) + (s2 + s3)
template <class F>
__device__ __forceinline__ double rk_four(F s) {
#pragma clang fp contract(off)
    return (s(0) + s(1)) + (s(2) + s(3));
}
template <class F>
__device__ __forceinline__ int32_t rk_four_or(F s) {
#pragma clang fp contract(off)
    return s(0) | s(1) | s(2) | s(3);
}

// option q of a book as lane q % 256 of a pass sees it: NaN, a zero quantity and a call beyond Q
struct RkOption {
    double u, tau, qty;
    bool valid, put;
    // G0: a quantity that is not finite kills the option; ok = every placement of it is
    __device__ __forceinline__ bool live(bool ok) const {
#pragma clang fp contract(off)
        return valid && ok && qty - qty == 0.0;
    }
};

template <class P>
__device__ __forceinline__ RkOption rk_option(const P& p, int64_t b, int64_t q) {
#pragma clang fp contract(off)
    RkOption o;
    o.valid = q < p.Q;
    o.u = o.valid ? p.u[b * p.q_stride + q] : qnan();
    o.tau = o.valid ? p.tau[b * p.q_stride + q] : qnan();
    o.qty = o.valid ? p.qty[q] : 0.0;
    o.put = o.valid && p.is_put ? p.is_put[q] != 0 : false;
    return o;
}

// the dead options of a pass: each wavefront counts its own into dpart, and after a barrier every thread has the pass's count
__device__ __forceinline__ void rk_dead_part(int32_t* dpart, int wave, int lane, bool dead) {
#pragma clang fp contract(off)
    const unsigned long long dm = __ballot(dead);
    if (lane == 0) dpart[wave] = __popcll(dm);
}
__device__ __forceinline__ int32_t rk_dead_sum(const int32_t* dpart) {
#pragma clang fp contract(off)
    return dpart[0] + dpart[1] + dpart[2] + dpart[3];
}

__global__ __launch_bounds__(RK_BLOCK) void svi_book_kernel(BookParams p) {
#pragma clang fp contract(off)
    __shared__ double sl[ST_MAX_T * 6];
    __shared__ double part[RK_WAVES][RK_MAX_CELLS][2];                   // wavefront sums per cell and dynamic
    __shared__ int32_t pflag[RK_WAVES][RK_MAX_CELLS];
    __shared__ double npart[RK_WAVES][RK_NET];
    __shared__ int32_t dpart[RK_WAVES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t b = blockIdx.x / p.nchunk;
    const int ch = (int)(blockIdx.x - b * p.nchunk);
    const int ncell = p.nA * p.nV;
    const int c0 = ch * p.cpb;
    const int nc = ncell - c0 < p.cpb ? ncell - c0 : p.cpb;              // <= RK_MAX_CELLS; 0 without a grid
    const bool first = ch == 0;                                          // this workgroup also owns net and n_dead
    const double S = p.spot[b];
    st_stage(sl, p.params, p.Tq, p.tq_stride, b, p.mT, S);
    __syncthreads();

    double tot_ss = 0.0, tot_sm = 0.0, ntot = 0.0;                       // thread t: cell c0 + t; thread k < 8: net figure k
    int32_t tflag = 0, dead = 0;
    bool degenerate = false;
    for (int64_t q0 = 0; q0 < p.Q; q0 += RK_BLOCK) {
        const RkOption opt = rk_option(p, b, q0 + tid);
        const double tq = opt.tau, qty = opt.qty;
        const bool put = opt.put;
        bool unordered, any;
        const RkPoint pt = rk_locate(sl, p.mT, S, opt.u, tq, p.rate, p.strike_mode, unordered, any);
        degenerate = unordered || !any;                                  // the snapshot's: the same in every thread and pass
        const bool live = opt.live(pt.ok);
        rk_dead_part(dpart, wave, lane, opt.valid && !live);

        if (first) {                                                     // B1
            double o[RK_NET];
            for (int k = 0; k < RK_NET; ++k) o[k] = 0.0;
            if (live) {
                double W, W1, W2, V;
                rk_surface(sl, pt, W, W1, W2, V);
                rk_greeks(RK_ALL, S, pt.K, pt.D, pt.x, tq, p.rate, W, W1, W2, V, put, o);
                o[7] = fabs(qty) * o[0];
                for (int k = 0; k < 7; ++k) o[k] = qty * o[k];
            }
            for (int k = 0; k < RK_NET; ++k) {
                const double s = rk_wave_sum(o[k]);
                if (lane == 0) npart[wave][k] = s;
            }
        }

        // B2: the option's own state; the base goes through the code of a cell with both shocks zero (B4)
        const double KD = pt.K * pt.D;
        const double sqt = sqrt(tq);
        const double sig0 = rk_sigma(sl, pt, pt.x, tq);
        double base_ss = 0.0, base_sm = 0.0;
        {
            const double S1 = S * (1.0 + 0.0);
            const double x1 = log(pt.K / S1) - pt.rt;
            if (p.pnl_ss) base_ss = rk_price(S1, KD, x1, (sig0 + 0.0) * sqt, put);
            if (p.pnl_sm) base_sm = rk_price(S1, KD, x1, (rk_sigma(sl, pt, x1, tq) + 0.0) * sqt, put);
        }
        int i = nc > 0 ? c0 / p.nV : 0;
        int k = nc > 0 ? c0 - i * p.nV : 0;
        double S1 = 0.0, x1 = 0.0, sig1 = 0.0;
        for (int c = 0; c < nc; ++c) {
            if (c == 0 || k == 0) {                                      // a new spot shock: the sticky-moneyness curve once
                S1 = S * (1.0 + p.a[i]);
                x1 = log(pt.K / S1) - pt.rt;
                if (p.pnl_sm) sig1 = rk_sigma(sl, pt, x1, tq);
            }
            const double v = p.v[k];
            double s_ss = 0.0, s_sm = 0.0;
            int32_t f = 0;
            if (p.pnl_ss) {
                const double sg = sig0 + v;
                const double pr = rk_price(S1, KD, x1, sg * sqt, put);
                s_ss = rk_wave_sum(live ? qty * (pr - base_ss) : 0.0);
                if (__ballot(live && sg <= 0.0) != 0ull) f |= IVS_SB_NEG_VOL_SS;
            }
            if (p.pnl_sm) {
                const double sg = sig1 + v;
                const double pr = rk_price(S1, KD, x1, sg * sqt, put);
                s_sm = rk_wave_sum(live ? qty * (pr - base_sm) : 0.0);
                if (__ballot(live && sg <= 0.0) != 0ull) f |= IVS_SB_NEG_VOL_SM;
            }
            if (lane == 0) { part[wave][c][0] = s_ss; part[wave][c][1] = s_sm; pflag[wave][c] = f; }
            if (++k == p.nV) { k = 0; ++i; }
        }
        __syncthreads();
        if (tid < nc) {                                                  // B5: rk_four, then the passes in turn
            tot_ss = tot_ss + rk_four([&](int w) { return part[w][tid][0]; });
            tot_sm = tot_sm + rk_four([&](int w) { return part[w][tid][1]; });
            tflag |= rk_four_or([&](int w) { return pflag[w][tid]; });
        }
        if (first && tid < RK_NET) ntot = ntot + rk_four([&](int w) { return npart[w][tid]; });
        dead += rk_dead_sum(dpart);
        __syncthreads();
    }

    if (tid < nc) {                                                      // B3
        const int64_t at = b * ncell + c0 + tid;
        if (p.pnl_ss) p.pnl_ss[at] = degenerate || (tflag & IVS_SB_NEG_VOL_SS) ? qnan() : tot_ss;
        if (p.pnl_sm) p.pnl_sm[at] = degenerate || (tflag & IVS_SB_NEG_VOL_SM) ? qnan() : tot_sm;
        p.cell_flags[at] = tflag;
    }
    if (first && tid < RK_NET) p.net[b * RK_NET + tid] = degenerate ? qnan() : ntot;
    if (first && tid == 0) p.n_dead[b] = degenerate ? (int32_t)p.Q : dead;
}

}  // namespace ivs
