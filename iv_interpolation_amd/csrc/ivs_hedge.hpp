// Minimum-variance hedge of a book over its historical scenarios (rules M0-M11): which of up to 64
// candidate instruments (the underlying and options), in which sizes, remove the most of the variance of the book's scenario P&L
// row of section 19, in at most 8 steps of an orthogonal matching pursuit (pivoted modified Gram-Schmidt: nothing is inverted).
//
// svi_inst_pnl_kernel (M2): the structure of svi_hsim_kernel with lane = candidate and no sum.  A workgroup is ONE wavefront: it
// owns snapshot p and a run of scenarios, stages today's slices once, forms every candidate's own state (its bracket on p, K D,
// sqrt(tau) and H3's base price) once and keeps it in registers while the scenarios of the run go by.  The ends of a scenario are
// staged into svi_hsim_kernel's ring of four slice buffers, and with lag == 1 the end of scenario s is the start of scenario s - 1:
// it is then neither staged nor bracketed again.  Several such workgroups share a CU, which is how several scenarios run at once.
// A candidate's P&L is svi_hsim_kernel's term at quantity 1.0 through the same device functions in the same order (rk_locate,
// rk_sigma, rk_price).  inst_pnl is scenario-major: a wavefront writes one whole row per scenario.
//
// hedge_pursuit_kernel (M1, M3-M10): one wavefront per snapshot.  The residual e and the directions v_k live in LDS, (K + 1) x
// window doubles, sized by the call.  The serial sums over the scenarios run with lane = candidate over coalesced rows of
// inst_pnl (one pass per round yields p, a and E together); the row updates run with lane = scenario.  The round loops are fully
// unrolled, so p_hj sits in registers under static indices.  The pick is a fixed xor butterfly, ties to the lower candidate.
// The tail of the hedged row is hsim_tail_kernel, launched as it is.
//
// Contraction is off throughout (B4): every product and every sum is rounded on its own, in the order the rules give.
#pragma once
#include "ivs_hsim.hpp"

namespace ivs {

constexpr int HG_MAX_INST = 64;        // candidates: one per lane
constexpr int HG_MAX_ROUNDS = 8;
constexpr int HG_WORDS = HS_MAX_WINDOW / 64;

struct InstPnlParams {
    const double* params; const double* Tq; const double* spot;
    const double* inst_u; const double* inst_tau; const uint8_t* inst_kind;
    int64_t tq_stride, inst_stride;                      // 0 = shared
    double rate;
    int32_t mT, strike_mode, lag, window, nH, spw, nchunk;               // spw = scenarios per workgroup, nchunk = workgroups per snapshot
    double* inst_pnl;                                    // [B][window][nH]
    double* inst_value;                                  // [B][nH], may be null
};

struct PursuitParams {
    const double* params; const double* Tq; const double* spot;
    const double* inst_u; const double* inst_tau; const uint8_t* inst_kind;
    int64_t tq_stride, inst_stride;
    double rate, tol, min_gain;
    int32_t mT, strike_mode, lag, window, nH, K, n_forced, min_scen;
    const double* pnl; const int32_t* scen_flags;        // [B][window]
    const double* inst_pnl;                              // [B][window][nH]
    int32_t* inst_flags;                                 // [B][nH]
    int32_t* pick; double* ss; int32_t* n_rounds;        // [B][K], [B][K+1], [B]
    double* hedge; double* pnl_hedged;                   // [B][nH], [B][window]
    double* solo_qty; double* solo_left;                 // [B][nH], each may be null
};

// candidate `lane` of snapshot b as both kernels see it: its placement on today's slices and whether it is dead there (M3)
struct HgInst {
    RkPoint pt;
    double tq;
    bool has, und, put, dead, degenerate;
};

template <class P>
__device__ __forceinline__ HgInst hg_inst(const P& p, const double* sl, int64_t b, int lane, double S) {
#pragma clang fp contract(off)
    HgInst c;
    c.has = lane < p.nH;
    const int kind = c.has ? p.inst_kind[lane] : 0;
    c.und = c.has && kind == 2;
    c.put = kind == 1;
    const bool opt = c.has && !c.und;
    const double u = opt ? p.inst_u[b * p.inst_stride + lane] : qnan();
    c.tq = opt ? p.inst_tau[b * p.inst_stride + lane] : qnan();
    bool unordered, any;
    c.pt = rk_locate(sl, p.mT, S, u, c.tq, p.rate, p.strike_mode, unordered, any);
    c.degenerate = unordered || !any;                                    // the snapshot's: the same in every lane
    c.dead = c.has && (c.und ? c.degenerate : !c.pt.ok);
    return c;
}

__global__ __launch_bounds__(64) void svi_inst_pnl_kernel(InstPnlParams p) {
#pragma clang fp contract(off)
    __shared__ double sl[ST_MAX_T * 6];                                  // today's slices
    __shared__ double hist[4][ST_MAX_T * 6];                             // the ring of the scenarios' ends
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x / p.nchunk;
    const int ch = (int)(blockIdx.x - b * p.nchunk);
    const int s0 = ch * p.spw;
    const int s1 = p.window - s0 < p.spw ? p.window : s0 + p.spw;        // this workgroup's scenarios: s0 <= s < s1
    const int64_t np64 = b - p.lag + 1;                                  // H0: the scenarios that exist
    const int n_p = np64 < 0 ? 0 : (np64 > p.window ? p.window : (int)np64);
    const bool reuse = p.lag == 1;
    const double S = p.spot[b];
    st_stage(sl, p.params, p.Tq, p.tq_stride, b, p.mT, S);
    __syncthreads();

    const HgInst in = hg_inst(p, sl, b, lane, S);
    const RkPoint pt = in.pt;
    const double tq = in.tq;
    const bool live = in.has && !in.dead;
    // H3: the candidate's own state; the base goes through the code of a scenario with the quotient 1.0 and the change +0.0
    const double KD = pt.K * pt.D;
    const double sqt = sqrt(tq);
    const double S0 = S * 1.0;
    double base;
    {
        const double x1 = log(pt.K / S0) - pt.rt;
        base = rk_price(S0, KD, x1, (rk_sigma(sl, pt, x1, tq) + 0.0) * sqt, in.put);
    }
    if (ch == 0 && p.inst_value && in.has) p.inst_value[b * p.nH + lane] = live ? (in.und ? S0 : base) : qnan();

    double* out = p.inst_pnl + (b * p.window + s0) * p.nH + lane;        // consecutive lanes, consecutive elements
    RkPoint ea;                                                          // the candidate on the start of the previous scenario
    bool una = false, anya = false;
    for (int c = 0; c < s1 - s0; ++c) {
        double x = qnan();
        if (s0 + c < n_p) {
            const int64_t ja = b - p.lag - (s0 + c), jb = ja + p.lag;    // H0
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
            // H1: the pair's, the same in every lane
            const bool vd = una || !anya || unb || !anyb || !finite_pos(Sa) || !finite_pos(Sb) || in.degenerate;
            if (!__builtin_amdgcn_readfirstlane((int)vd)) {
                const double S1 = S * (Sb / Sa);                         // H1: the quotient first
                if (in.und) x = S1 - S0;
                else {
                    const double x1 = log(pt.K / S1) - pt.rt;
                    const double sg = rk_sigma(sl, pt, x1, tq) + (rk_sigma(hist[ib], eb, x1, tq) - rk_sigma(hist[ia], ea, x1, tq));       // H2
                    const double pr = rk_price(S1, KD, x1, sg * sqt, in.put);
                    x = live && sg > 0.0 ? pr - base : qnan();
                }
            }
        }
        if (in.has) out[(int64_t)c * p.nH] = x;
    }
}

// the scenarios of word i that are ranked, as a scalar
__device__ __forceinline__ unsigned long long hg_word(const unsigned long long* rkm, int i) {
    const unsigned long long m = rkm[i];
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)m), hi = __builtin_amdgcn_readfirstlane((unsigned)(m >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(64) void hedge_pursuit_kernel(PursuitParams p) {
#pragma clang fp contract(off)
    extern __shared__ double hg_rows[];                                  // e [window], then v_k [K][window]
    __shared__ double sl[ST_MAX_T * 6];
    __shared__ unsigned long long rkm[HG_WORDS];                         // M1: bit s % 64 of word s / 64 = scenario s is ranked
    __shared__ double s_nu[HG_MAX_ROUNDS], s_t[HG_MAX_ROUNDS], s_R[HG_MAX_ROUNDS][HG_MAX_ROUNDS];
    __shared__ int32_t s_pick[HG_MAX_ROUNDS];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int W = p.window, nW = (W + 63) >> 6;
    const int64_t np64 = b - p.lag + 1;                                  // H0
    const int n_p = np64 < 0 ? 0 : (np64 > W ? W : (int)np64);
    const int64_t row0 = b * W;
    double* e = hg_rows;
    const double S = p.spot[b];
    st_stage(sl, p.params, p.Tq, p.tq_stride, b, p.mT, S);

    int n = 0;                                                           // M1
    for (int i = 0; i < nW; ++i) {
        const int s = i * 64 + lane;
        const bool in = s < W;
        const double y = in ? p.pnl[row0 + s] : qnan();
        const bool ok = in && s < n_p && p.scen_flags[row0 + s] == 0 && y == y;
        const unsigned long long m = __ballot(ok);
        if (lane == 0) rkm[i] = m;
        n += __popcll(m);
        if (in) e[s] = ok ? y : 0.0;
    }
    if (lane < HG_MAX_ROUNDS) s_pick[lane] = -1;
    __syncthreads();
    const bool active = n >= p.min_scen && n > 0;

    const HgInst in = hg_inst(p, sl, b, lane, S);
    const double* xrow = p.inst_pnl + row0 * p.nH + (in.has ? lane : 0);  // lane = candidate: element s * nH of it

    double g0 = 0.0, a0 = 0.0, E0 = 0.0;                                 // M3, M4
    bool bad = false;
    for (int i = 0; i < nW; ++i) {
        const unsigned long long m = hg_word(rkm, i);
        for (int j = 0; j < 64; ++j) {
            if (!((m >> j) & 1ull)) continue;
            const int s = i * 64 + j;
            const double x = in.has ? xrow[(int64_t)s * p.nH] : 0.0, ys = e[s];
            g0 = g0 + x * x;
            a0 = a0 + x * ys;
            E0 = E0 + ys * ys;
            bad = bad || !(x == x);
        }
    }
    int32_t fl = (in.dead ? IVS_HG_DEAD : 0) | (bad ? IVS_HG_NEG_VOL : 0) | (!(g0 > 0.0) ? IVS_HG_FLAT : 0);
    const bool usable = in.has && fl == 0;

    double g = g0, a = a0, Ecur = E0;
    double pj[HG_MAX_ROUNDS];
    bool ne[HG_MAX_ROUNDS];
    bool chosen = false, spent = false, stop = !active;
    int nr = 0;
    if (lane == 0) p.ss[b * (p.K + 1)] = active ? E0 : qnan();
#pragma unroll
    for (int k = 0; k < HG_MAX_ROUNDS; ++k) {
        pj[k] = 0.0;
        ne[k] = false;
        if (k < p.K) {
            int c = -1;
            if (!stop) {
                bool elig = usable && !chosen && !spent;                 // M5
                if (elig && !(g > p.tol * g0)) { spent = true; elig = false; }
                if (k < p.n_forced) {                                    // M6
                    c = (__ballot(elig) >> k) & 1ull ? k : -1;
                } else {
                    const double gain = (a * a) / g;
                    double bv = elig && gain == gain ? gain : -__builtin_inf();
                    int bi = lane;
                    for (int o = 32; o > 0; o >>= 1) {                   // the largest gain, ties to the lower candidate
                        const double ov = __shfl_xor(bv, o);
                        const int oi = __shfl_xor(bi, o);
                        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
                    }
                    if (bv > p.min_gain * Ecur) c = bi;
                    else stop = true;
                }
                c = __builtin_amdgcn_readfirstlane(c);
            }
            if (c >= 0) {
                double* vk = hg_rows + (int64_t)(k + 1) * W;
                double rj[HG_MAX_ROUNDS];                                // M7: p_cj / nu_j
#pragma unroll
                for (int j = 0; j < HG_MAX_ROUNDS; ++j) {
                    rj[j] = 0.0;
                    if (j < k && ne[j]) {
                        rj[j] = __shfl(pj[j], c) / s_nu[j];
                        if (lane == 0) s_R[k][j] = rj[j];
                    }
                }
                for (int i = 0; i < nW; ++i) {                           // lane = scenario
                    const int s = i * 64 + lane;
                    if (s < W) {
                        double vv = 0.0;
                        if ((rkm[i] >> lane) & 1ull) {
                            vv = p.inst_pnl[(row0 + s) * p.nH + c];
#pragma unroll
                            for (int j = 0; j < HG_MAX_ROUNDS; ++j)
                                if (j < k && ne[j]) vv = vv - rj[j] * hg_rows[(int64_t)(j + 1) * W + s];
                        }
                        vk[s] = vv;
                    }
                }
                __syncthreads();
                double nu = 0.0, dot = 0.0;
                for (int i = 0; i < nW; ++i) {
                    const unsigned long long m = hg_word(rkm, i);
                    for (int j = 0; j < 64; ++j) {
                        if (!((m >> j) & 1ull)) continue;
                        const double vv = vk[i * 64 + j];
                        nu = nu + vv * vv;
                        dot = dot + vv * e[i * 64 + j];
                    }
                }
                if (!(nu > 0.0)) {
                    if (lane == c) spent = true;
                } else {                                                 // M8
                    // no barrier between the reads of e above and the writes below: a workgroup is ONE wavefront (launch bounds
                    // and launch of 64), whose lanes have all left the loop above; with more wavefronts one is needed here
                    const double t = dot / nu;
                    for (int i = 0; i < nW; ++i) {
                        const int s = i * 64 + lane;
                        if (s < W && ((rkm[i] >> lane) & 1ull)) e[s] = e[s] - t * vk[s];
                    }
                    __syncthreads();
                    double pk = 0.0, a2 = 0.0, E2 = 0.0;
                    for (int i = 0; i < nW; ++i) {
                        const unsigned long long m = hg_word(rkm, i);
                        for (int j = 0; j < 64; ++j) {
                            if (!((m >> j) & 1ull)) continue;
                            const int s = i * 64 + j;
                            const double x = in.has ? xrow[(int64_t)s * p.nH] : 0.0, es = e[s];
                            pk = pk + x * vk[s];
                            a2 = a2 + x * es;
                            E2 = E2 + es * es;
                        }
                    }
                    pj[k] = pk;
                    a = a2;
                    g = g - (pk * pk) / nu;
                    if (lane == c) chosen = true;
                    Ecur = E2;
                    ne[k] = true;
                    ++nr;
                    if (lane == 0) { s_nu[k] = nu; s_t[k] = t; s_pick[k] = c; }
                }
            }
            if (lane == 0) {
                p.pick[b * p.K + k] = ne[k] ? c : -1;
                p.ss[b * (p.K + 1) + k + 1] = active ? Ecur : qnan();
            }
            __syncthreads();
        }
    }

    double tau[HG_MAX_ROUNDS], q[HG_MAX_ROUNDS];                         // M9
#pragma unroll
    for (int k = 0; k < HG_MAX_ROUNDS; ++k) { tau[k] = ne[k] ? s_t[k] : 0.0; q[k] = 0.0; }
#pragma unroll
    for (int k = HG_MAX_ROUNDS - 1; k >= 0; --k) {
        if (ne[k]) {
            q[k] = 0.0 - tau[k];
#pragma unroll
            for (int j = 0; j < HG_MAX_ROUNDS; ++j)
                if (j < k && ne[j]) tau[j] = tau[j] - tau[k] * s_R[k][j];
        }
    }
    if (in.has) {
        double hq = 0.0;
#pragma unroll
        for (int k = 0; k < HG_MAX_ROUNDS; ++k)
            if (ne[k] && s_pick[k] == lane) hq = q[k];
        const int64_t at = b * p.nH + lane;
        p.hedge[at] = active ? hq : qnan();
        p.inst_flags[at] = fl | (spent ? IVS_HG_SPENT : 0) | (chosen ? IVS_HG_CHOSEN : 0);
        const bool solo = usable && active;
        if (p.solo_qty) p.solo_qty[at] = solo ? 0.0 - a0 / g0 : qnan();
        if (p.solo_left) p.solo_left[at] = solo ? (E0 - (a0 * a0) / g0) / E0 : qnan();
    }
    if (lane == 0) p.n_rounds[b] = nr;
    for (int i = 0; i < nW; ++i) {                                       // M10, lane = scenario
        const int s = i * 64 + lane;
        if (s < W) {
            double r = qnan();
            if ((rkm[i] >> lane) & 1ull) {
                r = p.pnl[row0 + s];
#pragma unroll
                for (int k = 0; k < HG_MAX_ROUNDS; ++k)
                    if (ne[k]) r = r + q[k] * p.inst_pnl[(row0 + s) * p.nH + s_pick[k]];
            }
            p.pnl_hedged[row0 + s] = r;
        }
    }
}

}  // namespace ivs
