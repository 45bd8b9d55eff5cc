// Arbitrage-free SSVI surface per snapshot, fitted jointly across tenors (rules J1-J8): one (rho, eta,
// gamma) per snapshot and one ATM total variance theta_j per tenor, w(x) = theta/2 (1 + rho phi x + sqrt((phi x + rho)^2 + 1 -
// rho^2)), phi = eta theta^-gamma, fitted to the total variances of every valid node of every live row in relative least
// squares.  theta is made non-decreasing in the tenor (no calendar arbitrage) and eta stays under the two closed-form butterfly
// bounds; every slice leaves as its exact raw-SVI form, the `params` of ivs_svi_slices_f64.
//
// One workgroup of four wavefronts per snapshot.  Phase 1, wavefront = row, lane = strike in 64-strike chunks read coalesced:
// a first pass counts each row's valid nodes; wavefront 0, lane = tenor, turns the counts into offsets, checks the order of
// the live tenors (one ballot, one lane permute) and takes theta's running maximum (lane scans); a second pass compacts the
// valid (x, w) into dynamic LDS in (tenor, node) order (ballot and prefix popcount).  Phase 2, thread = candidate of a
// 6 x 6 x 6 grid on the current box of (rho, gamma, ln(eta / eta_max)), `rounds` times: eta_max over the rows, then the SSE over
// rows and nodes (every LDS read at a workgroup-uniform address: a broadcast), a fixed xor butterfly over (SSE, candidate) per
// wavefront, the four winners through LDS, the winner's own point through LDS to everybody.  Phase 3, wavefront = row, lane =
// strike: the fitted vols, the vol errors and Durrleman's g, reduced by fixed butterflies; thread j stores row j.  Every loop
// is bounded by mT, mK, `rounds` or a constant; every barrier is reached by all 256 threads; plain loads and stores, no atomics.
#pragma once
#include "ivs_device.hpp"
#include "ivs_distribution.hpp"
#include "ivs_svi_surface.hpp"

namespace ivs {

constexpr int SS_WAVES = 4;
constexpr int SS_THREADS = SS_WAVES * 64;
constexpr int SS_MAX_T = 64;            // rule T2: tenors per snapshot (one ballot)
constexpr int SS_MAX_NODES = 3072;      // mT * mK: 16 B per node in LDS
constexpr int SS_MAX_ROUNDS = 32;
constexpr int SS_DEFAULT_ROUNDS = 20;
constexpr int SS_G = 6;                 // grid points per axis
constexpr int SS_CAND = SS_G * SS_G * SS_G;
constexpr double SS_EDGE_BAND = 0x1p-20;
constexpr double SS_RHO_MAX = 1.0 - 0x1p-10;
constexpr double SS_S_MIN = -6.931471805599453;   // ln 2^-10

struct SsviParams {
    const double* vol; const double* Kq; const double* Tq; const double* spot;
    const double* raw; const double* theta0;             // exactly one is non-null
    int64_t kq_stride, tq_stride;                        // 0 = shared
    double rate;
    int32_t mK, mT, rounds;
    double* surface; double* theta; double* params; double* fit;   // [B][4], [B][mT], [B][mT][5], [B][mT][3]
    int32_t* flags; int32_t* sflags; double* fitted;     // [B][mT], [B], [B][mT][mK] or null
};

// rule J1 with `raw`: theta0 = w(0) by T3, each operation rounded on its own
__device__ __forceinline__ double ss_w0(const DistRow& r) {
#pragma clang fp contract(off)
    const double dx = 0.0 - r.m;
    const double t = dx * dx;
    const double u = r.sig * r.sig;
    const double rr = sqrt(t + u);
    const double v = r.rho * dx;
    return r.a + r.b * (v + rr);
}

__device__ __forceinline__ double ss_point(double lo, double hi, int i) {
    const double h = (hi - lo) / 5.0;
    return i == SS_G - 1 ? hi : lo + i * h;
}

__global__ __launch_bounds__(SS_THREADS) void ssvi_surface_kernel(SsviParams p) {
    extern __shared__ __align__(16) unsigned char ss_lds[];
    double2* nodes = reinterpret_cast<double2*>(ss_lds);                 // (x, w) of the valid nodes, (tenor, node) order
    __shared__ double t_th0[SS_MAX_T];                                   // per row j: theta0 (NaN = dead)
    __shared__ int t_cnt[SS_MAX_T], t_hole[SS_MAX_T], t_lidx[SS_MAX_T], t_raised[SS_MAX_T];
    __shared__ double l_th[SS_MAX_T], l_L[SS_MAX_T], l_q[SS_MAX_T], l_inv[SS_MAX_T];   // per live row l, tenor order
    __shared__ int l_off[SS_MAX_T + 1];
    __shared__ int hdr[4];                                               // live rows, valid nodes, sflags, ok
    __shared__ double red_v[SS_WAVES];
    __shared__ int red_c[SS_WAVES];
    __shared__ double win[5];                                            // rho, gamma, s, eta, sse of a round's winner
    __shared__ double r_out[SS_MAX_T][9];                                // theta, a, b, rho, m, sigma, rmse_vol, max_vol_err, g_min

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t b = blockIdx.x;
    const int mT = p.mT, mK = p.mK;
    const double S = p.spot[b];
    const double* kr = p.Kq + b * p.kq_stride;
    const double* tr = p.Tq + b * p.tq_stride;

    // ---- phase 1a, wavefront = row: J1, the counts
    for (int j = wave; j < mT; j += SS_WAVES) {
        const int64_t row = b * mT + j;
        const double tau = tr[j];
        double th0;
        if (p.theta0) th0 = p.theta0[row];
        else {
            const DistRow r = st_row(p.raw + row * 5);
            th0 = ds_live(r, S, tau) ? ss_w0(r) : qnan();
        }
        const bool live = finite_pos(S) && finite_pos(tau) && finite_pos(th0);
        int n = 0, ifirst = -1, ilast = -1;
        if (live) {
            const double* vr = p.vol + row * mK;
            for (int c0 = 0; c0 < mK; c0 += 64) {
                const int i = c0 + lane;
                const bool in = i < mK;
                const double k = in ? kr[i] : qnan(), s = in ? vr[i] : qnan();
                const unsigned long long vm = __ballot(finite_pos(k) && finite_pos(s));
                if (vm) {
                    if (n == 0) ifirst = c0 + __builtin_ctzll(vm);
                    ilast = c0 + 63 - __builtin_clzll(vm);
                }
                n += __popcll(vm);
            }
        }
        if (lane == 0) {
            t_th0[j] = live ? th0 : qnan();
            t_cnt[j] = n;
            t_hole[j] = n > 0 && ilast - ifirst + 1 > n;
        }
    }
    __syncthreads();

    // ---- phase 1b, wavefront 0, lane = tenor: T2, J3, the offsets
    if (wave == 0) {
        const bool in = lane < mT;
        const double th0 = in ? t_th0[lane] : qnan();
        const double tau = in ? tr[lane] : 0.0;
        const bool lv = th0 == th0;
        const unsigned long long live = __ballot(lv);
        const unsigned long long above = live & ~((2ull << lane) - 1ull);
        const double tnext = __shfl(tau, above ? __builtin_ctzll(above) : lane);
        const bool unordered = __ballot(lv && above != 0ull && !(tnext > tau)) != 0ull;
        double th = lv ? th0 : -__builtin_inf();                         // J3: an inclusive max scan over the lanes
        int off = in && lv ? t_cnt[lane] : 0;                            // ... and an inclusive sum scan
        for (int d = 1; d < 64; d <<= 1) {
            const double ot = __shfl_up(th, d);
            const int oo = __shfl_up(off, d);
            if (lane >= d) { th = ot > th ? ot : th; off += oo; }
        }
        const int ntot = __shfl(off, 63);
        const int nl = __popcll(live);
        const int l = __popcll(live & ((1ull << lane) - 1ull));
        if (in) {
            t_lidx[lane] = lv ? l : -1;
            t_raised[lane] = lv && th > th0;
        }
        if (lv) {
            l_th[l] = th; l_L[l] = log(th); l_q[l] = sqrt(th); l_inv[l] = 1.0 / th;
            l_off[l] = off - t_cnt[lane];
        }
        if (lane == 0) {
            const bool sdead = nl == 0 || ntot < 5;
            l_off[nl] = ntot;
            hdr[0] = nl; hdr[1] = ntot;
            hdr[2] = (sdead ? IVS_SF_SURF_DEAD : 0) | (unordered ? IVS_SF_UNORDERED : 0);
            hdr[3] = !sdead && !unordered;
        }
    }
    __syncthreads();
    const int nl = hdr[0], ntot = hdr[1];
    const bool ok = hdr[3] != 0;                                         // uniform over the workgroup

    // ---- phase 1c, wavefront = row: J2, the valid (x, w) in (tenor, node) order
    if (ok) {
        for (int j = wave; j < mT; j += SS_WAVES) {
            const int l = t_lidx[j];
            if (l < 0) continue;
            const double tau = tr[j], rt = p.rate * tau;
            const double* vr = p.vol + (b * mT + j) * mK;
            int n = l_off[l];
            for (int c0 = 0; c0 < mK; c0 += 64) {
                const int i = c0 + lane;
                const bool in = i < mK;
                const double k = in ? kr[i] : qnan(), s = in ? vr[i] : qnan();
                const bool valid = finite_pos(k) && finite_pos(s);
                const unsigned long long vm = __ballot(valid);
                if (valid) {
                    const int at = n + __popcll(vm & ((1ull << lane) - 1ull));   // at < l_off[l + 1] <= mT * mK
                    nodes[at] = double2{log(k / S) - rt, s * s * tau};
                }
                n += __popcll(vm);
            }
        }
    }
    __syncthreads();

    // ---- phase 2, thread = candidate: J4 - J7
    double rlo = -SS_RHO_MAX, rhi = SS_RHO_MAX, glo = 0.0, ghi = 1.0, slo = SS_S_MIN, shi = 0.0;
    const int ir = tid % SS_G, ig = (tid / SS_G) % SS_G, is = tid / (SS_G * SS_G);
    const int rounds = ok ? p.rounds : 0;                                // uniform: a dead snapshot skips every round
    for (int round = 0; round < rounds; ++round) {
        const double hr = (rhi - rlo) / 5.0, hg = (ghi - glo) / 5.0, hs = (shi - slo) / 5.0;
        const double rho = ss_point(rlo, rhi, ir), gam = ss_point(glo, ghi, ig), s = ss_point(slo, shi, is < SS_G ? is : 0);
        double sse = __builtin_inf(), eta = qnan();
        if (tid < SS_CAND) {
            const double A = 1.0 + __builtin_fabs(rho), sA = sqrt(A);
            double emax = __builtin_inf();                               // J5, tenor order
            for (int l = 0; l < nl; ++l) {
                const double e = exp(-gam * l_L[l]);
                const double c1 = 4.0 / (l_th[l] * e * A), c2 = 2.0 / (l_q[l] * e * sA);
                const double c = c1 < c2 ? c1 : c2;
                emax = c < emax ? c : emax;
            }
            eta = exp(s) * emax;
            const double omr = 1.0 - rho * rho;
            sse = 0.0;
            for (int l = 0; l < nl; ++l) {                               // J6, (tenor, node) order
                const double th = l_th[l], inv = l_inv[l];
                const double phi = eta * exp(-gam * l_L[l]);
                const int i1 = l_off[l + 1];
                for (int i = l_off[l]; i < i1; ++i) {
                    const double2 xw = nodes[i];
                    const double px = phi * xw.x;
                    const double t = px + rho;
                    const double wf = 0.5 * th * (1.0 + rho * px + sqrt(t * t + omr));
                    const double r = (wf - xw.y) * inv;
                    sse += r * r;
                }
            }
        }
        // the smallest SSE, the lowest candidate among equals; a NaN never wins
        double best = sse == sse ? sse : __builtin_inf();
        int who = tid;
        for (int d = 32; d > 0; d >>= 1) {
            const double ob = __shfl_xor(best, d);
            const int ow = __shfl_xor(who, d);
            const bool take = ob < best || (ob == best && ow < who);
            best = take ? ob : best;
            who = take ? ow : who;
        }
        if (lane == 0) { red_v[wave] = best; red_c[wave] = who; }
        __syncthreads();
        best = red_v[0]; who = red_c[0];
        for (int w = 1; w < SS_WAVES; ++w) {                             // the same order in every thread
            const double ob = red_v[w];
            const int ow = red_c[w];
            const bool take = ob < best || (ob == best && ow < who);
            best = take ? ob : best;
            who = take ? ow : who;
        }
        if (tid == who) { win[0] = rho; win[1] = gam; win[2] = s; win[3] = eta; win[4] = sse; }
        __syncthreads();
        const double wr = win[0], wg = win[1], ws = win[2];              // the winner's own bits
        rlo = wr - hr > -SS_RHO_MAX ? wr - hr : -SS_RHO_MAX; rhi = wr + hr < SS_RHO_MAX ? wr + hr : SS_RHO_MAX;
        glo = wg - hg > 0.0 ? wg - hg : 0.0; ghi = wg + hg < 1.0 ? wg + hg : 1.0;
        slo = ws - hs > SS_S_MIN ? ws - hs : SS_S_MIN; shi = ws + hs < 0.0 ? ws + hs : 0.0;
    }
    const double rho = ok ? win[0] : qnan(), gam = ok ? win[1] : qnan(), sw = ok ? win[2] : qnan();
    const double eta = ok ? win[3] : qnan(), sse = ok ? win[4] : qnan();

    // ---- phase 3, wavefront = row, lane = strike: J8
    for (int j = wave; j < mT; j += SS_WAVES) {
        const int64_t row = b * mT + j;
        const int l = t_lidx[j];
        double* fr = p.fitted ? p.fitted + row * mK : nullptr;
        if (!ok || l < 0) {
            if (fr) for (int i = lane; i < mK; i += 64) fr[i] = qnan();
            if (lane == 0) for (int t = 0; t < 9; ++t) r_out[j][t] = qnan();
            continue;
        }
        const double th = l_th[l], tau = tr[j], rt = p.rate * tau;
        const double phi = eta * exp(-gam * l_L[l]);
        const double omr = 1.0 - rho * rho;
        const double pa = th * omr / 2.0, pb = th * phi / 2.0, pm = -rho / phi, psig = sqrt(omr) / phi;
        const double* vr = p.vol + row * mK;
        double se2 = 0.0, emax = 0.0, gmin = __builtin_inf();
        for (int c0 = 0; c0 < mK; c0 += 64) {
            const int i = c0 + lane;
            if (i >= mK) continue;
            const double k = kr[i], s = vr[i];
            const bool kpos = finite_pos(k);
            const double x = log(k / S) - rt;
            const double px = phi * x;
            const double t = px + rho;
            const double wf = 0.5 * th * (1.0 + rho * px + sqrt(t * t + omr));
            const double vf = sqrt((wf > 0.0 ? wf : 0.0) / tau);
            if (fr) fr[i] = kpos ? vf : qnan();
            if (kpos && finite_pos(s)) {
                const double e = vf - s;
                se2 += e * e;
                emax = __builtin_fabs(e) > emax ? __builtin_fabs(e) : emax;
                const double dx = x - pm;
                const double r = sqrt(dx * dx + psig * psig);
                const double w1 = pb * (rho + dx / r);
                const double w2 = pb * psig * psig / (r * r * r);
                const double u = 1.0 - x * w1 / (2.0 * wf);
                const double g = u * u - (w1 * w1 / 4.0) * (1.0 / wf + 0.25) + w2 / 2.0;
                gmin = g < gmin ? g : gmin;
            }
        }
        for (int d = 32; d > 0; d >>= 1) {                               // fixed order: the same bits in every lane
            se2 += __shfl_xor(se2, d);
            const double oe = __shfl_xor(emax, d), og = __shfl_xor(gmin, d);
            emax = oe > emax ? oe : emax;
            gmin = og < gmin ? og : gmin;
        }
        if (lane == 0) {
            const int n = t_cnt[j];
            r_out[j][0] = th; r_out[j][1] = pa; r_out[j][2] = pb; r_out[j][3] = rho; r_out[j][4] = pm; r_out[j][5] = psig;
            r_out[j][6] = n > 0 ? sqrt(se2 / (double)n) : qnan();
            r_out[j][7] = n > 0 ? emax : qnan();
            r_out[j][8] = n > 0 ? gmin : qnan();
        }
    }
    __syncthreads();
    if (tid < mT) {
        const int64_t row = b * mT + tid;
        const int l = t_lidx[tid];
        const double* o = r_out[tid];
        p.theta[row] = o[0];
        for (int t = 0; t < 5; ++t) p.params[row * 5 + t] = o[1 + t];
        for (int t = 0; t < 3; ++t) p.fit[row * 3 + t] = o[6 + t];
        int32_t fl = IVS_SS_DEAD;
        if (ok && l >= 0)
            fl = (t_raised[tid] ? IVS_SS_RAISED : 0) | (t_hole[tid] ? IVS_SS_HOLES : 0) | (o[8] < 0.0 ? IVS_SS_BUTTERFLY : 0);
        p.flags[row] = fl;
    }
    if (tid == 0) {
        int32_t sf = hdr[2];
        if (ok) {
            const double br = 2.0 * SS_RHO_MAX * SS_EDGE_BAND, bg = SS_EDGE_BAND, bs = (0.0 - SS_S_MIN) * SS_EDGE_BAND;
            if (rho + SS_RHO_MAX <= br || SS_RHO_MAX - rho <= br) sf |= IVS_SF_EDGE_RHO;
            if (gam <= bg || 1.0 - gam <= bg) sf |= IVS_SF_EDGE_GAMMA;
            if (sw - SS_S_MIN <= bs) sf |= IVS_SF_EDGE_ETA_LOW;
            if (0.0 - sw <= bs) sf |= IVS_SF_AT_BOUND;
        }
        double* su = p.surface + b * 4;
        su[0] = rho; su[1] = eta; su[2] = gam; su[3] = ok ? sqrt(sse / (double)ntot) : qnan();
        p.sflags[b] = sf;
    }
}

}  // namespace ivs
