// Static-arbitrage report, risk-neutral density and Dupire local vol off snapshot surfaces (rules
// A1-A7): a 5-point stencil over vol [B][mT][mK] in (ln k, tau) on the total variance w = s * s * tau.
//
// A workgroup owns `spw` consecutive snapshots, so the per-snapshot report needs no step across workgroups.  A snapshot is
// cut into tasks = (64-strike chunk) x (strip of tenor rows); the workgroup's tasks go round its four wavefronts.  In a
// task lane = strike: the strike-only part of the stencil (spacings by log1p, the six coefficients, ln(k / S)) is formed
// once, then the wavefront walks the strip's rows with the previous, current and next row of its own lane in registers
// and the row after those in flight.  Strike neighbours are lane shifts; the two nodes beyond a chunk's edges (lane 0's
// left, lane 63's right) and the two rows beyond a strip's ends are read again from global memory -- lines this
// workgroup reads in the same pass, so they come from L1 / L2.  Counts are ballots + popcounts, the two minima one wave
// reduction per task; the wavefronts meet once in LDS (one slot per snapshot and wavefront, summed in wavefront order).
// Plain stores only, no atomics, no scratch; no result depends on how the snapshots were cut.
#pragma once
#include "ivs_device.hpp"

namespace ivs {

constexpr int AR_WAVES = 4;       // wavefronts per workgroup
constexpr int AR_MAX_SPW = 4;     // snapshots per workgroup (a snapshot with one task per wavefront needs no more)

struct ArbParams {
    const double* vol; const double* Kq; const double* Tq; const double* spot;
    int64_t kq_stride, tq_stride;                        // 0 = shared
    double rate;
    int32_t mK, mT;
    int64_t B;
    int32_t spw, strip, nchunk, nstrip;                  // snapshots per workgroup, rows per strip, chunks / strips per snapshot
    int32_t* flags; int32_t* counts; double* worst;      // [B][mT][mK], [B][4], [B][2]
    double* local_vol; double* density;                  // [B][mT][mK] or NULL
};

struct ArbSlot { int32_t c[4]; double mn[2]; };

// 3-point first-derivative weights on the spacings hm (to the left) and hp (to the right), rule A3
__device__ __forceinline__ void ar_d1_weights(double hm, double hp, double& am, double& a0, double& ap) {
    am = -hp / (hm * (hm + hp));
    a0 = (hp - hm) / (hm * hp);
    ap = hm / (hp * (hm + hp));
}

__global__ __launch_bounds__(AR_WAVES * 64) void surface_arbitrage_kernel(ArbParams p) {
    __shared__ ArbSlot slot[AR_MAX_SPW][AR_WAVES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t b0 = (int64_t)blockIdx.x * p.spw;
    const int nsnap = (int)((p.B - b0) < p.spw ? (p.B - b0) : p.spw);
    if (threadIdx.x < AR_MAX_SPW * AR_WAVES) {
        ArbSlot& s = slot[threadIdx.x / AR_WAVES][threadIdx.x % AR_WAVES];
        s.c[0] = s.c[1] = s.c[2] = s.c[3] = 0;
        s.mn[0] = s.mn[1] = __builtin_inf();
    }
    __syncthreads();

    const int per_snap = p.nchunk * p.nstrip;
    const int ntask = nsnap * per_snap;
    const double rate = p.rate;
    for (int t = wave; t < ntask; t += AR_WAVES) {
        const int ls = t / per_snap, rem = t - ls * per_snap;
        const int strip = rem / p.nchunk, chunk = rem - strip * p.nchunk;
        const int64_t b = b0 + ls;
        const int c0 = chunk * 64, i = c0 + lane;
        const bool in = i < p.mK;
        const bool halo_l = c0 > 0, halo_r = c0 + 64 < p.mK;              // uniform
        const int j0 = strip * p.strip;
        const int j1 = j0 + p.strip < p.mT ? j0 + p.strip : p.mT;
        const double S = p.spot[b];
        const bool s_ok = finite_pos(S);
        const double* kr = p.Kq + b * p.kq_stride;
        const double* tq = p.Tq + b * p.tq_stride;
        const double* vb = p.vol + b * (int64_t)p.mT * p.mK;

        // ---- the strike-only part (A2, A3)
        const double k = in ? kr[i] : qnan();
        const double km = (in && i > 0) ? kr[i - 1] : qnan();
        const double kp = (i + 1 < p.mK) ? kr[i + 1] : qnan();
        const bool kv = finite_pos(k), kvm = finite_pos(km), kvp = finite_pos(kp);
        const double hm = log1p((k - km) / km), hp = log1p((kp - k) / k);
        const bool k_stencil = kv && kvm && kvp && hm > 0.0 && hp > 0.0;
        double am, a0, ap;
        ar_d1_weights(hm, hp, am, a0, ap);
        const double bm = 2.0 / (hm * (hm + hp)), bc = -2.0 / (hm * hp), bp = 2.0 / (hp * (hm + hp));
        const double x = log(k / S);

        // one row: the lane's own node, and in `halo` what lane 0 / lane 63 need from beyond the chunk
        auto load_row = [&](int j, double& s, double& halo, double& tau) {
            s = qnan(); halo = qnan(); tau = qnan();
            if (j >= 0 && j < p.mT) {                                     // uniform
                const double* vr = vb + (int64_t)j * p.mK;
                tau = tq[j];
                if (in) s = vr[i];
                if (halo_l && lane == 0) halo = vr[c0 - 1];
                if (halo_r && lane == 63) halo = vr[c0 + 64];
            }
        };
        double s_p, s_c, s_n, s_f, h_p, h_c, h_n, h_f, t_p, t_c, t_n, t_f;   // previous, current, next, in flight
        load_row(j0 - 1, s_p, h_p, t_p);
        load_row(j0, s_c, h_c, t_c);
        load_row(j0 + 1, s_n, h_n, t_n);

        int c_eval = 0, c_cal = 0, c_bfly = 0, c_lv = 0;
        double mnN = __builtin_inf(), mnG = __builtin_inf();
        for (int j = j0; j < j1; ++j) {
            load_row(j + 2, s_f, h_f, t_f);
            const bool live = s_ok && finite_pos(t_c);                    // A1
            const bool valid = live && kv && finite_pos(s_c);
            const double w = s_c * s_c * t_c;                             // A2
            // A3: strike neighbours by lane shifts, the chunk's edges from the halo
            double sm = __shfl_up(s_c, 1), sp = __shfl_down(s_c, 1);
            if (lane == 0) sm = h_c;
            if (lane == 63) sp = h_c;
            const bool st_k = k_stencil && finite_pos(sm) && finite_pos(sp);
            const double wm = sm * sm * t_c, wp = sp * sp * t_c;
            const double w1 = am * wm + a0 * w + ap * wp;
            const double w2 = bm * wm + bc * w + bp * wp;
            // A4: tenor neighbours at the same strike
            const bool up = s_ok && finite_pos(t_n) && t_n > t_c && kv && finite_pos(s_n);
            const bool dn = s_ok && finite_pos(t_p) && t_p < t_c && kv && finite_pos(s_p);
            const double wu = s_n * s_n * t_n, wd = s_p * s_p * t_p;
            const double dm = t_c - t_p, dp = t_n - t_c;
            double cm, cc, cp;
            ar_d1_weights(dm, dp, cm, cc, cp);
            const double wt = (up && dn) ? cm * wd + cc * w + cp * wu : (up ? (wu - w) / dp : (wd - w) / (t_p - t_c));
            const bool eval = valid && st_k && (up || dn);
            // A5
            const double y = x - rate * t_c;
            const double N = wt + rate * w1;
            const double yw = y / w;
            const double g = 1.0 - yw * w1 + 0.25 * (-0.25 - 1.0 / w + yw * yw) * (w1 * w1) + 0.5 * w2;
            const bool cal = eval && N < 0.0, bfly = eval && g < 0.0;
            // A6
            const double lv = (eval && N >= 0.0 && g > 0.0) ? sqrt(N / g) : qnan();
            const int64_t o = (b * p.mT + j) * (int64_t)p.mK + i;
            if (in) p.flags[o] = !valid ? IVS_AR_DEAD : (!eval ? IVS_AR_NO_STENCIL : ((cal ? IVS_AR_CALENDAR : 0) | (bfly ? IVS_AR_BUTTERFLY : 0)));
            if (p.local_vol && in) p.local_vol[o] = lv;
            if (p.density) {
                const double sq = sqrt(w);
                const double d2 = -y / sq - 0.5 * sq;
                const double den = g * exp(-0.5 * (d2 * d2)) / (k * sqrt(6.283185307179586 * w));
                if (in) p.density[o] = eval ? den : qnan();
            }
            // A7
            c_eval += __popcll(__ballot(eval));
            c_cal += __popcll(__ballot(cal));
            c_bfly += __popcll(__ballot(bfly));
            c_lv += __popcll(__ballot(lv - lv == 0.0));                   // finite
            if (eval && N < mnN) mnN = N;
            if (eval && g < mnG) mnG = g;
            s_p = s_c; s_c = s_n; s_n = s_f;
            h_c = h_n; h_n = h_f;
            t_p = t_c; t_c = t_n; t_n = t_f;
        }
        for (int d = 32; d > 0; d >>= 1) {
            const double oN = __shfl_xor(mnN, d), oG = __shfl_xor(mnG, d);
            mnN = oN < mnN ? oN : mnN;
            mnG = oG < mnG ? oG : mnG;
        }
        if (lane == 0) {                                                  // this wavefront's own slot: no other writer
            ArbSlot& s = slot[ls][wave];
            s.c[0] += c_eval; s.c[1] += c_cal; s.c[2] += c_bfly; s.c[3] += c_lv;
            s.mn[0] = mnN < s.mn[0] ? mnN : s.mn[0];
            s.mn[1] = mnG < s.mn[1] ? mnG : s.mn[1];
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < nsnap) {
        const int ls = threadIdx.x;
        int32_t c[4] = {0, 0, 0, 0};
        double mn0 = __builtin_inf(), mn1 = __builtin_inf();
        for (int w = 0; w < AR_WAVES; ++w) {
            const ArbSlot& s = slot[ls][w];
            c[0] += s.c[0]; c[1] += s.c[1]; c[2] += s.c[2]; c[3] += s.c[3];
            mn0 = s.mn[0] < mn0 ? s.mn[0] : mn0;
            mn1 = s.mn[1] < mn1 ? s.mn[1] : mn1;
        }
        const int64_t b = b0 + ls;
        p.counts[b * 4 + 0] = c[0]; p.counts[b * 4 + 1] = c[1]; p.counts[b * 4 + 2] = c[2]; p.counts[b * 4 + 3] = c[3];
        p.worst[b * 2 + 0] = c[0] > 0 ? mn0 : qnan();
        p.worst[b * 2 + 1] = c[0] > 0 ? mn1 : qnan();
    }
}

}  // namespace ivs
