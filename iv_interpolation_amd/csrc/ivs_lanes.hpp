// Cross-lane building blocks shared by the surface kernels and the 1-D / frame kernels: DPP moves of doubles, the 2x2
// matrix scan, the not-a-knot factor tables and the 16-lane segment products.  Device helpers only: no kernel, no launcher.
#pragma once
#include "ivs_device.hpp"

namespace ivs {

// ---- cross-lane helpers (DPP moves stay in the VALU; ds_bpermute shuffles cost an LDS round trip)
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ double dpp_f64(double old, double src) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(src), CTRL, ROW_MASK, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(src), CTRL, ROW_MASK, 0xF, false);
    return __hiloint2double(hi, lo);
}
// old = 0.0 with full row / bank masks: bound_ctrl supplies the zero for lanes without a source, which saves the two
// v_mov that would otherwise seed the destination with `old` before every pair of DPP moves
template <int CTRL>
__device__ __forceinline__ double dpp0_f64(double src) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(src), CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(src), CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
constexpr int DPP_ROW_SHL(int n) { return 0x100 | n; }   // lane i <- lane i+n (within a row of 16)
constexpr int DPP_ROW_SHR(int n) { return 0x110 | n; }   // lane i <- lane i-n (within a row of 16)
constexpr int DPP_WAVE_SHL1 = 0x130, DPP_WAVE_SHR1 = 0x138, DPP_ROW_BCAST15 = 0x142, DPP_ROW_BCAST31 = 0x143;

__device__ __forceinline__ double readlane_f64(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// Inclusive scan over lanes 0..N-1 (N = 16 or 64) of 2x2 matrix products P_i <- P_i * P_{i-1} * ... * P_0.
template <int N>
__device__ __forceinline__ void scan_mat2(double& p00, double& p01, double& p10, double& p11, int lane) {
    // lanes without a valid source (row start, rows masked off) receive the IDENTITY through the DPP
    // `old` operand, so every lane multiplies unconditionally: no compare/select per step
#define IVS_SCAN_STEP(CTRL, MASK)                                                              \
    {                                                                                          \
        const double e = dpp_f64<CTRL, MASK>(1.0, p00), h = dpp_f64<CTRL, MASK>(1.0, p11);     \
        const double f = MASK == 0xF ? dpp0_f64<CTRL>(p01) : dpp_f64<CTRL, MASK>(0.0, p01);    \
        const double g = MASK == 0xF ? dpp0_f64<CTRL>(p10) : dpp_f64<CTRL, MASK>(0.0, p10);    \
        const double n00 = p00 * e + p01 * g, n01 = p00 * f + p01 * h;                         \
        const double n10 = p10 * e + p11 * g, n11 = p10 * f + p11 * h;                         \
        p00 = n00; p01 = n01; p10 = n10; p11 = n11;                                            \
    }
    (void)lane;
    IVS_SCAN_STEP(DPP_ROW_SHR(1), 0xF)
    IVS_SCAN_STEP(DPP_ROW_SHR(2), 0xF)
    IVS_SCAN_STEP(DPP_ROW_SHR(4), 0xF)
    IVS_SCAN_STEP(DPP_ROW_SHR(8), 0xF)
    if (N > 16) {
        IVS_SCAN_STEP(DPP_ROW_BCAST15, 0xA)     // rows 1,3 <- lane 15 of rows 0,2
        IVS_SCAN_STEP(DPP_ROW_BCAST31, 0xC)     // rows 2,3 <- lane 31
    }
#undef IVS_SCAN_STEP
}

// Factorisation tables of the not-a-knot slope system on N knots X[0..N) (N = 64 or 16), computed by
// lanes 0..N-1.  Conventions (oracle nak_slopes()):  forward  dp_i = PP_i*dyA + QQ_i*dyB - AL_i*dp_{i-1},
// backward s_i = dp_i - CP_i*s_{i+1};  (dyA, dyB) = (dy_{i-1}, dy_i) for interior rows,
// (dy_0, dy_1) for row 0 and (dy_{N-3}, dy_{N-2}) for row N-1.
template <int N>
__device__ __forceinline__ void factor_tables(const double* X, int lane, double& al, double& cp, double& pp,
                                              double& qq, double& rdx_out) {
    const int i = lane < N ? lane : N - 1;
    const double x0 = X[i];
    const double xp = X[i + 1 < N ? i + 1 : N - 1];
    const double xpp = X[i + 2 < N ? i + 2 : N - 1];
    const double xm = X[i > 0 ? i - 1 : 0];
    const double xmm = X[i > 1 ? i - 2 : 0];
    const double dxc = xp - x0;          // dx[i]
    const double dxm = x0 - xm;          // dx[i-1]
    const double dxp = xpp - xp;         // dx[i+1]
    const double dxmm = xm - xmm;        // dx[i-2]
    const double rdxc = refined_rcp(dxc);
    double a, b, c;
    if (i == 0) { a = 0.0; b = dxp; c = dxc + dxp; }
    else if (i == N - 1) { a = dxmm + dxm; b = dxmm; c = 0.0; }
    else { a = dxc; b = 2.0 * (dxm + dxc); c = dxm; }
    const double rb = refined_rcp(b);
    // g_i = a_i c_{i-1} / (b_i b_{i-1})
    const double crb = c * rb;                                          // c_i / b_i
    const double crb_prev = dpp0_f64<DPP_WAVE_SHR1>(crb);
    const double g = i == 0 ? 0.0 : a * rb * crb_prev;
    // omega_i = 1 - g_i / omega_{i-1}: prefix product of M_i = [[1,-g_i],[1,0]] (identity on lane 0)
    double p00 = 1.0, p01 = i == 0 ? 0.0 : -g, p10 = i == 0 ? 0.0 : 1.0, p11 = i == 0 ? 1.0 : 0.0;
    scan_mat2<N>(p00, p01, p10, p11, lane);
    const double num = p00 + p01, den = p10 + p11;          // omega_i = num / den (applied to omega_0 = 1)
    const double rw = i == 0 ? rb : den * rb * refined_rcp(num);   // 1 / w_i
    al = a * rw;
    cp = c * rw;
    const double rdx_prev = dpp0_f64<DPP_WAVE_SHR1>(rdxc);   // 1/dx[i-1]
    const double rdx_next = dpp0_f64<DPP_WAVE_SHL1>(rdxc);   // 1/dx[i+1]
    // (DPP reads need the SOURCE lane active: keep every cross-lane move outside divergent branches)
    const double rdxmm = dpp0_f64<DPP_WAVE_SHR1>(rdx_prev);  // 1/dx[i-2]
    // edge rows need 1/d with d = x_{i+2}-x_i (row 0) or x_i - x_{i-2} (row N-1)
    const double d = i == 0 ? dxc + dxp : dxmm + dxm;
    const double rd = refined_rcp(d);
    if (i == 0) {
        pp = (dxc + 2.0 * d) * dxp * rdxc * rd * rw;         // * dy_0
        qq = dxc * dxc * rdx_next * rd * rw;                 // * dy_1
    } else if (i == N - 1) {
        pp = dxm * dxm * rdxmm * rd * rw;                    // * dy_{N-3}
        qq = (2.0 * d + dxm) * dxmm * rdx_prev * rd * rw;    // * dy_{N-2}
    } else {
        pp = 3.0 * dxc * rdx_prev * rw;                      // * dy_{i-1}
        qq = 3.0 * dxm * rdxc * rw;                          // * dy_i
    }
    rdx_out = rdxc;
}

// segmented inclusive prefix / suffix products within aligned rows of 16 lanes
__device__ __forceinline__ double seg16_prefix_prod(double v, int lane) {
    (void)lane;                                   // out-of-row sources read as 1.0 (DPP `old`)
    v *= dpp_f64<DPP_ROW_SHR(1)>(1.0, v);
    v *= dpp_f64<DPP_ROW_SHR(2)>(1.0, v);
    v *= dpp_f64<DPP_ROW_SHR(4)>(1.0, v);
    v *= dpp_f64<DPP_ROW_SHR(8)>(1.0, v);
    return v;
}
__device__ __forceinline__ double seg16_suffix_prod(double v, int lane) {
    (void)lane;
    v *= dpp_f64<DPP_ROW_SHL(1)>(1.0, v);
    v *= dpp_f64<DPP_ROW_SHL(2)>(1.0, v);
    v *= dpp_f64<DPP_ROW_SHL(4)>(1.0, v);
    v *= dpp_f64<DPP_ROW_SHL(8)>(1.0, v);
    return v;
}

}  // namespace ivs
