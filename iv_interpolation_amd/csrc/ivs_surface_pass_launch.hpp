// Launcher of the row-pass kernels (ivs_surface_pass.hpp).  Defines an ordinary function: exactly one unit of a library
// includes it (ivs_surface_pass.hip; tools/pass_api.hip for the diagnostic libraries).
#pragma once
#include "ivs_surface_launch.hpp"
#include "ivs_surface_pass.hpp"

namespace ivs {

#ifdef IVS_DIAG_MINIMAL      // diagnostic builds (tools/pass_api.hip): the cubic kernels only
using PassMethods = Methods<IVS_CUBIC>;
#else
using PassMethods = TableMethods;
#endif
// Dispatch of the row-pass kernels.  Returns 1 if dispatched (pass kernel(s) + redo tail), 0 if the call is outside
// their scope (see the head of this file), -1 on a launch error.  *family: the kernel's name without its method.
int launch_surface_pass(const SurfaceParams& p_in, const LaunchCtx& cx, const char** family) {
    SurfaceParams p = p_in;
    const bool lerp = p.method == IVS_LINEAR || p.method == IVS_SLINEAR || d_is_step(p.method);
    const bool local = d_is_local(p.method);
    if (!(p.method == IVS_CUBIC || p.method == IVS_CUBICSPLINE || p.method == IVS_QUADRATIC || lerp || local)) return 0;
    const bool tsh = p.t_stride == 0 && p.tq_stride == 0;
    if (!tsh && !(p.method == IVS_LINEAR && p.mT <= D_WLDS_MAX_MT)) return 0;
    if (p.mK > 64 || p.mT > D_MAX_MT) return 0;
    if (p.nT < 4 || p.nT > DT || p.nK < 4 || p.nK > 128) return 0;
    if (!p.k_off && p.k_stride != 0 && p.k_stride < p.nK) return 0;
    if (p.k_off && p.B > 0x7fffffffLL) return 0;
    const bool fixed64 = !p.k_off && p.nK == DK && p.nT == DT && !(reinterpret_cast<uintptr_t>(p.sigma) & 15);
    const bool nt16 = p.nT == DT;       // run-time-shape kernels: maturity count fixed at compile time (NT16)
    if (!(fixed64 || nt16 ? launch_tq_or_zero_queue<false>(p, cx, tsh, fixed64)      // 16 maturities: the fixed-count tables
                          : launch_tq_or_zero_queue<true>(p, cx, tsh, fixed64))) return -1;
    // one launch of surface_pass_kernel<M, NKB, VAR> over `list`, at most `cap` workgroups per CU
    auto launch = [&](auto m, auto nkb, auto var, int cap, const VarList& list) {
        constexpr int M = decltype(m)::value, NKB = decltype(nkb)::value;
        constexpr bool VAR = decltype(var)::value;
        // the lerp methods carry no S plane and no tables; per-surface maturities: TT + W behind the planes
        const size_t lds = pass_lds_bytes<NKB, d_is_local(M) ? 2 : (d_is_hermite(M) || d_is_quad(M)) ? 0 : 1>() + (tsh ? 0 : PASS_TQ_DOUBLES * 8);
        // LDS is granted in 1280-byte granules; 3 wavefronts per SIMD (168 VGPRs), the run-time-maturity-count local rules 2
        int per_cu = workgroups_per_cu(lds, (d_is_local(M) && VAR && !nt16) ? 8 : cap, 1280);
#ifdef IVS_PASS_PER_CU
        per_cu = IVS_PASS_PER_CU;                                              // diagnostic builds (tools/pass_api.hip)
#endif
        int64_t grid = (int64_t)cx.num_cu * per_cu;
        if (grid > p.B) grid = p.B;
        if (!VAR) p.map_groups = dense_map_groups(grid, p.B, cx.map_groups);
        if constexpr (M == IVS_LINEAR) {
            if (!tsh) {
                hipLaunchKernelGGL((surface_pass_kernel<M, NKB, VAR, false>), dim3((unsigned)grid), dim3(64), lds, cx.st, p, list);
                return;
            }
        }
        // run-time-shape batches with the full 16 maturities take the NT16 instantiation
        // ... and where it pays (see KQS) the kernel knows at compile time that the batch shares its query strikes
        with_bool(VAR && nt16, [&](auto n) {
            constexpr bool N16 = VAR && decltype(n)::value;
            constexpr bool KQS_OK = VAR ? N16 && (M == IVS_LINEAR || M == IVS_SLINEAR) : !d_is_step(M);
            with_bool(KQS_OK && p.kq_stride == 0, [&](auto k) {
                constexpr bool KQS = KQS_OK && decltype(k)::value;
                // ... and the leaner bookkeeping (see RW) where that measured a gain: the fixed shared-grid kernels of the
                // methods with slopes.  linear / slinear stayed inside the noise with it and keep the old row walk.
                constexpr int RWF = !(!VAR && KQS) ? 0 : (d_is_nak(M) || d_is_quad(M)) ? 5 : d_is_local(M) ? 4 : 0;
                hipLaunchKernelGGL((surface_pass_kernel<M, NKB, VAR, true, N16, KQS, RWF>),dim3((unsigned)grid), dim3(64), lds, cx.st, p, list);
            });
        });
    };
    bool ok = true;
    const bool known = with_method(p.method, PassMethods{}, [&](auto m) {
        using std::integral_constant;
        if (fixed64) {
            launch(m, integral_constant<int, 1>{}, std::false_type{}, 12, VarList{nullptr, nullptr});
            *family = "surface_pass_kernel";
        } else {
            VarWork vw;
            if (!(ok = var_work_lists(p, cx, vw))) return;
            if (vw.need1) launch(m, integral_constant<int, 1>{}, std::true_type{}, 12, vw.wl1);
            if (vw.need2) launch(m, integral_constant<int, 2>{}, std::true_type{}, PASS_CAP2, vw.wl2);
            *family = "surface_pass_var_kernel";
        }
    });
    if (!known) return 0;
    if (!ok || hipGetLastError() != hipSuccess) return -1;
    launch_redo_tail(p, cx, fixed64);
    return 1;
}

}  // namespace ivs
