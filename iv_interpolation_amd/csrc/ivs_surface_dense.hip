// Unit of libivs.so: the one-pass surface kernels (64 x 16 dense, variable strike counts on one and two wavefronts)
// and their launchers.
#include <hip/hip_runtime.h>

#include "ivs_surface_dense_var2.hpp"
#include "ivs_surface_tables_launch.hpp"

namespace ivs {

// Dense dispatch.  Returns 1 if dispatched (dense kernel + redo tail), 0 if the shape is not covered by a dense kernel,
// -1 on a launch error.  *family: the kernel's name without its method.
int launch_surface_dense(const SurfaceParams& p_in, const LaunchCtx& cx, const char** family) {
    SurfaceParams p = p_in;
    if (p.k_off || p.nK != DK || p.nT != DT) return 0;
    if (p.k_stride != 0 && p.k_stride < DK) return 0;
    if (reinterpret_cast<uintptr_t>(p.sigma) & 15) return 0;
    if (p.mT > D_MAX_MT) return 0;
    const size_t lds = dense_lds_bytes(p.mT);
    if (generic_lds_bytes(p.nK, p.nT) > 160 * 1024) return 0;
    int64_t grid = (int64_t)cx.num_cu * workgroups_per_cu(lds, 8);
    if (grid > p.B) grid = p.B;
    if (cx.grid_out) *cx.grid_out = grid;
    p.map_groups = dense_map_groups(grid, p.B, cx.map_groups);
    const bool tsh = p.t_stride == 0 && p.tq_stride == 0;
    const bool wl = p.mT <= D_WLDS_MAX_MT;
    if (!launch_tq_or_zero_queue<false>(p, cx, tsh, true)) return -1;
    if (p.map_groups > 16) p.map_groups = 16;
    if (cx.stamps) {   // diagnostic run: cubic and linear, shared T only
        if (!tsh) return 0;
        with_bool(p.method == IVS_CUBIC, [&](auto cubic) {
            with_bool(wl, [&](auto w) {
                hipLaunchKernelGGL((surface_dense_kernel<decltype(cubic)::value ? IVS_CUBIC : IVS_LINEAR, true, decltype(w)::value, true>), dim3((unsigned)grid), dim3(64),
                                   lds, cx.st, p, cx.stamps);
            });
        });
        *family = "surface_dense_kernel<stamp>";
        return hipGetLastError() == hipSuccess ? 1 : -1;
    }
    const bool known = with_method(p.method, DenseMethods{}, [&](auto m) {
        with_bool(tsh, [&](auto t) {
            with_bool(wl, [&](auto w) {
                hipLaunchKernelGGL((surface_dense_kernel<decltype(m)::value, decltype(t)::value, decltype(w)::value, false>), dim3((unsigned)grid), dim3(64), lds, cx.st, p,
                                   nullptr);
            });
        });
    });
    if (!known) return 0;
    *family = "surface_dense_kernel";
    if (hipGetLastError() != hipSuccess) return -1;
    launch_redo_tail(p, cx, true);
    return 1;
}

// Dispatch for variable strike counts: class 4..64 on the one-wavefront kernel, class 65..128 on the two-wavefront
// kernel, then the filtered generic redo pass.  Returns 1 if dispatched, 0 if the batch is not covered, -1 on a launch
// error.  Scratch (ragged work lists + counters, batch-wide maturity tables) comes from the caller's workspace: no allocation.
int launch_surface_dense_var(const SurfaceParams& p_in, const LaunchCtx& cx, const char** family) {
    SurfaceParams p = p_in;
    if (p.nT < 4 || p.nT > DT || p.mT > D_MAX_MT) return 0;
    const bool tsh = p.t_stride == 0 && p.tq_stride == 0;
    if (p.nK < 4 || p.nK > 128) return 0;
    if (!p.k_off && p.k_stride != 0 && p.k_stride < p.nK) return 0;
    if (generic_lds_bytes(p.nK, p.nT) > 160 * 1024) return 0;
    if (!(d_is_hermite(p.method) || p.method == IVS_LINEAR || p.method == IVS_SLINEAR)) return 0;
    const bool wl = p.mT <= D_WLDS_MAX_MT;
    if (!launch_tq_or_zero_queue<true>(p, cx, tsh, false)) return -1;
    if (p.k_off && p.B > 0x7fffffffLL) return 0;
    VarWork vw;
    if (!var_work_lists(p, cx, vw)) return -1;
    auto grid_for = [&](size_t lds) {
        const int64_t g = (int64_t)cx.num_cu * workgroups_per_cu(lds, 8);
        return dim3((unsigned)(g > p.B ? p.B : g));
    };
    const bool known = with_method(p.method, DenseMethods{}, [&](auto m) {
        constexpr int M = decltype(m)::value;
        with_bool(wl, [&](auto w) {
            with_bool(tsh, [&](auto t) {
                constexpr bool W = decltype(w)::value, T = decltype(t)::value;
                const size_t lds1 = dense_var_lds_bytes<1>(p.mT), lds2 = dense_var2_lds_bytes(p.mT);      // 40 KB: below the 64 KiB default limit
                if (vw.need1) hipLaunchKernelGGL((surface_dense_var_kernel<M, 1, W, T>), grid_for(lds1), dim3(64), lds1, cx.st, p, vw.wl1);
                if (vw.need2) hipLaunchKernelGGL((surface_dense_var2_kernel<M, W, T>), grid_for(lds2), dim3(128), lds2, cx.st, p, vw.wl2);
            });
        });
    });
    if (!known) return 0;
    *family = "surface_dense_var_kernel";
    if (hipGetLastError() != hipSuccess) return -1;
    launch_redo_tail(p, cx, false);
    return 1;
}

}  // namespace ivs
