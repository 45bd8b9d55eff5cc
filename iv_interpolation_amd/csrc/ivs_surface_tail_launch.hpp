// Launchers of the surface tail: ragged work lists and the redo passes (masked, masked row-pass, generic).  Defines
// ordinary functions: exactly one unit of a library includes it (ivs_surface.hip; tools/pass_api.hip for the diagnostic
// libraries).
#pragma once
#include <atomic>

#include "ivs_surface_classify.hpp"
#include "ivs_surface_launch.hpp"
#include "ivs_surface_masked_pass.hpp"

namespace ivs {

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device attribute: set once per (kernel slot, device)
inline void ensure_max_lds(const void* fn, int slot, int dev) {
    static std::atomic<unsigned long long> done[IVS_MAX_DEV];
    const int d = (dev >= 0 && dev < IVS_MAX_DEV) ? dev : 0;
    const unsigned long long bit = 1ull << (slot & 63);
    if (dev < 0 || dev >= IVS_MAX_DEV || !(done[d].load(std::memory_order_relaxed) & bit)) {
        (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        done[d].fetch_or(bit, std::memory_order_relaxed);
    }
}

// Launch the generic kernel (FILTER selects the "only tagged surfaces" variant).  Returns false if the
// shape does not fit in LDS.
template <bool FILTER>
inline bool launch_surface_generic(const SurfaceParams& p, const LaunchCtx& cx) {
    if (p.nK > 65535) return false;                               // 16-bit strike indices
    const size_t lds = generic_lds_bytes(p.nK, p.nT, method_is_cubic(p.method));
    if (lds > 160 * 1024) return false;
    if (lds > 64 * 1024) ensure_max_lds(reinterpret_cast<const void*>(surface_generic_kernel<FILTER>), FILTER ? 1 : 0, cx.dev);
    int64_t grid = (int64_t)cx.num_cu * workgroups_per_cu(lds, 16) * 2;
    const int64_t work = FILTER ? (p.B + 63) / 64 : p.B;
    if (grid > work) grid = work;
    hipLaunchKernelGGL(surface_generic_kernel<FILTER>, dim3((unsigned)grid), dim3(64), lds, cx.st, p);
    return true;
}

// Second pass behind the dense / row-pass kernel for uniform 64 x 16 batches: returns true when launched.
using MaskedLerpMethods = Methods<IVS_LINEAR, IVS_SLINEAR, IVS_NEAREST, IVS_ZERO, IVS_FROM_DERIVATIVES>;      // surface_masked_kernel
using MaskedSlopeMethods = Methods<IVS_CUBIC, IVS_CUBICSPLINE, IVS_QUADRATIC, IVS_PCHIP, IVS_AKIMA>;         // surface_masked_pass_kernel
inline bool launch_surface_masked(const SurfaceParams& p, const LaunchCtx& cx) {
    if (p.k_off || p.nK != DK || p.nT != DT || p.mK > 64 || p.mT > D_MAX_MT) return false;
    if (p.t_stride != 0 || p.tq_stride != 0 || !p.tqs) return false;
    int64_t grid = (int64_t)cx.num_cu * 12;
    const int64_t work = (p.B + 63) / 64;
    if (grid > work) grid = work;
    return with_method(p.method, MaskedLerpMethods{}, [&](auto m) {
               hipLaunchKernelGGL((surface_masked_kernel<decltype(m)::value>), dim3((unsigned)grid), dim3(64), masked_lds_bytes(), cx.st, p);
           }) ||
           with_method(p.method, MaskedSlopeMethods{}, [&](auto m) {
               hipLaunchKernelGGL((surface_masked_pass_kernel<decltype(m)::value>), dim3((unsigned)grid), dim3(64), masked_pass_lds_bytes(), cx.st, p);
           });
}

// The tail of every fast-path launcher: surfaces the fast kernel tagged (missing quotes) go to the masked pass when the
// batch is the fixed 64 x 16 form (shared T / Tq only, see launch_surface_masked), then the filtered generic kernel takes
// whatever is still tagged (it returns at once when its counter is 0).
void launch_redo_tail(SurfaceParams& p, const LaunchCtx& cx, bool fixed64) {
    if (fixed64 && launch_surface_masked(p, cx) && p.redo) ++p.redo;
    launch_surface_generic<true>(p, cx);
}

// Work lists of a call.  Ragged batch: classified once into one list per size class (workspace: counters, then
// V_NCLASS x B items); uniform batch: the empty lists.  need1 / need2: the size classes the call has to launch.
bool var_work_lists(const SurfaceParams& p, const LaunchCtx& cx, VarWork& w) {
    VarItem* lists = nullptr;
    int32_t* counts = nullptr;
    if (p.k_off) {
        counts = reinterpret_cast<int32_t*>(cx.ws + WS_TQ_BYTES);
        lists = reinterpret_cast<VarItem*>(cx.ws + WS_TQ_BYTES + WS_COUNTS_BYTES);
        if (hipMemsetAsync(counts, 0, WS_COUNTS_BYTES, cx.st) != hipSuccess) return false;
        hipLaunchKernelGGL(var_classify_kernel, dim3((unsigned)capped_blocks(p.B, cx.num_cu, 1024, 8)), dim3(256), 0, cx.st, p, lists, lists + p.B, counts);
    }
    w.wl1 = VarList{lists, counts, 0};
    w.wl2 = VarList{lists ? lists + p.B : nullptr, counts ? counts + 1 : nullptr, 1};
    w.need1 = p.k_off ? true : p.nK <= 64;
    w.need2 = p.nK > 64;
    return true;
}

}  // namespace ivs
