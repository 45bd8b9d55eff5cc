// Unit of libivs.so: the surface entry points, and the tail of the surface kernels -- batch-wide tables, ragged work
// lists, the masked and generic redo passes -- with their launchers.
// Argument validation happens here on the host; kernels assume validated shapes.
#include <hip/hip_runtime.h>

#include "ivs_host.hpp"
#include "ivs_surface_tail_launch.hpp"

using namespace ivs::host;

extern "C" {

size_t ivs_surface_workspace_bytes(int64_t B, int32_t ragged) { return ivs::surface_ws_bytes(B, ragged != 0); }

int ivs_surface_batch_f64(const double* K, const int64_t* k_off, int64_t k_stride, int32_t nK,
                          const double* T, int64_t t_stride, int32_t nT,
                          const double* sigma, int64_t B,
                          const double* Kq, int64_t kq_stride, int32_t mK,
                          const double* Tq, int64_t tq_stride, int32_t mT,
                          double* out, int32_t* status, int32_t method, int32_t flags,
                          void* workspace, size_t workspace_bytes, void* stream) {
    g_err[0] = 0;
    g_last_kernel = "";
    if (!valid_method(method)) return fail(IVS_EINVAL, "ivs_surface_batch_f64: unknown method %d", method);
    if (ivs::method_is_poly(method)) return fail(IVS_EINVAL, "ivs_surface_batch_f64: method %d ('barycentric' / 'krogh') is 1-D only", method);
    if (B < 0 || nK < 0 || nT < 0 || mK < 0 || mT < 0) return fail(IVS_EINVAL, "ivs_surface_batch_f64: negative size");
    if (B == 0 || mK == 0 || mT == 0) return IVS_OK;
    if (!K || !T || !sigma || !Kq || !Tq || !out) return fail(IVS_EINVAL, "ivs_surface_batch_f64: null pointer");
    if (nT < 1 || nT > ivs::GEN_NTMAX) return fail(IVS_ERANGE, "ivs_surface_batch_f64: nT=%d outside [1,%d]", nT, ivs::GEN_NTMAX);
    if (nK < 1) return fail(IVS_ERANGE, "ivs_surface_batch_f64: nK=%d < 1", nK);
    if (!k_off && k_stride != 0 && k_stride < nK) return fail(IVS_EINVAL, "ivs_surface_batch_f64: k_stride < nK");
    if (t_stride < 0 || kq_stride < 0 || tq_stride < 0 || k_stride < 0)
        return fail(IVS_EINVAL, "ivs_surface_batch_f64: negative stride");
    if (ivs::generic_lds_bytes(nK, nT, ivs::method_is_cubic(method)) > 160 * 1024)
        return fail(IVS_ERANGE, "ivs_surface_batch_f64: nK=%d x nT=%d needs %zu B of LDS (> 160 KiB)", nK, nT,
                    ivs::generic_lds_bytes(nK, nT, ivs::method_is_cubic(method)));
    const size_t need = ivs::surface_ws_bytes(B, k_off != nullptr);
    if (!workspace || workspace_bytes < need)
        return fail(IVS_ENOMEM, "ivs_surface_batch_f64: workspace %zu < %zu bytes (ivs_surface_workspace_bytes)",
                    workspace ? workspace_bytes : (size_t)0, need);
    if (reinterpret_cast<uintptr_t>(workspace) & 255)
        return fail(IVS_EINVAL, "ivs_surface_batch_f64: workspace must be 256-byte aligned");

    ivs::SurfaceParams p;
    p.K = K; p.k_off = k_off; p.k_stride = k_off ? 0 : k_stride; p.nK = nK; p.k_total = k_off ? k_stride : 0;
    p.T = T; p.t_stride = t_stride; p.nT = nT;
    p.sigma = sigma; p.B = B; p.map_groups = 1; p.tqs = nullptr; p.redo = nullptr; p.queue = nullptr; p.mode = nullptr;
    p.Kq = Kq; p.kq_stride = kq_stride; p.mK = mK;
    p.Tq = Tq; p.tq_stride = tq_stride; p.mT = mT;
    p.out = out; p.status = status; p.method = method;
    ivs::LaunchCtx cx;
    current_device(cx.dev, cx.num_cu);
    cx.st = static_cast<hipStream_t>(stream);
    cx.ws = static_cast<unsigned char*>(workspace);
    cx.ws_bytes = workspace_bytes;
    cx.map_groups = (flags >> 8) & 0xff;

    if (!(flags & IVS_FLAG_FORCE_GENERIC)) {
        const int64_t need_blocks = (int64_t)cx.num_cu * 8;
        cx.stamps = (g_stamp_buf && g_stamp_cap >= need_blocks * ivs::D_NSTAMP) ? g_stamp_buf : nullptr;
        cx.grid_out = &g_last_grid;
        // the fast paths in order; each answers 1 = dispatched, 0 = not covered (try the next), < 0 = launch error
        const struct {
            bool on;
            int (*launch)(const ivs::SurfaceParams&, const ivs::LaunchCtx&, const char**);
            const char* what;
        } attempts[] = {{!cx.stamps && !(flags & IVS_FLAG_ONE_PASS), ivs::launch_surface_pass, "row-pass"},
                        {true, ivs::launch_surface_dense, "dense"},
                        {!g_stamp_buf, ivs::launch_surface_dense_var, "dense-var"}};
        for (const auto& a : attempts) {
            if (!a.on) continue;
            const char* family = nullptr;
            const int rc = a.launch(p, cx, &family);
            if (rc == 1) {
                set_last_kernel(family, method);
                return check_launch(g_last_kernel);
            }
            if (rc < 0) return fail(IVS_ELAUNCH, "ivs_surface_batch_f64: %s dispatch failed", a.what);
        }
    }

    if (!ivs::launch_surface_generic<false>(p, cx))
        return fail(IVS_ERANGE, "ivs_surface_batch_f64: nK=%d x nT=%d needs %zu B of LDS (> 160 KiB)", nK, nT,
                    ivs::generic_lds_bytes(nK, nT, ivs::method_is_cubic(method)));
    g_last_kernel = "surface_generic_kernel";
    return check_launch("surface_generic_kernel");
}

}  // extern "C"
