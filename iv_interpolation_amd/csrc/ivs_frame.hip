// Unit of libivs.so: the 1-D interpolation, forward-fill, gather and frame entry points.
// Argument validation happens here on the host; kernels assume validated shapes.
#include <hip/hip_runtime.h>

#include "ivs_dispatch.hpp"
#include "ivs_frame.hpp"
#include "ivs_host.hpp"
#include "ivs_interp1d.hpp"

using namespace ivs::host;

extern "C" {

size_t ivs_interp1d_workspace_bytes(int64_t total_knots, int64_t n_series, int32_t n_channels) {
    if (total_knots < 0 || n_series < 0 || n_channels < 0) return 0;
    return ivs::interp1d_ws_bytes(total_knots, n_series, n_channels);
}

namespace {
// inside extern "C" an unnamed namespace does not keep a name local: hidden keeps it out of the dynamic symbol table
__attribute__((visibility("hidden"))) int interp1d_impl(const char* fn, const double* xk, const double* yk, int64_t yk_stride, const int64_t* knot_off,
                  int64_t n_series, int32_t n_channels, int64_t total_knots, const double* xq, const int64_t* q_off,
                  int64_t total_queries, double* out, int64_t out_stride, int32_t* status, int32_t method, void* workspace,
                  size_t workspace_bytes, void* stream, ivs::Interp1dParams& p) {
    g_err[0] = 0;
    if (!valid_method(method)) return fail(IVS_EINVAL, "%s: unknown method %d", fn, method);
    if (n_series < 0 || n_channels < 0 || total_knots < 0 || total_queries < 0) return fail(IVS_EINVAL, "%s: negative size", fn);
    if (n_series == 0 || n_channels == 0) return IVS_OK;
    if (!knot_off || !q_off || !status) return fail(IVS_EINVAL, "%s: null offsets/status", fn);
    if (total_knots > 0 && (!xk || !yk)) return fail(IVS_EINVAL, "%s: null knots", fn);
    if (total_queries > 0 && !out) return fail(IVS_EINVAL, "%s: null out", fn);
    if (yk_stride < total_knots || out_stride < total_queries)
        return fail(IVS_EINVAL, "%s: channel stride smaller than row length", fn);
    if (n_series * (int64_t)n_channels > 0x7fffffffLL || (total_queries + 255) / 256 > 0x7fffffffLL)
        return fail(IVS_ERANGE, "%s: batch too large for one launch", fn);
    size_t need = ivs::interp1d_ws_bytes(total_knots, n_series, n_channels);
    if (!workspace || workspace_bytes < need) return fail(IVS_ENOMEM, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, need);
    p.xk = xk; p.yk = yk; p.yk_stride = yk_stride; p.knot_off = knot_off;
    p.S = n_series; p.C = n_channels; p.total_knots = total_knots;
    p.xq = xq; p.q_off = q_off; p.total_q = total_queries;
    p.out = out; p.out_stride = out_stride; p.status = status; p.method = method;
    double* w = static_cast<double*>(workspace);
    size_t plane = (size_t)n_channels * (size_t)total_knots;
    p.wx = w; p.wy = w + plane; p.ws = w + 2 * plane; p.wcp = w + 3 * plane;
    p.wn = reinterpret_cast<int32_t*>(w + 4 * plane);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ivs::interp1d_prepare_kernel, dim3((unsigned)(n_series * n_channels)), dim3(256), 0, st, p);
    int rc = check_launch("interp1d_prepare_kernel");
    if (rc) return rc;
    if (total_queries > 0) {
        hipLaunchKernelGGL(ivs::interp1d_eval_kernel, dim3((unsigned)((total_queries + ivs::E1_ROWS - 1) / ivs::E1_ROWS)), dim3(256), 0, st, p);
        rc = check_launch("interp1d_eval_kernel");
    }
    return rc;
}
}  // namespace

int ivs_interp1d_batch_f64(const double* xk, const double* yk, int64_t yk_stride, const int64_t* knot_off,
                           int64_t n_series, int32_t n_channels, int64_t total_knots,
                           const double* xq, const int64_t* q_off, int64_t total_queries,
                           double* out, int64_t out_stride, int32_t* status, int32_t method,
                           void* workspace, size_t workspace_bytes, void* stream) {
    ivs::Interp1dParams p{};
    p.greeks = nullptr;
    return interp1d_impl("ivs_interp1d_batch_f64", xk, yk, yk_stride, knot_off, n_series, n_channels, total_knots, xq, q_off,
                         total_queries, out, out_stride, status, method, workspace, workspace_bytes, stream, p);
}

int ivs_interp1d_greeks_batch_f64(const double* xk, const double* yk, int64_t yk_stride, const int64_t* knot_off,
                                  int64_t n_series, int32_t n_channels, int64_t total_knots,
                                  const double* xq, const int64_t* q_off, int64_t total_queries,
                                  double* out, int64_t out_stride, int32_t* status, int32_t method,
                                  int32_t ch_iv, int32_t ch_underlying, int32_t ch_ttm,
                                  const int32_t* fill_idx, int64_t fill_stride, int32_t row_strike, int32_t row_rate,
                                  int32_t row_callput, const double* strike_src, const double* rate_src,
                                  const uint8_t* is_put_src, double* greeks, int64_t greeks_stride,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "ivs_interp1d_greeks_batch_f64";
    g_err[0] = 0;
    if (n_series > 0 && n_channels > 0 && total_queries > 0) {
        if (!greeks || greeks_stride < total_queries) return fail(IVS_EINVAL, "%s: null / short greeks output", fn);
        if (ch_iv < 0 || ch_iv >= n_channels || ch_underlying < 0 || ch_underlying >= n_channels || ch_ttm < 0 || ch_ttm >= n_channels)
            return fail(IVS_EINVAL, "%s: channel numbers outside [0, %d)", fn, n_channels);
        if ((row_strike >= 0 || row_rate >= 0 || row_callput >= 0) && (!fill_idx || fill_stride < total_queries))
            return fail(IVS_EINVAL, "%s: null / short fill index", fn);
        if ((row_strike >= 0 && !strike_src) || (row_rate >= 0 && !rate_src) || (row_callput >= 0 && !is_put_src))
            return fail(IVS_EINVAL, "%s: a present column needs its source array", fn);
    }
    ivs::Interp1dParams p{};
    p.fidx = fill_idx; p.fidx_stride = fill_stride; p.fi_strike = row_strike; p.fi_rate = row_rate; p.fi_put = row_callput;
    p.strike_src = strike_src; p.rate_src = rate_src; p.put_src = is_put_src;
    p.ch_iv = ch_iv; p.ch_S = ch_underlying; p.ch_T = ch_ttm;
    p.greeks = greeks; p.greeks_stride = greeks_stride;
    return interp1d_impl(fn, xk, yk, yk_stride, knot_off, n_series, n_channels, total_knots, xq, q_off, total_queries, out,
                         out_stride, status, method, workspace, workspace_bytes, stream, p);
}

int ivs_ffill_index_batch(const int64_t* src_pos, const int64_t* src_off, const uint8_t* valid, int64_t valid_stride,
                          int32_t n_cols, const int64_t* q_off, int64_t n_series, int64_t total_queries,
                          int32_t* idx_out, int64_t out_stride, void* stream) {
    g_err[0] = 0;
    if (n_cols < 0 || n_series < 0 || total_queries < 0) return fail(IVS_EINVAL, "ivs_ffill_index_batch: negative size");
    if (n_cols == 0 || n_series == 0 || total_queries == 0) return IVS_OK;
    if (!src_pos || !src_off || !valid || !q_off || !idx_out) return fail(IVS_EINVAL, "ivs_ffill_index_batch: null pointer");
    if (out_stride < total_queries) return fail(IVS_EINVAL, "ivs_ffill_index_batch: out_stride < total_queries");
    if ((total_queries + 255) / 256 > 0x7fffffffLL) return fail(IVS_ERANGE, "ivs_ffill_index_batch: too many rows");
    if (valid_stride > 0x7fffffffLL) return fail(IVS_ERANGE, "ivs_ffill_index_batch: %lld source rows exceed the int32 gather index", (long long)valid_stride);
    ivs::FfillParams p{src_pos, src_off, valid, valid_stride, n_cols, q_off, n_series, total_queries, idx_out, out_stride};
    hipLaunchKernelGGL(ivs::ffill_index_kernel, dim3((unsigned)((total_queries + ivs::F1_ROWS - 1) / ivs::F1_ROWS)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), p);
    return check_launch("ffill_index_kernel");
}

extern "C++" {
namespace {
template <class T>
int gather_impl(const char* fn, const void* src, int64_t src_stride, const int32_t* idx, int64_t idx_stride, const int32_t* idx_row,
                int32_t n_cols, int64_t n, void* out, int64_t out_stride, T missing, void* stream) {
    g_err[0] = 0;
    if (n_cols < 0 || n < 0) return fail(IVS_EINVAL, "%s: negative size", fn);
    if (n_cols == 0 || n == 0) return IVS_OK;
    if (!src || !idx || !idx_row || !out) return fail(IVS_EINVAL, "%s: null pointer", fn);
    if (idx_stride < n || out_stride < n) return fail(IVS_EINVAL, "%s: stride smaller than row count", fn);
    if (src_stride > 0x7fffffffLL) return fail(IVS_ERANGE, "%s: %lld source rows exceed the int32 gather index", fn, (long long)src_stride);
    ivs::GatherParams p{src, src_stride, idx, idx_stride, idx_row, n_cols, n, out, out_stride};
    hipLaunchKernelGGL(ivs::gather_rows_kernel<T>, dim3((unsigned)ivs::capped_blocks(n, num_cu())), dim3(256), 0, static_cast<hipStream_t>(stream), p, missing);
    return check_launch(fn);
}
}  // namespace
}  // extern "C++"

int ivs_gather_rows_f64(const double* src, int64_t src_stride, const int32_t* idx, int64_t idx_stride, const int32_t* idx_row,
                        int32_t n_cols, int64_t n, double* out, int64_t out_stride, void* stream) {
    return gather_impl<double>("ivs_gather_rows_f64", src, src_stride, idx, idx_stride, idx_row, n_cols, n, out, out_stride,
                               __builtin_nan(""), stream);
}

int ivs_gather_rows_i32(const int32_t* src, int64_t src_stride, const int32_t* idx, int64_t idx_stride, const int32_t* idx_row,
                        int32_t n_cols, int64_t n, int32_t* out, int64_t out_stride, void* stream) {
    return gather_impl<int32_t>("ivs_gather_rows_i32", src, src_stride, idx, idx_stride, idx_row, n_cols, n, out, out_stride,
                                (int32_t)-1, stream);
}

int ivs_frame_rows(const int64_t* q_off, int64_t n_series, int64_t total_queries, const int64_t* first_ns,
                   const double* chan, int64_t chan_stride, int32_t n_channels, const int32_t* sym_code,
                   const int32_t* status, const uint8_t* needs, int64_t* date_ns, uint8_t* keep, void* stream) {
    g_err[0] = 0;
    if (n_series < 0 || total_queries < 0 || n_channels < 0) return fail(IVS_EINVAL, "ivs_frame_rows: negative size");
    if (n_series == 0 || total_queries == 0) return IVS_OK;
    if (!q_off || !first_ns || !date_ns || !keep || (n_channels > 0 && (!chan || !status || !needs)))
        return fail(IVS_EINVAL, "ivs_frame_rows: null pointer");
    if (chan_stride < total_queries) return fail(IVS_EINVAL, "ivs_frame_rows: chan_stride < total_queries");
    ivs::FrameRowsParams p{q_off, n_series, total_queries, first_ns, chan, chan_stride, n_channels, sym_code, status, needs, date_ns, keep};
    hipLaunchKernelGGL(ivs::frame_rows_kernel, dim3((unsigned)ivs::capped_blocks(total_queries, num_cu())), dim3(256), 0, static_cast<hipStream_t>(stream), p);
    return check_launch("frame_rows_kernel");
}

namespace {
__attribute__((visibility("hidden"))) __global__ __launch_bounds__(256) void i64_to_f64_kernel(const int64_t* a, double* o, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) o[i] = (double)a[i];
}
}  // namespace

size_t ivs_frame_workspace_bytes(int64_t total_src, int64_t n_series, int32_t n_channels) {
    if (total_src < 0 || n_series < 0 || n_channels < 0) return 0;
    // the 1-D workspace, the positions as doubles, the channels' knot-rank tables
    return ((ivs::interp1d_ws_bytes(total_src, n_series, n_channels) + 63) & ~(size_t)63) + (size_t)total_src * 8 +
           (size_t)n_channels * (size_t)total_src * 4 + 64;
}

int ivs_frame_columns_f64(const ivs_frame_args* a, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "ivs_frame_columns_f64";
    g_err[0] = 0;
    if (!a) return fail(IVS_EINVAL, "%s: null args", fn);
    if (!valid_method(a->method)) return fail(IVS_EINVAL, "%s: unknown method %d", fn, a->method);
    if (a->n_series < 0 || a->total_src < 0 || a->total_queries < 0 || a->n_channels < 0 || a->n_valid < 0 || a->n_f < 0 ||
        a->n_c < 0 || a->n_idx < 0)
        return fail(IVS_EINVAL, "%s: negative size", fn);
    if (a->n_series == 0 || a->total_queries == 0) return IVS_OK;
    if (!a->src_pos || !a->src_off || !a->q_off) return fail(IVS_EINVAL, "%s: null offsets / positions", fn);
    if (a->n_channels > 0 && (!a->yk || !a->chan_out || !a->status)) return fail(IVS_EINVAL, "%s: null channel arrays", fn);
    if (a->n_channels > 0 && (a->yk_stride < a->total_src || a->chan_stride < a->total_queries))
        return fail(IVS_EINVAL, "%s: channel stride smaller than row length", fn);
    if (a->n_valid > 0 && (!a->valid || a->valid_stride < a->total_src)) return fail(IVS_EINVAL, "%s: null / short validity rows", fn);
    if (a->n_f > 0 && (!a->fsrc || !a->f_rows || !a->f_out || a->f_stride < a->total_queries || a->fsrc_stride < a->total_src))
        return fail(IVS_EINVAL, "%s: bad f64 column arguments", fn);
    if (a->n_c > 0 && (!a->csrc || !a->c_rows || !a->c_out || a->c_stride < a->total_queries || a->csrc_stride < a->total_src))
        return fail(IVS_EINVAL, "%s: bad code column arguments", fn);
    if (a->n_idx > 0 && (!a->idx_rows || !a->idx_out || a->idx_stride < a->total_queries)) return fail(IVS_EINVAL, "%s: bad index row arguments", fn);
    if (a->date_ns && (!a->keep || !a->first_ns)) return fail(IVS_EINVAL, "%s: date_ns needs keep and first_ns", fn);
    if (a->sym_col >= a->n_c) return fail(IVS_EINVAL, "%s: sym_col outside the code columns", fn);
    if (a->greeks) {
        if (a->greeks_stride < a->total_queries) return fail(IVS_EINVAL, "%s: short greeks output", fn);
        if (a->ch_iv < 0 || a->ch_iv >= a->n_channels || a->ch_underlying < 0 || a->ch_underlying >= a->n_channels || a->ch_ttm < 0 ||
            a->ch_ttm >= a->n_channels || a->n_channels > 3)
            return fail(IVS_EINVAL, "%s: Greeks need the three channels iv / underlying / ttm", fn);
        if (a->g_strike >= a->n_valid || a->g_rate >= a->n_valid || a->g_put >= a->n_valid) return fail(IVS_EINVAL, "%s: Greek validity row outside valid", fn);
        if ((a->g_strike >= 0 && !a->strike_src) || (a->g_rate >= 0 && !a->rate_src) || (a->g_put >= 0 && !a->put_src))
            return fail(IVS_EINVAL, "%s: a present column needs its source array", fn);
    }
    if (a->total_src > 0x7fffffffLL || a->n_series * (int64_t)(a->n_channels > 0 ? a->n_channels : 1) > 0x7fffffffLL ||
        (a->total_queries + ivs::FR_ROWS - 1) / ivs::FR_ROWS > 0x7fffffffLL)
        return fail(IVS_ERANGE, "%s: batch too large for one launch", fn);
    const size_t need = ivs_frame_workspace_bytes(a->total_src, a->n_series, a->n_channels);
    if (!workspace || workspace_bytes < need) return fail(IVS_ENOMEM, "%s: workspace %zu < %zu bytes", fn, workspace ? workspace_bytes : (size_t)0, need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    ivs::Interp1dParams p{};
    double* w = static_cast<double*>(workspace);
    const size_t plane = (size_t)a->n_channels * (size_t)a->total_src;
    p.wx = w; p.wy = w + plane; p.ws = w + 2 * plane; p.wcp = w + 3 * plane;
    p.wn = reinterpret_cast<int32_t*>(w + 4 * plane);
    double* xk = reinterpret_cast<double*>(reinterpret_cast<unsigned char*>(workspace) + ((ivs::interp1d_ws_bytes(a->total_src, a->n_series, a->n_channels) + 63) & ~(size_t)63));
    p.wr = reinterpret_cast<int32_t*>(xk + a->total_src);
    p.xk = xk; p.yk = a->yk; p.yk_stride = a->yk_stride; p.knot_off = a->src_off;
    p.S = a->n_series; p.C = a->n_channels; p.total_knots = a->total_src;
    p.xq = nullptr; p.q_off = a->q_off; p.total_q = a->total_queries;
    p.out = a->chan_out; p.out_stride = a->chan_stride; p.status = a->status; p.method = a->method;
    p.greeks = nullptr;
    if (a->total_src > 0)
        hipLaunchKernelGGL(i64_to_f64_kernel, dim3((unsigned)ivs::capped_blocks(a->total_src, num_cu())), dim3(256), 0, st, a->src_pos, xk, a->total_src);
    if (a->n_channels > 0) {
        hipLaunchKernelGGL(ivs::interp1d_prepare_kernel, dim3((unsigned)(a->n_series * a->n_channels)), dim3(256), 0, st, p);
        const int rc = check_launch("interp1d_prepare_kernel");
        if (rc) return rc;
    }
    ivs::FrameParams f{};
    f.src_pos = a->src_pos; f.src_off = a->src_off; f.q_off = a->q_off; f.S = a->n_series; f.total_src = a->total_src; f.total_q = a->total_queries;
    f.valid = a->valid; f.valid_stride = a->valid_stride; f.n_valid = a->n_valid;
    f.fsrc = a->fsrc; f.fsrc_stride = a->fsrc_stride; f.f_rows = a->f_rows; f.n_f = a->n_f; f.f_out = a->f_out; f.f_stride = a->f_stride;
    f.csrc = a->csrc; f.csrc_stride = a->csrc_stride; f.c_rows = a->c_rows; f.n_c = a->n_c; f.c_out = a->c_out; f.c_stride = a->c_stride;
    f.idx_rows = a->idx_rows; f.n_idx = a->n_idx; f.idx_out = a->idx_out; f.idx_stride = a->idx_stride;
    f.first_ns = a->first_ns; f.needs = a->needs; f.sym_col = a->sym_col; f.date_ns = a->date_ns; f.keep = a->keep;
    f.g_strike = a->g_strike; f.g_rate = a->g_rate; f.g_put = a->g_put; f.strike_src = a->strike_src; f.rate_src = a->rate_src; f.put_src = a->put_src;
    f.ch_iv = a->ch_iv; f.ch_S = a->ch_underlying; f.ch_T = a->ch_ttm; f.greeks = a->greeks; f.greeks_stride = a->greeks_stride;
    const dim3 fgrid((unsigned)((a->total_queries + ivs::FR_ROWS - 1) / ivs::FR_ROWS));
    ivs::with_method(ivs::frame_method_class(p.method), ivs::Methods<0, 1, 2>{}, [&](auto c) {
        hipLaunchKernelGGL(ivs::frame_fused_kernel<decltype(c)::value>, fgrid, dim3(256), 0, st, f, p);
    });
    return check_launch("frame_fused_kernel");
}

}  // extern "C"
