// extern "C" entry points of libivs.so (declared in include/ivs.h).
// Argument validation happens here on the host; kernels assume validated shapes.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "../../include/ivs.h"
#include "ivs_arbitrage.hpp"
#include "ivs_bridge.hpp"
#include "ivs_candles.hpp"
#include "ivs_distribution.hpp"
#include "ivs_svi_surface.hpp"
#include "ivs_risk.hpp"
#include "ivs_explain.hpp"
#include "ivs_hsim.hpp"
#include "ivs_hsim_attrib.hpp"
#include "ivs_interp1d.hpp"
#include "ivs_frame.hpp"
#include "ivs_implied.hpp"
#include "ivs_moments.hpp"
#include "ivs_smile.hpp"
#include "ivs_snapshot.hpp"
#include "ivs_svi.hpp"
#include "ivs_ssvi.hpp"
#include "ivs_surface_dense.hpp"
#include "ivs_surface_dense_var2.hpp"
#include "ivs_surface_pass.hpp"
#include "ivs_surface_generic.hpp"

namespace {

thread_local char g_err[512] = "";
thread_local const char* g_last_kernel = "";
thread_local char g_kernel_name[64] = "";             // ivs_last_kernel() of the surface fast paths: family<method>
// diagnostics (ivs_debug_stamps): per calling thread, like the error string
thread_local unsigned long long* g_stamp_buf = nullptr;   // device buffer for the diagnostic (stamped) dense kernel
thread_local int64_t g_stamp_cap = 0;
thread_local int64_t g_last_grid = 0;

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(IVS_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
    return IVS_OK;
}

// family<method>; a family that already carries its argument ("surface_dense_kernel<stamp>") is reported as it is
void set_last_kernel(const char* family, int method) {
    if (strchr(family, '<')) snprintf(g_kernel_name, sizeof(g_kernel_name), "%s", family);
    else snprintf(g_kernel_name, sizeof(g_kernel_name), "%s<%s>", family, ivs::method_name(method));
    g_last_kernel = g_kernel_name;
}

bool valid_method(int m) { return m >= IVS_LINEAR && m <= IVS_BFILL; }

// CU count of the CURRENT device, cached per device index (a process may drive several devices)
std::atomic<int> g_cu[ivs::IVS_MAX_DEV];
void current_device(int& dev, int& cus) {
    dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
    const bool cached = dev >= 0 && dev < ivs::IVS_MAX_DEV;
    cus = cached ? g_cu[dev].load(std::memory_order_relaxed) : 0;
    if (cus <= 0) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) { (void)hipGetLastError(); v = 0; }
        cus = v > 0 ? v : 256;
        if (cached) g_cu[dev].store(cus, std::memory_order_relaxed);
    }
}
int num_cu() { int d, c; current_device(d, c); return c; }

// ---- the checks and launch steps the snapshot-analytics calls (ivs_*_args) share; each returns IVS_OK or the failure

// opens a call: no error, no kernel yet.  None of these calls takes device scratch, so their workspace arguments go unnamed.
int begin_call(const char* fn, const void* args) {
    g_err[0] = 0;
    g_last_kernel = "";
    return args ? IVS_OK : fail(IVS_EINVAL, "%s: null args", fn);
}

// closes a call after its one launch
int end_call(const char* kernel) {
    g_last_kernel = kernel;
    return check_launch(kernel);
}

// a query grid is shared by all surfaces (stride 0) or dense per surface (stride = its length)
int check_grid_stride(const char* fn, int64_t stride, int64_t len) {
    return stride == 0 || stride == len ? IVS_OK : fail(IVS_EINVAL, "%s: grid stride is neither 0 nor the grid's length", fn);
}

// B x mT rows are indexed, and spread over a grid, as int32
int check_rows(const char* fn, int64_t B, int32_t mT) {
    return B > 0x7fffffffLL / mT ? fail(IVS_ERANGE, "%s: %lld x %d rows exceed one launch", fn, (long long)B, mT) : IVS_OK;
}

// rows per wavefront of the kernels whose inversion phase packs several rows into one wavefront: fill its 64 lanes (`cap`
// rows do), but keep ~16 wavefronts per CU while the batch is small; `forced` > 0 is the tuning / testing override
int32_t rows_per_wave(int64_t rows, int cap, int forced) {
    int dev, cus;
    current_device(dev, cus);
    int64_t group = rows / ((int64_t)cus * 16);
    group = group < 1 ? 1 : (group > cap ? cap : group);
    return (int32_t)(forced > 0 ? forced : group);
}

// ivs_svi_eval_f64, ivs_svi_greeks_f64, ivs_svi_book_f64, ivs_svi_explain_f64: the shape of B snapshots of mT slices and Q queries / options each
int check_query_shape(const char* fn, int64_t B, int32_t mT, int64_t Q, int64_t tq_stride, int64_t q_stride, int32_t strike_mode) {
    if (B < 0 || mT < 0 || Q < 0 || tq_stride < 0 || q_stride < 0) return fail(IVS_EINVAL, "%s: negative size", fn);
    if (strike_mode != 0 && strike_mode != 1) return fail(IVS_EINVAL, "%s: strike_mode=%d is neither 0 nor 1", fn, strike_mode);
    if (mT > ivs::ST_MAX_T) return fail(IVS_ERANGE, "%s: mT=%d > %d tenors of one snapshot", fn, mT, ivs::ST_MAX_T);
    return IVS_OK;
}

// ... and, for a batch that is not empty, their strides and launch limits; `noun` is what the call names its Q entries
int check_query_launch(const char* fn, const char* noun, int64_t B, int32_t mT, int64_t Q, int64_t tq_stride, int64_t q_stride) {
    if ((tq_stride != 0 && tq_stride != mT) || (q_stride != 0 && q_stride != Q))
        return fail(IVS_EINVAL, "%s: grid or query stride is neither 0 nor the full length", fn);
    if (int rc = check_rows(fn, B, mT)) return rc;
    if (B > 0x7fffffffLL / Q) return fail(IVS_ERANGE, "%s: %lld x %lld %s exceed one launch", fn, (long long)B, (long long)Q, noun);
    return IVS_OK;
}

// ... and what their kernels' params take over from the args field for field: the names agree; svi_eval has no sides, and
// neither it nor svi_greeks has quantities
template <class P, class A>
void set_query_fields(P& p, const A* a) {
    p.params = a->params; p.Tq = a->Tq; p.spot = a->spot; p.u = a->u; p.tau = a->tau;
    p.tq_stride = a->tq_stride; p.q_stride = a->q_stride; p.rate = a->rate;
    p.mT = a->mT; p.strike_mode = a->strike_mode; p.Q = a->Q;
    if constexpr (!std::is_same_v<P, ivs::EvalParams>) p.is_put = a->is_put;
    if constexpr (!std::is_same_v<P, ivs::EvalParams> && !std::is_same_v<P, ivs::RiskParams>) p.qty = a->qty;
}

// items (scenario cells, scenarios) per workgroup of the kernels that split the n >= 1 items of each of B snapshots into runs:
// all n, or the fewest runs of at most `cap`, while the snapshots alone give every CU `per_cu` workgroups, shorter runs below
// that; `forced` > 0 is the tuning / testing override.  The sums of an item do not depend on the split.
int items_per_wg(int64_t B, int n, int per_cu, int cap, int forced) {
    int dev, cus;
    current_device(dev, cus);
    int64_t need = (per_cu * (int64_t)cus + B - 1) / B;
    const int least = (n + cap - 1) / cap;
    need = need < least ? least : (need > n ? n : need);
    return forced > 0 ? forced : (int)((n + need - 1) / need);
}

}  // namespace

extern "C" {

int ivs_version(void) { return IVS_ABI_VERSION; }

const char* ivs_last_error(void) { return g_err; }

const char* ivs_last_kernel(void) { return g_last_kernel; }

int ivs_debug_stamps(void* device_buf, int64_t n_u64) {
    g_stamp_buf = static_cast<unsigned long long*>(device_buf);
    g_stamp_cap = device_buf ? n_u64 : 0;
    return (int)ivs::D_NSTAMP;
}

int64_t ivs_debug_last_grid(void) { return g_last_grid; }
int64_t ivs_debug_mode_offset(void) { return (int64_t)offsetof(ivs::TqShared, mode); }

int ivs_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

size_t ivs_interp1d_workspace_bytes(int64_t total_knots, int64_t n_series, int32_t n_channels) {
    if (total_knots < 0 || n_series < 0 || n_channels < 0) return 0;
    return ivs::interp1d_ws_bytes(total_knots, n_series, n_channels);
}

namespace {
int interp1d_impl(const char* fn, const double* xk, const double* yk, int64_t yk_stride, const int64_t* knot_off,
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
__global__ __launch_bounds__(256) void i64_to_f64_kernel(const int64_t* a, double* o, int64_t n) {
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

int ivs_snapshot_assemble_f64(const ivs_snapshot_args* a, void*, size_t, void* stream) {
    const char* fn = "ivs_snapshot_assemble_f64";
    if (int rc = begin_call(fn, a)) return rc;
    if (a->n_rows < 0 || a->n_contracts < 0 || a->nT < 0 || a->nK < 0 || a->n_snapshots < 0 || a->mK < 0)
        return fail(IVS_EINVAL, "%s: negative size", fn);
    if (a->nT > 32) return fail(IVS_ERANGE, "%s: nT=%d expiries exceed the surface engine's 32", fn, a->nT);
    if (a->n_snapshots == 0) return IVS_OK;
    if (a->nT < 1 || a->nK < 1) return fail(IVS_ERANGE, "%s: nT=%d x nK=%d: empty axis", fn, a->nT, a->nK);
    if (!a->cells || !a->strike || !a->expiry_ns || !a->row_off || !a->sigma || !a->T || !a->spot || !a->quotes)
        return fail(IVS_EINVAL, "%s: null pointer", fn);
    if (a->n_rows > 0 && (!a->date_ns || !a->iv || !a->underlying)) return fail(IVS_EINVAL, "%s: null row columns", fn);
    if (a->Kq && (!a->moneyness || a->mK < 1)) return fail(IVS_EINVAL, "%s: Kq needs moneyness [mK >= 1]", fn);
    if (a->n_contracts > 0x7fffffffLL || (int64_t)a->nT * a->nK > 0x7fffffffLL)
        return fail(IVS_ERANGE, "%s: %lld contracts / %lld cells exceed the int32 tables", fn, (long long)a->n_contracts,
                    (long long)a->nT * a->nK);
    int dev, cus;
    current_device(dev, cus);
    // minutes per workgroup: enough workgroups for ~2 per CU, at least 8 minutes to amortise the per-tile row search
    int64_t tile = (a->n_snapshots + 2LL * cus - 1) / (2LL * cus);
    tile = tile < 8 ? 8 : (tile > ivs::SN_MAX_TILE ? ivs::SN_MAX_TILE : tile);
    const int64_t n_tiles = (a->n_snapshots + tile - 1) / tile;
    if (n_tiles > 0x7fffffffLL || a->n_snapshots > 0x7fffffffLL) return fail(IVS_ERANGE, "%s: %lld snapshots exceed one launch", fn, (long long)a->n_snapshots);
    const int64_t ncell = (int64_t)a->nT * a->nK;
    int waves = (int)((ncell + 63) / 64);
    waves = waves > ivs::SN_MAX_WAVES ? ivs::SN_MAX_WAVES : waves;
    ivs::SnapshotParams p{};
    p.date = a->date_ns; p.iv = a->iv; p.und = a->underlying; p.row_off = a->row_off;
    p.cells = a->cells; p.strike = a->strike; p.expiry = a->expiry_ns;
    p.moneyness = a->moneyness; p.mK = a->mK; p.kq_empty = a->kq_empty;
    p.t0 = a->t0_ns; p.B = a->n_snapshots; p.nT = a->nT; p.nK = a->nK;
    p.tile = (int32_t)tile; p.n_tiles = (int32_t)n_tiles; p.n_waves = waves;
    p.sigma = a->sigma; p.T = a->T; p.spot = a->spot; p.quotes = a->quotes; p.Kq = a->Kq;
    hipLaunchKernelGGL(ivs::snapshot_assemble_kernel, dim3((unsigned)n_tiles), dim3((unsigned)(waves * 64)), 0,
                       static_cast<hipStream_t>(stream), p);
    return end_call("snapshot_assemble_kernel");
}

int ivs_smile_delta_points_f64(const ivs_smile_args* a, void*, size_t, void* stream) {
    const char* fn = "ivs_smile_delta_points_f64";
    if (int rc = begin_call(fn, a)) return rc;
    if (a->B < 0 || a->mT < 0 || a->mK < 0 || a->kq_stride < 0 || a->tq_stride < 0) return fail(IVS_EINVAL, "%s: negative size", fn);
    if (a->nD < 1 || a->nD > ivs::SM_MAX_D) return fail(IVS_ERANGE, "%s: nD=%d outside [1,%d]", fn, a->nD, ivs::SM_MAX_D);
    if (a->mK < 2) return fail(IVS_ERANGE, "%s: mK=%d < 2: a bracket needs two nodes", fn, a->mK);
    if (a->rows_per_wave < 0 || a->rows_per_wave > 64 / a->nD)
        return fail(IVS_ERANGE, "%s: rows_per_wave=%d outside [0,%d] for nD=%d", fn, a->rows_per_wave, 64 / a->nD, a->nD);
    if (a->B == 0 || a->mT == 0) return IVS_OK;
    if (!a->vol || !a->Kq || !a->Tq || !a->spot || !a->z || !a->q_vol || !a->q_strike || !a->q_flags)
        return fail(IVS_EINVAL, "%s: null pointer", fn);
    if ((a->kq_stride != 0 && a->kq_stride < a->mK) || (a->tq_stride != 0 && a->tq_stride < a->mT))
        return fail(IVS_EINVAL, "%s: grid stride smaller than the grid", fn);
    if (int rc = check_rows(fn, a->B, a->mT)) return rc;
    ivs::SmileParams p{};
    p.vol = a->vol; p.Kq = a->Kq; p.Tq = a->Tq; p.spot = a->spot;
    p.kq_stride = a->kq_stride; p.tq_stride = a->tq_stride; p.rate = a->rate;
    for (int t = 0; t < a->nD; ++t) p.z[t] = a->z[t];
    p.mK = a->mK; p.mT = a->mT; p.nD = a->nD; p.rows = a->B * a->mT;
    p.q_vol = a->q_vol; p.q_strike = a->q_strike; p.q_flags = a->q_flags;
    p.group = rows_per_wave(p.rows, 64 / a->nD, a->rows_per_wave);
    const int64_t waves = (p.rows + p.group - 1) / p.group;
    hipLaunchKernelGGL(ivs::smile_delta_kernel, dim3((unsigned)((waves + ivs::SM_WAVES - 1) / ivs::SM_WAVES)),
                       dim3(ivs::SM_WAVES * 64), 0, static_cast<hipStream_t>(stream), p);
    return end_call("smile_delta_kernel");
}

int ivs_surface_arbitrage_f64(const ivs_arbitrage_args* a, void*, size_t, void* stream) {
    const char* fn = "ivs_surface_arbitrage_f64";
    if (int rc = begin_call(fn, a)) return rc;
    if (a->B < 0 || a->mT < 0 || a->mK < 0 || a->kq_stride < 0 || a->tq_stride < 0) return fail(IVS_EINVAL, "%s: negative size", fn);
    if (a->mK < 3) return fail(IVS_ERANGE, "%s: mK=%d < 3: the strike stencil needs three nodes", fn, a->mK);
    if (a->mT < 2) return fail(IVS_ERANGE, "%s: mT=%d < 2: the tenor stencil needs two rows", fn, a->mT);
    if (a->B == 0) return IVS_OK;
    if (!a->vol || !a->Kq || !a->Tq || !a->spot || !a->flags || !a->counts || !a->worst)
        return fail(IVS_EINVAL, "%s: null pointer", fn);
    if (int rc = check_grid_stride(fn, a->kq_stride, a->mK)) return rc;
    if (int rc = check_grid_stride(fn, a->tq_stride, a->mT)) return rc;
    if (int rc = check_rows(fn, a->B, a->mT)) return rc;
    ivs::ArbParams p{};
    p.vol = a->vol; p.Kq = a->Kq; p.Tq = a->Tq; p.spot = a->spot;
    p.kq_stride = a->kq_stride; p.tq_stride = a->tq_stride; p.rate = a->rate;
    p.mK = a->mK; p.mT = a->mT; p.B = a->B;
    p.flags = a->flags; p.counts = a->counts; p.worst = a->worst; p.local_vol = a->local_vol; p.density = a->density;
    // A snapshot is cut into 64-strike chunks x strips of tenor rows, one wavefront each.  Whole snapshots per wavefront
    // while the batch fills the device (~16 wavefronts per CU); below that, strips of at least 4 rows (each strip reads its
    // two neighbouring rows again).  A workgroup takes as many snapshots as give each of its wavefronts a task.
    int dev, cus;
    current_device(dev, cus);
    p.nchunk = (a->mK + 63) / 64;
    const int64_t whole = a->B * p.nchunk, want = (int64_t)cus * 16;
    int64_t nstrip = (want + whole - 1) / whole;
    const int64_t most = a->mT / 4 > 1 ? a->mT / 4 : 1;
    nstrip = nstrip < 1 ? 1 : (nstrip > most ? most : nstrip);
    p.strip = (int32_t)((a->mT + nstrip - 1) / nstrip);
    p.nstrip = (a->mT + p.strip - 1) / p.strip;
    const int per_snap = p.nchunk * p.nstrip;
    int spw = (ivs::AR_WAVES + per_snap - 1) / per_snap;
    p.spw = spw < 1 ? 1 : (spw > ivs::AR_MAX_SPW ? ivs::AR_MAX_SPW : spw);
    const int64_t grid = (a->B + p.spw - 1) / p.spw;
    hipLaunchKernelGGL(ivs::surface_arbitrage_kernel, dim3((unsigned)grid), dim3(ivs::AR_WAVES * 64), 0,
                       static_cast<hipStream_t>(stream), p);
    return end_call("surface_arbitrage_kernel");
}

int ivs_surface_moments_f64(const ivs_moments_args* a, void*, size_t, void* stream) {
    const char* fn = "ivs_surface_moments_f64";
    if (int rc = begin_call(fn, a)) return rc;
    if (a->B < 0 || a->mT < 0 || a->mK < 0 || a->nH < 0 || a->kq_stride < 0 || a->tq_stride < 0)
        return fail(IVS_EINVAL, "%s: negative size", fn);
    if (a->mK < 2) return fail(IVS_ERANGE, "%s: mK=%d < 2: a segment needs two nodes", fn, a->mK);
    if (a->nH > ivs::MM_MAX_H) return fail(IVS_ERANGE, "%s: nH=%d outside [0,%d]", fn, a->nH, ivs::MM_MAX_H);
    if (a->snapshots_per_wg < 0 || a->snapshots_per_wg > ivs::MM_MAX_SPW)
        return fail(IVS_ERANGE, "%s: snapshots_per_wg=%d outside [0,%d]", fn, a->snapshots_per_wg, ivs::MM_MAX_SPW);
    if (!(a->min_mass >= 0.0 && a->min_mass <= 1.0)) return fail(IVS_EINVAL, "%s: min_mass=%g outside [0,1]", fn, a->min_mass);
    if (a->nH > 0 && !a->horizons) return fail(IVS_EINVAL, "%s: null horizons", fn);
    for (int t = 0; t < a->nH; ++t)
        if (!(a->horizons[t] > 0.0 && a->horizons[t] < __builtin_inf()))
            return fail(IVS_EINVAL, "%s: horizon %d (%g) is not a finite positive number", fn, t, a->horizons[t]);
    if (a->B == 0 || a->mT == 0) return IVS_OK;
    if (!a->vol || !a->Kq || !a->Tq || !a->spot || !a->raw || !a->stats || !a->mass || !a->flags)
        return fail(IVS_EINVAL, "%s: null pointer", fn);
    if (a->nH > 0 && (!a->index || !a->index_flags)) return fail(IVS_EINVAL, "%s: null index / index_flags with nH=%d", fn, a->nH);
    if (int rc = check_grid_stride(fn, a->kq_stride, a->mK)) return rc;
    if (int rc = check_grid_stride(fn, a->tq_stride, a->mT)) return rc;
    if (int rc = check_rows(fn, a->B, a->mT)) return rc;
    if (a->mT > ivs::MM_MAX_T) return fail(IVS_ERANGE, "%s: mT=%d > %d row slots per snapshot", fn, a->mT, ivs::MM_MAX_T);
    ivs::MomParams p{};
    p.vol = a->vol; p.Kq = a->Kq; p.Tq = a->Tq; p.spot = a->spot;
    p.kq_stride = a->kq_stride; p.tq_stride = a->tq_stride; p.rate = a->rate; p.min_mass = a->min_mass;
    for (int t = 0; t < a->nH; ++t) p.h[t] = a->horizons[t];
    p.mK = a->mK; p.mT = a->mT; p.nH = a->nH; p.B = a->B;
    p.raw = a->raw; p.stats = a->stats; p.mass = a->mass; p.flags = a->flags;
    p.index = a->index; p.index_flags = a->index_flags;
    // a workgroup takes as many whole snapshots as give each of its wavefronts a row
    int spw = (ivs::MM_WAVES + a->mT - 1) / a->mT;
    if (a->snapshots_per_wg > 0) spw = a->snapshots_per_wg;  // tuning / testing override
    p.spw = spw;
    const int64_t grid = (a->B + spw - 1) / spw;
    const size_t lds = (size_t)spw * a->mT * sizeof(ivs::MomSlot);
    hipLaunchKernelGGL(ivs::surface_moments_kernel, dim3((unsigned)grid), dim3(ivs::MM_WAVES * 64), lds,
                       static_cast<hipStream_t>(stream), p);
    return end_call("surface_moments_kernel");
}

int ivs_svi_slices_f64(const ivs_svi_args* a, void*, size_t, void* stream) {
    const char* fn = "ivs_svi_slices_f64";
    if (int rc = begin_call(fn, a)) return rc;
    if (a->B < 0 || a->mT < 0 || a->mK < 0 || a->kq_stride < 0 || a->tq_stride < 0) return fail(IVS_EINVAL, "%s: negative size", fn);
    if (a->mK < 5) return fail(IVS_ERANGE, "%s: mK=%d < 5: five parameters need five nodes", fn, a->mK);
    if (a->mK > ivs::SV_MAX_K) return fail(IVS_ERANGE, "%s: mK=%d > %d nodes of the LDS slot", fn, a->mK, ivs::SV_MAX_K);
    if (a->rounds < 0 || a->rounds > ivs::SV_MAX_ROUNDS)
        return fail(IVS_ERANGE, "%s: rounds=%d outside [0,%d]", fn, a->rounds, ivs::SV_MAX_ROUNDS);
    if (a->rows_per_wg < 0 || a->rows_per_wg > ivs::SV_WAVES)
        return fail(IVS_ERANGE, "%s: rows_per_wg=%d outside [0,%d]", fn, a->rows_per_wg, ivs::SV_WAVES);
    if (a->B == 0 || a->mT == 0) return IVS_OK;
    if (!a->vol || !a->Kq || !a->Tq || !a->spot || !a->params || !a->fit || !a->flags)
        return fail(IVS_EINVAL, "%s: null pointer", fn);
    if (int rc = check_grid_stride(fn, a->kq_stride, a->mK)) return rc;
    if (int rc = check_grid_stride(fn, a->tq_stride, a->mT)) return rc;
    if (int rc = check_rows(fn, a->B, a->mT)) return rc;
    ivs::SviParams p{};
    p.vol = a->vol; p.Kq = a->Kq; p.Tq = a->Tq; p.spot = a->spot;
    p.kq_stride = a->kq_stride; p.tq_stride = a->tq_stride; p.rate = a->rate;
    p.mK = a->mK; p.mT = a->mT; p.rows = a->B * a->mT;
    p.rounds = a->rounds == 0 ? ivs::SV_DEFAULT_ROUNDS : a->rounds;
    p.params = a->params; p.fit = a->fit; p.flags = a->flags; p.fitted = a->fitted;
    // one row per wavefront; a workgroup takes four rows once that still leaves every CU a workgroup, fewer below that
    int dev, cus;
    current_device(dev, cus);
    int rpw = p.rows >= 4 * (int64_t)cus ? 4 : (p.rows >= 2 * (int64_t)cus ? 2 : 1);
    if (a->rows_per_wg > 0) rpw = a->rows_per_wg;           // tuning / testing override
    p.rpw = rpw;
    const int64_t grid = (p.rows + rpw - 1) / rpw;
    const size_t lds = (size_t)rpw * a->mK * 16;
    hipLaunchKernelGGL(ivs::svi_slice_kernel, dim3((unsigned)grid), dim3(ivs::SV_WAVES * 64), lds,
                       static_cast<hipStream_t>(stream), p);
    return end_call("svi_slice_kernel");
}

int ivs_svi_distribution_f64(const ivs_distribution_args* a, void*, size_t, void* stream) {
    const char* fn = "ivs_svi_distribution_f64";
    if (int rc = begin_call(fn, a)) return rc;
    if (a->B < 0 || a->mT < 0 || a->tq_stride < 0) return fail(IVS_EINVAL, "%s: negative size", fn);
    if (a->nP < 1 || a->nP > ivs::DS_MAX_P) return fail(IVS_ERANGE, "%s: nP=%d outside [1,%d]", fn, a->nP, ivs::DS_MAX_P);
    if (a->nL < 0 || a->nL > ivs::DS_MAX_L) return fail(IVS_ERANGE, "%s: nL=%d outside [0,%d]", fn, a->nL, ivs::DS_MAX_L);
    if (a->rows_per_wave < 0 || a->rows_per_wave > 64 / a->nP)
        return fail(IVS_ERANGE, "%s: rows_per_wave=%d outside [0,%d] with nP=%d", fn, a->rows_per_wave, 64 / a->nP, a->nP);
    if (!(a->max_tail >= 0.0 && a->max_tail <= 1.0)) return fail(IVS_EINVAL, "%s: max_tail=%g outside [0,1]", fn, a->max_tail);
    if (!a->probs) return fail(IVS_EINVAL, "%s: null probs", fn);
    if (a->nL > 0 && !a->levels) return fail(IVS_EINVAL, "%s: null levels", fn);
    for (int t = 0; t < a->nP; ++t)
        if (!(a->probs[t] > 0.0 && a->probs[t] < 1.0))
            return fail(IVS_EINVAL, "%s: probability %d (%g) is not strictly inside (0, 1)", fn, t, a->probs[t]);
    for (int l = 0; l < a->nL; ++l)
        if (!(a->levels[l] > 0.0 && a->levels[l] < __builtin_inf()))
            return fail(IVS_EINVAL, "%s: level %d (%g) is not a finite positive number", fn, l, a->levels[l]);
    if (a->B == 0 || a->mT == 0) return IVS_OK;
    if (!a->params || !a->Tq || !a->spot || !a->q_x || !a->q_strike || !a->q_flags || !a->tails || !a->flags)
        return fail(IVS_EINVAL, "%s: null pointer", fn);
    if (a->nL > 0 && (!a->p_below || !a->p_above)) return fail(IVS_EINVAL, "%s: null p_below / p_above with nL=%d", fn, a->nL);
    if (int rc = check_grid_stride(fn, a->tq_stride, a->mT)) return rc;
    if (int rc = check_rows(fn, a->B, a->mT)) return rc;
    ivs::DistParams p{};
    p.params = a->params; p.Tq = a->Tq; p.spot = a->spot;
    p.tq_stride = a->tq_stride; p.rate = a->rate; p.max_tail = a->max_tail;
    for (int t = 0; t < a->nP; ++t) p.probs[t] = a->probs[t];
    for (int l = 0; l < a->nL; ++l) p.levels[l] = a->levels[l];
    p.mT = a->mT; p.nP = a->nP; p.nL = a->nL; p.rows = a->B * a->mT;
    p.q_x = a->q_x; p.q_strike = a->q_strike; p.q_flags = a->q_flags;
    p.p_below = a->nL > 0 ? a->p_below : nullptr; p.p_above = a->nL > 0 ? a->p_above : nullptr;
    p.tails = a->tails; p.flags = a->flags;
    p.group = rows_per_wave(p.rows, 64 / a->nP, a->rows_per_wave);
    const int64_t waves = (p.rows + p.group - 1) / p.group;
    hipLaunchKernelGGL(ivs::svi_distribution_kernel, dim3((unsigned)((waves + ivs::DS_WAVES - 1) / ivs::DS_WAVES)),
                       dim3(ivs::DS_WAVES * 64), 0, static_cast<hipStream_t>(stream), p);
    return end_call("svi_distribution_kernel");
}

int ivs_svi_calendar_f64(const ivs_calendar_args* a, void*, size_t, void* stream) {
    const char* fn = "ivs_svi_calendar_f64";
    if (int rc = begin_call(fn, a)) return rc;
    if (a->B < 0 || a->mT < 0 || a->tq_stride < 0) return fail(IVS_EINVAL, "%s: negative size", fn);
    if (a->mT > ivs::ST_MAX_T) return fail(IVS_ERANGE, "%s: mT=%d > %d tenors of one ballot", fn, a->mT, ivs::ST_MAX_T);
    if (a->rows_per_wave < 0 || a->rows_per_wave > ivs::SC_MAX_GROUP)
        return fail(IVS_ERANGE, "%s: rows_per_wave=%d outside [0,%d]", fn, a->rows_per_wave, ivs::SC_MAX_GROUP);
    if (a->B == 0 || a->mT == 0) return IVS_OK;
    if (!a->params || !a->Tq || !a->spot || !a->d_min || !a->x_min || !a->d_atm || !a->x_cross || !a->n_cross || !a->flags)
        return fail(IVS_EINVAL, "%s: null pointer", fn);
    if (int rc = check_grid_stride(fn, a->tq_stride, a->mT)) return rc;
    if (int rc = check_rows(fn, a->B, a->mT)) return rc;
    ivs::CalParams p{};
    p.params = a->params; p.Tq = a->Tq; p.spot = a->spot; p.tq_stride = a->tq_stride;
    p.mT = a->mT; p.rows = a->B * a->mT;
    p.d_min = a->d_min; p.x_min = a->x_min; p.d_atm = a->d_atm; p.x_cross = a->x_cross;
    p.n_cross = a->n_cross; p.flags = a->flags;
    p.group = rows_per_wave(p.rows, ivs::SC_MAX_GROUP, a->rows_per_wave);
    const int64_t waves = (p.rows + p.group - 1) / p.group;
    hipLaunchKernelGGL(ivs::svi_calendar_kernel, dim3((unsigned)((waves + ivs::SC_WAVES - 1) / ivs::SC_WAVES)),
                       dim3(ivs::SC_WAVES * 64), 0, static_cast<hipStream_t>(stream), p);
    return end_call("svi_calendar_kernel");
}

int ivs_svi_eval_f64(const ivs_eval_args* a, void*, size_t, void* stream) {
    const char* fn = "ivs_svi_eval_f64";
    if (int rc = begin_call(fn, a)) return rc;
    if (int rc = check_query_shape(fn, a->B, a->mT, a->Q, a->tq_stride, a->q_stride, a->strike_mode)) return rc;
    if (a->B == 0 || a->mT == 0 || a->Q == 0) return IVS_OK;
    if (!a->params || !a->Tq || !a->spot || !a->u || !a->tau || !a->flags) return fail(IVS_EINVAL, "%s: null pointer", fn);
    if (int rc = check_query_launch(fn, "queries", a->B, a->mT, a->Q, a->tq_stride, a->q_stride)) return rc;
    ivs::EvalParams p{};
    set_query_fields(p, a);
    p.nqb = (int32_t)((a->Q + ivs::SE_BLOCK - 1) / ivs::SE_BLOCK);
    p.w = a->w; p.vol = a->vol; p.call = a->call; p.put = a->put; p.fwd_var = a->fwd_var; p.g = a->g; p.local_vol = a->local_vol;
    p.flags = a->flags;
    const int64_t grid = a->B * p.nqb;                      // <= B * Q < 2^31
    hipLaunchKernelGGL(ivs::svi_eval_kernel, dim3((unsigned)grid), dim3(ivs::SE_BLOCK), 0, static_cast<hipStream_t>(stream), p);
    return end_call("svi_eval_kernel");
}

int ivs_svi_greeks_f64(const ivs_greeks_args* a, void*, size_t, void* stream) {
    const char* fn = "ivs_svi_greeks_f64";
    if (int rc = begin_call(fn, a)) return rc;
    if (int rc = check_query_shape(fn, a->B, a->mT, a->Q, a->tq_stride, a->q_stride, a->strike_mode)) return rc;
    if (a->B == 0 || a->mT == 0 || a->Q == 0) return IVS_OK;
    if (!a->params || !a->Tq || !a->spot || !a->u || !a->tau || !a->flags) return fail(IVS_EINVAL, "%s: null pointer", fn);
    if (int rc = check_query_launch(fn, "options", a->B, a->mT, a->Q, a->tq_stride, a->q_stride)) return rc;
    ivs::RiskParams p{};
    set_query_fields(p, a);
    p.nqb = (int32_t)((a->Q + ivs::RK_BLOCK - 1) / ivs::RK_BLOCK);
    p.out[0] = a->price; p.out[1] = a->delta_ss; p.out[2] = a->delta_sm; p.out[3] = a->gamma_ss; p.out[4] = a->gamma_sm;
    p.out[5] = a->vega; p.out[6] = a->theta;
    p.flags = a->flags;
    const int64_t grid = a->B * p.nqb;                      // <= B * Q < 2^31
    hipLaunchKernelGGL(ivs::svi_greeks_kernel, dim3((unsigned)grid), dim3(ivs::RK_BLOCK), 0, static_cast<hipStream_t>(stream), p);
    return end_call("svi_greeks_kernel");
}

int ivs_svi_book_f64(const ivs_book_args* a, void*, size_t, void* stream) {
    const char* fn = "ivs_svi_book_f64";
    if (int rc = begin_call(fn, a)) return rc;
    if (a->nA < 0 || a->nV < 0) return fail(IVS_EINVAL, "%s: negative size", fn);
    if (int rc = check_query_shape(fn, a->B, a->mT, a->Q, a->tq_stride, a->q_stride, a->strike_mode)) return rc;
    if (a->nA > ivs::RK_MAX_SHOCKS || a->nV > ivs::RK_MAX_SHOCKS)
        return fail(IVS_ERANGE, "%s: nA=%d or nV=%d > %d shocks per axis", fn, a->nA, a->nV, ivs::RK_MAX_SHOCKS);
    if (a->nA * a->nV > ivs::RK_MAX_GRID) return fail(IVS_ERANGE, "%s: nA*nV=%d > %d cells", fn, a->nA * a->nV, ivs::RK_MAX_GRID);
    if (a->cells_per_wg < 0 || a->cells_per_wg > ivs::RK_MAX_CELLS)
        return fail(IVS_ERANGE, "%s: cells_per_wg=%d outside [0,%d]", fn, a->cells_per_wg, ivs::RK_MAX_CELLS);
    const int ncell = a->nA * a->nV;
    if (ncell > 0 && (!a->spot_shocks || !a->vol_shocks)) return fail(IVS_EINVAL, "%s: null shocks", fn);
    for (int i = 0; ncell > 0 && i < a->nA; ++i)
        if (!(a->spot_shocks[i] > -1.0 && a->spot_shocks[i] < __builtin_inf()))
            return fail(IVS_ERANGE, "%s: spot shock %d (%g) is not a finite number above -1", fn, i, a->spot_shocks[i]);
    for (int k = 0; ncell > 0 && k < a->nV; ++k)
        if (!(a->vol_shocks[k] > -__builtin_inf() && a->vol_shocks[k] < __builtin_inf()))
            return fail(IVS_ERANGE, "%s: vol shock %d (%g) is not finite", fn, k, a->vol_shocks[k]);
    if (a->B == 0 || a->mT == 0 || a->Q == 0) return IVS_OK;
    if (!a->params || !a->Tq || !a->spot || !a->u || !a->tau || !a->qty || !a->net || !a->n_dead) return fail(IVS_EINVAL, "%s: null pointer", fn);
    if (ncell > 0 && !a->cell_flags) return fail(IVS_EINVAL, "%s: null pointer (cell_flags)", fn);
    if (int rc = check_query_launch(fn, "options", a->B, a->mT, a->Q, a->tq_stride, a->q_stride)) return rc;
    if (ncell > 0 && a->B > 0x7fffffffLL / ncell)
        return fail(IVS_ERANGE, "%s: %lld x %d cells exceed one launch", fn, (long long)a->B, ncell);
    ivs::BookParams p{};
    set_query_fields(p, a);
    p.nA = a->nA; p.nV = a->nV;
    for (int i = 0; ncell > 0 && i < a->nA; ++i) p.a[i] = a->spot_shocks[i];
    for (int k = 0; ncell > 0 && k < a->nV; ++k) p.v[k] = a->vol_shocks[k];
    p.net = a->net; p.n_dead = a->n_dead; p.pnl_ss = a->pnl_ss; p.pnl_sm = a->pnl_sm; p.cell_flags = a->cell_flags;
    // cells per workgroup: a whole grid of up to 256 cells while the snapshots alone give every CU two workgroups
    p.cpb = ncell > 0 ? items_per_wg(a->B, ncell, 2, ivs::RK_MAX_CELLS, a->cells_per_wg) : 0;
    p.nchunk = ncell > 0 ? (ncell + p.cpb - 1) / p.cpb : 1;
    const int64_t grid = a->B * p.nchunk;                   // <= B * max(ncell, 1) < 2^31
    hipLaunchKernelGGL(ivs::svi_book_kernel, dim3((unsigned)grid), dim3(ivs::RK_BLOCK), 0, static_cast<hipStream_t>(stream), p);
    return end_call("svi_book_kernel");
}

int ivs_svi_explain_f64(const ivs_explain_args* a, void*, size_t, void* stream) {
    const char* fn = "ivs_svi_explain_f64";
    if (int rc = begin_call(fn, a)) return rc;
    if (int rc = check_query_shape(fn, a->B, a->mT, a->Q, a->tq_stride, a->q_stride, a->strike_mode)) return rc;
    if (a->lag < 1) return fail(IVS_ERANGE, "%s: lag=%d < 1", fn, a->lag);
    if (a->B <= a->lag || a->mT == 0 || a->Q == 0) return IVS_OK;                                  // X9
    if (!a->params || !a->Tq || !a->spot || !a->u || !a->tau || !a->qty || !a->net || !a->n_dead || !a->flags)
        return fail(IVS_EINVAL, "%s: null pointer", fn);
    if (int rc = check_query_launch(fn, "options", a->B, a->mT, a->Q, a->tq_stride, a->q_stride)) return rc;
    ivs::ExplainParams p{};
    set_query_fields(p, a);
    p.lag = a->lag;
    p.out[0] = a->actual; p.out[1] = a->theta_pnl; p.out[2] = a->delta_ss; p.out[3] = a->gamma_ss; p.out[4] = a->vega_ss;
    p.out[5] = a->resid_ss; p.out[6] = a->delta_sm; p.out[7] = a->gamma_sm; p.out[8] = a->vega_sm; p.out[9] = a->resid_sm;
    p.net = a->net; p.n_dead = a->n_dead; p.flags = a->flags;
    const int64_t pairs = a->B - a->lag;                    // one workgroup each; P * Q <= B * Q < 2^31
    hipLaunchKernelGGL(ivs::svi_explain_kernel, dim3((unsigned)pairs), dim3(ivs::RK_BLOCK), 0, static_cast<hipStream_t>(stream), p);
    return end_call("svi_explain_kernel");
}

int ivs_svi_hsim_f64(const ivs_hsim_args* a, void*, size_t, void* stream) {
    const char* fn = "ivs_svi_hsim_f64";
    if (int rc = begin_call(fn, a)) return rc;
    if (a->nL < 0) return fail(IVS_EINVAL, "%s: negative size", fn);
    if (int rc = check_query_shape(fn, a->B, a->mT, a->Q, a->tq_stride, a->q_stride, a->strike_mode)) return rc;
    if (a->lag < 1) return fail(IVS_ERANGE, "%s: lag=%d < 1", fn, a->lag);
    if (a->window < 1 || a->window > ivs::HS_MAX_WINDOW)
        return fail(IVS_ERANGE, "%s: window=%d outside [1,%d]", fn, a->window, ivs::HS_MAX_WINDOW);
    if (a->nL > ivs::HS_MAX_LEVELS) return fail(IVS_ERANGE, "%s: nL=%d > %d tail probabilities", fn, a->nL, ivs::HS_MAX_LEVELS);
    if (a->nL > 0 && !a->tail_probs) return fail(IVS_EINVAL, "%s: null tail probabilities", fn);
    for (int l = 0; l < a->nL; ++l)
        if (!(a->tail_probs[l] > 0.0 && a->tail_probs[l] < 1.0))
            return fail(IVS_ERANGE, "%s: tail probability %d (%g) is not inside (0, 1)", fn, l, a->tail_probs[l]);
    if (a->min_scen < 1) return fail(IVS_ERANGE, "%s: min_scen=%d < 1", fn, a->min_scen);
    if (a->scen_per_wg < 0 || a->scen_per_wg > a->window)
        return fail(IVS_ERANGE, "%s: scen_per_wg=%d outside [0,%d]", fn, a->scen_per_wg, a->window);
    if (a->stages < 0 || a->stages > 2) return fail(IVS_ERANGE, "%s: stages=%d outside [0,2]", fn, a->stages);
    if (a->B == 0 || a->mT == 0 || a->Q == 0) return IVS_OK;                                       // H9
    if (!a->params || !a->Tq || !a->spot || !a->u || !a->tau || !a->qty || !a->pnl || !a->scen_flags || !a->n_valid || !a->n_dead ||
        !a->worst || (a->nL > 0 && (!a->var || !a->es)))
        return fail(IVS_EINVAL, "%s: null pointer", fn);
    if (int rc = check_query_launch(fn, "options", a->B, a->mT, a->Q, a->tq_stride, a->q_stride)) return rc;
    if (a->B > 0x7fffffffLL / a->window)
        return fail(IVS_ERANGE, "%s: %lld x %d scenarios exceed one launch", fn, (long long)a->B, a->window);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a->stages != 2) {
        ivs::HsimParams p{};
        set_query_fields(p, a);
        p.lag = a->lag; p.window = a->window;
        p.pnl = a->pnl; p.scen_flags = a->scen_flags; p.value = a->value; p.n_dead = a->n_dead;
        // scenarios per workgroup: the whole window while the snapshots alone give every CU sixteen workgroups.  Sixteen, not
        // the book's two: a workgroup that takes 256 scenarios of a 1024-option book runs for milliseconds, and with only five
        // rounds of them per CU the last round stands half empty (131.0 ms against 126.4 ms with runs of 128 or 64 on the
        // bench of DESIGN.md section 19).
        p.spw = items_per_wg(a->B, a->window, 16, a->window, a->scen_per_wg);
        p.nchunk = (a->window + p.spw - 1) / p.spw;
        const int64_t grid = a->B * p.nchunk;                   // <= B * window < 2^31
        hipLaunchKernelGGL(ivs::svi_hsim_kernel, dim3((unsigned)grid), dim3(ivs::RK_BLOCK), 0, st, p);
        if (int rc = end_call("svi_hsim_kernel")) return rc;
    }
    if (a->stages != 1) {
        ivs::HsimTailParams t{};
        t.pnl = a->pnl; t.scen_flags = a->scen_flags; t.window = a->window; t.nL = a->nL; t.min_scen = a->min_scen;
        for (int l = 0; l < a->nL; ++l) t.tp[l] = a->tail_probs[l];
        t.var = a->var; t.es = a->es; t.n_valid = a->n_valid; t.worst = a->worst;
        hipLaunchKernelGGL(ivs::hsim_tail_kernel, dim3((unsigned)a->B), dim3(ivs::RK_BLOCK), 0, st, t);
        return end_call("hsim_tail_kernel");
    }
    return IVS_OK;
}

int ivs_svi_hsim_attrib_f64(const ivs_hsim_attrib_args* a, void*, size_t, void* stream) {
    const char* fn = "ivs_svi_hsim_attrib_f64";
    if (int rc = begin_call(fn, a)) return rc;
    if (a->nL < 0) return fail(IVS_EINVAL, "%s: negative size", fn);
    if (int rc = check_query_shape(fn, a->B, a->mT, a->Q, a->tq_stride, a->q_stride, a->strike_mode)) return rc;
    if (a->lag < 1) return fail(IVS_ERANGE, "%s: lag=%d < 1", fn, a->lag);
    if (a->window < 1 || a->window > ivs::HS_MAX_WINDOW)
        return fail(IVS_ERANGE, "%s: window=%d outside [1,%d]", fn, a->window, ivs::HS_MAX_WINDOW);
    if (a->nL > ivs::HS_MAX_LEVELS) return fail(IVS_ERANGE, "%s: nL=%d > %d tail probabilities", fn, a->nL, ivs::HS_MAX_LEVELS);
    if (a->nL > 0 && !a->tail_probs) return fail(IVS_EINVAL, "%s: null tail probabilities", fn);
    for (int l = 0; l < a->nL; ++l)
        if (!(a->tail_probs[l] > 0.0 && a->tail_probs[l] < 1.0))
            return fail(IVS_ERANGE, "%s: tail probability %d (%g) is not inside (0, 1)", fn, l, a->tail_probs[l]);
    if (a->min_scen < 1) return fail(IVS_ERANGE, "%s: min_scen=%d < 1", fn, a->min_scen);
    if (a->nG < 1 || a->nG > ivs::HA_MAX_GROUPS) return fail(IVS_ERANGE, "%s: nG=%d outside [1,%d]", fn, a->nG, ivs::HA_MAX_GROUPS);
    for (int l = 0; l < a->nL; ++l) {                                                              // A7, formed as H7 forms m
        const int m = (int)__builtin_floor((double)a->window * a->tail_probs[l]);
        if ((m < 1 ? 1 : m) > ivs::HA_MAX_TAIL)
            return fail(IVS_ERANGE, "%s: tail probability %d (%g) of window=%d is a tail of %d > %d scenarios", fn, l, a->tail_probs[l],
                        a->window, m, ivs::HA_MAX_TAIL);
    }
    if (a->B == 0 || a->mT == 0 || a->Q == 0) return IVS_OK;                                       // A8
    if (!a->params || !a->Tq || !a->spot || !a->u || !a->tau || !a->qty || !a->pnl || !a->scen_flags || (a->nL > 0 && !a->n_tail))
        return fail(IVS_EINVAL, "%s: null pointer", fn);
    if (int rc = check_query_launch(fn, "options", a->B, a->mT, a->Q, a->tq_stride, a->q_stride)) return rc;
    if (a->B > 0x7fffffffLL / a->window)
        return fail(IVS_ERANGE, "%s: %lld x %d scenarios exceed one launch", fn, (long long)a->B, a->window);
    ivs::HsimAttribParams p{};
    set_query_fields(p, a);
    p.lag = a->lag; p.window = a->window; p.nL = a->nL; p.min_scen = a->min_scen; p.nG = a->nG;
    for (int l = 0; l < a->nL; ++l) p.tp[l] = a->tail_probs[l];
    p.pnl = a->pnl; p.scen_flags = a->scen_flags; p.group = a->group;
    p.ces = a->ces; p.cvar = a->cvar; p.ces_group = a->ces_group; p.cvar_group = a->cvar_group;
    p.n_tail = a->n_tail; p.order = a->order;
    hipLaunchKernelGGL(ivs::svi_hsim_attrib_kernel, dim3((unsigned)a->B), dim3(ivs::RK_BLOCK), 0, static_cast<hipStream_t>(stream), p);
    return end_call("svi_hsim_attrib_kernel");
}

int ivs_ssvi_surface_f64(const ivs_ssvi_args* a, void*, size_t, void* stream) {
    const char* fn = "ivs_ssvi_surface_f64";
    if (int rc = begin_call(fn, a)) return rc;
    if (a->B < 0 || a->mT < 0 || a->mK < 0 || a->kq_stride < 0 || a->tq_stride < 0) return fail(IVS_EINVAL, "%s: negative size", fn);
    if ((a->raw != nullptr) == (a->theta0 != nullptr))
        return fail(IVS_EINVAL, "%s: exactly one of raw and theta0 must be given", fn);
    if (a->mT > ivs::SS_MAX_T) return fail(IVS_ERANGE, "%s: mT=%d > %d tenors of one ballot", fn, a->mT, ivs::SS_MAX_T);
    if (a->mK < 1) return fail(IVS_ERANGE, "%s: mK=%d < 1", fn, a->mK);
    if ((int64_t)a->mT * a->mK > ivs::SS_MAX_NODES)
        return fail(IVS_ERANGE, "%s: mT*mK=%lld > %d nodes of the LDS", fn, (long long)a->mT * a->mK, ivs::SS_MAX_NODES);
    if (a->rounds < 0 || a->rounds > ivs::SS_MAX_ROUNDS)
        return fail(IVS_ERANGE, "%s: rounds=%d outside [0,%d]", fn, a->rounds, ivs::SS_MAX_ROUNDS);
    if (a->B == 0 || a->mT == 0) return IVS_OK;
    if (!a->vol || !a->Kq || !a->Tq || !a->spot || !a->surface || !a->theta || !a->params || !a->fit || !a->flags || !a->sflags)
        return fail(IVS_EINVAL, "%s: null pointer", fn);
    if (int rc = check_grid_stride(fn, a->kq_stride, a->mK)) return rc;
    if (int rc = check_grid_stride(fn, a->tq_stride, a->mT)) return rc;
    if (a->B > 0x7fffffffLL / ((int64_t)a->mT * a->mK))
        return fail(IVS_ERANGE, "%s: %lld x %d x %d nodes exceed one launch", fn, (long long)a->B, a->mT, a->mK);
    ivs::SsviParams p{};
    p.vol = a->vol; p.Kq = a->Kq; p.Tq = a->Tq; p.spot = a->spot; p.raw = a->raw; p.theta0 = a->theta0;
    p.kq_stride = a->kq_stride; p.tq_stride = a->tq_stride; p.rate = a->rate;
    p.mK = a->mK; p.mT = a->mT;
    p.rounds = a->rounds == 0 ? ivs::SS_DEFAULT_ROUNDS : a->rounds;
    p.surface = a->surface; p.theta = a->theta; p.params = a->params; p.fit = a->fit;
    p.flags = a->flags; p.sflags = a->sflags; p.fitted = a->fitted;
    const size_t lds = (size_t)a->mT * a->mK * 16;          // one workgroup per snapshot, its valid nodes in LDS
    hipLaunchKernelGGL(ivs::ssvi_surface_kernel, dim3((unsigned)a->B), dim3(ivs::SS_THREADS), lds,
                       static_cast<hipStream_t>(stream), p);
    return end_call("ssvi_surface_kernel");
}

int ivs_candle_aggregate_f64(const int64_t* ts_ns, const double* open, const double* high, const double* low,
                             const double* close, const double* volume, const int64_t* series_off, int64_t n_series,
                             int64_t n_rows, int64_t freq_ns, int64_t* out_ts, double* out_open, double* out_high,
                             double* out_low, double* out_close, double* out_volume, int32_t* out_count, void* stream) {
    g_err[0] = 0;
    if (n_rows < 0 || n_series < 0 || freq_ns <= 0) return fail(IVS_EINVAL, "ivs_candle_aggregate_f64: bad size / frequency");
    if (n_rows == 0 || n_series == 0) return IVS_OK;
    if (!ts_ns || !open || !high || !low || !close || !volume || !series_off || !out_ts || !out_open || !out_high ||
        !out_low || !out_close || !out_volume || !out_count)
        return fail(IVS_EINVAL, "ivs_candle_aggregate_f64: null pointer");
    if ((n_rows + 255) / 256 > 0x7fffffffLL) return fail(IVS_ERANGE, "ivs_candle_aggregate_f64: too many rows");
    ivs::CandleParams p{ts_ns, open, high, low, close, volume, series_off, n_series, n_rows, freq_ns,
                        out_ts, out_open, out_high, out_low, out_close, out_volume, out_count};
    hipLaunchKernelGGL(ivs::candle_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), p);
    return check_launch("candle_kernel");
}

size_t ivs_bridge_workspace_bytes(int64_t total_rows) { return ivs::bridge_ws_bytes(total_rows < 0 ? 0 : total_rows); }

int ivs_mt19937_words_u32(uint32_t seed, uint32_t* words, int64_t n_words, void* stream) {
    g_err[0] = 0;
    if (n_words < 0) return fail(IVS_EINVAL, "ivs_mt19937_words_u32: negative size");
    if (n_words == 0) return IVS_OK;
    if (!words) return fail(IVS_EINVAL, "ivs_mt19937_words_u32: null pointer");
    hipLaunchKernelGGL(ivs::mt19937_words_kernel, dim3(1), dim3(ivs::MT_THREADS), 0, static_cast<hipStream_t>(stream), seed, words, n_words);
    return check_launch("mt19937_words_kernel");
}

int ivs_bridge_candles_f64(const double* price, const double* volume, const int64_t* row_off, int64_t S,
                           int64_t total_rows, int32_t strategy, double base_spread_pct, double vol_factor,
                           const uint32_t* words, int64_t n_words, double* out, uint8_t* valid, int64_t* rng_tail,
                           void* workspace, size_t workspace_bytes, void* stream) {
    g_err[0] = 0;
    if (S < 0 || total_rows < 0 || n_words < 0) return fail(IVS_EINVAL, "ivs_bridge_candles_f64: negative size");
    if (strategy < 0 || strategy > 4) return fail(IVS_EINVAL, "ivs_bridge_candles_f64: unknown strategy %d", strategy);
    if (!rng_tail) return fail(IVS_EINVAL, "ivs_bridge_candles_f64: null rng_tail");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (S == 0 || total_rows == 0) {
        if (hipMemsetAsync(rng_tail, 0, 8, st) != hipSuccess || hipMemsetAsync(rng_tail + 3, 0, 8, st) != hipSuccess)
            return fail(IVS_ELAUNCH, "ivs_bridge_candles_f64: memset failed");
        return IVS_OK;
    }
    if (!price || !row_off || !words || !out || !valid || !workspace)
        return fail(IVS_EINVAL, "ivs_bridge_candles_f64: null pointer");
    if (workspace_bytes < ivs::bridge_ws_bytes(total_rows)) return fail(IVS_ENOMEM, "ivs_bridge_candles_f64: workspace too small");
    const int64_t nb = ivs::bridge_blocks(total_rows);
    if (nb > 0x7fffffffLL) return fail(IVS_ERANGE, "ivs_bridge_candles_f64: too many rows");
    if (n_words > 0x7fffffffLL) return fail(IVS_ERANGE, "ivs_bridge_candles_f64: %lld words exceed the int32 per-row stream offsets", (long long)n_words);
    auto align64 = [](uintptr_t a) { return (a + 63) & ~(uintptr_t)63; };
    uintptr_t w = align64(reinterpret_cast<uintptr_t>(workspace));
    ivs::BridgeParams p;
    p.price = price; p.volume = volume; p.row_off = row_off; p.S = S; p.total_rows = total_rows;
    p.strategy = strategy; p.base_spread_pct = base_spread_pct; p.vol_factor = vol_factor;
    p.words = words; p.n_words = n_words; p.out = out; p.valid = valid; p.rng_tail = rng_tail;
    p.woff = reinterpret_cast<int32_t*>(w); w = align64(w + (size_t)total_rows * 4);
    p.bbase = reinterpret_cast<int64_t*>(w); w = align64(w + (size_t)(nb + 1) * 8);
    p.gauss = reinterpret_cast<double*>(w); w = align64(w + (size_t)total_rows * 8);
    p.expu = reinterpret_cast<double*>(w); w = align64(w + (size_t)total_rows * 8);
    p.acc = reinterpret_cast<uint8_t*>(w); w = align64(w + ivs::bridge_acc_capacity(total_rows));
    p.gauss0 = reinterpret_cast<double*>(w);
    if (hipMemsetAsync(rng_tail + 3, 0, 8, st) != hipSuccess) return fail(IVS_ELAUNCH, "ivs_bridge_candles_f64: memset failed");
    if (strategy == ivs::BR_TREND) {
        int64_t nd = n_words / 2;                                   // doubles of the stream this call may look at
        const int64_t cap = (int64_t)ivs::bridge_acc_capacity(total_rows);
        if (nd > cap) { nd = cap; p.n_words = 2 * nd; }
        int64_t ab = ivs::capped_blocks(nd, num_cu());
        if (ab < 1) ab = 1;
        hipLaunchKernelGGL(ivs::bridge_accept_kernel, dim3((unsigned)ab), dim3(256), 0, st, p, nd);
        hipLaunchKernelGGL(ivs::bridge_gauss_walk_kernel, dim3(1), dim3(64), 0, st, p, nd);
    } else {
        hipLaunchKernelGGL(ivs::bridge_count_kernel, dim3((unsigned)nb), dim3(256), 0, st, p);
        hipLaunchKernelGGL(ivs::bridge_scan_blocks_kernel, dim3(1), dim3(256), 0, st, p, nb);
    }
    int64_t grid = (int64_t)num_cu() * 8;
    if (grid > S) grid = S;
    ivs::with_method(strategy, ivs::Methods<ivs::BR_SPREAD, ivs::BR_MIDPOINT, ivs::BR_TREND, ivs::BR_SIMPLE, ivs::BR_PIPELINE>{}, [&](auto strat) {
        hipLaunchKernelGGL(ivs::bridge_candles_kernel<decltype(strat)::value>, dim3((unsigned)grid), dim3(64), 0, st, p);
    });
    return check_launch("bridge_candles_kernel");
}

int ivs_bs_greeks_f64(const double* S, const double* K, const double* T, const double* r, const double* sigma,
                      const uint8_t* is_put, int32_t default_is_put, int64_t n, double* delta, double* gamma,
                      double* theta, double* vega, double* rho, void* stream) {
    g_err[0] = 0;
    if (n < 0) return fail(IVS_EINVAL, "ivs_bs_greeks_f64: negative size");
    if (n == 0) return IVS_OK;
    if (!S || !K || !T || !r || !sigma || !delta || !gamma || !theta || !vega || !rho)
        return fail(IVS_EINVAL, "ivs_bs_greeks_f64: null pointer");
    ivs::GreeksParams p{S, K, T, r, sigma, is_put, default_is_put, n, delta, gamma, theta, vega, rho};
    hipLaunchKernelGGL(ivs::greeks_kernel, dim3((unsigned)ivs::capped_blocks(n, num_cu())), dim3(256), 0, static_cast<hipStream_t>(stream), p);
    return check_launch("greeks_kernel");
}

int ivs_bs_price_f64(const double* S, const double* K, const double* T, const double* r, const double* sigma,
                     const uint8_t* is_put, int32_t default_is_put, int64_t n, double* price, double* vega, int32_t* flags,
                     void* stream) {
    const char* fn = "ivs_bs_price_f64";
    g_err[0] = 0;
    g_last_kernel = "";
    if (n < 0) return fail(IVS_EINVAL, "%s: negative size n=%lld", fn, (long long)n);
    if (n > 0x7fffffffLL) return fail(IVS_ERANGE, "%s: n=%lld options exceed one launch", fn, (long long)n);
    if (n == 0) return IVS_OK;
    if (!S || !K || !T || !r || !sigma || !price) return fail(IVS_EINVAL, "%s: null pointer", fn);
    ivs::BsPriceParams p{S, K, T, r, sigma, is_put, default_is_put, n, price, vega, flags};
    hipLaunchKernelGGL(ivs::bs_price_kernel, dim3((unsigned)ivs::capped_blocks(n, num_cu())), dim3(256), 0, static_cast<hipStream_t>(stream), p);
    g_last_kernel = "bs_price_kernel";
    return check_launch("bs_price_kernel");
}

int ivs_bs_implied_vol_f64(const double* price, const double* S, const double* K, const double* T, const double* r,
                           const uint8_t* is_put, int32_t default_is_put, int32_t price_mode, int64_t n, double* vol,
                           int32_t* flags, void* stream) {
    const char* fn = "ivs_bs_implied_vol_f64";
    g_err[0] = 0;
    g_last_kernel = "";
    if (n < 0) return fail(IVS_EINVAL, "%s: negative size n=%lld", fn, (long long)n);
    if (price_mode != 0 && price_mode != 1) return fail(IVS_EINVAL, "%s: price_mode=%d is neither 0 nor 1", fn, price_mode);
    if (n > 0x7fffffffLL) return fail(IVS_ERANGE, "%s: n=%lld options exceed one launch", fn, (long long)n);
    if (n == 0) return IVS_OK;
    if (!price || !S || !K || !T || !r || !vol || !flags) return fail(IVS_EINVAL, "%s: null pointer", fn);
    ivs::ImpliedParams p{price, S, K, T, r, is_put, default_is_put, price_mode, n, vol, flags};
    hipLaunchKernelGGL(ivs::bs_implied_vol_kernel, dim3((unsigned)ivs::capped_blocks(n, num_cu())), dim3(256), 0, static_cast<hipStream_t>(stream), p);
    g_last_kernel = "bs_implied_vol_kernel";
    return check_launch("bs_implied_vol_kernel");
}

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
