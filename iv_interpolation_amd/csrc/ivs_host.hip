// Host unit of libivs.so: the per-thread call state, the checks and launch steps the units of entry points share
// (declared in ivs_host.hpp), and the entry points that launch nothing.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "ivs_dispatch.hpp"
#include "ivs_host.hpp"
#include "ivs_surface_dense.hpp"      // D_NSTAMP, TqShared

namespace ivs::host {

IVS_TLS char g_err[512] = "";
IVS_TLS const char* g_last_kernel = "";
// diagnostics (ivs_debug_stamps): per calling thread, like the error string
IVS_TLS unsigned long long* g_stamp_buf = nullptr;   // device buffer for the diagnostic (stamped) dense kernel
IVS_TLS int64_t g_stamp_cap = 0;
IVS_TLS int64_t g_last_grid = 0;
namespace {
thread_local char g_kernel_name[64] = "";             // ivs_last_kernel() of the surface fast paths: family<method>
}

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
namespace {
std::atomic<int> g_cu[ivs::IVS_MAX_DEV];
}
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

}  // namespace ivs::host

using namespace ivs::host;

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

}  // extern "C"
