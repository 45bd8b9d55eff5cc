// Internal to libivs.so: the per-thread call state and the host-side checks that the units of entry points share.
// Everything here is defined once, in ivs_host.hip, and has hidden visibility: none of it is exported.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/ivs.h"

#pragma GCC visibility push(hidden)
namespace ivs::host {

// constant-initialised, and declared so: a unit that uses one reads it directly, with no call to an initialiser
#define IVS_TLS __attribute__((require_constant_initialization)) thread_local
extern IVS_TLS char g_err[512];                      // ivs_last_error()
extern IVS_TLS const char* g_last_kernel;            // ivs_last_kernel()
extern IVS_TLS unsigned long long* g_stamp_buf;      // ivs_debug_stamps()
extern IVS_TLS int64_t g_stamp_cap;
extern IVS_TLS int64_t g_last_grid;                  // ivs_debug_last_grid()

int fail(int code, const char* fmt, ...);
int check_launch(const char* what);
void set_last_kernel(const char* family, int method);
bool valid_method(int m);
void current_device(int& dev, int& cus);
int num_cu();

int begin_call(const char* fn, const void* args);
int end_call(const char* kernel);
int check_grid_stride(const char* fn, int64_t stride, int64_t len);
int check_rows(const char* fn, int64_t B, int32_t mT);
int32_t rows_per_wave(int64_t rows, int cap, int forced);
int check_query_shape(const char* fn, int64_t B, int32_t mT, int64_t Q, int64_t tq_stride, int64_t q_stride, int32_t strike_mode);
int check_query_launch(const char* fn, const char* noun, int64_t B, int32_t mT, int64_t Q, int64_t tq_stride, int64_t q_stride);
int items_per_wg(int64_t B, int n, int per_cu, int cap, int forced);

}  // namespace ivs::host
#pragma GCC visibility pop
