// What the surface launchers share across translation units: the launch context, the workspace layout, and the
// declarations of the launchers that one unit defines and another calls (hidden: none of them is exported).  The two
// inline functions are arithmetic on sizes; nothing in this header launches or names a kernel.
#pragma once
#include "ivs_dispatch.hpp"
#include "ivs_surface_dense_var.hpp"

namespace ivs {

// Everything a launcher needs from the entry point: the CURRENT device (index, CU count), the caller's stream and
// workspace, and the tuning override of the surface -> workgroup mapping (flags bits 8..15).  No process-global state:
// the kernel attribute that unlocks > 64 KiB of dynamic LDS is per device and is tracked per device (ensure_max_lds).
struct LaunchCtx {
    int dev = 0, num_cu = 256;
    hipStream_t st = nullptr;
    unsigned char* ws = nullptr;
    size_t ws_bytes = 0;
    int map_groups = 0;
    unsigned long long* stamps = nullptr;            // diagnostics (ivs_debug_stamps): buffer of the stamped dense kernel
    int64_t* grid_out = nullptr;                     // diagnostics (ivs_debug_last_grid): receives the dense kernel's grid
};
constexpr size_t WS_TQ_BYTES = 8192;                 // TqShared at offset 0
constexpr size_t WS_COUNTS_BYTES = 256;              // ragged: per-class counters
constexpr int V_NCLASS = 4;                          // ragged: work lists (one per size class), B items each
static_assert(sizeof(TqShared) <= WS_TQ_BYTES, "TqShared must fit its workspace slot");
inline size_t surface_ws_bytes(int64_t B, bool ragged) {
    return WS_TQ_BYTES + (ragged ? WS_COUNTS_BYTES + (size_t)V_NCLASS * (size_t)(B < 0 ? 0 : B) * 16 : 0);
}

// number of workgroup groups (= regions of the batch = work-queue heads; see the mapping comment in surface_dense_kernel);
// `forced` > 0 is the caller's IVS_FLAG_MAP_GROUPS override (experiments).  With static striding small batches had to fall
// back to one group (uneven shares); with the work queues they must NOT: one head for 3072 workgroups runs at the atomic
// unit's pace (a 125 000-surface shard -- config 3 split over 8 GPUs -- ran at 252 instead of 317 M surfaces/s).
inline int dense_map_groups(int64_t grid, int64_t B, int forced) {
    int r = forced > 0 ? forced : 8;
    if (r > 16) r = 16;                                   // queue heads in the workspace
    while (r > 1 && (B < (int64_t)r * 256 || grid < r)) r >>= 1;      // tiny batches / grids: fewer, fuller regions
    return r < 1 ? 1 : r;
}

using TableMethods = Methods<IVS_LINEAR, IVS_CUBIC, IVS_CUBICSPLINE, IVS_SLINEAR, IVS_PCHIP, IVS_AKIMA, IVS_NEAREST, IVS_ZERO,
                             IVS_FROM_DERIVATIVES, IVS_QUADRATIC>;                                             // tq_tables_kernel, row-pass kernels
using DenseMethods = Methods<IVS_LINEAR, IVS_CUBIC, IVS_CUBICSPLINE, IVS_SLINEAR, IVS_PCHIP, IVS_AKIMA>;      // the one-pass kernels

struct VarWork { VarList wl1, wl2; bool need1, need2; };      // the work lists of a call (var_work_lists)

#pragma GCC visibility push(hidden)
// the set-up (ivs_surface_tables_launch.hpp) and the tail (ivs_surface_tail_launch.hpp) every fast path calls
template <bool NTR> bool launch_tq_or_zero_queue(SurfaceParams& p, const LaunchCtx& cx, bool tsh, bool set_mode);
bool var_work_lists(const SurfaceParams& p, const LaunchCtx& cx, VarWork& w);
void launch_redo_tail(SurfaceParams& p, const LaunchCtx& cx, bool fixed64);
// the fast paths: 1 = dispatched, 0 = not covered, -1 = launch error; *family: the kernel's name without its method
int launch_surface_pass(const SurfaceParams& p_in, const LaunchCtx& cx, const char** family);            // ivs_surface_pass_launch.hpp
int launch_surface_dense(const SurfaceParams& p_in, const LaunchCtx& cx, const char** family);           // ivs_surface_dense.hip
int launch_surface_dense_var(const SurfaceParams& p_in, const LaunchCtx& cx, const char** family);       // ivs_surface_dense.hip
#pragma GCC visibility pop

}  // namespace ivs
