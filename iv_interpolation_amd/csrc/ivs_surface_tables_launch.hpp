// Launcher of tq_tables_kernel (ivs_surface_dense.hpp): the set-up step of every fast path.  Defines ordinary functions:
// exactly one unit of a library includes it (ivs_surface_dense.hip, beside the kernels that share the T-phase;
// tools/pass_api.hip for the diagnostic libraries).
#pragma once
#include "ivs_surface_launch.hpp"

namespace ivs {

template <bool NTR>
inline void launch_tq_tables(const SurfaceParams& p, TqShared* o, hipStream_t st) {
    with_method(p.method, TableMethods{}, [&](auto m) {
        hipLaunchKernelGGL((tq_tables_kernel<decltype(m)::value, NTR>), dim3(1), dim3(64), 0, st, p, o);
    });
}

// Maturity tables and queue heads of a call, shared by the surface launchers.  Shared T / Tq: the batch-wide tables go
// into the workspace on the same stream (NTR: run-time maturity count; the table kernel also zeroes the queue heads);
// per-surface maturities: no table kernel runs, the queue heads are zeroed here.  Returns false on a stream error.
template <bool NTR>
inline bool launch_tq_or_zero_queue(SurfaceParams& p, const LaunchCtx& cx, bool tsh, bool set_mode) {
    TqShared* tq = reinterpret_cast<TqShared*>(cx.ws);
    if (tsh) {
        launch_tq_tables<NTR>(p, tq, cx.st);
        p.tqs = tq;
        p.redo = tq->redo;
        p.mode = set_mode ? &tq->mode : nullptr;
    } else {
        if (hipMemsetAsync(tq->queue, 0, sizeof(TqShared::queue), cx.st) != hipSuccess) return false;
        p.tqs = nullptr;
        p.redo = nullptr;
    }
    p.queue = tq->queue;
    return true;
}
template bool launch_tq_or_zero_queue<false>(SurfaceParams&, const LaunchCtx&, bool, bool);
template bool launch_tq_or_zero_queue<true>(SurfaceParams&, const LaunchCtx&, bool, bool);

}  // namespace ivs
