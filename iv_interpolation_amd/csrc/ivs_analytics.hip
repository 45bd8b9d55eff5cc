// Unit of libivs.so: the snapshot analytics (snapshot, smile, arbitrage, moments, SVI, SSVI, distribution, calendar,
// evaluation, the book family), the Black-Scholes calls, candles and the bridge.
// Argument validation happens here on the host; kernels assume validated shapes.
#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>

#include "ivs_arbitrage.hpp"
#include "ivs_bootstrap.hpp"
#include "ivs_bridge.hpp"
#include "ivs_candles.hpp"
#include "ivs_dispatch.hpp"
#include "ivs_distribution.hpp"
#include "ivs_explain.hpp"
#include "ivs_greeks.hpp"
#include "ivs_hedge.hpp"
#include "ivs_host.hpp"
#include "ivs_hsim.hpp"
#include "ivs_hsim_attrib.hpp"
#include "ivs_hsim_weighted.hpp"
#include "ivs_implied.hpp"
#include "ivs_moments.hpp"
#include "ivs_risk.hpp"
#include "ivs_smile.hpp"
#include "ivs_snapshot.hpp"
#include "ivs_ssvi.hpp"
#include "ivs_svi.hpp"
#include "ivs_svi_surface.hpp"
#include "ivs_whatif.hpp"

using namespace ivs::host;

namespace {

// what the kernels' params of ivs_svi_eval_f64, ivs_svi_greeks_f64, ivs_svi_book_f64, ivs_svi_explain_f64 and the hsim calls take
// over from the args field for field: the names agree; svi_eval has no sides, and neither it nor svi_greeks has quantities
template <class P, class A>
void set_query_fields(P& p, const A* a) {
    p.params = a->params; p.Tq = a->Tq; p.spot = a->spot; p.u = a->u; p.tau = a->tau;
    p.tq_stride = a->tq_stride; p.q_stride = a->q_stride; p.rate = a->rate;
    p.mT = a->mT; p.strike_mode = a->strike_mode; p.Q = a->Q;
    if constexpr (!std::is_same_v<P, ivs::EvalParams>) p.is_put = a->is_put;
    if constexpr (!std::is_same_v<P, ivs::EvalParams> && !std::is_same_v<P, ivs::RiskParams>) p.qty = a->qty;
}

// stage 1 of the hedge and of the what-if ladder (M2, W2): svi_inst_pnl_kernel on the candidates of either args struct
template <class A>
int launch_inst_pnl(const A* a, hipStream_t st) {
    ivs::InstPnlParams p{};
    p.params = a->params; p.Tq = a->Tq; p.spot = a->spot; p.inst_u = a->inst_u; p.inst_tau = a->inst_tau; p.inst_kind = a->inst_kind;
    p.tq_stride = a->tq_stride; p.inst_stride = a->inst_stride; p.rate = a->rate;
    p.mT = a->mT; p.strike_mode = a->strike_mode; p.lag = a->lag; p.window = a->window; p.nH = a->nH;
    p.inst_pnl = a->inst_pnl; p.inst_value = a->inst_value;
    // scenarios per workgroup: a workgroup is one wavefront, so thirty-two of them per CU before the runs are cut shorter (at
    // lag 1 a long run stages and brackets every snapshot once, a short one its first end twice)
    p.spw = items_per_wg(a->B, a->window, 32, a->window, a->scen_per_wg);
    p.nchunk = (a->window + p.spw - 1) / p.spw;
    const int64_t grid = a->B * p.nchunk;                   // <= B * window < 2^31
    hipLaunchKernelGGL(ivs::svi_inst_pnl_kernel, dim3((unsigned)grid), dim3(64), 0, st, p);
    return end_call("svi_inst_pnl_kernel");
}

}  // namespace

extern "C" {

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

int ivs_svi_hedge_f64(const ivs_hedge_args* a, void*, size_t, void* stream) {
    const char* fn = "ivs_svi_hedge_f64";
    if (int rc = begin_call(fn, a)) return rc;
    if (a->nL < 0) return fail(IVS_EINVAL, "%s: negative size", fn);
    if (int rc = check_query_shape(fn, a->B, a->mT, a->nH, a->tq_stride, a->inst_stride, a->strike_mode)) return rc;
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
    if (a->nH > ivs::HG_MAX_INST) return fail(IVS_ERANGE, "%s: nH=%d > %d candidates", fn, a->nH, ivs::HG_MAX_INST);
    if (a->rounds < 1 || a->rounds > ivs::HG_MAX_ROUNDS)
        return fail(IVS_ERANGE, "%s: rounds=%d outside [1,%d]", fn, a->rounds, ivs::HG_MAX_ROUNDS);
    if (a->n_forced < 0 || a->n_forced > a->rounds || a->n_forced > a->nH)
        return fail(IVS_ERANGE, "%s: n_forced=%d outside [0,min(rounds=%d, nH=%d)]", fn, a->n_forced, a->rounds, a->nH);
    if (!(a->tol >= 0.0 && a->tol < 1.0)) return fail(IVS_ERANGE, "%s: tol=%g is not inside [0, 1)", fn, a->tol);
    if (!(a->min_gain >= 0.0 && a->min_gain < __builtin_inf())) return fail(IVS_ERANGE, "%s: min_gain=%g is not finite and >= 0", fn, a->min_gain);
    if (a->stages < 0 || a->stages > 2) return fail(IVS_ERANGE, "%s: stages=%d outside [0,2]", fn, a->stages);
    if (a->nH > 0 && a->B > 0x7fffffffLL / ((int64_t)a->window * a->nH))
        return fail(IVS_ERANGE, "%s: %lld x %d x %d candidate scenarios exceed one launch", fn, (long long)a->B, a->window, a->nH);
    if (a->B == 0 || a->mT == 0 || a->nH == 0) return IVS_OK;                                      // M11
    if (!a->params || !a->Tq || !a->spot || !a->inst_u || !a->inst_tau || !a->inst_kind || !a->inst_pnl)
        return fail(IVS_EINVAL, "%s: null pointer", fn);
    if (a->stages != 1 && (!a->pnl || !a->scen_flags || !a->inst_flags || !a->pick || !a->ss || !a->n_rounds || !a->hedge || !a->pnl_hedged ||
                           !a->worst_h || !a->n_scen || (a->nL > 0 && (!a->var_h || !a->es_h))))
        return fail(IVS_EINVAL, "%s: null pointer", fn);
    if (int rc = check_query_launch(fn, "candidates", a->B, a->mT, a->nH, a->tq_stride, a->inst_stride)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a->stages != 2)
        if (int rc = launch_inst_pnl(a, st)) return rc;
    if (a->stages != 1) {
        ivs::PursuitParams p{};
        p.params = a->params; p.Tq = a->Tq; p.spot = a->spot; p.inst_u = a->inst_u; p.inst_tau = a->inst_tau; p.inst_kind = a->inst_kind;
        p.tq_stride = a->tq_stride; p.inst_stride = a->inst_stride; p.rate = a->rate; p.tol = a->tol; p.min_gain = a->min_gain;
        p.mT = a->mT; p.strike_mode = a->strike_mode; p.lag = a->lag; p.window = a->window; p.nH = a->nH;
        p.K = a->rounds; p.n_forced = a->n_forced; p.min_scen = a->min_scen;
        p.pnl = a->pnl; p.scen_flags = a->scen_flags; p.inst_pnl = a->inst_pnl;
        p.inst_flags = a->inst_flags; p.pick = a->pick; p.ss = a->ss; p.n_rounds = a->n_rounds;
        p.hedge = a->hedge; p.pnl_hedged = a->pnl_hedged; p.solo_qty = a->solo_qty; p.solo_left = a->solo_left;
        const size_t lds = (size_t)(a->rounds + 1) * a->window * sizeof(double);         // e and the directions: <= 72 KB
        // above 48 KB the kernel's limit on dynamic LDS is raised first: a function attribute, not a stream operation, set once per
        // size reached and remembered (so a call that repeats an earlier shape, a captured one included, makes no runtime call
        // besides its launches); a size the device refuses is reported by the launch itself
        static std::atomic<size_t> lds_allowed{48 * 1024};
        if (lds > lds_allowed.load(std::memory_order_relaxed)) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(ivs::hedge_pursuit_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds) == hipSuccess)
                lds_allowed.store(lds, std::memory_order_relaxed);
            else
                (void)hipGetLastError();
        }
        hipLaunchKernelGGL(ivs::hedge_pursuit_kernel, dim3((unsigned)a->B), dim3(64), lds, st, p);
        if (int rc = end_call("hedge_pursuit_kernel")) return rc;
        ivs::HsimTailParams t{};                                // H7 on the hedged row, the kernel as it is
        t.pnl = a->pnl_hedged; t.scen_flags = a->scen_flags; t.window = a->window; t.nL = a->nL; t.min_scen = a->min_scen;
        for (int l = 0; l < a->nL; ++l) t.tp[l] = a->tail_probs[l];
        t.var = a->var_h; t.es = a->es_h; t.n_valid = a->n_scen; t.worst = a->worst_h;
        hipLaunchKernelGGL(ivs::hsim_tail_kernel, dim3((unsigned)a->B), dim3(ivs::RK_BLOCK), 0, st, t);
        return end_call("hsim_tail_kernel");
    }
    return IVS_OK;
}

int ivs_svi_whatif_f64(const ivs_whatif_args* a, void*, size_t, void* stream) {
    const char* fn = "ivs_svi_whatif_f64";
    if (int rc = begin_call(fn, a)) return rc;
    if (a->nL < 0 || a->size_stride < 0) return fail(IVS_EINVAL, "%s: negative size", fn);
    if (int rc = check_query_shape(fn, a->B, a->mT, a->nH, a->tq_stride, a->inst_stride, a->strike_mode)) return rc;
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
    if (a->nH > ivs::HG_MAX_INST) return fail(IVS_ERANGE, "%s: nH=%d > %d candidates", fn, a->nH, ivs::HG_MAX_INST);
    if (a->nQ < 1 || a->nQ > ivs::WI_MAX_RUNGS) return fail(IVS_ERANGE, "%s: nQ=%d outside [1,%d]", fn, a->nQ, ivs::WI_MAX_RUNGS);
    if (a->stages < 0 || a->stages > 2) return fail(IVS_ERANGE, "%s: stages=%d outside [0,2]", fn, a->stages);
    if (a->nH > 0 && a->B > 0x7fffffffLL / ((int64_t)a->window * a->nH))
        return fail(IVS_ERANGE, "%s: %lld x %d x %d candidate scenarios exceed one launch", fn, (long long)a->B, a->window, a->nH);
    if (a->nH > 0 && a->B > 0x7fffffffLL / ((int64_t)a->nH * a->nQ * (a->nL > 0 ? a->nL : 1)))
        return fail(IVS_ERANGE, "%s: %lld x %d x %d rungs at %d levels exceed one launch", fn, (long long)a->B, a->nH, a->nQ, a->nL);
    if (a->size_stride != 0 && a->size_stride != (int64_t)a->nH * a->nQ)
        return fail(IVS_EINVAL, "%s: size_stride=%lld is neither 0 nor nH*nQ", fn, (long long)a->size_stride);
    if (a->B == 0 || a->mT == 0 || a->nH == 0) return IVS_OK;                                      // W9
    if (!a->params || !a->Tq || !a->spot || !a->inst_u || !a->inst_tau || !a->inst_kind || !a->inst_pnl)
        return fail(IVS_EINVAL, "%s: null pointer", fn);
    if (a->stages != 1 && (!a->pnl || !a->scen_flags || !a->size || !a->trade_flags || !a->worst0 || !a->n_scen ||
                           (a->nL > 0 && (!a->var_w || !a->es_w || !a->best || !a->var0 || !a->es0))))
        return fail(IVS_EINVAL, "%s: null pointer", fn);
    if (int rc = check_query_launch(fn, "candidates", a->B, a->mT, a->nH, a->tq_stride, a->inst_stride)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a->stages != 2)
        if (int rc = launch_inst_pnl(a, st)) return rc;                                            // W2
    if (a->stages != 1) {
        ivs::WhatIfParams p{};
        p.pnl = a->pnl; p.scen_flags = a->scen_flags; p.inst_pnl = a->inst_pnl; p.size = a->size; p.size_stride = a->size_stride;
        p.lag = a->lag; p.window = a->window; p.nH = a->nH; p.nQ = a->nQ; p.nL = a->nL; p.min_scen = a->min_scen;
        for (int l = 0; l < a->nL; ++l) p.tp[l] = a->tail_probs[l];
        p.trade_flags = a->trade_flags; p.var_w = a->var_w; p.es_w = a->es_w; p.worst_w = a->worst_w; p.best = a->best;
        p.var0 = a->var0; p.es0 = a->es0; p.worst0 = a->worst0; p.n_scen = a->n_scen;
        // candidates per workgroup: a wavefront takes one candidate at a time, so a workgroup takes four or more; all nH of a
        // snapshot while the snapshots alone give every CU eight workgroups, fewer below that (W8: the same bits)
        p.cpw = items_per_wg(a->B, (a->nH + ivs::WI_WAVES - 1) / ivs::WI_WAVES, 8, (a->nH + ivs::WI_WAVES - 1) / ivs::WI_WAVES, 0) * ivs::WI_WAVES;
        p.nchunk = (a->nH + p.cpw - 1) / p.cpw;
        const dim3 grid((unsigned)(a->B * p.nchunk)), block(ivs::WI_WAVES * 64);                   // <= B * nH < 2^31
        const int nw = (a->window + 63) / 64;                   // registers per lane: the row of a window is 64 x NW scenarios
        if (nw <= 1) hipLaunchKernelGGL(ivs::whatif_tail_kernel<1>, grid, block, 0, st, p);
        else if (nw <= 2) hipLaunchKernelGGL(ivs::whatif_tail_kernel<2>, grid, block, 0, st, p);
        else if (nw <= 4) hipLaunchKernelGGL(ivs::whatif_tail_kernel<4>, grid, block, 0, st, p);
        else if (nw <= 8) hipLaunchKernelGGL(ivs::whatif_tail_kernel<8>, grid, block, 0, st, p);
        else hipLaunchKernelGGL(ivs::whatif_tail_kernel<16>, grid, block, 0, st, p);
        return end_call("whatif_tail_kernel");
    }
    return IVS_OK;
}

// elements of replicate values per call: what rep, or the workspace in its place, holds
static int64_t bootstrap_rep_elems(int64_t B, int32_t n_rep, int32_t nL) { return B * n_rep * 2 * nL; }

size_t ivs_hsim_bootstrap_workspace_bytes(int64_t B, int32_t n_rep, int32_t nL) {
    if (B <= 0 || n_rep < 1 || n_rep > ivs::BT_MAX_REP || nL < 1 || nL > ivs::HS_MAX_LEVELS || B > 0x7fffffffLL / ((int64_t)n_rep * 2 * nL)) return 0;
    return (size_t)bootstrap_rep_elems(B, n_rep, nL) * sizeof(double);
}

int ivs_hsim_bootstrap_f64(const ivs_bootstrap_args* a, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "ivs_hsim_bootstrap_f64";
    if (int rc = begin_call(fn, a)) return rc;
    if (a->B < 0 || a->nL < 0 || a->nC < 0) return fail(IVS_EINVAL, "%s: negative size", fn);
    if (a->window < 1 || a->window > ivs::HS_MAX_WINDOW)
        return fail(IVS_ERANGE, "%s: window=%d outside [1,%d]", fn, a->window, ivs::HS_MAX_WINDOW);
    if (a->nL > ivs::HS_MAX_LEVELS) return fail(IVS_ERANGE, "%s: nL=%d > %d tail probabilities", fn, a->nL, ivs::HS_MAX_LEVELS);
    if (a->nL > 0 && !a->tail_probs) return fail(IVS_EINVAL, "%s: null tail probabilities", fn);
    for (int l = 0; l < a->nL; ++l)
        if (!(a->tail_probs[l] > 0.0 && a->tail_probs[l] < 1.0))
            return fail(IVS_ERANGE, "%s: tail probability %d (%g) is not inside (0, 1)", fn, l, a->tail_probs[l]);
    if (a->min_scen < 1) return fail(IVS_ERANGE, "%s: min_scen=%d < 1", fn, a->min_scen);
    if (a->n_rep < 1 || a->n_rep > ivs::BT_MAX_REP) return fail(IVS_ERANGE, "%s: n_rep=%d outside [1,%d]", fn, a->n_rep, ivs::BT_MAX_REP);
    if (a->block < 1 || a->block > ivs::BT_MAX_BLOCK) return fail(IVS_ERANGE, "%s: block=%d outside [1,%d]", fn, a->block, ivs::BT_MAX_BLOCK);
    if (a->nC > ivs::BT_MAX_CI) return fail(IVS_ERANGE, "%s: nC=%d > %d interval probabilities", fn, a->nC, ivs::BT_MAX_CI);
    if (a->nC > 0 && !a->ci_probs) return fail(IVS_EINVAL, "%s: null interval probabilities", fn);
    for (int c = 0; c < a->nC; ++c)
        if (!(a->ci_probs[c] > 0.0 && a->ci_probs[c] < 1.0))
            return fail(IVS_ERANGE, "%s: interval probability %d (%g) is not inside (0, 1)", fn, c, a->ci_probs[c]);
    const int64_t nl1 = a->nL > 0 ? a->nL : 1, nc1 = a->nC > 0 ? a->nC : 1;
    if (a->B > 0x7fffffffLL / a->window || a->B > 0x7fffffffLL / ((int64_t)a->n_rep * 2 * nl1) || a->B > 0x7fffffffLL / (2 * nl1 * nc1))
        return fail(IVS_ERANGE, "%s: %lld rows x %d scenarios, x %d replicates or x %d quantiles at %d levels exceed one launch", fn,
                    (long long)a->B, a->window, a->n_rep, a->nC, a->nL);
    if (a->B == 0) return IVS_OK;                                                                  // C9
    if (!a->pnl || !a->scen_flags || !a->n_scen || (a->nL > 0 && (!a->var0 || !a->es0 || !a->mean || !a->variance || (a->nC > 0 && !a->quant))))
        return fail(IVS_EINVAL, "%s: null pointer", fn);
    const size_t need = (size_t)bootstrap_rep_elems(a->B, a->n_rep, a->nL) * sizeof(double);
    if (!a->rep && need > 0 && (!workspace || workspace_bytes < need))
        return fail(IVS_EINVAL, "%s: workspace of %zu bytes, %zu needed without rep", fn, workspace ? workspace_bytes : (size_t)0, need);
    ivs::BootParams p{};
    p.pnl = a->pnl; p.scen_flags = a->scen_flags; p.window = a->window; p.nL = a->nL; p.min_scen = a->min_scen;
    p.R = a->n_rep; p.L = a->block; p.nC = a->nC; p.seed = a->seed;
    for (int l = 0; l < a->nL; ++l) p.tp[l] = a->tail_probs[l];
    for (int c = 0; c < a->nC; ++c) p.ci[c] = a->ci_probs[c];
    p.var0 = a->var0; p.es0 = a->es0; p.n_scen = a->n_scen; p.mean = a->mean; p.variance = a->variance; p.quant = a->quant;
    p.rep = a->rep ? a->rep : static_cast<double*>(workspace);          // C9: the one way through global memory
    hipLaunchKernelGGL(ivs::hsim_bootstrap_kernel, dim3((unsigned)a->B), dim3(ivs::RK_BLOCK), 0, static_cast<hipStream_t>(stream), p);
    return end_call("hsim_bootstrap_kernel");
}

int ivs_hsim_weighted_f64(const ivs_hsim_weighted_args* a, void*, size_t, void* stream) {
    const char* fn = "ivs_hsim_weighted_f64";
    if (int rc = begin_call(fn, a)) return rc;
    if (a->B < 0 || a->nL < 0) return fail(IVS_EINVAL, "%s: negative size", fn);
    if (a->lag < 1) return fail(IVS_ERANGE, "%s: lag=%d < 1", fn, a->lag);
    if (a->window < 1 || a->window > ivs::HS_MAX_WINDOW)
        return fail(IVS_ERANGE, "%s: window=%d outside [1,%d]", fn, a->window, ivs::HS_MAX_WINDOW);
    if (a->nL > ivs::HS_MAX_LEVELS) return fail(IVS_ERANGE, "%s: nL=%d > %d tail probabilities", fn, a->nL, ivs::HS_MAX_LEVELS);
    if (a->nL > 0 && !a->tail_probs) return fail(IVS_EINVAL, "%s: null tail probabilities", fn);
    for (int l = 0; l < a->nL; ++l)
        if (!(a->tail_probs[l] > 0.0 && a->tail_probs[l] < 1.0))
            return fail(IVS_ERANGE, "%s: tail probability %d (%g) is not inside (0, 1)", fn, l, a->tail_probs[l]);
    if (a->min_scen < 1) return fail(IVS_ERANGE, "%s: min_scen=%d < 1", fn, a->min_scen);
    const int M = a->vol_span;
    if (M < 0 || M > ivs::HW_MAX_SPAN) return fail(IVS_ERANGE, "%s: vol_span=%d outside [0,%d]", fn, M, ivs::HW_MAX_SPAN);
    if (M > 0 && (a->min_returns < 1 || a->min_returns > M))
        return fail(IVS_ERANGE, "%s: min_returns=%d outside [1,%d]", fn, a->min_returns, M);
    if (M > 0 && !(a->scale_cap >= 1.0 && a->scale_cap < __builtin_inf()))
        return fail(IVS_ERANGE, "%s: scale_cap=%g is not finite and >= 1", fn, a->scale_cap);
    if (a->stages < 0 || a->stages > 2) return fail(IVS_ERANGE, "%s: stages=%d outside [0,2]", fn, a->stages);
    if (a->B > 0x7fffffffLL / a->window)
        return fail(IVS_ERANGE, "%s: %lld rows x %d scenarios exceed one launch", fn, (long long)a->B, a->window);
    if (a->B == 0) return IVS_OK;                                                                  // W9
    const bool ewma = M > 0 && a->stages != 2, tail = a->stages != 1;
    if ((M > 0 && !a->sigma) || (ewma && (!a->spot || !a->vol_weight)) ||
        (tail && (!a->pnl || !a->scen_flags || !a->flags_w || !a->n_valid_w || !a->worst_w || !a->wsum || !a->n_eff ||
                  (a->nL > 0 && (!a->var_w || !a->es_w)))))
        return fail(IVS_EINVAL, "%s: null pointer", fn);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (ewma) {
        ivs::SpotEwmaParams e{};
        e.spot = a->spot; e.vol_weight = a->vol_weight; e.B = a->B; e.M = M; e.min_returns = a->min_returns; e.sigma = a->sigma;
        const int64_t grid = (a->B + ivs::RK_BLOCK - 1) / ivs::RK_BLOCK;
        hipLaunchKernelGGL(ivs::spot_ewma_kernel, dim3((unsigned)grid), dim3(ivs::RK_BLOCK), 0, st, e);
        if (int rc = end_call("spot_ewma_kernel")) return rc;
    }
    if (tail) {
        ivs::WTailParams t{};
        t.pnl = a->pnl; t.scen_flags = a->scen_flags; t.weight = a->weight; t.sigma = M > 0 ? a->sigma : nullptr;
        t.window = a->window; t.nL = a->nL; t.min_scen = a->min_scen; t.lag = a->lag;
        t.cap = M > 0 ? a->scale_cap : 1.0; t.cap_lo = 1.0 / t.cap;     // W0: formed once, here
        for (int l = 0; l < a->nL; ++l) t.tp[l] = a->tail_probs[l];
        t.var_w = a->var_w; t.es_w = a->es_w; t.n_valid_w = a->n_valid_w; t.worst_w = a->worst_w; t.wsum = a->wsum; t.n_eff = a->n_eff;
        t.pnl_w = a->pnl_w; t.scale = a->scale; t.flags_w = a->flags_w;
        hipLaunchKernelGGL(ivs::hsim_wtail_kernel, dim3((unsigned)a->B), dim3(ivs::RK_BLOCK), 0, st, t);
        return end_call("hsim_wtail_kernel");
    }
    return IVS_OK;
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

}  // extern "C"
