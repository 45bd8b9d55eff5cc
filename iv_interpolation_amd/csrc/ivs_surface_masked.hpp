// Surfaces with MISSING quotes (NaN in sigma), 64 strikes x 16 maturities, methods without per-knot slopes (linear,
// slinear, nearest, zero, from_derivatives): the fast second pass.
//
// A missing quote changes the KNOT SET of its row.  The correctness-first generic kernel (18 M surfaces/s) runs one binary
// search per row and query over lane-private columns in 51 KB of LDS; this kernel removes what makes that slow:
//   * rows are compacted by wave ballot; besides the compacted quotes each row keeps an IDX table (strike number of its
//     j-th valid knot, one byte) and a RANK table (valid knots at or below strike k, one byte), so that the interval of a
//     query in ANY row is one LDS byte away from its interval in the full strike grid -- no per-row binary searches, and
//     no per-knot table next to the quotes (the RANK byte gives the interval, the IDX byte the strike);
//   * strike-pass values stay in registers; a column whose values are all there takes the dense register pass with the
//     batch-wide tables from the scalar cache, the few columns with a missing value (a row that lost its outermost
//     quotes does not reach the outermost output strikes) are evaluated in place by the generic per-column code.
//     Surfaces with a row of fewer than 2 quotes, a column with too few values or more than 8 masked columns keep
//     their "redo" tag and fall through to the generic kernel (third launch, cheap when nothing is left).
// LDS: one plane [16][66] + the strikes + two byte tables = 11 KB; 12 wavefronts per CU.
// The methods with slopes or coefficients (cubic, cubicspline, quadratic, pchip, akima) ride on the same compaction in
// ivs_surface_masked_pass.hpp, which borrows MK_RS, MK_MAXCOL, MaskedX and MaskedT from here.
// Scope: uniform 64 x 16 batches, T / Tq shared, mK <= 64; runs in FILTER mode behind the dense / row-pass kernel (only
// surfaces tagged with the sentinel).  Device code only; launched, like the kernel of ivs_surface_masked_pass.hpp, from
// ivs_surface_tail_launch.hpp.
#pragma once
#include "ivs_surface_dense.hpp"

namespace ivs {

constexpr int MK_RS = 66;                          // row stride (doubles) of the compacted planes
__host__ __device__ constexpr size_t masked_lds_bytes() { return (size_t)(DT * MK_RS + DK) * 8 + 2 * DT * DK + DT * 4; }

struct MaskedT { const double* T; const uint8_t* idx; __device__ __forceinline__ double operator()(int i) const { return T[idx[i]]; } };
constexpr int MK_MAXCOL = 8;                      // masked output columns handled in place per surface (more: generic kernel)
// strikes of a compacted row
struct MaskedX { const double* Ksh; const uint8_t* idx; __device__ __forceinline__ double operator()(int i) const { return Ksh[idx[i]]; } };

template <int METHOD>
__global__ __launch_bounds__(64, 3) void surface_masked_kernel(SurfaceParams p) {
    constexpr bool STEP = d_is_step(METHOD);                      // nearest / zero / from_derivatives
    static_assert(METHOD == IVS_LINEAR || METHOD == IVS_SLINEAR || METHOD == IVS_NEAREST || METHOD == IVS_ZERO || METHOD == IVS_FROM_DERIVATIVES,
                  "linear, slinear, nearest, zero, from_derivatives (the other dense methods: surface_masked_pass_kernel)");
    constexpr int MINROW = 2;                                     // fewer quotes in a row: the generic kernel's business
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const int mT = p.mT, mK = p.mK;
    double* YC = reinterpret_cast<double*>(smem);
    double* Ksh = YC + DT * MK_RS;
    uint8_t* IDX = reinterpret_cast<uint8_t*>(Ksh + DK);
    uint8_t* RANK = IDX + DT * DK;
    int* NROW = reinterpret_cast<int*>(RANK + DT * DK);
    const double nanv = __builtin_nan("");
    auto nostamp = [](int) {};

    TqTables tt;
    const double* TTp = nullptr;
    const double* Wp = nullptr;
    tq_from_shared(p.tqs, tt, TTp, Wp);

    const bool kq_shared = p.kq_stride == 0;
    const bool act = lane < mK;
    double xq = (kq_shared && act) ? p.Kq[lane] : nanv;
    const unsigned long long lt_mask = (1ull << lane) - 1ull, le_mask = lt_mask | (1ull << lane);

    const bool all = p.mode && *p.mode != 0;               // "missing quotes first": nothing was tagged, every surface is ours
    if (!all && p.redo && *p.redo == 0) return;            // nothing was tagged (wave-uniform)
    bool told = false;
    double* tag_at = nullptr;                              // the current surface's first output cell
    auto leave = [&]() {                                   // the surface keeps (or, in `all` mode, gets) its tag: generic kernel
        if (lane == 0) {
            if (all) reinterpret_cast<unsigned long long*>(tag_at)[0] = REDO_SENTINEL;
            if (p.redo && !told) { *reinterpret_cast<volatile int*>(p.redo + 1) = 1; told = true; }
        }
    };
    const int64_t n_outer = (p.B + 63) / 64;
    // blocks of 64 tags are claimed from a work queue (head 16 of the workspace; WorkQueue, ivs_surface_generic.hpp): the
    // tagged surfaces are spread unevenly over the blocks, and so is the speed of the workgroups
    WorkQueue wq;
    wq.init(p.queue + 16 * QUEUE_STRIDE, 1, n_outer, 1, lane);
    for (int64_t ob = p.queue ? wq.take() : (int64_t)blockIdx.x; ob >= 0 && ob < n_outer; ob = p.queue ? wq.take() : ob + gridDim.x) {
      const int64_t bi = ob * 64 + lane;
      const bool tagged = bi < p.B &&
          (all || reinterpret_cast<const unsigned long long*>(p.out + bi * (int64_t)mT * mK)[0] == REDO_SENTINEL);
      unsigned long long todo = __ballot(tagged);
      // quotes and strikes of the NEXT tagged surface of the block are requested while the current one is processed
      double vn[DT], kn = 0.0;
      auto request = [&](int64_t bb) {
          const double* sb = p.sigma + bb * (int64_t)(DT * DK);
#pragma unroll
          for (int t = 0; t < DT; ++t) vn[t] = sb[t * DK + lane];
          kn = p.K[bb * p.k_stride + lane];
      };
      if (todo) request(ob * 64 + __builtin_ctzll(todo));
      while (todo) {
        const int bit = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int64_t b = ob * 64 + bit;
        double* outb = p.out + b * (int64_t)mT * mK;
        tag_at = outb;
        double v[DT];
#pragma unroll
        for (int t = 0; t < DT; ++t) v[t] = vn[t];
        const double kx = kn;
        if (!kq_shared) xq = act ? p.Kq[b * p.kq_stride + lane] : nanv;
        if (todo) request(ob * 64 + __builtin_ctzll(todo));
        __syncthreads();                                   // the previous surface's readers are done with LDS
        Ksh[lane] = kx;
        // ---- compact every row by ballot; RANK[t][k] = valid knots of row t at or below strike k
        bool give_up = tt.unsorted != 0;
#pragma unroll
        for (int t = 0; t < DT; ++t) {
            const bool valid = !__builtin_isnan(v[t]);         // NaN = missing quote
            const unsigned long long m = __ballot(valid);
            give_up = give_up || __ballot(__builtin_isinf(v[t])) != 0ull;      // an infinity is a VALUE (it propagates): generic kernel
            const int rank = __popcll(m & lt_mask);
            if (valid) { YC[t * MK_RS + rank] = v[t]; IDX[t * DK + rank] = (uint8_t)lane; }      // compacted quotes and their strike numbers
            RANK[t * DK + lane] = (uint8_t)__popcll(m & le_mask);
            const int nt = __popcll(m);
            if (lane == 0) NROW[t] = nt;
            give_up = give_up || nt < MINROW;                  // too few knots (or an empty row): the generic kernel's business
        }
        if (give_up) { leave(); continue; }                    // wave-uniform; the sentinel stays, the generic pass redoes it
        __syncthreads();
        __syncthreads();      // redundant (the slope phases that stood between the two barriers are gone): kept because without
                              // it the zero / from_derivatives instantiations come out with another register assignment
        // ---- strike evaluation (q-lane): interval in the full grid once, per row one RANK byte away
        int jf = -1;
        if (Ksh[0] <= xq) {
            jf = 0;
#pragma unroll
            for (int m = 1; m < 8; ++m) jf += (Ksh[8 * m] <= xq) ? 8 : 0;
#pragma unroll
            for (int st = 4; st >= 1; st >>= 1) if (Ksh[jf + st] <= xq) jf += st;
        }
        double z[DT];
        bool all_ok = true;
#pragma unroll
        for (int t = 0; t < DT; ++t) {
            const int n = NROW[t];
            const int j = jf >= 0 ? (int)RANK[t * DK + jf] - 1 : -1;
            const MaskedX X{Ksh, IDX + t * DK};
            const CView Y{YC + t * MK_RS, 1};
            if (METHOD == IVS_NEAREST) {
                // the row's interval j is known (RANK): one midpoint compare (ties to the left knot, as searchsorted side='left'
                // over the midpoints decides for strictly increasing strikes) instead of eval_nearest's binary search over the
                // midpoints -- 6 steps of two two-level LDS gathers per row (10 % of the quotes missing: 148 -> 242 M surfaces/s)
                double r = nanv;
                if (j >= 0 && xq <= X(n - 1)) {
                    const int jj = j > n - 2 ? n - 2 : j;
                    r = j > n - 2 ? Y(n - 1) : step_eval<IVS_NEAREST>(xq, X(jj), X(jj + 1), Y(jj), Y(jj + 1));
                }
                z[t] = r;
            } else if (STEP) z[t] = eval_method(METHOD, X, Y, Y, n, j, xq);      // (no slopes: the second view is never read)
            else z[t] = eval_linear(X, Y, n, j, xq, METHOD == IVS_LINEAR);      // (np.interp's division through div_shared_rcp: measured -5 % here -- the per-row range checks cost more than the 16 divisions)
            all_ok = all_ok && !__builtin_isnan(z[t]);
        }
        // ---- maturity direction.  A column whose strike-pass values are all there takes the dense register pass with the
        // batch-wide tables; a column with a missing value (a row whose outermost quotes are gone does not reach the
        // outermost output strikes) has its own maturity knot set: up to MK_MAXCOL of them are evaluated in place by the
        // generic kernel's per-column code, in slots carved out of the (now dead) quote plane.
        const bool col_masked = act && !all_ok;
        const unsigned long long mm = __ballot(col_masked);
        if (mm != 0ull) {
            if (__popcll(mm) > MK_MAXCOL) { leave(); continue; }      // the generic kernel redoes the surface
            __syncthreads();                                   // every lane is done with the planes
            double* Tsh = Ksh;                                 // 16 maturities
            double* cz = YC;
            uint8_t* cti = IDX;
            if (lane < DT) Tsh[lane] = p.T[lane];
            const int slot = __popcll(mm & lt_mask);
            int cn = 0;
            if (col_masked) {
#pragma unroll
                for (int t = 0; t < DT; ++t)
                    if (!__builtin_isnan(z[t])) { cz[slot * DT + cn] = z[t]; cti[slot * DT + cn] = (uint8_t)t; ++cn; }
            }
            if (__ballot(col_masked && cn > 0 && cn < method_min_knots(METHOD)) != 0ull) { leave(); continue; }    // too-few-knots status: generic kernel
            __syncthreads();
            if (col_masked) {
                const MaskedT cx{Tsh, cti + slot * DT};
                const CView cy{cz + slot * DT, 1};
                int jc = -1;
                for (int tq = 0; tq < mT; ++tq) {
                    const double x = p.Tq[tq];
                    double r = nanv;
                    if (cn > 0) {
                        while (jc + 1 < cn && cx(jc + 1) <= x) ++jc;          // Tq ascending (checked: tt.unsorted)
                        r = eval_method(METHOD, cx, cy, cy, cn, jc, x);
                    }
                    outb[(int64_t)tq * mK + lane] = r;
                }
            }
        }
        if (act && all_ok) dense_maturity_pass<METHOD, true, false, false, true>(z, tt, TTp, Wp, outb, 0, lane, true, mT, mK, nostamp);
        if (p.status && lane == 0) p.status[b] = IVS_ST_OK;
      }
    }
}

}  // namespace ivs
