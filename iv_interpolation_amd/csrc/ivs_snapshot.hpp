// Per-minute surface snapshots of one underlying from its interpolated option chain (rules S4-S7):
// sigma [B][nT][nK], T [B][nT], spot [B], quotes [B] and the per-snapshot strike query grid Kq [B][mK], in one launch.
//
// Lane = cell (expiry e, strike k), cell = e*nK + k.  A workgroup owns `tile` consecutive minutes and as many waves as the
// cells need (<= 16; wider chains loop over cell slots).  A lane walks the date-sorted rows of its <= 2 contracts (call,
// put) forward through the tile: the tile's first row comes from one probe at the "one row per minute" guess plus a
// binary search, after that every minute is a short forward scan that resolves last-row-wins, NaN = absent and the OTM
// choice in registers.  Consecutive lanes store consecutive cells, so every cell of a minute -- NaN ones included -- is
// written once by one coalesced pass; no fill pass, no atomics.  quotes / spot: a wave ballot per minute gives the count
// and the wave's lowest quoted cell; lane m of the wave keeps minute m's running values, and the waves meet in LDS once
// per tile.  Everything is plain loads, vector stores and integer/double arithmetic in a fixed order: bitwise
// deterministic.
#pragma once
#include "ivs_device.hpp"

namespace ivs {

constexpr int SN_MAX_WAVES = 16;                          // 1024 threads
constexpr int SN_MAX_TILE = 64;                           // minutes per workgroup (one lane of a wave per minute)
constexpr int64_t SN_MINUTE_NS = 60000000000LL;
constexpr double SN_YEAR_NS = 365.0 * 86400.0 * 1e9;     // YEAR = 365 days (rule S2), exact in fp64

struct SnapshotParams {
    const int64_t* date; const double* iv; const double* und;   // rows [n_rows], date-sorted inside a contract
    const int64_t* row_off;                                     // [C+1]
    const int32_t* cells;                                       // [nT*nK][2]: call / put contract or -1
    const double* strike;                                       // [nK]
    const int64_t* expiry;                                      // [nT] E_e (ns)
    const double* moneyness; int32_t mK; double kq_empty;       // Kq[b] = (spot[b] or kq_empty) * moneyness
    int64_t t0, B;
    int32_t nT, nK, tile, n_tiles, n_waves;
    double* sigma; double* T; double* spot; int32_t* quotes; double* Kq;
};

// first row in [lo, hi) whose date is >= t (rows date-sorted); probes the row a one-row-per-minute series would hold first
__device__ __forceinline__ int64_t sn_seek(const int64_t* date, int64_t lo, int64_t hi, int64_t t) {
    if (lo >= hi) return hi;
    const int64_t first = date[lo];
    if (first >= t) return lo;
    int64_t a = lo + 1, b = hi;                               // answer in [a, b]; date[a-1] < t
    if (a < b) {
        int64_t g = lo + (int64_t)__builtin_ceil((double)(t - first) * (1.0 / (double)SN_MINUTE_NS));
        g = g < a ? a : (g > b - 1 ? b - 1 : g);
        if (date[g] >= t) {
            b = g;
            if (g > a && date[g - 1] < t) a = g;
        } else {
            a = g + 1;
        }
    }
    while (a < b) {
        const int64_t mid = a + ((b - a) >> 1);
        if (date[mid] < t) a = mid + 1; else b = mid;
    }
    return a;
}

// XCD-aware bijective remap: consecutive tiles (which read the same cache lines of every contract) share an XCD's L2
__device__ __forceinline__ int sn_tile_of(int wg, int n) {
    if (n <= 8) return wg;
    const int q = n / 8, r = n % 8, x = wg % 8;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + wg / 8;
}

__global__ __launch_bounds__(1024) void snapshot_assemble_kernel(SnapshotParams p) {
    __shared__ int32_t s_cnt[SN_MAX_WAVES][SN_MAX_TILE];
    __shared__ int32_t s_first[SN_MAX_WAVES][SN_MAX_TILE];
    __shared__ double s_spot[SN_MAX_WAVES][SN_MAX_TILE];
    __shared__ double s_base[SN_MAX_TILE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nthr = p.n_waves * 64;
    const int64_t b0 = (int64_t)sn_tile_of(blockIdx.x, p.n_tiles) * p.tile;
    const int nb = (int)((p.B - b0) < p.tile ? (p.B - b0) : p.tile);       // minutes of this tile (>= 1)
    const int ncell = p.nT * p.nK;
    const int64_t tb0 = p.t0 + b0 * SN_MINUTE_NS;

    // lane m of every wave carries minute m's running count / lowest quoted cell / that cell's underlying price
    int32_t my_cnt = 0, my_first = 0x7fffffff;
    double my_spot = qnan();

    for (int base = 0; base < ncell; base += nthr) {                  // uniform over the block: ballots see every lane
        const int cell = base + tid;
        const bool live = cell < ncell;
        int64_t rc = 0, ec = 0, rp = 0, ep = 0;
        double K = 0.0;
        int64_t E = 0;
        if (live) {
            const int cc = p.cells[2 * cell], pc = p.cells[2 * cell + 1];
            K = p.strike[cell % p.nK];
            E = p.expiry[cell / p.nK];
            if (cc >= 0) { ec = p.row_off[cc + 1]; rc = sn_seek(p.date, p.row_off[cc], ec, tb0); }
            if (pc >= 0) { ep = p.row_off[pc + 1]; rp = sn_seek(p.date, p.row_off[pc], ep, tb0); }
        }
        int64_t tb = tb0;
        for (int m = 0; m < nb; ++m, tb += SN_MINUTE_NS) {
            const int64_t thr = tb + SN_MINUTE_NS;
            int64_t cand_c = -1, cand_p = -1;                          // last row of the minute (S5: last wins)
            while (rc < ec && p.date[rc] < thr) cand_c = rc++;
            while (rp < ep && p.date[rp] < thr) cand_p = rp++;
            double v = qnan(), u = qnan();
            if (live && E - tb > 0) {                                  // S6: a passed expiry leaves its row NaN
                const double vc = cand_c >= 0 ? p.iv[cand_c] : qnan();
                const double vp = cand_p >= 0 ? p.iv[cand_p] : qnan();
                const double fp = cand_p >= 0 ? p.und[cand_p] : qnan();
                const bool hc = !__builtin_isnan(vc), hp = !__builtin_isnan(vp);
                const bool put = hp && (!hc || K < fp);                // S5: OTM side, put iff strike < F
                if (put) { v = vp; u = fp; }
                else if (hc) { v = vc; u = p.und[cand_c]; }
            }
            if (live) p.sigma[(b0 + m) * (int64_t)ncell + cell] = v;
            const unsigned long long q = __ballot(!__builtin_isnan(v));
            const int lo = q ? __builtin_ctzll(q) : 0;
            const double u0 = __shfl(u, lo);
            if (lane == m) {
                my_cnt += __popcll(q);
                if (q && my_first == 0x7fffffff) { my_first = base + wave * 64 + lo; my_spot = u0; }
            }
        }
    }
    s_cnt[wave][lane] = my_cnt;
    s_first[wave][lane] = my_first;
    s_spot[wave][lane] = my_spot;
    __syncthreads();
    if (tid < nb) {
        int32_t cnt = 0, first = 0x7fffffff;
        double sp = qnan();
        for (int w = 0; w < p.n_waves; ++w) {
            cnt += s_cnt[w][tid];
            if (s_first[w][tid] < first) { first = s_first[w][tid]; sp = s_spot[w][tid]; }
        }
        if (cnt == 0) sp = qnan();
        p.quotes[b0 + tid] = cnt;
        p.spot[b0 + tid] = sp;
        s_base[tid] = __builtin_isnan(sp) ? p.kq_empty : sp;
    }
    for (int i = tid; i < nb * p.nT; i += nthr) {                      // S6: analytic maturities
        const int m = i / p.nT, e = i - m * p.nT;
        p.T[(b0 + m) * p.nT + e] = (double)(p.expiry[e] - (tb0 + m * SN_MINUTE_NS)) / SN_YEAR_NS;
    }
    if (p.Kq) {
        __syncthreads();
        for (int i = tid; i < nb * p.mK; i += nthr) {
            const int m = i / p.mK, j = i - m * p.mK;
            p.Kq[(b0 + m) * p.mK + j] = s_base[m] * p.moneyness[j];
        }
    }
}

}  // namespace ivs
