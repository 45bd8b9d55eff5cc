// SVI term structure (rules T1-T4, C1-C6, E1-E6): what the raw SVI slices of one snapshot say ACROSS
// tenors.  Two kernels on params [B][mT][5] (a, b, rho, m, sigma per row, the `params` of ivs_svi_slices_f64), the tenors and
// the spots:
//
// svi_calendar_kernel: per row j of a snapshot the pair (j, j') with j' the next live row (T4), the difference
// d(x) = w_j'(x) - w_j(x) of the two total-variance curves on a 64-point grid around the forward plus the two vertices m_j,
// m_j': its minimum and where, its value at the forward, how many grid cells it changes sign in, the first and the last of
// those crossings located by 52 bisection steps, and the comparison of the wing slopes, which says what happens beyond any
// grid.  A wavefront owns `group` <= 32 consecutive rows.  Scan phase, row after row: on entering a snapshot the live rows
// become one ballot with lane = tenor and the order of their tenors is checked by one lane permute; then lane = grid point,
// both slices read at wave-uniform addresses, a fixed xor butterfly over (d, index) for the minimum, one ballot of d < 0 for the
// crossings.  Lane g keeps the figures of row g, lane 2g + c the cell of crossing c.  Inversion phase, once: lane 2g + c
// bisects crossing c of row g; consecutive lanes store consecutive elements.  No LDS, no atomics, no scratch.
//
// svi_eval_kernel: per (snapshot, query) the surface at (strike, expiry): the two live slices that bracket the expiry,
// total variance linear in the tenor at fixed x = ln(K / F), from it vol, call, put, the forward variance, Durrleman's g and
// the local vol.  A block takes one snapshot and 256 queries, lane = query; the snapshot's mT x 6 doubles are staged in LDS
// once (a dead slice with a NaN tenor, so that no comparison ever picks it) and read at uniform addresses.
//
// Every value is a function of the row's / query's inputs alone: a result depends neither on `group` nor on the block that
// took the query.
#pragma once
#include "ivs_device.hpp"
#include "ivs_distribution.hpp"
#include "ivs_bs_formulas.hpp"

namespace ivs {

constexpr int SC_WAVES = 4;        // wavefronts per workgroup of the calendar kernel
constexpr int SC_MAX_GROUP = 32;   // rows per wavefront: two inversion lanes each
constexpr int SC_STEPS = 52;       // rule C4
constexpr int SE_BLOCK = 256;      // queries per block of the evaluation kernel

struct CalParams {
    const double* params; const double* Tq; const double* spot;
    int64_t tq_stride;                                   // 0 = shared
    int32_t mT, group;
    int64_t rows;                                        // B * mT
    double* d_min; double* x_min; double* d_atm;         // [rows]
    double* x_cross;                                     // [rows][2]
    int32_t* n_cross; int32_t* flags;                    // [rows]
};

struct EvalParams {
    const double* params; const double* Tq; const double* spot;
    const double* u; const double* tau;
    int64_t tq_stride, q_stride;                         // 0 = shared
    double rate;
    int32_t mT, strike_mode, nqb;                        // nqb = blocks per snapshot
    int64_t Q;
    double* w; double* vol; double* call; double* put; double* fwd_var; double* g; double* local_vol;   // [B][Q], each may be null
    int32_t* flags;                                      // [B][Q]
};

// rule T3: w at x
__device__ __forceinline__ double st_w(const DistRow& r, double x) {
    const double dx = x - r.m;
    return r.a + r.b * (r.rho * dx + sqrt(dx * dx + r.sig * r.sig));
}

// rule T3: w, w', w'' at x
__device__ __forceinline__ void st_w012(const DistRow& r, double x, double& w, double& w1, double& w2) {
    const double dx = x - r.m;
    const double s2 = r.sig * r.sig;
    const double rr = sqrt(dx * dx + s2);
    w = r.a + r.b * (r.rho * dx + rr);
    w1 = r.b * (r.rho + dx / rr);
    w2 = r.b * s2 / (rr * rr * rr);
}

// rule C2
__device__ __forceinline__ double sc_d(const DistRow& lo, const DistRow& hi, double x) { return st_w(hi, x) - st_w(lo, x); }

// rule C1: the grid in units of s0, exact in fp64
__device__ __forceinline__ double sc_y(int i) {
    const double t = (double)i - 31.5;
    return t * (1.0 + t * t / 1024.0) / 8.0;
}

__device__ __forceinline__ double sc_s0(const DistRow& lo, const DistRow& hi) {
    const double a = st_w(lo, 0.0), b = st_w(hi, 0.0);
    return sqrt(a > b ? a : b);
}

__device__ __forceinline__ DistRow st_row(const double* pr) { return DistRow{pr[0], pr[1], pr[2], pr[3], pr[4]}; }

// Where a (strike, expiry) sits between the slices of snapshot b.  svi_eval_kernel and the two kernels of ivs_risk.hpp place
// a query through these two functions, so they cannot disagree.
//
// rule T1 into LDS: a, b, rho, m, sigma, tau (NaN = dead, so that no comparison ever picks it) per tenor; the caller
// synchronises the block before it reads sl
__device__ __forceinline__ void st_stage(double* sl, const double* params, const double* Tq, int64_t tq_stride, int64_t b, int mT, double S) {
    if ((int)threadIdx.x < mT) {
        const int j = threadIdx.x;
        const DistRow r = st_row(params + (b * mT + j) * 5);
        const double tau = Tq[b * tq_stride + j];
        const bool lv = ds_live(r, S, tau);
        sl[j * 6 + 0] = r.a; sl[j * 6 + 1] = r.b; sl[j * 6 + 2] = r.rho; sl[j * 6 + 3] = r.m; sl[j * 6 + 4] = r.sig;
        sl[j * 6 + 5] = lv ? tau : qnan();
    }
}

// rules T2 and E2 on the staged slices: lo = the last live slice with tenor <= tq, hi = the first with tenor > tq (-1 = none);
// unordered = the live tenors do not strictly increase; any = there is a live slice.  A fixed loop at uniform LDS addresses,
// comparisons only: no floating-point setting can change what it yields.  The loop runs on locals and the four results are
// handed over once, after it: written through the references inside the loop, the same code made svi_eval_kernel about 1 %
// slower on MI355X (profiles/analytics_refactor/bench.txt).
__device__ __forceinline__ void st_bracket(const double* sl, int mT, double tq, int& lo_, int& hi_, bool& unordered_, bool& any_) {
    int lo = -1, hi = -1;
    bool unordered = false;
    double prev = -__builtin_inf();
    for (int j = 0; j < mT; ++j) {
        const double t = sl[j * 6 + 5];
        if (t == t) {
            unordered = unordered || !(t > prev);
            prev = t;
        }
        if (t <= tq) lo = j;
        if (t > tq && hi < 0) hi = j;
    }
    lo_ = lo; hi_ = hi; unordered_ = unordered; any_ = prev > 0.0;
}

__global__ __launch_bounds__(SC_WAVES * 64) void svi_calendar_kernel(CalParams p) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t row0 = ((int64_t)blockIdx.x * SC_WAVES + wave) * p.group;
    if (row0 >= p.rows) return;                                          // the whole wavefront
    const int ng = (int)((p.rows - row0) < p.group ? (p.rows - row0) : p.group);
    const double y = sc_y(lane);

    // lane g: the figures of row g; lane 2g + c: crossing c of row g
    double r_dmin = qnan(), r_xmin = qnan(), r_datm = qnan();
    int32_t r_cnt = 0, r_flags = 0;
    int c_cell = -1, c_jp = 0;
    bool c_neg = false;
    double c_s0 = 0.0;

    int64_t cur_b = -1;
    unsigned long long live = 0ull;
    bool unordered = false;
    for (int g = 0; g < ng; ++g) {
        const int64_t row = row0 + g;
        const int64_t b = row / p.mT;
        const int j = (int)(row - b * p.mT);
        if (b != cur_b) {                                                // T1, T2, T4: lane = tenor
            cur_b = b;
            bool lv = false;
            double tau = 0.0;
            if (lane < p.mT) {
                tau = p.Tq[b * p.tq_stride + lane];
                lv = ds_live(st_row(p.params + (b * p.mT + lane) * 5), p.spot[b], tau);
            }
            live = __ballot(lv);
            const unsigned long long above = live & ~((2ull << lane) - 1ull);
            const double tnext = __shfl(tau, above ? __builtin_ctzll(above) : lane);
            unordered = __ballot(lv && above != 0ull && !(tnext > tau)) != 0ull;
        }
        const unsigned long long above_j = live & ~((2ull << j) - 1ull);
        const bool is_live = (live >> j) & 1ull;
        int32_t fl = 0, cnt = 0;
        double dmin = qnan(), xmin = qnan(), datm = qnan();
        int first = -1, last = -1;
        unsigned long long nm = 0ull;
        double s0 = 0.0;
        int jp = j;
        if (unordered) fl = IVS_SC_UNORDERED;
        else if (!is_live) fl = IVS_SC_DEAD;
        else if (!above_j) fl = IVS_SC_LAST;
        else {                                                           // all of this is uniform over the wavefront
            jp = __builtin_ctzll(above_j);
            const DistRow lo = st_row(p.params + row * 5), hi = st_row(p.params + (b * p.mT + jp) * 5);
            s0 = sc_s0(lo, hi);                                          // C1
            const double x = s0 * y;
            const double d = sc_d(lo, hi, x);                            // C2: the grid, then the two vertices in lanes 0 and 1
            const double xe = lane == 0 ? lo.m : hi.m;
            const double de = sc_d(lo, hi, xe);
            datm = sc_d(lo, hi, 0.0);
            double best = d == d ? d : __builtin_inf();
            int who = lane;
            if (lane < 2 && de < best) { best = de; who = 64 + lane; }
            for (int s = 32; s > 0; s >>= 1) {
                const double ob = __shfl_xor(best, s);
                const int ow = __shfl_xor(who, s);
                const bool take = ob < best || (ob == best && ow < who);
                best = take ? ob : best;
                who = take ? ow : who;
            }
            who = __builtin_amdgcn_readfirstlane(who);
            dmin = who < 64 ? __shfl(d, who) : __shfl(de, who - 64);
            xmin = who < 64 ? __shfl(x, who) : __shfl(xe, who - 64);
            nm = __ballot(d < 0.0);                                      // C3
            const unsigned long long cells = (nm ^ (nm >> 1)) & 0x7fffffffffffffffull;
            cnt = __popcll(cells);
            if (cells) { first = __builtin_ctzll(cells); last = 63 - __builtin_clzll(cells); }
            if (dmin < 0.0) fl |= IVS_SC_CALENDAR;                       // C6
            if (hi.b * (1.0 - hi.rho) < lo.b * (1.0 - lo.rho)) fl |= IVS_SC_WING_LEFT;     // C5
            if (hi.b * (1.0 + hi.rho) < lo.b * (1.0 + lo.rho)) fl |= IVS_SC_WING_RIGHT;
        }
        if (lane == g) { r_dmin = dmin; r_xmin = xmin; r_datm = datm; r_cnt = cnt; r_flags = fl; }
        if ((lane >> 1) == g) {
            c_cell = (lane & 1) ? last : first;
            c_neg = c_cell >= 0 && ((nm >> c_cell) & 1ull);
            c_s0 = s0;
            c_jp = jp;
        }
    }

    if (lane < ng) {                                                     // every element, consecutive lanes
        const int64_t o = row0 + lane;
        p.d_min[o] = r_dmin; p.x_min[o] = r_xmin; p.d_atm[o] = r_datm;
        p.n_cross[o] = r_cnt; p.flags[o] = r_flags;
    }
    if (lane >= 2 * ng) return;
    double xc = qnan();
    if (c_cell >= 0) {                                                   // C4
        const int64_t row = row0 + (lane >> 1);
        const int64_t b = row / p.mT;
        const DistRow lo_r = st_row(p.params + row * 5), hi_r = st_row(p.params + (b * p.mT + c_jp) * 5);
        double lo = c_s0 * sc_y(c_cell), hi = c_s0 * sc_y(c_cell + 1);
        for (int it = 0; it < SC_STEPS; ++it) {
            const double mid = 0.5 * (lo + hi);
            if ((sc_d(lo_r, hi_r, mid) < 0.0) == c_neg) lo = mid; else hi = mid;
        }
        xc = 0.5 * (lo + hi);
    }
    p.x_cross[row0 * 2 + lane] = xc;
}

__global__ __launch_bounds__(SE_BLOCK) void svi_eval_kernel(EvalParams p) {
    __shared__ double sl[ST_MAX_T * 6];                                  // a, b, rho, m, sigma, tau (NaN = dead) per tenor
    const int64_t b = blockIdx.x / p.nqb;
    const int qb = (int)(blockIdx.x - b * p.nqb);
    const double S = p.spot[b];
    st_stage(sl, p.params, p.Tq, p.tq_stride, b, p.mT, S);               // T1
    __syncthreads();
    const int64_t q = (int64_t)qb * SE_BLOCK + threadIdx.x;
    if (q >= p.Q) return;
    const double u = p.u[b * p.q_stride + q], tq = p.tau[b * p.q_stride + q];

    int lo, hi;
    bool unordered, any;
    st_bracket(sl, p.mT, tq, lo, hi, unordered, any);                    // T2 and E2
    const bool ok = finite_pos(u) && finite_pos(tq) && finite_pos(S) && any;  // E1

    int32_t fl = 0;
    double W = qnan(), vol = qnan(), call = qnan(), put = qnan(), V = qnan(), g = qnan(), lv = qnan();
    if (unordered) fl = IVS_SE_UNORDERED;
    else if (!ok) fl = IVS_SE_DEAD;
    else {
        const double K = p.strike_mode == 0 ? S * u : u;
        const double rt = p.rate * tq;
        const double F = S * exp(rt), D = exp(-rt);
        const double x = log(K / S) - rt;
        double W1, W2;
        if (lo >= 0 && hi >= 0) {                                        // E3
            const double* a = sl + lo * 6;
            const double* c = sl + hi * 6;
            double wl, wl1, wl2, wh, wh1, wh2;
            st_w012(DistRow{a[0], a[1], a[2], a[3], a[4]}, x, wl, wl1, wl2);
            st_w012(DistRow{c[0], c[1], c[2], c[3], c[4]}, x, wh, wh1, wh2);
            const double dt = c[5] - a[5];
            const double lam = (tq - a[5]) / dt;
            W = wl + (wh - wl) * lam;
            W1 = wl1 + (wh1 - wl1) * lam;
            W2 = wl2 + (wh2 - wl2) * lam;
            V = (wh - wl) / dt;
        } else {
            const double* a = sl + (lo >= 0 ? lo : hi) * 6;
            fl |= lo >= 0 ? IVS_SE_LONG : IVS_SE_SHORT;
            double w0, w1, w2;
            st_w012(DistRow{a[0], a[1], a[2], a[3], a[4]}, x, w0, w1, w2);
            const double sc = tq / a[5];
            W = w0 * sc; W1 = w1 * sc; W2 = w2 * sc;
            V = w0 / a[5];
        }
        const double th = sqrt(W);                                       // E4
        const double d1 = -x / th + 0.5 * th, d2 = d1 - th;
        vol = sqrt(W / tq);
        if (p.call) call = D * (F * norm_cdf(d1) - K * norm_cdf(d2));
        if (p.put) put = D * (K * norm_cdf(-d2) - F * norm_cdf(-d1));
        const double h = 1.0 - x * W1 / (2.0 * W);                       // E5
        g = h * h - (W1 * W1 / 4.0) * (1.0 / W + 0.25) + W2 / 2.0;
        if (V < 0.0) fl |= IVS_SE_NEG_FWD;
        if (g <= 0.0) fl |= IVS_SE_NEG_G;
        if (!(V < 0.0) && !(g <= 0.0)) lv = sqrt(V / g);
    }
    const int64_t o = b * p.Q + q;                                       // E6: consecutive lanes, consecutive elements
    if (p.w) p.w[o] = W;
    if (p.vol) p.vol[o] = vol;
    if (p.call) p.call[o] = call;
    if (p.put) p.put[o] = put;
    if (p.fwd_var) p.fwd_var[o] = V;
    if (p.g) p.g[o] = g;
    if (p.local_vol) p.local_vol[o] = lv;
    p.flags[o] = fl;
}

}  // namespace ivs
