// Black-Scholes pricer and its inverse, price -> implied volatility (rules V1-V8): elementwise on
// (S, K, T, r, sigma) -> price [, vega] and on (price, S, K, T, r) -> vol, flags.  Lane = option, grid-stride, SoA arrays
// -> coalesced 8-byte accesses, no atomics, no LDS.  The inversion runs the SAME number of steps in every lane (two border
// tests and IV_STEPS halvings of log2 of the total vol, 2 erfc + 1 exp2 + 1 division each), so a wavefront never diverges on
// the search and a value depends on nothing but its own option: not on n, its index or the launch geometry.
#pragma once
#include "ivs_device.hpp"

namespace ivs {

constexpr int IV_STEPS = 64;                    // rule V7: halvings of t = log2 s
constexpr double IV_T_LO = -40.0, IV_T_HI = 6.0;   // ... on [2^-40, 2^6]

struct BsPriceParams {
    const double* S; const double* K; const double* T; const double* r; const double* sigma;
    const uint8_t* is_put; int default_put; int64_t n;
    double* price; double* vega; int32_t* flags;      // vega, flags may be null
};

struct ImpliedParams {
    const double* price; const double* S; const double* K; const double* T; const double* r;
    const uint8_t* is_put; int default_put; int price_mode; int64_t n;
    double* vol; int32_t* flags;
};

// rule V6: the normalised out-of-the-money price at |log-moneyness| h and total vol s; em = exp(-h/2), ep = exp(h/2)
__device__ __forceinline__ double iv_b(double h, double em, double ep, double s) {
    const double q = h / s, hs = 0.5 * s;
    return em * norm_cdf(-q + hs) - ep * norm_cdf(-q - hs);
}

// rules V1, V8
__device__ __forceinline__ void bs_price_one(double S, double K, double T, double r, double sg, bool put, double& price,
                                             double& vega, int32_t& flags) {
    const bool live = is_finite(S) && is_finite(K) && is_finite(T) && is_finite(r) && is_finite(sg) && S > 0.0 && K > 0.0 &&
                      T > 0.0 && sg > 0.0;
    const double sq = sqrt(T);
    const double KD = K * exp(-r * T);
    const double x = log(S / K) + r * T;
    const double s = sg * sq;
    const double d1 = x / s + 0.5 * s, d2 = d1 - s;
    const double v = put ? KD * norm_cdf(-d2) - S * norm_cdf(-d1) : S * norm_cdf(d1) - KD * norm_cdf(d2);
    price = live ? v : qnan();
    vega = live ? S * norm_pdf(d1) * sq : qnan();
    flags = live ? 0 : IVS_IV_DEAD;
}

// rules V1-V7
__device__ __forceinline__ void bs_implied_one(double price, double S, double K, double T, double r, bool put, int price_mode,
                                               double& vol, int32_t& flags) {
    const bool live = is_finite(price) && is_finite(S) && is_finite(K) && is_finite(T) && is_finite(r) && S > 0.0 && K > 0.0 &&
                      T > 0.0 && price >= 0.0;
    const double P = price_mode ? price * S : price;                       // V2
    const double KD = K * exp(-r * T);                                     // V3
    const double x = log(S / K) + r * T, h = __builtin_fabs(x);
    const bool itm = put ? x < 0.0 : x > 0.0;
    const double gap = put ? KD - S : S - KD;
    const double intrinsic = gap > 0.0 ? gap : 0.0, upper = put ? KD : S;
    const double tv = itm ? P - intrinsic : P;                             // V5
    const double beta = tv / sqrt(S * KD);
    const double em = exp(-0.5 * h), ep = exp(0.5 * h);
    // V7: the borders, then IV_STEPS halvings in every lane (a comparison with a NaN is false)
    const bool at_lo = iv_b(h, em, ep, exp2(IV_T_LO)) >= beta, at_hi = iv_b(h, em, ep, exp2(IV_T_HI)) < beta;
    double lo = IV_T_LO, hi = IV_T_HI;
#pragma unroll 1
    for (int i = 0; i < IV_STEPS; ++i) {
        const double mid = 0.5 * (lo + hi);
        const bool below = iv_b(h, em, ep, exp2(mid)) < beta;
        lo = below ? mid : lo;
        hi = below ? hi : mid;
    }
    const double t = at_lo ? IV_T_LO : (at_hi ? IV_T_HI : 0.5 * (lo + hi));
    double v = exp2(t) / sqrt(T);
    int32_t f = (itm ? IVS_IV_ITM : 0) | ((at_lo || at_hi) ? IVS_IV_EDGE : 0);
    if (P >= upper) { v = qnan(); f = (itm ? IVS_IV_ITM : 0) | IVS_IV_ABOVE; }            // V4, in price space
    else if (P < intrinsic) { v = qnan(); f = (itm ? IVS_IV_ITM : 0) | IVS_IV_BELOW; }
    else if (P == intrinsic) { v = 0.0; f = (itm ? IVS_IV_ITM : 0) | IVS_IV_BELOW; }
    vol = live ? v : qnan();
    flags = live ? f : IVS_IV_DEAD;
}

__global__ __launch_bounds__(256) void bs_price_kernel(BsPriceParams p) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < p.n; i += (int64_t)gridDim.x * 256) {
        const bool put = p.is_put ? p.is_put[i] != 0 : p.default_put != 0;
        double pr, ve; int32_t fl;
        bs_price_one(p.S[i], p.K[i], p.T[i], p.r[i], p.sigma[i], put, pr, ve, fl);
        p.price[i] = pr;
        if (p.vega) p.vega[i] = ve;
        if (p.flags) p.flags[i] = fl;
    }
}

__global__ __launch_bounds__(256) void bs_implied_vol_kernel(ImpliedParams p) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < p.n; i += (int64_t)gridDim.x * 256) {
        const bool put = p.is_put ? p.is_put[i] != 0 : p.default_put != 0;
        double v; int32_t fl;
        bs_implied_one(p.price[i], p.S[i], p.K[i], p.T[i], p.r[i], put, p.price_mode, v, fl);
        p.vol[i] = v;
        p.flags[i] = fl;
    }
}

}  // namespace ivs
