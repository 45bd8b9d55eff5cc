// Black-Scholes Greeks of one option, for the kernels of more than one unit (greeks_kernel, the 1-D / frame Greeks
// columns, the snapshot analytics).  Device helper only.
#pragma once
#include "ivs_device.hpp"

namespace ivs {

// one option: the reference's formulas statement by statement (greeks.py:21-35)
__device__ __forceinline__ void bs_greeks_one(double S, double K, double T, double r, double sg, bool put, double& delta,
                                              double& gamma, double& theta, double& vega, double& rho) {
    const double sq = sqrt(T);
    const double d1 = (log(S / K) + (r + 0.5 * sg * sg) * T) / (sg * sq);
    const double d2 = d1 - sg * sq;
    const double pdf1 = norm_pdf(d1);
    const double cdf1 = norm_cdf(d1);
    const double cdf2 = norm_cdf(put ? -d2 : d2);
    const double disc = exp(-r * T);
    const double common = -S * pdf1 * sg / (2.0 * sq);
    delta = put ? cdf1 - 1.0 : cdf1;
    gamma = pdf1 / (S * sg * sq);
    theta = (put ? common + r * K * disc * cdf2 : common - r * K * disc * cdf2) / 365.0;
    vega = S * pdf1 * sq / 100.0;
    rho = K * T * disc * cdf2 / 100.0;
}

}  // namespace ivs
