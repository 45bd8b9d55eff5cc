// Black-Scholes Greeks epilogue: elementwise on (S, K, T, r, sigma) -> delta, gamma,
// theta, vega, rho.  Formulas and their quirks follow the reference src/interpolation/greeks.py:21-35 (put rho
// has no sign flip there).  Grid-stride, one element per lane per step, SoA arrays -> fully coalesced
// 8-byte accesses; 80 B per element move through HBM, ~150 fp64 instructions of math per element.
#pragma once
#include "ivs_bs_formulas.hpp"

namespace ivs {

struct GreeksParams {
    const double* S; const double* K; const double* T; const double* r; const double* sigma;
    const uint8_t* is_put; int default_put; int64_t n;
    double* delta; double* gamma; double* theta; double* vega; double* rho;
};

__global__ __launch_bounds__(256) void greeks_kernel(GreeksParams p) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < p.n; i += (int64_t)gridDim.x * 256) {
        const bool put = p.is_put ? p.is_put[i] != 0 : p.default_put != 0;
        double de, ga, th, ve, rh;
        bs_greeks_one(p.S[i], p.K[i], p.T[i], p.r[i], p.sigma[i], put, de, ga, th, ve, rh);
        p.delta[i] = de; p.gamma[i] = ga; p.theta[i] = th; p.vega[i] = ve; p.rho[i] = rh;
    }
}

}  // namespace ivs
