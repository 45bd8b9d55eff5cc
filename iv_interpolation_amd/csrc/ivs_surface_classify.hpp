// Ragged batches: the kernel that sorts the surfaces of a call into one work list per size class (VarList,
// ivs_surface_dense_var.hpp).  Not a template, so exactly one unit includes this header.
#pragma once
#include "ivs_surface_dense_var.hpp"

namespace ivs {

__global__ __launch_bounds__(256) void var_classify_kernel(SurfaceParams p, VarItem* l1, VarItem* l2, int32_t* counts) {
    // 1024 consecutive surfaces per block and step, 4 per thread; block-level exclusive scan of the per-thread class
    // counts, ONE global atomic per class, block and step (a per-wavefront atomic cost 0.36 ms per million surfaces)
    __shared__ int wsum[2][4];
    __shared__ int base_s[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t b0 = (int64_t)blockIdx.x * 1024; b0 < p.B; b0 += (int64_t)gridDim.x * 1024) {      // block-uniform trip count
        int64_t ko[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) { const int64_t b = b0 + 4 * tid + k; ko[k] = b <= p.B ? p.k_off[b] : 0; }
        int cls[4]; int c[2] = {0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t b = b0 + 4 * tid + k;
            const int64_t nn = ko[k + 1] - ko[k];
            cls[k] = b >= p.B ? -1 : ((nn >= 4 && nn <= 64) ? 0 : ((nn >= 65 && nn <= 128) ? 1 : 2));
            if (cls[k] >= 0 && (nn < 0 || nn > p.nK || ko[k] < 0 || (p.k_total > 0 && ko[k + 1] > p.k_total))) {
                // offsets no kernel can serve (the LDS carve is sized by nK) or that leave the caller's K / sigma arrays
                cls[k] = -1;
                if (p.status) p.status[b] = IVS_ST_BAD_SHAPE;
            }
            if (cls[k] == 2) {                                  // not served by a dense kernel: generic redo pass
                reinterpret_cast<unsigned long long*>(p.out + b * (int64_t)p.mT * p.mK)[0] = D_SENTINEL;
                count_redo(p);
            }
            if (cls[k] == 0) ++c[0];
            if (cls[k] == 1) ++c[1];
        }
        int pre[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            int incl = c[j];
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
            if (lane == 63) wsum[j][wave] = incl;
            pre[j] = incl - c[j];
        }
        __syncthreads();
        if (tid < 2) {
            const int tot = wsum[tid][0] + wsum[tid][1] + wsum[tid][2] + wsum[tid][3];
            base_s[tid] = tot ? atomicAdd(&counts[tid], tot) : 0;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            int w0 = 0;
            for (int w = 0; w < wave; ++w) w0 += wsum[j][w];
            pre[j] += base_s[j] + w0;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (cls[k] == 0) l1[pre[0]++] = VarItem{(int32_t)(b0 + 4 * tid + k), (int32_t)(ko[k + 1] - ko[k]), ko[k]};
            if (cls[k] == 1) l2[pre[1]++] = VarItem{(int32_t)(b0 + 4 * tid + k), (int32_t)(ko[k + 1] - ko[k]), ko[k]};
        }
        __syncthreads();                                         // wsum / base_s are reused by the next step
    }
}

}  // namespace ivs
