// lin_common.hpp -- what the kernels of linear.hip (forming the linear-test randomness) and diagnose.hip (evaluating the constraints)
// share: the workgroup size, the heavy-segment threshold, the fixed LDS summation tree and the conversion of a coefficient table.
#pragma once
#include "fr.hpp"

namespace lig {
static constexpr uint32_t LIN_WG = 256;
static constexpr uint32_t HEAVY_MIN = 2048;       // a segment (the terms of one slot / of one constraint) with more terms than this is summed by whole workgroups
static constexpr uint32_t COEFS_MAX_BLOCKS = 1024;      // block cap of the grid-stride passes over a table or over constraints
static constexpr uint32_t LIN_NOT_LOCAL = 0xFFFFFFFFu;  // entry of a rank's global -> local row table: another rank holds that row

// sum of the workgroup's LIN_WG values (fixed tree: the same bytes on every run); valid in thread 0
static __device__ __forceinline__ fr lin_block_sum(fr v, fr* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t w = LIN_WG / 2; w; w >>= 1) {
        if (threadIdx.x < w) sh[threadIdx.x] = fr_add(sh[threadIdx.x], sh[threadIdx.x + w]);
        __syncthreads();
    }
    return sh[0];
}
// tab[0 .. n): canonical -> Montgomery form in place (k_lin_coefs_mont, linear.hip), enqueued on `st`; every entry must be < p
void launch_lin_coefs_mont(hipStream_t st, fr* tab, uint64_t n);
}  // namespace lig
