// Wave and workgroup prefix sums of one uint32 per thread: what the scan and radix kernels (radix_sort.hip) and the tile-list
// kernels (binning.hip) both build on.
#pragma once

#include "ogs_common.h"

namespace ogs {

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        uint32_t t = __shfl_up(v, d, kWave);
        if (lane_id() >= d) v += t;
    }
    return v;
}

// Exclusive scan of one value per thread across the 256-thread block; returns the block total.
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t& total, uint32_t* wave_sums /*[4]*/) {
    const int wave = threadIdx.x >> 6;
    const uint32_t inc = wave_inclusive_scan(v);
    if (lane_id() == kWave - 1) wave_sums[wave] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) {
        const uint32_t s = wave_sums[w];
        if (w < wave) base += s;
        tot += s;
    }
    total = tot;
    __syncthreads();
    return base + inc - v;
}

}  // namespace ogs
