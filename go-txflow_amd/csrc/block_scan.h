// block_scan.h — exclusive scan of one 64-bit value per thread over a block of kWaves waves
// (the per-batch list builders: kernels_update.hip, kernels_store.hip)
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

// exclusive scan of x over the 64 * kWaves threads of a block; *total = block sum.  Every thread of
// the block calls it; it may be called again right after it returns.
template <int kWaves = 4>
__device__ __forceinline__ uint64_t block_excl_scan64(uint64_t x, uint64_t* total) {
  __shared__ uint64_t wsum[kWaves];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint64_t inc = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t y = (uint64_t)__shfl_up((long long)inc, d, 64);
    if (lane >= d) inc += y;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  uint64_t before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < kWaves; ++k) {
    if (k < w) before += wsum[k];
    all += wsum[k];
  }
  __syncthreads();
  *total = all;
  return before + inc - x;
}
