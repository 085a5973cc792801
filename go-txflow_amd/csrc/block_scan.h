// block_scan.h — the reductions and scans over a wave, and the exclusive scan of one 64-bit value
// per thread over a block of kWaves waves (the per-batch list builders: arrival_list.h and the
// emit kernel of kernels_store.hip; the route and load kernels: kernels_route.hip, kernels_load.hip)
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
  for (int d = 32; d; d >>= 1) x += (uint32_t)__shfl_xor((int)x, d, 64);
  return x;
}
__device__ __forceinline__ uint64_t wave_sum(uint64_t x) {
#pragma unroll
  for (int d = 32; d; d >>= 1) x += (uint64_t)__shfl_xor((long long)x, d, 64);
  return x;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t x) {
#pragma unroll
  for (int d = 32; d; d >>= 1) x = max(x, (uint32_t)__shfl_xor((int)x, d, 64));
  return x;
}
// exclusive scan over the wave; *total (when asked for) = the wave's sum
__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t x, uint32_t* total = nullptr) {
  const uint32_t lane = threadIdx.x & 63;
  uint32_t inc = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)inc, d, 64);
    if (lane >= (uint32_t)d) inc += y;
  }
  if (total) *total = (uint32_t)__shfl((int)inc, 63, 64);
  return inc - x;
}

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
