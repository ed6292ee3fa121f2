// Cross-lane and workgroup building blocks shared by the kernels: reductions and scans over the 64 lanes of a wave, and
// the two workgroup reductions of the volume entries (integer counters, a fixed fp64 tree).  One copy: every kernel that
// uses one of these compiles to what it did with its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---------------------------------------------------------------------------------------------
// wave helpers (wave = 64 lanes): every lane ends with the result
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
    v = max(v, ((unsigned long long)hi << 32) | lo);
  }
  return v;
}
// inclusive prefix sum over the wave: lane l ends with v of the lanes 0..l
__device__ __forceinline__ uint32_t wave_scan_incl_u32(uint32_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(v, o, 64);
    if (lane >= o) v += up;
  }
  return v;
}
// brk: the ballot of the lanes at which a stretch of equal lanes starts (or that belong to none).  The distance from
// `lane` to the end of its stretch -- for a head lane: the run's length.
__device__ __forceinline__ int wave_run_len(unsigned long long brk, int lane) {
  const unsigned long long above = lane == 63 ? 0ull : brk >> (lane + 1);
  return above ? __ffsll((long long)above) : 64 - lane;
}

// ---------------------------------------------------------------------------------------------
// workgroups of 256 threads (four waves)
// A fixed tree over the 256 threads of a workgroup: xor shuffles inside a wave, then the four waves in order.  The order
// of the additions is part of the contract: the callers' sums agree between two runs in every bit.  wsum: double[4] in LDS.
__device__ __forceinline__ double block_sum_f64(double v, double* wsum) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  return (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// K per-thread counters (each below 2^32 over a wave) added to dst[0..K): per wave, per workgroup, then one integer atomic
// per workgroup and non-zero counter.  Called by every thread of the workgroup, once per kernel: with an array, or with a
// braced list of scalars, block_add_counts({cnt, chg}, result).  (static: the LDS array is each kernel's own.)
template <int K>
static __device__ __forceinline__ void block_add_counts(const uint32_t (&cnt)[K], unsigned long long* __restrict__ dst) {
  __shared__ uint32_t red[4][K];
  uint32_t w[K];
#pragma unroll
  for (int k = 0; k < K; k++) w[k] = wave_sum_u32(cnt[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; k++) red[threadIdx.x >> 6][k] = w[k];
  }
  __syncthreads();
  if (threadIdx.x < K) {
    const unsigned long long s = (unsigned long long)red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] +
                                 red[3][threadIdx.x];
    if (s) atomicAdd(dst + threadIdx.x, s);
  }
}
