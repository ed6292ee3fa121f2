// What the window entries (sw_infer.hip) and the slice entries (slice_infer.hip) of the inference tail share: the launch
// shape, the order of the mirror variants and the fp32 softmax of one voxel.
#pragma once
#include "metrics.h"

// every rounding in the units that include this is written out (a fused multiply-add is spelled __builtin_fmaf)
#pragma clang fp contract(off)

namespace {
constexpr int SW_MAXC = HDF_CLASS_SLOTS;
constexpr int SW_MAX_TABLE = 4096;   // doubles of the per-axis tables held in LDS (32 KiB)
constexpr int SW_THREADS = 256;
constexpr int SW_MAX_BLOCKS = 4096;

// code of the k-th mirror variant: the subsets of `mask` (at most three bits) in ascending order of their code, i.e. the
// bits of k dealt out to the set bits of mask from the lowest up
__device__ __forceinline__ unsigned sw_variant(unsigned mask, unsigned k) {
  unsigned m = 0;
#pragma unroll
  for (unsigned b = 0; b < 3; b++)
    if ((mask >> b) & 1u) {
      m |= (k & 1u) << b;
      k >>= 1;
    }
  return m;
}

// fp32 softmax over the classes of one voxel, as sw_accumulate_kernel (metrics.hip) takes it: v[c] = exp(l_c - max),
// returns 1 / sum; the softmax is v[c] * that
template <typename T>
__device__ __forceinline__ float sw_softmax(const T* __restrict__ p, int64_t plane, int C, float* v) {
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < SW_MAXC; c++)
    if (c < C) {
      v[c] = ST<T>::ld(p + c * plane);
      mx = fmaxf(mx, v[c]);
    }
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < SW_MAXC; c++)
    if (c < C) {
      v[c] = expf(v[c] - mx);
      sum += v[c];
    }
  return 1.f / sum;
}

inline unsigned sw_grid(int64_t n) { return (unsigned)std::min<int64_t>(ceil_div64(n, SW_THREADS), SW_MAX_BLOCKS); }
}  // namespace
