// What the three units of unet_ops.h share (private to norm_ops.hip, pool_ops.hip and head_ops.hip): the 16-byte channel
// chunk every thread of these HBM-bound kernels moves (8 bf16 / 4 f32 of a channels-last row, the coalescing sweet spot on
// CDNA4), the storage rounding of one value, and the grid rule of the flat grid-stride kernels.
#pragma once
#include "unet_ops.h"

namespace {

constexpr int MAX_BLOCKS = 4096;

template <typename T>
__device__ __forceinline__ void load_chunk(const T* p, float* f) {
  u32x4 v = *reinterpret_cast<const u32x4*>(p);
  ST<T>::unpack(v, f);
}
template <typename T>
__device__ __forceinline__ void store_chunk(T* p, const float* f) {
  *reinterpret_cast<u32x4*>(p) = ST<T>::pack(f);
}
// storage rounding of one value (what a later pass would read back)
template <typename T>
__device__ __forceinline__ float storage_round(float v) {
  T t;
  ST<T>::st(&t, v);
  return ST<T>::ld(&t);
}

inline unsigned grid_for(int64_t total, int block = 256) {
  return (unsigned)std::min<int64_t>(ceil_div64(total, block), MAX_BLOCKS);
}

}  // namespace
