// What the attention kernels of transformer.hip and the attention phases of the persistent kernels (tf_chain.h) share.
// tests/test_gpu_chain.py holds the two to each other bit for bit: the pieces of that contract that are the same text on
// both sides are defined here, once.
#pragma once
#include "transformer.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 lo2(const float4& v) { return f2{v.x, v.y}; }
__device__ __forceinline__ f2 hi2(const float4& v) { return f2{v.z, v.w}; }
// keys per trip = one 16 x 16 block of the score MFMA; the per-sequence LDS arrays are padded to whole trips
constexpr int ATRIP = 16;
__host__ __device__ inline int attn_rows(int N) { return (N + ATRIP - 1) / ATRIP * ATRIP; }

// 16-bit operands of v_mfma_f32_16x16x16 in the 16-bit storage modes (LP = HDF_BF16 / HDF_F16): one value, four packed
// values (a lane's A or B operand), the matrix instruction
template <int LP>
struct LpPack;
template <>
struct LpPack<1> {  // bf16
  static __device__ __forceinline__ uint16_t one(float v) { return f2bf(v); }
  static __device__ __forceinline__ u32x2 four(float a, float b, float c, float d) { return u32x2{pack_bf2(a, b), pack_bf2(c, d)}; }
  static __device__ __forceinline__ f32x4 mma(const u32x2& a, const u32x2& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, a), __builtin_bit_cast(s16x4, b), c, 0, 0, 0);
  }
};
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
template <>
struct LpPack<2> {  // f16
  static __device__ __forceinline__ uint16_t one(float v) { return f2h(v); }
  static __device__ __forceinline__ u32x2 four(float a, float b, float c, float d) { return u32x2{pack_h2(a, b), pack_h2(c, d)}; }
  static __device__ __forceinline__ f32x4 mma(const u32x2& a, const u32x2& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(f16x4, a), __builtin_bit_cast(f16x4, b), c, 0, 0, 0);
  }
};

}  // namespace
