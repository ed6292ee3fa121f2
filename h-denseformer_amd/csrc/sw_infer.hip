// Sliding-window inference with a Gaussian importance map and mirror test-time augmentation: the three launches of one
// window next to its forward -- gather the K mirrored copies of the window into the forward's batch, (once per call) the
// floor of the importance map, and the tail that un-mirrors, averages and accumulates the K softmaxes.
//
// Reference: the importance map is SemanticSeg.get_gaussian (trainer.py:620-638), whose use sits commented out beside the
// accumulation (trainer.py:566-576); include/hdf.h states the arithmetic.
#include "sw_common.h"   // the launch shape, sw_variant (here bit 0 = z, 1 = y, 2 = x), sw_softmax; fp contract(off)

namespace {
// out[k][c][z][y][x] = the window's voxel mirrored WITHIN the clipped extent (flip the content, then pad): zeros beyond
// the extent stay at the high end of every axis.  One thread per VEC consecutive output elements of a row (4 in one
// store where the row length and the address allow it: the index arithmetic, not the traffic, bounds the scalar form);
// along x a wave reads one contiguous segment of the image (backwards when x is mirrored) and writes one.
template <int VEC>
__global__ __launch_bounds__(SW_THREADS) void sw_gather_kernel(const float* __restrict__ image, int C, int D, int H, int W,
                                                              int z0, int y0, int x0, int ed, int eh, int ew, int Pd,
                                                              int Ph, int Pw, unsigned mask, uint32_t groups,
                                                              float* __restrict__ out) {
  const uint32_t per_row = (uint32_t)Pw / VEC;
  for (uint32_t i = blockIdx.x * SW_THREADS + threadIdx.x; i < groups; i += gridDim.x * SW_THREADS) {
    uint32_t r = i;
    const int x = (int)(r % per_row) * VEC;
    r /= per_row;
    const int y = (int)(r % (uint32_t)Ph);
    r /= (uint32_t)Ph;
    const int z = (int)(r % (uint32_t)Pd);
    r /= (uint32_t)Pd;
    const int c = (int)(r % (uint32_t)C);
    const unsigned m = sw_variant(mask, r / (uint32_t)C);
    float val[VEC];
#pragma unroll
    for (int j = 0; j < VEC; j++) val[j] = 0.f;
    if (z < ed && y < eh) {
      const int sz = (m & 1u) ? ed - 1 - z : z, sy = (m & 2u) ? eh - 1 - y : y;
      const float* row = image + (((int64_t)c * D + (z0 + sz)) * H + (y0 + sy)) * W + x0;
#pragma unroll
      for (int j = 0; j < VEC; j++)
        if (x + j < ew) val[j] = row[(m & 4u) ? ew - 1 - (x + j) : x + j];
    }
    if constexpr (VEC == 4)
      *reinterpret_cast<f32x4*>(out + (int64_t)i * 4) = f32x4{val[0], val[1], val[2], val[3]};
    else
      out[i] = val[0];
  }
}

// the three tables (tz | ty | tx) into LDS; ends with the barrier after which every thread may read them
__device__ __forceinline__ void sw_load_tables(const double* __restrict__ tables, int n, double* tab) {
  for (int i = threadIdx.x; i < n; i += SW_THREADS) tab[i] = tables[i];
  __syncthreads();
}
// fp64 in this order, one rounding to fp32 (scipy's separable gaussian_filter on a unit impulse, divided by its maximum)
__device__ __forceinline__ float sw_weight(const double* tab, int ed, int eh, double peak, int z, int y, int x) {
  return (float)(((tab[z] * tab[ed + y]) * tab[ed + eh + x]) / peak);
}
__device__ __forceinline__ double sw_peak(const double* tab, int ed, int eh, int ew) {
  return (tab[ed / 2] * tab[ed + eh / 2]) * tab[ed + eh + ew / 2];
}

// smallest non-zero weight of the window: positive floats order like their bit patterns, so an integer minimum over the
// patterns is exact and does not depend on arrival order
__global__ __launch_bounds__(SW_THREADS) void sw_floor_kernel(const double* __restrict__ tables, int ed, int eh, int ew,
                                                             unsigned* __restrict__ floor_bits) {
  extern __shared__ double tab[];
  __shared__ unsigned blk;
  if (threadIdx.x == 0) blk = 0xffffffffu;
  sw_load_tables(tables, ed + eh + ew, tab);
  const double peak = sw_peak(tab, ed, eh, ew);
  const uint32_t ev = (uint32_t)ed * eh * ew;
  unsigned lo = 0xffffffffu;
  for (uint32_t i = blockIdx.x * SW_THREADS + threadIdx.x; i < ev; i += gridDim.x * SW_THREADS) {
    const int x = (int)(i % (uint32_t)ew), y = (int)((i / (uint32_t)ew) % (uint32_t)eh);
    const int z = (int)(i / ((uint32_t)ew * eh));
    const unsigned bits = __float_as_uint(sw_weight(tab, ed, eh, peak, z, y, x));
    if (bits != 0u) lo = min(lo, bits);
  }
  if (lo != 0xffffffffu) atomicMin(&blk, lo);
  __syncthreads();
  if (threadIdx.x == 0 && blk != 0xffffffffu) atomicMin(floor_bits, blk);
}

// One thread per voxel of the clipped window.  The K variants of the logits [K][C][Pd][Ph][Pw] are read at their mirrored
// places with the patch's strides (a wave reads one contiguous segment per class and variant, backwards when x is
// mirrored), their softmaxes summed in registers; the weight comes from the three tables in LDS; then one
// read-modify-write per class plane and one on weight_sum.  Windows follow each other on one stream: no atomics.
template <typename T>
__global__ __launch_bounds__(SW_THREADS) void sw_accumulate_tta_kernel(const T* __restrict__ logits, unsigned mask, int K,
                                                                      int C, int ed, int eh, int ew, int Pd, int Ph,
                                                                      int Pw, const double* __restrict__ tables,
                                                                      const float* __restrict__ floor,
                                                                      float* __restrict__ psum, float* __restrict__ wsum,
                                                                      int D, int H, int W, int z0, int y0, int x0) {
  extern __shared__ double tab[];
  const bool weighted = tables != nullptr;
  double peak = 1.0;
  float lowest = 0.f;
  if (weighted) {
    sw_load_tables(tables, ed + eh + ew, tab);
    peak = sw_peak(tab, ed, eh, ew);
    lowest = *floor;
  }
  const uint32_t ev = (uint32_t)ed * eh * ew;
  const int64_t pv = (int64_t)Pd * Ph * Pw, V = (int64_t)D * H * W;
  const float inv_k = 1.f / (float)K;   // a power of two
  for (uint32_t i = blockIdx.x * SW_THREADS + threadIdx.x; i < ev; i += gridDim.x * SW_THREADS) {
    const int x = (int)(i % (uint32_t)ew), y = (int)((i / (uint32_t)ew) % (uint32_t)eh);
    const int z = (int)(i / ((uint32_t)ew * eh));
    const int64_t o = ((int64_t)(z0 + z) * H + (y0 + y)) * W + (x0 + x);
    float v[SW_MAXC];
    if (K == 1 && !weighted) {
      // hdf_sw_accumulate on a strided patch: its operations (it adds the softmax with one fused multiply-add), its bits
      const float inv = sw_softmax(logits + ((int64_t)z * Ph + y) * Pw + x, pv, C, v);
#pragma unroll
      for (int c = 0; c < SW_MAXC; c++)
        if (c < C) psum[c * V + o] = __builtin_fmaf(v[c], inv, psum[c * V + o]);
      wsum[o] += 1.f;
      continue;
    }
    float p[SW_MAXC];
#pragma unroll
    for (int c = 0; c < SW_MAXC; c++) p[c] = 0.f;
    for (int k = 0; k < K; k++) {
      const unsigned m = sw_variant(mask, (unsigned)k);
      const int lz = (m & 1u) ? ed - 1 - z : z, ly = (m & 2u) ? eh - 1 - y : y, lx = (m & 4u) ? ew - 1 - x : x;
      const float inv = sw_softmax(logits + (int64_t)k * C * pv + ((int64_t)lz * Ph + ly) * Pw + lx, pv, C, v);
#pragma unroll
      for (int c = 0; c < SW_MAXC; c++)
        if (c < C) p[c] += v[c] * inv;
    }
    float w = 1.f;
    if (weighted) {
      w = sw_weight(tab, ed, eh, peak, z, y, x);
      if (w == 0.f) w = lowest;
    }
#pragma unroll
    for (int c = 0; c < SW_MAXC; c++)
      if (c < C) psum[c * V + o] += w * (inv_k * p[c]);
    wsum[o] += w;
  }
}

// the checks the three entries share; `what` names the entry in the message
int sw_check_window(const char* what, int D, int H, int W, int z0, int y0, int x0, int ed, int eh, int ew) {
  HDF_CHECK_ARG(ed >= 1 && eh >= 1 && ew >= 1 && (int64_t)ed * eh * ew < (int64_t)1 << 31,
                "%s: window extent %dx%dx%d (every axis >= 1, fewer than 2^31 voxels)", what, ed, eh, ew);
  HDF_CHECK_ARG(z0 >= 0 && y0 >= 0 && x0 >= 0 && z0 <= D - ed && y0 <= H - eh && x0 <= W - ew,
                "%s: window (%d,%d,%d)+(%d,%d,%d) outside the %dx%dx%d volume", what, z0, y0, x0, ed, eh, ew, D, H, W);
  return HDF_OK;
}
int sw_check_patch(const char* what, int ed, int eh, int ew, int Pd, int Ph, int Pw, unsigned mask) {
  HDF_CHECK_ARG(ed <= Pd && eh <= Ph && ew <= Pw, "%s: extent %dx%dx%d exceeds the patch %dx%dx%d", what, ed, eh, ew, Pd,
                Ph, Pw);
  HDF_CHECK_ARG(mask < 8u, "%s: mirror_mask %u (bit 0 = z, 1 = y, 2 = x: at most 7)", what, mask);
  return HDF_OK;
}
}  // namespace

int hdf_launch_sw_gather(const float* image, int C, int D, int H, int W, int z0, int y0, int x0, int ed, int eh, int ew,
                         int Pd, int Ph, int Pw, unsigned mask, float* out, hipStream_t st) {
  HDF_TRY(sw_check_window("sw_gather", D, H, W, z0, y0, x0, ed, eh, ew));
  HDF_TRY(sw_check_patch("sw_gather", ed, eh, ew, Pd, Ph, Pw, mask));
  const int K = 1 << __builtin_popcount(mask);
  HDF_CHECK_ARG(C >= 1 && (int64_t)K * C * Pd * Ph * Pw < (int64_t)1 << 31,
                "sw_gather: %d variants x %d channels x %dx%dx%d (channels >= 1, fewer than 2^31 elements)", K, C, Pd, Ph, Pw);
  const int64_t total = (int64_t)K * C * Pd * Ph * Pw;
  if (Pw % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0)
    hipLaunchKernelGGL(sw_gather_kernel<4>, dim3(sw_grid(total / 4)), dim3(SW_THREADS), 0, st, image, C, D, H, W, z0, y0, x0,
                       ed, eh, ew, Pd, Ph, Pw, mask, (uint32_t)(total / 4), out);
  else
    hipLaunchKernelGGL(sw_gather_kernel<1>, dim3(sw_grid(total)), dim3(SW_THREADS), 0, st, image, C, D, H, W, z0, y0, x0, ed,
                       eh, ew, Pd, Ph, Pw, mask, (uint32_t)total, out);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_sw_importance_floor(const double* tables, int ed, int eh, int ew, float* floor_out, hipStream_t st) {
  HDF_CHECK_ARG(ed >= 1 && eh >= 1 && ew >= 1 && (int64_t)ed * eh * ew < (int64_t)1 << 31,
                "sw_importance_floor: window extent %dx%dx%d (every axis >= 1, fewer than 2^31 voxels)", ed, eh, ew);
  HDF_CHECK_ARG((int64_t)ed + eh + ew <= SW_MAX_TABLE, "sw_importance_floor: %dx%dx%d: tables of more than %d entries", ed, eh,
                ew, SW_MAX_TABLE);
  hipError_t e = hipMemsetAsync(floor_out, 0xff, sizeof(float), st);   // the identity of the unsigned minimum
  if (e != hipSuccess) {
    hdf_set_error("sw_importance_floor: memset failed: %s", hipGetErrorString(e));
    return HDF_ERR_HIP;
  }
  hipLaunchKernelGGL(sw_floor_kernel, dim3(sw_grid((int64_t)ed * eh * ew)), dim3(SW_THREADS),
                     (size_t)(ed + eh + ew) * sizeof(double), st, tables, ed, eh, ew, (unsigned*)floor_out);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_sw_accumulate_tta(int dtype, const void* logits, unsigned mask, int C, int ed, int eh, int ew, int Pd, int Ph,
                                 int Pw, const double* tables, const float* floor, float* psum, float* wsum, int D, int H,
                                 int W, int z0, int y0, int x0, hipStream_t st) {
  HDF_CHECK_ARG(C >= 1 && C <= SW_MAXC, "sw_accumulate_tta: n_cls=%d (max %d)", C, SW_MAXC);
  HDF_TRY(sw_check_window("sw_accumulate_tta", D, H, W, z0, y0, x0, ed, eh, ew));
  HDF_TRY(sw_check_patch("sw_accumulate_tta", ed, eh, ew, Pd, Ph, Pw, mask));
  HDF_CHECK_ARG((tables == nullptr) == (floor == nullptr), "sw_accumulate_tta: tables and floor go together (%s is null)",
                tables ? "floor" : "tables");
  HDF_CHECK_ARG(!tables || (int64_t)ed + eh + ew <= SW_MAX_TABLE, "sw_accumulate_tta: %dx%dx%d: tables of more than %d entries",
                ed, eh, ew, SW_MAX_TABLE);
  const int K = 1 << __builtin_popcount(mask);
  const size_t lds = tables ? (size_t)(ed + eh + ew) * sizeof(double) : 0;
  HDF_DISPATCH_T(dtype, hipLaunchKernelGGL(sw_accumulate_tta_kernel<T>, dim3(sw_grid((int64_t)ed * eh * ew)),
                                           dim3(SW_THREADS), lds, st, (const T*)logits, mask, K, C, ed, eh, ew, Pd, Ph, Pw,
                                           tables, floor, psum, wsum, D, H, W, z0, y0, x0));
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
