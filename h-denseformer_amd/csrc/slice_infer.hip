// Slice-wise volume inference for the 2-D model: what stands around the forward of a group of slices of one in-plane
// window -- the maxima of the volume's planes (once per call), the gather of the slices' mirrored and normalised copies
// into the forward's batch [slices x K variants], and the tail that un-mirrors, averages and accumulates their softmaxes
// into the volume's accumulators.  The per-voxel arithmetic is that of sw_infer.hip on windows of depth 1.
//
// Reference: eval.py:112-123 / :208-230 (Normalize_2d, predict_process), data_utils/data_loader.py:39-50 (MRNormalize per
// plane, the validation chain of trainer.py:173-176), SemanticSeg.get_gaussian on a plane (trainer.py:620-638);
// include/hdf.h states the arithmetic.
#include "sw_common.h"

namespace {
constexpr int PM_THREADS = 1024;

// max_out[p] = the maximum of plane p.  One workgroup per plane (a slice is a few hundred KiB: 16 waves of 128-bit
// loads keep a compute unit's share of the bandwidth busy, and a volume has more planes than the chip has compute units
// to spare), so a plane's maximum is formed in one place: no atomics, nothing to initialise.
template <int VEC>
__global__ __launch_bounds__(PM_THREADS) void plane_max_kernel(const float* __restrict__ image, int planes, int64_t pv,
                                                              float* __restrict__ max_out) {
  __shared__ float red[PM_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int p = blockIdx.x; p < planes; p += gridDim.x) {
    const float* src = image + (int64_t)p * pv;
    float mx = -INFINITY;
    if constexpr (VEC == 4) {
      const f32x4* src4 = reinterpret_cast<const f32x4*>(src);
#pragma unroll 4
      for (int64_t i = threadIdx.x; i < pv / 4; i += PM_THREADS) {
        const f32x4 v = src4[i];
        mx = fmaxf(fmaxf(mx, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
      }
    } else {
#pragma unroll 4
      for (int64_t i = threadIdx.x; i < pv; i += PM_THREADS) mx = fmaxf(mx, src[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int w = 1; w < PM_THREADS / 64; w++) mx = fmaxf(mx, red[w]);
      max_out[p] = mx;
    }
    __syncthreads();   // red is free again for the next plane
  }
}

// out[s][k][c][y][x] = the voxel of slice z0 + s, mirrored WITHIN the clipped extent (flip the content, then pad: the
// zeros stay at the high end of both axes) and divided by its plane's maximum.  One thread per VEC consecutive output
// elements of a row, as sw_gather_kernel: along x a wave reads one contiguous segment of the image (backwards when x is
// mirrored) and writes one.
template <int VEC>
__global__ __launch_bounds__(SW_THREADS) void slice_gather_kernel(const float* __restrict__ image, int C, int D, int H,
                                                                 int W, int z0, int y0, int x0, int eh, int ew, int Ph,
                                                                 int Pw, unsigned mask, int K, int mode,
                                                                 const float* __restrict__ plane_max, uint32_t groups,
                                                                 float* __restrict__ out) {
  const uint32_t per_row = (uint32_t)Pw / VEC;
  for (uint32_t i = blockIdx.x * SW_THREADS + threadIdx.x; i < groups; i += gridDim.x * SW_THREADS) {
    uint32_t r = i;
    const int x = (int)(r % per_row) * VEC;
    r /= per_row;
    const int y = (int)(r % (uint32_t)Ph);
    r /= (uint32_t)Ph;
    const int c = (int)(r % (uint32_t)C);
    r /= (uint32_t)C;
    const unsigned m = sw_variant(mask, r % (uint32_t)K);   // bit 0 = y, bit 1 = x
    const int z = z0 + (int)(r / (uint32_t)K);
    float val[VEC];
#pragma unroll
    for (int j = 0; j < VEC; j++) val[j] = 0.f;
    if (y < eh) {
      const int sy = (m & 1u) ? eh - 1 - y : y;
      const float* row = image + (((int64_t)c * D + z) * H + (y0 + sy)) * W + x0;
      const float mx = mode ? plane_max[c * D + z] : 0.f;
#pragma unroll
      for (int j = 0; j < VEC; j++)
        if (x + j < ew) {
          float v = row[(m & 2u) ? ew - 1 - (x + j) : x + j];
          if (mx != 0.f) v = v / mx;               // one IEEE division, as norm_apply_kernel (augment.hip)
          if (mode == 1) v = v < 0.f ? 0.f : v;
          val[j] = v;
        }
    }
    if constexpr (VEC == 4)
      *reinterpret_cast<f32x4*>(out + (int64_t)i * 4) = f32x4{val[0], val[1], val[2], val[3]};
    else
      out[i] = val[0];
  }
}

// One thread per voxel of the nz clipped windows, slices outer.  sw_accumulate_tta_kernel on a window of depth 1, slice
// after slice in one launch: the K variants of a slice's logits [K][C][Ph][Pw] are read at their mirrored places with the
// patch's strides, their softmaxes summed in registers; the weight comes from the two tables in LDS; then one
// read-modify-write per class plane and one on weight_sum.  The slices' voxels are disjoint: no atomics.
template <typename T>
__global__ __launch_bounds__(SW_THREADS) void slice_accumulate_kernel(const T* __restrict__ logits, unsigned mask, int K,
                                                                     int C, int nz, int eh, int ew, int Ph, int Pw,
                                                                     const double* __restrict__ tables, float lowest,
                                                                     float* __restrict__ psum, float* __restrict__ wsum,
                                                                     int D, int H, int W, int z0, int y0, int x0) {
  extern __shared__ double tab[];
  const bool weighted = tables != nullptr;
  double peak = 1.0;
  if (weighted) {
    for (int i = threadIdx.x; i < eh + ew; i += SW_THREADS) tab[i] = tables[i];
    __syncthreads();
    peak = tab[eh / 2] * tab[eh + ew / 2];
  }
  const uint32_t ev = (uint32_t)nz * eh * ew;
  const int64_t pv = (int64_t)Ph * Pw, V = (int64_t)D * H * W;
  const float inv_k = 1.f / (float)K;   // a power of two
  for (uint32_t i = blockIdx.x * SW_THREADS + threadIdx.x; i < ev; i += gridDim.x * SW_THREADS) {
    const int x = (int)(i % (uint32_t)ew), y = (int)((i / (uint32_t)ew) % (uint32_t)eh);
    const int s = (int)(i / ((uint32_t)ew * eh));
    const int64_t o = ((int64_t)(z0 + s) * H + (y0 + y)) * W + (x0 + x);
    const T* slice = logits + (int64_t)s * K * C * pv;
    float v[SW_MAXC];
    if (K == 1 && !weighted) {
      // hdf_sw_accumulate on a strided patch: its operations (it adds the softmax with one fused multiply-add), its bits
      const float inv = sw_softmax(slice + (int64_t)y * Pw + x, pv, C, v);
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
      const int ly = (m & 1u) ? eh - 1 - y : y, lx = (m & 2u) ? ew - 1 - x : x;
      const float inv = sw_softmax(slice + (int64_t)k * C * pv + (int64_t)ly * Pw + lx, pv, C, v);
#pragma unroll
      for (int c = 0; c < SW_MAXC; c++)
        if (c < C) p[c] += v[c] * inv;
    }
    float w = 1.f;
    if (weighted) {
      // fp64, one rounding to fp32 (scipy's separable gaussian_filter on a unit impulse of the plane, over its maximum)
      w = (float)((tab[y] * tab[eh + x]) / peak);
      if (w == 0.f) w = lowest;
    }
#pragma unroll
    for (int c = 0; c < SW_MAXC; c++)
      if (c < C) psum[c * V + o] += w * (inv_k * p[c]);
    wsum[o] += w;
  }
}

// the checks the two window entries share; `what` names the entry in the message
int slice_check_window(const char* what, int D, int H, int W, int z0, int nz, int y0, int x0, int eh, int ew, int Ph, int Pw,
                       unsigned mask) {
  HDF_CHECK_ARG(D >= 1 && nz >= 1 && z0 >= 0 && z0 <= D - nz, "%s: slices %d..%d of a volume of %d", what, z0,
                z0 + nz - 1, D);
  HDF_CHECK_ARG(eh >= 1 && ew >= 1 && eh <= Ph && ew <= Pw, "%s: window extent %dx%d (every axis >= 1, within the patch %dx%d)",
                what, eh, ew, Ph, Pw);
  HDF_CHECK_ARG(y0 >= 0 && x0 >= 0 && y0 <= H - eh && x0 <= W - ew, "%s: window (%d,%d)+(%d,%d) outside the %dx%d plane",
                what, y0, x0, eh, ew, H, W);
  HDF_CHECK_ARG(mask < 4u, "%s: mirror_mask %u (bit 0 = y, 1 = x: at most 3)", what, mask);
  return HDF_OK;
}
}  // namespace

int hdf_launch_plane_max(const float* image, int planes, int64_t pv, float* max_out, hipStream_t st) {
  HDF_CHECK_ARG(planes >= 1 && pv >= 1, "plane_max: %d planes of %lld voxels (both >= 1)", planes, (long long)pv);
  const dim3 grid((unsigned)std::min(planes, SW_MAX_BLOCKS));
  if (pv % 4 == 0 && (reinterpret_cast<uintptr_t>(image) & 15) == 0)
    hipLaunchKernelGGL(plane_max_kernel<4>, grid, dim3(PM_THREADS), 0, st, image, planes, pv, max_out);
  else
    hipLaunchKernelGGL(plane_max_kernel<1>, grid, dim3(PM_THREADS), 0, st, image, planes, pv, max_out);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_slice_gather(const float* image, int C, int D, int H, int W, int z0, int nz, int y0, int x0, int eh, int ew,
                            int Ph, int Pw, unsigned mask, int mode, const float* plane_max, float* out, hipStream_t st) {
  HDF_TRY(slice_check_window("slice_gather", D, H, W, z0, nz, y0, x0, eh, ew, Ph, Pw, mask));
  HDF_CHECK_ARG(mode >= 0 && mode <= 2, "slice_gather: norm_mode %d (0 copy, 1 MRNormalize, 2 Normalize_2d)", mode);
  HDF_CHECK_ARG(mode == 0 || plane_max, "slice_gather: norm_mode %d needs plane_max", mode);
  const int K = 1 << __builtin_popcount(mask);
  HDF_CHECK_ARG(C >= 1 && (double)nz * K * C * Ph * Pw < 2147483648.0,
                "slice_gather: %d slices x %d variants x %d channels x %dx%d (channels >= 1, fewer than 2^31 elements)", nz, K,
                C, Ph, Pw);
  const int64_t total = (int64_t)nz * K * C * Ph * Pw;
  if (Pw % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0)
    hipLaunchKernelGGL(slice_gather_kernel<4>, dim3(sw_grid(total / 4)), dim3(SW_THREADS), 0, st, image, C, D, H, W, z0, y0,
                       x0, eh, ew, Ph, Pw, mask, K, mode, plane_max, (uint32_t)(total / 4), out);
  else
    hipLaunchKernelGGL(slice_gather_kernel<1>, dim3(sw_grid(total)), dim3(SW_THREADS), 0, st, image, C, D, H, W, z0, y0, x0,
                       eh, ew, Ph, Pw, mask, K, mode, plane_max, (uint32_t)total, out);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_slice_accumulate(int dtype, const void* logits, unsigned mask, int C, int nz, int eh, int ew, int Ph, int Pw,
                                const double* tables, float floor, float* psum, float* wsum, int D, int H, int W, int z0,
                                int y0, int x0, hipStream_t st) {
  HDF_CHECK_ARG(C >= 1 && C <= SW_MAXC, "slice_accumulate: n_cls=%d (max %d)", C, SW_MAXC);
  HDF_TRY(slice_check_window("slice_accumulate", D, H, W, z0, nz, y0, x0, eh, ew, Ph, Pw, mask));
  HDF_CHECK_ARG((double)nz * eh * ew < 2147483648.0, "slice_accumulate: %d slices of %dx%d: 2^31 or more voxels", nz, eh,
                ew);
  HDF_CHECK_ARG(!tables || (int64_t)eh + ew <= SW_MAX_TABLE, "slice_accumulate: %dx%d: tables of more than %d entries", eh, ew,
                SW_MAX_TABLE);
  const int K = 1 << __builtin_popcount(mask);
  const size_t lds = tables ? (size_t)(eh + ew) * sizeof(double) : 0;
  HDF_DISPATCH_T(dtype, hipLaunchKernelGGL(slice_accumulate_kernel<T>, dim3(sw_grid((int64_t)nz * eh * ew)), dim3(SW_THREADS),
                                           lds, st, (const T*)logits, mask, K, C, nz, eh, ew, Ph, Pw, tables, floor, psum, wsum,
                                           D, H, W, z0, y0, x0));
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
