// InstanceNorm around the convolutions: the statistics' finalise (forward), norm+ReLU(+skip) materialisation, and the
// InstanceNorm+ReLU backward (reduce / finalise / apply).  The conv kernels write the forward (sum, sumsq) partials.
//
// Reference semantics: HDenseFormer.py:148-175 (BasicConv3d / UpConv); torch semantics restated in SURVEY.md appendix A
// items 7-9.
#include "unet_ops_internal.h"

namespace {

// ------------------------------------------------------------------------------ IN statistics
// one workgroup per (n, 8-channel group): 32 tile lanes x 8 channels, 4 independent loads in flight per
// thread, double accumulation in a fixed order (bitwise reproducible).  256 threads and few registers ON PURPOSE: the
// 1024-thread form (32 x 32, 128 registers) needed a compute unit with every SIMD empty, and next to a persistent conv /
// weight-gradient kernel of another stream (one wave per SIMD, 300-430 registers) this 5 us kernel waited 60-95 us for
// that kernel to END (r03c timeline: five such waits on the caller's stream in one backward).
constexpr int FIN_LANES = 32, FIN_CG = 8;
__global__ __launch_bounds__(256, 4) void in_finalize_kernel(const float* __restrict__ partials, int tiles, int C, int CP,
                                                           int64_t vox, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float eps,
                                                           float* __restrict__ mean, float* __restrict__ rstd,
                                                           float* __restrict__ scale, float* __restrict__ shift) {
  HDF_LIGHT_PRIO();
  __shared__ double red[FIN_LANES][FIN_CG][2];
  const int n = blockIdx.y, cg = blockIdx.x;
  const int cl = threadIdx.x & (FIN_CG - 1), c = cg * FIN_CG + cl, tl = threadIdx.x / FIN_CG;
  double s1 = 0.0, s2 = 0.0;
  if (c < CP) {
    const float* p = partials + ((int64_t)n * tiles * CP + c) * 2;
    const int64_t ts = (int64_t)CP * 2;
    int t = tl;
    for (; t + 3 * FIN_LANES < tiles; t += 4 * FIN_LANES) {
      float2 v0 = *reinterpret_cast<const float2*>(p + (int64_t)t * ts);
      float2 v1 = *reinterpret_cast<const float2*>(p + (int64_t)(t + FIN_LANES) * ts);
      float2 v2 = *reinterpret_cast<const float2*>(p + (int64_t)(t + 2 * FIN_LANES) * ts);
      float2 v3 = *reinterpret_cast<const float2*>(p + (int64_t)(t + 3 * FIN_LANES) * ts);
      s1 += ((double)v0.x + (double)v1.x) + ((double)v2.x + (double)v3.x);
      s2 += ((double)v0.y + (double)v1.y) + ((double)v2.y + (double)v3.y);
    }
    for (; t < tiles; t += FIN_LANES) {
      float2 v = *reinterpret_cast<const float2*>(p + (int64_t)t * ts);
      s1 += (double)v.x;
      s2 += (double)v.y;
    }
  }
  red[tl][cl][0] = s1;
  red[tl][cl][1] = s2;
  __syncthreads();
  if (tl == 0 && c < C) {
    for (int k = 1; k < FIN_LANES; k++) {
      s1 += red[k][cl][0];
      s2 += red[k][cl][1];
    }
    double m = s1 / (double)vox;
    double var = s2 / (double)vox - m * m;  // biased variance
    if (var < 0.0) var = 0.0;
    float r = (float)(1.0 / sqrt(var + (double)eps));
    float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
    int64_t o = (int64_t)n * C + c;
    mean[o] = (float)m;
    rstd[o] = r;
    scale[o] = g * r;
    shift[o] = b - (float)m * g * r;
  }
}

// ------------------------------------------------------------------------------ norm+relu(+skip)
template <typename T>
__global__ void norm_relu_add_kernel(const T* __restrict__ y, int64_t y_pitch, const float* __restrict__ scale,
                                     const float* __restrict__ shift, const T* __restrict__ skip, int64_t skip_pitch,
                                     T* __restrict__ out, int64_t out_pitch, int N, int C, int64_t vox) {
  HDF_LIGHT_PRIO();
  constexpr int EPC = ST<T>::EPC;
  const int cols = C / EPC;
  int64_t total = (int64_t)N * vox * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t row = i / cols;
    int c0 = (int)(i - row * cols) * EPC;
    int n = (int)(row / vox);
    float f[EPC], s[EPC];
    load_chunk<T>(y + row * y_pitch + c0, f);
    if (skip) load_chunk<T>(skip + row * skip_pitch + c0, s);
#pragma unroll
    for (int e = 0; e < EPC; e++) {
      float v = fmaxf(f[e] * scale[(int64_t)n * C + c0 + e] + shift[(int64_t)n * C + c0 + e], 0.f);
      f[e] = skip ? v + s[e] : v;
    }
    store_chunk<T>(out + row * out_pitch + c0, f);
  }
}

// ------------------------------------------------------------------------------ IN + ReLU backward
// grid (blocks, N).  thread = (voxel lane, channel chunk).  The two streaming passes take FOUR channels per thread for
// every storage type (16-bit: 8-byte loads; fp32: one 16-byte load).  Why not 8 with 16-byte loads in the 16-bit modes:
// those forms needed 160 / 114 registers, and backward runs these passes on the caller's stream NEXT TO a persistent
// weight-gradient kernel of the side stream that holds one wave per SIMD with 301-376 of its 512 registers: the heavy
// forms then got one wave per SIMD or none at all (a reduce pass of 60 us took 237 us, and the weight gradient it was
// supposed to hide cost as much as it saved); these fit two to three waves into what is left.  The occupancy hint of
// the launch bounds holds for 16-bit storage only: under it the fp32 instantiations spill (apply 26 registers, reduce 2).
// apply: the 7 per-(n, channel) coefficient vectors are loaded ONCE per thread (re-reading them per chunk made the
// kernel load-issue bound: 56 scalar loads per 2 streaming loads).
template <typename T>
__global__ __launch_bounds__(256, sizeof(T) == 2 ? 6 : 1) void in_bwd_reduce4_kernel(const T* __restrict__ da, int64_t da_pitch,
                                                                const T* __restrict__ y, int64_t y_pitch,
                                                                const float* __restrict__ scale,
                                                                const float* __restrict__ shift,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ rstd,
                                                                float* __restrict__ partials, int blocks, int C,
                                                                int64_t vox) {
  HDF_LIGHT_PRIO();
  extern __shared__ float red[];  // [vlanes][C][2]
  const int n = blockIdx.y;
  const int cols = C >> 2, vlanes = 256 / cols;
  const int col = threadIdx.x % cols, vl = threadIdx.x / cols, c0 = col * 4;
  float s1[4], s2[4], sc[4], sh[4], mu[4], rs[4];
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const int64_t o = (int64_t)n * C + c0 + e;
    s1[e] = s2[e] = 0.f;
    sc[e] = scale[o], sh[e] = shift[o], mu[e] = mean[o], rs[e] = rstd[o];
  }
  if (vl < vlanes) {
    const int64_t per = (vox + blocks - 1) / blocks;
    const int64_t vb = (int64_t)blockIdx.x * per, ve = min(vox, vb + per);
    constexpr int U = 4;
    const T* dap = da + (int64_t)n * vox * da_pitch + c0;
    const T* yp = y + (int64_t)n * vox * y_pitch + c0;
    for (int64_t v0 = vb + vl; v0 < ve; v0 += U * vlanes) {
      float g[U][4], f[U][4];
#pragma unroll
      for (int u = 0; u < U; u++) {  // clamped (never branch around a load); the tail is masked below
        const int64_t v = min(v0 + (int64_t)u * vlanes, ve - 1);
        ST<T>::ld4(dap + v * da_pitch, g[u]);
        ST<T>::ld4(yp + v * y_pitch, f[u]);
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const bool live = v0 + (int64_t)u * vlanes < ve;
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const float gg = (live && f[u][e] * sc[e] + sh[e] > 0.f) ? g[u][e] : 0.f;
          s1[e] += gg;
          s2[e] += gg * ((f[u][e] - mu[e]) * rs[e]);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; e++) {
      red[(vl * C + c0 + e) * 2 + 0] = s1[e];
      red[(vl * C + c0 + e) * 2 + 1] = s2[e];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < C * 2; i += 256) {
    float s = 0.f;
    for (int k = 0; k < vlanes; k++) s += red[k * C * 2 + i];
    partials[((int64_t)n * blocks + blockIdx.x) * C * 2 + i] = s;
  }
}

template <typename T>
__global__ __launch_bounds__(256, sizeof(T) == 2 ? 8 : 1) void in_bwd_apply4_kernel(const T* __restrict__ da, int64_t da_pitch,
                                                               const T* __restrict__ y, int64_t y_pitch,
                                                               const float* __restrict__ scale,
                                                               const float* __restrict__ shift,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ rstd,
                                                               const float* __restrict__ k1,
                                                               const float* __restrict__ ka,
                                                               const float* __restrict__ kb, T* __restrict__ dy,
                                                               int64_t dy_pitch, int C, int64_t vox) {
  HDF_LIGHT_PRIO();
  constexpr int U = 4;
  const int n = blockIdx.y;
  const int cols = C >> 2, vlanes = 256 / cols;
  const int col = threadIdx.x % cols, vl = threadIdx.x / cols, c0 = col * 4;
  if (vl >= vlanes) return;
  float sc[4], sh[4], mu[4], rs[4], c1[4], ca[4], cb[4];
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const int64_t o = (int64_t)n * C + c0 + e;
    sc[e] = scale[o], sh[e] = shift[o], mu[e] = mean[o], rs[e] = rstd[o];
    c1[e] = k1[o], ca[e] = ka[o], cb[e] = kb[o];
  }
  const int64_t per = (vox + gridDim.x - 1) / gridDim.x;
  const int64_t vb = (int64_t)blockIdx.x * per, ve = min(vox, vb + per);
  const T* dap = da + (int64_t)n * vox * da_pitch + c0;
  const T* yp = y + (int64_t)n * vox * y_pitch + c0;
  T* dyp = dy + (int64_t)n * vox * dy_pitch + c0;
  for (int64_t v0 = vb + vl; v0 < ve; v0 += (int64_t)U * vlanes) {
    float g[U][4], f[U][4];
#pragma unroll
    for (int u = 0; u < U; u++) {  // clamped: never branch around a load
      const int64_t v = min(v0 + (int64_t)u * vlanes, ve - 1);
      ST<T>::ld4(dap + v * da_pitch, g[u]);
      ST<T>::ld4(yp + v * y_pitch, f[u]);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t v = v0 + (int64_t)u * vlanes;
      if (v < ve) {
        float d[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
          d[e] = in_bwd_elem(g[u][e], f[u][e], sc[e], sh[e], mu[e], rs[e], c1[e], ca[e], cb[e]);
        }
        ST<T>::st4(dyp + v * dy_pitch, d[0], d[1], d[2], d[3]);
      }
    }
  }
}

// grid (ceil(C/8), N), 256 threads = 32 block-lanes x 8 channels (with 8 lanes the 1024-row partial table of a
// 128^3 level cost 49 us of serial fp64 adds on two workgroups); fixed summation order; light on purpose (in_finalize)
__global__ __launch_bounds__(256, 4) void in_bwd_finalize_kernel(const float* __restrict__ partials, int blocks, int N,
                                                               int C, int64_t vox, const float* __restrict__ gamma,
                                                               const float* __restrict__ rstd, float* __restrict__ k1,
                                                               float* __restrict__ ka, float* __restrict__ kb,
                                                               float* __restrict__ dgamma, float* __restrict__ dbeta) {
  HDF_LIGHT_PRIO();
  constexpr int BL = 32;
  __shared__ double red[BL][FIN_CG][2];
  const int n = blockIdx.y, cl = threadIdx.x & (FIN_CG - 1), c = blockIdx.x * FIN_CG + cl, bl = threadIdx.x / FIN_CG;
  double s1 = 0.0, s2 = 0.0;
  if (c < C) {
    const float* p = partials + ((int64_t)n * blocks * C + c) * 2;
    const int64_t bs = (int64_t)C * 2;
    int b = bl;
    for (; b + 3 * BL < blocks; b += 4 * BL) {  // four independent loads in flight (the rows are L2 round trips)
      const float2 v0 = *reinterpret_cast<const float2*>(p + (int64_t)b * bs);
      const float2 v1 = *reinterpret_cast<const float2*>(p + (int64_t)(b + BL) * bs);
      const float2 v2 = *reinterpret_cast<const float2*>(p + (int64_t)(b + 2 * BL) * bs);
      const float2 v3 = *reinterpret_cast<const float2*>(p + (int64_t)(b + 3 * BL) * bs);
      s1 += ((double)v0.x + (double)v1.x) + ((double)v2.x + (double)v3.x);
      s2 += ((double)v0.y + (double)v1.y) + ((double)v2.y + (double)v3.y);
    }
    for (; b < blocks; b += BL) {
      const float2 v = *reinterpret_cast<const float2*>(p + (int64_t)b * bs);
      s1 += (double)v.x;
      s2 += (double)v.y;
    }
  }
  red[bl][cl][0] = s1;
  red[bl][cl][1] = s2;
  __syncthreads();
  if (bl == 0 && c < C) {
    for (int k = 1; k < BL; k++) {
      s1 += red[k][cl][0];
      s2 += red[k][cl][1];
    }
    int64_t o = (int64_t)n * C + c;
    float g = gamma ? gamma[c] : 1.f;
    k1[o] = g * rstd[o];
    ka[o] = (float)(s1 / (double)vox);
    kb[o] = (float)(s2 / (double)vox);
    if (dgamma) atomicAdd(dgamma + c, (float)s2);  // N adders per word
    if (dbeta) atomicAdd(dbeta + c, (float)s1);
  }
}

}  // namespace

// out[c] += sum over `rows` partial rows of partials[row][c][0] (the per-channel SUM column of the conv kernels'
// InstanceNorm partial table), c < C.  grid ceil(C/8), 256 threads = 32 row lanes x 8 channels, fixed order.
__global__ __launch_bounds__(256, 6) void stat_rows_sum_kernel(const float* __restrict__ partials, int rows, int C, int CP,
                                                             float* __restrict__ out) {
  HDF_LIGHT_PRIO();
  __shared__ double red[32][FIN_CG];
  const int cl = threadIdx.x & (FIN_CG - 1), c = blockIdx.x * FIN_CG + cl, rl = threadIdx.x / FIN_CG;
  double s = 0.0;
  if (c < C) {
    const float* p = partials + (int64_t)c * 2;
    const int64_t rs = (int64_t)CP * 2;
    int r = rl;
    for (; r + 96 < rows; r += 128)
      s += ((double)p[(int64_t)r * rs] + (double)p[(int64_t)(r + 32) * rs]) +
           ((double)p[(int64_t)(r + 64) * rs] + (double)p[(int64_t)(r + 96) * rs]);
    for (; r < rows; r += 32) s += (double)p[(int64_t)r * rs];
  }
  red[rl][cl] = s;
  __syncthreads();
  if (rl == 0 && c < C) {
    for (int k = 1; k < 32; k++) s += red[k][cl];
    out[c] += (float)s;
  }
}

int hdf_launch_stat_rows_sum(const float* partials, int rows, int C, int CP, float* out, hipStream_t st) {
  hipLaunchKernelGGL(stat_rows_sum_kernel, dim3(ceil_div(C, FIN_CG)), dim3(256), 0, st, partials, rows, C, CP, out);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_in_finalize(const float* partials, int N, int tiles, int C, int CP, int64_t vox, const float* gamma,
                           const float* beta, float eps, NormStatsOut out, hipStream_t st) {
  hipLaunchKernelGGL(in_finalize_kernel, dim3(ceil_div(CP, FIN_CG), N), dim3(256), 0, st, partials, tiles, C, CP, vox, gamma,
                     beta, eps, out.mean, out.rstd, out.scale, out.shift);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_norm_relu_add(int dtype, CRows y, NormStats ys, CRows skip, Rows out, int N, int C, int64_t vox,
                             hipStream_t st) {
  HDF_CHECK_ARG(C % 16 == 0, "norm_relu_add: C=%d", C);
  HDF_DISPATCH_T(dtype, hipLaunchKernelGGL(norm_relu_add_kernel<T>, dim3(grid_for((int64_t)N * vox * (C / ST<T>::EPC))),
                                       dim3(256), 0, st, (const T*)y.p, y.pitch, ys.scale, ys.shift, (const T*)skip.p,
                                       skip.pitch, (T*)out.p, out.pitch, N, C, vox));
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

// workgroups per sample of the IN-backward passes: ~2K 16-byte chunks each, so the low-resolution levels (few
// voxels, many channels) still fill the chip (with a voxel-only rule the 16^3 level ran on 4 workgroups: 85 us for 4 MB)
int hdf_in_bwd_blocks(int64_t vox, int C) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(1024, vox * (C / 8) / 2048));
}

int hdf_launch_in_bwd_reduce(int dtype, CRows da, CRows y, NormStats ys, float* partials, int blocks, int N, int C,
                             int64_t vox, hipStream_t st) {
  HDF_CHECK_ARG(C % 16 == 0 && C <= 1024, "in_bwd: C=%d", C);
  const int vlanes = 256 / (C / 4);
  HDF_DISPATCH_T(dtype, hipLaunchKernelGGL(in_bwd_reduce4_kernel<T>, dim3(blocks, N), dim3(256),
                                       (size_t)vlanes * C * 2 * sizeof(float), st, (const T*)da.p, da.pitch, (const T*)y.p,
                                       y.pitch, ys.scale, ys.shift, ys.mean, ys.rstd, partials, blocks, C, vox));
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_in_bwd_finalize(const float* partials, int blocks, int N, int C, int64_t vox, const float* gamma,
                               const float* rstd, InBwdCoefOut k, float* dgamma, float* dbeta, hipStream_t st) {
  hipLaunchKernelGGL(in_bwd_finalize_kernel, dim3(ceil_div(C, FIN_CG), N), dim3(256), 0, st, partials, blocks, N, C, vox, gamma,
                     rstd, k.k1, k.ka, k.kb, dgamma, dbeta);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_in_bwd_apply(int dtype, CRows da, CRows y, NormStats ys, InBwdCoef k, Rows dy, int N, int C, int64_t vox,
                            hipStream_t st) {
  HDF_CHECK_ARG(C % 16 == 0 && C <= 1024, "in_bwd_apply: C=%d", C);
  // ~1K chunks per workgroup, at most 2048 workgroups per sample
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(2048, vox * (C / 8) / 1024));
  HDF_DISPATCH_T(dtype, hipLaunchKernelGGL(in_bwd_apply4_kernel<T>, dim3(blocks, N), dim3(256), 0, st, (const T*)da.p,
                                       da.pitch, (const T*)y.p, y.pitch, ys.scale, ys.shift, ys.mean, ys.rstd, k.k1, k.ka,
                                       k.kb, (T*)dy.p, dy.pitch, C, vox));
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
