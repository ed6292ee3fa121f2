// The 1x1x1 heads, forward and backward (the backward optionally with the first pass of the producing layer's
// InstanceNorm backward).
//
// Reference semantics: HDenseFormer.py:223-227.
#include "unet_ops_internal.h"

namespace {

// ------------------------------------------------------------------------------ 1x1x1 heads
constexpr int HEAD_MAXCLS = 8;

// Streaming form (as head_bwd below): thread = (voxel lane, 8-channel chunk) so a wave reads whole contiguous voxel
// rows; the per-chunk partial dot products are summed over the `cols` chunk lanes of a voxel with xor shuffles
// (cols is a power of two <= 32), the block's logits are staged in LDS as [class][voxel] and written plane by plane,
// coalesced.  (One thread per voxel walked a 64..512-byte row alone: 58 us for the 4 MB of the 16^3 level.)
template <typename T, int MC>
__global__ __launch_bounds__(256) void head_fwd_kernel(const T* __restrict__ in, int64_t in_pitch,
                                                       const float* __restrict__ scale, const float* __restrict__ shift,
                                                       const float* __restrict__ w, const float* __restrict__ b,
                                                       T* __restrict__ logits, int N, int C, int ncls, int64_t vox,
                                                       int per, int vec4) {
  HDF_LIGHT_PRIO();
  constexpr int EPC = ST<T>::EPC;
  extern __shared__ float outs[];  // [MC][per], then [256][MC] partials when cols is not a power of two
  float* part = outs + MC * per;
  const int n = blockIdx.y;
  const int cols = C / EPC;
  // shuffle reduction when a voxel's chunk lanes are a power of two within one wave; else (n_filters = 48: 6 chunk
  // lanes straddle waves; fp32 storage at 512 channels: 128 lanes per voxel) through LDS
  const bool pow2 = (cols & (cols - 1)) == 0 && cols <= 64;
  const int vlanes = 256 / cols;
  const int col = threadIdx.x % cols, vl = min((int)threadIdx.x / cols, vlanes - 1);
  const bool lane_on = (int)threadIdx.x < vlanes * cols;
  const int c0 = col * EPC;
  float sc[EPC], sh[EPC], wv[MC][EPC];
#pragma unroll
  for (int e = 0; e < EPC; e++) {
    sc[e] = scale ? scale[(int64_t)n * C + c0 + e] : 1.f;
    sh[e] = scale ? shift[(int64_t)n * C + c0 + e] : 0.f;
#pragma unroll
    for (int o = 0; o < MC; o++) wv[o][e] = (o < ncls) ? w[min(o, ncls - 1) * C + c0 + e] : 0.f;
  }
  const int64_t vb = (int64_t)blockIdx.x * per, ve = min(vox, vb + per);
  constexpr int U = 4;
  const int iters = (per + U * vlanes - 1) / (U * vlanes);  // the same for every thread: shuffles / barriers below
  for (int it = 0; it < iters; it++) {
    const int64_t v0 = vb + vl + (int64_t)it * U * vlanes;
    float f[U][EPC];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t v = min(v0 + (int64_t)u * vlanes, ve - 1);  // clamped: never branch around a load
      load_chunk<T>(in + ((int64_t)n * vox + v) * in_pitch + c0, f[u]);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      float acc[MC];
#pragma unroll
      for (int o = 0; o < MC; o++) acc[o] = 0.f;
#pragma unroll
      for (int e = 0; e < EPC; e++) {
        float x = f[u][e];
        if (scale) x = fmaxf(x * sc[e] + sh[e], 0.f);
#pragma unroll
        for (int o = 0; o < MC; o++) acc[o] += x * wv[o][e];
      }
      if (pow2) {
        for (int off = 1; off < cols; off <<= 1) {
#pragma unroll
          for (int o = 0; o < MC; o++) acc[o] += __shfl_xor(acc[o], off, 64);
        }
      } else {  // uniform branch and trip count: the barriers are reached by every thread
        __syncthreads();
#pragma unroll
        for (int o = 0; o < MC; o++) part[threadIdx.x * MC + o] = acc[o];
        __syncthreads();
        if (col == 0) {
          for (int k = 1; k < cols; k++)
#pragma unroll
            for (int o = 0; o < MC; o++) acc[o] += part[(threadIdx.x + k) * MC + o];
        }
      }
      const int64_t lv = v0 + (int64_t)u * vlanes - vb;
      if (col == 0 && lane_on && lv < per) {
#pragma unroll
        for (int o = 0; o < MC; o++) outs[o * per + (int)lv] = acc[o];
      }
    }
  }
  __syncthreads();
  for (int o = 0; o < ncls; o++) {
    const float bo = b[o];
    if (vec4) {  // four voxels of the class plane per store
      for (int lv = threadIdx.x * 4; lv < per; lv += 1024)
        if (vb + lv < vox)
          ST<T>::st4(logits + ((int64_t)n * ncls + o) * vox + vb + lv, outs[o * per + lv] + bo, outs[o * per + lv + 1] + bo,
                     outs[o * per + lv + 2] + bo, outs[o * per + lv + 3] + bo);
    } else {
      for (int lv = threadIdx.x; lv < per; lv += 256)
        if (vb + lv < vox) ST<T>::st(logits + ((int64_t)n * ncls + o) * vox + vb + lv, outs[o * per + lv] + bo);
    }
  }
}

// Streaming form: thread = (voxel lane, 8-channel chunk), so a wave reads whole contiguous voxel rows; the weight-
// gradient outer products accumulate in registers over the thread's voxels (ncls x 8 accumulators) and are reduced
// across the block ONCE at the end (the first version rebuilt a 256-voxel LDS tile and ran a 256-deep serial LDS
// reduction per tile: 3x the HBM time).  grid (blocks, N); C <= 256 (cols = C/8 <= 32).
constexpr int HEAD_VOX_MAX = 2048;  // voxels per workgroup (fewer at the low-resolution levels: see head_vox)
// voxels per workgroup: a multiple of 64; at least 128 (backward: every workgroup ends with a block reduction and 132
// atomics; 512 per sample was slower, 39.8 -> 49.4 us at 64^3) / 1024 (forward: with 128 per sample the 64^3 level ran
// one workgroup per CU at 1.7 TB/s) workgroups per sample when the level has that many 64-voxel groups
inline int head_vox(int64_t vox, int wgs = 128) {
  return (int)std::max<int64_t>(64, std::min<int64_t>(HEAD_VOX_MAX, (vox / wgs) & ~63));
}
// MC: class slots held in registers (4 or 8); ACC: dx += (else dx =).  FOUR channels per thread for every storage type
// (16-bit: 8-byte loads, two voxel rows in flight, <= 128 registers).  The 8-channel form for 16-bit storage needed 238
// registers: below the top level the head gradient runs next to a persistent weight-gradient kernel of the side stream
// (one wave per SIMD, 301-376 registers) and WAITED for that kernel to end (179 us instead of 58 at 64^3 in the r03c
// timeline); alone the light form is as fast at 128^3 (151 vs 159 us), slower at 64^3 (52 vs 38 us).
template <typename T, int MC, bool ACC>
__global__ __launch_bounds__(256, (MC == 4 && sizeof(T) == 2) ? 4 : 1) void head_bwd_kernel(const T* __restrict__ dlogits, const T* __restrict__ in,
                                                       int64_t in_pitch, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, const float* __restrict__ w,
                                                       T* __restrict__ dx, int64_t dx_pitch,
                                                       float* __restrict__ dw, float* __restrict__ db, int N, int C,
                                                       int ncls, int64_t vox, int per,
                                                       const float* __restrict__ in_mean,
                                                       const float* __restrict__ in_rstd,
                                                       float* __restrict__ inb_partials, int vec4) {
  HDF_LIGHT_PRIO();
  constexpr int EPC = 4;
  // inb_partials (optional): this kernel produces the complete gradient dx of the activation relu(IN(in)), so it
  // also writes the first pass of that InstanceNorm's backward -- per workgroup and channel (sum g, sum g*xhat) with
  // g = dx where the activation is positive, row layout of in_bwd_reduce4_kernel with gridDim.x rows per sample -- and
  // saves a full read of dx and in.  The sums use the STORED (storage-rounded) dx, as a separate pass would.
  // LDS: first the block's logit gradients [voxel][MC] (loaded class plane by class plane, coalesced, once), then
  // reused as [vlanes][C + 1][MC] for the final reduction
  extern __shared__ float red[];
  const int n = blockIdx.y;
  const int cols = C / EPC;
  const int vlanes = 256 / cols;
  const int col = threadIdx.x % cols, vl = threadIdx.x / cols;
  const int c0 = col * EPC;
  float sc[EPC], sh[EPC], wv[MC][EPC], accw[MC][EPC], accb[MC];
  float mu[EPC], rs[EPC], s1[EPC], s2[EPC];
#pragma unroll
  for (int e = 0; e < EPC; e++) {
    sc[e] = scale ? scale[(int64_t)n * C + c0 + e] : 1.f;
    sh[e] = scale ? shift[(int64_t)n * C + c0 + e] : 0.f;
    mu[e] = inb_partials ? in_mean[(int64_t)n * C + c0 + e] : 0.f;
    rs[e] = inb_partials ? in_rstd[(int64_t)n * C + c0 + e] : 0.f;
    s1[e] = s2[e] = 0.f;
  }
#pragma unroll
  for (int o = 0; o < MC; o++) {
    accb[o] = 0.f;
#pragma unroll
    for (int e = 0; e < EPC; e++) {
      wv[o][e] = (o < ncls) ? w[min(o, ncls - 1) * C + c0 + e] : 0.f;
      accw[o][e] = 0.f;
    }
  }
  const int64_t vb = (int64_t)blockIdx.x * per, ve = min(vox, vb + per);
  if (vec4) {  // four voxels of a class plane per load (the plane rows are aligned and whole: see the launcher)
    for (int i = threadIdx.x; i < MC * (per >> 2); i += 256) {
      const int o = i / (per >> 2), lv = (i - o * (per >> 2)) * 4;
      float v[4];
      ST<T>::ld4(dlogits + ((int64_t)n * ncls + min(o, ncls - 1)) * vox + min(vb + lv, vox - 4), v);
#pragma unroll
      for (int j = 0; j < 4; j++) red[(lv + j) * MC + o] = (o < ncls && vb + lv < vox) ? v[j] : 0.f;
    }
  } else {
    for (int o = 0; o < MC; o++) {
      const T* src = dlogits + ((int64_t)n * ncls + min(o, ncls - 1)) * vox;
      for (int lv = threadIdx.x; lv < per; lv += 256) {
        const float v = ST<T>::ld(src + min(vb + lv, vox - 1));
        red[lv * MC + o] = (o < ncls && vb + lv < vox) ? v : 0.f;
      }
    }
  }
  __syncthreads();
  if (vl < vlanes) {
    constexpr int U = sizeof(T) == 2 ? 2 : 4;  // 16-bit storage: 128 registers (four rows in flight for the top level's
                                               // launch, alone on the chip: 153 vs 141 us)
    for (int64_t v0 = vb + vl; v0 < ve; v0 += (int64_t)U * vlanes) {
      float f[U][EPC], g[ACC ? U : 1][EPC], dl[U][MC];
      int64_t row[U];
#pragma unroll
      for (int u = 0; u < U; u++) {  // clamped: never branch around a load; the tail is masked below
        const int64_t v = min(v0 + (int64_t)u * vlanes, ve - 1);
        row[u] = (int64_t)n * vox + v;
        ST<T>::ld4(in + row[u] * in_pitch + c0, f[u]);
        if (ACC) ST<T>::ld4(dx + row[u] * dx_pitch + c0, g[ACC ? u : 0]);
#pragma unroll
        for (int o = 0; o < MC; o++) dl[u][o] = red[(int)(v - vb) * MC + o];
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const bool live = v0 + (int64_t)u * vlanes < ve;
#pragma unroll
        for (int o = 0; o < MC; o++) dl[u][o] = live ? dl[u][o] : 0.f;
        float d[EPC];
#pragma unroll
        for (int e = 0; e < EPC; e++) {
          float x = f[u][e];
          if (scale) x = fmaxf(x * sc[e] + sh[e], 0.f);
          float t = ACC ? g[ACC ? u : 0][e] : 0.f;
#pragma unroll
          for (int o = 0; o < MC; o++) {
            t += dl[u][o] * wv[o][e];
            accw[o][e] += dl[u][o] * x;
          }
          // relu of the producing norm is handled by the IN backward of that layer (dx is d/d activation)
          d[e] = t;
        }
        if (live) ST<T>::st4(dx + row[u] * dx_pitch + c0, d[0], d[1], d[2], d[3]);
        if (inb_partials) {
#pragma unroll
          for (int e = 0; e < EPC; e++) {
            const float gg = (live && f[u][e] * sc[e] + sh[e] > 0.f) ? storage_round<T>(d[e]) : 0.f;
            s1[e] += gg;
            s2[e] += gg * ((f[u][e] - mu[e]) * rs[e]);
          }
        }
        if (col == 0) {
#pragma unroll
          for (int o = 0; o < MC; o++) accb[o] += dl[u][o];
        }
      }
    }
  }
  // ---- block reduction over the voxel lanes, then one atomic per (class, channel) and block
  __syncthreads();  // everybody is done with the logit gradients: the region is reused
  const int ld = (C + 1) * MC;
  if (vl < vlanes) {
#pragma unroll
    for (int o = 0; o < MC; o++) {
#pragma unroll
      for (int e = 0; e < EPC; e++) red[vl * ld + (c0 + e) * MC + o] = accw[o][e];
      if (col == 0) red[vl * ld + C * MC + o] = accb[o];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < (C + 1) * MC; i += 256) {
    const int c = i / MC, o = i - c * MC;
    if (o >= ncls) continue;
    float t = 0.f;
    for (int k = 0; k < vlanes; k++) t += red[k * ld + i];
    if (c < C)
      atomicAdd(dw + o * C + c, t);
    else
      atomicAdd(db + o, t);
  }
  if (inb_partials) {  // same fixed-order reduction over the voxel lanes as in_bwd_reduce4_kernel
    __syncthreads();
    if (vl < vlanes) {
#pragma unroll
      for (int e = 0; e < EPC; e++) {
        red[(vl * C + c0 + e) * 2 + 0] = s1[e];
        red[(vl * C + c0 + e) * 2 + 1] = s2[e];
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * 2; i += 256) {
      float t = 0.f;
      for (int k = 0; k < vlanes; k++) t += red[k * C * 2 + i];
      inb_partials[((int64_t)n * gridDim.x + blockIdx.x) * C * 2 + i] = t;
    }
  }
}

}  // namespace

// dynamic LDS above 64 KiB has to be allowed per kernel
static int allow_big_lds(const void* kern, size_t bytes) {
  if (bytes <= 64 * 1024) return HDF_OK;
  hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (e != hipSuccess) {
    hdf_set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed: %s", hipGetErrorString(e));
    return HDF_ERR_HIP;
  }
  return HDF_OK;
}

int hdf_launch_head_fwd(int dtype, CRows in, NormStats ins, const float* w, const float* b, void* logits, int N, int C,
                        int ncls, int64_t vox, hipStream_t st) {
  HDF_CHECK_ARG(ncls <= HEAD_MAXCLS, "head: n_cls=%d > %d", ncls, HEAD_MAXCLS);
  HDF_CHECK_ARG(C % 16 == 0 && C <= 1024, "head_fwd: C=%d", C);
  // >= 1024 workgroups per sample where that still leaves 256 voxels each (64^3: 42 -> 32 us), else the backward's rule
  // (64-voxel workgroups at 32^3 were slower: 28 vs 18.5 us)
  const int per = head_vox(vox, 1024) >= 256 ? head_vox(vox, 1024) : head_vox(vox);
  const unsigned gx = (unsigned)ceil_div64(vox, per);
  const int vec4 = (vox % 4 == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0) ? 1 : 0;
  HDF_DISPATCH_T(dtype, {
    // 8 class slots at per = 2048 (the 128^3 level) need 72 KiB of dynamic LDS: above 64 KiB it is allowed per kernel
    auto go = [&](auto kern, int mc) -> int {
      const size_t shm = (size_t)mc * (per + 256) * sizeof(float);
      HDF_TRY(allow_big_lds((const void*)kern, shm));
      hipLaunchKernelGGL(kern, dim3(gx, N), dim3(256), shm, st, (const T*)in.p, in.pitch, ins.scale, ins.shift, w, b,
                         (T*)logits, N, C, ncls, vox, per, vec4);
      return HDF_OK;
    };
    if (ncls <= 4)
      HDF_TRY(go(head_fwd_kernel<T, 4>, 4));
    else
      HDF_TRY(go(head_fwd_kernel<T, 8>, 8));
  });
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

// workgroups per sample of head_bwd_kernel (= rows per sample of its optional InstanceNorm-backward partials)
int hdf_head_bwd_blocks(int64_t vox) { return (int)ceil_div64(vox, head_vox(vox)); }

int hdf_launch_head_bwd(int dtype, const void* dlogits, CRows in, NormStats ins, const float* w, HeadGrads g, int N, int C,
                        int ncls, int64_t vox, hipStream_t st) {
  HDF_CHECK_ARG(ncls <= HEAD_MAXCLS, "head: n_cls=%d > %d", ncls, HEAD_MAXCLS);
  HDF_CHECK_ARG(C % 16 == 0 && C <= 1024, "head_bwd: C=%d", C);  // (C / 4 <= 256 chunk lanes)
  HDF_CHECK_ARG(g.inb_partials == nullptr || (ins.scale && ins.mean && ins.rstd),
                "head_bwd: IN partials need the layer's statistics");
  const int per = head_vox(vox);
  const unsigned gx = (unsigned)hdf_head_bwd_blocks(vox);
  // logit-gradient planes by 4-voxel loads: whole aligned groups (per is a multiple of 64)
  const int vec4 = (vox % 4 == 0 && (reinterpret_cast<uintptr_t>(dlogits) & 15) == 0) ? 1 : 0;
  HDF_DISPATCH_T(dtype, {
    const int cols = C / 4, vlanes = 256 / cols;
    const int mc = ncls <= 4 ? 4 : 8;
    const size_t shm =
        std::max(std::max((size_t)vlanes * (C + 1) * mc, (size_t)per * mc), (size_t)vlanes * C * 2) * sizeof(float);
    auto go = [&](auto kern) -> int {
      HDF_TRY(allow_big_lds((const void*)kern, shm));
      hipLaunchKernelGGL(kern, dim3(gx, N), dim3(256), shm, st, (const T*)dlogits, (const T*)in.p, in.pitch, ins.scale,
                         ins.shift, w, (T*)g.dx.p, g.dx.pitch, g.dw, g.db, N, C, ncls, vox, per, ins.mean, ins.rstd,
                         g.inb_partials, vec4);
      return HDF_OK;
    };
    if (mc == 4)
      HDF_TRY(g.accumulate_dx ? go(head_bwd_kernel<T, 4, true>) : go(head_bwd_kernel<T, 4, false>));
    else
      HDF_TRY(g.accumulate_dx ? go(head_bwd_kernel<T, 8, true>) : go(head_bwd_kernel<T, 8, false>));
  });
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
