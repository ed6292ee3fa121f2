// Layout conversion, pooling and resampling around the convolutions: MaxPool3d(2,2) fwd/bwd, the fused encoder tail
// (norm + ReLU + skip + pool, with or without the up-sampling inside), trilinear x2 fwd/bwd, and the pooling backward that
// takes the first pass of an InstanceNorm backward along.  2-D forms (FLAT) on depth-1 tensors.
//
// Reference semantics: HDenseFormer.py:168-175 (UpConv), :199-207 (MaxPool3d), :237-243; torch semantics restated in
// SURVEY.md appendix A items 7-9,18.
#include "unet_ops_internal.h"

namespace {

// ------------------------------------------------------------------------------ layout conversion
template <typename T>
__global__ void nchw_to_ndhwc_kernel(const float* __restrict__ x, T* __restrict__ out, int N, int C, int CP,
                                     int64_t vox) {
  HDF_LIGHT_PRIO();
  int64_t total = (int64_t)N * vox;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t n = i / vox, v = i - n * vox;
    for (int c0 = 0; c0 < CP; c0 += ST<T>::EPC) {
      float f[ST<T>::EPC];
#pragma unroll
      for (int e = 0; e < ST<T>::EPC; e++) f[e] = (c0 + e < C) ? x[(n * C + c0 + e) * vox + v] : 0.f;
      store_chunk<T>(out + i * CP + c0, f);
    }
  }
}

// ------------------------------------------------------------------------------ maxpool 2x2x2
template <typename T>
__global__ void maxpool_fwd_kernel(const T* __restrict__ in, int64_t in_pitch, T* __restrict__ out, int64_t out_pitch,
                                   uint8_t* __restrict__ idx, int N, int C, int Do, int Ho, int Wo) {
  constexpr int EPC = ST<T>::EPC;
  const int cols = C / EPC;
  const int Hi = Ho * 2, Wi = Wo * 2, Di = Do * 2;
  int64_t total = (int64_t)N * Do * Ho * Wo * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t row = i / cols;
    int c0 = (int)(i - row * cols) * EPC;
    int64_t t = row;
    int ow = t % Wo;
    t /= Wo;
    int oh = t % Ho;
    t /= Ho;
    int od = t % Do;
    int n = (int)(t / Do);
    float best[EPC];
    int bi[EPC];
#pragma unroll
    for (int e = 0; e < EPC; e++) {
      best[e] = -INFINITY;
      bi[e] = 0;
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {  // scan order d,h,w; strict > keeps the FIRST maximum (torch tie rule)
      int dz = k >> 2, dy = (k >> 1) & 1, dx = k & 1;
      int64_t irow = (((int64_t)n * Di + 2 * od + dz) * Hi + 2 * oh + dy) * Wi + 2 * ow + dx;
      float f[EPC];
      load_chunk<T>(in + irow * in_pitch + c0, f);
#pragma unroll
      for (int e = 0; e < EPC; e++) {
        if (f[e] > best[e] || f[e] != f[e]) {
          best[e] = f[e];
          bi[e] = k;
        }
      }
    }
    store_chunk<T>(out + row * out_pitch + c0, best);
    if constexpr (EPC == 8) {
      uint32_t lo = bi[0] | (bi[1] << 8) | (bi[2] << 16) | (bi[3] << 24);
      uint32_t hi = bi[4] | (bi[5] << 8) | (bi[6] << 16) | (bi[7] << 24);
      *reinterpret_cast<uint2*>(idx + row * C + c0) = make_uint2(lo, hi);
    } else {
      *reinterpret_cast<uint32_t*>(idx + row * C + c0) = bi[0] | (bi[1] << 8) | (bi[2] << 16) | (bi[3] << 24);
    }
  }
}

template <typename T>
__global__ void maxpool_bwd_kernel(const T* __restrict__ dout, int64_t dout_pitch, const uint8_t* __restrict__ idx,
                                   T* __restrict__ din, int64_t din_pitch, int N, int C, int Do, int Ho, int Wo,
                                   int accumulate) {
  constexpr int EPC = ST<T>::EPC;
  const int cols = C / EPC;
  const int Hi = Ho * 2, Wi = Wo * 2, Di = Do * 2;
  int64_t total = (int64_t)N * Do * Ho * Wo * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t row = i / cols;
    int c0 = (int)(i - row * cols) * EPC;
    int64_t t = row;
    int ow = t % Wo;
    t /= Wo;
    int oh = t % Ho;
    t /= Ho;
    int od = t % Do;
    int n = (int)(t / Do);
    float g[EPC];
    int bi[EPC];
    load_chunk<T>(dout + row * dout_pitch + c0, g);
    if constexpr (EPC == 8) {
      uint2 pk = *reinterpret_cast<const uint2*>(idx + row * C + c0);
#pragma unroll
      for (int e = 0; e < 4; e++) bi[e] = (pk.x >> (8 * e)) & 255, bi[4 + e] = (pk.y >> (8 * e)) & 255;
    } else {
      uint32_t pk = *reinterpret_cast<const uint32_t*>(idx + row * C + c0);
#pragma unroll
      for (int e = 0; e < 4; e++) bi[e] = (pk >> (8 * e)) & 255;
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
      int dz = k >> 2, dy = (k >> 1) & 1, dx = k & 1;
      int64_t irow = (((int64_t)n * Di + 2 * od + dz) * Hi + 2 * oh + dy) * Wi + 2 * ow + dx;
      T* p = din + irow * din_pitch + c0;
      float f[EPC];
      if (accumulate)
        load_chunk<T>(p, f);
      else {
#pragma unroll
        for (int e = 0; e < EPC; e++) f[e] = 0.f;
      }
#pragma unroll
      for (int e = 0; e < EPC; e++)
        if (bi[e] == k) f[e] += g[e];
      store_chunk<T>(p, f);
    }
  }
}

// ------------------------------------------------------------------------------ fused encoder tail
// ds = relu(y*s+t) + skip ;  pooled, idx = MaxPool3d(2)(ds)        (HDenseFormer.py:237-243)
// One thread owns a 2x2x2 block of ds voxels (one pooled voxel) x one 16-byte channel chunk, so ds is written
// once and never re-read for pooling.  (Round 1 also evaluated the trilinear x2 of up3's output inside this kernel so
// that at3 was never materialised; with the 27-loads-per-8-outputs upsample kernel reading the materialised tensor is
// 0.09 ms per step faster, and that variant -- VALU-bound with register spills -- was removed in round 3.)
// FLAT (round 6): the 2-D form (models/HDenseFormer_2D.py:232-240: MaxPool2d(2)) on depth-1 tensors -- a thread owns a
// 1x2x2 block, the depth axis is not pooled; window index k = 2 dy + dx as in the 3-D form with dz = 0.
template <typename T, bool FLAT = false>
__global__ __launch_bounds__(256, 2) void enc_tail_kernel(const T* __restrict__ y, int64_t y_pitch,
                                                          const float* __restrict__ scale,
                                                          const float* __restrict__ shift, const T* __restrict__ skip,
                                                          int64_t skip_pitch, T* __restrict__ ds,
                                                          int64_t ds_pitch, T* __restrict__ pooled,
                                                          int64_t pooled_pitch, uint8_t* __restrict__ idx, int N, int C,
                                                          int Do, int Ho, int Wo) {
  HDF_LIGHT_PRIO();
  constexpr int EPC = ST<T>::EPC;
  const int cols = C / EPC;
  const int Hi = 2 * Ho, Wi = 2 * Wo;
  const int64_t total = (int64_t)N * Do * Ho * Wo * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / cols;
    const int c0 = (int)(i - row * cols) * EPC;
    // (n, od) by one 64-bit division, the in-plane coordinates in 32 bits
    const int plane = Ho * Wo;
    const int64_t nz = row / plane;
    const int rem = (int)(row - nz * plane);
    const int oh = rem / Wo, ow = rem - oh * Wo;
    const int od = (int)(nz % Do), n = (int)(nz / Do);
    float sc[EPC], sh[EPC], best[EPC];
    int bi[EPC];
#pragma unroll
    for (int e = 0; e < EPC; e++) {
      sc[e] = scale[(int64_t)n * C + c0 + e];
      sh[e] = shift[(int64_t)n * C + c0 + e];
      best[e] = -INFINITY;
      bi[e] = 0;
    }
    // one output z plane (dz) of the 2x2x2 block: ds = relu(y*s+t) + skip, stored, and folded into the running
    // maximum in scan order d,h,w (strict > keeps the FIRST maximum: torch's tie rule)
    const int64_t row0 = (((int64_t)nz * (FLAT ? 1 : 2)) * Hi + 2 * oh) * Wi + 2 * ow;  // first voxel of the 2x2x2 block
    const T* const ybase = y + row0 * y_pitch + c0;
    T* const dbase = ds + row0 * ds_pitch + c0;
    auto finish_plane = [&](int dz, const float (&sk)[4][EPC]) __attribute__((always_inline)) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int dy = q >> 1, dx = q & 1, k = dz * 4 + q;
        const int64_t orow = ((int64_t)dz * Hi + dy) * Wi + dx;  // uniform
        float f[EPC];
        load_chunk<T>(ybase + orow * y_pitch, f);
#pragma unroll
        for (int e = 0; e < EPC; e++) f[e] = fmaxf(f[e] * sc[e] + sh[e], 0.f) + sk[q][e];
        store_chunk<T>(dbase + orow * ds_pitch, f);
        // pool over the STORED (storage-rounded) values so that backward/recompute sees the same maxima
        float g[EPC];
        ST<T>::unpack(ST<T>::pack(f), g);
#pragma unroll
        for (int e = 0; e < EPC; e++) {
          if (g[e] > best[e] || g[e] != g[e]) {
            best[e] = g[e];
            bi[e] = k;
          }
        }
      }
    };
#pragma unroll
    for (int dz = 0; dz < (FLAT ? 1 : 2); dz++) {
      float sk[4][EPC];
#pragma unroll
      for (int q = 0; q < 4; q++)
        load_chunk<T>(skip + (row0 + ((int64_t)dz * Hi + (q >> 1)) * Wi + (q & 1)) * skip_pitch + c0, sk[q]);
      finish_plane(dz, sk);
    }
    store_chunk<T>(pooled + row * pooled_pitch + c0, best);
    if constexpr (EPC == 8) {
      uint32_t lo = bi[0] | (bi[1] << 8) | (bi[2] << 16) | (bi[3] << 24);
      uint32_t hi = bi[4] | (bi[5] << 8) | (bi[6] << 16) | (bi[7] << 24);
      *reinterpret_cast<uint2*>(idx + row * C + c0) = make_uint2(lo, hi);
    } else {
      *reinterpret_cast<uint32_t*>(idx + row * C + c0) = bi[0] | (bi[1] << 8) | (bi[2] << 16) | (bi[3] << 24);
    }
  }
}

// ------------------------------------------------------------------------------ trilinear x2
// per dim, output o reads inputs (ia, wa), (ib, wb):  o=2i: (max(i-1,0), .25), (i, .75) ; o=2i+1: (i, .75), (min(i+1,n-1), .25)
__device__ __forceinline__ void up_taps(int o, int n, int& ia, float& wa, int& ib, float& wb) {
  int i = o >> 1;
  if (o & 1) {
    ia = i;
    wa = 0.75f;
    ib = min(i + 1, n - 1);
    wb = 0.25f;
  } else {
    ia = max(i - 1, 0);
    wa = 0.25f;
    ib = i;
    wb = 0.75f;
  }
}

// One thread per LOW-resolution voxel chunk: it produces the 2 x 2 x 2 block of outputs from the 3 x 3 x 3 input
// neighbourhood (27 loads and transforms per 8 outputs, separable interpolation plane by plane: x, then y, then z).  The
// first version gave every OUTPUT chunk its own 8 loads + 8 transforms (64 per block) and was VALU-bound: 204 us for the
// 268 MB of at3 (1.5 TB/s).  Edge voxels: the clamped neighbour index makes the .25 / .75 pair collapse onto the same
// voxel, which is torch's align_corners=False edge rule.
// FLAT (round 6): bilinear x2 of a depth-1 tensor (models/HDenseFormer_2D.py:166-170: F.interpolate(scale_factor=2,
// mode='bilinear', align_corners=False)): the y / x arithmetic of the 3-D form, the depth axis untouched.
template <typename T, bool FLAT = false>
__global__ __launch_bounds__(256) void upsample_fwd_kernel(const T* __restrict__ y, int64_t y_pitch,
                                                           const float* __restrict__ scale,
                                                           const float* __restrict__ shift, T* __restrict__ out,
                                                           int64_t out_pitch, int N, int C, int Di, int Hi, int Wi) {
  HDF_LIGHT_PRIO();
  constexpr int EPC = ST<T>::EPC;
  const int cols = C / EPC;
  const int Ho = 2 * Hi, Wo = 2 * Wi;
  const int64_t total = (int64_t)N * Di * Hi * Wi * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / cols;
    const int c0 = (int)(i - row * cols) * EPC;
    const int plane = Hi * Wi;
    const int64_t nz = row / plane;
    const int rem = (int)(row - nz * plane);
    const int ih = rem / Wi, iw = rem - ih * Wi;
    const int id = (int)(nz % Di), n = (int)(nz / Di);
    float sc[EPC], sh[EPC];
#pragma unroll
    for (int e = 0; e < EPC; e++) {
      sc[e] = scale[(int64_t)n * C + c0 + e];
      sh[e] = shift[(int64_t)n * C + c0 + e];
    }
    const int xs[3] = {max(iw - 1, 0), iw, min(iw + 1, Wi - 1)};
    const int ys[3] = {max(ih - 1, 0), ih, min(ih + 1, Hi - 1)};
    const int zs[3] = {max(id - 1, 0), id, min(id + 1, Di - 1)};
    const T* const lbase = y + (int64_t)n * Di * Hi * Wi * y_pitch + c0;
    const int lp = (int)y_pitch;
    // low-resolution plane a interpolated in y and x: P[dy][dx]
    auto plane_yx = [&](int a, float (&P)[4][EPC]) __attribute__((always_inline)) {
#pragma unroll
      for (int q = 0; q < 4; q++)
#pragma unroll
        for (int e = 0; e < EPC; e++) P[q][e] = 0.f;
#pragma unroll
      for (int b = 0; b < 3; b++) {
        float L[3][EPC];
#pragma unroll
        for (int c = 0; c < 3; c++) {
          float f[EPC];
          load_chunk<T>(lbase + ((int64_t)(zs[a] * Hi + ys[b]) * Wi + xs[c]) * lp, f);
#pragma unroll
          for (int e = 0; e < EPC; e++) L[c][e] = fmaxf(f[e] * sc[e] + sh[e], 0.f);
        }
        const float wy0 = (b == 0) ? 0.25f : (b == 1 ? 0.75f : 0.f);  // weight of row b for dy = 0
        const float wy1 = (b == 0) ? 0.f : (b == 1 ? 0.75f : 0.25f);   // ... for dy = 1
#pragma unroll
        for (int e = 0; e < EPC; e++) {
          const float x0 = 0.25f * L[0][e] + 0.75f * L[1][e], x1 = 0.75f * L[1][e] + 0.25f * L[2][e];
          P[0][e] += wy0 * x0, P[1][e] += wy0 * x1;
          P[2][e] += wy1 * x0, P[3][e] += wy1 * x1;
        }
      }
    };
    T* const obase = out + ((((int64_t)nz * (FLAT ? 1 : 2)) * Ho + 2 * ih) * Wo + 2 * iw) * out_pitch + c0;
    auto store_plane = [&](int dz, const float (&A)[4][EPC], float wa, const float (&B)[4][EPC], float wb)
        __attribute__((always_inline)) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        float f[EPC];
#pragma unroll
        for (int e = 0; e < EPC; e++) f[e] = wa * A[q][e] + wb * B[q][e];
        store_chunk<T>(obase + (((int64_t)dz * Ho + (q >> 1)) * Wo + (q & 1)) * out_pitch, f);
      }
    };
    float P0[4][EPC], P1[4][EPC];
    if constexpr (FLAT) {
      plane_yx(1, P1);                       // zs[1] = id: the tensor's one plane
      store_plane(0, P1, 1.f, P1, 0.f);
    } else {
      plane_yx(0, P0);
      plane_yx(1, P1);
      store_plane(0, P0, 0.25f, P1, 0.75f);
      plane_yx(2, P0);
      store_plane(1, P1, 0.75f, P0, 0.25f);
    }
  }
}

// ------------------------------------------------------------------------------ encoder tail with the up-sampling inside
// ds = relu(y*s+t) + trilinear_x2(relu(low*ls+lt)) ;  pooled, idx = MaxPool3d(2)(ds)     (HDenseFormer.py:168-175,237-243)
// enc_tail_kernel and upsample_fwd_kernel share their decomposition -- a thread owns one LOW-resolution voxel chunk, i.e.
// one 2 x 2 x 2 block of ds -- so the level-0 feature at3 = up3(...) need not exist in memory: this kernel interpolates
// the block from the 3 x 3 x 3 low-resolution neighbourhood (the same separable x, y, z arithmetic as
// upsample_fwd_kernel, plane by plane) and adds it in registers.  What it is for: at3's up-sampling (268 MB written at
// 128^3, batch 2: 103 us) was the LAST launch of the transformer / UpConv chain the caller's stream waits for in the
// forward (exec.hip: forward3d); with it here the wait ends at up3's InstanceNorm statistics, and this pass reads the
// 33 MB low-resolution tensor (L2-resident neighbours) instead of 268 MB.  The interpolated value is added in fp32
// (the materialised at3 was rounded to the storage type first).
// Registers: two interpolated planes (64 floats at 8 channels) + four norm vectors + the running maxima: one workgroup
// of 256 per SIMD set, no spills (the round-1 attempt at this fusion kept all eight interpolated chunks live and spilled).
template <typename T>
__global__ __launch_bounds__(256, 2) void enc_tail_up_kernel(const T* __restrict__ y, int64_t y_pitch,
                                                             const float* __restrict__ scale,
                                                             const float* __restrict__ shift, const T* __restrict__ low,
                                                             int64_t low_pitch, const float* __restrict__ lscale,
                                                             const float* __restrict__ lshift, T* __restrict__ ds,
                                                             int64_t ds_pitch, T* __restrict__ pooled,
                                                             int64_t pooled_pitch, uint8_t* __restrict__ idx, int N, int C,
                                                             int Do, int Ho, int Wo) {
  HDF_LIGHT_PRIO();
  constexpr int EPC = 4;  // four channels per thread (8-byte accesses in the 16-bit modes): two workgroups per SIMD set
  // grid (x tiles, oh, n * Do + od): the plane and row coordinates are uniform per workgroup, so every base address is
  // scalar arithmetic and a thread adds 32-bit offsets inside one row (the first version, a flat index with 64-bit
  // divisions and one 64-bit multiply per neighbour, spent a third of its vector cycles on addresses)
  const int cols = C / EPC;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= Wo * cols) return;
  const int ow = t / cols, c0 = (t - ow * cols) * EPC;
  const int oh = blockIdx.y;
  const int nz = blockIdx.z, n = nz / Do, od = nz - n * Do;
  const int Hi = 2 * Ho, Wi = 2 * Wo;
  const int yp = (int)y_pitch, dp = (int)ds_pitch, lp = (int)low_pitch;
  float sc[EPC], sh[EPC], lsc[EPC], lsh[EPC], best[EPC];
  int bi[EPC];
#pragma unroll
  for (int e = 0; e < EPC; e++) {
    sc[e] = scale[(int64_t)n * C + c0 + e];
    sh[e] = shift[(int64_t)n * C + c0 + e];
    lsc[e] = lscale[(int64_t)n * C + c0 + e];
    lsh[e] = lshift[(int64_t)n * C + c0 + e];
    best[e] = -INFINITY;
    bi[e] = 0;
  }
  // ---- the low-resolution neighbourhood (upsample_fwd_kernel's plane_yx, same order of operations)
  const int zs[3] = {max(od - 1, 0), od, min(od + 1, Do - 1)};
  const int ys[3] = {max(oh - 1, 0), oh, min(oh + 1, Ho - 1)};
  const int xo[3] = {max(ow - 1, 0) * lp + c0, ow * lp + c0, min(ow + 1, Wo - 1) * lp + c0};
  auto plane_yx = [&](int a, float (&P)[4][EPC]) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
      for (int e = 0; e < EPC; e++) P[q][e] = 0.f;
#pragma unroll
    for (int b = 0; b < 3; b++) {
      const T* const lrow = low + (((int64_t)n * Do + zs[a]) * Ho + ys[b]) * Wo * low_pitch;  // uniform
      float L[3][EPC];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        float f[EPC];
        ST<T>::ld4(lrow + xo[c], f);
#pragma unroll
        for (int e = 0; e < EPC; e++) L[c][e] = fmaxf(f[e] * lsc[e] + lsh[e], 0.f);
      }
      const float wy0 = (b == 0) ? 0.25f : (b == 1 ? 0.75f : 0.f);
      const float wy1 = (b == 0) ? 0.f : (b == 1 ? 0.75f : 0.25f);
#pragma unroll
      for (int e = 0; e < EPC; e++) {
        const float x0 = 0.25f * L[0][e] + 0.75f * L[1][e], x1 = 0.75f * L[1][e] + 0.25f * L[2][e];
        P[0][e] += wy0 * x0, P[1][e] += wy0 * x1;
        P[2][e] += wy1 * x0, P[3][e] += wy1 * x1;
      }
    }
  };
  // first voxel row of the workgroup's 2 x 2 x (2 Wo) slab (uniform) + this thread's x offset
  const int64_t slab = (((int64_t)nz * 2) * Hi + 2 * oh) * Wi;
  const T* const ybase = y + slab * y_pitch + 2 * ow * yp + c0;
  T* const dbase = ds + slab * ds_pitch + 2 * ow * dp + c0;
  // one output z plane of the block: ds = relu(y*s+t) + (wa A + wb B), stored, folded into the running maximum in scan
  // order d,h,w (strict > keeps the FIRST maximum: torch's tie rule; over the STORED values, as enc_tail_kernel)
  auto finish_plane = [&](int dz, const float (&A)[4][EPC], float wa, const float (&B)[4][EPC], float wb)
      __attribute__((always_inline)) {
    float yv[4][EPC];
#pragma unroll
    for (int q = 0; q < 4; q++) ST<T>::ld4(ybase + ((int64_t)(dz * Hi + (q >> 1)) * Wi) * y_pitch + (q & 1) * yp, yv[q]);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int k = dz * 4 + q;
      float f[EPC];
#pragma unroll
      for (int e = 0; e < EPC; e++) f[e] = fmaxf(yv[q][e] * sc[e] + sh[e], 0.f) + (wa * A[q][e] + wb * B[q][e]);
      ST<T>::st4(dbase + ((int64_t)(dz * Hi + (q >> 1)) * Wi) * ds_pitch + (q & 1) * dp, f[0], f[1], f[2], f[3]);
      float g[EPC];
#pragma unroll
      for (int e = 0; e < EPC; e++) {
        T tmp;
        ST<T>::st(&tmp, f[e]);
        g[e] = ST<T>::ld(&tmp);
      }
#pragma unroll
      for (int e = 0; e < EPC; e++) {
        if (g[e] > best[e] || g[e] != g[e]) {
          best[e] = g[e];
          bi[e] = k;
        }
      }
    }
  };
  float P0[4][EPC], P1[4][EPC];
  plane_yx(0, P0);
  plane_yx(1, P1);
  finish_plane(0, P0, 0.25f, P1, 0.75f);
  plane_yx(2, P0);
  finish_plane(1, P1, 0.75f, P0, 0.25f);
  const int64_t prow = ((int64_t)nz * Ho + oh) * Wo + ow;
  ST<T>::st4(pooled + prow * pooled_pitch + c0, best[0], best[1], best[2], best[3]);
  *reinterpret_cast<uint32_t*>(idx + prow * C + c0) = bi[0] | (bi[1] << 8) | (bi[2] << 16) | (bi[3] << 24);
}

// input i receives from outputs 2i-1 (.25, i>=1), 2i (.75 [+.25 at i==0]), 2i+1 (.75 [+.25 at i==n-1]), 2i+2 (.25, i<=n-2)
__device__ __forceinline__ void up_bwd_taps(int i, int n, int* o, float* w) {
  o[0] = 2 * i - 1;
  w[0] = (i >= 1) ? 0.25f : 0.f;
  o[1] = 2 * i;
  w[1] = (i == 0) ? 1.0f : 0.75f;
  o[2] = 2 * i + 1;
  w[2] = (i == n - 1) ? 1.0f : 0.75f;
  o[3] = 2 * i + 2;
  w[3] = (i <= n - 2) ? 0.25f : 0.f;
  if (i < 1) o[0] = 0;
  if (i > n - 2) o[3] = 2 * n - 1;
}

// XCD-aware workgroup order.  The dispatcher deals consecutive workgroup ids round-robin to the 8 XCDs, each with its own
// L2: with tiles in raster order, a tile's neighbours in y and z -- which share its halo -- run on OTHER XCDs and every
// halo row is fetched from the fabric once per XCD that touches it.  logical tile = xcd * (W / 8) + id / 8 gives every
// XCD one contiguous range of the raster instead (W a multiple of 8; else the identity).
__device__ __forceinline__ int xcd_slab_id(int L, int W) { return (W & 7) ? L : (L & 7) * (W >> 3) + (L >> 3); }

// One thread per low-resolution voxel chunk: 4 x 4 x 4 output taps.  Grid = x tiles * Hi * (N * Di) workgroups, one
// low-resolution row segment each: plane and row are uniform per workgroup (scalar address arithmetic; the flat-index
// version decoded its coordinates with 64-bit divisions), and the XCD slab order above keeps the 16 output rows a
// workgroup reads in the L2 that read them for the previous row (the raster order fetched 1.1 GB per step for 0.35 GB of
// operands: three XCDs per output row).
template <typename T, bool FLAT = false>   // FLAT: the adjoint of the bilinear x2 of a depth-1 tensor (4 x 4 taps)
__global__ __launch_bounds__(256) void upsample_bwd_kernel(const T* __restrict__ dout, int64_t dout_pitch,
                                                           T* __restrict__ din, int64_t din_pitch, int N, int C, int Di,
                                                           int Hi, int Wi, int gx) {
  HDF_LIGHT_PRIO();
  constexpr int EPC = ST<T>::EPC;
  const int cols = C / EPC;
  const int Ho = 2 * Hi, Wo = 2 * Wi;
  const int vb = xcd_slab_id(blockIdx.x, gridDim.x);
  const int xt = vb % gx, r = vb / gx;
  const int ih = r % Hi, nz = r / Hi;
  const int id = nz % Di, n = nz / Di;
  const int t = xt * 256 + threadIdx.x;
  if (t >= Wi * cols) return;
  const int iw = t / cols, c0 = (t - iw * cols) * EPC;
  int oz[4], oy[4], ox[4];
  float wz[4], wy[4], wx[4];
  if constexpr (FLAT) {
#pragma unroll
    for (int q = 0; q < 4; q++) oz[q] = 0, wz[q] = q == 0 ? 1.f : 0.f;
  } else {
    up_bwd_taps(id, Di, oz, wz);
  }
  up_bwd_taps(ih, Hi, oy, wy);
  up_bwd_taps(iw, Wi, ox, wx);
  float acc[EPC];
#pragma unroll
  for (int e = 0; e < EPC; e++) acc[e] = 0.f;
  // all 64 taps unconditionally (indices are clamped into range, out-of-range taps carry weight 0): no branch around
  // any load, so the loads of a thread are all in flight together.  Addresses: one 64-bit sample base, 32-bit element
  // offsets z + y (uniform) + x (the launcher checks that a sample fits 2^31 elements)
  const T* const sbase = dout + (int64_t)n * ((FLAT ? 1 : 2) * Di) * Ho * Wo * dout_pitch + c0;
  const int pit = (int)dout_pitch;
  int zo[4], yo[4], xo[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    zo[q] = oz[q] * Ho * Wo * pit;
    yo[q] = oy[q] * Wo * pit;
    xo[q] = ox[q] * pit;
  }
#pragma unroll
  for (int a = 0; a < (FLAT ? 1 : 4); a++) {
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const float wzy = wz[a] * wy[b];
      const int zy = zo[a] + yo[b];
      float f[4][EPC];
#pragma unroll
      for (int c = 0; c < 4; c++) load_chunk<T>(sbase + (zy + xo[c]), f[c]);
#pragma unroll
      for (int c = 0; c < 4; c++)
#pragma unroll
        for (int e = 0; e < EPC; e++) acc[e] += (wzy * wx[c]) * f[c][e];
    }
  }
  store_chunk<T>(din + (((int64_t)nz * Hi + ih) * Wi + iw) * din_pitch + c0, acc);
}

}  // namespace

int hdf_launch_nchw_to_ndhwc(int dtype, const float* x, void* out, int N, int C, int CP, int64_t vox, hipStream_t st) {
  HDF_CHECK_ARG(CP % 16 == 0 && CP >= C, "nchw_to_ndhwc: CP=%d", CP);
  HDF_DISPATCH_T(dtype, hipLaunchKernelGGL(nchw_to_ndhwc_kernel<T>, dim3(grid_for((int64_t)N * vox)), dim3(256), 0, st, x,
                                       (T*)out, N, C, CP, vox));
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_enc_tail(int dtype, CRows y, NormStats ys, CRows skip, Rows ds, Rows pooled, uint8_t* idx, Extent x,
                        hipStream_t st) {
  HDF_CHECK_ARG(x.C % 16 == 0, "enc_tail: C=%d", x.C);
  HDF_CHECK_ARG(!x.flat || x.D == 1, "enc_tail: the 2-D form takes depth-1 tensors");
  // (a form with the two x neighbours of a pooled voxel on neighbouring lanes -- whole contiguous rows per instruction, the
  // partial maxima merged through one lane exchange -- was built and measured: 163 vs 155 us at 128^3; this form already
  // streams at 5.5 TB/s alone, the 206 us it shows inside a step come from what runs around it)
  HDF_DISPATCH_T(dtype, {
    unsigned g = grid_for((int64_t)x.N * x.D * x.H * x.W * (x.C / ST<T>::EPC));
    auto kern = x.flat ? enc_tail_kernel<T, true> : enc_tail_kernel<T, false>;
    hipLaunchKernelGGL(kern, dim3(g), dim3(256), 0, st, (const T*)y.p, y.pitch, ys.scale, ys.shift, (const T*)skip.p,
                       skip.pitch, (T*)ds.p, ds.pitch, (T*)pooled.p, pooled.pitch, idx, x.N, x.C, x.D, x.H, x.W);
  });
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_enc_tail_up(int dtype, CRows y, NormStats ys, CRows low, NormStats ls, Rows ds, Rows pooled, uint8_t* idx,
                           Extent x, hipStream_t st) {
  HDF_CHECK_ARG(x.C % 16 == 0, "enc_tail_up: C=%d", x.C);
  HDF_DISPATCH_T(dtype, {
    HDF_CHECK_ARG(x.H <= 65535 && (int64_t)x.N * x.D <= 65535, "enc_tail_up: extent %d x %d x %d", x.D, x.H, x.W);
    hipLaunchKernelGGL((enc_tail_up_kernel<T>), dim3(ceil_div(x.W * (x.C / 4), 256), x.H, x.N * x.D), dim3(256), 0, st,
                       (const T*)y.p, y.pitch, ys.scale, ys.shift, (const T*)low.p, low.pitch, ls.scale, ls.shift, (T*)ds.p,
                       ds.pitch, (T*)pooled.p, pooled.pitch, idx, x.N, x.C, x.D, x.H, x.W);
  });
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_maxpool_fwd(int dtype, CRows in, Rows out, uint8_t* idx, Extent x, hipStream_t st) {
  HDF_CHECK_ARG(x.C % 16 == 0, "maxpool: C=%d", x.C);
  HDF_DISPATCH_T(dtype,
             hipLaunchKernelGGL(maxpool_fwd_kernel<T>, dim3(grid_for((int64_t)x.N * x.D * x.H * x.W * (x.C / ST<T>::EPC))),
                                dim3(256), 0, st, (const T*)in.p, in.pitch, (T*)out.p, out.pitch, idx, x.N, x.C, x.D, x.H,
                                x.W));
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

// MaxPool3d(2) backward, accumulating into din, for the encoder levels: din (= the gradient of ds_k = relu(IN(y)) + at_k)
// is COMPLETE once the pooled branch's gradient has been added, so the pass that adds it also takes the first pass of that
// layer's InstanceNorm(+ReLU) backward -- per workgroup and channel (sum g, sum g * xhat) with g = the STORED din where
// relu(IN(y)) is positive, rows of in_bwd_reduce4_kernel's layout with gridDim.x rows per sample -- and saves that pass its
// read of din (one of its two tensors; y is read here instead).  grid (blocks, N); thread = (pooled-voxel lane, 4 channels).
// FLAT (round 6): MaxPool2d(2) windows (1x2x2) of a depth-1 tensor, window index k = 2 dy + dx.
template <typename T, bool FLAT = false>
__global__ __launch_bounds__(256, 4) void maxpool_bwd_inb_kernel(const T* __restrict__ dout, int64_t dout_pitch,
                                                                 const uint8_t* __restrict__ idx, T* __restrict__ din,
                                                                 int64_t din_pitch, const T* __restrict__ y,
                                                                 int64_t y_pitch, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift,
                                                                 const float* __restrict__ mean,
                                                                 const float* __restrict__ rstd,
                                                                 float* __restrict__ partials, int C, int Do, int Ho,
                                                                 int Wo) {
  HDF_LIGHT_PRIO();
  extern __shared__ float red[];  // [vlanes][C][2]
  const int n = blockIdx.y, blocks = gridDim.x;
  const int cols = C >> 2, vlanes = 256 / cols;
  const int col = threadIdx.x % cols, vl = threadIdx.x / cols, c0 = col * 4;
  const int Hi = 2 * Ho, Wi = 2 * Wo;
  const int pvox = Do * Ho * Wo;
  float sc[4], sh[4], mu[4], rs[4], s1[4], s2[4];
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const int64_t o = (int64_t)n * C + c0 + e;
    sc[e] = scale[o], sh[e] = shift[o], mu[e] = mean[o], rs[e] = rstd[o];
    s1[e] = s2[e] = 0.f;
  }
  if (vl < vlanes) {
    const int per = (pvox + blocks - 1) / blocks;
    const int vb = blockIdx.x * per, ve = min(pvox, vb + per);
    for (int v = vb + vl; v < ve; v += vlanes) {
      const int ow = v % Wo, oh = (v / Wo) % Ho, od = v / (Wo * Ho);
      const int64_t prow = (int64_t)n * pvox + v;
      float g[4];
      ST<T>::ld4(dout + prow * dout_pitch + c0, g);
      const uint32_t pk = *reinterpret_cast<const uint32_t*>(idx + prow * C + c0);
      constexpr int NZ = FLAT ? 1 : 2;
      const int64_t row0 = (((int64_t)n * NZ * Do + NZ * od) * Hi + 2 * oh) * Wi + 2 * ow;
      // both z planes of the 2x2x2 block: 16 loads in flight per thread (one plane at a time, 8 loads: 203 vs 177 us at 128^3)
      float f[NZ][4][4], yv[NZ][4][4];
#pragma unroll
      for (int half = 0; half < NZ; half++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int64_t irow = row0 + ((int64_t)half * Hi + (q >> 1)) * Wi + (q & 1);
          ST<T>::ld4(din + irow * din_pitch + c0, f[half][q]);
          ST<T>::ld4(y + irow * y_pitch + c0, yv[half][q]);
        }
#pragma unroll
      for (int half = 0; half < NZ; half++) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int k = half * 4 + q;
          const int64_t irow = row0 + ((int64_t)half * Hi + (q >> 1)) * Wi + (q & 1);
#pragma unroll
          for (int e = 0; e < 4; e++)
            if ((int)((pk >> (8 * e)) & 255u) == k) f[half][q][e] += g[e];
          ST<T>::st4(din + irow * din_pitch + c0, f[half][q][0], f[half][q][1], f[half][q][2], f[half][q][3]);
#pragma unroll
          for (int e = 0; e < 4; e++) {
            const float gg = (yv[half][q][e] * sc[e] + sh[e] > 0.f) ? storage_round<T>(f[half][q][e]) : 0.f;
            s1[e] += gg;
            s2[e] += gg * ((yv[half][q][e] - mu[e]) * rs[e]);
          }
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

// rows per sample of the partials maxpool_bwd_inb_kernel writes: ~256 pooled voxels x chunk lanes per workgroup, <= 1024
int hdf_maxpool_bwd_in_blocks(int64_t pooled_vox, int C) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(1024, pooled_vox * (C / 4) / 2048));
}

int hdf_launch_maxpool_bwd_in(int dtype, CRows dout, const uint8_t* idx, Rows din, CRows y, NormStats ys, float* partials,
                              Extent x, hipStream_t st) {
  HDF_CHECK_ARG(x.C % 16 == 0 && x.C <= 1024, "maxpool_bwd_in: C=%d", x.C);
  HDF_CHECK_ARG((int64_t)x.D * x.H * x.W < ((int64_t)1 << 28), "maxpool_bwd_in: %dx%dx%d pooled voxels per sample", x.D, x.H,
                x.W);
  const int blocks = hdf_maxpool_bwd_in_blocks((int64_t)x.D * x.H * x.W, x.C);
  const int vlanes = 256 / (x.C / 4);
  HDF_DISPATCH_T(dtype, {
    auto kern = x.flat ? maxpool_bwd_inb_kernel<T, true> : maxpool_bwd_inb_kernel<T, false>;
    hipLaunchKernelGGL(kern, dim3(blocks, x.N), dim3(256), (size_t)vlanes * x.C * 2 * sizeof(float), st, (const T*)dout.p,
                       dout.pitch, idx, (T*)din.p, din.pitch, (const T*)y.p, y.pitch, ys.scale, ys.shift, ys.mean, ys.rstd,
                       partials, x.C, x.D, x.H, x.W);
  });
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_maxpool_bwd(int dtype, CRows dout, const uint8_t* idx, Rows din, Extent x, int accumulate, hipStream_t st) {
  HDF_DISPATCH_T(dtype, hipLaunchKernelGGL(maxpool_bwd_kernel<T>,
                                       dim3(grid_for((int64_t)x.N * x.D * x.H * x.W * (x.C / ST<T>::EPC))), dim3(256), 0, st,
                                       (const T*)dout.p, dout.pitch, idx, (T*)din.p, din.pitch, x.N, x.C, x.D, x.H, x.W,
                                       accumulate));
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_upsample_fwd(int dtype, CRows y, NormStats ys, Rows out, Extent x, hipStream_t st) {
  HDF_CHECK_ARG(x.C % 16 == 0, "upsample: C=%d", x.C);
  HDF_CHECK_ARG(ys.scale && ys.shift, "upsample_fwd: the producer's InstanceNorm scale / shift are required");
  HDF_CHECK_ARG(!x.flat || x.D == 1, "upsample_fwd: the 2-D form takes depth-1 tensors");
  HDF_DISPATCH_T(dtype, {
    auto kern = x.flat ? upsample_fwd_kernel<T, true> : upsample_fwd_kernel<T, false>;
    hipLaunchKernelGGL(kern, dim3(grid_for((int64_t)x.N * x.D * x.H * x.W * (x.C / ST<T>::EPC))), dim3(256), 0, st,
                       (const T*)y.p, y.pitch, ys.scale, ys.shift, (T*)out.p, out.pitch, x.N, x.C, x.D, x.H, x.W);
  });
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_upsample_bwd(int dtype, CRows dout, Rows din, Extent x, hipStream_t st) {
  HDF_CHECK_ARG(!x.flat || x.D == 1, "upsample_bwd: the 2-D form takes depth-1 tensors");
  HDF_CHECK_ARG((int64_t)8 * x.D * x.H * x.W * dout.pitch < ((int64_t)1 << 31),
                "upsample_bwd: a sample of %dx%dx%d voxels x pitch %lld exceeds 32-bit element offsets", 2 * x.D, 2 * x.H,
                2 * x.W, (long long)dout.pitch);
  HDF_DISPATCH_T(dtype, {
    const int gx = ceil_div(x.W * (x.C / ST<T>::EPC), 256);
    const int64_t wgs = (int64_t)gx * x.H * x.N * x.D;
    HDF_CHECK_ARG(wgs < ((int64_t)1 << 31), "upsample_bwd: %lld workgroups", (long long)wgs);
    auto kern = x.flat ? upsample_bwd_kernel<T, true> : upsample_bwd_kernel<T, false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)wgs), dim3(256), 0, st, (const T*)dout.p, dout.pitch, (T*)din.p, din.pitch, x.N,
                       x.C, x.D, x.H, x.W, gx);
  });
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
