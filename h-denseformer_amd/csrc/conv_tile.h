// Pieces shared by the convolution kernels: the MFMA wrapper per storage type, the generic halo-box staging (PITCH,
// stage_box), the MFMA-row -> tile-voxel map of the 4x8x8 tile family, the LDS-only workgroup barrier, the persistent
// kernels' tile record and schedule (conv_schedule.h, included here), the zero line of the LDS-DMA kernels and the phase
// stamps of a -DWS_DBG_STAMPS build.
// Users: conv_igemm.hip, conv_s2.hip and, through conv_wgrad_tile.h, conv_wgrad.hip (stage_box, Mma, WS_BARRIER),
// conv_wgrad2.hip (Mma, WS_BARRIER, WsTile, WsSchedule, the stamps) and conv_wgrad_s2.hip (Mma, WS_BARRIER, the zero line);
// conv_wr.hip (Mma, the row maps, WS_BARRIER, WsTile, WsSchedule, the zero line) and conv_first.hip (Mma, the row maps,
// WS_BARRIER, WsTile).
#pragma once
#include "conv_schedule.h"
#include "hdf_common.h"

namespace {

template <typename T>
struct Mma;
template <>
struct Mma<bf16_t> {
  static __device__ __forceinline__ void run(const u32x4& a, const u32x4& b, f32x16& c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
};
template <>
struct Mma<f16_t> {
  static __device__ __forceinline__ void run(const u32x4& a, const u32x4& b, f32x16& c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
};
template <>
struct Mma<float> {
  // lane (r, h) holds channels 4h..4h+3 of an 8-channel group: step s contracts channels {s, 4+s}
  static __device__ __forceinline__ void run(const u32x4& a, const u32x4& b, f32x16& c) {
#pragma unroll
    for (int s = 0; s < 4; s++)
      c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a[s]), __uint_as_float(b[s]), c, 0, 0, 0);
  }
};

constexpr int PITCH = 80;  // LDS bytes per voxel row: 64 payload + 16 pad

// Stage a box of voxels (channels [c0, c0 + chunk_elems)) of a pitched NDHWC tensor into LDS with the
// optional per-(n,channel) affine(+relu) transform.  Voxels outside the tensor and channels >= C
// become zeros (zero padding applies to the TRANSFORMED activation).
template <typename T, int BD, int BH, int BW, int ROWB /*payload bytes per row*/, int LPITCH>
__device__ __forceinline__ void stage_box(char* lds, const T* __restrict__ src, int64_t pitch, int C, int n, int D,
                                          int H, int W, int oz, int oy, int ox, int c0, int row_bytes,
                                          const float* __restrict__ scale, const float* __restrict__ shift, int relu) {
  constexpr int EPC = ST<T>::EPC;
  const int cpv = row_bytes >> 4;  // 16-B chunks per voxel row (power of two)
  const int cpv_shift = (cpv == 32) ? 5 : (cpv == 16) ? 4 : (cpv == 8) ? 3 : (cpv == 4) ? 2 : (cpv == 2) ? 1 : 0;
  const int total = (BD * BH * BW) << cpv_shift;
  const int part = threadIdx.x & (cpv - 1);  // constant per thread (256 % cpv == 0)
  const int cbase = c0 + part * EPC;
  float sc[EPC], sh[EPC];
  const bool xf = (scale != nullptr);
  if (xf) {
#pragma unroll
    for (int e = 0; e < EPC; e++) {
      bool ok = (cbase + e) < C;
      sc[e] = ok ? scale[(int64_t)n * C + cbase + e] : 0.f;
      sh[e] = ok ? shift[(int64_t)n * C + cbase + e] : 0.f;
    }
  }
  const bool chan_ok = cbase < C;  // C is a multiple of EPC
  // Batches of U chunks per thread: all U loads are issued back to back (UNCONDITIONAL, from a clamped address:
  // a per-element `if (ok) v = load` makes hipcc branch around every load and wait for each one in turn --
  // cdna_hip_programming.md, projection-GEMM trap (c)), then transformed and written to LDS.
  constexpr int U = 5;
  for (int id0 = threadIdx.x; id0 < total; id0 += 256 * U) {
    u32x4 v[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      int id = min(id0 + 256 * u, total - 1);
      int vox = id >> cpv_shift;
      int bz = vox / (BH * BW);
      int rem = vox - bz * (BH * BW);
      int by = rem / BW;
      int bx = rem - by * BW;
      int iz = oz + bz, iy = oy + by, ix = ox + bx;
      ok[u] = chan_ok && (unsigned)iz < (unsigned)D && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
      const T* p = ok[u] ? src + ((((int64_t)n * D + iz) * H + iy) * W + ix) * pitch + cbase : src;
      v[u] = *reinterpret_cast<const u32x4*>(p);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      int id = id0 + 256 * u;
      u32x4 w = v[u];
      if (xf) {
        float f[EPC];
        ST<T>::unpack(w, f);
#pragma unroll
        for (int e = 0; e < EPC; e++) {
          f[e] = f[e] * sc[e] + sh[e];
          if (relu) f[e] = fmaxf(f[e], 0.f);
        }
        w = ST<T>::pack(f);
      }
      if (!ok[u]) w = u32x4{0u, 0u, 0u, 0u};
      if (id < total) *reinterpret_cast<u32x4*>(lds + (id >> cpv_shift) * LPITCH + part * 16) = w;
    }
  }
}

// MFMA row (0..31) -> (dz in 0..3, x in 0..7).  ds_read_b128 services lanes {0-3,12-15,20-27} and {4-11,16-19,
// 28-31} (and the same +32) as groups; group 1 gets z in {0,2}, group 2 z in {1,3}: box row = 100*z + 10*y + x
// (BH = BW = 10) is then distinct mod 16 inside each group.
constexpr int WS_STAT_ROWS = 512;  // conv_ws2_kernel: InstanceNorm partial rows per sample (2 passes x 256 workgroup slots)
// (g2, rank): which of the two ds_read_b128 service groups MFMA row r (0..31) belongs to, and its position 0..15 there
__device__ __forceinline__ void ds128_group(int r, int& g2, int& rank) {
  g2 = ((r >= 4 && r < 12) || (r >= 16 && r < 20) || r >= 28) ? 1 : 0;
  rank = g2 ? (r < 12 ? r - 4 : (r < 20 ? r - 8 : r - 16)) : (r < 4 ? r : (r < 16 ? r - 8 : r - 12));
}
__device__ __forceinline__ void ws_row_to_zx(int r, int& dz, int& x) {
  int g2, rank;
  ds128_group(r, g2, rank);
  dz = 2 * (rank >> 3) + g2;
  x = rank & 7;
}

// workgroup barrier that orders LDS traffic only: unlike __syncthreads() it does not drain the vector-memory
// counter, so prefetch loads and epilogue stores stay in flight across it
#define WS_BARRIER()                                     \
  do {                                                   \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   \
    __builtin_amdgcn_s_barrier();                        \
    asm volatile("" ::: "memory");                       \
  } while (0)

// 16 zero bytes: the source of LDS-DMA slots that lie outside the tensor (zero padding)
__device__ __attribute__((aligned(16))) uint32_t g_zero_line[4] = {0u, 0u, 0u, 0u};

}  // namespace

// -DWS_DBG_STAMPS: shader-clock stamps per phase of a persistent kernel (conv_ws2_kernel, conv_wgrad2_kernel).  The kernel
// declares `unsigned long long tacc[8]` and `tlast`; WS2_STAMP(k) adds the cycles since the previous stamp to tacc[k].
#ifdef WS_DBG_STAMPS
#define WS2_STAMP(k)                                       \
  {                                                        \
    __builtin_amdgcn_sched_barrier(0);                     \
    unsigned long long t_ = __builtin_amdgcn_s_memtime();  \
    __builtin_amdgcn_s_waitcnt(0xC07F);                    \
    __builtin_amdgcn_sched_barrier(0);                     \
    tacc[k] += t_ - tlast;                                 \
    tlast = t_;                                            \
  }
#else
#define WS2_STAMP(k)
#endif
