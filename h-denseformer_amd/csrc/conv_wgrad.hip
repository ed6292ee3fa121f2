// Weight gradients of the 3x3x3 convolution family:  D[tap][sc][lc] = sum_{n,i} S[n,i][sc] * L[n, STRIDE*i-1+tap][lc]
//   conv_wgrad_kernel     every storage type, stride 1 and 2, 3-D and FLAT (the 2-D operators)
//   conv_wgrad2_kernel    16-bit stride 1: persistent, double-buffered tiles, optional fused InstanceNorm(+ReLU) backward
//   conv_wgrad_s2_kernel  16-bit stride 2 (ConvTranspose3d): LDS-DMA double-buffered
// Every kernel leaves fp32 partial slabs [G][27][SCp][LCp]; wgrad_reduce_kernel / wgrad_reduce_rows_kernel sum them in a fixed
// order into the torch layout.
#include "conv_igemm.h"
#include "conv_tile.h"
#include <type_traits>

namespace {

// weight gradient:  D[tap][sc][lc] = sum_{n,i} S[n,i][sc] * L[n, STRIDE*i-1+tap][lc]
// bf16: both operands are contracted over VOXELS, which are the slow axis of the channels-last LDS
// rows -> read with ds_read_b64_tr_b16 (hardware transpose, 4 voxels x 16 channels per 16 lanes).
// f32: v_mfma_f32_32x32x2_f32 takes one scalar per lane, plain ds_read_b32.
template <typename T>
struct WG;
template <>
struct WG<bf16_t> {
  static constexpr int KV = 16;  // voxels contracted per MFMA step
};
template <>
struct WG<f16_t> {
  static constexpr int KV = 16;
};
template <>
struct WG<float> {
  static constexpr int KV = 2;
};

// FLAT (round 6): the 2-D weight gradients of models/HDenseFormer_2D.py (Conv2d, ConvTranspose2d) on depth-1 tensors: the 9
// taps of the centre depth plane (three per wave, the fourth wave only stages), a one-plane box of the large operand, a
// depth axis that is never strided; the other 18 taps of the [27] slab are written as zeros.
template <typename T, int TD, int TH, int TW, int S, bool FLAT = false>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(WgradArgs a) {
  static_assert(!FLAT || TD == 1, "flat tiles are one voxel deep");
  constexpr int MT = TD * TH * TW;
  constexpr int BD = FLAT ? 1 : S * (TD - 1) + 3, BH = S * (TH - 1) + 3, BW = S * (TW - 1) + 3;
  constexpr int NTAP = FLAT ? 9 : 27, TAP0 = FLAT ? 9 : 0, ZO = FLAT ? 0 : 1;   // taps, first tap of the slab, z halo
  constexpr int ROWB = 32 * sizeof(T);  // 32 channels per LDS row
  // LDS row pitch.  bf16 transposed reads touch 4 voxel rows x 16 dwords per half-wave: with stride 2 those rows are
  // 2 box rows apart, and a 96-byte pitch (24 dwords: 0, 48, 32, 16 mod 64) tiles the 64 banks exactly; 80 bytes
  // overlapped the 1st and 4th row (2-way conflicts).  (Stride 1 bf16 runs conv_wgrad2_kernel with 64-byte rows.)
  constexpr int LP = (sizeof(T) == 2 && S == 2) ? ROWB + 32 : ROWB + 16;
  constexpr int TAPS_PER_WAVE = FLAT ? 3 : 7;
  __shared__ __attribute__((aligned(16))) char lds[(MT + BD * BH * BW) * LP];
  char* s_lds = lds;
  char* l_lds = lds + MT * LP;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int scb = blockIdx.y, lcb = blockIdx.z;
  const int ntz = (a.Ds + TD - 1) / TD, nty = (a.Hs + TH - 1) / TH, ntx = (a.Ws + TW - 1) / TW;

  f32x16 acc[TAPS_PER_WAVE];
#pragma unroll
  for (int j = 0; j < TAPS_PER_WAVE; j++)
#pragma unroll
    for (int i = 0; i < 16; i++) acc[j][i] = 0.f;

  int tapoff[TAPS_PER_WAVE];
#pragma unroll
  for (int j = 0; j < TAPS_PER_WAVE; j++) {
    int tap = wave * TAPS_PER_WAVE + j;
    if (tap >= NTAP) tap = 0;  // dummy slot of the last wave (never stored)
    int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
    tapoff[j] = ((kz * BH + ky) * BW + kx) * LP;
  }
  const int ntaps_here = max(0, min(TAPS_PER_WAVE, NTAP - wave * TAPS_PER_WAVE));  // 7,7,7,6 (flat: 3,3,3,0)

  const int t_begin = blockIdx.x * a.tiles_per_group;
  const int t_end = min(a.num_tiles, t_begin + a.tiles_per_group);
  auto tile_origin = [&](int tile, int& n, int& z0, int& y0, int& x0) {
    int t = tile;
    x0 = (t % ntx) * TW;
    t /= ntx;
    y0 = (t % nty) * TH;
    t /= nty;
    z0 = (t % ntz) * TD;
    n = t / ntz;
  };

  if constexpr (sizeof(T) == 2) {
    // ---- bf16: register-prefetched tiles (the next tile's global loads fly during this tile's MFMAs) ----------
    constexpr int CPV = ROWB / 16;                       // 4 chunks of 16 B per voxel row
    constexpr int BOXL = BD * BH * BW;
    constexpr int NS_ = (MT * CPV + 255) / 256, NL_ = (BOXL * CPV + 255) / 256;
    constexpr int EPC = ST<T>::EPC;
    const int part = threadIdx.x & (CPV - 1);
    u32x4 ps[NS_], pl[NL_];
    uint32_t vs = 0, vl = 0;
    auto prefetch = [&](int tile) {
      int n, z0, y0, x0;
      tile_origin(tile, n, z0, y0, x0);
      const T* ssrc = reinterpret_cast<const T*>(a.sm) + scb * 32 + part * EPC;
      const T* lsrc = reinterpret_cast<const T*>(a.lg) + lcb * 32 + part * EPC;
      const bool sc_ok = scb * 32 + part * EPC < a.SC, lc_ok = lcb * 32 + part * EPC < a.LC;
      vs = vl = 0;
#pragma unroll
      for (int j = 0; j < NS_; j++) {
        int vox = min((int)threadIdx.x + 256 * j, MT * CPV - 1) / CPV;
        int bz = vox / (TH * TW), rem = vox - bz * (TH * TW), by = rem / TW, bx = rem - by * TW;
        int iz = z0 + bz, iy = y0 + by, ix = x0 + bx;
        bool ok = sc_ok && iz < a.Ds && iy < a.Hs && ix < a.Ws;
        const T* p = ok ? ssrc + ((((int64_t)n * a.Ds + iz) * a.Hs + iy) * a.Ws + ix) * a.sm_pitch : ssrc - part * EPC - scb * 32;
        ps[j] = *reinterpret_cast<const u32x4*>(p);
        vs |= (ok ? 1u : 0u) << j;
      }
#pragma unroll
      for (int j = 0; j < NL_; j++) {
        int vox = min((int)threadIdx.x + 256 * j, BOXL * CPV - 1) / CPV;
        int bz = vox / (BH * BW), rem = vox - bz * (BH * BW), by = rem / BW, bx = rem - by * BW;
        int iz = (FLAT ? z0 : S * z0 - ZO) + bz, iy = S * y0 - 1 + by, ix = S * x0 - 1 + bx;
        bool ok = lc_ok && (unsigned)iz < (unsigned)a.Dl && (unsigned)iy < (unsigned)a.Hl && (unsigned)ix < (unsigned)a.Wl;
        const T* p = ok ? lsrc + ((((int64_t)n * a.Dl + iz) * a.Hl + iy) * a.Wl + ix) * a.lg_pitch : lsrc - part * EPC - lcb * 32;
        pl[j] = *reinterpret_cast<const u32x4*>(p);
        vl |= (ok ? 1u : 0u) << j;
      }
    };
    auto xform = [&](u32x4 v, const float* sc, const float* sh, int relu) {
      float f[EPC];
      ST<T>::unpack(v, f);
#pragma unroll
      for (int e = 0; e < EPC; e++) {
        f[e] = f[e] * sc[e] + sh[e];
        if (relu) f[e] = fmaxf(f[e], 0.f);
      }
      return ST<T>::pack(f);
    };
    auto commit = [&](int tile) {
      int n, z0, y0, x0;
      tile_origin(tile, n, z0, y0, x0);
      float sc[EPC], sh[EPC];
      if (a.sm_scale) {
#pragma unroll
        for (int e = 0; e < EPC; e++) {
          int c = min(scb * 32 + part * EPC + e, a.SC - 1);
          sc[e] = a.sm_scale[(int64_t)n * a.SC + c];
          sh[e] = a.sm_shift[(int64_t)n * a.SC + c];
        }
      }
#pragma unroll
      for (int j = 0; j < NS_; j++) {
        int id = threadIdx.x + 256 * j;
        if (id < MT * CPV) {
          u32x4 v = ps[j];
          if (a.sm_scale) v = xform(v, sc, sh, a.sm_relu);
          if (!((vs >> j) & 1u)) v = u32x4{0u, 0u, 0u, 0u};
          *reinterpret_cast<u32x4*>(s_lds + (id / CPV) * LP + part * 16) = v;
        }
      }
      if (a.lg_scale) {
#pragma unroll
        for (int e = 0; e < EPC; e++) {
          int c = min(lcb * 32 + part * EPC + e, a.LC - 1);
          sc[e] = a.lg_scale[(int64_t)n * a.LC + c];
          sh[e] = a.lg_shift[(int64_t)n * a.LC + c];
        }
      }
#pragma unroll
      for (int j = 0; j < NL_; j++) {
        int id = threadIdx.x + 256 * j;
        if (id < BOXL * CPV) {
          u32x4 v = pl[j];
          if (a.lg_scale) v = xform(v, sc, sh, a.lg_relu);
          if (!((vl >> j) & 1u)) v = u32x4{0u, 0u, 0u, 0u};
          *reinterpret_cast<u32x4*>(l_lds + (id / CPV) * LP + part * 16) = v;
        }
      }
    };
    // lane roles for ds_read_b64_tr_b16: group g4 = lane>>4 ; within group i = lane&15, q = i>>2, p = i&3
    const int g4 = lane >> 4, i16 = lane & 15, q = i16 >> 2, p4 = i16 & 3;
    const int hh = g4 >> 1, cb = (g4 & 1) * 16;
    const int colb = (cb + 4 * p4) * 2;
    using lds_s16x4 = s16x4 __attribute__((address_space(3)));
    auto tr_read = [&](const char* ptr) {
      s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)ptr);
      return __builtin_bit_cast(u32x2, v);
    };
    if (t_begin < t_end) prefetch(t_begin);
    for (int tile = t_begin; tile < t_end; tile++) {
      commit(tile);
      WS_BARRIER();
      if (tile + 1 < t_end) prefetch(tile + 1);
      for (int ks = 0; ks < MT / 16; ks++) {
        // the two 4-voxel groups this lane addresses: k = 8*hh + 4*t + q
        int sA[2], lB[2];
#pragma unroll
        for (int tt = 0; tt < 2; tt++) {
          int lin = ks * 16 + 8 * hh + 4 * tt + q;
          int lz = lin / (TH * TW), ly = (lin / TW) % TH, lx = lin % TW;
          sA[tt] = lin * LP + colb;
          lB[tt] = ((((FLAT ? 0 : S * lz)) * BH + S * ly) * BW + S * lx) * LP + colb;
        }
        // all 16 transposed reads of this k-step are requested before its 7 MFMAs (wave 3's 7th tap is a dummy
        // pointing at tap 0: uniform instruction stream, its accumulator is never stored)
        u32x2 a0u = tr_read(s_lds + sA[0]), a1u = tr_read(s_lds + sA[1]);
        u32x2 b0u[TAPS_PER_WAVE], b1u[TAPS_PER_WAVE];
#pragma unroll
        for (int j = 0; j < TAPS_PER_WAVE; j++) {
          b0u[j] = tr_read(l_lds + lB[0] + tapoff[j]);
          b1u[j] = tr_read(l_lds + lB[1] + tapoff[j]);
        }
        __builtin_amdgcn_sched_barrier(0);
        u32x4 af = {a0u[0], a0u[1], a1u[0], a1u[1]};
#pragma unroll
        for (int j = 0; j < TAPS_PER_WAVE; j++) {
          u32x4 bf = {b0u[j][0], b0u[j][1], b1u[j][0], b1u[j][1]};
          Mma<T>::run(af, bf, acc[j]);
        }
      }
      WS_BARRIER();
    }
  } else {
    // ---- f32 (parity path): plain stage -> barrier -> compute -> barrier ------------------------------------------
    for (int tile = t_begin; tile < t_end; tile++) {
      int n, z0, y0, x0;
      tile_origin(tile, n, z0, y0, x0);
      if (tile > t_begin) __syncthreads();
      stage_box<T, TD, TH, TW, ROWB, LP>(s_lds, reinterpret_cast<const T*>(a.sm), a.sm_pitch, a.SC, n, a.Ds, a.Hs, a.Ws,
                                         z0, y0, x0, scb * 32, ROWB, a.sm_scale, a.sm_shift, a.sm_relu);
      stage_box<T, BD, BH, BW, ROWB, LP>(l_lds, reinterpret_cast<const T*>(a.lg), a.lg_pitch, a.LC, n, a.Dl, a.Hl, a.Wl,
                                         FLAT ? z0 : S * z0 - 1, S * y0 - 1, S * x0 - 1, lcb * 32, ROWB, a.lg_scale, a.lg_shift,
                                         a.lg_relu);
      __syncthreads();
      const int r = lane & 31, hh = lane >> 5;
      for (int ks = 0; ks < MT / 2; ks++) {
        int lin = ks * 2 + hh;
        int lz = lin / (TH * TW), ly = (lin / TW) % TH, lx = lin % TW;
        float av = *reinterpret_cast<const float*>(s_lds + lin * LP + r * 4);
        const char* lb = l_lds + ((((FLAT ? 0 : S * lz)) * BH + S * ly) * BW + S * lx) * LP + r * 4;
#pragma unroll
        for (int j = 0; j < TAPS_PER_WAVE; j++) {
          if (j < ntaps_here) {
            float bv = *reinterpret_cast<const float*>(lb + tapoff[j]);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[j], 0, 0, 0);
          }
        }
      }
    }
  }

  // partial[g][tap][SCp][LCp]
  const int col = lane & 31, hh2 = lane >> 5;
#pragma unroll
  for (int j = 0; j < TAPS_PER_WAVE; j++) {
    if (j < ntaps_here) {
      int tap = TAP0 + wave * TAPS_PER_WAVE + j;
      float* base = a.partials + (((int64_t)blockIdx.x * 27 + tap) * a.SCp + scb * 32) * a.LCp + lcb * 32 + col;
#pragma unroll
      for (int i = 0; i < 16; i++) {
        int row = (i & 3) + 8 * (i >> 2) + 4 * hh2;
        base[(int64_t)row * a.LCp] = acc[j][i];
      }
    }
  }
  if constexpr (FLAT) {   // the 18 taps off the centre depth plane: zero blocks (the slab reduction sums all 27)
    for (int t = wave; t < 18; t += 4) {
      const int tap = t < 9 ? t : t + 9;
      float* base = a.partials + (((int64_t)blockIdx.x * 27 + tap) * a.SCp + scb * 32) * a.LCp + lcb * 32 + col;
#pragma unroll
      for (int i = 0; i < 16; i++) base[(int64_t)((i & 3) + 8 * (i >> 2) + 4 * hh2) * a.LCp] = 0.f;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// conv_wgrad2: bf16 stride-1 weight gradient with DOUBLE-BUFFERED tiles (same idea as conv_ws2_kernel).
// conv_wgrad_kernel spends ~3 cycles outside the matrix pipe per MFMA cycle: per-slot index arithmetic in the
// prefetch, the transform + LDS commit, and a transposed-read latency exposed in every k-step.  Here the tile
// under the MFMAs (T0, buffer PAR) is read with a one-k-step look-ahead while, in the gaps of the same stream,
// tile T1 goes registers -> (InstanceNorm/ReLU) -> the other buffer and tile T2's loads refill the registers.
// One barrier per tile; slot offsets are per-thread constants; tile coordinates advance incrementally.
// AP (WgradArgs::ap_*): the small operand arrives as d(activation); its InstanceNorm(+ReLU) backward is applied on the way
// into LDS (in_bwd_elem) from a second staged stream (the layer's raw output y), and the rows leave for ap_out as well.
template <typename T, bool XFL, bool AP = false>
__global__ __launch_bounds__(256) void conv_wgrad2_kernel(WgradArgs a) {
  static_assert(sizeof(T) == 2, "16-bit storage only");
  constexpr int TD = 4, TH = 8, TW = 8, MT = TD * TH * TW, BD = TD + 2, BH = TH + 2, BW = TW + 2, BOXL = BD * BH * BW;
  // unpadded 64-byte rows: the 4 voxel rows x 16 dwords a ds_read_b64_tr_b16 half-wave touches then tile the 64
  // banks exactly (an 80-byte pitch wraps the 4th row onto the 1st: 2-way conflicts on every read)
  constexpr int LP = 64, CPV = 4, EPC = 8;
  constexpr int SBUF = MT * LP, LBUF = BOXL * LP, BUF = SBUF + LBUF;
  constexpr int NS_ = MT * CPV / 256, NL_ = (BOXL * CPV + 255) / 256, NSLOT = NS_ + NL_;
  constexpr int KS = MT / 16, NT = 7;  // k-steps per tile, taps per wave (7,7,7,6 + one dummy)
  constexpr int PD = 6, NPF = PD + 1;  // a slot's global load is issued PD k-steps before its commit; register ring
  static_assert(NSLOT + 2 <= KS && NSLOT >= PD, "slot schedule: commits at k-steps 0..NSLOT-1, loads PD steps ahead");
  __shared__ __attribute__((aligned(256))) char lds[2 * BUF + 256 + (AP ? 7 * 32 * 4 : 0)];
  float* const s_xf = reinterpret_cast<float*>(lds + 2 * BUF);  // [32 scale][32 shift] of the large operand
  float* const s_ap = reinterpret_cast<float*>(lds + 2 * BUF + 256);  // AP: [7][32] constants of the small operand's block

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int scb = blockIdx.y, lcb = blockIdx.z;
  const int part = tid & (CPV - 1);
  const int ntz = (a.Ds + TD - 1) / TD, nty = (a.Hs + TH - 1) / TH, ntx = (a.Ws + TW - 1) / TW;
  const float relu_lo = (XFL && a.lg_relu) ? 0.f : -INFINITY;

  // ---- transposed-read addresses (lane roles of ds_read_b64_tr_b16: 4 voxels x 16 channels per 16 lanes)
  const int g4 = lane >> 4, i16 = lane & 15, q = i16 >> 2, p4 = i16 & 3;
  const int hh = g4 >> 1, cb = (g4 & 1) * 16;
  const int colb = (cb + 4 * p4) * 2;
  // per tap; the voxel group tt and the k-step ride in the 16-bit immediate offset, the buffer is added per tile
  int sA, lB[NT];
  sA = (8 * hh + q) * LP + colb;
#pragma unroll
  for (int j = 0; j < NT; j++) {
    int tap = wave * NT + j;
    if (tap >= 27) tap = 0;  // dummy slot of the last wave (never stored)
    const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
    lB[j] = SBUF + (((kz * BH + ky + hh) * BW) + kx + q) * LP + colb;
  }
  const int ntaps_here = min(NT, 27 - wave * NT);

  // ---- staging slots (per-thread constants): slot s < NS_ -> small tile, else large box
  // small tile: slot s holds voxel v0 + 64 s = one z-plane further (everything else is a compile-time offset);
  // large box: explicit per-slot constants
  const int v0 = tid >> 2, s_by = (v0 >> 3) & 7, s_bx = v0 & 7;  // v0 < 64: z-plane 0
  const int s_goff0 = (s_by * a.Ws + s_bx) * (int)a.sm_pitch;
  const int s_plane = a.Hs * a.Ws * (int)a.sm_pitch;
  const int w0 = v0 * LP + part * 16;
  int goffL[NL_], gxyzL[NL_];
#pragma unroll
  for (int k = 0; k < NL_; k++) {
    // threads past the end of the last slot redo the box's last voxel (same part): no predicate needed
    const int vox = min(tid + 256 * k, BOXL * CPV - CPV + part) >> 2;
    const int bz = vox / (BH * BW), rem = vox - bz * (BH * BW), by = rem / BW, bx = rem - by * BW;
    goffL[k] = ((bz * a.Hl + by) * a.Wl + bx) * (int)a.lg_pitch;
    gxyzL[k] = (bz << 16) | (by << 8) | bx;
  }
  const int w_last = SBUF + (min(tid + 256 * (NL_ - 1), BOXL * CPV - CPV + part) >> 2) * LP + part * 16;
  auto goff = [&](int s) { return s < NS_ ? s_goff0 + s * s_plane : goffL[s - NS_]; };
  auto woff = [&](int s) {
    return s < NS_ ? w0 + s * 64 * LP : (s < NSLOT - 1 ? SBUF + w0 + (s - NS_) * 64 * LP : w_last);
  };
  const bool sc_ok = scb * 32 + part * EPC < a.SC, lc_ok = lcb * 32 + part * EPC < a.LC;
  const bool chan_all = (a.SC % 32 == 0) && (a.LC % 32 == 0);
  // AP: y is read and dy written through buffer descriptors with 32-bit byte offsets (launcher: both tensors < 2 GiB); an
  // offset with bit 31 set is out of range -- such a load returns 0 and such a store is dropped, so neither is ever
  // branched around.  Slot s of a tile: tile offset (uniform) + v0 offset + s planes.
  constexpr uint32_t AP_OOB = 0x80000000u;
  const __amdgpu_buffer_rsrc_t ap_ry =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(AP ? a.ap_y : nullptr), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t ap_ro = __builtin_amdgcn_make_buffer_rsrc(AP ? a.ap_out : nullptr, 0, 0x7fffffff, 0x00020000);
  const uint32_t ap_yv0 = AP ? (uint32_t)(((s_by * a.Ws + s_bx) * (int)a.ap_y_pitch + scb * 32 + part * EPC) * 2) : 0u;
  const uint32_t ap_yplane = AP ? (uint32_t)(a.Hs * a.Ws * (int)a.ap_y_pitch * 2) : 0u;
  const uint32_t ap_ov0 = AP ? (uint32_t)(((s_by * a.Ws + s_bx) * (int)a.ap_out_pitch + scb * 32 + part * EPC) * 2) : 0u;
  const uint32_t ap_oplane = AP ? (uint32_t)(a.Hs * a.Ws * (int)a.ap_out_pitch * 2) : 0u;
  auto ap_tile_vox = [&](const WsTile& c) { return (uint32_t)(((c.n * a.Ds + c.z0) * a.Hs + c.y0) * a.Ws + c.x0); };
  auto ap_ty_of = [&](const WsTile& c, bool valid) { return valid ? ap_tile_vox(c) * (uint32_t)a.ap_y_pitch * 2u : AP_OOB; };
  auto ap_to_of = [&](const WsTile& c, bool valid) {  // only the workgroups of large-channel block 0 store
    return (valid && lcb == 0) ? ap_tile_vox(c) * (uint32_t)a.ap_out_pitch * 2u : AP_OOB;
  };
  const T* const s_safe = reinterpret_cast<const T*>(a.sm);
  const T* const l_safe = reinterpret_cast<const T*>(a.lg);
  const T* const s_src = s_safe + scb * 32 + part * EPC;
  const T* const l_src = l_safe + lcb * 32 + part * EPC;

  // Tile schedule (as in conv_ws2_kernel, conv_igemm.hip): an interior pass (unchecked copy of the phase, one long run) and
  // a border pass (checked copy); inside each, XCD x owns the x-th eighth of the raster-ordered list and its
  // gridDim.x/8 workgroups walk it interleaved, so neighbouring tiles' halos meet in that XCD's L2.
  const bool has_int = chan_all && ntz >= 3 && nty >= 3 && ntx >= 3;
  const int ipz = ntz - 2, ipy = nty - 2, ipx = ntx - 2;
  const int n_int = has_int ? a.N * ipz * ipy * ipx : 0;
  const int per_bor = ntz * nty * ntx - (has_int ? ipz * ipy * ipx : 0);
  const int n_bor = a.N * per_bor;
  const int G = gridDim.x;
  const int NX = (G % 8 == 0) ? 8 : 1;
  const int WPX = G / NX;
  const int xcd = blockIdx.x % NX, slot = blockIdx.x / NX;
  auto split = [&](int total, int& begin, int& cnt) {
    const int r0 = (int)((int64_t)total * xcd / NX), r1 = (int)((int64_t)total * (xcd + 1) / NX);
    begin = r0 + slot;
    cnt = (r1 - r0 > slot) ? (r1 - r0 - slot + WPX - 1) / WPX : 0;
  };
  int int_begin, int_cnt, bor_begin, bor_cnt;
  split(n_int, int_begin, int_cnt);
  split(n_bor, bor_begin, bor_cnt);
  int sdx = 0, sdy = 0, sdz = 0, sdn = 0;  // mixed-radix digits of the stride WPX over the interior tile grid
  if (has_int) {
    int t = WPX;
    sdx = t % ipx, t /= ipx;
    sdy = t % ipy, t /= ipy;
    sdz = t % ipz, sdn = t / ipz;
  }
  auto int_init = [&](WsTile& c, int k) {
    int t = k;
    c.x0 = (t % ipx + 1) * TW;
    t /= ipx;
    c.y0 = (t % ipy + 1) * TH;
    t /= ipy;
    c.z0 = (t % ipz + 1) * TD;
    c.n = t / ipz;
    c.k = k;
  };
  auto int_next = [&](WsTile& c) {  // + WPX tiles in raster order of the interior grid
    int xi = (c.x0 >> 3) - 1 + sdx, yi = (c.y0 >> 3) - 1 + sdy, zi = (c.z0 >> 2) - 1 + sdz;
    c.n += sdn;
    if (xi >= ipx) xi -= ipx, yi++;
    if (yi >= ipy) yi -= ipy, zi++;
    if (zi >= ipz) zi -= ipz, c.n++;
    c.x0 = (xi + 1) * TW, c.y0 = (yi + 1) * TH, c.z0 = (zi + 1) * TD;
  };
  auto bor_init = [&](WsTile& c, int k) {
    int tz, ty, tx;
    c.k = k;
    c.n = k / per_bor;
    int rem = k - c.n * per_bor;
    if (!has_int) {
      tx = rem % ntx, ty = (rem / ntx) % nty, tz = rem / (ntx * nty);
    } else {
      const int plane = nty * ntx, ring = plane - ipy * ipx;  // border tiles of a z-plane: all of it / its rim
      if (rem < plane) {
        tz = 0, ty = rem / ntx, tx = rem % ntx;
      } else if (rem - plane < ipz * ring) {
        rem -= plane;
        tz = 1 + rem / ring;
        rem %= ring;
        if (rem < ntx) {
          ty = 0, tx = rem;
        } else if (rem - ntx < 2 * ipy) {
          rem -= ntx;
          ty = 1 + (rem >> 1), tx = (rem & 1) ? ntx - 1 : 0;
        } else {
          ty = nty - 1, tx = rem - ntx - 2 * ipy;
        }
      } else {
        rem -= plane + ipz * ring;
        tz = ntz - 1, ty = rem / ntx, tx = rem % ntx;
      }
    }
    c.z0 = tz * TD, c.y0 = ty * TH, c.x0 = tx * TW;
  };
  auto bor_next = [&](WsTile& c) { bor_init(c, c.k + WPX); };
  auto s_org_of = [&](const WsTile& c) -> const T* {
    return s_src + ((((int64_t)c.n * a.Ds + c.z0) * a.Hs + c.y0) * a.Ws + c.x0) * a.sm_pitch;
  };
  auto l_org_of = [&](const WsTile& c) -> const T* {
    return l_src + ((((int64_t)c.n * a.Dl + (c.z0 - 1)) * a.Hl + (c.y0 - 1)) * a.Wl + (c.x0 - 1)) * a.lg_pitch;
  };
  auto slot_ok = [&](int s, const WsTile& c) {
    if (s < NS_) return sc_ok & (c.z0 + s < a.Ds) & (c.y0 + s_by < a.Hs) & (c.x0 + s_bx < a.Ws);
    const int g = gxyzL[s - NS_];
    const int bz = g >> 16, by = (g >> 8) & 255, bx = g & 255;
    return lc_ok & ((unsigned)(c.z0 - 1 + bz) < (unsigned)a.Dl) & ((unsigned)(c.y0 - 1 + by) < (unsigned)a.Hl) &
           ((unsigned)(c.x0 - 1 + bx) < (unsigned)a.Wl);
  };

  u32x4 pf[NPF];  // slot s lives in pf[s % NPF] from its load to its commit PD k-steps later
  u32x4 py[AP ? NS_ : 1];  // AP: the y chunk of small slot s, requested together with its d(activation) chunk
  // unconditional loads from a clamped address (never branch around a load)
  // ty (AP): byte offset of the tile's first voxel in y, or AP_OOB for a tile past the end of the list
  auto load_one = [&](auto fast_tag, int s, const WsTile& c, bool valid, const T* sorg, const T* lorg, uint32_t ty) {
    const T* org = (s < NS_) ? sorg : lorg;
    if constexpr (decltype(fast_tag)::value) {
      pf[s % NPF] = *reinterpret_cast<const u32x4*>(org + goff(s));
      if constexpr (AP)
        if (s < NS_) py[s] = __builtin_amdgcn_raw_buffer_load_b128(ap_ry, ty + ap_yv0 + s * ap_yplane, 0, 0);
    } else {
      const bool ok = valid & slot_ok(s, c);
      const T* p = ok ? org + goff(s) : ((s < NS_) ? s_safe : l_safe);
      pf[s % NPF] = *reinterpret_cast<const u32x4*>(p);
      if constexpr (AP)
        if (s < NS_) py[s] = __builtin_amdgcn_raw_buffer_load_b128(ap_ry, ok ? ty + ap_yv0 + s * ap_yplane : AP_OOB, 0, 0);
    }
  };
  float sc[EPC], sh[EPC];
  auto read_xf = [&]() {
#pragma unroll
    for (int e = 0; e < EPC; e += 4) {
      f32x4 u = *reinterpret_cast<const f32x4*>(s_xf + part * EPC + e);
      f32x4 v = *reinterpret_cast<const f32x4*>(s_xf + 32 + part * EPC + e);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        sc[e + k] = u[k];
        sh[e + k] = v[k];
      }
    }
  };
  // AP: the seven constants of this thread's 8 channels, re-read from s_ap at the top of every tile (56 registers that live
  // for the four small-slot commits only)
  float apk[AP ? 7 : 1][EPC];
  auto read_ap = [&]() {
    if constexpr (AP) {
#pragma unroll
      for (int k = 0; k < 7; k++)
#pragma unroll
        for (int e = 0; e < EPC; e += 4) {
          const f32x4 u = *reinterpret_cast<const f32x4*>(s_ap + k * 32 + part * EPC + e);
#pragma unroll
          for (int i = 0; i < 4; i++) apk[k][e + i] = u[i];
        }
    }
  };
  // to (AP): byte offset of the tile's first voxel in ap_out, or AP_OOB (tile past the end / not this workgroup's to store)
  auto commit_one = [&](auto fast_tag, int s, const WsTile& c, char* dst, uint32_t to) {
    u32x4 v = pf[s % NPF];
    if constexpr (XFL) {
      if (s >= NS_) {
        float f[EPC];
        ST<T>::unpack(v, f);
#pragma unroll
        for (int e = 0; e < EPC; e++) f[e] = fmaxf(f[e] * sc[e] + sh[e], relu_lo);
        v = ST<T>::pack(f);
      }
    }
    if constexpr (AP) {
      if (s < NS_) {
        float g[EPC], f[EPC];
        ST<T>::unpack(v, g);
        ST<T>::unpack(py[s < NS_ ? s : 0], f);
#pragma unroll
        for (int e = 0; e < EPC; e++)
          g[e] = in_bwd_elem(g[e], f[e], apk[0][e], apk[1][e], apk[2][e], apk[3][e], apk[4][e], apk[5][e], apk[6][e]);
        v = ST<T>::pack(g);
      }
    }
    bool ok = true;
    if constexpr (!decltype(fast_tag)::value) {
      ok = slot_ok(s, c);
#pragma unroll
      for (int k = 0; k < 4; k++) v[k] = ok ? v[k] : 0u;
    }
    *reinterpret_cast<u32x4*>(dst + woff(s)) = v;
    if constexpr (AP)
      if (s < NS_) __builtin_amdgcn_raw_buffer_store_b128(v, ap_ro, ok ? to + ap_ov0 + s * ap_oplane : AP_OOB, 0, 0);
  };
  int tbl_n = -1;
  auto refresh_xf = [&](int n) {  // uniform; nobody reads the old tables any more (sc/sh hold theirs; apk is per tile)
    if constexpr (XFL) {
      if (tid < 32) {
        const int c = min(lcb * 32 + tid, a.LC - 1);
        s_xf[tid] = a.lg_scale[(int64_t)n * a.LC + c];
        s_xf[32 + tid] = a.lg_shift[(int64_t)n * a.LC + c];
      }
    }
    if constexpr (AP) {
      if (tid >= 32) {
        const int i = tid - 32, k = i >> 5, c = min(scb * 32 + (i & 31), a.SC - 1);
        s_ap[i] = a.ap_tab[k][(int64_t)n * a.SC + c];
      }
    }
    tbl_n = n;
    __syncthreads();
    if constexpr (XFL) read_xf();
  };

  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; j++)
#pragma unroll
    for (int i = 0; i < 16; i++) acc[j][i] = 0.f;

#ifdef WS_DBG_STAMPS
  unsigned long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long tlast = __builtin_amdgcn_s_memtime();
#endif
  {
    WsTile T0, T1, T2;
    bool v1 = false, v2 = false;
    const T *so1 = s_safe, *lo1 = l_safe, *so2 = s_safe, *lo2 = l_safe;
    uint32_t ty1 = AP_OOB, ty2 = AP_OOB, to1 = AP_OOB, to2 = AP_OOB;  // AP: tile offsets in y / ap_out (see load_one, commit_one)
    int left = 0, par = 0;
    // start a pass at its k-th tile: T0 -> buffer 0 (not overlapped, NPF slots at a time), first PD slots of T1 ->
    // registers
    auto begin_pass = [&](auto border_tag, int k, int count) __attribute__((always_inline)) {
      constexpr bool BORDER = decltype(border_tag)::value;
      auto next = [&](WsTile& c) {
        if constexpr (BORDER)
          bor_next(c);
        else
          int_next(c);
      };
      if constexpr (BORDER)
        bor_init(T0, k);
      else
        int_init(T0, k);
      left = count - 1;
      T1 = T0;
      next(T1);
      T2 = T1;
      next(T2);
      v1 = left >= 1, v2 = left >= 2;
      so1 = v1 ? s_org_of(T1) : s_safe;
      lo1 = v1 ? l_org_of(T1) : l_safe;
      so2 = v2 ? s_org_of(T2) : s_safe;
      lo2 = v2 ? l_org_of(T2) : l_safe;
      const T* so0 = s_org_of(T0);
      const T* lo0 = l_org_of(T0);
      ty1 = ap_ty_of(T1, v1), ty2 = ap_ty_of(T2, v2);
      to1 = ap_to_of(T1, v1), to2 = ap_to_of(T2, v2);
      __syncthreads();  // the previous pass is done with both buffers
      par = 0;
      if constexpr (XFL || AP) refresh_xf(T0.n);
      read_ap();
#pragma unroll
      for (int s0 = 0; s0 < NSLOT; s0 += NPF) {
#pragma unroll
        for (int s = s0; s < s0 + NPF && s < NSLOT; s++) load_one(std::false_type{}, s, T0, true, so0, lo0, ap_ty_of(T0, true));
#pragma unroll
        for (int s = s0; s < s0 + NPF && s < NSLOT; s++) commit_one(std::false_type{}, s, T0, lds, ap_to_of(T0, true));
      }
#pragma unroll
      for (int s = 0; s < PD; s++) load_one(std::false_type{}, s, T1, v1, so1, lo1, ty1);
      WS_BARRIER();
    };

    using lds_s16x4 = s16x4 __attribute__((address_space(3)));
    auto tr_read = [&](int off) {
      s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lds + off));
      return __builtin_bit_cast(u32x2, v);
    };
    // The buffer parity is a RUN-TIME value folded into the 8 read-address registers: with it as a template
    // parameter the copies of the phase disagreed on where the in-flight staging registers live, and the compiler
    // drained every outstanding load (s_waitcnt vmcnt(0)) at the loop's back edge.
    auto tile_phase = [&](auto fast_tag) __attribute__((always_inline)) {
      constexpr int FASTI = decltype(fast_tag)::value ? 0 : 4;
      (void)FASTI;
      char* const a_wr = lds + (1 - par) * BUF;
      const int sAw = sA + par * BUF;
      int lBw[NT];
#pragma unroll
      for (int j = 0; j < NT; j++) lBw[j] = lB[j] + par * BUF;
      if constexpr (XFL || AP) {
        if (v1 && T1.n != tbl_n) refresh_xf(T1.n);
      }
      read_ap();
      WS2_STAMP(0)
      // B fragments: ONE register set, re-read for k-step ks+1 right behind the MFMA that consumed them (the arch
      // VGPR file is 256 deep: a second set pushed the staging ring into AGPR/scratch spills); A: two sets
      u32x2 A0[2], A1[2], B0[NT], B1[NT];
      auto koff = [&](int ks) { return ((ks >> 2) * BH * BW + 2 * (ks & 3) * BW) * LP; };
      auto read_a = [&](int ks) {
        A0[ks & 1] = tr_read(sAw + ks * 16 * LP);
        A1[ks & 1] = tr_read(sAw + ks * 16 * LP + 4 * LP);
      };
      auto read_b = [&](int ks, int j) {
        B0[j] = tr_read(lBw[j] + koff(ks));
        B1[j] = tr_read(lBw[j] + koff(ks) + 4 * LP);
      };
      read_a(0);
#pragma unroll
      for (int j = 0; j < NT; j++) read_b(0, j);
#pragma unroll
      for (int ks = 0; ks < KS; ks++) {
        if (ks + 1 < KS) read_a(ks + 1);
        // staging: commit slot ks of T1; load the slot that commits PD k-steps from now (T1's, or T2's when that
        // falls into the next tile phase)
        if (ks < NSLOT) commit_one(fast_tag, ks, T1, a_wr, to1);
        if (ks + PD < NSLOT)
          load_one(fast_tag, ks + PD, T1, v1, so1, lo1, ty1);
        else if (ks + PD >= KS)
          load_one(fast_tag, ks + PD - KS, T2, v2, so2, lo2, ty2);
        const u32x4 af = {A0[ks & 1][0], A0[ks & 1][1], A1[ks & 1][0], A1[ks & 1][1]};
#pragma unroll
        for (int j = 0; j < NT; j++) {
          const u32x4 bf = {B0[j][0], B0[j][1], B1[j][0], B1[j][1]};
          Mma<T>::run(af, bf, acc[j]);
          if (ks + 1 < KS) read_b(ks + 1, j);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      WS2_STAMP(1 + FASTI)
      WS_BARRIER();  // buffer PAR fully read, buffer 1-PAR fully written
      WS2_STAMP(2)
      // pin the loop-carried accumulators to AGPRs: left alone the compiler carries them in VGPRs between tile
      // phases and pays 2 x 112 v_accvgpr moves per tile
#pragma unroll
      for (int j = 0; j < NT; j++) asm volatile("" : "+a"(acc[j]));
    };

    bool more = true;
    auto step = [&](auto border_tag) __attribute__((always_inline)) {
      constexpr bool BORDER = decltype(border_tag)::value;
      par ^= 1;
      more = v1;
      if (!more) return;
      left--;
      T0 = T1;
      T1 = T2;
      v1 = v2;
      so1 = so2;
      lo1 = lo2;
      ty1 = ty2, to1 = to2;
      if constexpr (BORDER)
        bor_next(T2);
      else
        int_next(T2);
      v2 = left >= 2;
      so2 = v2 ? s_org_of(T2) : s_safe;
      lo2 = v2 ? l_org_of(T2) : l_safe;
      ty2 = ap_ty_of(T2, v2), to2 = ap_to_of(T2, v2);
    };
    if (int_cnt > 0) {  // interior pass: the unchecked copy, one run (its own back edge: nothing drained per tile)
      begin_pass(std::false_type{}, int_begin, int_cnt);
      more = true;
      while (more) {
        tile_phase(std::true_type{});
        step(std::false_type{});
      }
    }
    if (bor_cnt > 0) {  // border pass: the checked copy
      begin_pass(std::true_type{}, bor_begin, bor_cnt);
      more = true;
      while (more) {
        tile_phase(std::false_type{});
        step(std::true_type{});
      }
    }
  }

  // partial[g][tap][SCp][LCp]
  const int col = lane & 31, hh2 = lane >> 5;
#pragma unroll
  for (int j = 0; j < NT; j++) {
    if (j < ntaps_here) {
      int tap = wave * NT + j;
      float* base = a.partials + (((int64_t)blockIdx.x * 27 + tap) * a.SCp + scb * 32) * a.LCp + lcb * 32 + col;
#pragma unroll
      for (int i = 0; i < 16; i++) {
        int row = (i & 3) + 8 * (i >> 2) + 4 * hh2;
        base[(int64_t)row * a.LCp] = acc[j][i];
      }
    }
  }
#ifdef WS_DBG_STAMPS
  __syncthreads();
  if (tid == 0 && blockIdx.y == 0 && blockIdx.z == 0)  // debug only: overwrites the head of this group's slab
    for (int k = 0; k < 8; k++) a.partials[(int64_t)blockIdx.x * 27 * a.SCp * a.LCp + k] = (float)tacc[k];
#endif
}

// ------------------------------------------------------------------------------------------------
// conv_wgrad_s2: 16-bit STRIDE-2 weight gradient (ConvTranspose3d: small = its input x, large = dy), double-buffered
// through LDS-DMA.  conv_wgrad_kernel<.,4,4,4,2> issued ~620 VALU instructions per tile and wave (per-slot div/mod,
// 64-bit addresses and bounds tests of 13 staging slots) for 28 MFMAs, with one tile of loads in flight and the LDS
// commit serialised with the MFMAs: 9 % matrix-pipe utilisation.  Here
//  * a workgroup owns SB = 2 small-channel blocks: a staged dy box and every B fragment feed two MFMAs (half the
//    L2->LDS bytes and LDS reads per FLOP).  The 2 x 7 x 16 accumulators fill the AGPR file, so nothing is staged through
//    registers: every 16-byte slot is a global_load_lds_dwordx4 (lane-linear LDS image = consecutive 64-byte rows,
//    4 lanes per row), slots outside the tensor / beyond the channel count read a zero line instead;
//  * tile t+1 is in flight while tile t is under the MFMAs (two LDS buffers, one barrier per tile); slot offsets are
//    per-thread constants (32-bit offsets from a per-tile origin);
//  * the InstanceNorm/ReLU transform of x is applied in place by the thread that loaded the chunk (its own 16 bytes
//    are visible to it once vmcnt says so; the small-operand loads are issued first, so they retire first);
//  * the 9x9x9 dy box is stored with each x-line split into even then odd positions: the 4 voxels a transposed
//    read addresses (2 apart in x) are then 4 consecutive 64-byte rows = all 64 banks once, without row padding.
// Tile = 4x4x4 small voxels (whole tiles only: launcher check); wave w owns taps 7w..7w+6 (27 + one dummy).
template <typename T, int SB>
__global__ __launch_bounds__(256) void conv_wgrad_s2_kernel(WgradArgs a) {
  static_assert(sizeof(T) == 2, "16-bit storage only");
  constexpr int MT = 64, BX = 9, BOXL = BX * BX * BX;
  constexpr int LP = 64, CPV = 4, EPC = 8;
  constexpr int NL_ = (BOXL * CPV + 255) / 256, NSLOT = SB + NL_;
  constexpr int SBUF = SB * MT * LP, LBUF = NL_ * 256 * 16, BUF = SBUF + LBUF;  // the last slot's tail lanes land in padding
  constexpr int KS = MT / 16, NT = 7;  // k-steps per tile, taps per wave
  static_assert(NSLOT <= 32, "slot validity bits");
  __shared__ __attribute__((aligned(256))) char lds[2 * BUF + SB * 64 * 4];
  float* const s_xf = reinterpret_cast<float*>(lds + 2 * BUF);  // [SB*32 scale][SB*32 shift] of the small operand

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int scb = blockIdx.y, lcb = blockIdx.z;
  const int part = tid & (CPV - 1), v0 = tid >> 2;
  const int ntz = a.Ds / 4, nty = a.Hs / 4, ntx = a.Ws / 4;
  const bool xfs = a.sm_scale != nullptr;
  const float relu_lo = (xfs && a.sm_relu) ? 0.f : -INFINITY;

  // ---- transposed-read addresses (lane roles of ds_read_b64_tr_b16: 4 voxels x 16 channels per 16 lanes).  Voxel
  // lin = 16 ks + 8 hh + 4 tt + q of the tile is (lz, ly, lx) = (ks, 2 hh + tt, q); k-step and tt are immediates,
  // the buffer parity is folded into the registers (toggled once per tile)
  const int g4 = lane >> 4, i16 = lane & 15, q = i16 >> 2, p4 = i16 & 3;
  const int hh = g4 >> 1, cb = (g4 & 1) * 16;
  const int colb = (cb + 4 * p4) * 2;
  int sA = (8 * hh + q) * LP + colb;
  int lB[NT];
#pragma unroll
  for (int j = 0; j < NT; j++) {
    int tap = wave * NT + j;
    if (tap >= 27) tap = 0;  // dummy slot of the last wave (never stored)
    const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
    const int pb = kx == 0 ? 0 : (kx == 1 ? 5 : 1);  // line position of box x = kx (even x first: 0,2,4,6,8,1,3,5,7)
    lB[j] = SBUF + ((kz * BX + 4 * hh + ky) * BX + pb + q) * LP + colb;
  }
  const int ntaps_here = min(NT, 27 - wave * NT);

  // ---- staging slots (per-thread constants): slot s < SB -> channel block s of small voxel v0, else box row
  // v0 + 64 (s - SB).  Only the LOW faces of a box can leave the tensor (whole tiles, Dl = 2 Ds): emz/emy/emx flag
  // the slots on them; chan_ok the slots whose channels (and box row) exist.
  const int s_goff = ((((v0 >> 4) * a.Hs) + ((v0 >> 2) & 3)) * a.Ws + (v0 & 3)) * (int)a.sm_pitch;
  int goffL[NL_];
  uint32_t emz = 0, emy = 0, emx = 0, chan_ok = 0;
  const bool lc_ok = lcb * 32 + part * EPC < a.LC;
#pragma unroll
  for (int k = 0; k < NL_; k++) {
    const int row = v0 + 64 * k;  // LDS row
    const int rc = min(row, BOXL - 1);
    const int line = rc / BX, pos = rc - line * BX;
    const int bx = pos < 5 ? 2 * pos : 2 * pos - 9, by = line % BX, bz = line / BX;
    goffL[k] = ((bz * a.Hl + by) * a.Wl + bx) * (int)a.lg_pitch;
    emz |= (bz == 0 ? 1u : 0u) << (SB + k);
    emy |= (by == 0 ? 1u : 0u) << (SB + k);
    emx |= (bx == 0 ? 1u : 0u) << (SB + k);
    chan_ok |= ((lc_ok && row < BOXL) ? 1u : 0u) << (SB + k);
  }
#pragma unroll
  for (int b = 0; b < SB; b++) chan_ok |= ((scb * SB + b) * 32 + part * EPC < a.SC ? 1u : 0u) << b;
  const T* const zero_src = reinterpret_cast<const T*>(g_zero_line);
  const T* const s_src = reinterpret_cast<const T*>(a.sm) + scb * SB * 32 + part * EPC;
  const T* const l_src = reinterpret_cast<const T*>(a.lg) + lcb * 32 + part * EPC;

  struct Tl {
    int n, z0, y0, x0;
  };
  auto decode = [&](int t, Tl& c) {
    c.x0 = (t % ntx) * 4;
    t /= ntx;
    c.y0 = (t % nty) * 4;
    t /= nty;
    c.z0 = (t % ntz) * 4;
    c.n = t / ntz;
  };
  const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)lds;
  // all slots of one tile, small operand first (its loads retire first: vmcnt(NL_) = "my x chunks have landed")
  auto issue_tile = [&](const Tl& c, int buf_off) __attribute__((always_inline)) {
    const T* const sorg = s_src + ((((int64_t)c.n * a.Ds + c.z0) * a.Hs + c.y0) * a.Ws + c.x0) * a.sm_pitch + s_goff;
    // box origin; may lie before the tensor (those slots read the zero line)
    const T* const lorg =
        l_src + ((((int64_t)c.n * a.Dl + (2 * c.z0 - 1)) * a.Hl + (2 * c.y0 - 1)) * a.Wl + (2 * c.x0 - 1)) * a.lg_pitch;
    const uint32_t off = (c.z0 == 0 ? emz : 0u) | (c.y0 == 0 ? emy : 0u) | (c.x0 == 0 ? emx : 0u);
    const uint32_t m = chan_ok & ~off;
    // wave-uniform LDS byte address of slot 0 (+ lane * 16 by the hardware)
    const uint32_t wbase = __builtin_amdgcn_readfirstlane(lds_base + buf_off + wave * 1024);
#pragma unroll
    for (int s = 0; s < NSLOT; s++) {
      const bool ok = (m >> s) & 1u;
      const T* p = (s < SB) ? sorg + s * 32 : lorg + goffL[s < SB ? 0 : s - SB];
      p = ok ? p : zero_src;
      // inline asm on purpose: hipcc drains a builtin LDS-DMA (vmcnt(0)) in front of the next LDS read of ANY buffer;
      // these are counted by hand (s_waitcnt vmcnt below).  M0 = LDS destination, saved and restored per statement.
      uint32_t keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep)
                   : "v"(p), "s"(wbase + (uint32_t)(s < SB ? s * MT * LP : SBUF + (s - SB) * 4096))
                   : "memory");
    }
  };
  int tbl_n = -1;
  auto refresh_xf = [&](int n) {  // uniform
    __syncthreads();              // nobody still reads the previous table
    if (tid < SB * 32) {
      const int c = scb * SB * 32 + tid;
      const bool live = c < a.SC;  // channels past the end stay exactly zero under the transform
      s_xf[tid] = live ? a.sm_scale[(int64_t)n * a.SC + c] : 0.f;
      s_xf[SB * 32 + tid] = live ? a.sm_shift[(int64_t)n * a.SC + c] : 0.f;
    }
    tbl_n = n;
    __syncthreads();
  };
  // x*scale+shift (+relu) on this thread's own chunks of the small tile in buffer buf_off
  auto transform_own = [&](int buf_off) __attribute__((always_inline)) {
#pragma unroll
    for (int b = 0; b < SB; b++) {
      u32x4* const slot = reinterpret_cast<u32x4*>(lds + buf_off + b * MT * LP + tid * 16);
      float f[EPC];
      ST<T>::unpack(*slot, f);
      const float* tb = s_xf + b * 32 + part * EPC;
#pragma unroll
      for (int e = 0; e < EPC; e += 4) {
        const f32x4 u = *reinterpret_cast<const f32x4*>(tb + e);
        const f32x4 w = *reinterpret_cast<const f32x4*>(tb + SB * 32 + e);
#pragma unroll
        for (int k = 0; k < 4; k++) f[e + k] = fmaxf(f[e + k] * u[k] + w[k], relu_lo);
      }
      *slot = ST<T>::pack(f);
    }
  };

  f32x16 acc[SB][NT];
#pragma unroll
  for (int b = 0; b < SB; b++)
#pragma unroll
    for (int j = 0; j < NT; j++)
#pragma unroll
      for (int i = 0; i < 16; i++) acc[b][j][i] = 0.f;

  const int t_begin = blockIdx.x * a.tiles_per_group;
  const int t_end = min(a.num_tiles, t_begin + a.tiles_per_group);
  if (t_begin < t_end) {
    using lds_s16x4 = s16x4 __attribute__((address_space(3)));
    auto tr_read = [&](int off) {
      s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lds + off));
      return __builtin_bit_cast(u32x2, v);
    };
    Tl T1;
    decode(t_begin, T1);
    if (xfs) refresh_xf(T1.n);
    issue_tile(T1, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (xfs) transform_own(0);
    WS_BARRIER();
    int wr_off = BUF;  // byte offset of the buffer being filled (the other one is read)
    for (int t = t_begin; t < t_end; t++) {
      const bool v1 = t + 1 < t_end;
      if (v1) {  // uniform
        decode(t + 1, T1);
        issue_tile(T1, wr_off);
      }
      u32x2 A0[2][SB], A1[2][SB], B0[NT], B1[NT];
      auto read_a = [&](int ks) {
#pragma unroll
        for (int b = 0; b < SB; b++) {
          A0[ks & 1][b] = tr_read(sA + b * MT * LP + ks * 16 * LP);
          A1[ks & 1][b] = tr_read(sA + b * MT * LP + ks * 16 * LP + 4 * LP);
        }
      };
      auto read_b = [&](int ks, int j) {
        B0[j] = tr_read(lB[j] + ks * 2 * BX * BX * LP);
        B1[j] = tr_read(lB[j] + ks * 2 * BX * BX * LP + 2 * BX * LP);
      };
      read_a(0);
#pragma unroll
      for (int j = 0; j < NT; j++) read_b(0, j);
#pragma unroll
      for (int ks = 0; ks < KS; ks++) {
        if (ks + 1 < KS) read_a(ks + 1);
#pragma unroll
        for (int j = 0; j < NT; j++) {
          const u32x4 bf = {B0[j][0], B0[j][1], B1[j][0], B1[j][1]};
#pragma unroll
          for (int b = 0; b < SB; b++) {
            const u32x4 af = {A0[ks & 1][b][0], A0[ks & 1][b][1], A1[ks & 1][b][0], A1[ks & 1][b][1]};
            Mma<T>::run(af, bf, acc[b][j]);
          }
          if (ks + 1 < KS) read_b(ks + 1, j);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      if (xfs && v1) {
        if (T1.n != tbl_n) refresh_xf(T1.n);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NL_) : "memory");  // this thread's x chunks of tile t+1 have landed
        transform_own(wr_off);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      WS_BARRIER();  // one buffer fully read, the other fully written
#pragma unroll
      for (int b = 0; b < SB; b++)
#pragma unroll
        for (int j = 0; j < NT; j++) asm volatile("" : "+a"(acc[b][j]));  // loop-carried accumulators stay in AGPRs
      // swap the buffers (the read addresses carry the parity)
      const int d = wr_off ? BUF : -BUF;
      sA += d;
#pragma unroll
      for (int j = 0; j < NT; j++) lB[j] += d;
      wr_off = BUF - wr_off;
    }
  }

  // partial[g][tap][SCp][LCp]
  const int col = lane & 31, hh2 = lane >> 5;
#pragma unroll
  for (int b = 0; b < SB; b++) {
    if ((scb * SB + b) * 32 >= a.SCp) continue;
#pragma unroll
    for (int j = 0; j < NT; j++) {
      if (j < ntaps_here) {
        const int tap = wave * NT + j;
        float* base = a.partials + (((int64_t)blockIdx.x * 27 + tap) * a.SCp + (scb * SB + b) * 32) * a.LCp + lcb * 32 + col;
#pragma unroll
        for (int i = 0; i < 16; i++) {
          const int row = (i & 3) + 8 * (i >> 2) + 4 * hh2;
          base[(int64_t)row * a.LCp] = acc[b][j][i];
        }
      }
    }
  }
}

// out[(sc*LC + lc)*27 + tap] (+)= sum_g partial[g][tap][sc][lc].  256 threads = 32 group-lanes x 8 lanes of 4 entries
// (16-byte loads; a workgroup owns 32 consecutive entries = one 128-byte line per slab); fixed summation order
// (bitwise reproducible)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ partials, float* __restrict__ dw,
                                                           int G, int SCp, int LCp, int SC, int LC, int accumulate) {
  __shared__ float red[32][36];
  const int e4 = threadIdx.x & 7, gl = threadIdx.x >> 3;
  const int64_t per = (int64_t)27 * SCp * LCp;  // a multiple of 32
  const float* src = partials + (int64_t)blockIdx.x * 32 + e4 * 4;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  int g = gl;
  for (; g + 32 < G; g += 64) {
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(src + (int64_t)g * per);
    const f32x4 a1 = *reinterpret_cast<const f32x4*>(src + (int64_t)(g + 32) * per);
    s += a0 + a1;
  }
  if (g < G) s += *reinterpret_cast<const f32x4*>(src + (int64_t)g * per);
  *reinterpret_cast<f32x4*>(&red[gl][e4 * 4]) = s;
  __syncthreads();
  if (threadIdx.x < 32) {
    const int el = threadIdx.x;
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 32; k++) t += red[k][el];
    const int64_t idx = (int64_t)blockIdx.x * 32 + el;
    const int lc = idx % LCp;
    const int sc = (idx / LCp) % SCp;
    const int tap = idx / ((int64_t)LCp * SCp);
    if (lc < LC && sc < SC) {
      float* o = dw + ((int64_t)sc * LC + lc) * 27 + tap;
      *o = accumulate ? (*o + t) : t;
    }
  }
}

// The same reduction for FEW slabs and a LARGE matrix (the low-resolution layers: G <= 8, up to 27 x 512 x 512
// entries).  There the cost is the transposed store (4-byte writes 108 bytes apart: 7 M sectors for 512 x 512), not
// the slab reads: a workgroup owns one sc row x 32 lc columns x all 27 taps, sums into LDS and writes the 864 outputs
// as one contiguous run.
__global__ __launch_bounds__(256) void wgrad_reduce_rows_kernel(const float* __restrict__ partials,
                                                                float* __restrict__ dw, int G, int SCp, int LCp, int SC,
                                                                int LC, int accumulate) {
  __shared__ float red[27][33];
  const int sc = blockIdx.y, lc0 = blockIdx.x * 32;
  const int64_t per = (int64_t)27 * SCp * LCp;
  for (int i = threadIdx.x; i < 27 * 32; i += 256) {
    const int tap = i >> 5, l = i & 31;
    const float* src = partials + ((int64_t)tap * SCp + sc) * LCp + lc0 + l;
    float s = 0.f;
    for (int g = 0; g < G; g++) s += src[(int64_t)g * per];
    red[tap][l] = s;
  }
  __syncthreads();
  if (sc >= SC) return;
  float* const out = dw + ((int64_t)sc * LC + lc0) * 27;
  const int n_out = min(32, LC - lc0) * 27;
  for (int j = threadIdx.x; j < n_out; j += 256) {
    const int l = j / 27, tap = j - l * 27;
    out[j] = accumulate ? out[j] + red[tap][l] : red[tap][l];
  }
}

template <typename T, int TD, int TH, int TW, int S, bool FLAT = false>
int launch_wgrad_t(WgradArgs a, float* dw, int sc_store, int lc_store, int accumulate, void* ws, size_t ws_bytes,
                   hipStream_t st) {
  a.SCp = round_up(a.SC, 32);
  a.LCp = round_up(a.LC, 32);
  a.num_tiles = a.N * ceil_div(a.Ds, TD) * ceil_div(a.Hs, TH) * ceil_div(a.Ws, TW);
  // 16-bit stride 2 without a transform of the large operand: conv_wgrad_s2_kernel, SB small-channel blocks per workgroup
  const bool use_s2 = !FLAT && sizeof(T) == 2 && S == 2 && !a.lg_scale && a.Ds % 4 == 0 && a.Hs % 4 == 0 &&
                      a.Ws % 4 == 0 && a.Dl == 2 * a.Ds && a.Hl == 2 * a.Hs && a.Wl == 2 * a.Ws;
  const int sb = (use_s2 && a.SCp >= 64) ? 2 : 1;
  const int sblocks = ceil_div(a.SCp / 32, sb);
  const int pairs = sblocks * (a.LCp / 32);
  const int64_t per = (int64_t)27 * a.SCp * a.LCp * sizeof(float);
  const bool use_new = !FLAT && sizeof(T) == 2 && S == 1 && !a.sm_scale;
  const int wg_target = hdf_cu_budget();  // one workgroup per CU
  int G = ceil_div(wg_target, pairs);
  G = (int)std::min<int64_t>(G, std::max<int64_t>(1, (int64_t)ws_bytes / per));
  G = std::min(G, a.num_tiles);
  a.tiles_per_group = ceil_div(a.num_tiles, G);
  G = ceil_div(a.num_tiles, a.tiles_per_group);
  HDF_CHECK_ARG((size_t)(G * per) <= ws_bytes, "wgrad workspace too small: need %lld have %zu", (long long)(G * per),
                ws_bytes);
  a.partials = reinterpret_cast<float*>(ws);
  dim3 grid(G, sblocks, a.LCp / 32);
  if constexpr (sizeof(T) == 2 && S == 2) {
    if (use_s2) {
      if (sb == 2)
        hipLaunchKernelGGL((conv_wgrad_s2_kernel<T, 2>), grid, dim3(256), 0, st, a);
      else
        hipLaunchKernelGGL((conv_wgrad_s2_kernel<T, 1>), grid, dim3(256), 0, st, a);
    }
  }
  if constexpr (sizeof(T) == 2 && S == 1) {
    if (use_new) {
      if (a.ap_y) {
        if (a.lg_scale)
          hipLaunchKernelGGL((conv_wgrad2_kernel<T, true, true>), grid, dim3(256), 0, st, a);
        else
          hipLaunchKernelGGL((conv_wgrad2_kernel<T, false, true>), grid, dim3(256), 0, st, a);
      } else if (a.lg_scale)
        hipLaunchKernelGGL((conv_wgrad2_kernel<T, true>), grid, dim3(256), 0, st, a);
      else
        hipLaunchKernelGGL((conv_wgrad2_kernel<T, false>), grid, dim3(256), 0, st, a);
    }
  }
  if (!use_new && !use_s2) {
    hipLaunchKernelGGL((conv_wgrad_kernel<T, TD, TH, TW, S, FLAT>), grid, dim3(256), 0, st, a);
  }
  HDF_LAUNCH_CHECK();
  int64_t n = (int64_t)27 * a.SCp * a.LCp;
  if (G <= 8)
    hipLaunchKernelGGL(wgrad_reduce_rows_kernel, dim3(a.LCp / 32, a.SCp), dim3(256), 0, st, a.partials, dw, G, a.SCp,
                       a.LCp, sc_store, lc_store, accumulate);
  else
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)ceil_div64(n, 32)), dim3(256), 0, st, a.partials, dw, G,
                       a.SCp, a.LCp, sc_store, lc_store, accumulate);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

}  // namespace

size_t hdf_wgrad_workspace_bytes(int stride, int N, int Ds, int Hs, int Ws, int SC, int LC) {
  int SCp = round_up(SC, 32), LCp = round_up(LC, 32);
  int64_t per = (int64_t)27 * SCp * LCp * sizeof(float);
  int pairs = (SCp / 32) * (LCp / 32);
  int tiles = stride == 1 ? N * ceil_div(Ds, 4) * ceil_div(Hs, 8) * ceil_div(Ws, 8)
                          : N * ceil_div(Ds, 4) * ceil_div(Hs, 4) * ceil_div(Ws, 4);
  if (Ds == 1) tiles = stride == 1 ? N * ceil_div(Hs, 16) * ceil_div(Ws, 16) : N * ceil_div(Hs, 8) * ceil_div(Ws, 8);   // flat tiles
  int G = std::min(ceil_div(1024, pairs), tiles);
  int64_t bytes = std::min<int64_t>((int64_t)G * per, std::max<int64_t>(per, (int64_t)96 << 20));
  return (size_t)bytes;
}

// the launches conv_wgrad2_kernel<., ., true> serves: 16-bit storage, stride 1, untransformed small operand, 16-byte rows
// on both extra tensors, and 32-bit byte offsets into them with bit 31 free for the out-of-range marker
bool hdf_wgrad_apply_takes(int dtype, int stride, const WgradArgs& a) {
  if (hdf_esz(dtype) != 2 || stride != 1 || a.sm_scale || !a.ap_y || !a.ap_out || a.Ds == 1) return false;
  for (int k = 0; k < 7; k++)
    if (!a.ap_tab[k]) return false;
  const int64_t vox = (int64_t)a.N * a.Ds * a.Hs * a.Ws;
  if (vox * a.ap_y_pitch * 2 >= (1ll << 31) || vox * a.ap_out_pitch * 2 >= (1ll << 31)) return false;
  if (a.ap_y_pitch % 8 || a.ap_out_pitch % 8 || a.SC % 16) return false;
  if ((reinterpret_cast<uintptr_t>(a.ap_y) | reinterpret_cast<uintptr_t>(a.ap_out)) & 15) return false;
  return a.Ds == a.Dl && a.Hs == a.Hl && a.Ws == a.Wl;
}

int hdf_launch_wgrad(int dtype, int stride, WgradArgs a, float* dw, int sc_store, int lc_store, int accumulate,
                     void* workspace, size_t workspace_bytes, hipStream_t st) {
  HDF_CHECK_ARG(a.SC % 16 == 0 && a.LC % 16 == 0, "wgrad: channel counts must be multiples of 16 (SC=%d LC=%d)", a.SC,
                a.LC);
  HDF_CHECK_ARG(stride == 1 || stride == 2, "wgrad: stride %d", stride);
  HDF_CHECK_ARG(!a.ap_y || hdf_wgrad_apply_takes(dtype, stride, a),
                "wgrad: the fused InstanceNorm backward does not take this launch (ask hdf_wgrad_apply_takes first)");
  HDF_DISPATCH_T(dtype, {
    if (a.Ds == 1) {   // depth-1 operands: the 2-D weight gradients (Conv2d / ConvTranspose2d, models/HDenseFormer_2D.py)
      HDF_CHECK_ARG(a.Dl == 1 && !a.ap_y, "wgrad: depth-1 small operand selects the 2-D operator (large operand of depth 1, no fused InstanceNorm backward)");
      if (stride == 1)
        return launch_wgrad_t<T, 1, 16, 16, 1, true>(a, dw, sc_store, lc_store, accumulate, workspace, workspace_bytes, st);
      return launch_wgrad_t<T, 1, 8, 8, 2, true>(a, dw, sc_store, lc_store, accumulate, workspace, workspace_bytes, st);
    }
    if (stride == 1)
      return launch_wgrad_t<T, 4, 8, 8, 1>(a, dw, sc_store, lc_store, accumulate, workspace, workspace_bytes, st);
    return launch_wgrad_t<T, 4, 4, 4, 2>(a, dw, sc_store, lc_store, accumulate, workspace, workspace_bytes, st);
  });
  return HDF_ERR_UNSUPPORTED;
}
