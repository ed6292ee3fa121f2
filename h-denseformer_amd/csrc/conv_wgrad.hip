// Weight gradients of the 3x3x3 convolution family:  D[tap][sc][lc] = sum_{n,i} S[n,i][sc] * L[n, STRIDE*i-1+tap][lc]
//   conv_wgrad_kernel     (here) every storage type, stride 1 and 2, 3-D and FLAT (the 2-D operators)
//   conv_wgrad2_kernel    (conv_wgrad2.hip) 16-bit stride 1: persistent, double-buffered tiles, optional fused
//                         InstanceNorm(+ReLU) backward
//   conv_wgrad_s2_kernel  (conv_wgrad_s2.hip) 16-bit stride 2 (ConvTranspose3d): LDS-DMA double-buffered
// Every kernel leaves fp32 partial slabs [G][27][SCp][LCp]; wgrad_reduce_kernel / wgrad_reduce_rows_kernel sum them in a fixed
// order into the torch layout.  The host side is here too: wgrad_route picks the kernel and its tile (WGRAD_TILES,
// conv_wgrad_tile.h), and the launch, the workspace size and hdf_wgrad_apply_takes all go by it.
#include "conv_wgrad_tile.h"

namespace {

// weight gradient:  D[tap][sc][lc] = sum_{n,i} S[n,i][sc] * L[n, STRIDE*i-1+tap][lc]
// bf16: both operands are contracted over VOXELS, which are the slow axis of the channels-last LDS
// rows -> read with ds_read_b64_tr_b16 (hardware transpose, 4 voxels x 16 channels per 16 lanes).
// f32: v_mfma_f32_32x32x2_f32 takes one scalar per lane, plain ds_read_b32.

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
    int tap = wave * TAPS_PER_WAVE + j;   // (wgrad_tap and TrLane of conv_wgrad_tile.h change this kernel's code: written out)
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

// ---- the route: which kernel a launch runs, by what tile.  The launch, the workspace size and hdf_wgrad_apply_takes all ask
// here, so a tile extent or a condition exists once.
enum class WgradKernel { generic, wgrad2, s2 };
struct WgradRoute {
  WgradKernel kernel;
  WgradTile tile;
  int sb;  // conv_wgrad_s2_kernel: small-channel blocks per workgroup (1 elsewhere)
};
WgradTile wgrad_tile(int stride, bool flat) { return WGRAD_TILES[stride == 1 ? 0 : 1][flat]; }
int wgrad_num_tiles(const WgradTile& t, int N, int Ds, int Hs, int Ws) {
  return N * ceil_div(Ds, t.td) * ceil_div(Hs, t.th) * ceil_div(Ws, t.tw);
}
WgradRoute wgrad_route(int dtype, int stride, const WgradArgs& a) {
  WgradRoute r{WgradKernel::generic, wgrad_tile(stride, a.Ds == 1), 1};
  if (hdf_wgrad_s2_takes(dtype, stride, a)) {
    r.kernel = WgradKernel::s2;
    r.sb = round_up(a.SC, 32) >= 64 ? 2 : 1;
  } else if (hdf_wgrad2_takes(dtype, stride, a)) {
    r.kernel = WgradKernel::wgrad2;
  }
  return r;
}

template <typename T, int S, bool FLAT>
void launch_wgrad_generic(const WgradArgs& a, dim3 grid, hipStream_t st) {
  constexpr WgradTile t = WGRAD_TILES[S - 1][FLAT];
  hipLaunchKernelGGL((conv_wgrad_kernel<T, t.td, t.th, t.tw, S, FLAT>), grid, dim3(256), 0, st, a);
}

// Workgroups the workspace is sized for: an upper bound of hdf_cu_budget() (at most 256) times the 2 small-channel blocks
// a conv_wgrad_s2 workgroup may own (the size query does not know the storage type, so it counts pairs of single blocks),
// with room to spare -- the workspace never limits G on this chip; the cap below does, on the 512 x 512 layers.
constexpr int WGRAD_WS_WORKGROUPS = 1024;

}  // namespace

size_t hdf_wgrad_workspace_bytes(int stride, int N, int Ds, int Hs, int Ws, int SC, int LC) {
  int SCp = round_up(SC, 32), LCp = round_up(LC, 32);
  int64_t per = (int64_t)27 * SCp * LCp * sizeof(float);
  int pairs = (SCp / 32) * (LCp / 32);
  int tiles = wgrad_num_tiles(wgrad_tile(stride, Ds == 1), N, Ds, Hs, Ws);
  int G = std::min(ceil_div(WGRAD_WS_WORKGROUPS, pairs), tiles);
  int64_t bytes = std::min<int64_t>((int64_t)G * per, std::max<int64_t>(per, (int64_t)96 << 20));
  return (size_t)bytes;
}

// the launches conv_wgrad2_kernel<., ., true> serves: conv_wgrad2's, with all of the fused pass's operands, 16-byte rows on
// both extra tensors, and 32-bit byte offsets into them with bit 31 free for the out-of-range marker
bool hdf_wgrad_apply_takes(int dtype, int stride, const WgradArgs& a) {
  if (wgrad_route(dtype, stride, a).kernel != WgradKernel::wgrad2 || !a.ap_y || !a.ap_out) return false;
  for (int k = 0; k < 7; k++)
    if (!a.ap_tab[k]) return false;
  const int64_t vox = (int64_t)a.N * a.Ds * a.Hs * a.Ws;
  if (vox * a.ap_y_pitch * 2 >= (1ll << 31) || vox * a.ap_out_pitch * 2 >= (1ll << 31)) return false;
  if (a.ap_y_pitch % 8 || a.ap_out_pitch % 8 || a.SC % 16) return false;
  if ((reinterpret_cast<uintptr_t>(a.ap_y) | reinterpret_cast<uintptr_t>(a.ap_out)) & 15) return false;
  return a.Ds == a.Dl && a.Hs == a.Hl && a.Ws == a.Wl;
}

int hdf_launch_wgrad(int dtype, int stride, WgradArgs a, float* dw, int sc_store, int lc_store, int accumulate, void* ws,
                     size_t ws_bytes, hipStream_t st) {
  HDF_CHECK_ARG(a.SC % 16 == 0 && a.LC % 16 == 0, "wgrad: channel counts must be multiples of 16 (SC=%d LC=%d)", a.SC,
                a.LC);
  HDF_CHECK_ARG(stride == 1 || stride == 2, "wgrad: stride %d", stride);
  HDF_CHECK_ARG(!a.ap_y || hdf_wgrad_apply_takes(dtype, stride, a),
                "wgrad: the fused InstanceNorm backward does not take this launch (ask hdf_wgrad_apply_takes first)");
  if (dtype != HDF_BF16 && dtype != HDF_F16 && dtype != HDF_F32) {
    hdf_set_error("unsupported dtype %d", dtype);
    return HDF_ERR_UNSUPPORTED;
  }
  const bool flat = a.Ds == 1;  // depth-1 operands: the 2-D weight gradients (Conv2d / ConvTranspose2d, models/HDenseFormer_2D.py)
  HDF_CHECK_ARG(!flat || (a.Dl == 1 && !a.ap_y), "wgrad: depth-1 small operand selects the 2-D operator (large operand of depth 1, no fused InstanceNorm backward)");
  const WgradRoute r = wgrad_route(dtype, stride, a);
  a.SCp = round_up(a.SC, 32);
  a.LCp = round_up(a.LC, 32);
  a.num_tiles = wgrad_num_tiles(r.tile, a.N, a.Ds, a.Hs, a.Ws);
  const int sblocks = ceil_div(a.SCp / 32, r.sb);
  const int pairs = sblocks * (a.LCp / 32);
  const int64_t per = (int64_t)27 * a.SCp * a.LCp * sizeof(float);
  const int wg_target = hdf_cu_budget();  // one workgroup per CU
  int G = ceil_div(wg_target, pairs);
  G = (int)std::min<int64_t>(G, std::max<int64_t>(1, (int64_t)ws_bytes / per));
  G = std::min(G, a.num_tiles);
  a.tiles_per_group = ceil_div(a.num_tiles, G);
  G = ceil_div(a.num_tiles, a.tiles_per_group);
  HDF_CHECK_ARG((size_t)(G * per) <= ws_bytes, "wgrad workspace too small: need %lld have %zu", (long long)(G * per),
                ws_bytes);
  a.partials = reinterpret_cast<float*>(ws);
  const dim3 grid(G, sblocks, a.LCp / 32);
  if (r.kernel == WgradKernel::s2) {
    HDF_TRY(hdf_launch_wgrad_s2(dtype, a, r.sb, grid, st));
  } else if (r.kernel == WgradKernel::wgrad2) {
    HDF_TRY(hdf_launch_wgrad2(dtype, a, grid, st));
  } else {
    HDF_DISPATCH_T(dtype, {
      if (flat && stride == 1)
        launch_wgrad_generic<T, 1, true>(a, grid, st);
      else if (flat)
        launch_wgrad_generic<T, 2, true>(a, grid, st);
      else if (stride == 1)
        launch_wgrad_generic<T, 1, false>(a, grid, st);
      else
        launch_wgrad_generic<T, 2, false>(a, grid, st);
    });
    HDF_LAUNCH_CHECK();
  }
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

