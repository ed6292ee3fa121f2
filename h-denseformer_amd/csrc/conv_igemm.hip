// Implicit-GEMM 3x3x3 convolution family on the gfx950 matrix cores.
//
// One kernel template covers
//   mode 0  Conv3d(k3,s1,p1)            -- forward of BasicConv3d / UpConv convs (HDenseFormer.py:151,167)
//                                          and, with flipped+transposed packed weights, their dgrad
//   mode 1  Conv3d(k3,s2,p1) gather     -- dgrad of ConvTranspose3d(k3,s2,p1,op1)   (HDenseFormer.py:211,215,219)
//   mode 2  ConvTranspose3d(k3,s2,p1,op1) forward, one launch z-slice per output parity class
// This file: conv_igemm_kernel, the weights-stationary persistent conv_ws2_kernel of the high-resolution stride-1 layers, and
// the routing of a launch (launch_conv_t).  The specialised stride-2 kernels live in conv_s2.hip, the weight gradients in
// conv_wgrad.hip (routing, generic kernel) with conv_wgrad2.hip / conv_wgrad_s2.hip (the 16-bit kernels), the weight packers in conv_pack.hip, the weights-in-registers stride-1 form in conv_wr.hip.
//
// Data layout: activations are channels-last (NDHWC) with an explicit voxel pitch, storage bf16 or
// f32.  GEMM view: M = output voxels of a 3-D tile, N = output channels, K = taps x input channels.
// A workgroup (4 waves) stages the input halo box of its tile in LDS, 64 bytes of channels per
// voxel row (32 bf16 / 16 f32) padded to an 80-byte pitch (conflict-free for ds_read_b128), applies
// the producer's InstanceNorm+ReLU on the way in (so normalised activations are never written to
// HBM), then walks taps x channel chunks issuing v_mfma_f32_32x32x16_bf16 (bf16 storage) or
// v_mfma_f32_32x32x2_f32 (f32 storage: exact fp32 fma chains, the parity path).  The epilogue adds
// bias, stores the raw conv output once and emits per-tile (sum, sum^2) partials for the following
// InstanceNorm, reduced deterministically by in_finalize (no float atomics).
#include "conv_igemm.h"
#include "conv_tile.h"
#include <type_traits>

namespace {

// ------------------------------------------------------------------------------------------------
// forward-style kernel (modes 0,1,2)
// FLAT (round 6): the 2-D operators of models/HDenseFormer_2D.py (Conv2d k3, ConvTranspose2d k3 s2 p1 op1 and its data
// gradient) on tensors of depth 1 -- TD = 1 tiles, only the 9 taps of the centre depth plane of the [27][CoutP][Cin] panel
// (a Conv2d kernel sits on depth tap 1 of the Conv3d panel: plan.hip "2-D embedding"), a one-plane box, and a depth axis
// that is never strided (stride-2 gather and transposed conv stride y and x only: 4 output-parity classes, not 8).  For the
// stride-1 conv this is exactly the 3-D operator on a depth-1 volume (the other 18 taps meet zero padding only).
template <typename T, int TD, int TH, int TW, int WM, int WN, int MB, int S, bool CONVT, bool FLAT = false>
// (256, 2): two workgroups per compute unit.  Left to itself hipcc let the big-tile instantiations grow past 256 registers
// (276 for the 256-voxel x 64-channel tile: one workgroup per unit, nobody to run while a workgroup stages its next channel
// chunk); with the bound it fits them into 178-201 without scratch.  Same-box pairs (round 6, call c37): bench step -0.09 ms
// (4 of 4), the 2-D PI-CAI step 16.8 -> 15.95 ms.
// The flat (2-D) stride-1 instantiations take three (<= 168 registers, no scratch; their step -0.1 ms of 15.9; the stride-2
// gather would spill); for the 3-D ones three cost the
// bench step +0.07 ms (call c38).
__global__ __launch_bounds__(256, (FLAT && S == 1) ? 3 : 2) void conv_igemm_kernel(ConvArgs a) {
  if (a.prio) HDF_LIGHT_PRIO();
  static_assert(WM * WN == 4, "4 waves");
  static_assert(WM * MB * 32 == TD * TH * TW, "tile/wave decomposition");
  static_assert(!FLAT || TD == 1, "flat tiles are one voxel deep");
  constexpr int BD = FLAT ? 1 : (CONVT ? TD + 1 : S * (TD - 1) + 3);
  constexpr int BH = CONVT ? TH + 1 : S * (TH - 1) + 3;
  constexpr int BW = CONVT ? TW + 1 : S * (TW - 1) + 3;
  constexpr int SS = CONVT ? 1 : S;
  constexpr int ESZ = sizeof(T);
  __shared__ __attribute__((aligned(16))) char lds[BD * BH * BW * PITCH + 4 * 32 * 2 * 4];
  float* s_red = reinterpret_cast<float*>(lds + BD * BH * BW * PITCH);  // [WN*32][2]

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int wm = wave / WN, wn = wave % WN;

  // tile space: output voxels (conv) or input voxels m (convT)
  const int Td = CONVT ? a.Di : a.Do, Th = CONVT ? a.Hi : a.Ho, Tw = CONVT ? a.Wi : a.Wo;
  const int ntz = (Td + TD - 1) / TD, nty = (Th + TH - 1) / TH, ntx = (Tw + TW - 1) / TW;
  int t = blockIdx.x;
  const int tx = t % ntx;
  t /= ntx;
  const int ty = t % nty;
  t /= nty;
  const int tz = t % ntz;
  const int n = t / ntz;
  const int z0 = tz * TD, y0 = ty * TH, x0 = tx * TW;
  const int n_base = blockIdx.y * (WN * 32) + wn * 32;
  const int cls = CONVT ? blockIdx.z : 0;
  const int pz = FLAT ? 0 : (cls >> 2) & 1, py = (cls >> 1) & 1, px = cls & 1;
  const int ntapz = FLAT ? 1 : (CONVT ? (pz ? 2 : 1) : 3), ntapy = CONVT ? (py ? 2 : 1) : 3, ntapx = CONVT ? (px ? 2 : 1) : 3;

  const int oz = (CONVT || FLAT) ? z0 : S * z0 - 1, oy = CONVT ? y0 : S * y0 - 1, ox = CONVT ? x0 : S * x0 - 1;

  // MFMA row -> tile voxel.  Tile order (32 consecutive voxels per M-block) put the 16 lanes of a ds_read_b128 service
  // group (conv_tile.h: ds128_group) on box rows that repeat mod 16 -- with the 80-byte pitch that is the same 16-byte
  // bank slot up to three times (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.66 in every round's kernel table: the A
  // fragment reads of this kernel took 3x their LDS cycles).  Where the tile shape allows it the M-block is a slab whose
  // groups see 16 distinct rows mod 16:
  //  ZXMAP (8-wide tiles 4 deep, stride 1): M-block = one y, rows -> (z, x) as in conv_ws2_kernel (a group = z {0,2} or
  //        {1,3}: 2 BH BW = 8 mod 16 for BH BW = 100 and 60)
  //  YXMAP (flat 16-wide tiles): M-block = two y rows, one whole x row of 16 per group
  // Which voxel an accumulator row stands for changes nothing in a voxel's own arithmetic; only the order in which the
  // InstanceNorm partial sums of a workgroup add their voxels moves.
  constexpr bool ZXMAP = !CONVT && !FLAT && S == 1 && TD == 4 && TW == 8 && WM * MB == TH && (2 * BH * BW) % 16 == 8;
  constexpr bool YXMAP = FLAT && SS == 1 && TW == 16 && 2 * WM * MB == TH;
  auto mrow_voxel = [](int mblk, int row, int& lz, int& ly, int& lx) {
    if constexpr (ZXMAP) {
      ws_row_to_zx(row, lz, lx);
      ly = mblk;
    } else if constexpr (YXMAP) {
      int g2;
      ds128_group(row, g2, lx);
      lz = 0;
      ly = 2 * mblk + g2;
    } else {
      const int lin = mblk * 32 + row;
      lz = lin / (TH * TW), ly = (lin / TW) % TH, lx = lin % TW;
    }
  };
  int rowbase[MB];
#pragma unroll
  for (int mb = 0; mb < MB; mb++) {
    int lz, ly, lx;
    mrow_voxel(wm * MB + mb, r, lz, ly, lx);
    rowbase[mb] = (((FLAT ? 0 : SS * lz)) * BH + SS * ly) * BW + SS * lx;
  }
  const bool n_active = n_base < a.CoutP;  // wave-uniform
  const char* wrow = reinterpret_cast<const char*>(a.w) + ((int64_t)(n_base + r) * a.Cin) * ESZ + h * 16;
  const int64_t wtap_stride = (int64_t)a.CoutP * a.Cin * ESZ;
  const int chunk_elems_max = 64 / ESZ;

  // weight fragment addressing: row-major panels [27][CoutP][Cin] or fragment-major (a.wfrag, see below)
  const char* const wfr = a.wfrag ? reinterpret_cast<const char*>(a.w) +
                                        (int64_t)(n_base >> 5) * ((a.Cin * ESZ) >> 5) * 1024 + r * 32 + h * 16
                                  : wrow;
  const int cstride = a.wfrag ? 2048 : 64, fstride = a.wfrag ? 1024 : 32;  // per 64-byte chunk / per 32-byte step

  bool done = false;
  f32x16 acc[MB];
#pragma unroll
  for (int mb = 0; mb < MB; mb++)
#pragma unroll
    for (int i = 0; i < 16; i++) acc[mb][i] = 0.f;
  if constexpr (!CONVT) {
    // Conv (stride 1 or the stride-2 gather) with whole 64-byte channel chunks: the 27 taps x 2 fragment steps of a chunk are unrolled and
    // software-pipelined.  The weight fragments come straight from L2 (~500+ cycles): a register ring keeps RING
    // steps of them in flight, across chunk boundaries too (the loads of the next chunk's first steps are issued
    // before its box is staged); the A fragments of step s+1 are read from LDS under the MFMAs of step s.  The
    // plain loop below waited for one L2 round trip per step, which at the low resolutions (one or two workgroups
    // per CU, nothing to switch to) left the matrix pipe idle 70-90 % of the time.
    if ((a.Cin * ESZ) % 64 == 0) {
      constexpr int NS = FLAT ? 18 : 54;           // fragment steps per chunk (taps x 2)
      constexpr int TAP0 = FLAT ? 9 : 0;           // first tap of the panel this kernel uses (flat: the centre depth plane)
      constexpr int V1_RING_BIG = 6, V1_RING_SMALL = 9;
      constexpr int RING = (MB >= 4) ? V1_RING_BIG : V1_RING_SMALL;  // divides 54: the ring position is the same in every chunk
      const int nchunk_all = a.Cin * ESZ / 64;
      // split-K (a.ksplit > 1: low-resolution layers with fewer tiles than CUs): this workgroup contracts chunks
      // [c_lo, c_hi) and leaves an fp32 partial tile to conv_ksplit_reduce_kernel
      const int kz = a.ksplit > 1 ? (int)blockIdx.z : 0;
      const int c_lo = a.ksplit > 1 ? kz * (nchunk_all / a.ksplit) : 0;
      const int nchunk = a.ksplit > 1 ? c_lo + nchunk_all / a.ksplit : nchunk_all;
      u32x4 bq[RING];
      // fragment-major panels (a.wfrag, see hdf_conv_weight_layout): the 32 rows x 32 B of one fragment step are one
      // contiguous 1 KB block, steps of a row follow each other, then the next 32-channel block; a tap plane has
      // the same size in both layouts.  With row-major panels a fragment load touched 32 cache lines for 1 KB and
      // the vector cache's line rate, not latency, bounded the low-resolution layers.
      auto b_load = [&](int chunk, int s_) -> u32x4 {
        const int tap = TAP0 + (s_ >> 1), fs = s_ & 1;
        const char* p = wfr + tap * wtap_stride + (int64_t)chunk * cstride + fs * fstride;
        return *reinterpret_cast<const u32x4*>(n_active ? p : reinterpret_cast<const char*>(a.w));
      };
      auto a_off = [&](int s_) {
        const int tap = s_ >> 1, fs = s_ & 1;   // (flat: tap = 3 ky + kx in the one staged plane)
        return ((tap / 9 * BH + (tap / 3) % 3) * BW + tap % 3) * PITCH + h * 16 + fs * 32;
      };
#pragma unroll
      for (int k = 0; k < RING; k++) bq[k] = b_load(c_lo, k);
      for (int chunk = c_lo; chunk < nchunk; chunk++) {
        if (chunk > c_lo) __syncthreads();
        stage_box<T, BD, BH, BW, 64, PITCH>(lds, reinterpret_cast<const T*>(a.in), a.in_pitch, a.Cin, n, a.Di, a.Hi,
                                            a.Wi, oz, oy, ox, chunk * chunk_elems_max, 64, a.in_scale, a.in_shift,
                                            a.in_relu);
        __syncthreads();
        u32x4 af[2][MB];
#pragma unroll
        for (int mb = 0; mb < MB; mb++) af[0][mb] = *reinterpret_cast<const u32x4*>(lds + rowbase[mb] * PITCH + a_off(0));
        const bool more = chunk + 1 < nchunk;
#pragma unroll
        for (int s_ = 0; s_ < NS; s_++) {
          if (s_ + 1 < NS) {
#pragma unroll
            for (int mb = 0; mb < MB; mb++)
              af[(s_ + 1) & 1][mb] = *reinterpret_cast<const u32x4*>(lds + rowbase[mb] * PITCH + a_off(s_ + 1));
          }
          const u32x4 bcur = bq[s_ % RING];
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int mb = 0; mb < MB; mb++) Mma<T>::run(af[s_ & 1][mb], bcur, acc[mb]);
          // refill the slot just consumed: RING steps ahead, in this chunk or the next one
          if (s_ + RING < NS)
            bq[s_ % RING] = b_load(chunk, s_ + RING);
          else if (more)
            bq[s_ % RING] = b_load(chunk + 1, s_ + RING - NS);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      done = true;
    }
  }
  for (int c0 = 0; !done && c0 < a.Cin; c0 += chunk_elems_max) {
    const int chunk_elems = min(chunk_elems_max, a.Cin - c0);
    const int row_bytes = chunk_elems * ESZ;  // 64 or 32
    if (c0 > 0) __syncthreads();
    stage_box<T, BD, BH, BW, 64, PITCH>(lds, reinterpret_cast<const T*>(a.in), a.in_pitch, a.Cin, n, a.Di, a.Hi, a.Wi,
                                        oz, oy, ox, c0, row_bytes, a.in_scale, a.in_shift, a.in_relu);
    __syncthreads();
    if (n_active) {
      const int nfs = row_bytes >> 5;  // fragment steps (32 B each) in this chunk
      for (int jz = 0; jz < ntapz; jz++) {
        const int offz = FLAT ? 0 : (CONVT ? (pz ? 1 - jz : 0) : jz), wz = FLAT ? 1 : (CONVT ? (pz ? 2 * jz : 1) : jz);
        for (int jy = 0; jy < ntapy; jy++) {
          const int offy = CONVT ? (py ? 1 - jy : 0) : jy, wy = CONVT ? (py ? 2 * jy : 1) : jy;
#pragma unroll
          for (int jx = 0; jx < 3; jx++) {
            if (jx < ntapx) {
              const int offx = CONVT ? (px ? 1 - jx : 0) : jx, wx = CONVT ? (px ? 2 * jx : 1) : jx;
              const int tapoff = ((offz * BH + offy) * BW + offx) * PITCH + h * 16;
              const char* wp = wfr + ((wz * 3 + wy) * 3 + wx) * wtap_stride + (int64_t)(c0 * ESZ / 64) * cstride;
              for (int fs = 0; fs < nfs; fs++) {
                u32x4 bfrag = *reinterpret_cast<const u32x4*>(wp + fs * fstride);
                u32x4 afrag[MB];
#pragma unroll
                for (int mb = 0; mb < MB; mb++)
                  afrag[mb] = *reinterpret_cast<const u32x4*>(lds + rowbase[mb] * PITCH + tapoff + fs * 32);
#pragma unroll
                for (int mb = 0; mb < MB; mb++) Mma<T>::run(afrag[mb], bfrag, acc[mb]);
              }
            }
          }
        }
      }
    }
  }

  // ------------------------------------------------------------------------------- epilogue
  const int ch = n_base + r;
  if constexpr (!CONVT) {
    if (a.ksplit > 1) {  // fp32 partial tile [split][voxel][CoutP]: bias, storage rounding and statistics in the reduce pass
      if (n_active) {
        const int64_t mtot = (int64_t)a.N * a.Do * a.Ho * a.Wo;
#pragma unroll
        for (int mb = 0; mb < MB; mb++) {
#pragma unroll
          for (int i = 0; i < 16; i++) {
            const int row = (i & 3) + 8 * (i >> 2) + 4 * h;
            int lz, ly, lx;
            mrow_voxel(wm * MB + mb, row, lz, ly, lx);
            const int gz = z0 + lz, gy = y0 + ly, gx = x0 + lx;
            if (gz < Td && gy < Th && gx < Tw)
              a.kpart[((int64_t)blockIdx.z * mtot + (((int64_t)n * a.Do + gz) * a.Ho + gy) * a.Wo + gx) * a.CoutP + ch] =
                  acc[mb][i];
          }
        }
      }
      return;
    }
  }
  const bool ch_ok = n_active && ch < a.Cout;
  const float bias = (a.bias && ch_ok) ? a.bias[ch] : 0.f;
  float s1 = 0.f, s2 = 0.f;
  // split output: this wave's 32-channel block lies entirely on one side (split is a multiple of 32)
  T* outp = (a.split && n_base >= a.split) ? reinterpret_cast<T*>(a.out2) - a.split : reinterpret_cast<T*>(a.out);
#pragma unroll
  for (int mb = 0; mb < MB; mb++) {
    // an accumulating launch requests the 16 old values of this row block together (one 2-byte load at a time behind
    // the bounds branch doubled the launch: 82 vs 40 us for the 64 -> 128 conv at 32^3)
    float old[16];
    if (a.accumulate) {
#pragma unroll
      for (int i = 0; i < 16; i++) {
        int row = (i & 3) + 8 * (i >> 2) + 4 * h;
        int lz, ly, lx;
        mrow_voxel(wm * MB + mb, row, lz, ly, lx);
        int gz = z0 + lz, gy = y0 + ly, gx = x0 + lx;
        const bool ok = ch_ok && gz < Td && gy < Th && gx < Tw;
        int qz = (CONVT && !FLAT) ? 2 * gz + pz : gz, qy = CONVT ? 2 * gy + py : gy, qx = CONVT ? 2 * gx + px : gx;
        const T* p = outp + ((((int64_t)n * a.Do + qz) * a.Ho + qy) * a.Wo + qx) * a.out_pitch + ch;
        old[i] = ST<T>::ld(ok ? p : outp);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; i++) old[i] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < 16; i++) {
      int row = (i & 3) + 8 * (i >> 2) + 4 * h;
      int lz, ly, lx;
      mrow_voxel(wm * MB + mb, row, lz, ly, lx);
      int gz = z0 + lz, gy = y0 + ly, gx = x0 + lx;
      if (ch_ok && gz < Td && gy < Th && gx < Tw) {
        int qz = (CONVT && !FLAT) ? 2 * gz + pz : gz, qy = CONVT ? 2 * gy + py : gy, qx = CONVT ? 2 * gx + px : gx;
        T* p = outp + ((((int64_t)n * a.Do + qz) * a.Ho + qy) * a.Wo + qx) * a.out_pitch + ch;
        float v = acc[mb][i] + bias + old[i];
        ST<T>::st(p, v);
        s1 += v;
        s2 += v * v;
      }
    }
  }
  if (a.stat_partials) {
    // lanes r and r+32 hold the same channel (different rows): fold, then reduce over the WM waves
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 32, 64);
    __syncthreads();
    if (h == 0) {  // one slot per wave, summed below in a fixed order: bitwise reproducible statistics
      s_red[((wm * WN + wn) * 32 + r) * 2 + 0] = s1;
      s_red[((wm * WN + wn) * 32 + r) * 2 + 1] = s2;
    }
    __syncthreads();
    if (threadIdx.x < WN * 32) {
      int c = blockIdx.y * (WN * 32) + threadIdx.x;
      if (c < a.CoutP) {
        float t1 = 0.f, t2 = 0.f;
#pragma unroll
        for (int k = 0; k < WM; k++) {
          t1 += s_red[(k * WN * 32 + threadIdx.x) * 2 + 0];
          t2 += s_red[(k * WN * 32 + threadIdx.x) * 2 + 1];
        }
        float* q = a.stat_partials + ((int64_t)blockIdx.x * a.CoutP + c) * 2;
        q[0] = t1;
        q[1] = t2;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------------
// conv_ws2: weights-stationary persistent kernel with a DOUBLE-BUFFERED activation tile.
//
// One wave per SIMD leaves nothing to hide the staging work behind, and in the single-buffered predecessor of this
// kernel (round-1 conv_ws_kernel, see git history) the commit (global ->
// InstanceNorm/ReLU transform -> LDS), the bounds logic and the prefetch issue cost as many cycles as the MFMAs.
// Here a pass over item i (= one 4x8x8 tile x one CH-byte channel chunk) reads tile buffer i&1 while the SAME
// instruction stream, in the gaps between its MFMAs, transforms and writes item i+1 into the other buffer and
// re-loads the freed registers with item i+2: one workgroup barrier per pass, staging under the MFMAs.
//  * unpadded rows (pitch == CH) + XOR swizzle of the 16-byte slots keep both buffers and the whole weight
//    panel (27 x 32 x RB bytes) inside 160 KiB; a_swz makes every ds_read_b128 lane group conflict-free
//  * a wave owns the M-blocks y = 2w, 2w+1: the A fragment of box row y' serves (mb, jy) with mb + jy == y', so a
//    (jz, jx) group issues 4 A + 3 B fragment reads for 6 MFMAs (one fragment pair per MFMA: 9 reads)
//  * the NCH passes of a tile are unrolled inside one "tile phase": chunk indices, buffer parities and the
//    accumulators' lifetime are compile-time, tile coordinates advance incrementally once per tile (every
//    instruction outside the MFMA shadow costs ~5 cycles with one wave per SIMD), scale/shift sit in an LDS table
//  * epilogue: accumulators (+bias) -> storage type -> element stores (32 lanes = one voxel row of 32 channels), no
//    LDS staging and no barrier; the cross-wave reduction of the InstanceNorm partials rides on the next pass's
//    barrier
//  * schedule: an interior pass (unchecked copy of the phase) then a border pass (checked copy) per workgroup, both
//    split XCD-aware (see the kernel body)
template <int CH>
__device__ __forceinline__ int a_swz(int row) {
  return CH == 64 ? ((row >> 2) & 3) : ((row >> 3) & 1);
}

// NB: 32-channel output blocks per workgroup.  NB = 2 (64-byte rows, Cout % 64 == 0) stages every tile once for both
// blocks (two workgroups with 32 channels each staged it twice: the 32->64 dgrad at 128^3 was the costliest launch of
// the step) and shares each A fragment between two MFMAs.
// (An LDS-DMA staging variant of the transform-free 32-byte-chunk layers -- global_load_lds_dwordx4 instead of the pf
// registers and ds_write commits -- was built at the end of round 2, measured neutral (536 vs 539 us) and removed in
// round 3: DESIGN.md section 6d.)
// TDP (round 6): tile depth, 4 or 8.  TDP = 8 -- an 8x8x8 tile, taken by the 64-byte-row single-block layers (32 -> 32
// channels at the top level: the four launches of a step that are co-bound by HBM and MFMA, VERDICT r05 #1a) -- stages a
// 10x10x10 box for 512 outputs instead of 6x10x10 for 256: 1.95 instead of 2.34 box voxels per output through L2 ->
// registers -> LDS, the z halo fetched 1.25x instead of 1.5x, 8 A + 3 B fragment reads per 12 MFMAs instead of 4 + 3 per
// 6, one epilogue / barrier / tile step per 108 MFMAs instead of per 54.  A wave then owns four M-blocks (z half zh, row
// mb): MFMA row -> (dz + 4 zh, x) with the same ws_row_to_zx map, so the fragment addresses of z half 1 are those of half
// 0 plus a compile-time offset.  Needs the padded tile-buffer layout (two 1000-row buffers + the panel: 150 KiB).
template <typename T, int CH, int RB, bool XF, int NB, bool BS = false, int TDP = 4>
__global__ __launch_bounds__(256) void conv_ws2_kernel(ConvArgs a) {
  if (a.prio) HDF_LIGHT_PRIO();
  constexpr int TD = TDP, ZH = TDP / 4, TH = 8, TW = 8, BD = TD + 2, BH = TH + 2, BW = TW + 2, BOX = BD * BH * BW;
  static_assert(TDP == 4 || TDP == 8, "tile depth");
  constexpr int ESZ = sizeof(T), EPC = ST<T>::EPC;
  constexpr int CIN = RB / ESZ;
  constexpr int NCH = RB / CH, NFS = CH / 32, NG = 9 * NFS;
  constexpr int CPV = CH / 16, CPV_SHIFT = (CPV == 4) ? 2 : 1;
  constexpr int TOTAL = BOX * CPV, NJ = (TOTAL + 255) / 256;
  // tile-buffer row pitch: padded by 16 bytes (conflict-free, see ws_row_to_zx; fragment addresses = one lane
  // base + compile-time offsets) whenever two padded buffers and the weight panel fit in 160 KiB; else unpadded
  // rows with XOR-swizzled 16-byte slots (a 36-entry per-lane address table)
  constexpr bool SWZ = (2 * BOX * (CH + 16) + 4096 + 512 + 27 * 32 * NB * RB > 160 * 1024);
  constexpr int AP = SWZ ? CH : CH + 16;
  constexpr int ABUF = BOX * AP;
  constexpr int OFF_RED = 2 * ABUF, OFF_XF = OFF_RED + 2048 * NB, OFF_W = OFF_XF + 512;
  constexpr int NC = 32 * NB;  // output channels of the workgroup
  constexpr int CPR = RB / 16, RP256 = 16 / CPR;
  static_assert(CH == 32 || CH == 64, "chunk bytes");
  static_assert(NCH == 1 || NCH % 2 == 0, "buffer parity at tile start must be compile-time");
  static_assert(2 * CIN * 4 <= 512, "scale/shift table");
  static_assert(OFF_W + 27 * NC * RB <= 160 * 1024, "LDS budget");
  static_assert(ZH == 1 || !SWZ, "the 8-deep tile needs the padded layout");
  __shared__ __attribute__((aligned(256))) char lds[OFF_W + 27 * NC * RB];
#ifdef WS_DBG_STAMPS
  const unsigned long long t_entry = __builtin_amdgcn_s_memrealtime();
#endif
  char* const a_lds = lds;
  float* const s_red = reinterpret_cast<float*>(lds + OFF_RED);  // [2 halves][4 waves][NC][2]
  float* const s_xf = reinterpret_cast<float*>(lds + OFF_XF);
  char* const w_lds = lds + OFF_W;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int n0 = blockIdx.y * NC;
  const int part = tid & (CPV - 1);
  constexpr bool xf = XF;  // input transform x*scale+shift (+relu) on the way into LDS; else a plain copy
  const float relu_lo = (xf && a.in_relu) ? 0.f : -INFINITY;

  // ---- weights -> LDS, once (rows [tap][cout 32][RB bytes], 16-byte slots XOR-swizzled by row).  ALL of a thread's
  // loads are issued before its first LDS store: written as load / store pairs in a loop, hipcc waited for every load
  // in turn (s_waitcnt vmcnt(0) in front of each ds_write), and with all 256 workgroups asking the same L2 lines for
  // the same rows at the same moment one round trip took ~1.6 us -- 27 of them in a row were 45-55 us of a 480 us
  // launch (real-time stamps: 575 us per launch against 520 us from the first to the last instruction after this loop).
  // The batches start at a different 4 KB slice per workgroup so the requests of a round spread over the L2 channels.
  {
    constexpr int WTOT = 27 * NC * CPR, WIT = (WTOT + 255) / 256;
    u32x4 wv[WIT];
    const int rot = blockIdx.x % WIT;
#pragma unroll
    for (int u = 0; u < WIT; u++) {
      int it = u + rot;
      it -= (it >= WIT) ? WIT : 0;
      const int id = min(tid + 256 * it, WTOT - 1);
      const int row = id / CPR, ch = id - row * CPR;
      const int tap = row / NC, rr = row - tap * NC;
      wv[u] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(a.w) +
                                             ((int64_t)(tap * a.CoutP + n0 + rr) * CIN) * ESZ + ch * 16);
    }
#pragma unroll
    for (int u = 0; u < WIT; u++) {
      int it = u + rot;
      it -= (it >= WIT) ? WIT : 0;
      const int id = tid + 256 * it;
      const int row = id / CPR, ch = id - row * CPR;
      const int sw = ch ^ ((row / RP256) & (CPR - 1));
      if (id < WTOT) *reinterpret_cast<u32x4*>(w_lds + row * RB + sw * 16) = wv[u];
    }
  }
  const int bswz = (r / RP256) & (CPR - 1);

  // (This kernel keeps its OWN COPY of the schedule that conv_wgrad2_kernel and conv_wr_kernel take from
  // conv_schedule.h (WsSchedule): through the header five of its forms spilled one or two more scalar registers, under
  // every spelling of the header that was tried.  A change of the schedule is made there AND here;
  // tests/test_gpu_tile_schedule.py holds both to the same results.)
  // Tile schedule: every workgroup first runs a contiguous share of the INTERIOR tiles (halo box inside the volume:
  // no bounds logic, one long run inside the hot copy of the phase), then a share of the
  // BORDER tiles with the checked copy.  Walking all tiles in raster order switched between the copies at every
  // x-row (two border tiles per 16), and each switch re-fetched cold code and drained the staging pipeline.
  const int ntz = (a.Do + TD - 1) / TD, nty = (a.Ho + TH - 1) / TH, ntx = (a.Wo + TW - 1) / TW;
  const bool has_int = ntz >= 3 && nty >= 3 && ntx >= 3;
  const int ipz = ntz - 2, ipy = nty - 2, ipx = ntx - 2;                // interior tile grid per sample
  const int n_int = has_int ? a.N * ipz * ipy * ipx : 0;
  const int per_all = ntz * nty * ntx, per_bor = per_all - (has_int ? ipz * ipy * ipx : 0);
  const int n_bor = a.N * per_bor;
  // XCD-aware split: workgroup b runs on XCD b % 8 (round-robin dispatch), and each XCD has its own 4 MiB L2.  XCD x
  // owns the x-th eighth of the raster-ordered tile list and its G/8 workgroups walk that range interleaved (tile
  // r0 + slot, + G/8, ...): at any moment the XCD works on ~G/8 consecutive tiles, so the halo planes neighbouring
  // tiles share are fetched from HBM once and hit in that L2 (a contiguous chunk per workgroup re-fetched them:
  // FETCH_SIZE 2.8x the input).
  const int G = gridDim.x;
  const int NX = (G % 8 == 0) ? 8 : 1;  // ranges
  const int WPX = G / NX;               // workgroups per range = stride of a workgroup inside its range
  const int xcd = blockIdx.x % NX, slot = blockIdx.x / NX;
  auto split = [&](int total, int& begin, int& cnt) {
    const int r0 = (int)((int64_t)total * xcd / NX), r1 = (int)((int64_t)total * (xcd + 1) / NX);
    begin = r0 + slot;
    cnt = (r1 - r0 > slot) ? (r1 - r0 - slot + WPX - 1) / WPX : 0;
  };
  int int_begin, int_cnt, bor_begin, bor_cnt;
  split(n_int, int_begin, int_cnt);
  split(n_bor, bor_begin, bor_cnt);
  if (int_cnt + bor_cnt == 0) return;
  // mixed-radix digits of the stride WPX over the interior tile grid (x, y, z, n): int_next adds them with carries
  int sdx = 0, sdy = 0, sdz = 0, sdn = 0;
  if (has_int) {
    int t = WPX;
    sdx = t % ipx, t /= ipx;
    sdy = t % ipy, t /= ipy;
    sdz = t % ipz, sdn = t / ipz;
  }

  // ---- per-lane constants
  // fragment read addresses: [jz][y'][jx] -> byte offset of this lane's 16-byte slot inside a tile buffer
  // (swizzled layout: a table; padded layout: abase + a compile-time offset)
  int aaddr[SWZ ? 3 : 1][SWZ ? 4 : 1][SWZ ? 3 : 1];
  int abase;
  {
    int dz, x;
    ws_row_to_zx(r, dz, x);
    abase = ((dz * BH + 2 * wave) * BW + x) * AP + h * 16;
    if constexpr (SWZ) {
#pragma unroll
      for (int jz = 0; jz < 3; jz++)
#pragma unroll
        for (int yp = 0; yp < 4; yp++)
#pragma unroll
          for (int jx = 0; jx < 3; jx++) {
            int row = ((dz + jz) * BH + 2 * wave + yp) * BW + x + jx;
            aaddr[jz][yp][jx] = row * CH + ((h ^ a_swz<CH>(row)) << 4);
          }
    }
  }
  auto a_addr = [&](int jz, int yp, int jx, int fs, int zh = 0) {
    if constexpr (SWZ)
      return aaddr[jz][yp][jx] ^ (fs * 32);
    else
      return abase + (((jz + 4 * zh) * BH + yp) * BW + jx) * AP + fs * 32;
  };
  int bvar[NCH];  // this lane's 16-byte slot inside a weight row, per channel chunk
#pragma unroll
  for (int c = 0; c < NCH; c++) bvar[c] = r * RB + (((c * CPV + h) ^ bswz) << 4);
  // staging slots of this thread: source element offset, packed box coordinates, LDS byte offset
  int boff[NJ], bxyz[NJ], woff_t[SWZ ? NJ : 2];
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    // threads past the end of the last slot redo the box's last voxel (same part): identical bytes to the same
    // address, so neither the load nor the LDS write needs a predicate
    int vox = min(tid + 256 * j, TOTAL - CPV + part) >> CPV_SHIFT;
    int bz = vox / (BH * BW), rem = vox - bz * (BH * BW), by = rem / BW, bx = rem - by * BW;
    boff[j] = ((bz * a.Hi + by) * a.Wi + bx) * (int)a.in_pitch;
    bxyz[j] = (bz << 16) | (by << 8) | bx;
    if constexpr (SWZ) {
      woff_t[j] = vox * CH + ((part ^ a_swz<CH>(vox)) << 4);
    } else {  // slot j = slot 0 + 256/CPV voxels * j: a compile-time offset (the clamped last slot apart)
      if (j == 0) woff_t[0] = vox * AP + part * 16;
      if (j == NJ - 1) woff_t[1] = vox * AP + part * 16;
    }
  }
  auto woff = [&](int j) {
    if constexpr (SWZ)
      return woff_t[j];
    else
      return j == NJ - 1 ? woff_t[1] : woff_t[0] + j * (256 / CPV) * AP;
  };

  // linear index of a tile in raster order (the InstanceNorm partial row it owns)
  auto tile_lin = [&](const WsTile& c) { return ((c.n * ntz + c.z0 / TD) * nty + (c.y0 >> 3)) * ntx + (c.x0 >> 3); };
  // k-th interior tile / k-th border tile, in raster order
  auto int_init = [&](WsTile& c, int k) {
    int t = k;
    c.x0 = (t % ipx + 1) * TW;
    t /= ipx;
    c.y0 = (t % ipy + 1) * TH;
    t /= ipy;
    c.z0 = (t % ipz + 1) * TD;
    c.n = t / ipz;
    c.tile = tile_lin(c);
  };
  auto int_next = [&](WsTile& c) {  // + WPX tiles in raster order of the interior grid
    int xi = (c.x0 >> 3) - 1 + sdx, yi = (c.y0 >> 3) - 1 + sdy, zi = c.z0 / TD - 1 + sdz;
    c.n += sdn;
    if (xi >= ipx) xi -= ipx, yi++;
    if (yi >= ipy) yi -= ipy, zi++;
    if (zi >= ipz) zi -= ipz, c.n++;
    c.x0 = (xi + 1) * TW, c.y0 = (yi + 1) * TH, c.z0 = (zi + 1) * TD;
    c.tile = tile_lin(c);
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
    c.tile = tile_lin(c);
  };
  // border tiles are re-decoded from their list index (a few integer divisions per tile of the checked path)
  auto bor_next = [&](WsTile& c) { bor_init(c, c.k + WPX); };
  auto tile_interior = [&](const WsTile& c) {
    return c.z0 >= 1 && c.y0 >= 1 && c.x0 >= 1 && c.z0 + TD + 1 <= a.Di && c.y0 + TH + 1 <= a.Hi &&
           c.x0 + TW + 1 <= a.Wi;
  };
  const T* const src_safe = reinterpret_cast<const T*>(a.in) + part * EPC;
  // first box voxel of the tile (channel chunk 0, this thread's part); may lie outside the tensor for border tiles
  auto tile_org = [&](const WsTile& c) -> const T* {
    return src_safe + ((((int64_t)c.n * a.Di + (c.z0 - 1)) * a.Hi + (c.y0 - 1)) * a.Wi + (c.x0 - 1)) * a.in_pitch;
  };

  u32x4 pf[NJ];
  // box voxel of slot j inside the volume?  (border tiles only)
  auto slot_ok = [&](int j, const WsTile& c) {
    int iz = c.z0 - 1 + (bxyz[j] >> 16), iy = c.y0 - 1 + ((bxyz[j] >> 8) & 255), ix = c.x0 - 1 + (bxyz[j] & 255);
    return ((unsigned)iz < (unsigned)a.Di) & ((unsigned)iy < (unsigned)a.Hi) & ((unsigned)ix < (unsigned)a.Wi);
  };
  // loads are UNCONDITIONAL (clamped address + select): one load per slot on every path, so the compiler's
  // vmcnt bookkeeping stays exact and nothing ever branches around a load.
  // FAST: the tile is a valid interior tile (no test at all); else `inter` (uniform) short-cuts the test.
  auto load_one = [&](auto fast_tag, int j, int chunk, const WsTile& c, bool valid, bool inter, const T* org) {
    if constexpr (decltype(fast_tag)::value) {
      pf[j] = *reinterpret_cast<const u32x4*>(org + boff[j] + chunk * (CH / ESZ));
    } else {
      const bool ok = inter | (valid & slot_ok(j, c));  // bitwise: no short-circuit branches
      const T* p = ok ? org + boff[j] + chunk * (CH / ESZ) : src_safe;
      pf[j] = *reinterpret_cast<const u32x4*>(p);
    }
  };
  float sc[EPC], sh[EPC];
  auto read_xf = [&](int chunk) {
    const int cb = chunk * (CH / ESZ) + part * EPC;
#pragma unroll
    for (int e = 0; e < EPC; e += 4) {
      f32x4 u = *reinterpret_cast<const f32x4*>(s_xf + cb + e);
      f32x4 v = *reinterpret_cast<const f32x4*>(s_xf + CIN + cb + e);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        sc[e + k] = u[k];
        sh[e + k] = v[k];
      }
    }
  };
  // straight-line on purpose (no branch may split an MFMA group); relu_lo is -inf when there is no ReLU
  auto commit_one = [&](auto fast_tag, int j, const WsTile& c, bool inter, char* dst) {
    u32x4 v = pf[j];
    if constexpr (XF) {
      float f[EPC];
      ST<T>::unpack(v, f);
#pragma unroll
      for (int e = 0; e < EPC; e++) f[e] = fmaxf(f[e] * sc[e] + sh[e], relu_lo);
      v = ST<T>::pack(f);
    }
    if constexpr (!decltype(fast_tag)::value) {
      const bool ok = inter | slot_ok(j, c);
#pragma unroll
      for (int k = 0; k < 4; k++) v[k] = ok ? v[k] : 0u;
    }
    *reinterpret_cast<u32x4*>(dst + woff(j)) = v;
  };
  int tbl_n = -1;
  auto refresh_xf = [&](int n) {  // uniform; callers guarantee nobody still reads the old table
    if (tid < CIN) {
      s_xf[tid] = xf ? a.in_scale[(int64_t)n * CIN + tid] : 1.f;
      s_xf[CIN + tid] = xf ? a.in_shift[(int64_t)n * CIN + tid] : 0.f;
    }
    tbl_n = n;
    __syncthreads();
  };

  // T0: tile under the MFMAs, T1 / T2: the next two (T2 only feeds the loads when a tile is a single pass)
  WsTile T0, T1, T2;
  bool v1 = false, v2 = false, i0 = false, i1 = false, i2 = false;
  const T *org0 = src_safe, *org1 = src_safe, *org2 = src_safe;
  int left = 0;  // tiles of the current pass after T0
  // start a pass at its k-th tile: T0 -> buffer 0 (not overlapped), the next item -> registers
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
    i0 = BORDER ? tile_interior(T0) : true;
    i1 = v1 && (BORDER ? tile_interior(T1) : true);
    i2 = v2 && (BORDER ? tile_interior(T2) : true);
    org0 = tile_org(T0);
    org1 = v1 ? tile_org(T1) : src_safe;
    org2 = v2 ? tile_org(T2) : src_safe;
    __syncthreads();  // the previous pass is done with both tile buffers
#pragma unroll
    for (int j = 0; j < NJ; j++) load_one(std::false_type{}, j, 0, T0, true, i0, org0);
    if constexpr (XF) {
      refresh_xf(T0.n);
      read_xf(0);
    }
#pragma unroll
    for (int j = 0; j < NJ; j++) commit_one(std::false_type{}, j, T0, i0, a_lds);
#pragma unroll
    for (int j = 0; j < NJ; j++) {
      if (NCH > 1)
        load_one(std::false_type{}, j, 1, T0, true, i0, org0);
      else
        load_one(std::false_type{}, j, 0, T1, v1, i1, org1);
    }
    // (round 4) drained once per pass: hipcc derives the N of every `s_waitcnt vmcnt(N)` in the tile loop from the
    // predecessor with the FEWEST younger operations -- entered with these loads pending and no store behind them, the
    // first commit of every tile waits for the acknowledgements of the previous tile's stores (see `epilogue`)
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    WS_BARRIER();
  };

  const bool plain = !a.accumulate && n0 + NC <= a.Cout;  // uniform: see `epilogue`
  const int ch = n0 + r;                 // channel of output block 0 (block nb: + 32 nb)
  bool ch_ok[NB];
  float bias[NB];
#pragma unroll
  for (int nb = 0; nb < NB; nb++) {
    ch_ok[nb] = ch + 32 * nb < a.Cout;
    bias[nb] = (a.bias && ch_ok[nb]) ? a.bias[ch + 32 * nb] : 0.f;
  }
  T* outp[NB];  // split output: a 32-channel block lies entirely on one side (split is a multiple of 32)
#pragma unroll
  for (int nb = 0; nb < NB; nb++)
    outp[nb] = (a.split && n0 + 32 * nb >= a.split) ? reinterpret_cast<T*>(a.out2) - a.split : reinterpret_cast<T*>(a.out);
  // accumulator register i of this lane: tile voxel (dz, 2w + mb, x) with x = (i & 3) + 4 * ((i >> 2) & 1) and
  // dz = {0,1,3,2}[i >> 2] (h == 0) or {1,0,2,3}[i >> 2] (h == 1)   (ws_row_to_zx of row (i&3) + 8*(i>>2) + 4h)
  int edz[4], eplane[4];
#pragma unroll
  for (int q4 = 0; q4 < 4; q4++) {
    int dz, x;
    ws_row_to_zx(8 * q4 + 4 * h, dz, x);
    edz[q4] = dz;
    eplane[q4] = dz * a.Ho * a.Wo * (int)a.out_pitch;
  }
  auto eoff = [&](int i) { return eplane[i >> 2] + ((i & 3) + 4 * ((i >> 2) & 1)) * (int)a.out_pitch; };
  const int ezh = 4 * a.Ho * a.Wo * (int)a.out_pitch;   // z half 1 of an 8-deep tile: four planes further
  // InstanceNorm partial rows are per WORKGROUP, not per tile: sample n owns WS_STAT_ROWS rows, row
  // pass * 256 + blockIdx.x (+ k gridDim.x for the slots no workgroup has) holds this workgroup's sums over its
  // tiles of n in that pass.  Every lane keeps running sums of ITS channel over the voxels it has produced (lr1 / lr2:
  // two registers per output block, two adds per tile); lanes and waves are combined through s_red only when the sample
  // changes or the pass ends (stats_to_row, a handful of times per launch).  Round 2 sent every tile's per-wave sums
  // through LDS and had tid < NC collect them behind the next barrier: a shuffle pair, two LDS writes, eight LDS reads
  // and two branches per tile inside the hot loop.  The rows are zeroed here first, so in_finalize reads 512 rows
  // instead of one per tile.
  float lr1[NB], lr2[NB];
#pragma unroll
  for (int nb = 0; nb < NB; nb++) lr1[nb] = lr2[nb] = 0.f;
  int racc_n = -1, cur_pass = 0;
  auto stat_row = [&](int n, int pass, int b) {
    return a.stat_partials + (((int64_t)n * WS_STAT_ROWS + pass * 256 + b) * a.CoutP + n0 + tid) * 2;
  };
  if (a.stat_partials && tid < NC) {
    for (int n = 0; n < a.N; n++)
      for (int pass = 0; pass < 2; pass++)
        for (int b = blockIdx.x; b < 256; b += gridDim.x) {
          float* q = stat_row(n, pass, b);
          q[0] = 0.f;
          q[1] = 0.f;
        }
  }
  // uniform (every wave takes the same path): lanes -> waves -> this workgroup's row of sample racc_n, fixed order
  auto stats_to_row = [&]() __attribute__((always_inline)) {
    if (a.stat_partials && racc_n >= 0) {
#pragma unroll
      for (int nb = 0; nb < NB; nb++) {
        const float u1 = lr1[nb] + __shfl_xor(lr1[nb], 32, 64), u2 = lr2[nb] + __shfl_xor(lr2[nb], 32, 64);
        if (h == 0) {
          s_red[(wave * NC + 32 * nb + r) * 2 + 0] = u1;
          s_red[(wave * NC + 32 * nb + r) * 2 + 1] = u2;
        }
      }
      __syncthreads();
      if (tid < NC) {
        float t1 = 0.f, t2 = 0.f;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          t1 += s_red[(k * NC + tid) * 2 + 0];
          t2 += s_red[(k * NC + tid) * 2 + 1];
        }
        float* q = stat_row(racc_n, cur_pass, blockIdx.x);
        q[0] += t1;
        q[1] += t2;
      }
      __syncthreads();
    }
#pragma unroll
    for (int nb = 0; nb < NB; nb++) lr1[nb] = lr2[nb] = 0.f;
    racc_n = -1;
  };
  // the tile about to be summed belongs to sample n (uniform)
  // BS (backward statistics, ConvArgs::bs_*): this lane's channel constants of the sample being summed
  float bsc = 0.f, bsh = 0.f, bmu = 0.f, brs = 0.f;
  auto stats_sample = [&](int n) __attribute__((always_inline)) {
    if (n != racc_n) {
      if (racc_n >= 0) stats_to_row();
      racc_n = n;
      if constexpr (BS) {
        const int64_t o = (int64_t)n * a.Cout + min(n0 + r, a.Cout - 1);
        bsc = a.bs_scale[o], bsh = a.bs_shift[o], bmu = a.bs_mean[o], brs = a.bs_rstd[o];
      }
    }
  };

#ifdef WS_DBG_STAMPS
  unsigned long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const unsigned long long treal0 = __builtin_amdgcn_s_memrealtime();  // 100 MHz, the same counter on every CU
  unsigned long long tlast = __builtin_amdgcn_s_memtime();
  const unsigned long long tcyc0 = tlast;
#endif

  // this lane's first output element of a tile: channel n0 + r, rows y0 + 2w (+ mb), voxel (z0, ., x0)
  auto out_base = [&](const WsTile& t, int nb) -> T* {
    return outp[nb] + ((((int64_t)t.n * a.Do + t.z0) * a.Ho + t.y0 + 2 * wave) * a.Wo + t.x0) * a.out_pitch + ch + 32 * nb;
  };
  // PLAIN (compile-time, round 4): the launch stores whole 32-channel blocks without accumulating (`plain`, uniform) and
  // the tile is whole (every interior tile is): the epilogue is then branch-free, a FIXED number of stores.  vmcnt counts
  // stores too and retires in order; with a conditional store path in the loop hipcc assumes that no store is younger than
  // the loads the next tile's first commit waits for, emits vmcnt(4) and thereby waits for the write acknowledgements of
  // this tile's 32 NB stores at every tile top (the "tile top" share of the round-3 stamps).
  auto epilogue = [&](f32x16 (&acc)[2 * NB * ZH], const WsTile& ET, auto plain_tag) __attribute__((always_inline)) {
    constexpr bool PLAIN = decltype(plain_tag)::value;
    const int z0 = ET.z0, y0 = ET.y0, x0 = ET.x0;
    const bool full = PLAIN || (z0 + TD <= a.Do && y0 + TH <= a.Ho && x0 + TW <= a.Wo);
    stats_sample(ET.n);
#pragma unroll
    for (int nb = 0; nb < NB; nb++) {
      float s1 = 0.f, s2 = 0.f;
      T* const obase = out_base(ET, nb);
      if (PLAIN || (full && ch_ok[nb] && !a.accumulate)) {
        if constexpr (BS) {
          // the y values of the tile's 32 voxels are requested first, the outputs stored under their latency; the sums
          // use the STORED (storage-rounded) gradient, as in_bwd_reduce would read it back
#pragma unroll
          for (int zh = 0; zh < ZH; zh++) {
          const T* const ybase = reinterpret_cast<const T*>(a.bs_y) +
                                 ((((int64_t)ET.n * a.Do + z0 + 4 * zh) * a.Ho + y0 + 2 * wave) * a.Wo + x0) * a.bs_y_pitch + ch;
          float yv[2][16];
#pragma unroll
          for (int mb = 0; mb < 2; mb++)
#pragma unroll
            for (int i = 0; i < 16; i++)
              yv[mb][i] = ST<T>::ld(ybase + ((int64_t)(edz[i >> 2] * a.Ho + mb) * a.Wo + (i & 3) + 4 * ((i >> 2) & 1)) *
                                                a.bs_y_pitch);
#pragma unroll
          for (int mb = 0; mb < 2; mb++) {
            T* const orow = obase + (int64_t)mb * a.Wo * a.out_pitch + zh * ezh;
#pragma unroll
            for (int i = 0; i < 16; i++) {
              const float v = acc[(nb * ZH + zh) * 2 + mb][i] + bias[nb];
              ST<T>::st(orow + eoff(i), v);
              T tmp;
              ST<T>::st(&tmp, v);
              const float g = (yv[mb][i] * bsc + bsh > 0.f) ? ST<T>::ld(&tmp) : 0.f;
              s1 += g;
              s2 += g * ((yv[mb][i] - bmu) * brs);
            }
          }
          }
        } else {
#pragma unroll
        for (int zh = 0; zh < ZH; zh++)
#pragma unroll
        for (int mb = 0; mb < 2; mb++) {
          T* const orow = obase + (int64_t)mb * a.Wo * a.out_pitch + zh * ezh;
#pragma unroll
          for (int i = 0; i < 16; i++) {
            const float v = acc[(nb * ZH + zh) * 2 + mb][i] + bias[nb];
            ST<T>::st(orow + eoff(i), v);
            s1 += v;
            s2 += v * v;
          }
        }
        }
      } else if (full && ch_ok[nb]) {
        // accumulating launch (the UpConv chain's data gradients add into the skip gradient), whole tile: the 16 old
        // values of a row are requested together, then added and stored -- the generic path below asks for one
        // 2-byte value at a time behind a branch (up3's data gradient at 64^3: 252 us against 76 us for the same conv
        // without accumulation, on the critical path of the backward)
#pragma unroll
        for (int zh = 0; zh < ZH; zh++)
#pragma unroll
        for (int mb = 0; mb < 2; mb++) {
          T* const orow = obase + (int64_t)mb * a.Wo * a.out_pitch + zh * ezh;
          float old[16];
#pragma unroll
          for (int i = 0; i < 16; i++) old[i] = ST<T>::ld(orow + eoff(i));
#pragma unroll
          for (int i = 0; i < 16; i++) {
            const float v = acc[(nb * ZH + zh) * 2 + mb][i] + bias[nb];
            ST<T>::st(orow + eoff(i), v + old[i]);
            s1 += v;
            s2 += v * v;
          }
        }
      } else {
#pragma unroll
        for (int zh = 0; zh < ZH; zh++)
#pragma unroll
        for (int mb = 0; mb < 2; mb++) {
          const int gy = y0 + 2 * wave + mb;
          T* const orow = obase + (int64_t)mb * a.Wo * a.out_pitch + zh * ezh;
#pragma unroll
          for (int i = 0; i < 16; i++) {
            const int gz = z0 + edz[i >> 2] + 4 * zh, gx = x0 + (i & 3) + 4 * ((i >> 2) & 1);
            const float v = acc[(nb * ZH + zh) * 2 + mb][i] + bias[nb];
            const bool ok = gz < a.Do && gy < a.Ho && gx < a.Wo;
            if (ok && ch_ok[nb]) {
              float o = v;
              if (a.accumulate) o += ST<T>::ld(orow + eoff(i));
              ST<T>::st(orow + eoff(i), o);
            }
            const float mk = ok ? 1.f : 0.f;
            s1 += mk * v;
            s2 += mk * v * v;
          }
        }
      }
      if (PLAIN || ch_ok[nb]) {
        lr1[nb] += s1;
        lr2[nb] += s2;
      }
    }
  };

  // One tile: NCH passes.  Pass c runs the MFMAs of chunk c out of buffer (PAR0 + c) & 1 and, in their shadow,
  // commits item c+1 (chunk (c+1) % NCH of T0 or T1) into the other buffer and loads item c+2 into the freed pf.
  // (Rounds 1-2 deferred the epilogue of single-pass tiles into the MFMA gaps of the next tile, with two accumulator
  // register sets; once the 64-byte-row layers became two-pass that served only the 16->32 first layer, where it was
  // worth 3 % of the launch and nothing in the step, at 30 more registers: removed in round 3.)
  f32x16 acc[2 * NB * ZH];  // [(nb * ZH + zh) * 2 + mb]
  auto tile_phase = [&](auto par_tag, auto fast_tag, auto plain_tag) __attribute__((always_inline)) {
    constexpr int PAR0 = decltype(par_tag)::value;
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      constexpr int dummy = 0;
      (void)dummy;
      const int PAR = (PAR0 + c) & 1;
      char* const a_rd = a_lds + PAR * ABUF;
      char* const a_wr = a_lds + (1 - PAR) * ABUF;
      // commit target: item c+1; load target: item c+2
      const bool c_next = (c + 1 >= NCH);                  // commit goes to T1
      const int c_chunk = (c + 1) % NCH;
      const int l_tile = (c + 2) / NCH;                    // 0: T0, 1: T1, 2: T2
      const int l_chunk = (c + 2) % NCH;
      const WsTile& CT = c_next ? T1 : T0;
      const bool c_int = c_next ? (i1 | !v1) : i0;         // an invalid next tile is committed as garbage, unchecked
      const WsTile& LT = l_tile == 0 ? T0 : (l_tile == 1 ? T1 : T2);
      const bool l_val = l_tile == 0 ? true : (l_tile == 1 ? v1 : v2);
      const bool l_int = l_tile == 0 ? i0 : (l_tile == 1 ? i1 : i2);
      const T* const l_org = l_tile == 0 ? org0 : (l_tile == 1 ? org1 : org2);
      WS2_STAMP(3)
      if constexpr (XF) {
        if (CT.n != tbl_n && (!c_next || v1)) refresh_xf(CT.n);
        read_xf(c_chunk);
      }
      WS2_STAMP(0)
      u32x4 af[2][4 * ZH], bf[2][3 * NB];
      // RB == 32: the 27 weight fragments of the single pass are the same LDS words for every tile, and hipcc hoists
      // their reads out of the tile loop into 108 AGPRs (384 registers in all: nothing of another stream fits beside
      // the workgroup -- the branch stream's first token kernels waited 150 us for the first encoder conv).  The
      // laundered pointer keeps the reads in the loop, as in the wider variants.
      const char* w_rd = w_lds;
      if constexpr (RB == 32) asm volatile("" : "+v"(w_rd));
      auto read_group = [&](int g, u32x4 (&A)[4 * ZH], u32x4 (&B)[3 * NB]) {
        const int t = g / NFS, fs = g % NFS, jz = t / 3, jx = t % 3;
        auto rdA = [&](int yp) {
#pragma unroll
          for (int zh = 0; zh < ZH; zh++) A[zh * 4 + yp] = *reinterpret_cast<const u32x4*>(a_rd + a_addr(jz, yp, jx, fs, zh));
        };
        auto rdB = [&](int jy) {
#pragma unroll
          for (int nb = 0; nb < NB; nb++)
            B[jy * NB + nb] = *reinterpret_cast<const u32x4*>(w_rd + ((jz * 9 + jy * 3 + jx) * NC + 32 * nb) * RB +
                                                              (bvar[c] ^ (fs * 32)));
        };
        // in order of first use (LDS returns in order, the waits are counted)
        rdB(0);
        rdA(0);
        rdA(1);
        rdB(1);
        rdA(2);
        rdB(2);
        rdA(3);
      };
      read_group(0, af[0], bf[0]);
#pragma unroll
      for (int g = 0; g < NG; g++) {
        if (g + 1 < NG) read_group(g + 1, af[(g + 1) & 1], bf[(g + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);  // look-ahead reads stay ABOVE this group's MFMAs
#pragma unroll
        for (int j = 0; j < NJ; j++) {
          if ((j * NG) / NJ == g) {
            commit_one(fast_tag, j, CT, c_int, a_wr);
            load_one(fast_tag, j, l_chunk, LT, l_val, l_int, l_org);
          }
        }
        u32x4(&A)[4 * ZH] = af[g & 1];
        u32x4(&B)[3 * NB] = bf[g & 1];
        if (c == 0 && g == 0) {  // first MFMAs of the tile take a zero C operand: no accumulator clearing
#pragma unroll
          for (int q2 = 0; q2 < 2 * NB * ZH; q2++)
#pragma unroll
            for (int i = 0; i < 16; i++) acc[q2][i] = 0.f;
        }
#pragma unroll
        for (int jy = 0; jy < 3; jy++)
#pragma unroll
          for (int nb = 0; nb < NB; nb++)
#pragma unroll
            for (int zh = 0; zh < ZH; zh++) {
              Mma<T>::run(A[zh * 4 + jy], B[jy * NB + nb], acc[(nb * ZH + zh) * 2 + 0]);      // mb 0: box row y' = jy
              Mma<T>::run(A[zh * 4 + jy + 1], B[jy * NB + nb], acc[(nb * ZH + zh) * 2 + 1]);  // mb 1: box row y' = jy + 1
            }
        __builtin_amdgcn_sched_barrier(0);
      }
      WS2_STAMP(1)
      WS_BARRIER();  // buffer PAR fully read, buffer 1-PAR fully written
      WS2_STAMP(2)
    }
    epilogue(acc, T0, plain_tag);
    WS2_STAMP(4)
  };

  using P0 = std::integral_constant<int, 0>;
  using P1 = std::integral_constant<int, 1>;
  using Yes = std::true_type;
  using No = std::false_type;
  bool more = true;
  auto step = [&](auto border_tag) __attribute__((always_inline)) {
    constexpr bool BORDER = decltype(border_tag)::value;
    more = v1;
    if (!more) return;
    left--;
    T0 = T1;
    T1 = T2;
    i0 = i1;
    i1 = i2;
    v1 = v2;
    org0 = org1;
    org1 = org2;
    if constexpr (BORDER)
      bor_next(T2);
    else
      int_next(T2);
    v2 = left >= 2;
    i2 = v2 && (BORDER ? tile_interior(T2) : true);
    org2 = v2 ? tile_org(T2) : src_safe;
  };

  // ---- pass A: interior tiles: the unchecked copy of the phase (single-pass tiles alternate the buffer parity)
  if (int_cnt > 0) {
    begin_pass(No{}, int_begin, int_cnt);
    more = true;
    int par = 0;
    // (two loops, not one loop with a branch: the two epilogues must not meet at one loop head, see `epilogue`)
    if (plain) {
      while (more) {
        if (NCH > 1 || par == 0)
          tile_phase(P0{}, Yes{}, Yes{});
        else
          tile_phase(P1{}, Yes{}, Yes{});
        if (NCH == 1) par ^= 1;
        step(No{});
      }
    } else {
      while (more) {
        if (NCH > 1 || par == 0)
          tile_phase(P0{}, Yes{}, No{});
        else
          tile_phase(P1{}, Yes{}, No{});
        if (NCH == 1) par ^= 1;
        step(No{});
      }
    }
  }
  // ---- pass B: border tiles (checked copy)
  if (bor_cnt > 0) {
    begin_pass(Yes{}, bor_begin, bor_cnt);
    stats_to_row();
    cur_pass = 1;
    more = true;
    int par = 0;
    while (more) {
      if (NCH > 1 || par == 0)
        tile_phase(P0{}, No{}, No{});
      else
        tile_phase(P1{}, No{}, No{});
      if (NCH == 1) par ^= 1;
      step(Yes{});
    }
  }
  stats_to_row();
#ifdef WS_DBG_STAMPS
  if (tid == 0 && blockIdx.y == 0) {
    for (int k = 0; k < 5; k++) a.stat_partials[(int64_t)blockIdx.x * 8 + k] = (float)tacc[k];
    // slots 5, 6: low words of the 100 MHz real-time counter at entry / exit (bit patterns); slot 7: shader cycles
    a.stat_partials[(int64_t)blockIdx.x * 8 + 5] = __uint_as_float((uint32_t)treal0);
    a.stat_partials[(int64_t)blockIdx.x * 8 + 6] = __uint_as_float((uint32_t)__builtin_amdgcn_s_memrealtime());
    a.stat_partials[(int64_t)blockIdx.x * 8 + 7] = (float)(__builtin_amdgcn_s_memtime() - tcyc0);
    a.stat_partials[2048 + blockIdx.x] = __uint_as_float((uint32_t)t_entry);  // kernel entry of this workgroup
  }
#endif
}

// Second pass of a split-K conv launch: one workgroup per (TILE of the conv's tiling, 64-channel block) -- so that the
// InstanceNorm partial rows keep their geometry -- thread = (voxel lane, 4 consecutive channels): the partial tiles are
// summed in split order, + bias (+ the old output when accumulating), stored in the storage type, and the per-channel
// (sum, sum of squares) of the tile reduced over the 16 voxel lanes in a fixed order.
template <typename T, int TD, int TH, int TW>
__global__ __launch_bounds__(256) void conv_ksplit_reduce_kernel(ConvArgs a) {
  if (a.prio) HDF_LIGHT_PRIO();
  __shared__ float red[16][64][2];
  const int ntz = (a.Do + TD - 1) / TD, nty = (a.Ho + TH - 1) / TH, ntx = (a.Wo + TW - 1) / TW;
  int t = blockIdx.x;
  const int tx = t % ntx;
  t /= ntx;
  const int ty = t % nty;
  t /= nty;
  const int tz = t % ntz, n = t / ntz;
  const int cl = ((int)threadIdx.x & 15) * 4, c0 = blockIdx.y * 64 + cl, vl = (int)threadIdx.x >> 4;
  const bool c_on = c0 < a.CoutP;
  const int64_t mtot = (int64_t)a.N * a.Do * a.Ho * a.Wo;
  float bias[4], s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; e++) bias[e] = (a.bias && c0 + e < a.Cout) ? a.bias[c0 + e] : 0.f;
  constexpr int TV = TD * TH * TW, IT = (TV + 15) / 16;
  static_assert(TV % 16 == 0, "tile voxels per voxel lane");
  if (c_on) {
#pragma unroll 2
    for (int it = 0; it < IT; it++) {
      const int lin = vl + 16 * it;
      const int gz = tz * TD + lin / (TH * TW), gy = ty * TH + (lin / TW) % TH, gx = tx * TW + lin % TW;
      const bool ok = gz < a.Do && gy < a.Ho && gx < a.Wo;
      const int64_t vox = ok ? (((int64_t)n * a.Do + gz) * a.Ho + gy) * a.Wo + gx : 0;
      f32x4 pv[4];
#pragma unroll
      for (int k = 0; k < 4; k++)   // (ksplit <= 4; clamped: never branch around a load)
        pv[k] = *reinterpret_cast<const f32x4*>(a.kpart + ((int64_t)min(k, a.ksplit - 1) * mtot + vox) * a.CoutP + c0);
      f32x4 v = pv[0];
      for (int k = 1; k < a.ksplit; k++) v += pv[k];
      if (ok) {
        T* p = reinterpret_cast<T*>(a.out) + vox * a.out_pitch + c0;
#pragma unroll
        for (int e = 0; e < 4; e++) {
          if (c0 + e < a.Cout) {
            float o = v[e] + bias[e];
            if (a.accumulate) o += ST<T>::ld(p + e);
            ST<T>::st(p + e, o);
            s1[e] += o;
            s2[e] += o * o;
          }
        }
      }
    }
  }
  if (a.stat_partials) {
#pragma unroll
    for (int e = 0; e < 4; e++) red[vl][cl + e][0] = s1[e], red[vl][cl + e][1] = s2[e];
    __syncthreads();
    if (threadIdx.x < 128) {
      const int c = threadIdx.x >> 1, j = threadIdx.x & 1;
      if (blockIdx.y * 64 + c < a.CoutP) {
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < 16; k++) sum += red[k][c][j];
        a.stat_partials[((int64_t)blockIdx.x * a.CoutP + blockIdx.y * 64 + c) * 2 + j] = sum;
      }
    }
  }
}

template <typename T, int TD, int TH, int TW, int WM, int WN, int MB, int S, bool CONVT, bool FLAT = false>
int launch_cfg(const ConvArgs& a0, hipStream_t st) {
  ConvArgs a = a0;
  const int Td = CONVT ? a.Di : a.Do, Th = CONVT ? a.Hi : a.Ho, Tw = CONVT ? a.Wi : a.Wo;
  const int tiles = a.N * ceil_div(Td, TD) * ceil_div(Th, TH) * ceil_div(Tw, TW), nblk = ceil_div(a.CoutP, WN * 32);
  a.ksplit = 1;
  if constexpr (!CONVT && S == 1) {
    // split-K: a low-resolution layer whose tiles x output blocks leave CUs idle, whole 64-byte chunks (the pipelined
    // path), one plain output; 4 or 2 ways while every workgroup keeps >= 2 chunks and the partial tiles fit the scratch
    const int nchunk = (a.Cin * (int)sizeof(T)) % 64 == 0 ? a.Cin * (int)sizeof(T) / 64 : 0;
    if (a.kpart && !a.split && a.CoutP <= 1024 && a.CoutP % 4 == 0 && a.out_pitch % 4 == 0) {
      for (int ks = 4; ks >= 2; ks >>= 1) {
        const size_t need = (size_t)ks * a.N * a.Do * a.Ho * a.Wo * a.CoutP * sizeof(float);
        if (tiles * nblk * ks <= hdf_cu_budget() && nchunk % ks == 0 && nchunk / ks >= 2 && need <= a.kpart_bytes) {
          a.ksplit = ks;
          break;
        }
      }
    }
  }
  dim3 grid(tiles, nblk, CONVT ? (FLAT ? 4 : 8) : a.ksplit);   // transposed conv: one grid slice per output-parity class
  hipLaunchKernelGGL((conv_igemm_kernel<T, TD, TH, TW, WM, WN, MB, S, CONVT, FLAT>), grid, dim3(256), 0, st, a);
  HDF_LAUNCH_CHECK();
  if constexpr (!CONVT && S == 1) {
    if (a.ksplit > 1) {
      hipLaunchKernelGGL((conv_ksplit_reduce_kernel<T, TD, TH, TW>), dim3(tiles, ceil_div(a.CoutP, 64)), dim3(256), 0, st, a);
      HDF_LAUNCH_CHECK();
    }
  }
  return HDF_OK;
}

// tile-shape choice: shared by the launcher and by hdf_conv_stat_tiles (partials geometry)
inline bool small_tile(int Do, int Ho, int Wo) {
  return (int64_t)Do * Ho * Wo <= 32 * 32 * 32 / 2;
}
// 8^3-class volumes (the bottleneck UpConv): 64-voxel tiles, or a handful of workgroups would carry the whole layer
inline bool tiny_tile(int Do, int Ho, int Wo) {
  return (int64_t)Do * Ho * Wo <= 8 * 8 * 16;
}
// weights-stationary kernel: mode 0, whole Cin row <= 128 B, enough tiles to amortise the weight panel
inline int ws_cfg(int mode, int Do, int Ho, int Wo, int row_bytes) {
  if (mode != 0 || row_bytes > 128 || (int64_t)Do * Ho * Wo < 48 * 48 * 48 || Do == 1) return 0;   // (depth 1: the flat kernels)
  return (row_bytes == 32 || row_bytes == 64 || row_bytes == 128) ? 1 : 0;
}

template <typename T, int CH, int RB, int NB>
int launch_ws2(const ConvArgs& a, hipStream_t st) {
  const int budget = a.cu_budget > 0 ? std::min(a.cu_budget, hdf_cu_budget()) : hdf_cu_budget();
  const int cout_tiles = a.CoutP / (32 * NB);
#ifndef HDF_NO_WS2_TD8   // (A/B builds: the 4-deep tile everywhere)
  // 64-byte rows, one output block, 16-bit storage, WITH an input transform (32 -> 32 channels at the top level, forward:
  // block_1_2_left / block_1_2_right): the 8x8x8 tile (TDP = 8, see the kernel) when the depth is a whole number of tiles.
  // Measured (tools/td8_ab.sh, same box, 32 -> 32 @128^3 batch 2): with the transform 303 vs 328 us; without 297 vs 300;
  // data gradient with the statistics epilogue 351 vs 356 -- but the 8-deep form needs all 512 registers (384 spill 203),
  // and a 512-register workgroup shares its compute unit with nothing: with all four launches of a step on it the step
  // was 0.1 ms SLOWER (2 of 3 pairs).  So only the two forward launches take it: they run with the other streams idle or
  // on their own quarter of the chip (forward3d), and they are where the gain is.
  if constexpr (sizeof(T) == 2 && NB == 1 && RB == 64) {
    if (a.in_scale && !a.bs_y && a.Do % 8 == 0 && a.Do >= 24 && a.Ho >= 24 && a.Wo >= 24) {
      const int tiles8 = a.N * (a.Do / 8) * ceil_div(a.Ho, 8) * ceil_div(a.Wo, 8);
      const int gx8 = std::min(tiles8, std::max(1, budget / cout_tiles));
      hipLaunchKernelGGL((conv_ws2_kernel<T, CH, RB, true, NB, false, 8>), dim3(gx8, cout_tiles), dim3(256), 0, st, a);
      HDF_LAUNCH_CHECK();
      return HDF_OK;
    }
  }
#endif
  const int tiles = a.N * ceil_div(a.Do, 4) * ceil_div(a.Ho, 8) * ceil_div(a.Wo, 8);
  const int gx = std::min(tiles, std::max(1, budget / cout_tiles));  // one workgroup per CU; the kernel splits the tiles
  if constexpr (sizeof(T) == 2 && NB == 1 && RB == 64) {   // the level-0 32 -> 32 data gradient (hdf_conv_bwd_stats_ok)
    if (a.bs_y && !a.in_scale) {
      hipLaunchKernelGGL((conv_ws2_kernel<T, CH, RB, false, NB, true>), dim3(gx, cout_tiles), dim3(256), 0, st, a);
      HDF_LAUNCH_CHECK();
      return HDF_OK;
    }
  }
  HDF_CHECK_ARG(a.bs_y == nullptr, "conv: backward statistics are not available for this launch (hdf_conv_bwd_stats_ok)");
  if (a.in_scale)
    hipLaunchKernelGGL((conv_ws2_kernel<T, CH, RB, true, NB>), dim3(gx, cout_tiles), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((conv_ws2_kernel<T, CH, RB, false, NB>), dim3(gx, cout_tiles), dim3(256), 0, st, a);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

// Tile of a flat (depth-1, 2-D) stride-1 conv: 1x16x16 (256 voxels), 1x8x16 below 64x64, 1x8x8 below 32x32
inline int flat_tile(int Ho, int Wo) { return (int64_t)Ho * Wo <= 32 * 32 ? 0 : ((int64_t)Ho * Wo <= 64 * 64 ? 1 : 2); }

template <typename T>
int launch_conv_t(int mode, const ConvArgs& a, hipStream_t st) {
  if (a.Di == 1) {
    // ---- the 2-D operators (models/HDenseFormer_2D.py:125-170): depth-1 tensors, centre-plane taps, y / x strides only
    HDF_CHECK_ARG(a.Do == 1 && !a.bs_y, "conv: a depth-1 input selects the 2-D operator (output depth 1, no statistics epilogue of the 3-D data gradient)");
    if (mode == 0) {
      const int ft = flat_tile(a.Ho, a.Wo);
      if (ft == 0) return launch_cfg<T, 1, 8, 8, 2, 2, 1, 1, false, true>(a, st);        // 64 vox x 64 ch
      if (ft == 1) return launch_cfg<T, 1, 8, 16, 2, 2, 2, 1, false, true>(a, st);       // 128 vox x 64 ch
      if (a.CoutP <= 32) return launch_cfg<T, 1, 16, 16, 4, 1, 2, 1, false, true>(a, st);  // 256 vox x 32 ch
      return launch_cfg<T, 1, 16, 16, 2, 2, 4, 1, false, true>(a, st);                   // 256 vox x 64 ch
    } else if (mode == 1) {
      if (a.CoutP <= 64) return launch_cfg<T, 1, 8, 8, 2, 2, 1, 2, false, true>(a, st);   // 64 vox x 64 ch, stride 2 in y, x
      return launch_cfg<T, 1, 8, 8, 1, 4, 2, 2, false, true>(a, st);                      // 64 vox x 128 ch
    } else {
      if (hdf_convt_fused_takes(ST<T>::DT, a)) return hdf_launch_convt_fused(ST<T>::DT, a, st);   // conv_s2.hip
      if (a.CoutP <= 32) return launch_cfg<T, 1, 16, 16, 4, 1, 2, 1, true, true>(a, st);
      return launch_cfg<T, 1, 8, 16, 2, 2, 2, 1, true, true>(a, st);
    }
  }
  if (mode == 0) {
    const int rb = a.Cin * (int)sizeof(T);
    const int ws = ws_cfg(mode, a.Do, a.Ho, a.Wo, rb);
    if (ws) {
      if (rb == 32) return launch_ws2<T, 32, 32, 1>(a, st);
      if (rb == 64 && a.CoutP % 64 == 0) return launch_ws2<T, 32, 64, 2>(a, st);
      // 64-byte rows, one output block: two 32-byte passes per tile.  (Rounds 1-2 ran these layers as ONE 64-byte pass
      // with the deferred epilogue: 512 registers, 500 B of scratch per lane in the border copies, 1.2x the output in
      // HBM writes; the two-pass form needs 303 registers and is 7 % faster without / 1 % with an input transform.)
      if (rb == 64) return launch_ws2<T, 32, 64, 1>(a, st);
      if (rb == 128) return launch_ws2<T, 32, 128, 1>(a, st);
    }
    if (tiny_tile(a.Do, a.Ho, a.Wo)) return launch_cfg<T, 2, 4, 8, 2, 2, 1, 1, false>(a, st);   // 64 vox x 64 ch
    if (small_tile(a.Do, a.Ho, a.Wo)) return launch_cfg<T, 4, 4, 8, 2, 2, 2, 1, false>(a, st);  // 128 vox x 64 ch
    if (a.CoutP <= 32) return launch_cfg<T, 4, 8, 8, 4, 1, 2, 1, false>(a, st);                  // 256 vox x 32 ch
    return launch_cfg<T, 4, 8, 8, 2, 2, 4, 1, false>(a, st);                                     // 256 vox x 64 ch
  } else if (mode == 1) {
    if (hdf_conv_gather_s2_takes(ST<T>::DT, a)) return hdf_launch_conv_gather_s2(ST<T>::DT, a, st);   // conv_s2.hip
    if (a.CoutP <= 64) return launch_cfg<T, 2, 4, 8, 2, 2, 1, 2, false>(a, st);  // 64 vox x 64 ch, stride 2
    return launch_cfg<T, 4, 4, 4, 1, 4, 2, 2, false>(a, st);  // 64 vox x 128 ch, stride 2
  } else {
    // the specialised kernels of conv_s2.hip first; row widths they do not take (n_filters = 48: 192-byte rows) run per class
    if (hdf_convt_ws_takes(ST<T>::DT, a)) return hdf_launch_convt_ws(ST<T>::DT, a, st);
    if (hdf_convt_fused_takes(ST<T>::DT, a)) return hdf_launch_convt_fused(ST<T>::DT, a, st);
    if (a.CoutP <= 32) return launch_cfg<T, 4, 8, 8, 4, 1, 2, 1, true>(a, st);
    return launch_cfg<T, 4, 4, 8, 2, 2, 2, 1, true>(a, st);
  }
}

}  // namespace

int hdf_conv_weight_layout(int dtype, int mode, int Cin, int Do, int Ho, int Wo) {
  const int rb = Cin * hdf_esz(dtype);
  if (rb % 64 != 0) return 0;                       // the pipelined path needs whole 64-byte chunks
  if (Do == 1)                                      // depth 1 (the 2-D operators): conv_igemm_kernel, but the transposed conv
    return (mode == 2 && hdf_convt_fused_rows(rb)) ? 0 : 1;   // runs convt_fused_kernel<FLAT> (row-major panels)
  if (mode == 0) return ws_cfg(mode, Do, Ho, Wo, rb) ? 0 : 1;  // conv_ws2_kernel stages row-major panels
  if (mode == 1) return 1;                                 // stride-2 gather conv: pipelined path
  return hdf_convt_fused_rows(rb) ? 0 : 1;  // transposed conv: convt_fused_kernel reads row-major panels, other widths run per class
}

bool hdf_conv_bwd_stats_ok(int dtype, const ConvArgs& a) {
  const int rb = a.Cin * hdf_esz(dtype);
  return dtype != HDF_F32 && rb == 64 && a.Cout == 32 && a.CoutP == 32 && !a.in_scale && !a.accumulate && !a.split &&
         a.Do % 4 == 0 && a.Ho % 8 == 0 && a.Wo % 8 == 0 && ws_cfg(0, a.Do, a.Ho, a.Wo, rb) && a.stat_partials &&
#ifndef HDF_NO_CONV_WR
         !hdf_conv_wr_takes(dtype, a) &&
#endif
         a.Di == a.Do && a.Hi == a.Ho && a.Wi == a.Wo;
}

int hdf_conv_stat_tiles(int mode, int Do, int Ho, int Wo, int row_bytes) {
  if (mode != 0) return 0;
  if (Do == 1) {   // the flat tiles of launch_conv_t
    const int ft = flat_tile(Ho, Wo);
    return ft == 0 ? ceil_div(Ho, 8) * ceil_div(Wo, 8) : (ft == 1 ? ceil_div(Ho, 8) * ceil_div(Wo, 16) : ceil_div(Ho, 16) * ceil_div(Wo, 16));
  }
  if (ws_cfg(mode, Do, Ho, Wo, row_bytes)) return WS_STAT_ROWS;  // per-workgroup rows (conv_ws2_kernel)
  if (tiny_tile(Do, Ho, Wo)) return ceil_div(Do, 2) * ceil_div(Ho, 4) * ceil_div(Wo, 8);
  if (small_tile(Do, Ho, Wo)) return ceil_div(Do, 4) * ceil_div(Ho, 4) * ceil_div(Wo, 8);
  return ceil_div(Do, 4) * ceil_div(Ho, 8) * ceil_div(Wo, 8);
}

int hdf_launch_conv(int dtype, int mode, const ConvArgs& a, hipStream_t st) {
  HDF_CHECK_ARG(a.Cin % 16 == 0, "conv: Cin=%d must be a multiple of 16 (pad the first layer)", a.Cin);
  HDF_CHECK_ARG(a.CoutP % 32 == 0 && a.CoutP >= a.Cout, "conv: bad CoutP=%d for Cout=%d", a.CoutP, a.Cout);
  HDF_CHECK_ARG(a.in_pitch % 8 == 0 && (((uintptr_t)a.in) & 15) == 0, "conv: input view must be 16-byte aligned");
  HDF_CHECK_ARG(mode == 0 || a.stat_partials == nullptr, "conv: stats only in mode 0");
  HDF_CHECK_ARG(a.wfrag == 0 || hdf_conv_weight_layout(dtype, mode, a.Cin, a.Do, a.Ho, a.Wo) == 1,
                "conv: fragment-major weights given to a launch that reads row-major panels (mode %d Cin %d)", mode, a.Cin);
  HDF_CHECK_ARG(a.split == 0 || (mode == 0 && a.split % 32 == 0 && a.split < a.Cout && a.out2 != nullptr),
                "conv: split output needs mode 0, split %% 32 == 0 and a second buffer (split=%d)", a.split);
#ifndef HDF_NO_CONV_WR  // (A/B builds: the weights-stationary kernels for every launch)
  if (mode == 0 && hdf_conv_wr_takes(dtype, a)) return hdf_launch_conv_wr(dtype, a, st);
#endif
  HDF_DISPATCH_T(dtype, return launch_conv_t<T>(mode, a, st));
  return HDF_ERR_UNSUPPORTED;
}
