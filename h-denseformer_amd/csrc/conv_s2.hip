// The specialised stride-2 kernels of the transposed convolution ConvTranspose3d(k3,s2,p1,op1) and of its data gradient, the
// stride-2 gather conv.  conv_igemm.hip's launch_conv_t routes a launch here when a *_takes predicate accepts it and runs
// conv_igemm_kernel (one grid slice per output-parity class, or the generic stride-2 tiles) otherwise:
//   convt_fused_kernel     transposed conv, all parity classes in one workgroup; 3-D and FLAT (ConvTranspose2d)
//   convt_ws_kernel        16-bit transposed conv of the highest resolution (64 -> 32 channels): persistent, LDS-DMA
//   conv_gather_s2_kernel  16-bit data gradient of the same layer (32 -> 64 channels): persistent, LDS-DMA
#include "conv_igemm.h"
#include "conv_tile.h"
#include <type_traits>

namespace {

// ConvTranspose3d(k3,s2,p1,op1) forward with ALL 8 output-parity classes in one workgroup (Cin*sizeof(T) <= 128 B):
// the (TD+1)x(TH+1)x(TW+1) input box is staged ONCE with full-Cin rows, then each class runs its 1..8 taps and
// writes its 2x-strided outputs through an LDS staging tile as whole 16-byte chunks.  (The per-class launch of
// conv_igemm_kernel<CONVT> restaged the same box 8 times for ~3 taps of work each.)
// NFS = 32-byte fragment steps per voxel row (Cin*sizeof(T)/32): with the class and tap loops unrolled at compile time
// a class is straight-line code.  Written as run-time loops, hipcc carried the accumulators in VGPRs and bracketed
// EVERY pair of MFMAs with 64 v_accvgpr moves (SQ_INSTS_VALU 88 M against 57 M MFMA-busy cycles per launch: the kernel
// was VALU-bound at 280 TF); an `asm("" : "+a"(acc))` pin does not survive the dynamic-trip-count loop nest.
// (round 6) The weight fragments come straight from L2, one per pair of MFMAs, and hipcc kept ONE of them in flight
// (`s_waitcnt vmcnt(1)` in front of every pair: a 64-cycle pair waited out a 500+ cycle load -- 0.086 of the MFMA roof for
// upconv_2).  The 27 x NFS fragment steps of a workgroup are one compile-time sequence (class, tap, step): a register ring
// keeps CT_RING of them in flight across tap and class boundaries, as conv_igemm_kernel does for its chunks.
constexpr int CT_RING = 8;
// tap (in the [27] panel) of the k-th (class, tap) pair in the order the classes walk them, and the first pair of a class
constexpr int ct_class_base(int cls) {
  int n = 0;
  for (int c = 0; c < cls; c++) n += (((c >> 2) & 1) ? 2 : 1) * (((c >> 1) & 1) ? 2 : 1) * ((c & 1) ? 2 : 1);
  return n;
}
constexpr int ct_pair_tap(int k) {
  int idx = 0;
  for (int cls = 0; cls < 8; cls++) {
    const int pz = (cls >> 2) & 1, py = (cls >> 1) & 1, px = cls & 1;
    for (int jz = 0; jz < (pz ? 2 : 1); jz++)
      for (int jy = 0; jy < (py ? 2 : 1); jy++)
        for (int jx = 0; jx < (px ? 2 : 1); jx++) {
          if (idx == k) return (((pz ? 2 * jz : 1) * 3 + (py ? 2 * jy : 1)) * 3 + (px ? 2 * jx : 1));
          idx++;
        }
  }
  return 0;
}
// FLAT (round 6): ConvTranspose2d(k3, s2, p1, op1) of the 2-D model on depth-1 tensors -- the four (y, x) parity classes, the
// 9 taps of the panel's centre depth plane, a one-plane box; until then the 2-D decoder ran one launch slice per class
// through conv_igemm_kernel's unpipelined fallback loop.
template <typename T, int TD, int TH, int TW, int MB, int NFS, bool FLAT = false>
__global__ __launch_bounds__(256) void convt_fused_kernel(ConvArgs a) {
  static_assert(4 * MB * 32 == TD * TH * TW, "tile/wave decomposition");
  static_assert(!FLAT || TD == 1, "flat tiles are one voxel deep");
  constexpr int BD = FLAT ? 1 : TD + 1, BH = TH + 1, BW = TW + 1, BOX = BD * BH * BW;
  constexpr int ESZ = sizeof(T), EPC = ST<T>::EPC;
  constexpr int ROWB = NFS > 8 ? 512 : (NFS > 4 ? 256 : 128);  // row payload the box is laid out for (full Cin: up to 128 / 256 / 512 B)
  constexpr int LP = ROWB + 16;              // box row pitch
  static_assert(BOX * LP <= 160 * 1024, "LDS budget");
  __shared__ __attribute__((aligned(16))) char lds[BOX * LP];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int ntz = (a.Di + TD - 1) / TD, nty = (a.Hi + TH - 1) / TH, ntx = (a.Wi + TW - 1) / TW;
  int t = blockIdx.x;
  const int tx = t % ntx;
  t /= ntx;
  const int ty = t % nty;
  t /= nty;
  const int tz = t % ntz;
  const int n = t / ntz;
  const int z0 = tz * TD, y0 = ty * TH, x0 = tx * TW;
  const int n0 = blockIdx.y * 32;
  const int RB = a.Cin * ESZ;                // 32, 64, 128 or 256 bytes of channels per voxel (= 32 * NFS)

  stage_box<T, BD, BH, BW, ROWB, LP>(lds, reinterpret_cast<const T*>(a.in), a.in_pitch, a.Cin, n, a.Di, a.Hi, a.Wi, z0,
                                    y0, x0, 0, RB, a.in_scale, a.in_shift, a.in_relu);
  __syncthreads();

  int rowbase[MB];
#pragma unroll
  for (int mb = 0; mb < MB; mb++) {
    int lin = (wave * MB + mb) * 32 + r;
    int lz = lin / (TH * TW), ly = (lin / TW) % TH, lx = lin % TW;
    rowbase[mb] = ((lz * BH + ly) * BW + lx) * LP + h * 16;
  }
  const int ch = n0 + r;
  const bool ch_ok = ch < a.Cout;
  const float bias = (a.bias && ch_ok) ? a.bias[ch] : 0.f;
  const char* wrow = reinterpret_cast<const char*>(a.w) + ((int64_t)(n0 + r) * a.Cin) * ESZ + h * 16;
  const int64_t wtap_stride = (int64_t)a.CoutP * a.Cin * ESZ;
  // output voxel (2z, 2y, 2x) of every accumulator row of this lane, as an element offset inside the sample (-1: the
  // tile voxel lies outside the volume); a class adds its parity offset
  T* obase = reinterpret_cast<T*>(a.out) + (int64_t)n * a.Do * a.Ho * a.Wo * a.out_pitch + ch;
  int voff[MB][16];
#pragma unroll
  for (int mb = 0; mb < MB; mb++)
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const int lin = (wave * MB + mb) * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
      const int gz = z0 + lin / (TH * TW), gy = y0 + (lin / TW) % TH, gx = x0 + lin % TW;
      voff[mb][i] = (gz < a.Di && gy < a.Hi && gx < a.Wi) ? (((FLAT ? gz : 2 * gz) * a.Ho + 2 * gy) * a.Wo + 2 * gx) * (int)a.out_pitch : -1;
    }

  constexpr int NSTEP = (FLAT ? 9 : 27) * NFS;   // (flat: classes 0..3, the first 9 pairs of the sequence, all on depth tap 1)
  auto b_load = [&](int g) -> u32x4 {   // g: compile-time after unrolling
    return *reinterpret_cast<const u32x4*>(wrow + ct_pair_tap(g / NFS) * wtap_stride + (g % NFS) * 32);
  };
  u32x4 bq[CT_RING];
#pragma unroll
  for (int g = 0; g < CT_RING; g++) bq[g] = b_load(g);

  auto do_class = [&](auto cls_tag) __attribute__((always_inline)) {
    constexpr int cls = decltype(cls_tag)::value;
    constexpr int pz = (cls >> 2) & 1, py = (cls >> 1) & 1, px = cls & 1;
    constexpr int ntapz = pz ? 2 : 1, ntapy = py ? 2 : 1, ntapx = px ? 2 : 1;
    constexpr int g0 = ct_class_base(cls) * NFS;   // first fragment step of this class
    f32x16 acc[MB];
#pragma unroll
    for (int mb = 0; mb < MB; mb++)
#pragma unroll
      for (int i = 0; i < 16; i++) acc[mb][i] = 0.f;
#pragma unroll
    for (int jz = 0; jz < ntapz; jz++) {
      constexpr int dummy = 0;
      (void)dummy;
      const int offz = pz ? 1 - jz : 0, wz = pz ? 2 * jz : 1;
#pragma unroll
      for (int jy = 0; jy < ntapy; jy++) {
        const int offy = py ? 1 - jy : 0, wy = py ? 2 * jy : 1;
#pragma unroll
        for (int jx = 0; jx < ntapx; jx++) {
          const int offx = px ? 1 - jx : 0, wx = px ? 2 * jx : 1;
          const int tapoff = ((offz * BH + offy) * BW + offx) * LP;
          (void)wz, (void)wy, (void)wx;   // (the tap's panel index is ct_pair_tap of its position in the sequence)
#pragma unroll
          for (int fs = 0; fs < NFS; fs++) {
            const int g = g0 + ((jz * ntapy + jy) * ntapx + jx) * NFS + fs;
            const u32x4 bfrag = bq[g % CT_RING];
            u32x4 afrag[MB];
#pragma unroll
            for (int mb = 0; mb < MB; mb++)
              afrag[mb] = *reinterpret_cast<const u32x4*>(lds + rowbase[mb] + tapoff + fs * 32);
#pragma unroll
            for (int mb = 0; mb < MB; mb++) Mma<T>::run(afrag[mb], bfrag, acc[mb]);
            if (g + CT_RING < NSTEP) bq[g % CT_RING] = b_load(g + CT_RING);
            __builtin_amdgcn_sched_barrier(0);   // (without it hipcc sinks the refill down to its use again)
          }
        }
      }
    }
    // epilogue straight from the accumulators (lane = channel r, 16 tile voxels per M-block): 2-byte stores, 32 lanes =
    // one 64-byte voxel row.  No LDS staging, no barrier: a wave's stores of class c run under its MFMAs of class c+1
    // and under the other waves' work (the staged form cost two workgroup barriers and an LDS round trip per class)
    const int coff = ((pz * a.Ho + py) * a.Wo + px) * (int)a.out_pitch;
#pragma unroll
    for (int mb = 0; mb < MB; mb++)
#pragma unroll
      for (int i = 0; i < 16; i++)
        if (ch_ok && voff[mb][i] >= 0) ST<T>::st(obase + voff[mb][i] + coff, acc[mb][i] + bias);
  };
  do_class(std::integral_constant<int, 0>{});
  do_class(std::integral_constant<int, 1>{});
  do_class(std::integral_constant<int, 2>{});
  do_class(std::integral_constant<int, 3>{});
  if constexpr (!FLAT) {
    do_class(std::integral_constant<int, 4>{});
    do_class(std::integral_constant<int, 5>{});
    do_class(std::integral_constant<int, 6>{});
    do_class(std::integral_constant<int, 7>{});
  }
}

// ------------------------------------------------------------------------------------------------
// conv_gather_s2: 16-bit stride-2 gather conv with 64-byte input rows and 64 output channels -- the data gradient of
// the highest-resolution ConvTranspose3d (dX[v] = sum_tap W[tap]^T dY[2v - 1 + tap], 32 -> 64 channels): persistent
// workgroups, the same LDS-DMA double-buffered 9x9x9 box as conv_wgrad_s2_kernel, and WEIGHTS-STATIONARY REGISTERS.
// The generic kernel it replaces (conv_igemm_kernel<.,2,4,8,..,S=2>) ran one 64-voxel tile per workgroup (8192
// workgroups, each staging its box with per-slot index arithmetic and fetching every weight fragment from L2): 23 VALU
// instructions per MFMA, 63 % of the LDS cycles in bank conflicts (rows 2 apart), 268 TF.  Here
//  * wave (mb, nb) owns 32 of the tile's 64 voxels x 32 of the 64 output channels; its 27 x 2 weight fragments
//    (216 registers) are loaded once per launch;
//  * per tile a wave issues 54 MFMAs and 54 ds_read_b128 (two accumulator chains, A fragments two steps ahead) and
//    its share of the next tile's 12 LDS-DMA slots; nothing else;
//  * box rows keep the even-then-odd x order of conv_wgrad_s2_kernel (stride-2 neighbours = consecutive 64-byte rows),
//    and the 16-byte chunks of a row are XOR-swizzled by (box y >> 1) & 3 on the SOURCE side of the DMA (the LDS image
//    of an LDS-DMA is lane-linear), so the 16 lanes a ds_read_b128 services together (4 x positions x 4 different y)
//    cover all 64 banks.
template <typename T>
__global__ __launch_bounds__(256) void conv_gather_s2_kernel(ConvArgs a) {
  static_assert(sizeof(T) == 2, "16-bit storage only");
  constexpr int BX = 9, BOXL = BX * BX * BX, LP = 64, EPC = 8;
  constexpr int NL_ = (BOXL * 4 + 255) / 256, LBUF = NL_ * 256 * 16;  // the last slot's tail lanes land in padding
  constexpr int NS = 54;                                              // fragment steps per tile: 27 taps x 2
  __shared__ __attribute__((aligned(256))) char lds[2 * LBUF];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int mb = wave >> 1, nb = wave & 1;
  const int part = tid & 3, v0 = tid >> 2;
  const int ntz = a.Do / 4, nty = a.Ho / 4, ntx = a.Wo / 4;  // whole tiles (launcher check)
  const int num_tiles = a.N * ntz * nty * ntx;
  const int per = (num_tiles + gridDim.x - 1) / gridDim.x;
  const int t_begin = blockIdx.x * per, t_end = min(num_tiles, t_begin + per);
  if (t_begin >= t_end) return;

  // ---- weights -> registers (B operand: lane r = output channel, 8 k values at h)
  u32x4 wf[NS];
  {
    const char* wb = a.wfrag ? reinterpret_cast<const char*>(a.w) + nb * 2 * 1024 + r * 32 + h * 16
                             : reinterpret_cast<const char*>(a.w) + ((int64_t)(nb * 32 + r) * a.Cin) * 2 + h * 16;
    const int fstride = a.wfrag ? 1024 : 32;
    const int64_t wtap_stride = (int64_t)a.CoutP * a.Cin * 2;
#pragma unroll
    for (int s_ = 0; s_ < NS; s_++) wf[s_] = *reinterpret_cast<const u32x4*>(wb + (s_ >> 1) * wtap_stride + (s_ & 1) * fstride);
  }

  // ---- A fragment addresses: M-block row r = (lz & 1) * 16 + ly * 4 + lx, lz = 2 mb + (r >> 4)
  const int a_ly = (r >> 2) & 3;
  const int abase = (((2 * (2 * mb + (r >> 4))) * BX + 2 * a_ly) * BX + (r & 3)) * LP;
  int aoff[2][2];  // [tap y == 2][k-step]: byte offset of this lane's 16-byte chunk inside its row
#pragma unroll
  for (int y2 = 0; y2 < 2; y2++)
#pragma unroll
    for (int ks = 0; ks < 2; ks++) aoff[y2][ks] = abase + (((2 * ks + h) ^ ((a_ly + y2) & 3)) << 4);

  // ---- staging slots (per-thread constants): slot k = box row v0 + 64 k, this lane's chunk = part ^ swizzle(row)
  int goffL[NL_];
  uint32_t emz = 0, emy = 0, emx = 0, row_ok = 0;
#pragma unroll
  for (int k = 0; k < NL_; k++) {
    const int row = v0 + 64 * k;
    const int rc = min(row, BOXL - 1);
    const int line = rc / BX, pos = rc - line * BX;
    const int bx = pos < 5 ? 2 * pos : 2 * pos - 9, by = line % BX, bz = line / BX;
    const int chunk = part ^ ((by >> 1) & 3);
    goffL[k] = ((bz * a.Hi + by) * a.Wi + bx) * (int)a.in_pitch + chunk * EPC;
    emz |= (bz == 0 ? 1u : 0u) << k;
    emy |= (by == 0 ? 1u : 0u) << k;
    emx |= (bx == 0 ? 1u : 0u) << k;
    row_ok |= (row < BOXL ? 1u : 0u) << k;
  }
  const T* const zero_src = reinterpret_cast<const T*>(g_zero_line);
  const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)lds;
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
  auto issue_tile = [&](const Tl& c, int buf_off) __attribute__((always_inline)) {
    // box origin; may lie before the tensor (those slots read the zero line)
    const T* const lorg = reinterpret_cast<const T*>(a.in) +
                          ((((int64_t)c.n * a.Di + (2 * c.z0 - 1)) * a.Hi + (2 * c.y0 - 1)) * a.Wi + (2 * c.x0 - 1)) * a.in_pitch;
    const uint32_t off = (c.z0 == 0 ? emz : 0u) | (c.y0 == 0 ? emy : 0u) | (c.x0 == 0 ? emx : 0u);
    const uint32_t m = row_ok & ~off;
    const uint32_t wbase = __builtin_amdgcn_readfirstlane(lds_base + buf_off + wave * 1024);
#pragma unroll
    for (int k = 0; k < NL_; k++) {
      const T* p = ((m >> k) & 1u) ? lorg + goffL[k] : zero_src;
      uint32_t keep;  // inline asm: see conv_wgrad_s2_kernel
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep)
                   : "v"(p), "s"(wbase + (uint32_t)(k * 4096))
                   : "memory");
    }
  };

  // ---- epilogue constants: accumulator register i = M-block row (i & 3) + 8 (i >> 2) + 4 h
  const int ch = nb * 32 + r;
  const bool ch_ok = ch < a.Cout;
  const float bias = (a.bias && ch_ok) ? a.bias[ch] : 0.f;
  const bool ch_odd = r & 1;
  int eoff[8];  // accumulator rows 2 j and 2 j + 1 leave as one dword per lane (st_rows2)
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int i = 2 * j + (ch_odd ? 1 : 0);
    const int rr = (i & 3) + 8 * (i >> 2) + 4 * h;
    eoff[j] = (((2 * mb + (rr >> 4)) * a.Ho + ((rr >> 2) & 3)) * a.Wo + (rr & 3)) * (int)a.out_pitch - (ch_odd ? 1 : 0);
  }

  Tl T1;
  decode(t_begin, T1);
  issue_tile(T1, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  WS_BARRIER();
  int rd_off = 0;
  for (int t = t_begin; t < t_end; t++) {
    const Tl T0 = T1;
    if (t + 1 < t_end) {  // uniform
      decode(t + 1, T1);
      issue_tile(T1, LBUF - rd_off);
    }
    f32x16 acc[2];
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
      for (int i = 0; i < 16; i++) acc[c][i] = 0.f;
    auto rd = [&](int s_) {
      const int tap = s_ >> 1, ks = s_ & 1;
      const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
      const int pb = kx == 0 ? 0 : (kx == 1 ? 5 : 1);
      return *reinterpret_cast<const u32x4*>(lds + rd_off + aoff[ky == 2][ks] + ((kz * BX + ky) * BX + pb) * LP);
    };
    u32x4 af[3];
    af[0] = rd(0);
    af[1] = rd(1);
#pragma unroll
    for (int s_ = 0; s_ < NS; s_++) {
      if (s_ + 2 < NS) af[(s_ + 2) % 3] = rd(s_ + 2);
      Mma<T>::run(af[s_ % 3], wf[s_], acc[s_ & 1]);
      __builtin_amdgcn_sched_barrier(0);
    }
    // The next tile's box must have landed before the barrier.  vmcnt counts stores too and retires in order, so the
    // wait sits BEFORE this tile's stores (behind them it also waited for their write acknowledgements, ~1 us per
    // tile); the stores then drain under the next tile's MFMAs.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // epilogue: one dword per lane and pair of accumulator rows (16 lanes = 64 contiguous bytes of one voxel row)
    T* const obase = reinterpret_cast<T*>(a.out) +
                     ((((int64_t)T0.n * a.Do + T0.z0) * a.Ho + T0.y0) * a.Wo + T0.x0) * a.out_pitch + ch;
    if (ch_ok) {
#pragma unroll
      for (int j = 0; j < 8; j++)
        st_rows2<T>(obase + eoff[j], acc[0][2 * j] + acc[1][2 * j] + bias, acc[0][2 * j + 1] + acc[1][2 * j + 1] + bias, ch_odd);
    }
    WS_BARRIER();  // one buffer fully read, the other fully written
    rd_off = LBUF - rd_off;
  }
}

// ------------------------------------------------------------------------------------------------
// convt_ws: 16-bit ConvTranspose3d(k3,s2,p1,op1) forward for 128-byte input rows and <= 32 output channels (the
// highest-resolution up-convolution, 64 -> 32): persistent workgroups, LDS-DMA double-buffered input box, weights in
// registers.  convt_fused_kernel ran one 256-voxel tile per workgroup: generic per-slot staging, every weight
// fragment fetched from L2 at its point of use by all four waves, 3360 VALU instructions per wave for 216 MFMAs,
// SQ_WAIT_ANY 64 % of the wave cycles (310 TF).  Here
//  * the 8 output-parity classes (1,2,2,2,4,4,4,8 taps) are dealt to the waves as {7}, {6,5}, {3,4,0}, {1,2}: a
//    wave keeps the 16..32 weight fragments of ITS classes in registers for the whole launch and runs them over all
//    four 32-voxel M-blocks of a 4x4x8 tile (8 : 8 : 7 : 4 taps -- the matrix pipe is not the bound here);
//  * the (4+1)x(4+1)x(8+1) input box of tile t+1 lands by LDS-DMA while tile t is under the MFMAs; its
//    InstanceNorm/ReLU transform is applied in place, by the thread that loaded the chunk, between the two halves of
//    the wave's MFMA work (zero padding = slots that read the zero line and are skipped by the transform);
//  * 128-byte rows: the 16-byte chunk c of a box row sits in slot c ^ ((x >> 1) & 1 | (y & 3) << 1) (applied on the
//    source side of the DMA), so the 16 lanes one ds_read_b128 pass services (4 x 4 voxels in x, y) cover the 64 banks.
template <typename T>
__global__ __launch_bounds__(256) void convt_ws_kernel(ConvArgs a) {
  static_assert(sizeof(T) == 2, "16-bit storage only");
  constexpr int BD = 5, BH = 5, BW = 9, BOX = BD * BH * BW, LP = 128, EPC = 8;
  constexpr int NJ = (BOX * 8 + 255) / 256, LBUF = NJ * 256 * 16;  // 8 slots per thread; tail lanes land in padding
  __shared__ __attribute__((aligned(256))) char lds[2 * LBUF + 128 * 4];
  float* const s_xf = reinterpret_cast<float*>(lds + 2 * LBUF);  // [64 scale][64 shift]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int ntz = a.Di / 4, nty = a.Hi / 4, ntx = a.Wi / 8;  // whole tiles (launcher check)
  const int num_tiles = a.N * ntz * nty * ntx;
  const int per = (num_tiles + gridDim.x - 1) / gridDim.x;
  const int t_begin = blockIdx.x * per, t_end = min(num_tiles, t_begin + per);
  if (t_begin >= t_end) return;
  const bool xf = a.in_scale != nullptr;
  const float relu_lo = (xf && a.in_relu) ? 0.f : -INFINITY;

  // ---- A fragment addresses: M-block mb = tile z, row r = (ly, lx) = (r >> 3, r & 7)
  const int a_ly = r >> 3, a_lx = r & 7;
  const int abase = (a_ly * BW + a_lx) * LP;
  int aoff[2][2][4];  // [tap offset y][tap offset x][k-step]: byte offset of this lane's 16-byte chunk inside its row
#pragma unroll
  for (int oy = 0; oy < 2; oy++)
#pragma unroll
    for (int ox = 0; ox < 2; ox++) {
      const int gsw = (((a_lx + ox) >> 1) & 1) | (((a_ly + oy) & 3) << 1);
#pragma unroll
      for (int ks = 0; ks < 4; ks++) aoff[oy][ox][ks] = abase + (((2 * ks + h) ^ gsw) << 4);
    }

  // ---- staging slots (per-thread constants): slot k = 16-byte slot tid + 256 k of the lane-linear box image
  int goff[NJ], tboff[NJ];
  uint32_t emz = 0, emy = 0, emx = 0, row_ok = 0;
#pragma unroll
  for (int k = 0; k < NJ; k++) {
    const int q = tid + 256 * k, row = q >> 3, sl = q & 7;
    const int rc = min(row, BOX - 1);
    const int bz = rc / (BH * BW), by = (rc / BW) % BH, bx = rc % BW;
    const int chunk = sl ^ (((bx >> 1) & 1) | ((by & 3) << 1));
    goff[k] = ((bz * a.Hi + by) * a.Wi + bx) * (int)a.in_pitch + chunk * EPC;
    tboff[k] = chunk * EPC;
    emz |= (bz == BD - 1 ? 1u : 0u) << k;
    emy |= (by == BH - 1 ? 1u : 0u) << k;
    emx |= (bx == BW - 1 ? 1u : 0u) << k;
    row_ok |= (row < BOX ? 1u : 0u) << k;
  }
  const T* const zero_src = reinterpret_cast<const T*>(g_zero_line);
  const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)lds;
  struct Tl {
    int n, z0, y0, x0;
  };
  auto decode = [&](int t, Tl& c) {
    c.x0 = (t % ntx) * 8;
    t /= ntx;
    c.y0 = (t % nty) * 4;
    t /= nty;
    c.z0 = (t % ntz) * 4;
    c.n = t / ntz;
  };
  // only the HIGH faces of a box can leave the tensor (whole tiles)
  auto slots_ok = [&](const Tl& c) -> uint32_t {
    const uint32_t off = (c.z0 + 4 == a.Di ? emz : 0u) | (c.y0 + 4 == a.Hi ? emy : 0u) | (c.x0 + 8 == a.Wi ? emx : 0u);
    return row_ok & ~off;
  };
  auto issue_tile = [&](const Tl& c, uint32_t m, int buf_off) __attribute__((always_inline)) {
    const T* const org = reinterpret_cast<const T*>(a.in) + ((((int64_t)c.n * a.Di + c.z0) * a.Hi + c.y0) * a.Wi + c.x0) * a.in_pitch;
    const uint32_t wbase = __builtin_amdgcn_readfirstlane(lds_base + buf_off + wave * 1024);
#pragma unroll
    for (int k = 0; k < NJ; k++) {
      const T* p = ((m >> k) & 1u) ? org + goff[k] : zero_src;
      uint32_t keep;  // inline asm: see conv_wgrad_s2_kernel
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep)
                   : "v"(p), "s"(wbase + (uint32_t)(k * 4096))
                   : "memory");
    }
  };
  int tbl_n = -1;
  auto refresh_xf = [&](int n) {  // uniform
    __syncthreads();              // nobody still reads the previous table
    if (tid < 64) {
      s_xf[tid] = a.in_scale[(int64_t)n * a.Cin + tid];
      s_xf[64 + tid] = a.in_shift[(int64_t)n * a.Cin + tid];
    }
    tbl_n = n;
    __syncthreads();
  };
  // x*scale+shift (+relu) on this thread's own chunks of the box in buffer buf_off; padding slots stay zero
  auto transform_own = [&](uint32_t m, int buf_off) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < NJ; k++) {
      if ((m >> k) & 1u) {
        u32x4* const slot = reinterpret_cast<u32x4*>(lds + buf_off + (tid + 256 * k) * 16);
        float f[EPC];
        ST<T>::unpack(*slot, f);
        const float* tb = s_xf + tboff[k];
#pragma unroll
        for (int e = 0; e < EPC; e += 4) {
          const f32x4 u = *reinterpret_cast<const f32x4*>(tb + e);
          const f32x4 w = *reinterpret_cast<const f32x4*>(tb + 64 + e);
#pragma unroll
          for (int q = 0; q < 4; q++) f[e + q] = fmaxf(f[e + q] * u[q] + w[q], relu_lo);
        }
        *slot = ST<T>::pack(f);
      }
    }
  };

  // ---- epilogue constants: accumulator register i = M-block row (i & 3) + 8 (i >> 2) + 4 h = (ly, lx)
  const bool ch_ok = r < a.Cout;
  const float bias = (a.bias && ch_ok) ? a.bias[r] : 0.f;
  const bool ch_odd = r & 1;
  int eoff[8];  // accumulator rows 2 j and 2 j + 1 leave as one dword per lane (st_rows2)
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int i = 2 * j + (ch_odd ? 1 : 0);
    const int rr = (i & 3) + 8 * (i >> 2) + 4 * h;
    eoff[j] = ((2 * (rr >> 3)) * a.Wo + 2 * (rr & 7)) * (int)a.out_pitch - (ch_odd ? 1 : 0);
  }
  const int64_t wtap_stride = (int64_t)a.CoutP * a.Cin * 2;
  const char* const wrow = reinterpret_cast<const char*>(a.w) + ((int64_t)r * a.Cin) * 2 + h * 16;

  // One parity class = (pz, py, px); tap j of it = (jz, jy, jx) in [0, ntap) per axis: box offset (parity ? 1 - j : 0),
  // weight index (parity ? 2 j : 1).  The per-wave code below is straight-line: classes, taps and weight slots are
  // compile-time.
  u32x4 wf[32];
  int rd_off = 0;
  T* obase = nullptr;
  auto load_class_w = [&](auto cls_tag, auto slot0_tag) __attribute__((always_inline)) {
    constexpr int cls = decltype(cls_tag)::value, slot0 = decltype(slot0_tag)::value;
    constexpr int pz = (cls >> 2) & 1, py = (cls >> 1) & 1, px = cls & 1;
    constexpr int ny = py ? 2 : 1, nx = px ? 2 : 1, ntap = (pz ? 2 : 1) * ny * nx;
#pragma unroll
    for (int j = 0; j < ntap; j++) {
      const int jz = j / (ny * nx), jy = (j / nx) % ny, jx = j % nx;
      const int wz = pz ? 2 * jz : 1, wy = py ? 2 * jy : 1, wx = px ? 2 * jx : 1;
#pragma unroll
      for (int ks = 0; ks < 4; ks++)
        wf[slot0 + 4 * j + ks] = *reinterpret_cast<const u32x4*>(wrow + ((wz * 3 + wy) * 3 + wx) * wtap_stride + ks * 32);
    }
  };
  // taps [J0, J1) of class cls into acc (zeroed first when J0 == 0)
  auto run_class = [&](auto cls_tag, auto slot0_tag, auto j0_tag, auto j1_tag, f32x16 (&acc)[4]) __attribute__((always_inline)) {
    constexpr int cls = decltype(cls_tag)::value, slot0 = decltype(slot0_tag)::value;
    constexpr int J0 = decltype(j0_tag)::value, J1 = decltype(j1_tag)::value;
    constexpr int pz = (cls >> 2) & 1, py = (cls >> 1) & 1, px = cls & 1;
    constexpr int ny = py ? 2 : 1, nx = px ? 2 : 1;
    if constexpr (J0 == 0) {
#pragma unroll
      for (int mb = 0; mb < 4; mb++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[mb][i] = 0.f;
    }
    // step s = (tap j, k-step ks); the four A fragments of step s+1 are read under the MFMAs of step s
    u32x4 af[2][4];
    auto rd = [&](int s_) {
      const int j = s_ >> 2, ks = s_ & 3;
      const int jz = j / (ny * nx), jy = (j / nx) % ny, jx = j % nx;
      const int oz = pz ? 1 - jz : 0, oy = py ? 1 - jy : 0, ox = px ? 1 - jx : 0;
#pragma unroll
      for (int mb = 0; mb < 4; mb++)
        af[s_ & 1][mb] = *reinterpret_cast<const u32x4*>(lds + rd_off + aoff[oy][ox][ks] + (((mb + oz) * BH + oy) * BW + ox) * LP);
    };
    rd(4 * J0);
#pragma unroll
    for (int s_ = 4 * J0; s_ < 4 * J1; s_++) {
      if (s_ + 1 < 4 * J1) rd(s_ + 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int mb = 0; mb < 4; mb++) Mma<T>::run(af[s_ & 1][mb], wf[slot0 + s_], acc[mb]);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // stores of a finished class: one dword per lane and pair of accumulator rows (16 lanes = one 64-byte voxel row)
  auto store_class = [&](auto cls_tag, const f32x16 (&acc)[4]) __attribute__((always_inline)) {
    constexpr int cls = decltype(cls_tag)::value;
    constexpr int pz = (cls >> 2) & 1, py = (cls >> 1) & 1, px = cls & 1;
    const int coff = ((pz * a.Ho + py) * a.Wo + px) * (int)a.out_pitch;
    if (ch_ok) {
#pragma unroll
      for (int mb = 0; mb < 4; mb++) {
        T* const ob = obase + coff + (int64_t)(2 * mb) * a.Ho * a.Wo * a.out_pitch;
#pragma unroll
        for (int j = 0; j < 8; j++) st_rows2<T>(ob + eoff[j], acc[mb][2 * j] + bias, acc[mb][2 * j + 1] + bias, ch_odd);
      }
    }
  };
  using I0 = std::integral_constant<int, 0>;
  using I4 = std::integral_constant<int, 4>;
  using I8 = std::integral_constant<int, 8>;
  using I16 = std::integral_constant<int, 16>;
  using I24 = std::integral_constant<int, 24>;
#define CLS(c) std::integral_constant<int, c>{}
  if (wave == 0) {
    load_class_w(CLS(7), I0{});
  } else if (wave == 1) {
    load_class_w(CLS(6), I0{});
    load_class_w(CLS(5), I16{});
  } else if (wave == 2) {
    load_class_w(CLS(3), I0{});
    load_class_w(CLS(4), I16{});
    load_class_w(CLS(0), I24{});
  } else {
    load_class_w(CLS(1), I0{});
    load_class_w(CLS(2), I8{});
  }

  Tl T1;
  decode(t_begin, T1);
  uint32_t m1 = slots_ok(T1);
  if (xf) refresh_xf(T1.n);
  issue_tile(T1, m1, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (xf) transform_own(m1, 0);
  WS_BARRIER();
  for (int t = t_begin; t < t_end; t++) {
    const Tl T0 = T1;
    const bool v1 = t + 1 < t_end;
    if (v1) {  // uniform
      decode(t + 1, T1);
      m1 = slots_ok(T1);
      issue_tile(T1, m1, LBUF - rd_off);
      if (xf && T1.n != tbl_n) refresh_xf(T1.n);
    }
    obase = reinterpret_cast<T*>(a.out) + ((((int64_t)T0.n * a.Do + 2 * T0.z0) * a.Ho + 2 * T0.y0) * a.Wo + 2 * T0.x0) * a.out_pitch + r;
    // The next tile's box must have landed (and be transformed) before the barrier.  vmcnt counts stores too and
    // retires in order, so the wait sits after the first half of the wave's MFMAs and BEFORE the phase's first store:
    // behind stores it would also wait for their write acknowledgements.  The stores drain under the MFMAs that follow
    // (this phase's second half, the next phase's first).
    auto mid = [&]() __attribute__((always_inline)) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (xf && v1) transform_own(m1, LBUF - rd_off);
    };
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    f32x16 acc[4];
    if (wave == 0) {
      run_class(CLS(7), I0{}, I0{}, I4{}, acc);
      mid();
      run_class(CLS(7), I0{}, I4{}, I8{}, acc);
      store_class(CLS(7), acc);
    } else if (wave == 1) {
      run_class(CLS(6), I0{}, I0{}, I4{}, acc);
      mid();
      store_class(CLS(6), acc);
      run_class(CLS(5), I16{}, I0{}, I4{}, acc);
      store_class(CLS(5), acc);
    } else if (wave == 2) {
      run_class(CLS(3), I0{}, I0{}, I4{}, acc);
      mid();
      store_class(CLS(3), acc);
      run_class(CLS(4), I16{}, I0{}, I2{}, acc);
      store_class(CLS(4), acc);
      run_class(CLS(0), I24{}, I0{}, I1{}, acc);
      store_class(CLS(0), acc);
    } else {
      run_class(CLS(1), I0{}, I0{}, I2{}, acc);
      mid();
      store_class(CLS(1), acc);
      run_class(CLS(2), I8{}, I0{}, I2{}, acc);
      store_class(CLS(2), acc);
    }
    WS_BARRIER();  // one buffer fully read, the other fully written (and transformed)
    rd_off = LBUF - rd_off;
  }
#undef CLS
}

}  // namespace

// transposed conv: row widths convt_fused_kernel is instantiated for
bool hdf_convt_fused_rows(int row_bytes) {
  return row_bytes == 32 || row_bytes == 64 || row_bytes == 128 || row_bytes == 256 || row_bytes == 512;
}

// all parity classes in one workgroup: rows of 32 .. 512 bytes (n_filters = 48: 192-byte rows run per class); the flat form
// reads row-major panels only
bool hdf_convt_fused_takes(int dtype, const ConvArgs& a) {
  return hdf_convt_fused_rows(a.Cin * hdf_esz(dtype)) && !a.accumulate && (a.Di != 1 || !a.wfrag);
}

namespace {

template <typename T>
int launch_convt_fused_t(const ConvArgs& a, hipStream_t st) {
  const int nfs = a.Cin * (int)sizeof(T) / 32;
  if (a.Di == 1) {
    // all four parity classes in one workgroup, the box staged once, the weight fragments through a register ring
    dim3 grid(a.N * ceil_div(a.Hi, 16) * ceil_div(a.Wi, 16), a.CoutP / 32);
    if (nfs == 16)
      hipLaunchKernelGGL((convt_fused_kernel<T, 1, 16, 16, 2, 16, true>), grid, dim3(256), 0, st, a);
    else if (nfs == 8)
      hipLaunchKernelGGL((convt_fused_kernel<T, 1, 16, 16, 2, 8, true>), grid, dim3(256), 0, st, a);
    else if (nfs == 4)
      hipLaunchKernelGGL((convt_fused_kernel<T, 1, 16, 16, 2, 4, true>), grid, dim3(256), 0, st, a);
    else if (nfs == 2)
      hipLaunchKernelGGL((convt_fused_kernel<T, 1, 16, 16, 2, 2, true>), grid, dim3(256), 0, st, a);
    else
      hipLaunchKernelGGL((convt_fused_kernel<T, 1, 16, 16, 2, 1, true>), grid, dim3(256), 0, st, a);
    HDF_LAUNCH_CHECK();
    return HDF_OK;
  }
  dim3 grid(a.N * ceil_div(a.Di, 4) * ceil_div(a.Hi, 8) * ceil_div(a.Wi, 8), a.CoutP / 32);
  if (nfs == 16) {   // 512-byte rows (16-bit upconv_1: 256 -> 128 channels at the bottom of the decoder): 2-deep tiles, a 128 KB box
    dim3 grid2(a.N * ceil_div(a.Di, 2) * ceil_div(a.Hi, 8) * ceil_div(a.Wi, 8), a.CoutP / 32);
    hipLaunchKernelGGL((convt_fused_kernel<T, 2, 8, 8, 1, 16>), grid2, dim3(256), 0, st, a);
  } else if (nfs == 8)
    hipLaunchKernelGGL((convt_fused_kernel<T, 4, 8, 8, 2, 8>), grid, dim3(256), 0, st, a);
  else if (nfs == 4)
    hipLaunchKernelGGL((convt_fused_kernel<T, 4, 8, 8, 2, 4>), grid, dim3(256), 0, st, a);
  else if (nfs == 2)
    hipLaunchKernelGGL((convt_fused_kernel<T, 4, 8, 8, 2, 2>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((convt_fused_kernel<T, 4, 8, 8, 2, 1>), grid, dim3(256), 0, st, a);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

}  // namespace

int hdf_launch_convt_fused(int dtype, const ConvArgs& a, hipStream_t st) {
  HDF_CHECK_ARG(hdf_convt_fused_takes(dtype, a), "convt_fused: not a launch of this kernel (ask hdf_convt_fused_takes first)");
  HDF_DISPATCH_T(dtype, return launch_convt_fused_t<T>(a, st));
  return HDF_ERR_UNSUPPORTED;
}

bool hdf_conv_gather_s2_takes(int dtype, const ConvArgs& a) {
  // (st_rows2: one dword per lane pair = channels (c, c + 1): even channel count / pitch, 4-byte aligned view)
  return hdf_esz(dtype) == 2 && a.Cin * 2 == 64 && a.CoutP == 64 && a.Cout % 2 == 0 && a.out_pitch % 2 == 0 &&
         (reinterpret_cast<uintptr_t>(a.out) & 3) == 0 && !a.in_scale && !a.accumulate && a.Do % 4 == 0 && a.Ho % 4 == 0 &&
         a.Wo % 4 == 0 && a.Di == 2 * a.Do && a.Hi == 2 * a.Ho && a.Wi == 2 * a.Wo;
}

int hdf_launch_conv_gather_s2(int dtype, const ConvArgs& a, hipStream_t st) {
  HDF_CHECK_ARG(hdf_conv_gather_s2_takes(dtype, a), "conv_gather_s2: not a launch of this kernel (ask hdf_conv_gather_s2_takes first)");
  const int tiles = a.N * (a.Do / 4) * (a.Ho / 4) * (a.Wo / 4);
  const dim3 grid(std::min(tiles, hdf_cu_budget()));
  if (dtype == HDF_BF16)
    hipLaunchKernelGGL((conv_gather_s2_kernel<bf16_t>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((conv_gather_s2_kernel<f16_t>), grid, dim3(256), 0, st, a);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

bool hdf_convt_ws_takes(int dtype, const ConvArgs& a) {
  return hdf_esz(dtype) == 2 && a.Cin * 2 == 128 && a.CoutP == 32 && a.Cout % 2 == 0 && a.out_pitch % 2 == 0 &&
         (reinterpret_cast<uintptr_t>(a.out) & 3) == 0 && !a.accumulate && a.Di % 4 == 0 && a.Hi % 4 == 0 && a.Wi % 8 == 0 &&
         a.Do == 2 * a.Di && a.Ho == 2 * a.Hi && a.Wo == 2 * a.Wi;
}

int hdf_launch_convt_ws(int dtype, const ConvArgs& a, hipStream_t st) {
  HDF_CHECK_ARG(hdf_convt_ws_takes(dtype, a), "convt_ws: not a launch of this kernel (ask hdf_convt_ws_takes first)");
  const int tiles = a.N * (a.Di / 4) * (a.Hi / 4) * (a.Wi / 8);
  const dim3 grid(std::min(tiles, hdf_cu_budget()));
  if (dtype == HDF_BF16)
    hipLaunchKernelGGL((convt_ws_kernel<bf16_t>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((convt_ws_kernel<f16_t>), grid, dim3(256), 0, st, a);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
