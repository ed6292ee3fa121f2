// conv_wgrad2_kernel: the 16-bit stride-1 weight gradient, persistent and double-buffered, with the optional fused
// InstanceNorm(+ReLU) backward.  conv_wgrad.hip's hdf_launch_wgrad routes a launch here when hdf_wgrad2_takes accepts it,
// and sums the partial slabs the kernel leaves.
#include "conv_wgrad_tile.h"
#include <type_traits>

namespace {

// conv_wgrad2: bf16 stride-1 weight gradient with DOUBLE-BUFFERED tiles (same idea as conv_ws2_kernel).
// conv_wgrad_kernel (conv_wgrad.hip) spends ~3 cycles outside the matrix pipe per MFMA cycle: per-slot index arithmetic in the
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
  static_assert(wgrad_tile_is(1, TD, TH, TW), "the host counts tiles by WGRAD_TILES");
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
  const TrLane tl(lane);
  const int q = tl.q, hh = tl.hh, colb = tl.colb;
  // per tap; the voxel group tt and the k-step ride in the 16-bit immediate offset, the buffer is added per tile
  int sA, lB[NT];
  sA = (8 * hh + q) * LP + colb;
#pragma unroll
  for (int j = 0; j < NT; j++) {
    int kz, ky, kx;
    wgrad_tap(wave * NT + j, 27, kz, ky, kx);
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

  // tile schedule (conv_schedule.h): interior pass, then border pass; ragged channel blocks run every tile checked
  const WsSchedule<TD, TH, TW> sch(a.N, ntz, nty, ntx, chan_all, (int)gridDim.x, (int)blockIdx.x);
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
          sch.bor_next(c);
        else
          sch.int_next(c);
      };
      if constexpr (BORDER)
        sch.bor_init(T0, k);
      else
        sch.int_init(T0, k);
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
        A0[ks & 1] = tr_read(lds + sAw + ks * 16 * LP);
        A1[ks & 1] = tr_read(lds + sAw + ks * 16 * LP + 4 * LP);
      };
      auto read_b = [&](int ks, int j) {
        B0[j] = tr_read(lds + lBw[j] + koff(ks));
        B1[j] = tr_read(lds + lBw[j] + koff(ks) + 4 * LP);
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
        sch.bor_next(T2);
      else
        sch.int_next(T2);
      v2 = left >= 2;
      so2 = v2 ? s_org_of(T2) : s_safe;
      lo2 = v2 ? l_org_of(T2) : l_safe;
      ty2 = ap_ty_of(T2, v2), to2 = ap_to_of(T2, v2);
    };
    if (sch.int_cnt > 0) {  // interior pass: the unchecked copy, one run (its own back edge: nothing drained per tile)
      begin_pass(std::false_type{}, sch.int_begin, sch.int_cnt);
      more = true;
      while (more) {
        tile_phase(std::true_type{});
        step(std::false_type{});
      }
    }
    if (sch.bor_cnt > 0) {  // border pass: the checked copy
      begin_pass(std::true_type{}, sch.bor_begin, sch.bor_cnt);
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

template <typename T>
void launch_wgrad2_t(const WgradArgs& a, dim3 grid, hipStream_t st) {
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

}  // namespace

// 16-bit storage, stride 1, 3-D, no transform of the small operand (the large one: XFL)
bool hdf_wgrad2_takes(int dtype, int stride, const WgradArgs& a) {
  return hdf_esz(dtype) == 2 && stride == 1 && !a.sm_scale && a.Ds != 1;
}

int hdf_launch_wgrad2(int dtype, const WgradArgs& a, dim3 grid, hipStream_t st) {
  if (dtype == HDF_BF16)
    launch_wgrad2_t<bf16_t>(a, grid, st);
  else
    launch_wgrad2_t<f16_t>(a, grid, st);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
