// Forward direction of the persistent chain kernels: tf_chain_fwd_kernel and its launcher (structure, hand-off protocol and
// everything shared with the backward: tf_chain.h).
#include "tf_chain.h"

namespace {

template <bool TRAIN>
__global__ __launch_bounds__(CT) void tf_chain_fwd_kernel(ChainFwd a) {
  HDF_CHAIN_PRIO();
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const TfDims& d = a.d;
  const int DM = d.DM, DMF = d.DMF, ldF = DMF + 4, N = d.N, BN = d.B * N;
  float* s_F = sm;                        // [16][ldF] feature rows of the current block
  float* s_x = s_F + TT * ldF;            // [16][36]
  float* s_h = s_x + TT * LD32;           // [16][36]
  float* s_z = s_h + TT * LD32;           // [16][68]
  float* s_red = s_z + TT * LD64;         // [2][16][16]
  float* s_ob = s_red + 2 * 16 * 16;      // [16][36] attention output of the tile
  float* s_q = s_ob + TT * LD32;          // [16][100] q|k|v of the tile
  float* s_kv = s_q + TT * LDQ;           // [2][KVC][68] key / value chunks
  const int tid = threadIdx.x, lane = tid & 63, wave8 = tid >> 6, wave = wave8 & 3, col = lane & 15, g = lane >> 4;
  const bool cw = tid < 256;              // the token stages run on the first four waves (as tok_fwd_kernel)
  // blocks b and b + 8 share an XCD (speed only): the workgroups of a sequence meet in as few L2s as possible
  const int seq = blockIdx.x % a.nseq, tile = blockIdx.x / a.nseq;
  const int m = seq / d.B, bsm = seq - m * d.B;
  const int n0 = tile * TT, nvalid = min(TT, N - n0);
  const int t0k = bsm * N + n0;           // modality-local token index of tile row 0 (dropout index, row addresses)
  const int64_t mo = (int64_t)m * d.mstride, rb = (int64_t)m * BN;
  const DropF dr{TRAIN ? 1 : 0, d.seed, d.thresh24, d.keep_scale};   // (compile-time: no branch per element)
  auto tok = [&](int row) { return t0k + min(row, nvalid - 1); };
  float* pm = const_cast<float*>(a.params);
  unsigned* cnt = a.sync + seq * SYNC_LINE;
  unsigned* tmo = a.sync + a.nseq * SYNC_LINE;
  bool dead = false;
  const int nl = a.nb * 4;
  const int cw_col = 16 * (wave & 1) + col, c4w = 16 * wave + col;

  WFrag<2> f_wo{}, f_w1{};
  WFrag<4> f_w2{};
  WFrag<11> f_w0{};
  WFrag<2> f_q0{}, f_q1{};
  float p_bout = 0.f, p_b1 = 0.f, p_b2 = 0.f, p_b0 = 0.f;
  LnP ln2{}, ln1{};
  float h0r[4] = {0.f, 0.f, 0.f, 0.f};

  // Weights of the token phase that finishes layer L - 1 (POST): requested one attention phase ahead; those of the stages
  // that start layer L (PRE) at the top of the token phase, so that they arrive under the POST stages.  Only the four
  // waves that run the token stages load; the others ZERO their fragment registers (an `if` without that else keeps
  // the previous contents of all 92 registers live across the whole layer loop on the path that skips the request, and
  // the kernel spilled).  The last iteration re-requests the last layer for the same reason.
  auto request_post = [&](int L) __attribute__((always_inline)) {   // L >= 1
    const int Lp = L - 1;
    if (cw) {
      const float4* slot = a.wpack + ((int64_t)m * nl + Lp) * (CH_SLOT * 64);
      const float* rest = chain_w0(a.cw, pm, Lp >> 2, Lp & 3) + mo + 32 * (DM + 32 * (Lp & 3));
      pload(f_wo, slot, CH_WO + 2 * (wave & 1), 2);
      pload(f_w2, slot, CH_W2 + 4 * (wave & 1), 4);
      pload(f_w1, slot, CH_W1 + 2 * wave, 2);
      p_bout = rest[CO_BOUT + cw_col], p_b2 = rest[CO_B2 + cw_col], p_b1 = rest[CO_B1 + c4w];
      ln2 = ln_load(rest + CO_LN2G, rest + CO_LN2B);
    } else {
      f_wo = WFrag<2>{}, f_w2 = WFrag<4>{}, f_w1 = WFrag<2>{};
      p_bout = p_b2 = p_b1 = 0.f, ln2 = LnP{};
    }
  };
  auto request_pre = [&](int L) __attribute__((always_inline)) {
    const int Lc = min(L, nl - 1);
    if (cw) {
      const float4* slot = a.wpack + ((int64_t)m * nl + Lc) * (CH_SLOT * 64);
      const float* rest = chain_w0(a.cw, pm, Lc >> 2, Lc & 3) + mo + 32 * (DM + 32 * (Lc & 3));
      pload(f_w0, slot, CH_W0 + 11 * wave, (DM + 32 * (Lc & 3)) >> 5);   // fragment (k half = wave >> 1, tile = wave & 1)
      pload(f_q0, slot, CH_WQ + 2 * wave, 2);
      pload(f_q1, slot, CH_WQ + 2 * ((wave & 1) + 4), 2);
      p_b0 = rest[CO_B0 + cw_col];
      ln1 = ln_load(rest + CO_LN1G, rest + CO_LN1B);
    } else {
      f_w0 = WFrag<11>{}, f_q0 = WFrag<2>{}, f_q1 = WFrag<2>{};
      p_b0 = 0.f, ln1 = LnP{};
    }
  };

  {  // block 0's input rows (the patch embedding's output)
    const int c4n = DM >> 2;
    for (int i = tid; i < TT * c4n; i += CT) {
      const int row = i / c4n, c4 = (i - row * c4n) * 4;
      *reinterpret_cast<float4*>(s_F + row * ldF + c4) =
          *reinterpret_cast<const float4*>(a.F0 + (rb + tok(row)) * DMF + c4);
    }
  }

  for (int L = 0; L <= nl; L++) {
    const bool POST = L > 0, PRE = L < nl, OUT = POST && (L & 3) == 0;
    const int bp = (L - 1) >> 2, lp = (L - 1) & 3;   // layer finished here
    const int bq = L >> 2, lq = L & 3;               // layer started here
    // (laundered per iteration: left loop-invariant, hipcc hoists every row address of every stage out of the layer
    // loop as 64-bit values and spills them)
    int t0 = t0k;
    asm volatile("" : "+s"(t0));
    request_pre(L);
    CHAIN_STAMP(8);
    __syncthreads();
    CHAIN_STAMP(0);
    // ------------------------------------------------------------------ POST(bp, lp)
    if (POST) {
      float* sv = a.save + (int64_t)(L - 1) * a.rows * 232;
      float* h1s = sv + a.rows * 168;
      float* h2s = sv + a.rows * 200;
      float* Fp = a.F0 + (int64_t)bp * a.rows * DMF;
      const uint32_t site0 = hdf_site_id(m, bp, lp, 0);
      float h1r[4] = {0.f, 0.f, 0.f, 0.f};
      if (cw && wave < 2) {  // to_out + dropout + residual
        f32x4 acc = zero4();
        wmma(acc, f_wo, s_ob, LD32, 8, 0, 2);
        const int c = 16 * wave + col;
        const float bo = p_bout;
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = 4 * g + r, t = t0 + row;
          const float v = (acc[r] + bo) * dr.mask(site0 + 0, (uint32_t)t * 32 + c) + h0r[r];
          h1r[r] = v;
          s_h[row * LD32 + c] = v;
          if (row < nvalid) h1s[(rb + t) * 32 + c] = v;
        }
      }
      __syncthreads();
      CHAIN_STAMP(9);
#pragma unroll
      for (int pass = 0; pass < 2; pass++) {  // pass 0: h2 = ff(LN2(h1)) + h1 ; pass 1: feature = ff(LN2(h2))
        if (cw) ln32(s_h, s_x, ln2);
        __syncthreads();
        if (cw) {
          f32x4 acc = zero4();
          wmma(acc, f_w1, s_x, LD32, 8, 0, 2);
          const int c = 16 * wave + col;
          const float b1 = p_b1;
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const int row = 4 * g + r, t = t0 + row;
            s_z[row * LD64 + c] = gelu_f(acc[r] + b1) * dr.mask(site0 + 1 + 2 * pass, (uint32_t)t * 64 + c);
          }
        }
        __syncthreads();
        if (cw && wave < 2) {
          f32x4 acc = zero4();
          wmma(acc, f_w2, s_z, LD64, 16, 0, 4);
          const int c = 16 * wave + col;
          const float b2 = p_b2;
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const int row = 4 * g + r, t = t0 + row;
            const float gv = (acc[r] + b2) * dr.mask(site0 + 2 + 2 * pass, (uint32_t)t * 32 + c);
            if (pass == 0) {
              const float h2 = gv + h1r[r];
              s_h[row * LD32 + c] = h2;
              if (row < nvalid) h2s[(rb + t) * 32 + c] = h2;
            } else {
              const int fc = DM + 32 * lp + c;
              s_F[row * ldF + fc] = gv;
              if (row < nvalid) Fp[(rb + t) * DMF + fc] = gv;
            }
          }
        }
        __syncthreads();
        if (pass == 0) CHAIN_STAMP(10);
      }
    }
    CHAIN_STAMP(13);
    // ------------------------------------------------------------------ OUT(bp): DenseForward(DM+128 -> 64 -> DM)
    if (OUT) {
      const TfOutP po = chain_out(a.cw, pm, bp);
      const float4* oslot = a.wpack + (int64_t)d.M * nl * (CH_SLOT * 64) + ((int64_t)m * a.nb + bp) * (CO_SLOT * 64);
      float* next_F = PRE ? a.F0 + (int64_t)bq * a.rows * DMF : nullptr;
      const uint32_t siteo = hdf_site_id(m, bp, 4, 0);
      if (cw) {
        f32x4 acc = zero4();
        wmma_stream_p(acc, oslot, OA_F + 24 * wave, DMF >> 4, s_F, ldF, DMF >> 2);
        const int c = 16 * wave + col;
        const float ba = po.ba[mo + c];
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = 4 * g + r, t = t0 + row;
          s_z[row * LD64 + c] = gelu_f(acc[r] + ba) * dr.mask(siteo + 0, (uint32_t)t * 64 + c);
        }
      }
      __syncthreads();  // every wave is done reading s_F: its first DM columns become the next block's input
      if (cw) {
        for (int nn = 16 * wave; nn < DM; nn += 64) {
          f32x4 acc = zero4();
          wmma_stream_p(acc, oslot, OB_F + 4 * (nn >> 4), 4, s_z, LD64, 16);
          const int c = nn + col;
          const float bb = po.bb[mo + c];
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const int row = 4 * g + r, t = t0 + row;
            const float v = (acc[r] + bb) * dr.mask(siteo + 1, (uint32_t)t * DM + c);
            if (next_F) {
              s_F[row * ldF + c] = v;
              if (row < nvalid) next_F[(rb + t) * DMF + c] = v;
            } else if (row < nvalid) {
              const int64_t ai = ((int64_t)bsm * N + n0 + row) * ((int64_t)d.M * DM) + (int64_t)m * DM + c;
              if (a.dtype == HDF_BF16)
                ST<bf16_t>::st(reinterpret_cast<bf16_t*>(a.attnall) + ai, v);
              else if (a.dtype == HDF_F16)
                ST<f16_t>::st(reinterpret_cast<f16_t*>(a.attnall) + ai, v);
              else
                reinterpret_cast<float*>(a.attnall)[ai] = v;
            }
          }
        }
      }
      __syncthreads();
    }
    CHAIN_STAMP(1);
    if (!PRE) break;
    // ------------------------------------------------------------------ PRE(bq, lq): Linear0 + LN1 + to_qkv
    float* sv = a.save + (int64_t)L * a.rows * 232;
    {
      float* h0_out = sv;
      const int Kq = DM + 32 * lq;
      f32x4 acc = zero4();
      if (cw) {
        wmma(acc, f_w0, s_F, ldF, Kq >> 2, (wave >> 1) * (Kq >> 3), Kq >> 5);
        if (wave >= 2) {
#pragma unroll
          for (int r = 0; r < 4; r++) s_red[((wave & 1) * 16 + 4 * g + r) * 16 + col] = acc[r];
        }
      }
      __syncthreads();
      if (cw && wave < 2) {
        const int c = 16 * wave + col;
        const float b0 = p_b0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = 4 * g + r, t = t0 + row;
          const float h = acc[r] + s_red[(wave * 16 + row) * 16 + col] + b0;
          h0r[r] = h;
          s_h[row * LD32 + c] = h;
          if (row < nvalid) h0_out[(rb + t) * 32 + c] = h;
        }
      }
      __syncthreads();
      CHAIN_STAMP(11);
      if (cw) ln32(s_h, s_x, ln1);
      __syncthreads();
      CHAIN_STAMP(12);
      if (cw) {
        f32x4 acc1 = zero4();
        wmma(acc1, f_q0, s_x, LD32, 8, 0, 2);
#pragma unroll
        for (int r = 0; r < 4; r++) s_q[(4 * g + r) * LDQ + 16 * wave + col] = acc1[r];
        if (wave < 2) {
          f32x4 acc2 = zero4();
          wmma(acc2, f_q1, s_x, LD32, 8, 0, 2);
#pragma unroll
          for (int r = 0; r < 4; r++) s_q[(4 * g + r) * LDQ + 16 * (wave + 4) + col] = acc2[r];
        }
      }
      __syncthreads();
    }
    CHAIN_STAMP(2);
    // ------------------------------------------------------------------ publish q|k|v, per-sequence barrier
    float* qkvL = sv + a.rows * 32;                               // [rows][96] of this layer
    const __amdgpu_buffer_rsrc_t rq = chain_rsrc(qkvL + (rb + (int64_t)bsm * N) * 96);   // this sequence's rows
    if (tid < TT * 24) {
      const int row = tid / 24, c4 = (tid - row * 24) * 4;
      if (row < nvalid)
        st16_sc1(rq, (uint32_t)(((n0 + row) * 96 + c4) * 4), *reinterpret_cast<const float4*>(s_q + row * LDQ + c4));
    }
    if (a.frag) {   // the backward's operand records of this block: every wave its head (see FR_*)
      float* rec = a.frag + ((((int64_t)L * a.nseq + seq) * a.ntile + tile) * 8 + wave8) * FR_W;
      const bool vrow = col < nvalid;
      const float* qr = s_q + col * LDQ + wave8 * 4 + g;
      rec[FR_KA + lane] = vrow ? qr[32] : 0.f;
      rec[FR_VA + lane] = vrow ? qr[64] : 0.f;
      rec[FR_QA + lane] = vrow ? qr[0] * (0.5f * LOG2E) : 0.f;
      if (lane < 20) {
        const int c = lane >> 2, gg = lane & 3;
        float kq[4] = {0.f, 0.f, 0.f, 0.f}, qq[4] = {0.f, 0.f, 0.f, 0.f};
        if (c < 4) {
#pragma unroll
          for (int e = 0; e < 4; e++) {
            const float* r = s_q + (4 * gg + e) * LDQ + wave8 * 4 + c;
            const bool v = 4 * gg + e < nvalid;
            kq[e] = v ? r[32] : 0.f, qq[e] = v ? r[0] : 0.f;
          }
        }
        u32x2* ru = reinterpret_cast<u32x2*>(rec);
        if (a.dtype == HDF_F16) {
          ru[FR_KB / 2 + lane] = u32x2{pack_h2(kq[0], kq[1]), pack_h2(kq[2], kq[3])};
          ru[FR_QB / 2 + lane] = u32x2{pack_h2(qq[0], qq[1]), pack_h2(qq[2], qq[3])};
        } else {
          ru[FR_KB / 2 + lane] = u32x2{pack_bf2(kq[0], kq[1]), pack_bf2(kq[2], kq[3])};
          ru[FR_QB / 2 + lane] = u32x2{pack_bf2(qq[0], qq[1]), pack_bf2(qq[2], qq[3])};
        }
      }
    }
    chain_arrive(cnt);
    CHAIN_STAMP(3);
    request_post(L + 1);   // parameters: never written during the launch, plain loads
    const int head = wave8;
    const float bqv = s_q[col * LDQ + head * 4 + g] * (0.5f * LOG2E);
    chain_wait(cnt, (unsigned)(a.ntile * (L + 1)), tmo, a.ctl, dead);
    CHAIN_STAMP(4);
    // ------------------------------------------------------------------ attention of layer L: head = wave
    {
#pragma clang fp contract(off)   // explicit fmas only: attn_fwd_kernel's arithmetic, bit for bit (see there)
      const int NP = attn_rows(N), nchunk = (NP + KVC - 1) / KVC;
      // staging: thread -> rows (tid >> 3) and (tid >> 3) + 64 of the chunk, 16-byte part (tid & 7) of their K and V halves
      const int srow = tid >> 3, spart = tid & 7;
      float4 pk[2], pv[2];
      auto stage_load = [&](int c) __attribute__((always_inline)) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
          const int j = min(c * KVC + srow + 64 * h, N - 1);
          pk[h] = ld16_sc1(rq, (uint32_t)((j * 96 + 32 + 4 * spart) * 4));
          pv[h] = ld16_sc1(rq, (uint32_t)((j * 96 + 64 + 4 * spart) * 4));
        }
      };
      auto stage_store = [&](int c) __attribute__((always_inline)) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
          const bool real = c * KVC + srow + 64 * h < N;
          float* dst = s_kv + (c & 1) * (KVC * KVP) + (srow + 64 * h) * KVP + 4 * spart;
          // (component selects: `real ? pk : zero` on the float4s is a select between two ADDRESSES and goes through scratch)
          *reinterpret_cast<float4*>(dst) =
              make_float4(real ? pk[h].x : 0.f, real ? pk[h].y : 0.f, real ? pk[h].z : 0.f, real ? pk[h].w : 0.f);
          *reinterpret_cast<float4*>(dst + 32) =
              make_float4(real ? pv[h].x : 0.f, real ? pv[h].y : 0.f, real ? pv[h].z : 0.f, real ? pv[h].w : 0.f);
        }
      };
      stage_load(0);
      stage_store(0);
      __syncthreads();
      CHAIN_STAMP(5);
      float mx = -INFINITY, l = 0.f;
      f2 a01 = {0.f, 0.f}, a23 = {0.f, 0.f};
      // one block of 16 keys against the wave's 16 queries (attn_fwd_kernel's trip, operation for operation)
      auto trip = [&](const float4 (&v)[4], int j0, const f32x4& sc4, auto masked) __attribute__((always_inline)) {
        float sc[4];
        float mn = mx;
#pragma unroll
        for (int u = 0; u < 4; u++) {
          sc[u] = sc4[u];
          if (decltype(masked)::value) sc[u] = (j0 + 4 * g + u < N) ? sc[u] : -INFINITY;
          mn = fmaxf(mn, sc[u]);
        }
        const float mr = (mn == -INFINITY) ? 0.f : mn;
        const float cfac = __builtin_amdgcn_exp2f(mx - mr);
        float ps = 0.f;
        f2 b01 = {0.f, 0.f}, b23 = {0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const float pr = __builtin_amdgcn_exp2f(sc[u] - mr);
          const f2 pp = {pr, pr};
          ps += pr;
          b01 = __builtin_elementwise_fma(pp, lo2(v[u]), b01);
          b23 = __builtin_elementwise_fma(pp, hi2(v[u]), b23);
        }
        const f2 cc = {cfac, cfac};
        l = __builtin_fmaf(l, cfac, ps);
        a01 = __builtin_elementwise_fma(a01, cc, b01);
        a23 = __builtin_elementwise_fma(a23, cc, b23);
        mx = mn;
      };
      for (int c = 0; c < nchunk; c++) {
        if (c + 1 < nchunk) stage_load(c + 1);
        const float* sK = s_kv + (c & 1) * (KVC * KVP);
        const float* sKq = sK + col * KVP + head * 4 + g;         // + 16 k rows: the score MFMA's A operand of block k
        const float* sVq = sK + 4 * g * KVP + 32 + head * 4;      // + (16 k + u) rows: this lane's value rows of block k
        const int jbase = c * KVC;
        auto scores = [&](float ka) __attribute__((always_inline)) {
          f32x4 z = {0.f, 0.f, 0.f, 0.f};
          return __builtin_amdgcn_mfma_f32_16x16x4f32(ka, bqv, z, 0, 0, 0);
        };
        if (jbase + KVC <= N) {
          // whole chunk, no mask: all eight K operands requested at once, the value rows one block ahead of their use (with
          // one LDS round trip in front of the MFMA and one in front of the first P.V of every block the loop took 600
          // cycles per block at two waves per SIMD)
          constexpr int NT = KVC / ATRIP;
          float ka[NT];
#pragma unroll
          for (int k = 0; k < NT; k++) ka[k] = sKq[k * ATRIP * KVP];
          float4 v[2][4];
#pragma unroll
          for (int u = 0; u < 4; u++) v[0][u] = *reinterpret_cast<const float4*>(sVq + u * KVP);
          f32x4 cur = scores(ka[0]);
#pragma unroll
          for (int k = 0; k < NT; k++) {
            f32x4 nxt = cur;
            if (k + 1 < NT) {
              nxt = scores(ka[k + 1]);
#pragma unroll
              for (int u = 0; u < 4; u++)
                v[(k + 1) & 1][u] = *reinterpret_cast<const float4*>(sVq + ((k + 1) * ATRIP + u) * KVP);
            }
            __builtin_amdgcn_sched_barrier(0);
            trip(v[k & 1], jbase + k * ATRIP, cur, std::false_type{});
            cur = nxt;
          }
        } else {
          const int ntrip = (NP - jbase) / ATRIP;
          f32x4 cur = scores(sKq[0]);
          for (int k = 0; k < ntrip; k++) {
            const int j0 = jbase + k * ATRIP;
            const f32x4 nxt = scores(sKq[min(k + 1, ntrip - 1) * ATRIP * KVP]);
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) v[u] = *reinterpret_cast<const float4*>(sVq + (k * ATRIP + u) * KVP);
            __builtin_amdgcn_sched_barrier(0);
            if (j0 + ATRIP <= N)
              trip(v, j0, cur, std::false_type{});
            else
              trip(v, j0, cur, std::true_type{});
            cur = nxt;
          }
        }
        if (c + 1 < nchunk) stage_store(c + 1);
        __syncthreads();
      }
      CHAIN_STAMP(6);
      // merge the 4 key subsets of a query (lanes q, q + 16, q + 32, q + 48)
      // (same text in transformer.hip: attn_fwd_kernel: as one shared function it changed tf_chain_fwd_kernel's instruction order)
#pragma unroll
      for (int off = 16; off < 64; off <<= 1) {
        const float m2 = __shfl_xor(mx, off, 64), l2 = __shfl_xor(l, off, 64);
        const f2 b01 = {__shfl_xor(a01.x, off, 64), __shfl_xor(a01.y, off, 64)};
        const f2 b23 = {__shfl_xor(a23.x, off, 64), __shfl_xor(a23.y, off, 64)};
        const float mn = fmaxf(mx, m2);
        const float mr = (mn == -INFINITY) ? 0.f : mn;
        const float ca = __builtin_amdgcn_exp2f(mx - mr), cb = __builtin_amdgcn_exp2f(m2 - mr);
        const f2 ca2 = {ca, ca}, cb2 = {cb, cb};
        l = __builtin_fmaf(l, ca, l2 * cb);
        a01 = __builtin_elementwise_fma(a01, ca2, b01 * cb2);
        a23 = __builtin_elementwise_fma(a23, ca2, b23 * cb2);
        mx = mn;
      }
      if (g == 0) {
        const float inv = 1.f / l;
        const float4 o = make_float4(a01.x * inv, a01.y * inv, a23.x * inv, a23.y * inv);
        *reinterpret_cast<float4*>(s_ob + col * LD32 + head * 4) = o;
        const float lsv = __builtin_fmaf(mx, LN2, __logf(l));
        if (col < nvalid) {
          float* ob = sv + a.rows * 128;
          float* lse = sv + a.rows * 160;
          const int64_t R = rb + t0 + col;
          *reinterpret_cast<float4*>(ob + R * 32 + head * 4) = o;
          lse[R * 8 + head] = lsv;
        }
        if (a.frag)   // -lse log2(e) of every query, head-major: [layer][sequence][head][ntile * 16] behind the records
          a.frag[(int64_t)nl * a.nseq * a.ntile * 8 * FR_W + (((int64_t)L * a.nseq + seq) * 8 + head) * (a.ntile * TT) + n0 + col] =
              col < nvalid ? -lsv * LOG2E : -INFINITY;
      }
      CHAIN_STAMP(7);
    }
  }
  // a workgroup that gave up at a barrier overwrites its rows of the branch output with NaN (chain_wait; a marker of WHICH
  // rows were lost -- what makes the step's loss NaN is exec.hip's chain_poison_outputs_kernel)
  if (chain_any_dead(dead, reinterpret_cast<unsigned*>(s_red))) {
    const float qnan = __builtin_nanf("");
    for (int i = tid; i < nvalid * DM; i += CT) {
      const int row = i / DM, c = i - row * DM;
      const int64_t ai = ((int64_t)bsm * N + n0 + row) * ((int64_t)d.M * DM) + (int64_t)m * DM + c;
      if (a.dtype == HDF_BF16)
        ST<bf16_t>::st(reinterpret_cast<bf16_t*>(a.attnall) + ai, qnan);
      else if (a.dtype == HDF_F16)
        ST<f16_t>::st(reinterpret_cast<f16_t*>(a.attnall) + ai, qnan);
      else
        reinterpret_cast<float*>(a.attnall)[ai] = qnan;
    }
  }
}

}  // namespace

int tf_chain_forward(const TfDims& d, const TfChainP& cp, int nb, const float* params, float* F0, float* save,
                     void* attnall, unsigned* sync, void* wpack, float* frag, int dtype, hipStream_t st,
                     const TfChainCtl& ctl) {
  ChainFwd a{};
  const size_t shm = chain_fwd_lds(d);
  HDF_TRY(chain_args(a, tf_chain_shape_ok(d), "transformer chain", shm, d, cp, nb, dtype, wpack, sync, ctl));
  a.params = params, a.F0 = F0, a.save = save, a.attnall = attnall;
  a.frag = dtype == HDF_F32 ? nullptr : frag;
  const void* kern = d.training ? reinterpret_cast<const void*>(tf_chain_fwd_kernel<true>)
                                : reinterpret_cast<const void*>(tf_chain_fwd_kernel<false>);
  return chain_launch(kern, &a, a.nseq * a.ntile, shm, d, sync, st);
}
