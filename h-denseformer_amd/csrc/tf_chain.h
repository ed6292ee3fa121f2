// Persistent "chain" kernels of the multi-path dense Transformer branch: ALL dense layers of all blocks of every
// (modality, sample) sequence in ONE launch per direction (round 5).
//
// Reference: models/HDenseFormer.py:78-145 (DensePreConv_AttentionBlock.forward, Dense_TransformerBlock.forward) and
// :47-75 (Dense_Attention).  The launch chain it replaces (transformer_fused.hip + the attention kernels of
// transformer.hip: token kernel, attention, token kernel, ... = 49 + 24 launches per direction) stays as the path of
// shapes this kernel does not take, and as the bit-for-bit reference of its tests: every stage below performs the SAME
// fp32 operations in the SAME order as the kernel it mirrors.
//
// Structure.  A workgroup (512 threads) owns 16 consecutive tokens of ONE sequence for the whole launch.  Everything of a
// dense layer except the attention core is local to a token: the feature rows (the growing concat of
// HDenseFormer.py:91-98), h0 and the attention output stay in LDS / registers from layer to layer, the saved tensors of
// the backward are written on the way.  The attention of layer L needs the keys and values of the whole sequence: the
// workgroups of a sequence publish their 16 rows of q|k|v (write-through stores), add to the sequence's arrival counter
// and wait until all of them have arrived -- a per-sequence barrier, one per layer; sequences never wait for each other
// (HDenseFormer.py:93-101 has no cross-sequence term).  Then each of the 8 waves takes one head: its 16 queries against
// all keys, streamed through LDS in chunks of 128 keys (double-buffered), scores on v_mfma_f32_16x16x4_f32, exponentials
// and P.V on the VALU exactly as attn_fwd_kernel.  The weights of the next token phase are requested before the wait.
//
// Hand-off protocol (cdna_hip_programming.md Guideline 16, R1 with a counter; MI355X_MICROARCH.md "Valid forms", first
// row of the sc1 table): every payload store is a 16-byte sc1 (write-through) store, every storing wave drains
// (s_waitcnt vmcnt(0)), the workgroup's barrier, ONE lane adds to the agent-scope counter; the consumer polls that word
// with relaxed agent-scope loads from ONE lane, joins the workgroup's barrier, and EVERY load of handed-off bytes is an
// sc1 buffer load to registers.  Counters are monotonic within a launch (target = tiles x (phase + 1)) and zeroed by a
// hipMemsetAsync in front of every launch.  All workgroups of the grid must be resident (grid <= compute units, checked
// by the launcher); every spin is bounded by the 100 MHz real-time counter and leaves a timeout word behind.
//
// This header: what two or more of the three units share (private to them).  tf_chain_fwd.hip and tf_chain_bwd.hip hold
// one kernel and its launcher each; tf_chain_host.hip the weight-pack kernel, the sizes and support predicates of
// transformer.h, and the one place persistent launches are issued from (chain_launch).
#pragma once
#include "tf_attn.h"
#include "tf_tok.h"

// tf_chain_host.hip.  One persistent launch of `kern` (CT threads per workgroup, `args`: its ChainFwd / ChainBwd): opts the
// kernel into `shm` bytes of LDS, orders `st` behind the previous persistent launch of the process on this device, zeroes
// the arrival counters, launches, and records the launch for the next one.
int chain_launch(const void* kern, void* args, int grid, size_t shm, const TfDims& d, unsigned* sync, hipStream_t st);

namespace {

using namespace tftok;

constexpr int CT = 512;     // threads per workgroup: 8 waves = the 8 heads of Dense_Attention
constexpr int KVC = 128;    // keys per staged chunk
constexpr int KVP = 68;     // floats per row of a chunk image: K (8 heads x 4) | V (8 heads x 4) | pad
constexpr int LDQ = 100;    // row pitch of the q|k|v tile
constexpr int SYNC_LINE = 32;  // unsigned words per counter (128-byte lines)
// Operand records of the attention BACKWARD in the 16-bit storage modes.  A workgroup's tile is exactly one block of 16
// tokens of the score / accumulation MFMAs, so the token's owner can leave every operand any wave of the sequence will
// ever want from that block in the order the 64 lanes consume it: the backward's key / query loops then run on coalesced
// loads straight into registers -- no LDS image, no barrier, a prefetch ring -- where the first version staged every
// chunk of the sequence through LDS in each of the sequence's 32 workgroups (30 us per layer; this form: see DESIGN).
// Forward record per (layer, sequence, block, head), FR_W floats (plain stores: read by the backward LAUNCH):
constexpr int FR_KA = 0;      // [64] k of key (lane & 15), component (lane >> 4), zero for padded rows: score MFMA A operand
constexpr int FR_VA = 64;     // [64] v likewise                                                   (T = dO . v)
constexpr int FR_QA = 128;    // [64] q x 0.5 log2(e)                                              (dK/dV half)
constexpr int FR_KB = 192;    // [5][4] x 8 B: 16-bit k of keys 4g .. 4g+3, component c (row 4: zeros): B operand of dS . K
constexpr int FR_QB = 232;    // [5][4] x 8 B: 16-bit q likewise                                    (dS^T . Q)
constexpr int FR_W = 288;      // (16 spare floats: whole 128-byte lines)
// -lse log2(e) of the queries (-inf for padded rows) follows the records as [layer][sequence][head][ntile * 16]: a wave
// stages its head's row with two 16-byte loads per lane
// hand-off record of the backward per (layer parity, sequence, block, head), XG_W floats (sc1 stores and loads):
constexpr int XG_GA = 0;      // [64] dO of query (lane & 15), component (lane >> 4)
constexpr int XG_GB = 64;     // [5][4] x 8 B: 16-bit dO
constexpr int XG_W = 128;
// -delta of the queries follows the hand-off records as [parity][sequence][head][ntile * 16]

// ---- fragment-major weight copies.  A token-stage weight fragment (tf_tok.h: wload) is, per lane, a run of float4s of ONE
// row of the torch Linear weight: the 64 lanes of a load instruction touch 64 different cache lines, and 19 such loads per
// wave and layer made the REQUEST of a layer's weights cost 2-4 us of vector-cache line lookups per workgroup (measured:
// the phase scaled with the number of loading waves).  tf_chain_pack_kernel permutes every layer's matrices once per
// forward into units of 64 lanes x float4 = 1 KB in exactly the order the lanes consume them, so a fragment load reads 8
// whole lines.  Unit map of a layer's slot (CH_SLOT units):
constexpr int CH_WO = 0;     // to_out  [32][32]:  tile (0..1) x j (0..1)
constexpr int CH_W2 = 4;     // net.3   [32][64]:  tile (0..1) x j (0..3)
constexpr int CH_W1 = 12;    // net.0   [64][32]:  tile (0..3) x j (0..1)
constexpr int CH_WQ = 20;    // to_qkv  [96][32]:  tile (0..5) x j (0..1)
constexpr int CH_W0 = 32;    // Linear0 [32][Kq]:  (k half x tile) (0..3) x j (0 .. Kq/32 - 1 <= 10)
// backward (tok_bwd_kernel's column fragments: cload), same slot:
constexpr int CB_Q = 76;     // dt = dqkv Wqkv:   (o half x tile) (0..3) x j (0..2)      (12 scalars per lane)
constexpr int CB_W0 = 88;    // dF += dh0 W0:     tile (0 .. Kq/16 - 1 <= 23) x j (0..1)
constexpr int CB_W2 = 136;   // df = dg W2:       tile (0..3) x j (0..1)
constexpr int CB_W1 = 144;   // du = dz W1:       (o half x tile) (0..3) x j (0..1)
constexpr int CB_WO = 152;   // dO = dgo Wout:    (o half x tile) (0..3)
constexpr int CH_SLOT = 156;
// a block's out_layer, behind all layer slots: [M][nb][CO_SLOT] units
constexpr int OA_F = 0;      // wa rows   (wmma_stream: z = Wa F):        tile (0..3) x j (0 .. DMF/16 - 1 <= 23)
constexpr int OB_F = 96;     // wb rows   (wmma_stream: out = Wb f):      tile (0 .. DM/16 - 1 <= 15) x j (0..3)
constexpr int OB_B = 160;    // wb columns (cmma_stream: df = do Wb):     tile (0..3) x j (0 .. DM/16 - 1 <= 15)
constexpr int OA_B = 224;    // wa columns (cmma_stream: dF = dz Wa):     tile (0 .. DMF/16 - 1 <= 23) x j (0..3)
constexpr int CO_SLOT = 320;
// offsets (floats) of a layer's tensors behind its Linear0 weight [32][Kq] in the flat parameter buffer (state_dict order,
// entries padded to 16 floats; growth 32, mlp 64: HDenseFormer.py:79-89).  chain_digest checks the plan's table against them.
constexpr int CO_B0 = 0, CO_LN1G = 32, CO_LN1B = 64, CO_WQKV = 96, CO_WOUT = 3168, CO_BOUT = 4192, CO_LN2G = 4224,
              CO_LN2B = 4256, CO_W1 = 4288, CO_B1 = 6336, CO_W2 = 6400, CO_B2 = 8448;

struct ChainW {              // device-side parameter addressing (a checked digest of TfChainP)
  int32_t l0[4];             // Linear0 weight of layer l, floats from the block's base
  int32_t ooff[4];           // out_layer wa, ba, wb, bb
  int64_t blk0, blk_stride;
};
__device__ __forceinline__ float* chain_w0(const ChainW& cw, float* base, int b, int l) {
  return base + cw.blk0 + (int64_t)b * cw.blk_stride + cw.l0[l];
}
__device__ __forceinline__ TfOutP chain_out(const ChainW& cw, float* base, int b) {
  float* q = base + cw.blk0 + (int64_t)b * cw.blk_stride;
  return TfOutP{q + cw.ooff[0], q + cw.ooff[1], q + cw.ooff[2], q + cw.ooff[3]};
}

// this lane's fragment: units [unit0, unit0 + n4) of the slot (clamped like wload: never branch around a load)
template <int NF4>
__device__ __forceinline__ void pload(WFrag<NF4>& f, const float4* __restrict__ slot, int unit0, int n4) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < NF4; j++) f.v[j] = slot[(unit0 + (j < n4 ? j : 0)) * 64 + lane];
}
// column fragment of NS scalars = NS / 4 units
template <int NS>
__device__ __forceinline__ void cpload(CFrag<NS>& f, const float4* __restrict__ slot, int unit0) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < NS / 4; j++) {
    const float4 v = slot[(unit0 + j) * 64 + lane];
    f.v[4 * j] = v.x, f.v[4 * j + 1] = v.y, f.v[4 * j + 2] = v.z, f.v[4 * j + 3] = v.w;
  }
}
// wmma_stream / cmma_stream (tf_tok.h) on packed units: the same MFMA order, the weights of the next chunk in flight
__device__ __forceinline__ void wmma_stream_p(f32x4& acc, const float4* __restrict__ slot, int unit0, int n4, const float* sA,
                                              int lda, int KQ) {
  const int lane = threadIdx.x & 63;
  const float4* pw = slot + unit0 * 64 + lane;
  const float4* pa = reinterpret_cast<const float4*>(sA + (lane & 15) * lda + (lane >> 4) * KQ);
  float4 w[4], wn[4];
#pragma unroll
  for (int j = 0; j < 4; j++) w[j] = pw[min(j, n4 - 1) * 64];
  for (int c = 0; c < n4; c += 4) {
#pragma unroll
    for (int j = 0; j < 4; j++) wn[j] = pw[min(c + 4 + j, n4 - 1) * 64];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (c + j < n4) {
        const float4 av = pa[c + j];
        acc = mma4(acc, av, w[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) w[j] = wn[j];
  }
}
// OQ scalars per lane = OQ / 4 units
__device__ __forceinline__ void cmma_stream_p(f32x4& acc, const float4* __restrict__ slot, int unit0, const float* sA, int lda,
                                              int OQ) {
  const int lane = threadIdx.x & 63;
  const float4* pw = slot + unit0 * 64 + lane;
  const float4* pa = reinterpret_cast<const float4*>(sA + (lane & 15) * lda + (lane >> 4) * OQ);
  const int n4 = OQ >> 2;
  for (int c = 0; c < n4; c += 2) {
    const float4 w0 = pw[c * 64], w1 = pw[min(c + 1, n4 - 1) * 64];
    {
      const float4 av = pa[c];
      acc = mma4(acc, av, w0);
    }
    if (c + 1 < n4) {
      const float4 av = pa[c + 1];
      acc = mma4(acc, av, w1);
    }
  }
}

// ---- hand-off pieces
// 16-byte write-through store / L1-bypassing load (sc1): buffer instructions with a raw resource over the whole tensor
__device__ __forceinline__ __amdgpu_buffer_rsrc_t chain_rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ void st16_sc1(__amdgpu_buffer_rsrc_t r, uint32_t byte_off, const float4& v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, byte_off, 0, 16);
}
__device__ __forceinline__ float4 ld16_sc1(__amdgpu_buffer_rsrc_t r, uint32_t byte_off) {
  return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 16));
}
// arrival: called by the whole workgroup after its payload stores
__device__ __forceinline__ void chain_arrive(unsigned* cnt, bool storing = true) {
  if (storing) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // EVERY storing wave drains its write-through stores
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// wait until the counter reaches `target`; one lane polls, the workgroup's barrier releases the others.  `dead` is the
// workgroup's sticky give-up flag (lane 0's copy decides; after a timeout no further wait is attempted).
// Giving up (round 6; rounds 5 trapped here, which killed the caller's HIP context): a sibling that has not arrived within
// `c.ticks` of the 100 MHz real-time counter means the grid is not resident together -- the device is shared with something
// that holds compute units.  The workgroup then leaves 1 + its id in the sync region's timeout word AND in the plan's
// host-mapped flag word (system scope: the host reads it without synchronising, exec.hip chain_flag_check), stops waiting
// for the rest of the launch and runs to the end on whatever it reads; every other workgroup sees the word in its own poll
// loop and does the same, so the launch ends within about one timeout.  Its results are garbage BY DEFINITION: dead
// workgroups overwrite their rows of the branch output with NaN at the end of the kernel (which rows were lost: NaN does
// not survive relu(InstanceNorm(.)) = fmaxf(.., 0) downstream), the plan's last launch of the call turns the head of every
// output / of the gradient buffer into NaN when the timeout word is set (exec.hip: chain_poison_*_kernel), so the step's
// loss and optimizer step are NaN rather than plausible, and the plan's next call returns HDF_ERR_CHAIN_TIMEOUT once and
// routes this plan to the launch chain from then on.
using ChainCtl = TfChainCtl;   // (transformer.h: host-mapped flag word + give-up deadline)
__device__ __forceinline__ void chain_wait(unsigned* cnt, unsigned target, unsigned* tmo, const ChainCtl& c, bool& dead) {
  if (threadIdx.x == 0 && !dead) {
    const uint64_t t_start = __builtin_amdgcn_s_memrealtime();
    unsigned spins = 0;
    while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      __builtin_amdgcn_s_sleep(2);
      if ((++spins & 31u) == 0u && __hip_atomic_load(tmo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
        dead = true;   // a sibling (of any sequence) gave up: the launch is lost, do not sit out a deadline of our own
        break;
      }
      if (__builtin_amdgcn_s_memrealtime() - t_start > (uint64_t)c.ticks) {
        __hip_atomic_store(tmo, 1u + blockIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c.host_flag) __hip_atomic_store(c.host_flag, 1u + blockIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        dead = true;
        break;
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // (no instruction: keeps the loads below the poll)
  __syncthreads();
}
// lane 0's give-up flag -> the whole workgroup (uniform result); `word`: any LDS word nobody reads across this call
__device__ __forceinline__ bool chain_any_dead(bool dead, unsigned* word) {
  __syncthreads();
  if (threadIdx.x == 0) *word = dead ? 1u : 0u;
  __syncthreads();
  return *word != 0u;
}

// -DCHAIN_DBG_STAMPS: lane 0 of every workgroup leaves the 100 MHz real-time counter at the phase boundaries of every layer
// in the second megabyte of the sync region (tools/chain_stamps.py); measurement builds only
#ifdef CHAIN_DBG_STAMPS
#define CHAIN_STAMP(k)                                                                                   \
  do {                                                                                                   \
    if (threadIdx.x == 0)                                                                                \
      reinterpret_cast<uint64_t*>(a.sync + (1 << 18))[((size_t)blockIdx.x * 32 + L) * 16 + (k)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#define CHAIN_STAMPB(k)                                                                                  \
  do {                                                                                                   \
    if (threadIdx.x == 0)                                                                                \
      reinterpret_cast<uint64_t*>(a.sync + (1 << 18) + (1 << 17))[((size_t)blockIdx.x * 32 + (L + 1)) * 16 + (k)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#else
#define CHAIN_STAMP(k) ((void)0)
#define CHAIN_STAMPB(k) ((void)0)
#endif

// ---- kernel arguments (the members the two structs share are filled by chain_args)
struct ChainFwd {
  TfDims d;
  ChainW cw;
  const float* params;
  const float4* wpack;   // [M][nl][CH_SLOT][64] fragment-major weights (tf_chain_pack_kernel)
  int dtype;             // storage type of attnall
  float* F0;        // [nb][rows][DMF]
  float* save;      // [nb*4][rows][232] (tf_save layout: h0 | qkv | ob | lse | h1 | h2, segment-major)
  void* attnall;    // channels-last [B][N][M*DM], storage dtype
  unsigned* sync;   // [nseq + 1][SYNC_LINE]: arrival counters, then the timeout word
  TfChainCtl ctl;
  float* frag;      // [nl][nseq][ntile][8][FR_W] operand records for the backward (16-bit storage modes), or null
  int nb, ntile, nseq;
  int64_t rows;
};

struct ChainBwd {
  TfDims d;
  ChainW cw;
  const float* params;
  float* grads;
  const float* F0;        // [nb][rows][DMF]
  const float* save;      // tf_save layout
  float* dF;              // [rows][DMF]: columns [0, DM) = gradient of block 0's input on return
  const void* d_attnall;  // storage dtype
  const float4* wpack;    // fragment-major weights (written by the forward's pack launch: same parameters)
  float* tape;            // [nb*4][TF_TAPE_W segments][rows]
  float* otape;           // [nb][DMF segments][rows]
  float* xchg;            // hand-off scratch, by layer parity: [2][rows][40] dO | delta rows (exact mode) or
                          // [2][nseq][ntile][8][XG_W] operand records (16-bit modes)
  const float* frag;      // the forward's operand records (16-bit modes)
  unsigned* sync;         // [nseq + 1][SYNC_LINE]
  TfChainCtl ctl;
  int nb, ntile, nseq, dtype;
  int64_t rows;
};

constexpr int QC = 64;      // rows per staged chunk of the attention backward
constexpr int QP = 84;      // floats per row of the dK/dV chunk image: q (32) | dO (32) | pad; K|V image uses KVP
constexpr int XW = 40;      // hand-off row: dO (32) | delta (8)

// dynamic LDS of the two kernels (their s_* layouts)
inline size_t chain_bwd_lds(const TfDims& d, int dtype) {
  const size_t tiles = (size_t)2 * TT * (d.DMF + 4) + TT * (d.DM + 4) + TT * 100 + 7 * TT * LD32 + 2 * TT * LD64 + 2 * 16 * 16 + TT * 8;
  const size_t att = dtype == HDF_F32 ? (size_t)2 * (QC * QP + 2 * 8 * QC + 2 * (8 * 5 * QC / 2)) : (size_t)2 * 8 * attn_rows(d.N);
  return (tiles + att) * sizeof(float);
}
inline size_t chain_fwd_lds(const TfDims& d) {
  return (size_t)(TT * (d.DMF + 4) + 2 * TT * LD32 + TT * LD64 + 2 * 16 * 16 + TT * LD32 + TT * LDQ + 2 * KVC * KVP) *
         sizeof(float);
}

// the plan's parameter table in the form the kernels address it; false when it is not the regular layout they assume
// (CO_*).  Here and not in tf_chain_host.hip: ChainW is part of the kernels' signatures and so of this unnamed namespace.
inline bool chain_digest(const TfChainP& cp, int DM, ChainW& w) {
  static const int rel[13] = {0, CO_B0, CO_LN1G, CO_LN1B, CO_WQKV, CO_WOUT, CO_BOUT, CO_LN2G, CO_LN2B, CO_W1, CO_B1, CO_W2, CO_B2};
  for (int l = 0; l < 4; l++) {
    w.l0[l] = cp.loff[l][0];
    for (int k = 1; k < 13; k++)
      if (cp.loff[l][k] != cp.loff[l][0] + 32 * (DM + 32 * l) + rel[k]) return false;
  }
  for (int k = 0; k < 4; k++) w.ooff[k] = cp.ooff[k];
  w.blk0 = cp.blk0, w.blk_stride = cp.blk_stride;
  return true;
}

// what tf_chain_forward and tf_chain_backward check and fill alike (Args = ChainFwd / ChainBwd; `shape_ok`: the direction's
// own predicate, `shm`: its LDS bytes, `what`: its name in the LDS message)
template <typename Args>
int chain_args(Args& a, bool shape_ok, const char* what, size_t shm, const TfDims& d, const TfChainP& cp, int nb, int dtype,
               const void* wpack, unsigned* sync, const TfChainCtl& ctl) {
  HDF_CHECK_ARG(shape_ok, "transformer chain: shape not supported (M %d B %d N %d DM %d)", d.M, d.B, d.N, d.DM);
  HDF_CHECK_ARG(chain_digest(cp, d.DM, a.cw), "transformer chain: irregular parameter layout");
  HDF_CHECK_ARG(shm <= LDS_LIMIT, "%s: %zu B of LDS", what, shm);
  HDF_CHECK_ARG(dtype == HDF_F32 || dtype == HDF_BF16 || dtype == HDF_F16, "unsupported dtype %d", dtype);
  a.d = d, a.dtype = dtype, a.wpack = reinterpret_cast<const float4*>(wpack), a.sync = sync, a.ctl = ctl;
  a.nb = nb, a.ntile = ceil_div(d.N, TT), a.nseq = d.M * d.B, a.rows = (int64_t)d.M * d.B * d.N;
  return HDF_OK;
}

}  // namespace
