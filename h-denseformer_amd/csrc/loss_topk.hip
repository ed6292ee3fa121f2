// TopKLoss (reference loss/cross_entropy.py:26-43) on the device, and the stand-alone exact top-K select it rests on.
//
//   topk_ce_kernel     one read of the logits: res[v] = w[t_v] * nll_v (0 where t_v == ignore_index), fp32, to the workspace,
//                      and the first radix histogram in the same pass
//   topk_hist_kernel   one radix pass (11 / 11 / 10 bits of the 32-bit key): grid-stride, LDS histogram, one global
//                      integer atomic per non-empty bin (the shape of surface_gather_kernel)
//   topk_pick_kernel   one workgroup between passes: the bin that holds the K-th largest key and what is left to take in it
//   topk_count_kernel  per block (a contiguous range of indices): how many keys are above the threshold, how many equal it
//   topk_scan_kernel   one workgroup: exclusive scans of the block counts -> each block's first output position and the
//                      number of ties before it
//   topk_write_kernel  rank[v] (-1: not selected), the selected values in index order, fp64 partial sums in a fixed order
//   topk_mean_kernel   one workgroup: the fp64 mean, rounded to fp32 once
//   topk_bwd_kernel    g * w[t] * (p_c - [c == t]) on the selected voxels, exact zeros elsewhere
//
// The key orders every float like its value: sign-flip (negative: all bits inverted; else the sign bit set), so -0.0 is
// below +0.0, and every NaN maps to the largest key (torch.topk counts NaN as the largest value).  Among values equal to the
// threshold the lowest index is taken first.  No kernel waits on another workgroup: every dependency between the phases is
// a kernel boundary on the caller's stream.  The only atomics are integer adds, so two runs on one input agree in every bit.
#include <algorithm>
#include <type_traits>

#include "../../include/hdf.h"
#include "loss_topk.h"

namespace {
constexpr int MAXC = HDF_CLASS_SLOTS;
constexpr int TOPK_BLOCKS = 1024;   // cap of the block rows of the compaction and of the forward voxel pass (all samples)
constexpr int HIST0 = 0, HIST1 = 2048, HIST2 = 4096, HIST_WORDS = 5120;

struct TopkState {
  uint32_t prefix;  // key bits decided so far, in place; after the last pick the threshold key
  uint32_t krem;    // values still to take inside the chosen bin; after the last pick the ties taken
  uint32_t gt;      // values above the chosen bin
  uint32_t pad;
};
// layout of the select's state (HDF_TOPK_SELECT_WS bytes); hist and state are zeroed by one memset per call
struct TopkWs {
  uint32_t* hist;       // [HIST_WORDS]
  TopkState* state;
  uint32_t* blockcnt;   // [TOPK_BLOCKS][2]: above, equal
  uint32_t* blockoff;   // [TOPK_BLOCKS][2]: first output position, ties before the block
  double* blocksum;     // [TOPK_BLOCKS]
};
constexpr int64_t OFF_STATE = HIST_WORDS * 4, OFF_CNT = OFF_STATE + 64, OFF_OFF = OFF_CNT + TOPK_BLOCKS * 8,
                  OFF_SUM = OFF_OFF + TOPK_BLOCKS * 8, OFF_END = OFF_SUM + TOPK_BLOCKS * 8;
static_assert(OFF_END <= HDF_TOPK_SELECT_WS && OFF_SUM % 8 == 0, "select workspace layout");

TopkWs topk_ws(void* ws) {
  char* b = reinterpret_cast<char*>(ws);
  return TopkWs{reinterpret_cast<uint32_t*>(b), reinterpret_cast<TopkState*>(b + OFF_STATE),
                reinterpret_cast<uint32_t*>(b + OFF_CNT), reinterpret_cast<uint32_t*>(b + OFF_OFF),
                reinterpret_cast<double*>(b + OFF_SUM)};
}

__device__ __forceinline__ uint32_t topk_key(float f) {
  const uint32_t u = __float_as_uint(f);
  if (f != f) return 0xffffffffu;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint32_t topk_key_bits(uint32_t key) {   // the float whose key this is (NaN: the quiet NaN)
  if (key == 0xffffffffu) return 0x7fc00000u;
  return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
}

template <int PASS>
struct Radix {
  static constexpr int BITS = PASS == 2 ? 10 : 11;
  static constexpr int SHIFT = PASS == 0 ? 21 : PASS == 1 ? 10 : 0;
  static constexpr int BINS = 1 << BITS;
  static constexpr uint32_t DECIDED = PASS == 0 ? 0u : PASS == 1 ? 0xffe00000u : 0xfffffc00u;
  static constexpr int HIST = PASS == 0 ? HIST0 : PASS == 1 ? HIST1 : HIST2;
};

__device__ __forceinline__ void flush_hist(const uint32_t* lh, int bins, uint32_t* __restrict__ hist) {
  for (int b = threadIdx.x; b < bins; b += blockDim.x)
    if (lh[b]) atomicAdd(&hist[b], lh[b]);
}

// ------------------------------------------------------------------------------------------------ radix pass
// HIST_THREADS threads a block and at most HIST_GRID blocks: a pass whose candidates fill every bin flushes blocks x bins
// global atomics onto the same 8 KiB (1024 blocks of 256 threads: 2 M adds, 22 us at 2 x 128^3; this shape: a quarter)
constexpr int HIST_THREADS = 1024, HIST_GRID = 256;
template <int PASS>
__global__ __launch_bounds__(HIST_THREADS) void topk_hist_kernel(const float* __restrict__ values, int64_t n,
                                                        const TopkState* __restrict__ state,
                                                        uint32_t* __restrict__ hist_all) {
  using R = Radix<PASS>;
  __shared__ uint32_t lh[R::BINS];
  for (int b = threadIdx.x; b < R::BINS; b += HIST_THREADS) lh[b] = 0;
  __syncthreads();
  const uint32_t prefix = PASS ? state->prefix : 0u;
  auto add = [&](float f) {
    const uint32_t key = topk_key(f);
    if ((key & R::DECIDED) == prefix) atomicAdd(&lh[(key >> R::SHIFT) & (R::BINS - 1)], 1u);
  };
  const int64_t gtid = (int64_t)blockIdx.x * HIST_THREADS + threadIdx.x, gstride = (int64_t)gridDim.x * HIST_THREADS;
  const int64_t nq = (reinterpret_cast<uintptr_t>(values) & 15) == 0 ? n >> 2 : 0;   // 16-byte loads where aligned
  for (int64_t q = gtid; q < nq; q += gstride) {
    const f32x4 v = reinterpret_cast<const f32x4*>(values)[q];
    add(v[0]), add(v[1]), add(v[2]), add(v[3]);
  }
  for (int64_t i = nq * 4 + gtid; i < n; i += gstride) add(values[i]);
  __syncthreads();
  flush_hist(lh, R::BINS, hist_all + R::HIST);
}

// One workgroup.  Walking the bins from the top, the chosen bin is the one in which the running count first reaches what
// is still to take; exactly one (thread, bin) pair meets the condition (1 <= krem <= the histogram's total).
template <int PASS>
__global__ __launch_bounds__(256) void topk_pick_kernel(const uint32_t* __restrict__ hist_all, int64_t K,
                                                        TopkState* __restrict__ state,
                                                        unsigned long long* __restrict__ result) {
  using R = Radix<PASS>;
  constexpr int PER = R::BINS / 256;
  __shared__ uint32_t part[256];
  const uint32_t* hist = hist_all + R::HIST;
  const uint32_t krem = PASS ? state->krem : (uint32_t)K;
  uint32_t h[PER], s = 0;
#pragma unroll
  for (int j = 0; j < PER; j++) {
    h[j] = hist[threadIdx.x * PER + j];
    s += h[j];
  }
  part[threadIdx.x] = s;
  __syncthreads();
  uint32_t run = 0;
  for (int j = threadIdx.x + 1; j < 256; j++) run += part[j];
#pragma unroll
  for (int j = PER - 1; j >= 0; j--) {
    if (run < krem && run + h[j] >= krem) {
      const uint32_t prefix = (PASS ? state->prefix : 0u) | ((uint32_t)(threadIdx.x * PER + j) << R::SHIFT);
      const uint32_t gt = (PASS ? state->gt : 0u) + run;
      state->prefix = prefix;
      state->krem = krem - run;
      state->gt = gt;
      if (PASS == 2 && result) {
        result[0] = topk_key_bits(prefix);
        result[1] = gt;
        result[2] = krem - run;
        result[3] = 0;
      }
    }
    run += h[j];
  }
}

// ------------------------------------------------------------------------------------------------ rank and compaction
// block b owns the indices [b * chunk, min(n, (b + 1) * chunk)): output order is index order
__global__ __launch_bounds__(256) void topk_count_kernel(const float* __restrict__ values, int64_t n, int64_t chunk,
                                                         const TopkState* __restrict__ state,
                                                         uint32_t* __restrict__ blockcnt) {
  __shared__ uint32_t red[4][2];
  const uint32_t T = state->prefix;
  const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
  uint32_t g = 0, t = 0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
    const uint32_t key = topk_key(values[i]);
    g += key > T;
    t += key == T;
  }
  g = wave_sum_u32(g), t = wave_sum_u32(t);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][0] = g, red[threadIdx.x >> 6][1] = t;
  __syncthreads();
  if (threadIdx.x < 2)
    blockcnt[2 * blockIdx.x + threadIdx.x] =
        red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t* sh) {   // 1024 threads; sh free on entry
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int o = 1; o < TOPK_BLOCKS; o <<= 1) {
    const uint32_t x = t >= o ? sh[t - o] : 0u;
    __syncthreads();
    sh[t] += x;
    __syncthreads();
  }
  const uint32_t r = sh[t] - v;
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(TOPK_BLOCKS) void topk_scan_kernel(const uint32_t* __restrict__ blockcnt, int nb,
                                                                const TopkState* __restrict__ state,
                                                                uint32_t* __restrict__ blockoff) {
  __shared__ uint32_t sh[TOPK_BLOCKS];
  const int b = threadIdx.x;
  const uint32_t ties = state->krem;
  const uint32_t g = b < nb ? blockcnt[2 * b] : 0u, t = b < nb ? blockcnt[2 * b + 1] : 0u;
  const uint32_t tbefore = block_scan_excl(t, sh);
  const uint32_t take = min(t, ties > tbefore ? ties - tbefore : 0u);   // the lowest indices among the ties
  const uint32_t first = block_scan_excl(g + take, sh);
  if (b < nb) blockoff[2 * b] = first, blockoff[2 * b + 1] = tbefore;
}

__global__ __launch_bounds__(256) void topk_write_kernel(const float* __restrict__ values, int64_t n, int64_t chunk,
                                                         const TopkState* __restrict__ state,
                                                         const uint32_t* __restrict__ blockoff,
                                                         int32_t* __restrict__ rank_out, float* __restrict__ values_out,
                                                         uint32_t K, double* __restrict__ blocksum) {
  __shared__ uint32_t wt[4], wsel[4];
  __shared__ double wsum[4];
  const uint32_t T = state->prefix, ties = state->krem;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
  uint32_t outbase = blockoff[2 * blockIdx.x], tiebase = blockoff[2 * blockIdx.x + 1];
  double acc = 0.0;
  for (int64_t base = lo; base < hi; base += 256) {   // (uniform over the block)
    const int64_t i = base + threadIdx.x;
    const bool in = i < hi;
    const float v = in ? values[i] : 0.f;
    const uint32_t key = topk_key(v);
    const bool isg = in && key > T, ist = in && key == T;
    const unsigned long long bt = __ballot(ist);
    if (lane == 0) wt[wave] = (uint32_t)__popcll(bt);
    __syncthreads();
    uint32_t tw = 0, ttot = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      tw += w < wave ? wt[w] : 0u;
      ttot += wt[w];
    }
    const uint32_t tidx = tiebase + tw + (uint32_t)__popcll(bt & below);
    const bool sel = isg || (ist && tidx < ties);
    const unsigned long long bs = __ballot(sel);
    if (lane == 0) wsel[wave] = (uint32_t)__popcll(bs);
    __syncthreads();
    uint32_t sw = 0, stot = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      sw += w < wave ? wsel[w] : 0u;
      stot += wsel[w];
    }
    if (in) {
      const uint32_t r = outbase + sw + (uint32_t)__popcll(bs & below);
      if (rank_out) rank_out[i] = sel ? (int32_t)r : -1;
      if (sel) {
        if (values_out && r < K) values_out[r] = v;   // (r < K always: the counts come from the same keys)
        acc += (double)v;
      }
    }
    tiebase += ttot, outbase += stot;
    __syncthreads();   // wt / wsel are rewritten by the next trip
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) wsum[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) blocksum[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

__global__ __launch_bounds__(256) void topk_mean_kernel(const double* __restrict__ blocksum, int nb, int64_t K,
                                                        float* __restrict__ mean_out) {
  __shared__ double wsum[4];
  double acc = 0.0;
  for (int b = threadIdx.x; b < nb; b += 256) acc += blocksum[b];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) *mean_out = (float)((((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]) / (double)K);
}

// ------------------------------------------------------------------------------------------------ per-voxel CE
// The loads and the softmax arithmetic are those of loss_fwd_kernel (loss.hip): VEC = 4 consecutive voxels of a row a
// thread where the row width and the addresses allow, the fast exp2 / log2 intrinsics.
template <typename T>
__device__ __forceinline__ void ld_vox(const T* p, float* f, std::integral_constant<int, 1>) {
  f[0] = ST<T>::ld(p);
}
template <typename T>
__device__ __forceinline__ void ld_vox(const T* p, float* f, std::integral_constant<int, 4>) {
  ST<T>::ld4(p, f);
}
template <typename T>
__device__ __forceinline__ void st_vox(T* p, const float* f, std::integral_constant<int, 1>) {
  ST<T>::st(p, f[0]);
}
template <typename T>
__device__ __forceinline__ void st_vox(T* p, const float* f, std::integral_constant<int, 4>) {
  ST<T>::st4(p, f[0], f[1], f[2], f[3]);
}
template <int VEC>
__device__ __forceinline__ void ld_tgt(const float* p, int stride, float* t) {
  if (VEC == 4 && stride == 1) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
    t[0] = v[0], t[1] = v[1], t[2] = v[2], t[3] = v[3];
  } else {
#pragma unroll
    for (int j = 0; j < VEC; j++) t[j] = p[(int64_t)j * stride];
  }
}

// logits [N][C][D][H][W] (D == 1: 2-D), target [N][C][D << s][H << s][W << s] (depth 1 stays 1); nearest down-sampling
// by 2^s reads index dst << s
struct TopkGeom {
  int C, D, H, W, stride, nblk, vec, ignore;
};
__device__ __forceinline__ int64_t target_index(const TopkGeom& g, int64_t v) {
  if (g.stride == 1) return v;
  const int64_t x = v % g.W, y = (v / g.W) % g.H, z = v / ((int64_t)g.W * g.H);
  return ((z * g.stride * ((int64_t)g.H * g.stride) + y * g.stride) * ((int64_t)g.W * g.stride)) + x * g.stride;
}

// The logits of VEC voxels of every class and, per voxel, the target's class (the arg-max of the one-hot row, the first
// maximum).  One running address a tensor: eight per-class bases held at once cost more scalar registers than there are;
// the target row is reduced as it arrives, so it is never held whole.
template <typename T, int VEC, int MC>
__device__ __forceinline__ void load_classes(const T* lp, int64_t V, const float* tp, int64_t Vf, int stride, int C,
                                             float (&lg)[MC][VEC], int (&tc)[VEC]) {
  const std::integral_constant<int, VEC> vt{};
  float tbest[VEC];
#pragma unroll
  for (int j = 0; j < VEC; j++) tbest[j] = -INFINITY, tc[j] = 0;
#pragma unroll
  for (int c = 0; c < MC; c++)
    if (c < C) {
      float t[VEC];
      ld_vox(lp, lg[c], vt);
      ld_tgt<VEC>(tp, stride, t);
#pragma unroll
      for (int j = 0; j < VEC; j++)
        if (t[j] > tbest[j]) tbest[j] = t[j], tc[j] = c;
      lp += V, tp += Vf;
    }
}

// The per-voxel losses of a batch share a handful of exponents, so the top 11 key bits of a wave's 64 voxels fall into a
// few bins and its LDS adds serialise on them: the first histogram is kept in CE_COPIES interleaved copies (a lane adds to
// copy lane % CE_COPIES: neighbouring banks) that are summed at the flush.
constexpr int CE_COPIES = 4;
static_assert(CE_COPIES == 4, "the flush reads the copies of a bin as one 16-byte vector");
template <typename T, int VEC, int MC>
__device__ __forceinline__ void topk_ce_body(const T* __restrict__ logits, const float* __restrict__ target,
                                             const TopkGeom& g, const float* __restrict__ cw, float* __restrict__ res,
                                             uint32_t* lh) {
  const int n = blockIdx.y, C = g.C;
  const int64_t V = (int64_t)g.D * g.H * g.W;
  const int64_t Vf = (g.D == 1 ? 1 : (int64_t)g.D * g.stride) * ((int64_t)g.H * g.stride) * ((int64_t)g.W * g.stride);
  const std::integral_constant<int, VEC> vt{};
  for (int64_t v = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC; v < V; v += (int64_t)g.nblk * 256 * VEC) {
    const int64_t vf = target_index(g, v);
    float lg[MC][VEC], out[VEC];
    int tcv[VEC];
    load_classes<T, VEC, MC>(logits + (int64_t)n * C * V + v, V, target + (int64_t)n * C * Vf + vf, Vf, g.stride, C, lg, tcv);
#pragma unroll
    for (int j = 0; j < VEC; j++) {
      const int tc = tcv[j];
      float mx = -INFINITY;
#pragma unroll
      for (int c = 0; c < MC; c++)
        if (c < C) mx = fmaxf(mx, lg[c][j]);
      float se = 0.f, lt = 0.f;
#pragma unroll
      for (int c = 0; c < MC; c++)
        if (c < C) {
          se += __expf(lg[c][j] - mx);
          if (c == tc) lt = lg[c][j];
        }
      // log(sum exp(x - max)) - (x_t - max): both terms are >= 0, so the value orders like its bit pattern
      const float nll = __logf(se) - (lt - mx);
      out[j] = tc == g.ignore ? 0.f : cw ? cw[tc] * nll : nll;
      const uint32_t key = topk_key(out[j]);
      atomicAdd(&lh[(key >> Radix<0>::SHIFT) * CE_COPIES + (threadIdx.x & (CE_COPIES - 1))], 1u);
    }
    st_vox(res + (int64_t)n * V + v, out, vt);
  }
}

template <typename T, int VEC, int MC>
__global__ __launch_bounds__(256) void topk_ce_kernel(const T* __restrict__ logits, const float* __restrict__ target,
                                                      TopkGeom g, const float* __restrict__ cw, float* __restrict__ res,
                                                      uint32_t* __restrict__ hist_all) {
  __shared__ __attribute__((aligned(16))) uint32_t lh[Radix<0>::BINS * CE_COPIES];
  for (int b = threadIdx.x; b < Radix<0>::BINS * CE_COPIES; b += 256) lh[b] = 0;
  __syncthreads();
  topk_ce_body<T, VEC, MC>(logits, target, g, cw, res, lh);
  __syncthreads();
  for (int b = threadIdx.x; b < Radix<0>::BINS; b += 256) {
    const u32x4 c = *reinterpret_cast<const u32x4*>(&lh[b * CE_COPIES]);
    const uint32_t sum = (c[0] + c[1]) + (c[2] + c[3]);
    if (sum) atomicAdd(&hist_all[HIST0 + b], sum);
  }
}

// ------------------------------------------------------------------------------------------------ backward
template <typename T, int VEC, int MC>
__device__ __forceinline__ void topk_bwd_body(const T* __restrict__ logits, const float* __restrict__ target,
                                              const TopkGeom& g, const float* __restrict__ cw,
                                              const int32_t* __restrict__ rank, const float* __restrict__ grad_values,
                                              float gmean, T* __restrict__ dlogits) {
  const int n = blockIdx.y, C = g.C;
  const int64_t V = (int64_t)g.D * g.H * g.W;
  const int64_t Vf = (g.D == 1 ? 1 : (int64_t)g.D * g.stride) * ((int64_t)g.H * g.stride) * ((int64_t)g.W * g.stride);
  const std::integral_constant<int, VEC> vt{};
  for (int64_t v = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC; v < V; v += (int64_t)g.nblk * 256 * VEC) {
    int32_t r[VEC];
    bool any = false;
#pragma unroll
    for (int j = 0; j < VEC; j++) {
      r[j] = rank[(int64_t)n * V + v + j];
      any = any || r[j] >= 0;
    }
    float lg[MC][VEC];
    if (!any) {   // nine voxels in ten at k = 10: zeros without a read of the logits
#pragma unroll
      for (int j = 0; j < VEC; j++) lg[0][j] = 0.f;
      T* zp = dlogits + (int64_t)n * C * V + v;
#pragma unroll
      for (int c = 0; c < MC; c++)
        if (c < C) {
          st_vox(zp, lg[0], vt);
          zp += V;
        }
      continue;
    }
    const int64_t vf = target_index(g, v);
    int tcv[VEC];
    load_classes<T, VEC, MC>(logits + (int64_t)n * C * V + v, V, target + (int64_t)n * C * Vf + vf, Vf, g.stride, C, lg, tcv);
#pragma unroll
    for (int j = 0; j < VEC; j++) {
      const int tc = tcv[j];
      float mx = -INFINITY;
#pragma unroll
      for (int c = 0; c < MC; c++)
        if (c < C) mx = fmaxf(mx, lg[c][j]);
      float se = 0.f, p[MC];
#pragma unroll
      for (int c = 0; c < MC; c++)
        if (c < C) {
          p[c] = __expf(lg[c][j] - mx);
          se += p[c];
        }
      const float inv = 1.f / se;
      const bool live = r[j] >= 0 && tc != g.ignore;
      const float k = live ? (grad_values ? grad_values[r[j]] : gmean) * (cw ? cw[tc] : 1.f) : 0.f;
#pragma unroll
      for (int c = 0; c < MC; c++)
        if (c < C) lg[c][j] = live ? k * (p[c] * inv - (c == tc ? 1.f : 0.f)) : 0.f;
    }
    T* dp = dlogits + (int64_t)n * C * V + v;
#pragma unroll
    for (int c = 0; c < MC; c++)
      if (c < C) {
        st_vox(dp, lg[c], vt);
        dp += V;
      }
  }
}

template <typename T, int VEC, int MC>
__global__ __launch_bounds__(256) void topk_bwd_kernel(const T* __restrict__ logits, const float* __restrict__ target,
                                                       TopkGeom g, const float* __restrict__ cw,
                                                       const int32_t* __restrict__ rank,
                                                       const float* __restrict__ grad_values,
                                                       const float* __restrict__ grad_mean, int64_t K,
                                                       T* __restrict__ dlogits) {
  // g / K with K exact (a float holds K only up to 2^24), rounded to fp32 once
  const float gmean = grad_mean ? (float)((double)*grad_mean / (double)K) : 0.f;
  topk_bwd_body<T, VEC, MC>(logits, target, g, cw, rank, grad_values, gmean, dlogits);
}

// ------------------------------------------------------------------------------------------------ launchers
int check_select_args(int64_t n, int64_t K, const void* ws, int64_t ws_bytes, int64_t need) {
  HDF_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 31), "topk: n=%lld outside [1, 2^31)", (long long)n);
  HDF_CHECK_ARG(K >= 1 && K <= n, "topk: K=%lld outside [1, n=%lld]", (long long)K, (long long)n);
  HDF_CHECK_ARG(ws != nullptr && ws_bytes >= need, "topk: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
                (long long)need);
  HDF_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "topk: workspace not aligned to 16 bytes");
  return HDF_OK;
}

int zero_select_state(const TopkWs& w, hipStream_t st) {
  if (hipMemsetAsync(w.hist, 0, OFF_STATE + 64, st) != hipSuccess) {
    hdf_set_error("topk: memset failed: %s", hipGetErrorString(hipGetLastError()));
    return HDF_ERR_HIP;
  }
  return HDF_OK;
}

// the select proper on `values` (device, n floats); first_hist_done: HIST0 was filled by the caller's own pass
int run_select(const float* values, int64_t n, int64_t K, const TopkWs& w, bool first_hist_done,
               unsigned long long* result, int32_t* rank_out, float* values_out, float* mean_out, hipStream_t st) {
  const int gh = (int)std::min<int64_t>(ceil_div64(n, 4 * HIST_THREADS), HIST_GRID);
  if (!first_hist_done)
    hipLaunchKernelGGL(topk_hist_kernel<0>, dim3(gh), dim3(HIST_THREADS), 0, st, values, n, w.state, w.hist);
  hipLaunchKernelGGL(topk_pick_kernel<0>, dim3(1), dim3(256), 0, st, w.hist, K, w.state, result);
  hipLaunchKernelGGL(topk_hist_kernel<1>, dim3(gh), dim3(HIST_THREADS), 0, st, values, n, w.state, w.hist);
  hipLaunchKernelGGL(topk_pick_kernel<1>, dim3(1), dim3(256), 0, st, w.hist, K, w.state, result);
  hipLaunchKernelGGL(topk_hist_kernel<2>, dim3(gh), dim3(HIST_THREADS), 0, st, values, n, w.state, w.hist);
  hipLaunchKernelGGL(topk_pick_kernel<2>, dim3(1), dim3(256), 0, st, w.hist, K, w.state, result);
  HDF_LAUNCH_CHECK();
  if (!rank_out && !values_out && !mean_out) return HDF_OK;
  // contiguous index ranges, a multiple of 256 long, at most TOPK_BLOCKS of them
  const int64_t chunk = ceil_div64(ceil_div64(n, TOPK_BLOCKS), 256) * 256;
  const int nb = (int)ceil_div64(n, chunk);
  hipLaunchKernelGGL(topk_count_kernel, dim3(nb), dim3(256), 0, st, values, n, chunk, w.state, w.blockcnt);
  hipLaunchKernelGGL(topk_scan_kernel, dim3(1), dim3(TOPK_BLOCKS), 0, st, w.blockcnt, nb, w.state, w.blockoff);
  hipLaunchKernelGGL(topk_write_kernel, dim3(nb), dim3(256), 0, st, values, n, chunk, w.state, w.blockoff, rank_out,
                     values_out, (uint32_t)K, w.blocksum);
  if (mean_out) hipLaunchKernelGGL(topk_mean_kernel, dim3(1), dim3(256), 0, st, w.blocksum, nb, K, mean_out);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int64_t res_bytes(int64_t n) { return ceil_div64(n * 4, 256) * 256; }

int loss_geometry(const void* logits, const void* other, const float* target, int batch, int n_cls, int D, int H, int W,
                  int scale_shift, int ignore_index, int max_blocks, TopkGeom& g, int64_t& n) {
  HDF_CHECK_ARG(batch >= 1 && D >= 1 && H >= 1 && W >= 1, "topk: batch=%d D=%d H=%d W=%d", batch, D, H, W);
  HDF_CHECK_ARG(batch <= 65535, "topk: batch=%d, at most 65535 supported (one grid row a sample)", batch);
  n = (int64_t)batch * D * H * W;
  HDF_CHECK_ARG(n < ((int64_t)1 << 31), "topk: n=%lld voxels, fewer than 2^31 supported", (long long)n);
  HDF_CHECK_ARG(n_cls >= 2 && n_cls <= MAXC, "topk: n_cls=%d unsupported (2..%d)", n_cls, MAXC);
  HDF_CHECK_ARG(scale_shift >= 0 && scale_shift <= 3, "topk: scale_shift=%d outside 0..3", scale_shift);
  HDF_CHECK_ARG(ignore_index == -100 || (ignore_index >= 0 && ignore_index < n_cls),
                "topk: ignore_index %d is neither -100 nor in [0, %d)", ignore_index, n_cls);
  HDF_CHECK_ARG(logits && target, "topk: logits or target missing");
  const int64_t V = (int64_t)D * H * W;
  const uintptr_t al = reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(other) |
                       reinterpret_cast<uintptr_t>(target);
  g.C = n_cls, g.D = D, g.H = H, g.W = W, g.stride = 1 << scale_shift, g.ignore = ignore_index;
  g.vec = (W % 4 == 0 && (al & 15) == 0) ? 4 : 1;
  g.nblk = (int)std::min<int64_t>(std::max<int64_t>(ceil_div64(V, 256 * g.vec), 1), std::max(max_blocks / batch, 1));
  return HDF_OK;
}
}  // namespace

// ================================================================================================ C ABI
extern "C" {

int64_t hdf_loss_topk_workspace_bytes(int batch, int D, int H, int W) {
  if (batch < 1 || D < 1 || H < 1 || W < 1) return -1;
  const int64_t n = (int64_t)batch * D * H * W;
  if (n >= ((int64_t)1 << 31)) return -1;
  return HDF_TOPK_SELECT_WS + 2 * res_bytes(n);
}

int hdf_op_topk_select(const float* values, int64_t n, int64_t K, void* workspace, int64_t workspace_bytes,
                       uint64_t* result, int32_t* rank_out, float* values_out, float* mean_out, hdf_stream stream) {
  HDF_TRY(check_select_args(n, K, workspace, workspace_bytes, HDF_TOPK_SELECT_WS));
  HDF_CHECK_ARG(values != nullptr, "topk: values missing");
  const TopkWs w = topk_ws(workspace);
  HDF_TRY(zero_select_state(w, (hipStream_t)stream));
  return run_select(values, n, K, w, false, reinterpret_cast<unsigned long long*>(result), rank_out, values_out,
                    mean_out, (hipStream_t)stream);
}

int hdf_loss_topk_forward(int dtype, const void* logits, const float* target_onehot, int batch, int n_cls, int D, int H,
                          int W, int scale_shift, const float* class_weight, int ignore_index, int64_t K,
                          void* workspace, int64_t workspace_bytes, float* values_out, float* mean_out,
                          hdf_stream stream) {
  TopkGeom g;
  int64_t n = 0;
  // the forward pass zeroes and flushes 32 KiB of LDS a block: about four blocks a compute unit in all
  HDF_TRY(loss_geometry(logits, nullptr, target_onehot, batch, n_cls, D, H, W, scale_shift, ignore_index, TOPK_BLOCKS, g, n));
  HDF_TRY(check_select_args(n, K, workspace, workspace_bytes, HDF_TOPK_SELECT_WS + 2 * res_bytes(n)));
  HDF_CHECK_ARG((values_out != nullptr) != (mean_out != nullptr),
                "topk: exactly one of values_out and mean_out must be given");
  HDF_CHECK_ARG(dtype == HDF_F32 || dtype == HDF_BF16 || dtype == HDF_F16, "topk: unsupported dtype %d", dtype);
  hipStream_t st = (hipStream_t)stream;
  const TopkWs w = topk_ws(workspace);
  float* res = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + HDF_TOPK_SELECT_WS);
  int32_t* rank = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(res) + res_bytes(n));
  HDF_TRY(zero_select_state(w, st));
#define TOPK_CE(VEC, MC)                                                                        \
  hipLaunchKernelGGL((topk_ce_kernel<T, VEC, MC>), dim3(g.nblk, batch), dim3(256), 0, st,        \
                     reinterpret_cast<const T*>(logits), target_onehot, g, class_weight, res, w.hist)
  HDF_DISPATCH_T(dtype, {
    if (g.vec == 4 && n_cls <= 4)
      TOPK_CE(4, 4);
    else if (g.vec == 4)
      TOPK_CE(4, MAXC);
    else if (n_cls <= 4)
      TOPK_CE(1, 4);
    else
      TOPK_CE(1, MAXC);
  });
#undef TOPK_CE
  HDF_LAUNCH_CHECK();
  return run_select(res, n, K, w, true, nullptr, rank, values_out, mean_out, st);
}

int hdf_loss_topk_backward(int dtype, const void* logits, const float* target_onehot, int batch, int n_cls, int D, int H,
                           int W, int scale_shift, const float* class_weight, int ignore_index, int64_t K,
                           const void* workspace, int64_t workspace_bytes, const float* grad_values,
                           const float* grad_mean, void* dlogits, hdf_stream stream) {
  TopkGeom g;
  int64_t n = 0;
  HDF_TRY(loss_geometry(logits, dlogits, target_onehot, batch, n_cls, D, H, W, scale_shift, ignore_index,
                        2 * TOPK_BLOCKS, g, n));
  HDF_TRY(check_select_args(n, K, workspace, workspace_bytes, HDF_TOPK_SELECT_WS + 2 * res_bytes(n)));
  HDF_CHECK_ARG((grad_values != nullptr) != (grad_mean != nullptr),
                "topk: exactly one of grad_values and grad_mean must be given");
  HDF_CHECK_ARG(dlogits != nullptr, "topk: dlogits missing");
  HDF_CHECK_ARG(dtype == HDF_F32 || dtype == HDF_BF16 || dtype == HDF_F16, "topk: unsupported dtype %d", dtype);
  hipStream_t st = (hipStream_t)stream;
  const int32_t* rank = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(workspace) + HDF_TOPK_SELECT_WS +
                                                         res_bytes(n));
#define TOPK_BWD(VEC, MC)                                                                                          \
  hipLaunchKernelGGL((topk_bwd_kernel<T, VEC, MC>), dim3(g.nblk, batch), dim3(256), 0, st,                          \
                     reinterpret_cast<const T*>(logits), target_onehot, g, class_weight, rank, grad_values, grad_mean, \
                     K, reinterpret_cast<T*>(dlogits))
  HDF_DISPATCH_T(dtype, {
    if (g.vec == 4 && n_cls <= 4)
      TOPK_BWD(4, 4);
    else if (g.vec == 4)
      TOPK_BWD(4, MAXC);
    else if (n_cls <= 4)
      TOPK_BWD(1, 4);
    else
      TOPK_BWD(1, MAXC);
  });
#undef TOPK_BWD
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
}
