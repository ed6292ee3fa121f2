// Surface distances in physical units: the Hausdorff distance, its 95th percentile and the average surface distance of one
// class with a voxel spacing (sz, sy, sx), where surface.hip / surface_asd.hip count in voxels.  Flags, seed sets and
// contour / edge sets are theirs (hdf_launch_mask_flags, hdf_launch_edge_flags); only the metric changes, and with it the
// number format: squared distances are fp64, so there is no histogram to count them in.  Definitions: include/hdf.h.
//
//   (surface.hip)         edt_row_kernel: c^2, the exact integer squared distance along W, into the low word of each fp64 slot
//   edt_col_mm_kernel     g(i) = min_j fl(f(j) + fl(w (i-j)^2)) along H (loading fl(wx c^2)), then along D, a tile of lines in LDS
//   hd_max_mm_kernel      the maximum of D2_T over P \ T and of D2_P over T \ P, as bit patterns (one integer atomicMax a block)
//   select_*_kernel       exact order statistics S[lo], S[lo + 1] over 64-bit keys: six radix passes (11 11 11 11 10 10 bits,
//                         from the top), a one-workgroup pick between them, one pass for the smallest key above S[lo]
//   asd_sum_mm_kernel     sum sqrt(D2) over either edge set: a block per contiguous run of voxels, a fixed tree inside it
//   (surface_asd.hip)     asd_final_kernel, one workgroup: the partial sums in index order, result[4]
//
// Exactness of the transform.  D2(v) = min over seeds of fl(fl(wz a^2) + fl(fl(wy b^2) + fl(wx c^2))) (include/hdf.h).  fl(x + y)
// and fl(w k) are monotone in each argument, so the minimum over c^2 can be taken first (the row pass), then over b, then
// over a: each pass keeps, per line, the minimum of a monotone function of the pass before.  The outward search stops at
// q = fl(w dl^2) >= best: every candidate further out is fl(f + q') >= q' >= q.  This holds only while a product and the sum
// that uses it are rounded separately, and hipcc contracts them into one fma by default -- also through __dmul_rn / __dadd_rn,
// which are a plain `x * y` and `x + y` in a header compiled without the pragma.  mul_rn / add_rn below carry it themselves.
//
// The select's keys are the bit patterns of non-negative doubles, which order like the values.  Only integer atomics are
// used, so two runs agree in every bit.  The surface entry reads its keys from the flags and the two maps on every pass
// (nothing is compacted: the workspace stays at 17 bytes a voxel); hdf_op_select_u64 runs the same kernels on an array.
#include "surface.h"

#include <algorithm>
#include <cmath>

namespace {
constexpr int32_t SENT = HDF_EDT_NO_SEED;
constexpr unsigned long long INF_BITS = 0x7FF0000000000000ull;

__device__ __forceinline__ unsigned long long bits_of(double x) { return (unsigned long long)__double_as_longlong(x); }
// one IEEE rounding each, never half of an fma (as adam_elem, optim.h)
__device__ __forceinline__ double mul_rn(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ double add_rn(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}

// ------------------------------------------------------------------------------------------------ weighted column pass
// The volume seen as [outer][L][inner], lines along L, as edt_col_kernel (surface.hip) sees it: a workgroup holds TW
// neighbouring lines in LDS, L x TW x 8 + TW x 4 bytes <= 64 KiB, and writes them back in place.
// FROM_ROW (the pass along H): slot v holds the int32 c^2 of the row pass in its low word (HDF_EDT_NO_SEED: no seed in the
// row); it is loaded as fl(wrow c^2), +inf for the sentinel, and every slot is rewritten as an fp64 -- a tile reads and
// writes its own slots only.  Otherwise (the pass along D) a line without a finite value is left alone: it holds +inf already.
template <int TW, bool FROM_ROW>
__global__ __launch_bounds__(256) void edt_col_mm_kernel(double* __restrict__ d2, double w, double wrow, int L, int64_t inner,
                                                         int64_t ntiles, int64_t tiles_per_outer) {
#pragma clang fp contract(off)
  extern __shared__ double colmm[];
  int32_t* seeded = reinterpret_cast<int32_t*>(colmm + (size_t)L * TW);   // one word per line of the tile
  constexpr int ROWS = 256 / TW;
  const double inf = __longlong_as_double((long long)INF_BITS);
  const int wl = threadIdx.x % TW, i0 = threadIdx.x / TW;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t o = tile / tiles_per_outer, c = (tile % tiles_per_outer) * TW + wl;
    const bool live = c < inner;
    double* base = d2 + o * L * inner + (live ? c : 0);
    if (threadIdx.x < TW) seeded[threadIdx.x] = 0;
    __syncthreads();
    bool any = false;
    for (int i = i0; i < L; i += ROWS) {
      double f = inf;
      if (live) {
        f = base[(int64_t)i * inner];
        if (FROM_ROW) {
          const int32_t r = (int32_t)(uint32_t)bits_of(f);   // (the slot's high word is whatever the buffer held)
          f = r >= SENT ? inf : mul_rn(wrow, (double)r);
        }
      }
      colmm[i * TW + wl] = f;
      any |= f < inf;
    }
    if (any) seeded[wl] = 1;   // (every writer stores the same value)
    __syncthreads();
    const bool search = live && seeded[wl];
    if (search || (FROM_ROW && live))
      for (int i = i0; i < L; i += ROWS) {
        double best = colmm[i * TW + wl];
        if (search)
          for (int dl = 1; dl < L; dl++) {
            const double q = mul_rn(w, (double)(dl * dl));
            const int a = i - dl, b = i + dl;
            if (q >= best || (a < 0 && b >= L)) break;
            if (a >= 0) best = fmin(best, add_rn(colmm[a * TW + wl], q));
            if (b < L) best = fmin(best, add_rn(colmm[b * TW + wl], q));
          }
        base[(int64_t)i * inner] = best;
      }
    __syncthreads();
  }
}

template <bool FROM_ROW>
int launch_col_mm(double* d2, int64_t outer, int L, int64_t inner, double w, double wrow, hipStream_t st) {
  if (L == 1 && !FROM_ROW) return HDF_OK;
  int tw = 32;   // the widest tile whose lines and per-line flags fit 64 KiB: 32 up to L = 255, 16 to 511, 8 to 1023, then 4
  while ((size_t)L * tw * sizeof(double) + tw * sizeof(int32_t) > 64 * 1024) tw >>= 1;
  const int64_t per = ceil_div64(inner, tw), ntiles = outer * per;
  const unsigned gx = (unsigned)std::min<int64_t>(ntiles, 1 << 16);
  const size_t lds = (size_t)L * tw * sizeof(double) + tw * sizeof(int32_t);
  if (tw == 32)
    hipLaunchKernelGGL((edt_col_mm_kernel<32, FROM_ROW>), dim3(gx), dim3(256), lds, st, d2, w, wrow, L, inner, ntiles, per);
  else if (tw == 16)
    hipLaunchKernelGGL((edt_col_mm_kernel<16, FROM_ROW>), dim3(gx), dim3(256), lds, st, d2, w, wrow, L, inner, ntiles, per);
  else if (tw == 8)
    hipLaunchKernelGGL((edt_col_mm_kernel<8, FROM_ROW>), dim3(gx), dim3(256), lds, st, d2, w, wrow, L, inner, ntiles, per);
  else
    hipLaunchKernelGGL((edt_col_mm_kernel<4, FROM_ROW>), dim3(gx), dim3(256), lds, st, d2, w, wrow, L, inner, ntiles, per);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

// ------------------------------------------------------------------------------------------------ Hausdorff maximum
// max(max over P \ T of D2_T, max over T \ P of D2_P) as a bit pattern; +inf (a map without seeds: such a call is not
// valid) is not a distance.  *hd2 is 0 on entry.
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned long long)__shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(256) void hd_max_mm_kernel(const uint8_t* __restrict__ flags, const double* __restrict__ d2T,
                                                        const double* __restrict__ d2P, int64_t V,
                                                        unsigned long long* __restrict__ hd2) {
  __shared__ unsigned long long wmax[4];
  unsigned long long mx = 0;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
    const uint32_t f = flags[v] & 3;
    if (f == HDF_SF_IN_P) {
      const unsigned long long x = bits_of(d2T[v]);
      if (x < INF_BITS) mx = max(mx, x);
    } else if (f == HDF_SF_IN_T) {
      const unsigned long long x = bits_of(d2P[v]);
      if (x < INF_BITS) mx = max(mx, x);
    }
  }
  mx = wave_max_u64(mx);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long m = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
    if (m) atomicMax(hd2, m);
  }
}

// ------------------------------------------------------------------------------------------------ select over 64-bit keys
// Where the keys come from: an array, or the surface distances of one class read off the flags and the two maps.
struct ArrayKeys {
  const unsigned long long* keys;
  int64_t n;
  __device__ int64_t size() const { return n; }
  template <typename F>
  __device__ void at(int64_t i, F&& emit) const {
    emit(keys[i]);
  }
};
struct SurfaceKeys {   // S = { D2_T(v) : v in C6(P) } + { D2_P(v) : v in C6(T) }
  const uint8_t* flags;
  const double *d2T, *d2P;
  int64_t V;
  __device__ int64_t size() const { return V; }
  template <typename F>
  __device__ void at(int64_t v, F&& emit) const {
    const uint32_t f = flags[v];
    if (f & HDF_SF_C6_P) emit(bits_of(d2T[v]));
    if (f & HDF_SF_C6_T) emit(bits_of(d2P[v]));
  }
};

constexpr int SEL_PASSES = 6, SEL_BINS = 2048;
constexpr int SEL_SHIFT[SEL_PASSES] = {53, 42, 31, 20, 10, 0};
constexpr int SEL_BITS[SEL_PASSES] = {11, 11, 11, 11, 10, 10};
struct SelState {
  unsigned long long prefix;   // key bits decided so far, in place; after the last pick S[lo]
  unsigned long long rank;     // 0-based rank still to find among the keys that share the prefix
  unsigned long long next;     // the smallest key above S[lo]; all ones where there is none
  uint32_t cnt;                // keys in the chosen bin; after the last pick the keys equal to S[lo]
  uint32_t pad;
};
constexpr int64_t SEL_OFF_STATE = (int64_t)SEL_PASSES * SEL_BINS * 4;
static_assert(SEL_OFF_STATE + 256 == HDF_SELECT_U64_WS && sizeof(SelState) <= 256, "hdf.h: HDF_SELECT_U64_WS");

// the histograms and the state have been zeroed; lo comes from the caller, or from the counts of the surface call
__global__ void select_setup_kernel(SelState* __restrict__ state, unsigned long long lo) {
  state->rank = lo;
  state->next = ~0ull;
}
__device__ __forceinline__ void surface_ranks(const unsigned long long* counts, unsigned long long V, bool& valid,
                                              unsigned long long& n, unsigned long long& lo, unsigned long long& r) {
  const unsigned long long nT = counts[0], nP = counts[1];
  valid = nT > 0 && nP > 0 && nT < V && nP < V;
  n = valid ? counts[3] + counts[4] : 0;
  const unsigned long long q = n ? 95ull * (n - 1) : 0;
  lo = q / 100, r = q % 100;
}
__global__ void surface_setup_mm_kernel(const unsigned long long* __restrict__ counts, unsigned long long V,
                                        SelState* __restrict__ state) {
  bool valid;
  unsigned long long n, lo, r;
  surface_ranks(counts, V, valid, n, lo, r);
  state->rank = lo;
  state->next = ~0ull;
}

// One radix pass: the keys that share the decided prefix, counted by their next `bits` bits.  Grid-stride, LDS histogram,
// one global integer atomic per non-empty bin and workgroup (the shape of topk_hist_kernel, loss_topk.hip).
template <typename Src>
__global__ __launch_bounds__(256) void select_hist_kernel(Src src, int shift, int bits, const SelState* __restrict__ state,
                                                          uint32_t* __restrict__ hist) {
  __shared__ uint32_t lh[SEL_BINS];
  for (int b = threadIdx.x; b < SEL_BINS; b += 256) lh[b] = 0;
  __syncthreads();
  const unsigned long long decided = shift + bits >= 64 ? 0ull : ~0ull << (shift + bits);
  const unsigned long long prefix = state->prefix;
  const uint32_t mask = (1u << bits) - 1u;
  const int64_t n = src.size();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    src.at(i, [&](unsigned long long key) {
      if ((key & decided) == prefix) atomicAdd(&lh[(uint32_t)(key >> shift) & mask], 1u);
    });
  __syncthreads();
  for (int b = threadIdx.x; b < SEL_BINS; b += 256)
    if (lh[b]) atomicAdd(&hist[b], lh[b]);
}

// One workgroup.  Walking the bins from the bottom, the chosen bin is the one in which the running count first exceeds the
// rank; exactly one (thread, bin) pair meets the condition (rank < the histogram's total).
__global__ __launch_bounds__(256) void select_pick_kernel(const uint32_t* __restrict__ hist, int shift,
                                                          SelState* __restrict__ state) {
  constexpr int PER = SEL_BINS / 256;
  __shared__ uint32_t part[256];
  const unsigned long long rank = state->rank;
  uint32_t h[PER], s = 0;
#pragma unroll
  for (int j = 0; j < PER; j++) {
    h[j] = hist[threadIdx.x * PER + j];
    s += h[j];
  }
  part[threadIdx.x] = s;
  __syncthreads();   // (every thread has read the rank before one of them rewrites it)
  unsigned long long run = 0;
  for (int j = 0; j < (int)threadIdx.x; j++) run += part[j];
#pragma unroll
  for (int j = 0; j < PER; j++) {
    if (run <= rank && rank < run + h[j]) {
      state->prefix |= (unsigned long long)(threadIdx.x * PER + j) << shift;
      state->rank = rank - run;
      state->cnt = h[j];
    }
    run += h[j];
  }
}

// the smallest key above S[lo]: S[lo + 1] when S[lo] is the last of its equals
template <typename Src>
__global__ __launch_bounds__(256) void select_next_kernel(Src src, SelState* __restrict__ state) {
  __shared__ unsigned long long wmin[4];
  const unsigned long long x = state->prefix;
  unsigned long long mn = ~0ull;
  const int64_t n = src.size();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    src.at(i, [&](unsigned long long key) {
      if (key > x) mn = min(mn, key);
    });
  mn = wave_min_u64(mn);
  if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = mn;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long m = min(min(wmin[0], wmin[1]), min(wmin[2], wmin[3]));
    if (m != ~0ull) atomicMin(&state->next, m);
  }
}

// sorted[lo + 1] from the final state: S[lo] again while it has equals above rank lo, else the next key
__device__ __forceinline__ unsigned long long select_second(const SelState* state) {
  return state->rank + 1 < state->cnt ? state->prefix : state->next;
}
__global__ void select_out_kernel(const SelState* __restrict__ state, unsigned long long n, unsigned long long lo,
                                  unsigned long long* __restrict__ out2) {
  out2[0] = state->prefix;
  out2[1] = lo + 1 < n ? select_second(state) : state->prefix;
}

// result[12] = nT nP nI |C6(T)| |C6(P)| bits(hd2) n bits(S[lo]) bits(S[hi]) lo r valid, hi = min(lo + (r > 0), n - 1)
__global__ void surface_result_mm_kernel(const unsigned long long* __restrict__ counts, unsigned long long V,
                                         const unsigned long long* __restrict__ hd2, const SelState* __restrict__ state,
                                         unsigned long long* __restrict__ result) {
  bool valid;
  unsigned long long n, lo, r;
  surface_ranks(counts, V, valid, n, lo, r);
  const bool second = valid && r > 0 && lo + 1 < n;
  for (int k = 0; k < 5; k++) result[k] = counts[k];
  result[5] = valid ? *hd2 : 0;
  result[6] = n;
  result[7] = valid ? state->prefix : 0;
  result[8] = valid ? (second ? select_second(state) : state->prefix) : 0;
  result[9] = lo, result[10] = r, result[11] = valid;
}

template <typename Src>
int run_select(const Src& src, int64_t items, void* ws, hipStream_t st) {
  uint32_t* hist = reinterpret_cast<uint32_t*>(ws);
  SelState* state = reinterpret_cast<SelState*>(reinterpret_cast<char*>(ws) + SEL_OFF_STATE);
  const unsigned gx = (unsigned)std::min<int64_t>(ceil_div64(items, 1024), 1024);
  for (int p = 0; p < SEL_PASSES; p++) {
    hipLaunchKernelGGL(select_hist_kernel<Src>, dim3(gx), dim3(256), 0, st, src, SEL_SHIFT[p], SEL_BITS[p], state,
                       hist + p * SEL_BINS);
    hipLaunchKernelGGL(select_pick_kernel, dim3(1), dim3(256), 0, st, hist + p * SEL_BINS, SEL_SHIFT[p], state);
  }
  hipLaunchKernelGGL(select_next_kernel<Src>, dim3(gx), dim3(256), 0, st, src, state);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

// ------------------------------------------------------------------------------------------------ the two ASD sums
// (block_sum_f64, wave_ops.h: a fixed tree over the 256 threads of a workgroup)
// Workgroup b adds the voxels [b chunk, min(V, (b + 1) chunk)): thread t those at t, t + 256, ... of the run in rising
// order, then the tree.  chunk and the number of workgroups follow from V alone (AsdSplit), so does the order of every sum.
// A: sqrt(D2_ET) over E6(P) into partial[b], B: sqrt(D2_EP) over E6(T) into partial[nblk + b].
__global__ __launch_bounds__(256) void asd_sum_mm_kernel(const uint8_t* __restrict__ flags, const double* __restrict__ d2ET,
                                                         const double* __restrict__ d2EP, int64_t V, int64_t chunk,
                                                         double* __restrict__ partial) {
  __shared__ double wsum[2][4];
  const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < V ? lo + chunk : V;
  double a = 0.0, b = 0.0;
  for (int64_t v = lo + threadIdx.x; v < hi; v += 256) {
    const uint32_t f = flags[v];
    if (f & HDF_SF_E6_P) a += sqrt(d2ET[v]);
    if (f & HDF_SF_E6_T) b += sqrt(d2EP[v]);
  }
  a = block_sum_f64(a, wsum[0]);
  b = block_sum_f64(b, wsum[1]);
  if (threadIdx.x == 0) partial[blockIdx.x] = a, partial[gridDim.x + blockIdx.x] = b;
}

// The partial sums end in result[4] through surface_asd.hip's asd_final_kernel (hdf_launch_asd_final): in index order, both
// sums +0 when either edge set is empty (one map is all +inf).

// at most 4096 runs of a multiple of 256 voxels, at least 4096 voxels each
struct AsdSplit {
  int64_t chunk, nblk;
  explicit AsdSplit(int64_t V) {
    const int64_t want = std::min<int64_t>(ceil_div64(V, 4096), 4096);
    chunk = ceil_div64(ceil_div64(V, want), 256) * 256;
    nblk = ceil_div64(V, chunk);
  }
};

// one workspace for the three entries, every part on a 256-byte boundary: the flag bytes, two fp64 maps, the counts and
// the maximum, the select's state, the partial sums of the ASD
struct CarveMm {
  int64_t flags, d2A, d2B, scalars, select, partial, total;
  CarveMm(int D, int H, int W) {
    const int64_t V = (int64_t)D * H * W;
    Carver c;
    flags = c.take(V);
    d2A = c.take(V * 8);
    d2B = c.take(V * 8);
    scalars = c.take(256);   // counts[5] uint64, then the maximum (uint64) at byte 64
    select = c.take(HDF_SELECT_U64_WS);
    partial = c.take(2 * AsdSplit(V).nblk * 8);
    total = c.at;
  }
};
}  // namespace

int hdf_surface_check_spacing(const char* who, const double* spacing, SurfaceSpacing* out) {
  HDF_CHECK_ARG(spacing, "surface: %s: null spacing", who);
  const double lo = 1.0 / 1024, hi = 1024.0;
  for (int k = 0; k < 3; k++)
    HDF_CHECK_ARG(std::isfinite(spacing[k]) && spacing[k] >= lo && spacing[k] <= hi,
                  "surface: %s: spacing (%g, %g, %g): each component must be finite and in [2^-10, 2^10]", who, spacing[0],
                  spacing[1], spacing[2]);
  out->wz = spacing[0] * spacing[0], out->wy = spacing[1] * spacing[1], out->wx = spacing[2] * spacing[2];
  return HDF_OK;
}

int64_t hdf_surface_mm_ws_bytes(int D, int H, int W) { return CarveMm(D, H, W).total; }

int hdf_launch_edt_sq_mm(const uint8_t* flags, int seed_mask, int D, int H, int W, const SurfaceSpacing& sp, double* d2,
                         hipStream_t st) {
  HDF_TRY(hdf_launch_edt_row(flags, seed_mask, D, H, W, reinterpret_cast<int32_t*>(d2), true, st));
  HDF_TRY(launch_col_mm<true>(d2, D, H, W, sp.wy, sp.wx, st));                     // along H: D slabs of H lines-of-W
  return launch_col_mm<false>(d2, 1, D, (int64_t)H * W, sp.wz, 0.0, st);           // along D: the (h, w) plane is contiguous
}

int hdf_launch_select_u64(const unsigned long long* keys, int64_t n, int64_t lo, void* ws, unsigned long long* out2,
                          hipStream_t st) {
  HDF_TRY(hdf_zero_async("surface", ws, HDF_SELECT_U64_WS, st));
  SelState* state = reinterpret_cast<SelState*>(reinterpret_cast<char*>(ws) + SEL_OFF_STATE);
  hipLaunchKernelGGL(select_setup_kernel, dim3(1), dim3(1), 0, st, state, (unsigned long long)lo);
  HDF_TRY(run_select(ArrayKeys{keys, n}, n, ws, st));
  hipLaunchKernelGGL(select_out_kernel, dim3(1), dim3(1), 0, st, state, (unsigned long long)n, (unsigned long long)lo, out2);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_surface_distances_mm(const uint8_t* tgt, const uint8_t* pred, int label, int D, int H, int W,
                                    const SurfaceSpacing& sp, void* ws, unsigned long long* result, hipStream_t st) {
  const CarveMm cv(D, H, W);
  const int64_t V = (int64_t)D * H * W;
  char* w = (char*)ws;
  uint8_t* flags = (uint8_t*)(w + cv.flags);
  double *d2T = (double*)(w + cv.d2A), *d2P = (double*)(w + cv.d2B);
  unsigned long long* counts = (unsigned long long*)(w + cv.scalars);
  unsigned long long* hd2 = (unsigned long long*)(w + cv.scalars + 64);
  SelState* state = reinterpret_cast<SelState*>(w + cv.select + SEL_OFF_STATE);
  // the scalars and the select's state of an earlier call on this workspace are cleared on the stream, ahead of the kernels
  HDF_TRY(hdf_zero_async("surface", w + cv.scalars, (size_t)(cv.partial - cv.scalars), st));
  HDF_TRY(hdf_launch_mask_flags(tgt, pred, label, D, H, W, flags, counts, true, st));
  HDF_TRY(hdf_launch_edt_sq_mm(flags, HDF_SF_B26_T, D, H, W, sp, d2T, st));
  HDF_TRY(hdf_launch_edt_sq_mm(flags, HDF_SF_B26_P, D, H, W, sp, d2P, st));
  const unsigned gx = (unsigned)std::min<int64_t>(ceil_div64(V, 256), 2048);
  hipLaunchKernelGGL(hd_max_mm_kernel, dim3(gx), dim3(256), 0, st, flags, d2T, d2P, V, hd2);
  hipLaunchKernelGGL(surface_setup_mm_kernel, dim3(1), dim3(1), 0, st, counts, (unsigned long long)V, state);
  HDF_LAUNCH_CHECK();
  HDF_TRY(run_select(SurfaceKeys{flags, d2T, d2P, V}, V, w + cv.select, st));
  hipLaunchKernelGGL(surface_result_mm_kernel, dim3(1), dim3(1), 0, st, counts, (unsigned long long)V, hd2, state, result);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_surface_asd_mm(const uint8_t* tgt, const uint8_t* pred, int label, int D, int H, int W,
                              const SurfaceSpacing& sp, void* ws, unsigned long long* result, hipStream_t st) {
  const CarveMm cv(D, H, W);
  const int64_t V = (int64_t)D * H * W;
  const AsdSplit split(V);
  char* w = (char*)ws;
  uint8_t* flags = (uint8_t*)(w + cv.flags);
  double *d2ET = (double*)(w + cv.d2A), *d2EP = (double*)(w + cv.d2B);
  unsigned long long* counts = (unsigned long long*)(w + cv.scalars);
  double* partial = (double*)(w + cv.partial);
  // the counts of an earlier call are cleared on the stream (every partial sum is written before it is read)
  HDF_TRY(hdf_zero_async("surface", w + cv.scalars, 256, st));
  HDF_TRY(hdf_launch_edge_flags(tgt, pred, label, D, H, W, flags, counts, true, st));
  HDF_TRY(hdf_launch_edt_sq_mm(flags, HDF_SF_E6_T, D, H, W, sp, d2ET, st));
  HDF_TRY(hdf_launch_edt_sq_mm(flags, HDF_SF_E6_P, D, H, W, sp, d2EP, st));
  hipLaunchKernelGGL(asd_sum_mm_kernel, dim3((unsigned)split.nblk), dim3(256), 0, st, flags, d2ET, d2EP, V, split.chunk,
                     partial);
  HDF_LAUNCH_CHECK();
  return hdf_launch_asd_final(counts, partial, (uint32_t)split.nblk, result, st);
}
