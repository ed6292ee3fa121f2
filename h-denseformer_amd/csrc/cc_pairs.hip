// The overlap table of two int32 id maps [D][H][W]: one row (a, b, n, m) per distinct pair of ids that share a voxel -- what
// a user does today with np.unique over 64-bit keys on the host after copying both id maps back (the reference has no such
// code).  Definitions: include/hdf.h.
//
//   pairs_init_kernel        the header, the table and the key list of an earlier call cleared
//   pairs_voxel_kernel       the voxel pass: runs of a wave, collected per workgroup in LDS, flushed into the global table
//   pairs_compact_kernel     the occupied slots' keys gathered into a list (in any order), n and m summed
//   pairs_sort_chunk_kernel  bitonic sort of up to SORT_CHUNK keys by one workgroup in LDS
//   pairs_merge_global_kernel / pairs_merge_local_kernel   the bitonic steps across / inside chunks of longer lists
//   pairs_rows_kernel        rows in key order, the tail zeroed, the four result words, the overflow rule
//
// The global table is open addressing with linear probing over SLOTS = a power of two >= 2 * capacity slots: keys (64-bit,
// a << 32 | b; 0 = empty, which no counted pair has), n and m (32-bit: fewer than 2^31 voxels).  An insert claims an empty
// slot by compare-and-swap on the key and adds to n and m; the claim that makes the table hold more than `capacity` keys
// sets the overflow word, and so does a probe that walked all SLOTS slots without finding room.  Once the word is set every
// later insert returns at once: the table stays about half empty, probes stay short, and the outputs of an overflowing call
// are all zeros whatever was inserted.  Sums of integers and a sort of distinct keys: no output depends on arrival order.
// No thread waits for another one: a probe ends after at most SLOTS steps, the sort networks have fixed lengths.
#include "cc_pairs.h"

#include <algorithm>

namespace {
constexpr int TRIP = HDF_PAIRS_TRIP, SPAN = HDF_PAIRS_SPAN, SPAN_TRIPS = SPAN / TRIP, LSLOTS = HDF_PAIRS_LDS_SLOTS;
constexpr int UNROLL = 4;   // trips whose loads are issued together
constexpr int CHUNK = HDF_PAIRS_SORT_CHUNK, SORT_THREADS = 1024;
static_assert(LSLOTS == 256 && TRIP == 256, "one LDS slot a thread at the flush, slot = the hash's top 8 bits");
static_assert(SPAN_TRIPS % UNROLL == 0, "whole groups of trips");
typedef unsigned long long u64;

struct Header {   // the first 256 bytes of the workspace
  uint32_t overflow;   // more than `capacity` distinct pairs, or no room in the table
  uint32_t used;       // slots claimed
  uint32_t listed;     // keys in the list
  uint32_t pad;
  u64 sum_n, sum_m;
};
struct Table {
  Header* hdr;
  u64* keys;       // [slots]
  u64* list;       // [slots]: the occupied slots' keys, ~0 behind them
  uint32_t* n;     // [slots]
  uint32_t* m;     // [slots]
  uint32_t mask;   // slots - 1
  uint32_t capacity;
};

// relaxed atomics at device scope for what several workgroups read and write inside one kernel (as in components.hip)
__device__ __forceinline__ u64 ld64(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t ld32(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t hash_key(u64 k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  return (uint32_t)k;
}
__device__ __forceinline__ uint32_t pow2_ceil(uint32_t n) { return n <= 1 ? 1u : 1u << (32 - __clz((int)(n - 1))); }

__global__ __launch_bounds__(256) void pairs_init_kernel(Table t) {
  const uint32_t slots = t.mask + 1;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < slots; i += gridDim.x * 256)
    t.keys[i] = 0, t.list[i] = ~0ull, t.n[i] = 0, t.m[i] = 0;
  if (blockIdx.x == 0 && threadIdx.x < 4) ((u64*)t.hdr)[threadIdx.x] = 0;
}

// n voxels of the pair `key`, m of them under the mask
__device__ __forceinline__ void pairs_insert(const Table& t, u64 key, uint32_t n, uint32_t m) {
  if (ld32(&t.hdr->overflow)) return;
  uint32_t s = hash_key(key) & t.mask;
  for (uint32_t probe = 0; probe <= t.mask; probe++, s = (s + 1) & t.mask) {
    u64 cur = ld64(t.keys + s);
    if (cur == 0) {
      cur = atomicCAS(t.keys + s, 0ull, key);
      if (cur == 0) {
        if (atomicAdd(&t.hdr->used, 1u) >= t.capacity) atomicCAS(&t.hdr->overflow, 0u, 1u);
        cur = key;
      }
    }
    if (cur == key) {
      atomicAdd(t.n + s, n);
      if (m) atomicAdd(t.m + s, m);
      return;
    }
  }
  atomicCAS(&t.hdr->overflow, 0u, 1u);   // every slot holds another key
}

// The voxel pass.  The lanes of a wave hold 64 consecutive voxels; a wave without a counted voxel -- most of a volume -- does
// nothing beyond its loads.  A run is a maximal stretch of lanes with the same counted pair that does not cross a row start:
// its first lane speaks for all of it, with the run's length and the number of its lanes under the mask (two ballots).  A
// workgroup collects its runs in LSLOTS LDS slots, a slot claimed by the first pair that asks (compare-and-swap on its key);
// a run whose slot belongs to another pair goes to the global table directly.  The slots are flushed once per workgroup.
template <bool MASK>
__global__ __launch_bounds__(256) void pairs_voxel_kernel(const int32_t* __restrict__ ids_a, const int32_t* __restrict__ ids_b,
                                                          const uint8_t* __restrict__ mask, int flags, int W, int64_t V,
                                                          Table t) {
  __shared__ u64 skey[LSLOTS];
  __shared__ uint32_t sn[LSLOTS], sm[LSLOTS];
  __shared__ uint32_t s_over;
  skey[threadIdx.x] = 0, sn[threadIdx.x] = 0, sm[threadIdx.x] = 0;
  if (threadIdx.x == 0) s_over = ld32(&t.hdr->overflow);
  __syncthreads();
  if (s_over) return;   // (one value for the whole workgroup) the outputs are zeros already
  const bool zero_a = flags & HDF_PAIRS_A0, zero_b = flags & HDF_PAIRS_B0;
  const int lane = threadIdx.x & 63;
  const int64_t begin = (int64_t)blockIdx.x * SPAN;
  for (int g = 0; g < SPAN_TRIPS; g += UNROLL) {   // (uniform: the wave operations below need every lane)
    const int64_t base = begin + g * TRIP + threadIdx.x;
    if (begin + g * TRIP >= V) break;
    int va[UNROLL], vb[UNROLL], vm[UNROLL];
#pragma unroll
    for (int k = 0; k < UNROLL; k++) {
      const int64_t v = base + k * TRIP;
      const bool in = v < V;
      va[k] = in ? ids_a[v] : 0, vb[k] = in ? ids_b[v] : 0;
      vm[k] = MASK && in ? mask[v] : 0;
    }
#pragma unroll
    for (int k = 0; k < UNROLL; k++) {
      const int a = max(va[k], 0), b = max(vb[k], 0);
      const bool counted = (a > 0 && b > 0) || (zero_a && a == 0 && b > 0) || (zero_b && a > 0 && b == 0);
      if (__ballot(counted) == 0) continue;
      const uint32_t x = (uint32_t)(base + k * TRIP) % (uint32_t)W;
      const int pa = __shfl_up(a, 1, 64), pb = __shfl_up(b, 1, 64);
      const bool head = counted && (lane == 0 || pa != a || pb != b || x == 0);
      const u64 brk = __ballot(head || !counted), under = __ballot(counted && vm[k] != 0);
      if (head) {
        const int len = wave_run_len(brk, lane);
        const u64 run = (len == 64 ? ~0ull : (1ull << len) - 1) << lane;
        const uint32_t m = (uint32_t)__popcll(under & run);
        const u64 key = ((u64)(uint32_t)a << 32) | (uint32_t)b;
        const uint32_t slot = ((uint32_t)a * 0x9E3779B1u ^ (uint32_t)b * 0x85EBCA77u) >> 24;
        u64 owner = __hip_atomic_load(&skey[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (owner == 0) {
          owner = atomicCAS(&skey[slot], 0ull, key);
          if (owner == 0) owner = key;
        }
        if (owner == key) {
          atomicAdd(&sn[slot], (uint32_t)len);
          if (m) atomicAdd(&sm[slot], m);
        } else {
          pairs_insert(t, key, (uint32_t)len, m);
        }
      }
    }
  }
  __syncthreads();
  if (skey[threadIdx.x] != 0) pairs_insert(t, skey[threadIdx.x], sn[threadIdx.x], sm[threadIdx.x]);
}

__global__ __launch_bounds__(256) void pairs_compact_kernel(Table t) {
  const uint32_t slots = t.mask + 1;
  uint32_t n = 0, m = 0;   // (all of n is below 2^31)
  for (uint32_t s = blockIdx.x * 256 + threadIdx.x; s < slots; s += gridDim.x * 256) {
    const u64 key = t.keys[s];
    if (key == 0) continue;
    t.list[atomicAdd(&t.hdr->listed, 1u)] = key;   // at most `slots` keys
    n += t.n[s], m += t.m[s];
  }
  n = wave_sum_u32(n), m = wave_sum_u32(m);
  if ((threadIdx.x & 63) == 0) {
    if (n) atomicAdd(&t.hdr->sum_n, (u64)n);
    if (m) atomicAdd(&t.hdr->sum_m, (u64)m);
  }
}

// ------------------------------------------------------------------------------------------------ sort
// A bitonic network over the first N = 2^ceil(log2 listed) entries of the list (the ~0 entries behind the keys sort last).
// Step (k, j) compares i and i + j for every i with bit j clear, ascending where bit k of i is clear.  Steps with j < CHUNK
// stay inside an aligned chunk of CHUNK entries and run in LDS; a list of at most CHUNK entries is one launch of one workgroup.
__device__ __forceinline__ void order(u64& lo, u64& hi, bool ascending) {
  if ((lo > hi) == ascending) {
    const u64 x = lo;
    lo = hi, hi = x;
  }
}
// the steps j = j0, j0 / 2 .. 1 of stage k on the n entries in LDS that start at list index `base`
__device__ __forceinline__ void steps_in_lds(u64* s, uint32_t n, uint32_t base, uint32_t k, uint32_t j0) {
  for (uint32_t j = j0; j > 0; j >>= 1) {
    __syncthreads();
    for (uint32_t p = threadIdx.x; p < n / 2; p += SORT_THREADS) {
      const uint32_t i = 2 * p - (p & (j - 1));
      order(s[i], s[i + j], ((base + i) & k) == 0);
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(SORT_THREADS) void pairs_sort_chunk_kernel(Table t) {
  __shared__ u64 s[CHUNK];
  if (t.hdr->overflow) return;
  const uint32_t N = pow2_ceil(t.hdr->listed), base = blockIdx.x * CHUNK;
  if (base >= N) return;
  const uint32_t n = min(N, (uint32_t)CHUNK);
  for (uint32_t i = threadIdx.x; i < n; i += SORT_THREADS) s[i] = t.list[base + i];
  for (uint32_t k = 2; k <= n; k <<= 1) steps_in_lds(s, n, base, k, k / 2);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n; i += SORT_THREADS) t.list[base + i] = s[i];
}

__global__ __launch_bounds__(256) void pairs_merge_global_kernel(Table t, uint32_t k, uint32_t j) {
  if (t.hdr->overflow) return;
  const uint32_t N = pow2_ceil(t.hdr->listed);
  if (k > N) return;
  for (uint32_t p = blockIdx.x * 256 + threadIdx.x; p < N / 2; p += gridDim.x * 256) {
    const uint32_t i = 2 * p - (p & (j - 1));
    const u64 lo = t.list[i], hi = t.list[i + j];
    if ((lo > hi) == ((i & k) == 0)) t.list[i] = hi, t.list[i + j] = lo;
  }
}

__global__ __launch_bounds__(SORT_THREADS) void pairs_merge_local_kernel(Table t, uint32_t k) {
  __shared__ u64 s[CHUNK];
  if (t.hdr->overflow) return;
  const uint32_t N = pow2_ceil(t.hdr->listed), base = blockIdx.x * CHUNK;
  if (k > N || base >= N) return;   // (k > CHUNK here: N is at least two chunks)
  for (uint32_t i = threadIdx.x; i < CHUNK; i += SORT_THREADS) s[i] = t.list[base + i];
  steps_in_lds(s, CHUNK, base, k, CHUNK / 2);
  for (uint32_t i = threadIdx.x; i < CHUNK; i += SORT_THREADS) t.list[base + i] = s[i];
}

// ------------------------------------------------------------------------------------------------ rows
__global__ __launch_bounds__(256) void pairs_rows_kernel(Table t, long long* __restrict__ pairs, u64* __restrict__ result) {
  const bool over = t.hdr->overflow != 0;
  const uint32_t P = over ? 0 : t.hdr->listed;   // (without overflow: at most `capacity`)
  for (uint32_t r = blockIdx.x * 256 + threadIdx.x; r < t.capacity; r += gridDim.x * 256) {
    long long a = 0, b = 0, n = 0, m = 0;
    if (r < P) {
      const u64 key = t.list[r];
      uint32_t s = hash_key(key) & t.mask;
      for (uint32_t probe = 0; probe <= t.mask && t.keys[s] != key; probe++) s = (s + 1) & t.mask;   // (the key is there)
      a = (long long)(key >> 32), b = (long long)(key & 0xffffffffu), n = t.n[s], m = t.m[s];
    }
    long long* row = pairs + (int64_t)r * 4;
    row[0] = a, row[1] = b, row[2] = n, row[3] = m;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    result[0] = P, result[1] = over ? 0 : t.hdr->sum_n, result[2] = over ? 0 : t.hdr->sum_m, result[3] = over ? 1 : 0;
  }
}

Table carve(void* ws, int64_t capacity) {
  const int64_t slots = hdf_cc_pairs_slots(capacity);
  char* w = (char*)ws;
  Table t;
  t.hdr = (Header*)w;
  t.keys = (u64*)(w + 256);
  t.list = t.keys + slots;
  t.n = (uint32_t*)(t.list + slots);
  t.m = t.n + slots;
  t.mask = (uint32_t)(slots - 1);
  t.capacity = (uint32_t)capacity;
  return t;
}
}  // namespace

int64_t hdf_cc_pairs_slots(int64_t capacity) {
  int64_t s = 64;
  while (s < 2 * capacity) s *= 2;
  return s;
}
int64_t hdf_cc_pairs_ws_bytes(int64_t capacity) { return 256 + hdf_cc_pairs_slots(capacity) * 24; }

int hdf_launch_cc_pairs(const int32_t* ids_a, const int32_t* ids_b, const uint8_t* mask, int flags, int D, int H, int W,
                        int64_t capacity, long long* pairs, unsigned long long* result, void* ws, hipStream_t stream) {
  const int64_t V = (int64_t)D * H * W;
  const Table t = carve(ws, capacity);
  const uint32_t slots = t.mask + 1;
  const unsigned gs = std::min(slots / 256u, 512u);   // slots is a multiple of 64: at least one workgroup
  hipLaunchKernelGGL(pairs_init_kernel, dim3(std::max(gs, 1u)), dim3(256), 0, stream, t);
  HDF_LAUNCH_CHECK();
  const unsigned gv = (unsigned)ceil_div64(V, SPAN);
  if (mask)
    hipLaunchKernelGGL(pairs_voxel_kernel<true>, dim3(gv), dim3(256), 0, stream, ids_a, ids_b, mask, flags, W, V, t);
  else
    hipLaunchKernelGGL(pairs_voxel_kernel<false>, dim3(gv), dim3(256), 0, stream, ids_a, ids_b, mask, flags, W, V, t);
  HDF_LAUNCH_CHECK();
  hipLaunchKernelGGL(pairs_compact_kernel, dim3(std::max(gs, 1u)), dim3(256), 0, stream, t);
  HDF_LAUNCH_CHECK();
  hipLaunchKernelGGL(pairs_sort_chunk_kernel, dim3(std::max(slots / CHUNK, 1u)), dim3(SORT_THREADS), 0, stream, t);
  HDF_LAUNCH_CHECK();
  for (uint32_t k = 2 * CHUNK; k <= slots; k <<= 1) {
    for (uint32_t j = k / 2; j >= (uint32_t)CHUNK; j >>= 1) {
      hipLaunchKernelGGL(pairs_merge_global_kernel, dim3(std::min(slots / 512u, 512u)), dim3(256), 0, stream, t, k, j);
      HDF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(pairs_merge_local_kernel, dim3(slots / CHUNK), dim3(SORT_THREADS), 0, stream, t, k);
    HDF_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(pairs_rows_kernel, dim3((unsigned)std::min<int64_t>(ceil_div64(capacity, 256), 256)), dim3(256), 0, stream,
                     t, pairs, (u64*)result);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
