// Connected components of a uint8 label map [D][H][W]: what a user does today with scipy.ndimage.label / find_objects on
// the host after copying the map back (the reference has no such code).  Definitions: include/hdf.h.
//
//   cc_init_kernel      parent[v] = v for a foreground voxel, -1 for background
//   cc_merge_kernel     union of every voxel with the already-visited half of its neighbourhood (3 / 9 / 13 neighbours),
//                       less the unions that another voxel is known to make
//   cc_flatten_kernel   parent[v] = root of v; roots and foreground voxels counted per block of 1024 voxels
//   cc_scan_kernel      one workgroup: exclusive prefix sum over the block counts, result[2]
//   cc_rank_kernel      a root at rank r (1-based, in index order) leaves -(r + 1) in its own slot
//   cc_ids_kernel       ids[v] from the slot of v's root
//   cc_table_*          rows of the component table by integer atomics: runs of a wave, collected per workgroup in LDS
//   cc_size / cc_select / cc_keep / cc_filter_result   the filter
//
// The parent map is a forest in which a parent's index is never above its child's: a root is hooked (compare-and-swap on
// its own slot, so only while it still is a root) under a smaller index of the other tree, and a non-root's slot is only
// ever rewritten with one of its ancestors.  Every walk and every retry therefore moves to a strictly smaller index and
// ends after fewer than D*H*W steps whatever the other workgroups do; no thread waits for another one.  The root of a
// finished tree is the smallest index of its component, which is what makes the numbering scipy's.
#include "components.h"

#include <algorithm>

#include "cc_runs.h"

namespace {
constexpr int CHUNK = 1024;   // voxels per workgroup in the three passes that rank the roots: four consecutive ones a thread

// The slots are read and written by several workgroups inside one kernel: relaxed atomics at device scope, so that no
// access is a data race and none is served from a stale line for longer than the hardware needs.  A stale value would
// still be an ancestor (every value a slot ever held is one), only a longer way round.
__device__ __forceinline__ int ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above x as far as this thread can see, every slot passed on the way moved one ancestor up (p only decreases)
__device__ __forceinline__ int find_root(int32_t* L, int x) {
  int p = ld(L + x);
  if (p != x) {
    int prev = x, next;
    while (p > (next = ld(L + p))) {
      st(L + prev, next);
      prev = p, p = next;
    }
  }
  return p;
}

// a and b: any voxel of the two trees.  Returns a voxel of the joined tree that is no larger than either.  A failed swap
// hands back the slot's present parent, which is below the index tried: max(a, b) falls with every trip.
__device__ __forceinline__ int unite(int32_t* L, int a, int b) {
  while (a != b) {
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = atomicCAS(L + a, a, b);
    if (old == a) return b;
    a = old;
  }
  return a;
}

// ------------------------------------------------------------------------------------------------ label
__global__ __launch_bounds__(256) void cc_init_kernel(const uint8_t* __restrict__ vol, int label, int64_t V,
                                                      int32_t* __restrict__ L) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
    const int val = vol[v];
    L[v] = (label ? val == label : val != 0) ? (int)v : -1;
  }
}

// MAXNZ: how many of (dz, dy, dx) may be non-zero -- 1 / 2 / 3 for 6 / 18 / 26.  Only neighbours BEFORE v in linear order
// are looked at (the later half looks back at v).  A neighbour is tested per coordinate, not by its linear index: x = W - 1
// is not next to x = 0 of the following row, nor the last row of a plane to the first of the next.
template <int MAXNZ>
__global__ __launch_bounds__(256) void cc_merge_kernel(const uint8_t* __restrict__ vol, int label, int D, int H, int W,
                                                       int32_t* __restrict__ L) {
  const int64_t V = (int64_t)D * H * W;
  const uint32_t HW = (uint32_t)H * W;
  for (int64_t v64 = (int64_t)blockIdx.x * 256 + threadIdx.x; v64 < V; v64 += (int64_t)gridDim.x * 256) {
    const int v = (int)v64;
    const int val = vol[v];
    if (label ? val != label : val == 0) continue;
    const uint32_t u = (uint32_t)v;
    const int z = (int)(u / HW), y = (int)((u % HW) / (uint32_t)W), x = (int)(u % (uint32_t)W);
    int r = v;
#ifdef HDF_CC_NO_PRUNE   // A/B builds: every neighbour before v, 3 / 9 / 13 unions a voxel
#pragma unroll
    for (int dz = -1; dz <= 0; dz++) {
#pragma unroll
      for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
          if (dz == 0 && (dy > 0 || (dy == 0 && dx >= 0))) continue;      // not before v
          if ((dz != 0) + (dy != 0) + (dx != 0) > MAXNZ) continue;
          if ((unsigned)(z + dz) >= (unsigned)D || (unsigned)(y + dy) >= (unsigned)H || (unsigned)(x + dx) >= (unsigned)W)
            continue;
          const int n = v + (dz * H + dy) * W + dx;
          if (vol[n] != val) continue;
          r = unite(L, find_root(L, r), find_root(L, n));
        }
      }
    }
#else
    // The voxel before v in its row, then the four rows before v's: (z-1, y-1), (z-1, y), (z-1, y+1), (z, y-1).  A union
    // that others are known to make is left out: inside an object one union a voxel remains, with v - 1.  With `left` =
    // v - 1 holds v's value, a the row's voxel at x - 1, c at x, b at x + 1 (each: in the volume and of v's value):
    //   rows that admit dx = +-1:  c -> v ~ c unless left (v - 1 looks at c as ITS x + 1, and a ~ c ~ b inside their row);
    //                              not c -> v ~ a unless left (a is v - 1's centre), v ~ b
    //   rows that admit dx = 0 only: c -> v ~ c unless left and a (v ~ v - 1 ~ a ~ c)
    // By induction along the run that holds v, every voxel ends connected to each of its neighbours in these rows.
    const bool left = x > 0 && vol[v - 1] == val;
    if (left) r = unite(L, find_root(L, r), find_root(L, v - 1));
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int dz = k < 3 ? -1 : 0, dy = k < 3 ? k - 1 : -1;
      const int nz = (dz != 0) + (dy != 0);
      if (nz > MAXNZ) continue;
      if ((unsigned)(z + dz) >= (unsigned)D || (unsigned)(y + dy) >= (unsigned)H) continue;
      const int m = v + (dz * H + dy) * W;
      const bool c = vol[m] == val;
      const bool a = x > 0 && vol[m - 1] == val;
      if (nz + 1 <= MAXNZ) {
        const bool b = x + 1 < W && vol[m + 1] == val;
        if (c) {
          if (!left) r = unite(L, find_root(L, r), find_root(L, m));
        } else {
          if (a && !left) r = unite(L, find_root(L, r), find_root(L, m - 1));
          if (b) r = unite(L, find_root(L, r), find_root(L, m + 1));
        }
      } else if (c && !(left && a)) {
        r = unite(L, find_root(L, r), find_root(L, m));
      }
    }
#endif
  }
}

// blk[2 b] = roots, blk[2 b + 1] = foreground voxels of the voxels [b CHUNK, (b + 1) CHUNK)
__global__ __launch_bounds__(256) void cc_flatten_kernel(int32_t* __restrict__ L, int64_t V, uint32_t* __restrict__ blk) {
  __shared__ uint32_t red[4][2];
  const int64_t v0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  uint32_t roots = 0, fg = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int64_t v = v0 + k;
    if (v >= V) break;
    const int p = ld(L + v);
    if (p < 0) continue;
    int r = p, q;
    while ((q = ld(L + r)) != r) r = q;   // q < r
    if (r != p) st(L + v, r);
    fg++, roots += r == (int)v;
  }
  roots = wave_sum_u32(roots), fg = wave_sum_u32(fg);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][0] = roots, red[threadIdx.x >> 6][1] = fg;
  __syncthreads();
  if (threadIdx.x < 2)
    blk[2 * (int64_t)blockIdx.x + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// blk[2 b] becomes the number of roots in the blocks before b; result = components, foreground voxels
constexpr int SCAN_THREADS = 1024;
__global__ __launch_bounds__(SCAN_THREADS) void cc_scan_kernel(uint32_t* __restrict__ blk, int64_t nblk,
                                                               unsigned long long* __restrict__ result) {
  __shared__ uint32_t wtot[2][SCAN_THREADS / 64];
  __shared__ unsigned long long wfg[SCAN_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t carry = 0;   // fewer than 2^31 voxels
  unsigned long long fg = 0;
  int par = 0;
  for (int64_t b0 = 0; b0 < nblk; b0 += SCAN_THREADS, par ^= 1) {
    const int64_t b = b0 + threadIdx.x;
    const uint32_t c = b < nblk ? blk[2 * b] : 0;
    fg += b < nblk ? blk[2 * b + 1] : 0;
    const uint32_t inc = wave_scan_incl_u32(c, lane);
    if (lane == 63) wtot[par][wave] = inc;
    __syncthreads();   // (the other parity's slots are rewritten only after the next trip's barrier)
    uint32_t off = carry + (inc - c), total = 0;
#pragma unroll
    for (int w = 0; w < SCAN_THREADS / 64; w++) {
      if (w < wave) off += wtot[par][w];
      total += wtot[par][w];
    }
    if (b < nblk) blk[2 * b] = off;
    carry += total;
  }
  const uint32_t lo = wave_sum_u32((uint32_t)(fg & 0xffffu)), hi = wave_sum_u32((uint32_t)(fg >> 16));   // fg < 2^31 a thread
  if (lane == 0) wfg[wave] = ((unsigned long long)hi << 16) + lo;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
    for (int w = 0; w < SCAN_THREADS / 64; w++) s += wfg[w];
    result[0] = carry, result[1] = s;
  }
}

__global__ __launch_bounds__(256) void cc_rank_kernel(int32_t* __restrict__ L, int64_t V, const uint32_t* __restrict__ blk) {
  __shared__ uint32_t wtot[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t v0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  bool root[4];
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    root[k] = v0 + k < V && L[v0 + k] == (int)(v0 + k);
    c += root[k];
  }
  const uint32_t inc = wave_scan_incl_u32(c, lane);
  if (lane == 63) wtot[wave] = inc;
  __syncthreads();
  uint32_t rank = blk[2 * (int64_t)blockIdx.x] + (inc - c);   // roots before this thread's first voxel
  for (int w = 0; w < wave; w++) rank += wtot[w];
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (root[k]) L[v0 + k] = -(int)(++rank) - 1;   // rank <= 2^31 - 1
}

__global__ __launch_bounds__(256) void cc_ids_kernel(const int32_t* __restrict__ L, int64_t V, int32_t* __restrict__ ids) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
    int p = L[v];
    if (p >= 0) p = L[p];
    ids[v] = -p - 1;   // background -1 -> 0, a root's -(rank + 1) -> rank
  }
}

// ------------------------------------------------------------------------------------------------ table
constexpr long long NONE = 0x7fffffffffffffffll;
__device__ __forceinline__ bool is_min_col(int c) { return c == 2 || c == 3 || c == 5 || c == 7; }

__global__ __launch_bounds__(256) void cc_table_init_kernel(long long* __restrict__ table, int64_t capacity,
                                                            float* __restrict__ smax) {
  const int64_t n = capacity * HDF_CC_TABLE_COLS;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    table[i] = is_min_col((int)(i % HDF_CC_TABLE_COLS)) ? NONE : 0;
    if (smax && i < capacity) smax[i] = 0.f;
  }
}

// (the runs of a wave, the LDS slots of a workgroup and the atomics on a row: cc_runs.h)
__device__ __forceinline__ void table_to_memory(long long* __restrict__ table, int* __restrict__ smax, int id, int len, int val,
                                                int first, int z0, int z1, int y0, int y1, int x0, int x1, int key) {
  long long* row = table + (int64_t)(id - 1) * HDF_CC_TABLE_COLS;
  CC_ADD(row + 0, (long long)len);
  CC_MAX(row + 1, val);
  CC_MIN(row + 2, first);
  CC_MIN(row + 3, z0), CC_MAX(row + 4, z1);
  CC_MIN(row + 5, y0), CC_MAX(row + 6, y1);
  CC_MIN(row + 7, x0), CC_MAX(row + 8, x1);
  if (smax) __hip_atomic_fetch_max(smax + (id - 1), key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void cc_table_kernel(const uint8_t* __restrict__ vol, const int32_t* __restrict__ ids,
                                                       const float* __restrict__ score, int H, int W, int64_t V,
                                                       int64_t capacity, long long* __restrict__ table,
                                                       int* __restrict__ smax) {
  // per slot: id, size, value, first, zmin, zmax, ymin, ymax, xmin, xmax, score key (every one fits an int: V < 2^31)
  __shared__ int sl[11][SLOTS];
  const int BIG = 0x7fffffff;
  if (threadIdx.x < SLOTS) {
    const int t = threadIdx.x;
    sl[0][t] = 0, sl[1][t] = 0, sl[2][t] = 0, sl[3][t] = BIG, sl[4][t] = BIG, sl[5][t] = 0, sl[6][t] = BIG, sl[7][t] = 0;
    sl[8][t] = BIG, sl[9][t] = 0, sl[10][t] = 0;
  }
  __syncthreads();
  const uint32_t HW = (uint32_t)H * W;
  const int64_t begin = (int64_t)blockIdx.x * SPAN;
  for (int trip = 0; trip < SPAN_TRIPS; trip++) {   // (uniform: the wave operations below need every lane)
    const int64_t base = begin + trip * 256;
    if (base >= V) break;
    const int64_t v = base + threadIdx.x;
    const int id = v < V ? ids[v] : 0;
    const uint32_t u = (uint32_t)v;
    const int x = (int)(u % (uint32_t)W);
    bool head;
    const int len = wave_run(id, x == 0, &head);
    // a non-negative float orders like its bit pattern read as an int; a negative one reads as a negative int and loses to
    // the 0 the slot starts from
    int key = 0;
    if (score) {
      key = id > 0 ? __float_as_int(score[v]) : 0;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int other = __shfl_down(key, o, 64);
        if (o < len) key = max(key, other);   // lane + o is still inside this lane's stretch
      }
    }
    if (head && id <= capacity) {
      const int z = (int)(u / HW), y = (int)((u % HW) / (uint32_t)W), val = vol[v];
      if (claim_slot(sl[0], id)) {
        const int t = id & (SLOTS - 1);
        atomicAdd(&sl[1][t], len), atomicMax(&sl[2][t], val), atomicMin(&sl[3][t], (int)v);
        atomicMin(&sl[4][t], z), atomicMax(&sl[5][t], z), atomicMin(&sl[6][t], y), atomicMax(&sl[7][t], y);
        atomicMin(&sl[8][t], x), atomicMax(&sl[9][t], x + len - 1);
        if (score) atomicMax(&sl[10][t], key);
      } else {
        table_to_memory(table, score ? smax : nullptr, id, len, val, (int)v, z, z, y, y, x, x + len - 1, key);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < SLOTS && sl[0][threadIdx.x] != 0) {
    const int t = threadIdx.x;
    table_to_memory(table, score ? smax : nullptr, sl[0][t], sl[1][t], sl[2][t], sl[3][t], sl[4][t], sl[5][t], sl[6][t], sl[7][t],
                    sl[8][t], sl[9][t], sl[10][t]);
  }
}

// a row no voxel reached (id above the number of components) is all zeros
__global__ __launch_bounds__(256) void cc_table_finish_kernel(long long* __restrict__ table, int64_t capacity) {
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < capacity; c += (int64_t)gridDim.x * 256) {
    long long* row = table + c * HDF_CC_TABLE_COLS;
    if (row[0] == 0) row[2] = 0, row[3] = 0, row[5] = 0, row[7] = 0;
  }
}

// ------------------------------------------------------------------------------------------------ filter
struct FilterScalars {          // the first 256 bytes of the workspace, then best[256]
  uint32_t nmax, pad;           // the largest id met
  unsigned long long comps, voxels;
};

// (collected per workgroup like the table's runs)
__global__ __launch_bounds__(256) void cc_size_kernel(const uint8_t* __restrict__ vol, const int32_t* __restrict__ ids,
                                                      int64_t V, uint32_t* __restrict__ sizes, uint8_t* __restrict__ value,
                                                      FilterScalars* __restrict__ sc) {
  __shared__ uint32_t wmax[4];
  __shared__ int sl[3][SLOTS];   // id, size, value
  if (threadIdx.x < SLOTS) sl[0][threadIdx.x] = 0, sl[1][threadIdx.x] = 0, sl[2][threadIdx.x] = 0;
  __syncthreads();
  uint32_t mx = 0;
  const int64_t begin = (int64_t)blockIdx.x * SPAN;
  for (int trip = 0; trip < SPAN_TRIPS; trip++) {
    const int64_t base = begin + trip * 256;
    if (base >= V) break;
    const int64_t v = base + threadIdx.x;
    const int id = v < V ? ids[v] : 0;
    bool head;
    const int len = wave_run(id, false, &head);
    if (head && id <= V) {   // (ids of hdf_cc_label never exceed the voxel count: an id from elsewhere must not leave the arrays)
      if (claim_slot(sl[0], id)) {
        atomicAdd(&sl[1][id & (SLOTS - 1)], len);
        sl[2][id & (SLOTS - 1)] = vol[v];   // (every writer stores the same value)
      } else {
        atomicAdd(sizes + (id - 1), (uint32_t)len);
        value[id - 1] = vol[v];
      }
      mx = max(mx, (uint32_t)id);
    }
  }
  mx = wave_max_u32(mx);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x < SLOTS && sl[0][threadIdx.x] != 0) {
    atomicAdd(sizes + (sl[0][threadIdx.x] - 1), (uint32_t)sl[1][threadIdx.x]);
    value[sl[0][threadIdx.x] - 1] = (uint8_t)sl[2][threadIdx.x];
  }
  if (threadIdx.x == 0) {
    const uint32_t m = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
    if (m) atomicMax(&sc->nmax, m);
  }
}

// keep_largest: best[value] = max over the components of (size << 32 | ~id) -- the largest, a tie to the smallest id.
// Otherwise the components of at least min_size voxels are counted.
__global__ __launch_bounds__(256) void cc_select_kernel(const uint32_t* __restrict__ sizes, const uint8_t* __restrict__ value,
                                                        long long min_size, int keep_largest,
                                                        unsigned long long* __restrict__ best,
                                                        FilterScalars* __restrict__ sc) {
  __shared__ uint32_t wsum[4];
  const int lane = threadIdx.x & 63;
  const int64_t n = sc->nmax;
  uint32_t cnt = 0;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {   // uniform trip count
    const int64_t c = base + threadIdx.x;
    const bool live = c < n;
    const uint32_t s = live ? sizes[c] : 0;
    if (!keep_largest) {
      cnt += live && (long long)s >= min_size;
      continue;
    }
    const int val = live ? value[c] : -1;
    const unsigned long long key = ((unsigned long long)s << 32) | (uint32_t)~(uint32_t)(c + 1);
    // one atomic per distinct value in the wave: every trip retires its leader's lanes, 64 trips at the most
    unsigned long long todo = __ballot(live);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int lv = __shfl(val, leader, 64);
      const bool mine = live && val == lv;
      const unsigned long long k = wave_max_u64(mine ? key : 0ull);
      if (lane == leader) atomicMax(best + lv, k);
      todo &= ~__ballot(mine);
    }
  }
  if (keep_largest) return;
  // (written out, not block_add_counts: behind the early return the shared form compiles to one instruction more)
  cnt = wave_sum_u32(cnt);
  if (lane == 0) wsum[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long t = (unsigned long long)wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (t) atomicAdd(&sc->comps, t);
  }
}

// out may be vol: a voxel is read and written by one thread only
__global__ __launch_bounds__(256) void cc_keep_kernel(const uint8_t* vol, const int32_t* __restrict__ ids, int64_t V,
                                                      const uint32_t* __restrict__ sizes,
                                                      const unsigned long long* __restrict__ best, long long min_size,
                                                      int keep_largest, uint8_t* out, FilterScalars* __restrict__ sc) {
  uint32_t cnt = 0;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
    const int id = ids[v];
    const uint8_t val = vol[v];
    bool keep = false;
    if (id > 0 && id <= V) {
      keep = (long long)sizes[id - 1] >= min_size;
      if (keep && keep_largest) keep = (uint32_t)best[val] == ~(uint32_t)id;
    }
    out[v] = keep ? val : (uint8_t)0;
    cnt += keep;
  }
  block_add_counts({cnt}, &sc->voxels);
}

// one workgroup of 256: thread t looks at value t
__global__ __launch_bounds__(256) void cc_filter_result_kernel(const unsigned long long* __restrict__ best, long long min_size,
                                                               int keep_largest, const FilterScalars* __restrict__ sc,
                                                               unsigned long long* __restrict__ result) {
  __shared__ uint32_t wsum[4];
  const unsigned long long b = best[threadIdx.x];
  uint32_t cnt = keep_largest && b != 0 && (long long)(b >> 32) >= min_size;
  cnt = wave_sum_u32(cnt);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    result[0] = keep_largest ? (unsigned long long)(wsum[0] + wsum[1] + wsum[2] + wsum[3]) : sc->comps;
    result[1] = sc->voxels;
  }
}

// one workspace for the label and the filter entry, every part on a 256-byte boundary
struct Carve {
  int64_t scalars, best, words, bytes, blk, total, nblk;
  Carve(int D, int H, int W) {
    const int64_t V = (int64_t)D * H * W;
    Carver c;
    nblk = ceil_div64(V, CHUNK);
    scalars = c.take(256);
    best = c.take(2048);         // 256 uint64
    words = c.take(V * 4);       // label: the parent map; filter: the size of every component (there are at most V)
    bytes = c.take(V);           // filter: the value of every component
    blk = c.take(nblk * 8);      // label: two uint32 per block of CHUNK voxels
    total = c.at;
  }
};
}  // namespace

int64_t hdf_cc_ws_bytes(int D, int H, int W) { return Carve(D, H, W).total; }

int hdf_launch_cc_label(const uint8_t* vol, int label, int connectivity, int D, int H, int W, int32_t* ids,
                        unsigned long long* result, void* ws, hipStream_t stream) {
  const Carve cv(D, H, W);
  const int64_t V = (int64_t)D * H * W;
  int32_t* L = (int32_t*)((char*)ws + cv.words);
  uint32_t* blk = (uint32_t*)((char*)ws + cv.blk);
  const unsigned gv = vol_grid(V, 1 << 22), gb = (unsigned)cv.nblk;
  hipLaunchKernelGGL(cc_init_kernel, dim3(gv), dim3(256), 0, stream, vol, label, V, L);
  HDF_LAUNCH_CHECK();
  if (connectivity == 6)
    hipLaunchKernelGGL(cc_merge_kernel<1>, dim3(gv), dim3(256), 0, stream, vol, label, D, H, W, L);
  else if (connectivity == 18)
    hipLaunchKernelGGL(cc_merge_kernel<2>, dim3(gv), dim3(256), 0, stream, vol, label, D, H, W, L);
  else
    hipLaunchKernelGGL(cc_merge_kernel<3>, dim3(gv), dim3(256), 0, stream, vol, label, D, H, W, L);
  HDF_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(gb), dim3(256), 0, stream, L, V, blk);
  HDF_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, blk, cv.nblk, result);
  HDF_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_rank_kernel, dim3(gb), dim3(256), 0, stream, L, V, (const uint32_t*)blk);
  HDF_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_ids_kernel, dim3(gv), dim3(256), 0, stream, (const int32_t*)L, V, ids);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_cc_table(const uint8_t* vol, const int32_t* ids, const float* score, int D, int H, int W, int64_t capacity,
                        long long* table, float* score_max, hipStream_t stream) {
  const int64_t V = (int64_t)D * H * W;
  const unsigned gc = vol_grid(capacity * HDF_CC_TABLE_COLS, 4096);
  hipLaunchKernelGGL(cc_table_init_kernel, dim3(gc), dim3(256), 0, stream, table, capacity, score ? score_max : nullptr);
  HDF_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_table_kernel, dim3((unsigned)ceil_div64(V, SPAN)), dim3(256), 0, stream, vol, ids, score, H, W, V,
                     capacity, table,
                     (int*)score_max);
  HDF_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_table_finish_kernel, dim3(gc), dim3(256), 0, stream, table, capacity);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_cc_filter(const uint8_t* vol, const int32_t* ids, int D, int H, int W, int64_t min_size, int keep_largest,
                         uint8_t* out, unsigned long long* result, void* ws, hipStream_t stream) {
  const Carve cv(D, H, W);
  const int64_t V = (int64_t)D * H * W;
  char* w = (char*)ws;
  FilterScalars* sc = (FilterScalars*)(w + cv.scalars);
  unsigned long long* best = (unsigned long long*)(w + cv.best);
  uint32_t* sizes = (uint32_t*)(w + cv.words);
  uint8_t* value = (uint8_t*)(w + cv.bytes);
  // the scalars, the per-value maxima and the sizes of an earlier call are cleared on the stream, ahead of the kernels
  HDF_TRY(hdf_zero_async("components", w, (size_t)(cv.words + V * 4), stream));
  hipLaunchKernelGGL(cc_size_kernel, dim3((unsigned)ceil_div64(V, SPAN)), dim3(256), 0, stream, vol, ids, V, sizes, value, sc);
  HDF_LAUNCH_CHECK();
  const unsigned gs = vol_grid(V, 4096);   // over the components, whose number only the device knows
  hipLaunchKernelGGL(cc_select_kernel, dim3(gs), dim3(256), 0, stream, (const uint32_t*)sizes, (const uint8_t*)value,
                     (long long)min_size, keep_largest, best, sc);
  HDF_LAUNCH_CHECK();
  // (every workgroup ends with one atomic on the same counter: a few thousand of them, not one per 256 voxels)
  hipLaunchKernelGGL(cc_keep_kernel, dim3(gs), dim3(256), 0, stream, vol, ids, V, (const uint32_t*)sizes,
                     (const unsigned long long*)best, (long long)min_size, keep_largest, out, sc);
  HDF_LAUNCH_CHECK();
  hipLaunchKernelGGL(cc_filter_result_kernel, dim3(1), dim3(256), 0, stream, (const unsigned long long*)best,
                     (long long)min_size, keep_largest, (const FilterScalars*)sc, result);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
