// Order statistics of a fp32 image [C][D][H][W] under an int32 id map [D][H][W]: the median and the percentiles of every
// id, what a user does today with scipy.ndimage.median or np.percentile per id, channel and level after a copy of the id
// map and of every channel and a full sort of every component (the reference has no such code).  Definitions: include/hdf.h.
//
//   measure_table_kernel     (measure.hip, with no channel: its key loops do not run) leaves n and the box of every id
//   quantile_select_kernel   one workgroup per (id, channel): an exact radix select for all levels at once.  A level asks
//                            for the ranks lo and hi, so there are T = 2 Q targets, kept sorted by rank.  The key of a
//                            voxel is order_of(bits), 32 bits, fixed in four rounds of 8 bits from the top.  In a round
//                            the workgroup walks the id's box in the box's own linear order and counts, for every voxel
//                            that holds the id and whose key starts with the prefix of a target, the next digit: 256
//                            32-bit counters in LDS per distinct prefix (targets with the same prefix share them; in
//                            round 1 all do).  Then one wave per target scans the 256 counters: the digit whose
//                            cumulative count first exceeds the target's rank is the target's next digit, and the rank
//                            that remains is the rank among the voxels with that longer prefix.  After round 4 a
//                            target's key is complete: value_of gives s_lo and s_hi, one thread per level the interpolant.
//
// Counting.  In round 1 nearly every voxel of a lesion has the same sign and exponent, so 64 lanes would add to two or
// three counters.  A wave therefore counts the digit of its first live lane once for all lanes that hold it (a ballot),
// three times over, and only what is left goes to the counters lane by lane: a constant image costs one LDS atomic a wave
// in every round, spread digits a few wasted ballots.
//
// Everything is an integer: counts, ranks, keys.  So every output is the same in every bit from call to call, for every
// capacity and whatever the workspace held.  A NaN or an infinity is a key like any other (the values of that component
// mean nothing then); the only address formed from a value of the image is a counter index of 8 bits.  The work is four
// walks over the summed box volumes, times C -- not over the volume -- and a component whose box is the whole volume is
// one workgroup's work.  No thread waits for another workgroup, every loop is bounded by the box.
#include "quantiles.h"

#include "cc_runs.h"

namespace {
constexpr int MAXQ = HDF_QUANTILES_MAX_LEVELS, MAXT = 2 * MAXQ;
constexpr int WAVE_PASSES = 3;   // digits a wave counts once for all its lanes before the rest goes lane by lane

struct Levels {
  double q[MAXQ];
};

// h = fl(q (n - 1)), one rounding, split into floor(h) and frac = h - floor(h), which is exact (no fused multiply-add:
// it would subtract from the unrounded product)
__device__ __forceinline__ double split_rank(double q, uint32_t n, double* frac) {
#pragma clang fp contract(off)
  const double h = q * (double)(n - 1);
  const double fl = floor(h);
  *frac = h - fl;
  return fl;
}

// the third number of a row: fl(s_lo + fl(frac * fl(s_hi - s_lo))), three roundings (no fused multiply-add)
__device__ __forceinline__ double interpolate(double s_lo, double s_hi, double frac) {
#pragma clang fp contract(off)
  const double d = s_hi - s_lo;
  const double p = frac * d;
  return s_lo + p;
}

// geom: [capacity][4] with n first, box: [capacity][CC_BOX_COLS] (the walk's).  count: [capacity], values: [C][capacity][Q][3].
// Dynamic LDS: 2 Q x 256 counters.
__global__ __launch_bounds__(256) void quantile_select_kernel(const int32_t* __restrict__ ids, const float* __restrict__ image,
                                                              int H, int W, int64_t V, int64_t capacity,
                                                              const long long* __restrict__ geom, const int* __restrict__ box,
                                                              Levels lv, int Q, long long* __restrict__ count,
                                                              double* __restrict__ values) {
  extern __shared__ uint32_t hist[];   // [groups][256]
  __shared__ double s_q[MAXQ], s_frac[MAXQ];
  __shared__ uint32_t raw[MAXT];                                          // the ranks in the order of the levels: lo, hi
  __shared__ uint32_t t_rank[MAXT], t_key[MAXT], t_grp[MAXT], t_of[MAXT];   // targets sorted by rank; t_of: level order -> sorted
  __shared__ uint32_t g_prefix[MAXT];                                     // the distinct prefixes, ascending
  __shared__ int s_groups;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = blockIdx.x;
  const int c = blockIdx.y, T = 2 * Q;
  const uint32_t n = (uint32_t)geom[row * 4];   // at most 2^30
  if (c == 0 && tid == 0) count[row] = (long long)n;
  double* out = values + ((int64_t)c * capacity + row) * Q * 3;
  if (n == 0) {   // (one answer for the workgroup)
    if (tid < 3 * Q) out[tid] = 0.0;
    return;
  }
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < MAXQ; i++)
      if (i < Q) s_q[i] = lv.q[i];
  }
  __syncthreads();
  if (tid < Q) {
    double frac;
    const uint32_t lo = (uint32_t)split_rank(s_q[tid], n, &frac);
    raw[2 * tid] = lo, raw[2 * tid + 1] = lo + (frac > 0.0 ? 1u : 0u);   // h <= n - 1, so hi <= n - 1
    s_frac[tid] = frac;
  }
  __syncthreads();
  if (tid < T) {   // sort the ranks by counting: equal ranks keep the order of the levels
    const uint32_t r = raw[tid];
    uint32_t p = 0;
    for (int u = 0; u < T; u++) p += (raw[u] < r || (raw[u] == r && u < tid)) ? 1u : 0u;
    t_of[tid] = p, t_rank[p] = r, t_key[p] = 0u, t_grp[p] = 0u;
  }
  if (tid == 0) s_groups = 1, g_prefix[0] = 0u;

  const int* b = box + row * CC_BOX_COLS;
  const int z0 = CC_BOX_BIG - b[0], y0 = CC_BOX_BIG - b[2], x0 = CC_BOX_BIG - b[4];
  const uint32_t dy = (uint32_t)(b[3] - y0 + 1), dx = (uint32_t)(b[5] - x0 + 1), dydx = dy * dx;
  const uint32_t B = (uint32_t)(b[1] - z0 + 1) * dydx;   // at most 2^30
  const int id = (int)row + 1;
  const float* img = image + (int64_t)c * V;

  for (int shift = 24; shift >= 0; shift -= 8) {   // (uniform)
    __syncthreads();
    const int G = s_groups;
    for (int i = tid; i < G * 256; i += 256) hist[i] = 0u;
    __syncthreads();
    for (uint32_t base = 0; base < B; base += 256) {   // (uniform: the ballots below need every lane)
      const uint32_t i = base + tid;
      int slot = -1;   // the counter of this lane's voxel, if it counts
      if (i < B) {
        const uint32_t bz = i / dydx, r = i - bz * dydx, by = r / dx, bx = r - by * dx;
        const int64_t v = ((int64_t)(z0 + (int)bz) * H + (y0 + (int)by)) * W + (x0 + (int)bx);
        if (ids[v] == id) {
          const uint32_t key = order_of(__float_as_uint(img[v]));
          const int digit = (int)((key >> shift) & 255u);
          if (shift == 24) {
            slot = digit;
          } else {
            const uint32_t prefix = key >> (shift + 8);
            int lo = 0, hi = G;   // the first group whose prefix is not below this one
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (g_prefix[mid] < prefix) lo = mid + 1;
              else hi = mid;
            }
            if (lo < G && g_prefix[lo] == prefix) slot = lo * 256 + digit;
          }
        }
      }
      unsigned long long live = __ballot(slot >= 0);
      for (int pass = 0; pass < WAVE_PASSES && live != 0ull; pass++) {   // (one answer for the wave)
        const int leader = __ffsll((long long)live) - 1;
        const int ls = __shfl(slot, leader, 64);
        const unsigned long long same = __ballot(slot == ls);
        if (lane == leader) atomicAdd(&hist[ls], (uint32_t)__popcll(same));
        if (slot == ls) slot = -1;
        live &= ~same;
      }
      if (slot >= 0) atomicAdd(&hist[slot], 1u);
    }
    __syncthreads();
    for (int t = wave; t < T; t += 4) {   // one wave per target: lane l holds the counters 4 l .. 4 l + 3
      const uint32_t rank = t_rank[t];
      const uint4 cnt = *reinterpret_cast<const uint4*>(&hist[t_grp[t] * 256 + 4 * lane]);
      const uint32_t s = cnt.x + cnt.y + cnt.z + cnt.w, incl = wave_scan_incl_u32(s, lane);
      const unsigned long long hit = __ballot(rank < incl);
      const int at = hit ? __ffsll((long long)hit) - 1 : 63;   // (the group holds more voxels than the rank: there is a hit)
      if (lane == at) {
        uint32_t r = rank - (incl - s), d = 0;
        if (r >= cnt.x) {
          r -= cnt.x, d = 1;
          if (r >= cnt.y) {
            r -= cnt.y, d = 2;
            if (r >= cnt.z) r -= cnt.z, d = 3;
          }
        }
        t_key[t] = (t_key[t] << 8) | (uint32_t)(4 * at) | d, t_rank[t] = r;
      }
    }
    __syncthreads();
    if (shift > 0 && wave == 0) {   // the distinct prefixes of the sorted targets are the next round's groups
      const bool fresh = lane < T && (lane == 0 || t_key[lane] != t_key[lane - 1]);
      const unsigned long long m = __ballot(fresh);
      if (lane < T) {
        const int g = __popcll(m & ((2ull << lane) - 1ull)) - 1;
        t_grp[lane] = (uint32_t)g;
        if (fresh) g_prefix[g] = t_key[lane];
      }
      if (lane == 0) s_groups = __popcll(m);
      // The other waves read these after the barrier at the loop's top.  Built without this fence, the writes above had
      // no wait between them and that barrier (the back edge reached s_barrier with LDS writes in flight), and a wave now
      // and then counted with the groups of the round before.
      __threadfence_block();
    }
  }
  __syncthreads();
  if (tid < Q) {
    const double s_lo = (double)value_of(t_key[t_of[2 * tid]]), s_hi = (double)value_of(t_key[t_of[2 * tid + 1]]);
    out[3 * tid] = s_lo, out[3 * tid + 1] = s_hi, out[3 * tid + 2] = interpolate(s_lo, s_hi, s_frac[tid]);
  }
}

// geom and the box side by side: one memset clears both
struct Carve {
  int64_t geom, box, total;
  explicit Carve(int64_t capacity) {
    Carver c;
    geom = c.take(capacity * 4 * 8);
    box = c.take(capacity * CC_BOX_COLS * 4);
    total = c.at;
  }
};
}  // namespace

int64_t hdf_cc_quantiles_ws_bytes(int64_t capacity) { return Carve(capacity).total; }

int hdf_launch_cc_quantiles(const int32_t* ids, const float* image, int C, int D, int H, int W, int64_t capacity, const double* q,
                            int Q, long long* count, double* values, unsigned long long* result, void* ws, hipStream_t stream) {
  const Carve cv(capacity);
  const int64_t V = (int64_t)D * H * W;
  char* w = (char*)ws;
  long long* geom = (long long*)(w + cv.geom);
  int* box = (int*)(w + cv.box);
  Levels lv;
  for (int i = 0; i < MAXQ; i++) lv.q[i] = i < Q ? q[i] : 0.0;
  // what the walk's atomics add to or raise starts from zero
  HDF_TRY(hdf_zero_async("components", result, 32, stream));
  HDF_TRY(hdf_zero_async("components", w, (size_t)cv.total, stream));
  HDF_TRY(hdf_launch_cc_measure_walk(ids, nullptr, 0, H, W, V, capacity, geom, box, nullptr, result, stream));
  hipLaunchKernelGGL(quantile_select_kernel, dim3((unsigned)capacity, (unsigned)C), dim3(256), (size_t)(2 * Q) * 256 * 4, stream,
                     ids, image, H, W, V, capacity, (const long long*)geom, (const int*)box, lv, Q, count, values);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
