// Measurements of a fp32 image [C][D][H][W] under an int32 id map [D][H][W]: what a user does today with scipy.ndimage's
// sum_labels / mean / variance / minimum / maximum / *_position / center_of_mass on the host, one call per statistic and
// channel, after a copy of the id map and of every channel (the reference has no such code).  Definitions: include/hdf.h.
//
//   measure_table_kernel   one walk over the voxels.  The runs of a wave (cc_runs.h), collected per workgroup in LDS, leave
//                          by integer atomics: n and the coordinate sums in geom, the box, and per channel the two keys
//                          (order(x) << 32 | ~index for the maximum, ~order(x) << 32 | ~index for the minimum: both are
//                          maxima, and the smallest index wins a tie in either).  The image is read where an id counts.
//   measure_slab_kernel    one workgroup per (id, slab, channel): slab s of HDF_MEASURE_SLABS is the range [s per, (s + 1) per)
//                          of the box's own linear order, per = ceil(box voxels / HDF_MEASURE_SLABS).  Thread t takes the
//                          voxels t, t + 256, ... of the slab in that order, adds those of its id in fp64, block_sum_f64
//                          joins the threads.  <false>: S1, Wz, Wy, Wx; <true>: M2 with the finished mean.
//   measure_finish_kernel  one thread per (channel, id): the slabs added in index order, mean, min, max, the positions
//   measure_m2_kernel      the same for M2
//
// The fp64 sums use no atomic: which voxels a thread adds and in which order the partial sums meet follows from the box
// alone, and the box is exact.  So a row is the same in every bit from call to call, whatever the workspace held and
// whatever the capacity (its partial sums live at another place, with the same values).  The work of the two slab passes is
// the summed box volumes, not the volume: a component whose box holds many foreign voxels pays for them.  No thread waits
// for another one, every loop is bounded by the volume.
#include "measure.h"

#include "cc_runs.h"

namespace {
typedef unsigned long long u64;
constexpr int MAXC = HDF_MEASURE_MAX_CHANNELS, NSLAB = HDF_MEASURE_SLABS;
constexpr int BOX_COLS = CC_BOX_COLS, BIG = CC_BOX_BIG;   // (cc_runs.h, with order_of / value_of)
__device__ __forceinline__ u64 shfl_down_u64(u64 v, int o) {
  const uint32_t lo = __shfl_down((uint32_t)v, o, 64), hi = __shfl_down((uint32_t)(v >> 32), o, 64);
  return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ void geom_to_memory(long long* __restrict__ geom, int* __restrict__ box, int id, int n, int sz, int sy,
                                               int sx, int nz0, int z1, int ny0, int y1, int nx0, int x1) {
  long long* g = geom + (int64_t)(id - 1) * 4;
  CC_ADD(g + 0, (long long)n), CC_ADD(g + 1, (long long)sz), CC_ADD(g + 2, (long long)sy), CC_ADD(g + 3, (long long)sx);
  int* b = box + (int64_t)(id - 1) * BOX_COLS;
  atomicMax(b + 0, nz0), atomicMax(b + 1, z1), atomicMax(b + 2, ny0), atomicMax(b + 3, y1), atomicMax(b + 4, nx0);
  atomicMax(b + 5, x1);
}

// keys: [C][capacity][2] = the minimum's key, the maximum's.  result: [0] max id, [1] voxels with id > 0, [2] those counted.
__global__ __launch_bounds__(256) void measure_table_kernel(const int32_t* __restrict__ ids, const float* __restrict__ image,
                                                            int C, int H, int W, int64_t V, int64_t capacity,
                                                            long long* __restrict__ geom, int* __restrict__ box,
                                                            u64* __restrict__ keys, u64* __restrict__ result) {
  // per slot: id, n, sum z, sum y, sum x (a workgroup sees 8192 voxels: each fits an int), the six box maxima; the keys
  __shared__ int sl[11][SLOTS];
  __shared__ u64 sk[2 * MAXC][SLOTS];
  __shared__ uint32_t wmax[4];
  for (int i = threadIdx.x; i < 11 * SLOTS; i += 256) (&sl[0][0])[i] = 0;
  for (int i = threadIdx.x; i < 2 * MAXC * SLOTS; i += 256) (&sk[0][0])[i] = 0ull;
  __syncthreads();
  const uint32_t HW = (uint32_t)H * W;
  const int64_t begin = (int64_t)blockIdx.x * SPAN;
  uint32_t fg = 0, counted = 0, mx = 0;
  for (int trip = 0; trip < SPAN_TRIPS; trip++) {   // (uniform: the wave operations below need every lane)
    const int64_t base = begin + trip * 256;
    if (base >= V) break;
    const int64_t v = base + threadIdx.x;
    const int raw = v < V ? ids[v] : 0;
    const bool in = raw > 0 && raw <= capacity;
    fg += raw > 0, counted += in;
    mx = max(mx, (uint32_t)max(raw, 0));
    const int id = in ? raw : 0;   // an id above the capacity ends a run like background does
    if (__ballot(id > 0) == 0ull) continue;   // (one answer for the wave)
    const uint32_t u = (uint32_t)v;
    const int x = (int)(u % (uint32_t)W);
    bool head;
    const int len = wave_run(id, x == 0, &head);
    const int t = id & (SLOTS - 1);
    bool slot = false;
    if (head) {
      const int z = (int)(u / HW), y = (int)((u % HW) / (uint32_t)W);
      const int sx = len * x + len * (len - 1) / 2;
      slot = claim_slot(sl[0], id);
      if (slot) {
        atomicAdd(&sl[1][t], len), atomicAdd(&sl[2][t], z * len), atomicAdd(&sl[3][t], y * len), atomicAdd(&sl[4][t], sx);
        atomicMax(&sl[5][t], BIG - z), atomicMax(&sl[6][t], z), atomicMax(&sl[7][t], BIG - y), atomicMax(&sl[8][t], y);
        atomicMax(&sl[9][t], BIG - x), atomicMax(&sl[10][t], x + len - 1);
      } else {
        geom_to_memory(geom, box, id, len, z * len, y * len, sx, BIG - z, z, BIG - y, y, BIG - x, x + len - 1);
      }
    }
    for (int c = 0; c < C; c++) {   // (uniform)
      u64 kmin = 0ull, kmax = 0ull;   // below every key: a key's low word is ~index, never 0
      if (id > 0) {
        const uint32_t o = order_of(__float_as_uint(image[(int64_t)c * V + v]));
        kmin = ((u64)(~o) << 32) | (uint32_t)~u, kmax = ((u64)o << 32) | (uint32_t)~u;
      }
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const u64 a = shfl_down_u64(kmin, o), b = shfl_down_u64(kmax, o);
        if (o < len) kmin = max(kmin, a), kmax = max(kmax, b);   // lane + o is still inside this lane's stretch
      }
      if (head) {
        if (slot) {
          atomicMax(&sk[2 * c][t], kmin), atomicMax(&sk[2 * c + 1][t], kmax);
        } else {
          u64* k = keys + ((int64_t)c * capacity + (id - 1)) * 2;
          atomicMax(k, kmin), atomicMax(k + 1, kmax);
        }
      }
    }
  }
  mx = wave_max_u32(mx);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x < SLOTS && sl[0][threadIdx.x] != 0) {
    const int t = threadIdx.x, id = sl[0][t];
    geom_to_memory(geom, box, id, sl[1][t], sl[2][t], sl[3][t], sl[4][t], sl[5][t], sl[6][t], sl[7][t], sl[8][t], sl[9][t],
                   sl[10][t]);
    for (int c = 0; c < C; c++) {
      u64* k = keys + ((int64_t)c * capacity + (id - 1)) * 2;
      atomicMax(k, sk[2 * c][t]), atomicMax(k + 1, sk[2 * c + 1][t]);
    }
  }
  if (threadIdx.x == 0) {
    const uint32_t m = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
    if (m) atomicMax(result, (u64)m);
  }
  block_add_counts({fg, counted}, result + 1);
}

// partial: [C][capacity][NSLAB][4].  <false> leaves S1, Wz, Wy, Wx of the slab there, <true> M2 in the first of the four.
template <bool M2>
__global__ __launch_bounds__(256) void measure_slab_kernel(const int32_t* __restrict__ ids, const float* __restrict__ image,
                                                           int H, int W, int64_t V, int64_t capacity,
                                                           const long long* __restrict__ geom, const int* __restrict__ box,
                                                           const double* __restrict__ stats, double* __restrict__ partial) {
  __shared__ double wsum[4][4];
  const int64_t row = blockIdx.x / NSLAB;
  const int slab = blockIdx.x % NSLAB, c = blockIdx.y;
  if (geom[row * 4] == 0) return;   // (one answer for the workgroup) nobody reads the partial sums of an absent id
  const int* b = box + row * BOX_COLS;
  const int z0 = BIG - b[0], y0 = BIG - b[2], x0 = BIG - b[4];
  const uint32_t dy = (uint32_t)(b[3] - y0 + 1), dx = (uint32_t)(b[5] - x0 + 1), dydx = dy * dx;
  const uint32_t B = (uint32_t)(b[1] - z0 + 1) * dydx;   // at most 2^30
  const uint32_t per = (B + NSLAB - 1) / NSLAB, lo = (uint32_t)slab * per, hi = min(lo + per, B);
  const int id = (int)row + 1;
  const int64_t at = (int64_t)c * capacity + row;
  const float* img = image + (int64_t)c * V;
  const double mean = M2 ? stats[at * 8 + 1] : 0.0;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (uint32_t i = lo + threadIdx.x; i < hi; i += 256) {   // (lo >= hi where the box has fewer voxels than slabs)
    const uint32_t bz = i / dydx, r = i - bz * dydx, by = r / dx, bx = r - by * dx;
    const int z = z0 + (int)bz, y = y0 + (int)by, x = x0 + (int)bx;
    const int64_t v = ((int64_t)z * H + y) * W + x;
    if (ids[v] != id) continue;
    const double xv = (double)img[v];
    if (M2) {
      const double d = xv - mean;
      a0 = fma(d, d, a0);
    } else {
      a0 += xv, a1 = fma((double)z, xv, a1), a2 = fma((double)y, xv, a2), a3 = fma((double)x, xv, a3);   // exact products
    }
  }
  double* out = partial + (at * NSLAB + slab) * 4;
  a0 = block_sum_f64(a0, wsum[0]);
  if (!M2) a1 = block_sum_f64(a1, wsum[1]), a2 = block_sum_f64(a2, wsum[2]), a3 = block_sum_f64(a3, wsum[3]);
  if (threadIdx.x == 0) {
    out[0] = a0;
    if (!M2) out[1] = a1, out[2] = a2, out[3] = a3;
  }
}

__global__ __launch_bounds__(256) void measure_finish_kernel(int64_t rows /* C * capacity */, int64_t capacity,
                                                             const long long* __restrict__ geom, const u64* __restrict__ keys,
                                                             const double* __restrict__ partial, double* __restrict__ stats,
                                                             long long* __restrict__ pos) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  double* s = stats + i * 8;
  const long long n = geom[(i % capacity) * 4];
  if (n == 0) {
#pragma unroll
    for (int k = 0; k < 8; k++) s[k] = 0.0;
    pos[2 * i] = 0, pos[2 * i + 1] = 0;
    return;
  }
  const double* q = partial + i * NSLAB * 4;
  double t[4] = {q[0], q[1], q[2], q[3]};
  for (int slab = 1; slab < NSLAB; slab++) {
#pragma unroll
    for (int k = 0; k < 4; k++) t[k] += q[slab * 4 + k];
  }
  const u64 kmin = keys[2 * i], kmax = keys[2 * i + 1];
  s[0] = t[0], s[1] = t[0] / (double)n, s[2] = 0.0;
  s[3] = (double)value_of(~(uint32_t)(kmin >> 32)), s[4] = (double)value_of((uint32_t)(kmax >> 32));
  s[5] = t[1], s[6] = t[2], s[7] = t[3];
  pos[2 * i] = (long long)(uint32_t)~(uint32_t)kmin, pos[2 * i + 1] = (long long)(uint32_t)~(uint32_t)kmax;
}

__global__ __launch_bounds__(256) void measure_m2_kernel(int64_t rows, int64_t capacity, const long long* __restrict__ geom,
                                                         const double* __restrict__ partial, double* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows || geom[(i % capacity) * 4] == 0) return;
  const double* q = partial + i * NSLAB * 4;
  double t = q[0];
  for (int slab = 1; slab < NSLAB; slab++) t += q[slab * 4];
  stats[i * 8 + 2] = t;
}

// the box and the keys side by side: one memset clears both
struct Carve {
  int64_t box, keys, cleared, partial, total;
  Carve(int C, int64_t capacity) {
    Carver c;
    box = c.take(capacity * BOX_COLS * 4);
    keys = c.take((int64_t)C * capacity * 2 * 8);
    cleared = c.at;
    partial = c.take((int64_t)C * capacity * NSLAB * 4 * 8);
    total = c.at;
  }
};
}  // namespace

int64_t hdf_cc_measure_ws_bytes(int C, int64_t capacity) { return Carve(C, capacity).total; }

// The walk alone, for the units that need n and the box of every id (quantiles.hip): with C = 0 the key loops do not run
// and neither image nor keys is read.  geom, box and result must have been cleared on the stream.
int hdf_launch_cc_measure_walk(const int32_t* ids, const float* image, int C, int H, int W, int64_t V, int64_t capacity,
                               long long* geom, int* box, unsigned long long* keys, unsigned long long* result,
                               hipStream_t stream) {
  hipLaunchKernelGGL(measure_table_kernel, dim3((unsigned)ceil_div64(V, SPAN)), dim3(256), 0, stream, ids, image, C, H, W, V,
                     capacity, geom, box, keys, result);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_cc_measure(const int32_t* ids, const float* image, int C, int D, int H, int W, int64_t capacity, long long* geom,
                          double* stats, long long* pos, unsigned long long* result, void* ws, hipStream_t stream) {
  const Carve cv(C, capacity);
  const int64_t V = (int64_t)D * H * W, rows = (int64_t)C * capacity;
  char* w = (char*)ws;
  int* box = (int*)(w + cv.box);
  u64* keys = (u64*)(w + cv.keys);
  double* partial = (double*)(w + cv.partial);
  // what the atomics add to or raise starts from zero: the result words, the integer rows, the boxes and the keys
  HDF_TRY(hdf_zero_async("components", result, 32, stream));
  HDF_TRY(hdf_zero_async("components", geom, (size_t)capacity * 32, stream));
  HDF_TRY(hdf_zero_async("components", w, (size_t)cv.cleared, stream));
  HDF_TRY(hdf_launch_cc_measure_walk(ids, image, C, H, W, V, capacity, geom, box, keys, result, stream));
  const dim3 gs((unsigned)(capacity * NSLAB), (unsigned)C);   // at most 524 288 x 8
  const unsigned gf = (unsigned)ceil_div64(rows, 256);        // at most 2048
  hipLaunchKernelGGL(measure_slab_kernel<false>, gs, dim3(256), 0, stream, ids, image, H, W, V, capacity, (const long long*)geom,
                     (const int*)box, (const double*)stats, partial);
  HDF_LAUNCH_CHECK();
  hipLaunchKernelGGL(measure_finish_kernel, dim3(gf), dim3(256), 0, stream, rows, capacity, (const long long*)geom,
                     (const u64*)keys, (const double*)partial, stats, pos);
  HDF_LAUNCH_CHECK();
  hipLaunchKernelGGL(measure_slab_kernel<true>, gs, dim3(256), 0, stream, ids, image, H, W, V, capacity, (const long long*)geom,
                     (const int*)box, (const double*)stats, partial);
  HDF_LAUNCH_CHECK();
  hipLaunchKernelGGL(measure_m2_kernel, dim3(gf), dim3(256), 0, stream, rows, capacity, (const long long*)geom,
                     (const double*)partial, stats);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
