// Average surface distance of one class of a label map against the ground truth: what the reference's cal_asd / multi_asd
// do with MONAI's SurfaceDistanceMetric on the host (utils.py:165-191 -- per class two binary erosions and two fp64
// distance transforms over the whole volume), on the device.  Definitions: include/hdf.h.
//
//   edge_flags_kernel   one pass over the two uint8 maps: a flag byte per voxel (in T, in P, in E6(T), in E6(P)), two counts
//   (surface.hip)       hdf_launch_edt_sq seeded from bit 64 and from bit 128: the squared distance to either edge set
//   asd_gather_kernel   d2_ET at E6(P) and d2_EP at E6(T) into two histograms over the squared distance
//   asd_partial_kernel  sum_k hist[k] sqrt(k) in fp64 over 4096 bins a workgroup, per direction
//   asd_final_kernel    one workgroup: the partial sums of both directions, result[4]
//
// Everything up to the histograms is an exact integer.  The two sums are fp64 without a floating-point atomic: which bins
// a thread adds, and in which order the threads' sums meet, depends on the bin count alone, so two runs agree in every bit.
#include "surface.h"

#include <algorithm>

namespace {
// ------------------------------------------------------------------------------------------------ edge flags
// E6(M): voxels of M with a face neighbour that is not in M; a neighbour outside the volume is not in M (this is where E6
// and the C6 of mask_flags_kernel differ).  A voxel outside both masks costs two byte loads.
__global__ __launch_bounds__(256) void edge_flags_kernel(const uint8_t* __restrict__ tgt, const uint8_t* __restrict__ pred,
                                                         int label, int D, int H, int W, uint8_t* __restrict__ flags,
                                                         unsigned long long* __restrict__ counts) {
  const int64_t V = (int64_t)D * H * W;
  const uint32_t HW = (uint32_t)H * W;
  uint32_t cnt[2] = {0, 0};   // |E6(T)| |E6(P)|: a thread sees fewer than 2^31 voxels
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
    const bool inT = tgt[v] == label, inP = pred[v] == label;
    uint32_t f = (inT ? HDF_SF_IN_T : 0) | (inP ? HDF_SF_IN_P : 0);
    if (f) {
      const uint32_t u = (uint32_t)v;
      const int z = (int)(u / HW), y = (int)((u % HW) / (uint32_t)W), x = (int)(u % (uint32_t)W);
      // the six face neighbours: (in the volume, offset).  A missing neighbour makes the voxel an edge of every mask it is in.
      const bool have[6] = {z > 0, z + 1 < D, y > 0, y + 1 < H, x > 0, x + 1 < W};
      const int64_t off[6] = {-(int64_t)HW, (int64_t)HW, -(int64_t)W, (int64_t)W, -1, 1};
      bool allT = true, allP = true;
#pragma unroll
      for (int k = 0; k < 6; k++) {
        if (!have[k]) {
          allT = allP = false;
          continue;
        }
        if (inT) allT &= tgt[v + off[k]] == label;
        if (inP) allP &= pred[v + off[k]] == label;
      }
      if (inT && !allT) f |= HDF_SF_E6_T;
      if (inP && !allP) f |= HDF_SF_E6_P;
    }
    flags[v] = (uint8_t)f;
    cnt[0] += (f & HDF_SF_E6_T) != 0, cnt[1] += (f & HDF_SF_E6_P) != 0;
  }
  block_add_counts(cnt, counts);
}

// ------------------------------------------------------------------------------------------------ gather
// A = { d2_ET(v) : v in E6(P) } into hist[0][.], B = { d2_EP(v) : v in E6(T) } into hist[1][.], the rows `row` entries
// apart.  Like surface_gather_kernel the low bins are counted in LDS and flushed once per workgroup.  Each direction keeps
// the full window of that kernel: 2 x 2048 x 4 bytes = 16 KiB a workgroup, ten of which fit the 160 KiB of a CU -- more than
// the eight workgroups of 256 threads it can hold, so LDS does not lower the occupancy and the window need not be split.
constexpr int ASD_LDS_BINS = 2048;
__global__ __launch_bounds__(256) void asd_gather_kernel(const uint8_t* __restrict__ flags, const int32_t* __restrict__ d2ET,
                                                         const int32_t* __restrict__ d2EP, int64_t V, uint32_t nbins,
                                                         int64_t row, uint32_t* __restrict__ hist) {
  __shared__ uint32_t lh[2][ASD_LDS_BINS];
  for (int b = threadIdx.x; b < 2 * ASD_LDS_BINS; b += 256) (&lh[0][0])[b] = 0;
  __syncthreads();
  auto add = [&](int dir, uint32_t x) {
    if (x < (uint32_t)ASD_LDS_BINS)
      atomicAdd(&lh[dir][x], 1u);
    else if (x < nbins)            // (the sentinel of a map without seeds is not a distance: nothing is counted)
      atomicAdd(&hist[dir * row + x], 1u);
  };
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
    const uint32_t f = flags[v];
    if (f & HDF_SF_E6_P) add(0, (uint32_t)d2ET[v]);
    if (f & HDF_SF_E6_T) add(1, (uint32_t)d2EP[v]);
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < (uint32_t)ASD_LDS_BINS && b < nbins; b += 256) {
    if (lh[0][b]) atomicAdd(&hist[b], lh[0][b]);
    if (lh[1][b]) atomicAdd(&hist[row + b], lh[1][b]);
  }
}

// ------------------------------------------------------------------------------------------------ the two sums
// (block_sum_f64, wave_ops.h: a fixed tree over the 256 threads of a workgroup)
// Workgroup (blk, dir) adds the bins blk * 4096 .. + 4095 of direction dir: thread t the sixteen bins t, t + 256, ... of
// that span in rising order (a chain of 16), then the tree (depth 8).  Most bins of a fair prediction are empty: they
// cost no square root.
constexpr int ASD_BINS_PER_BLOCK = 4096;
__global__ __launch_bounds__(256) void asd_partial_kernel(const uint32_t* __restrict__ hist, int64_t row, uint32_t nbins,
                                                          uint32_t nblk, double* __restrict__ partial) {
  __shared__ double wsum[4];
  const uint32_t blk = blockIdx.x, dir = blockIdx.y;
  const uint32_t* h = hist + dir * row;
  double s = 0.0;
#pragma unroll 4
  for (int j = 0; j < ASD_BINS_PER_BLOCK / 256; j++) {
    const uint32_t k = blk * ASD_BINS_PER_BLOCK + j * 256 + threadIdx.x;
    const uint32_t c = k < nbins ? h[k] : 0;
    if (c) s += (double)c * sqrt((double)k);
  }
  s = block_sum_f64(s, wsum);
  if (threadIdx.x == 0) partial[dir * nblk + blk] = s;
}

// One workgroup.  result[4] = |E6(T)| |E6(P)| bits(sum A) bits(sum B).  Thread t adds the partial sums t, t + 256, ... of
// a direction (at most 3 * 1023^2 / 4096 / 256 + 1 = 3 of them), then the tree.  A direction has no distances when either
// edge set is empty (nothing to measure from, or nothing to measure to): both sums are +0 then.  surface_mm.hip ends with
// the same kernel (hdf_launch_asd_final) over the partial sums of its voxel runs.
__global__ __launch_bounds__(256) void asd_final_kernel(const unsigned long long* __restrict__ counts,
                                                        const double* __restrict__ partial, uint32_t nblk,
                                                        unsigned long long* __restrict__ result) {
  __shared__ double wsum[2][4];
  const bool any = counts[0] > 0 && counts[1] > 0;
  double s[2];
#pragma unroll
  for (int dir = 0; dir < 2; dir++) {
    double a = 0.0;
    for (uint32_t b = threadIdx.x; b < nblk; b += 256) a += partial[dir * nblk + b];
    s[dir] = block_sum_f64(a, wsum[dir]);
  }
  if (threadIdx.x == 0) {
    result[0] = counts[0], result[1] = counts[1];
    result[2] = (unsigned long long)__double_as_longlong(any ? s[0] : 0.0);
    result[3] = (unsigned long long)__double_as_longlong(any ? s[1] : 0.0);
  }
}

// workspace of hdf_surface_asd, every part on a 256-byte boundary.  Through the scalars it is laid out like that of
// hdf_surface_distances and it holds one histogram more, so it is never the smaller of the two.
struct Carve {
  int64_t flags, d2ET, d2EP, scalars, hist, row, partial, nblk, total;
  Carve(int D, int H, int W) {
    const int64_t V = (int64_t)D * H * W, nbins = hdf_surface_hist_bins(D, H, W);
    Carver c;
    flags = c.take(V);
    d2ET = c.take(V * 4);
    d2EP = c.take(V * 4);
    scalars = c.take(256);            // counts[2] uint64
    row = up256(nbins * 4) / 4;       // entries from histogram A to histogram B
    hist = c.take(2 * row * 4);
    nblk = ceil_div64(nbins, ASD_BINS_PER_BLOCK);
    partial = c.take(2 * nblk * 8);
    total = c.at;
  }
};
}  // namespace

int hdf_launch_asd_final(const unsigned long long* counts, const double* partial, uint32_t nblk, unsigned long long* result,
                         hipStream_t st) {
  hipLaunchKernelGGL(asd_final_kernel, dim3(1), dim3(256), 0, st, counts, partial, nblk, result);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int64_t hdf_surface_asd_ws_bytes(int D, int H, int W) { return Carve(D, H, W).total; }

int hdf_launch_edge_flags(const uint8_t* tgt, const uint8_t* pred, int label, int D, int H, int W, uint8_t* flags,
                          unsigned long long* counts, bool counts_are_zero, hipStream_t st) {
  const int64_t V = (int64_t)D * H * W;
  if (!counts_are_zero) HDF_TRY(hdf_zero_async("surface", counts, 2 * sizeof(unsigned long long), st));
  const unsigned gx = (unsigned)std::min<int64_t>(ceil_div64(V, 256), 8192);
  hipLaunchKernelGGL(edge_flags_kernel, dim3(gx), dim3(256), 0, st, tgt, pred, label, D, H, W, flags, counts);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_surface_asd(const uint8_t* tgt, const uint8_t* pred, int label, int D, int H, int W, void* ws,
                           unsigned long long* result, uint32_t* hist_out, int64_t hist_len, hipStream_t st) {
  const Carve cv(D, H, W);
  const int64_t V = (int64_t)D * H * W, nbins = hdf_surface_hist_bins(D, H, W);
  char* w = (char*)ws;
  uint8_t* flags = (uint8_t*)(w + cv.flags);
  int32_t *d2ET = (int32_t*)(w + cv.d2ET), *d2EP = (int32_t*)(w + cv.d2EP);
  unsigned long long* counts = (unsigned long long*)(w + cv.scalars);
  uint32_t* hist = (uint32_t*)(w + cv.hist);
  double* partial = (double*)(w + cv.partial);
  // the counts and both histograms of an earlier call on this workspace are cleared on the stream, ahead of the kernels
  // (every partial sum is written before it is read)
  HDF_TRY(hdf_zero_async("surface", w + cv.scalars, (size_t)(cv.partial - cv.scalars), st));
  HDF_TRY(hdf_launch_edge_flags(tgt, pred, label, D, H, W, flags, counts, true, st));
  HDF_TRY(hdf_launch_edt_sq(flags, HDF_SF_E6_T, D, H, W, d2ET, st));
  HDF_TRY(hdf_launch_edt_sq(flags, HDF_SF_E6_P, D, H, W, d2EP, st));
  const unsigned gx = (unsigned)std::min<int64_t>(ceil_div64(V, 256), 2048);
  hipLaunchKernelGGL(asd_gather_kernel, dim3(gx), dim3(256), 0, st, flags, d2ET, d2EP, V, (uint32_t)nbins, cv.row, hist);
  HDF_LAUNCH_CHECK();
  hipLaunchKernelGGL(asd_partial_kernel, dim3((unsigned)cv.nblk, 2), dim3(256), 0, st, hist, cv.row, (uint32_t)nbins,
                     (uint32_t)cv.nblk, partial);
  HDF_LAUNCH_CHECK();
  HDF_TRY(hdf_launch_asd_final(counts, partial, (uint32_t)cv.nblk, result, st));
  if (hist_out && hist_len > 0)
    for (int dir = 0; dir < 2; dir++)
      HDF_TRY(hdf_copy_hist_out("surface", hist_out + dir * hist_len, hist_len, hist + dir * cv.row, nbins, st));
  return HDF_OK;
}
