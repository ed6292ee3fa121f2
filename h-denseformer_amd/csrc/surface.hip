// Surface-distance evaluation of one class of a label map against the ground truth: what the reference's cal_score does
// with SimpleITK on the host (metrics.py:156-309 -- overlap measures, two Maurer distance maps, two label contours, a
// percentile over the surface distances), as integer work on the device.  Definitions: include/hdf.h.
//
//   mask_flags_kernel      one pass over the two uint8 maps: a flag byte per voxel, five counts
//   edt_row_kernel         squared distance to the nearest seed along W (one wave per line, ballots)
//   edt_col_kernel         lower envelope g(i) = min_j f(j) + (i-j)^2 along H, then along D, a tile of lines in LDS
//   surface_gather_kernel  histogram of squared distances at the contour voxels, maximum over the set differences
//   surface_select_kernel  one workgroup: the two order statistics of the 95th percentile
//
// Everything is an exact integer; the floats are formed by the caller.
#include "surface.h"

#include <algorithm>

namespace {
constexpr int32_t SENT = HDF_EDT_NO_SEED;

// ------------------------------------------------------------------------------------------------ mask flags
// A voxel outside both masks (most of a volume) costs two byte loads; one inside a mask reads its in-volume neighbours.
// Neighbours outside the volume do not exist: they never make a voxel a border voxel.
__global__ __launch_bounds__(256) void mask_flags_kernel(const uint8_t* __restrict__ tgt, const uint8_t* __restrict__ pred,
                                                         int label, int D, int H, int W, uint8_t* __restrict__ flags,
                                                         unsigned long long* __restrict__ counts) {
  const int64_t V = (int64_t)D * H * W;
  const uint32_t HW = (uint32_t)H * W;
  uint32_t cnt[5] = {0, 0, 0, 0, 0};   // nT nP nI |C6(T)| |C6(P)|: a thread sees fewer than 2^31 voxels
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
    const bool inT = tgt[v] == label, inP = pred[v] == label;
    uint32_t f = (inT ? HDF_SF_IN_T : 0) | (inP ? HDF_SF_IN_P : 0);
    if (f) {
      const uint32_t u = (uint32_t)v;
      const int z = (int)(u / HW), y = (int)((u % HW) / (uint32_t)W), x = (int)(u % (uint32_t)W);
      bool allT26 = true, allP26 = true, allT6 = true, allP6 = true;
      for (int dz = -1; dz <= 1; dz++) {
        if ((unsigned)(z + dz) >= (unsigned)D) continue;
        for (int dy = -1; dy <= 1; dy++) {
          if ((unsigned)(y + dy) >= (unsigned)H) continue;
          for (int dx = -1; dx <= 1; dx++) {
            if ((unsigned)(x + dx) >= (unsigned)W) continue;
            const int64_t n = v + ((int64_t)dz * H + dy) * W + dx;
            const bool nT = tgt[n] == label, nP = pred[n] == label;
            const bool face = (dz != 0) + (dy != 0) + (dx != 0) == 1;
            allT26 &= nT, allP26 &= nP;
            if (face) allT6 &= nT, allP6 &= nP;
          }
        }
      }
      if (inT && !allT26) f |= HDF_SF_B26_T;
      if (inP && !allP26) f |= HDF_SF_B26_P;
      if (inT && !allT6) f |= HDF_SF_C6_T;
      if (inP && !allP6) f |= HDF_SF_C6_P;
    }
    flags[v] = (uint8_t)f;
    cnt[0] += inT, cnt[1] += inP, cnt[2] += (inT && inP);
    cnt[3] += (f & HDF_SF_C6_T) != 0, cnt[4] += (f & HDF_SF_C6_P) != 0;
  }
  block_add_counts(cnt, counts);
}

// ------------------------------------------------------------------------------------------------ exact squared EDT
// First axis (W, contiguous): one wave per line.  Lane l owns the voxels l, l + 64, ... of the line (coalesced); a chunk
// of 64 voxels gives one 64-bit ballot of its seeds, so the nearest seed to the left / right inside the chunk is a
// count of leading / trailing zeros and the nearest one in another chunk is a wave-uniform running index.
constexpr int ROW_CHUNKS = HDF_SURFACE_MAX_DIM / 64;
constexpr int FAR = 1 << 20;   // "no seed on that side": any real index distance is below 2^10
// STRIDE: int32 words from one voxel's result to the next (2: the low word of an fp64 slot, surface_mm.hip)
template <int STRIDE>
__global__ __launch_bounds__(256) void edt_row_kernel(const uint8_t* __restrict__ flags, int seed_mask, int64_t nlines,
                                                      int W, int32_t* __restrict__ d2) {
  const int lane = threadIdx.x & 63, nc = (W + 63) >> 6;
  for (int64_t line = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); line < nlines; line += (int64_t)gridDim.x * 4) {
    const uint8_t* f = flags + line * W;
    unsigned long long m[ROW_CHUNKS];
#pragma unroll
    for (int c = 0; c < ROW_CHUNKS; c++) {
      m[c] = 0;
      if (c < nc) {   // wave-uniform: a line of 144 voxels casts three ballots, not sixteen
        const int i = c * 64 + lane;
        m[c] = __ballot(i < W && (f[i] & seed_mask) != 0);
      }
    }
    int before[ROW_CHUNKS], after[ROW_CHUNKS];   // last seed in the chunks before c, first seed in the chunks after c
    int run = -FAR;
#pragma unroll
    for (int c = 0; c < ROW_CHUNKS; c++)
      if (c < nc) {
        before[c] = run;
        if (m[c]) run = c * 64 + 63 - __clzll((long long)m[c]);
      }
    run = FAR;
#pragma unroll
    for (int c = ROW_CHUNKS - 1; c >= 0; c--)
      if (c < nc) {
        after[c] = run;
        if (m[c]) run = c * 64 + __ffsll((long long)m[c]) - 1;
      }
#pragma unroll
    for (int c = 0; c < ROW_CHUNKS; c++) {
      const int i = c * 64 + lane;
      if (c < nc && i < W) {
        const unsigned long long le = m[c] & ((2ull << lane) - 1ull);   // seeds at or left of this lane
        const unsigned long long ge = m[c] >> lane;                      // seeds at or right of it
        const int left = le ? c * 64 + 63 - __clzll((long long)le) : before[c];
        const int right = ge ? i + __ffsll((long long)ge) - 1 : after[c];
        const int d = min(i - left, right - i);
        d2[(line * W + i) * STRIDE] = d >= FAR / 2 ? SENT : d * d;
      }
    }
  }
}

// Later axes: the volume seen as [outer][L][inner] with the lines along L, `inner` apart in memory.  A workgroup holds a
// tile of TW neighbouring lines (consecutive lanes = consecutive inner index: coalesced) in LDS, (L + 1) x TW x 4 bytes <= 64 KiB,
// and replaces every f(i) by min_j f(j) + (i-j)^2, searching outwards from i until (i-j)^2 reaches the best value so far.
// The tile is written back in place: a line depends on nothing outside itself.  A line that holds no finite value (no
// seed in its whole plane so far: most lines of a volume with a small object) would never prune, L steps for each of its
// L voxels; it is found while loading and left as it is.
template <int TW>
__global__ __launch_bounds__(256) void edt_col_kernel(int32_t* __restrict__ d2, int L, int64_t inner, int64_t ntiles,
                                                      int64_t tiles_per_outer) {
  extern __shared__ int32_t col[];
  int32_t* seeded = col + L * TW;   // one word per line of the tile
  constexpr int ROWS = 256 / TW;
  const int wl = threadIdx.x % TW, i0 = threadIdx.x / TW;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t o = tile / tiles_per_outer, c = (tile % tiles_per_outer) * TW + wl;
    const bool live = c < inner;
    int32_t* base = d2 + o * L * inner + (live ? c : 0);
    if (threadIdx.x < TW) seeded[threadIdx.x] = 0;
    __syncthreads();
    bool any = false;
    for (int i = i0; i < L; i += ROWS) {
      const int32_t f = live ? base[(int64_t)i * inner] : SENT;
      col[i * TW + wl] = f;
      any |= f < SENT;
    }
    if (any) seeded[wl] = 1;   // (every writer stores the same value)
    __syncthreads();
    if (live && seeded[wl])
      for (int i = i0; i < L; i += ROWS) {
        int best = col[i * TW + wl];
        for (int dl = 1; dl < L; dl++) {
          const int q = dl * dl, a = i - dl, b = i + dl;
          if (q >= best || (a < 0 && b >= L)) break;
          if (a >= 0) best = min(best, col[a * TW + wl] + q);   // <= SENT + 1023^2 < 2^31
          if (b < L) best = min(best, col[b * TW + wl] + q);
        }
        base[(int64_t)i * inner] = best;
      }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ gather
// S = { d2_T(v) : v in C6(P) } u { d2_P(v) : v in C6(T) } as a histogram over the squared distance, and the maximum of
// d2_T over P \ T and of d2_P over T \ P.  Most surface voxels of a fair prediction lie within a few voxels of the other
// surface: the first LDS_BINS bins are counted in LDS and flushed once per workgroup, the rest go to memory directly.
constexpr int LDS_BINS = 2048;
__global__ __launch_bounds__(256) void surface_gather_kernel(const uint8_t* __restrict__ flags,
                                                             const int32_t* __restrict__ d2T,
                                                             const int32_t* __restrict__ d2P, int64_t V, uint32_t nbins,
                                                             uint32_t* __restrict__ hist, uint32_t* __restrict__ hd2) {
  __shared__ uint32_t lh[LDS_BINS];
  __shared__ uint32_t wmax[4];
  for (int b = threadIdx.x; b < LDS_BINS; b += 256) lh[b] = 0;
  __syncthreads();
  uint32_t mx = 0;
  auto add = [&](uint32_t x) {
    if (x < (uint32_t)LDS_BINS)
      atomicAdd(&lh[x], 1u);
    else if (x < nbins)            // (the sentinel of a map without seeds is not a distance: such a call is not valid)
      atomicAdd(&hist[x], 1u);
  };
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
    const uint32_t f = flags[v];
    if (!f) continue;
    const bool onlyP = (f & 3) == HDF_SF_IN_P, onlyT = (f & 3) == HDF_SF_IN_T;
    if ((f & HDF_SF_C6_P) || onlyP) {
      const uint32_t x = (uint32_t)d2T[v];
      if (f & HDF_SF_C6_P) add(x);
      if (onlyP && x < nbins) mx = max(mx, x);
    }
    if ((f & HDF_SF_C6_T) || onlyT) {
      const uint32_t x = (uint32_t)d2P[v];
      if (f & HDF_SF_C6_T) add(x);
      if (onlyT && x < nbins) mx = max(mx, x);
    }
  }
  mx = wave_max_u32(mx);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < (uint32_t)LDS_BINS && b < nbins; b += 256)
    if (lh[b]) atomicAdd(&hist[b], lh[b]);
  if (threadIdx.x == 0) {
    const uint32_t m = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
    if (m) atomicMax(hd2, m);
  }
}

// ------------------------------------------------------------------------------------------------ select
// One workgroup.  result[12] = nT nP nI |C6(T)| |C6(P)| hd2 n S[lo] S[hi] lo r valid.  With n = |S|, q = 95 (n - 1),
// lo = q div 100, r = q mod 100, hi = min(lo + (r > 0), n - 1): S[lo] is the bin in which the running count first exceeds
// lo.  The scan takes 4096 bins a trip (four consecutive bins a thread) and stops once both are found.
constexpr int SEL_THREADS = 1024;
__global__ __launch_bounds__(SEL_THREADS) void surface_select_kernel(const unsigned long long* __restrict__ counts,
                                                                     const uint32_t* __restrict__ hd2,
                                                                     const uint32_t* __restrict__ hist, uint32_t nbins,
                                                                     unsigned long long V,
                                                                     unsigned long long* __restrict__ result) {
  __shared__ uint32_t wtot[2][SEL_THREADS / 64];
  const unsigned long long nT = counts[0], nP = counts[1];
  const bool valid = nT > 0 && nP > 0 && nT < V && nP < V;
  const unsigned long long n = valid ? counts[3] + counts[4] : 0;
  const unsigned long long q = n ? 95ull * (n - 1) : 0, lo = q / 100, r = q % 100;
  const unsigned long long hi = n ? min(lo + (r > 0), n - 1) : 0;
  if (threadIdx.x == 0) {
    for (int k = 0; k < 5; k++) result[k] = counts[k];
    result[5] = valid ? *hd2 : 0;
    result[6] = n, result[7] = 0, result[8] = 0, result[9] = lo, result[10] = r, result[11] = valid;
  }
  if (!valid) return;
  __syncthreads();   // the zeros of result[7..8] are written before a thread stores what it found
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long carry = 0;   // count of the bins before this trip
  int par = 0;
  for (uint32_t b0 = 0; b0 < nbins && carry <= hi; b0 += SEL_THREADS * 4, par ^= 1) {
    const uint32_t b = b0 + threadIdx.x * 4;
    uint32_t h[4];
#pragma unroll
    for (int k = 0; k < 4; k++) h[k] = b + k < nbins ? hist[b + k] : 0;
    const uint32_t mine = h[0] + h[1] + h[2] + h[3];
    const uint32_t inc = wave_scan_incl_u32(mine, lane);
    if (lane == 63) wtot[par][wave] = inc;
    __syncthreads();   // (the other parity's slots are rewritten only after the next trip's barrier)
    unsigned long long cum = carry + (inc - mine), total = 0;
#pragma unroll
    for (int w = 0; w < SEL_THREADS / 64; w++) {
      if (w < wave) cum += wtot[par][w];
      total += wtot[par][w];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (cum <= lo && lo < cum + h[k]) result[7] = b + k;
      if (cum <= hi && hi < cum + h[k]) result[8] = b + k;
      cum += h[k];
    }
    carry += total;
  }
}

// workspace of hdf_surface_distances, every part on a 256-byte boundary
struct Carve {
  int64_t flags, d2T, d2P, scalars, hist, total;
  Carve(int D, int H, int W) {
    const int64_t V = (int64_t)D * H * W;
    Carver c;
    flags = c.take(V);
    d2T = c.take(V * 4);
    d2P = c.take(V * 4);
    scalars = c.take(256);   // counts[5] uint64, then hd2 uint32 at byte 64
    hist = c.take(hdf_surface_hist_bins(D, H, W) * 4);
    total = c.at;
  }
};
}  // namespace

int64_t hdf_surface_hist_bins(int D, int H, int W) {
  return (int64_t)(D - 1) * (D - 1) + (int64_t)(H - 1) * (H - 1) + (int64_t)(W - 1) * (W - 1) + 1;
}
int64_t hdf_surface_ws_bytes(int D, int H, int W) { return Carve(D, H, W).total; }

int hdf_launch_mask_flags(const uint8_t* tgt, const uint8_t* pred, int label, int D, int H, int W, uint8_t* flags,
                          unsigned long long* counts, bool counts_are_zero, hipStream_t st) {
  const int64_t V = (int64_t)D * H * W;
  if (!counts_are_zero) HDF_TRY(hdf_zero_async("surface", counts, 5 * sizeof(unsigned long long), st));
  const unsigned gx = (unsigned)std::min<int64_t>(ceil_div64(V, 256), 8192);
  hipLaunchKernelGGL(mask_flags_kernel, dim3(gx), dim3(256), 0, st, tgt, pred, label, D, H, W, flags, counts);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

namespace {
int launch_col(int32_t* d2, int64_t outer, int L, int64_t inner, hipStream_t st) {
  if (L == 1) return HDF_OK;
  int tw = 64;   // the widest tile whose lines and per-line flags fit 64 KiB: 64 up to L = 255, 32 to 511, 16 to 1023, then 8
  while ((L + 1) * tw * (int)sizeof(int32_t) > 64 * 1024) tw >>= 1;
  const int64_t per = ceil_div64(inner, tw), ntiles = outer * per;
  const unsigned gx = (unsigned)std::min<int64_t>(ntiles, 1 << 16);
  const size_t lds = (size_t)(L + 1) * tw * sizeof(int32_t);
  if (tw == 64)
    hipLaunchKernelGGL(edt_col_kernel<64>, dim3(gx), dim3(256), lds, st, d2, L, inner, ntiles, per);
  else if (tw == 32)
    hipLaunchKernelGGL(edt_col_kernel<32>, dim3(gx), dim3(256), lds, st, d2, L, inner, ntiles, per);
  else if (tw == 16)
    hipLaunchKernelGGL(edt_col_kernel<16>, dim3(gx), dim3(256), lds, st, d2, L, inner, ntiles, per);
  else
    hipLaunchKernelGGL(edt_col_kernel<8>, dim3(gx), dim3(256), lds, st, d2, L, inner, ntiles, per);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
}  // namespace

int hdf_launch_edt_row(const uint8_t* flags, int seed_mask, int D, int H, int W, int32_t* d2, bool in_fp64_slots,
                       hipStream_t st) {
  const int64_t nlines = (int64_t)D * H;
  const unsigned gx = (unsigned)std::min<int64_t>(ceil_div64(nlines, 4), 1 << 16);
  if (in_fp64_slots)
    hipLaunchKernelGGL(edt_row_kernel<2>, dim3(gx), dim3(256), 0, st, flags, seed_mask, nlines, W, d2);
  else
    hipLaunchKernelGGL(edt_row_kernel<1>, dim3(gx), dim3(256), 0, st, flags, seed_mask, nlines, W, d2);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_edt_sq(const uint8_t* flags, int seed_mask, int D, int H, int W, int32_t* d2, hipStream_t st) {
  HDF_TRY(hdf_launch_edt_row(flags, seed_mask, D, H, W, d2, false, st));
  HDF_TRY(launch_col(d2, D, H, W, st));                  // along H: D slabs of H lines-of-W
  return launch_col(d2, 1, D, (int64_t)H * W, st);       // along D: the (h, w) plane is contiguous
}

int hdf_launch_surface_distances(const uint8_t* tgt, const uint8_t* pred, int label, int D, int H, int W, void* ws,
                                 unsigned long long* result, uint32_t* hist_out, int64_t hist_len, hipStream_t st) {
  const Carve cv(D, H, W);
  const int64_t V = (int64_t)D * H * W, nbins = hdf_surface_hist_bins(D, H, W);
  char* w = (char*)ws;
  uint8_t* flags = (uint8_t*)(w + cv.flags);
  int32_t *d2T = (int32_t*)(w + cv.d2T), *d2P = (int32_t*)(w + cv.d2P);
  unsigned long long* counts = (unsigned long long*)(w + cv.scalars);
  uint32_t* hd2 = (uint32_t*)(w + cv.scalars + 64);
  uint32_t* hist = (uint32_t*)(w + cv.hist);
  // the scalars and the histogram of an earlier call on this workspace are cleared on the stream, ahead of the kernels
  HDF_TRY(hdf_zero_async("surface", w + cv.scalars, (size_t)(cv.total - cv.scalars), st));
  HDF_TRY(hdf_launch_mask_flags(tgt, pred, label, D, H, W, flags, counts, true, st));
  HDF_TRY(hdf_launch_edt_sq(flags, HDF_SF_B26_T, D, H, W, d2T, st));
  HDF_TRY(hdf_launch_edt_sq(flags, HDF_SF_B26_P, D, H, W, d2P, st));
  const unsigned gx = (unsigned)std::min<int64_t>(ceil_div64(V, 256), 2048);
  hipLaunchKernelGGL(surface_gather_kernel, dim3(gx), dim3(256), 0, st, flags, d2T, d2P, V, (uint32_t)nbins, hist, hd2);
  HDF_LAUNCH_CHECK();
  hipLaunchKernelGGL(surface_select_kernel, dim3(1), dim3(SEL_THREADS), 0, st, counts, hd2, hist, (uint32_t)nbins,
                     (unsigned long long)V, result);
  HDF_LAUNCH_CHECK();
  if (hist_out && hist_len > 0) HDF_TRY(hdf_copy_hist_out("surface", hist_out, hist_len, hist, nbins, st));
  return HDF_OK;
}
