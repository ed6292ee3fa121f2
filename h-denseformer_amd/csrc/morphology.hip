// Binary morphology of a uint8 label map [D][H][W]: what a user does today with scipy.ndimage.binary_dilation / _erosion /
// _opening / _closing / _fill_holes on the host after copying the map back (the reference has no such code).  Definitions:
// include/hdf.h.
//
//   morph_pack_kernel     the uint8 map, read once, to 1 bit a voxel: 32-bit words along x, every row starts on a word
//   morph_step_kernel     one dilation or erosion on packed words, from one packed buffer into the other
//   morph_unpack_kernel   the packed result and the original map to `out` (MASK or MAP mode) and the two result words
//   fill_complement / fill_faces / fill_write   fill holes: the complement of the mask is labelled by hdf_launch_cc_label,
//                         the components met on a face of the volume are flagged, the others are the holes
//
// Bit i of word j of a row is voxel x = 32 j + i.  A lane of the pack and unpack kernels holds 16 consecutive voxels of a
// row (one 16-byte access of the byte map when W is a multiple of 16 and the maps are aligned), so two neighbouring lanes
// make one word.  The bits of a row's last word at x >= W hold nothing: the step kernel replaces them by border_value in
// every word it loads, the unpack kernel leaves them out of the counts and writes nothing for them.
#include "morphology.h"

#include <algorithm>

#include "components.h"

namespace {
constexpr int LANE_VOX = 16;   // voxels a lane of the pack / unpack kernels holds: half a word

struct Bytes16 {
  union {
    u32x4 v;
    uint8_t b[16];
  };
};

__device__ __forceinline__ bool in_mask(int val, int label) { return label ? val == label : val != 0; }

// n of the 16 voxels at p exist (the others read as 0, which is in no mask)
__device__ __forceinline__ void load16(const uint8_t* p, int n, bool vec, Bytes16* d) {
  if (vec) {
    d->v = *reinterpret_cast<const u32x4*>(p);
  } else {
#pragma unroll
    for (int k = 0; k < LANE_VOX; k++) d->b[k] = k < n ? p[k] : (uint8_t)0;
  }
}
__device__ __forceinline__ uint32_t mask_bits(const Bytes16& d, int label) {
  uint32_t bits = 0;
#pragma unroll
  for (int k = 0; k < LANE_VOX; k++) bits |= (uint32_t)in_mask(d.b[k], label) << k;
  return bits;
}

// ------------------------------------------------------------------------------------------------ pack
// lanes = rows * 2 * wpr (even): lane t holds the voxels [16 c, 16 c + 16) of row t / (2 wpr), c = t % (2 wpr)
__global__ __launch_bounds__(256) void morph_pack_kernel(const uint8_t* __restrict__ vol, int label, int W, int wpr,
                                                         uint32_t lanes, bool vec, uint32_t* __restrict__ dst) {
  const uint32_t lpr = 2u * (uint32_t)wpr;
  for (uint32_t base = blockIdx.x * 256u; base < lanes; base += gridDim.x * 256u) {   // (uniform: the exchange needs both lanes)
    const uint32_t t = base + threadIdx.x;
    uint32_t bits = 0;
    if (t < lanes) {
      const uint32_t row = t / lpr, c = t % lpr;
      const int n = W - (int)c * LANE_VOX;
      if (n > 0) {
        Bytes16 d;
        load16(vol + (int64_t)row * W + c * LANE_VOX, n, vec, &d);
        bits = mask_bits(d, label);
      }
    }
    const uint32_t other = __shfl_xor(bits, 1, 64);
    if (t < lanes && !(t & 1)) dst[t >> 1] = bits | (other << 16);
  }
}

// ------------------------------------------------------------------------------------------------ step
// word j of the row at p; the bits past W of the row's last word read as the border
__device__ __forceinline__ uint32_t load_word(const uint32_t* __restrict__ p, int j, int wpr, uint32_t tail, uint32_t fill) {
  const uint32_t w = p[j];
  return j == wpr - 1 ? (w & tail) | (fill & ~tail) : w;
}

// C = 1 / 2 / 3 for 6 / 18 / 26.  A row offset (dz, dy) with m = |dz| + |dy| admits dx = +-1 when m <= C - 1, dx = 0 only
// when m == C and nothing when m > C.  fill: 32 copies of border_value, what a row, a plane or a word outside the volume
// reads as.  flat: the depth-1 volume, which has no z neighbours and no z border.  A carry comes from the neighbouring
// word of the SAME row or from the border, never from another row.
template <int C, bool ERODE>
__global__ __launch_bounds__(256) void morph_step_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int D,
                                                         int H, int wpr, uint32_t tail, uint32_t fill, bool flat,
                                                         uint32_t words) {
  for (uint32_t t = blockIdx.x * 256u + threadIdx.x; t < words; t += gridDim.x * 256u) {
    const uint32_t row = t / (uint32_t)wpr;
    const int j = (int)(t % (uint32_t)wpr), z = (int)(row / (uint32_t)H), y = (int)(row % (uint32_t)H);
    uint32_t acc = ERODE ? ~0u : 0u;
#pragma unroll
    for (int dz = -1; dz <= 1; dz++) {
#pragma unroll
      for (int dy = -1; dy <= 1; dy++) {
        const int m = (dz != 0) + (dy != 0);
        if (m > C) continue;
        if (flat && dz != 0) continue;
        uint32_t r = fill;
        if ((unsigned)(z + dz) < (unsigned)D && (unsigned)(y + dy) < (unsigned)H) {
          const uint32_t* p = src + ((int64_t)(z + dz) * H + (y + dy)) * wpr;
          const uint32_t w = load_word(p, j, wpr, tail, fill);
          r = w;
          if (m <= C - 1) {
            const uint32_t lo = j > 0 ? p[j - 1] : fill;                                   // (never a row's last word)
            const uint32_t hi = j + 1 < wpr ? load_word(p, j + 1, wpr, tail, fill) : fill;
            const uint32_t from_left = (w << 1) | (lo >> 31), from_right = (w >> 1) | (hi << 31);
            r = ERODE ? w & from_left & from_right : w | from_left | from_right;
          }
        }
        acc = ERODE ? acc & r : acc | r;
      }
    }
    dst[t] = acc;
  }
}

// ------------------------------------------------------------------------------------------------ unpack
// out may be vol: a voxel is read and written by one thread only
template <bool MAP>
__global__ __launch_bounds__(256) void morph_unpack_kernel(const uint32_t* __restrict__ packed, const uint8_t* vol, int label,
                                                           int W, int wpr, uint32_t lanes, bool vec, uint8_t* out,
                                                           unsigned long long* __restrict__ result) {
  const uint32_t lpr = 2u * (uint32_t)wpr;
  uint32_t cnt = 0, chg = 0;
  for (uint32_t t = blockIdx.x * 256u + threadIdx.x; t < lanes; t += gridDim.x * 256u) {
    const uint32_t row = t / lpr, c = t % lpr;
    const int n = W - (int)c * LANE_VOX;
    if (n <= 0) continue;
    const uint32_t valid = n < LANE_VOX ? (1u << n) - 1u : 0xffffu;
    const uint32_t now = (packed[t >> 1] >> (16 * (c & 1))) & valid;
    const int64_t at = (int64_t)row * W + c * LANE_VOX;
    Bytes16 d, o;
    load16(vol + at, n, vec, &d);
    const uint32_t was = mask_bits(d, label);
    cnt += __popc(now), chg += __popc(now ^ was);
#pragma unroll
    for (int k = 0; k < LANE_VOX; k++) {
      const bool a = (now >> k) & 1, b = (was >> k) & 1;
      if (MAP)
        o.b[k] = a == b ? d.b[k] : (a ? (d.b[k] ? d.b[k] : (uint8_t)label) : (uint8_t)0);
      else
        o.b[k] = a;
    }
    if (vec) {
      *reinterpret_cast<u32x4*>(out + at) = o.v;
    } else {
#pragma unroll
      for (int k = 0; k < LANE_VOX; k++)
        if (k < n) out[at + k] = o.b[k];
    }
  }
  block_add_counts({cnt, chg}, result);   // one pair of integer atomics a workgroup
}

// ------------------------------------------------------------------------------------------------ fill holes
// comp = 1 on the background of the mask; flag[0 .. V] cleared (component ids run 1 .. n <= V)
__global__ __launch_bounds__(256) void fill_complement_kernel(const uint8_t* __restrict__ vol, int label, int64_t V,
                                                              uint8_t* __restrict__ comp, uint8_t* __restrict__ flag) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
    comp[v] = in_mask(vol[v], label) ? 0 : 1;
    flag[v] = 0;
    if (v == 0) flag[V] = 0;
  }
}

// the voxels of the faces (edges of a depth-1 volume), a face after the other: z = 0 | D-1, y = 0 | H-1, x = 0 | W-1.  Every
// writer of a flag stores the same byte.
__global__ __launch_bounds__(256) void fill_faces_kernel(const int32_t* __restrict__ ids, int D, int H, int W, int64_t nz,
                                                         int64_t ny, int64_t nx, int64_t V, uint8_t* __restrict__ flag) {
  const int64_t total = 2 * (nz + ny + nx);
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    int z, y, x;
    if (t < 2 * nz) {
      const int64_t r = t % nz;
      z = t < nz ? 0 : D - 1, y = (int)(r / W), x = (int)(r % W);
    } else if (t < 2 * (nz + ny)) {
      const int64_t u = t - 2 * nz, r = u % ny;
      y = u < ny ? 0 : H - 1, z = (int)(r / W), x = (int)(r % W);
    } else {
      const int64_t u = t - 2 * (nz + ny), r = u % nx;
      x = u < nx ? 0 : W - 1, z = (int)(r / H), y = (int)(r % H);
    }
    const int id = ids[((int64_t)z * H + y) * W + x];
    if (id > 0 && id <= V) flag[id] = 1;
  }
}

// a background voxel is filled iff its component met no face.  out may be vol.
template <bool MAP>
__global__ __launch_bounds__(256) void fill_write_kernel(const uint8_t* vol, const int32_t* __restrict__ ids,
                                                         const uint8_t* __restrict__ flag, int label, int64_t V, uint8_t* out,
                                                         unsigned long long* __restrict__ result) {
  uint32_t cnt = 0, chg = 0;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
    const uint8_t val = vol[v];
    const bool was = in_mask(val, label);
    const int id = ids[v];
    const bool hole = !was && id > 0 && id <= V && !flag[id];
    cnt += was || hole, chg += hole;
    if (MAP)
      out[v] = hole && val == 0 ? (uint8_t)label : val;
    else
      out[v] = was || hole;
  }
  block_add_counts({cnt, chg}, result);
}

int words_per_row(int W) { return (W + 31) / 32; }
int64_t packed_bytes(int D, int H, int W) { return up256((int64_t)D * H * words_per_row(W) * 4); }

// fill holes: every part on a 256-byte boundary
struct FillCarve {
  int64_t scalars, comp, ids, flag, cc, total;
  FillCarve(int D, int H, int W) {
    const int64_t V = (int64_t)D * H * W;
    Carver c;
    scalars = c.take(256);                      // result[2] of the labelling
    comp = c.take(V);                           // the complement map, uint8
    ids = c.take(V * 4);                        // its component ids, int32
    flag = c.take(V + 1);                       // a byte per id 0 .. V
    cc = c.take(hdf_cc_ws_bytes(D, H, W));      // the labelling's own workspace
    total = c.at;
  }
};

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <bool ERODE>
void launch_step(int c, unsigned grid, hipStream_t stream, const uint32_t* src, uint32_t* dst, int D, int H, int wpr, uint32_t tail,
                 uint32_t fill, bool flat, uint32_t words) {
  if (c == 1)
    hipLaunchKernelGGL((morph_step_kernel<1, ERODE>), dim3(grid), dim3(256), 0, stream, src, dst, D, H, wpr, tail, fill, flat, words);
  else if (c == 2)
    hipLaunchKernelGGL((morph_step_kernel<2, ERODE>), dim3(grid), dim3(256), 0, stream, src, dst, D, H, wpr, tail, fill, flat, words);
  else
    hipLaunchKernelGGL((morph_step_kernel<3, ERODE>), dim3(grid), dim3(256), 0, stream, src, dst, D, H, wpr, tail, fill, flat, words);
}
}  // namespace

int hdf_morph_check_mask_args(const char* who, int label, int connectivity, int mode) {
  HDF_CHECK_ARG(connectivity == 6 || connectivity == 18 || connectivity == 26, "morphology: %s: connectivity %d (6, 18 or 26)",
                who, connectivity);
  HDF_CHECK_ARG(label >= 0 && label <= 255, "morphology: %s: label %d (0..255)", who, label);
  HDF_CHECK_ARG(mode == HDF_MORPH_MASK || mode == HDF_MORPH_MAP, "morphology: %s: mode %d (HDF_MORPH_MASK or HDF_MORPH_MAP)", who,
                mode);
  HDF_CHECK_ARG(mode != HDF_MORPH_MAP || label >= 1, "morphology: %s: HDF_MORPH_MAP needs a label of 1..255", who);
  return HDF_OK;
}
int64_t hdf_morph_ws_bytes(int D, int H, int W) { return 2 * packed_bytes(D, H, W); }
int64_t hdf_fill_holes_ws_bytes(int D, int H, int W) { return FillCarve(D, H, W).total; }

int hdf_launch_morph(const uint8_t* vol, int label, int op, int connectivity, int iterations, int border_value, int mode, int D,
                     int H, int W, uint8_t* out, unsigned long long* result, void* ws, hipStream_t stream) {
  const int wpr = words_per_row(W), c = connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3;
  const uint32_t words = (uint32_t)((int64_t)D * H * wpr), lanes = 2 * words;   // at most 2^25 and 2^26
  const uint32_t tail = W % 32 ? (1u << (W % 32)) - 1u : ~0u, fill = border_value ? ~0u : 0u;
  const bool vec = W % LANE_VOX == 0 && aligned16(vol) && aligned16(out);
  uint32_t* buf[2] = {(uint32_t*)ws, (uint32_t*)((char*)ws + packed_bytes(D, H, W))};
  hipLaunchKernelGGL(morph_pack_kernel, dim3(vol_grid(lanes, 1 << 22)), dim3(256), 0, stream, vol, label, W, wpr, lanes, vec,
                     buf[0]);
  HDF_LAUNCH_CHECK();
  const bool erode_first = op == HDF_MORPH_ERODE || op == HDF_MORPH_OPEN;
  const int halves = op == HDF_MORPH_OPEN || op == HDF_MORPH_CLOSE ? 2 : 1;
  const unsigned gs = vol_grid(words, 1 << 22);
  int cur = 0;
  for (int half = 0; half < halves; half++) {
    const bool erode = erode_first != (half == 1);
    for (int i = 0; i < iterations; i++, cur ^= 1) {
      if (erode)
        launch_step<true>(c, gs, stream, buf[cur], buf[cur ^ 1], D, H, wpr, tail, fill, D == 1, words);
      else
        launch_step<false>(c, gs, stream, buf[cur], buf[cur ^ 1], D, H, wpr, tail, fill, D == 1, words);
      HDF_LAUNCH_CHECK();
    }
  }
  HDF_TRY(hdf_zero_async("morphology", result, 16, stream));
  // (every workgroup ends with one atomic a result word: a few thousand of them)
  const unsigned gu = vol_grid(lanes, 4096);
  if (mode == HDF_MORPH_MAP)
    hipLaunchKernelGGL(morph_unpack_kernel<true>, dim3(gu), dim3(256), 0, stream, (const uint32_t*)buf[cur], vol, label, W, wpr,
                       lanes, vec, out, result);
  else
    hipLaunchKernelGGL(morph_unpack_kernel<false>, dim3(gu), dim3(256), 0, stream, (const uint32_t*)buf[cur], vol, label, W, wpr,
                       lanes, vec, out, result);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_fill_holes(const uint8_t* vol, int label, int connectivity, int mode, int D, int H, int W, uint8_t* out,
                          unsigned long long* result, void* ws, hipStream_t stream) {
  const FillCarve cv(D, H, W);
  const int64_t V = (int64_t)D * H * W;
  char* w = (char*)ws;
  uint8_t* comp = (uint8_t*)(w + cv.comp);
  int32_t* ids = (int32_t*)(w + cv.ids);
  uint8_t* flag = (uint8_t*)(w + cv.flag);
  const unsigned gv = vol_grid(V, 1 << 22);
  hipLaunchKernelGGL(fill_complement_kernel, dim3(gv), dim3(256), 0, stream, vol, label, V, comp, flag);
  HDF_LAUNCH_CHECK();
  HDF_TRY(hdf_launch_cc_label(comp, 1, connectivity, D, H, W, ids, (unsigned long long*)(w + cv.scalars), w + cv.cc, stream));
  const int64_t nz = D > 1 ? (int64_t)H * W : 0, ny = (int64_t)D * W, nx = (int64_t)D * H;   // a depth-1 volume has no z face
  hipLaunchKernelGGL(fill_faces_kernel, dim3(vol_grid(2 * (nz + ny + nx), 1 << 22)), dim3(256), 0, stream, (const int32_t*)ids, D,
                     H, W, nz, ny, nx, V, flag);
  HDF_LAUNCH_CHECK();
  HDF_TRY(hdf_zero_async("morphology", result, 16, stream));
  const unsigned gw = vol_grid(V, 4096);
  if (mode == HDF_MORPH_MAP)
    hipLaunchKernelGGL(fill_write_kernel<true>, dim3(gw), dim3(256), 0, stream, vol, (const int32_t*)ids, (const uint8_t*)flag, label,
                       V, out, result);
  else
    hipLaunchKernelGGL(fill_write_kernel<false>, dim3(gw), dim3(256), 0, stream, vol, (const int32_t*)ids, (const uint8_t*)flag,
                       label, V, out, result);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
