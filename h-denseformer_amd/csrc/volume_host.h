// Host-side pieces shared by the entries on a [D][H][W] volume (surface*.hip, components.hip, cc_pairs.hip,
// morphology.hip, api_volume.hip): workspace carving, grids, the dimension check, memset and histogram copy-out.
#pragma once
#include <algorithm>

#include "hdf_common.h"

static inline int64_t up256(int64_t b) { return (b + 255) / 256 * 256; }

// workgroups of 256 threads for n items: at least one, at most cap
static inline unsigned vol_grid(int64_t n, int64_t cap) {
  return (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div64(n, 256), 1), cap);
}

// consecutive parts of a workspace, every one on a 256-byte boundary: take() returns the offset of a part of `bytes`
// bytes, `at` is the offset behind the last one (the total)
struct Carver {
  int64_t at = 0;
  int64_t take(int64_t bytes) {
    const int64_t off = at;
    at += up256(bytes);
    return off;
  }
};

// [a, a + na) and [b, b + nb) share a byte
static inline bool hdf_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

// every dimension of 1..HDF_VOL_MAX_DIM: HDF_ERR_ARG with a "<prefix>: <who>: " message.  Each family names its own cap
// (HDF_SURFACE_MAX_DIM, HDF_CC_MAX_DIM, HDF_MORPH_MAX_DIM) and asserts beside it that it is this one.
constexpr int HDF_VOL_MAX_DIM = 1024;
static inline int hdf_vol_check_dims(const char* prefix, const char* who, int D, int H, int W) {
  const int M = HDF_VOL_MAX_DIM;
  HDF_CHECK_ARG(D >= 1 && D <= M && H >= 1 && H <= M && W >= 1 && W <= M, "%s: %s: volume %dx%dx%d (each of 1..%d)", prefix,
                who, D, H, W, M);
  // (belt and braces: with every dimension at most 1024 the product is at most 2^30; the kernels' 32-bit voxel, word and
  // lane arithmetic rests on this bound, so it is stated where the cap could one day be raised)
  HDF_CHECK_ARG((int64_t)D * H * W < (1ll << 31), "%s: %s: %dx%dx%d has 2^31 voxels or more", prefix, who, D, H, W);
  return HDF_OK;
}

// what an earlier call left in a part of the workspace (or a result) cleared on the stream, ahead of the kernels
static inline int hdf_zero_async(const char* prefix, void* p, size_t bytes, hipStream_t st) {
  if (hipMemsetAsync(p, 0, bytes, st) != hipSuccess) {
    hdf_set_error("%s: memset failed", prefix);
    return HDF_ERR_HIP;
  }
  return HDF_OK;
}

// the first min(len, nbins) bins of a device histogram to the caller's buffer of `len` entries, zeros behind them
static inline int hdf_copy_hist_out(const char* prefix, uint32_t* dst, int64_t len, const uint32_t* hist, int64_t nbins,
                                    hipStream_t st) {
  const int64_t take = std::min(len, nbins);
  hipError_t e = hipMemcpyAsync(dst, hist, (size_t)take * 4, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess && len > take) e = hipMemsetAsync(dst + take, 0, (size_t)(len - take) * 4, st);
  if (e != hipSuccess) {
    hdf_set_error("%s: histogram copy failed: %s", prefix, hipGetErrorString(e));
    return HDF_ERR_HIP;
  }
  return HDF_OK;
}
