// Per-lesion surface distances on crops (lesion_surface.hip): the join of the overlap table (cc_pairs.hip) with the
// surface entries (surface.hip, surface_mm.hip).  Definitions: include/hdf.h.
#pragma once
#include <vector>

#include "../../include/hdf.h"
#include "surface.h"

constexpr int HDF_LESION_CHUNK = 64;          // lesions one carve launch takes in its kernel arguments
constexpr int HDF_LESION_BLOCK_VOX = 1024;    // consecutive crop voxels a workgroup of the carve kernel writes: four a thread

// one lesion's crop: its box grown by one voxel and clamped to the volume
struct LesionCrop {
  int32_t j;             // the truth id
  int32_t z0, y0, x0;    // the crop's first voxel in the volume
  int32_t cd, ch, cw;    // its extents
  int64_t off;           // byte offset of its truth crop in the workspace; the predicted crop follows at off + cd ch cw
};
// the workspace of a call: the packed crops from byte 0 (2 bytes a crop voxel, in the order of the lesion rows, no padding),
// then, on a 256-byte boundary, one scratch area for the surface entry on the largest crop
struct LesionPlan {
  std::vector<LesionCrop> crops;
  int64_t scratch = 0, total = 0;   // offset of the scratch area, bytes in all
};

// the host arithmetic: every row of lesions[L][7] checked (HDF_ERR_ARG, "surface: <who>: ..."), crops and offsets formed
int hdf_lesion_surface_plan(const char* who, const int32_t* lesions, int64_t L, int D, int H, int W, bool mm, LesionPlan* plan);

// sp: null for distances in voxels.  ws: plan.total bytes, aligned to 8.
int hdf_launch_lesion_surface(const int32_t* ids_pred, const int32_t* ids_truth, const uint8_t* truth_mask, int H, int W,
                              const long long* pairs, int64_t n_pairs, const LesionPlan& plan, const SurfaceSpacing* sp,
                              void* ws, unsigned long long* results, hipStream_t st);
