// Lesion candidates from a probability map (detect.hip): peak, threshold at peak / factor, the component of the peak,
// drop what touches an accepted candidate, repeat.  Definitions: include/hdf.h.
#pragma once
#include "../../include/hdf.h"
#include "hdf_common.h"
#include "volume_host.h"

constexpr int HDF_DETECT_GRID_CAP = 2048;   // workgroups of 256 of every voxel pass here: eight a compute unit
constexpr int HDF_DETECT_TABLE_COLS = 6;    // index, bits of m, size, a, status, fp64 bits of thr
constexpr int HDF_DETECT_STATE_BYTES = 256;

struct DetectArgs {
  int num_lesions, connectivity, remove_adjacent, first_round, rounds;
  double factor, stop;
  int64_t min_voxels, table_rows;
};

int64_t hdf_detect_ws_bytes(int D, int H, int W);

int hdf_launch_detect(const float* prob, int D, int H, int W, const DetectArgs& args, float* det, int32_t* idx, long long* table,
                      unsigned long long* result, void* ws, hipStream_t st);
