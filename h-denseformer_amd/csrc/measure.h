// Measurements of a fp32 image [C][D][H][W] under an int32 id map (measure.hip): per id the voxel count and coordinate
// sums, and per channel sum, mean, M2, minimum and maximum with their positions, and the weighted coordinate sums.
// Definitions and the numerical contract: include/hdf.h.
#pragma once
#include "../../include/hdf.h"
#include "hdf_common.h"
#include "volume_host.h"

constexpr int HDF_MEASURE_MAX_DIM = 1024;
static_assert(HDF_MEASURE_MAX_DIM == HDF_VOL_MAX_DIM, "hdf_vol_check_dims: one cap");
constexpr int HDF_MEASURE_MAX_CHANNELS = 8;
constexpr int64_t HDF_MEASURE_MAX_CAPACITY = 65536;
constexpr int HDF_MEASURE_SLABS = 8;   // partial sums per (channel, id): part of the documented order of the additions

int64_t hdf_cc_measure_ws_bytes(int C, int64_t capacity);

int hdf_launch_cc_measure(const int32_t* ids, const float* image, int C, int D, int H, int W, int64_t capacity, long long* geom,
                          double* stats, long long* pos, unsigned long long* result, void* ws, hipStream_t st);
