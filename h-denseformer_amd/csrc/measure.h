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

// measure_table_kernel alone: n and the coordinate sums of every id in geom [capacity][4], its box in box
// [capacity][CC_BOX_COLS] (cc_runs.h), the four result words; with C = 0 no key is formed and image and keys may be null
int hdf_launch_cc_measure_walk(const int32_t* ids, const float* image, int C, int H, int W, int64_t V, int64_t capacity,
                               long long* geom, int* box, unsigned long long* keys, unsigned long long* result, hipStream_t st);
