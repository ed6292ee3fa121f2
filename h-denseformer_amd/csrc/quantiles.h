// Order statistics of a fp32 image [C][D][H][W] under an int32 id map (quantiles.hip): per id the voxel count, and per
// channel and level the two neighbouring order statistics and their interpolant.  Definitions and the numerical contract:
// include/hdf.h.
#pragma once
#include "measure.h"

constexpr int HDF_QUANTILES_MAX_LEVELS = 16;

int64_t hdf_cc_quantiles_ws_bytes(int64_t capacity);

// q: HOST, Q levels in [0, 1] (checked by the caller); it is read before the call returns
int hdf_launch_cc_quantiles(const int32_t* ids, const float* image, int C, int D, int H, int W, int64_t capacity, const double* q,
                            int Q, long long* count, double* values, unsigned long long* result, void* ws, hipStream_t st);
