// Connected components of a uint8 label map (components.hip): labelling by union-find, the per-component table, the
// size / largest-of-its-value filter.  Definitions: include/hdf.h.
#pragma once
#include "../../include/hdf.h"
#include "hdf_common.h"
#include "volume_host.h"

constexpr int HDF_CC_MAX_DIM = 1024;
static_assert(HDF_CC_MAX_DIM == HDF_VOL_MAX_DIM, "hdf_vol_check_dims: one cap");
constexpr int HDF_CC_TABLE_COLS = 9;   // size value first zmin zmax ymin ymax xmin xmax

int64_t hdf_cc_ws_bytes(int D, int H, int W);

int hdf_launch_cc_label(const uint8_t* vol, int label, int connectivity, int D, int H, int W, int32_t* ids,
                        unsigned long long* result, void* ws, hipStream_t st);
int hdf_launch_cc_table(const uint8_t* vol, const int32_t* ids, const float* score, int D, int H, int W, int64_t capacity,
                        long long* table, float* score_max, hipStream_t st);
int hdf_launch_cc_filter(const uint8_t* vol, const int32_t* ids, int D, int H, int W, int64_t min_size, int keep_largest,
                         uint8_t* out, unsigned long long* result, void* ws, hipStream_t st);
