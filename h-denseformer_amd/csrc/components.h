// Connected components of a uint8 label map (components.hip): labelling by union-find, the per-component table, the
// size / largest-of-its-value filter.  Definitions: include/hdf.h.
#pragma once
#include "../../include/hdf.h"
#include "hdf_common.h"

constexpr int HDF_CC_MAX_DIM = 1024;
constexpr int HDF_CC_TABLE_COLS = 9;   // size value first zmin zmax ymin ymax xmin xmax

// host-side argument checks shared by the entries: HDF_ERR_ARG with a "components:" message
int hdf_cc_check_dims(const char* who, int D, int H, int W);
// [a, a + na) and [b, b + nb) share a byte
bool hdf_cc_overlap(const void* a, int64_t na, const void* b, int64_t nb);
int64_t hdf_cc_ws_bytes(int D, int H, int W);

int hdf_launch_cc_label(const uint8_t* vol, int label, int connectivity, int D, int H, int W, int32_t* ids,
                        unsigned long long* result, void* ws, hipStream_t st);
int hdf_launch_cc_table(const uint8_t* vol, const int32_t* ids, const float* score, int D, int H, int W, int64_t capacity,
                        long long* table, float* score_max, hipStream_t st);
int hdf_launch_cc_filter(const uint8_t* vol, const int32_t* ids, int D, int H, int W, int64_t min_size, int keep_largest,
                         uint8_t* out, unsigned long long* result, void* ws, hipStream_t st);
