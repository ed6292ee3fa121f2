// The overlap table of two id maps (cc_pairs.hip): which component of A meets which component of B, in how many voxels,
// and in how many voxels under a mask.  Definitions: include/hdf.h.
#pragma once
#include "../../include/hdf.h"
#include "hdf_common.h"

constexpr int64_t HDF_PAIRS_MAX_CAPACITY = 65536;
constexpr int HDF_PAIRS_TRIP = 256;                    // voxels a workgroup reads per trip: one a thread
constexpr int HDF_PAIRS_SPAN = HDF_PAIRS_TRIP * 32;    // consecutive voxels a workgroup of the voxel pass walks
constexpr int HDF_PAIRS_LDS_SLOTS = 256;               // pairs a workgroup collects in LDS before it goes to memory
constexpr int HDF_PAIRS_SORT_CHUNK = 8192;             // keys one workgroup sorts in LDS: 64 KB

// slots of the global table for a capacity: a power of two, at least twice the capacity
int64_t hdf_cc_pairs_slots(int64_t capacity);
int64_t hdf_cc_pairs_ws_bytes(int64_t capacity);

int hdf_launch_cc_pairs(const int32_t* ids_a, const int32_t* ids_b, const uint8_t* mask, int flags, int D, int H, int W,
                        int64_t capacity, long long* pairs, unsigned long long* result, void* ws, hipStream_t st);
