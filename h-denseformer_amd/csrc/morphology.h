// Binary morphology of a uint8 label map (morphology.hip): dilate / erode / open / close on a bit-packed mask, fill holes
// through the labelling of the complement (components.hip).  Definitions: include/hdf.h.
#pragma once
#include "../../include/hdf.h"
#include "hdf_common.h"
#include "volume_host.h"

constexpr int HDF_MORPH_MAX_DIM = 1024;
static_assert(HDF_MORPH_MAX_DIM == HDF_VOL_MAX_DIM, "hdf_vol_check_dims: one cap");
constexpr int HDF_MORPH_MAX_ITER = 256;

// host-side argument check shared by the entries: HDF_ERR_ARG with a "morphology:" message
int hdf_morph_check_mask_args(const char* who, int label, int connectivity, int mode);
int64_t hdf_morph_ws_bytes(int D, int H, int W);
int64_t hdf_fill_holes_ws_bytes(int D, int H, int W);

int hdf_launch_morph(const uint8_t* vol, int label, int op, int connectivity, int iterations, int border_value, int mode, int D,
                     int H, int W, uint8_t* out, unsigned long long* result, void* ws, hipStream_t st);
int hdf_launch_fill_holes(const uint8_t* vol, int label, int connectivity, int mode, int D, int H, int W, uint8_t* out,
                          unsigned long long* result, void* ws, hipStream_t st);
