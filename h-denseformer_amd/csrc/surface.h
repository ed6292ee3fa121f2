// Surface-distance evaluation (surface.hip): mask flags, the exact squared Euclidean distance transform, the gather of
// surface distances into a histogram and the order-statistic select; the average surface distance on top of that
// transform (surface_asd.hip); both with a voxel spacing, in fp64 (surface_mm.hip).  Definitions: include/hdf.h.
#pragma once
#include "../../include/hdf.h"  // HDF_EDT_NO_SEED
#include "hdf_common.h"
#include "volume_host.h"

// flag byte of one voxel (hdf_op_mask_flags)
enum {
  HDF_SF_IN_T = 1,    // target == label
  HDF_SF_IN_P = 2,    // prediction == label
  HDF_SF_B26_T = 4,   // in T with an in-volume 26-neighbour outside T: the seeds of d2_T
  HDF_SF_B26_P = 8,
  HDF_SF_C6_T = 16,   // in T with an in-volume face neighbour outside T: the contour
  HDF_SF_C6_P = 32,
  // set by hdf_op_edge_flags only (surface_asd.hip), which leaves bits 4..32 clear
  HDF_SF_E6_T = 64,   // in T with a face neighbour outside T, a neighbour outside the volume included: MONAI's edge set
  HDF_SF_E6_P = 128,
};
// "no seed anywhere" is HDF_EDT_NO_SEED (include/hdf.h): + 1023^2 = 1 074 788 352 < 2^31, and every real squared
// distance (at most 3 * 1023^2) is below it
constexpr int HDF_SURFACE_MAX_DIM = 1024;
static_assert(HDF_SURFACE_MAX_DIM == HDF_VOL_MAX_DIM, "hdf_vol_check_dims: one cap");

int64_t hdf_surface_ws_bytes(int D, int H, int W);
// bins of the squared-distance histogram: (D-1)^2 + (H-1)^2 + (W-1)^2 + 1
int64_t hdf_surface_hist_bins(int D, int H, int W);

// counts_are_zero: the caller has cleared counts[5] on the stream already
int hdf_launch_mask_flags(const uint8_t* tgt, const uint8_t* pred, int label, int D, int H, int W, uint8_t* flags,
                          unsigned long long* counts, bool counts_are_zero, hipStream_t st);
int hdf_launch_edt_sq(const uint8_t* flags, int seed_mask, int D, int H, int W, int32_t* d2, hipStream_t st);
// the first pass of that transform alone (along W).  in_fp64_slots: voxel v's int32 goes to the low word of the fp64 slot
// v (d2[2 v]) and the high words are left as they are -- where surface_mm.hip's pass along H picks it up
int hdf_launch_edt_row(const uint8_t* flags, int seed_mask, int D, int H, int W, int32_t* d2, bool in_fp64_slots,
                       hipStream_t st);
int hdf_launch_surface_distances(const uint8_t* tgt, const uint8_t* pred, int label, int D, int H, int W, void* ws,
                                 unsigned long long* result, uint32_t* hist_out, int64_t hist_len, hipStream_t st);

// average surface distance (surface_asd.hip).  hdf_surface_asd_ws_bytes >= hdf_surface_ws_bytes for every volume.
int64_t hdf_surface_asd_ws_bytes(int D, int H, int W);
// counts_are_zero: the caller has cleared counts[2] on the stream already
int hdf_launch_edge_flags(const uint8_t* tgt, const uint8_t* pred, int label, int D, int H, int W, uint8_t* flags,
                          unsigned long long* counts, bool counts_are_zero, hipStream_t st);
int hdf_launch_surface_asd(const uint8_t* tgt, const uint8_t* pred, int label, int D, int H, int W, void* ws,
                           unsigned long long* result, uint32_t* hist_out, int64_t hist_len, hipStream_t st);
// asd_final_kernel, one workgroup: result[4] from counts[2] and the 2 x nblk partial sums (also what surface_mm.hip ends with)
int hdf_launch_asd_final(const unsigned long long* counts, const double* partial, uint32_t nblk, unsigned long long* result,
                         hipStream_t st);

// the same measures in physical units (surface_mm.hip): squared distances are fp64, weighted per axis by the squared spacing
struct SurfaceSpacing {
  double wz, wy, wx;   // fl(sz sz), fl(sy sy), fl(sx sx)
};
// host-side check of a spacing triple (host pointer): HDF_ERR_ARG with a "surface:" message
int hdf_surface_check_spacing(const char* who, const double* spacing, SurfaceSpacing* out);
int64_t hdf_surface_mm_ws_bytes(int D, int H, int W);
int hdf_launch_edt_sq_mm(const uint8_t* flags, int seed_mask, int D, int H, int W, const SurfaceSpacing& sp, double* d2,
                         hipStream_t st);
// ws: HDF_SELECT_U64_WS bytes
int hdf_launch_select_u64(const unsigned long long* keys, int64_t n, int64_t lo, void* ws, unsigned long long* out2,
                          hipStream_t st);
int hdf_launch_surface_distances_mm(const uint8_t* tgt, const uint8_t* pred, int label, int D, int H, int W,
                                    const SurfaceSpacing& sp, void* ws, unsigned long long* result, hipStream_t st);
int hdf_launch_surface_asd_mm(const uint8_t* tgt, const uint8_t* pred, int label, int D, int H, int W,
                              const SurfaceSpacing& sp, void* ws, unsigned long long* result, hipStream_t st);
