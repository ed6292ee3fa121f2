// The evaluation path (metrics.hip, sw_infer.hip, slice_infer.hip): the on-device Dice metric and the sliding-window inference tail.
#pragma once
#include "loss.h"  // HDF_CLASS_SLOTS

// counts[n][c][3] = (|P=c & T=c|, |P=c|, |T=c|), n < N, c < HDF_CLASS_SLOTS
int hdf_launch_dice_counts(int dtype, const void* logits, const float* target, int N, int C, int64_t V,
                           unsigned long long* counts, hipStream_t st);
// conf[t][p] (HDF_CLASS_SLOTS x HDF_CLASS_SLOTS) (+)= voxels of target class t predicted as p, from logits + one-hot ...
int hdf_launch_confusion(int dtype, const void* logits, const float* target, int N, int C, int64_t V,
                         unsigned long long* conf, int accumulate, hipStream_t st);
// ... or from two uint8 class maps
int hdf_launch_confusion_labels(const uint8_t* tgt, const uint8_t* pred, int C, int64_t n, unsigned long long* conf,
                                int accumulate, hipStream_t st);
int hdf_launch_sw_accumulate(int dtype, const void* logits, int C, int pd, int ph, int pw, float* psum, float* cnt,
                             int D, int H, int W, int z0, int y0, int x0, hipStream_t st);
int hdf_launch_sw_finalize(const float* psum, const float* cnt, int C, int64_t V, uint8_t* label, hipStream_t st);
// sw_infer.hip: the window's K mirrored copies for the forward, the floor of its importance map, and the tail that
// un-mirrors, averages and accumulates the K softmaxes under that map
int hdf_launch_sw_gather(const float* image, int C, int D, int H, int W, int z0, int y0, int x0, int ed, int eh, int ew,
                         int Pd, int Ph, int Pw, unsigned mask, float* out, hipStream_t st);
int hdf_launch_sw_importance_floor(const double* tables, int ed, int eh, int ew, float* floor_out, hipStream_t st);
int hdf_launch_sw_accumulate_tta(int dtype, const void* logits, unsigned mask, int C, int ed, int eh, int ew, int Pd, int Ph,
                                 int Pw, const double* tables, const float* floor, float* psum, float* wsum, int D, int H,
                                 int W, int z0, int y0, int x0, hipStream_t st);
// slice_infer.hip: the same around the 2-D model's forward of a group of slices -- the maxima of the volume's planes, the
// slices' mirrored and normalised copies, and the tail over all of them in one launch
int hdf_launch_plane_max(const float* image, int planes, int64_t pv, float* max_out, hipStream_t st);
int hdf_launch_slice_gather(const float* image, int C, int D, int H, int W, int z0, int nz, int y0, int x0, int eh, int ew,
                            int Ph, int Pw, unsigned mask, int mode, const float* plane_max, float* out, hipStream_t st);
int hdf_launch_slice_accumulate(int dtype, const void* logits, unsigned mask, int C, int nz, int eh, int ew, int Ph, int Pw,
                                const double* tables, float floor, float* psum, float* wsum, int D, int H, int W, int z0,
                                int y0, int x0, hipStream_t st);
