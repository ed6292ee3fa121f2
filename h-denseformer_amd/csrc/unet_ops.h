// HBM-bound U-Net ops around the convolutions: norm_ops.hip (InstanceNorm finalise / backward, norm+ReLU+skip),
// pool_ops.hip (layout conversion, pooling, up-sampling, the encoder tails) and head_ops.hip (the 1x1x1 heads).  All
// tensors channels-last with a voxel pitch; storage bf16, f16 or f32 (dtype enum), statistics and parameters fp32.
#pragma once
#include "hdf_common.h"

// ---- what the launchers take
// a channels-last tensor: first element + voxel pitch (elements from one voxel's channel row to the next)
struct CRows {
  const void* p = nullptr;
  int64_t pitch = 0;
};
struct Rows {  // the same, written
  void* p = nullptr;
  int64_t pitch = 0;
  operator CRows() const { return CRows{p, pitch}; }
};
// the forward constants of an InstanceNorm, each [N][C]: scale = gamma*rstd, shift = beta - mean*scale.  A launcher that
// reads only some of them says so; the rest may be null.
struct NormStats {
  const float *scale = nullptr, *shift = nullptr, *mean = nullptr, *rstd = nullptr;
};
struct NormStatsOut {  // the same, written
  float *scale = nullptr, *shift = nullptr, *mean = nullptr, *rstd = nullptr;
  operator NormStats() const { return NormStats{scale, shift, mean, rstd}; }
};
// the coefficients of an InstanceNorm(+ReLU) backward, each [N][C]: dy = k1 * (g - ka - xhat*kb)
struct InBwdCoef {
  const float *k1 = nullptr, *ka = nullptr, *kb = nullptr;
};
struct InBwdCoefOut {  // the same, written
  float *k1 = nullptr, *ka = nullptr, *kb = nullptr;
  operator InBwdCoef() const { return InBwdCoef{k1, ka, kb}; }
};
// batch, channels and the extent a pooling / resampling launcher works at: the LOW-resolution side (pooled voxels, the
// input of an up-sampling).  flat = 1: the 2-D form on depth-1 tensors (MaxPool2d(2) / bilinear x2, round 6) where the
// launcher has one (enc_tail, maxpool_bwd_in, upsample_fwd / bwd); the others do not look at it.
struct Extent {
  int N = 0, C = 0, D = 0, H = 0, W = 0;
  int flat = 0;
};

// ---- pool_ops.hip
// x [N,C,D,H,W] fp32 (the reference's input layout) -> [N,D,H,W,CP] storage type, channels >= C zero
int hdf_launch_nchw_to_ndhwc(int dtype, const float* x, void* out, int N, int C, int CP, int64_t vox, hipStream_t st);

// fused encoder tail: ds = relu(y*scale+shift) + skip, pooled/idx = MaxPool3d(2)(ds); skip a materialised
// full-resolution tensor; x: the pooled extent.  ys: scale, shift
int hdf_launch_enc_tail(int dtype, CRows y, NormStats ys, CRows skip, Rows ds, Rows pooled, uint8_t* idx, Extent x,
                        hipStream_t st);
// the same with skip = trilinear x2 of relu(low * ls.scale + ls.shift), low at the pooled extent: the skip tensor is never
// materialised
int hdf_launch_enc_tail_up(int dtype, CRows y, NormStats ys, CRows low, NormStats ls, Rows ds, Rows pooled, uint8_t* idx,
                           Extent x, hipStream_t st);
int hdf_launch_maxpool_fwd(int dtype, CRows in, Rows out, uint8_t* idx, Extent x, hipStream_t st);
// din[8 positions] (+)= (pos == idx) ? dout : 0
int hdf_launch_maxpool_bwd(int dtype, CRows dout, const uint8_t* idx, Rows din, Extent x, int accumulate, hipStream_t st);
// MaxPool3d(2) backward accumulating into din + the first pass of the InstanceNorm(+ReLU) backward of the layer whose
// activation gradient din then is (hdf_maxpool_bwd_in_blocks rows per sample in `partials`).  ys: all four
int hdf_maxpool_bwd_in_blocks(int64_t pooled_vox, int C);
int hdf_launch_maxpool_bwd_in(int dtype, CRows dout, const uint8_t* idx, Rows din, CRows y, NormStats ys, float* partials,
                              Extent x, hipStream_t st);

// trilinear x2, align_corners=False, of relu(y*scale+shift); x: the extent of y
int hdf_launch_upsample_fwd(int dtype, CRows y, NormStats ys, Rows out, Extent x, hipStream_t st);
// transposed stencil: din[lo-res] = sum of weighted dout[hi-res]; x: the extent of din
int hdf_launch_upsample_bwd(int dtype, CRows dout, Rows din, Extent x, hipStream_t st);

// ---- head_ops.hip
// 1x1x1 head: logits[N][ncls][vox] (NCDHW) = W[ncls][C] . act(in) + b ;  act = relu(in*scale+shift) if ins.scale
int hdf_launch_head_fwd(int dtype, CRows in, NormStats ins, const float* w, const float* b, void* logits, int N, int C,
                        int ncls, int64_t vox, hipStream_t st);
// dX (+)= W^T dlogits ; dW += dlogits . act(in)^T ; db += sum dlogits   (dW, db accumulated with float atomics).
// inb_partials (optional; needs ins.scale / mean / rstd): the first pass of the InstanceNorm(+ReLU) backward of the layer
// that produced `in`, hdf_head_bwd_blocks rows per sample
struct HeadGrads {
  Rows dx;
  int accumulate_dx = 0;
  float *dw = nullptr, *db = nullptr;
  float* inb_partials = nullptr;
};
int hdf_head_bwd_blocks(int64_t vox);
int hdf_launch_head_bwd(int dtype, const void* dlogits, CRows in, NormStats ins, const float* w, HeadGrads g, int N, int C,
                        int ncls, int64_t vox, hipStream_t st);

// ---- norm_ops.hip
// (sum,sumsq) partials [N][tiles][CP][2] -> per-(n,c) mean, rstd, scale = gamma*rstd, shift = beta - mean*scale
int hdf_launch_in_finalize(const float* partials, int N, int tiles, int C, int CP, int64_t vox, const float* gamma,
                           const float* beta, float eps, NormStatsOut out, hipStream_t st);

// out = relu(y*scale+shift) + skip   (skip.p may be null)
int hdf_launch_norm_relu_add(int dtype, CRows y, NormStats ys, CRows skip, Rows out, int N, int C, int64_t vox,
                             hipStream_t st);

// InstanceNorm+ReLU backward, stage 1: g = da * [y*scale+shift > 0]; partial sums of g and g*xhat.  ys: all four
int hdf_launch_in_bwd_reduce(int dtype, CRows da, CRows y, NormStats ys, float* partials /*[N][blocks][C][2]*/, int blocks,
                             int N, int C, int64_t vox, hipStream_t st);
// stage 2: per (n,c) coefficients + dgamma/dbeta (accumulated, may be null for non-affine norms)
int hdf_launch_in_bwd_finalize(const float* partials, int blocks, int N, int C, int64_t vox, const float* gamma,
                               const float* rstd, InBwdCoefOut k, float* dgamma, float* dbeta, hipStream_t st);
// stage 3: dy = k1 * (g - ka - xhat*kb)
int hdf_launch_in_bwd_apply(int dtype, CRows da, CRows y, NormStats ys, InBwdCoef k, Rows dy, int N, int C, int64_t vox,
                            hipStream_t st);
int hdf_in_bwd_blocks(int64_t vox, int C);

// out[c] += column sums (sum column) of a conv InstanceNorm partial table [rows][CP][2], c < C
int hdf_launch_stat_rows_sum(const float* partials, int rows, int C, int CP, float* out, hipStream_t st);
