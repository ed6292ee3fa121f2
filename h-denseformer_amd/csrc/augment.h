// The device-side input pipeline (augment.hip): normalisation, one-hot staging, the 3-D and 2-D training augmentation.
#pragma once
#include "hdf_common.h"

// [A | t] of RandomTranslationRotationZoom3D, row-major 3x4, passed to the kernel by value
struct AugAffine {
  double m[12];
};

// one training sample through warp + flip (+ one-hot): image [C][D][H][W] fp32, labels [D][H][W] uint8 (null when
// neither label output is asked for); every output may be null.  data_utils/transformer_3d.py:45-169
int hdf_launch_augment3d(const float* image, const uint8_t* labels, int C, int n_cls, int D, int H, int W,
                         const AugAffine& aff, int flip_h, int flip_w, float* image_out, uint8_t* labels_out,
                         float* onehot_out, hipStream_t st);

// the parameters of one sample of the 2-D augmentation: PIL's AFFINE matrix (a, b, c, d, e, f), the 16.16 coefficients
// a0 .. a5 of its affine_fixed, the flip code (0 none, 1 W, 2 H); a chunk of them is one kernel argument, passed by value
struct Aug2DSample {
  double m[6];
  int64_t fx[6];
  int flip, pad;
};
constexpr int AUG2D_CHUNK = 32;   // 32 x 104 bytes + the scalars stay under the 4 KB of kernel arguments
struct Aug2DChunk {
  Aug2DSample s[AUG2D_CHUNK];
};

// a batch through RandomRotate2D + RandomFlip2D (+ To_Tensor), bit-exact to PIL: image [B][C][H][W] fp32, labels
// [B][H][W] uint8, matrices [B][6] and flips [B] on the HOST (read during the call); ceil(B / AUG2D_CHUNK) launches.
// data_utils/transformer_2d.py:80-173
int hdf_launch_augment2d(const float* image, const uint8_t* labels, int B, int C, int n_cls, int H, int W,
                         const double* matrices, const uint8_t* flips, float* image_out, uint8_t* labels_out,
                         float* onehot_out, hipStream_t st);

// in-place input normalisation of one sample [C][V] fp32 (data_utils/data_loader.py:39-68); mode 0 MR, 1 PET/CT
size_t hdf_norm_ws_bytes(int C);
int hdf_launch_normalize(float* img, int C, int64_t V, int mode, float pmean, float pw, void* ws, hipStream_t st);
// class maps [N][V] uint8 -> one-hot [N][C][V] fp32 (labels outside [1, C) count as background)
int hdf_launch_onehot(const uint8_t* lab, float* oh, int N, int C, int64_t V, hipStream_t st);
