// The device-side input pipeline (augment.hip): normalisation, one-hot staging, the 3-D and 2-D training augmentation
// (rotation + flip + one-hot; label bounding box; erase + zoom; gamma + noise).
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

// the parameters of one sample of the 2-D zoom: the keep-rectangle of the erase, rows [r0, r1) x columns [c0, c1), and the
// canvas, sw wide and sh high with the plane's origin at (oy, ox); a chunk of them is one kernel argument, passed by value
struct Zoom2DSample {
  int r0, r1, c0, c1, sw, sh, ox, oy;
};
struct Zoom2DChunk {
  Zoom2DSample s[AUG2D_CHUNK];
};

// a batch through RandomErase2D + RandomZoom2D, bit-exact to PIL's crop / expand + resize: image [B][C][H][W] fp32,
// labels [B][H][W] uint8, keep [B][4] and canvas [B][4] int32 on the HOST (read during the call); ceil(B / AUG2D_CHUNK)
// launches.  data_utils/transformer_2d.py:11-77, 177-275
int hdf_launch_zoom2d(const float* image, const uint8_t* labels, int B, int C, int H, int W, const int32_t* keep,
                      const int32_t* canvas, float* image_out, uint8_t* labels_out, hipStream_t st);

// (non-zero count, rmin, rmax, cmin, cmax) of each class map of labels [B][H][W] into bbox [B][5] int32 on the device
size_t hdf_label_bbox_ws_bytes(int B);
int hdf_launch_label_bbox2d(const uint8_t* labels, int B, int H, int W, int32_t* bbox, void* ws, hipStream_t st);

// RandomAdjust2D + RandomNoise2D in place on image [B][n] fp32: gamma [B] doubles and noise [B] bytes on the HOST
// (read during the call); ceil(B / AUG2D_CHUNK) launches.  data_utils/transformer_2d.py:279-322
struct Intensity2DChunk {
  double gamma[AUG2D_CHUNK];
  uint8_t noise[AUG2D_CHUNK];
};
int hdf_launch_intensity2d(float* image, int B, int64_t n, const double* gamma, const uint8_t* noise, uint64_t seed,
                           float low_clip, hipStream_t st);

// in-place input normalisation of one sample [C][V] fp32 (data_utils/data_loader.py:39-68); mode 0 MR, 1 PET/CT
size_t hdf_norm_ws_bytes(int C);
int hdf_launch_normalize(float* img, int C, int64_t V, int mode, float pmean, float pw, void* ws, hipStream_t st);
// class maps [N][V] uint8 -> one-hot [N][C][V] fp32 (labels outside [1, C) count as background)
int hdf_launch_onehot(const uint8_t* lab, float* oh, int N, int C, int64_t V, hipStream_t st);

// one axis of skimage.transform.resize(order=1) as scipy computes it (resize.hip): n_in -> n_out samples, f = n_in / n_out,
// the 2r + 1 normalised Gaussian weights of the anti-aliasing filter (r = 0, w = {1}: none), constant != 0 for scipy's
// 'grid-constant' with cval 0 (labels), else 'mirror' (image).  Computed on the host in fp64 and passed to the kernel by
// value: r <= 14 at the factor cap of 8.
constexpr int RESIZE_MAX_RADIUS = 14;
struct ResizeAxis {
  int n_in, n_out, r, constant;
  double f;
  double w[2 * RESIZE_MAX_RADIUS + 1];
};

// CropResize's resize of one sample (data_utils/data_loader.py:103-119): image [C][Di][Hi][Wi] fp32 -> image_out
// [C][Do][Ho][Wo], labels [Di][Hi][Wi] uint8 -> labels_out [Do][Ho][Wo]; either pair may be null.  At most three launches
// per image channel and per class 1 .. n_cls-1; ws holds the fp64 intermediates of ONE plane.  -1: shapes out of range
int64_t hdf_resize_ws_bytes(int Di, int Hi, int Wi, int Do, int Ho, int Wo);
int hdf_launch_resize3d(const float* image, const uint8_t* labels, int C, int n_cls, int Di, int Hi, int Wi, int Do, int Ho,
                        int Wo, float* image_out, uint8_t* labels_out, void* ws, int64_t ws_bytes, hipStream_t st);
// Trunc_and_Normalize in place (data_utils/data_loader.py:16-36): ((x - lo) clamped to [0, hi - lo]) / (hi - lo) in fp32
int hdf_launch_trunc_normalize(float* image, int64_t n, float lo, float hi, hipStream_t st);
