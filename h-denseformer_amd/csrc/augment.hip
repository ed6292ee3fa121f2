// The reference's 3-D training augmentation on the device, one launch per sample: RandomTranslationRotationZoom3D
// (data_utils/transformer_3d.py:45-120), RandomFlip3D (:123-169) and the To_Tensor one-hot (data_utils/data_loader.py:
// 126-159).  A memory-bound gather: every output voxel reads the eight corners of its source coordinate, per image channel
// and once for the labels.  The reference's angles are +-5 degrees, so a wave's 64 source addresses stay within a few rows
// of one plane: the corners come from L2, nothing is staged through LDS.
//
// All arithmetic between the loads and the one rounding of the store is fp64 (about 60 operations per voxel against about
// 50 bytes of traffic): the reference interpolates in fp64 (scipy.ndimage.map_coordinates, order 1), so the image matches
// it to one fp32 rounding and the labels' 0.5 threshold does not move.
#include <algorithm>
#include <cmath>

#include "augment.h"

namespace {
constexpr int AUG_MAXCLS = 8;   // SW_MAXC of loss.hip: the class slots of the staging and inference kernels
constexpr int AUG_MAXCH = 64;   // the cap of hdf_launch_normalize

// one axis of the trilinear stencil: corner indices i0, i0 + 1, their weights 1 - f, f and whether each lies in [0, n).
// `grid-constant`: the volume is zero-padded to infinity, so a corner outside contributes 0 and a coordinate in (-1, 0)
// blends the edge voxel with 0.  A coordinate far outside (or NaN) is clamped to a cell with both corners outside BEFORE
// the conversion to int.
struct Axis {
  int i0;
  double w0, w1;
  bool in0, in1;
};
__device__ __forceinline__ Axis axis_of(double c, int n) {
  const double fl = floor(c);
  Axis a;
  a.w1 = c - fl;
  a.w0 = 1.0 - a.w1;
  a.i0 = (int)fmin(fmax(fl, -2.0), (double)n);
  a.in0 = a.i0 >= 0 && a.i0 < n;
  a.in1 = a.i0 + 1 >= 0 && a.i0 + 1 < n;
  return a;
}

__global__ void __launch_bounds__(256)
augment3d_kernel(const float* __restrict__ img, const uint8_t* __restrict__ lab, int C, int n_cls, int D, int H, int W,
                 AugAffine aff, int flip_h, int flip_w, float* __restrict__ img_out, uint8_t* __restrict__ lab_out,
                 float* __restrict__ oh_out) {
  const int64_t V = (int64_t)D * H * W;
  const double s0 = D / 2.0, s1 = H / 2.0, s2 = W / 2.0;   // size / 2, not (size - 1) / 2 (transformer_3d.py:66-67)
  const double* m = aff.m;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % W), y = (int)((i / W) % H), z = (int)(i / ((int64_t)W * H));
    // the flip follows the warp: out[d, h, w] = warped[d, H-1-h, w]
    const int ph = flip_h ? H - 1 - y : y, pw = flip_w ? W - 1 - x : x;
    double c0, c1, c2;
    {
      // c = A (p - s) + t + s in the order numpy evaluates it (transformer_3d.py:102-105), no contraction
#pragma clang fp contract(off)
      const double q0 = z - s0, q1 = ph - s1, q2 = pw - s2;
      c0 = m[0] * q0 + m[1] * q1 + m[2] * q2 + m[3] + s0;
      c1 = m[4] * q0 + m[5] * q1 + m[6] * q2 + m[7] + s1;
      c2 = m[8] * q0 + m[9] * q1 + m[10] * q2 + m[11] + s2;
    }
    const Axis ad = axis_of(c0, D), ah = axis_of(c1, H), aw = axis_of(c2, W);
    // eight corners, once per voxel: offset and weight; a corner outside the volume gets weight 0 and is never loaded
    int64_t off[8];
    double wt[8];
    bool in[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int kd = k >> 2, kh = (k >> 1) & 1, kw = k & 1;
      in[k] = (kd ? ad.in1 : ad.in0) && (kh ? ah.in1 : ah.in0) && (kw ? aw.in1 : aw.in0);
      wt[k] = in[k] ? (kd ? ad.w1 : ad.w0) * (kh ? ah.w1 : ah.w0) * (kw ? aw.w1 : aw.w0) : 0.0;
      off[k] = in[k] ? ((int64_t)(ad.i0 + kd) * H + (ah.i0 + kh)) * W + (aw.i0 + kw) : 0;
    }
    if (img_out) {
      for (int c = 0; c < C; c++) {
        const float* src = img + (int64_t)c * V;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 8; k++)
          if (in[k]) acc += wt[k] * (double)src[off[k]];
        img_out[(int64_t)c * V + i] = (float)acc;   // the one rounding
      }
    }
    if (lab_out || oh_out) {
      int l[8];
#pragma unroll
      for (int k = 0; k < 8; k++) l[k] = in[k] ? (int)lab[off[k]] : 0;
      // temp_z = warp(label == z); new_label[temp_z >= 0.5] = z for z ascending: the LAST class reaching 0.5 wins, `>=`
      // is inclusive, and a label >= n_cls matches no z (background), transformer_3d.py:113-116
      int res = 0;
#pragma unroll
      for (int zc = 1; zc < AUG_MAXCLS; zc++)
        if (zc < n_cls) {
          double acc = 0.0;
#pragma unroll
          for (int k = 0; k < 8; k++) acc += (l[k] == zc) ? wt[k] : 0.0;
          if (acc >= 0.5) res = zc;
        }
      if (lab_out) lab_out[i] = (uint8_t)res;
      if (oh_out) {
        // To_Tensor: channel 0 is "no other class"
        oh_out[i] = res == 0 ? 1.f : 0.f;
        for (int zc = 1; zc < n_cls; zc++) oh_out[(int64_t)zc * V + i] = res == zc ? 1.f : 0.f;
      }
    }
  }
}

bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b) return false;
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}
}  // namespace

int hdf_launch_augment3d(const float* image, const uint8_t* labels, int C, int n_cls, int D, int H, int W,
                         const AugAffine& aff, int flip_h, int flip_w, float* image_out, uint8_t* labels_out,
                         float* onehot_out, hipStream_t st) {
  HDF_CHECK_ARG(D >= 1 && H >= 1 && W >= 1, "augment_3d: volume %dx%dx%d", D, H, W);
  HDF_CHECK_ARG(n_cls >= 2 && n_cls <= AUG_MAXCLS, "augment_3d: n_cls=%d (2..%d)", n_cls, AUG_MAXCLS);
  HDF_CHECK_ARG(image_out || labels_out || onehot_out, "augment_3d: no output asked for");
  HDF_CHECK_ARG(!image_out || (image && C >= 1 && C <= AUG_MAXCH),
                "augment_3d: an image output needs an image of 1..%d channels (channels=%d)", AUG_MAXCH, C);
  HDF_CHECK_ARG(labels || (!labels_out && !onehot_out), "augment_3d: a label output without labels");
  for (int k = 0; k < 12; k++) HDF_CHECK_ARG(std::isfinite(aff.m[k]), "augment_3d: affine[%d] is not finite", k);
  const size_t V = (size_t)D * H * W;
  const size_t in_b[2] = {image_out ? (size_t)C * V * 4 : 0, V};
  const void* ins[2] = {image_out ? image : nullptr, (labels_out || onehot_out) ? labels : nullptr};
  const size_t out_b[3] = {(size_t)C * V * 4, V, (size_t)n_cls * V * 4};
  const void* outs[3] = {image_out, labels_out, onehot_out};
  for (int a = 0; a < 2; a++)
    for (int b = 0; b < 3; b++)
      HDF_CHECK_ARG(!overlaps(ins[a], in_b[a], outs[b], out_b[b]),
                    "augment_3d: an output overlaps a source (the gather reads voxels other threads have written)");
  const unsigned gx = (unsigned)std::min<int64_t>(ceil_div64((int64_t)V, 256), 2048);
  hipLaunchKernelGGL(augment3d_kernel, dim3(gx), dim3(256), 0, st, image_out ? image : nullptr, labels, C, n_cls, D, H, W,
                     aff, flip_h != 0, flip_w != 0, image_out, labels_out, onehot_out);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
