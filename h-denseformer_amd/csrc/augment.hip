// The device-side input pipeline: the in-place input normalisation of one sample (hdf_launch_normalize,
// data_utils/data_loader.py:39-68), the one-hot staging of a batch of class maps (hdf_launch_onehot), and the reference's
// 3-D training augmentation, one launch per sample (hdf_launch_augment3d): RandomTranslationRotationZoom3D
// (data_utils/transformer_3d.py:45-120), RandomFlip3D (:123-169) and the To_Tensor one-hot (data_utils/data_loader.py:
// 126-159), and the default 2-D one, one launch per 32 samples (hdf_launch_augment2d, further down): RandomRotate2D +
// RandomFlip2D + To_Tensor (data_utils/transformer_2d.py:80-173), and the rest of the 2-D list: the label bounding box
// (hdf_launch_label_bbox2d), RandomErase2D + RandomZoom2D (hdf_launch_zoom2d) and RandomAdjust2D + RandomNoise2D
// (hdf_launch_intensity2d).  The 3-D augmentation is a memory-bound gather: every output voxel reads the eight corners of its source coordinate, per image channel
// and once for the labels.  The reference's angles are +-5 degrees, so a wave's 64 source addresses stay within a few rows
// of one plane: the corners come from L2, nothing is staged through LDS.
//
// All arithmetic between the loads and the one rounding of the store is fp64 (about 60 operations per voxel against about
// 50 bytes of traffic): the reference interpolates in fp64 (scipy.ndimage.map_coordinates, order 1), so the image matches
// it to one fp32 rounding and the labels' 0.5 threshold does not move.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "augment.h"
#include "loss.h"

namespace {
constexpr int AUG_MAXCLS = HDF_CLASS_SLOTS;   // the class slots of the staging and inference kernels
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

// ---------------------------------------------------------------------------------- 2-D training augmentation
// RandomRotate2D + RandomFlip2D + To_Tensor (data_utils/transformer_2d.py:80-173) for a chunk of up to AUG2D_CHUNK
// samples in one launch, bit for bit what PIL computes (include/hdf.h, hdf_augment_2d): the image through PIL's
// affine_transform + bilinear_filter32F in fp64 with ONE fp32 subtraction per row, the labels through its 16.16
// fixed-point affine_fixed.  Each thread works out the stencil of one output pixel once -- two rows, two clamped columns,
// dx, dy, the label index -- and then walks the channels.  A memory-bound gather like the 3-D kernel: at +-15 degrees a
// wave's 64 sources span a handful of rows of one plane, which L2 serves; nothing is staged through LDS.
// The per-sample parameters travel BY VALUE in the kernel arguments (104 bytes a sample, 32 samples under the 4 KB
// limit): the host arrays are read during the call and no staging buffer has a lifetime to manage.
__global__ void __launch_bounds__(256)
augment2d_kernel(const float* __restrict__ img, const uint8_t* __restrict__ lab, int nb, int C, int n_cls, int H, int W,
                 Aug2DChunk prm, float* __restrict__ img_out, uint8_t* __restrict__ lab_out,
                 float* __restrict__ oh_out) {
  const int64_t P = (int64_t)H * W, total = (int64_t)nb * P;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    // a fused multiply-add anywhere below changes bits: PIL's build rounds every product
#pragma clang fp contract(off)
    const int b = (int)(i / P);
    const int64_t r = i - (int64_t)b * P;
    const int y = (int)(r / W), x = (int)(r - (int64_t)y * W);
    const Aug2DSample& s = prm.s[b];
    // the flip follows the rotation: out[y][x] = rotated[y][W-1-x] (1) or rotated[H-1-y][x] (2)
    const int px = s.flip == 1 ? W - 1 - x : x, py = s.flip == 2 ? H - 1 - y : y;
    if (img_out) {
      const double xc = px + 0.5, yc = py + 0.5;
      double xin = s.m[0] * xc + s.m[1] * yc + s.m[2];
      double yin = s.m[3] * xc + s.m[4] * yc + s.m[5];
      const bool inside = !(xin < 0.0 || xin >= (double)W || yin < 0.0 || yin >= (double)H);
      // inside: xin - 0.5 lies in [-0.5, W - 0.5), its floor in [-1, W - 1]; outside nothing is loaded
      xin -= 0.5, yin -= 0.5;
      const double fx = floor(xin), fy = floor(yin);
      const double dx = xin - fx, dy = yin - fy;
      const int x0 = inside ? (int)fx : 0, y0 = inside ? (int)fy : 0;
      const int xa = min(max(x0, 0), W - 1), xb = min(max(x0 + 1, 0), W - 1);
      const int64_t row1 = (int64_t)min(max(y0, 0), H - 1) * W;
      const bool below = y0 + 1 >= 0 && y0 + 1 < H;
      const int64_t row2 = below ? (int64_t)(y0 + 1) * W : row1;
      for (int c = 0; c < C; c++) {
        const int64_t plane = ((int64_t)b * C + c) * P;
        float res = 0.f;
        if (inside) {
          const float* src = img + plane;
          const float p0 = src[row1 + xa], p1 = src[row1 + xb];
          const double v1 = (double)p0 + (double)(p1 - p0) * dx;   // the neighbour difference is an fp32 subtraction
          double v2 = v1;
          if (below) {
            const float q0 = src[row2 + xa], q1 = src[row2 + xb];
            v2 = (double)q0 + (double)(q1 - q0) * dx;
          }
          res = (float)(v1 + (v2 - v1) * dy);
        }
        img_out[plane + r] = res;
      }
    }
    if (lab_out || oh_out) {
      // closed form of PIL's running sums: exact integers, arithmetic shift
      const int64_t xi = (s.fx[2] + py * s.fx[1] + px * s.fx[0]) >> 16;
      const int64_t yi = (s.fx[5] + py * s.fx[4] + px * s.fx[3]) >> 16;
      const bool in_l = xi >= 0 && xi < W && yi >= 0 && yi < H;
      const int l = in_l ? (int)lab[(int64_t)b * P + yi * W + xi] : 0;
      if (lab_out) lab_out[i] = (uint8_t)l;   // the raw byte moves unchanged
      if (oh_out) {
        // To_Tensor: channel 0 is "no other class", a value >= n_cls is background
        float* o = oh_out + (int64_t)b * n_cls * P + r;
        o[0] = (l >= 1 && l < n_cls) ? 0.f : 1.f;
        for (int zc = 1; zc < n_cls; zc++) o[(int64_t)zc * P] = l == zc ? 1.f : 0.f;
      }
    }
  }
}

// ---------------------------------------------------------------------------------- 2-D label bounding box
// (non-zero count, rmin, rmax, cmin, cmax) of each class map, what RandomErase2D and RandomZoom2D branch on: blocks of a
// sample reduce their share to one partial in the caller's workspace, one wave per sample folds the partials.  Integer
// minima, maxima and sums: the result does not depend on the order.
constexpr int BBOX_BLOCKS = 64;   // partials per sample; one wave of bbox_finalize_kernel folds them
struct BBox {
  int n, rmin, rmax, cmin, cmax;
};
__device__ __forceinline__ BBox bbox_merge(BBox a, const BBox& b) {
  a.n += b.n;
  a.rmin = min(a.rmin, b.rmin), a.rmax = max(a.rmax, b.rmax);
  a.cmin = min(a.cmin, b.cmin), a.cmax = max(a.cmax, b.cmax);
  return a;
}
__device__ __forceinline__ BBox bbox_wave(BBox v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    BBox u;
    u.n = __shfl_xor(v.n, o, 64);
    u.rmin = __shfl_xor(v.rmin, o, 64), u.rmax = __shfl_xor(v.rmax, o, 64);
    u.cmin = __shfl_xor(v.cmin, o, 64), u.cmax = __shfl_xor(v.cmax, o, 64);
    v = bbox_merge(v, u);
  }
  return v;
}
__global__ void __launch_bounds__(256)
bbox_partial_kernel(const uint8_t* __restrict__ lab, int H, int W, BBox* __restrict__ part /*[B][gridDim.x]*/) {
  __shared__ BBox red[4];
  const int P = H * W;   // at most 2^28
  const uint8_t* p = lab + (int64_t)blockIdx.y * P;
  BBox v = {0, H, -1, W, -1};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < P; i += gridDim.x * 256)
    if (p[i]) {
      const int y = i / W, x = i - y * W;
      v = bbox_merge(v, BBox{1, y, y, x, x});
    }
  v = bbox_wave(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = bbox_merge(bbox_merge(red[0], red[1]), bbox_merge(red[2], red[3]));
}
__global__ void __launch_bounds__(64)
bbox_finalize_kernel(const BBox* __restrict__ part, int blocks, int H, int W, int32_t* __restrict__ out /*[B][5]*/) {
  BBox v = {0, H, -1, W, -1};
  if ((int)threadIdx.x < blocks) v = part[(int64_t)blockIdx.x * blocks + threadIdx.x];   // blocks <= BBOX_BLOCKS = 64
  v = bbox_wave(v);
  if (threadIdx.x == 0) {
    int32_t* o = out + (int64_t)blockIdx.x * 5;
    o[0] = v.n, o[1] = v.rmin, o[2] = v.rmax, o[3] = v.cmin, o[4] = v.cmax;
  }
}

// ---------------------------------------------------------------------------------- 2-D erase + zoom
// RandomErase2D + RandomZoom2D (data_utils/transformer_2d.py:11-77, 177-275) for a chunk of up to AUG2D_CHUNK samples in
// one launch, bit for bit what PIL computes (include/hdf.h, hdf_zoom_2d): crop / ImageOps.expand as a canvas around the
// plane, then resize(BILINEAR) of the mode-F planes through ImagingResample's two separable passes and resize(NEAREST)
// of the mode-L class map through ImagingScaleAffine.  A gather: each thread owns one output pixel, works out the taps of
// both axes once and walks the channels; the horizontal results a vertical tap needs are recomputed (at most 3 x 3 taps
// within the reference's factors 0.8 .. 1.2, at most 9 x 9 at the limits), not stored as an intermediate plane -- the
// bits are the same.  The coefficients are built here, in fp64 with every operation rounded: k = w / sum(w) is an IEEE
// division, as in PIL.
struct ZoomAxis {
  int lo, n;   // the taps are the canvas indices lo .. lo + n - 1
  double center, ss, ww;
};
// the weight of tap t before the normalisation: bilinear_filter((t + lo - center + 0.5) * ss)
__device__ __forceinline__ double zoom_w(const ZoomAxis& a, int t) {
#pragma clang fp contract(off)
  const double v = fabs(((double)(t + a.lo) - a.center + 0.5) * a.ss);
  return v < 1.0 ? 1.0 - v : 0.0;
}
__device__ __forceinline__ double zoom_k(const ZoomAxis& a, int t) {
  const double w = zoom_w(a, t);
  return a.ww != 0.0 ? w / a.ww : w;
}
// precompute_coeffs of PIL's Resample.c for output index xx of an axis resized from n_in to n_out
__device__ __forceinline__ ZoomAxis zoom_axis(int n_in, int n_out, int xx) {
#pragma clang fp contract(off)
  const double scale = (double)n_in / (double)n_out;
  const double fs = scale < 1.0 ? 1.0 : scale;   // the support of the bilinear filter is 1 * fs
  ZoomAxis a;
  a.ss = 1.0 / fs;
  a.center = ((double)xx + 0.5) * scale;
  const int lo = max((int)(a.center - fs + 0.5), 0);
  const int hi = min((int)(a.center + fs + 0.5), n_in);
  a.lo = lo, a.n = hi - lo, a.ww = 0.0;
  for (int t = 0; t < a.n; t++) a.ww += zoom_w(a, t);
  return a;
}
// canvas pixel (cy, cx) of one image plane: the source pixel (cy - oy, cx - ox) inside the keep-rectangle (which lies
// inside the plane), else 0
__device__ __forceinline__ float zoom_src(const float* __restrict__ plane, int W, const Zoom2DSample& s, int cy, int cx) {
  const int sy = cy - s.oy, sx = cx - s.ox;
  return (sy >= s.r0 && sy < s.r1 && sx >= s.c0 && sx < s.c1) ? plane[(int64_t)sy * W + sx] : 0.f;
}
// the horizontal pass at output column x of canvas row cy, rounded to fp32; skipped (the pixel itself) when sw == W
__device__ __forceinline__ float zoom_hpass(const float* __restrict__ plane, int W, const Zoom2DSample& s,
                                            const ZoomAxis& ax, int cy, int x) {
#pragma clang fp contract(off)
  if (s.sw == W) return zoom_src(plane, W, s, cy, x);
  double ss = 0.0;
  for (int t = 0; t < ax.n; t++) ss += (double)zoom_src(plane, W, s, cy, ax.lo + t) * zoom_k(ax, t);
  return (float)ss;
}

__global__ void __launch_bounds__(256)
zoom2d_kernel(const float* __restrict__ img, const uint8_t* __restrict__ lab, int C, int H, int W, Zoom2DChunk prm,
              float* __restrict__ img_out, uint8_t* __restrict__ lab_out) {
  extern __shared__ uint16_t zoom_tab[];   // [W] source columns, [H] source rows of the nearest resize (labels only)
  const int b = blockIdx.y;
  const Zoom2DSample& s = prm.s[b];
  const int P = H * W;   // at most 2^28
  if (lab_out) {
    // ImagingScaleAffine keeps a RUNNING sum, xo += a0 per output index, whose roundings no closed form reproduces: one
    // thread per axis walks it (two waves, side by side).  An index stays below n_in <= 4 * 16384 = 2^16.
    if (threadIdx.x == 0 || threadIdx.x == 64) {
#pragma clang fp contract(off)
      const bool cols = threadIdx.x == 0;
      const int n_out = cols ? W : H;
      uint16_t* tab = cols ? zoom_tab : zoom_tab + W;
      const double a0 = (double)(cols ? s.sw : s.sh) / (double)n_out;
      double xo = a0 * 0.5;
      for (int k = 0; k < n_out; k++) {
        tab[k] = (uint16_t)(int)xo;
        xo += a0;
      }
    }
    __syncthreads();
  }
  for (int i = blockIdx.x * 256 + threadIdx.x; i < P; i += gridDim.x * 256) {
    const int y = i / W, x = i - y * W;
    if (img_out) {
#pragma clang fp contract(off)
      const ZoomAxis ax = zoom_axis(s.sw, W, x), ay = zoom_axis(s.sh, H, y);
      for (int c = 0; c < C; c++) {
        const int64_t plane = ((int64_t)b * C + c) * P;
        const float* src = img + plane;
        float res;
        if (s.sh == H) {
          res = zoom_hpass(src, W, s, ax, y, x);   // the vertical pass is skipped
        } else {
          double ss = 0.0;
          for (int t = 0; t < ay.n; t++) ss += (double)zoom_hpass(src, W, s, ax, ay.lo + t, x) * zoom_k(ay, t);
          res = (float)ss;
        }
        img_out[plane + i] = res;
      }
    }
    if (lab_out) {
      const int cx = zoom_tab[x], cy = zoom_tab[W + y];
      const int sx = cx - s.ox, sy = cy - s.oy;
      const bool in_l = cx < s.sw && cy < s.sh && sx >= 0 && sx < W && sy >= 0 && sy < H;
      lab_out[(int64_t)b * P + i] = in_l ? lab[(int64_t)b * P + (int64_t)sy * W + sx] : (uint8_t)0;
    }
  }
}

// ---------------------------------------------------------------------------------- 2-D gamma + Gaussian noise
// RandomAdjust2D + RandomNoise2D (data_utils/transformer_2d.py:279-322) in place, one launch per AUG2D_CHUNK samples.
// Philox-4x32-10 (Salmon et al., SC'11) on the counter (element index low, high, sample, 0) under the key (seed low,
// high): the normal of an element is a pure function of (seed, sample, index), whatever the launch geometry.
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
  c[1] = (uint32_t)p1, c[3] = (uint32_t)p0, c[0] = n0, c[2] = n2;
}
__device__ __forceinline__ double philox_normal(uint64_t seed, uint32_t sample, uint64_t index) {
  uint32_t c[4] = {(uint32_t)index, (uint32_t)(index >> 32), sample, 0u};
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; r++) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  // Box-Muller in fp64: u1 in (0, 1) from 52 bits, u2 from 32
  const double u1 = ((double)(((uint64_t)c[0] << 20) | (c[1] >> 12)) + 0.5) * 0x1p-52;
  const double u2 = ((double)c[2] + 0.5) * 0x1p-32;
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}
__global__ void __launch_bounds__(256)
intensity2d_kernel(float* __restrict__ img, int64_t n, Intensity2DChunk prm, uint64_t seed, int b0, float low_clip) {
  const int b = blockIdx.y;
  const double g = prm.gamma[b];
  const bool noisy = prm.noise[b] != 0;
  if (g == 1.0 && !noisy) return;   // the sample is left alone, bits and all
  float* p = img + (int64_t)b * n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float x = p[i];
    // skimage's adjust_gamma on a float image, (x / 1) ** gamma * 1; MRNormalize leaves no negative, 0 stays 0
    if (g != 1.0) x = x > 0.f ? (float)pow((double)x, g) : 0.f;
    // skimage's random_noise(mode='gaussian'): mean 0, var 0.01, clipped to [low_clip, 1]
    if (noisy)
      x = (float)fmin(fmax((double)x + 0.1 * philox_normal(seed, (uint32_t)(b0 + b), (uint64_t)i), (double)low_clip), 1.0);
    p[i] = x;
  }
}

// ---------------------------------------------------------------------------------- input normalisation
// data_utils/data_loader.py:39-68.  Per-channel reductions over the volume in a fixed order (block partials in
// fp64, then one block), then one elementwise pass.  stats[c] = (max, sum, sum of squares, unused).
constexpr int NORM_BLOCKS = 512;
__global__ __launch_bounds__(256) void norm_reduce_kernel(const float* __restrict__ img, int64_t V,
                                                          double* __restrict__ part /*[C][NORM_BLOCKS][3]*/) {
  __shared__ double red[4][3];
  const int c = blockIdx.y;
  const float* p = img + (int64_t)c * V;
  double mx = -INFINITY, s = 0.0, ss = 0.0;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
    const double x = (double)p[v];
    mx = fmax(mx, x);
    s += x;
    ss += x * x;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mx = fmax(mx, __shfl_xor(mx, o, 64));
    s += __shfl_xor(s, o, 64);
    ss += __shfl_xor(ss, o, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave][0] = mx, red[wave][1] = s, red[wave][2] = ss;
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = part + ((int64_t)c * gridDim.x + blockIdx.x) * 3;
    o[0] = fmax(fmax(red[0][0], red[1][0]), fmax(red[2][0], red[3][0]));
    o[1] = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    o[2] = red[0][2] + red[1][2] + red[2][2] + red[3][2];
  }
}
__global__ void norm_finalize_kernel(const double* __restrict__ part, int blocks, int64_t V,
                                     double* __restrict__ stats /*[C][4]: max, mean, std (population), 0*/) {
  const int c = blockIdx.x;
  if (threadIdx.x == 0) {
    double mx = -INFINITY, s = 0.0, ss = 0.0;
    for (int b = 0; b < blocks; b++) {
      const double* q = part + ((int64_t)c * blocks + b) * 3;
      mx = fmax(mx, q[0]);
      s += q[1];
      ss += q[2];
    }
    const double mean = s / (double)V;
    stats[c * 4 + 0] = mx;
    stats[c * 4 + 1] = mean;
    stats[c * 4 + 2] = sqrt(fmax(ss / (double)V - mean * mean, 0.0));
    stats[c * 4 + 3] = 0.0;
  }
}
// mode 0 (MRNormalize, data_loader.py:39-50): x / max(channel) when the max is non-zero, then negatives -> 0.
// mode 1 (PETandCTNormalize, :53-68): channel 0 -> (clip(x, mean-w, mean+w) - mean) / w ; channel 1 -> (x - mean_1)
//         / (std_1 + 1e-3) ; further channels untouched.
__global__ void norm_apply_kernel(float* __restrict__ img, int64_t V, const double* __restrict__ stats, int mode,
                                  float pmean, float pw) {
  const int c = blockIdx.y;
  float* p = img + (int64_t)c * V;
  const float mx = (float)stats[c * 4 + 0], mean = (float)stats[c * 4 + 1], sd = (float)stats[c * 4 + 2];
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) {
    float x = p[v];
    if (mode == 0) {
      if (mx != 0.f) x = x / mx;
      x = x < 0.f ? 0.f : x;
    } else if (c == 0) {
      x = (fminf(fmaxf(x, pmean - pw), pmean + pw) - pmean) / pw;
    } else if (c == 1) {
      x = (x - mean) / (sd + 1e-3f);
    }
    p[v] = x;
  }
}

__global__ void onehot_kernel(const uint8_t* __restrict__ lab, float* __restrict__ oh, int C, int64_t V) {
  const int n = blockIdx.y;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (int64_t)gridDim.x * blockDim.x) {
    const int l = lab[(int64_t)n * V + i];
    float* o = oh + (int64_t)n * C * V + i;
    const bool fg = l >= 1 && l < C;
    o[0] = fg ? 0.f : 1.f;
    for (int c = 1; c < C; c++) o[(int64_t)c * V] = (l == c) ? 1.f : 0.f;
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

// FIX of PIL's affine_fixed: 16.16, round half up
static int64_t fix16(double v) {
#pragma clang fp contract(off)
  return (int64_t)std::floor(v * 65536.0 + 0.5);
}

int hdf_launch_augment2d(const float* image, const uint8_t* labels, int B, int C, int n_cls, int H, int W,
                         const double* matrices, const uint8_t* flips, float* image_out, uint8_t* labels_out,
                         float* onehot_out, hipStream_t st) {
  HDF_CHECK_ARG(B >= 1, "augment_2d: batch=%d", B);
  HDF_CHECK_ARG(H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "augment_2d: plane %dx%d (1..16384 a side)", H, W);
  HDF_CHECK_ARG(n_cls >= 2 && n_cls <= AUG_MAXCLS, "augment_2d: n_cls=%d (2..%d)", n_cls, AUG_MAXCLS);
  HDF_CHECK_ARG(image_out || labels_out || onehot_out, "augment_2d: no output asked for");
  HDF_CHECK_ARG(!image_out || (image && C >= 1 && C <= AUG_MAXCH),
                "augment_2d: an image output needs an image of 1..%d channels (channels=%d)", AUG_MAXCH, C);
  HDF_CHECK_ARG(labels || (!labels_out && !onehot_out), "augment_2d: a label output without labels");
  HDF_CHECK_ARG(matrices && flips, "augment_2d: null %s", matrices ? "flips" : "matrices");
  for (int b = 0; b < B; b++) {
#pragma clang fp contract(off)
    const double* m = matrices + 6 * (size_t)b;
    for (int k = 0; k < 6; k++)
      HDF_CHECK_ARG(std::isfinite(m[k]), "augment_2d: matrices[%d][%d] is not finite", b, k);
    // PIL's check_fixed at the four corners: past it PIL leaves the 16.16 path, so the label contract would not hold
    const int cx[4] = {0, W, 0, W}, cy[4] = {0, 0, H, H};
    for (int k = 0; k < 4; k++)
      HDF_CHECK_ARG(std::fabs(cx[k] * m[0] + cy[k] * m[1] + m[2]) < 32768.0 &&
                        std::fabs(cx[k] * m[3] + cy[k] * m[4] + m[5]) < 32768.0,
                    "augment_2d: matrices[%d] maps corner (%d, %d) beyond +-32768 (the range of PIL's fixed-point path)",
                    b, cx[k], cy[k]);
    HDF_CHECK_ARG(flips[b] <= 2, "augment_2d: flips[%d]=%d (0 none, 1 W, 2 H)", b, (int)flips[b]);
  }
  const size_t P = (size_t)H * W;
  const size_t in_b[2] = {image_out ? (size_t)B * C * P * 4 : 0, (size_t)B * P};
  const void* ins[2] = {image_out ? image : nullptr, (labels_out || onehot_out) ? labels : nullptr};
  const size_t out_b[3] = {(size_t)B * C * P * 4, (size_t)B * P, (size_t)B * n_cls * P * 4};
  const void* outs[3] = {image_out, labels_out, onehot_out};
  for (int a = 0; a < 2; a++)
    for (int o = 0; o < 3; o++)
      HDF_CHECK_ARG(!overlaps(ins[a], in_b[a], outs[o], out_b[o]),
                    "augment_2d: an output overlaps a source (the gather reads pixels other threads have written)");
  if (!image_out) image = nullptr, C = 0;
  for (int b0 = 0; b0 < B; b0 += AUG2D_CHUNK) {
    const int nb = std::min(AUG2D_CHUNK, B - b0);
    Aug2DChunk prm;
    for (int k = 0; k < AUG2D_CHUNK; k++) {
#pragma clang fp contract(off)
      Aug2DSample& s = prm.s[k];
      const double* m = matrices + 6 * (size_t)(b0 + std::min(k, nb - 1));   // the unused tail repeats the last sample
      for (int j = 0; j < 6; j++) s.m[j] = m[j];
      s.fx[0] = fix16(m[0]), s.fx[1] = fix16(m[1]), s.fx[2] = fix16(m[2] + m[0] * 0.5 + m[1] * 0.5);
      s.fx[3] = fix16(m[3]), s.fx[4] = fix16(m[4]), s.fx[5] = fix16(m[5] + m[3] * 0.5 + m[4] * 0.5);
      s.flip = flips[b0 + std::min(k, nb - 1)];
      s.pad = 0;
    }
    const size_t o = (size_t)b0 * P;
    const unsigned gx = (unsigned)std::min<int64_t>(ceil_div64((int64_t)nb * (int64_t)P, 256), 2048);
    hipLaunchKernelGGL(augment2d_kernel, dim3(gx), dim3(256), 0, st, image ? image + o * C : nullptr,
                       labels ? labels + o : nullptr, nb, C, n_cls, H, W, prm, image_out ? image_out + o * C : nullptr,
                       labels_out ? labels_out + o : nullptr, onehot_out ? onehot_out + o * n_cls : nullptr);
    HDF_LAUNCH_CHECK();
  }
  return HDF_OK;
}

size_t hdf_label_bbox_ws_bytes(int B) { return (size_t)std::max(B, 0) * BBOX_BLOCKS * sizeof(BBox); }
int hdf_launch_label_bbox2d(const uint8_t* labels, int B, int H, int W, int32_t* bbox, void* ws, hipStream_t st) {
  HDF_CHECK_ARG(B >= 1 && B <= 65535, "label_bbox_2d: batch=%d (1..65535)", B);
  HDF_CHECK_ARG(H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "label_bbox_2d: plane %dx%d (1..16384 a side)", H, W);
  HDF_CHECK_ARG(labels && bbox && ws, "label_bbox_2d: null argument");
  const int blocks = (int)std::min<int64_t>(ceil_div64((int64_t)H * W, 256 * 8), BBOX_BLOCKS);
  hipLaunchKernelGGL(bbox_partial_kernel, dim3(blocks, B), dim3(256), 0, st, labels, H, W, (BBox*)ws);
  HDF_LAUNCH_CHECK();
  hipLaunchKernelGGL(bbox_finalize_kernel, dim3(B), dim3(64), 0, st, (const BBox*)ws, blocks, H, W, bbox);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_zoom2d(const float* image, const uint8_t* labels, int B, int C, int H, int W, const int32_t* keep,
                      const int32_t* canvas, float* image_out, uint8_t* labels_out, hipStream_t st) {
  HDF_CHECK_ARG(B >= 1, "zoom_2d: batch=%d", B);
  HDF_CHECK_ARG(H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "zoom_2d: plane %dx%d (1..16384 a side)", H, W);
  HDF_CHECK_ARG(image_out || labels_out, "zoom_2d: no output asked for");
  HDF_CHECK_ARG(!image_out || (image && C >= 1 && C <= AUG_MAXCH),
                "zoom_2d: an image output needs an image of 1..%d channels (channels=%d)", AUG_MAXCH, C);
  HDF_CHECK_ARG(!labels_out || labels, "zoom_2d: a label output without labels");
  HDF_CHECK_ARG(keep && canvas, "zoom_2d: null %s", keep ? "canvas" : "keep");
  for (int b = 0; b < B; b++) {
    const int32_t* k = keep + 4 * (size_t)b;
    const int32_t* v = canvas + 4 * (size_t)b;
    HDF_CHECK_ARG(0 <= k[0] && k[0] <= k[1] && k[1] <= H && 0 <= k[2] && k[2] <= k[3] && k[3] <= W,
                  "zoom_2d: keep[%d] = rows [%d, %d) x columns [%d, %d) leaves the %dx%d plane", b, k[0], k[1], k[2],
                  k[3], H, W);
    // the tap count and the 16-bit label index of the kernel rest on these bounds
    HDF_CHECK_ARG(v[0] >= ceil_div(W, 4) && v[0] <= 4 * W, "zoom_2d: canvas[%d] is %d wide (%d..%d for W=%d)", b, v[0],
                  ceil_div(W, 4), 4 * W, W);
    HDF_CHECK_ARG(v[1] >= ceil_div(H, 4) && v[1] <= 4 * H, "zoom_2d: canvas[%d] is %d high (%d..%d for H=%d)", b, v[1],
                  ceil_div(H, 4), 4 * H, H);
    HDF_CHECK_ARG(std::abs((int64_t)v[2]) <= 4 * 16384 && std::abs((int64_t)v[3]) <= 4 * 16384,
                  "zoom_2d: canvas[%d] places the plane at (%d, %d) (within +-65536)", b, v[3], v[2]);
  }
  const size_t P = (size_t)H * W;
  const size_t in_b[2] = {image_out ? (size_t)B * C * P * 4 : 0, (size_t)B * P};
  const void* ins[2] = {image_out ? image : nullptr, labels_out ? labels : nullptr};
  const size_t out_b[2] = {(size_t)B * C * P * 4, (size_t)B * P};
  const void* outs[2] = {image_out, labels_out};
  for (int a = 0; a < 2; a++)
    for (int o = 0; o < 2; o++)
      HDF_CHECK_ARG(!overlaps(ins[a], in_b[a], outs[o], out_b[o]),
                    "zoom_2d: an output overlaps a source (the gather reads pixels other threads have written)");
  HDF_CHECK_ARG(!overlaps(image_out, out_b[0], labels_out, out_b[1]), "zoom_2d: the two outputs overlap");
  if (!image_out) image = nullptr, C = 0;
  const size_t lds = labels_out ? (size_t)(W + H) * sizeof(uint16_t) : 0;   // at most 64 KB
  for (int b0 = 0; b0 < B; b0 += AUG2D_CHUNK) {
    const int nb = std::min(AUG2D_CHUNK, B - b0);
    Zoom2DChunk prm;
    for (int k = 0; k < AUG2D_CHUNK; k++) {
      const size_t q = 4 * (size_t)(b0 + std::min(k, nb - 1));   // the unused tail repeats the last sample
      prm.s[k] = Zoom2DSample{keep[q], keep[q + 1], keep[q + 2], keep[q + 3], canvas[q], canvas[q + 1], canvas[q + 2],
                              canvas[q + 3]};
    }
    const size_t o = (size_t)b0 * P;
    // few, long-lived blocks per sample: each walks the label index tables once before its pixels
    const unsigned gx = (unsigned)std::min<int64_t>(ceil_div64((int64_t)P, 256 * 16), 64);
    hipLaunchKernelGGL(zoom2d_kernel, dim3(gx, nb), dim3(256), lds, st, image ? image + o * C : nullptr,
                       labels_out ? labels + o : nullptr, C, H, W, prm, image_out ? image_out + o * C : nullptr,
                       labels_out ? labels_out + o : nullptr);
    HDF_LAUNCH_CHECK();
  }
  return HDF_OK;
}

int hdf_launch_intensity2d(float* image, int B, int64_t n, const double* gamma, const uint8_t* noise, uint64_t seed,
                           float low_clip, hipStream_t st) {
  HDF_CHECK_ARG(B >= 1, "intensity_2d: batch=%d", B);
  HDF_CHECK_ARG(n >= 1 && n <= (int64_t)AUG_MAXCH * 16384 * 16384, "intensity_2d: %lld elements a sample", (long long)n);
  HDF_CHECK_ARG(image && gamma && noise, "intensity_2d: null argument");
  HDF_CHECK_ARG(std::isfinite(low_clip) && low_clip <= 1.f, "intensity_2d: low_clip=%g (finite, at most 1)",
                (double)low_clip);
  for (int b = 0; b < B; b++) {
    HDF_CHECK_ARG(std::isfinite(gamma[b]) && gamma[b] >= 0.0, "intensity_2d: gamma[%d]=%g (finite, not negative)", b,
                  gamma[b]);
    HDF_CHECK_ARG(noise[b] <= 1, "intensity_2d: noise[%d]=%d (0 or 1)", b, (int)noise[b]);
  }
  for (int b0 = 0; b0 < B; b0 += AUG2D_CHUNK) {
    const int nb = std::min(AUG2D_CHUNK, B - b0);
    Intensity2DChunk prm;
    for (int k = 0; k < AUG2D_CHUNK; k++) {
      prm.gamma[k] = (double)(float)gamma[b0 + std::min(k, nb - 1)];   // pow runs on the fp32-rounded gamma
      prm.noise[k] = noise[b0 + std::min(k, nb - 1)];
    }
    const unsigned gx = (unsigned)std::min<int64_t>(ceil_div64(n, 256 * 4), 256);
    hipLaunchKernelGGL(intensity2d_kernel, dim3(gx, nb), dim3(256), 0, st, image + (size_t)b0 * n, n, prm, seed, b0,
                       low_clip);
    HDF_LAUNCH_CHECK();
  }
  return HDF_OK;
}

size_t hdf_norm_ws_bytes(int C) { return ((size_t)C * NORM_BLOCKS * 3 + (size_t)C * 4) * sizeof(double); }
int hdf_launch_normalize(float* img, int C, int64_t V, int mode, float pmean, float pw, void* ws, hipStream_t st) {
  HDF_CHECK_ARG(C >= 1 && C <= 64 && V >= 1, "normalize: channels=%d voxels=%lld", C, (long long)V);
  HDF_CHECK_ARG(mode == 0 || mode == 1, "normalize: mode %d", mode);
  HDF_CHECK_ARG(mode == 0 || (C >= 2 && pw != 0.f), "normalize: PET/CT mode needs >= 2 channels and w != 0");
  double* part = (double*)ws;
  double* stats = part + (size_t)C * NORM_BLOCKS * 3;
  hipLaunchKernelGGL(norm_reduce_kernel, dim3(NORM_BLOCKS, C), dim3(256), 0, st, img, V, part);
  HDF_LAUNCH_CHECK();
  hipLaunchKernelGGL(norm_finalize_kernel, dim3(C), dim3(64), 0, st, part, NORM_BLOCKS, V, stats);
  HDF_LAUNCH_CHECK();
  unsigned gx = (unsigned)std::min<int64_t>(ceil_div64(V, 256), 4096);
  hipLaunchKernelGGL(norm_apply_kernel, dim3(gx, C), dim3(256), 0, st, img, V, stats, mode, pmean, pw);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_onehot(const uint8_t* lab, float* oh, int N, int C, int64_t V, hipStream_t st) {
  HDF_CHECK_ARG(C >= 2 && C <= 255 && N >= 1, "onehot: n_cls=%d batch=%d", C, N);
  dim3 grid((unsigned)std::min<int64_t>(ceil_div64(V, 256), 4096), N);
  hipLaunchKernelGGL(onehot_kernel, grid, dim3(256), 0, st, lab, oh, C, V);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
