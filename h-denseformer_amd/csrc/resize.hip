// CropResize of the reference's 3-D transform list (data_utils/data_loader.py:71-123) and Trunc_and_Normalize (:16-36) on
// the device.  skimage.transform.resize(order=1) is scipy's gaussian_filter (anti-aliasing) followed by
// zoom(grid_mode=True); both are separable, so one axis is ONE banded operator Z.G -- the two interpolation taps applied to
// the filter rows -- and the volume goes through at most three gather passes.  Accumulation and the intermediates are
// fp64; the last pass rounds once (image) or thresholds `>= 0.5` (labels).  Semantics: include/hdf.h, hdf_resize_3d.
#include <algorithm>
#include <cmath>

#include "augment.h"

namespace {

// --------------------------------------------------------------------------------------------------- one axis
// what a pass reads and writes: the source (fp32 image plane, or the uint8 class map seen as the indicator of one
// class), an fp64 intermediate, or the result (fp32 rounded once, or the uint8 class map after the threshold)
template <typename T>
struct Src;
template <>
struct Src<float> {
  __device__ static __forceinline__ double ld(const float* p, int64_t i, int) { return (double)p[i]; }
};
template <>
struct Src<double> {
  __device__ static __forceinline__ double ld(const double* p, int64_t i, int) { return p[i]; }
};
template <>
struct Src<uint8_t> {
  __device__ static __forceinline__ double ld(const uint8_t* p, int64_t i, int cls) { return p[i] == cls ? 1.0 : 0.0; }
};
template <typename T>
struct Dst;
template <>
struct Dst<double> {
  __device__ static __forceinline__ void st(double* p, int64_t i, double v, int, bool) { p[i] = v; }
};
template <>
struct Dst<float> {
  __device__ static __forceinline__ void st(float* p, int64_t i, double v, int, bool) { p[i] = (float)v; }
};
template <>
struct Dst<uint8_t> {
  // classes come in ascending order, one launch each, on one stream: the first writes every voxel, a later one only
  // where it reaches 0.5, so the last class that does wins
  __device__ static __forceinline__ void st(uint8_t* p, int64_t i, double v, int cls, bool first) {
    const bool hit = v >= 0.5;
    if (first) p[i] = hit ? (uint8_t)cls : (uint8_t)0;
    else if (hit) p[i] = (uint8_t)cls;
  }
};

// index p of an axis of n samples under scipy's 'mirror' (reflection about the end samples, period 2n - 2, repeated as
// often as the radius needs), or -1 outside [0, n) under 'grid-constant' (the sample reads as 0)
__device__ __forceinline__ int boundary(int p, int n, bool constant) {
  if (constant) return (p >= 0 && p < n) ? p : -1;
  if (n == 1) return 0;
  const int period = 2 * n - 2;
  int q = (p < 0 ? -p : p) % period;
  return q >= n ? period - q : q;
}

// source coordinate of output index o, every operation rounded as on the host (a fused multiply-add would move an exact
// half-way coordinate, and with it a class sum that sits exactly on 0.5)
__device__ __forceinline__ double source_coord(int o, double f) {
#pragma clang fp contract(off)
  const double scaled = ((double)o + 0.5) * f;
  return scaled - 0.5;
}

// in [A][n_in][B] -> out [A][n_out][B] along the middle axis.  Output index o reads c = (o + 0.5) f - 0.5, i0 = floor(c),
// t = c - i0: out = (1 - t) F(i0) + t F(i0 + 1), F(j) = sum_k w[k] in(j + k) the Gaussian row at j (w = {1} when the axis
// is not filtered).  The two rows share their 2r + 2 loads.  The thread index runs over b fastest, so on the D and H
// passes (B >= W) a wavefront reads and writes consecutive W; on the W pass (B = 1) it covers consecutive outputs of a row,
// whose windows overlap.  Every pass output holds at most 1024^3 = 2^30 elements: the flat index fits 32 bits.
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void resize_pass_kernel(const TI* __restrict__ in, TO* __restrict__ out, uint32_t total,
                                                          int B, ResizeAxis ax, int cls, bool first) {
  const int n_in = ax.n_in, n_out = ax.n_out, r = ax.r;
  const bool constant = ax.constant != 0;
  for (uint32_t idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
    const uint32_t rest = idx / (uint32_t)B;
    const int b = (int)(idx - rest * (uint32_t)B);
    const uint32_t a = rest / (uint32_t)n_out;
    const int o = (int)(rest - a * (uint32_t)n_out);
    const double c = source_coord(o, ax.f);
    const double fl = floor(c);
    const int i0 = (int)fl;
    const double t = c - fl;
    const TI* base = in + ((int64_t)a * n_in) * B + b;
    double acc0 = 0.0, acc1 = 0.0;
    for (int m = 0; m <= 2 * r + 1; m++) {           // m is wave-uniform: the weights are scalar loads of the arguments
      const int q = boundary(i0 - r + m, n_in, constant);
      const double x = q >= 0 ? Src<TI>::ld(base, (int64_t)q * B, cls) : 0.0;
      if (m <= 2 * r) acc0 += ax.w[m] * x;
      if (m >= 1) acc1 += ax.w[m - 1] * x;
    }
    // 'grid-constant': an interpolation tap outside the axis reads 0, not the filter's value there
    const double a0 = (constant && (i0 < 0 || i0 >= n_in)) ? 0.0 : 1.0 - t;
    const double a1 = (t == 0.0 || (constant && (i0 + 1 < 0 || i0 + 1 >= n_in))) ? 0.0 : t;
    Dst<TO>::st(out, (int64_t)idx, a0 * acc0 + a1 * acc1, cls, first);
  }
}

template <typename TI, typename TO>
int launch_pass(const void* in, void* out, int64_t A, int B, const ResizeAxis& ax, int cls, bool first, hipStream_t st) {
  const int64_t total = A * ax.n_out * B;
  const unsigned gx = (unsigned)std::min<int64_t>(ceil_div64(total, 256), 2048);
  hipLaunchKernelGGL((resize_pass_kernel<TI, TO>), dim3(gx), dim3(256), 0, st, (const TI*)in, (TO*)out, (uint32_t)total, B,
                     ax, cls, first);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

// the per-axis operator of skimage's resize: f = n_in / n_out, sigma = max(0, (f - 1) / 2), radius int(4 sigma + 0.5),
// weights exp(-0.5 k^2 / sigma^2) normalised to sum 1 -- scipy's _gaussian_kernel1d, in fp64 on the host
ResizeAxis make_axis(int n_in, int n_out, bool constant) {
  ResizeAxis ax = {};
  ax.n_in = n_in, ax.n_out = n_out, ax.constant = constant ? 1 : 0;
  ax.f = (double)n_in / (double)n_out;
  const double sigma = std::max(0.0, (ax.f - 1.0) / 2.0);
  ax.r = sigma > 1e-15 ? (int)(4.0 * sigma + 0.5) : 0;
  if (ax.r == 0) {             // no filter (or one whose only tap is the centre: its normalised weight is 1)
    ax.w[0] = 1.0;
    return ax;
  }
  double sum = 0.0;
  for (int k = -ax.r; k <= ax.r; k++) sum += (ax.w[k + ax.r] = std::exp(-0.5 / (sigma * sigma) * (double)(k * k)));
  for (int k = 0; k <= 2 * ax.r; k++) ax.w[k] /= sum;
  return ax;
}

// The passes of one call.  Order: the axis with the smallest n_out / n_in first.  A pass costs (its output size) x (its
// taps) reads and the next pass reads what it wrote, so shrinking the volume early makes every later pass smaller and
// growing it last keeps the fp64 intermediates small; with equal ratios the outer axis goes first, which leaves the W
// pass -- the one whose lanes read overlapping windows instead of consecutive words -- the smallest input.  An axis that
// keeps its size is the identity operator and is skipped; if all three do, one W pass makes the copy.
struct ResizePlan {
  int n;              // passes, 1..3
  int axis[3];        // 0 D, 1 H, 2 W
  int64_t A[3];       // outer count of each pass
  int B[3];           // inner stride of each pass
  int64_t elems[2];   // fp64 elements of the intermediates after pass 0 and pass 1
};
ResizePlan make_plan(const int* ni, const int* no) {
  ResizePlan p = {};
  int order[3] = {0, 1, 2};
  std::stable_sort(order, order + 3, [&](int x, int y) { return (int64_t)no[x] * ni[y] < (int64_t)no[y] * ni[x]; });
  int cur[3] = {ni[0], ni[1], ni[2]};
  for (int k = 0; k < 3; k++) {
    const int a = order[k];
    if (ni[a] == no[a]) continue;
    p.axis[p.n] = a;
    p.A[p.n] = a == 0 ? 1 : a == 1 ? cur[0] : (int64_t)cur[0] * cur[1];
    p.B[p.n] = a == 0 ? cur[1] * cur[2] : a == 1 ? cur[2] : 1;
    cur[a] = no[a];
    if (p.n < 2) p.elems[p.n] = (int64_t)cur[0] * cur[1] * cur[2];
    p.n++;
  }
  if (p.n == 0) p.n = 1, p.axis[0] = 2, p.A[0] = (int64_t)ni[0] * ni[1], p.B[0] = 1;
  for (int k = p.n - 1; k < 2; k++) p.elems[k] = 0;      // the last pass writes the result, not the workspace
  return p;
}

bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b || !na || !nb) return false;
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}

int check_shapes(const int* ni, const int* no) {
  for (int a = 0; a < 3; a++) {
    HDF_CHECK_ARG(ni[a] >= 1 && ni[a] <= 1024 && no[a] >= 1 && no[a] <= 1024,
                  "resize_3d: %dx%dx%d -> %dx%dx%d (every dimension 1..1024)", ni[0], ni[1], ni[2], no[0], no[1], no[2]);
    HDF_CHECK_ARG(ni[a] <= 8 * no[a], "resize_3d: axis %d shrinks %d -> %d, a factor above 8 (the tap tables hold 30)", a,
                  ni[a], no[a]);
  }
  return HDF_OK;
}

__global__ void trunc_normalize_kernel(float* __restrict__ img, int64_t n, float lo, float range) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float x = img[i] - lo;
    x = x < 0.f ? 0.f : x;
    x = x > range ? range : x;
    img[i] = x / range;
  }
}
}  // namespace

int64_t hdf_resize_ws_bytes(int Di, int Hi, int Wi, int Do, int Ho, int Wo) {
  const int ni[3] = {Di, Hi, Wi}, no[3] = {Do, Ho, Wo};
  if (check_shapes(ni, no) != HDF_OK) return -1;
  const ResizePlan p = make_plan(ni, no);
  return (p.elems[0] + p.elems[1]) * (int64_t)sizeof(double);
}

int hdf_launch_resize3d(const float* image, const uint8_t* labels, int C, int n_cls, int Di, int Hi, int Wi, int Do, int Ho,
                        int Wo, float* image_out, uint8_t* labels_out, void* ws, int64_t ws_bytes, hipStream_t st) {
  const int ni[3] = {Di, Hi, Wi}, no[3] = {Do, Ho, Wo};
  HDF_TRY(check_shapes(ni, no));
  HDF_CHECK_ARG((image != nullptr) == (image_out != nullptr), "resize_3d: image and image_out come as a pair");
  HDF_CHECK_ARG((labels != nullptr) == (labels_out != nullptr), "resize_3d: labels and labels_out come as a pair");
  HDF_CHECK_ARG(image || labels, "resize_3d: no output asked for");
  HDF_CHECK_ARG(C >= 0 && C <= 64 && (!image || C >= 1), "resize_3d: channels=%d (0..64, at least 1 with an image)", C);
  HDF_CHECK_ARG(n_cls >= 2 && n_cls <= 8, "resize_3d: n_cls=%d (2..8)", n_cls);
  const ResizePlan p = make_plan(ni, no);
  const int64_t need = (p.elems[0] + p.elems[1]) * (int64_t)sizeof(double);
  HDF_CHECK_ARG(ws_bytes >= need && (ws || need == 0), "resize_3d: workspace of %lld bytes, %lld needed",
                (long long)(ws ? ws_bytes : 0), (long long)need);
  HDF_CHECK_ARG(need == 0 || (uintptr_t)ws % sizeof(double) == 0, "resize_3d: the workspace is not 8-byte aligned");
  const size_t Vi = (size_t)Di * Hi * Wi, Vo = (size_t)Do * Ho * Wo;
  const void* buf[5] = {image, labels, image_out, labels_out, need ? ws : nullptr};
  const size_t len[5] = {(size_t)C * Vi * 4, Vi, (size_t)C * Vo * 4, Vo, (size_t)need};
  for (int a = 0; a < 5; a++)
    for (int b = std::max(a + 1, 2); b < 5; b++)
      HDF_CHECK_ARG(!overlaps(buf[a], len[a], buf[b], len[b]),
                    "resize_3d: an output or the workspace overlaps another buffer (the gather reads voxels other threads "
                    "have written)");

  double* mid[2] = {(double*)ws, (double*)ws + p.elems[0]};
  // one plane (an image channel, or the indicator of one class) through the passes of the plan
  auto plane = [&](const void* src, bool is_label, void* dst, int cls, bool first) -> int {
    const void* in = src;
    for (int k = 0; k < p.n; k++) {
      const int a = p.axis[k];
      const ResizeAxis ax = make_axis(ni[a], no[a], is_label);
      const bool head = k == 0, tail = k == p.n - 1;
      void* out = tail ? dst : (void*)mid[k];
      if (head && tail)
        HDF_TRY(is_label ? (launch_pass<uint8_t, uint8_t>(in, out, p.A[k], p.B[k], ax, cls, first, st))
                         : (launch_pass<float, float>(in, out, p.A[k], p.B[k], ax, cls, first, st)));
      else if (head)
        HDF_TRY(is_label ? (launch_pass<uint8_t, double>(in, out, p.A[k], p.B[k], ax, cls, first, st))
                         : (launch_pass<float, double>(in, out, p.A[k], p.B[k], ax, cls, first, st)));
      else if (tail)
        HDF_TRY(is_label ? (launch_pass<double, uint8_t>(in, out, p.A[k], p.B[k], ax, cls, first, st))
                         : (launch_pass<double, float>(in, out, p.A[k], p.B[k], ax, cls, first, st)));
      else
        HDF_TRY((launch_pass<double, double>(in, out, p.A[k], p.B[k], ax, cls, first, st)));
      in = out;
    }
    return HDF_OK;
  };
  if (image)
    for (int c = 0; c < C; c++) HDF_TRY(plane(image + (size_t)c * Vi, false, image_out + (size_t)c * Vo, 0, false));
  if (labels)
    for (int z = 1; z < n_cls; z++) HDF_TRY(plane(labels, true, labels_out, z, z == 1));
  return HDF_OK;
}

int hdf_launch_trunc_normalize(float* image, int64_t n, float lo, float hi, hipStream_t st) {
  HDF_CHECK_ARG(image, "trunc_normalize: null image");
  HDF_CHECK_ARG(n >= 1, "trunc_normalize: n=%lld", (long long)n);
  HDF_CHECK_ARG(std::isfinite(lo) && std::isfinite(hi) && hi > lo && std::isfinite(hi - lo),
                "trunc_normalize: scale (%g, %g) must be finite with hi > lo", (double)lo, (double)hi);
  const unsigned gx = (unsigned)std::min<int64_t>(ceil_div64(n, 256), 2048);
  hipLaunchKernelGGL(trunc_normalize_kernel, dim3(gx), dim3(256), 0, st, image, n, lo, hi - lo);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
