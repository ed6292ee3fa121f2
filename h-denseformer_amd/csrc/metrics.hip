// The evaluation path: the on-device Dice metric (per-sample counts, the batch confusion matrix from logits or from two
// class maps) and the sliding-window inference tail (softmax accumulation per window, the vote).
//
// Reference: metric trainer.py:891-945, metrics.py:104-133.
#include "metrics.h"

namespace {
constexpr int MAXC = HDF_CLASS_SLOTS;   // fixes the [B, 8, 3] counts and the 8 x 8 confusion matrix of the ABI

// ---------------------------------------------------------------------------------- Dice metric
// counts[n][c][3] = (|P=c & T=c|, |P=c|, |T=c|) from hard argmax of logits / one-hot (trainer.py:919-945)
template <typename T>
__global__ __launch_bounds__(256) void dice_count_kernel(const T* __restrict__ logits, const float* __restrict__ target,
                                                         int C, int64_t V, unsigned long long* __restrict__ counts) {
  __shared__ unsigned int red[MAXC * 3];
  const int n = blockIdx.y;
  if (threadIdx.x < MAXC * 3) red[threadIdx.x] = 0;
  __syncthreads();
  unsigned int loc[MAXC * 3];
#pragma unroll
  for (int i = 0; i < MAXC * 3; i++) loc[i] = 0;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
    float bl = -INFINITY, bt = -INFINITY;
    int pc = 0, tc = 0;
#pragma unroll
    for (int c = 0; c < MAXC; c++)
      if (c < C) {
        float l = ST<T>::ld(logits + ((int64_t)n * C + c) * V + v);
        float t = target[((int64_t)n * C + c) * V + v];
        if (l > bl) bl = l, pc = c;
        if (t > bt) bt = t, tc = c;
      }
#pragma unroll
    for (int c = 0; c < MAXC; c++) {
      loc[c * 3 + 0] += (pc == c && tc == c);
      loc[c * 3 + 1] += (pc == c);
      loc[c * 3 + 2] += (tc == c);
    }
  }
#pragma unroll
  for (int i = 0; i < MAXC * 3; i++) atomicAdd(&red[i], loc[i]);
  __syncthreads();
  if (threadIdx.x < C * 3) atomicAdd(counts + (int64_t)n * MAXC * 3 + threadIdx.x, (unsigned long long)red[threadIdx.x]);
}

// confusion[t][p] += #voxels with target class t and predicted class p, summed over the batch (the matrix that
// metrics.RunningDice.update_matrix builds with sklearn on the CPU, metrics.py:104-133)
template <typename T>
__global__ __launch_bounds__(256) void confusion_kernel(const T* __restrict__ logits, const float* __restrict__ target,
                                                        int C, int64_t V, unsigned long long* __restrict__ conf) {
  __shared__ unsigned int red[MAXC * MAXC];
  const int n = blockIdx.y;
  if (threadIdx.x < MAXC * MAXC) red[threadIdx.x] = 0;
  __syncthreads();
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
    float bl = -INFINITY, bt = -INFINITY;
    int pc = 0, tc = 0;
#pragma unroll
    for (int c = 0; c < MAXC; c++)
      if (c < C) {
        float l = ST<T>::ld(logits + ((int64_t)n * C + c) * V + v);
        float t = target[((int64_t)n * C + c) * V + v];
        if (l > bl) bl = l, pc = c;
        if (t > bt) bt = t, tc = c;
      }
    atomicAdd(&red[tc * MAXC + pc], 1u);
  }
  __syncthreads();
  if (threadIdx.x < MAXC * MAXC && red[threadIdx.x])
    atomicAdd(conf + threadIdx.x, (unsigned long long)red[threadIdx.x]);
}

// the same from two uint8 class maps (the reference's call signature: RunningDice.update_matrix(ground_truth,
// prediction), metrics.py:104); labels >= C are not counted (sklearn's confusion_matrix(labels=...) drops them)
__global__ __launch_bounds__(256) void confusion_labels_kernel(const uint8_t* __restrict__ tgt,
                                                               const uint8_t* __restrict__ pred, int C, int64_t n,
                                                               unsigned long long* __restrict__ conf) {
  __shared__ unsigned int red[MAXC * MAXC];
  if (threadIdx.x < MAXC * MAXC) red[threadIdx.x] = 0;
  __syncthreads();
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
    const int tc = tgt[v], pc = pred[v];
    if (tc < C && pc < C) atomicAdd(&red[tc * MAXC + pc], 1u);
  }
  __syncthreads();
  if (threadIdx.x < MAXC * MAXC && red[threadIdx.x])
    atomicAdd(conf + threadIdx.x, (unsigned long long)red[threadIdx.x]);
}
}  // namespace

int hdf_launch_dice_counts(int dtype, const void* logits, const float* target, int N, int C, int64_t V,
                           unsigned long long* counts, hipStream_t st) {
  HDF_CHECK_ARG(C >= 1 && C <= MAXC && V >= 1 && N >= 1, "dice: n_cls=%d (1..%d) voxels=%lld batch=%d", C, MAXC, (long long)V,
                N);
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)N * MAXC * 3 * sizeof(unsigned long long), st);
  if (e != hipSuccess) {
    hdf_set_error("dice: memset failed: %s", hipGetErrorString(e));
    return HDF_ERR_HIP;
  }
  unsigned gx = (unsigned)std::min<int64_t>(ceil_div64(V, 256), 1024);
  HDF_DISPATCH_T(dtype, hipLaunchKernelGGL(dice_count_kernel<T>, dim3(gx, N), dim3(256), 0, st, (const T*)logits, target,
                                           C, V, counts));
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_confusion(int dtype, const void* logits, const float* target, int N, int C, int64_t V,
                         unsigned long long* conf, int accumulate, hipStream_t st) {
  HDF_CHECK_ARG(C >= 1 && C <= MAXC && V >= 1 && N >= 1, "confusion: n_cls=%d (1..%d) voxels=%lld batch=%d", C, MAXC,
                (long long)V, N);
  if (!accumulate) {
    hipError_t e = hipMemsetAsync(conf, 0, (size_t)MAXC * MAXC * sizeof(unsigned long long), st);
    if (e != hipSuccess) {
      hdf_set_error("confusion: memset failed: %s", hipGetErrorString(e));
      return HDF_ERR_HIP;
    }
  }
  unsigned gx = (unsigned)std::min<int64_t>(ceil_div64(V, 256), 1024);
  HDF_DISPATCH_T(dtype, hipLaunchKernelGGL(confusion_kernel<T>, dim3(gx, N), dim3(256), 0, st, (const T*)logits, target, C,
                                           V, conf));
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_confusion_labels(const uint8_t* tgt, const uint8_t* pred, int C, int64_t n, unsigned long long* conf,
                                int accumulate, hipStream_t st) {
  HDF_CHECK_ARG(C >= 1 && C <= MAXC, "confusion: n_cls=%d", C);
  if (!accumulate) {
    hipError_t e = hipMemsetAsync(conf, 0, (size_t)MAXC * MAXC * sizeof(unsigned long long), st);
    if (e != hipSuccess) {
      hdf_set_error("confusion: memset failed: %s", hipGetErrorString(e));
      return HDF_ERR_HIP;
    }
  }
  unsigned gx = (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div64(n, 256), 1), 1024);
  hipLaunchKernelGGL(confusion_labels_kernel, dim3(gx), dim3(256), 0, st, tgt, pred, C, n, conf);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

// ------------------------------------------------------------------------------ sliding-window inference tail
namespace {
constexpr int SW_MAXC = HDF_CLASS_SLOTS;
// one thread per window voxel: softmax over classes (fp32, max-subtracted like F.softmax) and accumulate
template <typename T>
__global__ void sw_accumulate_kernel(const T* __restrict__ logits, int C, int pd, int ph, int pw,
                                     float* __restrict__ psum, float* __restrict__ cnt, int D, int H, int W, int z0,
                                     int y0, int x0) {
  const int64_t pv = (int64_t)pd * ph * pw;
  const int64_t V = (int64_t)D * H * W;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pv; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % pw), y = (int)((i / pw) % ph), z = (int)(i / ((int64_t)pw * ph));
    float v[SW_MAXC], mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < SW_MAXC; c++)
      if (c < C) {
        v[c] = ST<T>::ld(logits + c * pv + i);
        mx = fmaxf(mx, v[c]);
      }
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < SW_MAXC; c++)
      if (c < C) {
        v[c] = expf(v[c] - mx);
        sum += v[c];
      }
    const float inv = 1.f / sum;
    const int64_t o = ((int64_t)(z0 + z) * H + (y0 + y)) * W + (x0 + x);
#pragma unroll
    for (int c = 0; c < SW_MAXC; c++)
      if (c < C) psum[c * V + o] += v[c] * inv;
    cnt[o] += 1.f;
  }
}
__global__ void sw_finalize_kernel(const float* __restrict__ psum, const float* __restrict__ cnt, int C, int64_t V,
                                   uint8_t* __restrict__ label) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (int64_t)gridDim.x * blockDim.x) {
    const float n = cnt[i];
    float best = -INFINITY;
    int bi = 0;
    if (n > 0.f) {
      // argmax(softmax(p / n)): softmax is monotonic, so the vote is the first maximum of the mean probabilities
#pragma unroll
      for (int c = 0; c < SW_MAXC; c++)
        if (c < C) {
          const float m = psum[c * V + i] / n;
          if (m > best) best = m, bi = c;
        }
    }
    label[i] = (uint8_t)bi;
  }
}
}  // namespace

int hdf_launch_sw_accumulate(int dtype, const void* logits, int C, int pd, int ph, int pw, float* psum, float* cnt,
                             int D, int H, int W, int z0, int y0, int x0, hipStream_t st) {
  HDF_CHECK_ARG(C >= 1 && C <= SW_MAXC, "sw_accumulate: n_cls=%d (max %d)", C, SW_MAXC);
  HDF_CHECK_ARG(z0 >= 0 && y0 >= 0 && x0 >= 0 && z0 + pd <= D && y0 + ph <= H && x0 + pw <= W,
                "sw_accumulate: window (%d,%d,%d)+(%d,%d,%d) outside the %dx%dx%d volume", z0, y0, x0, pd, ph, pw, D, H,
                W);
  const int64_t pv = (int64_t)pd * ph * pw;
  dim3 grid((unsigned)std::min<int64_t>(ceil_div64(pv, 256), 4096));
  HDF_DISPATCH_T(dtype, hipLaunchKernelGGL(sw_accumulate_kernel<T>, grid, dim3(256), 0, st, (const T*)logits, C, pd, ph, pw,
                                           psum, cnt, D, H, W, z0, y0, x0));
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
int hdf_launch_sw_finalize(const float* psum, const float* cnt, int C, int64_t V, uint8_t* label, hipStream_t st) {
  HDF_CHECK_ARG(C >= 1 && C <= SW_MAXC, "sw_finalize: n_cls=%d (max %d)", C, SW_MAXC);
  dim3 grid((unsigned)std::min<int64_t>(ceil_div64(V, 256), 8192));
  hipLaunchKernelGGL(sw_finalize_kernel, grid, dim3(256), 0, st, psum, cnt, C, V, label);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
