// Weight packers: fp32 torch-layout parameters -> the [27][CoutP][Cin] (or fragment-major, hdf_conv_weight_layout) panels in
// the storage type that the convolution kernels read.
#include "conv_igemm.h"

namespace {

// dst[t][o][i] = src[o*so + i*si + (flip ? 26-t : t)]  (zero for o>=O or i>=I); dst is [27][OP][IP]
template <typename T>
__global__ void pack_w_kernel(const float* __restrict__ src, T* __restrict__ dst, int O, int I, int OP, int IP,
                              int64_t so, int64_t si, int flip) {
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t total = (int64_t)27 * OP * IP;
  if (idx >= total) return;
  int i = idx % IP;
  int o = (idx / IP) % OP;
  int t = idx / ((int64_t)IP * OP);
  float v = 0.f;
  if (o < O && i < I) v = src[o * so + i * si + (flip ? 26 - t : t)];
  ST<T>::st(dst + idx, v);
}

struct PackBatch {
  PackJob j[HDF_MAX_PACK_JOBS];
};
// grid (blocks, jobs): job blockIdx.y, grid-stride over its OP*IP (out, in) pairs; a thread reads the pair's 27 taps
// (both source layouts keep them contiguous: 108 bytes) and writes one element of each of the 27 tap planes, where
// consecutive threads are consecutive `in` indices, i.e. coalesced
template <typename T>
__global__ void pack_batch_kernel(PackBatch b, const float* __restrict__ params, char* __restrict__ ws) {
  HDF_LIGHT_PRIO();   // (runs beside the first level-0 conv since round 5: plan.hip forward3d)
  const PackJob& jb = b.j[blockIdx.y];
  const float* src = params + jb.src_off;
  T* dst = reinterpret_cast<T*>(ws + jb.dst_off);
  const int64_t pairs = (int64_t)jb.OP * jb.IP;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < pairs; idx += (int64_t)gridDim.x * blockDim.x) {
    const int i = idx % jb.IP, o = idx / jb.IP;
    const bool live = o < jb.O && i < jb.I;
    const float* sp = src + (live ? (int64_t)o * jb.so + (int64_t)i * jb.si : 0);
    float v[27];
#pragma unroll
    for (int t = 0; t < 27; t++) v[t] = sp[t];
    constexpr int E32 = 32 / (int)sizeof(T);  // elements per 32-byte fragment step
    const int64_t at = jb.frag ? (((int64_t)(o >> 5) * (jb.IP / E32) + i / E32) * 32 + (o & 31)) * E32 + i % E32 : idx;
#pragma unroll
    for (int t = 0; t < 27; t++) ST<T>::st(dst + (int64_t)t * pairs + at, live ? (jb.flip ? v[26 - t] : v[t]) : 0.f);
  }
}

}  // namespace

int hdf_launch_pack_batch(int dtype, const float* params, char* ws, const PackJob* jobs, int njobs, hipStream_t st) {
  HDF_CHECK_ARG(njobs >= 0 && njobs <= HDF_MAX_PACK_JOBS, "pack batch: %d jobs", njobs);
  if (njobs == 0) return HDF_OK;
  PackBatch b;
  for (int k = 0; k < njobs; k++) b.j[k] = jobs[k];
  dim3 grid(64, njobs);
  HDF_DISPATCH_T(dtype, hipLaunchKernelGGL(pack_batch_kernel<T>, grid, dim3(256), 0, st, b, params, ws));
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_pack_w(int dtype, const float* src, void* dst, int O, int I, int OP, int IP, int64_t so, int64_t si,
                      int flip, hipStream_t st) {
  int64_t total = (int64_t)27 * OP * IP;
  dim3 grid((unsigned)ceil_div64(total, 256));
  HDF_DISPATCH_T(dtype, hipLaunchKernelGGL(pack_w_kernel<T>, grid, dim3(256), 0, st, src, (T*)dst, O, I, OP, IP, so, si,
                                           flip));
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
