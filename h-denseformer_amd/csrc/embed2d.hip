// The 2-D model as a 3-D one: parameter embedding / gradient extraction and the depth-axis copies (hdf_forward,
// hdf_backward* of a 2-D plan: exec.hip).
#include <algorithm>

#include "plan_internal.h"

// ---------------------------------------------------------------------------------------------- 2-D embedding
// HDenseFormer_2D (reference models/HDenseFormer_2D.py:172-250) is the 3-D graph with 2-D primitives.  It equals,
// EXACTLY, the 3-D network applied to the image replicated along a depth axis of 16 when its parameters are embedded as
//   Conv2d [o,i,3,3]            -> Conv3d [o,i,3,3,3]   with the 2-D kernel on depth tap 1, zeros on taps 0 and 2
//   ConvTranspose2d [i,o,3,3]   -> ConvTranspose3d      with the 2-D kernel on depth taps 1 AND 2 (output slice 2z
//                                  takes tap 1 of input slice z, slice 2z+1 takes tap 2 of the same slice), zero on tap 0
//   patch Conv2d [c,1,16,16]    -> Conv3d [c,1,16,16,16] with the 2-D kernel on depth slice 0, zeros elsewhere
//   everything else             -> unchanged
// Every activation then consists of identical depth slices (InstanceNorm statistics, MaxPool3d, trilinear x2 and the
// token grid all reduce to their 2-D forms), the 2-D logits are depth slice 0 of the 3-D logits, and by the chain
// rule the 2-D parameter gradient is the sum of the 3-D gradient over the embedded positions.  The cost is the 16
// (at level 0) .. 2 (level 3) redundant slices; a native depth-1 mode of the pooling / up-sampling / transposed-conv
// kernels would remove it.
struct Embed2dBatch {
  Embed2dJob j[HDF_MAX_EMBED_JOBS];
};
__device__ __forceinline__ bool embed_live(int kind, int z) {
  return kind == 0 || (kind == 1 && z == 1) || (kind == 2 && (z == 1 || z == 2)) || (kind == 3 && z == 0);
}
// 3-D parameters from the 2-D ones (grid (blocks, jobs))
__global__ void embed2d_kernel(Embed2dBatch b, const float* __restrict__ p2, float* __restrict__ p3) {
  const Embed2dJob& jb = b.j[blockIdx.y];
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < jb.n3; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t outer = e / ((int64_t)jb.rep * jb.inner);
    const int z = (int)((e / jb.inner) % jb.rep), r = (int)(e % jb.inner);
    p3[jb.off3 + e] = embed_live(jb.kind, z) ? p2[jb.off2 + outer * jb.inner + r] : 0.f;
  }
}
// 2-D gradients from the 3-D ones: the transpose of the embedding (sum over the embedded positions)
__global__ void extract2d_kernel(Embed2dBatch b, const float* __restrict__ g3, float* __restrict__ g2) {
  const Embed2dJob& jb = b.j[blockIdx.y];
  const int64_t n2 = jb.n3 / jb.rep;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n2; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t outer = e / jb.inner;
    const int r = (int)(e % jb.inner);
    float s = 0.f;
    for (int z = 0; z < jb.rep; z++)
      if (embed_live(jb.kind, z)) s += g3[jb.off3 + (outer * jb.rep + z) * jb.inner + r];
    g2[jb.off2 + e] = s;
  }
}
// x [rows][HW] -> [rows][reps][HW]
__global__ void replicate_depth_kernel(const float* __restrict__ x2, float* __restrict__ x3, int64_t rows, int reps,
                                       int64_t hw) {
  const int64_t total = rows * reps * hw;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x)
    x3[e] = x2[(e / (reps * hw)) * hw + e % hw];
}
// depth slice 0 of [rows][reps][HW] -> [rows][HW]  (to2d) or its transpose: slice 0 <- src, other slices <- 0
template <typename T>
__global__ void depth_slice_kernel(T* __restrict__ t3, T* __restrict__ t2, int64_t rows, int reps, int64_t hw,
                                   int to2d) {
  if (to2d) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < rows * hw; e += (int64_t)gridDim.x * blockDim.x)
      t2[e] = t3[(e / hw) * reps * hw + e % hw];
  } else {
    T zero;
    zero.v = 0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < rows * reps * hw;
         e += (int64_t)gridDim.x * blockDim.x) {
      const int64_t row = e / (reps * hw), rem = e % (reps * hw);
      t3[e] = rem < hw ? t2[row * hw + rem] : zero;
    }
  }
}
struct f32w {  // float wrapper with the .v member the 16-bit storage structs have
  float v;
};

int hdf_launch_embed2d(hdf_plan* p, const float* p2, float* p3, hipStream_t st) {
  Embed2dBatch b;
  for (size_t k = 0; k < p->ejobs.size(); k++) b.j[k] = p->ejobs[k];
  hipLaunchKernelGGL(embed2d_kernel, dim3(64, (unsigned)p->ejobs.size()), dim3(256), 0, st, b, p2, p3);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
int hdf_launch_extract2d(hdf_plan* p, int stages, const float* g3, float* g2, hipStream_t st) {
  Embed2dBatch b;
  unsigned n = 0;
  for (const Embed2dJob& j : p->ejobs)
    if (j.stage & stages) b.j[n++] = j;
  if (n == 0) return HDF_OK;
  hipLaunchKernelGGL(extract2d_kernel, dim3(64, n), dim3(256), 0, st, b, g3, g2);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
int hdf_launch_replicate_depth(const float* x2, float* x3, int64_t rows, int reps, int64_t hw, hipStream_t st) {
  hipLaunchKernelGGL(replicate_depth_kernel, dim3(2048), dim3(256), 0, st, x2, x3, rows, reps, hw);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
// depth slice 0 of a [rows][reps][hw] tensor of the plan's storage type <-> [rows][hw]
int hdf_launch_depth_slice(int dtype, void* t3, void* t2, int64_t rows, int reps, int64_t hw, int to2d, hipStream_t st) {
  const unsigned gx = (unsigned)std::min<int64_t>(ceil_div64(rows * (to2d ? 1 : reps) * hw, 256), 4096);
  if (dtype == HDF_F32)
    hipLaunchKernelGGL(depth_slice_kernel<f32w>, dim3(gx), dim3(256), 0, st, (f32w*)t3, (f32w*)t2, rows, reps, hw, to2d);
  else  // bf16 / f16: same 2-byte moves
    hipLaunchKernelGGL(depth_slice_kernel<bf16_t>, dim3(gx), dim3(256), 0, st, (bf16_t*)t3, (bf16_t*)t2, rows, reps, hw,
                       to2d);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
