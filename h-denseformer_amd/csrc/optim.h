// Flat optimizer steps over the fp32 parameter buffer: the update rules of trainer.py:793-840 (Adam, AdamW, SGD with
// Nesterov momentum), one streaming kernel per step.
#pragma once
#include "hdf_common.h"

#define HDF_OPTIM_ADAM 0
#define HDF_OPTIM_ADAMW 1
#define HDF_OPTIM_SGD 2

// The device-resident step state of hdf_optim_step: word 0 (the count of steps TAKEN) persists between calls, the rest is
// rewritten by the one-thread prologue of every call and read by every block of the update kernel launched behind it.
struct OptimCtl {
  int step;      // steps taken so far, this one included unless it is skipped
  int skip;      // *found_inf != 0: the update kernel returns at once
  float bc1;     // 1 - beta1^step
  float bc2s;    // sqrt(1 - beta2^step)
  float gdiv;    // *grad_scale, or 1
  int pad[3];
};
static_assert(sizeof(OptimCtl) == 32, "hdf.h: HDF_OPTIM_STATE_WORDS");

// One element of torch.optim.Adam (L2 decay added to the gradient where `dec`).  The ONE copy of the arithmetic:
// adam_kernel (hdf_adam_step) and optim_kernel (hdf_optim_step), both in optim.hip, inline it, and
// tests/test_gpu_optim.py holds the two to the same bits.  The fusing is pinned (as in_bwd_elem, hdf_common.h): left to
// -ffp-contract hipcc fused b2*v + ... in the vectorised kernel and not in the scalar one.  The two explicit fma are the
// ones adam_kernel has always had.
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, bool dec, float gscale, float lr,
                                          float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt) {
#pragma clang fp contract(off)
  float pi = p;
  float gi = __builtin_fmaf(g, gscale, dec ? wd * pi : 0.f);
  float mi = b1 * m + (1.f - b1) * gi;
  float vi = b2 * v + (1.f - b2) * gi * gi;
  m = mi;
  v = vi;
  float denom = sqrtf(vi) / bc2_sqrt + eps;
  p = __builtin_fmaf(-(lr / bc1), mi / denom, pi);
}

// rule: HDF_OPTIM_*; s1 / s2: exp_avg / exp_avg_sq (Adam, AdamW) or momentum buffer / null (SGD); lr, wd: [0] where the
// mask byte is set, [1] elsewhere; b1: beta1, or the momentum of SGD
int hdf_launch_optim(int rule, float* p, const float* g, float* s1, float* s2, const uint8_t* mask, int64_t n, float lr0,
                     float lr1, float wd0, float wd1, float b1, float b2, float eps, int nesterov, float gmul,
                     const float* grad_scale, const float* found_inf, int* step_state, hipStream_t st);
// hdf_adam_step: one Adam step with the bias corrections of `step` formed on the host
int hdf_launch_adam(float* p, const float* g, float* m, float* v, const uint8_t* decay, int64_t n, float lr, float b1,
                    float b2, float eps, float wd, int step, float gscale, hipStream_t st);
