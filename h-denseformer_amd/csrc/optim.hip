// Flat optimizer steps (hdf_optim_step): torch.optim.Adam / AdamW / SGD(momentum, nesterov) as trainer.py:793-840 builds
// them, over the flat fp32 parameter and gradient buffers.  Two launches per step:
//   optim_prologue_kernel  one thread: reads *found_inf and *grad_scale, advances the device step counter unless the step
//                          is skipped, and leaves the bias corrections of that step in the OptimCtl words;
//   optim_kernel<RULE>     the streaming update; every block reads the OptimCtl the prologue finished writing (stream
//                          order: no block can see a half-advanced counter) and returns at once on a skipped step.
// Nothing comes back to the host.  The kernels are HBM-bound (29 B per element for Adam / AdamW, 21 for SGD): 16-byte
// accesses on the fp32 buffers, one 4-byte mask word per four elements, a grid-stride loop, and no more.
#include <algorithm>

#include "optim.h"

namespace {

struct OptimArgs {
  float lr[2], wd[2];   // [0]: mask byte set (the decay group), [1]: the rest
  float keep[2];        // AdamW: 1 - lr*wd of each group, formed on the host in double and rounded once (as torch does)
  float b1, b2, eps;    // SGD: b1 is the momentum
  float gmul;           // host-side multiplier on the gradient
  int nesterov;
};

__global__ void optim_prologue_kernel(OptimCtl* __restrict__ ctl, const float* __restrict__ grad_scale,
                                      const float* __restrict__ found_inf, float b1, float b2) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const bool skip = found_inf && *found_inf != 0.f;   // inf / NaN count as found
  const int step = ctl->step + (skip ? 0 : 1);
  ctl->step = step;
  ctl->skip = skip ? 1 : 0;
  // 1 - b^step and sqrt(1 - b2^step) of the fp32 betas, formed in double and rounded to fp32 ONCE, at the end.  The power
  // must not be rounded before the subtraction: 1 - b2^k is about k * 1e-3 in the first steps, and a power rounded to
  // fp32 leaves its 2^-25 there as up to 3.3e-6 of sqrt(1 - b2^k) (step 2), 200 times the final rounding.  The host forms
  // the same two expressions for hdf_adam_step (hdf_launch_adam); both pows are within an ulp of a double, so the two
  // entries agree unless 1 - b^k lies that close to the middle of two fp32 values
  ctl->bc1 = (float)(1.0 - pow((double)b1, (double)step));
  ctl->bc2s = (float)sqrt(1.0 - pow((double)b2, (double)step));
  ctl->gdiv = grad_scale ? *grad_scale : 1.f;
}

template <int RULE>
__device__ __forceinline__ void optim_elem(float& p, float g, float& s1, float& s2, bool dec, const OptimCtl& c,
                                           const OptimArgs& a) {
  // no contraction left to the compiler (as in adam_elem): the 16-byte loop and the scalar tail must give the same bits
#pragma clang fp contract(off)
  const float lr = dec ? a.lr[0] : a.lr[1];
  const float wd = dec ? a.wd[0] : a.wd[1];
  g = g / c.gdiv;   // torch's fused steps divide by the scale too (x / 1 is x)
  if (RULE == HDF_OPTIM_ADAM) {
    // torch adds the decay only where weight_decay != 0; the masked group keeps hdf_adam_step's form exactly
    adam_elem(p, g, s1, s2, dec || wd != 0.f, a.gmul, lr, a.b1, a.b2, a.eps, wd, c.bc1, c.bc2s);
  } else if (RULE == HDF_OPTIM_ADAMW) {
    p = p * (dec ? a.keep[0] : a.keep[1]);
    adam_elem(p, g, s1, s2, false, a.gmul, lr, a.b1, a.b2, a.eps, 0.f, c.bc1, c.bc2s);
  } else {
    const float gi = g * a.gmul + (wd != 0.f ? wd * p : 0.f);
    const float buf = c.step == 1 ? gi : a.b1 * s1 + gi;   // the first step initialises the buffer to the gradient
    s1 = buf;
    p = p - lr * (a.nesterov ? gi + a.b1 * buf : buf);
  }
}

template <int RULE>
__global__ __launch_bounds__(256) void optim_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ s1, float* __restrict__ s2,
                                                    const uint8_t* __restrict__ mask, int64_t n,
                                                    const OptimCtl* __restrict__ ctl, OptimArgs a) {
  const OptimCtl c = *ctl;
  if (c.skip) return;
  constexpr bool TWO = RULE != HDF_OPTIM_SGD;
  const int64_t nvec = n >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    float pv[4], gv[4], av[4], bv[4] = {0.f, 0.f, 0.f, 0.f};
    ST<float>::ld4(p + 4 * i, pv);
    ST<float>::ld4(g + 4 * i, gv);
    ST<float>::ld4(s1 + 4 * i, av);
    if (TWO) ST<float>::ld4(s2 + 4 * i, bv);
    const uint32_t mk = reinterpret_cast<const uint32_t*>(mask)[i];
#pragma unroll
    for (int j = 0; j < 4; j++) optim_elem<RULE>(pv[j], gv[j], av[j], bv[j], ((mk >> (8 * j)) & 0xffu) != 0, c, a);
    ST<float>::st4(p + 4 * i, pv[0], pv[1], pv[2], pv[3]);
    ST<float>::st4(s1 + 4 * i, av[0], av[1], av[2], av[3]);
    if (TWO) ST<float>::st4(s2 + 4 * i, bv[0], bv[1], bv[2], bv[3]);
  }
  // tail: n % 4 elements, one thread each
  const int64_t t = 4 * nvec + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    float pi = p[t], ai = s1[t], bi = TWO ? s2[t] : 0.f;
    optim_elem<RULE>(pi, g[t], ai, bi, mask[t] != 0, c, a);
    p[t] = pi;
    s1[t] = ai;
    if (TWO) s2[t] = bi;
  }
}

// ---------------------------------------------------------------------------------- Adam
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, const uint8_t* __restrict__ decay, int64_t n, float lr, float b1,
                            float b2, float eps, float wd, float bc1, float bc2_sqrt, float gscale) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float pi = p[i], mi = m[i], vi = v[i];
    adam_elem(pi, g[i], mi, vi, decay && decay[i], gscale, lr, b1, b2, eps, wd, bc1, bc2_sqrt);   // optim.h
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
  }
}

}  // namespace

int hdf_launch_optim(int rule, float* p, const float* g, float* s1, float* s2, const uint8_t* mask, int64_t n, float lr0,
                     float lr1, float wd0, float wd1, float b1, float b2, float eps, int nesterov, float gmul,
                     const float* grad_scale, const float* found_inf, int* step_state, hipStream_t st) {
  HDF_CHECK_ARG(rule == HDF_OPTIM_ADAM || rule == HDF_OPTIM_ADAMW || rule == HDF_OPTIM_SGD,
                "optim_step: unknown rule %d (0 Adam, 1 AdamW, 2 SGD)", rule);
  HDF_CHECK_ARG(n >= 0, "optim_step: n=%lld", (long long)n);
  const bool two = rule != HDF_OPTIM_SGD;
  HDF_CHECK_ARG(p && g && s1 && mask && step_state && (s2 || !two), "optim_step: null argument");
  if (two)
    HDF_CHECK_ARG(b1 >= 0.f && b1 < 1.f && b2 >= 0.f && b2 < 1.f, "optim_step: betas (%g, %g) outside [0, 1)", b1, b2);
  else
    HDF_CHECK_ARG(b1 >= 0.f && b1 < 1.f && (!nesterov || b1 > 0.f),
                  "optim_step: momentum %g outside [0, 1) (Nesterov needs a momentum above 0)", b1);
  const uintptr_t al = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(s1) |
                       reinterpret_cast<uintptr_t>(s2);
  HDF_CHECK_ARG((al & 15) == 0 && (reinterpret_cast<uintptr_t>(mask) & 3) == 0,
                "optim_step: the fp32 buffers must be 16-byte aligned and the mask 4-byte aligned");
  if (n == 0) return HDF_OK;
  OptimCtl* ctl = reinterpret_cast<OptimCtl*>(step_state);
  hipLaunchKernelGGL(optim_prologue_kernel, dim3(1), dim3(64), 0, st, ctl, grad_scale, found_inf, two ? b1 : 0.f,
                     two ? b2 : 0.f);
  HDF_LAUNCH_CHECK();
  const OptimArgs a = {{lr0, lr1}, {wd0, wd1}, {(float)(1.0 - (double)lr0 * wd0), (float)(1.0 - (double)lr1 * wd1)},
                       b1, b2, eps, gmul, nesterov};
  // memory-bound: at most 8 blocks on each of the 256 compute units, the rest of the buffer by grid stride
  const dim3 grid((unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div64(n >> 2, 256), 1), 2048));
#define HDF_OPTIM_LAUNCH(R) \
  hipLaunchKernelGGL(optim_kernel<R>, grid, dim3(256), 0, st, p, g, s1, s2, mask, n, (const OptimCtl*)ctl, a)
  if (rule == HDF_OPTIM_ADAM) HDF_OPTIM_LAUNCH(HDF_OPTIM_ADAM);
  else if (rule == HDF_OPTIM_ADAMW) HDF_OPTIM_LAUNCH(HDF_OPTIM_ADAMW);
  else HDF_OPTIM_LAUNCH(HDF_OPTIM_SGD);
#undef HDF_OPTIM_LAUNCH
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_adam(float* p, const float* g, float* m, float* v, const uint8_t* decay, int64_t n, float lr, float b1,
                    float b2, float eps, float wd, int step, float gscale, hipStream_t st) {
  // as optim_prologue_kernel: in double, rounded to fp32 once
  float bc1 = (float)(1.0 - pow((double)b1, (double)step));
  float bc2s = (float)sqrt(1.0 - pow((double)b2, (double)step));
  unsigned gx = (unsigned)std::min<int64_t>(ceil_div64(n, 256), 4096);
  hipLaunchKernelGGL(adam_kernel, dim3(gx), dim3(256), 0, st, p, g, m, v, decay, n, lr, b1, b2, eps, wd, bc1, bc2s,
                     gscale);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}
