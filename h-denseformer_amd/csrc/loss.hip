// Fused DeepSuperloss(CEPlusDice) and DeepSuperloss(FocalLoss / FLPlusDice), forward and backward, and nothing else: the
// evaluation metrics and the inference tail are metrics.hip, the input staging augment.hip, the optimizer steps optim.hip.
//
// Reference: loss/combine_loss.py:8-79 ; loss/dice_loss.py:5-87 ; loss/cross_entropy.py:8-22,45-73.
// One pass per scale reads the logits once (NCDHW, coalesced along voxels) and the fp32 one-hot target
// at the 2^i-strided positions (nearest down-sampling), producing per-(sample,class) sums
// sum(p*t), sum(p), sum(t) and the CE (or focal) sum; backward recomputes the softmax from the logits.
#include <type_traits>

#include "loss.h"

namespace {
constexpr int MAXC = HDF_CLASS_SLOTS;
constexpr int LOSS_BLOCKS = 1024;
constexpr int NSTAT = 3 * MAXC + 2;  // per class: sum p*t, sum p, sum t; then the (weighted) CE sum and the sum of CE weights

// All scales of the deep supervision in ONE launch: grid (sum of the scales' block counts, N); a block finds its scale from
// the block ranges in LossLevels.  A thread owns VEC = 4 consecutive voxels of a row of the scale's grid (one 8-byte load
// of 16-bit logits and -- at scale 0 -- one 16-byte load of the one-hot target per class: the scalar form had 2 + 4 bytes
// per lane and class in flight and ran at 1.1 TB/s); rows whose width is not a multiple of 4, or unaligned views, take
// VEC = 1.  The sums of a thread are taken in voxel order, of a block in a fixed order: bitwise reproducible.
struct LossLevel {
  const void* logits;
  void* dlogits;
  int Ds, Hs, Ws, stride;
  int blk0, nblk, vec;
};
struct LossLevels {
  LossLevel L[4];
  int nscale;
};

template <typename T>
__device__ __forceinline__ void ld_vox(const T* p, float* f, std::integral_constant<int, 1>) {
  f[0] = ST<T>::ld(p);
}
template <typename T>
__device__ __forceinline__ void ld_vox(const T* p, float* f, std::integral_constant<int, 4>) {
  ST<T>::ld4(p, f);
}
template <typename T>
__device__ __forceinline__ void st_vox(T* p, const float* f, std::integral_constant<int, 1>) {
  ST<T>::st(p, f[0]);
}
template <typename T>
__device__ __forceinline__ void st_vox(T* p, const float* f, std::integral_constant<int, 4>) {
  ST<T>::st4(p, f[0], f[1], f[2], f[3]);
}
// one-hot target of VEC voxels that are `stride` apart in the full-resolution row
template <int VEC>
__device__ __forceinline__ void ld_tgt(const float* p, int stride, float* t) {
  if (VEC == 4 && stride == 1) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
    t[0] = v[0], t[1] = v[1], t[2] = v[2], t[3] = v[3];
  } else {
#pragma unroll
    for (int j = 0; j < VEC; j++) t[j] = p[(int64_t)j * stride];
  }
}

// FocalLoss (loss/cross_entropy.py:45-73) per (voxel, class) on the fp32 softmax p, as torch evaluates it:
// bce = F.binary_cross_entropy (both logs clamped at -100), p_t = p t + (1-p)(1-t), loss = alpha_t bce (1-p_t)^gamma with
// alpha_t = alpha t + (1-alpha)(1-t) (no factor when alpha < 0).  log p is the log-softmax (torch's log of the rounded
// p up to one rounding; p underflowing to 0 clamps at -100 in both), log(1-p) is taken of the rounded 1-p as in torch.
// The focal forms have no CE term: their sum takes the CE slot of the partials.
struct FocalP {
  float alpha, gamma;  // gamma is 0 or >= 1 (the launcher checks)
  int mean;            // reduction 'mean' (divide by N*C*V of the scale) or 'sum'
};
// torch's pow(Tensor, Scalar) evaluates the small integer exponents as products
__device__ __forceinline__ float focal_pow(float x, float g) {
  return g == 2.f ? x * x : g == 1.f ? x : g == 0.f ? 1.f : g == 3.f ? x * x * x : powf(x, g);
}
struct FocalEl {
  float bce, q, a;  // BCE, 1 - p_t, alpha_t
};
__device__ __forceinline__ FocalEl focal_el(float logp, float p, float t, const FocalP& fp) {
  FocalEl r;
  r.bce = -(t * fmaxf(logp, -100.f) + (1.f - t) * fmaxf(__logf(1.f - p), -100.f));
  r.q = 1.f - (p * t + (1.f - p) * (1.f - t));
  r.a = fp.alpha >= 0.f ? fp.alpha * t + (1.f - fp.alpha) * (1.f - t) : 1.f;
  return r;
}
__device__ __forceinline__ float focal_loss_el(float logp, float p, float t, const FocalP& fp) {
  const FocalEl e = focal_el(logp, p, t, fp);
  return e.a * (e.bce * focal_pow(e.q, fp.gamma));
}
// d loss / d p by torch's autograd: BCE's backward is (p - t) / max(p (1-p), 1e-12) (not the derivative of the clamped
// logs), and pow's backward is 0 for gamma == 0
__device__ __forceinline__ float focal_dp_el(float logp, float p, float t, const FocalP& fp) {
  const FocalEl e = focal_el(logp, p, t, fp);
  float d = focal_pow(e.q, fp.gamma) * ((p - t) / fmaxf((1.f - p) * p, 1e-12f));
  if (fp.gamma != 0.f) d += e.bce * (fp.gamma * focal_pow(e.q, fp.gamma - 1.f)) * (1.f - 2.f * t);
  return e.a * d;
}

template <typename T, int VEC, int MC, bool FOCAL>
__device__ __forceinline__ void loss_fwd_body(const LossLevel& L, int bx, const float* __restrict__ target, int C, int D,
                                              int H, int W, const float* __restrict__ cw, const FocalP& fp,
                                              float* acc) {
  const T* logits = reinterpret_cast<const T*>(L.logits);
  const int n = blockIdx.y, Ws = L.Ws, Hs = L.Hs, stride = L.stride;
  const int64_t V = (int64_t)L.Ds * Hs * Ws, Vf = (int64_t)D * H * W;
  const std::integral_constant<int, VEC> vt{};
  // (32-bit voxel indices inside a sample: the launcher checks D*H*W < 2^31; at scale 0 the two grids coincide)
  for (int v = (bx * 256 + (int)threadIdx.x) * VEC; v < (int)V; v += L.nblk * 256 * VEC) {
    int64_t vf = v;
    if (stride > 1) {
      const int x = v % Ws, y = (v / Ws) % Hs, z = v / (Ws * Hs);
      vf = ((int64_t)z * stride * H + (int64_t)y * stride) * W + (int64_t)x * stride;
    }
    float lg[MC][VEC], t[MC][VEC];
#pragma unroll
    for (int c = 0; c < MC; c++)
      if (c < C) {
        ld_vox(logits + ((int64_t)n * C + c) * V + v, lg[c], vt);
        ld_tgt<VEC>(target + ((int64_t)n * C + c) * Vf + vf, stride, t[c]);
      }
#pragma unroll
    for (int j = 0; j < VEC; j++) {
      float mx = -INFINITY, tbest = -INFINITY;
      int tc = 0;
#pragma unroll
      for (int c = 0; c < MC; c++)
        if (c < C) {
          mx = fmaxf(mx, lg[c][j]);
          if (t[c][j] > tbest) {
            tbest = t[c][j];
            tc = c;
          }
        }
      float se = 0.f, e[MC];
#pragma unroll
      for (int c = 0; c < MC; c++)
        if (c < C) {
          e[c] = __expf(lg[c][j] - mx);
          se += e[c];
        }
      const float inv = 1.f / se;
      const float lse = mx + __logf(se);
#pragma unroll
      for (int c = 0; c < MC; c++)
        if (c < C) {
          const float p = e[c] * inv;
          acc[c] += p * t[c][j];
          acc[MAXC + c] += p;
          acc[2 * MAXC + c] += t[c][j];
          if constexpr (FOCAL) {
            acc[3 * MAXC] += focal_loss_el(lg[c][j] - lse, p, t[c][j], fp);
          } else if (c == tc) {
            // torch CrossEntropyLoss(weight=w, reduction='mean'): sum_v w[t_v] * nll_v / sum_v w[t_v]
            const float wv = cw ? cw[c] : 1.f;
            acc[3 * MAXC] += cw ? wv * (lse - lg[c][j]) : lse - lg[c][j];
            acc[3 * MAXC + 1] += wv;
          }
        }
    }
  }
}

// The kernel bodies below are written out per kernel rather than shared through a device function: that keeps the
// code objects of the CE/Dice kernels exactly what they were before the focal forms were added (a function boundary
// changes their scheduling).
template <typename T, int MC>  // MC: class slots held in registers (4 or 8)
__global__ __launch_bounds__(256) void loss_fwd_kernel(LossLevels lv, const float* __restrict__ target, int C, int D,
                                                       int H, int W,
                                                       const float* __restrict__ cw /*[C] class weights or null*/,
                                                       float* __restrict__ partials /*[scale][N][LOSS_BLOCKS][NSTAT]*/) {
  __shared__ float red[4][NSTAT];
  int i = 0;
#pragma unroll
  for (int k = 1; k < 4; k++)
    if (k < lv.nscale && (int)blockIdx.x >= lv.L[k].blk0) i = k;
  const LossLevel& L = lv.L[i];
  const int bx = blockIdx.x - L.blk0;
  float acc[NSTAT];
#pragma unroll
  for (int k = 0; k < NSTAT; k++) acc[k] = 0.f;
  if (L.vec == 4)
    loss_fwd_body<T, 4, MC, false>(L, bx, target, C, D, H, W, cw, FocalP{}, acc);
  else
    loss_fwd_body<T, 1, MC, false>(L, bx, target, C, D, H, W, cw, FocalP{}, acc);
#pragma unroll
  for (int k = 0; k < NSTAT; k++) acc[k] = wave_sum(acc[k]);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < NSTAT; k++) red[wave][k] = acc[k];
  __syncthreads();
  if (threadIdx.x < NSTAT)
    partials[(((int64_t)i * gridDim.y + blockIdx.y) * LOSS_BLOCKS + bx) * NSTAT + threadIdx.x] =
        red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}
// the focal forms: the same sums with the focal sum in the CE slot (class weights act on the Dice term only, in the
// finalize)
template <typename T, int MC>
__global__ __launch_bounds__(256) void focal_fwd_kernel(LossLevels lv, const float* __restrict__ target, int C, int D,
                                                        int H, int W, FocalP fp, float* __restrict__ partials) {
  __shared__ float red[4][NSTAT];
  int i = 0;
#pragma unroll
  for (int k = 1; k < 4; k++)
    if (k < lv.nscale && (int)blockIdx.x >= lv.L[k].blk0) i = k;
  const LossLevel& L = lv.L[i];
  const int bx = blockIdx.x - L.blk0;
  float acc[NSTAT];
#pragma unroll
  for (int k = 0; k < NSTAT; k++) acc[k] = 0.f;
  if (L.vec == 4)
    loss_fwd_body<T, 4, MC, true>(L, bx, target, C, D, H, W, nullptr, fp, acc);
  else
    loss_fwd_body<T, 1, MC, true>(L, bx, target, C, D, H, W, nullptr, fp, acc);
#pragma unroll
  for (int k = 0; k < NSTAT; k++) acc[k] = wave_sum(acc[k]);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < NSTAT; k++) red[wave][k] = acc[k];
  __syncthreads();
  if (threadIdx.x < NSTAT)
    partials[(((int64_t)i * gridDim.y + blockIdx.y) * LOSS_BLOCKS + bx) * NSTAT + threadIdx.x] =
        red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// grid = nscale*N blocks of 256 threads (one per partial slot): per-(scale, sample) loss term + the backward
// coefficients coef[(i*N+n)*MAXC + c] = (A, B) of the Dice gradient; terms[i*N+n] is summed by loss_total_kernel
// FOCAL: the CE slot holds the focal sum, divided by N*C*V for focal_mean and taken as it is for 'sum'
template <bool FOCAL>
__device__ __forceinline__ void loss_finalize_block(const float* __restrict__ partials, int nscale, int N, int C,
                                                    const LossScales& sc, float smooth, float w_ce, float w_dice,
                                                    const float* __restrict__ cw, int ignore, int focal_mean,
                                                    float* __restrict__ terms, float* __restrict__ coefA,
                                                    float* __restrict__ coefB, float* __restrict__ wsum_out) {
  __shared__ double red[4][NSTAT];
  const int i = blockIdx.x / N, n = blockIdx.x % N, blocks = sc.blocks[i];
  const float* base = partials + ((int64_t)i * N + n) * LOSS_BLOCKS * NSTAT;
  double s[NSTAT];
#pragma unroll
  for (int k = 0; k < NSTAT; k++) s[k] = 0.0;
  for (int b = threadIdx.x; b < blocks; b += 256)
#pragma unroll
    for (int k = 0; k < NSTAT; k++) s[k] += (double)base[(int64_t)b * NSTAT + k];
  if (!FOCAL && cw) {  // weighted CE: the denominator is the weight sum over ALL samples of the scale (slot NSTAT-1 of every n)
    double wall = 0.0;
    for (int m = 0; m < N; m++) {
      const float* bm = partials + ((int64_t)i * N + m) * LOSS_BLOCKS * NSTAT;
      for (int b = threadIdx.x; b < blocks; b += 256) wall += (double)bm[(int64_t)b * NSTAT + 3 * MAXC + 1];
    }
    s[3 * MAXC + 1] = wall;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NSTAT; k++) {
    double v = s[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t[NSTAT];
    for (int k = 0; k < NSTAT; k++) t[k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
    double V = (double)sc.V[i];
    double ce;
    if constexpr (FOCAL) {
      ce = focal_mean ? t[3 * MAXC] / (V * N * C) : t[3 * MAXC];
    } else {
      ce = cw ? t[3 * MAXC] / t[3 * MAXC + 1] : t[3 * MAXC] / (V * N);
      if (n == 0) wsum_out[i] = cw ? (float)t[3 * MAXC + 1] : (float)(V * N);
    }
    double dice = 0.0;
    for (int c = 0; c < C; c++) {
      float A = 0.f, B = 0.f;
      if (c != ignore) {  // dice_loss.py:75-84: every class but ignore_index, times its class weight
        const double wc = cw ? (double)cw[c] : 1.0;
        double I = t[c], U = t[MAXC + c] + t[2 * MAXC + c];
        dice += wc * (1.0 - (2.0 * I + smooth) / (U + smooth)) / (double)N;
        A = (float)(wc * 2.0 / (U + smooth));
        B = (float)(wc * (2.0 * I + smooth) / ((U + smooth) * (U + smooth)));
      }
      coefA[((int64_t)i * N + n) * MAXC + c] = A;
      coefB[((int64_t)i * N + n) * MAXC + c] = B;
    }
    dice /= (double)(ignore >= 0 ? C - 1 : C);  // dice_loss.py:84-87
    // CE is already a mean over all N samples' voxels: every (scale, n) block contributes its own share
    terms[blockIdx.x] = (float)(((double)w_ce * ce + (double)w_dice * dice) * (double)sc.weight[i]);
  }
}

__global__ __launch_bounds__(256) void loss_finalize_kernel(const float* __restrict__ partials, int nscale, int N, int C,
                                                            LossScales sc, float smooth, float w_ce,
                                                            float w_dice, const float* __restrict__ cw, int ignore,
                                                            float* __restrict__ terms, float* __restrict__ coefA,
                                                            float* __restrict__ coefB, float* __restrict__ wsum_out) {
  loss_finalize_block<false>(partials, nscale, N, C, sc, smooth, w_ce, w_dice, cw, ignore, 0, terms, coefA, coefB,
                             wsum_out);
}
__global__ __launch_bounds__(256) void focal_finalize_kernel(const float* __restrict__ partials, int nscale, int N, int C,
                                                             LossScales sc, float smooth, float w_focal, int focal_mean,
                                                             float w_dice, const float* __restrict__ cw, int ignore,
                                                             float* __restrict__ terms, float* __restrict__ coefA,
                                                             float* __restrict__ coefB) {
  loss_finalize_block<true>(partials, nscale, N, C, sc, smooth, w_focal, w_dice, cw, ignore, focal_mean, terms, coefA,
                            coefB, nullptr);
}

__global__ void loss_total_kernel(const float* __restrict__ terms, int count, float* __restrict__ loss_out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double t = 0.0;
    for (int k = 0; k < count; k++) t += (double)terms[k];   // fixed order
    *loss_out = (float)t;
  }
}

struct LossBwdP {
  const float *coefA, *coefB;  // [scale][N][MAXC]
  const float* wsum;           // [scale]
  const float* gup;
  const float* cw;
  float w_ce, w_dice;
  int ignore;
};

template <typename T, int VEC, int MC, bool FOCAL>
__device__ __forceinline__ void loss_bwd_body(const LossLevel& L, int i, int bx, const float* __restrict__ target, int N,
                                              int C, int D, int H, int W, const LossBwdP& q, const FocalP& fp) {
  const T* logits = reinterpret_cast<const T*>(L.logits);
  T* dlogits = reinterpret_cast<T*>(L.dlogits);
  const int n = blockIdx.y, Ws = L.Ws, Hs = L.Hs, stride = L.stride;
  const int64_t V = (int64_t)L.Ds * Hs * Ws, Vf = (int64_t)D * H * W;
  const float g = (*q.gup) / (float)stride;   // scale weight 1 / 2^i (combine_loss.py:68-79)
  const float kce0 = q.cw ? q.w_ce * g / q.wsum[i] : q.w_ce * g / ((float)V * (float)N);
  const float kd = q.w_dice * g / ((float)(q.ignore >= 0 ? C - 1 : C) * (float)N);
  // focal: w_focal times the scale weight, over N*C*V for 'mean' (loss.mean() of the reference)
  const float kf = FOCAL ? (fp.mean ? q.w_ce * g / ((float)V * (float)N * (float)C) : q.w_ce * g) : 0.f;
  float cwr[MC], cA[MC], cB[MC];
#pragma unroll
  for (int c = 0; c < MC; c++) {
    cwr[c] = (q.cw && c < C) ? q.cw[c] : 1.f;
    cA[c] = c < C ? q.coefA[((int64_t)i * N + n) * MAXC + c] : 0.f;
    cB[c] = c < C ? q.coefB[((int64_t)i * N + n) * MAXC + c] : 0.f;
  }
  const std::integral_constant<int, VEC> vt{};
  // (32-bit voxel indices inside a sample: the launcher checks D*H*W < 2^31; at scale 0 the two grids coincide)
  for (int v = (bx * 256 + (int)threadIdx.x) * VEC; v < (int)V; v += L.nblk * 256 * VEC) {
    int64_t vf = v;
    if (stride > 1) {
      const int x = v % Ws, y = (v / Ws) % Hs, z = v / (Ws * Hs);
      vf = ((int64_t)z * stride * H + (int64_t)y * stride) * W + (int64_t)x * stride;
    }
    float lg[MC][VEC], t[MC][VEC];
#pragma unroll
    for (int c = 0; c < MC; c++)
      if (c < C) {
        ld_vox(logits + ((int64_t)n * C + c) * V + v, lg[c], vt);
        ld_tgt<VEC>(target + ((int64_t)n * C + c) * Vf + vf, stride, t[c]);
      }
#pragma unroll
    for (int j = 0; j < VEC; j++) {
      float mx = -INFINITY, tbest = -INFINITY;
      int tc = 0;
#pragma unroll
      for (int c = 0; c < MC; c++)
        if (c < C) {
          mx = fmaxf(mx, lg[c][j]);
          if (t[c][j] > tbest) {
            tbest = t[c][j];
            tc = c;
          }
        }
      float se = 0.f, p[MC];
#pragma unroll
      for (int c = 0; c < MC; c++)
        if (c < C) {
          p[c] = __expf(lg[c][j] - mx);
          se += p[c];
        }
      float inv = 1.f / se, dot = 0.f, G[MC];
      const float lse = FOCAL ? mx + __logf(se) : 0.f;
#pragma unroll
      for (int c = 0; c < MC; c++)
        if (c < C) {
          p[c] *= inv;
          G[c] = -kd * (cA[c] * t[c][j] - cB[c]);  // dDice/dp_c (the coefficients of the ignored class are zero)
          if constexpr (FOCAL) G[c] += kf * focal_dp_el(lg[c][j] - lse, p[c], t[c][j], fp);
          dot += G[c] * p[c];
        }
      if constexpr (FOCAL) {  // both terms through the softmax backward p (G - <G, p>)
#pragma unroll
        for (int c = 0; c < MC; c++)
          if (c < C) lg[c][j] = p[c] * (G[c] - dot);
      } else {
        float kce = kce0;
        if (q.cw) {
#pragma unroll
          for (int c = 0; c < MC; c++)
            if (c == tc) kce = kce0 * cwr[c];
        }
#pragma unroll
        for (int c = 0; c < MC; c++)
          if (c < C) lg[c][j] = kce * (p[c] - (c == tc ? 1.f : 0.f)) + p[c] * (G[c] - dot);
      }
    }
#pragma unroll
    for (int c = 0; c < MC; c++)
      if (c < C) st_vox(dlogits + ((int64_t)n * C + c) * V + v, lg[c], vt);
  }
}

template <typename T, int MC>
__global__ __launch_bounds__(256) void loss_bwd_kernel(LossLevels lv, const float* __restrict__ target, int N, int C,
                                                       int D, int H, int W, LossBwdP q) {
  int i = 0;
#pragma unroll
  for (int k = 1; k < 4; k++)
    if (k < lv.nscale && (int)blockIdx.x >= lv.L[k].blk0) i = k;
  const LossLevel& L = lv.L[i];
  const int bx = blockIdx.x - L.blk0;
  if (L.vec == 4)
    loss_bwd_body<T, 4, MC, false>(L, i, bx, target, N, C, D, H, W, q, FocalP{});
  else
    loss_bwd_body<T, 1, MC, false>(L, i, bx, target, N, C, D, H, W, q, FocalP{});
}
// q.w_ce carries w_focal and q.cw is null (the class weights are folded into the Dice coefficients by the finalize)
template <typename T, int MC>
__global__ __launch_bounds__(256) void focal_bwd_kernel(LossLevels lv, const float* __restrict__ target, int N, int C,
                                                        int D, int H, int W, LossBwdP q, FocalP fp) {
  int i = 0;
#pragma unroll
  for (int k = 1; k < 4; k++)
    if (k < lv.nscale && (int)blockIdx.x >= lv.L[k].blk0) i = k;
  const LossLevel& L = lv.L[i];
  const int bx = blockIdx.x - L.blk0;
  if (L.vec == 4)
    loss_bwd_body<T, 4, MC, true>(L, i, bx, target, N, C, D, H, W, q, fp);
  else
    loss_bwd_body<T, 1, MC, true>(L, i, bx, target, N, C, D, H, W, q, fp);
}
}  // namespace

int hdf_loss_blocks() { return LOSS_BLOCKS; }
size_t hdf_loss_workspace_floats(int N, int nscale) {
  return (size_t)nscale * N * LOSS_BLOCKS * NSTAT + 2 * (size_t)nscale * N * MAXC + (size_t)nscale * N + 16;
}

// geometry of the scales: nearest down-sampling by 2^i (combine_loss.py:68-79); D == 1: 2-D logits [N][C][H][W]
// (models/HDenseFormer_2D.py), the down-sampling then strides H and W only
static int loss_levels(const void* const* logits, void* const* dlogits, const float* target, int nscale, int D, int H,
                       int W, LossLevels& lv, LossScales& sc, int& blocks) {
  lv.nscale = nscale;
  int blk = 0;
  for (int i = 0; i < nscale; i++) {
    const int s = 1 << i;
    HDF_CHECK_ARG((D == 1 || D % s == 0) && H % s == 0 && W % s == 0, "loss: size not divisible by %d", s);
    HDF_CHECK_ARG((int64_t)D * H * W < ((int64_t)1 << 31) - 4096 * 256, "loss: %dx%dx%d voxels per sample", D, H, W);
    LossLevel& L = lv.L[i];
    L.logits = logits[i];
    L.dlogits = dlogits ? dlogits[i] : nullptr;
    L.Ds = D == 1 ? 1 : D / s, L.Hs = H / s, L.Ws = W / s, L.stride = s;
    const int64_t V = (int64_t)L.Ds * L.Hs * L.Ws;
    const uintptr_t al = reinterpret_cast<uintptr_t>(L.logits) | reinterpret_cast<uintptr_t>(L.dlogits) |
                         reinterpret_cast<uintptr_t>(target);
    L.vec = (L.Ws % 4 == 0 && (al & 15) == 0) ? 4 : 1;
    L.blk0 = blk;
    L.nblk = (int)std::min<int64_t>(std::max<int64_t>(ceil_div64(V, 256 * L.vec), 1), LOSS_BLOCKS);
    blk += L.nblk;
    sc.V[i] = (float)V;
    sc.weight[i] = 1.f / (float)s;
    sc.blocks[i] = L.nblk;
  }
  for (int i = nscale; i < 4; i++) lv.L[i] = lv.L[0], sc.V[i] = 0.f, sc.weight[i] = 0.f, sc.blocks[i] = 0;
  blocks = blk;
  return HDF_OK;
}

// fp == nullptr: the CE/Dice kernels (w_ce, class_weight of CEPlusDice); else the focal kernels with w_ce = w_focal
static int launch_loss_fwd(int dtype, const void* const* logits, const float* target, int nscale, int N, int C, int D,
                           int H, int W, float* ws, float* loss_out, hipStream_t st, float w_ce, float w_dice,
                           const float* class_weight, int dice_ignore, const FocalP* fp) {
  HDF_CHECK_ARG(C <= MAXC && C >= 2, "loss: n_cls=%d unsupported (2..%d)", C, MAXC);
  HDF_CHECK_ARG(dice_ignore >= -1 && dice_ignore < C, "loss: ignore_index %d outside [-1, %d)", dice_ignore, C);
  HDF_CHECK_ARG(nscale >= 1 && nscale <= 4 && nscale * N <= 256, "loss: nscale=%d N=%d", nscale, N);
  float* partials = ws;
  float* coefA = ws + (size_t)nscale * N * LOSS_BLOCKS * NSTAT;
  float* coefB = coefA + (size_t)nscale * N * MAXC;
  LossLevels lv;
  LossScales sc;
  int blocks = 0;
  HDF_TRY(loss_levels(logits, nullptr, target, nscale, D, H, W, lv, sc, blocks));
  HDF_DISPATCH_T(dtype, {
    if (fp && C <= 4)
      hipLaunchKernelGGL((focal_fwd_kernel<T, 4>), dim3(blocks, N), dim3(256), 0, st, lv, target, C, D, H, W, *fp,
                         partials);
    else if (fp)
      hipLaunchKernelGGL((focal_fwd_kernel<T, MAXC>), dim3(blocks, N), dim3(256), 0, st, lv, target, C, D, H, W, *fp,
                         partials);
    else if (C <= 4)
      hipLaunchKernelGGL((loss_fwd_kernel<T, 4>), dim3(blocks, N), dim3(256), 0, st, lv, target, C, D, H, W, class_weight,
                         partials);
    else
      hipLaunchKernelGGL((loss_fwd_kernel<T, MAXC>), dim3(blocks, N), dim3(256), 0, st, lv, target, C, D, H, W,
                         class_weight, partials);
  });
  HDF_LAUNCH_CHECK();
  float* terms = coefB + (size_t)nscale * N * MAXC;
  float* wsum = terms + (size_t)nscale * N;  // [nscale]: denominator of the cross-entropy mean (the 16 spare floats)
  if (fp)
    hipLaunchKernelGGL(focal_finalize_kernel, dim3(nscale * N), dim3(256), 0, st, partials, nscale, N, C, sc, 1e-5f, w_ce,
                       fp->mean, w_dice, class_weight, dice_ignore, terms, coefA, coefB);
  else
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(nscale * N), dim3(256), 0, st, partials, nscale, N, C, sc, 1e-5f, w_ce,
                       w_dice, class_weight, dice_ignore, terms, coefA, coefB, wsum);
  HDF_LAUNCH_CHECK();
  hipLaunchKernelGGL(loss_total_kernel, dim3(1), dim3(64), 0, st, terms, nscale * N, loss_out);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

static int launch_loss_bwd(int dtype, const void* const* logits, const float* target, int nscale, int N, int C, int D,
                           int H, int W, const float* ws, const float* grad_out, void* const* dlogits, hipStream_t st,
                           float w_ce, float w_dice, const float* class_weight, int dice_ignore, const FocalP* fp) {
  HDF_CHECK_ARG(nscale >= 1 && nscale <= 4, "loss: nscale=%d", nscale);
  LossBwdP q;
  q.coefA = ws + (size_t)nscale * N * LOSS_BLOCKS * NSTAT;
  q.coefB = q.coefA + (size_t)nscale * N * MAXC;
  q.wsum = q.coefB + (size_t)nscale * N * MAXC + (size_t)nscale * N;
  q.gup = grad_out, q.cw = fp ? nullptr : class_weight, q.w_ce = w_ce, q.w_dice = w_dice, q.ignore = dice_ignore;
  LossLevels lv;
  LossScales sc;
  int blocks = 0;
  HDF_TRY(loss_levels(logits, dlogits, target, nscale, D, H, W, lv, sc, blocks));
  HDF_DISPATCH_T(dtype, {
    if (fp && C <= 4)
      hipLaunchKernelGGL((focal_bwd_kernel<T, 4>), dim3(blocks, N), dim3(256), 0, st, lv, target, N, C, D, H, W, q, *fp);
    else if (fp)
      hipLaunchKernelGGL((focal_bwd_kernel<T, MAXC>), dim3(blocks, N), dim3(256), 0, st, lv, target, N, C, D, H, W, q,
                         *fp);
    else if (C <= 4)
      hipLaunchKernelGGL((loss_bwd_kernel<T, 4>), dim3(blocks, N), dim3(256), 0, st, lv, target, N, C, D, H, W, q);
    else
      hipLaunchKernelGGL((loss_bwd_kernel<T, MAXC>), dim3(blocks, N), dim3(256), 0, st, lv, target, N, C, D, H, W, q);
  });
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_launch_loss_fwd(int dtype, const void* const* logits, const float* target, int nscale, int N, int C, int D,
                        int H, int W, float* ws, float* loss_out, hipStream_t st, float w_ce, float w_dice,
                        const float* class_weight, int dice_ignore) {
  return launch_loss_fwd(dtype, logits, target, nscale, N, C, D, H, W, ws, loss_out, st, w_ce, w_dice, class_weight,
                         dice_ignore, nullptr);
}

int hdf_launch_loss_bwd(int dtype, const void* const* logits, const float* target, int nscale, int N, int C, int D,
                        int H, int W, const float* ws, const float* grad_out, void* const* dlogits, hipStream_t st,
                        float w_ce, float w_dice, const float* class_weight, int dice_ignore) {
  return launch_loss_bwd(dtype, logits, target, nscale, N, C, D, H, W, ws, grad_out, dlogits, st, w_ce, w_dice,
                         class_weight, dice_ignore, nullptr);
}

// gamma in (0, 1) is refused: the reference's pow backward gives NaN for a confidently right voxel there
static int focal_params(int C, float alpha, float gamma, int reduction, FocalP& fp) {
  HDF_CHECK_ARG(C <= MAXC && C >= 2, "focal loss: n_cls=%d unsupported (2..%d)", C, MAXC);
  HDF_CHECK_ARG(gamma == 0.f || gamma >= 1.f, "focal loss: gamma=%g unsupported (0 or >= 1)", (double)gamma);
  HDF_CHECK_ARG(alpha == alpha, "focal loss: alpha is NaN");
  HDF_CHECK_ARG(reduction == 0 || reduction == 1, "focal loss: reduction %d (0 sum, 1 mean)", reduction);
  fp.alpha = alpha, fp.gamma = gamma, fp.mean = reduction;
  return HDF_OK;
}

int hdf_launch_loss_focal_fwd(int dtype, const void* const* logits, const float* target, int nscale, int N, int C, int D,
                              int H, int W, float* ws, float* loss_out, hipStream_t st, float w_focal, float alpha,
                              float gamma, int reduction, float w_dice, const float* class_weight, int dice_ignore) {
  FocalP fp;
  HDF_TRY(focal_params(C, alpha, gamma, reduction, fp));
  return launch_loss_fwd(dtype, logits, target, nscale, N, C, D, H, W, ws, loss_out, st, w_focal, w_dice, class_weight,
                         dice_ignore, &fp);
}

int hdf_launch_loss_focal_bwd(int dtype, const void* const* logits, const float* target, int nscale, int N, int C, int D,
                              int H, int W, const float* ws, const float* grad_out, void* const* dlogits,
                              hipStream_t st, float w_focal, float alpha, float gamma, int reduction, float w_dice,
                              const float* class_weight, int dice_ignore) {
  FocalP fp;
  HDF_TRY(focal_params(C, alpha, gamma, reduction, fp));
  HDF_CHECK_ARG(dice_ignore >= -1 && dice_ignore < C, "loss: ignore_index %d outside [-1, %d)", dice_ignore, C);
  return launch_loss_bwd(dtype, logits, target, nscale, N, C, D, H, W, ws, grad_out, dlogits, st, w_focal, w_dice,
                         class_weight, dice_ignore, &fp);
}
