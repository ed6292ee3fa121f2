// The executor's transformer half: the launch sequences of the multi-path transformer branches (HDenseFormer.py:230) over a
// plan, forward and backward, as one persistent launch per direction or as the launch chain, and what a persistent launch
// that gave up leaves behind (the plan's status word, the NaN poison, the hdf_plan_chain_* entries).
#include <algorithm>
#include <cstring>

#include "exec_internal.h"

namespace {

// Tensor k of layer l of block b (modality 0; parameters or gradients) = base + blk0 + b * blk_stride + loff[l][k]: the
// plan's table (hdf_plan::tf_cp), which plan creation checked against the names.
TfLayerP tf_layer_ptrs(const hdf_plan* p, float* base, int b, int l) {
  float* q = base + p->tf_cp.blk0 + b * p->tf_cp.blk_stride;
  const int32_t* o = p->tf_cp.loff[l];
  return TfLayerP{q + o[0], q + o[1], q + o[2], q + o[3], q + o[4], q + o[5], q + o[6],
                  q + o[7], q + o[8], q + o[9], q + o[10], q + o[11], q + o[12]};
}
TfOutP tf_out_ptrs(const hdf_plan* p, float* base, int b) {
  float* q = base + p->tf_cp.blk0 + b * p->tf_cp.blk_stride;
  const int32_t* o = p->tf_cp.ooff;
  return TfOutP{q + o[0], q + o[1], q + o[2], q + o[3]};
}
TfLayerSave tf_save(const hdf_plan* p, const Exec& e, int b, int l) {
  const int64_t rows = (int64_t)p->M * e.B * p->Ntok;
  float* base = e.f(p->tf_save) + (int64_t)(b * 4 + l) * rows * 232;
  TfLayerSave s;
  s.h0 = base;
  s.qkv = base + rows * 32;
  s.ob = base + rows * 128;
  s.lse = base + rows * 160;
  s.h1 = base + rows * 168;
  s.h2 = base + rows * 200;
  return s;
}

TfChainCtl chain_ctl(const hdf_plan* p) {
  TfChainCtl c;
  c.host_flag = p->chain_flag_dev;
  c.ticks = p->chain_ticks;
  return c;
}

}  // namespace

namespace hdf_internal {

TfDims tf_dims(const hdf_plan* p, int B) {
  TfDims d;
  d.M = p->M;
  d.B = B;
  d.N = p->Ntok;
  d.DM = p->DM;
  d.DMF = p->DMF;
  d.mstride = p->mstride;
  d.training = p->training;
  d.seed = p->seed;
  d.thresh24 = 1u << 23;  // p = 0.5 (HDenseFormer.py:79,105)
  d.keep_scale = 2.0f;
  return d;
}

// The persistent kernels take the plan's transformer when every 16-token tile of every sequence gets a compute unit of
// its own (resident together: their per-sequence barriers need that).  HDF_NO_TF_CHAIN=1: the launch chain
// (tok_fwd / attention / tok_bwd ...) instead -- the third arrangement knob of tests/test_gpu_knobs.py.
// Decided ONCE per forward (forward3d stores the answer in p->tf_fwd_chain); the backward follows the forward it belongs
// to instead of reading the environment again (a knob flipped between the two calls made the persistent
// backward consume records the launch-chain forward never wrote).
bool tf_use_chain(const hdf_plan* p, int B) {
  const bool off = getenv("HDF_NO_TF_CHAIN") != nullptr;   // read per FORWARD call: tests switch it inside one process
  if (off || p->chain_off) return false;
  TfDims d = tf_dims(p, B);
  return p->chain_forced ? tf_chain_shape_ok(d) : tf_chain_supported(d);
}
// the plan's host-mapped give-up word, created on first use
int chain_flag_ensure(hdf_plan* p) {
  if (p->chain_flag) return HDF_OK;
  void* h = nullptr;
  if (hipHostMalloc(&h, 64, hipHostMallocMapped) != hipSuccess) {
    hdf_set_error("transformer chain: could not allocate the host-mapped status word");
    return HDF_ERR_HIP;
  }
  void* dv = nullptr;
  if (hipHostGetDevicePointer(&dv, h, 0) != hipSuccess) {
    (void)hipHostFree(h);
    hdf_set_error("transformer chain: no device address for the host-mapped status word");
    return HDF_ERR_HIP;
  }
  memset(h, 0, 64);
  p->chain_flag = reinterpret_cast<unsigned*>(h);
  p->chain_flag_dev = reinterpret_cast<unsigned*>(dv);
  return HDF_OK;
}
// Called at the top of every forward / backward: a persistent launch of an EARLIER call gave up at a barrier (the device
// was shared: its grid was not resident together within the deadline).  That call's outputs are NaN-poisoned garbage; this
// call reports it once -- HDF_ERR_CHAIN_TIMEOUT, nothing launched -- and the plan runs the launch chain from now on.
// (Asynchronous by nature: the host is ahead of the device, so the report can be one or more calls late; a caller that
// synchronises can ask at once with hdf_plan_chain_state.)
int chain_flag_check(hdf_plan* p) {
  if (!p->chain_flag) return HDF_OK;
  const unsigned v = __atomic_load_n(p->chain_flag, __ATOMIC_ACQUIRE);
  if (v == 0) return HDF_OK;
  __atomic_store_n(p->chain_flag, 0u, __ATOMIC_RELEASE);
  p->chain_last_giveup = v;
  p->chain_off = true;
  hdf_set_error("persistent transformer kernel: workgroup %u gave up at a per-sequence barrier (the compute units were not "
                "all available to the launch); the outputs of that call are NaN; this plan uses the launch chain from now on",
                v - 1);
  return HDF_ERR_CHAIN_TIMEOUT;
}

int transformer_forward(Exec& e, const float* x) {
  hdf_plan* p = e.p;
  TfDims d = tf_dims(p, e.B);
  float* pm = const_cast<float*>(e.params);
  const int64_t rows = (int64_t)p->M * e.B * p->Ntok;
  float* F0 = e.f(p->tf_F);
  const int PE_LP = p->dtype;
  // (flat: the 2-D input itself, depth 1, against depth slice 0 of the embedded 16^3 patch kernel)
  HDF_TRY(tf_patch_embed_fwd(d, x, p->flat ? 1 : p->D, p->H, p->W, pm + p->pe_w, pm + p->pe_b, pm + p->pe_pos, F0,
                             e.st, PE_LP, p->flat ? 1 : 16));
  if (p->tf_fwd_chain) {  // all layers of all blocks in one persistent launch (tf_chain_fwd.hip)
    if (e.tf_packed) HDF_TRY(e.wait(e.st, e.tf_packed, "the transformer's stream behind the weight packs"));
    return tf_chain_forward(d, p->tf_cp, p->nb, pm, F0, e.f(p->tf_save), e.at(p->attnall),
                            reinterpret_cast<unsigned*>(e.ws + p->tf_sync), e.ws + p->tf_wpack, e.f(p->tf_frag), p->dtype, e.st,
                            chain_ctl(p));
  }
  // token kernel, attention, token kernel, ...: between two attention launches ONE kernel finishes the previous
  // dense layer (and, at a block boundary, runs the block's out_layer) and starts the next one
  TfLayerP prev{}, cur{};
  TfOutP o{};
  for (int b = 0; b < p->nb; b++) {
    float* F = F0 + (int64_t)b * rows * p->DMF;
    for (int l = 0; l < 4; l++) {
      cur = tf_layer_ptrs(p, pm, b, l);
      TfTokenFwd t;
      if (l > 0) {
        t.post = &prev, t.post_save = tf_save(p, e, b, l - 1), t.bp = b, t.lp = l - 1, t.F_post = F;
      } else if (b > 0) {
        float* Fp = F0 + (int64_t)(b - 1) * rows * p->DMF;
        t.post = &prev, t.post_save = tf_save(p, e, b - 1, 3), t.bp = b - 1, t.lp = 3, t.F_post = Fp;
        o = tf_out_ptrs(p, pm, b - 1);
        t.out = &o, t.next_F = F;
      }
      t.pre = &cur, t.pre_save = tf_save(p, e, b, l), t.bq = b, t.lq = l, t.F_pre = F;
      HDF_TRY(tf_token_fwd(d, t, p->dtype, e.st));
      TfLayerSave s = tf_save(p, e, b, l);
      HDF_TRY(tf_attention_fwd(d.N, d.M * d.B, s.qkv, s.ob, s.lse, e.st));
      prev = cur;
    }
  }
  TfTokenFwd t;
  const int b = p->nb - 1;
  t.post = &prev, t.post_save = tf_save(p, e, b, 3), t.bp = b, t.lp = 3, t.F_post = F0 + (int64_t)b * rows * p->DMF;
  o = tf_out_ptrs(p, pm, b);
  t.out = &o, t.attnall = e.at(p->attnall);
  return tf_token_fwd(d, t, p->dtype, e.st);
}

int transformer_backward(Exec& e, const float* x) {
  hdf_plan* p = e.p;
  TfDims d = tf_dims(p, e.B);
  float* pm = const_cast<float*>(e.params);
  const int64_t rows = (int64_t)p->M * e.B * p->Ntok;
  float* F0 = e.f(p->tf_F);
  float* dF = e.f(p->tf_dF);
  float* scratch = e.f(p->tf_scratch);
  // token kernel, attention backward, token kernel, ...: one launch runs the Linear0 / LN1 / to_qkv backward of the
  // layer whose attention backward just finished, (at a block boundary) the previous block's out_layer backward, and
  // the ff / to_out backward of the next layer down
  float* dO = scratch;
  float* dh0acc = scratch + rows * 32;
  float* dqkv = scratch + rows * 64;
  // Every weight-matrix gradient of the branches comes from the tapes the token kernels leave behind (fixed-order
  // reductions, no atomics): one launch per block, issued on the side stream as soon as that block's last tape segment
  // is written (the token kernel that also starts the next block down), so that only block 0's -- next to the patch
  // embedding's -- is left at the end of the chain.  (One launch for all blocks after the chain: 114 us with nothing
  // else left to run beside it.)
  TfWgradArgs w{};
  std::copy(p->tf_wg, p->tf_wg + TF_WG_ENTRIES, w.e);
  w.grads = e.grads, w.mstride = p->mstride, w.block0 = p->tf_cp.blk0, w.block_stride = p->tf_cp.blk_stride;
  w.tape = e.f(p->tf_tape), w.otape = e.f(p->tf_otape), w.F = F0, w.save = e.f(p->tf_save);
  w.rows = rows, w.BN = e.B * p->Ntok, w.DMF = p->DMF, w.b0 = 0;
  auto wgrad_block = [&](int b) -> int {
    w.b0 = b;
    HDF_TRY(tf_wgrad(w, 1, p->M, e.wgrad_stream()));
    return e.side_done();
  };
  auto patch_embed_bwd = [&]() -> int {
    return tf_patch_embed_bwd(d, x, p->flat ? 1 : p->D, p->H, p->W, dF, e.grads + p->pe_w, e.grads + p->pe_b,
                              e.grads + p->pe_pos, scratch, e.st, p->flat ? 1 : 16);
  };
  p->tf_bwd_chain = p->tf_fwd_chain && tf_chain_backward_supported(d, p->dtype);
  if (p->tf_bwd_chain) {
    // one persistent launch for all layers (tf_chain_bwd.hip); then every block's weight-matrix gradients from the
    // tapes on the side stream, next to the patch embedding's backward on this one
    HDF_TRY(tf_chain_backward(d, p->tf_cp, p->nb, pm, e.grads, F0, e.f(p->tf_save), dF, e.at(p->dAttnall),
                              e.f(p->tf_tape), e.f(p->tf_otape), scratch, e.f(p->tf_frag), e.ws + p->tf_wpack,
                              reinterpret_cast<unsigned*>(e.ws + p->tf_sync) + (1 << 17), p->dtype, e.st, chain_ctl(p)));
    // (on this stream, not on the side stream: that one still holds the level-0 weight gradients, and tf_wgrad -- HBM-bound,
    // 110 us -- would run behind them as the last kernel of the step)
    HDF_TRY(patch_embed_bwd());
    w.b0 = 0;
    HDF_TRY(tf_wgrad(w, p->nb, p->M, e.st));
    return HDF_OK;
  }
  TfLayerP up{}, gup{}, cur{}, gcur{};
  TfOutP o{}, go{};
  bool have_up = false;
  int ub = 0, ul = 0;
  for (int b = p->nb - 1; b >= 0; b--) {
    float* F = F0 + (int64_t)b * rows * p->DMF;
    for (int l = 3; l >= 0; l--) {
      cur = tf_layer_ptrs(p, pm, b, l);
      gcur = tf_layer_ptrs(p, e.grads, b, l);
      TfTokenBwd t;
      t.dF = dF;
      float* tape = e.f(p->tf_tape);
      float* otape = e.f(p->tf_otape);
      if (have_up) {
        t.pre = &up, t.pre_grad = &gup, t.pre_save = tf_save(p, e, ub, ul), t.bq = ub, t.lq = ul;
        t.F_pre = F0 + (int64_t)ub * rows * p->DMF, t.dqkv = dqkv, t.dh0acc = dh0acc;
        if (tape) t.tape_pre = tape + (int64_t)(ub * 4 + ul) * rows * TF_TAPE_W;
      }
      if (l == 3) {
        o = tf_out_ptrs(p, pm, b);
        go = tf_out_ptrs(p, e.grads, b);
        t.out = &o, t.out_grad = &go, t.bo = b, t.F_out = F;
        if (!have_up) t.d_attnall = e.at(p->dAttnall);
        if (otape) t.tape_out = otape + (int64_t)b * rows * p->DMF;
      }
      t.post = &cur, t.post_grad = &gcur, t.post_save = tf_save(p, e, b, l), t.bp = b, t.lp = l;
      if (tape) t.tape_post = tape + (int64_t)(b * 4 + l) * rows * TF_TAPE_W;
      t.dO = dO, t.dh0acc_out = dh0acc;
      HDF_TRY(tf_token_bwd(d, t, p->dtype, e.st));
      if (have_up && l == 3) HDF_TRY(wgrad_block(ub));  // block b + 1 is complete
      TfLayerSave s = tf_save(p, e, b, l);
      HDF_TRY(tf_attention_bwd(d.N, d.M * d.B, s.qkv, s.ob, s.lse, dO, dqkv, e.st, p->dtype));
      up = cur, gup = gcur, ub = b, ul = l, have_up = true;
    }
  }
  TfTokenBwd t;
  t.dF = dF, t.pre = &up, t.pre_grad = &gup, t.pre_save = tf_save(p, e, 0, 0), t.bq = 0, t.lq = 0, t.F_pre = F0;
  t.dqkv = dqkv, t.dh0acc = dh0acc;
  t.tape_pre = e.f(p->tf_tape);
  HDF_TRY(tf_token_bwd(d, t, p->dtype, e.st));
  HDF_TRY(wgrad_block(0));
  return patch_embed_bwd();
}

}  // namespace hdf_internal

// A persistent transformer launch that gave up (tf_chain.h: chain_wait) leaves 1 + a workgroup id in its timeout
// word.  NaN written into the branch output does NOT survive the network -- relu(InstanceNorm(.)) is fmaxf(x * scale +
// shift, 0), and fmaxf returns the operand that is not NaN -- so the step would end with finite, plausible-looking logits
// and gradients.  These two launches (one workgroup each, the LAST launch of a forward / of a backward on the caller's
// stream, only when the persistent kernels ran) make the failure visible in the data itself: the first rows of every output
// / the head of the flat gradient buffer become NaN, so the loss, and the optimizer step, are NaN.
template <typename T>
__global__ void chain_poison_outputs_kernel(const unsigned* __restrict__ tmo, T* o0, T* o1, T* o2, T* o3, int n0, int n1,
                                            int n2, int n3) {
  if (__hip_atomic_load(tmo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) return;
  T* o[4] = {o0, o1, o2, o3};
  const int n[4] = {n0, n1, n2, n3};
  for (int k = 0; k < 4; k++)
    for (int i = threadIdx.x; i < n[k]; i += blockDim.x) ST<T>::st(o[k] + i, __builtin_nanf(""));
}
__global__ void chain_poison_grads_kernel(const unsigned* __restrict__ tmo, float* grads, int n) {
  if (__hip_atomic_load(tmo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) return;
  for (int i = threadIdx.x; i < n; i += blockDim.x) grads[i] = __builtin_nanf("");
}


namespace hdf_internal {

int chain_poison_outputs(Exec& e, void* const outs[4]) {
  hdf_plan* p = e.p;
  const unsigned* tmo = reinterpret_cast<const unsigned*>(e.ws + p->tf_sync) + p->M * e.B * 32;
  int n[4];
  for (int i = 0; i < 4; i++) n[i] = (int)std::min<int64_t>(p->vox(i) * p->ncls * e.B, 4096);
  HDF_DISPATCH_T(p->dtype, hipLaunchKernelGGL(chain_poison_outputs_kernel<T>, dim3(1), dim3(256), 0, e.st, tmo, (T*)outs[0],
                                              (T*)outs[1], (T*)outs[2], (T*)outs[3], n[0], n[1], n[2], n[3]));
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

// (the persistent backward's timeout word: the second half of the counters)
int chain_poison_grads(Exec& e) {
  hdf_plan* p = e.p;
  const unsigned* tmo = reinterpret_cast<const unsigned*>(e.ws + p->tf_sync) + (1 << 17) + p->M * e.B * 32;
  hipLaunchKernelGGL(chain_poison_grads_kernel, dim3(1), dim3(256), 0, e.st, tmo, e.grads,
                     (int)std::min<int64_t>(p->total_floats, 4096));
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

}  // namespace hdf_internal

extern "C" {

int hdf_plan_set_chain_timeout_us(hdf_plan* p, int64_t usec) {
  HDF_CHECK_ARG(p && usec >= 100 && usec <= 30000000, "plan_set_chain_timeout_us: 100 us .. 30 s");
  p->chain_ticks = (unsigned)(usec * 100);   // s_memrealtime: 100 MHz
  return HDF_OK;
}

int hdf_plan_force_persistent(hdf_plan* p, int on) {
  HDF_CHECK_ARG(p != nullptr, "plan_force_persistent: null plan");
  p->chain_forced = on != 0;
  return HDF_OK;
}

int hdf_plan_chain_state(hdf_plan* p, int batch, int* persistent, int* gave_up_workgroup) {
  HDF_CHECK_ARG(p && batch >= 1, "plan_chain_state: null plan / batch < 1");
  // (reads the host-mapped word like the next forward would, without consuming it: that call still reports the error)
  const unsigned pending = p->chain_flag ? __atomic_load_n(p->chain_flag, __ATOMIC_ACQUIRE) : 0u;
  if (gave_up_workgroup) *gave_up_workgroup = pending ? (int)pending - 1 : (p->chain_last_giveup ? (int)p->chain_last_giveup - 1 : -1);
  if (persistent) *persistent = (!pending && tf_use_chain(p, batch)) ? 1 : 0;
  return HDF_OK;
}

}  // extern "C"
