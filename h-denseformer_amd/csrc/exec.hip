// The executor: the forward / backward launch sequences of HDenseFormer.forward (HDenseFormer.py:229-255) and its
// autograd over a plan (plan.hip), around the transformer branches' own sequences (exec_tf.hip).
#include <algorithm>

#include "exec_internal.h"
#include "unet_ops.h"

namespace {

// The launch block of a 3x3x3 convolution `in` (Cin channels) -> `out` (Cout channels) with the packed weights at workspace
// offset `w`: stride 1, stride 2 or transposed by the levels the two views live at.  The callers add what differs (bias,
// Xf, statistics table, bs_*, split, budget, priority).
ConvArgs conv_args(const Exec& e, const View& in, int Cin, const View& out, int Cout, size_t w, int wfrag) {
  const int *di = e.dm(in.lvl), *dO = e.dm(out.lvl);
  ConvArgs a{};
  a.in = e.at(in), a.in_pitch = in.pitch, a.Cin = Cin;
  a.N = e.B;
  a.Di = di[0], a.Hi = di[1], a.Wi = di[2];
  a.Do = dO[0], a.Ho = dO[1], a.Wo = dO[2];
  a.w = e.ws + w, a.wfrag = wfrag;
  a.out = e.at(out), a.out_pitch = out.pitch, a.Cout = Cout, a.CoutP = round_up(Cout, 32);
  return a;
}
// the same for a weight gradient: `sm` (SC channels) is the tensor at the lower or equal resolution
WgradArgs wgrad_args(const Exec& e, const View& sm, int SC, const View& lg, int LC) {
  const int *ds = e.dm(sm.lvl), *dl = e.dm(lg.lvl);
  WgradArgs w{};
  w.sm = e.at(sm), w.sm_pitch = sm.pitch, w.SC = SC;
  w.lg = e.at(lg), w.lg_pitch = lg.pitch, w.LC = LC;
  w.N = e.B;
  w.Ds = ds[0], w.Hs = ds[1], w.Ws = ds[2];
  w.Dl = dl[0], w.Hl = dl[1], w.Wl = dl[2];
  return w;
}

// probe: record the plan's probe events immediately around the convolution launch (hdf_plan_set_probe)
int conv_forward(Exec& e, Conv3& c, const View& in, Xf xf, bool probe = false) {
  hdf_plan* p = e.p;
  const int* d = e.dm(c.lvl);
  ConvArgs a = conv_args(e, in, c.CinP, c.y, c.Cout, c.wf, c.wf_frag);  // weights: packed by hdf_forward's pack batch
  a.prio = e.on_branch;  // the UpConv chain's convolutions run next to the encoder's persistent ones (ConvArgs::prio)
  a.cu_budget = e.conv_budget;
  a.bias = e.P(c.b);
  a.in_scale = xf.scale, a.in_shift = xf.shift, a.in_relu = xf.relu;
  a.stat_partials = e.statp();
  a.kpart = e.kspl(), a.kpart_bytes = HDF_KSPLIT_BYTES;
  // the encoder's first layer (<= 4 real channels in a 16-channel row): K = (tap, channel), csrc/conv_first.hip
  if (c.Cin <= 4 && !xf.scale && hdf_conv_first_takes(p->dtype, c.Cin, c.Cout, d[0], d[1], d[2], in.pitch)) {
    HDF_TRY(hdf_launch_conv_first(p->dtype, e.at(in), in.pitch, c.Cin, e.B, d[0], d[1], d[2], e.P(c.w), e.P(c.b),
                                  e.at(c.y), c.y.pitch, c.Cout, e.statp(), e.st));
  } else {
    const bool pr = probe && p->probe_start && p->probe_stop;
    if (pr && hipEventRecord(p->probe_start, e.st) != hipSuccess) {
      hdf_set_error("probe: hipEventRecord failed");
      return HDF_ERR_HIP;
    }
    HDF_TRY(hdf_launch_conv(p->dtype, 0, a, e.st));
    if (pr && hipEventRecord(p->probe_stop, e.st) != hipSuccess) {
      hdf_set_error("probe: hipEventRecord failed");
      return HDF_ERR_HIP;
    }
  }
  int tiles = hdf_conv_stat_tiles(0, d[0], d[1], d[2], c.CinP * p->esz);
  HDF_TRY(hdf_launch_in_finalize(e.statp(), e.B, tiles, c.Cout, a.CoutP, p->vox(c.lvl), e.P(c.gamma),
                                 e.P(c.beta), 1e-5f, e.norm(c.st), e.st));
  return HDF_OK;
}

int convt_forward(Exec& e, ConvT3& t, const View& in, Xf xf, const View& out) {
  ConvArgs a = conv_args(e, in, t.Cin, out, t.Cout, t.wf, t.wf_frag);
  a.bias = e.P(t.b);
  a.in_scale = xf.scale, a.in_shift = xf.shift, a.in_relu = xf.relu;
  return hdf_launch_conv(e.p->dtype, 2, a, e.st);
}

int head_forward(Exec& e, const Head1& h, const View& in, Xf xf, void* out) {
  return hdf_launch_head_fwd(e.p->dtype, e.rows(in), NormStats{xf.scale, xf.shift}, e.P(h.w), e.P(h.b), out, e.B, h.C,
                             e.p->ncls, e.p->vox(h.lvl), e.st);
}

// InstanceNorm(+ReLU) backward of conv layer c: da (grad w.r.t. the activation) -> dy (grad w.r.t. raw conv out)
struct InBwd {
  int pre_blocks = 0;     // > 0: the producer of da already wrote that many partial rows per sample into e.inbp()
  bool apply = true;      // false: only the statistics passes (k1 / ka / kb); the consumer applies them itself
  float* kbuf = nullptr;  // where k1 | ka | kb go (default: the Exec's scratch, overwritten by its next in_backward)
};
int in_backward(Exec& e, const Conv3& c, const View& da, const View& dy, const InBwd& o = InBwd{}) {
  hdf_plan* p = e.p;
  const int64_t vox = p->vox(c.lvl);
  const int blocks = o.pre_blocks > 0 ? o.pre_blocks : hdf_in_bwd_blocks(vox, c.Cout);
  float* k = o.kbuf ? o.kbuf : e.inbk();
  const InBwdCoefOut coef{k, k + (size_t)e.B * c.Cout, k + (size_t)2 * e.B * c.Cout};
  if (o.pre_blocks == 0)
    HDF_TRY(hdf_launch_in_bwd_reduce(p->dtype, e.rows(da), e.rows(c.y), e.norm(c.st), e.inbp(), blocks, e.B, c.Cout, vox,
                                     e.st));
  HDF_TRY(hdf_launch_in_bwd_finalize(e.inbp(), blocks, e.B, c.Cout, vox, e.P(c.gamma), e.f(c.st.rstd), coef,
                                     e.G(c.gamma), e.G(c.beta), e.st));
  if (!o.apply) return HDF_OK;
  e.wait_readers(dy);  // a side-stream weight gradient may still read this buffer's previous contents
  return hdf_launch_in_bwd_apply(p->dtype, e.rows(da), e.rows(c.y), e.norm(c.st), coef, e.rows(dy), e.B, c.Cout, vox, e.st);
}

// ap: dy has NOT been written yet.  ap->da is the gradient w.r.t. c's activation and in_backward(.., apply = false) has
// left k1 | ka | kb at ap->k: the weight-gradient launch applies the second pass of the InstanceNorm backward to the rows it
// stages and writes dy as it goes (WgradArgs::ap_*); this stream waits for it before the data gradient.
struct InApply {
  const View* da;
  const float* k;
};
// conv backward: the weight gradient from (dy, input) and, with `din`, the input gradient.  Every field is optional.
// din_colsum: taken from the dgrad conv's own InstanceNorm-partials epilogue (fp32 accumulators): the bias gradient of the
// ConvTranspose3d that produced those channels, without a pass over the tensor.
// bs_next / bs_rows: where the data-gradient launch can (hdf_conv_bwd_stats_ok) its epilogue writes the first pass of
// bs_next's InstanceNorm(+ReLU) backward into e.inbp(); *bs_rows is then the next in_backward's pre_blocks, else 0.
struct ConvBwd {
  const View* din = nullptr;       // where the input gradient goes (null: none is computed)
  int accumulate = 0;              // 1: it is added to *din
  const View* din2 = nullptr;      // input channels [0, din->C) -> din, the rest -> din2 (two dense buffers of one pitch)
  float* din_colsum = nullptr;     // += per-channel sums over (sample, voxel) of the input gradient's first ...
  int colsum_C = 0;                // ... colsum_C channels
  const Conv3* bs_next = nullptr;  // the conv whose InstanceNorm(+ReLU) backward consumes *din next
  int* bs_rows = nullptr;          // <- rows per sample of that backward's first pass the data gradient left (0: none)
  int pre_blocks = 0;              // norm_conv_backward: InBwd::pre_blocks of c's own InstanceNorm backward
  const InApply* ap = nullptr;     // conv_backward: see InApply
};
// the weight-gradient launch of conv layer c (without the fused pass)
static WgradArgs conv_wgrad_args(Exec& e, const Conv3& c, const View& dy, const View& in, Xf xf) {
  WgradArgs w = wgrad_args(e, dy, c.Cout, in, c.CinP);
  w.lg_scale = xf.scale, w.lg_shift = xf.shift, w.lg_relu = xf.relu;
  return w;
}
static void wgrad_args_apply(WgradArgs& w, Exec& e, const Conv3& c, const View& dy, const InApply& ap) {
  w.sm = e.at(*ap.da);
  w.sm_pitch = ap.da->pitch;
  w.ap_y = e.at(c.y);
  w.ap_y_pitch = c.y.pitch;
  w.ap_out = e.at(dy);
  w.ap_out_pitch = dy.pitch;
  w.ap_tab[0] = e.f(c.st.scale), w.ap_tab[1] = e.f(c.st.shift), w.ap_tab[2] = e.f(c.st.mean), w.ap_tab[3] = e.f(c.st.rstd);
  w.ap_tab[4] = ap.k, w.ap_tab[5] = ap.k + (size_t)e.B * c.Cout, w.ap_tab[6] = ap.k + (size_t)2 * e.B * c.Cout;
}

int conv_backward(Exec& e, Conv3& c, const View& dy, const View& in, Xf xf, const ConvBwd& o) {
  hdf_plan* p = e.p;
  const int* d = e.dm(c.lvl);
  const InApply* ap = o.ap;  // (norm_conv_backward decides it)
  WgradArgs w = conv_wgrad_args(e, c, dy, in, xf);
  if (ap) wgrad_args_apply(w, e, c, dy, *ap);
  // the encoder's first layer: K = (tap, channel) from the other side, csrc/conv_first.hip
  if (!ap && c.Cin <= 4 && !xf.scale &&
      hdf_wgrad_first_takes(p->dtype, c.Cin, c.Cout, d[0], d[1], d[2], in.pitch, dy.pitch)) {
    HDF_TRY(hdf_launch_wgrad_first(p->dtype, e.at(dy), dy.pitch, c.Cout, e.at(in), in.pitch, c.Cin, e.B, d[0], d[1], d[2],
                                   e.G(c.w), 0, e.ws + p->wgrad_ws, p->wgrad_ws_bytes, e.wgrad_stream()));
  } else
  HDF_TRY(hdf_launch_wgrad(p->dtype, 1, w, e.G(c.w), c.Cout, c.Cin, 0, e.ws + p->wgrad_ws, p->wgrad_ws_bytes,
                           e.wgrad_stream()));
  HDF_TRY(e.wgrad_done(dy));
  // (the side stream runs its launches in order, so the earlier readers of dy's previous contents are done before this
  // launch writes it; the data gradient below is the first reader of the new contents)
  if (ap) e.wait_readers(dy);
  // Conv3 layers with a bias are the UpConvs (HDenseFormer.py:162-175): conv(bias) -> InstanceNorm3d(affine=False).
  // The norm subtracts the per-(sample, channel) mean, so dL/dbias = sum_voxels dy is identically zero (the reference
  // accumulates ~3e-8 of rounding noise there); the gradient buffer was zeroed at the start of backward,
  // so the four reduction passes over dy are simply not run.
  if (o.din) {
    // dgrad = the same conv with taps reversed and channel roles swapped: Wd[t][ci][co] = W[co][ci][26-t]
    ConvArgs a = conv_args(e, dy, c.Cout, *o.din, c.Cin, c.wd, c.wd_frag);
    a.prio = e.on_branch;
    a.accumulate = o.accumulate;
    if (o.din2) {
      a.out2 = e.at(*o.din2);
      a.split = o.din->C;
    }
    if (o.din_colsum) a.stat_partials = e.statp();  // forward scratch, free during backward
    a.kpart = e.kspl(), a.kpart_bytes = HDF_KSPLIT_BYTES;
    if (o.bs_rows) *o.bs_rows = 0;
    if (o.bs_next && o.bs_rows && !o.din_colsum && !o.din2) {
      const Conv3& n = *o.bs_next;
      ConvArgs b = a;
      b.stat_partials = e.inbp();
      b.bs_y = e.at(n.y), b.bs_y_pitch = n.y.pitch;
      b.bs_scale = e.f(n.st.scale), b.bs_shift = e.f(n.st.shift);
      b.bs_mean = e.f(n.st.mean), b.bs_rstd = e.f(n.st.rstd);
      if (n.Cout == a.Cout && hdf_conv_bwd_stats_ok(p->dtype, b)) {
        a = b;
        *o.bs_rows = hdf_conv_stat_tiles(0, d[0], d[1], d[2], a.Cin * p->esz);
      }
    }
    HDF_TRY(hdf_launch_conv(p->dtype, 0, a, e.st));
    if (o.din_colsum) {
      const int rows = e.B * hdf_conv_stat_tiles(0, d[0], d[1], d[2], a.Cin * p->esz);
      HDF_TRY(hdf_launch_stat_rows_sum(e.statp(), rows, o.colsum_C, a.CoutP, o.din_colsum, e.st));
    }
  }
  return HDF_OK;
}

// InstanceNorm(+ReLU) backward of conv layer c followed by the conv's own backward (in_backward + conv_backward).  Where the
// weight-gradient launch can take the norm's second pass along (16-bit stride-1 layers: conv_wgrad2_kernel<., ., true>) that
// pass need not run on its own: one launch, the read of d(activation) + y and the write + re-read of dy by a pass that does
// nothing else (in_bwd_apply4 at 128^3 x 32 channels: 86 us alone, 165 us inside the step, three times per step).
// Measured (round 5, same box, interleaved, bench geometry):
//   one stream, sum of kernel times: -0.27 ms with every level fused (apply -0.60 ms, weight gradients +0.33 ms: the pass
//     costs ~400 VALU instructions per tile and wave in a kernel with ONE wave per SIMD);
//   the step (three streams), when this was built: fused at 128^3 only 10.88 ms, not fused 10.90 ms, fused at >= 64^3
//     11.06 ms (6 rounds each); under the round's final schedule (light kernels prioritised, forward reordered): 10.42 vs
//     10.55 vs 10.60 ms, and 10.83 ms at >= 32^3 (7-8 rounds each, medians).  The stand-alone pass is HBM-bound and runs
//     UNDER the matrix kernels of the other streams; fused, its work sits in the matrix kernels' instruction stream, and the
//     data gradient waits for the weight gradient (i.e. for whatever the side stream still holds) -- at 128^3 x 32 channels
//     the saved traffic wins, at the smaller levels (more channels: every voxel's pass is redone per large-channel block) it
//     does not.
// So the default fuses the 128^3 layers only (0.8 GB of the step's HBM traffic and three launches less, -0.13 ms); HDF_FUSED_APPLY_MIN_VOX (environment, voxels per sample) moves the threshold, HDF_NO_FUSED_APPLY switches the
// fused form off.  The UpConv chain on the branch stream (the critical path) always keeps the stand-alone pass.
static int64_t fused_apply_min_vox() {
  static const int64_t v = [] {
    const char* s = getenv("HDF_FUSED_APPLY_MIN_VOX");
    return s ? (int64_t)atoll(s) : (int64_t)128 * 128 * 128;
  }();
  return v;
}
int norm_conv_backward(Exec& e, Conv3& c, const View& da, const View& dy, const View& in, Xf xf, ConvBwd o) {
  static const bool off = getenv("HDF_NO_FUSED_APPLY") != nullptr;  // A/B knob (tests/test_gpu_knobs.py)
  hdf_plan* p = e.p;
  const int* d = e.dm(c.lvl);
  InApply ap{&da, e.inbk()};
  bool fuse = !off && !e.on_branch && p->vox(c.lvl) >= fused_apply_min_vox();
  if (fuse) {
    if (c.Cin <= 4 && !xf.scale && hdf_wgrad_first_takes(p->dtype, c.Cin, c.Cout, d[0], d[1], d[2], in.pitch, dy.pitch))
      fuse = false;  // the first layer's own kernel
    WgradArgs w = conv_wgrad_args(e, c, dy, in, xf);
    wgrad_args_apply(w, e, c, dy, ap);
    fuse = fuse && hdf_wgrad_apply_takes(p->dtype, 1, w);
  }
  InBwd ib;
  ib.pre_blocks = o.pre_blocks, ib.apply = !fuse;
  HDF_TRY(in_backward(e, c, da, dy, ib));
  o.ap = fuse ? &ap : nullptr;
  return conv_backward(e, c, dy, in, xf, o);
}

// ConvTranspose3d backward: dOut (hi-res) -> dIn (lo-res, grad w.r.t. the activation fed to the convT)
int convt_backward(Exec& e, ConvT3& t, const View& dout, const View& in, Xf xf, const View& din) {
  hdf_plan* p = e.p;
  // (the bias gradient comes out of the epilogue of the dgrad conv that produced dout: conv_backward)
  WgradArgs w = wgrad_args(e, in, t.Cin, dout, t.Cout);
  w.sm_scale = xf.scale, w.sm_shift = xf.shift, w.sm_relu = xf.relu;
  HDF_TRY(hdf_launch_wgrad(p->dtype, 2, w, e.G(t.w), t.Cin, t.Cout, 0, e.ws + p->wgrad_ws, p->wgrad_ws_bytes,
                           e.wgrad_stream()));
  HDF_TRY(e.wgrad_done(dout));
  // dX[i][ci] = sum_k sum_co dY[2i-1+k][co] * W[ci][co][k]  -> stride-2 gather conv, packed [tap][CinP][Cout]
  return hdf_launch_conv(p->dtype, 1, conv_args(e, dout, t.Cout, din, t.Cin, t.wd, t.wd_frag), e.st);
}

struct HeadBwd {
  int accumulate = 0;               // 1: the input gradient is added to dx
  // fuse_in: the conv layer whose InstanceNorm+ReLU output the head reads -- the head gradient is then that activation's
  // complete gradient, and the kernel also writes the first pass of the layer's InstanceNorm backward (*pre_blocks rows
  // per sample in inb_partials; 0 when the table does not hold that many rows and the separate pass has to run)
  const Conv3* fuse_in = nullptr;
  int* pre_blocks = nullptr;
};
int head_backward(Exec& e, const Head1& h, const void* dlogits, const View& in, Xf xf, const View& dx, const HeadBwd& o) {
  hdf_plan* p = e.p;
  const int hb = hdf_head_bwd_blocks(p->vox(h.lvl));
  const bool fuse = o.fuse_in && o.pre_blocks && hb <= 1024;
  if (o.pre_blocks) *o.pre_blocks = fuse ? hb : 0;
  NormStats ins{xf.scale, xf.shift};
  HeadGrads g{e.rows(dx), o.accumulate, e.G(h.w), e.G(h.b)};
  if (fuse) ins.mean = e.f(o.fuse_in->st.mean), ins.rstd = e.f(o.fuse_in->st.rstd), g.inb_partials = e.inbp();
  return hdf_launch_head_bwd(p->dtype, dlogits, e.rows(in), ins, e.P(h.w), g, e.B, h.C, p->ncls, p->vox(h.lvl), e.st);
}

}  // namespace

// Stand-in for a collective's kernel (tests / tools): `workgroups` workgroups of 256 threads that each hold `lds_bytes` of
// LDS (160 KiB = a compute unit of its own) and `vgprs` vector registers per lane (0: a handful; 128: what a RCCL
// all-reduce kernel holds -- next to it a 304-register conv wave still fits a SIMD, a 512-register conv_wr wave or the
// two 252-register waves of a persistent transformer workgroup do not), spinning on the 100 MHz real-time counter for `usec`.
template <bool FAT>
__global__ __launch_bounds__(256) void occupy_kernel(unsigned ticks) {
  extern __shared__ char occ_lds[];
  if (threadIdx.x == 0) occ_lds[0] = 1;
  if (FAT) asm volatile("v_mov_b32 v127, 0" ::: "v127");   // forces an allocation of 128 VGPRs
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < (uint64_t)ticks) __builtin_amdgcn_s_sleep(8);
}

// ---- UpConv chain backward: at3 <- up3 <- at2 <- up2 <- at1 <- up1 <- attnout <- deep_conv <- attnall
static int upconv_chain_backward(Exec& e, int batch) {
  hdf_plan* p = e.p;
  Xf none;
  for (int k = 2; k >= 0; k--) {
    Conv3& c = p->up[k];                                   // up[k] output level c.lvl, upsampled to level c.lvl-1
    View dat = p->dSkip[c.lvl - 1];  // gradient of at_{..} == of ds
    View& da = p->dUa[4 - c.lvl];
    View& dy = p->dUy[4 - c.lvl];
    HDF_TRY(hdf_launch_upsample_bwd(p->dtype, e.rows(dat), e.rows(da), e.extent(c.lvl, c.Cout), e.st));
    HDF_TRY(in_backward(e, c, da, dy));
    // input of up[k]: attnout (k==0) or at_{lvl} ; its gradient buffer already holds the skip-path gradient
    const View& cin = (k == 0) ? p->attnout : p->at[c.lvl];
    View din = (k == 0) ? p->dX4 : p->dSkip[c.lvl];
    ConvBwd o;
    o.din = &din, o.accumulate = 1;
    HDF_TRY(conv_backward(e, c, dy, cin, none, o));
  }
  {
    Conv3& c = p->deep;
    HDF_TRY(hdf_launch_upsample_bwd(p->dtype, e.rows(p->dX4), e.rows(p->dUa[0]), e.extent(4, c.Cout), e.st));
    HDF_TRY(in_backward(e, c, p->dUa[0], p->dUy[0]));
    ConvBwd o;
    o.din = &p->dAttnall;
    HDF_TRY(conv_backward(e, c, p->dUy[0], p->attnall, none, o));
  }
  return HDF_OK;
}

static int forward3d(hdf_plan* p, const float* x, const float* params, void* workspace, int64_t workspace_bytes,
                     void* out0, void* out1, void* out2, void* out3, int batch, int training, uint64_t seed,
                     hdf_stream stream) {
  hdf_plan_layout(p, batch);
  HDF_CHECK_ARG((size_t)workspace_bytes >= p->ws_fwd_bytes, "forward: workspace %lld < %zu bytes",
                (long long)workspace_bytes, p->ws_fwd_bytes);
  HDF_TRY(chain_flag_check(p));
  p->training = training ? 1 : 0;
  p->seed = (uint32_t)(seed & 0xffffffffu);
  p->tf_fwd_chain = tf_use_chain(p, batch);
  if (p->tf_fwd_chain) HDF_TRY(chain_flag_ensure(p));
  Exec e{p, (char*)workspace, params, nullptr, batch, (hipStream_t)stream};
  const int nf = p->nf;
  const int ch[4] = {nf, 2 * nf, 4 * nf, 8 * nf};
  void* outs[4] = {out0, out1, out2, out3};
  Xf none;

  // ---- multi-path transformer (HDenseFormer.py:230) -> attnall, then the UpConv chain (:231-235).  Nothing on the
  // encoder's first level depends on it before ds0 = block_1_2_left(..) + at3 (:238), and it is ~100 launches of
  // latency-bound token / attention kernels plus low-resolution convs: it runs on the plan's BRANCH stream next to the
  // two 128^3 encoder convs of the caller's stream (matrix-bound at the package power cap, one wave per SIMD) and is
  // joined in front of the level-0 encoder tail.  HDF_NO_BRANCH_OVERLAP=1 keeps everything on the caller's stream.
  static const bool no_branch = getenv("HDF_NO_BRANCH_OVERLAP") != nullptr;  // A/B knob (tests/test_gpu_knobs.py)
  Exec eb = e;
  hipStream_t bst = no_branch ? nullptr : e.fork_branch();
  if (bst) eb.st = bst, eb.on_branch = true;
  Rejoin rejoin{e, eb, bst != nullptr};  // error returns below: no branch-stream work unordered behind the caller's stream
  const bool fused_at3 = !p->flat;   // (the 2-D model: materialised at3 + the 2-D encoder tail)
  // (round 5) Order of the first launches.  The first level-0 conv reads the fp32 weights itself (csrc/conv_first.hip) and
  // needs only the converted input, so where that kernel takes the layer the caller's stream starts with conversion +
  // conv, and the weight packs -- every conv's 16-bit panels and the persistent transformer kernel's fragment-major copies,
  // ~80 us of light kernels -- go to the BRANCH stream in front of the patch embedding: the conv runs beside them instead
  // of behind them, and the transformer kernel (which holds every unit and therefore effectively starts when that conv
  // ends) starts ~120 us earlier.  `packed` orders the second conv (and the branch's own convs, by stream order) behind the
  // packs.  Without a branch stream, or where the generic conv takes the first layer, the packs stay in front.
  const bool first_direct = bst && p->enc[0][0].Cin <= 4 &&
                            hdf_conv_first_takes(p->dtype, p->enc[0][0].Cin, p->enc[0][0].Cout, p->dims[0][0], p->dims[0][1],
                                                 p->dims[0][2], p->xin.pitch);
  hipStream_t pst = first_direct ? bst : e.st;
  auto first_layer = [&]() -> int {
    HDF_TRY(hdf_launch_nchw_to_ndhwc(p->dtype, x, e.at(p->xin), batch, p->M, 16, p->vox(0), e.st));
    return conv_forward(e, p->enc[0][0], p->xin, none);
  };
  if (first_direct) HDF_TRY(first_layer());
  HDF_TRY(hdf_launch_pack_batch(p->dtype, params, e.ws, p->pack_jobs.data(), (int)p->pack_jobs.size(), pst));
  if (p->tf_fwd_chain)
    HDF_TRY(tf_chain_pack(tf_dims(p, batch), p->tf_cp, p->nb, params, e.ws + p->tf_wpack, pst));
  // (the caller's stream waits here only where the packs went to the branch stream; the branch stream waits below)
  hipEvent_t packed = bst ? e.order(pst, e.st, "the caller's stream behind the weight packs", first_direct) : nullptr;
  if (bst && !packed) return HDF_ERR_HIP;
  // the caller's stream first (4 launches), then the ~65 launches of the branch: the host issues launches one after the
  // other, and whatever is issued second starts that much later when the host is not far ahead of the GPU
  if (!first_direct) HDF_TRY(first_layer());
  // (round 5) The second level-0 conv takes three quarters of the compute units: it runs while the branch stream works
  // through deep_conv / up1..3 (the persistent transformer kernel in front of them holds every unit, so the order on
  // the device is conv_first, transformer, then this conv NEXT TO the UpConv chain), and the chain's low-resolution
  // convs cannot share a unit with a persistent 128^3 workgroup (LDS, registers): at 256 workgroups they queued behind it
  // (deep_conv: 291 us instead of 72) and the caller's stream then waited 220 us for at3.  192 of 256: conv 277 -> 363 us,
  // at3 ready 85 us earlier (tools/timeline.py, profiles/r05_forward_timeline.txt).  The grid is the same in every
  // stream arrangement: the InstanceNorm partial sums are grouped per workgroup, and tests/test_gpu_knobs.py compares
  // arrangements bit for bit.
  // With the persistent transformer kernel the device order conv_first -> transformer -> this conv is made explicit: the
  // kernel needs every unit, and this conv's 192 workgroups in front of it would leave it spinning on the other 64 for the
  // conv's whole duration.  (The launch chain of small kernels co-runs with the conv instead: no wait.)
  const bool chain_first = first_direct && p->tf_fwd_chain;
  eb.tf_packed = first_direct ? nullptr : packed;   // (packs on the branch stream itself: stream order)
  if (chain_first) {
    HDF_TRY(transformer_forward(eb, x));
    if (!e.order(bst, e.st, "the caller's stream behind the branch stream's transformer (tf_done)")) return HDF_ERR_HIP;
  }
  e.conv_budget = (hdf_cu_budget() * 3 / 4) & ~7;
  HDF_TRY(conv_forward(e, p->enc[0][1], p->enc[0][0].y, xf_of(e, p->enc[0][0])));
  e.conv_budget = 0;
  if (!chain_first) HDF_TRY(transformer_forward(eb, x));
  if (packed) HDF_TRY(e.wait(bst, packed, "the branch stream behind the weight packs"));
  HDF_TRY(conv_forward(eb, p->deep, p->attnall, none));
  HDF_TRY(hdf_launch_upsample_fwd(p->dtype, eb.rows(p->deep.y), eb.norm(p->deep.st), eb.rows(p->attnout),
                                  eb.extent(4, 8 * nf), eb.st));
  {
    const View* src = &p->attnout;
    for (int k = 0; k < 3; k++) {  // up1 -> at1 (lvl 2), up2 -> at2 (lvl 1), up3 -> at3 (lvl 0)
      Conv3& c = p->up[k];
      HDF_TRY(conv_forward(eb, c, *src, none));
      const View& dst = p->at[2 - k];
      // at3 (k == 2) is not materialised: the level-0 encoder tail interpolates it from up3's output (enc_tail_up_kernel)
      if (k == 2 && fused_at3) break;
      HDF_TRY(hdf_launch_upsample_fwd(p->dtype, eb.rows(c.y), eb.norm(c.st), eb.rows(dst), eb.extent(c.lvl, c.Cout),
                                      eb.st));
      src = &dst;
    }
  }
  // ---- encoder (:237-244)
  const View* cur = &p->xin;
  for (int k = 0; k < 4; k++) {
    if (k > 0) {  // (level 0: issued above, in front of the branch)
      HDF_TRY(conv_forward(e, p->enc[k][0], *cur, none));
      HDF_TRY(conv_forward(e, p->enc[k][1], p->enc[k][0].y, xf_of(e, p->enc[k][0])));
    }
    Conv3& c = p->enc[k][1];
    if (k == 0 && bst) {  // at1..3 / attnout are needed from here on
      HDF_TRY(e.join_branch(eb));
      rejoin.forked = false;
    }
    if (k < 3) {
      View ds = hdf_plan_subview(p, p->cat[k], ch[k], ch[k]);
      // ds_k = relu(IN(y)) + at_k ; pooled = MaxPool(ds_k): one fused pass
      if (k == 0 && fused_at3) {
        Conv3& u = p->up[2];  // at3 = Upsample(relu(IN(up3 conv))), evaluated inside the pass
        HDF_TRY(hdf_launch_enc_tail_up(p->dtype, e.rows(c.y), e.norm(c.st), e.rows(u.y), e.norm(u.st), e.rows(ds),
                                       e.rows(p->pooled[k]), (uint8_t*)(e.ws + p->pool_idx[k]), e.extent(k + 1, ch[k]),
                                       e.st));
      } else
      HDF_TRY(hdf_launch_enc_tail(p->dtype, e.rows(c.y), e.norm(c.st), e.rows(p->at[k]), e.rows(ds), e.rows(p->pooled[k]),
                                  (uint8_t*)(e.ws + p->pool_idx[k]), e.extent(k + 1, ch[k]), e.st));
      cur = &p->pooled[k];
    } else {
      HDF_TRY(hdf_launch_norm_relu_add(p->dtype, e.rows(c.y), e.norm(c.st), e.rows(p->attnout), e.rows(p->x4), batch, ch[3],
                                       p->vox(3), e.st));
    }
  }
  // ---- decoder (:246-253)
  HDF_TRY(head_forward(e, p->head[3], p->x4, none, outs[3]));
  const View* dec_in = &p->x4;
  Xf dec_xf = none;
  for (int k = 2; k >= 0; k--) {
    View up_out = hdf_plan_subview(p, p->cat[k], 0, ch[k]);
    HDF_TRY(convt_forward(e, p->upc[k], *dec_in, dec_xf, up_out));
    HDF_TRY(conv_forward(e, p->dec[k][0], p->cat[k], none, k == 0));   // k == 0: block_1_1_right, the probed launch
    HDF_TRY(conv_forward(e, p->dec[k][1], p->dec[k][0].y, xf_of(e, p->dec[k][0])));
    dec_in = &p->dec[k][1].y;
    dec_xf = xf_of(e, p->dec[k][1]);
    HDF_TRY(head_forward(e, p->head[k], *dec_in, dec_xf, outs[k]));
  }
  // (a persistent launch that gave up must not leave plausible outputs: exec_tf.hip, chain_poison_outputs_kernel)
  if (p->tf_fwd_chain) HDF_TRY(chain_poison_outputs(e, outs));
  return HDF_OK;
}

// bev (optional, stages == 7): HDF_NUM_GRAD_BUCKETS events, recorded where the parameter gradients of a bucket
// (hdf_plan_grad_bucket: 0 decoder + heads, 1 UpConv chain, 2 transformer branches, 3 encoder levels 1-3, 4 encoder
// level 0) are final -- on the caller's stream, the side stream or the branch stream, whichever finishes them -- so that a
// communication stream can start a bucket's all-reduce while the rest of this one call is still running (no staged calls,
// the branch-stream fork stays).  Round 6: five buckets instead of three.  With one "encoder / decoder / heads" bucket 26
// of the 62 MB became final with the LAST kernel of the backward (the first encoder layer's weight gradient) and their
// all-reduce was fully exposed (profiles/r06_timeline_standin_32cu_300us.txt: two of three stand-in collectives ran
// behind the backward); now the decoder + heads (final a third of the way into the backward) and the encoder's levels
// 1-3 (final before the UpConv chain's backward starts) are reduced under the rest, and what is final at the very end is
// the first level's two layers: 0.1 MB.
static int backward3d(hdf_plan* p, const float* x, const float* params, void* workspace, int64_t workspace_bytes,
                      const void* dout0, const void* dout1, const void* dout2, const void* dout3, float* grads,
                      int batch, int stages, hdf_stream stream, hipEvent_t* bev = nullptr) {
  HDF_CHECK_ARG(p->batch == batch, "backward: batch %d differs from the forward's %d", batch, p->batch);
  HDF_TRY(chain_flag_check(p));
  auto record = [&](int k, hipStream_t s) -> int {
    if (bev && hipEventRecord(bev[k], s) != hipSuccess) {
      hdf_set_error("backward: could not record the event of gradient bucket %d", k);
      return HDF_ERR_HIP;
    }
    return HDF_OK;
  };
  enum { BK_DEC = 0, BK_CHAIN = 1, BK_TF = 2, BK_ENC = 3, BK_ENC0 = 4 };
  // "everything enqueued so far on the caller's stream AND on the side stream": the side stream (where the bucket's conv
  // weight gradients run) waits for the caller's position (InstanceNorm / head / bias gradients) and carries the event.
  // Every side-stream launch already waits for the caller's position of its own launch point, so this orders nothing new.
  auto record_joined = [&](int k, Exec& ex) -> int {
    if (!bev) return HDF_OK;
    if (ex.async && p->side) {
      if (!ex.order(ex.st, p->side, "the side stream behind the issuing stream (gradient bucket event)")) return HDF_ERR_HIP;
      return record(k, p->side);
    }
    return record(k, ex.st);
  };
  HDF_CHECK_ARG((size_t)workspace_bytes >= p->ws_bytes,
                "backward: workspace of %lld bytes holds a forward only (hdf_plan_workspace_bytes = %zu)",
                (long long)workspace_bytes, p->ws_bytes);
  Exec e{p, (char*)workspace, params, grads, batch, (hipStream_t)stream};
  static const bool no_async = getenv("HDF_NO_ASYNC_WGRAD") != nullptr;  // A/B knob: everything on the caller's stream
  if (!no_async) {
    // lowest priority: when a data-gradient conv (critical path) and a weight gradient are both ready, the data
    // gradient gets the CUs first and the weight gradient then runs next to the memory-bound passes that follow it
    if (!p->side) p->side = make_stream(false);
    e.async = p->side != nullptr;
  }
  const int nf = p->nf;
  const int ch[4] = {nf, 2 * nf, 4 * nf, 8 * nf};
  const void* douts[4] = {dout0, dout1, dout2, dout3};
  Xf none;
  // one call for all three stages: stages 2 and 4 fork onto the branch stream inside stage 1 (see the encoder loop).
  // Both streams send their weight gradients through the side stream (in order: one shared workspace), so the fork
  // needs it.  Staged calls (gradient buckets of hdf_rt.parallel) keep the three stages in order on the caller's stream.
  static const bool no_branch = getenv("HDF_NO_BRANCH_OVERLAP") != nullptr;  // A/B knob (tests/test_gpu_knobs.py)
  const bool fork_ok = stages == 7 && e.async && !no_branch;
  Exec eb = e;
  eb.last_side = nullptr;
  Rejoin rejoin{e, eb, false};
  bool& forked = rejoin.forked;
  if (stages & 1) {
  hipError_t me = hipMemsetAsync(grads, 0, (size_t)p->total_floats * sizeof(float), e.st);
  if (me != hipSuccess) {
    hdf_set_error("backward: memset failed: %s", hipGetErrorString(me));
    return HDF_ERR_HIP;
  }

  // ---- decoder, top (level 0) down to level 2
  for (int k = 0; k <= 2; k++) {
    Conv3 &c1 = p->dec[k][0], &c2 = p->dec[k][1];
    // gA[k] holds d/d(activation of c2): head gradient (+ convT input gradient from the level above, k>0)
    int pre = 0;
    HeadBwd ho;
    ho.accumulate = k > 0 ? 1 : 0, ho.fuse_in = &c2, ho.pre_blocks = &pre;
    HDF_TRY(head_backward(e, p->head[k], douts[k], c2.y, xf_of(e, c2), p->gA[k], ho));
    int bsr = 0;  // the data-gradient conv may leave the first pass of c1's InstanceNorm backward behind (level 0)
    ConvBwd o2;
    o2.pre_blocks = pre, o2.din = &p->gA[k], o2.bs_next = &c1, o2.bs_rows = &bsr;
    HDF_TRY(norm_conv_backward(e, c2, p->gA[k], p->gY[k], c1.y, xf_of(e, c1), o2));
    // the upconv half of d(cat) is the gradient of upconv_{k+1}'s output: its bias gradient rides on this conv
    ConvBwd o1;
    o1.pre_blocks = bsr, o1.din_colsum = e.G(p->upc[k].b), o1.colsum_C = ch[k];
    if (p->dcat_split[k])
      o1.din = &p->dUp[k], o1.din2 = &p->dSkip[k];
    else
      o1.din = &p->dCat[k];
    HDF_TRY(norm_conv_backward(e, c1, p->gA[k], p->gY2[k], p->cat[k], none, o1));
    // upconv_{k+1}: input is dec[k+1][1] activation (k<2) or the bottleneck x4 (k==2)
    const View& dup = p->dUp[k];
    if (k < 2)
      HDF_TRY(convt_backward(e, p->upc[k], dup, p->dec[k + 1][1].y, xf_of(e, p->dec[k + 1][1]), p->gA[k + 1]));
    else
      HDF_TRY(convt_backward(e, p->upc[k], dup, p->x4, none, p->dX4));
  }
  HeadBwd h3;
  h3.accumulate = 1;
  HDF_TRY(head_backward(e, p->head[3], douts[3], p->x4, none, p->dX4, h3));
  HDF_TRY(record_joined(BK_DEC, e));   // upconv_1..3, block_*_right, the four heads: nothing below touches their gradients

  // ---- encoder, bottom (level 3) up to level 0.  dskip: gradient of ds_k (= of the transformer feature at_k too)
  for (int k = 3; k >= 0; k--) {
    Conv3 &c1 = p->enc[k][0], &c2 = p->enc[k][1];
    View dskip = (k == 3) ? p->dX4 : p->dSkip[k];
    int pre = 0;
    if (k < 3) {
      // ds_k also feeds pool_{k+1}: with that gradient added d(ds_k) is complete, and the pass that adds it takes the first
      // pass of c2's InstanceNorm backward along (pre rows per sample in the partials table)
      pre = hdf_maxpool_bwd_in_blocks((int64_t)p->dims[k + 1][0] * p->dims[k + 1][1] * p->dims[k + 1][2], ch[k]);
      HDF_TRY(hdf_launch_maxpool_bwd_in(p->dtype, e.rows(p->dP[k]), (const uint8_t*)(e.ws + p->pool_idx[k]), e.rows(dskip),
                                        e.rows(c2.y), e.norm(c2.st), e.inbp(), e.extent(k + 1, ch[k]), e.st));
    }
    if (k == 0 && fork_ok) {
      // d(ds_0) = d(at3) is final.  What is left: (1) the UpConv chain backward, (2) the transformer branches' backward,
      // (3) the level-0 encoder backward (two InstanceNorm backward passes at 128^3, a 32->32 data-gradient conv, two
      // weight gradients).  (1) -> (2) is the critical path (~2.1 ms, of which (2) is ~100 latency-bound launches that
      // leave most of the chip idle); (3) is 1.4 ms of heavy kernels nothing waits for.  So (1) + (2) go to the BRANCH
      // stream, and the caller's stream runs (3) NEXT TO (2): it waits for the end of (1) first -- issued together, the
      // persistent convs of (3) held every CU while the chain's small kernels queued behind them (a 5 us
      // in_bwd_finalize waited 208 us for a slot; 3.5 ms from here to the end of the step instead of 2.4).
      // The chain only READS d(ds_k) of the levels the encoder has already finished with (it accumulates into
      // dSkip[1], dSkip[2] and dX4, which the loop above consumed at k = 1, 2, 3).
      hipStream_t bst = e.fork_branch();
      if (bst) {
        eb.st = bst, eb.on_branch = true, eb.async = e.async;
        forked = true;
        HDF_TRY(upconv_chain_backward(eb, batch));
        hipEvent_t chain_done = e.order(bst, e.st, "the caller's stream behind the branch stream's UpConv chain");
        if (!chain_done) return HDF_ERR_HIP;
        if (bev) {
          // bucket 2 = the chain's conv weight gradients: launched on the side stream (every one of them is enqueued by
          // now), the rest of the chain on the branch stream.  The side stream's later launches belong to the level-0
          // encoder work, which the caller's stream starts behind chain_done anyway.
          HDF_TRY(e.wait(p->side, chain_done, "the side stream behind the branch stream's UpConv chain"));
          HDF_TRY(record(BK_CHAIN, p->side));
        }
      }
    }
    int bsr = 0;
    ConvBwd o2;
    o2.pre_blocks = pre, o2.din = &p->gA[k], o2.bs_next = &c1, o2.bs_rows = &bsr;
    HDF_TRY(norm_conv_backward(e, c2, dskip, p->gY[k], c1.y, xf_of(e, c1), o2));
    bool first_fused = false;
    // The first layer has no input gradient: the second pass of its InstanceNorm backward would write dy (268 MB at the
    // benchmark size) only for the weight gradient to read it back.  wgrad_first_kernel applies that pass to the rows it
    // stages (from d(activation) and y) instead: one pass over two tensors less on the caller's stream.
    if (k == 0 && hdf_wgrad_first_takes(p->dtype, c1.Cin, c1.Cout, p->dims[0][0], p->dims[0][1], p->dims[0][2],
                                        p->xin.pitch, p->gA[k].pitch)) {
      float* kk = e.f(p->inb_k3);
      InBwd ib;
      ib.pre_blocks = bsr, ib.apply = false, ib.kbuf = kk;
      HDF_TRY(in_backward(e, c1, p->gA[k], p->gY2[k], ib));
      const WgradFirstIn fi{e.at(c1.y), c1.y.pitch, e.f(c1.st.scale), e.f(c1.st.shift), e.f(c1.st.mean), e.f(c1.st.rstd),
                            kk, kk + (size_t)e.B * c1.Cout, kk + (size_t)2 * e.B * c1.Cout};
      HDF_TRY(hdf_launch_wgrad_first(p->dtype, e.at(p->gA[k]), p->gA[k].pitch, c1.Cout, e.at(p->xin), p->xin.pitch, c1.Cin,
                                     e.B, p->dims[0][0], p->dims[0][1], p->dims[0][2], e.G(c1.w), 0, e.ws + p->wgrad_ws,
                                     p->wgrad_ws_bytes, e.wgrad_stream(), &fi));
      HDF_TRY(e.wgrad_done(p->gA[k]));
      first_fused = true;
    }
    if (!first_fused) {
      ConvBwd o1;  // (the first layer has no input gradient)
      o1.pre_blocks = bsr, o1.din = k > 0 ? &p->dP[k - 1] : nullptr;
      HDF_TRY(norm_conv_backward(e, c1, p->gA[k], p->gY2[k], k > 0 ? p->pooled[k - 1] : p->xin, none, o1));
    }
    if (k == 1) HDF_TRY(record_joined(BK_ENC, e));   // block_2_* .. block_4_*_left: the encoder below the top level is done
    // (host order: the ten level-0 launches of the caller's stream first, then the ~100 of the transformer backward)
    if (k == 0 && forked) {
      HDF_TRY(transformer_backward(eb, x));
      if (bev) {
        eb.join();  // (the branch's own side-stream launches, if any)
        HDF_TRY(record(BK_TF, eb.st));
      }
    }
  }

  if (!(stages & 6) || bev) e.join();  // staged call (gradient buckets) / bucket event: final here
  HDF_TRY(record(BK_ENC0, e.st));
  }  // stage 1: every gradient of the encoder / decoder / head parameters is final here
  if (forked) {
    HDF_TRY(e.join_branch(eb));
    forked = false;
  } else {
    if (stages & 2) {
      HDF_TRY(upconv_chain_backward(e, batch));
      if (!(stages & 4) || bev) e.join();  // staged call: final when it returns; else the transformer branches run under them
      HDF_TRY(record(BK_CHAIN, e.st));
    }  // stage 2: deep_conv / up1..3 gradients are final
    if (stages & 4) {
      HDF_TRY(transformer_backward(e, x));
      if (bev) {
        e.join();
        HDF_TRY(record(BK_TF, e.st));
      }
    }
  }
  e.join();
  if ((stages & 4) && p->tf_bwd_chain) HDF_TRY(chain_poison_grads(e));
  return HDF_OK;
}

static int backward_any(hdf_plan* p, const float* x, const float* params, void* workspace, int64_t workspace_bytes,
                        const void* dout0, const void* dout1, const void* dout2, const void* dout3, float* grads,
                        int batch, int stages, hdf_stream stream, hipEvent_t* bev) {
  HDF_CHECK_ARG(p && x && params && workspace && grads, "backward: null argument");
  if (!p->is2d)
    return backward3d(p, x, params, workspace, workspace_bytes, dout0, dout1, dout2, dout3, grads, batch, stages, stream,
                      bev);
  // 2-D model: the forward left the replicated input and the embedded parameters in the workspace
  HDF_CHECK_ARG(p->batch == batch && (size_t)workspace_bytes >= p->ws_bytes, "backward: batch / workspace mismatch");
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  void* d3[4];
  const void* d2[4] = {dout0, dout1, dout2, dout3};
  for (int i = 0; i < 4; i++) {
    if (p->flat) {   // the 2-D logit gradients are the depth-1 tensors the native path reads
      d3[i] = const_cast<void*>(d2[i]);
      continue;
    }
    d3[i] = ws + p->e_dout3d[i];
    if (stages & 1)  // the loss sees depth slice 0 only
      HDF_TRY(hdf_launch_depth_slice(p->dtype, d3[i], const_cast<void*>(d2[i]), (int64_t)batch * p->ncls, p->dims[i][0],
                                 (int64_t)p->dims[i][1] * p->dims[i][2], 0, st));
  }
  float* g3 = (float*)(ws + p->e_grads3d);
  if (p->flat)   // (x: the patch embedding's weight gradient reads the 2-D input itself)
    HDF_TRY(backward3d(p, x, (const float*)(ws + p->e_params3d), workspace, workspace_bytes, d3[0], d3[1], d3[2], d3[3], g3,
                       batch, stages, stream));
  else
  HDF_TRY(backward3d(p, (const float*)(ws + p->e_x3d), (const float*)(ws + p->e_params3d), workspace, workspace_bytes,
                     d3[0], d3[1], d3[2], d3[3], g3, batch, stages, stream));
  HDF_TRY(hdf_launch_extract2d(p, stages, g3, grads, st));
  if (bev) {  // the 2-D gradients exist only after the extraction: every bucket is final here
    for (int k = 0; k < HDF_NUM_GRAD_BUCKETS; k++)
      if (hipEventRecord(bev[k], st) != hipSuccess) {
        hdf_set_error("backward: could not record a bucket event");
        return HDF_ERR_HIP;
      }
  }
  return HDF_OK;
}

// ================================================================================================ C ABI
extern "C" {

int hdf_forward(hdf_plan* p, const float* x, const float* params, void* workspace, int64_t workspace_bytes, void* out0,
                void* out1, void* out2, void* out3, int batch, int training, uint64_t seed, hdf_stream stream) {
  HDF_CHECK_ARG(p && x && params && workspace, "forward: null argument");
  if (!p->is2d)
    return forward3d(p, x, params, workspace, workspace_bytes, out0, out1, out2, out3, batch, training, seed, stream);
  // 2-D model: x [B,C,H,W], params = the 2-D flat buffer, outputs [B,n_cls,H/2^i,W/2^i]
  hdf_plan_layout(p, batch);
  HDF_CHECK_ARG((size_t)workspace_bytes >= p->ws_fwd_bytes, "forward: workspace %lld < %zu bytes",
                (long long)workspace_bytes, p->ws_fwd_bytes);
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  float* p3 = (float*)(ws + p->e_params3d);
  float* x3 = (float*)(ws + p->e_x3d);
  HDF_TRY(hdf_launch_embed2d(p, params, p3, st));
  if (p->flat)
    // native 2-D path: depth-1 tensors throughout; the logits [B, n_cls, 1, H, W] ARE the 2-D outputs, and the patch
    // embedding contracts the input's 16 x 16 patches with depth slice 0 of the embedded kernels (kd = 1)
    return forward3d(p, x, p3, workspace, workspace_bytes, out0, out1, out2, out3, batch, training, seed, stream);
  const int64_t hw = (int64_t)p->H * p->W;
  HDF_TRY(hdf_launch_replicate_depth(x, x3, (int64_t)batch * p->M, p->D, hw, st));
  void* o3[4];
  for (int i = 0; i < 4; i++) o3[i] = ws + p->e_out3d[i];
  HDF_TRY(forward3d(p, x3, p3, workspace, workspace_bytes, o3[0], o3[1], o3[2], o3[3], batch, training, seed, stream));
  void* o2[4] = {out0, out1, out2, out3};
  for (int i = 0; i < 4; i++)
    HDF_TRY(hdf_launch_depth_slice(p->dtype, o3[i], o2[i], (int64_t)batch * p->ncls, p->dims[i][0],
                               (int64_t)p->dims[i][1] * p->dims[i][2], 1, st));
  return HDF_OK;
}

int hdf_backward(hdf_plan* p, const float* x, const float* params, void* workspace, int64_t workspace_bytes,
                 const void* dout0, const void* dout1, const void* dout2, const void* dout3, float* grads, int batch,
                 hdf_stream stream) {
  return hdf_backward_stages(p, x, params, workspace, workspace_bytes, dout0, dout1, dout2, dout3, grads, batch, 7,
                             stream);
}

int hdf_backward_stages(hdf_plan* p, const float* x, const float* params, void* workspace, int64_t workspace_bytes,
                        const void* dout0, const void* dout1, const void* dout2, const void* dout3, float* grads,
                        int batch, int stages, hdf_stream stream) {
  return backward_any(p, x, params, workspace, workspace_bytes, dout0, dout1, dout2, dout3, grads, batch, stages, stream,
                      nullptr);
}

int hdf_backward_events(hdf_plan* p, const float* x, const float* params, void* workspace, int64_t workspace_bytes,
                        const void* dout0, const void* dout1, const void* dout2, const void* dout3, float* grads,
                        int batch, hdf_stream stream, void** bucket_events) {
  HDF_CHECK_ARG(p && bucket_events, "backward_events: null argument");
  for (int k = 0; k < HDF_NUM_GRAD_BUCKETS; k++) {
    if (!p->bucket_ev[k] && hipEventCreateWithFlags(&p->bucket_ev[k], hipEventDisableTiming) != hipSuccess) {
      p->bucket_ev[k] = nullptr;
      hdf_set_error("backward_events: could not create an event");
      return HDF_ERR_HIP;
    }
    bucket_events[k] = (void*)p->bucket_ev[k];
  }
  return backward_any(p, x, params, workspace, workspace_bytes, dout0, dout1, dout2, dout3, grads, batch, 7, stream,
                      p->bucket_ev);
}

int hdf_op_occupy(int workgroups, int lds_bytes, int vgprs, int usec, hdf_stream stream) {
  HDF_CHECK_ARG(workgroups >= 1 && workgroups <= 4096 && lds_bytes >= 0 && lds_bytes <= 160 * 1024 && usec >= 1 &&
                    usec <= 10000000 && (vgprs == 0 || vgprs == 128),
                "op_occupy: workgroups 1..4096, lds 0..160 KiB, vgprs 0 or 128, 1 us..10 s");
  const void* fn = vgprs ? reinterpret_cast<const void*>(occupy_kernel<true>) : reinterpret_cast<const void*>(occupy_kernel<false>);
  if (lds_bytes > 64 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
    hdf_set_error("op_occupy: hipFuncSetAttribute failed");
    return HDF_ERR_HIP;
  }
  if (vgprs)
    hipLaunchKernelGGL(occupy_kernel<true>, dim3(workgroups), dim3(256), (size_t)lds_bytes, (hipStream_t)stream, (unsigned)usec * 100u);
  else
    hipLaunchKernelGGL(occupy_kernel<false>, dim3(workgroups), dim3(256), (size_t)lds_bytes, (hipStream_t)stream, (unsigned)usec * 100u);
  HDF_LAUNCH_CHECK();
  return HDF_OK;
}

int hdf_plan_set_probe(hdf_plan* p, void* ev_start, void* ev_stop) {
  HDF_CHECK_ARG(p && ((ev_start == nullptr) == (ev_stop == nullptr)), "plan_set_probe: both events or none");
  p->probe_start = (hipEvent_t)ev_start, p->probe_stop = (hipEvent_t)ev_stop;
  return HDF_OK;
}

int hdf_stream_wait_event(hdf_stream stream, void* event) {
  HDF_CHECK_ARG(event != nullptr, "stream_wait_event: null event");
  if (hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0) != hipSuccess) {
    hdf_set_error("hipStreamWaitEvent failed");
    return HDF_ERR_HIP;
  }
  return HDF_OK;
}

}  // extern "C"
