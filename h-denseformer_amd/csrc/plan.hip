// Model plan: owns the parameter table (= the reference state_dict, HDenseFormer.py:178-227), the layer table and
// the workspace layout.  Host arithmetic only -- no kernel, no launch (the launch sequences over a plan: exec.hip,
// exec_tf.hip); every device buffer is caller-owned.
#include <cstdarg>
#include <cstring>

#include "plan_internal.h"

namespace {

void add_param(hdf_plan* p, const std::string& name, std::vector<int64_t> shape) {
  ParamInfo pi;
  pi.name = name;
  pi.shape = shape;
  pi.numel = 1;
  for (auto s : shape) pi.numel *= s;
  pi.offset = p->total_floats;
  p->total_floats += (pi.numel + 15) / 16 * 16;
  p->pidx[name] = (int64_t)p->params.size();
  p->params.push_back(pi);
}

void build_params(hdf_plan* p) {
  const int nf = p->nf, DM = p->DM;
  char buf[256];
  for (int m = 0; m < p->M; m++) {
    int64_t start = p->total_floats;
    auto nm = [&](const char* fmt, ...) {
      va_list ap;
      va_start(ap, fmt);
      vsnprintf(buf, sizeof(buf), fmt, ap);
      va_end(ap);
      return std::string("attns.") + std::to_string(m) + "." + buf;
    };
    add_param(p, nm("position_embeddings"), {1, p->Ntok, DM});
    add_param(p, nm("patch_embeddings.weight"), {DM, 1, 16, 16, 16});
    add_param(p, nm("patch_embeddings.bias"), {DM});
    for (int b = 0; b < p->nb; b++) {
      for (int l = 0; l < 4; l++) {
        add_param(p, nm("blocks.%d.0.layers.%d.0.weight", b, l), {32, DM + 32 * l});
        add_param(p, nm("blocks.%d.0.layers.%d.0.bias", b, l), {32});
        add_param(p, nm("blocks.%d.0.layers.%d.1.norm.weight", b, l), {32});
        add_param(p, nm("blocks.%d.0.layers.%d.1.norm.bias", b, l), {32});
        add_param(p, nm("blocks.%d.0.layers.%d.1.fn.to_qkv.weight", b, l), {96, 32});
        add_param(p, nm("blocks.%d.0.layers.%d.1.fn.to_out.0.weight", b, l), {32, 32});
        add_param(p, nm("blocks.%d.0.layers.%d.1.fn.to_out.0.bias", b, l), {32});
        add_param(p, nm("blocks.%d.0.layers.%d.2.norm.weight", b, l), {32});
        add_param(p, nm("blocks.%d.0.layers.%d.2.norm.bias", b, l), {32});
        add_param(p, nm("blocks.%d.0.layers.%d.2.fn.net.0.weight", b, l), {64, 32});
        add_param(p, nm("blocks.%d.0.layers.%d.2.fn.net.0.bias", b, l), {64});
        add_param(p, nm("blocks.%d.0.layers.%d.2.fn.net.3.weight", b, l), {32, 64});
        add_param(p, nm("blocks.%d.0.layers.%d.2.fn.net.3.bias", b, l), {32});
      }
      add_param(p, nm("blocks.%d.0.out_layer.net.0.weight", b), {64, DM + 128});
      add_param(p, nm("blocks.%d.0.out_layer.net.0.bias", b), {64});
      add_param(p, nm("blocks.%d.0.out_layer.net.3.weight", b), {DM, 64});
      add_param(p, nm("blocks.%d.0.out_layer.net.3.bias", b), {DM});
    }
    if (m == 0) p->mstride = p->total_floats - start;
  }
  auto upc = [&](const std::string& n, int ci, int co) {
    add_param(p, n + ".double_conv.0.weight", {co, ci, 3, 3, 3});
    add_param(p, n + ".double_conv.0.bias", {co});
  };
  auto basic = [&](const std::string& n, int ci, int co) {
    add_param(p, n + ".conv.weight", {co, ci, 3, 3, 3});
    add_param(p, n + ".norm.weight", {co});
    add_param(p, n + ".norm.bias", {co});
  };
  auto convt = [&](const std::string& n, int ci, int co) {
    add_param(p, n + ".weight", {ci, co, 3, 3, 3});
    add_param(p, n + ".bias", {co});
  };
  auto head = [&](const std::string& n, int ci) {
    add_param(p, n + ".weight", {p->ncls, ci, 1, 1, 1});
    add_param(p, n + ".bias", {p->ncls});
  };
  upc("deep_conv", DM * p->M, 8 * nf);
  upc("up1", 8 * nf, 4 * nf);
  upc("up2", 4 * nf, 2 * nf);
  upc("up3", 2 * nf, nf);
  basic("block_1_1_left", p->M, nf);
  basic("block_1_2_left", nf, nf);
  basic("block_2_1_left", nf, 2 * nf);
  basic("block_2_2_left", 2 * nf, 2 * nf);
  basic("block_3_1_left", 2 * nf, 4 * nf);
  basic("block_3_2_left", 4 * nf, 4 * nf);
  basic("block_4_1_left", 4 * nf, 8 * nf);
  basic("block_4_2_left", 8 * nf, 8 * nf);
  convt("upconv_3", 8 * nf, 4 * nf);
  basic("block_3_1_right", 8 * nf, 4 * nf);
  basic("block_3_2_right", 4 * nf, 4 * nf);
  convt("upconv_2", 4 * nf, 2 * nf);
  basic("block_2_1_right", 4 * nf, 2 * nf);
  basic("block_2_2_right", 2 * nf, 2 * nf);
  convt("upconv_1", 2 * nf, nf);
  basic("block_1_1_right", 2 * nf, nf);
  basic("block_1_2_right", nf, nf);
  head("conv1x1", nf);
  head("conv1x1_d1", 2 * nf);
  head("conv1x1_d2", 4 * nf);
  head("conv1x1_d3", 8 * nf);
}

// Transformer addressing of modality 0 (hdf_plan::tf_cp / tf_wg / pe_*; modality m: + m * mstride).  The executor reaches
// tensor k of layer l of block b as blk0 + b * blk_stride + loff[l][k]: checked here, from the names, for every block.
int build_tf_tables(hdf_plan* p) {
  static const char* const LAYER[13] = {"0.weight", "0.bias", "1.norm.weight", "1.norm.bias", "1.fn.to_qkv.weight",
                                        "1.fn.to_out.0.weight", "1.fn.to_out.0.bias", "2.norm.weight", "2.norm.bias",
                                        "2.fn.net.0.weight", "2.fn.net.0.bias", "2.fn.net.3.weight", "2.fn.net.3.bias"};
  static const char* const OUT[4] = {"0.weight", "0.bias", "3.weight", "3.bias"};  // (the member order of TfLayerP / TfOutP)
  auto layer = [&](int b, int l, int k) {
    return p->P("attns.0.blocks." + std::to_string(b) + ".0.layers." + std::to_string(l) + "." + LAYER[k]);
  };
  auto out = [&](int b, int k) { return p->P("attns.0.blocks." + std::to_string(b) + ".0.out_layer.net." + OUT[k]); };
  TfChainP& c = p->tf_cp;
  c.blk0 = layer(0, 0, 0);
  c.blk_stride = p->nb > 1 ? layer(1, 0, 0) - c.blk0 : 0;
  for (int l = 0; l < 4; l++)
    for (int k = 0; k < 13; k++) c.loff[l][k] = (int32_t)(layer(0, l, k) - c.blk0);
  for (int k = 0; k < 4; k++) c.ooff[k] = (int32_t)(out(0, k) - c.blk0);
  for (int b = 0; b < p->nb; b++) {
    const int64_t blk = c.blk0 + b * c.blk_stride;
    bool ok = true;
    for (int l = 0; l < 4; l++)
      for (int k = 0; k < 13; k++) ok = ok && layer(b, l, k) >= 0 && layer(b, l, k) == blk + c.loff[l][k];
    for (int k = 0; k < 4; k++) ok = ok && out(b, k) >= 0 && out(b, k) == blk + c.ooff[k];
    HDF_CHECK_ARG(ok, "plan_create: transformer block %d is not laid out like block 0 at %lld + %d * %lld floats", b,
                  (long long)c.blk0, b, (long long)c.blk_stride);
  }
  const int DM = p->DM, DMF = p->DMF;
  TfWgradEntry* e = p->tf_wg;
  for (int l = 0; l < 4; l++) {
    const int32_t* o = c.loff[l];
    *e++ = TfWgradEntry{o[4], 96, 32, l, 0, 0, TF_T_DQ, TF_T_T, -1, -1, 96, 32};                                // to_qkv
    *e++ = TfWgradEntry{o[0], 32, DM + 32 * l, l, 0, 1, TF_T_DH0, 0, -1, -1, 32, DMF};                          // Linear0
    *e++ = TfWgradEntry{o[11], 32, 64, l, 0, 0, TF_T_P1, TF_T_P1 + 32, TF_T_P0, TF_T_P0 + 32, 32, 64};          // net.3
    *e++ = TfWgradEntry{o[9], 64, 32, l, 0, 0, TF_T_P1 + 96, TF_T_P1 + 160, TF_T_P0 + 96, TF_T_P0 + 160, 64, 32};  // net.0
    *e++ = TfWgradEntry{o[5], 32, 32, l, 0, 2, TF_T_DGO, 0, -1, -1, 32, 32};                                    // to_out
  }
  *e++ = TfWgradEntry{c.ooff[2], DM, 64, 0, 3, 3, 0, DM, -1, -1, DM, 64};          // out_layer.net.3
  *e++ = TfWgradEntry{c.ooff[0], 64, DMF, 0, 3, 1, DM + 64, 0, -1, -1, 64, DMF};   // out_layer.net.0
  p->pe_w = p->P("attns.0.patch_embeddings.weight");
  p->pe_b = p->P("attns.0.patch_embeddings.bias");
  p->pe_pos = p->P("attns.0.position_embeddings");
  return HDF_OK;
}

void init_conv(hdf_plan* p, Conv3& c, const std::string& name, int cin, int cout, int lvl, bool basic) {
  c.name = name;
  c.Cin = cin;
  c.CinP = round_up(cin, 16);
  c.Cout = cout;
  c.lvl = lvl;
  if (basic) {
    c.w = p->P(name + ".conv.weight");
    c.gamma = p->P(name + ".norm.weight");
    c.beta = p->P(name + ".norm.bias");
  } else {
    c.w = p->P(name + ".double_conv.0.weight");
    c.b = p->P(name + ".double_conv.0.bias");
  }
}

void build_layers(hdf_plan* p) {
  const int nf = p->nf;
  init_conv(p, p->deep, "deep_conv", p->DM * p->M, 8 * nf, 4, false);
  init_conv(p, p->up[0], "up1", 8 * nf, 4 * nf, 3, false);
  init_conv(p, p->up[1], "up2", 4 * nf, 2 * nf, 2, false);
  init_conv(p, p->up[2], "up3", 2 * nf, nf, 1, false);
  const int ch[4] = {nf, 2 * nf, 4 * nf, 8 * nf};
  for (int k = 0; k < 4; k++) {
    std::string b = "block_" + std::to_string(k + 1);
    init_conv(p, p->enc[k][0], b + "_1_left", k == 0 ? p->M : ch[k - 1], ch[k], k, true);
    init_conv(p, p->enc[k][1], b + "_2_left", ch[k], ch[k], k, true);
    if (k < 3) {
      init_conv(p, p->dec[k][0], b + "_1_right", 2 * ch[k], ch[k], k, true);
      init_conv(p, p->dec[k][1], b + "_2_right", ch[k], ch[k], k, true);
      ConvT3& t = p->upc[k];
      t.name = "upconv_" + std::to_string(k + 1);
      t.Cin = ch[k + 1];
      t.Cout = ch[k];
      t.lvl_in = k + 1;
      t.w = p->P(t.name + ".weight");
      t.b = p->P(t.name + ".bias");
    }
  }
  const char* hn[4] = {"conv1x1", "conv1x1_d1", "conv1x1_d2", "conv1x1_d3"};
  for (int k = 0; k < 4; k++) {
    p->head[k].name = hn[k];
    p->head[k].C = ch[k];
    p->head[k].lvl = k;
    p->head[k].w = p->P(std::string(hn[k]) + ".weight");
    p->head[k].b = p->P(std::string(hn[k]) + ".bias");
  }
}

// the 2-D state_dict (conv kernels lose their depth axis) and the embedding jobs; consecutive unchanged tensors are
// merged into one copy job (both flat layouts pad every tensor to 16 floats, so such runs have equal lengths)
int build_params2d(hdf_plan* p) {
  p->params2d.clear();
  p->ejobs.clear();
  p->total_floats2d = 0;
  int64_t unet0 = p->P("block_1_1_left.conv.weight"), chain0 = p->P("deep_conv.double_conv.0.weight");
  for (const ParamInfo& pi : p->params) {
    ParamInfo q = pi;
    int kind = 0, rep = 1, inner = 1;
    if (pi.shape.size() == 5) {
      rep = (int)pi.shape[2];
      inner = (int)(pi.shape[3] * pi.shape[4]);
      q.shape.erase(q.shape.begin() + 2);
      q.numel = pi.numel / rep;
      if (rep == 3)
        kind = pi.name.rfind("upconv_", 0) == 0 ? 2 : 1;
      else if (rep == 16)
        kind = 3;
      else
        rep = 1, inner = 1;  // 1x1x1 heads: plain copy
    }
    q.offset = p->total_floats2d;
    p->total_floats2d += (q.numel + 15) / 16 * 16;
    const char stage = pi.offset >= unet0 ? 1 : pi.offset >= chain0 ? 2 : 4;
    const int64_t n3 = kind ? pi.numel : (pi.numel + 15) / 16 * 16;
    if (kind == 0 && !p->ejobs.empty()) {
      Embed2dJob& last = p->ejobs.back();
      if (last.kind == 0 && last.stage == stage && last.off3 + last.n3 == pi.offset && last.off2 + last.n3 == q.offset) {
        last.n3 += n3;
        p->params2d.push_back(q);
        continue;
      }
    }
    p->ejobs.push_back(Embed2dJob{pi.offset, q.offset, n3, inner, (short)rep, (char)kind, stage});
    p->params2d.push_back(q);
  }
  HDF_CHECK_ARG((int)p->ejobs.size() <= HDF_MAX_EMBED_JOBS, "2-D plan: %d embedding jobs (max %d)", (int)p->ejobs.size(),
                HDF_MAX_EMBED_JOBS);
  return HDF_OK;
}

View mkview(hdf_plan* p, Bump& bp, const std::string& name, int lvl, int C, int batch) {
  View v;
  v.C = C;
  v.pitch = C;
  v.lvl = lvl;
  v.off = bp.take((size_t)batch * p->vox(lvl) * C * p->esz);
  if (!name.empty()) p->bufs[name] = v;
  return v;
}

}  // namespace

View hdf_plan_subview(hdf_plan* p, const View& v, int c0, int C, const std::string& name) {
  View s = v;
  s.off = v.off + (size_t)c0 * p->esz;
  s.C = C;
  if (!name.empty()) p->bufs[name] = s;
  return s;
}

void hdf_plan_layout(hdf_plan* p, int B) {
  if (p->batch == B) return;
  p->batch = B;
  p->bufs.clear();
  Bump bp;
  const int nf = p->nf;
  const int ch[4] = {nf, 2 * nf, 4 * nf, 8 * nf};
  auto conv_bufs = [&](Conv3& c) {
    c.y = mkview(p, bp, "y." + c.name, c.lvl, c.Cout, B);
    size_t s = (size_t)B * c.Cout * sizeof(float);
    c.st.mean = bp.take(s);
    c.st.rstd = bp.take(s);
    c.st.scale = bp.take(s);
    c.st.shift = bp.take(s);
    c.wf = bp.take((size_t)27 * round_up(c.Cout, 32) * c.CinP * p->esz);
    c.wd = bp.take((size_t)27 * round_up(c.CinP, 32) * round_up(c.Cout, 16) * p->esz);
  };
  // ---- forward (persistent until backward)
  p->xin = mkview(p, bp, "xin", 0, 16, B);
  const int64_t rows = (int64_t)p->M * B * p->Ntok;
  p->tf_F = bp.take((size_t)p->nb * rows * p->DMF * sizeof(float));
  p->tf_save = bp.take((size_t)p->nb * 4 * rows * 232 * sizeof(float));
  {
    TfDims dd{};
    dd.M = p->M;
    p->tf_wpack = bp.take(tf_chain_wpack_bytes(dd, p->nb));   // (forward region: the backward reads what the forward packed)
    dd.B = B, dd.N = p->Ntok;
    p->tf_frag = bp.take(p->dtype == HDF_F32 ? 256 : tf_chain_frag_bytes(dd, p->nb));
  }
  p->tf_sync = bp.take((size_t)3 << 20);  // forward | backward counters in the first megabyte (one half each), then
                                           // two megabytes of phase stamps in -DCHAIN_DBG_STAMPS builds
  p->attnall = mkview(p, bp, "attnall", 4, p->M * p->DM, B);
  conv_bufs(p->deep);
  p->attnout = mkview(p, bp, "attnout", 3, 8 * nf, B);
  for (int k = 0; k < 3; k++) conv_bufs(p->up[k]);
  p->at[2] = mkview(p, bp, "at1", 2, 4 * nf, B);
  p->at[1] = mkview(p, bp, "at2", 1, 2 * nf, B);
  // (at3 is evaluated inside the level-0 encoder tail: forward3d; the 2-D encoder tail reads a materialised at3)
  if (p->flat) p->at[0] = mkview(p, bp, "at3", 0, nf, B);
  for (int k = 0; k < 4; k++) {
    conv_bufs(p->enc[k][0]);
    conv_bufs(p->enc[k][1]);
    if (k < 3) {
      p->cat[k] = mkview(p, bp, "cat" + std::to_string(k + 1), k, 2 * ch[k], B);
      hdf_plan_subview(p, p->cat[k], ch[k], ch[k], "ds" + std::to_string(k));
      p->pooled[k] = mkview(p, bp, "pool" + std::to_string(k + 1), k + 1, ch[k], B);
      p->pool_idx[k] = bp.take((size_t)B * p->vox(k + 1) * ch[k]);
      conv_bufs(p->dec[k][0]);
      conv_bufs(p->dec[k][1]);
      ConvT3& t = p->upc[k];
      t.wf = bp.take((size_t)27 * round_up(t.Cout, 32) * t.Cin * p->esz);
      t.wd = bp.take((size_t)27 * round_up(t.Cin, 32) * t.Cout * p->esz);
    }
  }
  p->x4 = mkview(p, bp, "bottleneck", 3, 8 * nf, B);
  if (p->is2d) {  // depth-replicated input, embedded parameters / their gradients, 3-D logits and logit gradients
    p->e_x3d = bp.take((size_t)B * p->M * p->D * p->H * p->W * sizeof(float));   // depth-16 copy of the input
    p->e_params3d = bp.take((size_t)p->total_floats * sizeof(float));
    p->e_grads3d = bp.take((size_t)p->total_floats * sizeof(float));
    for (int i = 0; i < 4; i++) {
      p->e_out3d[i] = bp.take((size_t)B * p->ncls * p->vox(i) * p->esz);
      p->e_dout3d[i] = bp.take((size_t)B * p->ncls * p->vox(i) * p->esz);
    }
  }
  // ---- weight packs (see conv_forward / conv_backward / convt_* for the layouts)
  p->pack_jobs.clear();
  auto conv_jobs = [&](Conv3& c) {
    const int* d = p->dims[c.lvl];
    c.wf_frag = hdf_conv_weight_layout(p->dtype, 0, c.CinP, d[0], d[1], d[2]);
    c.wd_frag = hdf_conv_weight_layout(p->dtype, 0, c.Cout, d[0], d[1], d[2]);
    // forward [tap][CoutP][CinP] from torch [Cout][Cin][27]
    p->pack_jobs.push_back(
        PackJob{c.w, (int64_t)c.wf, c.Cout, c.Cin, round_up(c.Cout, 32), c.CinP, c.Cin * 27, 27, 0, c.wf_frag});
    // dgrad: taps reversed, channel roles swapped: Wd[t][ci][co] = W[co][ci][26-t]
    p->pack_jobs.push_back(
        PackJob{c.w, (int64_t)c.wd, c.Cin, c.Cout, round_up(c.Cin, 32), c.Cout, 27, c.Cin * 27, 1, c.wd_frag});
  };
  conv_jobs(p->deep);
  for (int k = 0; k < 3; k++) conv_jobs(p->up[k]);
  for (int k = 0; k < 4; k++) {
    conv_jobs(p->enc[k][0]);
    conv_jobs(p->enc[k][1]);
    if (k < 3) {
      conv_jobs(p->dec[k][0]);
      conv_jobs(p->dec[k][1]);
      ConvT3& t = p->upc[k];
      const int* d = p->dims[t.lvl_in];
      t.wf_frag = hdf_conv_weight_layout(p->dtype, 2, t.Cin, d[0], d[1], d[2]);
      t.wd_frag = hdf_conv_weight_layout(p->dtype, 1, t.Cout, d[0], d[1], d[2]);
      // forward: torch ConvTranspose3d weight [Cin][Cout][27] -> [tap][CoutP][Cin]
      p->pack_jobs.push_back(
          PackJob{t.w, (int64_t)t.wf, t.Cout, t.Cin, round_up(t.Cout, 32), t.Cin, 27, t.Cout * 27, 0, t.wf_frag});
      // input gradient: stride-2 gather conv, [tap][CinP][Cout]
      p->pack_jobs.push_back(
          PackJob{t.w, (int64_t)t.wd, t.Cin, t.Cout, round_up(t.Cin, 32), t.Cout, t.Cout * 27, 27, 0, t.wd_frag});
    }
  }
  // ---- scratch shared by forward and backward
  size_t maxtiles = 0;
  for (int l = 0; l < 5; l++)
    for (int rb : {32, 1 << 20})  // weights-stationary (per-workgroup rows) and tiled (per-tile rows) geometry
      maxtiles = std::max<size_t>(maxtiles, hdf_conv_stat_tiles(0, p->dims[l][0], p->dims[l][1], p->dims[l][2], rb));
  p->stat_partials = bp.take((size_t)B * maxtiles * round_up(8 * nf, 32) * 2 * sizeof(float));
  {  // branch stream: deep_conv (level 4) and up1..3 (levels 3, 2, 1) write their InstanceNorm partials here
    size_t mt = 0;
    for (int l = 1; l < 5; l++)
      for (int rb : {32, 1 << 20}) mt = std::max<size_t>(mt, hdf_conv_stat_tiles(0, p->dims[l][0], p->dims[l][1], p->dims[l][2], rb));
    p->stat_partials2 = bp.take((size_t)B * mt * round_up(8 * nf, 32) * 2 * sizeof(float));
  }
  p->ksplit_ws = bp.take(HDF_KSPLIT_BYTES);
  p->ksplit_ws2 = bp.take(HDF_KSPLIT_BYTES);
  // Everything above is what a forward touches: an inference-only caller (eval / sliding-window prediction) can hand
  // over just this prefix (hdf_plan_inference_workspace_bytes); the backward scratch below -- transformer tapes, second
  // dy buffers, the 128 MB weight-gradient workspace, ... -- is more than half of the arena at the benchmark size.
  p->ws_fwd_bytes = bp.cur;
  // ---- backward scratch
  p->tf_scratch = bp.take((size_t)rows * std::max(160, p->DM) * sizeof(float));
  p->tf_dF = bp.take((size_t)rows * p->DMF * sizeof(float));
  // weight-gradient operand tapes of the transformer branches (contracted by tf_wgrad at the end of backward)
  p->tf_tape = bp.take((size_t)p->nb * 4 * rows * TF_TAPE_W * sizeof(float));
  p->tf_otape = bp.take((size_t)p->nb * rows * p->DMF * sizeof(float));
  p->wgrad_ws_bytes = (size_t)128 << 20;
  p->wgrad_ws = bp.take(p->wgrad_ws_bytes);
  p->inb_partials = bp.take((size_t)B * 1024 * 8 * nf * 2 * sizeof(float));  // hdf_in_bwd_blocks <= 1024, C <= 8 nf
  p->inb_k = bp.take((size_t)3 * B * 8 * nf * sizeof(float));
  p->inb_partials2 = bp.take((size_t)B * 1024 * 8 * nf * 2 * sizeof(float));
  p->inb_k2 = bp.take((size_t)3 * B * 8 * nf * sizeof(float));
  p->inb_k3 = bp.take((size_t)3 * B * 8 * nf * sizeof(float));
  for (int k = 0; k < 4; k++) {
    // (named for tools/cos_probe.py: after a backward g.y_<k> holds the raw-output gradient of the encoder's SECOND conv of
    // level k and g.a_<k> the gradient of its input activation -- the last writers of the two buffers)
    p->gA[k] = mkview(p, bp, "g.a_" + std::to_string(k), k, ch[k], B);
    p->gY[k] = mkview(p, bp, "g.y_" + std::to_string(k), k, ch[k], B);
    p->gY2[k] = mkview(p, bp, "g.y2_" + std::to_string(k), k, ch[k], B);  // the level's second conv keeps its own dy (read by a side-stream wgrad)
    if (k < 3) {
      // gradient of cat_k = [upconv | ds]: two dense buffers when the halves are whole 32-channel blocks (every
      // consumer of a half -- InstanceNorm backward, max-pool backward, up-sampling backward, the transposed conv's
      // backward -- then streams whole lines instead of 64 of every 128 bytes), else one buffer with views
      p->dcat_split[k] = ch[k] % 32 == 0;
      if (p->dcat_split[k]) {
        p->dUp[k] = mkview(p, bp, "g.up" + std::to_string(k + 1), k, ch[k], B);
        p->dSkip[k] = mkview(p, bp, "g.ds" + std::to_string(k), k, ch[k], B);
        p->dCat[k] = p->dUp[k];
      } else {
        p->dCat[k] = mkview(p, bp, "g.cat" + std::to_string(k + 1), k, 2 * ch[k], B);
        p->dUp[k] = hdf_plan_subview(p, p->dCat[k], 0, ch[k]);
        p->dSkip[k] = hdf_plan_subview(p, p->dCat[k], ch[k], ch[k]);
      }
      p->dP[k] = mkview(p, bp, "g.pool" + std::to_string(k + 1), k + 1, ch[k], B);
    }
  }
  // UpConv chain: conv outputs live at levels 4,3,2,1 with channels 8nf,4nf,2nf,nf
  const int uc[4] = {8 * nf, 4 * nf, 2 * nf, nf};
  for (int k = 0; k < 4; k++) {
    p->dUa[k] = mkview(p, bp, "", 4 - k, uc[k], B);
    p->dUy[k] = mkview(p, bp, "", 4 - k, uc[k], B);
  }
  p->dX4 = mkview(p, bp, "g.attnout", 3, 8 * nf, B);
  p->dAttnall = mkview(p, bp, "g.attnall", 4, p->M * p->DM, B);
  p->ws_bytes = bp.cur;
}

extern "C" {

static int create_plan(int in_channels, int n_cls, int n_filters, int D, int H, int W, int transformer_depth, int dtype,
                       bool is2d, hdf_plan** out, bool flat = false) {
  HDF_CHECK_ARG(out != nullptr, "plan_create: null out");
  HDF_CHECK_ARG(in_channels >= 1 && in_channels <= 8, "plan_create: in_channels=%d unsupported (1..8)", in_channels);
  HDF_CHECK_ARG(n_cls >= 2 && n_cls <= 8, "plan_create: n_cls=%d unsupported (2..8)", n_cls);
  HDF_CHECK_ARG(n_filters >= 16 && n_filters % 16 == 0 && n_filters <= 64,
                "plan_create: n_filters=%d unsupported (multiple of 16, 16..64)", n_filters);
  HDF_CHECK_ARG(D % 16 == 0 && H % 16 == 0 && W % 16 == 0 && (D >= 32 || is2d) && H >= 32 && W >= 32,
                "plan_create: image_size (%d,%d,%d) must be multiples of 16 and >= 32", D, H, W);
  HDF_CHECK_ARG(transformer_depth >= 4, "plan_create: transformer_depth=%d < 4", transformer_depth);
  HDF_CHECK_ARG(dtype == HDF_F32 || dtype == HDF_BF16 || dtype == HDF_F16, "plan_create: dtype %d", dtype);
  hdf_plan* p = new hdf_plan();
  p->M = in_channels;
  p->ncls = n_cls;
  p->nf = n_filters;
  p->D = D, p->H = H, p->W = W;
  p->td = transformer_depth;
  p->nb = transformer_depth / 4;
  p->dtype = dtype;
  p->esz = hdf_esz(dtype);
  for (int l = 0; l < 5; l++) p->dims[l][0] = D >> l, p->dims[l][1] = H >> l, p->dims[l][2] = W >> l;
  p->flat = is2d && flat;
  if (p->flat)   // (p->D stays 16: the depth of the patch embedding's input copy)
    for (int l = 0; l < 5; l++) p->dims[l][0] = 1;
  p->DM = 4 * n_filters;
  p->DMF = p->DM + 128;
  p->Ntok = (D / 16) * (H / 16) * (W / 16);
  build_params(p);
  int rc = build_tf_tables(p);
  build_layers(p);
  p->is2d = is2d;
  if (rc == HDF_OK && is2d) rc = build_params2d(p);
  if (rc != HDF_OK) {
    delete p;
    return rc;
  }
  *out = p;
  return HDF_OK;
}

int hdf_plan_create(int in_channels, int n_cls, int n_filters, int D, int H, int W, int transformer_depth, int dtype,
                    hdf_plan** out) {
  return create_plan(in_channels, n_cls, n_filters, D, H, W, transformer_depth, dtype, false, out);
}
int hdf_plan_create_2d_embedded(int in_channels, int n_cls, int n_filters, int H, int W, int transformer_depth, int dtype,
                               hdf_plan** out) {
  return create_plan(in_channels, n_cls, n_filters, 16, H, W, transformer_depth, dtype, true, out, false);
}
int hdf_plan_create_2d(int in_channels, int n_cls, int n_filters, int H, int W, int transformer_depth, int dtype,
                       hdf_plan** out) {
  return create_plan(in_channels, n_cls, n_filters, 16, H, W, transformer_depth, dtype, true, out, true);
}

void hdf_plan_destroy(hdf_plan* p) { delete p; }
int64_t hdf_plan_num_params(const hdf_plan* p) { return (int64_t)(p->is2d ? p->params2d : p->params).size(); }
int64_t hdf_plan_param_floats(const hdf_plan* p) { return p->is2d ? p->total_floats2d : p->total_floats; }

int hdf_plan_param_info(const hdf_plan* p, int64_t idx, char* name, int name_cap, int64_t* offset, int64_t* numel,
                        int* ndim, int64_t* shape5) {
  const std::vector<ParamInfo>& tbl = p->is2d ? p->params2d : p->params;
  HDF_CHECK_ARG(idx >= 0 && idx < (int64_t)tbl.size(), "param_info: index %lld", (long long)idx);
  const ParamInfo& pi = tbl[idx];
  if (name && name_cap > 0) {
    strncpy(name, pi.name.c_str(), name_cap - 1);
    name[name_cap - 1] = 0;
  }
  if (offset) *offset = pi.offset;
  if (numel) *numel = pi.numel;
  if (ndim) *ndim = (int)pi.shape.size();
  if (shape5)
    for (size_t i = 0; i < 5; i++) shape5[i] = i < pi.shape.size() ? pi.shape[i] : 1;
  return HDF_OK;
}

int64_t hdf_plan_workspace_bytes(hdf_plan* p, int batch) {
  hdf_plan_layout(p, batch);
  return (int64_t)p->ws_bytes;
}
int64_t hdf_plan_inference_workspace_bytes(hdf_plan* p, int batch) {
  hdf_plan_layout(p, batch);
  return (int64_t)p->ws_fwd_bytes;
}

int hdf_plan_buffer_info(hdf_plan* p, int batch, const char* name, int64_t* byte_offset, int64_t* pitch_elems,
                         int* channels, int* d, int* h, int* w) {
  hdf_plan_layout(p, batch);
  auto it = p->bufs.find(name);
  HDF_CHECK_ARG(it != p->bufs.end(), "buffer_info: no buffer named '%s'", name);
  const View& v = it->second;
  *byte_offset = (int64_t)v.off;
  *pitch_elems = v.pitch;
  *channels = v.C;
  *d = p->dims[v.lvl][0];
  *h = p->dims[v.lvl][1];
  *w = p->dims[v.lvl][2];
  return HDF_OK;
}

int hdf_plan_region_info(hdf_plan* p, int batch, const char* name, int64_t* byte_offset, int64_t* bytes) {
  HDF_CHECK_ARG(p && name && byte_offset && bytes, "region_info: null argument");
  hdf_plan_layout(p, batch);
  const int64_t rows = (int64_t)p->M * batch * p->Ntok;
  const std::string n = name;
  if (n == "tf_F") *byte_offset = (int64_t)p->tf_F, *bytes = (int64_t)p->nb * rows * p->DMF * 4;
  else if (n == "tf_save") *byte_offset = (int64_t)p->tf_save, *bytes = (int64_t)p->nb * 4 * rows * 232 * 4;
  else if (n == "tf_sync") *byte_offset = (int64_t)p->tf_sync, *bytes = (int64_t)3 << 20;
  else if (n == "tf_dF") *byte_offset = (int64_t)p->tf_dF, *bytes = rows * p->DMF * 4;
  else if (n == "tf_tape") *byte_offset = (int64_t)p->tf_tape, *bytes = (int64_t)p->nb * 4 * rows * TF_TAPE_W * 4;
  else if (n == "tf_otape") *byte_offset = (int64_t)p->tf_otape, *bytes = (int64_t)p->nb * rows * p->DMF * 4;
  else {
    hdf_set_error("region_info: no region named '%s'", name);
    return HDF_ERR_ARG;
  }
  return HDF_OK;
}

int hdf_plan_grad_bucket(const hdf_plan* p, int k, int64_t* lo, int64_t* hi) {
  HDF_CHECK_ARG(p && lo && hi && k >= 0 && k < HDF_NUM_GRAD_BUCKETS, "plan_grad_bucket: bucket 0..%d", HDF_NUM_GRAD_BUCKETS - 1);
  HDF_CHECK_ARG(!p->is2d, "plan_grad_bucket: the 2-D plan's gradients are final together (one bucket: the whole buffer)");
  // state_dict order: attns.* | deep_conv, up1..3 | block_1_*_left | block_2_*_left .. block_4_*_left | upconv_3 .. heads
  const int64_t chain = p->P("deep_conv.double_conv.0.weight"), enc0 = p->P("block_1_1_left.conv.weight"),
                enc1 = p->P("block_2_1_left.conv.weight"), dec = p->P("upconv_3.weight"), end = p->total_floats;
  HDF_CHECK_ARG(0 < chain && chain < enc0 && enc0 < enc1 && enc1 < dec && dec < end, "plan_grad_bucket: unexpected parameter order");
  const int64_t b[HDF_NUM_GRAD_BUCKETS][2] = {{dec, end}, {chain, enc0}, {0, chain}, {enc1, dec}, {enc0, enc1}};
  *lo = b[k][0], *hi = b[k][1];
  return HDF_OK;
}

}  // extern "C"
