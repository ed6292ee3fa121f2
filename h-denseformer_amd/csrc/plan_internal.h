// The plan's types and the few functions its units call across each other (private to csrc/: not installed).
//   plan.hip     parameter table, layer table, workspace carving, the hdf_plan_* queries (host arithmetic only)
//   embed2d.hip  the 2-D embedding's kernels and launchers
//   exec.hip     the U-Net layer helpers, the forward / backward launch sequences, the rest of the C ABI
//   exec_tf.hip  the transformer branches' launch sequences and the persistent kernels' give-up handling
//   (exec_internal.h: what those two share -- Exec (streams, event ring), Rejoin, Xf)
#pragma once
#include <map>
#include <string>
#include <vector>

#include "../../include/hdf.h"
#include "conv_igemm.h"
#include "transformer.h"

// (a named namespace: the inline members and container instantiations of these types are weak symbols in the shared
// library's dynamic table, where a bare `View` invites a collision)
namespace hdf_internal {

struct ParamInfo {
  std::string name;
  std::vector<int64_t> shape;
  int64_t offset, numel;
};

struct View {  // channels-last view into the workspace
  size_t off = 0;
  int64_t pitch = 0;
  int C = 0;
  int lvl = 0;
};

struct Stats {  // per conv layer InstanceNorm statistics, each [B][C] floats
  size_t mean = 0, rstd = 0, scale = 0, shift = 0;
};

struct Conv3 {  // 3x3x3 conv + InstanceNorm (+ReLU)
  std::string name;
  int Cin = 0, CinP = 0, Cout = 0, lvl = 0;
  int64_t w = -1, b = -1, gamma = -1, beta = -1;
  View y;
  Stats st;
  size_t wf = 0, wd = 0;  // packed forward / dgrad weights
  int wf_frag = 0, wd_frag = 0;  // their layout (hdf_conv_weight_layout of the launch that reads them)
};
struct ConvT3 {
  std::string name;
  int Cin = 0, Cout = 0, lvl_in = 0;
  int64_t w = -1, b = -1;
  size_t wf = 0, wd = 0;
  int wf_frag = 0, wd_frag = 0;
};
struct Head1 {
  std::string name;
  int C = 0, lvl = 0;
  int64_t w = -1, b = -1;
};

struct Bump {
  size_t cur = 0;
  size_t take(size_t bytes) {
    size_t o = cur;
    cur += (bytes + 255) & ~(size_t)255;
    return o;
  }
};

}  // namespace hdf_internal
using namespace hdf_internal;

// one tensor of the 2-D embedding (embed2d.hip)
struct Embed2dJob {
  int64_t off3, off2;  // float offsets in the 3-D / 2-D flat parameter (or gradient) buffers
  int64_t n3;          // 3-D elements of the job
  int inner;           // elements of one 2-D kernel (9, 256) or 1
  short rep;           // depth taps / slices of the 3-D kernel (3, 16) or 1
  char kind;           // 0 copy, 1 conv (tap 1), 2 transposed conv (taps 1 and 2), 3 patch (slice 0)
  char stage;          // backward stage bit (1 U-Net, 2 UpConv chain, 4 transformer) whose gradients it carries
};
constexpr int HDF_MAX_EMBED_JOBS = 96;

struct hdf_plan {
  int M, ncls, nf, D, H, W, td, nb, dtype;
  int esz;
  int dims[5][3];
  int DM, DMF, Ntok;
  std::vector<ParamInfo> params;
  std::map<std::string, int64_t> pidx;
  int64_t total_floats = 0;
  int64_t mstride = 0;
  // Transformer parameter addressing, resolved from the names once at creation (plan.hip: build_tf_tables, which also checks
  // that every block is spaced as tf_cp says): the persistent kernels' offsets, tf_wgrad's matrices, the patch embedding
  TfChainP tf_cp{};
  TfWgradEntry tf_wg[TF_WG_ENTRIES];
  int64_t pe_w = -1, pe_b = -1, pe_pos = -1;
  // layers
  Conv3 deep, up[3], enc[4][2], dec[3][2];  // dec[k]: level k (0..2) right blocks
  ConvT3 upc[3];                            // upc[k] produces level k from level k+1
  Head1 head[4];
  std::vector<PackJob> pack_jobs;           // every conv's forward and dgrad weight pack (one launch per forward)
  // layout for the current batch
  int batch = -1;
  size_t ws_bytes = 0;
  size_t ws_fwd_bytes = 0;  // prefix of the workspace a forward-only (inference) call touches
  std::map<std::string, View> bufs;
  // forward buffers
  View xin, attnall, attnout, at[3] /*at[k] lives at level k*/, cat[3], pooled[3], x4;
  size_t pool_idx[3];
  size_t tf_F, tf_save, tf_scratch, tf_dF, tf_tape = 0, tf_otape = 0;
  size_t tf_sync = 0;   // arrival counters of the persistent transformer kernels (tf_chain.h)
  size_t tf_frag = 0;   // operand records the forward leaves for the attention backward (16-bit modes)
  size_t tf_wpack = 0;  // fragment-major copies of the dense layers' weight matrices for those kernels
  size_t stat_partials, wgrad_ws, inb_partials, inb_k;
  size_t stat_partials2 = 0, inb_partials2 = 0, inb_k2 = 0;  // the same scratch for the branch stream (see Exec::branch)
  size_t inb_k3 = 0;  // k1 / ka / kb of the first layer's InstanceNorm backward: read by its weight gradient on the SIDE stream,
                      // i.e. possibly after the caller's stream has run the next in_backward (which reuses inb_k)
  size_t ksplit_ws = 0, ksplit_ws2 = 0;                      // split-K partial tiles of the low-resolution convs, per stream
  size_t wgrad_ws_bytes = 0;
  // backward scratch
  View gA[4], gY[4], gY2[4], dCat[3], dUp[3], dSkip[3], dP[3], dUa[4], dUy[4], dX4, dAttnall;
  // Side stream of the backward pass (weight gradients; see Exec::wgrad_stream) and a ring of its events.  Created
  // lazily on first use, destroyed with the plan.
  hipStream_t side = nullptr;
  // Branch stream: the multi-path transformer + UpConv chain (forward), their backward (HDenseFormer.py:230-235), next
  // to the level-0 encoder convolutions the caller's stream runs meanwhile (forward3d / backward3d).
  hipStream_t branch = nullptr;
  std::vector<hipEvent_t> events;
  size_t ev_next = 0;
  // "gradient bucket k is final" (hdf_backward_events): recorded on whichever stream of the call finishes the bucket
  hipEvent_t bucket_ev[HDF_NUM_GRAD_BUCKETS] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  // hdf_plan_set_probe: caller-owned events recorded around the dominant conv launch of the forward (measurement only)
  hipEvent_t probe_start = nullptr, probe_stop = nullptr;
  // Persistent transformer kernels (tf_chain.h: chain_wait).  chain_flag: one host-mapped word a launch writes (system
  // scope) when one of its per-sequence barriers gives up; read by the next forward / backward call of the plan without
  // synchronising (chain_flag_check).  chain_off: sticky -- after a give-up the plan runs the launch chain.
  // tf_fwd_chain: which arrangement the LAST forward ran; its backward follows it (the operand records and the
  // fragment-major weight copies of the persistent backward exist only behind a persistent forward).
  unsigned* chain_flag = nullptr;      // host address
  unsigned* chain_flag_dev = nullptr;  // device address of the same word
  bool chain_off = false;
  bool chain_forced = false;           // hdf_plan_force_persistent (tests): skip the residency check
  bool tf_fwd_chain = false;
  bool tf_bwd_chain = false;           // the last backward ran the persistent kernel (its timeout word is valid)
  unsigned chain_last_giveup = 0;      // 1 + workgroup id of the last give-up seen (hdf_plan_chain_state)
  unsigned chain_ticks = 150000000u;   // deadline of one barrier wait, 100 MHz ticks (hdf_plan_set_chain_timeout_us)
  ~hdf_plan() {
    if (chain_flag) (void)hipHostFree(chain_flag);
    for (hipEvent_t ev : bucket_ev)
      if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : events) (void)hipEventDestroy(ev);
    if (side) (void)hipStreamDestroy(side);
    if (branch) (void)hipStreamDestroy(branch);
  }
  bool dcat_split[3] = {false, false, false};
  // ---- 2-D model (models/HDenseFormer_2D.py) run as its exact depth-replicated 3-D embedding (see embed2d.hip)
  bool is2d = false;
  // Round 6: the 2-D model runs NATIVELY on depth-1 tensors (flat): every level has depth 1, the convolutions / transposed
  // convolutions / weight gradients are the FLAT instantiations of conv_igemm.hip / conv_s2.hip / conv_wgrad.hip (conv_wgrad_kernel; centre-plane taps of the embedded 27-tap
  // panels), pooling and up-sampling their 2-D forms (pool_ops.hip), the patch embedding contracts depth slice 0 of the
  // embedded 16^3 kernels with the input's 16 x 16 patches (K = 256).  flat = false keeps the depth-16
  // replicated embedding of rounds 3-5 (hdf_plan_create_2d_embedded: the oracle of tests/test_gpu_model_2d.py).
  bool flat = false;
  std::vector<ParamInfo> params2d;  // the 2-D reference state_dict: conv kernels [..,3,3], patch kernels [..,16,16]
  int64_t total_floats2d = 0;
  std::vector<Embed2dJob> ejobs;
  size_t e_x3d = 0, e_params3d = 0, e_grads3d = 0, e_out3d[4] = {0, 0, 0, 0}, e_dout3d[4] = {0, 0, 0, 0};
  // state carried from forward to backward
  int training = 0;
  uint32_t seed = 0;

  int64_t vox(int lvl) const { return (int64_t)dims[lvl][0] * dims[lvl][1] * dims[lvl][2]; }
  int64_t P(const std::string& n) const {
    auto it = pidx.find(n);
    return it == pidx.end() ? -1 : params[it->second].offset;
  }
};

// plan.hip
void hdf_plan_layout(hdf_plan* p, int B);
View hdf_plan_subview(hdf_plan* p, const View& v, int c0, int C, const std::string& name = "");
// embed2d.hip
int hdf_launch_embed2d(hdf_plan* p, const float* p2, float* p3, hipStream_t st);
int hdf_launch_extract2d(hdf_plan* p, int stages, const float* g3, float* g2, hipStream_t st);
int hdf_launch_replicate_depth(const float* x2, float* x3, int64_t rows, int reps, int64_t hw, hipStream_t st);
int hdf_launch_depth_slice(int dtype, void* t3, void* t2, int64_t rows, int reps, int64_t hw, int to2d, hipStream_t st);
