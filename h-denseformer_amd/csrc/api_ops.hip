// Process state (last error, compute-unit budget) and the one-to-one C ABI wrappers of the operator launchers that work on
// activations, logits and parameters: losses, the Dice and confusion counts, normalisation, sliding-window and slice-wise
// inference, augmentation, Adam and the flat optimizer step, and the single operators hdf_op_*.  The entries on a label
// volume (surface distances, components, overlap table, morphology) are in api_volume.hip.  Nothing here touches a plan.
#include <atomic>
#include <algorithm>
#include <cstdarg>
#include <cstring>

#include "../../include/hdf.h"
#include "augment.h"
#include "conv_igemm.h"
#include "loss.h"
#include "metrics.h"
#include "optim.h"
#include "transformer.h"
#include "unet_ops.h"

static thread_local char g_err[1024] = "";
// process-wide (relaxed atomic): forward runs on the caller's thread and backward on autograd's worker thread, and both
// must size their grids -- and take their split-K decisions -- from the same value
static std::atomic<int> g_cu_budget{256};
// The budget is capped by what the CURRENT DEVICE has (round 6): on a partitioned MI355X (DPX / QPX / CPX: 128 /
// 64 / 32 compute units) or any smaller gfx950 part a literal 256 let the persistent transformer kernels -- whose
// per-sequence barriers need every workgroup resident at once -- launch a grid that could never be resident together.
// hdf_set_cu_budget stays a DOWNWARD override.  No device (CPU-only layout queries): the literal.
static int device_cus() {
  static std::atomic<int> cache[16];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 256;
  int v = cache[dev].load(std::memory_order_relaxed);
  if (v > 0) return v;
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 256;
  if (n >= 8) n &= ~7;   // grids of the persistent conv kernels are split over the 8 XCDs
  cache[dev].store(n, std::memory_order_relaxed);
  return n;
}
int hdf_cu_budget() { return std::min(g_cu_budget.load(std::memory_order_relaxed), device_cus()); }

void hdf_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ================================================================================================ C ABI
extern "C" {

const char* hdf_version(void) { return "hdf-hip 0.1 (gfx950)"; }
int hdf_set_cu_budget(int cus) {
  HDF_CHECK_ARG(cus >= 8 && cus <= 256 && cus % 8 == 0, "cu budget %d: a multiple of 8 in [8, 256]", cus);
  g_cu_budget.store(cus, std::memory_order_relaxed);
  return HDF_OK;
}
const char* hdf_last_error(void) { return g_err; }

// ---------------------------------------------------------------------------------------- loss / metric / adam
int64_t hdf_loss_workspace_bytes(int batch) { return (int64_t)hdf_loss_workspace_floats(batch, 4) * sizeof(float); }

int hdf_loss_forward(int dtype, const void* out0, const void* out1, const void* out2, const void* out3, int nscale,
                     const float* target_onehot, int batch, int n_cls, int D, int H, int W, void* workspace,
                     float* loss_out, hdf_stream stream) {
  const void* outs[4] = {out0, out1, out2, out3};
  return hdf_launch_loss_fwd(dtype, outs, target_onehot, nscale, batch, n_cls, D, H, W, (float*)workspace, loss_out,
                             (hipStream_t)stream);
}
int hdf_loss_backward(int dtype, const void* out0, const void* out1, const void* out2, const void* out3, int nscale,
                      const float* target_onehot, int batch, int n_cls, int D, int H, int W, const void* workspace,
                      const float* grad_out, void* dout0, void* dout1, void* dout2, void* dout3, hdf_stream stream) {
  const void* outs[4] = {out0, out1, out2, out3};
  void* douts[4] = {dout0, dout1, dout2, dout3};
  return hdf_launch_loss_bwd(dtype, outs, target_onehot, nscale, batch, n_cls, D, H, W, (const float*)workspace,
                             grad_out, douts, (hipStream_t)stream);
}
int hdf_loss_terms_forward(int dtype, const void* out0, const void* out1, const void* out2, const void* out3, int nscale,
                           const float* target_onehot, int batch, int n_cls, int D, int H, int W, float ce_weight,
                           float dice_weight, void* workspace, float* loss_out, hdf_stream stream) {
  const void* outs[4] = {out0, out1, out2, out3};
  return hdf_launch_loss_fwd(dtype, outs, target_onehot, nscale, batch, n_cls, D, H, W, (float*)workspace, loss_out,
                             (hipStream_t)stream, ce_weight, dice_weight);
}
int hdf_loss_terms_backward(int dtype, const void* out0, const void* out1, const void* out2, const void* out3,
                            int nscale, const float* target_onehot, int batch, int n_cls, int D, int H, int W,
                            float ce_weight, float dice_weight, const void* workspace, const float* grad_out,
                            void* dout0, void* dout1, void* dout2, void* dout3, hdf_stream stream) {
  const void* outs[4] = {out0, out1, out2, out3};
  void* douts[4] = {dout0, dout1, dout2, dout3};
  return hdf_launch_loss_bwd(dtype, outs, target_onehot, nscale, batch, n_cls, D, H, W, (const float*)workspace,
                             grad_out, douts, (hipStream_t)stream, ce_weight, dice_weight);
}
int hdf_loss_weighted_forward(int dtype, const void* out0, const void* out1, const void* out2, const void* out3,
                              int nscale, const float* target_onehot, int batch, int n_cls, int D, int H, int W,
                              float ce_weight, float dice_weight, const float* class_weight, int dice_ignore_index,
                              void* workspace, float* loss_out, hdf_stream stream) {
  const void* outs[4] = {out0, out1, out2, out3};
  return hdf_launch_loss_fwd(dtype, outs, target_onehot, nscale, batch, n_cls, D, H, W, (float*)workspace, loss_out,
                             (hipStream_t)stream, ce_weight, dice_weight, class_weight, dice_ignore_index);
}
int hdf_loss_weighted_backward(int dtype, const void* out0, const void* out1, const void* out2, const void* out3,
                               int nscale, const float* target_onehot, int batch, int n_cls, int D, int H, int W,
                               float ce_weight, float dice_weight, const float* class_weight, int dice_ignore_index,
                               const void* workspace, const float* grad_out, void* dout0, void* dout1, void* dout2,
                               void* dout3, hdf_stream stream) {
  const void* outs[4] = {out0, out1, out2, out3};
  void* douts[4] = {dout0, dout1, dout2, dout3};
  return hdf_launch_loss_bwd(dtype, outs, target_onehot, nscale, batch, n_cls, D, H, W, (const float*)workspace,
                             grad_out, douts, (hipStream_t)stream, ce_weight, dice_weight, class_weight,
                             dice_ignore_index);
}
int hdf_loss_focal_forward(int dtype, const void* out0, const void* out1, const void* out2, const void* out3, int nscale,
                           const float* target_onehot, int batch, int n_cls, int D, int H, int W, float focal_weight,
                           float focal_alpha, float focal_gamma, int focal_reduction, float dice_weight,
                           const float* class_weight, int dice_ignore_index, void* workspace, float* loss_out,
                           hdf_stream stream) {
  const void* outs[4] = {out0, out1, out2, out3};
  return hdf_launch_loss_focal_fwd(dtype, outs, target_onehot, nscale, batch, n_cls, D, H, W, (float*)workspace,
                                   loss_out, (hipStream_t)stream, focal_weight, focal_alpha, focal_gamma,
                                   focal_reduction, dice_weight, class_weight, dice_ignore_index);
}
int hdf_loss_focal_backward(int dtype, const void* out0, const void* out1, const void* out2, const void* out3,
                            int nscale, const float* target_onehot, int batch, int n_cls, int D, int H, int W,
                            float focal_weight, float focal_alpha, float focal_gamma, int focal_reduction,
                            float dice_weight, const float* class_weight, int dice_ignore_index, const void* workspace,
                            const float* grad_out, void* dout0, void* dout1, void* dout2, void* dout3,
                            hdf_stream stream) {
  const void* outs[4] = {out0, out1, out2, out3};
  void* douts[4] = {dout0, dout1, dout2, dout3};
  return hdf_launch_loss_focal_bwd(dtype, outs, target_onehot, nscale, batch, n_cls, D, H, W, (const float*)workspace,
                                   grad_out, douts, (hipStream_t)stream, focal_weight, focal_alpha, focal_gamma,
                                   focal_reduction, dice_weight, class_weight, dice_ignore_index);
}
int hdf_dice_counts(int dtype, const void* logits, const float* target_onehot, int batch, int n_cls, int64_t voxels,
                    uint64_t* counts, hdf_stream stream) {
  return hdf_launch_dice_counts(dtype, logits, target_onehot, batch, n_cls, voxels, (unsigned long long*)counts,
                                (hipStream_t)stream);
}
int hdf_confusion_matrix(int dtype, const void* logits, const float* target_onehot, int batch, int n_cls,
                         int64_t voxels, uint64_t* confusion, int accumulate, hdf_stream stream) {
  return hdf_launch_confusion(dtype, logits, target_onehot, batch, n_cls, voxels, (unsigned long long*)confusion,
                              accumulate, (hipStream_t)stream);
}
int hdf_confusion_matrix_labels(const uint8_t* target, const uint8_t* prediction, int n_cls, int64_t n,
                                uint64_t* confusion, int accumulate, hdf_stream stream) {
  HDF_CHECK_ARG(target && prediction && confusion, "confusion_matrix_labels: null argument");
  return hdf_launch_confusion_labels(target, prediction, n_cls, n, (unsigned long long*)confusion, accumulate,
                                     (hipStream_t)stream);
}
int64_t hdf_normalize_workspace_bytes(int channels) { return (int64_t)hdf_norm_ws_bytes(channels); }
int hdf_normalize_mr(float* image, int channels, int64_t voxels, void* workspace, hdf_stream stream) {
  HDF_CHECK_ARG(image && workspace, "normalize_mr: null argument");
  return hdf_launch_normalize(image, channels, voxels, 0, 0.f, 1.f, workspace, (hipStream_t)stream);
}
int hdf_normalize_petct(float* image, int channels, int64_t voxels, float mean, float w, void* workspace,
                        hdf_stream stream) {
  HDF_CHECK_ARG(image && workspace, "normalize_petct: null argument");
  return hdf_launch_normalize(image, channels, voxels, 1, mean, w, workspace, (hipStream_t)stream);
}
int hdf_sw_accumulate(int dtype, const void* logits, int n_cls, int pd, int ph, int pw, float* prob_sum, float* count,
                      int D, int H, int W, int z0, int y0, int x0, hdf_stream stream) {
  HDF_CHECK_ARG(logits && prob_sum && count, "sw_accumulate: null argument");
  return hdf_launch_sw_accumulate(dtype, logits, n_cls, pd, ph, pw, prob_sum, count, D, H, W, z0, y0, x0,
                                  (hipStream_t)stream);
}
int hdf_sw_finalize(const float* prob_sum, const float* count, int n_cls, int64_t voxels, uint8_t* label,
                    hdf_stream stream) {
  HDF_CHECK_ARG(prob_sum && count && label, "sw_finalize: null argument");
  return hdf_launch_sw_finalize(prob_sum, count, n_cls, voxels, label, (hipStream_t)stream);
}
int hdf_sw_gather(const float* image, int channels, int D, int H, int W, int z0, int y0, int x0, int ed, int eh, int ew,
                  int Pd, int Ph, int Pw, unsigned mirror_mask, float* out, hdf_stream stream) {
  HDF_CHECK_ARG(image && out, "sw_gather: null argument");
  return hdf_launch_sw_gather(image, channels, D, H, W, z0, y0, x0, ed, eh, ew, Pd, Ph, Pw, mirror_mask, out,
                              (hipStream_t)stream);
}
int hdf_sw_importance_floor(const double* tables, int ed, int eh, int ew, float* floor_out, hdf_stream stream) {
  HDF_CHECK_ARG(tables && floor_out, "sw_importance_floor: null argument");
  return hdf_launch_sw_importance_floor(tables, ed, eh, ew, floor_out, (hipStream_t)stream);
}
int hdf_sw_accumulate_tta(int dtype, const void* logits, unsigned mirror_mask, int n_cls, int ed, int eh, int ew, int Pd,
                          int Ph, int Pw, const double* tables, const float* floor, float* prob_sum, float* weight_sum,
                          int D, int H, int W, int z0, int y0, int x0, hdf_stream stream) {
  HDF_CHECK_ARG(logits && prob_sum && weight_sum, "sw_accumulate_tta: null argument");
  return hdf_launch_sw_accumulate_tta(dtype, logits, mirror_mask, n_cls, ed, eh, ew, Pd, Ph, Pw, tables, floor, prob_sum,
                                      weight_sum, D, H, W, z0, y0, x0, (hipStream_t)stream);
}
int hdf_plane_max(const float* image, int planes, int64_t plane_voxels, float* max_out, hdf_stream stream) {
  HDF_CHECK_ARG(image && max_out, "plane_max: null argument");
  return hdf_launch_plane_max(image, planes, plane_voxels, max_out, (hipStream_t)stream);
}
int hdf_slice_gather(const float* image, int channels, int D, int H, int W, int z0, int nz, int y0, int x0, int eh, int ew,
                     int Ph, int Pw, unsigned mirror_mask, int norm_mode, const float* plane_max, float* out,
                     hdf_stream stream) {
  HDF_CHECK_ARG(image && out, "slice_gather: null argument");
  return hdf_launch_slice_gather(image, channels, D, H, W, z0, nz, y0, x0, eh, ew, Ph, Pw, mirror_mask, norm_mode, plane_max,
                                 out, (hipStream_t)stream);
}
int hdf_slice_accumulate(int dtype, const void* logits, unsigned mirror_mask, int n_cls, int nz, int eh, int ew, int Ph,
                         int Pw, const double* tables, float floor, float* prob_sum, float* weight_sum, int D, int H, int W,
                         int z0, int y0, int x0, hdf_stream stream) {
  HDF_CHECK_ARG(logits && prob_sum && weight_sum, "slice_accumulate: null argument");
  return hdf_launch_slice_accumulate(dtype, logits, mirror_mask, n_cls, nz, eh, ew, Ph, Pw, tables, floor, prob_sum,
                                     weight_sum, D, H, W, z0, y0, x0, (hipStream_t)stream);
}
int hdf_onehot_from_labels(const uint8_t* labels, float* onehot, int batch, int n_cls, int64_t voxels,
                           hdf_stream stream) {
  HDF_CHECK_ARG(labels && onehot, "onehot_from_labels: null argument");
  return hdf_launch_onehot(labels, onehot, batch, n_cls, voxels, (hipStream_t)stream);
}
int hdf_augment_3d(const float* image, const uint8_t* labels, int channels, int n_cls, int D, int H, int W,
                   const double* affine, int flip_h, int flip_w, float* image_out, uint8_t* labels_out, float* onehot_out,
                   hdf_stream stream) {
  HDF_CHECK_ARG(affine, "augment_3d: null affine");
  AugAffine a;
  std::memcpy(a.m, affine, sizeof(a.m));   // read during the call: the caller may reuse the array at once
  return hdf_launch_augment3d(image, labels, channels, n_cls, D, H, W, a, flip_h, flip_w, image_out, labels_out,
                              onehot_out, (hipStream_t)stream);
}
int hdf_augment_2d(const float* image, const uint8_t* labels, int batch, int channels, int n_cls, int H, int W,
                   const double* matrices, const uint8_t* flips, float* image_out, uint8_t* labels_out, float* onehot_out,
                   hdf_stream stream) {
  HDF_CHECK_ARG(matrices, "augment_2d: null matrices");
  HDF_CHECK_ARG(flips, "augment_2d: null flips");
  // both host arrays are copied into the kernel arguments chunk by chunk: the caller may reuse them at once
  return hdf_launch_augment2d(image, labels, batch, channels, n_cls, H, W, matrices, flips, image_out, labels_out,
                              onehot_out, (hipStream_t)stream);
}
int64_t hdf_label_bbox_workspace_bytes(int batch) { return (int64_t)hdf_label_bbox_ws_bytes(batch); }
int hdf_label_bbox_2d(const uint8_t* labels, int batch, int H, int W, int32_t* bbox, void* workspace,
                      int64_t workspace_bytes, hdf_stream stream) {
  HDF_CHECK_ARG(labels && bbox && workspace, "label_bbox_2d: null argument");
  HDF_CHECK_ARG(workspace_bytes >= (int64_t)hdf_label_bbox_ws_bytes(batch),
                "label_bbox_2d: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)hdf_label_bbox_ws_bytes(batch));
  return hdf_launch_label_bbox2d(labels, batch, H, W, bbox, workspace, (hipStream_t)stream);
}
int hdf_zoom_2d(const float* image, const uint8_t* labels, int batch, int channels, int H, int W, const int32_t* keep,
                const int32_t* canvas, float* image_out, uint8_t* labels_out, hdf_stream stream) {
  HDF_CHECK_ARG(keep, "zoom_2d: null keep");
  HDF_CHECK_ARG(canvas, "zoom_2d: null canvas");
  // both host arrays are copied into the kernel arguments chunk by chunk: the caller may reuse them at once
  return hdf_launch_zoom2d(image, labels, batch, channels, H, W, keep, canvas, image_out, labels_out,
                           (hipStream_t)stream);
}
int hdf_intensity_2d(float* image, int batch, int channels, int H, int W, const double* gamma, const uint8_t* noise,
                     uint64_t seed, float low_clip, hdf_stream stream) {
  HDF_CHECK_ARG(image && gamma && noise, "intensity_2d: null argument");
  HDF_CHECK_ARG(H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "intensity_2d: plane %dx%d (1..16384 a side)", H, W);
  HDF_CHECK_ARG(channels >= 1 && channels <= 64, "intensity_2d: channels=%d (1..64)", channels);
  return hdf_launch_intensity2d(image, batch, (int64_t)channels * H * W, gamma, noise, seed, low_clip,
                                (hipStream_t)stream);
}
int64_t hdf_resize_workspace_bytes(int Di, int Hi, int Wi, int Do, int Ho, int Wo) {
  return hdf_resize_ws_bytes(Di, Hi, Wi, Do, Ho, Wo);
}
int hdf_resize_3d(const float* image, const uint8_t* labels, int channels, int n_cls, int Di, int Hi, int Wi, int Do, int Ho,
                  int Wo, float* image_out, uint8_t* labels_out, void* workspace, int64_t workspace_bytes,
                  hdf_stream stream) {
  return hdf_launch_resize3d(image, labels, channels, n_cls, Di, Hi, Wi, Do, Ho, Wo, image_out, labels_out, workspace,
                             workspace_bytes, (hipStream_t)stream);
}
int hdf_trunc_normalize(float* image, int64_t n, float lo, float hi, hdf_stream stream) {
  return hdf_launch_trunc_normalize(image, n, lo, hi, (hipStream_t)stream);
}
int hdf_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const uint8_t* decay_mask,
                  int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                  float grad_scale, hdf_stream stream) {
  HDF_CHECK_ARG(step >= 1, "adam: step=%d must start at 1", step);
  return hdf_launch_adam(params, grads, exp_avg, exp_avg_sq, decay_mask, n, lr, beta1, beta2, eps, weight_decay, step,
                         grad_scale, (hipStream_t)stream);
}
int hdf_optim_step(int rule, float* params, const float* grads, float* state1, float* state2, const uint8_t* decay_mask,
                   int64_t n, float lr_decay, float lr_rest, float wd_decay, float wd_rest, float beta1, float beta2,
                   float eps, int nesterov, float grad_mul, const float* grad_scale, const float* found_inf,
                   int32_t* step_state, hdf_stream stream) {
  return hdf_launch_optim(rule, params, grads, state1, state2, decay_mask, n, lr_decay, lr_rest, wd_decay, wd_rest, beta1,
                          beta2, eps, nesterov, grad_mul, grad_scale, found_inf, step_state, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------- operator level
int hdf_op_to_channels_last(int dtype, const float* x, void* out, int N, int C, int CP, int64_t voxels,
                            hdf_stream stream) {
  return hdf_launch_nchw_to_ndhwc(dtype, x, out, N, C, CP, voxels, (hipStream_t)stream);
}
int hdf_op_pack_weights(int dtype, const float* src, void* dst, int O, int I, int OP, int IP, int64_t so, int64_t si,
                        int flip, hdf_stream stream) {
  return hdf_launch_pack_w(dtype, src, dst, O, I, OP, IP, so, si, flip, (hipStream_t)stream);
}
int hdf_op_conv3d(int dtype, int mode, const void* in, int64_t in_pitch, int Cin, int N, int Di, int Hi, int Wi,
                  const void* w_packed, const float* bias, const float* in_scale, const float* in_shift, int in_relu,
                  void* out, int64_t out_pitch, int Cout, float* stat_partials, int accumulate, hdf_stream stream) {
  ConvArgs a{};
  a.in = in;
  a.in_pitch = in_pitch;
  a.Cin = Cin;
  a.N = N;
  a.Di = Di, a.Hi = Hi, a.Wi = Wi;
  if (mode == 0)
    a.Do = Di, a.Ho = Hi, a.Wo = Wi;
  else if (mode == 1)
    a.Do = Di / 2, a.Ho = Hi / 2, a.Wo = Wi / 2;
  else
    a.Do = 2 * Di, a.Ho = 2 * Hi, a.Wo = 2 * Wi;
  if (Di == 1) a.Do = 1;   // depth 1 selects the 2-D operator: the depth axis is never strided (include/hdf.h)
  a.w = w_packed;
  a.bias = bias;
  a.in_scale = in_scale;
  a.in_shift = in_shift;
  a.in_relu = in_relu;
  a.out = out;
  a.out_pitch = out_pitch;
  a.Cout = Cout;
  a.CoutP = round_up(Cout, 32);
  a.stat_partials = stat_partials;
  a.accumulate = accumulate;
  return hdf_launch_conv(dtype, mode, a, (hipStream_t)stream);
}
int hdf_op_conv3d_bwd_stats(int dtype, const void* in, int64_t in_pitch, int Cin, int N, int D, int H, int W,
                            const void* w_packed, void* out, int64_t out_pitch, int Cout, const void* y, int64_t y_pitch,
                            const float* scale, const float* shift, const float* mean, const float* rstd,
                            float* partials, hdf_stream stream) {
  HDF_CHECK_ARG(in && w_packed && out && y && scale && shift && mean && rstd && partials, "conv3d_bwd_stats: null argument");
  ConvArgs a{};
  a.in = in, a.in_pitch = in_pitch, a.Cin = Cin, a.N = N;
  a.Di = a.Do = D, a.Hi = a.Ho = H, a.Wi = a.Wo = W;
  a.w = w_packed, a.out = out, a.out_pitch = out_pitch, a.Cout = Cout, a.CoutP = round_up(Cout, 32);
  a.stat_partials = partials;
  a.bs_y = y, a.bs_y_pitch = y_pitch, a.bs_scale = scale, a.bs_shift = shift, a.bs_mean = mean, a.bs_rstd = rstd;
  HDF_CHECK_ARG(hdf_conv_bwd_stats_ok(dtype, a), "conv3d_bwd_stats: this launch cannot take the statistics epilogue "
                "(16-bit storage, 32 -> 32 channels, whole 4x8x8 tiles, >= 48^3)");
  return hdf_launch_conv(dtype, 0, a, (hipStream_t)stream);
}
int hdf_op_conv3d_split(int dtype, const void* in, int64_t in_pitch, int Cin, int N, int D, int H, int W,
                        const void* w_packed, void* out, void* out2, int64_t out_pitch, int Cout, int split,
                        float* stat_partials, float* colsum, int colsum_C, hdf_stream stream) {
  HDF_CHECK_ARG(colsum == nullptr || (stat_partials != nullptr && colsum_C > 0 && colsum_C <= Cout),
                "conv3d_split: column sums need the statistics buffer and 0 < colsum_C <= Cout");
  ConvArgs a{};
  a.in = in;
  a.in_pitch = in_pitch;
  a.Cin = Cin;
  a.N = N;
  a.Di = a.Do = D, a.Hi = a.Ho = H, a.Wi = a.Wo = W;
  a.w = w_packed;
  a.out = out;
  a.out2 = out2;
  a.split = split;
  a.out_pitch = out_pitch;
  a.Cout = Cout;
  a.CoutP = round_up(Cout, 32);
  a.stat_partials = stat_partials;
  HDF_TRY(hdf_launch_conv(dtype, 0, a, (hipStream_t)stream));
  if (colsum) {
    const int rows = N * hdf_conv_stat_tiles(0, D, H, W, Cin * hdf_esz(dtype));
    HDF_TRY(hdf_launch_stat_rows_sum(stat_partials, rows, colsum_C, a.CoutP, colsum, (hipStream_t)stream));
  }
  return HDF_OK;
}
int hdf_op_conv3d_first(int dtype, const void* in, int64_t in_pitch, int Cin, int N, int D, int H, int W, const float* weight,
                        const float* bias, void* out, int64_t out_pitch, int Cout, float* stat_partials,
                        hdf_stream stream) {
  HDF_CHECK_ARG(in && weight && out, "conv3d_first: null argument");
  return hdf_launch_conv_first(dtype, in, in_pitch, Cin, N, D, H, W, weight, bias, out, out_pitch, Cout, stat_partials,
                               (hipStream_t)stream);
}
int hdf_op_conv3d_first_wgrad(int dtype, const void* dy, int64_t dy_pitch, int Cout, const void* x, int64_t x_pitch,
                              int Cin, int N, int D, int H, int W, float* dweight, int accumulate, void* workspace,
                              int64_t workspace_bytes, hdf_stream stream) {
  HDF_CHECK_ARG(dy && x && dweight && workspace, "conv3d_first_wgrad: null argument");
  return hdf_launch_wgrad_first(dtype, dy, dy_pitch, Cout, x, x_pitch, Cin, N, D, H, W, dweight, accumulate, workspace,
                                (size_t)workspace_bytes, (hipStream_t)stream);
}
int hdf_op_conv3d_first_wgrad_in(int dtype, const void* da, int64_t da_pitch, int Cout, const void* y, int64_t y_pitch,
                                 const float* scale, const float* shift, const float* mean, const float* rstd,
                                 const float* k1, const float* ka, const float* kb, const void* x, int64_t x_pitch, int Cin,
                                 int N, int D, int H, int W, float* dweight, int accumulate, void* workspace,
                                 int64_t workspace_bytes, hdf_stream stream) {
  HDF_CHECK_ARG(da && x && dweight && workspace, "conv3d_first_wgrad_in: null argument");
  const WgradFirstIn fi{y, y_pitch, scale, shift, mean, rstd, k1, ka, kb};
  return hdf_launch_wgrad_first(dtype, da, da_pitch, Cout, x, x_pitch, Cin, N, D, H, W, dweight, accumulate, workspace,
                                (size_t)workspace_bytes, (hipStream_t)stream, &fi);
}
int hdf_op_conv3d_wr(int dtype, const void* in, int64_t in_pitch, int Cin, int N, int D, int H, int W,
                     const void* w_packed, const float* bias, const float* in_scale, const float* in_shift, int in_relu,
                     void* out, int64_t out_pitch, int Cout, float* stat_partials, int accumulate, hdf_stream stream) {
  ConvArgs a{};
  a.in = in, a.in_pitch = in_pitch, a.Cin = Cin, a.N = N;
  a.Di = a.Do = D, a.Hi = a.Ho = H, a.Wi = a.Wo = W;
  a.w = w_packed, a.bias = bias, a.in_scale = in_scale, a.in_shift = in_shift, a.in_relu = in_relu;
  a.out = out, a.out_pitch = out_pitch, a.Cout = Cout, a.CoutP = round_up(Cout, 32);
  a.stat_partials = stat_partials, a.accumulate = accumulate;
  HDF_CHECK_ARG(a.in_pitch % 8 == 0 && (((uintptr_t)a.in) & 15) == 0, "conv_wr: input view must be 16-byte aligned");
  if (!hdf_conv_wr_can(dtype, a)) {
    hdf_set_error("conv3d_wr: shape not handled by the weights-in-registers kernel (dtype %d Cin %d %dx%dx%d)", dtype, Cin, D, H, W);
    return HDF_ERR_UNSUPPORTED;
  }
  return hdf_launch_conv_wr(dtype, a, (hipStream_t)stream);
}
int hdf_op_conv3d_stat_tiles(int dtype, int Cin, int Do, int Ho, int Wo) {
  return hdf_conv_stat_tiles(0, Do, Ho, Wo, Cin * hdf_esz(dtype));
}
int64_t hdf_op_wgrad_workspace_bytes(int stride, int N, int Ds, int Hs, int Ws, int SC, int LC) {
  return (int64_t)hdf_wgrad_workspace_bytes(stride, N, Ds, Hs, Ws, SC, LC);
}
int hdf_op_conv3d_wgrad(int dtype, int stride, const void* sm, int64_t sm_pitch, int SC, const void* lg,
                        int64_t lg_pitch, int LC, int N, int Ds, int Hs, int Ws, const float* sm_scale,
                        const float* sm_shift, int sm_relu, const float* lg_scale, const float* lg_shift, int lg_relu,
                        float* dw, int sc_store, int lc_store, int accumulate, void* workspace, int64_t workspace_bytes,
                        hdf_stream stream) {
  WgradArgs w{};
  w.sm = sm, w.sm_pitch = sm_pitch, w.SC = SC;
  w.lg = lg, w.lg_pitch = lg_pitch, w.LC = LC;
  w.N = N;
  w.Ds = Ds, w.Hs = Hs, w.Ws = Ws;
  w.Dl = Ds == 1 ? 1 : stride * Ds, w.Hl = stride * Hs, w.Wl = stride * Ws;   // (depth 1: the 2-D operator)
  w.sm_scale = sm_scale, w.sm_shift = sm_shift, w.sm_relu = sm_relu;
  w.lg_scale = lg_scale, w.lg_shift = lg_shift, w.lg_relu = lg_relu;
  return hdf_launch_wgrad(dtype, stride, w, dw, sc_store, lc_store, accumulate, workspace, (size_t)workspace_bytes,
                          (hipStream_t)stream);
}
int hdf_op_in_finalize(const float* partials, int N, int tiles, int C, int CP, int64_t voxels, const float* gamma,
                       const float* beta, float eps, float* mean, float* rstd, float* scale, float* shift,
                       hdf_stream stream) {
  return hdf_launch_in_finalize(partials, N, tiles, C, CP, voxels, gamma, beta, eps, NormStatsOut{scale, shift, mean, rstd},
                                (hipStream_t)stream);
}
int64_t hdf_op_in_bwd_workspace_floats(int N, int C, int64_t voxels) {
  return (int64_t)N * hdf_in_bwd_blocks(voxels, C) * C * 2 + (int64_t)3 * N * C;
}
int hdf_op_in_bwd(int dtype, const void* da, int64_t da_pitch, const void* y, int64_t y_pitch, const float* scale,
                  const float* shift, const float* mean, const float* rstd, const float* gamma, void* dy,
                  int64_t dy_pitch, float* dgamma, float* dbeta, int N, int C, int64_t voxels, float* workspace,
                  hdf_stream stream) {
  HDF_CHECK_ARG(da && y && scale && shift && mean && rstd && dy && workspace, "in_bwd: null argument");
  const int blocks = hdf_in_bwd_blocks(voxels, C);
  float* partials = workspace;
  float* k1 = workspace + (int64_t)N * blocks * C * 2;
  const InBwdCoefOut coef{k1, k1 + (int64_t)N * C, k1 + (int64_t)2 * N * C};
  const NormStats ys{scale, shift, mean, rstd};
  hipStream_t st = (hipStream_t)stream;
  HDF_TRY(hdf_launch_in_bwd_reduce(dtype, CRows{da, da_pitch}, CRows{y, y_pitch}, ys, partials, blocks, N, C, voxels, st));
  HDF_TRY(hdf_launch_in_bwd_finalize(partials, blocks, N, C, voxels, gamma, rstd, coef, dgamma, dbeta, st));
  return hdf_launch_in_bwd_apply(dtype, CRows{da, da_pitch}, CRows{y, y_pitch}, ys, coef, Rows{dy, dy_pitch}, N, C, voxels,
                                 st);
}
int hdf_op_in_bwd_wgrad(int dtype, const void* da, int64_t da_pitch, const void* y, int64_t y_pitch, const float* scale,
                        const float* shift, const float* mean, const float* rstd, const float* gamma, void* dy,
                        int64_t dy_pitch, float* dgamma, float* dbeta, const void* x, int64_t x_pitch, int Cin,
                        const float* x_scale, const float* x_shift, int x_relu, int N, int Cout, int D, int H, int W,
                        float* dw, float* workspace, void* wgrad_workspace, int64_t wgrad_workspace_bytes,
                        hdf_stream stream) {
  HDF_CHECK_ARG(da && y && scale && shift && mean && rstd && dy && x && dw && workspace && wgrad_workspace,
                "in_bwd_wgrad: null argument");
  const int64_t voxels = (int64_t)D * H * W;
  const int blocks = hdf_in_bwd_blocks(voxels, Cout);
  float* partials = workspace;
  float* k1 = workspace + (int64_t)N * blocks * Cout * 2;
  float* ka = k1 + (int64_t)N * Cout;
  float* kb = ka + (int64_t)N * Cout;
  hipStream_t st = (hipStream_t)stream;
  WgradArgs w{};
  w.sm = da, w.sm_pitch = da_pitch, w.SC = Cout;
  w.lg = x, w.lg_pitch = x_pitch, w.LC = Cin;
  w.N = N;
  w.Ds = w.Dl = D, w.Hs = w.Hl = H, w.Ws = w.Wl = W;
  w.lg_scale = x_scale, w.lg_shift = x_shift, w.lg_relu = x_relu;
  w.ap_y = y, w.ap_y_pitch = y_pitch, w.ap_out = dy, w.ap_out_pitch = dy_pitch;
  w.ap_tab[0] = scale, w.ap_tab[1] = shift, w.ap_tab[2] = mean, w.ap_tab[3] = rstd;
  w.ap_tab[4] = k1, w.ap_tab[5] = ka, w.ap_tab[6] = kb;
  if (!hdf_wgrad_apply_takes(dtype, 1, w)) {
    hdf_set_error("in_bwd_wgrad: the fused kernel does not take this launch (dtype %d, %d -> %d channels, %dx%dx%d)", dtype,
                  Cin, Cout, D, H, W);
    return HDF_ERR_UNSUPPORTED;
  }
  HDF_TRY(hdf_launch_in_bwd_reduce(dtype, CRows{da, da_pitch}, CRows{y, y_pitch}, NormStats{scale, shift, mean, rstd},
                                   partials, blocks, N, Cout, voxels, st));
  HDF_TRY(hdf_launch_in_bwd_finalize(partials, blocks, N, Cout, voxels, gamma, rstd, InBwdCoefOut{k1, ka, kb}, dgamma, dbeta,
                                     st));
  return hdf_launch_wgrad(dtype, 1, w, dw, Cout, Cin, 0, wgrad_workspace, (size_t)wgrad_workspace_bytes, st);
}
int hdf_op_norm_relu_add(int dtype, const void* y, int64_t y_pitch, const float* scale, const float* shift,
                         const void* skip, int64_t skip_pitch, void* out, int64_t out_pitch, int N, int C,
                         int64_t voxels, hdf_stream stream) {
  return hdf_launch_norm_relu_add(dtype, CRows{y, y_pitch}, NormStats{scale, shift}, CRows{skip, skip_pitch},
                                  Rows{out, out_pitch}, N, C, voxels, (hipStream_t)stream);
}
int hdf_op_maxpool_fwd(int dtype, const void* in, int64_t in_pitch, void* out, int64_t out_pitch, uint8_t* idx, int N,
                       int C, int Do, int Ho, int Wo, hdf_stream stream) {
  return hdf_launch_maxpool_fwd(dtype, CRows{in, in_pitch}, Rows{out, out_pitch}, idx, Extent{N, C, Do, Ho, Wo},
                                (hipStream_t)stream);
}
int hdf_op_enc_tail(int dtype, const void* y, int64_t y_pitch, const float* scale, const float* shift, const void* skip,
                    int64_t skip_pitch, void* ds, int64_t ds_pitch, void* pooled, int64_t pooled_pitch, uint8_t* idx,
                    int N, int C, int Do, int Ho, int Wo, hdf_stream stream) {
  HDF_CHECK_ARG(y && scale && shift && skip && ds && pooled && idx, "enc_tail: null argument");
  return hdf_launch_enc_tail(dtype, CRows{y, y_pitch}, NormStats{scale, shift}, CRows{skip, skip_pitch}, Rows{ds, ds_pitch},
                             Rows{pooled, pooled_pitch}, idx, Extent{N, C, Do, Ho, Wo}, (hipStream_t)stream);
}
int hdf_op_enc_tail_up(int dtype, const void* y, int64_t y_pitch, const float* scale, const float* shift, const void* low,
                       int64_t low_pitch, const float* lscale, const float* lshift, void* ds, int64_t ds_pitch,
                       void* pooled, int64_t pooled_pitch, uint8_t* idx, int N, int C, int Do, int Ho, int Wo,
                       hdf_stream stream) {
  HDF_CHECK_ARG(y && scale && shift && low && lscale && lshift && ds && pooled && idx, "enc_tail_up: null argument");
  return hdf_launch_enc_tail_up(dtype, CRows{y, y_pitch}, NormStats{scale, shift}, CRows{low, low_pitch},
                                NormStats{lscale, lshift}, Rows{ds, ds_pitch}, Rows{pooled, pooled_pitch}, idx,
                                Extent{N, C, Do, Ho, Wo}, (hipStream_t)stream);
}
int hdf_op_maxpool_bwd(int dtype, const void* dout, int64_t dout_pitch, const uint8_t* idx, void* din,
                       int64_t din_pitch, int N, int C, int Do, int Ho, int Wo, int accumulate, hdf_stream stream) {
  return hdf_launch_maxpool_bwd(dtype, CRows{dout, dout_pitch}, idx, Rows{din, din_pitch}, Extent{N, C, Do, Ho, Wo},
                                accumulate, (hipStream_t)stream);
}
int hdf_op_maxpool_bwd_in_rows(int C, int Do, int Ho, int Wo) {
  return hdf_maxpool_bwd_in_blocks((int64_t)Do * Ho * Wo, C);
}
int hdf_op_maxpool_bwd_in(int dtype, const void* dout, int64_t dout_pitch, const uint8_t* idx, void* din,
                          int64_t din_pitch, const void* y, int64_t y_pitch, const float* scale, const float* shift,
                          const float* mean, const float* rstd, float* partials, int N, int C, int Do, int Ho, int Wo,
                          hdf_stream stream) {
  HDF_CHECK_ARG(dout && idx && din && y && scale && shift && mean && rstd && partials, "maxpool_bwd_in: null argument");
  return hdf_launch_maxpool_bwd_in(dtype, CRows{dout, dout_pitch}, idx, Rows{din, din_pitch}, CRows{y, y_pitch},
                                   NormStats{scale, shift, mean, rstd}, partials, Extent{N, C, Do, Ho, Wo},
                                   (hipStream_t)stream);
}
int hdf_op_upsample_fwd(int dtype, const void* y, int64_t y_pitch, const float* scale, const float* shift, void* out,
                        int64_t out_pitch, int N, int C, int Di, int Hi, int Wi, hdf_stream stream) {
  return hdf_launch_upsample_fwd(dtype, CRows{y, y_pitch}, NormStats{scale, shift}, Rows{out, out_pitch},
                                 Extent{N, C, Di, Hi, Wi}, (hipStream_t)stream);
}
int hdf_op_upsample_bwd(int dtype, const void* dout, int64_t dout_pitch, void* din, int64_t din_pitch, int N, int C,
                        int Di, int Hi, int Wi, hdf_stream stream) {
  return hdf_launch_upsample_bwd(dtype, CRows{dout, dout_pitch}, Rows{din, din_pitch}, Extent{N, C, Di, Hi, Wi},
                                 (hipStream_t)stream);
}
// The 2-D forms (models/HDenseFormer_2D.py:166-170, :194-202) of the four entries above, on depth-1 tensors: what the 2-D
// plan launches (exec.hip: e.extent sets flat).  A pooled depth of 1 is a legitimate 3-D call, so the form is chosen by
// the entry, not by the extent.
int hdf_op_enc_tail_2d(int dtype, const void* y, int64_t y_pitch, const float* scale, const float* shift, const void* skip,
                       int64_t skip_pitch, void* ds, int64_t ds_pitch, void* pooled, int64_t pooled_pitch, uint8_t* idx,
                       int N, int C, int Ho, int Wo, hdf_stream stream) {
  HDF_CHECK_ARG(y && scale && shift && skip && ds && pooled && idx, "enc_tail_2d: null argument");
  return hdf_launch_enc_tail(dtype, CRows{y, y_pitch}, NormStats{scale, shift}, CRows{skip, skip_pitch}, Rows{ds, ds_pitch},
                             Rows{pooled, pooled_pitch}, idx, Extent{N, C, 1, Ho, Wo, /*flat*/ 1}, (hipStream_t)stream);
}
int hdf_op_maxpool_bwd_in_2d(int dtype, const void* dout, int64_t dout_pitch, const uint8_t* idx, void* din,
                             int64_t din_pitch, const void* y, int64_t y_pitch, const float* scale, const float* shift,
                             const float* mean, const float* rstd, float* partials, int N, int C, int Ho, int Wo,
                             hdf_stream stream) {
  HDF_CHECK_ARG(dout && idx && din && y && scale && shift && mean && rstd && partials, "maxpool_bwd_in_2d: null argument");
  return hdf_launch_maxpool_bwd_in(dtype, CRows{dout, dout_pitch}, idx, Rows{din, din_pitch}, CRows{y, y_pitch},
                                   NormStats{scale, shift, mean, rstd}, partials, Extent{N, C, 1, Ho, Wo, /*flat*/ 1},
                                   (hipStream_t)stream);
}
int hdf_op_upsample_fwd_2d(int dtype, const void* y, int64_t y_pitch, const float* scale, const float* shift, void* out,
                           int64_t out_pitch, int N, int C, int Hi, int Wi, hdf_stream stream) {
  return hdf_launch_upsample_fwd(dtype, CRows{y, y_pitch}, NormStats{scale, shift}, Rows{out, out_pitch},
                                 Extent{N, C, 1, Hi, Wi, /*flat*/ 1}, (hipStream_t)stream);
}
int hdf_op_upsample_bwd_2d(int dtype, const void* dout, int64_t dout_pitch, void* din, int64_t din_pitch, int N, int C,
                           int Hi, int Wi, hdf_stream stream) {
  return hdf_launch_upsample_bwd(dtype, CRows{dout, dout_pitch}, Rows{din, din_pitch}, Extent{N, C, 1, Hi, Wi, /*flat*/ 1},
                                 (hipStream_t)stream);
}


// ---- transformer / head operator level (HDenseFormer.py:47-145,223-227) -------------------------------------------
namespace {
TfDims op_dims(int M, int B, int N, int DM, int64_t mstride, int training, uint64_t seed) {
  TfDims d;
  d.M = M, d.B = B, d.N = N, d.DM = DM, d.DMF = DM + 128;
  d.mstride = mstride;
  d.training = training ? 1 : 0;
  d.seed = (uint32_t)(seed & 0xffffffffu);
  d.thresh24 = 1u << 23;
  d.keep_scale = 2.0f;
  return d;
}
int op_dims_ok(int M, int B, int N, int DM) {
  HDF_CHECK_ARG(M >= 1 && B >= 1 && N >= 1, "transformer op: M=%d B=%d N=%d", M, B, N);
  HDF_CHECK_ARG(DM >= 32 && DM <= 256 && DM % 32 == 0, "transformer op: token dim %d unsupported (32..256, x32)", DM);
  return HDF_OK;
}
TfLayerP layer_ptrs(float* const* q) {
  return TfLayerP{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], q[10], q[11], q[12]};
}
TfLayerSave save_ptrs(float* base, int64_t rows) {
  TfLayerSave s;
  s.h0 = base, s.qkv = base + rows * 32, s.ob = base + rows * 128, s.lse = base + rows * 160;
  s.h1 = base + rows * 168, s.h2 = base + rows * 200;
  return s;
}
}  // namespace

int hdf_op_attention_fwd(const float* qkv, int nseq, int N, float* ob, float* lse, hdf_stream stream) {
  HDF_CHECK_ARG(qkv && ob && lse && nseq >= 1, "attention_fwd: null argument");
  return tf_attention_fwd(N, nseq, qkv, ob, lse, (hipStream_t)stream);
}
int hdf_op_attention_bwd(const float* qkv, const float* ob, const float* lse, const float* d_ob, float* dqkv, int nseq,
                         int N, hdf_stream stream) {
  HDF_CHECK_ARG(qkv && ob && lse && d_ob && dqkv && nseq >= 1, "attention_bwd: null argument");
  return tf_attention_bwd(N, nseq, qkv, ob, lse, d_ob, dqkv, (hipStream_t)stream);
}
int hdf_op_attention_amp_bwd(int dtype, const float* qkv, const float* ob, const float* lse, const float* d_ob,
                             float* dqkv, int nseq, int N, hdf_stream stream) {
  HDF_CHECK_ARG(qkv && ob && lse && d_ob && dqkv && nseq >= 1, "attention_amp_bwd: null argument");
  HDF_CHECK_ARG(dtype == HDF_F32 || dtype == HDF_BF16 || dtype == HDF_F16, "attention_amp_bwd: dtype %d", dtype);
  return tf_attention_bwd(N, nseq, qkv, ob, lse, d_ob, dqkv, (hipStream_t)stream, dtype);
}
int hdf_op_patch_embed_fwd(const float* x, int M, int B, int D, int H, int W, int DM, const float* weight,
                           const float* bias, const float* pos, int64_t mstride, float* F, int training, uint64_t seed,
                           hdf_stream stream) {
  HDF_CHECK_ARG(x && weight && bias && pos && F, "patch_embed_fwd: null argument");
  HDF_CHECK_ARG(D % 16 == 0 && H % 16 == 0 && W % 16 == 0, "patch_embed_fwd: size (%d,%d,%d) not x16", D, H, W);
  const int N = (D / 16) * (H / 16) * (W / 16);
  HDF_TRY(op_dims_ok(M, B, N, DM));
  return tf_patch_embed_fwd(op_dims(M, B, N, DM, mstride, training, seed), x, D, H, W, weight, bias, pos, F,
                            (hipStream_t)stream);
}
int hdf_op_patch_embed_bwd(const float* x, int M, int B, int D, int H, int W, int DM, const float* dF, int64_t mstride,
                           float* dweight, float* dbias, float* dpos, float* scratch, int training, uint64_t seed,
                           hdf_stream stream) {
  HDF_CHECK_ARG(x && dF && dweight && dbias && dpos && scratch, "patch_embed_bwd: null argument");
  const int N = (D / 16) * (H / 16) * (W / 16);
  HDF_TRY(op_dims_ok(M, B, N, DM));
  return tf_patch_embed_bwd(op_dims(M, B, N, DM, mstride, training, seed), x, D, H, W, dF, dweight, dbias, dpos, scratch,
                            (hipStream_t)stream);
}
int hdf_op_dense_layer_fwd(int M, int B, int N, int DM, int block, int layer, const float* const* params13,
                           int64_t mstride, float* F, float* save, int training, uint64_t seed, hdf_stream stream) {
  HDF_CHECK_ARG(params13 && F && save && layer >= 0 && layer < 4, "dense_layer_fwd: bad argument");
  HDF_TRY(op_dims_ok(M, B, N, DM));
  return tf_layer_fwd(op_dims(M, B, N, DM, mstride, training, seed), block, layer,
                      layer_ptrs(const_cast<float* const*>(reinterpret_cast<const float* const*>(params13))), F,
                      save_ptrs(save, (int64_t)M * B * N), (hipStream_t)stream);
}
int hdf_op_dense_layer_bwd(int M, int B, int N, int DM, int block, int layer, const float* const* params13,
                           float* const* grads13, int64_t mstride, const float* F, float* dF, const float* save,
                           float* scratch, int training, uint64_t seed, hdf_stream stream) {
  HDF_CHECK_ARG(params13 && grads13 && F && dF && save && scratch && layer >= 0 && layer < 4,
                "dense_layer_bwd: bad argument");
  HDF_TRY(op_dims_ok(M, B, N, DM));
  return tf_layer_bwd(op_dims(M, B, N, DM, mstride, training, seed), block, layer,
                      layer_ptrs(const_cast<float* const*>(reinterpret_cast<const float* const*>(params13))),
                      layer_ptrs(grads13), F, dF, save_ptrs(const_cast<float*>(save), (int64_t)M * B * N), scratch,
                      (hipStream_t)stream);
}
int hdf_op_block_out_fwd(int M, int B, int N, int DM, int block, const float* const* params4, int64_t mstride,
                         const float* F, float* next_F, void* attnall, int dtype, int training, uint64_t seed,
                         hdf_stream stream) {
  HDF_CHECK_ARG(params4 && F && ((next_F != nullptr) != (attnall != nullptr)), "block_out_fwd: bad argument");
  HDF_TRY(op_dims_ok(M, B, N, DM));
  TfOutP o{const_cast<float*>(params4[0]), const_cast<float*>(params4[1]), const_cast<float*>(params4[2]),
           const_cast<float*>(params4[3])};
  return tf_block_out_fwd(op_dims(M, B, N, DM, mstride, training, seed), block, o, F, next_F, attnall, dtype,
                          (hipStream_t)stream);
}
int hdf_op_block_out_bwd(int M, int B, int N, int DM, int block, const float* const* params4, float* const* grads4,
                         int64_t mstride, const float* F, const float* dF_next, const void* d_attnall, int dtype,
                         float* dF, int training, uint64_t seed, hdf_stream stream) {
  HDF_CHECK_ARG(params4 && grads4 && F && dF && ((dF_next != nullptr) != (d_attnall != nullptr)),
                "block_out_bwd: bad argument");
  HDF_TRY(op_dims_ok(M, B, N, DM));
  TfOutP o{const_cast<float*>(params4[0]), const_cast<float*>(params4[1]), const_cast<float*>(params4[2]),
           const_cast<float*>(params4[3])};
  TfOutP g{grads4[0], grads4[1], grads4[2], grads4[3]};
  return tf_block_out_bwd(op_dims(M, B, N, DM, mstride, training, seed), block, o, g, F, dF_next, d_attnall, dtype, dF,
                          (hipStream_t)stream);
}
int hdf_op_head_fwd(int dtype, const void* in, int64_t in_pitch, const float* in_scale, const float* in_shift,
                    const float* weight, const float* bias, void* logits, int N, int C, int n_cls, int64_t voxels,
                    hdf_stream stream) {
  HDF_CHECK_ARG(in && weight && bias && logits, "head_fwd: null argument");
  return hdf_launch_head_fwd(dtype, CRows{in, in_pitch}, NormStats{in_scale, in_shift}, weight, bias, logits, N, C, n_cls,
                             voxels, (hipStream_t)stream);
}
int hdf_op_head_bwd(int dtype, const void* dlogits, const void* in, int64_t in_pitch, const float* in_scale,
                    const float* in_shift, const float* weight, void* dx, int64_t dx_pitch, int accumulate_dx,
                    float* dweight, float* dbias, int N, int C, int n_cls, int64_t voxels, hdf_stream stream) {
  HDF_CHECK_ARG(dlogits && in && weight && dx && dweight && dbias, "head_bwd: null argument");
  return hdf_launch_head_bwd(dtype, dlogits, CRows{in, in_pitch}, NormStats{in_scale, in_shift}, weight,
                             HeadGrads{Rows{dx, dx_pitch}, accumulate_dx, dweight, dbias}, N, C, n_cls, voxels,
                             (hipStream_t)stream);
}

}  // extern "C"
