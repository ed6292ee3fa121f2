/* libhdf_hip.so -- C ABI of the MI355X-native H-DenseFormer 3D training hot path.
 *
 * Nothing like this exists in the reference (pure Python on torch ops); each entry point
 * replaces the torch call sequence cited next to it (file:line into the reference repository).  All
 * pointers are raw DEVICE pointers unless marked host.  The library never allocates or frees device
 * memory, never synchronises the device and enqueues everything on the caller's stream (hipStream_t
 * passed as void*; hdf_backward additionally forks work onto one internal stream of the plan and joins
 * it back before returning, see there), so it composes with torch's caching allocator, autograd
 * streams and RCCL side streams.  Errors: every function returns 0 on success, non-zero otherwise; hdf_last_error() gives the
 * message (thread-local).  No C++ exception crosses this boundary.
 *
 * dtype enum: 0 = float32 storage (v_mfma_f32_32x32x2_f32, exact fp32 -- the parity path),
 *             1 = bfloat16 storage with fp32 accumulation (v_mfma_f32_32x32x16_bf16 -- the bench path),
 *             2 = float16 storage with fp32 accumulation (v_mfma_f32_32x32x16_f16 -- what the reference's
 *                 torch.cuda.amp.autocast(True) + GradScaler run, trainer.py:20-21,257,369-377).
 */
#ifndef HDF_H
#define HDF_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hdf_plan hdf_plan;
typedef void* hdf_stream; /* hipStream_t */

const char* hdf_version(void);
const char* hdf_last_error(void);
/* Compute units the persistent kernels (conv_ws2 / conv_wgrad2 / the transposed-conv kernels) may assume: their grids
 * are one workgroup per CU.  256 = the whole MI355X (default); a multiple of 8 below that for launches on a stream the
 * CALLER created with hipExtStreamCreateWithCUMask, so that every workgroup of a launch is resident at once.  Process-wide
 * (forward and autograd's backward thread see the same value: it also enters the split-K decision of the low-resolution
 * convs, i.e. their summation order); a diagnostic knob -- the plan never changes it and owns no masked streams.
 * Round 6: a DOWNWARD override only -- the effective budget is min(this, the current device's compute-unit count
 * (hipDeviceAttributeMultiprocessorCount)), so partitioned or smaller gfx950 devices size their grids, and decide whether
 * the persistent transformer kernels can be resident together, from what they have. */
int hdf_set_cu_budget(int cus);

/* ---- model plan: models/HDenseFormer.py:177-227 (HDenseFormer.__init__) ------------------------------- */
int hdf_plan_create(int in_channels, int n_cls, int n_filters, int D, int H, int W, int transformer_depth, int dtype,
                    hdf_plan** out);
/* models/HDenseFormer_2D.py:172-229 (HDenseFormer_2D.__init__): the 2-D model.  The plan's parameter table is then the
 * 2-D reference state_dict (Conv2d / ConvTranspose2d kernels [..,3,3], patch kernels [..,16,16]); hdf_forward takes
 * x [B,C,H,W] and returns out_i [B,n_cls,H/2^i,W/2^i]; hdf_backward* take 2-D logit gradients and write 2-D parameter
 * gradients.  Round 6: the model runs NATIVELY on depth-1 tensors -- 2-D convolutions / transposed convolutions / weight
 * gradients (the 9 centre-plane taps of the embedded 27-tap panels), MaxPool2d, bilinear x2, 16 x 16 patches against depth
 * slice 0 of the embedded patch kernels.  hdf_plan_create_2d_embedded keeps the exact depth-16 replicated 3-D embedding of
 * rounds 3-5 (16x ... 2x the arithmetic): the oracle of tests/test_gpu_model_2d.py. */
int hdf_plan_create_2d(int in_channels, int n_cls, int n_filters, int H, int W, int transformer_depth, int dtype,
                       hdf_plan** out);
int hdf_plan_create_2d_embedded(int in_channels, int n_cls, int n_filters, int H, int W, int transformer_depth, int dtype,
                                hdf_plan** out);
/* Operator level (hdf_op_conv3d, hdf_op_conv3d_wgrad, below): a tensor depth of 1 selects the 2-D operator -- Conv2d(k3,p1),
 * the stride-2 gather in y and x, ConvTranspose2d(k3,s2,p1,op1) and their weight gradients; the depth axis is never
 * strided (output depth 1), the packed panel keeps its 27-tap layout with the 2-D kernel on depth tap 1, and a weight
 * gradient comes back as [.., 27] with zeros off the centre plane (tests/test_gpu_ops_2d.py). */
void hdf_plan_destroy(hdf_plan* p);
/* parameter table = the reference state_dict, in registration order; the flat fp32
 * parameter / gradient buffers place tensor i at offset_i (64-byte aligned) */
int64_t hdf_plan_num_params(const hdf_plan* p);
int64_t hdf_plan_param_floats(const hdf_plan* p);
int hdf_plan_param_info(const hdf_plan* p, int64_t idx, char* name, int name_cap, int64_t* offset, int64_t* numel,
                        int* ndim, int64_t* shape5);
int64_t hdf_plan_workspace_bytes(hdf_plan* p, int batch);
/* the prefix of that arena a forward touches: enough for hdf_forward when no hdf_backward follows (eval, sliding-window
 * prediction); hdf_backward* refuse a workspace smaller than hdf_plan_workspace_bytes */
int64_t hdf_plan_inference_workspace_bytes(hdf_plan* p, int batch);
/* named activation buffers inside the workspace (debug / parity tests): channels-last views */
int hdf_plan_buffer_info(hdf_plan* p, int batch, const char* name, int64_t* byte_offset, int64_t* pitch_elems,
                         int* channels, int* d, int* h, int* w);

/* raw fp32 regions of the transformer branches inside the workspace (debug / parity tests): "tf_F" (feature buffers of
 * HDenseFormer.py:91-99, [block][row][DM+128]), "tf_save" (per layer h0 | qkv | ob | lse | h1 | h2), "tf_dF", "tf_tape",
 * "tf_otape" (backward), "tf_sync" (arrival counters and the timeout words of the persistent transformer kernels: word
 * 32 * (in_channels * batch) of each half is non-zero after a launch whose per-sequence barrier gave up) */
int hdf_plan_region_info(hdf_plan* p, int batch, const char* name, int64_t* byte_offset, int64_t* bytes);

/* HDenseFormer.forward, models/HDenseFormer.py:229-255.  x: [B,Cin,D,H,W] fp32 NCDHW.  out_i: [B,n_cls,D/2^i,..]
 * NCDHW in the plan's storage dtype.  training!=0 enables the dropout sites (:39,41,61,138) with the
 * counter-hash masks of (seed).  The workspace keeps what backward needs. */
int hdf_forward(hdf_plan* p, const float* x, const float* params, void* workspace, int64_t workspace_bytes, void* out0,
                void* out1, void* out2, void* out3, int batch, int training, uint64_t seed, hdf_stream stream);
/* autograd of the above (trainer.py:374-380 loss.backward()).  dout_i: gradients w.r.t. the 4 outputs, same
 * layout/dtype.  grads: flat fp32 buffer, OVERWRITTEN with d loss / d params.
 * Streams: the conv weight gradients run on one internal side stream of the plan, forked from `stream` with an event;
 * `stream` waits for them before the call's work is complete on it (HDF_NO_ASYNC_WGRAD=1 disables). */
int hdf_backward(hdf_plan* p, const float* x, const float* params, void* workspace, int64_t workspace_bytes,
                 const void* dout0, const void* dout1, const void* dout2, const void* dout3, float* grads, int batch,
                 hdf_stream stream);

/* the same in stages so a caller can overlap the gradient all-reduce with the rest of backward (a stage needs the
 * earlier ones to have run):
 * stages bit 0: zero grads + decoder/encoder/heads (their parameter gradients are final afterwards);
 * stages bit 1: UpConv chain (deep_conv, up1..3);
 * stages bit 2: transformer branches.  7 = everything.  Replaces nn.DataParallel's reduce (trainer.py:228-229). */
int hdf_backward_stages(hdf_plan* p, const float* x, const float* params, void* workspace, int64_t workspace_bytes,
                        const void* dout0, const void* dout1, const void* dout2, const void* dout3, float* grads,
                        int batch, int stages, hdf_stream stream);

/* hdf_backward (ONE call, with its internal side / branch streams) that also tells the caller when each gradient BUCKET is
 * final.  The flat gradient buffer is cut into HDF_NUM_GRAD_BUCKETS contiguous ranges (hdf_plan_grad_bucket, floats):
 *   0  decoder + heads      (upconv_3 .. conv1x1_d3)        final a third of the way into the backward
 *   1  UpConv chain         (deep_conv, up1..3)             final when the chain's backward is through
 *   2  transformer branches (attns.*)                       final at the end of the branch stream
 *   3  encoder levels 1-3   (block_2_1_left .. block_4_2_left)   final before the UpConv chain's backward starts
 *   4  encoder level 0      (block_1_1_left, block_1_2_left: 0.1 MB)   final with the last kernel of the call
 * (round 6: five buckets; rounds 4-5 had three, and their "encoder / decoder / heads" bucket -- 26 of 62 MB at n_filters 32
 * -- was final only at the very end, i.e. its all-reduce was exposed.)  bucket_events[k] receives an event owned by the plan
 * -- the handles are stable for the plan's lifetime and RE-RECORDED by every hdf_backward_events call, so a waiter must
 * enqueue its wait before the next call --, already recorded, on whichever internal stream finishes that bucket, when the
 * call returns.  A communication stream that waits for event k (hdf_stream_wait_event, or hipStreamWaitEvent on the
 * handle) may all-reduce bucket k while the rest of the backward is still running: no host round trip between the stages,
 * the branch-stream fork of the one-call backward stays.  Order of finality in the default arrangement: 0, 3, 1, 2, 4.
 * 2-D plans: all five events are recorded at the end (their gradients are extracted from the embedding in one pass), and
 * hdf_plan_grad_bucket is refused.  Replaces nn.DataParallel's reduce (trainer.py:228-229). */
#define HDF_NUM_GRAD_BUCKETS 5
int hdf_plan_grad_bucket(const hdf_plan* p, int k, int64_t* lo, int64_t* hi);
int hdf_backward_events(hdf_plan* p, const float* x, const float* params, void* workspace, int64_t workspace_bytes,
                        const void* dout0, const void* dout1, const void* dout2, const void* dout3, float* grads,
                        int batch, hdf_stream stream, void** bucket_events /* [HDF_NUM_GRAD_BUCKETS] hipEvent_t out */);
/* ---- the persistent transformer kernels and a shared device (round 6) ----------------------------------------------
 * The plan runs all dense layers of the multi-path transformer (models/HDenseFormer.py:78-145) as ONE persistent launch per
 * direction when every 16-token tile gets a compute unit of its own (tiles <= the device's compute units; else, and under
 * HDF_NO_TF_CHAIN=1, as a chain of ~100 small launches).  Those launches wait on each other inside the kernel, so all their
 * workgroups must be resident together.  The library guarantees that within the PROCESS (one such launch in flight per
 * device at a time: each waits for the previous one's event).  If something else holds compute units long enough that a
 * per-sequence barrier is not completed within the deadline (default 1.5 s), the launch does NOT trap any more: it ends by
 * itself and writes a host-mapped status word; the call's last launch then turns the head of every output (forward) / of
 * the gradient buffer (backward) into NaN, so the loss and the optimizer step of that iteration are NaN, never plausible
 * garbage.  The plan's NEXT hdf_forward / hdf_backward* call then launches
 * nothing and returns HDF_ERR_CHAIN_TIMEOUT (4) once, and the plan uses the launch chain from then on: redo the step.
 * hdf_plan_set_chain_timeout_us: the deadline of one barrier wait (100 us .. 30 s).
 * hdf_plan_chain_state: *persistent = 1 when the next forward of `batch` samples would take the persistent kernels;
 * *gave_up_workgroup = id of the workgroup whose give-up is pending or was last reported, -1 if none.  Meaningful right
 * after the caller synchronised the device; never synchronises itself. */
#define HDF_ERR_CHAIN_TIMEOUT 4
int hdf_plan_set_chain_timeout_us(hdf_plan* p, int64_t usec);
int hdf_plan_chain_state(hdf_plan* p, int batch, int* persistent, int* gave_up_workgroup);
/* Tests only: take the persistent kernels even when their grid cannot be resident together (more 16-token tiles than
 * compute units).  Such a forward gives up by construction: this is how tests/test_gpu_chain.py exercises the path above. */
int hdf_plan_force_persistent(hdf_plan* p, int on);
/* Tests and tools: a stand-in for a collective's kernel -- `workgroups` workgroups of 256 threads, each holding `lds_bytes`
 * of LDS (160 KiB: a compute unit of its own) and `vgprs` (0 or 128) vector registers per lane, spinning for `usec` on the
 * device's real-time counter. */
int hdf_op_occupy(int workgroups, int lds_bytes, int vgprs, int usec, hdf_stream stream);

/* Measurement hook: every following hdf_forward on this plan records ev_start immediately before and ev_stop immediately
 * after the launch of the forward's dominant convolution (block_1_1_right, 64 -> 32 channels at full resolution: the
 * kernel bench.py's `roofline` object reports) on the caller's stream.  Two caller-owned HIP events created with timing
 * enabled; NULL, NULL switches it off.  The launch itself is unchanged. */
int hdf_plan_set_probe(hdf_plan* p, void* ev_start, void* ev_stop);
/* hipStreamWaitEvent(stream, event) for callers that hold streams and events as opaque handles */
int hdf_stream_wait_event(hdf_stream stream, void* event);

/* ---- loss: loss/combine_loss.py:68-79 DeepSuperloss(CEPlusDice(weight=None, ignore_index=0)) --------- */
int64_t hdf_loss_workspace_bytes(int batch);
int hdf_loss_forward(int dtype, const void* out0, const void* out1, const void* out2, const void* out3, int nscale,
                     const float* target_onehot, int batch, int n_cls, int D, int H, int W, void* workspace,
                     float* loss_out, hdf_stream stream);
int hdf_loss_backward(int dtype, const void* out0, const void* out1, const void* out2, const void* out3, int nscale,
                      const float* target_onehot, int batch, int n_cls, int D, int H, int W, const void* workspace,
                      const float* grad_out, void* dout0, void* dout1, void* dout2, void* dout3, hdf_stream stream);
/* the same with the two terms weighted (ce_weight * CE + dice_weight * Dice per scale): 1,1 is CEPlusDice
 * (loss/combine_loss.py:8-35); 0,1 is the stand-alone DiceLoss(ignore_index=0) of loss/dice_loss.py:53-87; 1,0 is
 * CrossentropyLoss (loss/cross_entropy.py:8-22).  nscale = 1 gives the un-supervised (single output) forms. */
int hdf_loss_terms_forward(int dtype, const void* out0, const void* out1, const void* out2, const void* out3, int nscale,
                           const float* target_onehot, int batch, int n_cls, int D, int H, int W, float ce_weight,
                           float dice_weight, void* workspace, float* loss_out, hdf_stream stream);
int hdf_loss_terms_backward(int dtype, const void* out0, const void* out1, const void* out2, const void* out3,
                            int nscale, const float* target_onehot, int batch, int n_cls, int D, int H, int W,
                            float ce_weight, float dice_weight, const void* workspace, const float* grad_out,
                            void* dout0, void* dout1, void* dout2, void* dout3, hdf_stream stream);
/* the general forms trainer.py:743-771 (_get_loss) can build: class_weight = device [n_cls] fp32 or NULL
 * (DiceLoss multiplies class i's Dice term by weight[i], loss/dice_loss.py:79-82; CrossEntropyLoss(weight) is
 * sum_v w[t_v] nll_v / sum_v w[t_v], loss/cross_entropy.py:8-22 on torch.nn.CrossEntropyLoss); dice_ignore_index =
 * the class DiceLoss skips (then the class sum is divided by n_cls - 1) or -1 for ignore_index=None (divided by
 * n_cls), loss/dice_loss.py:75-87.  NULL, 0 reproduce hdf_loss_terms_* bit for bit. */
int hdf_loss_weighted_forward(int dtype, const void* out0, const void* out1, const void* out2, const void* out3,
                              int nscale, const float* target_onehot, int batch, int n_cls, int D, int H, int W,
                              float ce_weight, float dice_weight, const float* class_weight, int dice_ignore_index,
                              void* workspace, float* loss_out, hdf_stream stream);
int hdf_loss_weighted_backward(int dtype, const void* out0, const void* out1, const void* out2, const void* out3,
                               int nscale, const float* target_onehot, int batch, int n_cls, int D, int H, int W,
                               float ce_weight, float dice_weight, const float* class_weight, int dice_ignore_index,
                               const void* workspace, const float* grad_out, void* dout0, void* dout1, void* dout2,
                               void* dout3, hdf_stream stream);
/* the two-class losses: trainer.py:755-757 builds FocalLoss(reduction='sum') when config.py:127 picks it (NUM_CLASSES
 * == 2, config.py:59), wrapped in DeepSuperloss (trainer.py:222-226, combine_loss.py:68-79).  Per scale
 * focal_weight * Focal + dice_weight * Dice, with Focal of loss/cross_entropy.py:45-73 on the softmax p of the logits and
 * the (soft, [0,1]) target t, per element alpha_t * BCE(p, t) * (1 - p_t)^gamma (BCE's logs clamped at -100, p_t =
 * p t + (1-p)(1-t), alpha_t = alpha t + (1-alpha)(1-t), no alpha factor when alpha < 0), summed over all batch x n_cls x
 * voxels (focal_reduction 0, 'sum') or averaged over them (1, 'mean'); gradients as torch's autograd (BCE backward
 * (p - t) / max(p (1-p), 1e-12); the pow backward is 0 at gamma 0).  gamma must be 0 or >= 1 (in (0, 1) the reference's
 * gradient is NaN for a confident right voxel).  The Dice term, class_weight and dice_ignore_index are those of
 * hdf_loss_weighted_*; the class weight acts on the Dice term only.  FocalLoss(alpha, gamma, reduction=r) is
 * (1, alpha, gamma, r, 0, NULL, 0); FLPlusDice(weight, ignore_index) (loss/combine_loss.py:37-64) is
 * (1, 1, 2, 1, 1, weight, ignore_index).  Same workspace as hdf_loss_weighted_* (hdf_loss_workspace_bytes). */
int hdf_loss_focal_forward(int dtype, const void* out0, const void* out1, const void* out2, const void* out3, int nscale,
                           const float* target_onehot, int batch, int n_cls, int D, int H, int W, float focal_weight,
                           float focal_alpha, float focal_gamma, int focal_reduction, float dice_weight,
                           const float* class_weight, int dice_ignore_index, void* workspace, float* loss_out,
                           hdf_stream stream);
int hdf_loss_focal_backward(int dtype, const void* out0, const void* out1, const void* out2, const void* out3,
                            int nscale, const float* target_onehot, int batch, int n_cls, int D, int H, int W,
                            float focal_weight, float focal_alpha, float focal_gamma, int focal_reduction,
                            float dice_weight, const float* class_weight, int dice_ignore_index, const void* workspace,
                            const float* grad_out, void* dout0, void* dout1, void* dout2, void* dout3,
                            hdf_stream stream);
/* ---- TopKLoss (loss/cross_entropy.py:26-43; config.py:125 offers it, trainer.py:751-753 builds it).  Per voxel v of the
 * logits [batch][n_cls][D][H][W] (D = 1: 2-D logits): res[v] = class_weight[t_v] * nll_v, t_v the arg-max of the one-hot
 * target (the first maximum wins), nll_v = log(sum_c exp(x_c - max)) - (x_t - max) >= 0 in fp32 from the stored logits;
 * res[v] = 0 where t_v == ignore_index (-100: none).  The K largest of the n = batch * D * H * W values are selected, K =
 * int(n * k / 100) formed by the caller as the reference forms it.  The reference's quirks, restated: its constructor hands
 * reduce=False to torch.nn.CrossEntropyLoss, which overwrites self.reduction with 'none', so for reduction None, 'mean' and
 * 'sum' alike forward returns the K-vector of torch.topk(res, K, sorted=False) -- in unspecified order, not a scalar: it
 * cannot be passed to backward() nor through DeepSuperloss, so the reference cannot train with this loss as trainer.py
 * builds it.  Here the vector's order is defined (ascending voxel index b, d, h, w) and the scalar mean of the K values
 * (named 'topk' after BinaryDiceLoss's reduction, loss/dice_loss.py:44-46) is the trainable form.
 *   Tie rule: among values equal to the K-th largest, the lowest voxel index is taken first.
 *   NaN rule: a NaN value counts as the largest, as in torch.topk; a NaN logit therefore reaches the result.
 * The target is [batch][n_cls][D << s][H << s][W << s] (depth 1 stays 1) with s = scale_shift in 0..3: nearest
 * down-sampling by 2^s reads index dst << s (DeepSuperloss, loss/combine_loss.py:68-79), no down-sampled copy is made.
 * forward: exactly one of values_out [K] (voxel order) and mean_out [1] (the fp64 mean rounded once).  backward: exactly one
 * of grad_values [K] and grad_mean [1] (device pointers: a GradScaler costs no host synchronisation); dlogits (the logits'
 * dtype) = g * class_weight[t] * (p_c - [c == t]) on the selected voxels with g = grad_values[rank] or *grad_mean / K (K exact, the quotient rounded to fp32 once),
 * exact zeros elsewhere and on ignored voxels.  The workspace (res and rank, 8 bytes a voxel, plus
 * HDF_TOPK_SELECT_WORKSPACE_BYTES) is the caller's, written by forward and read by backward; the library allocates nothing.
 * Its layout: the select's state (HDF_TOPK_SELECT_WORKSPACE_BYTES), then res fp32 [n], then, 4 n rounded up to a multiple
 * of 256 bytes later, rank int32 [n] (each voxel's position in the output, -1 = not selected).
 * Refused before anything is launched (HDF_ERR_ARG, message "topk: ..."): K < 1 or K > n, n >= 2^31, n_cls outside 2..8,
 * scale_shift outside 0..3, ignore_index outside {-100, 0..n_cls-1}, a workspace below the size function or not aligned
 * to 16 bytes, batch > 65535 (one grid row a sample), both or neither of the two outputs / gradients.  Logits of depth 1
 * are 2-D logits to these entries: with scale_shift > 0 their target has depth 1 too, never 1 << s. */
#define HDF_TOPK_SELECT_WORKSPACE_BYTES 65536
int64_t hdf_loss_topk_workspace_bytes(int batch, int D, int H, int W); /* D, H, W of the logits; -1 if refused */
int hdf_loss_topk_forward(int dtype, const void* logits, const float* target_onehot, int batch, int n_cls, int D, int H,
                          int W, int scale_shift, const float* class_weight, int ignore_index, int64_t K,
                          void* workspace, int64_t workspace_bytes, float* values_out, float* mean_out,
                          hdf_stream stream);
int hdf_loss_topk_backward(int dtype, const void* logits, const float* target_onehot, int batch, int n_cls, int D, int H,
                           int W, int scale_shift, const float* class_weight, int ignore_index, int64_t K,
                           const void* workspace, int64_t workspace_bytes, const float* grad_values,
                           const float* grad_mean, void* dlogits, hdf_stream stream);
/* the select on its own: the K largest of n floats (device), exact, for any input -- the order is that of the values with
 * -0.0 below +0.0 and every NaN above +inf; tie and NaN rules as above.  Multi-pass radix select over the 32-bit key; no
 * sort, no host round trip, integer atomics only (two runs agree in every bit).  workspace: at least
 * HDF_TOPK_SELECT_WORKSPACE_BYTES, aligned to 16 bytes (refused otherwise, like K < 1, K > n and n >= 2^31).  result[4] (or NULL) = bit pattern of the K-th largest value (a NaN threshold reads
 * 0x7fc00000), count above it, ties taken, 0; rank_out[n] (or NULL) = position in the output, -1 = not selected;
 * values_out[K] (or NULL) in index order; mean_out[1] (or NULL). */
int hdf_op_topk_select(const float* values, int64_t n, int64_t K, void* workspace, int64_t workspace_bytes,
                       uint64_t* result, int32_t* rank_out, float* values_out, float* mean_out, hdf_stream stream);
/* hard-argmax Dice counts of trainer.py:919-945: counts[batch][8][3] = (|P&T|, |P|, |T|) per class, uint64.
 * This and hdf_confusion_matrix refuse (HDF_ERR_ARG) batch < 1, voxels < 1 and n_cls outside 1..8. */
int hdf_dice_counts(int dtype, const void* logits, const float* target_onehot, int batch, int n_cls, int64_t voxels,
                    uint64_t* counts, hdf_stream stream);

/* running confusion matrix of metrics.RunningDice.update_matrix (metrics.py:104-133; the reference moves the argmax
 * maps to the host and calls sklearn): confusion[8][8] uint64, rows = target class, cols = predicted class, summed
 * over the batch; accumulate != 0 keeps the previous counts (running matrix over steps) */
int hdf_confusion_matrix(int dtype, const void* logits, const float* target_onehot, int batch, int n_cls,
                         int64_t voxels, uint64_t* confusion, int accumulate, hdf_stream stream);

/* the reference's own call signature, RunningDice.update_matrix(ground_truth, prediction) (metrics.py:104): two uint8
 * class maps of n voxels each; labels >= n_cls are dropped like sklearn's confusion_matrix(labels=...) does */
int hdf_confusion_matrix_labels(const uint8_t* target, const uint8_t* prediction, int n_cls, int64_t n,
                                uint64_t* confusion, int accumulate, hdf_stream stream);

/* ---- surface-distance evaluation of one class (metrics.py:156-309, cal_score and the multi_* wrappers; the reference
 * makes one SimpleITK pass per class on the host).  T = (target == label), P = (prediction == label) over one uint8
 * volume [D][H][W], unit spacing; a neighbour outside the volume does not exist (it is never background).
 * hdf_op_mask_flags: flags[v] = 1 v in T | 2 v in P | 4 v in B26(T) | 8 v in B26(P) | 16 v in C6(T) | 32 v in C6(P).
 * B26(M): voxels of M with an in-volume 26-neighbour outside M (the seeds of ITK's Maurer filter); C6(M): voxels of M with
 * an in-volume face neighbour outside M (sitk.LabelContour's default).  counts[5] uint64 = |T| |P| |T&P| |C6(T)| |C6(P)|.
 * hdf_op_edt_sq: d2[v] int32 = min over the voxels b with (flags[b] & seed_bit) of |v - b|^2, exact;
 * HDF_EDT_NO_SEED where the volume holds no such voxel.  seed_bit is a mask, 1..255.  The entry checks the workspace
 * size like hdf_surface_distances (one allocation serves both) and does not touch it: the transform runs in place.
 * hdf_surface_distances: the flags, d2_T (seeds B26(T)) and d2_P (seeds B26(P)), then
 * result[12] uint64 = |T| |P| |T&P| |C6(T)| |C6(P)| hd2 n S[lo] S[hi] lo r valid, where
 *   valid = neither T nor P is empty or fills the volume; when 0, hd2 .. r are 0 (the caller reports NaN);
 *   hd2   = max(max over P\T of d2_T, max over T\P of d2_P, 0): HausdorffDistance = sqrt(hd2);
 *   S     = the sorted multiset { d2_T(v) : v in C6(P) } + { d2_P(v) : v in C6(T) }, n = |S|, q = 95 (n - 1),
 *           lo = q div 100, r = q mod 100, hi = min(lo + (r > 0), n - 1):
 *           HausdorffDistance95 = sqrt(S[lo]) + (sqrt(S[hi]) - sqrt(S[lo])) r / 100 (np.percentile(., 95), linear).
 * histogram_out (nullable, device): the count of every squared distance in S, histogram_len entries (those past
 * (D-1)^2 + (H-1)^2 + (W-1)^2 are 0).  All pointers are device memory; the kernels are ordered on `stream`, nothing waits
 * on the host, and a workspace may be reused by the next call on the same stream.  Refused (HDF_ERR_ARG, message
 * "surface: ...") before anything is launched: a dimension outside 1..1024, D*H*W >= 2^31, label outside 1..255,
 * a workspace below hdf_surface_workspace_bytes(D, H, W) (-1 for refused dimensions). */
#define HDF_EDT_NO_SEED 0x3FFFFFFF /* + 1023^2 stays below 2^31 */
int64_t hdf_surface_workspace_bytes(int D, int H, int W);
int hdf_op_mask_flags(const uint8_t* target, const uint8_t* prediction, int label, int D, int H, int W,
                      uint8_t* flags, uint64_t* counts, hdf_stream stream);
int hdf_op_edt_sq(const uint8_t* flags, int seed_bit, int D, int H, int W, int32_t* d2, void* workspace,
                  int64_t workspace_bytes, hdf_stream stream);
int hdf_surface_distances(const uint8_t* target, const uint8_t* prediction, int label, int D, int H, int W,
                          void* workspace, int64_t workspace_bytes, uint64_t* result, uint32_t* histogram_out,
                          int64_t histogram_len, hdf_stream stream);

/* ---- average surface distance of one class (utils.py:165-191, cal_asd and multi_asd; the reference calls MONAI's
 * SurfaceDistanceMetric(symmetric=True) on the host).  T, P and the volume as above.  These definitions come from
 * reading MONAI's source (get_mask_edges, get_surface_distance, compute_average_surface_distance), not from running it;
 * what they are tested against is the sequence of scipy calls MONAI makes.  MONAI's surface and distance are not the
 * ones of hdf_surface_distances, so ASD cannot be read off that call's results:
 *   E6(M)  = the voxels of M with at least one of their six face neighbours not in M, where a neighbour outside the
 *            volume is NOT in M: M ^ scipy.ndimage.binary_erosion(M) with the default structure and border_value = 0.
 *            (MONAI crops to the bounding box of P | T first; outside that box there is no foreground, so nothing
 *            changes.)  A depth-1 volume is all edge; a mask that fills the volume has the volume's shell as its edge;
 *            E6(M) is empty only when M is; E6 and C6 differ exactly on the volume's faces.
 *   dE_T(v) = the Euclidean distance from v to the nearest voxel of E6(T) (distance_transform_edt(~E6(T))), not to the
 *            nearest voxel of T; its square d2_ET is an exact integer.  dE_P likewise.
 *   A = { dE_T(v) : v in E6(P) } (prediction to ground truth), B = { dE_P(v) : v in E6(T) }.
 *   ASD    = (sum A + sum B) / (|A| + |B|), the pooled mean (not the mean of the two means); the directed
 *            sum A / |A| (symmetric=False) and sum B / |B| come with it.
 *   Empty sets: E6(T) and E6(P) both empty -> NaN; exactly one empty -> +inf.  Directed, prediction to ground truth:
 *            E6(P) empty -> NaN, E6(T) empty with E6(P) non-empty -> +inf; the other direction with the roles swapped.
 * The reference's permute(1, 2, 0) ahead of the call only renames the axes: with unit spacing it changes nothing.
 * hdf_op_edge_flags: flags[v] = 1 v in T | 2 v in P | 64 v in E6(T) | 128 v in E6(P) -- the two bits hdf_op_mask_flags
 * leaves clear; bits 4..32 are 0 here.  counts[2] uint64 = |E6(T)| |E6(P)|.  hdf_op_edt_sq with seed_bit 64 / 128 gives
 * d2_ET / d2_EP; it accepts a workspace of hdf_surface_asd_workspace_bytes, which is never below
 * hdf_surface_workspace_bytes.
 * hdf_surface_asd: result[4] uint64 = |E6(T)| |E6(P)| bits(sum A) bits(sum B), the sums as IEEE fp64 bit patterns:
 * sum_k hist[k] sqrt((double)k) over the histogram of the squared distances, added in an order that depends on the
 * volume's dimensions alone (no floating-point atomics: two calls on the same inputs agree in every bit; relative error
 * below 5e-13).  Both sums are +0 when either edge set is empty; the caller forms NaN / +inf from the two counts.
 * histogram_out (nullable, device): [2][histogram_len], row 0 the count of every squared distance in A, row 1 in B
 * (entries past (D-1)^2 + (H-1)^2 + (W-1)^2 are 0); a row sums to |A| = |E6(P)| resp. |B| = |E6(T)| when neither edge set
 * is empty and is all 0 otherwise.  Pointers, stream ordering, workspace reuse and refusals ("surface: ...", before
 * anything is launched) as for hdf_surface_distances, with hdf_surface_asd_workspace_bytes(D, H, W) as the size (-1 for
 * refused dimensions) and a negative histogram_len refused as well. */
int64_t hdf_surface_asd_workspace_bytes(int D, int H, int W);
int hdf_op_edge_flags(const uint8_t* target, const uint8_t* prediction, int label, int D, int H, int W,
                      uint8_t* flags, uint64_t* counts, hdf_stream stream);
int hdf_surface_asd(const uint8_t* target, const uint8_t* prediction, int label, int D, int H, int W,
                    void* workspace, int64_t workspace_bytes, uint64_t* result, uint32_t* histogram_out,
                    int64_t histogram_len, hdf_stream stream);

/* ---- the same measures in physical units: a voxel spacing for HD, HD95 and ASD.  spacing = (sz, sy, sx), a HOST pointer
 * to three doubles in the axis order of the [D][H][W] array; the weights are wz = fl(sz sz), wy = fl(sy sy), wx = fl(sx sx)
 * in fp64.  For a seed set M,
 *   D2_M(v) = min over the seeds u in M of fl( fl(wz a^2) + fl( fl(wy b^2) + fl(wx c^2) ) ),  (a, b, c) = |v - u| per axis,
 * where a^2, b^2, c^2 are exact integers and every fl is one IEEE fp64 rounding (no fused multiply-add); +inf where M is
 * empty.  The separable transform (c^2 along W as an integer, then H, then D) computes exactly this minimum, because
 * fl(x + y) and fl(w k) are monotone; with spacing (1, 1, 1) every value equals the integer of hdf_op_edt_sq.
 * Flags, seed sets and contour / edge sets are those of the unit-spacing entries (hdf_op_mask_flags: seeds B26, contour
 * C6; hdf_op_edge_flags: E6); only the metric changes.
 * hdf_op_edt_sq_mm: d2[v] fp64 = D2_M(v) for M = the voxels with (flags[v] & seed_bit).
 * hdf_op_select_u64: out2[0] = sorted[lo], out2[1] = sorted[min(lo + 1, n - 1)] of n uint64 keys (device), an exact
 * multi-pass radix select: integer atomics only, no sort, no host round trip, the same bits from run to run.  Its
 * workspace is HDF_SELECT_U64_WS bytes (never above hdf_surface_mm_workspace_bytes).  Non-negative doubles order like
 * their bit patterns: hdf_surface_distances_mm runs this select over the bit patterns of the surface distances.
 * hdf_surface_distances_mm: result[12] uint64 laid out like hdf_surface_distances with d2_T = D2_B26(T), d2_P = D2_B26(P):
 * words 5, 7 and 8 (hd2, S[lo], S[hi]) are the fp64 BIT PATTERNS of squared physical distances, S is sorted as fp64, the
 * other words are the same integers; `valid` as there, and words 5..10 are 0 when it is 0.
 * hdf_surface_asd_mm: result[4] uint64 = |E6(T)| |E6(P)| bits(sum A) bits(sum B) with A = { sqrt(D2_E6(T)(v)) : v in E6(P) },
 * B = { sqrt(D2_E6(P)(v)) : v in E6(T) }: fp64 sums over contiguous runs of voxels whose bounds follow from D*H*W alone,
 * then one fixed tree -- no floating-point atomics, two calls agree in every bit.  Both sums are +0 when either edge set
 * is empty.
 * Refused (HDF_ERR_ARG, "surface: ...") before anything is launched, the spacing first: a null spacing; a component that
 * is not finite, not positive or outside [2^-10, 2^10]; whatever the unit-spacing entries refuse; a workspace below
 * hdf_surface_mm_workspace_bytes(D, H, W) (one size for the three entries that take a volume, about 17 bytes a voxel;
 * -1 for refused dimensions); hdf_op_select_u64: n < 1, n >= 2^31, lo outside 0..n-1, a workspace below
 * HDF_SELECT_U64_WS.  Pointers other than spacing are device memory; stream ordering and workspace reuse as above. */
#define HDF_SELECT_U64_WS 49408 /* six histograms of 2048 uint32, then the state */
int64_t hdf_surface_mm_workspace_bytes(int D, int H, int W);
int hdf_op_edt_sq_mm(const uint8_t* flags, int seed_bit, int D, int H, int W, const double* spacing, double* d2,
                     void* workspace, int64_t workspace_bytes, hdf_stream stream);
int hdf_op_select_u64(const uint64_t* keys, int64_t n, int64_t lo, void* workspace, int64_t workspace_bytes,
                      uint64_t* out2, hdf_stream stream);
int hdf_surface_distances_mm(const uint8_t* target, const uint8_t* prediction, int label, int D, int H, int W,
                             const double* spacing, void* workspace, int64_t workspace_bytes, uint64_t* result,
                             hdf_stream stream);
int hdf_surface_asd_mm(const uint8_t* target, const uint8_t* prediction, int label, int D, int H, int W,
                       const double* spacing, void* workspace, int64_t workspace_bytes, uint64_t* result,
                       hdf_stream stream);

/* ---- connected components of a label map (the reference has no such code: its users run scipy.ndimage.label and
 * find_objects on the host).  volume: uint8 [D][H][W] on the device.
 *   connectivity 6 / 18 / 26 = scipy's generate_binary_structure(3, 1 / 2 / 3): neighbours that differ by +-1 in at most
 *            1 / 2 / 3 coordinates.  A neighbour outside the volume does not exist.  A depth-1 volume is the 2-D case:
 *            6 / 18 / 26 are then the 4- / 8- / 8-neighbourhood by themselves.
 *   adjacent = neighbours under `connectivity` that hold the SAME non-zero value: two classes that touch never merge.
 *   label    = 0: every non-zero voxel is foreground, each value forming its own components; k in 1..255: only the voxels
 *            equal to k are.
 *   ids      = the components numbered 1..n in ascending order of their smallest linear voxel index, 0 for background.
 *            For one value this is scipy.ndimage.label's numbering; for several, the per-value labels renumbered by
 *            first voxel.  The result is unique: two calls agree in every element.
 * hdf_cc_label: ids[v] int32 for every voxel, result[2] uint64 = n, the number of foreground voxels.
 * hdf_cc_table: table[capacity][9] int64, row id-1 = size, value, first linear voxel index, zmin, zmax, ymin, ymax, xmin,
 * xmax (maxima inclusive) of component id, for the ids of hdf_cc_label on the same volume.  Components with id > capacity
 * are left out; rows n .. capacity-1 are all zeros.  score (nullable): a fp32 volume of non-negative values (a class
 * probability); score_max[id-1] (required with score, untouched without) = its maximum over the component, exact, 0 in
 * the rows past n.  The maximum is taken over the bit patterns read as signed integers: a negative score (-0 included)
 * counts as +0, and a NaN with a clear sign bit wins over every number -- either is the caller's error.
 * hdf_cc_filter: out[v] = volume[v] where the component of v is kept, 0 elsewhere (background and the voxels with
 * ids[v] = 0 included).  A component is kept iff size >= min_size and, when keep_largest != 0, it is the largest
 * component of its value, a tie going to the smallest id (np.argmax of the size list).  result[2] uint64 = components
 * kept, voxels kept.  out may be volume (in place), and may not overlap it otherwise.
 * Only integer atomics (add / min / max / compare-and-swap) are used, so no output depends on arrival order.  No kernel
 * waits on another workgroup and every loop is bounded by the volume (csrc/components.hip).  All pointers are device
 * memory, the kernels are ordered on `stream`, nothing waits on the host, and a workspace may be reused by the next call
 * on the same stream without clearing.  Refused (HDF_ERR_ARG, message "components: ...") before anything is launched: a
 * dimension outside 1..1024, D*H*W >= 2^31, connectivity not 6 / 18 / 26, label outside 0..255, capacity < 1 (or >= 2^31),
 * min_size < 0, a null required pointer, a workspace below hdf_cc_workspace_bytes(D, H, W) (one size for hdf_cc_label and
 * hdf_cc_filter, about 5 bytes a voxel; -1 for refused dimensions) or not aligned to 8 bytes, ids overlapping volume (or
 * out). */
int64_t hdf_cc_workspace_bytes(int D, int H, int W);
int hdf_cc_label(const uint8_t* volume, int label, int connectivity, int D, int H, int W, int32_t* ids, uint64_t* result,
                 void* workspace, int64_t workspace_bytes, hdf_stream stream);
int hdf_cc_table(const uint8_t* volume, const int32_t* ids, const float* score, int D, int H, int W, int64_t capacity,
                 int64_t* table, float* score_max, hdf_stream stream);
int hdf_cc_filter(const uint8_t* volume, const int32_t* ids, int D, int H, int W, int64_t min_size, int keep_largest,
                  uint8_t* out, uint64_t* result, void* workspace, int64_t workspace_bytes, hdf_stream stream);

/* ---- the overlap table of two id maps: which component of A meets which component of B, in how many voxels (the
 * reference has no such code: its users copy both id maps to the host and run np.unique over 64-bit keys).  ids_a, ids_b:
 * int32 [D][H][W] on the device, for example two outputs of hdf_cc_label; any non-negative numbering is valid, and a value
 * below 0 counts as 0.  ids_a == ids_b is allowed: the diagonal, a component's size and masked size in one pass.
 *   counted  a voxel with a > 0 and b > 0; with HDF_PAIRS_A0 also one with a == 0 and b > 0, with HDF_PAIRS_B0 also one
 *            with a > 0 and b == 0.  (0, 0) is never counted.
 *   pairs    int64 [capacity][4]: one row a, b, n, m per distinct counted (a, b), in ascending (a, b) with a major.  n = the
 *            voxels of the pair, m = those of them with mask[v] != 0 (mask: uint8 [D][H][W], nullable -- m is then 0 in every
 *            row).  Rows P .. capacity-1 are all zeros.
 *   result   [4] uint64 = P, the number of distinct pairs; the counted voxels (the sum of n); the counted voxels under the
 *            mask (the sum of m); the overflow flag, 1 iff there are more than `capacity` distinct pairs (exact: P ==
 *            capacity is no overflow, P == capacity + 1 is one), else 0.  On overflow result[0..2] and every row of pairs are
 *            0: no output depends on which pairs arrived first.
 * Only integer atomics (add and compare-and-swap) are used: every output is exact and the same from call to call.  No kernel
 * waits on another workgroup and every loop is bounded: a hash probe walks at most the table (csrc/cc_pairs.hip).  All
 * pointers are device memory, the kernels are ordered on `stream`, nothing waits on the host, and a workspace may be reused
 * by the next call on the same stream without clearing.  Refused (HDF_ERR_ARG, message "components: ...") before anything is
 * launched: a dimension outside 1..1024, D*H*W >= 2^31, capacity outside 1..65536, unknown flag bits, a null required
 * pointer, a workspace below hdf_cc_pairs_workspace_bytes(capacity) (256 + 24 bytes a slot of the table, the slots a power
 * of two >= 2 * capacity and >= 64; -1 for a refused capacity) or not aligned to 8 bytes, pairs, result or the workspace
 * overlapping an input or each other. */
#define HDF_PAIRS_A0 1   /* also count voxels with a == 0, b > 0 (rows with a = 0) */
#define HDF_PAIRS_B0 2   /* also count voxels with a > 0, b == 0 (rows with b = 0) */
int64_t hdf_cc_pairs_workspace_bytes(int64_t capacity);
int hdf_cc_pairs(const int32_t* ids_a, const int32_t* ids_b, const uint8_t* mask /* nullable */, int flags,
                 int D, int H, int W, int64_t capacity, int64_t* pairs /* [capacity][4] */, uint64_t* result /* [4] */,
                 void* workspace, int64_t workspace_bytes, hdf_stream stream);

/* ---- measurements of an image under an id map: what scipy.ndimage's sum_labels, mean, variance / standard_deviation,
 * minimum / maximum, minimum_position / maximum_position and center_of_mass give, one call per statistic and channel, on
 * the host (the reference has no such code).  ids: int32 [D][H][W], image: fp32 [C][D][H][W], both on the device.  Any
 * non-negative numbering is valid -- the ids of hdf_cc_label, the index map of hdf_detect_candidates, a class map widened to
 * int32; a value below 0 counts as 0, and ids above `capacity` are left out of everything but result[0] and result[1].
 * With z, y, x the coordinates of a voxel, x_v its value in channel c, and the sums running over the voxels of id:
 *   geom     int64 [capacity][4], row id-1 = n, sum z, sum y, sum x: exact integers.
 *   stats    fp64 [C][capacity][8], row id-1 of channel c = S1 = sum x_v, mean = S1 / n, M2 = sum (x_v - mean)^2, min, max,
 *            Wz = sum z x_v, Wy = sum y x_v, Wx = sum x x_v.  The variance scipy reports is M2 / n, its centre of mass W / S1.
 *   pos      int64 [C][capacity][2], row id-1 of channel c = the linear voxel index of the minimum and of the maximum; on a
 *            tie the SMALLEST index for both -- np.argmin / np.argmax and the peak of hdf_detect_candidates, not scipy,
 *            whose maximum_position returns the last one.
 *   result   [4] uint64 = the largest id met (capacity or not), the voxels with id > 0, the voxels with id in 1..capacity, 0.
 * A row whose id no voxel holds is all zero bytes in every output.  A -0 counts as +0 (min and max never return -0, and a sum that is zero is +0).  A NaN
 * or an infinity in a component is the caller's error: that component's fp64 outputs are unspecified, no other row
 * changes, nothing faults (no address is formed from a value of the image).
 * The numerical contract.  n, the coordinate sums, min, max, pos and result are exact: integer atomics, for the extrema
 * on the 64-bit keys (order(x) << 32 | ~index) and (~order(x) << 32 | ~index), order() mapping a float's bits to an
 * unsigned that orders like its value -- negative values included.  The fp64 sums use no floating-point atomic, and every
 * term is exact in fp64 (x_v; z x_v with 10 + 24 bits; x_v - mean is rounded once and squared inside a fused multiply-add),
 * so only the order of the additions is free, and it is fixed (csrc/measure.hip): the box of the id (exact) is cut, in its
 * own linear order, into HDF_MEASURE_SLABS = 8 contiguous slabs of ceil(box voxels / 8); one workgroup of 256 threads per
 * slab, thread t adding the voxels t, t + 256, ... of the slab that hold the id, in that order, from 0; the 256 sums joined by
 * the tree of block_sum_f64 (xor shuffles over 32, 16, ..., 1 lanes, then (w0 + w1) + (w2 + w3)); the eight slabs added in
 * index order.  M2 is a second such pass with the finished mean.  Hence the fp64 outputs of a row are the same in every
 * bit from call to call, whatever the workspace held before, and for every capacity >= the row's id.  Against the
 * exactly rounded sums they stay within n u sum|t| for a sum of n exact terms t (u = 2^-53), that / n + u |mean| for the
 * mean, and 2 [(n + 2) u M2 + n ((n + 1) u sum|x| / n)^2] for M2 (tests/measure_ref.py derives them).
 * The work: one pass over the id map that reads the image where an id counts, then two passes whose cost is the summed
 * voxels of the boxes (times C), not the volume -- as hdf_lesion_surface pays for its crops; a thin diagonal component
 * pays for its whole box.  No kernel waits on another workgroup and every loop is bounded by the volume.  All pointers
 * are device memory, the kernels are ordered on `stream`, nothing waits on the host, and a workspace may be reused by the
 * next call on the same stream without clearing.  Refused (HDF_ERR_ARG, message "components: measure: ...") before
 * anything is launched: C outside 1..8, a dimension outside 1..1024, capacity outside 1..65536, a null pointer, a
 * workspace below hdf_cc_measure_workspace_bytes(C, capacity) (24 bytes an id for the boxes, 16 C for the keys, 256 C for
 * the partial sums; -1 for a refused C or capacity) or not aligned to 8 bytes, geom, stats, pos or result not aligned to 8
 * bytes, any output or the workspace overlapping an input or each other. */
int64_t hdf_cc_measure_workspace_bytes(int C, int64_t capacity);
int hdf_cc_measure(const int32_t* ids, const float* image /* [C][D][H][W] */, int C, int D, int H, int W, int64_t capacity,
                   int64_t* geom /* [capacity][4] */, double* stats /* [C][capacity][8] */, int64_t* pos /* [C][capacity][2] */,
                   uint64_t* result /* [4] */, void* workspace, int64_t workspace_bytes, hdf_stream stream);

/* ---- order statistics of an image under an id map: the median and the percentiles of every id, what scipy.ndimage.median
 * or np.percentile give per id, channel and level on the host after a full sort of every component (the reference has no
 * such code).  ids and image are as hdf_cc_measure takes them: any non-negative numbering, a value below 0 counts as 0, ids
 * above `capacity` count only in result[0] and result[1].  q: a HOST pointer to Q levels, each in [0, 1], in any order,
 * duplicates allowed; it is read before the call returns.
 * The definition.  For an id with n voxels let s_0 <= ... <= s_{n-1} be its values in channel c, a -0 read as +0, and take a
 * level q.  Then h = fl(q * (double)(n - 1)), one fp64 multiplication; lo = floor(h); frac = h - lo, which is exact;
 * hi = lo + (frac > 0).
 *   count    int64 [capacity], row id-1 = n.
 *   values   fp64 [C][capacity][Q][3], row id-1 of channel c, level k = (double)s_lo, (double)s_hi -- each an fp32 value
 *            widened -- and fl(s_lo + fl(frac * fl(s_hi - s_lo))): three fp64 roundings in that order, never a fused
 *            multiply-add.  q = 0 gives the minimum and q = 1 the maximum, the min and max of hdf_cc_measure in every bit;
 *            q = 0.5 gives the median (the mean of the two middle values where n is even).
 *   result   [4] uint64 = the four words of hdf_cc_measure.
 * A row whose id no voxel holds is all zero bytes in every output.  A NaN or an infinity in a component is the caller's
 * error: that component's values are unspecified, no other row changes, nothing faults (the only address formed from a
 * value of the image is a counter index of 8 bits).
 * The numerical contract.  s_lo and s_hi are exact order statistics: an exact radix select (csrc/quantiles.hip) on the
 * 32-bit key order(x) of hdf_cc_measure, four rounds of 8 bits from the top, integer counts only.  Every output is
 * therefore the same in every bit from call to call, for every capacity >= the row's id, whatever the workspace held, and
 * a level's row does not depend on the other levels of the call.
 * The work: the walk of hdf_cc_measure over the id map (the image is not read there), then one workgroup per (id, channel)
 * that reads the id's box four times -- the summed box volumes times 4 C, not the volume; a component whose box is the
 * whole volume is served by one workgroup.  No kernel waits on another workgroup and every loop is bounded by the box.
 * All pointers but q are device memory, the kernels are ordered on `stream`, nothing waits on the host, and a workspace may
 * be reused by the next call on the same stream without clearing.  Refused (HDF_ERR_ARG, message "components: quantiles:
 * ...") before anything is launched: everything hdf_cc_measure refuses -- C outside 1..8, a dimension outside 1..1024,
 * capacity outside 1..65536, a null pointer, a workspace below hdf_cc_quantiles_workspace_bytes(C, capacity, Q) (56 bytes an
 * id; -1 for a refused C, capacity or Q) or not aligned to 8 bytes, count, values or result not aligned to 8 bytes, any
 * output or the workspace overlapping an input or each other -- and Q outside 1..16, a null q, a level that is NaN or
 * outside [0, 1]. */
int64_t hdf_cc_quantiles_workspace_bytes(int C, int64_t capacity, int Q);
int hdf_cc_quantiles(const int32_t* ids, const float* image /* [C][D][H][W] */, int C, int D, int H, int W, int64_t capacity,
                     const double* q /* HOST, [Q] */, int Q, int64_t* count /* [capacity] */,
                     double* values /* [C][capacity][Q][3] */, uint64_t* result /* [4] */, void* workspace,
                     int64_t workspace_bytes, hdf_stream stream);

/* ---- per-lesion surface distances: the second number of the BraTS-2023 lesion-wise protocol (the reference has no such
 * code: its users build two full-volume masks per truth lesion on the host and hand them to SimpleITK or scipy).  For row
 * i of `lesions`, with truth id j,
 *   T_i      = the voxels v with truth_mask[v] != 0 and ids_truth[v] == j
 *   P_i      = the voxels v with ids_pred[v] = a > 0 for which the row (a, j) is among the first n_pairs rows of `pairs`
 *   results  uint64 [L][12]: row i = the twelve words hdf_surface_distances leaves for the masks (T_i, P_i) over the whole
 *            volume; with a spacing (host pointer, as hdf_surface_distances_mm takes it; nullable) the twelve words of
 *            hdf_surface_distances_mm.  Every word is equal to that call's, not close to it.
 * ids_pred, ids_truth: int32 [D][H][W]; truth_mask: uint8 [D][H][W]; pairs: int64 rows a, b, n, m in ascending (a, b) as
 * hdf_cc_pairs leaves them (n and m are not read), all on the device.  lesions: HOST int32 [L][7] = j, zmin, zmax, ymin,
 * ymax, xmin, xmax (inclusive): a box that contains every voxel of T_i and of P_i -- a larger one is as good; one that
 * misses a voxel gives the distances of what is inside it (words 0 and 1 then fall short of the sizes the caller knows).
 * The entry grows the box by one voxel on every side, clamps it to the volume, carves both masks of every crop as 0 / 1
 * bytes into the workspace (one launch per 64 lesions, the rows passed in the kernel arguments: nothing is uploaded, and
 * `lesions` may be freed on return) and runs the surface entry once per lesion on its crop.  That is exact: every B26
 * seed, every C6 contour voxel and every 26-neighbour of a mask voxel lies inside the crop; where a side is clamped the
 * crop's face is the volume's face, where it is not the added layer is true background; and a mask fills the crop only if it
 * fills the volume.  The cost is that of the summed crop voxels, not of L volumes.
 *   workspace  hdf_lesion_surface_workspace_bytes(lesions, L, D, H, W, mm) bytes, mm = 1 when a spacing is given and 0 when not
 *            (neither size covers the other), aligned to 8 bytes.  From byte 0 the crops, packed without padding in row
 *            order: crop i takes 2 n_i bytes, n_i = its voxels, the mask of T_i in [D'][H'][W'] order first, that of P_i
 *            behind it -- both can be read back after the call.  Then, on a 256-byte boundary, one scratch area of
 *            hdf_surface_workspace_bytes / hdf_surface_mm_workspace_bytes of the largest crop, shared by all lesions.
 *            The size is the contract: crops that do not fit are refused, never processed in parts.
 * Integer compares and plain stores only (csrc/lesion_surface.hip), then the surface entry's own kernels: two calls agree
 * in every byte.  The kernels are ordered on `stream`, nothing waits on the host, and the workspace may be reused by the
 * next call on the same stream without clearing.  L = 0 launches nothing.  Refused (HDF_ERR_ARG, message "surface: ...")
 * before anything is launched: a spacing hdf_surface_distances_mm refuses, a dimension outside 1..1024, L < 0, n_pairs < 0,
 * a null required pointer (pairs may be null when n_pairs = 0), a row with j < 1 or with a box that has min > max or leaves
 * the volume, a workspace below the size function (which returns -1 for refused arguments) or not aligned to 8 bytes,
 * results or the workspace overlapping each other or an input. */
int64_t hdf_lesion_surface_workspace_bytes(const int32_t* lesions /* host [L][7] */, int64_t L, int D, int H, int W, int mm);
int hdf_lesion_surface(const int32_t* ids_pred, const int32_t* ids_truth, const uint8_t* truth_mask, int D, int H, int W,
                       const int64_t* pairs, int64_t n_pairs, const int32_t* lesions /* host [L][7] */, int64_t L,
                       const double* spacing /* host, nullable */, void* workspace, int64_t workspace_bytes,
                       uint64_t* results /* [L][12] */, hdf_stream stream);

/* ---- binary morphology of a label map (the reference has no such code: its users run scipy.ndimage.binary_dilation /
 * binary_erosion / binary_opening / binary_closing / binary_fill_holes on the host).  volume: uint8 [D][H][W] on the device.
 *   input mask   label = 0: every non-zero voxel is foreground; k in 1..255: only the voxels equal to k are.
 *   element      connectivity 6 / 18 / 26 = scipy's generate_binary_structure(3, c) with c = 1 / 2 / 3: the offsets
 *            (dz, dy, dx) in {-1, 0, 1}^3 with |dz| + |dy| + |dx| <= c.  A depth-1 volume is the 2-D case: the z axis does
 *            not exist, there are no z neighbours and no z border, 6 / 18 / 26 are the 4- / 8- / 8-neighbourhood.
 *   one step     a voxel outside the volume reads as border_value (0 or 1, scipy's parameter).  Dilate: a voxel is set if
 *            any voxel under the element is set.  Erode: a voxel is set if all voxels under the element are set.
 *   iterations   n steps, n in 1..256 (n < 1 is scipy's "until nothing changes" and is refused).
 *   op           HDF_MORPH_DILATE, HDF_MORPH_ERODE; HDF_MORPH_OPEN = n erosions, then n dilations; HDF_MORPH_CLOSE = n
 *            dilations, then n erosions.  Both halves use the same element and the same border_value: with border_value
 *            = 0 closing erodes an object that touches a face, as scipy's does.
 *   fill holes   new mask = input mask OR every background voxel whose background component, taken under `connectivity`
 *            (scipy's default: 6), touches no face of the volume (no edge, in the 2-D case) =
 *            binary_fill_holes(mask, generate_binary_structure(3, c)).
 *   mode         HDF_MORPH_MASK: out[v] = 1 where the new mask is set, else 0.  HDF_MORPH_MAP (needs label >= 1): out[v] =
 *            0 where a voxel left the mask, label where a voxel joined the mask and held 0, volume[v] everywhere else -- a
 *            voxel of another class is never overwritten, so the result is still a class map.  out may be volume (in
 *            place), and may not overlap it otherwise.
 *   result       [2] uint64 = the voxels of the new mask, the voxels where the new mask differs from the input mask.  Both
 *            are counted on masks, whatever the mode.
 * hdf_morph packs the mask to one bit a voxel (32-bit words along x, every row on a word), runs every step on packed words
 * between the two packed buffers of its workspace (2 * ceil(W / 32) * 4 bytes a row, each buffer rounded up to 256 bytes:
 * 0.25 byte a voxel when W is a multiple of 32) and unpacks once.  hdf_fill_holes labels the complement of the mask with
 * the kernels of hdf_cc_label; its workspace holds the complement map, the id map, a flag per id and that labelling's own
 * workspace, about 11 bytes a voxel.
 * Only integer operations and integer atomics are used: every output is exact and the same from call to call.  No kernel
 * waits on another workgroup (csrc/morphology.hip).  All pointers are device memory, the kernels are ordered on `stream`,
 * nothing waits on the host, and a workspace may be reused by the next call on the same stream without clearing.  Refused
 * (HDF_ERR_ARG, message "morphology: ...") before anything is launched: a dimension outside 1..1024, D*H*W >= 2^31,
 * connectivity not 6 / 18 / 26, label outside 0..255, iterations outside 1..256, border_value not 0 / 1, an unknown op or
 * mode, HDF_MORPH_MAP with label = 0, a null required pointer, a workspace below hdf_morph_workspace_bytes(D, H, W) or
 * hdf_fill_holes_workspace_bytes(D, H, W) (-1 for refused dimensions) or not aligned to 8 bytes, out overlapping volume
 * without being volume, the workspace or result overlapping volume, out or each other. */
#define HDF_MORPH_DILATE 0
#define HDF_MORPH_ERODE 1
#define HDF_MORPH_OPEN 2
#define HDF_MORPH_CLOSE 3
#define HDF_MORPH_MASK 0
#define HDF_MORPH_MAP 1
int64_t hdf_morph_workspace_bytes(int D, int H, int W);
int hdf_morph(const uint8_t* volume, int label, int op, int connectivity, int iterations, int border_value, int mode, int D,
              int H, int W, uint8_t* out, uint64_t* result, void* workspace, int64_t workspace_bytes, hdf_stream stream);
int64_t hdf_fill_holes_workspace_bytes(int D, int H, int W);
int hdf_fill_holes(const uint8_t* volume, int label, int connectivity, int mode, int D, int H, int W, uint8_t* out,
                   uint64_t* result, void* workspace, int64_t workspace_bytes, hdf_stream stream);

/* ---- lesion candidates from a probability map: the "dynamic" lesion extraction of detection evaluation (peak, threshold
 * at peak / factor, the component of the peak, drop what touches an accepted candidate, num_lesions lesions).  The reference
 * has no such code: its users copy the fp32 map to the host and run scipy.ndimage.label once per round.  prob: fp32
 * [D][H][W] on the device.  This text is the contract; it claims equality with no package.
 *   setup      w = prob where 0 < prob <= FLT_MAX, else 0 (NaN, negative, -0 and inf become 0); detection_map = 0 (fp32),
 *            indexed = 0 (int32), kept = 0, the table all zeros.
 *   one round  1. kept == num_lesions: finished, reason 1 (count).
 *            2. m = max(w), a = the smallest linear index with w[a] == m; (double)m < stop: finished, reason 2 (stop).
 *            3. thr = (double)m / factor, one fp64 division; the mask is (double)w[v] > thr (a is in it: factor > 1, m > 0).
 *            4. the mask labelled under `connectivity` (hdf_cc_label's kernels); cur = the component of a, size = |cur|.
 *            5. touch = some voxel of cur has a voxel with indexed > 0 in its 3x3x3 neighbourhood, itself included,
 *               clipped at the faces -- always the 26-neighbourhood, whatever `connectivity` is.
 *            6. status 1 (adjacent) if remove_adjacent and touch; else 2 (small) if size < min_voxels; else 0 (kept):
 *               kept += 1, detection_map = m and indexed = kept over cur.
 *            7. w = 0 over cur whatever the status; table row `round` = index (kept, or 0 for a dropped candidate), the
 *               bits of m, size, a, status, the fp64 bits of thr; round += 1.
 *            A dropped candidate takes no index and does not count towards num_lesions; it still leaves w, which is what
 *            ends the loop.  A finished call changes nothing in later rounds.
 *   rounds     the call runs `rounds` rounds.  first_round == 0 starts from the setup; first_round == k > 0 continues the
 *            state that the previous call left in the same workspace, detection_map, indexed and table, and must equal the
 *            rounds run so far -- where it does not (or the workspace holds no state) nothing is changed and result[2] is 3.
 *            This is a check on the device, not on the host.  The other arguments must be those of the first call.
 *   table      int64 [table_rows][6], one row per round run; a round past table_rows leaves no row and is counted instead.
 *   result     [4] uint64 = the rounds run so far (over all calls), kept, finished (0 running, 1 count, 2 stop, 3 a
 *            first_round that does not fit), the rows dropped for table_rows.
 * The peak is the maximum over (bits of w << 32 | 0xFFFFFFFF - index), one 64-bit integer atomicMax per workgroup:
 * non-negative floats order as their bits, so m, a and the first-index tie rule are exact.  Integer atomics only; every
 * output is exact and the same from call to call.  No kernel waits on another workgroup (csrc/detect.hip).  All pointers
 * are device memory, the kernels are ordered on `stream` and nothing waits on the host.  Refused (HDF_ERR_ARG, message
 * "detect: ...") before anything is launched: a dimension outside 1..1024, D*H*W >= 2^31, num_lesions < 1, factor <= 1 or
 * not finite, stop <= 0 or not finite, connectivity not 6 / 18 / 26, remove_adjacent not 0 / 1, min_voxels < 0, rounds < 1,
 * first_round < 0, table_rows < 0, a null required pointer (table may be null when table_rows = 0), a workspace below
 * hdf_detect_workspace_bytes(D, H, W) (w, the mask, the ids, 256 bytes of state and hdf_cc_workspace_bytes, about 14 bytes
 * a voxel; -1 for refused dimensions) or not aligned to 8 bytes, any of prob, detection_map, indexed, table, result and
 * the workspace overlapping another. */
int64_t hdf_detect_workspace_bytes(int D, int H, int W);
int hdf_detect_candidates(const float* prob, int D, int H, int W, int num_lesions, double factor, double stop,
                          int connectivity, int remove_adjacent, int64_t min_voxels, int first_round, int rounds,
                          float* detection_map, int32_t* indexed, int64_t* table /* [table_rows][6] */, int64_t table_rows,
                          uint64_t* result /* [4] */, void* workspace, int64_t workspace_bytes, hdf_stream stream);

/* ---- input normalisation on the device, in place on one fp32 sample [channels][voxels] -----------------------
 * hdf_normalize_mr: MRNormalize (data_utils/data_loader.py:39-50): every channel divided by its maximum when that is
 * non-zero, then negatives clamped to 0.  hdf_normalize_petct: PETandCTNormalize (:53-68): channel 0 ->
 * (clip(x, mean-w, mean+w) - mean) / w, channel 1 -> (x - mean_1) / (std_1 + 1e-3) (population std), others untouched.
 * workspace: hdf_normalize_workspace_bytes(channels) bytes. */
int64_t hdf_normalize_workspace_bytes(int channels);
int hdf_normalize_mr(float* image, int channels, int64_t voxels, void* workspace, hdf_stream stream);
int hdf_normalize_petct(float* image, int channels, int64_t voxels, float mean, float w, void* workspace,
                        hdf_stream stream);

/* ---- sliding-window inference (trainer.py:488-593): the per-window tail of the loop and the final vote.
 * hdf_sw_accumulate: softmax over classes of one window's full-resolution logits [n_cls][pd][ph][pw] (NCDHW, the
 * model's out0 for batch 1), added into prob_sum[n_cls][D][H][W] at (z0,y0,x0); count[D][H][W] += 1
 * (trainer.py:559-576; the reference keeps n_cls identical count planes).
 * hdf_sw_finalize: label[v] = argmax_c softmax(prob_sum[c][v] / count[v]) (trainer.py:580-584), uint8, first
 * maximum wins; voxels no window covered (count 0) give 0. */
int hdf_sw_accumulate(int dtype, const void* logits, int n_cls, int pd, int ph, int pw, float* prob_sum, float* count,
                      int D, int H, int W, int z0, int y0, int x0, hdf_stream stream);
int hdf_sw_finalize(const float* prob_sum, const float* count, int n_cls, int64_t voxels, uint8_t* label,
                    hdf_stream stream);

/* ---- the same loop with a Gaussian importance map (SemanticSeg.get_gaussian, trainer.py:620-638, whose use sits
 * commented out at trainer.py:566-576) and mirror test-time augmentation: three launches per window beside its forward.
 * A window has the origin (z0,y0,x0) and the clipped extent (ed,eh,ew) = min(size, patch) per axis inside the patch
 * (Pd,Ph,Pw) the net takes.  mirror_mask: bit 0 = z, bit 1 = y, bit 2 = x; the K = 2^popcount(mask) variants are the
 * subsets of the mask in ascending order of their 3-bit code m.
 * hdf_sw_gather: out[k][c][z][y][x] = image[c][z0 + z'][y0 + y'][x0 + x'] with z' = ed-1-z when bit 0 of m is set, else z
 * (likewise y, x) for z < ed, y < eh, x < ew, and 0 elsewhere: the content is mirrored within the extent and the zero
 * padding stays at the high end of every axis.  image [channels][D][H][W] fp32; every element of out is written.
 * hdf_sw_accumulate_tta: logits [K][n_cls][Pd][Ph][Pw] are the net's answers to those K inputs; logits voxel (z,y,x) of
 * variant m belongs to window voxel (z',y',x').  Per window voxel v at volume offset o: p_c = (1/K) * sum_m softmax_m(c)
 * (fp32, max-subtracted, e * (1 / sum), m ascending), prob_sum[c][o] += w * p_c, weight_sum[o] += w, each a separate fp32
 * rounding; the logits are read with the patch's strides, so a clipped window needs no copy.  w = 1 when tables is null;
 * with mask 0 and no tables the entry computes hdf_sw_accumulate's result in every bit.  Otherwise tables = tz[ed] | ty[eh]
 * | tx[ew] (device, fp64): per axis of length n, sigma = n * sigma_scale, r = int(4 sigma + 0.5), k[j] =
 * exp(-0.5 / sigma^2 * j^2) for |j| <= r normalised to sum 1, t[i] = k[i - n/2] where |i - n/2| <= r, else 0 (what
 * scipy.ndimage.gaussian_filter does to a unit impulse at n/2 along that axis; hdf_rt.inference.gaussian_tables).
 * w = float(((tz[z] * ty[y]) * tx[x]) / ((tz[ed/2] * ty[eh/2]) * tx[ew/2])), fp64 in this order, one rounding to fp32,
 * denormal results kept; where that is 0, w = *floor.  This is get_gaussian's map in every bit.
 * hdf_sw_importance_floor: *floor_out (device) = the smallest non-zero w of the window, an integer minimum over the bit
 * patterns: the same from call to call, and the host never waits for it.
 * hdf_sw_finalize votes on the result with weight_sum in the place of count.  Windows are accumulated one after the
 * other on one stream: no float atomics.  Refused (HDF_ERR_ARG) before anything is launched: n_cls outside 1..8, an
 * extent below 1 or beyond the patch, a window outside the volume, mirror_mask > 7, tables without floor or floor
 * without tables, ed + eh + ew > 4096 with tables, 2^31 or more elements in out or voxels in the window. */
int hdf_sw_gather(const float* image, int channels, int D, int H, int W, int z0, int y0, int x0, int ed, int eh, int ew,
                  int Pd, int Ph, int Pw, unsigned mirror_mask, float* out, hdf_stream stream);
int hdf_sw_importance_floor(const double* tables, int ed, int eh, int ew, float* floor_out, hdf_stream stream);
int hdf_sw_accumulate_tta(int dtype, const void* logits, unsigned mirror_mask, int n_cls, int ed, int eh, int ew, int Pd,
                          int Ph, int Pw, const double* tables, const float* floor, float* prob_sum, float* weight_sum,
                          int D, int H, int W, int z0, int y0, int x0, hdf_stream stream);

/* ---- slice-wise volume inference for the 2-D model (eval.py:125-230: normalise every plane, push the slices through
 * the net, softmax, stack to [n_cls][D][H][W], argmax): the launches around the forward of a group of slices.  image is
 * the volume [channels][D][H][W] fp32.  An in-plane window has the origin (y0,x0) and the clipped extent (eh,ew) =
 * min(size, patch) per axis inside the patch (Ph,Pw) the net takes, and covers the slices z0 .. z0+nz-1.  mirror_mask:
 * bit 0 = y, bit 1 = x; the K = 2^popcount(mask) variants are the subsets of the mask in ascending order of their code m.
 * hdf_plane_max: max_out[p] = the maximum of plane p of `planes` fp32 planes of plane_voxels each (for a volume:
 * planes = channels * D, p = c * D + z).  Exact: a maximum has no rounding.  The inputs must be finite (a NaN is
 * skipped, not propagated); of zeros of both signs either may come back.  One workgroup forms one plane's maximum: the
 * same from call to call.
 * hdf_slice_gather: out[s][k][c][y][x] = f(image[c][z0 + s][y0 + y'][x0 + x']) with y' = eh-1-y when bit 0 of m is set,
 * else y (likewise x) for y < eh, x < ew, and 0 elsewhere: slices outer, a slice's K variants side by side, the content
 * mirrored within the extent, the zero padding at the high end of both axes; every element of out is written.
 * norm_mode 0: f(v) = v.  1: MRNormalize plane by plane (data_utils/data_loader.py:39-50, the validation chain of
 * trainer.py:173-176): v / max when max != 0, else v, then negatives to 0.  2: Normalize_2d (eval.py:112-123): the same
 * without the clamp.  max = plane_max[c * D + z0 + s], the maximum of the whole plane (hdf_plane_max), not of the
 * window; the division is one IEEE fp32 division, as in hdf_normalize_mr.
 * hdf_slice_accumulate: logits [nz][K][n_cls][Ph][Pw] are the net's answers to that batch.  Per slice the arithmetic is
 * hdf_sw_accumulate_tta's on a window of depth 1, word for word: p_c = (1/K) * sum_m softmax_m(c) (fp32, max-subtracted,
 * e * (1 / sum), m ascending), prob_sum[c][o] += w * p_c, weight_sum[o] += w, each a separate fp32 rounding, the logits
 * read with the patch's strides; without mirroring and tables it is hdf_sw_accumulate's result in every bit.  w = 1 when
 * tables is null.  Otherwise tables = ty[eh] | tx[ew] (device, fp64; hdf_rt.inference.gaussian_tables((eh, ew))), w =
 * float((ty[y] * tx[x]) / (ty[eh/2] * tx[ew/2])), fp64, one rounding to fp32, denormal results kept; where that is 0,
 * w = floor, which the caller forms on the host from the same tables: the smallest non-zero w of the window.  This is
 * get_gaussian((eh, ew)) (trainer.py:620-638) in every bit.  One launch covers the nz slices; their voxels are disjoint:
 * no float atomics.  hdf_sw_finalize votes on the result.
 * Refused (HDF_ERR_ARG) before anything is launched: n_cls outside 1..8, nz < 1 or z0 + nz > D, a window outside the
 * plane, an extent below 1 or beyond the patch, mirror_mask > 3, norm_mode outside 0..2 or non-zero without plane_max,
 * eh + ew > 4096 with tables, 2^31 or more elements in out or voxels in the launch. */
int hdf_plane_max(const float* image, int planes, int64_t plane_voxels, float* max_out, hdf_stream stream);
int hdf_slice_gather(const float* image, int channels, int D, int H, int W, int z0, int nz, int y0, int x0, int eh, int ew,
                     int Ph, int Pw, unsigned mirror_mask, int norm_mode, const float* plane_max, float* out,
                     hdf_stream stream);
int hdf_slice_accumulate(int dtype, const void* logits, unsigned mirror_mask, int n_cls, int nz, int eh, int ew, int Ph,
                         int Pw, const double* tables, float floor, float* prob_sum, float* weight_sum, int D, int H, int W,
                         int z0, int y0, int x0, hdf_stream stream);

/* ---- label staging (data_utils/data_loader.py:126-159, To_Tensor): uint8 class map [N][voxels] -> fp32 one-hot
 * [N][n_cls][voxels]; channel z>=1 is (label == z), channel 0 is "no other class" (so values >= n_cls count as
 * background).  Ships 1 byte per voxel over PCIe instead of 4*n_cls. */
int hdf_onehot_from_labels(const uint8_t* labels, float* onehot, int batch, int n_cls, int64_t voxels,
                           hdf_stream stream);

/* ---- training augmentation of one sample on the device: RandomTranslationRotationZoom3D, RandomFlip3D and To_Tensor
 * (data_utils/transformer_3d.py:45-169, data_utils/data_loader.py:126-159) in one launch.
 * image [channels][D][H][W] fp32 and labels [D][H][W] uint8, both contiguous.  For output voxel p = (d, h, w) -- with
 * h -> H-1-h when flip_h and w -> W-1-w when flip_w, i.e. the flip follows the warp -- the source coordinate is
 * c = A (p - s) + t + s, s = (D/2, H/2, W/2), [A | t] = affine: 12 doubles on the HOST, row-major 3x4, read during the
 * call.  Interpolation is what skimage.transform.warp does on a 3-D array since release 0.19:
 * scipy.ndimage.map_coordinates(order=1, mode='grid-constant', cval=0), trilinear on the volume zero-padded to infinity
 * (a corner outside contributes 0; a coordinate in (-1, 0) blends the edge voxel with 0), accumulated in fp64 and
 * rounded once to fp32.  warp's clip=True is not applied (a no-op here whenever a channel's range contains 0).
 * Labels (transformer_3d.py:113-116): for z = 1 .. n_cls-1 ascending, the interpolated (label == z) mask is compared
 * with `>= 0.5` (inclusive) in fp64 and the LAST class that reaches it wins, else 0; label values >= n_cls match no
 * class and act as background.
 * Outputs, each written when non-null: image_out [channels][D][H][W], labels_out [D][H][W] uint8, onehot_out
 * [n_cls][D][H][W] fp32 in the To_Tensor layout of hdf_onehot_from_labels.  labels may be null only when both label
 * outputs are null (image likewise when image_out is null).  No output may overlap a source.  channels 1..64,
 * n_cls 2..8, every dimension >= 1. */
int hdf_augment_3d(const float* image, const uint8_t* labels, int channels, int n_cls, int D, int H, int W,
                   const double* affine, int flip_h, int flip_w, float* image_out, uint8_t* labels_out, float* onehot_out,
                   hdf_stream stream);

/* ---- training augmentation of a 2-D batch on the device: RandomRotate2D, RandomFlip2D and To_Tensor
 * (data_utils/transformer_2d.py:80-173, data_utils/data_loader.py:126-159), BIT FOR BIT what PIL computes (pinned to
 * PIL 12.2.0: Image.rotate(angle, BILINEAR) on a mode-F plane, Image.rotate(angle, NEAREST) on a mode-L label).
 * image [batch][channels][H][W] fp32 and labels [batch][H][W] uint8, both contiguous.  matrices: [batch][6] doubles on
 * the HOST, m = (a, b, c, d, e, f) in the convention of PIL's Image.transform(AFFINE) (output pixel -> input
 * coordinate); flips: [batch] bytes on the HOST, 0 none, 1 mirrors W, 2 mirrors H.  Both are read during the call.
 * For output pixel (y, x) of a sample, first the flip: x -> W-1-x (1) or y -> H-1-y (2), i.e. the flip follows the
 * rotation.  Then
 *   image (PIL's affine_transform + bilinear_filter32F; fp64, every operation rounded, nothing fused):
 *     xin = a*(x+0.5) + b*(y+0.5) + c,  yin = d*(x+0.5) + e*(y+0.5) + f, summed left to right.
 *     xin < 0 || xin >= W || yin < 0 || yin >= H: the output is 0.0f.  Otherwise xin -= 0.5, yin -= 0.5,
 *     x0 = floor(xin), y0 = floor(yin), dx = xin - x0, dy = yin - y0; on row clamp(y0, 0, H-1) the pixels p0, p1 of the
 *     columns clamp(x0, 0, W-1), clamp(x0+1, 0, W-1): v1 = (double)p0 + (double)(float)(p1 - p0) * dx -- the neighbour
 *     difference is an fp32 subtraction --; v2 the same on row y0+1 when 0 <= y0+1 < H, else v2 = v1;
 *     out = (float)(v1 + (v2 - v1) * dy).
 *   labels (PIL's affine_fixed, 16.16 fixed point): FIX(v) = (int64)floor(v*65536.0 + 0.5); a0 = FIX(a), a1 = FIX(b),
 *     a3 = FIX(d), a4 = FIX(e), a2 = FIX(c + a*0.5 + b*0.5), a5 = FIX(f + d*0.5 + e*0.5);
 *     xi = (a2 + y*a1 + x*a0) >> 16, yi = (a5 + y*a4 + x*a3) >> 16 (arithmetic shift; equal to PIL's running sums, the
 *     integers being exact); labels_out = labels[yi][xi] when 0 <= xi < W && 0 <= yi < H, else 0.  The raw byte moves
 *     unchanged.
 *   one-hot of the moved byte by the rule of hdf_onehot_from_labels.
 * Outputs, each written when non-null: image_out [batch][channels][H][W], labels_out [batch][H][W] uint8, onehot_out
 * [batch][n_cls][H][W] fp32.  labels may be null only when both label outputs are null (image likewise when image_out
 * is null).  No output may overlap a source.
 * Refused with a message before any launch: a null or non-finite matrix; a matrix for which
 * |x*a + y*b + c| < 32768 && |x*d + y*e + f| < 32768 fails at one of (0,0), (W,0), (0,H), (W,H) (PIL's check_fixed:
 * past it PIL itself leaves the fixed-point path); flips[i] > 2; H or W outside 1..16384, channels outside 1..64, n_cls
 * outside 2..8, batch < 1.
 * ceil(batch / 32) launches (the per-sample parameters travel in the kernel arguments), no host synchronisation, no
 * allocation. */
int hdf_augment_2d(const float* image, const uint8_t* labels, int batch, int channels, int n_cls, int H, int W,
                   const double* matrices, const uint8_t* flips, float* image_out, uint8_t* labels_out, float* onehot_out,
                   hdf_stream stream);

/* ---- the rest of the reference's 2-D transform list on the device: RandomErase2D (3), RandomZoom2D (4),
 * RandomAdjust2D (8) and RandomNoise2D (9) of trainer.py:152-168 (data_utils/transformer_2d.py).  They run before
 * (erase, zoom) and after (gamma, noise) hdf_augment_2d, which still makes the one-hot.
 *
 * hdf_label_bbox_2d: labels [batch][H][W] uint8 on the device -> bbox [batch][5] int32 on the device,
 * (nonzero_count, rmin, rmax, cmin, cmax) of the non-zero bytes of each sample; a sample without one gives
 * (0, H, -1, W, -1).  RandomErase2D and RandomZoom2D both branch on it before they draw.  Two launches for the batch, no
 * host synchronisation, no allocation; workspace: hdf_label_bbox_workspace_bytes(batch) bytes.  H and W 1..16384,
 * batch 1..65535. */
int64_t hdf_label_bbox_workspace_bytes(int batch);
int hdf_label_bbox_2d(const uint8_t* labels, int batch, int H, int W, int32_t* bbox, void* workspace,
                      int64_t workspace_bytes, hdf_stream stream);

/* hdf_zoom_2d: erase, crop or pad, and resample a batch in one gather launch per 32 samples, BIT FOR BIT what PIL 12.2.0
 * computes: resize((W, H), BILINEAR) of the mode-F canvas per image plane, resize((W, H), NEAREST) of the mode-L canvas
 * of the class map.  image [batch][channels][H][W] fp32 and labels [batch][H][W] uint8, both contiguous.  On the HOST,
 * read during the call, per sample:
 *   keep [batch][4] int32 = (r0, r1, c0, c1): source pixels of the IMAGE outside rows [r0, r1) or columns [c0, c1) read
 *     as 0.0f (RandomErase2D; the labels are not touched).  (0, H, 0, W) erases nothing, r0 == r1 everything.
 *   canvas [batch][4] int32 = (sw, sh, ox, oy): the canvas is sw wide and sh high; its pixel (cy, cx) is the source
 *     pixel (cy - oy, cx - ox) when that lies inside the plane, else 0.  PIL's crop((x1, y1, x1+tw, y1+th)) is
 *     (tw, th, -x1, -y1); ImageOps.expand(border=(p0, p1, tw-W, th-H), fill=0) is (tw+p0, th+p1, p0, p1).
 * image (ImagingResample: two separable passes, horizontal then vertical, fp64, every operation rounded, nothing
 *   fused).  One axis with input size n_in (sw or sh) and output size n_out, output index xx:
 *     scale = (double)n_in / n_out, fs = max(scale, 1.0), support = fs, ss = 1.0 / fs,
 *     center = (xx + 0.5) * scale,
 *     xmin = (int)(center - support + 0.5) clamped below at 0, xmax = (int)(center + support + 0.5) clamped above at n_in,
 *     for x in [0, xmax - xmin): t = (x + xmin - center + 0.5) * ss, w[x] = 1 - |t| if |t| < 1 else 0,
 *     ww = sum of w left to right, k[x] = w[x] / ww when ww != 0,
 *     out = (float)(sum of (double)pixel[xmin + x] * k[x], left to right from 0.0).
 *   The horizontal result is rounded to fp32 before the vertical pass reads it.  A pass whose n_in == n_out is skipped:
 *   the value passes through unchanged (so a canvas of (W, H, 0, 0) copies the erased plane, -0.0 included).
 * labels (ImagingScaleAffine, nearest): per axis a0 = (double)n_in / n_out and a RUNNING sum xo = a0 * 0.5; for each
 *   output index in order src = (int)xo, then xo += a0 -- the roundings of the running sum are part of the contract,
 *   (int)((x + 0.5) * a0) differs at some sizes.  labels_out = canvas[src_y][src_x]; the raw byte moves unchanged.
 * Outputs, each written when non-null: image_out [batch][channels][H][W], labels_out [batch][H][W].  labels may be null
 * when labels_out is (image likewise).  No output may overlap a source or the other output.
 * Refused with a message before any launch: null keep or canvas, no output, an output without its source, overlapping
 * buffers; sw outside [ceil(W/4), 4W] or sh outside [ceil(H/4), 4H]; |ox| or |oy| above 65536; a keep-rectangle that is
 * not 0 <= r0 <= r1 <= H, 0 <= c0 <= c1 <= W; H or W outside 1..16384, channels outside 1..64, batch < 1.
 * ceil(batch / 32) launches (the per-sample parameters travel in the kernel arguments), no host synchronisation, no
 * allocation. */
int hdf_zoom_2d(const float* image, const uint8_t* labels, int batch, int channels, int H, int W, const int32_t* keep,
                const int32_t* canvas, float* image_out, uint8_t* labels_out, hdf_stream stream);

/* hdf_intensity_2d: gamma and Gaussian noise in place on image [batch][channels][H][W] fp32, one launch per 32 samples.
 * On the HOST, read during the call: gamma [batch] doubles (1.0 leaves the sample alone) and noise [batch] bytes, 0 or 1.
 * gamma (skimage's adjust_gamma on a float image, (image / 1.0) ** gamma * 1.0): x > 0 -> (float)pow((double)x,
 *   (double)(float)gamma), one rounding; x <= 0 -> 0 (skimage raises on negative input; MRNormalize leaves none).  A
 *   gamma that rounds to 1.0f leaves the bits alone.
 * noise, after the gamma (skimage's random_noise(mode='gaussian'), mean 0, var 0.01): out = (float)clip((double)x +
 *   0.1 * z, low_clip, 1.0), z ~ N(0, 1).  skimage takes low_clip = -1 when the image holds a negative, else 0; the
 *   caller says which.  z = sqrt(-2 ln u1) * cos(2 pi u2) in fp64 from Philox-4x32-10 with the key (seed low word, seed
 *   high word) on the counter (e low word, e high word, sample, 0), e the element's index within its sample:
 *   u1 = ((w0 << 20 | w1 >> 12) + 0.5) * 2^-52, u2 = (w2 + 0.5) * 2^-32.  z is a pure function of (seed, sample, e): no
 *   generator state lives on the device and nothing depends on the launch geometry.  The field is statistical, not the
 *   reference's np.random stream.
 * Refused before any launch: a null argument, a gamma that is negative or not finite, noise[i] > 1, a low_clip that is
 * not finite or above 1, H or W outside 1..16384, channels outside 1..64, batch < 1.  No host synchronisation, no
 * allocation. */
int hdf_intensity_2d(float* image, int batch, int channels, int H, int W, const double* gamma, const uint8_t* noise,
                     uint64_t seed, float low_clip, hdf_stream stream);

/* ---- CropResize of the 3-D transform list (id 3 of trainer.py:128-142; data_utils/data_loader.py:71-123): the resize of
 * one sample to the network's input shape.  image [channels][Di][Hi][Wi] fp32 -> image_out [channels][Do][Ho][Wo], each
 * channel what skimage.transform.resize(image[i], dim, anti_aliasing=True) computes; labels [Di][Hi][Wi] uint8 ->
 * labels_out [Do][Ho][Wo]: for z = 1 .. n_cls-1 ascending, roi = resize((label == z) as fp32, dim, mode='constant') and
 * out[roi >= 0.5] = z -- the LAST class that reaches 0.5 wins, a class beats background at exactly 0.5, label values
 * >= n_cls match no class and become background.  The indicator is formed while the class map is read; no mask is stored.
 * resize(order=1) of scikit-image >= 0.19 is scipy, and this entry restates scipy 1.15 (agreement with scikit-image
 * itself is by reading its source, not by measurement).  Per axis, n_in -> n_out samples:
 *   f = n_in / n_out; sigma = max(0, (f - 1) / 2); an axis with sigma <= 1e-15 is not filtered; else
 *   gaussian_filter(truncate=4): radius r = int(4 sigma + 0.5), weights exp(-0.5 k^2 / sigma^2), k = -r..r, normalised to
 *   sum 1; then zoom(order=1, grid_mode=True): output index o reads the source coordinate c = (o + 0.5) f - 0.5, linear
 *   between floor(c) and floor(c) + 1.
 *   boundary, in the filter and in the interpolation alike: image 'mirror' -- index p reads p' = |p| mod (2 n_in - 2), or
 *   2 n_in - 2 - p' when p' >= n_in (0 when n_in = 1), as often as the radius needs; labels 'grid-constant' with cval 0 -- a
 *   sample outside [0, n_in) is 0.
 * The three axes commute.  scipy rounds to fp32 after every filtered axis and after the interpolation; this entry does
 * NOT: one axis is one banded operator (the interpolation row applied to the filter rows, at most 2r + 2 = 30 taps), the
 * operators are applied one after the other with fp64 accumulation and fp64 intermediates, and the result is rounded to
 * fp32 once, or compared with 0.5 in fp64.  It therefore differs from live scipy by scipy's own roundings: at most
 * (g + 1) 2^-24 max|image| with g filtered axes.  Class maps equal scipy's except where a class sum lies within 1e-7 of
 * 0.5 (an exact factor 2 puts edges there), where scipy's outcome is its rounding noise; there the result is unspecified.
 * skimage's final clip to the input range is a no-op (all weights are non-negative).
 * Either pair image / image_out or labels / labels_out may be null (a labels-only or an image-only call), not both.
 * Equal shapes are legal and give a copy (labels: values >= n_cls become 0).
 * workspace: hdf_resize_workspace_bytes(...) bytes, 8-byte aligned: the fp64 intermediates of ONE plane (the planes take
 * turns), 0 when at most one axis changes its size; -1 for shapes that hdf_resize_3d refuses.
 * Refused with HDF_ERR_ARG and a "resize_3d:" message before any launch: a dimension outside 1..1024; n_in > 8 n_out on
 * an axis (the cap that bounds the taps); n_cls outside 2..8; channels outside 0..64 (0 only without an image); a half
 * pair; no pair; a workspace that is too small; an output or the workspace overlapping any other buffer.
 * At most 3 (channels + n_cls - 1) launches, no host synchronisation, no copy, no allocation. */
int64_t hdf_resize_workspace_bytes(int Di, int Hi, int Wi, int Do, int Ho, int Wo);
int hdf_resize_3d(const float* image, const uint8_t* labels, int channels, int n_cls, int Di, int Hi, int Wi, int Do, int Ho,
                  int Wo, float* image_out, uint8_t* labels_out, void* workspace, int64_t workspace_bytes,
                  hdf_stream stream);

/* Trunc_and_Normalize (ids 7 / 11; data_utils/data_loader.py:16-36) in place on n fp32 values, bit for bit the numpy
 * sequence: x = x - lo; x < 0 -> 0; x > hi - lo -> hi - lo; x = x / (hi - lo), every step in fp32 (hi - lo is formed
 * in fp32 too).  Refused with a "trunc_normalize:" message: a null image, n < 1, hi <= lo, a value that is not finite. */
int hdf_trunc_normalize(float* image, int64_t n, float lo, float hi, hdf_stream stream);

/* ---- optimizer: torch.optim.Adam as configured by trainer.py:793-840 (L2 weight decay on the mask) ----
 * decay_mask may be null (no decay anywhere); grad_scale MULTIPLIES the gradient; step is 1-based.
 * The betas are taken at their fp32 values: the bias corrections 1 - beta1^step and sqrt(1 - beta2^step) are formed from
 * them in double and rounded to fp32 once.  torch forms its corrections from the Python doubles; for beta2 = 0.999 (0.999f
 * is 1.29e-8 above it) its sqrt(1 - beta2^step) lies 6.4e-6 (relative) from this entry's in the first steps, 6.1e-6 at
 * step 100 and still 1e-6 at step 3000, and every update differs by that factor (tests/test_optim_ref_cpu.py holds the
 * figures). */
int hdf_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const uint8_t* decay_mask,
                  int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                  float grad_scale, hdf_stream stream);

/* ---- flat optimizer step: the three optimizers of trainer.py:793-840 as torch computes them in fp32, one streaming
 * kernel over the flat buffers (plus a one-thread prologue), nothing read back by the host.
 * rule: HDF_OPTIM_ADAM (L2 decay added to the gradient: the rule of hdf_adam_step, same bits), HDF_OPTIM_ADAMW
 * (decoupled: p *= 1 - lr*wd before the moment update), HDF_OPTIM_SGD (L2 decay, momentum buffer with dampening 0,
 * initialised to the gradient by the first step; nesterov != 0: g + momentum*buf).
 * state1 / state2: exp_avg / exp_avg_sq, or the momentum buffer / null for SGD; beta1 is the momentum of SGD (beta2 and
 * eps unused).  Two parameter groups chosen by the decay_mask byte: lr_decay / wd_decay where it is set, lr_rest /
 * wd_rest elsewhere.  The gradient used is g * grad_mul / *grad_scale.  SGD's step 1 (word 0 of step_state at 0) REPLACES
 * the momentum buffer by the gradient, whatever the buffer held.
 * Every hyper-parameter is taken at its fp32 value.  The bias corrections 1 - beta1^step and sqrt(1 - beta2^step) are
 * formed from the fp32 betas in double and rounded to fp32 once.  torch forms its corrections from the Python doubles; for
 * beta2 = 0.999 (0.999f is 1.29e-8 above it) its sqrt(1 - beta2^step) lies 6.4e-6 (relative) from this entry's in the first
 * steps, 6.1e-6 at step 100 and still 1e-6 at step 3000, and every Adam / AdamW update differs by that factor
 * (tests/test_optim_ref_cpu.py holds the figures; tests/optim_ref.py is the fp64 statement of the three rules).
 * grad_scale, found_inf (each may be null): DEVICE pointers to one fp32, the protocol of torch.amp.GradScaler for
 * optimizers that unscale inside their step.  *found_inf != 0: the call leaves parameters, state buffers and the step
 * counter bit for bit untouched.
 * step_state: HDF_OPTIM_STATE_WORDS int32 on the device, zeroed by the caller before the first step and then left alone.
 * Word 0 is the number of steps taken (the bias correction's exponent; saved and restored with the state buffers); the
 * other words are scratch of the call.
 * params, grads, state1, state2 16-byte aligned, decay_mask 4-byte aligned; any n >= 0. */
#define HDF_OPTIM_ADAM 0
#define HDF_OPTIM_ADAMW 1
#define HDF_OPTIM_SGD 2
#define HDF_OPTIM_STATE_WORDS 8
int hdf_optim_step(int rule, float* params, const float* grads, float* state1, float* state2, const uint8_t* decay_mask,
                   int64_t n, float lr_decay, float lr_rest, float wd_decay, float wd_rest, float beta1, float beta2,
                   float eps, int nesterov, float grad_mul, const float* grad_scale, const float* found_inf,
                   int32_t* step_state, hdf_stream stream);

/* ---- operator level (what nn.Conv3d / ConvTranspose3d / InstanceNorm3d / MaxPool3d / F.interpolate bind
 *      in the reference, HDenseFormer.py:148-175,199-227).  Channels-last activations with a voxel pitch. -- */
int hdf_op_to_channels_last(int dtype, const float* x_ncdhw, void* out, int N, int C, int CP, int64_t voxels,
                            hdf_stream stream);
/* dst[27][OP][IP] = src[o*so + i*si + tap] (tap reversed if flip) */
int hdf_op_pack_weights(int dtype, const float* src, void* dst, int O, int I, int OP, int IP, int64_t so, int64_t si,
                        int flip, hdf_stream stream);
/* mode 0: Conv3d(k3,s1,p1); mode 1: Conv3d(k3,s2,p1); mode 2: ConvTranspose3d(k3,s2,p1,op1).
 * in_scale/in_shift ([N][Cin], may be null): input is relu?(x*scale+shift).  stat_partials may be null.
 * stat_partials (here, in hdf_op_conv3d_wr, hdf_op_conv3d_first and hdf_op_conv3d_split): every kernel sums the fp32
 * value conv + bias BEFORE it is rounded to the storage type, not the stored value (and in an accumulating launch the
 * kernels differ in whether the old output is included: do not combine accumulate with stat_partials). */
int hdf_op_conv3d(int dtype, int mode, const void* in, int64_t in_pitch, int Cin, int N, int Di, int Hi, int Wi,
                  const void* w_packed, const float* bias, const float* in_scale, const float* in_shift, int in_relu,
                  void* out, int64_t out_pitch, int Cout, float* stat_partials, int accumulate, hdf_stream stream);
/* The encoder's first layer as the plan runs it in a 16-bit storage mode (nn.Conv3d(in_channels <= 4, n_filters, 3, padding=1),
 * HDenseFormer.py:152-158,190; csrc/conv_first.hip: K = (tap, channel) instead of 27 quarter-empty channel rows).  in:
 * channels-last, the first Cin of in_pitch channels per voxel are read (in_pitch % 4 == 0); weight: the torch fp32 tensor
 * [Cout][Cin][3][3][3] itself (rounded to the storage type inside); stat_partials (optional): [N][512][round_up(Cout,32)][2]
 * InstanceNorm partial sums (sum, sum of squares of the fp32 results), every row written. */
int hdf_op_conv3d_first(int dtype, const void* in, int64_t in_pitch, int Cin, int N, int D, int H, int W, const float* weight,
                        const float* bias, void* out, int64_t out_pitch, int Cout, float* stat_partials,
                        hdf_stream stream);
/* ... and its weight gradient: dweight [Cout][Cin][3][3][3] fp32 (+)= sum over samples and voxels of dy (x) shifted x.
 * dy: channels-last, Cout (a multiple of 8) of dy_pitch channels; x as above; workspace: >= 2 * 256 * round_up(Cout,32) *
 * 512 bytes of scratch (fp32 partial sums per workgroup, reduced in a fixed order). */
int hdf_op_conv3d_first_wgrad(int dtype, const void* dy, int64_t dy_pitch, int Cout, const void* x, int64_t x_pitch,
                              int Cin, int N, int D, int H, int W, float* dweight, int accumulate, void* workspace,
                              int64_t workspace_bytes, hdf_stream stream);
/* The same with the second pass of the layer's InstanceNorm(+ReLU) backward applied to the rows as they are staged: da is
 * the gradient w.r.t. the activation relu(IN(y)), and dy = k1 * ((y*scale+shift > 0 ? da : 0) - ka - (y-mean)*rstd*kb)
 * (rounded to the storage type: what hdf_op_in_bwd's apply pass would have written) is what enters the weight gradient.
 * The first layer has no input gradient, so dy itself is never needed.  Vectors [N][Cout]. */
int hdf_op_conv3d_first_wgrad_in(int dtype, const void* da, int64_t da_pitch, int Cout, const void* y, int64_t y_pitch,
                                 const float* scale, const float* shift, const float* mean, const float* rstd,
                                 const float* k1, const float* ka, const float* kb, const void* x, int64_t x_pitch, int Cin,
                                 int N, int D, int H, int W, float* dweight, int accumulate, void* workspace,
                                 int64_t workspace_bytes, hdf_stream stream);
/* The same Conv3d(k3,s1,p1) forced through the weights-in-registers kernel (csrc/conv_wr.hip: 16-bit storage, Cin of 32
 * or 64, >= 48^3) whatever the plan's routing rule says; HDF_ERR_UNSUPPORTED for other shapes.  Tests and tools. */
int hdf_op_conv3d_wr(int dtype, const void* in, int64_t in_pitch, int Cin, int N, int D, int H, int W,
                     const void* w_packed, const float* bias, const float* in_scale, const float* in_shift, int in_relu,
                     void* out, int64_t out_pitch, int Cout, float* stat_partials, int accumulate, hdf_stream stream);
/* partial rows per sample of stat_partials ([N*rows][Cout rounded up to 32][2] floats: sum, sum of squares) for this
 * layer shape: one row per output tile, or 512 per-workgroup rows when the weights-stationary kernel takes the layer */
int hdf_op_conv3d_stat_tiles(int dtype, int Cin, int Do, int Ho, int Wo);
/* hdf_op_conv3d (mode 0) as a data gradient whose epilogue also takes the first pass of the NEXT InstanceNorm(+ReLU)
 * backward: out is the gradient w.r.t. the activation relu(IN(y)) of the layer below, and partials [N][512][Cout][2] receive
 * per channel (sum g, sum g * xhat), g = the stored out where y*scale+shift > 0, xhat = (y-mean)*rstd -- the rows
 * hdf_op_in_bwd's reduce pass would produce from (out, y), without that pass.  16-bit storage, Cin = Cout = 32, extents
 * multiples of (4, 8, 8) and >= 48^3 (the level-0 data gradients of the plan); other launches are refused. */
int hdf_op_conv3d_bwd_stats(int dtype, const void* in, int64_t in_pitch, int Cin, int N, int D, int H, int W,
                            const void* w_packed, void* out, int64_t out_pitch, int Cout, const void* y, int64_t y_pitch,
                            const float* scale, const float* shift, const float* mean, const float* rstd,
                            float* partials, hdf_stream stream);
/* Conv3d(k3,s1,p1) whose output channels [0, split) go to `out` and [split, Cout) to `out2` (two dense buffers of one
 * pitch; split % 32 == 0), the form the plan uses for the gradient of a decoder concat [upconv | skip]
 * (models/HDenseFormer.py:245-253 backward).  With stat_partials ([N * hdf_op_conv3d_stat_tiles][round_up(Cout,32)][2])
 * and colsum ([colsum_C] floats) the per-channel sums over all voxels of channels [0, colsum_C) are written too: the
 * ConvTranspose3d bias gradient taken from the conv's statistics epilogue. */
int hdf_op_conv3d_split(int dtype, const void* in, int64_t in_pitch, int Cin, int N, int D, int H, int W,
                        const void* w_packed, void* out, void* out2, int64_t out_pitch, int Cout, int split,
                        float* stat_partials, float* colsum, int colsum_C, hdf_stream stream);
int64_t hdf_op_wgrad_workspace_bytes(int stride, int N, int Ds, int Hs, int Ws, int SC, int LC);
/* dW[sc][lc][27] = sum S[i][sc] * L[stride*i-1+tap][lc]  (torch weight layout for both Conv3d and ConvTranspose3d) */
int hdf_op_conv3d_wgrad(int dtype, int stride, const void* sm, int64_t sm_pitch, int SC, const void* lg,
                        int64_t lg_pitch, int LC, int N, int Ds, int Hs, int Ws, const float* sm_scale,
                        const float* sm_shift, int sm_relu, const float* lg_scale, const float* lg_shift, int lg_relu,
                        float* dw, int sc_store, int lc_store, int accumulate, void* workspace, int64_t workspace_bytes,
                        hdf_stream stream);
int hdf_op_in_finalize(const float* partials, int N, int tiles, int C, int CP, int64_t voxels, const float* gamma,
                       const float* beta, float eps, float* mean, float* rstd, float* scale, float* shift,
                       hdf_stream stream);
/* InstanceNorm3d(+ReLU) backward of one layer (HDenseFormer.py:152-158): da = d/d(relu(IN(y))) -> dy = d/dy, plus
 * dgamma / dbeta (accumulated; may be null).  workspace: hdf_op_in_bwd_workspace_floats(N, C, voxels) floats. */
int64_t hdf_op_in_bwd_workspace_floats(int N, int C, int64_t voxels);
int hdf_op_in_bwd(int dtype, const void* da, int64_t da_pitch, const void* y, int64_t y_pitch, const float* scale,
                  const float* shift, const float* mean, const float* rstd, const float* gamma, void* dy,
                  int64_t dy_pitch, float* dgamma, float* dbeta, int N, int C, int64_t voxels, float* workspace,
                  hdf_stream stream);
/* The same backward with its second pass INSIDE the layer's weight gradient (round 5; 16-bit storage, Conv3d k3 s1 p1;
 * reference: models/HDenseFormer.py:148-159 backward): the reduce + finalize passes of hdf_op_in_bwd, then ONE launch that
 * applies the second pass to the rows of d(activation) it stages, writes dy (bit-identical to hdf_op_in_bwd's) and
 * contracts it with the layer's input x -- optionally x -> relu(x * x_scale + x_shift), [N][Cin] -- into
 * dw [Cout][Cin][27] (bit-identical to hdf_op_conv3d_wgrad on that dy).  What hdf_backward does for the 128^3 layers.
 * HDF_ERR_UNSUPPORTED where the fused kernel does not take the launch (fp32 storage, tensors of 2 GiB and more).
 * workspace: hdf_op_in_bwd_workspace_floats(N, Cout, D*H*W) floats; wgrad_workspace: hdf_op_wgrad_workspace_bytes(1, ...). */
int hdf_op_in_bwd_wgrad(int dtype, const void* da, int64_t da_pitch, const void* y, int64_t y_pitch, const float* scale,
                        const float* shift, const float* mean, const float* rstd, const float* gamma, void* dy,
                        int64_t dy_pitch, float* dgamma, float* dbeta, const void* x, int64_t x_pitch, int Cin,
                        const float* x_scale, const float* x_shift, int x_relu, int N, int Cout, int D, int H, int W,
                        float* dw, float* workspace, void* wgrad_workspace, int64_t wgrad_workspace_bytes,
                        hdf_stream stream);
int hdf_op_norm_relu_add(int dtype, const void* y, int64_t y_pitch, const float* scale, const float* shift,
                         const void* skip, int64_t skip_pitch, void* out, int64_t out_pitch, int N, int C,
                         int64_t voxels, hdf_stream stream);
int hdf_op_maxpool_fwd(int dtype, const void* in, int64_t in_pitch, void* out, int64_t out_pitch, uint8_t* idx, int N,
                       int C, int Do, int Ho, int Wo, hdf_stream stream);
/* The encoder tail of a level in one pass (models/HDenseFormer.py:238-243): ds = relu(y * scale + shift) + skip (the
 * InstanceNorm + ReLU of the level's second conv plus the transformer feature at_k), stored, and MaxPool3d(2) of the stored
 * values with the arg-max byte per channel (0..7 = dz*4 + dy*2 + dx, first maximum in scan order as torch).
 * (Do, Ho, Wo) = the pooled size. */
int hdf_op_enc_tail(int dtype, const void* y, int64_t y_pitch, const float* scale, const float* shift, const void* skip,
                    int64_t skip_pitch, void* ds, int64_t ds_pitch, void* pooled, int64_t pooled_pitch, uint8_t* idx,
                    int N, int C, int Do, int Ho, int Wo, hdf_stream stream);
/* hdf_op_enc_tail with skip = Upsample(x2, trilinear)(relu(low * lscale + lshift)) evaluated inside the pass (low at the
 * pooled extent Do x Ho x Wo): level 0 of the encoder, where the skip is the UpConv chain's last feature
 * (HDenseFormer.py:168-175, 237; the up-sampled tensor is not written). */
int hdf_op_enc_tail_up(int dtype, const void* y, int64_t y_pitch, const float* scale, const float* shift, const void* low,
                       int64_t low_pitch, const float* lscale, const float* lshift, void* ds, int64_t ds_pitch,
                       void* pooled, int64_t pooled_pitch, uint8_t* idx, int N, int C, int Do, int Ho, int Wo,
                       hdf_stream stream);
int hdf_op_maxpool_bwd(int dtype, const void* dout, int64_t dout_pitch, const uint8_t* idx, void* din,
                       int64_t din_pitch, int N, int C, int Do, int Ho, int Wo, int accumulate, hdf_stream stream);
/* hdf_op_maxpool_bwd with accumulate = 1 for the encoder levels: din becomes the complete gradient of
 * ds = relu(y * scale + shift) + skip, and the same pass writes the first pass of that InstanceNorm(+ReLU)'s backward:
 * partials[n][row][c][2] = per-workgroup (sum g, sum g * (y - mean) * rstd) with g = the stored din where the activation
 * is positive, hdf_op_maxpool_bwd_in_rows(C, Do, Ho, Wo) rows per sample (what hdf_op_in_bwd's reduce pass would write). */
int hdf_op_maxpool_bwd_in_rows(int C, int Do, int Ho, int Wo);
int hdf_op_maxpool_bwd_in(int dtype, const void* dout, int64_t dout_pitch, const uint8_t* idx, void* din,
                          int64_t din_pitch, const void* y, int64_t y_pitch, const float* scale, const float* shift,
                          const float* mean, const float* rstd, float* partials, int N, int C, int Do, int Ho, int Wo,
                          hdf_stream stream);
int hdf_op_upsample_fwd(int dtype, const void* y, int64_t y_pitch, const float* scale, const float* shift, void* out,
                        int64_t out_pitch, int N, int C, int Di, int Hi, int Wi, hdf_stream stream);
int hdf_op_upsample_bwd(int dtype, const void* dout, int64_t dout_pitch, void* din, int64_t din_pitch, int N, int C,
                        int Di, int Hi, int Wi, hdf_stream stream);
/* The 2-D forms of the four entries above, as the 2-D model's plan runs them, on depth-1 channels-last tensors
 * [N][H][W][pitch].  A pooled depth of 1 is a legitimate call of the 3-D entries (a 2 x 2 x 2 window), so the 2-D form has
 * entries of its own.  (Ho, Wo) / (Hi, Wi): the low-resolution side.
 * hdf_op_enc_tail_2d: ds = relu(y * scale + shift) + skip, stored, and MaxPool2d(2) (models/HDenseFormer_2D.py:194-202)
 * of the stored values with the arg-max byte per channel (0..3 = dy*2 + dx, first maximum in scan order as torch). */
int hdf_op_enc_tail_2d(int dtype, const void* y, int64_t y_pitch, const float* scale, const float* shift, const void* skip,
                       int64_t skip_pitch, void* ds, int64_t ds_pitch, void* pooled, int64_t pooled_pitch, uint8_t* idx,
                       int N, int C, int Ho, int Wo, hdf_stream stream);
/* MaxPool2d(2) backward (models/HDenseFormer_2D.py:194-202) accumulated into din, with the first pass of the
 * InstanceNorm(+ReLU) backward as in hdf_op_maxpool_bwd_in: partials[n][row][c][2] = (sum g, sum g * (y - mean) * rstd), g =
 * the stored din where y * scale + shift is positive, hdf_op_maxpool_bwd_in_rows(C, 1, Ho, Wo) rows per sample. */
int hdf_op_maxpool_bwd_in_2d(int dtype, const void* dout, int64_t dout_pitch, const uint8_t* idx, void* din,
                             int64_t din_pitch, const void* y, int64_t y_pitch, const float* scale, const float* shift,
                             const float* mean, const float* rstd, float* partials, int N, int C, int Ho, int Wo,
                             hdf_stream stream);
/* out [N][2 Hi][2 Wi] = F.interpolate(relu(y * scale + shift), scale_factor=2, mode='bilinear', align_corners=False)
 * (models/HDenseFormer_2D.py:166-170); scale / shift [N][C] are required. */
int hdf_op_upsample_fwd_2d(int dtype, const void* y, int64_t y_pitch, const float* scale, const float* shift, void* out,
                           int64_t out_pitch, int N, int C, int Hi, int Wi, hdf_stream stream);
/* din [N][Hi][Wi] = the adjoint of that bilinear x2 (models/HDenseFormer_2D.py:166-170 backward) applied to
 * dout [N][2 Hi][2 Wi]: 4 x 4 taps per low-resolution element. */
int hdf_op_upsample_bwd_2d(int dtype, const void* dout, int64_t dout_pitch, void* din, int64_t din_pitch, int N, int C,
                           int Hi, int Wi, hdf_stream stream);


/* ---- operator level, transformer branch and heads (what nn.Linear / LayerNorm / GELU / Softmax / matmul / Dropout and
 *      the 1x1x1 nn.Conv3d bind in the reference, HDenseFormer.py:11-145,223-227).  All fp32.
 * Token rows are ordered row = (m*B + b)*N + n (modality, sample, token); the parameters of modality m live at
 * pointer + m*mstride floats (the flat state_dict layout of the plan; pass M = 1 for a single Linear stack).
 * A block's dense feature buffer F is [rows][DM+128]: columns [0,DM) the block input, [DM+32l, DM+32l+32) the feature
 * dense layer l appends (HDenseFormer.py:91-101).  training != 0 applies the p = 0.5 hash dropout of (seed). */

/* Dense_Attention core (:67-74): qkv [nseq*N][96] = (q | k | v), 8 heads x 4 -> ob [nseq*N][32] (heads merged, before
 * to_out) and lse [nseq*N][8] (row log-sum-exp of the 0.5-scaled scores, natural log) */
int hdf_op_attention_fwd(const float* qkv, int nseq, int N, float* ob, float* lse, hdf_stream stream);
int hdf_op_attention_bwd(const float* qkv, const float* ob, const float* lse, const float* d_ob, float* dqkv, int nseq,
                         int N, hdf_stream stream);
/* The backward as the plan runs it in storage mode `dtype` (HDF_F32: identical to hdf_op_attention_bwd).  In the 16-bit
 * modes the scores and the softmax stay fp32 and the accumulations dS.k, dS^T.q and attn^T.d_ob take bf16 / f16 operands
 * with fp32 accumulation on the matrix core: what torch.cuda.amp.autocast does to the torch.matmul calls of
 * Dense_Attention (HDenseFormer.py:70-73 under trainer.py:369).  The forward is the exact one in every mode.
 * Same buffers as above, all fp32. */
int hdf_op_attention_amp_bwd(int dtype, const float* qkv, const float* ob, const float* lse, const float* d_ob,
                             float* dqkv, int nseq, int N, hdf_stream stream);
/* Dense_TransformerBlock front (:115-119,133-138): Conv3d(1 -> DM, k16, s16) + flatten + position embedding + dropout.
 * x: [B][M][D][H][W]; writes F[:, 0:DM].  backward: dF -> dweight (+=), dpos (+=), dbias (+=): all three gradients are
 * ACCUMULATED into what the buffers hold (hdf_backward zeroes the flat gradient buffer first), like every other
 * parameter gradient of this section; scratch rows*DM floats */
int hdf_op_patch_embed_fwd(const float* x, int M, int B, int D, int H, int W, int DM, const float* weight,
                           const float* bias, const float* pos, int64_t mstride, float* F, int training, uint64_t seed,
                           hdf_stream stream);
int hdf_op_patch_embed_bwd(const float* x, int M, int B, int D, int H, int W, int DM, const float* dF, int64_t mstride,
                           float* dweight, float* dbias, float* dpos, float* scratch, int training, uint64_t seed,
                           hdf_stream stream);
/* one dense layer of DensePreConv_AttentionBlock (:93-98): h0 = Linear(F[:, 0:DM+32l]); h1 = attn(LN(h0)) + h0;
 * h2 = ff(LN(h1)) + h1; F[:, DM+32l : +32] = ff(LN(h2)).  params13 / grads13: HOST arrays of 13 device pointers in
 * state_dict order (0.weight, 0.bias, 1.norm.weight, 1.norm.bias, 1.fn.to_qkv.weight, 1.fn.to_out.0.weight,
 * 1.fn.to_out.0.bias, 2.norm.weight, 2.norm.bias, 2.fn.net.0.weight, .bias, 2.fn.net.3.weight, .bias).
 * save: rows*232 floats kept for backward.  backward: dF[:, DM+32l..] is read, dF[:, 0:DM+32l] += ; parameter
 * gradients are ACCUMULATED; scratch rows*160 floats. */
int hdf_op_dense_layer_fwd(int M, int B, int N, int DM, int block, int layer, const float* const* params13,
                           int64_t mstride, float* F, float* save, int training, uint64_t seed, hdf_stream stream);
int hdf_op_dense_layer_bwd(int M, int B, int N, int DM, int block, int layer, const float* const* params13,
                           float* const* grads13, int64_t mstride, const float* F, float* dF, const float* save,
                           float* scratch, int training, uint64_t seed, hdf_stream stream);
/* out_layer of a block (:89,99-100): DenseForward(DM+128 -> 64 -> DM) of the whole feature buffer.  Exactly one of
 * next_F (fp32, next block's F[:, 0:DM]) / attnall (storage dtype, channels-last [B][N][M*DM], the 'b (d h w) c'
 * rearrange + modality concat of :144,230) is written.  params4 / grads4: net.0.weight, net.0.bias, net.3.weight,
 * net.3.bias.  backward writes dF[:, 0:DM+128] (overwrites) and accumulates the parameter gradients. */
int hdf_op_block_out_fwd(int M, int B, int N, int DM, int block, const float* const* params4, int64_t mstride,
                         const float* F, float* next_F, void* attnall, int dtype, int training, uint64_t seed,
                         hdf_stream stream);
int hdf_op_block_out_bwd(int M, int B, int N, int DM, int block, const float* const* params4, float* const* grads4,
                         int64_t mstride, const float* F, const float* dF_next, const void* d_attnall, int dtype,
                         float* dF, int training, uint64_t seed, hdf_stream stream);
/* 1x1x1 head (:223-227): logits [N][n_cls][voxels] (NCDHW, storage dtype) = W . act(in) + b with in channels-last,
 * act = relu(in*scale+shift) when in_scale is given.  backward: dx (+)= W^T dlogits (gradient w.r.t. act(in)),
 * dweight / dbias accumulated. */
int hdf_op_head_fwd(int dtype, const void* in, int64_t in_pitch, const float* in_scale, const float* in_shift,
                    const float* weight, const float* bias, void* logits, int N, int C, int n_cls, int64_t voxels,
                    hdf_stream stream);
int hdf_op_head_bwd(int dtype, const void* dlogits, const void* in, int64_t in_pitch, const float* in_scale,
                    const float* in_shift, const float* weight, void* dx, int64_t dx_pitch, int accumulate_dx,
                    float* dweight, float* dbias, int N, int C, int n_cls, int64_t voxels, hdf_stream stream);

#ifdef __cplusplus
}
#endif
#endif
