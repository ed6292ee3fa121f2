// What the executor's two units share (private to csrc/): Exec (the streams of one forward / backward call and the ordering
// between them), Rejoin, Xf, and the entry points exec.hip calls in exec_tf.hip.
#pragma once
#include <map>

#include "plan_internal.h"
#include "unet_ops.h"

namespace hdf_internal {

// A non-blocking stream at the highest / lowest priority the device offers (an unprioritised one where priorities are not
// to be had); nullptr: no stream.  The plan's branch (highest) and side (lowest) streams.
inline hipStream_t make_stream(bool highest) {
  hipStream_t s = nullptr;
  int least = 0, greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess ||
      hipStreamCreateWithPriority(&s, hipStreamNonBlocking, highest ? greatest : least) != hipSuccess) {
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) s = nullptr;
  }
  return s;
}

// Backward runs its weight gradients on the plan's side stream.  They are off the critical path (nothing in backward
// reads a weight gradient), MFMA-bound, and leave wave slots and 50 KB of LDS per CU free, while the chain they would
// otherwise delay is full of HBM-bound passes (InstanceNorm backward, pooling / up-sampling backward, heads): with both in
// flight the memory-bound kernels run under the matrix kernels (tools/overlap_probe.py: a 64->32 weight gradient plus
// three elementwise passes over 268 MB tensors take 708 us on two streams against 880 us back to back).  Ordering:
//  * fork: the side stream waits for an event recorded on the main stream after the producers of the operands;
//  * a buffer a side-stream kernel still reads (the dy of a conv) is not overwritten: wait_readers() before its next
//    writer on the main stream (each level keeps two dy buffers so that the wait is normally already satisfied);
//  * join: the main stream waits for the side stream's last event at the end of every backward call, so at the ABI
//    boundary all work is ordered on the caller's stream as before.
// The shared weight-gradient workspace is only touched on the side stream (its kernels run in order).
struct Exec {
  hdf_plan* p;
  char* ws;
  const float* params;
  float* grads;
  int B;
  hipStream_t st;
  int conv_budget = 0;                          // ConvArgs::cu_budget of the convolutions issued through this Exec (0: all)
  bool async = false;                           // weight gradients on the side stream
  bool on_branch = false;                       // this Exec issues onto the plan's branch stream (own scratch)
  hipEvent_t last_side = nullptr;               // last event recorded on the side stream in this call
  hipEvent_t tf_packed = nullptr;               // branch Exec: the persistent transformer kernel's weight copies are ready (forward3d)
  std::map<size_t, hipEvent_t> readers;         // workspace offset of a buffer -> side-stream event after its last reader
  hipEvent_t next_event() {
    if (p->events.size() < 256) {
      hipEvent_t ev = nullptr;
      if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return nullptr;
      p->events.push_back(ev);
      return ev;
    }
    return p->events[p->ev_next++ % p->events.size()];
  }
  // Stream ordering, all of it: a fresh ring event recorded on `from` that `to` waits for (wait = false: recorded only, for
  // a waiter that comes later).  Returns the event; nullptr: no event, or the record / the wait failed.  What that means
  // is the caller's decision: where it is an error (HDF_ERR_HIP) the caller names the `roles` for the message ("<waiting
  // stream> behind <recorded stream>"), where there is a fallback it does not.
  hipEvent_t order(hipStream_t from, hipStream_t to, const char* roles = nullptr, bool wait = true) {
    hipEvent_t ev = next_event();
    if (ev && hipEventRecord(ev, from) == hipSuccess && (!wait || hipStreamWaitEvent(to, ev, 0) == hipSuccess)) return ev;
    if (roles) hdf_set_error("stream ordering failed (event record / wait): %s", roles);
    return nullptr;
  }
  // `to` waits for an event recorded earlier
  int wait(hipStream_t to, hipEvent_t ev, const char* roles) {
    if (hipStreamWaitEvent(to, ev, 0) == hipSuccess) return HDF_OK;
    hdf_set_error("stream ordering failed (event wait): %s", roles);
    return HDF_ERR_HIP;
  }
  // stream for a weight-gradient launch whose operands are ready on the main stream now
  hipStream_t wgrad_stream() {
    if (!async) return st;
    if (!order(st, p->side)) {
      // fall back to in-order execution: first order this stream behind EVERYTHING the side stream holds -- the main and
      // the branch Exec both feed it and share the one weight-gradient workspace this stream is about to reuse, so this
      // Exec's own last_side is not enough.  A fresh event on the side stream, or, if events are what fails, a host wait.
      if (!order(p->side, st)) (void)hipStreamSynchronize(p->side);
      last_side = nullptr;
      readers.clear();
      async = false;
      return st;
    }
    return p->side;
  }
  // after the launch: remember that `buf` is read on the side stream until now
  // (an event that cannot be recorded would leave the launch outside every later join: a hard error, not a silent
  // loss of ordering)
  int wgrad_done(const View& buf) { return side_done(&buf); }
  // buf == nullptr: the same for a side-stream launch whose operands are never overwritten inside this call: only join()
  // waits for it
  int side_done(const View* buf = nullptr) {
    if (!async) return HDF_OK;
    hipEvent_t d = order(p->side, st, nullptr, false);
    if (!d) {
      (void)hipStreamSynchronize(p->side);
      hdf_set_error("backward: could not record the side stream's completion event");
      return HDF_ERR_HIP;
    }
    last_side = d;
    if (buf) readers[buf->off] = d;
    return HDF_OK;
  }
  void wait_readers(const View& buf) {
    auto it = readers.find(buf.off);
    if (it != readers.end()) {
      (void)hipStreamWaitEvent(st, it->second, 0);
      readers.erase(it);
    }
  }
  void join() {
    if (last_side) (void)hipStreamWaitEvent(st, last_side, 0);
    last_side = nullptr;
    readers.clear();
  }
  // scratch of this Exec's stream (two streams of one call must not share the per-launch partial-sum tables)
  float* statp() const { return f(on_branch ? p->stat_partials2 : p->stat_partials); }
  float* kspl() const { return f(on_branch ? p->ksplit_ws2 : p->ksplit_ws); }
  float* inbp() const { return f(on_branch ? p->inb_partials2 : p->inb_partials); }
  float* inbk() const { return f(on_branch ? p->inb_k2 : p->inb_k); }
  // fork: a second Exec on the plan's branch stream, ordered behind everything issued on this one so far.  nullptr
  // stream when the branch stream cannot be used (creation / event failure): the caller then stays in order.
  hipStream_t fork_branch() {
    if (!p->branch) p->branch = make_stream(true);  // the branch carries the longer dependency chain: highest priority
    if (!p->branch) return nullptr;
    return order(st, p->branch) ? p->branch : nullptr;
  }
  // join a branch Exec back: this stream waits for everything issued on the branch (incl. its side-stream work)
  int join_branch(Exec& b) {
    b.join();
    return order(b.st, st, "the forking stream behind the branch stream (join)") ? HDF_OK : HDF_ERR_HIP;
  }
  void* at(const View& v) const { return ws + v.off; }
  float* f(size_t off) const { return reinterpret_cast<float*>(ws + off); }
  // what the launchers of unet_ops.h take: a view's rows, a layer's InstanceNorm constants, C channels at a level's extent
  Rows rows(const View& v) const { return Rows{at(v), v.pitch}; }
  NormStatsOut norm(const Stats& s) const { return NormStatsOut{f(s.scale), f(s.shift), f(s.mean), f(s.rstd)}; }
  Extent extent(int lvl, int C) const { return Extent{B, C, dm(lvl)[0], dm(lvl)[1], dm(lvl)[2], p->flat ? 1 : 0}; }
  const float* P(int64_t off) const { return off < 0 ? nullptr : params + off; }
  float* G(int64_t off) const { return off < 0 ? nullptr : grads + off; }
  const int* dm(int lvl) const { return p->dims[lvl]; }
};

// Every return path of a forward / backward call (also the HDF_TRY error returns) orders the branch stream (while `forked`)
// and the side stream behind the caller's stream: the caller may free or reuse the workspace / gradient buffers as soon as
// its own stream gets there.  (A forward has nothing on the side stream: its e.join() issues nothing.)
struct Rejoin {
  Exec &e, &eb;
  bool forked;
  ~Rejoin() {
    if (forked) (void)e.join_branch(eb);
    e.join();
  }
};

// per-(n,c) input transform of a consumer: the producer's InstanceNorm scale/shift (+ReLU)
struct Xf {
  const float* scale = nullptr;
  const float* shift = nullptr;
  int relu = 0;
};
inline Xf xf_of(const Exec& e, const Conv3& c) { return Xf{e.f(c.st.scale), e.f(c.st.shift), 1}; }

// ---- exec_tf.hip: the multi-path transformer over a plan
TfDims tf_dims(const hdf_plan* p, int B);
bool tf_use_chain(const hdf_plan* p, int B);
int chain_flag_ensure(hdf_plan* p);
int chain_flag_check(hdf_plan* p);
int transformer_forward(Exec& e, const float* x);
int transformer_backward(Exec& e, const float* x);
// the last launch of a forward / of a backward whose persistent kernels ran (see chain_poison_outputs_kernel)
int chain_poison_outputs(Exec& e, void* const outs[4]);
int chain_poison_grads(Exec& e);

}  // namespace hdf_internal
