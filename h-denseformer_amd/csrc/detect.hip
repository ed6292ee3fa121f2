// Lesion candidates from a fp32 probability map [D][H][W]: what a user does today with a copy of the map to the host and
// one scipy.ndimage.label per round (the reference has no such code).  Definitions and the protocol: include/hdf.h.
//
//   detect_init_kernel     w = the sanitised copy of prob; det, idx, the table and the state cleared        (first_round == 0)
//   detect_resume_kernel   one thread: the state of an earlier call is there and stands at first_round      (first_round > 0)
// and per round
//   detect_peak_kernel     max over (bits of w << 32 | 0xFFFFFFFF - index): one 64-bit atomicMax a workgroup
//   detect_decide_kernel   one thread: m, a, thr and the finished reason formed once
//   detect_mask_kernel     mask = (double)w > thr as 0 / 1 bytes; zeros in a round that extracts nothing
//   (hdf_launch_cc_label on the mask: ids)
//   detect_select_kernel   size and touch of cur = the component of a
//   detect_commit_kernel   w = 0 over cur; a kept candidate also det = m and idx = its index
//   detect_finish_kernel   one thread: the table row, kept and round advanced, the peak key cleared, the result words
//
// The state is 256 bytes at the head of the workspace.  A launch with many workgroups only reads it, or only updates words
// by integer atomics that no workgroup of that launch reads (the peak key; size and touch); everything else is written by the
// one-thread kernels between them.  A round that extracts nothing (finished, or a call whose first_round does not fit) runs
// the same launches with nothing to do: its mask is all zeros, which is the cheapest input the labelling has.  Non-negative
// floats order as their bit patterns, so the peak is exact and the smallest index wins a tie.  Integer atomics only, no
// thread waits for another one, nothing waits on the host.
#include "detect.h"

#include "components.h"

namespace {
typedef unsigned long long u64;
constexpr uint32_t MAGIC = 0x44455431u;   // "DET1": the state was formed by detect_init_kernel

struct State {
  u64 key;             // the peak of this round; 0 between rounds
  u64 size;            // voxels of cur
  u64 cc_result[2];    // the labelling's own result words (not used)
  double thr;
  uint32_t m_bits, a;
  uint32_t touch;      // some voxel of cur has an indexed voxel in its 3x3x3 neighbourhood
  uint32_t active;     // this round extracts a candidate
  uint32_t finished;   // 0 running, 1 count, 2 stop
  uint32_t mismatch;   // this call's first_round is not the rounds run so far (or there is no state)
  uint32_t kept, round, dropped, magic;
};
static_assert(sizeof(State) <= HDF_DETECT_STATE_BYTES, "the state fits its part of the workspace");

__device__ __forceinline__ int status_of(const State* st, int remove_adjacent, long long min_voxels) {
  if (remove_adjacent && st->touch) return 1;
  if ((long long)st->size < min_voxels) return 2;
  return 0;
}

__global__ __launch_bounds__(256) void detect_init_kernel(const float* __restrict__ prob, int64_t V, float* __restrict__ w,
                                                          float* __restrict__ det, int32_t* __restrict__ idx,
                                                          long long* __restrict__ table, int64_t table_words, State* st) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += stride) {
    const uint32_t bits = __float_as_uint(prob[v]);   // 0 < p <= FLT_MAX: the sign clear, not zero, not inf, not NaN
    w[v] = __uint_as_float(bits >= 1u && bits <= 0x7F7FFFFFu ? bits : 0u);
    det[v] = 0.f, idx[v] = 0;
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < table_words; i += stride) table[i] = 0;
  if (blockIdx.x == 0 && threadIdx.x < HDF_DETECT_STATE_BYTES / 4) {
    ((uint32_t*)st)[threadIdx.x] = threadIdx.x == offsetof(State, magic) / 4 ? MAGIC : 0u;
  }
}

__global__ void detect_resume_kernel(State* st, uint32_t first_round) {
  if (threadIdx.x == 0) st->mismatch = st->magic != MAGIC || st->round != first_round;
}

__global__ __launch_bounds__(256) void detect_peak_kernel(const float* __restrict__ w, int64_t V, State* st) {
  __shared__ u64 red[4];
  if (st->finished || st->mismatch) return;   // (one value for every workgroup: nobody writes these words here)
  u64 best = 0;   // below every key: a key's low word is at least 0xFFFFFFFF - 2^31
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256)
    best = max(best, ((u64)__float_as_uint(w[v]) << 32) | (0xFFFFFFFFu - (uint32_t)v));
  best = wave_max_u64(best);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(&st->key, max(max(red[0], red[1]), max(red[2], red[3])));
}

__global__ void detect_decide_kernel(State* st, int64_t V, int num_lesions, double factor, double stop) {
  if (threadIdx.x != 0) return;
  st->active = 0;
  if (st->finished || st->mismatch) return;
  if (st->kept == (uint32_t)num_lesions) {
    st->finished = 1;
    return;
  }
  const u64 key = st->key;
  const uint32_t m_bits = (uint32_t)(key >> 32), a = 0xFFFFFFFFu - (uint32_t)key;
  const double m = (double)__uint_as_float(m_bits);
  if (m < stop) {
    st->finished = 2;
    return;
  }
  if ((int64_t)a >= V) {   // (cannot happen with a state of this volume)
    st->mismatch = 1;
    return;
  }
  st->m_bits = m_bits, st->a = a, st->thr = m / factor;
  st->size = 0, st->touch = 0, st->active = 1;
}

__global__ __launch_bounds__(256) void detect_mask_kernel(const float* __restrict__ w, int64_t V, const State* st,
                                                          uint8_t* __restrict__ mask) {
  const bool active = st->active != 0;
  const double thr = st->thr;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256)
    mask[v] = active && (double)w[v] > thr ? 1 : 0;
}

__global__ __launch_bounds__(256) void detect_select_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ idx,
                                                            int D, int H, int W, State* st) {
  if (!st->active) return;   // (one value for every workgroup)
  const int64_t V = (int64_t)D * H * W;
  const int32_t target = ids[st->a];
  uint32_t cnt = 0;
  bool touch = false;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
    if (target <= 0 || ids[v] != target) continue;
    cnt++;
    if (touch) continue;
    const int x = (int)(v % W), y = (int)(v / W % H), z = (int)(v / ((int64_t)W * H));
    for (int zz = max(z - 1, 0); zz <= min(z + 1, D - 1); zz++)
      for (int yy = max(y - 1, 0); yy <= min(y + 1, H - 1); yy++)
        for (int xx = max(x - 1, 0); xx <= min(x + 1, W - 1); xx++) touch |= idx[((int64_t)zz * H + yy) * W + xx] > 0;
  }
  block_add_counts({cnt}, &st->size);
  if (__syncthreads_or(touch) && threadIdx.x == 0) atomicOr(&st->touch, 1u);
}

__global__ __launch_bounds__(256) void detect_commit_kernel(const int32_t* __restrict__ ids, int64_t V, const State* st,
                                                            int remove_adjacent, long long min_voxels, float* __restrict__ w,
                                                            float* __restrict__ det, int32_t* __restrict__ idx) {
  if (!st->active) return;
  const int32_t target = ids[st->a];
  if (target <= 0) return;
  const bool keep = status_of(st, remove_adjacent, min_voxels) == 0;
  const float m = __uint_as_float(st->m_bits);
  const int32_t index = (int32_t)st->kept + 1;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (int64_t)gridDim.x * 256) {
    if (ids[v] != target) continue;
    w[v] = 0.f;
    if (keep) det[v] = m, idx[v] = index;
  }
}

__global__ void detect_finish_kernel(State* st, int remove_adjacent, long long min_voxels, long long* __restrict__ table,
                                     long long table_rows, u64* __restrict__ result) {
  if (threadIdx.x != 0) return;
  if (st->active) {
    const int status = status_of(st, remove_adjacent, min_voxels);
    if (status == 0) st->kept++;
    if ((long long)st->round < table_rows) {
      long long* row = table + (long long)st->round * HDF_DETECT_TABLE_COLS;
      row[0] = status == 0 ? st->kept : 0, row[1] = st->m_bits, row[2] = (long long)st->size, row[3] = st->a, row[4] = status;
      row[5] = __double_as_longlong(st->thr);
    } else {
      st->dropped++;
    }
    st->round++;
  }
  st->key = 0;
  result[0] = st->round, result[1] = st->kept, result[2] = st->mismatch ? 3 : st->finished, result[3] = st->dropped;
}

struct Carve {
  int64_t state, w, mask, ids, cc, total;
  Carve(int D, int H, int W) {
    const int64_t V = (int64_t)D * H * W;
    Carver c;
    state = c.take(HDF_DETECT_STATE_BYTES);
    w = c.take(V * 4);
    mask = c.take(V);
    ids = c.take(V * 4);
    cc = c.take(hdf_cc_ws_bytes(D, H, W));
    total = c.at;
  }
};
}  // namespace

int64_t hdf_detect_ws_bytes(int D, int H, int W) { return Carve(D, H, W).total; }

int hdf_launch_detect(const float* prob, int D, int H, int W, const DetectArgs& p, float* det, int32_t* idx, long long* table,
                      unsigned long long* result, void* ws, hipStream_t stream) {
  const Carve cv(D, H, W);
  const int64_t V = (int64_t)D * H * W, table_words = p.table_rows * HDF_DETECT_TABLE_COLS;
  char* base = (char*)ws;
  State* st = (State*)(base + cv.state);
  float* w = (float*)(base + cv.w);
  uint8_t* mask = (uint8_t*)(base + cv.mask);
  int32_t* ids = (int32_t*)(base + cv.ids);
  const unsigned gv = vol_grid(V, HDF_DETECT_GRID_CAP);
  if (p.first_round == 0) {
    hipLaunchKernelGGL(detect_init_kernel, dim3(vol_grid(std::max(V, table_words), HDF_DETECT_GRID_CAP)), dim3(256), 0, stream,
                       prob, V, w, det, idx, table, table_words, st);
  } else {
    hipLaunchKernelGGL(detect_resume_kernel, dim3(1), dim3(64), 0, stream, st, (uint32_t)p.first_round);
  }
  HDF_LAUNCH_CHECK();
  for (int r = 0; r < p.rounds; r++) {
    hipLaunchKernelGGL(detect_peak_kernel, dim3(gv), dim3(256), 0, stream, (const float*)w, V, st);
    HDF_LAUNCH_CHECK();
    hipLaunchKernelGGL(detect_decide_kernel, dim3(1), dim3(64), 0, stream, st, V, p.num_lesions, p.factor, p.stop);
    HDF_LAUNCH_CHECK();
    hipLaunchKernelGGL(detect_mask_kernel, dim3(gv), dim3(256), 0, stream, (const float*)w, V, (const State*)st, mask);
    HDF_LAUNCH_CHECK();
    HDF_TRY(hdf_launch_cc_label(mask, 1, p.connectivity, D, H, W, ids, st->cc_result, base + cv.cc, stream));
    hipLaunchKernelGGL(detect_select_kernel, dim3(gv), dim3(256), 0, stream, (const int32_t*)ids, (const int32_t*)idx, D, H, W,
                       st);
    HDF_LAUNCH_CHECK();
    hipLaunchKernelGGL(detect_commit_kernel, dim3(gv), dim3(256), 0, stream, (const int32_t*)ids, V, (const State*)st,
                       p.remove_adjacent, (long long)p.min_voxels, w, det, idx);
    HDF_LAUNCH_CHECK();
    hipLaunchKernelGGL(detect_finish_kernel, dim3(1), dim3(64), 0, stream, st, p.remove_adjacent, (long long)p.min_voxels, table,
                       (long long)p.table_rows, (u64*)result);
    HDF_LAUNCH_CHECK();
  }
  return HDF_OK;
}
