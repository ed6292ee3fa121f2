// What the per-id table kernels share (components.hip: the component table and the filter's sizes; measure.hip: the
// region measurements; quantiles.hip: the order statistics): the runs of a wave, the walk of a workgroup, its LDS slots,
// the integer atomics on a row, the orderable key of a float and the layout of an id's box.
#pragma once
#include "wave_ops.h"

// ------------------------------------------------------------------------------------------------ keys and boxes
// a float's bits as an unsigned that orders like the value; -0 is +0
__device__ __forceinline__ uint32_t order_of(uint32_t bits) {
  if (bits == 0x80000000u) bits = 0u;
  return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t order) {
  return __uint_as_float((order >> 31) ? order ^ 0x80000000u : ~order);
}
// the box of an id as the walk of measure.hip leaves it: six maxima that start from 0
constexpr int CC_BOX_COLS = 6;   // BIG - zmin, zmax, BIG - ymin, ymax, BIG - xmin, xmax
constexpr int CC_BOX_BIG = 0x7fffffff;

// ------------------------------------------------------------------------------------------------ runs
// The lanes of a wave hold 64 consecutive voxels.  A run is a maximal stretch of lanes with the same non-zero id that
// does not cross a row start: its first lane (the head) speaks for all of it, one set of atomics instead of `len`.
// Returns the distance from this lane to the end of its stretch (for a head: the run's length).
__device__ __forceinline__ int wave_run(int id, bool row_start, bool* head) {
  const int lane = threadIdx.x & 63;
  const int prev = __shfl_up(id, 1, 64);
  *head = id > 0 && (lane == 0 || prev != id || row_start);
  return wave_run_len(__ballot(*head || id <= 0), lane);
}

#define CC_MIN(p, x) __hip_atomic_fetch_min((p), (long long)(x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define CC_MAX(p, x) __hip_atomic_fetch_max((p), (long long)(x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define CC_ADD(p, x) __hip_atomic_fetch_add((p), (x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// Runs of one component arrive by the thousand at the same table row (a tumour is one component of millions of voxels), and
// atomics on one address are served one at a time.  A workgroup therefore walks SPAN consecutive voxels and collects its
// runs in LDS first: SLOTS slots, slot id % SLOTS claimed by the first id that asks (compare-and-swap on the slot's id); a
// run whose slot belongs to another id goes to memory directly.  The slots are flushed once per workgroup.  Sums, minima
// and maxima of integers: the grouping changes no result.  HDF_CC_NO_LDS_SLOTS: A/B builds, every run straight to memory.
constexpr int SLOTS = 64, SPAN_TRIPS = 32, SPAN = 256 * SPAN_TRIPS;
__device__ __forceinline__ bool claim_slot(int* slot_id, int id) {
#ifdef HDF_CC_NO_LDS_SLOTS
  return false;
#else
  int owner = __hip_atomic_load(slot_id + (id & (SLOTS - 1)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (owner == 0) {
    owner = atomicCAS(slot_id + (id & (SLOTS - 1)), 0, id);
    if (owner == 0) owner = id;
  }
  return owner == id;
#endif
}
