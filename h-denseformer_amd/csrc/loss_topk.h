// TopKLoss (loss_topk.hip): per-voxel weighted cross-entropy, an exact top-K select over it, and the gradient on the
// selected voxels.  The C entries (hdf_loss_topk_*, hdf_op_topk_select) are defined in that unit.
#pragma once
#include "../../include/hdf.h"
#include "loss.h"

// bytes of the select's own state at the head of every top-k workspace: three radix histograms, the decided prefix, the
// per-block counts, offsets and fp64 partial sums (HDF_TOPK_SELECT_WORKSPACE_BYTES of include/hdf.h)
constexpr int64_t HDF_TOPK_SELECT_WS = 65536;
static_assert(HDF_TOPK_SELECT_WS == HDF_TOPK_SELECT_WORKSPACE_BYTES, "include/hdf.h");
