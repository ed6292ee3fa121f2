// What the three weight-gradient units (conv_wgrad.hip, conv_wgrad2.hip, conv_wgrad_s2.hip) share: the tile extents the
// host sizes grids and workspaces by, and the device pieces around ds_read_b64_tr_b16 and the partial slabs.
#pragma once
#include "conv_igemm.h"
#include "conv_tile.h"

namespace {

// Tile of the small operand per (stride, flat): the kernels of one stride share it, so the host derives the tile count,
// G and the workspace from this table alone.  conv_wgrad_kernel is instantiated from it; conv_wgrad2_kernel and
// conv_wgrad_s2_kernel, whose schedules are written for one tile, assert their row.
struct WgradTile {
  int td, th, tw;
};
constexpr WgradTile WGRAD_TILES[2][2] = {{{4, 8, 8}, {1, 16, 16}},   // stride 1: 3-D, flat (depth-1 operands)
                                         {{4, 4, 4}, {1, 8, 8}}};    // stride 2
constexpr bool wgrad_tile_is(int stride, int td, int th, int tw) {
  return WGRAD_TILES[stride - 1][0].td == td && WGRAD_TILES[stride - 1][0].th == th && WGRAD_TILES[stride - 1][0].tw == tw;
}

// Lane roles of ds_read_b64_tr_b16 (hardware transpose, 4 voxels x 16 channels per 16 lanes): group g4 = lane >> 4, within
// it i = lane & 15.  The lane addresses voxel q = i >> 2 of a 4-voxel group in half hh = g4 >> 1 of the 16 voxels of a k-step
// (k = 8 hh + 4 t + q), at byte column colb of the 32-channel row.
struct TrLane {
  int q, hh, colb;
  __device__ __forceinline__ explicit TrLane(int lane) {
    // (this statement order: with q, hh and colb formed last conv_wgrad2_kernel came out with other registers)
    const int g4 = lane >> 4, i16 = lane & 15;
    q = i16 >> 2;
    const int p4 = i16 & 3;
    hh = g4 >> 1;
    const int cb = (g4 & 1) * 16;
    colb = (cb + 4 * p4) * 2;
  }
};
__device__ __forceinline__ u32x2 tr_read(const char* lds_ptr) {
  using lds_s16x4 = s16x4 __attribute__((address_space(3)));
  s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)lds_ptr);
  return __builtin_bit_cast(u32x2, v);
}

// (kz, ky, kx) of a wave's tap slot.  Slots past the last tap (the last wave's dummy: uniform instruction stream, its
// accumulator is never stored) decode as tap 0.
__device__ __forceinline__ void wgrad_tap(int tap, int ntap, int& kz, int& ky, int& kx) {
  if (tap >= ntap) tap = 0;
  kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
}

// What stays written out, because sharing it changed the compiled kernels (tools/codeobj.py --diff against the build
// before): the partial-slab store of an accumulator, base[row(i) * LCp] = acc[i] with the MFMA row map (i & 3) + 8 (i >> 2)
// + 4 (lane >> 5), in all three kernels -- as a function, even as the row map alone, it is optimised before it is inlined
// and every kernel came out different; and TrLane / wgrad_tap in conv_wgrad_kernel, which keeps its own text of both.

}  // namespace
