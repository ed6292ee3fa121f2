// The tile schedule of the persistent 3-D convolution kernels: which TD x TH x TW output tiles a workgroup computes, and in
// which order.  conv_wgrad2_kernel and conv_wr_kernel use it; conv_ws2_kernel (conv_igemm.hip) carries the same schedule
// as a copy of its own (reason there).  Pure integer code without a HIP dependency: a host compiler can include this
// header and walk the schedule (tests/tile_schedule_walk.cpp does).
//
// Two passes per workgroup.  Every workgroup first runs its share of the INTERIOR tiles (1 <= t < nt - 1 on all three
// axes: the halo box lies inside the volume, so the kernel's unchecked copy of the tile phase runs them in one long run),
// then its share of the BORDER tiles with the checked copy.  Walking all tiles in raster order switched between the two
// copies at every x-row (two border tiles per 16), and each switch re-fetched cold code and drained the staging pipeline.
// A kernel may forbid the interior pass (interior_allowed = false: ragged channels, an accumulating epilogue); then every
// tile is a border tile, in raster order.
//
// XCD-aware split of both lists.  Workgroup b runs on XCD b % 8 (round-robin dispatch), and each XCD has its own 4 MiB L2.
// XCD x owns the x-th eighth of the raster-ordered list and its WPX = grid_x / 8 workgroups walk that range interleaved
// (tile r0 + slot, + WPX, ...): at any moment the XCD works on ~WPX consecutive tiles, so the halo planes neighbouring
// tiles share are fetched from HBM once and hit in that L2 (a contiguous chunk per workgroup re-fetched them: FETCH_SIZE
// 2.8x the input).  A grid that is no multiple of 8 is one range walked with stride grid_x.
//
// Interior tiles advance incrementally: the stride WPX is held as mixed-radix digits over the interior grid (x, y, z, n)
// and int_next adds them with carries.  Border tiles are re-decoded from their list index (a few integer divisions per
// tile of the checked path, which is the short one).
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define WS_SCHED_FN __device__ __forceinline__
#else
#define WS_SCHED_FN inline
#endif

namespace {

// one output tile: sample, first output voxel, raster index ((n ntz + tz) nty + ty) ntx + tx (no kernel reads it today: the
// statistics rows are per workgroup; it is filled for the host walk and for schedules that claim tiles dynamically), and
// its index in the list (interior or border) it came from
struct WsTile {
  int n, z0, y0, x0, tile;
  int k;
};

constexpr int ws_log2(int v) { return v <= 1 ? 0 : 1 + ws_log2(v >> 1); }

// A bag of plain ints, held BY VALUE in the kernel (passed by reference, a struct of this kind once pushed conv_wr_kernel's
// staging state into scratch memory).
template <int TD, int TH, int TW>
struct WsSchedule {
  static_assert(TD > 0 && TH > 0 && TW > 0 && (TD & (TD - 1)) == 0 && (TH & (TH - 1)) == 0 && (TW & (TW - 1)) == 0,
                "tile extents are powers of two: tile index = coordinate >> log2");
  static constexpr int LD = ws_log2(TD), LH = ws_log2(TH), LW = ws_log2(TW);

  int ntz, nty, ntx;                            // tile grid of a sample
  bool has_int;                                 // the launch has an interior pass
  int ipz, ipy, ipx;                            // interior tile grid of a sample (meaningful with has_int)
  int per_bor;                                  // border tiles per sample
  int WPX;                                      // workgroups per range = stride of a workgroup inside its range
  int int_begin, int_cnt, bor_begin, bor_cnt;   // this workgroup's first list index and tile count, per pass
  int sdx, sdy, sdz, sdn;                       // mixed-radix digits of WPX over the interior grid

  WS_SCHED_FN WsSchedule(int N, int ntz_, int nty_, int ntx_, bool interior_allowed, int grid_x, int block_x)
      : ntz(ntz_), nty(nty_), ntx(ntx_) {
    has_int = interior_allowed && ntz >= 3 && nty >= 3 && ntx >= 3;
    ipz = ntz - 2, ipy = nty - 2, ipx = ntx - 2;
    const int n_int = has_int ? N * ipz * ipy * ipx : 0;
    per_bor = ntz * nty * ntx - (has_int ? ipz * ipy * ipx : 0);
    const int n_bor = N * per_bor;
    const int NX = (grid_x % 8 == 0) ? 8 : 1;  // ranges
    WPX = grid_x / NX;
    const unsigned xcd = (unsigned)block_x % (unsigned)NX, slot = (unsigned)block_x / (unsigned)NX;
    split(n_int, xcd, slot, NX, int_begin, int_cnt);
    split(n_bor, xcd, slot, NX, bor_begin, bor_cnt);
    sdx = sdy = sdz = sdn = 0;
    if (has_int) {
      int t = WPX;
      sdx = t % ipx, t /= ipx;
      sdy = t % ipy, t /= ipy;
      sdz = t % ipz, sdn = t / ipz;
    }
  }

  // range xcd of `total` list entries, walked from `slot` with stride WPX (nothing here is negative: unsigned divides)
  WS_SCHED_FN void split(int total, unsigned xcd, unsigned slot, int NX, int& begin, int& cnt) const {
    const int r0 = (int)((long long)total * xcd / NX), r1 = (int)((long long)total * (xcd + 1) / NX);
    const unsigned len = (unsigned)(r1 - r0);
    begin = (int)(r0 + slot);
    cnt = (len > slot) ? (int)((len - slot + (unsigned)WPX - 1) / (unsigned)WPX) : 0;
  }

  WS_SCHED_FN int tile_lin(const WsTile& c) const {
    return ((c.n * ntz + (c.z0 >> LD)) * nty + (c.y0 >> LH)) * ntx + (c.x0 >> LW);
  }

  // k-th interior tile, in raster order of the interior grid
  WS_SCHED_FN void int_init(WsTile& c, int k) const {
    int t = k;
    c.k = k;
    c.x0 = (t % ipx + 1) * TW;
    t /= ipx;
    c.y0 = (t % ipy + 1) * TH;
    t /= ipy;
    c.z0 = (t % ipz + 1) * TD;
    c.n = t / ipz;
    c.tile = tile_lin(c);
  }
  // + WPX tiles in raster order of the interior grid
  WS_SCHED_FN void int_next(WsTile& c) const {
    int xi = (c.x0 >> LW) - 1 + sdx, yi = (c.y0 >> LH) - 1 + sdy, zi = (c.z0 >> LD) - 1 + sdz;
    c.k += WPX;
    c.n += sdn;
    if (xi >= ipx) xi -= ipx, yi++;
    if (yi >= ipy) yi -= ipy, zi++;
    if (zi >= ipz) zi -= ipz, c.n++;
    c.x0 = (xi + 1) * TW, c.y0 = (yi + 1) * TH, c.z0 = (zi + 1) * TD;
    c.tile = tile_lin(c);
  }
  // k-th border tile.  With an interior pass the list of a sample is: the whole plane tz = 0, then per inner plane its
  // rim (row ty = 0, the two end tiles of each inner row, row ty = nty - 1), then the whole plane tz = ntz - 1.
  WS_SCHED_FN void bor_init(WsTile& c, int k) const {
    int tz, ty, tx;
    c.k = k;
    c.n = k / per_bor;
    int rem = k - c.n * per_bor;
    if (!has_int) {
      tx = rem % ntx, ty = (rem / ntx) % nty, tz = rem / (ntx * nty);
    } else {
      const int plane = nty * ntx, ring = plane - ipy * ipx;  // border tiles of a z-plane: all of it / its rim
      if (rem < plane) {
        tz = 0, ty = rem / ntx, tx = rem % ntx;
      } else if (rem - plane < ipz * ring) {
        rem -= plane;
        tz = 1 + rem / ring;
        rem %= ring;
        if (rem < ntx) {
          ty = 0, tx = rem;
        } else if (rem - ntx < 2 * ipy) {
          rem -= ntx;
          ty = 1 + (rem >> 1), tx = (rem & 1) ? ntx - 1 : 0;
        } else {
          ty = nty - 1, tx = rem - ntx - 2 * ipy;
        }
      } else {
        rem -= plane + ipz * ring;
        tz = ntz - 1, ty = rem / ntx, tx = rem % ntx;
      }
    }
    c.z0 = tz * TD, c.y0 = ty * TH, c.x0 = tx * TW;
    c.tile = tile_lin(c);
  }
  WS_SCHED_FN void bor_next(WsTile& c) const { bor_init(c, c.k + WPX); }
};

}  // namespace

#undef WS_SCHED_FN
