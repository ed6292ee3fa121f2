// Host walk of the persistent conv kernels' tile schedule (csrc/conv_schedule.h, the only include of the project's):
// for every case, every workgroup of the launch is walked the way the kernels walk it and the properties the kernels rely
// on are checked.  Prints one line per failure (at most 20) and a last line "PASS <cases>" or "FAIL <failures>".
// Built and run by tests/test_cpu_tile_schedule.py.
#include <cstdio>
#include <vector>

#include "conv_schedule.h"

static int g_fail = 0;

static void fail(const char* what, int TD, int N, const int* nt, int gx, bool allowed, int bx, int k) {
  if (g_fail++ < 20)
    std::printf("%s: tile depth %d, N %d, grid %dx%dx%d, grid_x %d, interior_allowed %d, block_x %d, k %d\n", what, TD, N,
                nt[0], nt[1], nt[2], gx, (int)allowed, bx, k);
}

static bool same(const WsTile& a, const WsTile& b) {
  return a.n == b.n && a.z0 == b.z0 && a.y0 == b.y0 && a.x0 == b.x0 && a.tile == b.tile && a.k == b.k;
}

template <int TD, int TH, int TW>
static int walk_all() {
  const int grids[9][3] = {{1, 1, 1}, {3, 3, 3}, {12, 6, 6}, {12, 7, 7}, {3, 2, 5}, {4, 3, 3}, {6, 16, 16}, {32, 16, 16}, {5, 4, 9}};
  const int grid_xs[9] = {1, 5, 8, 16, 20, 24, 64, 128, 256};
  int cases = 0;
  for (int N = 1; N <= 3; N++)
    for (const auto& nt : grids)
      for (int gx : grid_xs)
        for (int al = 0; al < 2; al++) {
          const bool allowed = al != 0;
          cases++;
          const int ntz = nt[0], nty = nt[1], ntx = nt[2], total = N * ntz * nty * ntx;
          const bool want_int = allowed && ntz >= 3 && nty >= 3 && ntx >= 3;
          const int n_int = want_int ? N * (ntz - 2) * (nty - 2) * (ntx - 2) : 0;
          std::vector<int> seen(total, 0);
          int sum_int = 0, sum_bor = 0;
          for (int bx = 0; bx < gx; bx++) {
            const WsSchedule<TD, TH, TW> s(N, ntz, nty, ntx, allowed, gx, bx);
            if (s.has_int != want_int) fail("has_int", TD, N, nt, gx, allowed, bx, -1);
            if (s.int_cnt < 0 || s.bor_cnt < 0) fail("negative count", TD, N, nt, gx, allowed, bx, -1);
            sum_int += s.int_cnt, sum_bor += s.bor_cnt;
            // a produced tile: inside the launch, `tile` its raster index, in the pass it belongs to, not seen before
            auto visit = [&](const WsTile& c, bool interior_pass) {
              const int tz = c.z0 / TD, ty = c.y0 / TH, tx = c.x0 / TW;
              if (c.z0 % TD || c.y0 % TH || c.x0 % TW || c.n < 0 || c.n >= N || tz < 0 || tz >= ntz || ty < 0 || ty >= nty ||
                  tx < 0 || tx >= ntx) {
                fail("tile outside the launch", TD, N, nt, gx, allowed, bx, c.k);
                return;
              }
              const int lin = ((c.n * ntz + tz) * nty + ty) * ntx + tx;
              if (c.tile != lin || s.tile_lin(c) != lin) fail("tile is not the raster index", TD, N, nt, gx, allowed, bx, c.k);
              const bool inner = tz >= 1 && tz < ntz - 1 && ty >= 1 && ty < nty - 1 && tx >= 1 && tx < ntx - 1;
              // (without an interior pass the border pass is the whole raster and holds the inner tiles too)
              if (interior_pass ? !inner : (want_int && inner)) fail("tile in the wrong pass", TD, N, nt, gx, allowed, bx, c.k);
              if (c.k < 0 || c.k >= (interior_pass ? n_int : total - n_int)) fail("list index out of range", TD, N, nt, gx, allowed, bx, c.k);
              seen[lin]++;
            };
            WsTile c, d;
            for (int i = 0; i < s.int_cnt; i++) {
              if (i == 0)
                s.int_init(c, s.int_begin);
              else
                s.int_next(c);
              s.int_init(d, s.int_begin + i * s.WPX);
              if (!same(c, d)) fail("int_next != int_init(k + WPX)", TD, N, nt, gx, allowed, bx, d.k);
              visit(c, true);
            }
            for (int i = 0; i < s.bor_cnt; i++) {
              if (i == 0)
                s.bor_init(c, s.bor_begin);
              else
                s.bor_next(c);
              s.bor_init(d, s.bor_begin + i * s.WPX);
              if (!same(c, d)) fail("bor_next != bor_init(k + WPX)", TD, N, nt, gx, allowed, bx, d.k);
              visit(c, false);
            }
          }
          if (sum_int != n_int || sum_bor != total - n_int) fail("counts do not add up to the lists", TD, N, nt, gx, allowed, -1, -1);
          for (int t = 0; t < total; t++)
            if (seen[t] != 1) {
              fail(seen[t] ? "tile produced more than once" : "tile never produced", TD, N, nt, gx, allowed, -1, t);
              break;
            }
        }
  return cases;
}

int main() {
  const int cases = walk_all<4, 8, 8>() + walk_all<8, 8, 8>();
  if (g_fail)
    std::printf("FAIL %d\n", g_fail);
  else
    std::printf("PASS %d\n", cases);
  return g_fail ? 1 : 0;
}
