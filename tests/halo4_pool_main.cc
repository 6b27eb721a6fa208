// Host-only probe of csrc/halo4_skip.h's row-split pooled order for tests/test_halo4_pool_skip_cpu.py.  Built with the host compiler alone (no HIP).
//   halo4_pool_main map W H y0     "E <eligible>"; for an eligible width one line per (wave-row, mi):
//                                  "B <wm> <mi> <block> <row> <top> <partner mi or -1> <first pooled row or -1>", then "N <wm> <dyi> <n>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "halo4_skip.h"

using namespace aocr;

// usable in constant expressions (the pooled epilogue needs them as template arguments and in if constexpr)
static_assert(halo4_pool_width(64) && halo4_pool_width(128) && !halo4_pool_width(32) && !halo4_pool_width(256), "eligible widths");
static_assert(halo4_pool_partner(64) == 1 && halo4_pool_partner(128) == 2, "partner offset");
static_assert(halo4_pool_top(0, 64) && !halo4_pool_top(1, 64) && halo4_pool_top(2, 64) && !halo4_pool_top(3, 64), "W = 64: tile rows 0 and 2 are upper rows");
static_assert(halo4_pool_top(0, 128) && halo4_pool_top(1, 128) && !halo4_pool_top(2, 128) && !halo4_pool_top(3, 128), "W = 128: tile row 0 is the upper row");
static_assert(halo4_pool_row(1, 2, 64) == 64 + 32 && halo4_pool_row(1, 1, 128) == 96, "pooled rows");

int main(int argc, char** argv) {
  if (argc == 5 && !std::strcmp(argv[1], "map")) {
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), y0 = std::atoi(argv[4]);
    const bool ok = halo4_pool_width(W);
    std::printf("E %d\n", ok ? 1 : 0);
    if (!ok) return 0;
    for (int wm = 0; wm < 2; ++wm)
      for (int mi = 0; mi < 4; ++mi) {
        const int blk = halo4_block(true, wm, mi);
        const bool top = halo4_pool_top(mi, W);
        std::printf("B %d %d %d %d %d %d %d\n", wm, mi, blk, halo4_block_row(blk, W, y0), top ? 1 : 0, top ? mi + halo4_pool_partner(W) : -1, top ? halo4_pool_row(wm, mi, W) : -1);
      }
    for (int wm = 0; wm < 2; ++wm)
      for (int dyi = 0; dyi < 3; ++dyi) std::printf("N %d %d %d\n", wm, dyi, halo4_ndead(wm, dyi, W, H, y0));
    return 0;
  }
  std::fprintf(stderr, "usage: halo4_pool_main map W H y0\n");
  return 2;
}
