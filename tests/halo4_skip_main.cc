// Host-only probe of csrc/halo4_skip.h for tests/test_halo4_skip_cpu.py.  Built with the host compiler alone (no HIP).
//   halo4_skip_main map W H y0          one line per (wave-row, mi) of both ownerships, then the dead counts of the interleaved one:
//                                       "B <interleaved> <wm> <mi> <block> <row> <dead dyi=0> <dead dyi=2>"  /  "N <wm> <dyi> <n>"
//   halo4_skip_main plan lo hi rlo rhi halo    "P <nm> <no>" and one "O <k> <code> <at>" per op of the shortened half-step
//   halo4_skip_main taps                "T <sgn> <tap> <dyi>" for both signs and the nine taps
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "halo4_skip.h"

using namespace aocr;

// the helpers are usable in constant expressions (the kernel needs them as template arguments)
static_assert(halo4_block(true, 1, 2) == 5 && halo4_block(false, 1, 2) == 6, "ownership");
static_assert(halo4_ndead(0, 0, 64, 4, 0) == 1 && halo4_ndead(1, 2, 64, 4, 0) == 1 && halo4_ndead(0, 1, 64, 4, 0) == 0, "4 x 64 map");
static_assert(halo4_nops(1, 4, true) == 10 && halo4_op(0, 1, 4, true) == 4 && halo4_op_at(9, 12, 10) == 10, "plan");

int main(int argc, char** argv) {
  if (argc == 5 && !std::strcmp(argv[1], "map")) {
    const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), y0 = std::atoi(argv[4]);
    for (int il = 0; il < 2; ++il)
      for (int wm = 0; wm < 2; ++wm)
        for (int mi = 0; mi < 4; ++mi) {
          const int blk = halo4_block(il != 0, wm, mi);
          std::printf("B %d %d %d %d %d %d %d\n", il, wm, mi, blk, halo4_block_row(blk, W, y0), halo4_dead(blk, 0, W, H, y0) ? 1 : 0, halo4_dead(blk, 2, W, H, y0) ? 1 : 0);
        }
    for (int wm = 0; wm < 2; ++wm)
      for (int dyi = 0; dyi < 3; ++dyi) std::printf("N %d %d %d\n", wm, dyi, halo4_ndead(wm, dyi, W, H, y0));
    return 0;
  }
  if (argc == 7 && !std::strcmp(argv[1], "plan")) {
    const int lo = std::atoi(argv[2]), hi = std::atoi(argv[3]), rlo = std::atoi(argv[4]), rhi = std::atoi(argv[5]);
    const bool halo = std::atoi(argv[6]) != 0;
    const int nm = 4 * (hi - lo), no = halo4_nops(rlo, rhi, halo);
    std::printf("P %d %d\n", nm, no);
    for (int k = 0; k < no; ++k) std::printf("O %d %d %d\n", k, halo4_op(k, rlo, rhi, halo), halo4_op_at(k, nm, no));
    return 0;
  }
  if (argc == 2 && !std::strcmp(argv[1], "taps")) {
    for (int sgn = -1; sgn <= 1; sgn += 2)
      for (int tap = 0; tap < 9; ++tap) std::printf("T %d %d %d\n", sgn, tap, halo4_tap_dyi(sgn, tap));
    return 0;
  }
  std::fprintf(stderr, "usage: halo4_skip_main map W H y0 | plan lo hi rlo rhi halo | taps\n");
  return 2;
}
