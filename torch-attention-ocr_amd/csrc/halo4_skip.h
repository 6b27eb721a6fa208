// halo4_skip.h -- which 32-pixel blocks of a 256-pixel tile a wave of gemm_halo4_bf16_kernel holds, which of them multiply nothing but the
// zero padding above / below the map in a given kernel row, and where the fragment reads and LDS-DMA pieces of a shortened half-step sit
// between the MFMAs that remain.  Plain constexpr C++17 without any device code: mfma_gemm.h uses it inside the kernel, and a host
// compiler builds it alone (tests/halo4_skip_main.cc checks it against an enumeration of the pixels).
//
// The tile is 256 consecutive pixels in plain order (LoadConvK::pmode == 0) of a map of H rows of W pixels, W % 32 == 0 and 256 % W == 0:
// eight blocks of 32 pixels, each inside one map row, the tile whole rows of one image, y0 the map row of its first pixel.
// Four waves as 2 (wave-row wm) x 2; a wave-row holds four blocks, accumulators mi = 0..3.
//   contiguous  (the kernel's first form):  block 4 wm + mi  -- wave-row 0 has the upper half of the tile, wave-row 1 the lower
//   interleaved (SKIP):                     block 2 mi + wm  -- both wave-rows have a part of every pair of blocks, so the first map row's
//                                           blocks (dead in kernel row dy = -1) and the last one's (dy = +1) are shared evenly
// dyi = dy + 1 is the halo row offset of a tap: forward kh, data gradient 2 - kh.
//
// The (2,1)-pooled layers (pmode == 2: the launch's rows are ordered in window pairs, row 2 j of the map beside row 2 j + 1) take SKIP too, with the
// ROW-SPLIT order inside the tile: the tile is the same 256 / W whole map rows, y0 its first, and a lane addresses its pixels in plain order exactly as
// above, so the blocks, their rows and the dead counts are those of the interleaved ownership.  What changes is where a pool window's two values sit:
// not in neighbouring accumulator entries of one lane but in the same entry of acc[mi] (map row 2 j) and acc[mi + W / 64] (row 2 j + 1: the same x
// range, so the same wave-row and lane), which needs W >= 64 -- at W = 32 the partner block 2 mi + wm + 1 belongs to the other wave-row.
#pragma once

namespace aocr {

constexpr int halo4_block(bool interleaved, int wm, int mi) { return interleaved ? 2 * mi + wm : 4 * wm + mi; }
constexpr int halo4_block_row(int blk, int W, int y0) { return y0 + (blk * 32) / W; }
constexpr int halo4_tap_dyi(int sgn, int tap) { return sgn > 0 ? tap / 3 : 2 - tap / 3; }
// the block's 32 x 32 products of halo row offset dyi are all (pixel of the padding row) x weight
constexpr bool halo4_dead(int blk, int dyi, int W, int H, int y0) {
  return (dyi == 0 && halo4_block_row(blk, W, y0) == 0) || (dyi == 2 && halo4_block_row(blk, W, y0) == H - 1);
}
// dead blocks of interleaved wave-row wm at halo row offset dyi.  Rows do not decrease with mi, so they are mi = 0 .. n-1 for dyi == 0
// and mi = 4-n .. 3 for dyi == 2; n <= 2 for W <= 128.
constexpr int halo4_ndead(int wm, int dyi, int W, int H, int y0) {
  int n = 0;
  for (int mi = 0; mi < 4; ++mi) n += halo4_dead(halo4_block(true, wm, mi), dyi, W, H, y0) ? 1 : 0;
  return n;
}

// ---- the row-split pooled order (interleaved ownership, W = 64 or 128)
constexpr bool halo4_pool_width(int W) { return W == 64 || W == 128; }
// acc[mi + halo4_pool_partner(W)] is the block one map row below acc[mi]'s: W / 32 blocks further on, two blocks per mi
constexpr int halo4_pool_partner(int W) { return W / 64; }
// acc[mi] is the upper row of its pool window (the tile's rows are whole windows: 256 / W is even and y0 with it); the same for both wave-rows
constexpr bool halo4_pool_top(int mi, int W) { return ((2 * mi * 32 / W) & 1) == 0; }
// first of the 32 pooled rows (of the tile's 128: window row * W + x) that the pair (acc[mi], acc[mi + partner]) of wave-row wm leaves
constexpr int halo4_pool_row(int wm, int mi, int W) { return (halo4_block(true, wm, mi) * 32 / W >> 1) * W + halo4_block(true, wm, mi) * 32 % W; }

// ---- a half-step with the live accumulators mi = lo .. hi-1: its MFMAs are j = 0 .. 4 (hi - lo) - 1 (mi = lo + j / 4, ni = j % 4).
// Between them go, in the order of the full half-step: per mi the A read of mi (only rlo <= mi < rhi: a dead block's fragment is not
// read), the B read number mi, and the DMA piece anchored at mi (weight pieces at mi = 0 and 1, the halo piece, if any, at mi = 2).
// Codes: 0..3 A read of mi, 4..7 B read, 8..9 weight piece, 12 the halo piece.  The DMA pieces keep their count and their order, which
// the kernel's vmcnt arithmetic depends on.
constexpr int halo4_nops(int rlo, int rhi, bool halo) { return (rhi - rlo) + 6 + (halo ? 1 : 0); }
constexpr int halo4_op(int k, int rlo, int rhi, bool halo) {
  int n = 0;
  for (int mi = 0; mi < 4; ++mi) {
    if (mi >= rlo && mi < rhi) { if (n == k) return mi; ++n; }
    if (n == k) return 4 + mi; ++n;
    if (mi < 2) { if (n == k) return 8 + mi; ++n; }
    if (mi == 2 && halo) { if (n == k) return 12; ++n; }
  }
  return -1;
}
// op k of `no` goes behind MFMA k nm / no of `nm`: spread evenly, the first behind MFMA 0, none behind the last (nm >= no: one per gap)
constexpr int halo4_op_at(int k, int nm, int no) { return k * nm / no; }

}  // namespace aocr
