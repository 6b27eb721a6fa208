// layout.hip -- page layout for multi-column pages (include/aocr.h: aocr_ink_integral, aocr_layout_blocks), the stage in front of
// aocr_segment_page: a summed-area table of the ink mask, then a recursive XY cut that reads every ink count from the table.  Integer
// arithmetic only (the Otsu threshold, when asked for, comes from segment.hip's otsu_threshold), so tests/layout_ref.py matches exactly.
//
// aocr_ink_integral.  The table is cut into tiles of SAT_ROWS rows (a row segment) x SAT_COLS columns (a column chunk).  What a tile needs
// from the rest of the page are two carries, both made from ink counts (1 byte read per pixel, small outputs), so that the table itself,
// 4 bytes per pixel, is written once and never read:
//   (Otsu only) otsu_threshold of segment.hip: memset, hist_kernel, otsu_kernel -- what aocr_segment_page enqueues for its steps 1-2.
//   sat_colcount_kernel  one thread per column and row segment: the ink of the column inside the segment (consecutive threads read
//                        consecutive bytes).
//   sat_rowcount_kernel  one wave per tile: the ink of each of its rows inside the chunk, with the tile loads of sat_tile_kernel.
//   sat_colscan_kernel   per column the exclusive prefix of the segment counts down the page, in place: the ink of the column above each
//                        segment.  A workgroup owns 64 columns x SCAN_GROUPS groups of segments; the groups' sums meet in LDS.
//   sat_tile_kernel      one wave per tile.  Top carry: S[y0][x+1] is the prefix over x of the column counts above the segment (a wave sum of
//                        the columns left of the chunk, then 16 wave prefixes), kept in 16 registers per lane, lane l owning the columns
//                        64k + l of the chunk.  Left carry of row y: the row counts of the chunks to its left, in lane y - y0.  Then row after
//                        row: the 16-byte load pattern of wave_row (page_common.h), cut to the chunk -- a chunk is 63 words wide, so the at most
//                        64 aligned words that cover it are one load per lane, a row whose word straddles the page's ends takes byte loads,
//                        and all SAT_ROWS loads are issued before the first is used -- a 16-bit ink mask per lane, a wave prefix of the
//                        popcounts, the row's prefix to LDS (padded by one word in 16: the lanes' 16-word runs start on distinct banks), and
//                        from there every lane adds its columns to its registers and stores them: consecutive lanes, consecutive words.
// No atomics (outside the Otsu histogram's integer ones); integer sums do not depend on their order: the table does not depend on the
// launch geometry.
//
// aocr_layout_blocks is ONE persistent workgroup of SEG_THREADS threads (DESIGN.md section 15 weighs it against a workgroup per region and a
// launch per level): the level list lives in scratch_dev as two arrays of max_blocks regions, the current level's and the next one's;
// regions are taken in list order, their profiles staged as flags in LDS, pieces found by find_runs (runs.h), children tightened and
// appended, so the list is in reading order by construction.  Every thread follows the same control flow; thread 0 writes the lists.
#include <algorithm>
#include "ops.h"
#include "page_common.h"
#include "runs.h"

namespace aocr {

namespace {

constexpr int SAT_ROWS = 8;                    // rows of a tile (a row segment): loads in flight per lane of sat_tile_kernel
constexpr int SAT_COLS = 1008;                 // columns of a tile (a column chunk): 63 16-byte words, so 64 aligned words cover it wherever it starts
constexpr int SAT_STAGE = SAT_COLS + SAT_COLS / 16 + 1;
constexpr int SCAN_GROUPS = 16;                // sat_colscan_kernel: groups of segments per workgroup of 64 columns
static_assert(SAT_COLS % 16 == 0 && SAT_COLS + 15 <= 64 * 16 && SAT_COLS <= 16 * 64, "a chunk is one aligned load and 16 stores per lane");

struct SatLayout {                             // byte offsets into scratch_dev
  size_t hist, hdr, cc, rc, total;
  int nseg, nch;
};

SatLayout sat_layout(int H, int W) {
  SatLayout l;
  ScratchCursor c;
  l.nseg = cdiv(H, SAT_ROWS);
  l.nch = cdiv(W, SAT_COLS);
  l.hist = c.take(256 * sizeof(uint32_t));
  l.hdr = c.take(4 * sizeof(int32_t));
  l.cc = c.take((size_t)l.nseg * W * sizeof(uint32_t));               // column counts per segment, then their prefix down the page
  l.rc = c.take((size_t)H * l.nch * sizeof(uint32_t));                // row counts per chunk
  l.total = c.total();
  return l;
}

// bit j: column xq + j of the row is ink and lies in [X0, X1); row + xq is 16-byte aligned; thr >= 0.  Every read is inside [0, W).
__device__ __forceinline__ uint32_t tile_mask(const uint8_t* __restrict__ row, int xq, int X0, int X1, int W, int thr, int light) {
  const int lo = max(X0 - xq, 0), hi = min(X1 - xq, 16);
  if (lo >= hi) return 0u;
  uint32_t m = 0;
  if (xq >= 0 && xq + 16 <= W) {                         // a whole aligned word inside the row
    m = ink_mask16(*reinterpret_cast<const uint4*>(row + xq), thr, light);
  } else {
    for (int j = lo; j < hi; ++j) m |= (uint32_t)is_ink(row[xq + j], thr, light) << j;       // X0 <= xq + j < X1 <= W
  }
  return m & ((1u << hi) - 1u) & ~((1u << lo) - 1u);
}

// the first column of lane `lane`'s word for the chunk that starts at column X0 of `row`
__device__ __forceinline__ int tile_word(const uint8_t* row, int X0, int lane) {
  return X0 - (int)((uintptr_t)(row + X0) & 15u) + 16 * lane;
}

__device__ __forceinline__ uint32_t wave_prefix_incl(uint32_t v, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  return v;
}

__global__ __launch_bounds__(256) void sat_colcount_kernel(const uint8_t* __restrict__ page, int64_t pitch, int H, int W, int light, int fixed,
                                                           const int32_t* __restrict__ hdr, uint32_t* __restrict__ cc) {
  const int thr = ink_thr(fixed, hdr);
  const int x = blockIdx.x * 256 + threadIdx.x, seg = blockIdx.y;
  if (x >= W) return;
  const int y0 = seg * SAT_ROWS, y1 = min(y0 + SAT_ROWS, H);
  const uint8_t* p = page + (int64_t)y0 * pitch + x;
  uint32_t c = 0;
  if (thr >= 0)
    for (int y = y0; y < y1; ++y, p += pitch) c += is_ink(*p, thr, light);
  cc[(size_t)seg * W + x] = c;
}

__global__ __launch_bounds__(256) void sat_rowcount_kernel(const uint8_t* __restrict__ page, int64_t pitch, int H, int W, int light, int fixed,
                                                           const int32_t* __restrict__ hdr, int nseg, int nch, uint32_t* __restrict__ rc) {
  const int lane = threadIdx.x & 63, seg = blockIdx.x * 4 + (threadIdx.x >> 6), chunk = blockIdx.y;
  if (seg >= nseg) return;
  const int thr = ink_thr(fixed, hdr);
  const int X0 = chunk * SAT_COLS, X1 = min(X0 + SAT_COLS, W), y0 = seg * SAT_ROWS;
  uint32_t m[SAT_ROWS];
#pragma unroll
  for (int r = 0; r < SAT_ROWS; ++r) {
    const uint8_t* row = page + (int64_t)min(y0 + r, H - 1) * pitch;
    m[r] = (y0 + r < H && thr >= 0) ? tile_mask(row, tile_word(row, X0, lane), X0, X1, W, thr, light) : 0u;
  }
#pragma unroll
  for (int r = 0; r < SAT_ROWS; ++r) {
    const uint32_t c = wave_sum((uint32_t)__popc(m[r]));
    if (lane == 0 && y0 + r < H) rc[(size_t)(y0 + r) * nch + chunk] = c;
  }
}

__global__ __launch_bounds__(64 * SCAN_GROUPS) void sat_colscan_kernel(uint32_t* __restrict__ cc, int W, int nseg) {
  __shared__ uint32_t part[SCAN_GROUPS][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int x = blockIdx.x * 64 + lane;
  const int per = (nseg + SCAN_GROUPS - 1) / SCAN_GROUPS;
  const int s0 = min(nseg, g * per), s1 = min(nseg, s0 + per);
  uint32_t sum = 0;
  if (x < W)
    for (int s = s0; s < s1; ++s) sum += cc[(size_t)s * W + x];
  part[g][lane] = sum;
  __syncthreads();
  uint32_t run = 0;
  for (int k = 0; k < g; ++k) run += part[k][lane];
  if (x < W)
    for (int s = s0; s < s1; ++s) {                      // exclusive: the ink of column x above segment s
      const uint32_t t = cc[(size_t)s * W + x];
      cc[(size_t)s * W + x] = run;
      run += t;
    }
}

__device__ __forceinline__ int stage_at(int c) { return c + (c >> 4); }

__global__ __launch_bounds__(256) void sat_tile_kernel(const uint8_t* __restrict__ page, int64_t pitch, int H, int W, int light, int fixed,
                                                       const int32_t* __restrict__ hdr, int nseg, int nch, const uint32_t* __restrict__ above,
                                                       const uint32_t* __restrict__ rc, uint32_t* __restrict__ S, int64_t sp,
                                                       int32_t* __restrict__ info) {
  __shared__ uint32_t stage[4][SAT_STAGE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int seg = blockIdx.x * 4 + wave, chunk = blockIdx.y;
  const bool live = seg < nseg;                          // every wave takes every barrier
  const int thr = ink_thr(fixed, hdr);
  const int X0 = chunk * SAT_COLS, X1 = min(X0 + SAT_COLS, W), y0 = seg * SAT_ROWS;
  const int nr = live ? min(SAT_ROWS, H - y0) : 0;
  uint32_t* st = stage[wave];
  uint32_t prev[16];                                     // S[y][X0 + 64k + lane + 1] of the row y above the one being written
  uint32_t rowc = 0;                                     // lane r: the ink of row y0 + r left of the chunk
#pragma unroll
  for (int k = 0; k < 16; ++k) prev[k] = 0;
  if (live) {
    const uint32_t* ca = above + (size_t)seg * W;
    uint32_t run = 0;
    for (int x = lane; x < X0; x += 64) run += ca[x];
    run = wave_sum(run);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int x = X0 + 64 * k + lane;
      const uint32_t inc = wave_prefix_incl(x < X1 ? ca[x] : 0u, lane);
      prev[k] = run + inc;
      run += __shfl(inc, 63);
    }
    if (lane < nr)
      for (int c = 0; c < chunk; ++c) rowc += rc[(size_t)(y0 + lane) * nch + c];
  }
  uint32_t m[SAT_ROWS];
  int xq[SAT_ROWS];
#pragma unroll
  for (int r = 0; r < SAT_ROWS; ++r) {
    const uint8_t* row = page + (int64_t)min(y0 + r, H - 1) * pitch;
    xq[r] = tile_word(row, X0, lane);
    m[r] = (r < nr && thr >= 0) ? tile_mask(row, xq[r], X0, X1, W, thr, light) : 0u;
  }
#pragma unroll
  for (int r = 0; r < SAT_ROWS; ++r) {
    if (r < nr) {                                        // the prefix of row y0 + r over [0, x], for the columns of this lane's word
      const uint32_t c = (uint32_t)__popc(m[r]);
      const uint32_t inc = wave_prefix_incl(c, lane);
      const uint32_t base = inc - c + __shfl(rowc, r);
      const int lo = max(X0 - xq[r], 0), hi = min(X1 - xq[r], 16);
      for (int j = lo; j < hi; ++j) st[stage_at(xq[r] + j - X0)] = base + (uint32_t)__popc(m[r] & ((2u << j) - 1u));
      const uint32_t tot = __shfl(inc, 63);
      if (lane == r) rowc += tot;
    }
    __syncthreads();
    if (r < nr) {
      uint32_t* out = S + (int64_t)(y0 + r + 1) * sp;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int c = 64 * k + lane;
        if (X0 + c < X1) {
          prev[k] += st[stage_at(c)];
          out[X0 + c + 1] = prev[k];
        }
      }
      if (X0 == 0 && lane == 0) out[0] = 0u;
    }
    __syncthreads();
  }
  if (!live) return;
  if (seg == 0) {                                        // row 0 of the table
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (X0 + 64 * k + lane < X1) S[X0 + 64 * k + lane + 1] = 0u;
    if (X0 == 0 && lane == 0) S[0] = 0u;
  }
  if (seg == nseg - 1 && chunk == nch - 1) {
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (X0 + 64 * k + lane == W - 1) info[1] = (int32_t)prev[k];      // S[H][W]
    if (lane == 0) { info[0] = thr; info[2] = 0; info[3] = 0; }
  }
}

// ---- the XY cut ------------------------------------------------------------------------------------------------------------------------------

struct Region { int32_t x0, y0, x1, y1, depth, leaf, pad[2]; };

struct SatView {
  const uint32_t* s;
  int64_t p;
  __device__ __forceinline__ uint32_t at(int y, int x) const { return s[(int64_t)y * p + x]; }
  __device__ __forceinline__ int rect(int x0, int y0, int x1, int y1) const {      // ink in [x0,x1) x [y0,y1): differences mod 2^32 are exact
    return (int)(at(y1, x1) - at(y0, x1) - at(y1, x0) + at(y0, x0));
  }
};

// first to last occupied column, then first to last occupied row of the narrowed region; false: the region is empty.  All threads call it
// and all return the same.
__device__ __forceinline__ bool tighten(const SatView& T, int min_ink, int* wtot, int& x0, int& y0, int& x1, int& y1) {
  auto imax = [](int a, int b) { return a > b ? a : b; };
  auto imin = [](int a, int b) { return a < b ? a : b; };
  int first = SEG_NONE, last = -1, f, l;
  for (int x = x0 + (int)threadIdx.x; x < x1; x += SEG_THREADS)
    if (T.rect(x, y0, x + 1, y1) >= min_ink) { first = imin(first, x); last = imax(last, x); }
  block_scan_excl<false>(first, SEG_NONE, imin, wtot, &f);
  block_scan_excl<false>(last, -1, imax, wtot, &l);
  if (l < 0) return false;
  x0 = f; x1 = l + 1;
  first = SEG_NONE; last = -1;
  for (int y = y0 + (int)threadIdx.x; y < y1; y += SEG_THREADS)
    if (T.rect(x0, y, x1, y + 1) >= min_ink) { first = imin(first, y); last = imax(last, y); }
  block_scan_excl<false>(first, SEG_NONE, imin, wtot, &f);
  block_scan_excl<false>(last, -1, imax, wtot, &l);
  if (l < 0) return false;
  y0 = f; y1 = l + 1;
  return true;
}

__global__ __launch_bounds__(SEG_THREADS) void xycut_kernel(const uint32_t* __restrict__ sat, int64_t sp, int H, int W, aocr_layout_params p,
                                                            Region* la, Region* lb, int max_blocks, aocr_box* __restrict__ blocks,
                                                            int32_t* __restrict__ counts) {
  __shared__ RunsShared sh;
  const int tid = threadIdx.x;
  const SatView T{sat, sp};
  Region* cur = la;                                      // not __restrict__: written and read here, a barrier in between
  Region* nxt = lb;
  int n = 0, levels = 0, overflow = 0;
  {
    int x0 = 0, y0 = 0, x1 = W, y1 = H;
    if (tighten(T, p.min_ink, sh.wtot, x0, y0, x1, y1)) {
      if (tid == 0) cur[0] = Region{x0, y0, x1, y1, 0, 0, {0, 0}};
      n = 1;
    }
  }
  __syncthreads();
  auto noop = [](int, int, int) {};
  for (int d = 0; d < p.max_depth && n > 0; ++d) {
    int m = 0;                                           // regions of the next list; beyond max_blocks they are counted, not written
    bool cut_any = false;
    auto push = [&](int x0, int y0, int x1, int y1, int depth, int leaf) {
      if (m < max_blocks && tid == 0) nxt[m] = Region{x0, y0, x1, y1, depth, leaf, {0, 0}};
      ++m;
    };
    for (int i = 0; i < n && m <= max_blocks; ++i) {
      const Region R = cur[i];
      if (R.leaf) { push(R.x0, R.y0, R.x1, R.y1, R.depth, 1); continue; }
      const int w = R.x1 - R.x0, h = R.y1 - R.y0;
      __syncthreads();                                   // the previous region's readers of sh are done
      for (int j = tid; j < w; j += SEG_THREADS) sh.flag[j] = T.rect(R.x0 + j, R.y0, R.x0 + j + 1, R.y1) >= p.min_ink;
      __syncthreads();
      int K = find_runs(sh, w, p.gap_x, 1, noop);
      int axis = 0;
      if (K < 2) {                                       // no column cut: rows, over the region's full columns
        __syncthreads();
        for (int j = tid; j < h; j += SEG_THREADS) sh.flag[j] = T.rect(R.x0, R.y0 + j, R.x1, R.y0 + j + 1) >= p.min_ink;
        __syncthreads();
        K = find_runs(sh, h, p.gap_y, 1, noop);
        axis = 1;
      }
      if (K < 2) { push(R.x0, R.y0, R.x1, R.y1, R.depth, 1); continue; }
      cut_any = true;
      for (int k = 0; k < K && m <= max_blocks; ++k) {   // sh.s, sh.e: the pieces (runs.h); tighten touches sh.wtot only
        const int s = sh.s[k], e = sh.e[k];
        int x0 = axis ? R.x0 : R.x0 + s, x1 = axis ? R.x1 : R.x0 + e, y0 = axis ? R.y0 + s : R.y0, y1 = axis ? R.y0 + e : R.y1;
        if (tighten(T, p.min_ink, sh.wtot, x0, y0, x1, y1)) push(x0, y0, x1, y1, d + 1, 0);
      }
    }
    if (m > max_blocks) { overflow = 1; break; }         // this level's cuts are discarded: the list stays as it was
    if (!cut_any) break;                                 // every region is a leaf: the list is final
    __syncthreads();                                     // thread 0's writes to nxt, before anyone reads them as cur
    Region* t = cur; cur = nxt; nxt = t;
    n = m;
    ++levels;
  }
  __syncthreads();
  int keep = 0, ink = 0;                                 // n <= max_blocks <= SEG_THREADS: one region per thread
  Region R{};
  if (tid < n) {
    R = cur[tid];
    ink = T.rect(R.x0, R.y0, R.x1, R.y1);
    keep = (R.x1 - R.x0 >= p.min_block_w) && (R.y1 - R.y0 >= p.min_block_h) && (ink >= p.min_block_ink);
  }
  int total;
  const int o = block_scan_excl<false>(keep, 0, [](int a, int b) { return a + b; }, sh.wtot, &total);
  if (keep) {
    aocr_box bx;
    bx.x0 = R.x0; bx.y0 = R.y0; bx.x1 = R.x1; bx.y1 = R.y1; bx.line = R.depth; bx.ink = ink;
    blocks[o] = bx;
  }
  if (tid == 0) { counts[0] = total; counts[1] = levels; counts[2] = n - total; counts[3] = overflow; }
}

}  // namespace

size_t integral_scratch_bytes(int H, int W) { return sat_layout(H, W).total; }

void ink_integral(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, int threshold, int light_text, void* scratch, uint32_t* sat,
                  int64_t sat_pitch, int32_t* info) {
  const SatLayout l = sat_layout(H, W);
  uint32_t* hist = scratch_at<uint32_t>(scratch, l.hist);
  int32_t* hdr = scratch_at<int32_t>(scratch, l.hdr);
  uint32_t* cc = scratch_at<uint32_t>(scratch, l.cc);
  uint32_t* rc = scratch_at<uint32_t>(scratch, l.rc);
  const int light = light_text ? 1 : 0, fixed = threshold;
  page_threshold(s, page, pitch, H, W, fixed, hist, hdr);
  const dim3 tiles(cdiv(l.nseg, 4), l.nch);
  hipLaunchKernelGGL(sat_colcount_kernel, dim3(cdiv(W, 256), l.nseg), dim3(256), 0, s, page, pitch, H, W, light, fixed, hdr, cc);
  hipLaunchKernelGGL(sat_rowcount_kernel, tiles, dim3(256), 0, s, page, pitch, H, W, light, fixed, hdr, l.nseg, l.nch, rc);
  hipLaunchKernelGGL(sat_colscan_kernel, dim3(cdiv(W, 64)), dim3(64 * SCAN_GROUPS), 0, s, cc, W, l.nseg);
  hipLaunchKernelGGL(sat_tile_kernel, tiles, dim3(256), 0, s, page, pitch, H, W, light, fixed, hdr, l.nseg, l.nch, cc, rc, sat, sat_pitch, info);
}

size_t layout_scratch_bytes(int max_blocks) {            // the two level lists
  ScratchCursor c;
  c.take((size_t)max_blocks * sizeof(Region));
  c.take((size_t)max_blocks * sizeof(Region));
  return c.total();
}

void layout_blocks(hipStream_t s, const uint32_t* sat, int64_t sat_pitch, int H, int W, const aocr_layout_params& p, void* scratch, int max_blocks,
                   aocr_box* blocks, int32_t* counts) {
  Region* la = scratch_at<Region>(scratch, 0);
  Region* lb = scratch_at<Region>(scratch, layout_scratch_bytes(max_blocks) / 2);
  hipLaunchKernelGGL(xycut_kernel, dim3(1), dim3(SEG_THREADS), 0, s, sat, sat_pitch, H, W, p, la, lb, max_blocks, blocks, counts);
}

}  // namespace aocr
