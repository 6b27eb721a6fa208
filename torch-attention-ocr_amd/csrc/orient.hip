// orient.hip -- page orientation (include/aocr.h: aocr_rotate_page, aocr_estimate_orientation), the stage in front of aocr_estimate_skew:
// every later stage assumes that the text lines run along x.  aocr_rotate_page turns the page by quarter turns, aocr_estimate_orientation
// counts where ink runs start along x and along y and says which way the lines run.  Integer arithmetic only (the Otsu threshold, when
// asked for, comes from segment.hip's otsu_threshold), so tests/orient_ref.py matches exactly.
//
// aocr_rotate_page is one launch.  The odd part of the turn comes from the host (it sets the output's shape), a half turn may be added
// from orient_dev[0] on the device:
//   rotate_rows_kernel  q = 0 or 2.  One wave per output row (wave_store_row of page_common.h).  The 16 source bytes of a store are four words when the source run is 4-byte
//                       aligned (one decision per row: all runs of a row are 16 bytes apart), else 16 byte loads; the half turn takes the
//                       words in reverse order and reverses the bytes within each.  No LDS.
//   rotate_tile_kernel  q = 1 or 3.  A workgroup owns a TILE x TILE block of the output.  Its source block goes into LDS row by row, 16
//                       bytes per thread (one 16-byte load, four words or 16 bytes, by the row address), the rows TILE + 4 bytes apart.  Then
//                       every thread takes a 4 x 4 block: four words down an LDS column (rows 17 words apart: lanes 8 blocks apart meet on a
//                       bank, a 2-way conflict on 4 reads per 16 bytes, far under the time of the global traffic), the 4 x 4 byte transpose
//                       in registers, and four word stores, 16 consecutive lanes writing 64 consecutive bytes of an output row; rows whose
//                       address is not 4-byte aligned, and blocks cut by the page's edge, take byte stores.
// Every output byte is written once, by a thread that its position alone selects, from a source byte that the mapping alone selects: the
// result does not depend on the launch geometry.
//
// Launches of one aocr_estimate_orientation, all on the caller's stream, intermediates in the caller's scratch:
//   (Otsu only) otsu_threshold of segment.hip: memset, hist_kernel, otsu_kernel -- what aocr_segment_page enqueues for its steps 1-2.
//   runs_kernel    the one page read.  A wave owns a 64-column strip and RUN_ROWS rows of it, one byte per lane and row, RUN_UNROLL rows in
//                  flight: m = ballot(ink); a run starts along x where m has a bit whose lower neighbour is clear (lane 0's neighbour is
//                  the byte left of the strip, read by lane 0), along y where the previous row's mask has none (the first row reads the row
//                  above the wave's range).  Three sums in (uniform) registers; the four waves of a workgroup meet in LDS and the
//                  workgroup writes its three sums to its own slot of the scratch.  (One atomic per wave and counter was measured first:
//                  13 000 waves on three words of one cache line took 0.12 ms on an A4 page, 87 x the page read.)
//   decide_kernel  one workgroup adds the slots and writes the eight words.
// No atomics (outside the Otsu histogram's integer ones); integer sums do not depend on their order: the words do not depend on the launch
// geometry.
#include <algorithm>
#include "ops.h"
#include "page_common.h"

namespace aocr {

namespace {

constexpr int TILE = 64;
constexpr int TILE_STRIDE = TILE + 4;          // bytes between the LDS rows: 17 words
constexpr int RUN_ROWS = 32;                   // rows of one wave of runs_kernel
constexpr int RUN_UNROLL = 8;                  // of them in flight

struct OrientLayout {                          // byte offsets into scratch_dev
  size_t hist, hdr, sums, total;
  int gx, gy;                                  // the grid of runs_kernel: strips x groups of 4 * RUN_ROWS rows
};

OrientLayout orient_layout(int H, int W) {
  OrientLayout l;
  ScratchCursor c;
  l.gx = cdiv(W, 64);
  l.gy = cdiv(H, 4 * RUN_ROWS);
  l.hist = c.take(256 * sizeof(uint32_t));
  l.hdr = c.take(4 * sizeof(int32_t));
  l.sums = c.take((size_t)l.gx * l.gy * sizeof(uint4));               // N_h, N_v, the ink, 0 per workgroup
  l.total = c.total();
  return l;
}

__device__ __forceinline__ uint32_t bytes_rev(uint32_t w) { return __builtin_bswap32(w); }

__global__ __launch_bounds__(256) void rotate_rows_kernel(const uint8_t* __restrict__ page, int64_t pitch, int H, int W,
                                                          const int32_t* __restrict__ orient, int quarter, uint8_t* __restrict__ out,
                                                          int64_t out_pitch) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool rev = ((quarter + (orient ? (orient[0] & 2) : 0)) & 3) == 2;
  for (int y = blockIdx.x * 4 + wave; y < H; y += gridDim.x * 4) {
    const uint8_t* src = page + (int64_t)(rev ? H - 1 - y : y) * pitch;
    uint8_t* o = out + (int64_t)y * out_pitch;
    const int head = row_head(o, W);                       // the first column of the row's first 16-byte store
    // output columns x .. x+15 come from source columns x .. x+15, or W-16-x .. W-1-x backwards; every run of the row has the same alignment
    const bool words = (((uintptr_t)src + (uintptr_t)(int64_t)(rev ? W - 16 - head : head)) & 3u) == 0;
    auto px1 = [&](int x) -> uint8_t { return src[rev ? W - 1 - x : x]; };
    auto px16 = [&](int x) -> uint4 {
      const uint8_t* p = src + (rev ? W - 16 - x : x);
      uint32_t w[4];
      if (words) {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = reinterpret_cast<const uint32_t*>(p)[k];
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          w[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) | ((uint32_t)p[4 * k + 3] << 24);
      }
      uint4 q;
      if (rev) { q.x = bytes_rev(w[3]); q.y = bytes_rev(w[2]); q.z = bytes_rev(w[1]); q.w = bytes_rev(w[0]); }
      else { q.x = w[0]; q.y = w[1]; q.z = w[2]; q.w = w[3]; }
      return q;
    };
    wave_store_row(o, W, lane, px1, px16);
  }
}

// the output is Ho = W rows of Wo = H bytes.  q = 1: out[y][x] = page[H-1-x][y];  q = 3: out[y][x] = page[x][W-1-y]
__global__ __launch_bounds__(256) void rotate_tile_kernel(const uint8_t* __restrict__ page, int64_t pitch, int H, int W,
                                                          const int32_t* __restrict__ orient, int quarter, uint8_t* __restrict__ out,
                                                          int64_t out_pitch) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[TILE * TILE_STRIDE];
  const int q = (quarter + (orient ? (orient[0] & 2) : 0)) & 3;       // 1 or 3: quarter is odd
  const int ox0 = blockIdx.x * TILE, oy0 = blockIdx.y * TILE;         // the output block; its source block starts at (sr0, sc0), maybe outside
  const int sr0 = q == 1 ? H - TILE - ox0 : ox0;
  const int sc0 = q == 1 ? oy0 : W - TILE - oy0;
  {
    const int r = threadIdx.x >> 2, c = (threadIdx.x & 3) << 4;       // 16 bytes of row r of the source block
    const int sy = sr0 + r, sx = sc0 + c;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if ((unsigned)sy < (unsigned)H) {
      const uint8_t* p = page + (int64_t)sy * pitch + sx;             // formed only; read where 0 <= sx + j < W
      if (sx >= 0 && sx + 16 <= W && ((uintptr_t)p & 15u) == 0) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
      } else if (sx >= 0 && sx + 16 <= W && ((uintptr_t)p & 3u) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = reinterpret_cast<const uint32_t*>(p)[k];
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if ((unsigned)(sx + j) < (unsigned)W) w[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
      }
    }
    uint32_t* d = reinterpret_cast<uint32_t*>(tile + r * TILE_STRIDE + c);
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = w[k];
  }
  __syncthreads();
  const int bc = threadIdx.x & 15, br = threadIdx.x >> 4;             // the 4 x 4 block: output rows oy0 + 4 br + m, columns ox0 + 4 bc + k
  uint32_t a[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {                                       // output column 4 bc + k of the block is LDS row ...
    const int r = q == 1 ? TILE - 1 - 4 * bc - k : 4 * bc + k;
    const int cw = q == 1 ? br : 15 - br;                             // ... and the block's four output rows are the bytes of this word of it
    a[k] = *reinterpret_cast<const uint32_t*>(tile + r * TILE_STRIDE + 4 * cw);
  }
  const int x = ox0 + 4 * bc;
  if (x >= H) return;                                                 // Wo = H
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int y = oy0 + 4 * br + m;
    if (y >= W) break;                                                // Ho = W
    const int sh = 8 * (q == 1 ? m : 3 - m);
    const uint32_t v = ((a[0] >> sh) & 0xffu) | (((a[1] >> sh) & 0xffu) << 8) | (((a[2] >> sh) & 0xffu) << 16) | (((a[3] >> sh) & 0xffu) << 24);
    uint8_t* o = out + (int64_t)y * out_pitch + x;
    if (x + 4 <= H && ((uintptr_t)o & 3u) == 0) {
      *reinterpret_cast<uint32_t*>(o) = v;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x + k < H) o[k] = (uint8_t)(v >> (8 * k));
    }
  }
}

__global__ __launch_bounds__(256) void runs_kernel(const uint8_t* __restrict__ page, int64_t pitch, int H, int W, int light, int fixed,
                                                   const int32_t* __restrict__ hdr, uint4* __restrict__ sums) {
  __shared__ uint32_t wsum[4][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int thr = ink_thr(fixed, hdr);
  const int x0 = blockIdx.x * 64, x = x0 + lane;
  const int y0 = (blockIdx.y * 4 + wave) * RUN_ROWS, y1 = thr < 0 ? y0 : min(H, y0 + RUN_ROWS);       // no threshold, or past the page: no rows
  const bool inside = x < W, left = lane == 0 && x0 > 0;
  const uint8_t* col = page + x;                         // read where inside; col[-1] where left
  uint64_t prev = 0;                                     // the mask of the row above: paper off the page
  if (y0 > 0 && y0 < y1) prev = __ballot(inside && is_ink(col[(int64_t)(y0 - 1) * pitch], thr, light));
  uint32_t nh = 0, nv = 0, total = 0;
  for (int y = y0; y < y1; y += RUN_UNROLL) {
    int v[RUN_UNROLL], c[RUN_UNROLL];
#pragma unroll
    for (int j = 0; j < RUN_UNROLL; ++j) {
      const bool row = y + j < y1;
      const uint8_t* p = col + (int64_t)(y + j) * pitch;
      v[j] = (row && inside) ? (int)p[0] : -1;
      c[j] = (row && left) ? (int)p[-1] : -1;
    }
#pragma unroll
    for (int j = 0; j < RUN_UNROLL; ++j) {
      if (y + j >= y1) break;                            // uniform
      const uint64_t m = __ballot(v[j] >= 0 && is_ink(v[j], thr, light));
      const uint64_t carry = __ballot(c[j] >= 0 && is_ink(c[j], thr, light));       // bit 0, or nothing
      nh += (uint32_t)__popcll(m & ~((m << 1) | carry));
      nv += (uint32_t)__popcll(m & ~prev);
      total += (uint32_t)__popcll(m);
      prev = m;
    }
  }
  if (lane == 0) { wsum[wave][0] = nh; wsum[wave][1] = nv; wsum[wave][2] = total; }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint4 o;
    o.x = wsum[0][0] + wsum[1][0] + wsum[2][0] + wsum[3][0];
    o.y = wsum[0][1] + wsum[1][1] + wsum[2][1] + wsum[3][1];
    o.z = wsum[0][2] + wsum[1][2] + wsum[2][2] + wsum[3][2];
    o.w = 0;
    sums[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = o;
  }
}

__global__ __launch_bounds__(256) void decide_kernel(const uint4* __restrict__ sums, int n, int fixed, const int32_t* __restrict__ hdr,
                                                     int32_t* __restrict__ orient) {
  __shared__ uint32_t part[256][3];
  uint32_t nh = 0, nv = 0, total = 0;                    // each at most 2^26
  for (int i = threadIdx.x; i < n; i += 256) { const uint4 v = sums[i]; nh += v.x; nv += v.y; total += v.z; }
  part[threadIdx.x][0] = nh; part[threadIdx.x][1] = nv; part[threadIdx.x][2] = total;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if ((int)threadIdx.x < d)
      for (int k = 0; k < 3; ++k) part[threadIdx.x][k] += part[threadIdx.x + d][k];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    orient[0] = part[0][1] > part[0][0] ? 1 : 0;         // a tie keeps the page
    orient[1] = (int32_t)part[0][0]; orient[2] = (int32_t)part[0][1];
    orient[3] = ink_thr(fixed, hdr);
    orient[4] = (int32_t)part[0][2];
    orient[5] = 0; orient[6] = 0; orient[7] = 0;
  }
}

}  // namespace

void rotate_page(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const int32_t* orient, int quarter, uint8_t* out,
                 int64_t out_pitch) {
  if (quarter & 1)
    hipLaunchKernelGGL(rotate_tile_kernel, dim3(cdiv(H, TILE), cdiv(W, TILE)), dim3(256), 0, s, page, pitch, H, W, orient, quarter, out, out_pitch);
  else
    hipLaunchKernelGGL(rotate_rows_kernel, dim3(std::min(cdiv(H, 4), 2048)), dim3(256), 0, s, page, pitch, H, W, orient, quarter, out, out_pitch);
}

size_t orient_scratch_bytes(int H, int W) { return orient_layout(H, W).total; }

void estimate_orientation(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, int threshold, int light_text, void* scratch,
                          int32_t* orient) {
  const OrientLayout l = orient_layout(H, W);
  uint32_t* hist = scratch_at<uint32_t>(scratch, l.hist);
  int32_t* hdr = scratch_at<int32_t>(scratch, l.hdr);
  uint4* sums = scratch_at<uint4>(scratch, l.sums);
  page_threshold(s, page, pitch, H, W, threshold, hist, hdr);
  hipLaunchKernelGGL(runs_kernel, dim3(l.gx, l.gy), dim3(256), 0, s, page, pitch, H, W, light_text ? 1 : 0, threshold, hdr, sums);
  hipLaunchKernelGGL(decide_kernel, dim3(1), dim3(256), 0, s, sums, l.gx * l.gy, threshold, hdr, orient);
}

}  // namespace aocr
