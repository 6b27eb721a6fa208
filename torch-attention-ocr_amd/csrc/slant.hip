// slant.hip -- word slant (include/aocr.h: aocr_estimate_slant, aocr_crop_lines_slanted), the stage between aocr_segment_page and the
// recogniser: for every box a sweep of sheared column profiles finds the lean of the writing, and the crops are taken with every row of
// the box moved back along x.  The estimate is integer arithmetic only, so tests/slant_ref.py matches exactly; the crops scale with
// resample.h's scale_elem, data.hip's arithmetic (this file is compiled with -ffp-contract=off like data.hip: Makefile, FLAGS_slant).
//
// Launches of one aocr_estimate_slant, all on the caller's stream, intermediates in the caller's scratch:
//   memset          the scratch: per box 2K+1 uint64 score slots and one ink slot.
//   profile_kernel  grid (column chunk, box): the box widths are known only on the device, so the grid is sized for the page width and a
//                   workgroup whose chunk starts beyond its box's profile range [x0 - D, x1 + D) exits.  A workgroup owns SLANT_CHUNK
//                   profile columns.  It reads the rows of its box once, its columns and a halo of D <= SLANT_HALO on either side, a wave
//                   per row (wave_row16 and ink_mask16 of page_common.h), and keeps the ink as bit rows in LDS: 256 rows of 512 bits,
//                   16 KiB.  The (candidate, column) pairs are then spread over the threads: a thread walks the rows of its pair, one LDS
//                   word and one bit test per row, squares the column sum and adds it to the candidate's uint32 slot in LDS (a chunk's
//                   share is at most 256 * 256^2 = 2^24).  The slots go to the box's scratch slots with 64-bit integer atomics: any split
//                   over columns is exact.  A box taller than AOCR_SLANT_MAX_H only has its ink counted, straight from the row walk.
//   pick_kernel     a thread per box: the winner by "larger score, then earlier in 0, -1, +1, -2, +2, ...", slant_dev and scores_dev.
// aocr_crop_lines_slanted is one launch, crop_slanted_kernel: crop_kernel of data.hip with the source column of every tap moved by the
// row's offset; one thread per output pixel.
#include <algorithm>
#include "ops.h"
#include "page_common.h"
#include "resample.h"

namespace aocr {

namespace {

constexpr int SLANT_CHUNK = 256;                               // profile columns of one profile_kernel workgroup = its threads
constexpr int SLANT_HALO = 128;                                // the largest |off|: |cy - y| <= 128 for h <= 256, |s| <= 65536
constexpr int SLANT_WORDS = (SLANT_CHUNK + 2 * SLANT_HALO) / 32;
constexpr int SLANT_MAX_K = 64;
constexpr int SLANT_S_MAX = 65536;                             // what aocr_crop_lines_slanted clamps a slant to

struct Rect { int x0, y0, x1, y1; };

__device__ __forceinline__ Rect clamp_box(const aocr_box& b, int H, int W) {
  return Rect{min(max(b.x0, 0), W), min(max(b.y0, 0), H), min(max(b.x1, 0), W), min(max(b.y1, 0), H)};
}

// off(y) of include/aocr.h: |cy - y| <= 16384 and |s| <= 65536 keep the product inside int32
__device__ __forceinline__ int slant_off(int cy, int y, int s) { return ((cy - y) * s + 32768) >> 16; }

// max over y in [y0, y1) of |off(y)|: off is monotonic in y, so it is at one of the two ends
__device__ __forceinline__ int slant_extent(int cy, int y0, int y1, int s) { return max(abs(slant_off(cy, y0, s)), abs(slant_off(cy, y1 - 1, s))); }

__global__ __launch_bounds__(SLANT_CHUNK) void profile_kernel(const uint8_t* __restrict__ page, int64_t pitch, int H, int W,
                                                              const aocr_box* __restrict__ boxes, const int32_t* __restrict__ count, int n_boxes,
                                                              int light, int fixed, const int32_t* __restrict__ threshold, int step, int K,
                                                              unsigned long long* __restrict__ slots) {
  __shared__ uint32_t bits[AOCR_SLANT_MAX_H][SLANT_WORDS];     // bit b of row r: the ink of page column cs - SLANT_HALO + b, row y0 + r
  __shared__ uint32_t part[2 * SLANT_MAX_K + 1];
  __shared__ uint32_t inkc;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.y, nc = 2 * K + 1;
  const int n = count ? min(n_boxes, count[0]) : n_boxes;
  if (i >= n) return;
  const Rect b = clamp_box(boxes[i], H, W);
  const int w = b.x1 - b.x0, h = b.y1 - b.y0;
  if (w <= 0 || h <= 0) return;
  const int thr = ink_thr(fixed, threshold);
  if (thr < 0) return;                                         // nothing is ink: the slots stay 0
  unsigned long long* sc = slots + (size_t)i * (nc + 1);       // nc scores, then the ink
  if (h > AOCR_SLANT_MAX_H) {                                  // not estimated: this chunk's share of the ink, straight from the rows
    const int cs = b.x0 + blockIdx.x * SLANT_CHUNK, ce = min(cs + SLANT_CHUNK, b.x1);
    if (cs >= b.x1) return;
    int c = 0;
    for (int y = b.y0 + wave; y < b.y1; y += SLANT_CHUNK / 64)
      wave_row(page + (int64_t)y * pitch + cs, ce - cs, lane, [&](uint32_t v, int m) { c += ink_bytes(v, m, thr, light); });
    c = wave_sum(c);
    if (lane == 0 && c) atomicAdd(&sc[nc], (unsigned long long)c);
    return;
  }
  const int cy = (b.y0 + b.y1) >> 1;
  const int D = max(slant_extent(cy, b.y0, b.y1, K * step), slant_extent(cy, b.y0, b.y1, -K * step));      // <= SLANT_HALO
  const int cs = b.x0 - D + blockIdx.x * SLANT_CHUNK, ce = min(cs + SLANT_CHUNK, b.x1 + D);                  // this chunk's profile columns
  if (cs >= b.x1 + D) return;
  for (int j = tid; j < h * SLANT_WORDS; j += SLANT_CHUNK) (&bits[0][0])[j] = 0;
  if (tid < nc) part[tid] = 0;
  if (tid == 0) inkc = 0;
  __syncthreads();
  const int lo = max(b.x0, cs - D), hi = min(b.x1, ce + D);    // the page columns that a profile column of this chunk can read
  const int base = lo - (cs - SLANT_HALO);                     // the bit of column lo: >= SLANT_HALO - D >= 0; the last one, hi - 1, is < 512
  if (hi > lo)
    for (int r = wave; r < h; r += SLANT_CHUNK / 64) {
      uint32_t* row = bits[r];
      wave_row16(page + (int64_t)(b.y0 + r) * pitch + lo, hi - lo, lane,
                 [&](int x, uint32_t v) {
                   if (is_ink((int)v, thr, light)) atomicOr(&row[(base + x) >> 5], 1u << ((base + x) & 31));
                 },
                 [&](int x, const uint4& q) {
                   const uint32_t m = ink_mask16(q, thr, light);
                   const int p = base + x, sh = p & 31;
                   if (m) atomicOr(&row[p >> 5], m << sh);
                   if (sh > 16 && (m >> (32 - sh))) atomicOr(&row[(p >> 5) + 1], m >> (32 - sh));      // p + 15 < 512: the word exists
                 });
    }
  __syncthreads();
  const int ncols = ce - cs, total = nc * ncols;
  for (int idx = tid; idx < total; idx += SLANT_CHUNK) {
    const int kk = idx / ncols, c = idx - kk * ncols;
    const int s = (kk - K) * step;
    int t = (cy - b.y0) * s + 32768;                           // (cy - y) * s + 32768 for y = y0, y0 + 1, ...
    const int p0 = c + SLANT_HALO;                             // p0 + off lies in [SLANT_HALO - D, SLANT_CHUNK + SLANT_HALO + D)
    uint32_t P = 0;
    for (int r = 0; r < h; ++r, t -= s) {
      const int p = p0 + (t >> 16);
      P += (bits[r][p >> 5] >> (p & 31)) & 1u;
    }
    if (P) {
      atomicAdd(&part[kk], P * P);
      if (kk == K) atomicAdd(&inkc, P);                        // candidate 0 is the box itself: its profile sums to the ink
    }
  }
  __syncthreads();
  if (tid < nc && part[tid]) atomicAdd(&sc[tid], (unsigned long long)part[tid]);
  if (tid == nc && inkc) atomicAdd(&sc[nc], (unsigned long long)inkc);
}

__global__ __launch_bounds__(256) void pick_kernel(const aocr_box* __restrict__ boxes, const int32_t* __restrict__ count, int n_boxes, int H, int W,
                                                   int step, int K, const unsigned long long* __restrict__ slots, int32_t* __restrict__ slant,
                                                   unsigned long long* __restrict__ scores) {
  const int i = blockIdx.x * 256 + threadIdx.x, nc = 2 * K + 1;
  const int n = count ? min(n_boxes, count[0]) : n_boxes;
  if (i >= n) return;
  const Rect b = clamp_box(boxes[i], H, W);
  const int w = b.x1 - b.x0, h = b.y1 - b.y0;
  const int flag = (w <= 0 || h <= 0) ? 2 : h > AOCR_SLANT_MAX_H ? 1 : 0;
  const unsigned long long* t = slots + (size_t)i * (nc + 1) + K;          // t[k], k in [-K, K]; t[K + 1] is the ink
  int bk = 0;
  if (flag == 0) {
    unsigned long long best = t[0];
    for (int a = 1; a <= K; ++a) {                             // 0, -1, +1, -2, +2, ...: only a strictly larger score replaces an earlier one
      if (t[-a] > best) { best = t[-a]; bk = -a; }
      if (t[a] > best) { best = t[a]; bk = a; }
    }
  }
  slant[4 * i] = bk; slant[4 * i + 1] = bk * step; slant[4 * i + 2] = flag; slant[4 * i + 3] = flag == 2 ? 0 : (int32_t)t[K + 1];
  if (scores)
    for (int k = -K; k <= K; ++k) scores[(size_t)i * nc + k + K] = flag == 0 ? t[k] : 0ull;
}

// crop_kernel of data.hip with every row of the box moved along x by its offset: the virtual rectangle V of include/aocr.h, h rows of
// w + 2D columns, scaled like aocr_preprocess_lines scales an image.  s == 0 gives D = 0 and off = 0: crop_kernel's taps, the same bits.
__global__ __launch_bounds__(256) void crop_slanted_kernel(const uint8_t* __restrict__ page, int64_t pitch, int H, int W,
                                                           const aocr_box* __restrict__ boxes, const int32_t* __restrict__ count, int n_boxes,
                                                           const int32_t* __restrict__ slant, float fill, int out_h, int out_w,
                                                           float* __restrict__ out) {
  const int img = blockIdx.y;
  const int id = blockIdx.x * 256 + threadIdx.x;
  const int n = count ? min(n_boxes, count[0]) : n_boxes;
  if (img >= n || id >= out_h * out_w) return;
  const int y = id / out_w, x = id - y * out_w;
  const Rect b = clamp_box(boxes[img], H, W);
  const int w = b.x1 - b.x0, h = b.y1 - b.y0;
  float v = 255.0f;
  if (w > 0 && h > 0) {
    const int s = slant ? min(max(slant[4 * img + 1], -SLANT_S_MAX), SLANT_S_MAX) : 0;
    const int cy = (b.y0 + b.y1) >> 1, D = slant_extent(cy, b.y0, b.y1, s);
    auto tmp = [&](int row) {
      const uint8_t* src = page + (int64_t)(b.y0 + row) * pitch;
      const int first = b.x0 - D + slant_off(cy, b.y0 + row, s);          // the page column of V's column 0 in this row
      return scale_elem([&](int col) { const int sx = first + col; return (sx >= b.x0 && sx < b.x1) ? (float)src[sx] : fill; }, w + 2 * D, out_w, x);
    };
    v = scale_elem(tmp, h, out_h, y);
  }
  out[((int64_t)img * out_h + y) * out_w + x] = v;
}

size_t slot_bytes(int n_boxes, int n_steps) { return (size_t)std::max(n_boxes, 1) * (2 * n_steps + 2) * sizeof(unsigned long long); }

}  // namespace

size_t slant_scratch_bytes(int n_boxes, int n_steps) {
  ScratchCursor c;
  c.take(slot_bytes(n_boxes, n_steps));
  return c.total();
}

void estimate_slant(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_box* boxes, const int32_t* count, int n_boxes,
                    const aocr_slant_params& p, const int32_t* threshold, void* scratch, int32_t* slant, uint64_t* scores) {
  if (n_boxes <= 0) return;
  unsigned long long* slots = static_cast<unsigned long long*>(scratch);
  const int K = p.n_steps, light = p.light_text ? 1 : 0;
  const int dcap = std::min(SLANT_HALO, (int)(((int64_t)SLANT_HALO * K * p.step_q16 + 32768) >> 16));     // no box's D exceeds it
  (void)hipMemsetAsync(slots, 0, slot_bytes(n_boxes, K), s);
  hipLaunchKernelGGL(profile_kernel, dim3(cdiv(W + 2 * dcap, SLANT_CHUNK), n_boxes), dim3(SLANT_CHUNK), 0, s, page, pitch, H, W, boxes, count,
                     n_boxes, light, p.threshold, threshold, p.step_q16, K, slots);
  hipLaunchKernelGGL(pick_kernel, dim3(cdiv(n_boxes, 256)), dim3(256), 0, s, boxes, count, n_boxes, H, W, p.step_q16, K, slots, slant,
                     reinterpret_cast<unsigned long long*>(scores));
}

void crop_lines_slanted(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_box* boxes, const int32_t* count,
                        int n_boxes, const int32_t* slant, int fill, int out_h, int out_w, float* out) {
  if (n_boxes <= 0) return;
  hipLaunchKernelGGL(crop_slanted_kernel, dim3(cdiv(out_h * out_w, 256), n_boxes), dim3(256), 0, s, page, pitch, H, W, boxes, count, n_boxes,
                     slant, (float)fill, out_h, out_w, out);
}

}  // namespace aocr
