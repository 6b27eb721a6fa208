// segment.hip -- page segmentation by projection profiles (include/aocr.h: aocr_segment_page): a gray uint8 page becomes the word boxes
// that aocr_crop_lines cuts out for the recogniser.  Everything is integer arithmetic except the Otsu scores, which are double precision
// with every operation rounded on its own: this file is compiled with -ffp-contract=off (Makefile: FLAGS_segment), so the numpy
// restatement (tests/segment_ref.py) matches exactly.
//
// Launches of one call, all on the caller's stream, intermediates in the caller's scratch:
//   hist_kernel     (Otsu only) one wave per row (wave_row of page_common.h, which holds the row walks, the ink test and the scratch
//                   layout of all the page kernels); a 256-bin LDS histogram per wave, flushed with integer global atomics
//                   (order-independent: exact).
//   otsu_kernel     one wave: lane l owns bins 4l..4l+3, int64 prefix sums over lanes, the 255 scores in parallel, then the argmax with
//                   "larger score, then lower t" (= the first strictly largest of the serial loop).  Otsu only: a fixed threshold is a
//                   launch argument of the kernels that need it.
//   rowprof_kernel  one wave per row, the same loads, per-lane byte compares and a wave sum; Otsu's threshold is read from the device.
//   bands_kernel    one workgroup: text-row flags in LDS -> bands (find_runs of runs.h).
//   colprof_kernel  one thread per column per band: consecutive threads read consecutive bytes, row after row of the band.
//   words_kernel    one workgroup per band: ink-column flags in LDS -> words (the same find_runs); the first `cap` words of each band are kept.
//                   words_spaced_kernel (aocr_segment_page_spaced) is the same body with the gap estimated per band in front of it: a first
//                   find_runs for the raw runs, a 256-bin LDS histogram of their gaps, otsu_kernel's wave function on it (band_gap).
//   offsets_kernel  one workgroup: exclusive prefix sum of the bands' word counts; writes counts_dev.
//   emit_kernel     one wave per written box: finds its band by bisection of the offsets, sums the box's ink from the column profile,
//                   pads, clamps and stores the box.
// find_runs (runs.h, shared with layout.hip) turns "flag[i], merge runs closer than gapmin, drop runs shorter than minlen" into three block scans: an element that is set
// starts a run iff the previous set element is at least gapmin clear elements away (prefix max of set indices), ends one iff the next set
// element is (suffix min), and the k-th start pairs with the k-th end (prefix sums).  No step depends on launch geometry or on atomics order.
#include <algorithm>
#include "ops.h"
#include "page_common.h"
#include "runs.h"

namespace aocr {

namespace {

struct SegLayout {                             // byte offsets into scratch_dev
  size_t hist, hdr, row_ink, bands, wcount, woffset, col, words, total;
  int max_bands, cap;
};

SegLayout seg_layout(int H, int W, int max_boxes) {
  SegLayout l;
  ScratchCursor c;
  l.max_bands = (H + 1) / 2;                   // bands are separated by at least one non-text row
  l.cap = std::min(max_boxes, (W + 1) / 2);    // words of one band that can reach boxes_dev
  l.hist = c.take(256 * sizeof(uint32_t));
  l.hdr = c.take(4 * sizeof(int32_t));                                  // threshold, bands, boxes found
  l.row_ink = c.take((size_t)H * sizeof(int32_t));
  l.bands = c.take((size_t)l.max_bands * sizeof(uint32_t));             // y0 | y1 << 16
  l.wcount = c.take((size_t)l.max_bands * sizeof(int32_t));
  l.woffset = c.take((size_t)l.max_bands * sizeof(int32_t));
  l.col = c.take((size_t)l.max_bands * W * sizeof(uint16_t));
  l.words = c.take((size_t)l.max_bands * l.cap * sizeof(uint32_t));     // x0 | x1 << 16, unpadded
  l.total = c.total();
  return l;
}

__global__ __launch_bounds__(256) void hist_kernel(const uint8_t* __restrict__ page, int64_t pitch, int H, int W, uint32_t* __restrict__ hist) {
  __shared__ uint32_t sh[4][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < 4 * 256; i += 256) (&sh[0][0])[i] = 0;
  __syncthreads();
  uint32_t* h = sh[wave];
  for (int y = blockIdx.x * 4 + wave; y < H; y += gridDim.x * 4) {
    wave_row(page + (int64_t)y * pitch, W, lane, [&](uint32_t w, int n) {
      const uint32_t b0 = w & 0xffu;
      if (n == 1) { atomicAdd(&h[b0], 1u); return; }
      if (w == b0 * 0x01010101u) { atomicAdd(&h[b0], 4u); return; }      // paper: four equal pixels, one add
      atomicAdd(&h[b0], 1u); atomicAdd(&h[(w >> 8) & 0xffu], 1u); atomicAdd(&h[(w >> 16) & 0xffu], 1u); atomicAdd(&h[w >> 24], 1u);
    });
  }
  __syncthreads();
  const uint32_t s = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
  if (s) atomicAdd(&hist[threadIdx.x], s);
}

// Otsu's split of a 256-bin histogram by one wave (step 2 of aocr_segment_page): lane l holds bins 4l..4l+3 in h.  The first t in 0..254 with
// the strictly largest score, -1 when no t has two non-empty classes; every lane returns it.
__device__ __forceinline__ int otsu_wave(const long long (&h)[4], int lane) {
  long long ln = 0, ls = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) { ln += h[k]; ls += (long long)(4 * lane + k) * h[k]; }
  long long pn = ln, ps = ls;                                               // inclusive prefix sums over lanes
  for (int d = 1; d < 64; d <<= 1) {
    const long long a = __shfl_up(pn, d), b = __shfl_up(ps, d);
    if (lane >= d) { pn += a; ps += b; }
  }
  const long long N = __shfl(pn, 63), S = __shfl(ps, 63);
  long long n0 = pn - ln, s0 = ps - ls;
  double best = -1.0; int bt = -1;                                          // scores are >= 0
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int t = 4 * lane + k;
    n0 += h[k]; s0 += (long long)t * h[k];
    const long long n1 = N - n0;
    if (t <= 254 && n0 > 0 && n1 > 0) {
      const double d = (double)s0 * (double)n1 - (double)(S - s0) * (double)n0;
      const double score = (d * d) / ((double)n0 * (double)n1);
      if (score > best) { best = score; bt = t; }
    }
  }
  for (int d = 32; d >= 1; d >>= 1) {
    const double ob = __shfl_xor(best, d); const int ot = __shfl_xor(bt, d);
    if (ob > best || (ob == best && ot < bt)) { best = ob; bt = ot; }
  }
  return bt;
}

__global__ __launch_bounds__(64) void otsu_kernel(const uint32_t* __restrict__ hist, int32_t* __restrict__ hdr) {
  const int lane = threadIdx.x;
  long long h[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) h[k] = hist[4 * lane + k];
  const int bt = otsu_wave(h, lane);
  if (lane == 0) hdr[0] = bt;                                               // -1: one gray value only, no ink
}

__global__ __launch_bounds__(256) void rowprof_kernel(const uint8_t* __restrict__ page, int64_t pitch, int H, int W, int light, int fixed,
                                                      const int32_t* __restrict__ hdr, int32_t* __restrict__ row_ink) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int thr = ink_thr(fixed, hdr);
  for (int y = blockIdx.x * 4 + wave; y < H; y += gridDim.x * 4) {
    int c = 0;
    if (thr >= 0) wave_row(page + (int64_t)y * pitch, W, lane, [&](uint32_t w, int n) { c += ink_bytes(w, n, thr, light); });
    c = wave_sum(c);
    if (lane == 0) row_ink[y] = c;
  }
}

__global__ __launch_bounds__(SEG_THREADS) void bands_kernel(const int32_t* __restrict__ row_ink, int H, int min_row_ink, int merge_gap,
                                                            int min_line_h, uint32_t* __restrict__ bands, int32_t* __restrict__ hdr) {
  __shared__ RunsShared sh;
  for (int y = threadIdx.x; y < H; y += SEG_THREADS) sh.flag[y] = row_ink[y] >= min_row_ink;
  __syncthreads();
  const int n = find_runs(sh, H, merge_gap + 1, min_line_h, [&](int k, int y0, int y1) { bands[k] = (uint32_t)y0 | ((uint32_t)y1 << 16); });
  if (threadIdx.x == 0) hdr[1] = n;
}

__global__ __launch_bounds__(256) void colprof_kernel(const uint8_t* __restrict__ page, int64_t pitch, int W, int light, int fixed, int max_bands,
                                                      const int32_t* __restrict__ hdr, const uint32_t* __restrict__ bands,
                                                      uint16_t* __restrict__ col) {
  const int thr = ink_thr(fixed, hdr), nb = min(hdr[1], max_bands);
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= W) return;
  for (int b = blockIdx.y; b < nb; b += gridDim.y) {
    const uint32_t yy = bands[b];
    const int y0 = (int)(yy & 0xffffu), y1 = (int)(yy >> 16);
    const uint8_t* p = page + (int64_t)y0 * pitch + x;
    int c = 0;
    for (int y = y0; y < y1; ++y, p += pitch) c += is_ink(*p, thr, light);
    col[(size_t)b * W + x] = (uint16_t)c;                 // <= SEG_MAX_DIM
  }
}

// The gap of one band for aocr_segment_page_spaced (include/aocr.h, step 5): sh.flag is staged.  The raw runs (find_runs with gapmin 1), the
// histogram of their clipped gaps in LDS (integer atomics: exact), then wave 0 alone: Otsu's split, the two occupied bins around it, the
// decision and the spacing row.  Every thread returns the gap; sh.flag is left as it was.
__device__ __forceinline__ int band_gap(RunsShared& sh, int W, int h, const aocr_spacing_params& sp, int32_t* __restrict__ row) {
  __shared__ uint32_t ghist[256];
  __shared__ int gap_sh;
  const int K = find_runs(sh, W, 1, 1, [](int, int, int) {});              // sh.s / sh.e: the raw runs
  if (threadIdx.x < 256) ghist[threadIdx.x] = 0;
  __syncthreads();
  const int lo = max(1, h * sp.lo_percent / 100), hi = max(lo, h * sp.hi_percent / 100), clip = min(hi, 255);
  for (int j = 1 + (int)threadIdx.x; j < K; j += SEG_THREADS) atomicAdd(&ghist[min((int)sh.s[j] - (int)sh.e[j - 1], clip)], 1u);
  __syncthreads();
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x, m = max(K - 1, 0);
    long long hh[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) hh[k] = ghist[4 * lane + k];
    const int t = otsu_wave(hh, lane);
    int a = -1, c = SEG_NONE;                                              // the largest occupied bin <= t, the smallest one > t
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int v = 4 * lane + k;
      if (hh[k] > 0) { if (v <= t) a = max(a, v); else c = min(c, v); }
    }
    for (int d = 32; d >= 1; d >>= 1) { a = max(a, __shfl_xor(a, d)); c = min(c, __shfl_xor(c, d)); }
    if (t < 0) a = c = 0;
    if (lane == 0) {
      const int flag = m < sp.min_gaps ? 1 : t < 0 ? 2 : c * 100 < a * sp.ratio_percent ? 3 : 0;
      const int est = flag == 0 ? (a + c + 1) >> 1 : max(1, h * sp.default_percent / 100);
      const int gap = min(max(est, lo), hi);
      gap_sh = gap;
      if (row) {
        row[0] = gap; row[1] = flag + (gap != est ? 4 : 0); row[2] = m; row[3] = a; row[4] = c; row[5] = h; row[6] = 0; row[7] = 0;
      }
    }
  }
  __syncthreads();
  return gap_sh;
}

// SPACED: the gap of every band is estimated from the band (band_gap) instead of being word_gap
template <bool SPACED>
__device__ __forceinline__ void words_body(const uint16_t* __restrict__ col, int W, int word_gap, int min_word_w, int max_bands, int cap,
                                           const int32_t* __restrict__ hdr, uint32_t* __restrict__ words, int32_t* __restrict__ wcount,
                                           const uint32_t* __restrict__ bands, const aocr_spacing_params& sp, int max_lines,
                                           int32_t* __restrict__ spacing) {
  __shared__ RunsShared sh;
  const int nb = min(hdr[1], max_bands);
  int gapmin = word_gap == 0 ? SEG_NONE : word_gap;                        // 0: nothing splits a band
  for (int b = blockIdx.x; b < nb; b += gridDim.x) {
    for (int x = threadIdx.x; x < W; x += SEG_THREADS) sh.flag[x] = col[(size_t)b * W + x] >= 1;
    __syncthreads();
    if constexpr (SPACED) {
      const uint32_t yy = bands[b];
      gapmin = band_gap(sh, W, (int)(yy >> 16) - (int)(yy & 0xffffu), sp, spacing && b < max_lines ? spacing + (size_t)b * 8 : nullptr);
    }
    uint32_t* out = words + (size_t)b * cap;
    const int n = find_runs(sh, W, gapmin, min_word_w, [&](int k, int x0, int x1) { if (k < cap) out[k] = (uint32_t)x0 | ((uint32_t)x1 << 16); });
    if (threadIdx.x == 0) wcount[b] = n;
    __syncthreads();
  }
}

__global__ __launch_bounds__(SEG_THREADS) void words_kernel(const uint16_t* __restrict__ col, int W, int word_gap, int min_word_w, int max_bands,
                                                            int cap, const int32_t* __restrict__ hdr, uint32_t* __restrict__ words,
                                                            int32_t* __restrict__ wcount) {
  words_body<false>(col, W, word_gap, min_word_w, max_bands, cap, hdr, words, wcount, nullptr, aocr_spacing_params{}, 0, nullptr);
}

__global__ __launch_bounds__(SEG_THREADS) void words_spaced_kernel(const uint16_t* __restrict__ col, int W, aocr_spacing_params sp, int min_word_w,
                                                                   int max_bands, int cap, const int32_t* __restrict__ hdr,
                                                                   const uint32_t* __restrict__ bands, uint32_t* __restrict__ words,
                                                                   int32_t* __restrict__ wcount, int max_lines, int32_t* __restrict__ spacing) {
  words_body<true>(col, W, 1, min_word_w, max_bands, cap, hdr, words, wcount, bands, sp, max_lines, spacing);
}

__global__ __launch_bounds__(SEG_THREADS) void offsets_kernel(const int32_t* __restrict__ wcount, int max_bands, int fixed, int32_t* __restrict__ woffset,
                                                              int32_t* __restrict__ hdr, int32_t* __restrict__ counts) {
  __shared__ int wtot[SEG_WAVES];
  const int nb = min(hdr[1], max_bands);
  const int ch = (nb + SEG_THREADS - 1) / SEG_THREADS;
  const int lo = min(nb, (int)threadIdx.x * ch), hi = min(nb, lo + ch);
  int sum = 0;
  for (int b = lo; b < hi; ++b) sum += wcount[b];
  int total;
  int o = block_scan_excl<false>(sum, 0, [](int a, int b) { return a + b; }, wtot, &total);
  for (int b = lo; b < hi; ++b) { woffset[b] = o; o += wcount[b]; }
  if (threadIdx.x == 0) { hdr[2] = total; counts[0] = total; counts[1] = nb; counts[2] = ink_thr(fixed, hdr); counts[3] = 0; }
}

__global__ __launch_bounds__(256) void emit_kernel(const int32_t* __restrict__ hdr, const uint32_t* __restrict__ bands,
                                                   const int32_t* __restrict__ woffset, const uint32_t* __restrict__ words,
                                                   const uint16_t* __restrict__ col, int H, int W, int max_bands, int cap, int pad_x, int pad_y,
                                                   int max_boxes, aocr_box* __restrict__ boxes) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nb = min(hdr[1], max_bands);
  if (i >= min(hdr[2], max_boxes)) return;
  int lo = 0, hi = nb - 1;                                 // the last band whose offset is <= i (empty bands share their successor's offset)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (woffset[mid] <= i) lo = mid; else hi = mid - 1;
  }
  const int b = lo, j = i - woffset[b];
  if (j < 0 || j >= cap) return;                           // cannot happen: j < the band's word count and j <= i < max_boxes
  const uint32_t xx = words[(size_t)b * cap + j], yy = bands[b];
  const int x0 = (int)(xx & 0xffffu), x1 = (int)(xx >> 16), y0 = (int)(yy & 0xffffu), y1 = (int)(yy >> 16);
  int ink = 0;
  for (int x = x0 + lane; x < x1; x += 64) ink += col[(size_t)b * W + x];
  ink = wave_sum(ink);
  if (lane == 0) {
    aocr_box bx;
    bx.x0 = max(0, x0 - pad_x); bx.y0 = max(0, y0 - pad_y); bx.x1 = min(W, x1 + pad_x); bx.y1 = min(H, y1 + pad_y);
    bx.line = b; bx.ink = ink;
    boxes[i] = bx;
  }
}

}  // namespace

size_t segment_scratch_bytes(int H, int W, int max_boxes) { return seg_layout(H, W, max_boxes).total; }

// steps 1-2 with Otsu: the histogram into hist (256 words), the threshold into hdr[0].  aocr_estimate_skew (skew.hip) enqueues the same three
void otsu_threshold(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, uint32_t* hist, int32_t* hdr) {
  (void)hipMemsetAsync(hist, 0, 256 * sizeof(uint32_t), s);
  hipLaunchKernelGGL(hist_kernel, dim3(std::min(cdiv(H, 4), 2048)), dim3(256), 0, s, page, pitch, H, W, hist);
  hipLaunchKernelGGL(otsu_kernel, dim3(1), dim3(64), 0, s, hist, hdr);
}

// spacing == nullptr: aocr_segment_page; else aocr_segment_page_spaced, whose words launch estimates a gap per band
static void segment_launches(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_segment_params& p,
                             const aocr_spacing_params* spacing, void* scratch, int max_boxes, aocr_box* boxes, int32_t* counts, int max_lines,
                             int32_t* spacing_rows) {
  const SegLayout l = seg_layout(H, W, max_boxes);
  uint32_t* hist = scratch_at<uint32_t>(scratch, l.hist);
  int32_t* hdr = scratch_at<int32_t>(scratch, l.hdr);
  int32_t* row_ink = scratch_at<int32_t>(scratch, l.row_ink);
  uint32_t* bands = scratch_at<uint32_t>(scratch, l.bands);
  int32_t* wcount = scratch_at<int32_t>(scratch, l.wcount);
  int32_t* woffset = scratch_at<int32_t>(scratch, l.woffset);
  uint16_t* col = scratch_at<uint16_t>(scratch, l.col);
  uint32_t* words = scratch_at<uint32_t>(scratch, l.words);
  const int light = p.light_text ? 1 : 0, fixed = p.threshold;    // >= 0: no histogram, no Otsu launch, hdr[0] unused
  const int row_blocks = std::min(cdiv(H, 4), 2048);
  page_threshold(s, page, pitch, H, W, fixed, hist, hdr);
  hipLaunchKernelGGL(rowprof_kernel, dim3(row_blocks), dim3(256), 0, s, page, pitch, H, W, light, fixed, hdr, row_ink);
  hipLaunchKernelGGL(bands_kernel, dim3(1), dim3(SEG_THREADS), 0, s, row_ink, H, p.min_row_ink,
                     std::min(p.merge_gap, SEG_MAX_DIM), p.min_line_h, bands, hdr);
  hipLaunchKernelGGL(colprof_kernel, dim3(cdiv(W, 256), std::min(l.max_bands, 128)), dim3(256), 0, s, page, pitch, W, light, fixed, l.max_bands,
                     hdr, bands, col);
  if (spacing)
    hipLaunchKernelGGL(words_spaced_kernel, dim3(std::min(l.max_bands, 128)), dim3(SEG_THREADS), 0, s, col, W, *spacing, p.min_word_w, l.max_bands,
                       l.cap, hdr, bands, words, wcount, max_lines, spacing_rows);
  else
    hipLaunchKernelGGL(words_kernel, dim3(std::min(l.max_bands, 128)), dim3(SEG_THREADS), 0, s, col, W, p.word_gap, p.min_word_w, l.max_bands,
                       l.cap, hdr, words, wcount);
  hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(SEG_THREADS), 0, s, wcount, l.max_bands, fixed, woffset, hdr, counts);
  hipLaunchKernelGGL(emit_kernel, dim3(cdiv(max_boxes, 4)), dim3(256), 0, s, hdr, bands, woffset, words, col, H, W, l.max_bands, l.cap, p.pad_x,
                     p.pad_y, max_boxes, boxes);
}

void segment_page(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_segment_params& p, void* scratch, int max_boxes,
                  aocr_box* boxes, int32_t* counts) {
  segment_launches(s, page, pitch, H, W, p, nullptr, scratch, max_boxes, boxes, counts, 0, nullptr);
}

void segment_page_spaced(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_segment_params& p,
                         const aocr_spacing_params& spacing, void* scratch, int max_boxes, aocr_box* boxes, int32_t* counts, int max_lines,
                         int32_t* spacing_rows) {
  segment_launches(s, page, pitch, H, W, p, &spacing, scratch, max_boxes, boxes, counts, max_lines, spacing_rows);
}

}  // namespace aocr
