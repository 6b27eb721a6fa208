// panels.hip -- reversed-out panels (include/aocr.h: aocr_invert_panels): a table header row, a section bar or a sidebar box is light text
// on a dark slab, one big connected component of the page's ink that holds no readable crop.  The slab is found among the components of
// components.hip (a wide and high tight box, a large share of its row-convex hull filled, something written inside), and the bytes inside
// its row spans are replaced by 255 - v, so that the words on it are dark text on light paper like the rest of the page.  Integer
// arithmetic only (the Otsu threshold, when asked for, comes from segment.hip's otsu_threshold); every result is a function of the page
// and the params: tests/panels_ref.py, loops over candidates and rows, matches exactly.
//
// Launches of one aocr_invert_panels, all on the caller's stream, intermediates in the caller's scratch:
//   label_components   of components.hip: the canonical labels (into the scratch), every root's record (area, min x, max x, max y; its
//                      min y is its own row) and [threshold, ink, components, 0].
//   pn_count_kernel    one wave per row segment of PN_SEG_W columns: a root (label == its own index) whose box passes min_w / min_h is a
//                      candidate; writes the number of candidates of the segment.
//   pn_scan_kernel     one workgroup: the exclusive prefix of the segment counts in raster order, in place (cc_scan_kernel's walk); the
//                      candidates found and the candidates examined.
//   pn_pick_kernel     pn_count_kernel's walk again: the k-th candidate in raster order of the roots, which is ascending label order,
//                      writes record k (the eight words of a panels_dev row; hull and accepted 0) when k < max_panels.
//   pn_rows_kernel     one workgroup, one thread per record: the exclusive prefix of the box heights, so that (candidate, row) pairs have
//                      one running index.
//   pn_spans_kernel    one wave per (candidate, row), a fixed grid that strides the running index: the lanes stride the box row of the
//                      label plane, a wave min / max gives lo and hi, lane 0 stores the span and adds hi - lo to the record's hull.
//   pn_judge_kernel    one workgroup, one thread per record: the two percent tests in 64 bits, the panels_dev row, and the counts from
//                      block sums (no atomics: the sum of the hulls is formed in 64 bits and capped).
//   pn_copy_kernel     one wave per row: the page to out_dev, 16 bytes per lane over the aligned middle, bytes at the ragged ends.
//   pn_invert_kernel   pn_spans_kernel's grid again, after the copy on the same stream: 255 - page over the span of every (accepted
//                      candidate, row), the same store walk.  Its source is the page, never out_dev, so spans that overlap store equal bytes.
// No workgroup waits on another.  Every loop is bounded by a constant or by the page: the row walks by W / 16 / 64 + 2 turns, the label
// walk by cdiv(W, 64), the search of a running index by log2(PN_MAX) = 10 turns, the strides by max_panels * H / the grid.  Integer sums,
// minima and maxima only: no result depends on the launch geometry or on the order of the atomics.
#include <cstddef>
#include "ops.h"
#include "page_common.h"
#include "runs.h"

namespace aocr {

namespace {

constexpr int PN_SEG_W = 64;                   // columns of a row segment of the candidate pick: one wave, its candidates are one ballot
constexpr int PN_THREADS = 256;
constexpr int PN_WAVES = PN_THREADS / 64;      // row segments (pick), rows (copy) or (candidate, row) pairs (spans, invert) of a workgroup at a time
constexpr int PN_MAX = 1024;                   // max_panels
constexpr int PN_GRID = 1024;                  // workgroups of the spans and invert kernels, whatever the page
constexpr int PN_BIG = 1 << 30;
static_assert(PN_SEG_W == 64, "a row segment is one wave");
static_assert(PN_MAX == SEG_THREADS, "pn_rows_kernel and pn_judge_kernel: one thread per record, one workgroup");

enum { HDR_INFO = 0, HDR_FOUND = 4, HDR_EXAM = 5, HDR_ROWS = 6, HDR_WORDS = 64 };     // words of hdr; hdr[0..3] is label_components' info
enum { REC_X0 = 0, REC_Y0, REC_X1, REC_Y1, REC_LABEL, REC_AREA, REC_HULL, REC_OK, REC_WORDS };      // a record: the words of a panels_dev row

struct PanelLayout {                           // byte offsets into scratch_dev
  size_t cc, labels, hdr, segs, recs, rowoff, spans, total;
  int ntx;
};

PanelLayout panel_layout(int H, int W, int max_panels) {
  PanelLayout l;
  ScratchCursor c;
  l.ntx = cdiv(W, PN_SEG_W);
  l.cc = c.take(components_scratch_bytes(H, W));
  l.labels = c.take((size_t)H * W * sizeof(int32_t));
  l.hdr = c.take(HDR_WORDS * sizeof(int32_t));
  l.segs = c.take((size_t)H * l.ntx * sizeof(int32_t));
  l.recs = c.take((size_t)PN_MAX * REC_WORDS * sizeof(int32_t));
  l.rowoff = c.take((size_t)PN_MAX * sizeof(int32_t));
  l.spans = c.take((size_t)max_panels * H * sizeof(int2));             // a candidate's box has at most H rows
  l.total = c.total();
  return l;
}

__device__ __forceinline__ uint64_t below(int lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }   // the bits under `lane`

__device__ __forceinline__ int wave_min_i(int v) {
  for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d));
  return v;
}

__device__ __forceinline__ int wave_max_i(int v) {
  for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
  return v;
}

// ---- the candidate pick -----------------------------------------------------------------------------------------------------------------------

// the wave's lane looks at column x of row y: is it the first pixel of a component whose tight box is at least min_w x min_h?
__device__ __forceinline__ bool is_candidate(const int32_t* __restrict__ labels, int W, const int32_t* __restrict__ rec, int sw, int x, int y, int min_w,
                                             int min_h, int* label) {
  const int l = x < W ? labels[(int64_t)y * W + x] : -1;
  *label = l;
  if (l < 0 || l != y * W + x) return false;
  const int32_t* s = rec + 4 * ((size_t)y * sw + (x >> 1));            // area, min x, max x, max y
  return s[2] - s[1] + 1 >= min_w && s[3] - y + 1 >= min_h;
}

__global__ __launch_bounds__(PN_THREADS) void pn_count_kernel(const int32_t* __restrict__ labels, int H, int W, const int32_t* __restrict__ rec, int sw,
                                                              int min_w, int min_h, int32_t* __restrict__ segs, int ntx) {
  const int lane = threadIdx.x & 63;
  const int tx = blockIdx.x, y = blockIdx.y * PN_WAVES + (threadIdx.x >> 6);
  if (y >= H) return;                                    // the whole wave
  int l;
  const uint64_t m = __ballot(is_candidate(labels, W, rec, sw, tx * PN_SEG_W + lane, y, min_w, min_h, &l));
  if (lane == 0) segs[(size_t)y * ntx + tx] = __popcll(m);
}

__global__ __launch_bounds__(SEG_THREADS) void pn_scan_kernel(int32_t* __restrict__ segs, int n, int max_panels, int32_t* __restrict__ hdr) {
  __shared__ int wtot[SEG_WAVES];
  const int ch = (n + SEG_THREADS - 1) / SEG_THREADS;
  const int lo = min(n, (int)threadIdx.x * ch), hi = min(n, lo + ch);
  int sum = 0;
  for (int i = lo; i < hi; ++i) sum += segs[i];
  int total;
  int o = block_scan_excl<false>(sum, 0, [](int a, int b) { return a + b; }, wtot, &total);
  for (int i = lo; i < hi; ++i) { const int c = segs[i]; segs[i] = o; o += c; }
  if (threadIdx.x == 0) { hdr[HDR_FOUND] = total; hdr[HDR_EXAM] = min(total, max_panels); }
}

__global__ __launch_bounds__(PN_THREADS) void pn_pick_kernel(const int32_t* __restrict__ labels, int H, int W, const int32_t* __restrict__ rec, int sw,
                                                             int min_w, int min_h, const int32_t* __restrict__ segs, int ntx, int max_panels,
                                                             int32_t* __restrict__ recs) {
  const int lane = threadIdx.x & 63;
  const int tx = blockIdx.x, y = blockIdx.y * PN_WAVES + (threadIdx.x >> 6);
  if (y >= H) return;                                    // the whole wave
  const int x = tx * PN_SEG_W + lane;
  int l;
  const bool cand = is_candidate(labels, W, rec, sw, x, y, min_w, min_h, &l);
  const uint64_t m = __ballot(cand);
  if (!cand) return;
  const int k = segs[(size_t)y * ntx + tx] + __popcll(m & below(lane));
  if (k >= max_panels) return;
  const int32_t* s = rec + 4 * ((size_t)y * sw + (x >> 1));
  int32_t* r = recs + (size_t)k * REC_WORDS;
  r[REC_X0] = s[1]; r[REC_Y0] = y; r[REC_X1] = s[2] + 1; r[REC_Y1] = s[3] + 1; r[REC_LABEL] = l; r[REC_AREA] = s[0]; r[REC_HULL] = 0; r[REC_OK] = 0;
}

// the running index of (candidate k, row y) is rowoff[k] + y - y0; hdr[HDR_ROWS] is their number, at most max_panels * H <= 2^24
__global__ __launch_bounds__(SEG_THREADS) void pn_rows_kernel(const int32_t* __restrict__ recs, int32_t* __restrict__ rowoff, int32_t* __restrict__ hdr) {
  __shared__ int wtot[SEG_WAVES];
  const int k = threadIdx.x, exam = hdr[HDR_EXAM];
  const int h = k < exam ? recs[(size_t)k * REC_WORDS + REC_Y1] - recs[(size_t)k * REC_WORDS + REC_Y0] : 0;
  int total;
  rowoff[k] = block_scan_excl<false>(h, 0, [](int a, int b) { return a + b; }, wtot, &total);
  if (k == 0) hdr[HDR_ROWS] = total;
}

// ---- the spans ----------------------------------------------------------------------------------------------------------------------------------

// the candidate of the running index i < hdr[HDR_ROWS]: the last k < exam with rowoff[k] <= i (every box has a row, so rowoff strictly
// increases over the examined records and rowoff[0] == 0)
__device__ __forceinline__ int candidate_of(const int32_t* __restrict__ rowoff, int exam, int i) {
  int a = 0, b = exam;
  while (b - a > 1) {                                    // at most log2(PN_MAX) turns
    const int m = (a + b) >> 1;
    if (rowoff[m] <= i) a = m; else b = m;
  }
  return a;
}

__global__ __launch_bounds__(PN_THREADS) void pn_spans_kernel(const int32_t* __restrict__ labels, int W, int32_t* recs, const int32_t* __restrict__ rowoff,
                                                              const int32_t* __restrict__ hdr, int2* __restrict__ spans) {
  const int lane = threadIdx.x & 63;
  const int total = hdr[HDR_ROWS], exam = hdr[HDR_EXAM];
  for (int i = blockIdx.x * PN_WAVES + (threadIdx.x >> 6); i < total; i += gridDim.x * PN_WAVES) {       // the same for the whole wave
    const int k = candidate_of(rowoff, exam, i);
    int32_t* r = recs + (size_t)k * REC_WORDS;
    const int x0 = r[REC_X0], x1 = r[REC_X1], label = r[REC_LABEL];
    const int y = r[REC_Y0] + i - rowoff[k];
    const int32_t* __restrict__ row = labels + (int64_t)y * W;
    int lo = PN_BIG, hi = 0;
    for (int x = x0 + lane; x < x1; x += 64)
      if (row[x] == label) { lo = min(lo, x); hi = max(hi, x + 1); }
    lo = wave_min_i(lo);
    hi = wave_max_i(hi);                                 // a component has a pixel in every row of its box: lo < hi
    if (lane == 0) {
      spans[i] = make_int2(lo, hi);
      atomicAdd(&r[REC_HULL], hi - lo);
    }
  }
}

// ---- the judge ----------------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(SEG_THREADS) void pn_judge_kernel(int32_t* __restrict__ recs, const int32_t* __restrict__ hdr, int fill_percent,
                                                               int min_inside_percent, int32_t* __restrict__ panels, int32_t* __restrict__ counts) {
  __shared__ int n_w[SEG_WAVES];
  __shared__ long long hull_w[SEG_WAVES];
  const int k = threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int exam = hdr[HDR_EXAM];
  int ok = 0;
  long long hull = 0;
  if (k < exam) {
    int32_t* r = recs + (size_t)k * REC_WORDS;
    const long long area = r[REC_AREA], h = r[REC_HULL];
    ok = area * 100 >= (long long)fill_percent * h && (h - area) * 100 >= (long long)min_inside_percent * h;
    r[REC_OK] = ok;
    if (ok) hull = h;
    if (panels) {
#pragma unroll
      for (int j = 0; j < REC_OK; ++j) panels[(size_t)k * REC_WORDS + j] = r[j];
      panels[(size_t)k * REC_WORDS + REC_OK] = ok;
    }
  }
  const int n = wave_sum(ok);
  hull = wave_sum(hull);
  if (lane == 0) { n_w[wave] = n; hull_w[wave] = hull; }
  __syncthreads();
  if (k == 0) {
    int inverted = 0;
    long long sum = 0;
    for (int w = 0; w < SEG_WAVES; ++w) { inverted += n_w[w]; sum += hull_w[w]; }
    counts[0] = hdr[HDR_INFO + 2];
    counts[1] = hdr[HDR_FOUND];
    counts[2] = exam;
    counts[3] = inverted;
    counts[4] = hdr[HDR_INFO + 0];
    counts[5] = hdr[HDR_INFO + 1];
    counts[6] = (int32_t)(sum < 0x7fffffffll ? sum : 0x7fffffffll);      // nested rings can have hulls that add up past 2^31: capped
    counts[7] = 0;
  }
}

// ---- the apply ----------------------------------------------------------------------------------------------------------------------------------

// columns x .. x + 15 of src, which need not be aligned like the output
__device__ __forceinline__ uint4 load16(const uint8_t* __restrict__ src, int x) {
  if ((((uintptr_t)(src + x)) & 15u) == 0) return *reinterpret_cast<const uint4*>(src + x);
  uint32_t w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    w[j] = (uint32_t)src[x + 4 * j] | ((uint32_t)src[x + 4 * j + 1] << 8) | ((uint32_t)src[x + 4 * j + 2] << 16) | ((uint32_t)src[x + 4 * j + 3] << 24);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(PN_THREADS) void pn_copy_kernel(const uint8_t* __restrict__ page, int64_t pitch, int H, int W, uint8_t* __restrict__ out,
                                                             int64_t out_pitch) {
  const int lane = threadIdx.x & 63;
  const int y = blockIdx.x * PN_WAVES + (threadIdx.x >> 6);
  if (y >= H) return;
  const uint8_t* __restrict__ src = page + (int64_t)y * pitch;
  wave_store_row(out + (int64_t)y * out_pitch, W, lane, [&](int x) -> uint32_t { return src[x]; }, [&](int x) -> uint4 { return load16(src, x); });
}

__global__ __launch_bounds__(PN_THREADS) void pn_invert_kernel(const uint8_t* __restrict__ page, int64_t pitch, const int32_t* __restrict__ recs,
                                                               const int32_t* __restrict__ rowoff, const int32_t* __restrict__ hdr,
                                                               const int2* __restrict__ spans, uint8_t* out, int64_t out_pitch) {
  const int lane = threadIdx.x & 63;
  const int total = hdr[HDR_ROWS], exam = hdr[HDR_EXAM];
  for (int i = blockIdx.x * PN_WAVES + (threadIdx.x >> 6); i < total; i += gridDim.x * PN_WAVES) {       // the same for the whole wave
    const int k = candidate_of(rowoff, exam, i);
    const int32_t* r = recs + (size_t)k * REC_WORDS;
    if (!r[REC_OK]) continue;
    const int y = r[REC_Y0] + i - rowoff[k];
    const int2 sp = spans[i];                            // 0 <= lo < hi <= W: columns of pixels of the component
    const uint8_t* __restrict__ src = page + (int64_t)y * pitch + sp.x;
    wave_store_row(out + (int64_t)y * out_pitch + sp.x, sp.y - sp.x, lane, [&](int x) -> uint32_t { return 255u - src[x]; },
                   [&](int x) -> uint4 { const uint4 q = load16(src, x); return make_uint4(~q.x, ~q.y, ~q.z, ~q.w); });
  }
}

}  // namespace

size_t panels_scratch_bytes(int H, int W, int max_panels) { return panel_layout(H, W, max_panels).total; }

void invert_panels(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_panel_params& p, void* scratch, uint8_t* out,
                   int64_t out_pitch, int max_panels, int32_t* panels, int32_t* counts) {
  const PanelLayout l = panel_layout(H, W, max_panels);
  void* cc = scratch_at<void>(scratch, l.cc);
  int32_t* labels = scratch_at<int32_t>(scratch, l.labels);
  int32_t* hdr = scratch_at<int32_t>(scratch, l.hdr);
  int32_t* segs = scratch_at<int32_t>(scratch, l.segs);
  int32_t* recs = scratch_at<int32_t>(scratch, l.recs);
  int32_t* rowoff = scratch_at<int32_t>(scratch, l.rowoff);
  int2* spans = scratch_at<int2>(scratch, l.spans);
  label_components(s, page, pitch, H, W, p.threshold, p.light_text, p.connectivity, cc, labels, W, 1, nullptr, hdr + HDR_INFO);
  const ComponentAreas a = component_areas(H, W, cc);
  const dim3 seg_grid(l.ntx, cdiv(H, PN_WAVES));
  hipLaunchKernelGGL(pn_count_kernel, seg_grid, dim3(PN_THREADS), 0, s, labels, H, W, a.rec, a.sw, p.min_w, p.min_h, segs, l.ntx);
  hipLaunchKernelGGL(pn_scan_kernel, dim3(1), dim3(SEG_THREADS), 0, s, segs, H * l.ntx, max_panels, hdr);
  hipLaunchKernelGGL(pn_pick_kernel, seg_grid, dim3(PN_THREADS), 0, s, labels, H, W, a.rec, a.sw, p.min_w, p.min_h, segs, l.ntx, max_panels, recs);
  hipLaunchKernelGGL(pn_rows_kernel, dim3(1), dim3(SEG_THREADS), 0, s, recs, rowoff, hdr);
  hipLaunchKernelGGL(pn_spans_kernel, dim3(PN_GRID), dim3(PN_THREADS), 0, s, labels, W, recs, rowoff, hdr, spans);
  hipLaunchKernelGGL(pn_judge_kernel, dim3(1), dim3(SEG_THREADS), 0, s, recs, hdr, p.fill_percent, p.min_inside_percent, panels, counts);
  hipLaunchKernelGGL(pn_copy_kernel, dim3(cdiv(H, PN_WAVES)), dim3(PN_THREADS), 0, s, page, pitch, H, W, out, out_pitch);
  hipLaunchKernelGGL(pn_invert_kernel, dim3(PN_GRID), dim3(PN_THREADS), 0, s, page, pitch, recs, rowoff, hdr, spans, out, out_pitch);
}

}  // namespace aocr
