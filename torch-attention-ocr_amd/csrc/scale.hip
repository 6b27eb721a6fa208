// scale.hip -- page scale normalisation (include/aocr.h: aocr_estimate_glyph_size, aocr_resize_page), the stage between aocr_flatten_page and
// aocr_clean_page: every later stage counts in pixels of text at 300 dpi, and nothing before this knew how large the text on a page is.
// aocr_estimate_glyph_size takes the median of min(w, h) over the tight boxes of the components that can be glyphs (the labels and boxes
// come from components.hip's launches, the Otsu threshold from segment.hip's); aocr_resize_page resamples the page by exact pixel areas to
// any size.  Integer arithmetic only: tests/scale_ref.py, numpy int64, matches bit for bit.
//
// Launches of one aocr_estimate_glyph_size, all on the caller's stream, intermediates in the caller's scratch:
//   label_components   of components.hip: the canonical labels (into the scratch), every root's record (area, min x, max x, max y; its
//                      min y is its own row) and [threshold, ink, components, 0].
//   memset             of the 1024 bins.
//   glyph_hist_kernel  a thread walks GLYPH_ROWS rows of one column of the labels (quad_sheet_kernel's walk); a root (label == its own
//                      index) whose box qualifies adds one to bin a - 1 of the workgroup's histogram in LDS.  A workgroup that saw a
//                      qualifying root adds its non-zero bins to the global histogram with integer atomicAdd; the others leave at once.
//   glyph_final_kernel one wave: lane l holds bins 16 l .. 16 l + 15 in registers, a wave prefix of the lane sums gives n and every lane's
//                      offset, and the lane whose bins contain a quartile's index finds the bin.  Lane 0 writes the other five words.
// Integer sums do not depend on their order: the words do not depend on the launch geometry or on the order of the atomics.
//
// aocr_resize_page is one launch: resize_kernel, one wave per output row (wave_store_row of page_common.h).  With a = X*W, b = a + W the source columns of output pixel X are a / Wo ..
// (b - 1) / Wo: a lane takes one 32-bit division for its first pixel and then steps quotient and remainder by W / Wo and W % Wo.  The row's
// source rows and their weights are the same for the whole wave (scalar registers).  Per pixel: for each source column the weighted
// column sum over the rows (below 2^22, 32 bits), times the column's weight into a 64-bit sum (one v_mad_u64_u32), then the division by H*W.
// The divisor is the same for the whole launch and the numerator n = S + H*W/2 is below 2^35, so with m = ceil(2^64 / d) and
// e = m*d - 2^64 < d <= 2^26, floor(n*m / 2^64) = floor(n/d + n*e / (d * 2^64)) = floor(n/d) because n*e < 2^61: the error term
// adds less than 1/d.  d = 1 (a page of one pixel) has no such m and takes n itself.
#include <algorithm>
#include "ops.h"
#include "page_common.h"

namespace aocr {

namespace {

constexpr int GLYPH_ROWS = 8;                  // rows of one thread of the walk
constexpr int GLYPH_THREADS = 256;
constexpr int GLYPH_BINS = GLYPH_SIZE_MAX;     // bin a - 1 counts the components of size a

struct GlyphLayout {                           // byte offsets into scratch_dev
  size_t cc, labels, hist, hdr, total;
};

GlyphLayout glyph_layout(int H, int W) {
  GlyphLayout l;
  ScratchCursor c;
  l.cc = c.take(components_scratch_bytes(H, W));
  l.labels = c.take((size_t)H * W * sizeof(int32_t));
  l.hist = c.take(GLYPH_BINS * sizeof(uint32_t));
  l.hdr = c.take(64);                                                  // info (4 words, padded to 64 bytes)
  l.total = c.total();
  return l;
}

__global__ __launch_bounds__(GLYPH_THREADS) void glyph_hist_kernel(const int32_t* __restrict__ labels, int H, int W, const int32_t* __restrict__ rec,
                                                                   int sw, int min_size, int max_size, int max_aspect, uint32_t* hist) {
  __shared__ uint32_t bins[GLYPH_BINS];
  __shared__ int any;
  for (int i = threadIdx.x; i < GLYPH_BINS; i += GLYPH_THREADS) bins[i] = 0;
  if (threadIdx.x == 0) any = 0;
  __syncthreads();
  const int x = blockIdx.x * GLYPH_THREADS + threadIdx.x;
  const int y0 = blockIdx.y * GLYPH_ROWS, y1 = min(H, y0 + GLYPH_ROWS);
  if (x < W)
    for (int y = y0; y < y1; ++y) {
      const int i = y * W + x;
      if (labels[i] != i) continue;                        // paper (-1), or not the first pixel of its component
      const int32_t* r = rec + 4 * ((size_t)y * sw + (x >> 1));
      const int w = r[2] - r[1] + 1, h = r[3] - y + 1;
      const int a = min(w, h), b = max(w, h);
      if (a < min_size || a > max_size || (int64_t)b > (int64_t)max_aspect * a) continue;       // max_size <= GLYPH_BINS
      atomicAdd(&bins[a - 1], 1u);
      any = 1;
    }
  __syncthreads();
  if (!any) return;
  for (int i = threadIdx.x; i < GLYPH_BINS; i += GLYPH_THREADS)
    if (const uint32_t c = bins[i]) atomicAdd(&hist[i], c);
}

__global__ __launch_bounds__(64) void glyph_final_kernel(const uint32_t* __restrict__ hist, const int32_t* __restrict__ info,
                                                         int32_t* __restrict__ glyph) {
  constexpr int PER = GLYPH_BINS / 64;
  static_assert(PER * 64 == GLYPH_BINS, "a lane holds a whole number of bins");
  const int lane = threadIdx.x;
  int c[PER];                                              // a page has at most 2^25 components: n and 3 * (n - 1) fit in 32 bits
  int mine = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) { c[j] = (int)hist[lane * PER + j]; mine += c[j]; }
  int incl = mine;
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(incl, d);
    if (lane >= d) incl += o;
  }
  const int n = __shfl(incl, 63), before = incl - mine;
  if (lane == 0) {
    if (n == 0) { glyph[0] = 0; glyph[1] = 0; glyph[2] = 0; }
    glyph[3] = n; glyph[4] = info[2]; glyph[5] = info[0]; glyph[6] = info[1]; glyph[7] = 0;
  }
  if (n == 0) return;
  for (int k = 1; k <= 3; ++k) {
    const int idx = k * (n - 1) / 4;
    if (idx < before || idx >= incl) continue;             // exactly one lane holds the index
    int run = before, s = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {                        // the smallest size whose running sum exceeds the index
      run += c[j];
      if (s == 0 && run > idx) s = lane * PER + j + 1;
    }
    glyph[k == 2 ? 0 : k == 1 ? 1 : 2] = s;
  }
}

struct ResizeArgs {
  int H, W, Ho, Wo;
  int dqx, drx;                                // W / Wo, W % Wo
  uint32_t half;                               // H*W / 2
  uint64_t recip;                              // ceil(2^64 / (H*W)); unused when H*W == 1
};

__global__ __launch_bounds__(256) void resize_kernel(const uint8_t* __restrict__ page, int64_t pitch, ResizeArgs k, uint8_t* __restrict__ out,
                                                     int64_t out_pitch) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int H = k.H, W = k.W, Ho = k.Ho, Wo = k.Wo;
  const bool one = H * W == 1;
  for (int Yv = blockIdx.x * 4 + wave; Yv < Ho; Yv += gridDim.x * 4) {
    const int Y = __builtin_amdgcn_readfirstlane(Yv);      // the same in every lane: the row's bounds and weights stay in scalar registers
    const int ya = Y * H, yb = ya + H;                     // the output row covers [ya, yb) in units of 1 / Ho source rows; <= 2^28
    const int sy0 = ya / Ho, sy1 = (yb - 1) / Ho;          // its source rows, sy1 <= H - 1; at most 9
    const uint8_t* row0 = page + (int64_t)sy0 * pitch;
    // the pixel X whose left edge X*W is q*Wo + r; steps q and r to those of X + 1
    auto px = [&](int X, int& q, int& r) -> uint32_t {
      const int a = X * W, b = a + W;
      int q2 = q + k.dqx, r2 = r + k.drx;
      if (r2 >= Wo) { r2 -= Wo; ++q2; }
      const int last = r2 > 0 ? q2 : q2 - 1;               // (b - 1) / Wo <= W - 1: every read is inside the page
      uint64_t S = 0;
      int xe = a - r;                                      // x * Wo
      for (int x = q; x <= last; ++x, xe += Wo) {
        const uint32_t wx = (uint32_t)(min(xe + Wo, b) - max(xe, a));
        const uint8_t* p = row0 + x;
        uint32_t v = 0;
        int ye = sy0 * Ho;
        for (int y = sy0; y <= sy1; ++y, ye += Ho, p += pitch) v += (uint32_t)(min(ye + Ho, yb) - max(ye, ya)) * (uint32_t)*p;   // < 2^22
        S += (uint64_t)wx * v;
      }
      q = q2; r = r2;
      const uint64_t n = S + k.half;                       // < 2^35
      return (uint32_t)(one ? n : __umul64hi(n, k.recip));
    };
    auto px4 = [&](int X, int& q, int& r) -> uint32_t {
      const uint32_t p0 = px(X, q, r), p1 = px(X + 1, q, r), p2 = px(X + 2, q, r), p3 = px(X + 3, q, r);
      return p0 | (p1 << 8) | (p2 << 16) | (p3 << 24);
    };
    auto start = [&](int X, int& q, int& r) { const int a = X * W; q = a / Wo; r = a - q * Wo; };
    auto px1 = [&](int X) -> uint32_t { int q, r; start(X, q, r); return px(X, q, r); };
    auto px16 = [&](int X) -> uint4 {                      // one division for the 16 pixels of a store
      int q, r;
      start(X, q, r);
      uint4 v;
      v.x = px4(X, q, r); v.y = px4(X + 4, q, r); v.z = px4(X + 8, q, r); v.w = px4(X + 12, q, r);
      return v;
    };
    wave_store_row(out + (int64_t)Y * out_pitch, Wo, lane, px1, px16);
  }
}

}  // namespace

size_t glyph_scratch_bytes(int H, int W) { return glyph_layout(H, W).total; }

void estimate_glyph_size(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_glyph_params& p, void* scratch,
                         int32_t* glyph) {
  const GlyphLayout l = glyph_layout(H, W);
  void* cc = scratch_at<char>(scratch, l.cc);
  int32_t* labels = scratch_at<int32_t>(scratch, l.labels);
  uint32_t* hist = scratch_at<uint32_t>(scratch, l.hist);
  int32_t* info = scratch_at<int32_t>(scratch, l.hdr);
  label_components(s, page, pitch, H, W, p.threshold, p.light_text, p.connectivity, cc, labels, W, 1, nullptr, info);
  const ComponentAreas a = component_areas(H, W, cc);
  (void)hipMemsetAsync(hist, 0, GLYPH_BINS * sizeof(uint32_t), s);
  hipLaunchKernelGGL(glyph_hist_kernel, dim3(cdiv(W, GLYPH_THREADS), cdiv(H, GLYPH_ROWS)), dim3(GLYPH_THREADS), 0, s, labels, H, W, a.rec, a.sw,
                     p.min_size, p.max_size, p.max_aspect, hist);
  hipLaunchKernelGGL(glyph_final_kernel, dim3(1), dim3(64), 0, s, hist, info, glyph);
}

void resize_page(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, uint8_t* out, int64_t out_pitch, int Ho, int Wo) {
  ResizeArgs k;
  k.H = H; k.W = W; k.Ho = Ho; k.Wo = Wo;
  k.dqx = W / Wo; k.drx = W % Wo;
  const uint64_t d = (uint64_t)H * W;
  k.half = (uint32_t)(d / 2);
  k.recip = d > 1 ? ~(uint64_t)0 / d + 1 : 0;              // ceil(2^64 / d): floor((2^64 - 1) / d) + 1, for a power of two as for any other d
  hipLaunchKernelGGL(resize_kernel, dim3(std::min(cdiv(Ho, 4), 2048)), dim3(256), 0, s, page, pitch, k, out, out_pitch);
}

}  // namespace aocr
