// curl.hip -- page dewarp (include/aocr.h: aocr_estimate_curl, aocr_dewarp_page), the stage between aocr_deskew_page and aocr_segment_page:
// neighbouring column groups are correlated along y to find how far the text lines of one sit below those of the other, the pair shifts
// are chained from the middle group outwards, and every column is resampled by its interpolated shift.  Integer arithmetic only (the Otsu
// threshold, when asked for, comes from segment.hip's otsu_threshold; the strip profiles from skew.hip's strip_profiles), so
// tests/curl_ref.py matches exactly.
//
// Launches of one aocr_estimate_curl, all on the caller's stream, intermediates in the caller's scratch:
//   (Otsu only) otsu_threshold of segment.hip: memset, hist_kernel, otsu_kernel -- what aocr_segment_page enqueues for its steps 1-2.
//   strips_kernel    of skew.hip, through strip_profiles: the one page read, R as uint8 [strip][row].
//   corr_kernel      grid (row chunk, pair): the workgroup adds the strips of its two groups for its CORR_ROWS rows (the second group with
//                    a halo of D rows on either side) into LDS as uint16; a wave takes every fourth shift and sums the products of the
//                    chunk: one uint64 partial per (pair, shift, chunk), and the ink of the chunk per group.  (ng > 1 only.)
//   chain_kernel     one workgroup: the partials of a (pair, shift) are added in chunk order and the scores written, a thread per pair takes
//                    the winner by "larger score, then earlier in 0, -1, +1, -2, +2, ...", thread 0 runs the chain and writes the outputs.
// aocr_dewarp_page is one launch: dewarp_kernel, one wave per output row (wave_store_row of page_common.h); both source rows of a pixel
// are read at the pixel's own column, so the reads of a wave are as coalesced as the writes; a lane takes one division and three shift
// loads for its 16 columns, and the floor division of every pixel is a multiply by a reciprocal.
#include <algorithm>
#include "ops.h"
#include "page_common.h"

namespace aocr {

namespace {

constexpr int CORR_ROWS = 256;                 // rows of one corr_kernel workgroup = its threads
constexpr int MAX_D = 64;                      // the largest max_shift
constexpr int MAX_GROUPS = 512;                // ceil(16384 / 32) strips, group = 1
constexpr int SHIFT_MAX = 16384;               // what aocr_dewarp_page clamps a shift to

struct CurlLayout {                            // byte offsets into scratch_dev
  size_t hist, hdr, strips, ink, partials, totals, total;
  int nb, hs, ng, nchunks;
};

CurlLayout curl_layout(int H, int W, int g, int D) {
  CurlLayout l;
  ScratchCursor c;
  l.nb = (W + 31) / 32;
  l.hs = strip_rows(H);
  l.ng = cdiv(l.nb, g);
  l.nchunks = cdiv(H, CORR_ROWS);
  const size_t cands = (size_t)(l.ng - 1) * (2 * D + 1);
  l.hist = c.take(256 * sizeof(uint32_t));
  l.hdr = c.take(4 * sizeof(int32_t));
  l.strips = c.take((size_t)l.nb * l.hs);
  l.ink = c.take((size_t)l.ng * l.nchunks * sizeof(uint32_t));
  l.partials = c.take(cands * l.nchunks * sizeof(uint64_t));
  l.totals = c.take(cands * sizeof(uint64_t));
  l.total = c.total();
  return l;
}

__global__ __launch_bounds__(CORR_ROWS) void corr_kernel(const uint8_t* __restrict__ R, int H, int nb, int hs, int g, int ng, int D,
                                                         uint32_t* __restrict__ ink, uint64_t* __restrict__ partials) {
  __shared__ uint16_t ga[CORR_ROWS], gb[CORR_ROWS + 2 * MAX_D];           // G[j][y0 + i] and G[j+1][y0 - D + i], at most 512 each
  __shared__ uint32_t wink[2][CORR_ROWS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = blockIdx.y, chunk = blockIdx.x, nchunks = gridDim.x, y0 = chunk * CORR_ROWS;
  auto group_row = [&](int jj, int y) -> uint32_t {                       // G[jj][y], 0 outside the page (rows >= H of R are not all written)
    if ((unsigned)y >= (unsigned)H) return 0u;
    const int b1 = min((jj + 1) * g, nb);
    uint32_t v = 0;
    for (int b = jj * g; b < b1; ++b) v += R[(size_t)b * hs + y];
    return v;
  };
  const uint32_t av = group_row(j, y0 + tid);
  ga[tid] = (uint16_t)av;
  for (int i = tid; i < CORR_ROWS + 2 * D; i += CORR_ROWS) gb[i] = (uint16_t)group_row(j + 1, y0 - D + i);
  __syncthreads();
  const uint32_t ia = wave_sum(av), ib = wave_sum((uint32_t)gb[D + tid]);
  if (lane == 0) { wink[0][wave] = ia; wink[1][wave] = ib; }
  for (int c = wave; c < 2 * D + 1; c += CORR_ROWS / 64) {                // shift d = c - D: row y0 + i against row y0 + i + d = gb[i + c]
    uint32_t acc = 0;
    for (int i = lane; i < CORR_ROWS; i += 64) acc += (uint32_t)ga[i] * (uint32_t)gb[i + c];
    acc = wave_sum(acc);                                                  // <= 256 * 512^2 = 2^26
    if (lane == 0) partials[((size_t)j * (2 * D + 1) + c) * nchunks + chunk] = acc;
  }
  __syncthreads();
  if (tid == 0) {
    ink[(size_t)j * nchunks + chunk] = wink[0][0] + wink[0][1] + wink[0][2] + wink[0][3];
    if (j == ng - 2) ink[(size_t)(ng - 1) * nchunks + chunk] = wink[1][0] + wink[1][1] + wink[1][2] + wink[1][3];   // the last group has no pair of its own
  }
}

__global__ __launch_bounds__(256) void chain_kernel(const uint64_t* __restrict__ partials, const uint32_t* __restrict__ ink, int nchunks, int ng,
                                                    int D, int min_ink, int fixed, const int32_t* __restrict__ hdr, uint64_t* __restrict__ totals,
                                                    int32_t* __restrict__ curl, int32_t* __restrict__ shifts, uint64_t* __restrict__ scores) {
  __shared__ uint32_t gink[MAX_GROUPS];
  __shared__ int delta[MAX_GROUPS];
  const int nd = 2 * D + 1, npairs = ng - 1;
  for (int c = threadIdx.x; c < npairs * nd; c += 256) {
    uint64_t s = 0;
    for (int i = 0; i < nchunks; ++i) s += partials[(size_t)c * nchunks + i];
    totals[c] = s;
    if (scores) scores[c] = s;
  }
  if (npairs > 0)
    for (int j = threadIdx.x; j < ng; j += 256) {
      uint32_t s = 0;
      for (int i = 0; i < nchunks; ++i) s += ink[(size_t)j * nchunks + i];
      gink[j] = s;                                       // <= 2^26
    }
  __syncthreads();
  for (int j = threadIdx.x; j < npairs; j += 256) {
    int bd = 0;
    if (gink[j] >= (uint32_t)min_ink && gink[j + 1] >= (uint32_t)min_ink) {
      const uint64_t* t = totals + (size_t)j * nd + D;   // t[d], d in [-D, D]
      uint64_t best = t[0];
      for (int a = 1; a <= D; ++a) {                     // 0, -1, +1, -2, +2, ...: only a strictly larger score replaces an earlier one
        if (t[-a] > best) { best = t[-a]; bd = -a; }
        if (t[a] > best) { best = t[a]; bd = a; }
      }
    }
    delta[j] = bd;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int jc = ng >> 1;
    int amax = 0, moved = 0, s = 0;
    shifts[jc] = 0;
    for (int j = jc; j < npairs; ++j) { s += delta[j]; shifts[j + 1] = s; amax = max(amax, s < 0 ? -s : s); }
    s = 0;
    for (int j = jc - 1; j >= 0; --j) { s -= delta[j]; shifts[j] = s; amax = max(amax, s < 0 ? -s : s); }
    for (int j = 0; j < npairs; ++j) moved += delta[j] != 0;
    curl[0] = ng; curl[1] = amax; curl[2] = ink_thr(fixed, hdr); curl[3] = moved;
  }
}

__global__ __launch_bounds__(256) void dewarp_kernel(const uint8_t* __restrict__ page, int64_t pitch, int H, int W, int g, int ng,
                                                     const int32_t* __restrict__ shifts, uint32_t fill, uint8_t* __restrict__ out,
                                                     int64_t out_pitch) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int w = 32 * g, h = 16 * g, c_last = (ng - 1) * w + h;
  auto shift = [&](int j) { return min(max(shifts[j], -SHIFT_MAX), SHIFT_MAX); };
  const int q_first = 256 * shift(0), q_last = 256 * shift(ng - 1);
  // floor((ds*t*256 + h) / w) with h = 16g, w = 32g is floor((ds*t*16 + g) / (2g)): numerator and denominator divided by 16 exactly.
  // |ds*t*16| <= 32768 * (32g - 1) * 16 < 2^24 g = bias, so n = ds*t*16 + g + bias lies in (0, 2^29) where the header's product needs
  // 64 bits, and floor(n / (2g)) = floor(num / (2g)) + 2^23.  For n < 2^29 and a divisor <= 2^5, floor(n / d) = (n * ceil(2^34 / d)) >> 34
  // exactly (Granlund and Montgomery): one 32 x 34-bit product per pixel instead of a division.
  const int bias = g << 24;
  const uint64_t magic = (((uint64_t)1 << 34) + (uint64_t)(2 * g) - 1) / (uint64_t)(2 * g);
  struct Span3 { int j0w, sa, sb, sc; };                 // the shifts that up to 16 columns from x on can need: w >= 32, at most one centre inside
  auto span_at = [&](int x) -> Span3 {
    const int j0 = min(max(x - h, 0) / w, max(ng - 2, 0));
    return Span3{j0 * w + h, shift(j0), shift(min(j0 + 1, ng - 1)), shift(min(j0 + 2, ng - 1))};
  };
  auto q_of = [&](int x, const Span3& sp) -> int {       // the column's shift in Q8; x in [first column of sp, that + 15]
    if (x <= h) return q_first;
    if (x >= c_last) return q_last;
    int t = x - sp.j0w, s0 = sp.sa, s1 = sp.sb;          // c_0 < x < c_last: sp.j0w is a centre at or left of x, 0 <= t < w + 15
    if (t >= w) { t -= w; s0 = sp.sb; s1 = sp.sc; }
    const uint32_t n = (uint32_t)((s1 - s0) * t * 16 + g + bias);
    return 256 * s0 + (int)(((uint64_t)n * magic) >> 34) - (1 << 23);
  };
  for (int y = blockIdx.x * 4 + wave; y < H; y += gridDim.x * 4) {
    auto pixel = [&](int x, const Span3& sp) -> uint32_t {      // every read is inside the page
      const int p = 256 * y + q_of(x, sp), sy = p >> 8, f = p & 255;
      const uint32_t a = (unsigned)sy < (unsigned)H ? (uint32_t)page[(int64_t)sy * pitch + x] : fill;
      if (f == 0) return a;                              // (a*256 + 128) >> 8 = a: the second row has weight 0 and is not read
      const uint32_t b = (unsigned)(sy + 1) < (unsigned)H ? (uint32_t)page[(int64_t)(sy + 1) * pitch + x] : fill;
      return (a * (uint32_t)(256 - f) + b * (uint32_t)f + 128u) >> 8;
    };
    auto px1 = [&](int x) -> uint32_t { return pixel(x, span_at(x)); };
    auto px16 = [&](int x) -> uint4 {                    // one division and three shift loads for the 16 columns
      const Span3 sp = span_at(x);
      auto px4 = [&](int x4) -> uint32_t {
        return pixel(x4, sp) | (pixel(x4 + 1, sp) << 8) | (pixel(x4 + 2, sp) << 16) | (pixel(x4 + 3, sp) << 24);
      };
      uint4 q;
      q.x = px4(x); q.y = px4(x + 4); q.z = px4(x + 8); q.w = px4(x + 12);
      return q;
    };
    wave_store_row(out + (int64_t)y * out_pitch, W, lane, px1, px16);
  }
}

}  // namespace

int curl_groups(int W, int group) { return cdiv(cdiv(W, 32), group); }

size_t curl_scratch_bytes(int H, int W, int group, int max_shift) { return curl_layout(H, W, group, max_shift).total; }

void estimate_curl(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_curl_params& p, void* scratch, int32_t* curl,
                   int32_t* shifts, uint64_t* scores) {
  const CurlLayout l = curl_layout(H, W, p.group, p.max_shift);
  uint32_t* hist = scratch_at<uint32_t>(scratch, l.hist);
  int32_t* hdr = scratch_at<int32_t>(scratch, l.hdr);
  uint8_t* R = scratch_at<uint8_t>(scratch, l.strips);
  uint32_t* ink = scratch_at<uint32_t>(scratch, l.ink);
  uint64_t* partials = scratch_at<uint64_t>(scratch, l.partials);
  uint64_t* totals = scratch_at<uint64_t>(scratch, l.totals);
  const int light = p.light_text ? 1 : 0, fixed = p.threshold, D = p.max_shift;
  page_threshold(s, page, pitch, H, W, fixed, hist, hdr);
  if (l.ng > 1) {
    strip_profiles(s, page, pitch, H, W, light, fixed, hdr, R);
    hipLaunchKernelGGL(corr_kernel, dim3(l.nchunks, l.ng - 1), dim3(CORR_ROWS), 0, s, R, H, l.nb, l.hs, p.group, l.ng, D, ink, partials);
  }
  hipLaunchKernelGGL(chain_kernel, dim3(1), dim3(256), 0, s, partials, ink, l.nchunks, l.ng, D, p.min_ink, fixed, hdr, totals, curl, shifts,
                     scores);
}

void dewarp_page(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, int group, const int32_t* shifts, int fill, uint8_t* out,
                 int64_t out_pitch) {
  hipLaunchKernelGGL(dewarp_kernel, dim3(std::min(cdiv(H, 4), 2048)), dim3(256), 0, s, page, pitch, H, W, group, curl_groups(W, group), shifts,
                     (uint32_t)fill, out, out_pitch);
}

}  // namespace aocr
