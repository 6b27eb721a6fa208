// rectify.hip -- page rectification (include/aocr.h: aocr_find_page_quad, aocr_rectify_plan, aocr_warp_page), the stage in front of
// aocr_flatten_page: a photographed page is a quadrilateral on a desk, seen in perspective.  aocr_find_page_quad finds the four corners of
// the paper (integers only: the labels and areas come from components.hip's launches, the Otsu threshold from segment.hip's),
// aocr_rectify_plan turns them into an output size and nine coefficients on the host, aocr_warp_page resamples the page through them.  The
// warp is double precision with every operation rounded on its own (the Makefile compiles this file with -ffp-contract=off), so
// tests/rectify_ref.py, one numpy operation per operation here, matches bit for bit.
//
// Launches of one aocr_find_page_quad, all on the caller's stream, intermediates in the caller's scratch:
//   label_components of components.hip with light_text = !dark_paper and 8-connectivity: the paper mask's canonical labels (into the
//                      scratch), every root's area in its statistics record, and [threshold, paper pixels, components, 0].
//   memset             of the five 64-bit keys.
//   quad_sheet_kernel  a thread walks QUAD_ROWS rows of one column of the labels; a root (label == its own index) offers the key
//                      area << 32 | (2^32 - 1 - label): the largest key is the largest area, and among equals the smallest label.  One
//                      reduction per wave, then one 64-bit atomicMax per wave that has a root and whose key beats what the word holds.
//   quad_corner_kernel the same walk; a pixel of the sheet offers four keys, all of them maxima (a minimum is the maximum of the negated
//                      pair), packed so that the second criterion sits in the low word.  Waves without a sheet pixel leave at once.
//   quad_final_kernel  one thread unpacks the keys, takes the four cross products in int64 and writes the 16 words.
// Integer maxima do not depend on their order: the words do not depend on the launch geometry or on the order of the atomics.
//
// aocr_warp_page is one launch: warp_kernel, one wave per output row (wave_store_row of page_common.h).  A lane's 16 pixels are 16 neighbouring source positions, the lanes of a wave
// continue them along the row: the four taps of a wave's pixels lie in two (for a keystone a few) source rows and stay in the same cache
// lines from lane to lane.  The products c1*y, c4*y, c7*y are taken once per row: (c0*x + c1*y) + c2 rounds the same whether c1*y was
// rounded now or before.  Two correctly rounded fp64 divisions per pixel (hipcc's default: no fast-math, no reciprocal shortcut).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include "ops.h"
#include "page_common.h"

namespace aocr {

namespace {

constexpr int QUAD_ROWS = 8;                   // rows of one thread of the two walks
constexpr int QUAD_THREADS = 256;
constexpr int QUAD_OFF = 16384;                // x - y + QUAD_OFF >= 1 on every legal page
enum { KEY_SHEET = 0, KEY_TL, KEY_TR, KEY_BR, KEY_BL, KEY_COUNT };

struct QuadLayout {                            // byte offsets into scratch_dev
  size_t cc, labels, hdr, total;
};

QuadLayout quad_layout(int H, int W) {
  QuadLayout l;
  ScratchCursor c;
  l.cc = c.take(components_scratch_bytes(H, W));
  l.labels = c.take((size_t)H * W * sizeof(int32_t));
  l.hdr = c.take(64 + KEY_COUNT * sizeof(uint64_t));                   // info (4 words, padded to 64 bytes), then the keys
  l.total = c.total();
  return l;
}

// one lane of a wave: the word only ever grows, so a key that does not beat a (possibly stale) read of it cannot beat its true value
__device__ __forceinline__ void offer(uint64_t* word, uint64_t key) {
  if (key > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(reinterpret_cast<unsigned long long*>(word), (unsigned long long)key);
}

__global__ __launch_bounds__(QUAD_THREADS) void quad_sheet_kernel(const int32_t* __restrict__ labels, int H, int W, const int32_t* __restrict__ rec,
                                                                  int sw, uint64_t* keys) {
  const int x = blockIdx.x * QUAD_THREADS + threadIdx.x;
  const int y0 = blockIdx.y * QUAD_ROWS, y1 = min(H, y0 + QUAD_ROWS);
  uint64_t best = 0;
  if (x < W)
    for (int y = y0; y < y1; ++y) {
      const int i = y * W + x;
      if (labels[i] != i) continue;                        // paper (-1), or not the first pixel of its component
      const uint64_t area = (uint64_t)(uint32_t)rec[4 * ((size_t)y * sw + (x >> 1))];                     // >= 1
      const uint64_t key = (area << 32) | (uint64_t)(0xffffffffu - (uint32_t)i);
      best = key > best ? key : best;
    }
  best = wave_max(best);
  if ((threadIdx.x & 63) == 0 && best) offer(&keys[KEY_SHEET], best);
}

__global__ __launch_bounds__(QUAD_THREADS) void quad_corner_kernel(const int32_t* __restrict__ labels, int H, int W, uint64_t* keys) {
  const uint64_t sk = keys[KEY_SHEET];                     // written by the launch before
  if (!sk) return;                                         // no component at all
  const int sheet = (int)(0xffffffffu - (uint32_t)sk);
  const int x = blockIdx.x * QUAD_THREADS + threadIdx.x;
  const int y0 = blockIdx.y * QUAD_ROWS, y1 = min(H, y0 + QUAD_ROWS);
  uint64_t tl = 0, tr = 0, br = 0, bl = 0;
  if (x < W)
    for (int y = y0; y < y1; ++y) {
      if (labels[y * W + x] != sheet) continue;
      const uint64_t uy = (uint64_t)y;
      const uint64_t k0 = ~(((uint64_t)(x + y) << 32) | uy);                                     // min (x+y, then y)
      const uint64_t k1 = ((uint64_t)(x - y + QUAD_OFF) << 32) | (uint64_t)(QUAD_OFF - y);       // max (x-y, then -y)
      const uint64_t k2 = ((uint64_t)(x + y + 1) << 32) | uy;                                    // max (x+y, then y); never 0
      const uint64_t k3 = ((uint64_t)(y - x + QUAD_OFF) << 32) | uy;                             // min (x-y, then -y) = max (y-x, then y)
      tl = k0 > tl ? k0 : tl; tr = k1 > tr ? k1 : tr; br = k2 > br ? k2 : br; bl = k3 > bl ? k3 : bl;
    }
  if (!__ballot(tl != 0)) return;                          // every key of a sheet pixel is non-zero
  tl = wave_max(tl); tr = wave_max(tr); br = wave_max(br); bl = wave_max(bl);
  if ((threadIdx.x & 63) == 0) { offer(&keys[KEY_TL], tl); offer(&keys[KEY_TR], tr); offer(&keys[KEY_BR], br); offer(&keys[KEY_BL], bl); }
}

__host__ __device__ inline bool quad_convex(const int64_t* q) {      // x0 y0 .. x3 y3 in the order TL TR BR BL: clockwise with y down
  for (int i = 0; i < 4; ++i) {
    const int a = i, b = (i + 1) & 3, c = (i + 2) & 3;
    const int64_t ux = q[2 * b] - q[2 * a], uy = q[2 * b + 1] - q[2 * a + 1], vx = q[2 * c] - q[2 * b], vy = q[2 * c + 1] - q[2 * b + 1];
    if (!(ux * vy - uy * vx > 0)) return false;
  }
  return true;
}

__global__ void quad_final_kernel(const uint64_t* __restrict__ keys, const int32_t* __restrict__ info, int32_t* __restrict__ quad) {
  if (threadIdx.x != 0) return;
  int64_t q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const uint64_t sk = keys[KEY_SHEET];
  int valid = 0;
  if (sk) {
    const uint64_t k0 = ~keys[KEY_TL], k1 = keys[KEY_TR], k2 = keys[KEY_BR], k3 = keys[KEY_BL];
    q[1] = (int64_t)(k0 & 0xffffffffu);            q[0] = (int64_t)(k0 >> 32) - q[1];
    q[3] = QUAD_OFF - (int64_t)(k1 & 0xffffffffu); q[2] = (int64_t)(k1 >> 32) - QUAD_OFF + q[3];
    q[5] = (int64_t)(k2 & 0xffffffffu);            q[4] = (int64_t)(k2 >> 32) - 1 - q[5];
    q[7] = (int64_t)(k3 & 0xffffffffu);            q[6] = q[7] - ((int64_t)(k3 >> 32) - QUAD_OFF);
    valid = quad_convex(q) ? 1 : 0;
  }
  for (int i = 0; i < 8; ++i) quad[i] = (int32_t)q[i];
  quad[8] = info[0]; quad[9] = (int32_t)(sk >> 32); quad[10] = info[2]; quad[11] = valid;
  quad[12] = 0; quad[13] = 0; quad[14] = 0; quad[15] = 0;
}

struct WarpCoef { double c[9]; };

__global__ __launch_bounds__(256) void warp_kernel(const uint8_t* __restrict__ page, int64_t pitch, int H, int W, WarpCoef k, uint32_t fill,
                                                   uint8_t* __restrict__ out, int64_t out_pitch, int Ho, int Wo) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double wmax = (double)W, hmax = (double)H;
  for (int y = blockIdx.x * 4 + wave; y < Ho; y += gridDim.x * 4) {
    const double yd = (double)y;
    const double r1 = k.c[1] * yd, r4 = k.c[4] * yd, r7 = k.c[7] * yd;          // the row's products, rounded as they would be per pixel
    auto tap = [&](int64_t tx, int64_t ty) -> uint32_t {   // every read is inside the page
      return ((uint64_t)tx < (uint64_t)W && (uint64_t)ty < (uint64_t)H) ? (uint32_t)page[ty * pitch + tx] : fill;
    };
    auto px = [&](int x) -> uint32_t {
      const double xd = (double)x;
      const double nx = (k.c[0] * xd + r1) + k.c[2];
      const double ny = (k.c[3] * xd + r4) + k.c[5];
      const double dn = (k.c[6] * xd + r7) + k.c[8];
      if (!(dn > 0.0)) return fill;
      const double X = nx / dn, Y = ny / dn;
      if (!(X >= -1.0 && X <= wmax) || !(Y >= -1.0 && Y <= hmax)) return fill;                  // NaN falls here
      const int64_t qx = (int64_t)floor(X * 256.0 + 0.5), qy = (int64_t)floor(Y * 256.0 + 0.5);   // within [-256, 256 * 16384]
      const int64_t ix = qx >> 8, iy = qy >> 8;
      const uint32_t fx = (uint32_t)(qx & 255), fy = (uint32_t)(qy & 255);
      const uint32_t top = tap(ix, iy) * (256u - fx) + tap(ix + 1, iy) * fx;
      const uint32_t bot = tap(ix, iy + 1) * (256u - fx) + tap(ix + 1, iy + 1) * fx;
      return (top * (256u - fy) + bot * fy + 32768u) >> 16;                                      // <= 255
    };
    wave_store_row(out + (int64_t)y * out_pitch, Wo, lane, px, px16_of(px));
  }
}

int64_t isqrt64(int64_t v) {                               // floor(sqrt(v)), v >= 0
  int64_t r = (int64_t)std::sqrt((double)v);
  while (r > 0 && r * r > v) --r;
  while ((r + 1) * (r + 1) <= v) ++r;
  return r;
}

struct PlanErr { char* buf; size_t len; };

int plan_fail(const PlanErr& err, const char* fmt, ...) {
  if (err.buf && err.len) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err.buf, err.len, fmt, ap);
    va_end(ap);
  }
  return 1;
}

}  // namespace

size_t quad_scratch_bytes(int H, int W) { return quad_layout(H, W).total; }

void find_page_quad(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, int threshold, int dark_paper, void* scratch,
                    int32_t* quad) {
  const QuadLayout l = quad_layout(H, W);
  void* cc = scratch_at<char>(scratch, l.cc);
  int32_t* labels = scratch_at<int32_t>(scratch, l.labels);
  int32_t* info = scratch_at<int32_t>(scratch, l.hdr);
  uint64_t* keys = scratch_at<uint64_t>(scratch, l.hdr + 64);
  label_components(s, page, pitch, H, W, threshold, dark_paper ? 0 : 1, 8, cc, labels, W, 1, nullptr, info);
  const ComponentAreas a = component_areas(H, W, cc);
  (void)hipMemsetAsync(keys, 0, KEY_COUNT * sizeof(uint64_t), s);
  const dim3 grid(cdiv(W, QUAD_THREADS), cdiv(H, QUAD_ROWS));
  hipLaunchKernelGGL(quad_sheet_kernel, grid, dim3(QUAD_THREADS), 0, s, labels, H, W, a.rec, a.sw, keys);
  hipLaunchKernelGGL(quad_corner_kernel, grid, dim3(QUAD_THREADS), 0, s, labels, H, W, keys);
  hipLaunchKernelGGL(quad_final_kernel, dim3(1), dim3(64), 0, s, keys, info, quad);
}

int rectify_plan(const int32_t* quad, int Wo_in, int Ho_in, int32_t* size, double* coef, char* err_buf, size_t err_len) {
  const PlanErr err{err_buf, err_len};
  int64_t q[8];
  for (int i = 0; i < 8; ++i) {
    q[i] = quad[i];
    if (q[i] < -RECTIFY_COORD_MAX || q[i] > RECTIFY_COORD_MAX)
      return plan_fail(err, "quad coordinate %lld is outside +-%d", (long long)q[i], RECTIFY_COORD_MAX);
  }
  if (!quad_convex(q)) return plan_fail(err, "the quad is not convex and clockwise in the order TL, TR, BR, BL (a cross product is <= 0)");
  const int64_t x0 = q[0], y0 = q[1], x1 = q[2], y1 = q[3], x2 = q[4], y2 = q[5], x3 = q[6], y3 = q[7];
  auto d2 = [](int64_t ax, int64_t ay, int64_t bx, int64_t by) { return (ax - bx) * (ax - bx) + (ay - by) * (ay - by); };
  const int64_t Wo = Wo_in > 0 ? Wo_in : isqrt64(std::max(d2(x1, y1, x0, y0), d2(x2, y2, x3, y3))) + 1;
  const int64_t Ho = Ho_in > 0 ? Ho_in : isqrt64(std::max(d2(x3, y3, x0, y0), d2(x2, y2, x1, y1))) + 1;
  if (Wo > 16384 || Ho > 16384 || Wo * Ho > ((int64_t)1 << 26))
    return plan_fail(err, "the rectified page would be Wo=%lld x Ho=%lld: at most 16384 each and Wo*Ho <= 2^26; pass a smaller width and height",
                     (long long)Wo, (long long)Ho);
  const int64_t dx1 = x1 - x2, dx2 = x3 - x2, dx3 = x0 - x1 + x2 - x3;
  const int64_t dy1 = y1 - y2, dy2 = y3 - y2, dy3 = y0 - y1 + y2 - y3;
  const int64_t den = dx1 * dy2 - dy1 * dx2, gn = dx3 * dy2 - dy3 * dx2, hn = dx1 * dy3 - dy1 * dx3;      // den != 0: the corner BR turns
  const double g = (double)gn / (double)den, h = (double)hn / (double)den;
  const double a = (double)(x1 - x0) + g * (double)x1, b = (double)(x3 - x0) + h * (double)x3, c = (double)x0;
  const double d = (double)(y1 - y0) + g * (double)y1, e = (double)(y3 - y0) + h * (double)y3, f = (double)y0;
  const double U = (double)std::max<int64_t>(Wo - 1, 1), V = (double)std::max<int64_t>(Ho - 1, 1);
  const double UV = U * V;
  size[0] = (int32_t)Wo; size[1] = (int32_t)Ho;
  coef[0] = a * V; coef[1] = b * U; coef[2] = c * UV;
  coef[3] = d * V; coef[4] = e * U; coef[5] = f * UV;
  coef[6] = g * V; coef[7] = h * U; coef[8] = UV;
  return 0;
}

void warp_page(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const double* coef, int fill, uint8_t* out, int64_t out_pitch,
               int Ho, int Wo) {
  WarpCoef k;
  for (int i = 0; i < 9; ++i) k.c[i] = coef[i];
  hipLaunchKernelGGL(warp_kernel, dim3(std::min(cdiv(Ho, 4), 2048)), dim3(256), 0, s, page, pitch, H, W, k, (uint32_t)fill, out, out_pitch, Ho,
                     Wo);
}

}  // namespace aocr
