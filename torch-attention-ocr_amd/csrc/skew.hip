// skew.hip -- page deskew (include/aocr.h: aocr_estimate_skew, aocr_deskew_page), the stage in front of aocr_segment_page: a sweep of sheared
// projection profiles finds the slope of the text lines, a combined vertical and horizontal shear removes it.  Integer arithmetic only
// (the Otsu threshold, when asked for, comes from segment.hip's otsu_threshold), so tests/skew_ref.py matches exactly.
//
// Launches of one aocr_estimate_skew, all on the caller's stream, intermediates in the caller's scratch:
//   (Otsu only) otsu_threshold of segment.hip: memset, hist_kernel, otsu_kernel -- what aocr_segment_page enqueues for its steps 1-2.
//   strips_kernel    the one page read.  A workgroup owns STRIP_ROWS consecutive rows, one wave per row at a time (wave_row16 of
//                    page_common.h): a 16-bit ink mask per 16-byte load split at the strip boundary (a load starts anywhere in its
//                    32-column strip: the row's base address is arbitrary) and added to the per-strip counters in LDS with integer
//                    atomics.  R is written as uint8 [strip][row], 8 rows per store.  curl.hip launches it too, through strip_profiles.
//   sweep_kernel     grid (row chunk, candidate): one thread per profile row r walks the strips (consecutive threads read consecutive
//                    bytes of R), squares its sum and the workgroup adds the squares in uint64: one partial per (candidate, chunk).
//   pick_kernel      one workgroup: the partials of a candidate are added in chunk order, the scores written, the winner taken by the
//                    total order "larger score, then earlier in 0, -1, +1, -2, +2, ...".
// aocr_deskew_page is one launch: deskew_kernel, one wave per output row (wave_store_row of page_common.h); the source of a row is one
// run of the page per 16-pixel group, shifted by the row's horizontal offset.
#include <algorithm>
#include "ops.h"
#include "page_common.h"

namespace aocr {

namespace {

constexpr int STRIP_ROWS = 8;                  // rows of one strips_kernel workgroup = bytes of one store to R
constexpr int MAX_STRIPS = 512;                // ceil(16384 / 32)
constexpr int SWEEP_THREADS = 256;
constexpr int SLOPE_MAX = 16384;               // Q16: 0.25 rows per column

struct SkewLayout {                            // byte offsets into scratch_dev
  size_t hist, hdr, strips, partials, total;
  int nb, hs, max_chunks;
};

// |off_k(b)| is largest at the first or the last strip (the offset is monotonic in b) and grows with |k|
__host__ __device__ inline int strip_off(int b, int cx, int slope) { return ((32 * b + 16 - cx) * slope + 32768) >> 16; }
__host__ __device__ inline int max_off(int nb, int cx, int slope) {
  const int a = strip_off(0, cx, slope), z = strip_off(nb - 1, cx, slope);
  const int aa = a < 0 ? -a : a, az = z < 0 ? -z : z;
  return aa > az ? aa : az;
}

SkewLayout skew_layout(int H, int W, int n_steps) {
  SkewLayout l;
  ScratchCursor c;
  l.nb = (W + 31) / 32;
  l.hs = strip_rows(H);
  const int dmax = std::max(max_off(l.nb, W >> 1, SLOPE_MAX), max_off(l.nb, W >> 1, -SLOPE_MAX));
  l.max_chunks = cdiv(H + 2 * dmax, SWEEP_THREADS);
  l.hist = c.take(256 * sizeof(uint32_t));
  l.hdr = c.take(4 * sizeof(int32_t));
  l.strips = c.take((size_t)l.nb * l.hs);
  l.partials = c.take((size_t)(2 * n_steps + 1) * l.max_chunks * sizeof(uint64_t));
  l.total = c.total();
  return l;
}

__global__ __launch_bounds__(256) void strips_kernel(const uint8_t* __restrict__ page, int64_t pitch, int H, int W, int light, int fixed,
                                                     const int32_t* __restrict__ hdr, int nb, int hs, uint8_t* __restrict__ R) {
  __shared__ uint32_t cnt[STRIP_ROWS][MAX_STRIPS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int thr = ink_thr(fixed, hdr);
  const int y0 = blockIdx.x * STRIP_ROWS;
  for (int i = threadIdx.x; i < STRIP_ROWS * MAX_STRIPS; i += 256) (&cnt[0][0])[i] = 0;
  __syncthreads();
  for (int j = wave; j < STRIP_ROWS; j += 4) {
    const int y = y0 + j;
    if (y >= H || thr < 0) continue;
    uint32_t* c = cnt[j];
    wave_row16(page + (int64_t)y * pitch, W, lane,
               [&](int x, uint32_t v) { if (is_ink((int)v, thr, light)) atomicAdd(&c[x >> 5], 1u); },
               [&](int x, const uint4& q) {                // columns x .. x+15 < W
                 const uint32_t m = ink_mask16(q, thr, light);
                 const int first = min(16, 32 - (x & 31)); // of them in strip x >> 5, the others in the next one
                 const int c0 = __popc(m & ((1u << first) - 1u)), c1 = __popc(m >> first);
                 if (c0) atomicAdd(&c[x >> 5], (uint32_t)c0);
                 if (c1) atomicAdd(&c[(x >> 5) + 1], (uint32_t)c1);      // c1 > 0: column x + first < W lies in that strip
               });
  }
  __syncthreads();
  for (int b = threadIdx.x; b < nb; b += 256) {          // rows >= H of the last workgroup are zero: y0 + 8 <= hs
    uint2 o;
    o.x = cnt[0][b] | (cnt[1][b] << 8) | (cnt[2][b] << 16) | (cnt[3][b] << 24);
    o.y = cnt[4][b] | (cnt[5][b] << 8) | (cnt[6][b] << 16) | (cnt[7][b] << 24);
    *reinterpret_cast<uint2*>(R + (size_t)b * hs + y0) = o;
  }
}

__global__ __launch_bounds__(SWEEP_THREADS) void sweep_kernel(const uint8_t* __restrict__ R, int H, int W, int nb, int hs, int K, int step,
                                                              uint64_t* __restrict__ partials) {
  __shared__ uint64_t wsum[SWEEP_THREADS / 64];
  const int slope = ((int)blockIdx.y - K) * step, cx = W >> 1;
  const int D = max_off(nb, cx, slope);
  const int r = (int)(blockIdx.x * SWEEP_THREADS + threadIdx.x) - D;      // this thread's profile row, in [-D, H + D)
  uint32_t P = 0;
  if (r < H + D) {
    const uint8_t* col = R;
    for (int b = 0; b < nb; ++b, col += hs) {
      const int y = r + strip_off(b, cx, slope);
      if ((unsigned)y < (unsigned)H) P += col[y];
    }
  }
  uint64_t v = (uint64_t)P * P;                                           // P <= W <= 2^14
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(256) void pick_kernel(const uint64_t* __restrict__ partials, int nchunks, int K, int step, int fixed,
                                                   const int32_t* __restrict__ hdr, int32_t* __restrict__ skew, uint64_t* __restrict__ scores) {
  __shared__ uint64_t bs[256];
  __shared__ int br[256];
  uint64_t best = 0;
  int rank = 1 << 30;                                    // every candidate comes before this one
  for (int c = threadIdx.x; c < 2 * K + 1; c += 256) {
    uint64_t s = 0;
    for (int i = 0; i < nchunks; ++i) s += partials[(size_t)c * nchunks + i];
    if (scores) scores[c] = s;
    const int k = c - K, rk = k == 0 ? 0 : (k < 0 ? -2 * k - 1 : 2 * k);   // place in 0, -1, +1, -2, +2, ...
    if (s > best || (s == best && rk < rank)) { best = s; rank = rk; }
  }
  bs[threadIdx.x] = best; br[threadIdx.x] = rank;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if ((int)threadIdx.x < d) {
      const uint64_t os = bs[threadIdx.x + d]; const int orank = br[threadIdx.x + d];
      if (os > bs[threadIdx.x] || (os == bs[threadIdx.x] && orank < br[threadIdx.x])) { bs[threadIdx.x] = os; br[threadIdx.x] = orank; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int rk = br[0];                                // candidate 0 always exists: rk <= 2K
    const int k = (rk & 1) ? -((rk + 1) >> 1) : (rk >> 1);
    skew[0] = k; skew[1] = k * step; skew[2] = ink_thr(fixed, hdr); skew[3] = 0;
  }
}

__global__ __launch_bounds__(256) void deskew_kernel(const uint8_t* __restrict__ page, int64_t pitch, int H, int W, const int32_t* __restrict__ skew,
                                                     int slope, uint32_t fill, uint8_t* __restrict__ out, int64_t out_pitch) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = min(max(skew ? skew[1] : slope, -SLOPE_MAX), SLOPE_MAX);
  const int cx = W >> 1, cy = H >> 1;
  for (int y = blockIdx.x * 4 + wave; y < H; y += gridDim.x * 4) {
    const int dx = ((y - cy) * s + 32768) >> 16;
    auto px = [&](int x) -> uint32_t {                   // every read is inside the page
      const int sy = y + (((x - cx) * s + 32768) >> 16), sx = x - dx;
      return ((unsigned)sy < (unsigned)H && (unsigned)sx < (unsigned)W) ? (uint32_t)page[(int64_t)sy * pitch + sx] : fill;
    };
    wave_store_row(out + (int64_t)y * out_pitch, W, lane, px, px16_of(px));
  }
}

}  // namespace

// rows of one strip of R, padded so that every 8-row store is aligned and inside
int strip_rows(int H) { return (H + 15) & ~15; }

// shared with curl.hip
void strip_profiles(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, int light, int fixed, const int32_t* hdr, uint8_t* R) {
  hipLaunchKernelGGL(strips_kernel, dim3(cdiv(H, STRIP_ROWS)), dim3(256), 0, s, page, pitch, H, W, light, fixed, hdr, (W + 31) / 32, strip_rows(H), R);
}

size_t skew_scratch_bytes(int H, int W, int n_steps) { return skew_layout(H, W, n_steps).total; }

void estimate_skew(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_skew_params& p, void* scratch, int32_t* skew,
                   uint64_t* scores) {
  const SkewLayout l = skew_layout(H, W, p.n_steps);
  uint32_t* hist = scratch_at<uint32_t>(scratch, l.hist);
  int32_t* hdr = scratch_at<int32_t>(scratch, l.hdr);
  uint8_t* R = scratch_at<uint8_t>(scratch, l.strips);
  uint64_t* partials = scratch_at<uint64_t>(scratch, l.partials);
  const int light = p.light_text ? 1 : 0, fixed = p.threshold, K = p.n_steps;
  const int dmax = std::max(max_off(l.nb, W >> 1, K * p.step_q16), max_off(l.nb, W >> 1, -K * p.step_q16));
  const int nchunks = cdiv(H + 2 * dmax, SWEEP_THREADS);                  // <= l.max_chunks: K * step_q16 <= SLOPE_MAX
  page_threshold(s, page, pitch, H, W, fixed, hist, hdr);
  strip_profiles(s, page, pitch, H, W, light, fixed, hdr, R);
  hipLaunchKernelGGL(sweep_kernel, dim3(nchunks, 2 * K + 1), dim3(SWEEP_THREADS), 0, s, R, H, W, l.nb, l.hs, K, p.step_q16, partials);
  hipLaunchKernelGGL(pick_kernel, dim3(1), dim3(256), 0, s, partials, nchunks, K, p.step_q16, fixed, hdr, skew, scores);
}

void deskew_page(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const int32_t* skew, int slope_q16, int fill, uint8_t* out,
                 int64_t out_pitch) {
  hipLaunchKernelGGL(deskew_kernel, dim3(std::min(cdiv(H, 4), 2048)), dim3(256), 0, s, page, pitch, H, W, skew, slope_q16, (uint32_t)fill, out,
                     out_pitch);
}

}  // namespace aocr
