// binarize.hip -- local adaptive binarisation (include/aocr.h: aocr_binarize_page), the stage behind aocr_flatten_page: a Sauvola threshold
// from the mean and the standard deviation of the window around every pixel.  Integer arithmetic, specified exactly, so
// tests/binarize_ref.py matches byte for byte; the one double sqrt and the one double division are stepped to the exact integer results.
// One fused launch, no page-sized intermediate: 1 byte per pixel read from HBM, 1 written.
//   bin_kernel   A workgroup of BIN_EW threads owns BIN_EW - 2r output columns x BIN_TH output rows and walks them downward.  Thread t owns
//                column X0 - r + t of the tile WITH its halo of r columns on either side, and carries that column's vertical window sums
//                (S1 of v <= 127 * 255, S2 of v^2 <= 127 * 65025) in two registers: one row added and one subtracted per output row, 2r + 1
//                rows to start, as flat_vsum_kernel does.  A window sum over a rectangle is separable and its axes commute; taking the
//                vertical axis first is what lets the leaving row be a single byte per column, re-read through L2, where the horizontal
//                sums of a leaving row would be a ring of 2r + 1 rows x 6 bytes per column in LDS (146 KB at r = 63 for 192 columns: one
//                workgroup per CU).  Per output row the BIN_EW column sums become an inclusive prefix across the workgroup (shuffles inside
//                a wave, the four wave totals through LDS, two barriers), so the window sum of an output column is a difference of two
//                prefix entries; columns outside the page hold 0 and need no clipping.  Then the threshold and the output byte, one thread
//                per pixel.  Halo rows and columns are read again by the neighbouring workgroups, out of L2.
//   bin_counts_init_kernel   counts_dev = {0, INT32_MAX, 0, 0} in front of the integer atomics of bin_kernel (one per workgroup and word).
// Integer sums do not depend on their order, and the atomics are integer add, min and max: the result does not depend on the launch
// geometry or the run.
#include <climits>
#include "ops.h"
#include "page_common.h"

namespace aocr {

namespace {

constexpr int BIN_EW = 256;                    // threads of a workgroup = the columns of its tile, the halo of r on either side included
constexpr int BIN_TH = 64;                     // output rows of a workgroup
constexpr int BIN_RMAX = 63;
static_assert(BIN_EW - 2 * BIN_RMAX >= 64, "a tile keeps at least a wave of output columns at the largest radius");

__device__ __forceinline__ int wave_min_i(int v) {
  for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d));
  return v;
}

__device__ __forceinline__ int wave_max_i(int v) {
  for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
  return v;
}

// the Sauvola threshold of a window of n pixels with sums S1 and S2: T of include/aocr.h, exactly
__device__ __forceinline__ uint32_t sauvola_t(uint64_t n, uint64_t S1, uint64_t S2, uint32_t kq, uint32_t range) {
  const uint64_t D = n * S2 - S1 * S1;                   // < 2^43: exact in a double
  uint64_t q = (uint64_t)sqrt((double)D);
  while (q * q > D) --q;
  while ((q + 1) * (q + 1) <= D) ++q;
  const uint64_t num = S1 * ((uint64_t)(256u - kq) * range * n + (uint64_t)kq * q);      // < 2^53
  const uint64_t den = (uint64_t)256 * range * n * n;                                    // < 2^45
  uint64_t t = (uint64_t)((double)num / (double)den);    // both exact in a double; the quotient is < 2^15 and at most one off
  while (t * den > num) --t;
  while ((t + 1) * den <= num) ++t;
  return (uint32_t)t;
}

__global__ void bin_counts_init_kernel(int32_t* __restrict__ counts) {
  counts[0] = 0; counts[1] = INT_MAX; counts[2] = 0; counts[3] = 0;
}

__global__ __launch_bounds__(BIN_EW) void bin_kernel(const uint8_t* __restrict__ page, int64_t pitch, int H, int W, int r, uint32_t kq, uint32_t range,
                                                     uint32_t inv8, int hard, uint8_t* __restrict__ out, int64_t out_pitch,
                                                     int32_t* __restrict__ counts) {
  __shared__ uint32_t P1[BIN_EW + 1], P2[BIN_EW + 1];    // P[u]: the sum of the column sums of the threads 0 .. u - 1
  __shared__ uint32_t wt1[BIN_EW / 64], wt2[BIN_EW / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int TW = BIN_EW - 2 * r;
  const int X0 = blockIdx.x * TW, x = X0 - r + t;
  const int Y0 = blockIdx.y * BIN_TH, Y1 = min(Y0 + BIN_TH, H);
  const bool incol = (unsigned)x < (unsigned)W;          // every thread takes every barrier and every shuffle
  const bool outcol = t >= r && t < BIN_EW - r && x < W; // x >= X0 >= 0 there
  const uint8_t* col = page + (incol ? x : 0);
  const uint32_t nx = (uint32_t)(min(x + r, W - 1) - max(x - r, 0) + 1);
  uint32_t s1 = 0, s2 = 0;
  if (incol)
    for (int y = max(Y0 - r, 0); y <= min(Y0 + r, H - 1); ++y) {
      const uint32_t v = (uint32_t)col[(int64_t)y * pitch] ^ inv8;
      s1 += v; s2 += v * v;
    }
  if (t == 0) { P1[0] = 0; P2[0] = 0; }
  int ink = 0, tmin = INT_MAX, tmax = 0;
  for (int y = Y0; y < Y1; ++y) {
    uint32_t a = s1, b = s2;                             // inclusive prefix: a <= 256 * 32385, b <= 256 * 127 * 65025 < 2^31
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t ta = __shfl_up(a, d), tb = __shfl_up(b, d);
      if (lane >= d) { a += ta; b += tb; }
    }
    if (lane == 63) { wt1[wave] = a; wt2[wave] = b; }
    __syncthreads();
    for (int w = 0; w < wave; ++w) { a += wt1[w]; b += wt2[w]; }
    P1[t + 1] = a; P2[t + 1] = b;
    __syncthreads();
    if (outcol) {
      const uint32_t ny = (uint32_t)(min(y + r, H - 1) - max(y - r, 0) + 1);
      const uint32_t S1 = P1[t + r + 1] - P1[t - r], S2 = P2[t + r + 1] - P2[t - r];
      const uint32_t T = sauvola_t((uint64_t)nx * ny, S1, S2, kq, range);
      const uint32_t v = (uint32_t)col[(int64_t)y * pitch] ^ inv8;
      uint32_t o;
      if (v <= T) {
        o = hard ? 0u : (v * 127u) / max(T, 1u);
        ++ink;
      } else {                                           // T < v <= 255
        o = hard ? 255u : min(255u, 128u + ((v - T - 1u) * 127u) / (uint32_t)max(254 - (int)T, 1));
      }
      out[(int64_t)y * out_pitch + x] = (uint8_t)(o ^ inv8);
      tmin = min(tmin, (int)T); tmax = max(tmax, (int)T);
    }
    if (incol) {                                         // the window of row y + 1: add before subtract, as the sums are unsigned
      if (y + r + 1 < H) { const uint32_t v = (uint32_t)col[(int64_t)(y + r + 1) * pitch] ^ inv8; s1 += v; s2 += v * v; }
      if (y - r >= 0) { const uint32_t v = (uint32_t)col[(int64_t)(y - r) * pitch] ^ inv8; s1 -= v; s2 -= v * v; }
    }
  }
  if (counts) {
    __shared__ int red[3][BIN_EW / 64];                  // counts is the same for every thread: the barrier is taken by all or none
    ink = wave_sum(ink); tmin = wave_min_i(tmin); tmax = wave_max_i(tmax);
    if (lane == 0) { red[0][wave] = ink; red[1][wave] = tmin; red[2][wave] = tmax; }
    __syncthreads();
    if (t == 0) {                                        // every workgroup has an output pixel: three atomics per workgroup
      for (int w = 1; w < BIN_EW / 64; ++w) { ink += red[0][w]; tmin = min(tmin, red[1][w]); tmax = max(tmax, red[2][w]); }
      atomicAdd(&counts[0], ink); atomicMin(&counts[1], tmin); atomicMax(&counts[2], tmax);
    }
  }
}

}  // namespace

size_t binarize_scratch_bytes(int, int, int) { return 256; }       // the fused kernel keeps its sums in registers and LDS: nothing is written there

void binarize_page(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_binarize_params& bp, uint8_t* out, int64_t out_pitch,
                   int32_t* counts) {
  const int r = bp.radius;
  if (counts) hipLaunchKernelGGL(bin_counts_init_kernel, dim3(1), dim3(1), 0, s, counts);
  hipLaunchKernelGGL(bin_kernel, dim3(cdiv(W, BIN_EW - 2 * r), cdiv(H, BIN_TH)), dim3(BIN_EW), 0, s, page, pitch, H, W, r, (uint32_t)bp.k_q8,
                     (uint32_t)bp.range, bp.light_text ? 0xffu : 0u, bp.hard, out, out_pitch, counts);
}

}  // namespace aocr
