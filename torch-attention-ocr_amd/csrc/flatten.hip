// flatten.hip -- page background flattening (include/aocr.h: aocr_flatten_page), the stage in front of aocr_estimate_skew and
// aocr_segment_page: the paper brightness near every pixel (a windowed max, then a windowed mean) is divided out.  Integer arithmetic only,
// so tests/flatten_ref.py matches exactly.  A max and a sum over a rectangle are separable and their two axes commute, so the four
// windowed passes run in the order that lets the row kernels own the unaligned page and output and the column kernels see aligned planes:
//   flat_hmax_kernel   page -> A (bytes).  A workgroup owns 4 rows of one segment of HSEG columns, one wave per row.  The segment and its
//                      halo of r columns go to LDS with 16-byte loads wherever a whole aligned chunk lies inside the row (the tile starts on a
//                      16-byte boundary of the row's address) and byte loads at the ragged ends; columns outside the page are 0, the identity
//                      of max.  Window doubling: m_2k[i] = max(m_k[i], m_k[i+k]) up to the largest power of two p <= 2r+1, then
//                      A[x] = max(m_p[x-r], m_p[x+r-p+1]): log2(p) + 1 LDS passes of 4-byte words, a funnel shift where i+k is not a
//                      multiple of 4.
//   flat_vmax_kernel   A -> M (bytes).  A workgroup owns 64 columns x VT_ROWS rows: the tile and r rows above and below in LDS (rows outside
//                      the page are 0), the same doubling down the rows; every access is a whole word, consecutive lanes read consecutive
//                      words of a row.
//   flat_vsum_kernel   M -> S (uint16, <= 255 * 255).  One thread per 4 columns and band of VS_ROWS rows carries the column sums of the window
//                      down the band: one row added and one subtracted per output row, 2r+1 rows to start; the four sums ride in two
//                      registers as 16-bit halves (add before subtract: no half exceeds 65025 + 255).
//   flat_div_kernel    S, page -> out.  A workgroup owns 4 rows of one segment of HSEG columns, one wave per row: the row of S with its halo
//                      becomes an exclusive prefix sum in LDS (each lane scans PCH consecutive entries, the lane totals are scanned with
//                      shuffles), so B is a difference of two entries; then the rounding, the two integer divisions and the row store of
//                      page_common.h (wave_store_row) over the segment.
// Integer sums and maxima do not depend on their order: the result does not depend on the launch geometry.  No atomics, no floats.
#include <algorithm>
#include "ops.h"
#include "page_common.h"

namespace aocr {

namespace {

constexpr int RMAX = 127;
constexpr int HSEG = 1024;                     // columns of one row segment (flat_hmax_kernel, flat_div_kernel)
constexpr int HROWS = 4;                       // rows of one workgroup of the row kernels: one per wave
constexpr int HM_WORDS = (HSEG + 2 * RMAX + 30 + 15) / 16 * 4;  // the tile: HSEG + 2r columns, < 16 more on either side for the alignment
constexpr int VT_COLS = 64;                    // flat_vmax_kernel: columns (16 words) and rows of one workgroup's tile
constexpr int VT_ROWS = 128;
constexpr int VS_WORDS = 64;                   // flat_vsum_kernel: a workgroup is 64 words (256 columns) x 4 bands of VS_ROWS rows
constexpr int VS_ROWS = 64;
constexpr int PCH = 21;                        // flat_div_kernel: prefix entries per lane; odd: the lanes' chunks start on distinct banks
static_assert(64 * PCH >= HSEG + 2 * RMAX + 1, "the prefix of a segment and its halo must fit");

struct FlatLayout {                            // byte offsets into scratch_dev; S overlays A, which is dead once M is written
  size_t a, s, m, total;
  int pa4;                                     // words (4 columns) per row of every plane
};

FlatLayout flat_layout(int H, int W) {
  FlatLayout l;
  l.pa4 = ((W + VT_COLS - 1) / VT_COLS) * (VT_COLS / 4);
  const size_t plane = (size_t)H * l.pa4 * 4;            // one byte per column
  ScratchCursor c;
  l.s = c.take(plane); c.take(plane);                    // two bytes per column: two planes
  l.a = l.s;
  l.m = c.take(plane);
  l.total = c.total();
  return l;
}

__device__ __forceinline__ uint32_t max4(uint32_t a, uint32_t b) {            // byte-wise max
  uint32_t r = 0;
#pragma unroll
  for (int j = 0; j < 32; j += 8) r |= max((a >> j) & 0xffu, (b >> j) & 0xffu) << j;
  return r;
}

// the 4 bytes at byte offset b >= 0 of a word array of nw words; bytes beyond the array are 0
__device__ __forceinline__ uint32_t ldu(const uint32_t* w, int nw, int b) {
  const int i = b >> 2;
  const uint32_t lo = i < nw ? w[i] : 0u, hi = i + 1 < nw ? w[i + 1] : 0u;
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (b & 3)));
}

__global__ __launch_bounds__(256) void flat_hmax_kernel(const uint8_t* __restrict__ page, int64_t pitch, int H, int W, int r, int p, uint32_t inv,
                                                        uint32_t* __restrict__ A, int pa4) {
  __shared__ __attribute__((aligned(16))) uint32_t buf[HROWS][2][HM_WORDS];           // rows of whole 16-byte chunks
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int y = blockIdx.y * HROWS + wave;
  const bool live = y < H;                               // every wave takes every barrier
  const int X0 = blockIdx.x * HSEG, X1 = min(X0 + HSEG, W);
  const uint8_t* row = page + (int64_t)(live ? y : 0) * pitch;
  int xb = X0 - r;                                       // the tile's first column: the last one <= X0 - r whose address is 16-byte aligned
  xb -= (xb + (int)((uintptr_t)row & 15u)) & 15;
  const int T = (X1 + r - xb + 15) & ~15;                // <= HSEG + 2r + 30
  const int nw = T >> 2;
  uint32_t* cur = buf[wave][0];
  uint32_t* nxt = buf[wave][1];
  if (live) {
    for (int q = lane; q < (T >> 4); q += 64) {
      const int x = xb + (q << 4);
      if (x >= 0 && x + 16 <= W) {                       // a whole aligned chunk inside the row
        uint4 v = *reinterpret_cast<const uint4*>(row + x);
        v.x ^= inv; v.y ^= inv; v.z ^= inv; v.w ^= inv;
        *reinterpret_cast<uint4*>(cur + (q << 2)) = v;
      } else {
        for (int j = 0; j < 4; ++j) {
          uint32_t w = 0;
          for (int b = 0; b < 4; ++b) {
            const int xx = x + 4 * j + b;
            if ((unsigned)xx < (unsigned)W) w |= ((uint32_t)row[xx] ^ (inv & 0xffu)) << (8 * b);
          }
          cur[(q << 2) + j] = w;
        }
      }
    }
  }
  __syncthreads();
  for (int k = 1; k < p; k <<= 1) {                      // m_k -> m_2k
    if (live)
      for (int j = lane; j < nw; j += 64) nxt[j] = max4(cur[j], ldu(cur, nw, 4 * j + k));
    __syncthreads();
    uint32_t* t = cur; cur = nxt; nxt = t;
  }
  if (live) {
    uint32_t* a = A + (size_t)y * pa4 + (X0 >> 2);
    for (int i = lane; i < ((X1 - X0 + 3) >> 2); i += 64) {   // whole words: the columns >= W of the last one are never read as pixels
      const int u = X0 + 4 * i - xb;                     // >= r
      a[i] = max4(ldu(cur, nw, u - r), ldu(cur, nw, u + r - p + 1));
    }
  }
}

__global__ __launch_bounds__(256) void flat_vmax_kernel(const uint32_t* __restrict__ A, int pa4, int H, int nw4, int r, int p,
                                                        uint32_t* __restrict__ M) {
  extern __shared__ __attribute__((aligned(16))) uint32_t vbuf[];             // 2 x (VT_ROWS + 2r) rows of 16 words
  const int T = VT_ROWS + 2 * r;
  uint32_t* cur = vbuf;
  uint32_t* nxt = vbuf + T * 16;
  const int c = threadIdx.x & 15, t0 = threadIdx.x >> 4;
  const int xw = blockIdx.x * 16 + c, y0 = blockIdx.y * VT_ROWS;
  const bool live = xw < nw4;
  for (int t = t0; t < T; t += 16) {
    const int y = y0 - r + t;
    cur[t * 16 + c] = (live && (unsigned)y < (unsigned)H) ? A[(size_t)y * pa4 + xw] : 0u;
  }
  __syncthreads();
  for (int k = 1; k < p; k <<= 1) {
    for (int t = t0; t < T; t += 16) nxt[t * 16 + c] = max4(cur[t * 16 + c], t + k < T ? cur[(t + k) * 16 + c] : 0u);
    __syncthreads();
    uint32_t* t = cur; cur = nxt; nxt = t;
  }
  for (int j = t0; j < VT_ROWS; j += 16) {
    const int y = y0 + j;                                // tile row j is page row y - r: the window of y starts there
    if (live && y < H) M[(size_t)y * pa4 + xw] = max4(cur[j * 16 + c], cur[(j + 2 * r + 1 - p) * 16 + c]);
  }
}

__global__ __launch_bounds__(256) void flat_vsum_kernel(const uint32_t* __restrict__ M, int pa4, int H, int nw4, int r, uint2* __restrict__ S) {
  const int xw = blockIdx.x * VS_WORDS + (threadIdx.x & 63);
  const int y0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * VS_ROWS;
  if (xw >= nw4 || y0 >= H) return;
  const int y1 = min(y0 + VS_ROWS, H);
  const uint32_t* col = M + xw;
  uint32_t e = 0, o = 0;                                 // columns 0 and 2, 1 and 3 of the word as 16-bit halves
  for (int y = max(y0 - r, 0); y <= min(y0 + r, H - 1); ++y) {
    const uint32_t w = col[(size_t)y * pa4];
    e += w & 0x00ff00ffu; o += (w >> 8) & 0x00ff00ffu;
  }
#pragma unroll 4
  for (int y = y0; y < y1; ++y) {
    S[(size_t)y * pa4 + xw] = make_uint2((e & 0xffffu) | (o << 16), (e >> 16) | (o & 0xffff0000u));
    if (y + r + 1 < H) {
      const uint32_t w = col[(size_t)(y + r + 1) * pa4];
      e += w & 0x00ff00ffu; o += (w >> 8) & 0x00ff00ffu;
    }
    if (y - r >= 0) {
      const uint32_t w = col[(size_t)(y - r) * pa4];
      e -= w & 0x00ff00ffu; o -= (w >> 8) & 0x00ff00ffu;
    }
  }
}

__global__ __launch_bounds__(256) void flat_div_kernel(const uint8_t* __restrict__ page, int64_t pitch, int H, int W, int r, uint32_t inv,
                                                       const uint16_t* __restrict__ S, int ps, uint8_t* __restrict__ out, int64_t out_pitch) {
  __shared__ uint32_t P[HROWS][64 * PCH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int y = blockIdx.y * HROWS + wave;
  const bool live = y < H;
  const int X0 = blockIdx.x * HSEG, X1 = min(X0 + HSEG, W), xb = X0 - r;
  uint32_t* Pw = P[wave];
  const uint16_t* srow = S + (size_t)(live ? y : 0) * ps;
  for (int u = lane; u < 64 * PCH; u += 64) {            // entry u is column xb + u; columns outside the page add nothing
    const int x = xb + u;
    Pw[u] = (live && (unsigned)x < (unsigned)W) ? (uint32_t)srow[x] : 0u;
  }
  __syncthreads();
  uint32_t run = 0;
#pragma unroll
  for (int i = 0; i < PCH; ++i) {                        // exclusive prefix inside the lane's chunk
    const uint32_t t = Pw[lane * PCH + i];
    Pw[lane * PCH + i] = run;
    run += t;
  }
  uint32_t incl = run;                                   // <= 64 * PCH * 65025 < 2^32
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(incl, d);
    if (lane >= d) incl += t;
  }
  const uint32_t base = incl - run;
#pragma unroll
  for (int i = 0; i < PCH; ++i) Pw[lane * PCH + i] += base;
  __syncthreads();                                       // Pw[u] = the sum of S over the columns xb .. xb + u - 1
  if (!live) return;
  const uint32_t ny = (uint32_t)(min(y + r, H - 1) - max(y - r, 0) + 1), inv8 = inv & 0xffu;
  const uint8_t* prow = page + (int64_t)y * pitch;
  auto px = [&](int u) -> uint32_t {                     // column X0 + u of the page, 0 <= u < X1 - X0
    const int x = X0 + u;
    const int lo = max(x - r, 0), hi = min(x + r, W - 1);
    const uint32_t n = (uint32_t)(hi - lo + 1) * ny;
    const uint32_t B = (Pw[hi + 1 - xb] - Pw[lo - xb] + (n >> 1)) / n;
    const uint32_t Bc = max(B, 1u), v = (uint32_t)prow[x] ^ inv8;
    return min(255u, (v * 255u + (Bc >> 1)) / Bc) ^ inv8;
  };
  wave_store_row(out + (int64_t)y * out_pitch + X0, X1 - X0, lane, px, px16_of(px));
}

}  // namespace

size_t flatten_scratch_bytes(int H, int W) { return flat_layout(H, W).total; }

void flatten_page(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_flatten_params& fp, void* scratch, uint8_t* out,
                  int64_t out_pitch) {
  const FlatLayout l = flat_layout(H, W);
  uint32_t* A = scratch_at<uint32_t>(scratch, l.a);
  uint32_t* M = scratch_at<uint32_t>(scratch, l.m);
  uint2* S = scratch_at<uint2>(scratch, l.s);
  const int r = fp.radius, nw4 = (W + 3) / 4;
  const uint32_t inv = fp.light_text ? 0xffffffffu : 0u;
  int p = 1;                                             // the largest power of two <= 2r + 1
  while (2 * p <= 2 * r + 1) p *= 2;
  const dim3 rows(cdiv(W, HSEG), cdiv(H, HROWS));
  hipLaunchKernelGGL(flat_hmax_kernel, rows, dim3(256), 0, s, page, pitch, H, W, r, p, inv, A, l.pa4);
  hipLaunchKernelGGL(flat_vmax_kernel, dim3(cdiv(nw4, 16), cdiv(H, VT_ROWS)), dim3(256), (size_t)2 * (VT_ROWS + 2 * r) * 16 * sizeof(uint32_t), s,
                     A, l.pa4, H, nw4, r, p, M);
  hipLaunchKernelGGL(flat_vsum_kernel, dim3(cdiv(nw4, VS_WORDS), cdiv(cdiv(H, VS_ROWS), 4)), dim3(256), 0, s, M, l.pa4, H, nw4, r, S);
  hipLaunchKernelGGL(flat_div_kernel, rows, dim3(256), 0, s, page, pitch, H, W, r, inv, reinterpret_cast<const uint16_t*>(S), l.pa4 * 4, out,
                     out_pitch);
}

}  // namespace aocr
