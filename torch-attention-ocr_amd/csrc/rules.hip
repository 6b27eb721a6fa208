// rules.hip -- rule removal that keeps the text (include/aocr.h: aocr_remove_rules): a rule is long one way and thin the other, and a stroke
// that crosses it is not thin, so the decision is made per pixel from run lengths and not per connected component.  Integer arithmetic only
// (the Otsu threshold, when asked for, comes from segment.hip's otsu_threshold); every result is a function of the page and the params:
// tests/rules_ref.py, which measures the run of every pixel, matches exactly.
//
// Everything after the row pass works on bit planes, one uint64 per 64 columns of a row (bit j of word i of row y: column 64 i + j; the
// bits past W are 0), so that one thread decides 64 pixels with a handful of word operations:
//   (Otsu only) otsu_threshold of segment.hip: memset, hist_kernel, otsu_kernel.
//   rules_row_kernel    one wave per row, RULES_ROWS rows per workgroup.  Thresholds the page bytes (wave_row16: one read of every byte) into
//                       the row's ink words in LDS, then marks Hc: a lane owns at most RULES_LANE_WORDS neighbouring words, the run that
//                       reaches a lane's first word from the left and its last word from the right come from two wave scans of
//                       (all ink, run at the end), and mark_runs does the rest per word.  Writes the ink plane and the Hc plane, adds the ink.
//   rules_col_summary   one wave per RULES_CHUNK rows x 64 columns: 64 ballots turn the 64 row words into one column mask per lane; writes
//                       the leading and the trailing run of every (chunk, column).
//   rules_col_scan      one thread per column, over the at most 16384 / RULES_CHUNK = 256 chunk summaries, down and up: the run that reaches
//                       every chunk from above and from below.
//   rules_col_mark      the tiles of rules_col_summary again: mark_runs on the column mask, 64 ballots back to row words, the Vc plane.
//   rules_apply_kernel  one wave per row, RULES_ROWS rows per workgroup.  Per word: cross = Hc & Vc; a column run is longer than T exactly
//                       when T + 1 rows in a row through the pixel are ink, which the prefix ANDs of the rows above and below give for 64
//                       columns at once (the same along the row with shifts over the neighbouring words); the Hc / Vc bits within `edge`
//                       and inside the run are ORed under the same prefixes.  The erase words go to LDS, wave_store_row writes the row, the
//                       counts are added per workgroup in LDS and then once per workgroup with integer atomics.
// No workgroup waits on another.  Every loop is bounded by a constant or by the page: the walks of a row by W / 16 / 64 + 2 turns, a lane's
// words by RULES_LANE_WORDS, the scans by 6 steps, the ballots by 64, rules_col_scan by cdiv(H, RULES_CHUNK) <= 256 turns each way, the
// prefix ANDs by T <= RULES_MAX_T.  Integer sums only: no result depends on the launch geometry or on the order of the atomics.
#include <cstddef>
#include "ops.h"
#include "page_common.h"

namespace aocr {

namespace {

constexpr int RULES_WORD = 64;                 // columns of a word of a bit plane
constexpr int RULES_CHUNK = 64;                // rows of a chunk of the column passes: one wave holds a chunk of 64 columns, a row per lane
constexpr int RULES_ROWS = 4;                  // rows of a workgroup of the row pass and of the apply pass: one wave each
constexpr int RULES_THREADS = 256;
constexpr int RULES_LANE_WORDS = 4;            // words of a row that one lane owns in the row pass: 64 lanes x 4 words x 64 columns = 16384
constexpr int RULES_ROW_WORDS = 256;           // words of the longest row
constexpr int RULES_MAX_T = 16;                // max_thick
static_assert(RULES_THREADS == RULES_ROWS * 64 && RULES_CHUNK == 64 && RULES_WORD == 64, "a wave per row; a chunk is one ballot");
static_assert(64 * RULES_LANE_WORDS == RULES_ROW_WORDS && RULES_ROW_WORDS * RULES_WORD == 16384, "the widest page");

enum { HDR_THR = 0, HDR_COUNTS = 8, HDR_WORDS = 64 };   // words of hdr; hdr[HDR_THR] is otsu_kernel's; the counts live here when counts_dev is NULL
enum { CNT_THR = 0, CNT_INK, CNT_ERASED, CNT_CROSS, CNT_BYH, CNT_BYV, CNT_KEPT };

struct RulesLayout {                           // byte offsets into scratch_dev
  size_t hist, hdr, ink, hc, vc, col, total;
  int w64, nch;
};

RulesLayout rules_layout(int H, int W) {
  RulesLayout l;
  ScratchCursor c;
  l.w64 = cdiv(W, RULES_WORD);
  l.nch = cdiv(H, RULES_CHUNK);
  l.hist = c.take(256 * sizeof(uint32_t));
  l.hdr = c.take(HDR_WORDS * sizeof(int32_t));
  l.ink = c.take((size_t)H * l.w64 * sizeof(uint64_t));
  l.hc = c.take((size_t)H * l.w64 * sizeof(uint64_t));
  l.vc = c.take((size_t)H * l.w64 * sizeof(uint64_t));
  l.col = c.take((size_t)l.nch * l.w64 * RULES_WORD * sizeof(uint32_t));
  l.total = c.total();
  return l;
}

constexpr uint64_t ALL = ~0ull;

// the ink runs of 64 pixels in a line (bit 0 first) that are part of a run of at least L pixels, when a run of `before` ink pixels ends
// right in front of bit 0 and one of `after` starts right behind bit 63.  Shifts stay below 64: t, tr in 1..63 where they are used, and the
// opening's k and L - k are at most L / 2 and L < 64.
__device__ __forceinline__ uint64_t mark_runs(uint64_t m, int before, int after, int L) {
  if (m == ALL) return before + 64 + after >= L ? ALL : 0ull;
  uint64_t out = 0;
  const int t = __ffsll((long long)~m) - 1;              // the leading run, 0..63
  if (t > 0 && before + t >= L) out |= (1ull << t) - 1;
  const int tr = __clzll((long long)~m);                 // the trailing run, 0..63
  if (tr > 0 && tr + after >= L) out |= ALL << (64 - tr);
  if (L < 64) {                                          // runs inside the word: the opening by L pixels, log2(L) <= 6 steps each way
    uint64_t e = m;
    int k = 1;
    for (; 2 * k <= L; k *= 2) e &= e >> k;              // bit r: pixels r .. r + k - 1 are ink
    if (k < L) e &= e >> (L - k);
    uint64_t d = e;
    k = 1;
    for (; 2 * k <= L; k *= 2) d |= d << k;
    if (k < L) d |= d << (L - k);
    out |= d;
  }
  return out;
}

__device__ __forceinline__ int lead_run(uint64_t m) { return m == ALL ? 64 : __ffsll((long long)~m) - 1; }
__device__ __forceinline__ int trail_run(uint64_t m) { return m == ALL ? 64 : __clzll((long long)~m); }

// ---- the row pass ---------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(RULES_THREADS) void rules_row_kernel(const uint8_t* __restrict__ page, int64_t pitch, int H, int W, int light, int fixed,
                                                                  const int32_t* __restrict__ hdr, int axes, int L, int w64,
                                                                  uint64_t* __restrict__ inkp, uint64_t* __restrict__ hcp, int32_t* counts) {
  __shared__ uint64_t bits[RULES_ROWS][RULES_ROW_WORDS];
  __shared__ int block_ink;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int y = blockIdx.x * RULES_ROWS + wave;
  const int thr = ink_thr(fixed, hdr + HDR_THR);
  for (int i = lane; i < w64; i += 64) bits[wave][i] = 0;
  if (threadIdx.x == 0) block_ink = 0;
  __syncthreads();
  if (y < H && thr >= 0) {
    uint32_t* b32 = reinterpret_cast<uint32_t*>(bits[wave]);
    wave_row16(page + (int64_t)y * pitch, W, lane,
               [&](int x, uint32_t b) { if (is_ink((int)b, thr, light)) atomicOr(&b32[x >> 5], 1u << (x & 31)); },
               [&](int x, const uint4& q) {
                 const uint32_t m = ink_mask16(q, thr, light);
                 const int s = x & 31;
                 if (m) {
                   atomicOr(&b32[x >> 5], m << s);
                   if (s > 16 && (m >> (32 - s))) atomicOr(&b32[(x >> 5) + 1], m >> (32 - s));     // x + 15 < W: the next word exists
                 }
               });
  }
  __syncthreads();
  int ink = 0;
  if (y < H) {
    const int nw = (w64 + 63) >> 6;                      // 1..RULES_LANE_WORDS: lane l owns the words l * nw .. l * nw + nw - 1 below w64
    const int first = lane * nw;
    uint64_t m[RULES_LANE_WORDS];
    int full = 1, tail = 0, head = 0, head_open = 1;     // of the lane's words: all ink; the run at their end; the run at their start
#pragma unroll
    for (int j = 0; j < RULES_LANE_WORDS; ++j) {
      const bool have = j < nw && first + j < w64;
      m[j] = have ? bits[wave][first + j] : ALL;         // a word the lane does not own is the scan's identity
      if (!have) continue;
      ink += __popcll(m[j]);
      if (m[j] == ALL) { tail += 64; } else { full = 0; tail = trail_run(m[j]); }
      if (head_open) { head += lead_run(m[j]); head_open = m[j] == ALL; }
    }
    // before: the run that ends in front of the lane's first word.  An inclusive scan of (full, tail) from the left, 6 steps, then one lane up
    int f = full, t = tail;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int of = __shfl_up(f, d), ot = __shfl_up(t, d);
      if (lane >= d) { t = f ? ot + t : t; f = f && of; }
    }
    int before = __shfl_up(t, 1);
    if (lane == 0) before = 0;
    // after: the run that starts behind the lane's last word.  The same from the right with (full, head)
    f = full;
    int h = head;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int of = __shfl_down(f, d), oh = __shfl_down(h, d);
      if (lane + d < 64) { h = f ? h + oh : h; f = f && of; }
    }
    int after_all = __shfl_down(h, 1);
    if (lane == 63) after_all = 0;
    int after[RULES_LANE_WORDS];                         // behind every word of the lane: from the lane's last word back
    int a = after_all;
#pragma unroll
    for (int j = RULES_LANE_WORDS - 1; j >= 0; --j) {
      after[j] = a;
      if (j < nw && first + j < w64) a = m[j] == ALL ? a + 64 : lead_run(m[j]);
    }
    int b = before;
#pragma unroll
    for (int j = 0; j < RULES_LANE_WORDS; ++j) {
      if (!(j < nw && first + j < w64)) continue;
      const size_t at = (size_t)y * w64 + first + j;
      inkp[at] = m[j];
      hcp[at] = (axes & 1) ? mark_runs(m[j], b, after[j], L) : 0ull;
      b = m[j] == ALL ? b + 64 : trail_run(m[j]);
    }
  }
  ink = wave_sum(ink);
  if (lane == 0 && ink) atomicAdd(&block_ink, ink);
  __syncthreads();
  if (threadIdx.x == 0 && block_ink) atomicAdd(&counts[CNT_INK], block_ink);
}

// ---- the column passes ----------------------------------------------------------------------------------------------------------------------

// lane c gets the mask of column c over the chunk's rows (bit r: row r) from the row words (lane r: row r); 64 ballots
__device__ __forceinline__ uint64_t transpose64(uint64_t w, int lane) {
  uint64_t mine = 0;
#pragma unroll 8
  for (int c = 0; c < 64; ++c) {
    const uint64_t b = __ballot((w >> c) & 1);
    if (lane == c) mine = b;
  }
  return mine;
}

__device__ __forceinline__ uint64_t chunk_columns(const uint64_t* __restrict__ inkp, int H, int w64, int wx, int k, int lane) {
  const int y = k * RULES_CHUNK + lane;
  return transpose64(y < H ? inkp[(size_t)y * w64 + wx] : 0ull, lane);   // rows past H are paper: a run ends at the page's edge
}

__global__ __launch_bounds__(RULES_THREADS) void rules_col_summary(const uint64_t* __restrict__ inkp, int H, int w64, uint32_t* __restrict__ col) {
  const int lane = threadIdx.x & 63;
  const int wx = blockIdx.x * RULES_ROWS + (threadIdx.x >> 6), k = blockIdx.y;
  if (wx >= w64) return;                                 // the whole wave
  const uint64_t c = chunk_columns(inkp, H, w64, wx, k, lane);
  col[((size_t)k * w64 + wx) * RULES_WORD + lane] = (uint32_t)lead_run(c) | ((uint32_t)trail_run(c) << 8);
}

// in: lead | trail << 8 per (chunk, column).  out: above | below << 16, the runs that reach the chunk from above and from below (<= 16384)
__global__ __launch_bounds__(RULES_THREADS) void rules_col_scan(uint32_t* __restrict__ col, int nch, int cols) {
  const int x = blockIdx.x * RULES_THREADS + threadIdx.x;
  if (x >= cols) return;
  int above = 0;
  for (int k = 0; k < nch; ++k) {                        // nch <= 256
    uint32_t* p = col + (size_t)k * cols + x;
    const uint32_t s = *p;
    *p = (s & 0xffffu) | ((uint32_t)above << 16);
    above = (s & 0xffu) == 64 ? above + 64 : (int)((s >> 8) & 0xffu);
  }
  int below = 0;
  for (int k = nch - 1; k >= 0; --k) {
    uint32_t* p = col + (size_t)k * cols + x;
    const uint32_t s = *p;
    *p = (s >> 16) | ((uint32_t)below << 16);
    below = (s & 0xffu) == 64 ? below + 64 : (int)(s & 0xffu);
  }
}

__global__ __launch_bounds__(RULES_THREADS) void rules_col_mark(const uint64_t* __restrict__ inkp, int H, int w64, const uint32_t* __restrict__ col, int L,
                                                                uint64_t* __restrict__ vcp) {
  const int lane = threadIdx.x & 63;
  const int wx = blockIdx.x * RULES_ROWS + (threadIdx.x >> 6), k = blockIdx.y;
  if (wx >= w64) return;                                 // the whole wave
  const uint64_t c = chunk_columns(inkp, H, w64, wx, k, lane);
  const uint32_t s = col[((size_t)k * w64 + wx) * RULES_WORD + lane];
  const uint64_t rows = transpose64(mark_runs(c, (int)(s & 0xffffu), (int)(s >> 16), L), lane);
  const int y = k * RULES_CHUNK + lane;
  if (y < H) vcp[(size_t)y * w64 + wx] = rows;
}

// ---- the apply pass -------------------------------------------------------------------------------------------------------------------------

struct RulePlanes {
  const uint64_t* ink;
  const uint64_t* hc;
  const uint64_t* vc;                                    // nullptr: no vertical rules asked for
  int H, w64;
  __device__ __forceinline__ uint64_t at(const uint64_t* p, int y, int i) const {
    return (y >= 0 && y < H && i >= 0 && i < w64) ? p[(size_t)y * w64 + i] : 0ull;
  }
};

// the pixels k columns to the right (left) of the word's own, 1 <= k <= 16
__device__ __forceinline__ uint64_t from_right(uint64_t c, uint64_t r, int k) { return (c >> k) | (r << (64 - k)); }
__device__ __forceinline__ uint64_t from_left(uint64_t c, uint64_t l, int k) { return (c << k) | (l >> (64 - k)); }

template <int T>
__global__ __launch_bounds__(RULES_THREADS) void rules_apply_kernel(const uint8_t* __restrict__ page, int64_t pitch, int H, int W, RulePlanes P, int e,
                                                                    int fill, uint8_t* __restrict__ out, int64_t out_pitch, int fixed,
                                                                    const int32_t* __restrict__ hdr, int32_t* counts) {
  __shared__ uint64_t er[RULES_ROWS][RULES_ROW_WORDS];
  __shared__ int block_n[5];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int y = blockIdx.x * RULES_ROWS + wave;
  if (threadIdx.x < 5) block_n[threadIdx.x] = 0;
  int n_erased = 0, n_cross = 0, n_h = 0, n_v = 0, n_kept = 0;
  if (y < H) {
    for (int i = lane; i < P.w64; i += 64) {             // at most RULES_LANE_WORDS turns
      const uint64_t c = P.at(P.ink, y, i), hc = P.at(P.hc, y, i), vc = P.vc ? P.at(P.vc, y, i) : 0ull;
      uint64_t erase = 0;
      if (hc | vc) {
        erase = hc & vc;
        n_cross += __popcll(erase);
      }
      if (c) {
        // along the column: up[k] (dn[k]): the k rows above (below) are ink like the pixel.  The column run is longer than T exactly when
        // up[i] & dn[T - i] for some i; a row within e that is joined to the pixel by ink lies inside the run
        uint64_t up[T + 1], dn[T + 1];
        up[0] = dn[0] = c;
        uint64_t hit = hc;
#pragma unroll
        for (int k = 1; k <= T; ++k) {
          up[k] = up[k - 1] & P.at(P.ink, y - k, i);
          dn[k] = dn[k - 1] & P.at(P.ink, y + k, i);
          if (k <= e && k <= 4) hit |= (up[k] & P.at(P.hc, y - k, i)) | (dn[k] & P.at(P.hc, y + k, i));
        }
        uint64_t tall = 0;
#pragma unroll
        for (int k = 0; k <= T; ++k) tall |= up[k] & dn[T - k];
        const uint64_t by_h = hit & ~tall & ~erase;
        n_h += __popcll(by_h);
        // along the row: the same with the neighbouring words shifted in
        uint64_t by_v = 0;
        if (P.vc) {
          const uint64_t cl = P.at(P.ink, y, i - 1), cr = P.at(P.ink, y, i + 1);
          const uint64_t vl = P.at(P.vc, y, i - 1), vr = P.at(P.vc, y, i + 1);
          uint64_t lf[T + 1], rt[T + 1];
          lf[0] = rt[0] = c;
          uint64_t hitv = vc;
#pragma unroll
          for (int k = 1; k <= T; ++k) {
            lf[k] = lf[k - 1] & from_left(c, cl, k);
            rt[k] = rt[k - 1] & from_right(c, cr, k);
            if (k <= e && k <= 4) hitv |= (lf[k] & from_left(vc, vl, k)) | (rt[k] & from_right(vc, vr, k));
          }
          uint64_t wide = 0;
#pragma unroll
          for (int k = 0; k <= T; ++k) wide |= lf[k] & rt[T - k];
          by_v = hitv & ~wide & ~erase & ~by_h;
          n_v += __popcll(by_v);
        }
        erase |= by_h | by_v;
      }
      n_erased += __popcll(erase);
      n_kept += __popcll((hc | vc) & ~erase);
      er[wave][i] = erase;
    }
  }
  __syncthreads();
  if (y < H) {
    const uint8_t* __restrict__ src = page + (int64_t)y * pitch;
    const uint64_t* mine = er[wave];
    auto px1 = [&](int x) -> uint32_t { return ((mine[x >> 6] >> (x & 63)) & 1) ? (uint32_t)fill : (uint32_t)src[x]; };
    auto px16 = [&](int x) -> uint4 {
      const int s = x & 63;
      uint32_t bits16 = (uint32_t)(mine[x >> 6] >> s);
      if (s > 48) bits16 |= (uint32_t)(mine[(x >> 6) + 1] << (64 - s));      // x + 15 < W: the next word exists
      bits16 &= 0xffffu;
      uint32_t w[4];
      if ((((uintptr_t)(src + x)) & 15u) == 0) {
        const uint4 q = *reinterpret_cast<const uint4*>(src + x);
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          w[j] = (uint32_t)src[x + 4 * j] | ((uint32_t)src[x + 4 * j + 1] << 8) | ((uint32_t)src[x + 4 * j + 2] << 16) | ((uint32_t)src[x + 4 * j + 3] << 24);
      }
      if (bits16) {
        const uint32_t f4 = (uint32_t)fill * 0x01010101u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t b = (bits16 >> (4 * j)) & 15u;
          const uint32_t sel = ((b & 1u) ? 0xffu : 0u) | ((b & 2u) ? 0xff00u : 0u) | ((b & 4u) ? 0xff0000u : 0u) | ((b & 8u) ? 0xff000000u : 0u);
          w[j] = (w[j] & ~sel) | (f4 & sel);
        }
      }
      uint4 q;
      q.x = w[0]; q.y = w[1]; q.z = w[2]; q.w = w[3];
      return q;
    };
    wave_store_row(out + (int64_t)y * out_pitch, W, lane, px1, px16);
  }
  n_erased = wave_sum(n_erased); n_cross = wave_sum(n_cross); n_h = wave_sum(n_h); n_v = wave_sum(n_v); n_kept = wave_sum(n_kept);
  if (lane == 0) {
    if (n_erased) atomicAdd(&block_n[0], n_erased);
    if (n_cross) atomicAdd(&block_n[1], n_cross);
    if (n_h) atomicAdd(&block_n[2], n_h);
    if (n_v) atomicAdd(&block_n[3], n_v);
    if (n_kept) atomicAdd(&block_n[4], n_kept);
  }
  __syncthreads();
  if (threadIdx.x < 5 && block_n[threadIdx.x]) atomicAdd(&counts[CNT_ERASED + threadIdx.x], block_n[threadIdx.x]);
  if (blockIdx.x == 0 && threadIdx.x == 0) counts[CNT_THR] = ink_thr(fixed, hdr + HDR_THR);
}

template <int T>
void launch_apply(hipStream_t s, int blocks, const uint8_t* page, int64_t pitch, int H, int W, const RulePlanes& P, int e, int fill, uint8_t* out,
                  int64_t out_pitch, int fixed, const int32_t* hdr, int32_t* counts) {
  hipLaunchKernelGGL(rules_apply_kernel<T>, dim3(blocks), dim3(RULES_THREADS), 0, s, page, pitch, H, W, P, e, fill, out, out_pitch, fixed, hdr, counts);
}

}  // namespace

size_t rules_scratch_bytes(int H, int W) { return rules_layout(H, W).total; }

void remove_rules(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_rule_params& p, void* scratch, uint8_t* out,
                  int64_t out_pitch, int32_t* counts) {
  const RulesLayout l = rules_layout(H, W);
  uint32_t* hist = scratch_at<uint32_t>(scratch, l.hist);
  int32_t* hdr = scratch_at<int32_t>(scratch, l.hdr);
  uint64_t* inkp = scratch_at<uint64_t>(scratch, l.ink);
  uint64_t* hcp = scratch_at<uint64_t>(scratch, l.hc);
  uint64_t* vcp = scratch_at<uint64_t>(scratch, l.vc);
  uint32_t* col = scratch_at<uint32_t>(scratch, l.col);
  if (!counts) counts = hdr + HDR_COUNTS;
  const int light = p.light_text ? 1 : 0, fixed = p.threshold, L = p.min_len;
  const int row_blocks = cdiv(H, RULES_ROWS);
  (void)hipMemsetAsync(counts, 0, 8 * sizeof(int32_t), s);
  page_threshold(s, page, pitch, H, W, fixed, hist, hdr + HDR_THR);
  hipLaunchKernelGGL(rules_row_kernel, dim3(row_blocks), dim3(RULES_THREADS), 0, s, page, pitch, H, W, light, fixed, hdr, p.axes, L, l.w64, inkp, hcp,
                     counts);
  const bool vertical = (p.axes & 2) != 0;
  if (vertical) {
    const dim3 tiles(cdiv(l.w64, RULES_ROWS), l.nch);
    const int cols = l.w64 * RULES_WORD;
    hipLaunchKernelGGL(rules_col_summary, tiles, dim3(RULES_THREADS), 0, s, inkp, H, l.w64, col);
    hipLaunchKernelGGL(rules_col_scan, dim3(cdiv(cols, RULES_THREADS)), dim3(RULES_THREADS), 0, s, col, l.nch, cols);
    hipLaunchKernelGGL(rules_col_mark, tiles, dim3(RULES_THREADS), 0, s, inkp, H, l.w64, col, L, vcp);
  }
  const RulePlanes P{inkp, hcp, vertical ? vcp : nullptr, H, l.w64};
  const int fill = light ? 0 : 255;
#define APPLY(T) case T: launch_apply<T>(s, row_blocks, page, pitch, H, W, P, p.edge, fill, out, out_pitch, fixed, hdr, counts); break;
  switch (p.max_thick) {
    APPLY(1) APPLY(2) APPLY(3) APPLY(4) APPLY(5) APPLY(6) APPLY(7) APPLY(8) APPLY(9) APPLY(10) APPLY(11) APPLY(12) APPLY(13) APPLY(14) APPLY(15)
    APPLY(16)
  }
#undef APPLY
  static_assert(RULES_MAX_T == 16, "one instance of rules_apply_kernel per max_thick");
}

}  // namespace aocr
