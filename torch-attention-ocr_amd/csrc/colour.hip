// colour.hip -- colour pages (include/aocr.h: aocr_estimate_page_colour, aocr_gray_page), the stage in front of every other page stage: an
// interleaved RGB page becomes the gray page the rest of the chain reads.  The paper colour is estimated from three channel histograms, every
// channel is stretched so that the paper becomes 255, and a pixel whose chroma marks it as coloured can be replaced by paper according to
// its hue class.  Integer arithmetic only, so tests/colour_ref.py matches exactly.
//
// Launches of one aocr_estimate_page_colour, all on the caller's stream, the histograms in the caller's scratch:
//   memset           the 3 x 256 bins.
//   hist3_kernel     one wave per row of 3W bytes.  A lane takes 48 consecutive bytes (three aligned 16-byte loads), so the channel of the
//                    lane's first byte is the same in every lane and the channel of every byte is known at compile time inside one of
//                    three instantiations; the row's head and tail go byte by byte with channel = index % 3.  The channel never comes from
//                    an address.  3 x 256 bins in LDS per wave, flushed with integer global atomics (order-independent: exact), as in
//                    segment.hip's hist_kernel; 48 bytes that are 16 equal pixels (paper) take three adds of 16.
//   paper_kernel     one workgroup: thread v scores bin v of every channel by the five-bin window sum and the three winners are taken by
//                    "larger sum, then larger v" with a 64-bit key; writes the 16 words.
// Launches of one aocr_gray_page:
//   begin_kernel     (colour_out_dev only) one wave: the paper used and its flag into words 0..3, zeros into words 4..15.
//   gray_kernel      a wave owns a segment of at most SEG pixels of one row.  The segment's 3n source bytes go into the wave's LDS stage through
//                    aligned 16-byte loads (head and tail bytes singly), stored at the same offset modulo 16 as in memory so that a loaded
//                    vector is one aligned 16-byte LDS store.  The output leaves through wave_store_row: a lane that stores 16 gray bytes
//                    needs 48 staged bytes at LDS address p; p modulo 4 is the same in every lane (lanes are 48 bytes apart), so the lane
//                    takes them in four turns of four pixels: the four aligned words around 12 bytes, lined up by one uniform byte
//                    shift.  (All sixteen pixels unrolled into one block spilled registers and ran three times slower.)  Lanes 12 words
//                    apart meet on 8 of the 32 banks of a 4-byte read: a 4-way conflict, 16 reads per 16 pixels, which stays far below the
//                    kernel's arithmetic (a lane reading pixel by pixel at a stride of three bytes would need 48 byte reads for them).
//                    The three balance tables are built in LDS by every workgroup from the paper words read on the device.  Counts: six
//                    5-bit fields per lane and segment, unpacked into per-lane words, summed over the wave and the workgroup at the end,
//                    then one integer global atomic per non-zero word and workgroup.
#include <algorithm>
#include "ops.h"
#include "page_common.h"

namespace aocr {

namespace {

constexpr int SEG = 1024;                      // pixels of one wave's segment: 64 lanes x 16
constexpr int STAGE = 16 + 3 * SEG + 16;       // the stage of one wave: up to 15 bytes of misalignment in front, one vector of slack behind

struct ColourLayout { size_t hist, total; };   // byte offsets into scratch_dev

ColourLayout colour_layout() {
  ColourLayout l;
  ScratchCursor c;
  l.hist = c.take(3 * 256 * sizeof(uint32_t));
  l.total = c.total();
  return l;
}

// ---- the estimate ----------------------------------------------------------------------------------------------------------------------------

// q[0..11]: 48 consecutive bytes of a row whose first byte has channel PH
template <int PH> __device__ __forceinline__ void hist48(const uint32_t (&q)[12], uint32_t* __restrict__ h) {
  uint32_t diff = 0;                           // 0: byte j equals byte j + 3 for every j < 45, 16 equal pixels
#pragma unroll
  for (int k = 0; k < 11; ++k) diff |= q[k] ^ (uint32_t)((((uint64_t)q[k + 1] << 32) | q[k]) >> 24);
  diff |= (q[11] ^ (q[11] >> 24)) & 0xffu;     // k = 10 ends at bytes 43 and 46: bytes 44 and 47 here
  if (diff == 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j) atomicAdd(&h[((PH + j) % 3) * 256 + ((q[0] >> (8 * j)) & 0xffu)], 16u);
    return;
  }
#pragma unroll
  for (int j = 0; j < 48; ++j) atomicAdd(&h[((PH + j) % 3) * 256 + ((q[j >> 2] >> (8 * (j & 3))) & 0xffu)], 1u);
}

__global__ __launch_bounds__(256) void hist3_kernel(const uint8_t* __restrict__ rgb, int64_t pitch, int H, int W, uint32_t* __restrict__ hist) {
  __shared__ uint32_t sh[4][3 * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < 4 * 3 * 256; i += 256) (&sh[0][0])[i] = 0;
  __syncthreads();
  uint32_t* h = sh[wave];
  const int n = 3 * W;
  for (int y = blockIdx.x * 4 + wave; y < H; y += gridDim.x * 4) {
    const uint8_t* row = rgb + (int64_t)y * pitch;
    const int head = row_head(row, n);
    const int n48 = (n - head) / 48;
    const int ph = head % 3;                   // the channel of the first aligned byte: wave-uniform
    if (lane < head) atomicAdd(&h[(lane % 3) * 256 + row[lane]], 1u);
    const uint4* v = reinterpret_cast<const uint4*>(row + head);
    for (int i = lane; i < n48; i += 64) {
      const uint4 a = v[3 * i], b = v[3 * i + 1], c = v[3 * i + 2];
      const uint32_t q[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
      if (ph == 0) hist48<0>(q, h);
      else if (ph == 1) hist48<1>(q, h);
      else hist48<2>(q, h);
    }
    for (int t = head + 48 * n48 + lane; t < n; t += 64) atomicAdd(&h[(t % 3) * 256 + row[t]], 1u);      // fewer than 48 + 16 bytes
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * 256; i += 256) {
    const uint32_t s = sh[0][i] + sh[1][i] + sh[2][i] + sh[3][i];
    if (s) atomicAdd(&hist[i], s);
  }
}

__global__ __launch_bounds__(256) void paper_kernel(const uint32_t* __restrict__ hist, int paper_min, int32_t* __restrict__ colour) {
  __shared__ uint32_t sh[3][256 + 4];          // two zero bins on either side
  __shared__ uint64_t best[3][4];
  const int v = threadIdx.x, lane = v & 63, wave = v >> 6;
  for (int i = v; i < 3 * 260; i += 256) (&sh[0][0])[i] = 0;
  __syncthreads();
  for (int c = 0; c < 3; ++c) sh[c][v + 2] = hist[c * 256 + v];
  __syncthreads();
  for (int c = 0; c < 3; ++c) {
    // bit 63: some pixel of the channel is >= paper_min; then the window sum (at most 2^26) above the bin
    uint64_t key = 0;
    if (v >= paper_min) {
      const uint64_t s = (uint64_t)sh[c][v] + sh[c][v + 1] + sh[c][v + 2] + sh[c][v + 3] + sh[c][v + 4];
      key = ((uint64_t)(sh[c][v + 2] != 0) << 63) | (s << 8) | (uint64_t)v;
    }
    const uint64_t any = wave_max(key & ((uint64_t)1 << 63)), m = wave_max(key & ~((uint64_t)1 << 63));
    if (lane == 0) best[c][wave] = any | m;
  }
  __syncthreads();
  if (v < 16) {
    int32_t w = 0;
    if (v < 3) {
      uint64_t any = 0, m = 0;
      for (int k = 0; k < 4; ++k) { any |= best[v][k] >> 63; const uint64_t b = best[v][k] & ~((uint64_t)1 << 63); m = b > m ? b : m; }
      w = any ? (int32_t)(m & 0xffu) : 255;
    } else if (v == 3) {
      w = 1;
    }
    colour[v] = w;
  }
}

// ---- the gray page ---------------------------------------------------------------------------------------------------------------------------

struct GrayArgs {
  int wr, wg, wb, mode, chroma_min, drop, fill;
  int paper[3], estimated;                     // used when there are no device words
};

// the paper of a launch: the device words when there are any, clamped to what a division takes
__device__ __forceinline__ int paper_word(const int32_t* words, const GrayArgs& a, int c) {
  return words ? min(max(words[c], 1), 255) : a.paper[c];
}

__global__ __launch_bounds__(64) void begin_kernel(const int32_t* in, GrayArgs a, int32_t* out) {
  const int i = threadIdx.x;
  int32_t w = 0;
  if (i < 3) w = paper_word(in, a, i);
  if (i == 3) w = in ? (in[3] != 0) : a.estimated;
  __syncthreads();                             // out may be in: every word is read before one is written
  if (i < 16) out[i] = w;
}

__global__ __launch_bounds__(256) void gray_kernel(const uint8_t* __restrict__ rgb, int64_t pitch, int H, int W, int seglen, int nseg,
                                                   const int32_t* paper, GrayArgs a, uint8_t* __restrict__ out, int64_t out_pitch,
                                                   int32_t* counts) {
  __shared__ __attribute__((aligned(16))) uint8_t stage_all[4][STAGE];
  __shared__ uint8_t lut[3 * 256];
  __shared__ uint32_t total[8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = 0; c < 3; ++c) {
    const uint32_t p = (uint32_t)paper_word(paper, a, c);
    lut[c * 256 + threadIdx.x] = (uint8_t)min(255u, (threadIdx.x * 255u + p / 2u) / p);
  }
  if (threadIdx.x < 8) total[threadIdx.x] = 0;
  uint8_t* stage = stage_all[wave];
  uint32_t cnt[7] = {0, 0, 0, 0, 0, 0, 0};     // per lane: the six classes, the dropped
  const int items = H * nseg, stride = gridDim.x * 4;
  const int rounds = (items + stride - 1) / stride;      // the same for every wave of the grid: the barriers below are workgroup-uniform
  for (int k = 0; k < rounds; ++k) {
    const int item = k * stride + blockIdx.x * 4 + wave;
    const bool active = item < items;
    const int y = active ? item / nseg : 0, x0 = active ? (item - y * nseg) * seglen : 0;
    const int n = active ? max(min(seglen, W - x0), 0) : 0, nb = 3 * n;
    const uint8_t* src = rgb + (int64_t)y * pitch + 3 * (int64_t)x0;
    const int mis = (int)((uintptr_t)src & 15u);          // source byte i is staged at stage[mis + i]
    __syncthreads();                           // the stage's readers of the round before are done (and, in round 0, the tables are built)
    wave_row16(src, nb, lane, [&](int i, uint32_t b) { stage[mis + i] = (uint8_t)b; },
               [&](int i, const uint4& q) { *reinterpret_cast<uint4*>(stage + mis + i) = q; });
    __syncthreads();
    if (!active) continue;
    uint32_t packed = 0, nd = 0;               // six 5-bit class counts of this lane in this segment: at most 18 pixels
    auto pixel = [&](uint32_t r, uint32_t g, uint32_t b) -> uint32_t {
      const int rr = lut[r], gg = lut[256 + g], bb = lut[512 + b];
      const int mx = max(rr, max(gg, bb)), mn = min(rr, min(gg, bb)), c = mx - mn;
      int cls;
      if (mx == rr) cls = 2 * (gg - bb) >= c ? 1 : (2 * (bb - gg) > c ? 5 : 0);
      else if (mx == gg) cls = 2 * (rr - bb) > c ? 1 : (2 * (bb - rr) >= c ? 3 : 2);
      else cls = 2 * (gg - rr) > c ? 3 : (2 * (rr - gg) >= c ? 5 : 4);
      const uint32_t coloured = c >= a.chroma_min, dropped = coloured & ((uint32_t)a.drop >> cls);
      packed += coloured << (5 * cls);
      nd += dropped;
      const uint32_t gray = a.mode ? (uint32_t)mn : (uint32_t)(a.wr * rr + a.wg * gg + a.wb * bb + 128) >> 8;
      return dropped ? (uint32_t)a.fill : gray;
    };
    auto px1 = [&](int x) -> uint32_t {
      const uint8_t* s = stage + mis + 3 * x;
      return pixel(s[0], s[1], s[2]);
    };
    auto px16 = [&](int x) -> uint4 {
      const int p = mis + 3 * x, sh = 8 * (p & 3);       // sh is wave-uniform: the lanes' x are 16 apart
      const uint32_t* w = reinterpret_cast<const uint32_t*>(stage + (p & ~3));
      uint4 q = {0u, 0u, 0u, 0u};
#pragma unroll 1
      for (int g = 0; g < 4; ++g) {            // four pixels a turn, not unrolled: sixteen pixels in flight together spill
        const uint32_t w0 = w[3 * g], w1 = w[3 * g + 1], w2 = w[3 * g + 2], w3 = w[3 * g + 3];   // w[12] lies inside the stage's slack at the latest
        const uint32_t d[3] = {(uint32_t)((((uint64_t)w1 << 32) | w0) >> sh), (uint32_t)((((uint64_t)w2 << 32) | w1) >> sh),
                               (uint32_t)((((uint64_t)w3 << 32) | w2) >> sh)};                     // the 12 bytes from p + 12 g on
        auto byte = [&](int j) -> uint32_t { return (d[j >> 2] >> (8 * (j & 3))) & 0xffu; };
        const uint32_t four = pixel(byte(0), byte(1), byte(2)) | (pixel(byte(3), byte(4), byte(5)) << 8) |
                              (pixel(byte(6), byte(7), byte(8)) << 16) | (pixel(byte(9), byte(10), byte(11)) << 24);
        q.x = q.y; q.y = q.z; q.z = q.w; q.w = four;     // after four turns the groups stand in order
      }
      return q;
    };
    wave_store_row(out + (int64_t)y * out_pitch + x0, n, lane, px1, px16);
#pragma unroll
    for (int c = 0; c < 6; ++c) cnt[c] += (packed >> (5 * c)) & 31u;
    cnt[6] += nd;
  }
  if (counts) {
#pragma unroll
    for (int c = 0; c < 7; ++c) {
      const uint32_t s = wave_sum(cnt[c]);
      if (lane == 0 && s) atomicAdd(&total[c], s);
    }
    __syncthreads();
    if (threadIdx.x < 7 && total[threadIdx.x]) atomicAdd(&counts[4 + threadIdx.x], (int32_t)total[threadIdx.x]);
  }
}

}  // namespace

size_t colour_scratch_bytes() { return colour_layout().total; }

void estimate_page_colour(hipStream_t s, const uint8_t* rgb, int64_t pitch, int H, int W, const aocr_colour_params& p, void* scratch,
                          int32_t* colour) {
  uint32_t* hist = scratch_at<uint32_t>(scratch, colour_layout().hist);
  (void)hipMemsetAsync(hist, 0, 3 * 256 * sizeof(uint32_t), s);
  hipLaunchKernelGGL(hist3_kernel, dim3(std::min(cdiv(H, 4), 2048)), dim3(256), 0, s, rgb, pitch, H, W, hist);
  hipLaunchKernelGGL(paper_kernel, dim3(1), dim3(256), 0, s, hist, p.paper_min, colour);
}

void gray_page(hipStream_t s, const uint8_t* rgb, int64_t pitch, int H, int W, const aocr_colour_params& p, const int32_t* colour_in,
               int32_t* colour_out, uint8_t* out, int64_t out_pitch) {
  GrayArgs a;
  a.wr = p.weights[0]; a.wg = p.weights[1]; a.wb = p.weights[2];
  a.mode = p.mode; a.chroma_min = p.chroma_min; a.drop = p.drop; a.fill = p.fill;
  const bool given = p.balance && p.paper[0] >= 0;
  for (int c = 0; c < 3; ++c) a.paper[c] = given ? p.paper[c] : 255;
  a.estimated = 0;
  const int32_t* paper = colour_in;
  if (colour_out) {
    hipLaunchKernelGGL(begin_kernel, dim3(1), dim3(64), 0, s, colour_in, a, colour_out);
    paper = colour_out;
  }
  const int nseg = cdiv(W, SEG), seglen = std::min(SEG, (cdiv(W, nseg) + 15) & ~15);
  hipLaunchKernelGGL(gray_kernel, dim3(std::min(cdiv(H * nseg, 4), 2048)), dim3(256), 0, s, rgb, pitch, H, W, seglen, nseg, paper, a, out,
                     out_pitch, colour_out);
}

}  // namespace aocr
