// page_common.h -- what the page kernels share (segment, skew, flatten, layout, components, orient, rectify, scale .hip): the walk of one
// wave over an unaligned row of bytes, for reading and for writing, the ink predicate and the threshold it takes, the wave reductions, and
// on the host the layout of scratch_dev and the Otsu preamble.  Integer arithmetic only: a translation unit's -ffp-contract setting does
// not reach anything here.
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>

namespace aocr {

// ---- one wave, one row of n bytes at any address -----------------------------------------------------------------------------------------------
// A row is a head of fewer than 16 bytes up to the first 16-byte boundary, whole aligned 16-byte words, and a tail of fewer than 16 bytes.
// Lane l takes byte l of the head, the words l, l + 64, ... and byte l of the tail: every byte of the row belongs to exactly one lane, which
// its position and the row's address alone select, and no access leaves [row, row + n).

// bytes in front of the first 16-byte boundary of p, at most n
__device__ __forceinline__ int row_head(const void* p, int n) { return min(n, (int)((16u - (uint32_t)((uintptr_t)p & 15u)) & 15u)); }

// f1(x, b): b is the byte at column x (head and tail).  f16(x, q): q holds columns x .. x+15.
template <class F1, class F16>
__device__ __forceinline__ void wave_row16(const uint8_t* __restrict__ row, int n, int lane, F1&& f1, F16&& f16) {
  const int head = row_head(row, n);
  const int nvec = (n - head) >> 4;
  if (lane < head) f1(lane, (uint32_t)row[lane]);
  const uint4* v = reinterpret_cast<const uint4*>(row + head);
  for (int i = lane; i < nvec; i += 64) {
    const uint4 q = v[i];                      // one 16-byte load, whatever f16 does with the words
    f16(head + (i << 4), q);
  }
  const int t = head + (nvec << 4) + lane;     // the tail is shorter than 16 bytes
  if (t < n) f1(t, (uint32_t)row[t]);
}

// f(word, k): the low k bytes of word are k consecutive pixels of the row; every pixel of the row is visited exactly once by the wave
template <class F> __device__ __forceinline__ void wave_row(const uint8_t* __restrict__ row, int n, int lane, F&& f) {
  wave_row16(row, n, lane, [&](int, uint32_t b) { f(b, 1); }, [&](int, const uint4& q) { f(q.x, 4); f(q.y, 4); f(q.z, 4); f(q.w, 4); });
}

// the same walk for writing: px1(x) is the byte of column x of the row at o, px16(x) the 16 bytes of columns x .. x+15.  o need not be
// the start of an image row: a caller that writes the segment [X0, X1) of a row passes o = the address of column X0 and adds X0 itself.
template <class P1, class P16>
__device__ __forceinline__ void wave_store_row(uint8_t* __restrict__ o, int n, int lane, P1&& px1, P16&& px16) {
  const int head = row_head(o, n);
  const int nvec = (n - head) >> 4;
  if (lane < head) o[lane] = (uint8_t)px1(lane);
  uint4* vec = reinterpret_cast<uint4*>(o + head);
  for (int i = lane; i < nvec; i += 64) vec[i] = px16(head + (i << 4));
  const int t = head + (nvec << 4) + lane;     // the tail is shorter than 16 bytes
  if (t < n) o[t] = (uint8_t)px1(t);
}

// px16 for a kernel whose pixels are independent of each other: 16 calls of px (which returns a value <= 255)
template <class P> __device__ __forceinline__ auto px16_of(P& px) {
  return [&px](int x) -> uint4 {
    auto px4 = [&px](int x) -> uint32_t { return px(x) | (px(x + 1) << 8) | (px(x + 2) << 16) | (px(x + 3) << 24); };
    uint4 q;
    q.x = px4(x); q.y = px4(x + 4); q.z = px4(x + 8); q.w = px4(x + 12);
    return q;
  };
}

// ---- ink -------------------------------------------------------------------------------------------------------------------------------------------

// the threshold of a launch: a fixed one is a launch argument, Otsu's was written to *hdr by otsu_kernel just before (-1: nothing is ink)
__device__ __forceinline__ int ink_thr(int fixed, const int32_t* __restrict__ hdr) { return fixed >= 0 ? fixed : hdr[0]; }

__device__ __forceinline__ bool is_ink(int v, int thr, int light) { return light ? (v > thr) : (v <= thr); }

// bit j of the result: byte j of w is ink
__device__ __forceinline__ uint32_t ink_mask4(uint32_t w, int thr, int light) {
  uint32_t m = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) m |= (uint32_t)is_ink((int)((w >> (8 * j)) & 0xffu), thr, light) << j;
  return m;
}

__device__ __forceinline__ uint32_t ink_mask16(const uint4& q, int thr, int light) {
  return ink_mask4(q.x, thr, light) | (ink_mask4(q.y, thr, light) << 4) | (ink_mask4(q.z, thr, light) << 8) | (ink_mask4(q.w, thr, light) << 12);
}

// the ink among the low n bytes of w
__device__ __forceinline__ int ink_bytes(uint32_t w, int n, int thr, int light) {
  int c = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < n) c += is_ink((int)((w >> (8 * j)) & 0xffu), thr, light);
  return c;
}

// ---- wave reductions: every lane gets the result -------------------------------------------------------------------------------------------------

template <class T> __device__ __forceinline__ T wave_sum(T v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

__device__ __forceinline__ uint64_t wave_max(uint64_t v) {
  for (int d = 32; d >= 1; d >>= 1) { const uint64_t o = __shfl_xor(v, d); v = o > v ? o : v; }
  return v;
}

// ---- host: the fields of scratch_dev ----------------------------------------------------------------------------------------------------------------

// hands out byte offsets in the order of the calls; every field starts on a multiple of 256 bytes, and so does the total
struct ScratchCursor {
  size_t o = 0;
  size_t take(size_t bytes) { const size_t at = o; o = (o + bytes + 255) & ~(size_t)255; return at; }
  size_t total() const { return o; }
};

template <class T> inline T* scratch_at(void* scratch, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(scratch) + off); }

// steps 1-2 of every stage that thresholds: with a fixed threshold nothing is enqueued and neither hist nor hdr[0] is used
void otsu_threshold(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, uint32_t* hist, int32_t* hdr);      // segment.hip
inline void page_threshold(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, int fixed, uint32_t* hist, int32_t* hdr) {
  if (fixed < 0) otsu_threshold(s, page, pitch, H, W, hist, hdr);
}

}  // namespace aocr
