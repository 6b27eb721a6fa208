// runs.h -- the run finder of the page kernels (segment.hip: bands and words; layout.hip: the pieces of an XY cut), for workgroups of
// SEG_THREADS threads: two block scans and find_runs.  Integer arithmetic only; no step depends on launch geometry or on atomics order.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace aocr {

constexpr int SEG_MAX_DIM = 16384;
constexpr int SEG_THREADS = 1024;             // find_runs: 16 elements per thread cover SEG_MAX_DIM
constexpr int SEG_WAVES = SEG_THREADS / 64;
constexpr int SEG_NONE = 1 << 30;

struct RunsShared {
  uint8_t flag[SEG_MAX_DIM];
  uint16_t s[SEG_MAX_DIM / 2], e[SEG_MAX_DIM / 2];     // runs start at least two elements apart
  int wtot[SEG_WAVES];
};

// exclusive scan of one value per thread over the workgroup (REV: from the last thread down); op commutative and associative
template <bool REV, class Op> __device__ __forceinline__ int block_scan_excl(int v, int ident, Op op, int* wtot, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int o = REV ? __shfl_down(inc, d) : __shfl_up(inc, d);
    if (REV ? (lane + d < 64) : (lane >= d)) inc = op(o, inc);
  }
  int ex = REV ? __shfl_down(inc, 1) : __shfl_up(inc, 1);
  if (lane == (REV ? 63 : 0)) ex = ident;
  __syncthreads();                                       // the previous scan's readers are done with wtot
  if (lane == (REV ? 0 : 63)) wtot[wave] = inc;
  __syncthreads();
  int acc = ident, tot = ident;
  for (int w = 0; w < SEG_WAVES; ++w) {
    const int x = wtot[w];
    tot = op(tot, x);
    if (REV ? (w > wave) : (w < wave)) acc = op(acc, x);
  }
  *total = tot;
  return op(acc, ex);
}

// sh.flag[0..n) is staged and a barrier has passed.  Set elements form runs; runs with fewer than gapmin clear elements between them are one
// interval; intervals shorter than minlen are dropped; emit(k, start, end) is called for the k-th survivor, in order.  Returns their number.
// Called by all SEG_THREADS threads.  On return (a barrier has passed) sh.s[k], sh.e[k] hold the k-th merged interval before the minlen filter, so
// with minlen <= 1 they are the survivors themselves.
template <class Emit> __device__ __forceinline__ int find_runs(RunsShared& sh, int n, int gapmin, int minlen, Emit&& emit) {
  const int tid = threadIdx.x;
  const int ch = (n + SEG_THREADS - 1) / SEG_THREADS;    // <= 16 consecutive elements per thread
  const int lo = min(n, tid * ch), hi = min(n, lo + ch);
  auto imax = [](int a, int b) { return a > b ? a : b; };
  auto imin = [](int a, int b) { return a < b ? a : b; };
  auto iadd = [](int a, int b) { return a + b; };
  int last = -1, first = SEG_NONE;
  for (int i = lo; i < hi; ++i) if (sh.flag[i]) { if (first == SEG_NONE) first = i; last = i; }
  int unused, K;
  int p = block_scan_excl<false>(last, -1, imax, sh.wtot, &unused);         // the last set element before this thread's chunk
  int q = block_scan_excl<true>(first, SEG_NONE, imin, sh.wtot, &unused);   // the first one after it
  uint32_t smask = 0, emask = 0;
  for (int i = lo; i < hi; ++i) if (sh.flag[i]) { if (p < 0 || i - p - 1 >= gapmin) smask |= 1u << (i - lo); p = i; }
  for (int i = hi - 1; i >= lo; --i) if (sh.flag[i]) { if (q == SEG_NONE || q - i - 1 >= gapmin) emask |= 1u << (i - lo); q = i; }
  int si = block_scan_excl<false>(__popc(smask), 0, iadd, sh.wtot, &K);
  int ei = block_scan_excl<false>(__popc(emask), 0, iadd, sh.wtot, &unused);
  for (; smask; smask &= smask - 1) sh.s[si++] = (uint16_t)(lo + __ffs(smask) - 1);
  for (; emask; emask &= emask - 1) sh.e[ei++] = (uint16_t)(lo + __ffs(emask));          // exclusive end
  __syncthreads();
  const int ch2 = (K + SEG_THREADS - 1) / SEG_THREADS;
  const int lo2 = min(K, tid * ch2), hi2 = min(K, lo2 + ch2);
  int keep = 0;
  for (int k = lo2; k < hi2; ++k) keep += ((int)sh.e[k] - (int)sh.s[k] >= minlen);
  int total;
  int o = block_scan_excl<false>(keep, 0, iadd, sh.wtot, &total);
  for (int k = lo2; k < hi2; ++k) if ((int)sh.e[k] - (int)sh.s[k] >= minlen) emit(o++, (int)sh.s[k], (int)sh.e[k]);
  return total;
}

}  // namespace aocr
