// components.hip -- connected components of the ink of a page (include/aocr.h: aocr_label_components, aocr_clean_page): every ink pixel gets
// the raster index of its component's first pixel, every component an area and a tight box, and aocr_clean_page paints over the components
// that cannot be text (specks, rules).  Integer arithmetic only (the Otsu threshold, when asked for, comes from segment.hip's
// otsu_threshold); the labels are canonical (the smallest pixel index of the component), so tests/components_ref.py, a flood fill, matches
// exactly whatever the order of the atomics below.
//
// A block-based union-find in separate launches.  parent[] IS the label array: parent[p] = the raster index (y*W + x) of a pixel of p's
// component that is <= p; a root has parent[p] == p; paper is -1 and is never followed.  Invariant of every write, LDS or global: the value
// written to parent[p] is a pixel of p's component and is <= p.  So a chain of parents strictly decreases until it ends at a root, and the
// smallest pixel of a component can only ever point to itself: once every union is in, it is the root of every pixel of the component.
//   (Otsu only) otsu_threshold of segment.hip: memset, hist_kernel, otsu_kernel.
//   cc_local_kernel    one workgroup per tile of CC_TILE_H x CC_TILE_W pixels, one wave per tile row at a time (the row's ink is one
//                      ballot).  Thresholds the page bytes (the "threshold" step has no launch and no mask of its own: one byte per pixel
//                      is read here, once), starts every pixel at the first pixel of its horizontal run, unions the runs of neighbouring
//                      rows in LDS, flattens in LDS and writes the tile-local root of every pixel as its global index (tile-local and global
//                      raster orders agree inside a tile).
//   cc_merge_kernel    one thread per pixel of a tile's first row (but the page's) and of a tile's first column (but the page's): unions
//                      across the tile borders on the global array.  find reads with agent-scope relaxed atomic loads, union is an atomicMin
//                      loop towards the smaller root.  Nothing waits on anything: a stale read only costs another turn of the loop.
//   cc_flatten_kernel  one thread per pixel: the root of its chain, stored over its label; a root also clears its statistics record.
//   cc_stats_kernel    one workgroup per tile: horizontal runs (one ballot per row) go into an LDS hash table keyed by root, which adds up
//                      area, min x, max x, max y per root and tile (min y is the root's own row: the first pixel in raster order); then
//                      one set of integer global atomics per root and tile, so a page-high rule costs one per tile and not one per pixel.
//                      It also writes the number of roots of every row segment (a tile's row).
//   cc_scan_kernel     one workgroup: the exclusive prefix of the row-segment root counts in raster order, in place; writes info / counts.
//   cc_emit_kernel     (aocr_label_components with comps_dev) one wave per row segment: the k-th root in raster order writes row k.
//   cc_apply_kernel    (aocr_clean_page) one thread per pixel: copies the byte, or `fill` when the pixel's root is a speck or a rule; roots
//                      add themselves to the speck / rule counts, removed pixels to the removed ink (integer atomics, one per wave).
// No workgroup ever waits on another: no look-back, no flags, no grid barrier.  Every loop is bounded by the data (DESIGN.md section 16
// gives each termination argument).  Integer atomics only: sums, minima and maxima do not depend on their order.
#include <algorithm>
#include <cstddef>
#include "ops.h"
#include "page_common.h"
#include "runs.h"

namespace aocr {

namespace {

constexpr int CC_TILE_H = 16;                  // rows of a tile
constexpr int CC_TILE_W = 64;                  // columns of a tile: one wave reads a tile row, its ink mask is one ballot
constexpr int CC_THREADS = 256;
constexpr int CC_WAVES = CC_THREADS / 64;
constexpr int CC_HASH = 1024;                  // cc_stats_kernel: slots of the LDS table; a tile has at most CC_TILE_H * CC_TILE_W / 2 runs
constexpr int CC_BIG = 1 << 30;
static_assert(CC_TILE_W == 64, "a tile row is one wave");
static_assert(CC_HASH >= CC_TILE_H * CC_TILE_W && (CC_HASH & (CC_HASH - 1)) == 0, "the table is never more than half full");

enum { HDR_THR = 0, HDR_INK = 4, HDR_WORDS = 64 };      // words of hdr; hdr[HDR_THR] is otsu_kernel's

struct CompStat { int32_t area, min_x, max_x, max_y; };  // of a root; its min y is its own row

struct CcLayout {                              // byte offsets into scratch_dev
  size_t hist, hdr, stats, segs, labels, total;
  int ntx, nty, sw;
};

CcLayout cc_layout(int H, int W, bool with_labels) {
  CcLayout l;
  ScratchCursor c;
  l.ntx = cdiv(W, CC_TILE_W);
  l.nty = cdiv(H, CC_TILE_H);
  l.sw = (W + 1) / 2;                          // a root has paper (or the page's edge) to its left: at most one per pixel pair of a row
  l.hist = c.take(256 * sizeof(uint32_t));
  l.hdr = c.take(HDR_WORDS * sizeof(int32_t));
  l.stats = c.take((size_t)H * l.sw * sizeof(CompStat));
  l.segs = c.take((size_t)H * l.ntx * sizeof(int32_t));
  l.labels = c.take(with_labels ? (size_t)H * W * sizeof(int32_t) : 0);
  l.total = c.total();
  return l;
}

__device__ __forceinline__ uint64_t below(int lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }   // the bits under `lane`

// ---- union-find in LDS (a tile) ------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int lds_load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// parents strictly decrease: at most x steps
__device__ __forceinline__ int lds_find(int* lab, int x) {
  for (int p = lds_load(lab + x); p != x; p = lds_load(lab + x)) x = p;
  return x;
}

// max(a, b) strictly decreases from turn to turn: at most max(a, b) turns
__device__ __forceinline__ void lds_union(int* lab, int a, int b) {
  for (;;) {
    a = lds_find(lab, a);
    b = lds_find(lab, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(lab + b, a);     // old <= b.  old == b: b was a root and now hangs under a
    if (old == b) return;
    b = old;                                   // b had the parent `old` (and may have lost it to a): a and old are still to be united
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_local_kernel(const uint8_t* __restrict__ page, int64_t pitch, int H, int W, int light, int fixed,
                                                              const int32_t* __restrict__ hdr, int conn8, int32_t* __restrict__ labels,
                                                              int64_t lp) {
  __shared__ int lab[CC_TILE_H * CC_TILE_W];
  __shared__ uint64_t rowmask[CC_TILE_H];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = blockIdx.x * CC_TILE_W, y0 = blockIdx.y * CC_TILE_H;
  const int thr = ink_thr(fixed, hdr + HDR_THR);
  const int x = x0 + lane;
  for (int r = wave; r < CC_TILE_H; r += CC_WAVES) {
    const int y = y0 + r;
    bool ink = false;
    if (y < H && x < W && thr >= 0) ink = is_ink(page[(int64_t)y * pitch + x], thr, light);
    const uint64_t m = __ballot(ink);
    if (lane == 0) rowmask[r] = m;
    const uint64_t z = ~m & below(lane);                 // paper left of this pixel: the run starts after the last of it
    const int start = z ? 64 - __clzll((long long)z) : 0;
    lab[r * CC_TILE_W + lane] = ink ? r * CC_TILE_W + start : -1;
  }
  __syncthreads();
  for (int r = wave; r < CC_TILE_H; r += CC_WAVES) {
    if (r == 0) continue;
    const uint64_t m = rowmask[r], up = rowmask[r - 1];
    if (!((m >> lane) & 1)) continue;
    const int i = r * CC_TILE_W + lane;
    const bool u = (up >> lane) & 1;
    const bool ul = lane > 0 && ((up >> (lane - 1)) & 1), ur = lane < 63 && ((up >> (lane + 1)) & 1);
    if (u) {                                             // one union per overlap of two runs: at its first column
      const bool l = lane > 0 && ((m >> (lane - 1)) & 1);
      if (!(l && ul)) lds_union(lab, i, i - CC_TILE_W);
    } else if (conn8) {                                  // with the pixel above set, its neighbours are in its run
      if (ul) lds_union(lab, i, i - CC_TILE_W - 1);
      if (ur) lds_union(lab, i, i - CC_TILE_W + 1);
    }
  }
  __syncthreads();
  for (int r = wave; r < CC_TILE_H; r += CC_WAVES) {
    const int y = y0 + r;
    if (y >= H || x >= W) continue;
    int v = -1;
    if ((rowmask[r] >> lane) & 1) {
      const int root = lds_find(lab, r * CC_TILE_W + lane);
      v = (y0 + root / CC_TILE_W) * W + x0 + root % CC_TILE_W;
    }
    labels[(int64_t)y * lp + x] = v;
  }
}

// ---- union-find on the global array ----------------------------------------------------------------------------------------------------------

struct Parents {
  int32_t* p;
  int64_t lp;
  int W;
  __device__ __forceinline__ int32_t* at(int i) const { return p + (int64_t)(i / W) * lp + i % W; }
  __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(at(i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ int load(int y, int x) const { return __hip_atomic_load(p + (int64_t)y * lp + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  // every value ever stored in parent[x] is <= x, a stale one included: at most x steps
  __device__ __forceinline__ int find(int x) const {
    for (int q = load(x); q != x; q = load(x)) x = q;
    return x;
  }
  // the atomicMin returns the true parent of b, so b strictly decreases from turn to turn whatever find has seen: at most max(a, b) turns
  __device__ __forceinline__ void unite(int a, int b) const {
    for (;;) {
      a = find(a);
      b = find(b);
      if (a == b) return;
      if (a > b) { const int t = a; a = b; b = t; }
      const int old = atomicMin(at(b), a);
      if (old == b) return;
      b = old;
    }
  }
};

__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(int32_t* labels, int64_t lp, int H, int W, int conn8, int n_rows, int n_cols) {
  const Parents P{labels, lp, W};
  const int64_t t = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  const int64_t n_h = (int64_t)n_rows * W;               // the pixels of the first rows of the tiles below the top ones
  if (t < n_h) {
    const int y = ((int)(t / W) + 1) * CC_TILE_H, x = (int)(t % W);       // 1 <= y < H
    if (P.load(y, x) < 0) return;
    const int i = y * W + x;
    const bool u = P.load(y - 1, x) >= 0;
    const bool ul = x > 0 && P.load(y - 1, x - 1) >= 0, ur = x + 1 < W && P.load(y - 1, x + 1) >= 0;
    if (u) {                                             // one union per overlap of two runs, per tile: at its first column (inside a tile
      const bool l = x % CC_TILE_W != 0 && P.load(y, x - 1) >= 0;       // cc_local_kernel has joined both pixels to their left neighbours)
      if (!(l && ul)) P.unite(i, i - W);
    } else if (conn8) {
      if (ul) P.unite(i, i - W - 1);
      if (ur) P.unite(i, i - W + 1);
    }
    return;
  }
  const int64_t s = t - n_h;                             // the pixels of the first columns of the tiles right of the leftmost ones
  if (s >= (int64_t)n_cols * H) return;
  const int x = ((int)(s / H) + 1) * CC_TILE_W, y = (int)(s % H);         // 1 <= x < W
  if (P.load(y, x) < 0) return;
  const int i = y * W + x;
  const bool l = P.load(y, x - 1) >= 0;
  const bool ul = y > 0 && P.load(y - 1, x - 1) >= 0, dl = y + 1 < H && P.load(y + 1, x - 1) >= 0;
  if (l) {                                               // the same, turned: never across a tile's first row, where the pixel above is not
    const bool u = y % CC_TILE_H != 0 && P.load(y - 1, x) >= 0;         // yet joined to this one
    if (!(u && ul)) P.unite(i, i - 1);
  } else if (conn8) {
    if (ul) P.unite(i, i - W - 1);
    if (dl) P.unite(i, i + W - 1);
  }
}

// a launch of its own: every union is in.  Threads store roots over parents that other threads are still following: what those read is the
// old parent or the root, both on the chain
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(int32_t* labels, int64_t lp, int H, int W, CompStat* __restrict__ stats, int sw) {
  const int x = blockIdx.x * CC_THREADS + threadIdx.x, y = blockIdx.y;
  if (x >= W) return;
  int32_t* mine = labels + (int64_t)y * lp + x;
  const int l = *mine;
  if (l < 0) return;
  const int i = y * W + x;
  int r = l;
  for (;;) {                                             // parents strictly decrease: at most l steps
    const int q = labels[(int64_t)(r / W) * lp + r % W];
    if (q == r) break;
    r = q;
  }
  if (r != l) *mine = r;
  if (r == i) stats[(size_t)y * sw + (x >> 1)] = CompStat{0, CC_BIG, -1, -1};
}

__global__ __launch_bounds__(CC_THREADS) void cc_stats_kernel(const int32_t* __restrict__ labels, int64_t lp, int H, int W, CompStat* stats, int sw,
                                                              int32_t* __restrict__ segs, int ntx, int32_t* hdr) {
  __shared__ int key[CC_HASH], area[CC_HASH], mnx[CC_HASH], mxx[CC_HASH], mxy[CC_HASH];
  __shared__ int tile_ink;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = blockIdx.x * CC_TILE_W, y0 = blockIdx.y * CC_TILE_H;
  for (int i = threadIdx.x; i < CC_HASH; i += CC_THREADS) { key[i] = -1; area[i] = 0; mnx[i] = CC_BIG; mxx[i] = -1; mxy[i] = -1; }
  if (threadIdx.x == 0) tile_ink = 0;
  __syncthreads();
  const int x = x0 + lane;
  for (int r = wave; r < CC_TILE_H; r += CC_WAVES) {
    const int y = y0 + r;
    if (y >= H) break;                                   // the same for the whole wave
    const int l = x < W ? labels[(int64_t)y * lp + x] : -1;
    const uint64_t m = __ballot(l >= 0), roots = __ballot(l >= 0 && l == y * W + x);
    if (lane == 0) segs[(size_t)y * ntx + blockIdx.x] = __popcll(roots);
    if (l < 0 || (lane > 0 && ((m >> (lane - 1)) & 1))) continue;         // the first pixel of a run speaks for it: one root per run
    const uint64_t rest = ~(m >> lane);                  // bit j: column lane + j is paper, or beyond the wave
    const int len = __ffsll((long long)rest) - 1;        // rest != 0: the shift cleared its top `lane` bits, or lane == 0 and then m may be full
    const int n = rest ? len : 64;
    int h = (int)(((uint32_t)l * 2654435761u) >> 22) & (CC_HASH - 1);
    for (int probe = 0; probe < CC_HASH; ++probe) {      // at most CC_HASH / 2 distinct keys: an empty slot exists
      const int old = atomicCAS(&key[h], -1, l);
      if (old == -1 || old == l) break;
      h = (h + 1) & (CC_HASH - 1);
    }
    atomicAdd(&area[h], n);
    atomicMin(&mnx[h], x);
    atomicMax(&mxx[h], x + n - 1);
    atomicMax(&mxy[h], y);
  }
  __syncthreads();
  int ink = 0;
  for (int i = threadIdx.x; i < CC_HASH; i += CC_THREADS) {
    const int k = key[i];
    if (k < 0) continue;
    int32_t* s = reinterpret_cast<int32_t*>(stats + (size_t)(k / W) * sw + ((k % W) >> 1));     // cleared by cc_flatten_kernel
    atomicAdd(s + 0, area[i]);
    atomicMin(s + 1, mnx[i]);
    atomicMax(s + 2, mxx[i]);
    atomicMax(s + 3, mxy[i]);
    ink += area[i];
  }
  ink = wave_sum(ink);
  if (lane == 0 && ink) atomicAdd(&tile_ink, ink);
  __syncthreads();
  if (threadIdx.x == 0 && tile_ink) atomicAdd(&hdr[HDR_INK], tile_ink);
}

// out: info_dev of aocr_label_components (clean == 0) or counts_dev of aocr_clean_page, whose sums cc_apply_kernel then adds to
__global__ __launch_bounds__(SEG_THREADS) void cc_scan_kernel(int32_t* __restrict__ segs, int n, int fixed, const int32_t* __restrict__ hdr, int clean,
                                                              int32_t* __restrict__ out) {
  __shared__ int wtot[SEG_WAVES];
  const int ch = (n + SEG_THREADS - 1) / SEG_THREADS;
  const int lo = min(n, (int)threadIdx.x * ch), hi = min(n, lo + ch);
  int sum = 0;
  for (int i = lo; i < hi; ++i) sum += segs[i];
  int total;
  int o = block_scan_excl<false>(sum, 0, [](int a, int b) { return a + b; }, wtot, &total);
  for (int i = lo; i < hi; ++i) { const int c = segs[i]; segs[i] = o; o += c; }
  if (threadIdx.x == 0) {
    const int thr = ink_thr(fixed, hdr + HDR_THR);
    if (clean) { out[0] = total; out[1] = 0; out[2] = 0; out[3] = thr; out[4] = hdr[HDR_INK]; out[5] = 0; out[6] = 0; out[7] = 0; }
    else { out[0] = thr; out[1] = hdr[HDR_INK]; out[2] = total; out[3] = 0; }
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_emit_kernel(const int32_t* __restrict__ labels, int64_t lp, int H, int W,
                                                             const CompStat* __restrict__ stats, int sw, const int32_t* __restrict__ segs, int ntx,
                                                             int max_components, aocr_box* __restrict__ comps) {
  const int lane = threadIdx.x & 63;
  const int tx = blockIdx.x, y = blockIdx.y * CC_WAVES + (threadIdx.x >> 6);
  if (y >= H) return;
  const int x = tx * CC_TILE_W + lane;
  const int l = x < W ? labels[(int64_t)y * lp + x] : -1;
  const bool root = l >= 0 && l == y * W + x;
  const uint64_t roots = __ballot(root);
  if (!root) return;
  const int k = segs[(size_t)y * ntx + tx] + __popcll(roots & below(lane));
  if (k >= max_components) return;
  const CompStat s = stats[(size_t)y * sw + (x >> 1)];
  aocr_box b;
  b.x0 = s.min_x; b.y0 = y; b.x1 = s.max_x + 1; b.y1 = s.max_y + 1; b.line = l; b.ink = s.area;
  comps[k] = b;
}

__global__ __launch_bounds__(CC_THREADS) void cc_apply_kernel(const uint8_t* __restrict__ page, int64_t pitch, int H, int W,
                                                              const int32_t* __restrict__ labels, const CompStat* __restrict__ stats, int sw,
                                                              int min_area, int max_w, int max_h, int fill, uint8_t* __restrict__ out,
                                                              int64_t out_pitch, int32_t* counts) {
  const int lane = threadIdx.x & 63;
  const int x = blockIdx.x * CC_THREADS + threadIdx.x, y = blockIdx.y;
  int kind = 0, root = 0;                                // 1: a speck, 2: a rule
  if (x < W) {
    int v = page[(int64_t)y * pitch + x];
    const int l = labels[(int64_t)y * W + x];
    if (l >= 0) {
      const int ry = l / W;
      const CompStat s = stats[(size_t)ry * sw + ((l % W) >> 1)];
      const int w = s.max_x - s.min_x + 1, h = s.max_y - ry + 1;
      if (s.area < min_area) kind = 1;                   // specks first: a short dash is a speck, never a rule
      else if ((max_w > 0 && w > max_w) || (max_h > 0 && h > max_h)) kind = 2;
      root = l == y * W + x;
      if (kind) v = fill;
    }
    out[(int64_t)y * out_pitch + x] = (uint8_t)v;
  }
  const int specks = __popcll(__ballot(root && kind == 1)), rules = __popcll(__ballot(root && kind == 2)), gone = __popcll(__ballot(kind != 0));
  if (lane == 0) {
    if (specks) atomicAdd(&counts[1], specks);
    if (rules) atomicAdd(&counts[2], rules);
    if (gone) atomicAdd(&counts[5], gone);
  }
}

// the launches both calls share: labels of the page (lp elements a row), statistics and root offsets in scratch, info / counts header in out
void label_launches(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, int threshold, int light_text, int connectivity,
                    const CcLayout& l, void* scratch, int32_t* labels, int64_t lp, int clean, int32_t* out) {
  uint32_t* hist = scratch_at<uint32_t>(scratch, l.hist);
  int32_t* hdr = scratch_at<int32_t>(scratch, l.hdr);
  CompStat* stats = scratch_at<CompStat>(scratch, l.stats);
  int32_t* segs = scratch_at<int32_t>(scratch, l.segs);
  const int light = light_text ? 1 : 0, fixed = threshold, conn8 = connectivity == 8;
  const dim3 tiles(l.ntx, l.nty), rows(cdiv(W, CC_THREADS), H);
  (void)hipMemsetAsync(hdr, 0, HDR_WORDS * sizeof(int32_t), s);
  page_threshold(s, page, pitch, H, W, fixed, hist, hdr + HDR_THR);
  hipLaunchKernelGGL(cc_local_kernel, tiles, dim3(CC_THREADS), 0, s, page, pitch, H, W, light, fixed, hdr, conn8, labels, lp);
  const int n_rows = l.nty - 1, n_cols = l.ntx - 1;
  const int64_t border = (int64_t)n_rows * W + (int64_t)n_cols * H;
  if (border > 0)
    hipLaunchKernelGGL(cc_merge_kernel, dim3(cdiv(border, CC_THREADS)), dim3(CC_THREADS), 0, s, labels, lp, H, W, conn8, n_rows, n_cols);
  hipLaunchKernelGGL(cc_flatten_kernel, rows, dim3(CC_THREADS), 0, s, labels, lp, H, W, stats, l.sw);
  hipLaunchKernelGGL(cc_stats_kernel, tiles, dim3(CC_THREADS), 0, s, labels, lp, H, W, stats, l.sw, segs, l.ntx, hdr);
  hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(SEG_THREADS), 0, s, segs, H * l.ntx, fixed, hdr, clean, out);
}

}  // namespace

size_t components_scratch_bytes(int H, int W) { return cc_layout(H, W, false).total; }
size_t clean_scratch_bytes(int H, int W) { return cc_layout(H, W, true).total; }

static_assert(sizeof(CompStat) == 4 * sizeof(int32_t) && offsetof(CompStat, area) == 0, "ops.h describes the record to rectify.hip");
ComponentAreas component_areas(int H, int W, void* scratch) {
  const CcLayout l = cc_layout(H, W, false);
  return ComponentAreas{scratch_at<const int32_t>(scratch, l.stats), l.sw};
}

void label_components(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, int threshold, int light_text, int connectivity,
                      void* scratch, int32_t* labels, int64_t labels_pitch, int max_components, aocr_box* comps, int32_t* info) {
  const CcLayout l = cc_layout(H, W, false);
  label_launches(s, page, pitch, H, W, threshold, light_text, connectivity, l, scratch, labels, labels_pitch, 0, info);
  if (comps)
    hipLaunchKernelGGL(cc_emit_kernel, dim3(l.ntx, cdiv(H, CC_WAVES)), dim3(CC_THREADS), 0, s, labels, labels_pitch, H, W,
                       scratch_at<const CompStat>(scratch, l.stats), l.sw, scratch_at<const int32_t>(scratch, l.segs), l.ntx,
                       max_components, comps);
}

void clean_page(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_clean_params& p, void* scratch, uint8_t* out,
                int64_t out_pitch, int32_t* counts) {
  const CcLayout l = cc_layout(H, W, true);
  int32_t* labels = scratch_at<int32_t>(scratch, l.labels);
  label_launches(s, page, pitch, H, W, p.threshold, p.light_text, p.connectivity, l, scratch, labels, W, 1, counts);
  hipLaunchKernelGGL(cc_apply_kernel, dim3(cdiv(W, CC_THREADS), H), dim3(CC_THREADS), 0, s, page, pitch, H, W, labels,
                     scratch_at<const CompStat>(scratch, l.stats), l.sw, p.min_area, p.max_w, p.max_h, p.light_text ? 0 : 255, out,
                     out_pitch, counts);
}

}  // namespace aocr
