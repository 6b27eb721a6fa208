// degrade.hip -- scan degradation of rendered or cropped line images (include/aocr.h: aocr_degrade_lines): an elastic displacement field, a
// stroke-weight blend towards the 3x3 minimum or maximum, and a separable 9-tap blur, in one launch.  A workgroup owns a TH x TW output tile and
// stages the three intermediate images in LDS with their halos (4 for each blur pass + 1 for the 3x3 window), so none of them goes through HBM.
// Every value is a function of the absolute pixel position only: the image edge is handled by clamping coordinates, never by reading a halo cell
// that lies outside the image, so a tile at the border computes what an interior tile would and the result does not depend on the tiling.
// Every float operation is one rounded single-precision op in the order of tests/degrade_ref.py (Makefile: FLAGS_degrade = -ffp-contract=off,
// see data.hip on why the flag and not a pragma).
#include "ops.h"

namespace aocr {

namespace {

constexpr int TW = 64, TH = 32;                           // output tile: TH = 32 covers the common line height in one workgroup row; TW = 64 keeps
                                                          // every LDS row access of a wave on consecutive words (no bank conflict)
constexpr int R = 4;                                      // blur radius
constexpr int MW = TW + 2 * R, MH = TH + 2 * R;           // M (after the stroke stage): what the two blur passes read
constexpr int EW = MW + 2, EH = MH + 2;                   // E (after the elastic stage): what the 3x3 window over M's cells reads
constexpr int OFF = R + 1;                                // E's origin is (tx0 - OFF, ty0 - OFF), M's and Bh's row origin is ty0 - R
constexpr int NX = (EW - 1) / 2 + 3, NY = (EH - 1) / 2 + 3;   // nodes an E region can touch at the smallest pitch (2): floor(b/p) - floor(a/p) <= (b-a)/p + 1, +1 for the far node, +1 for the count
static_assert(MH * TW <= EH * EW, "Bh reuses E's buffer");

__device__ __forceinline__ float blend(float g, float a, float p, float q) { return __fadd_rn(__fmul_rn(g, p), __fmul_rn(a, q)); }   // g = 1 - a

__global__ __launch_bounds__(256) void degrade_kernel(const float* __restrict__ in, const aocr_degrade* __restrict__ rec, int H, int W, int tiles_x,
                                                      unsigned long long base, float* __restrict__ out) {
  __shared__ float sE[EH * EW];                           // E, then (E is dead once M is complete) the horizontal blur Bh as [MH][TW]
  __shared__ float sM[MH * MW];
  __shared__ float nDx[NY * NX], nDy[NY * NX];            // displacement of the nodes this tile touches
  __shared__ float colA[EW], rowA[EH];                    // smoothstep weight of every column / row of the E region
  __shared__ int colG[EW], rowG[EH];                      // and its cell, relative to the tile's first node
  float* const sB = sE;
  const int img = blockIdx.y, tid = threadIdx.x;
  const aocr_degrade d = rec[img];
  if (d.pitch < 2) return;                                // include/aocr.h: such a record's image is left unwritten (uniform: before any barrier)
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const int tx0 = tile_x * TW, ty0 = tile_y * TH;
  const int ox = tx0 - OFF, oy = ty0 - OFF;
  // the part of the E region inside the image (inclusive), and the nodes around it
  const int ex0 = max(ox, 0), ex1 = min(ox + EW - 1, W - 1), ey0 = max(oy, 0), ey1 = min(oy + EH - 1, H - 1);
  const int gx0 = ex0 / d.pitch, gy0 = ey0 / d.pitch;
  const int ncx = min(ex1 / d.pitch + 2 - gx0, NX), ncy = min(ey1 / d.pitch + 2 - gy0, NY);
  const int GX = (W - 1) / d.pitch + 2, GY = (H - 1) / d.pitch + 2;
  const float k24 = 1.0f / 16777216.0f;

  for (int id = tid; id < ncx * ncy; id += 256) {
    const int ny = id / ncx, nx = id - ny * ncx;
    const unsigned long long node = ((unsigned long long)img * GY + (gy0 + ny)) * GX + (gx0 + nx);
    const unsigned long long r = splitmix64_(base + node);
    const float u1 = __fmul_rn((float)(uint32_t)(r >> 40), k24), u2 = __fmul_rn((float)(uint32_t)((r >> 16) & 0xFFFFFFull), k24);
    nDx[ny * NX + nx] = __fmul_rn(d.amp_x, __fsub_rn(__fadd_rn(u1, u1), 1.0f));
    nDy[ny * NX + nx] = __fmul_rn(d.amp_y, __fsub_rn(__fadd_rn(u2, u2), 1.0f));
  }
  for (int c = tid; c < EW + EH; c += 256) {              // columns first, then rows: one smoothstep per line of the region, not per pixel
    const bool col = c < EW;
    const int l = col ? c : c - EW, p = col ? ox + l : oy + l;
    if (p < 0 || p >= (col ? W : H)) continue;
    const int g = p / d.pitch;
    const float f = __fmul_rn((float)(p - g * d.pitch), d.inv_pitch);
    const float a = __fmul_rn(__fmul_rn(f, f), __fsub_rn(3.0f, __fadd_rn(f, f)));
    if (col) { colA[l] = a; colG[l] = g - gx0; } else { rowA[l] = a; rowG[l] = g - gy0; }
  }
  __syncthreads();

  // stage 1: E over the region's cells inside the image
  const float* src = in + (int64_t)img * H * W;
  auto tap = [&](int row, int col) { return (row >= 0 && row < H && col >= 0 && col < W) ? src[(int64_t)row * W + col] : d.fill; };
  for (int id = tid; id < EH * EW; id += 256) {
    const int r = id / EW, c = id - r * EW, x = ox + c, y = oy + r;
    if (x < 0 || x >= W || y < 0 || y >= H) continue;
    const float ax = colA[c], ay = rowA[r], bx = __fsub_rn(1.0f, ax), by = __fsub_rn(1.0f, ay);
    const int n = rowG[r] * NX + colG[c];
    const float ex = blend(by, ay, blend(bx, ax, nDx[n], nDx[n + 1]), blend(bx, ax, nDx[n + NX], nDx[n + NX + 1]));
    const float ey = blend(by, ay, blend(bx, ax, nDy[n], nDy[n + 1]), blend(bx, ax, nDy[n + NX], nDy[n + NX + 1]));
    float sx = __fadd_rn((float)x, ex), sy = __fadd_rn((float)y, ey);
    sx = fminf(fmaxf(sx, -1.0f), (float)W);               // as augment_kernel: keeps the int conversion defined; NaN -> -1
    sy = fminf(fmaxf(sy, -1.0f), (float)H);
    const float x0f = floorf(sx), y0f = floorf(sy);
    const float fx = __fsub_rn(sx, x0f), fy = __fsub_rn(sy, y0f);
    const int x0 = (int)x0f, y0 = (int)y0f;
    const float ta = tap(y0, x0), tb = tap(y0, x0 + 1), tc = tap(y0 + 1, x0), td = tap(y0 + 1, x0 + 1);
    const float gx = __fsub_rn(1.0f, fx), gy = __fsub_rn(1.0f, fy);
    sE[id] = blend(gy, fy, blend(gx, fx, ta, tb), blend(gx, fx, tc, td));
  }
  __syncthreads();

  // stage 2: M = E blended towards the 3x3 minimum (thick >= 0) or maximum
  const bool darken = d.thick >= 0.0f;
  const float t = darken ? d.thick : -d.thick, t1 = __fsub_rn(1.0f, t);
  for (int id = tid; id < MH * MW; id += 256) {
    const int r = id / MW, c = id - r * MW, x = tx0 - R + c, y = ty0 - R + r;
    if (x < 0 || x >= W || y < 0 || y >= H) continue;
    const int xs[3] = {max(x - 1, 0) - ox, x - ox, min(x + 1, W - 1) - ox};
    const int ys[3] = {max(y - 1, 0) - oy, y - oy, min(y + 1, H - 1) - oy};
    float lo = sE[ys[0] * EW + xs[0]], hi = lo;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float e = sE[ys[j] * EW + xs[i]];
        lo = fminf(lo, e); hi = fmaxf(hi, e);
      }
    sM[id] = blend(t1, t, sE[ys[1] * EW + xs[1]], darken ? lo : hi);
  }
  __syncthreads();                                        // M complete: E is dead, its buffer becomes Bh

  // stage 3a: Bh over the tile's columns and the rows the vertical pass reads
  for (int id = tid; id < MH * TW; id += 256) {
    const int r = id / TW, c = id - r * TW, x = tx0 + c, y = ty0 - R + r;
    if (x >= W || y < 0 || y >= H) continue;
    auto m = [&](int xx) { return sM[r * MW + xx - (tx0 - R)]; };                                 // M(xx, y)
    float acc = __fmul_rn(d.taps[0], m(x));
#pragma unroll
    for (int k = 1; k <= R; ++k) acc = __fadd_rn(acc, __fmul_rn(d.taps[k], __fadd_rn(m(max(x - k, 0)), m(min(x + k, W - 1)))));
    sB[id] = acc;
  }
  __syncthreads();

  // stage 3b: the vertical pass, clamp, store
  for (int id = tid; id < TH * TW; id += 256) {
    const int r = id / TW, c = id - r * TW, x = tx0 + c, y = ty0 + r;
    if (x >= W || y >= H) continue;
    auto b = [&](int yy) { return sB[(yy - (ty0 - R)) * TW + c]; };                               // Bh(x, yy)
    float acc = __fmul_rn(d.taps[0], b(y));
#pragma unroll
    for (int k = 1; k <= R; ++k) acc = __fadd_rn(acc, __fmul_rn(d.taps[k], __fadd_rn(b(max(y - k, 0)), b(min(y + k, H - 1)))));
    out[((int64_t)img * H + y) * W + x] = fminf(fmaxf(acc, 0.0f), 255.0f);
  }
}

}  // namespace

void degrade_lines(hipStream_t s, const float* in, const aocr_degrade* rec, int n_images, int H, int W, uint64_t seed, uint64_t counter, float* out) {
  if (n_images <= 0) return;
  const unsigned long long base = splitmix64_(seed ^ (counter * 0xD1342543DE82EF95ull) ^ AOCR_DEGRADE_STREAM);
  const int tiles_x = cdiv(W, TW), tiles_y = cdiv(H, TH);
  hipLaunchKernelGGL(degrade_kernel, dim3(tiles_x * tiles_y, n_images), dim3(256), 0, s, in, rec, H, W, tiles_x, base, out);
}

}  // namespace aocr
