// data.hip -- device side of the reference's data path (src/data/data_gen.lua:68-79):
// 255 * rgb2y of a decoded image, then image.scale(img, imgW, 32) -- rows to the target width first, then columns to the
// target height, enlarging by linear interpolation with scale (src-1)/(dst-1), shrinking by averaging the covered source span
// (torch/image generic/image.c: rgb2y, scaleBilinear -> scaleLinear_rowcol; restated in oracle/data_oracle.py).
// One thread per output pixel; every float operation is an explicitly rounded (non-contracted) single-precision op in the
// order of the restatement, so the result is bit-identical to it.  HBM-bound and tiny: the images of a batch are a few MB.
#include "ops.h"
#include "resample.h"

// HIP's __fmul_rn / __fadd_rn are plain operators and hipcc contracts a*b+c into an FMA by default (-ffp-contract=fast, which
// also ignores `#pragma clang fp contract`): this file is compiled with -ffp-contract=off (Makefile: FLAGS_data) so that every
// operation below rounds exactly like the single-precision restatement.

namespace aocr {

namespace {

struct Gray {                                            // 255 * rgb2y of source pixel (row, col), interleaved uint8 HWC, C in {1, 3}
  const uint8_t* img; int w, c;
  __device__ __forceinline__ float at(int row, int col) const {
    const uint8_t* p = img + ((int64_t)row * w + col) * c;
    if (c == 1) return (float)p[0];
    const float k = 1.0f / 255.0f;
    const float r = __fmul_rn((float)p[0], k), g = __fmul_rn((float)p[1], k), b = __fmul_rn((float)p[2], k);
    const float y = __fadd_rn(__fadd_rn(__fmul_rn(0.299f, r), __fmul_rn(0.587f, g)), __fmul_rn(0.114f, b));
    return __fmul_rn(255.0f, y);
  }
};

// scale_elem, element di of scaleLinear_rowcol: resample.h (shared with slant.hip's slanted crops)

__global__ __launch_bounds__(256) void preprocess_kernel(const uint8_t* __restrict__ src, const aocr_image_desc* __restrict__ desc,
                                                         int out_h, int out_w, float* __restrict__ out) {
  const int img = blockIdx.y;
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= out_h * out_w) return;
  const int y = id / out_w, x = id - y * out_w;
  const aocr_image_desc d = desc[img];
  Gray g; g.img = src + d.offset; g.w = d.width; g.c = d.channels;
  // column pass over the row-scaled intermediate tmp[row][x] = scale_elem(gray row, width -> out_w)[x]
  auto tmp = [&](int row) { return scale_elem([&](int col) { return g.at(row, col); }, d.width, out_w, x); };
  out[((int64_t)img * out_h + y) * out_w + x] = scale_elem(tmp, d.height, out_h, y);
}

// aocr_crop_lines: preprocess_kernel's arithmetic on a rectangle of a pitched one-channel page.  The box is clamped to the page before any
// read; an empty box gives paper (255).  The number of boxes may come from the device (the counts of aocr_segment_page): no host sync.
__global__ __launch_bounds__(256) void crop_kernel(const uint8_t* __restrict__ page, int64_t pitch, int H, int W, const aocr_box* __restrict__ boxes,
                                                   const int32_t* __restrict__ count, int n_boxes, int out_h, int out_w, float* __restrict__ out) {
  const int img = blockIdx.y;
  const int id = blockIdx.x * 256 + threadIdx.x;
  const int n = count ? min(n_boxes, count[0]) : n_boxes;
  if (img >= n || id >= out_h * out_w) return;
  const int y = id / out_w, x = id - y * out_w;
  const aocr_box b = boxes[img];
  const int x0 = min(max(b.x0, 0), W), x1 = min(max(b.x1, 0), W), y0 = min(max(b.y0, 0), H), y1 = min(max(b.y1, 0), H);
  const int w = x1 - x0, h = y1 - y0;
  float v = 255.0f;
  if (w > 0 && h > 0) {
    const uint8_t* src = page + (int64_t)y0 * pitch + x0;
    auto tmp = [&](int row) { return scale_elem([&](int col) { return (float)src[(int64_t)row * pitch + col]; }, w, out_w, x); };
    v = scale_elem(tmp, h, out_h, y);
  }
  out[((int64_t)img * out_h + y) * out_w + x] = v;
}

// Training augmentation behind preprocess_kernel (include/aocr.h: aocr_augment_lines): an affine warp with bilinear taps, gain / offset,
// additive triangular noise, clamp to 0..255.  One thread per output pixel, four gathers and one store; every float operation is one
// rounded single-precision op in the order of tests/augment_ref.py.  The noise is counter-based like the dropout masks (epilogues.h).
__global__ __launch_bounds__(256) void augment_kernel(const float* __restrict__ in, const aocr_warp* __restrict__ warp, int H, int W,
                                                      unsigned long long base, float* __restrict__ out) {
  const int img = blockIdx.y;
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id >= H * W) return;
  const int y = id / W, x = id - y * W;
  const aocr_warp w = warp[img];
  const float xf = (float)x, yf = (float)y;
  float sx = __fadd_rn(__fadd_rn(__fmul_rn(w.m00, xf), __fmul_rn(w.m01, yf)), w.m02);
  float sy = __fadd_rn(__fadd_rn(__fmul_rn(w.m10, xf), __fmul_rn(w.m11, yf)), w.m12);
  sx = fminf(fmaxf(sx, -1.0f), (float)W);                  // keeps the int conversion defined; NaN -> -1 (all taps outside)
  sy = fminf(fmaxf(sy, -1.0f), (float)H);
  const float x0f = floorf(sx), y0f = floorf(sy);
  const float fx = __fsub_rn(sx, x0f), fy = __fsub_rn(sy, y0f);
  const int x0 = (int)x0f, y0 = (int)y0f;
  const float* src = in + (int64_t)img * H * W;
  auto tap = [&](int row, int col) { return (row >= 0 && row < H && col >= 0 && col < W) ? src[(int64_t)row * W + col] : w.fill; };
  const float a = tap(y0, x0), b = tap(y0, x0 + 1), c = tap(y0 + 1, x0), d = tap(y0 + 1, x0 + 1);
  const float gx = __fsub_rn(1.0f, fx), gy = __fsub_rn(1.0f, fy);
  const float top = __fadd_rn(__fmul_rn(gx, a), __fmul_rn(fx, b));
  const float bot = __fadd_rn(__fmul_rn(gx, c), __fmul_rn(fx, d));
  const float s = __fadd_rn(__fmul_rn(gy, top), __fmul_rn(fy, bot));
  float v = __fadd_rn(__fmul_rn(w.gain, s), w.offset);
  const int64_t idx = ((int64_t)img * H + y) * W + x;
  const unsigned long long r = splitmix64_(base + (unsigned long long)idx);
  const float k24 = 1.0f / 16777216.0f;
  const float u1 = __fmul_rn((float)(uint32_t)(r >> 40), k24), u2 = __fmul_rn((float)(uint32_t)((r >> 16) & 0xFFFFFFull), k24);
  v = __fadd_rn(v, __fmul_rn(w.noise, __fsub_rn(__fadd_rn(u1, u2), 1.0f)));
  out[idx] = fminf(fmaxf(v, 0.0f), 255.0f);
}

}  // namespace

void augment_lines(hipStream_t s, const float* in, const aocr_warp* warp, int n_images, int H, int W, uint64_t seed, uint64_t counter,
                   float* out) {
  if (n_images <= 0) return;
  const unsigned long long base = splitmix64_(seed ^ (counter * 0xD1342543DE82EF95ull));
  hipLaunchKernelGGL(augment_kernel, dim3(cdiv((int64_t)H * W, 256), n_images), dim3(256), 0, s, in, warp, H, W, base, out);
}

void preprocess_lines(hipStream_t s, const uint8_t* src, const aocr_image_desc* desc, int n_images, int out_h, int out_w, float* out) {
  if (n_images <= 0) return;
  hipLaunchKernelGGL(preprocess_kernel, dim3(cdiv(out_h * out_w, 256), n_images), dim3(256), 0, s, src, desc, out_h, out_w, out);
}

void crop_lines(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_box* boxes, const int32_t* count, int n_boxes,
                int out_h, int out_w, float* out) {
  if (n_boxes <= 0) return;
  hipLaunchKernelGGL(crop_kernel, dim3(cdiv(out_h * out_w, 256), n_boxes), dim3(256), 0, s, page, pitch, H, W, boxes, count, n_boxes, out_h,
                     out_w, out);
}

}  // namespace aocr
