// synth.hip -- synthetic word lines (include/aocr.h: aocr_synth_lines): the ids of a lexicon row, drawn glyph by glyph from a device-resident
// atlas into one (1,H,W) fp32 line crop per image, and that word's targets / targets_eval rows.
//
// A gather-and-store kernel: one workgroup (256 threads) owns SYN_PIXELS consecutive pixels of one image.  It reads the word's row with
// 16-byte loads (the lexicon's stride rule aligns every row), looks the advances up in parallel, and ONE thread sums the pens into LDS in
// the sequential order the header states: p_0 = 0, p_{k+1} = (p_k + adv_k) + sp.  Advances and sp are >= 0 and rounded addition is monotone,
// so the pens never decrease and "the largest k with p_k <= u" is an upper-bound search (at most 8 probes of LDS) per pixel.  Then four byte
// gathers from the glyph's bitmap (the whole atlas is a few tens of KB: L1 / L2 resident), the bilinear blend of augment_kernel (data.hip)
// and one fp32 store; the threads of a wave store 256 consecutive bytes.  Every float operation is one rounded single-precision op in the
// order of tests/synth_ref.py (the file is compiled with -ffp-contract=off); nothing depends on the launch geometry, there are no atomics
// and no workgroup waits for another.
#include "ops.h"

namespace aocr {

namespace {

constexpr int SYN_THREADS = 256;            // also the largest lexicon stride: thread t owns id t of the row
constexpr int SYN_PIXELS = 1024;            // pixels of one workgroup: 4 per thread, so the pens are summed once per 1024 pixels
constexpr float SYN_MAX_COORD = 16384.0f;   // clamp of the atlas coordinates: keeps every float -> int conversion defined

__global__ __launch_bounds__(SYN_THREADS) void synth_lines_kernel(const uint8_t* __restrict__ words, int n_words, int stride,
                                                                  const uint8_t* __restrict__ pixels, const uint8_t* __restrict__ advance,
                                                                  int n_faces, int n_glyphs, int gh, int gw,
                                                                  const aocr_synth_style* __restrict__ style, int H, int W, int L,
                                                                  float* __restrict__ out, int32_t* __restrict__ targets,
                                                                  int32_t* __restrict__ targets_eval) {
  static_assert(SYN_THREADS == 256, "thread t owns id t of a row of at most 256 bytes");
  __shared__ __attribute__((aligned(16))) uint8_t ids[SYN_THREADS];
  __shared__ float adv[SYN_THREADS];
  __shared__ float pens[SYN_THREADS];
  __shared__ int n_sh;
  const int tid = threadIdx.x, img = blockIdx.y;
  const aocr_synth_style st = style[img];
  const bool have = st.word >= 0 && st.word < n_words && st.face >= 0 && st.face < n_faces;     // else: the empty word
  const float sp = fmaxf(st.spacing, 0.0f);                                                       // NaN -> 0

  if (have) {
    if (tid < (stride >> 4))
      reinterpret_cast<uint4*>(ids)[tid] = reinterpret_cast<const uint4*>(words + (int64_t)st.word * stride)[tid];
    __syncthreads();
    if (tid < stride) {
      const int g = (int)ids[tid] - 4;
      adv[tid] = (g >= 0 && g < n_glyphs) ? (float)advance[(int64_t)st.face * n_glyphs + g] : 0.0f;
    }
    __syncthreads();
  }
  if (tid == 0) {
    int n = 0;
    if (have) {
      float p = 0.0f;
      while (n < stride - 1 && ids[n] != 0) {                      // a row holds at most stride-1 ids
        pens[n] = p;
        p = __fadd_rn(__fadd_rn(p, adv[n]), sp);
        ++n;
      }
    }
    n_sh = n;
  }
  __syncthreads();
  const int n = n_sh;

  if (targets && blockIdx.x == 0) {
    for (int j = tid; j < L; j += SYN_THREADS) {
      const int64_t o = (int64_t)img * L + j;
      targets[o] = j == 0 ? 2 : (j - 1 < n ? (int32_t)ids[j - 1] : 1);
      targets_eval[o] = j < n ? (int32_t)ids[j] : (j == n ? 3 : 1);
    }
  }

  const int HW = H * W;
  const uint8_t* face_pixels = pixels + (int64_t)(have ? st.face : 0) * n_glyphs * gh * gw;
  const float dfb = __fsub_rn(st.fg, st.bg);
#pragma unroll
  for (int r = 0; r < SYN_PIXELS / SYN_THREADS; ++r) {
    const int id = blockIdx.x * SYN_PIXELS + r * SYN_THREADS + tid;
    if (id >= HW) break;
    const int y = id / W, x = id - y * W;
    float u = __fmul_rn(__fsub_rn((float)x, st.x0), st.sx);
    float v = __fmul_rn(__fsub_rn((float)y, st.y0), st.sy);
    u = fminf(fmaxf(u, -1.0f), SYN_MAX_COORD);                     // NaN -> -1: no glyph
    v = fminf(fmaxf(v, -1.0f), SYN_MAX_COORD);
    float s = 0.0f;
    if (n > 0 && u >= 0.0f) {
      int lo = 0, hi = n;                                          // pens[lo] <= u (pens[0] = 0), pens[hi] > u or hi = n
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pens[mid] <= u) lo = mid; else hi = mid;
      }
      const int g = (int)ids[lo] - 4;
      if (g >= 0 && g < n_glyphs) {
        const float lu = __fsub_rn(u, pens[lo]);
        const float xif = floorf(lu), yif = floorf(v);
        const float fx = __fsub_rn(lu, xif), fy = __fsub_rn(v, yif);
        const int xi = (int)xif, yi = (int)yif;
        const uint8_t* bmp = face_pixels + (int64_t)g * gh * gw;
        auto tap = [&](int row, int col) { return (row >= 0 && row < gh && col >= 0 && col < gw) ? (float)bmp[row * gw + col] : 0.0f; };
        const float a = tap(yi, xi), b = tap(yi, xi + 1), c = tap(yi + 1, xi), d = tap(yi + 1, xi + 1);
        const float gx = __fsub_rn(1.0f, fx), gy = __fsub_rn(1.0f, fy);
        const float top = __fadd_rn(__fmul_rn(gx, a), __fmul_rn(fx, b));
        const float bot = __fadd_rn(__fmul_rn(gx, c), __fmul_rn(fx, d));
        s = __fadd_rn(__fmul_rn(gy, top), __fmul_rn(fy, bot));
      }
    }
    const float o = __fadd_rn(st.bg, __fmul_rn(dfb, __fdiv_rn(s, 255.0f)));
    out[(int64_t)img * HW + id] = fminf(fmaxf(o, 0.0f), 255.0f);
  }
}

}  // namespace

void synth_lines(hipStream_t s, const aocr_lexicon& lex, const aocr_glyph_atlas& atlas, const aocr_synth_style* style, int n_images, int H,
                 int W, int L, float* out, int32_t* targets, int32_t* targets_eval) {
  if (n_images <= 0) return;
  hipLaunchKernelGGL(synth_lines_kernel, dim3(cdiv((int64_t)H * W, SYN_PIXELS), n_images), dim3(SYN_THREADS), 0, s, lex.words_dev, lex.n_words,
                     lex.stride, atlas.pixels_dev, atlas.advance_dev, atlas.n_faces, atlas.n_glyphs, atlas.gh, atlas.gw, style, H, W, L, out,
                     targets, targets_eval);
}

}  // namespace aocr
