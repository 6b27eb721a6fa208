// ops_gemm.hip -- instantiations + launchers of the MFMA contractions: plain GEMMs (nn.Linear forward /
// gradInput / gradWeight, LSTM.lua:79-88, model_utils.lua:57-116), implicit-GEMM convolutions
// (cudnn.SpatialConvolution, cnn.lua:17-42) and the fused recurrent-step kernels.
#include "ops.h"
#include "stepl.h"

namespace aocr {

static void split_k(int K, int chunk, int& ksplit, int& kper) {
  if (ksplit < 1) ksplit = 1;
  kper = cdiv(cdiv(K, ksplit), chunk) * chunk;
  if (kper < chunk) kper = chunk;
  ksplit = cdiv(K, kper); if (ksplit < 1) ksplit = 1;
}
// dispatch trace (AOCR_TRACE set, read per call): one stderr line per launch of the conv / GEMM / recurrent-step entry points, bf16-source and exact-fp32,
// "[aocr] <function>: <kernel>[<instantiation>] M N K", so the kernel tests can prove which branch a shape reached
static thread_local const char* t_trace_fn = nullptr;
// (the OUTERMOST scope names the line: grouped_wgrad's fp32 problems go through gemm, gemm's skinny products through launch_small_kk)
struct TraceScope {
  const char* outer;
  explicit TraceScope(const char* fn) : outer(t_trace_fn) { if (!outer) t_trace_fn = fn; }
  ~TraceScope() { t_trace_fn = outer; }
};
// (note: a word behind the line for a variant that keeps the kernel's name and instantiation -- gemm_halo4_bf16_kernel's "skip" / "pskip", gemm_f32w_kernel's effective k split)
static void trace_launch(const char* kernel, const char* inst, long long M, long long N, long long K, const char* note = nullptr) {
  if (t_trace_fn && knob::AOCR_TRACE()) fprintf(stderr, "[aocr] %s: %s[%s] %lld %lld %lld%s%s\n", t_trace_fn, kernel, inst, M, N, K, note ? " " : "", note ? note : "");
}
// the recurrent-step launchers' line: the instantiation names the template arguments that differ between their branches -- NT, the GATES kind (0 plain, 1 gate
// tiles, 2 half gate tiles), waves and, for two row tiles per workgroup, "mt2": gemm_step_kernel[2,2,w8], gemm_step_kernel[4,1,w4,mt2]
static void trace_step(int nt, int gates, int waves, int mt, long long M, long long N, long long K) {
  if (!t_trace_fn || !knob::AOCR_TRACE()) return;
  char inst[32]; snprintf(inst, sizeof inst, "%d,%d,w%d%s", nt, gates, waves, mt == 2 ? ",mt2" : "");
  trace_launch("gemm_step_kernel", inst, M, N, K);
}
// LDS-tiled bf16 kernel (any loader pair, fp32 or bf16 sources)
template <class AL, class BL, class EP>
static void launch_lds(hipStream_t s, const AL& a, const BL& b, const EP& ep, int M, int N, int K, int ksplit) {
  if (M <= 0 || N <= 0) return;
  int kper; split_k(K, 32, ksplit, kper);
  const int gx = cdiv(N, 128), gy = cdiv(M, 128);
  trace_launch("gemm_lds_bf16_kernel", "32", M, N, K);
  hipLaunchKernelGGL((gemm_lds_bf16_kernel<AL, BL, EP>), dim3(gx * gy, 1, ksplit), dim3(256), 0, s, a, b, ep, K, kper, gx, gy);
}
// 256 x 256 x 32 LDS-DMA kernel (bf16 K-contiguous operand pairs).  One workgroup per CU, so it is chosen only when the grid
// fills whole rounds of the 256 CUs well; AOCR_FORCE_DMA=1 forces it wherever its shape constraints hold (parity tests).
__device__ __attribute__((aligned(16))) unsigned char g_zero_page[64];
static const bf16_t* zero_page() {
  static const bf16_t* z = [] { void* p = nullptr; (void)hipGetSymbolAddress(&p, HIP_SYMBOL(g_zero_page)); return (const bf16_t*)p; }();
  return z;
}
static bool dma_eligible(int M, int N, int K, int C) {
  if (N % 256 || K % 32 || C % 32 || M < 256 || knob::AOCR_NO_DMA()) return false;
  if (knob::AOCR_FORCE_DMA()) return true;
  const int blocks = cdiv(M, 256) * (N / 256), rounds = cdiv(blocks, 256);
  return blocks >= 200 && blocks * 10 >= rounds * 256 * 8;          // >= 80 % of the CU-rounds it occupies
}
// narrow variant: N = 128 or 64 (two workgroups per CU)
static bool dma_narrow_eligible(int M, int N, int K, int C) {
  if ((N != 128 && N != 64) || K % 32 || C % 32 || M < 256 || knob::AOCR_NO_DMA()) return false;
  return knob::AOCR_FORCE_DMA() || cdiv(M, 256) >= 400;
}
template <class AL, class BL, class EP>
static void launch_dma_narrow(hipStream_t s, const AL& a, const BL& b, const EP& ep, int M, int N, int K) {
  const int gy = cdiv(M, 256);
  const int staged = !knob::AOCR_NO_NARROW_STAGED();       // A/B and parity: the quad epilogue
  trace_launch("gemm_dma_narrow_kernel", N % 128 == 0 ? "2" : "1", M, N, K);
  if (N % 128 == 0) { const int gx = N / 128; hipLaunchKernelGGL((gemm_dma_narrow_kernel<AL, BL, EP, 2>), dim3(gx * gy), dim3(512), 0, s, a, b, ep, K, gx, gy, zero_page(), staged); }   // (N > 128: column blocks of 128)
  else          hipLaunchKernelGGL((gemm_dma_narrow_kernel<AL, BL, EP, 1>), dim3(gy), dim3(512), 0, s, a, b, ep, K, 1, gy, zero_page(), staged);
}
// 128 x 128 tiles on the LDS-DMA ring (gemm_dma128_kernel): every bf16 K-contiguous pair the larger LDS-DMA kernels do not take (small / ragged M).
// AOCR_NO_DMA128=1: the register-staged 128 x 128 kernel (the parity reference: same k order, bit-identical)
static bool dma128_eligible(int M, int N, int K, int C) {
  return !(N % 128 || K % 32 || C % 32 || M < 1 || knob::AOCR_NO_DMA()) && !knob::AOCR_NO_DMA128();
}
template <class AL, class BL, class EP>
static void launch_dma128(hipStream_t s, const AL& a, const BL& b, const EP& ep, int M, int N, int K) {
  const int gx = N / 128, gy = cdiv(M, 128);
  // <= one workgroup per compute unit: a deep ring (7 tiles in flight) is all the latency hiding that workgroup has; otherwise two workgroups of 3 tiles in flight
  static const int cus = [] { int n = 0, dev = 0; (void)hipGetDevice(&dev); (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev); return n > 0 ? n : 256; }();
  const bool w4 = knob::AOCR_DMA128_W4();                  // A/B: the 4-wave form at every grid size
  trace_launch("gemm_dma128_kernel", gx * gy > cus ? "4,4" : w4 ? "8,4" : "8,8", M, N, K);
  if (gx * gy <= cus && !w4) hipLaunchKernelGGL((gemm_dma128_kernel<AL, BL, EP, 8, 8>), dim3(gx * gy), dim3(512), 0, s, a, b, ep, K, gx, gy, zero_page());
  else if (gx * gy <= cus) hipLaunchKernelGGL((gemm_dma128_kernel<AL, BL, EP, 8, 4>), dim3(gx * gy), dim3(256), 0, s, a, b, ep, K, gx, gy, zero_page());
  else hipLaunchKernelGGL((gemm_dma128_kernel<AL, BL, EP, 4, 4>), dim3(gx * gy), dim3(256), 0, s, a, b, ep, K, gx, gy, zero_page());
}
// 256 x 128 tiles of the narrow kernel for a WIDE product whose 256 x 256 grid would leave half the chip idle (conv7 forward: 63 x 2 tiles)
static bool dma_mid_eligible(int M, int N, int K, int C) {
  if (N % 128 || K % 32 || C % 32 || M < 256 || knob::AOCR_NO_DMA() || knob::AOCR_NO_NARROW_WIDE()) return false;      // conv forward 0.846 -> 0.825 ms per C3 step (conv7: 74.6 us on 128 x 128 tiles)
  const int blocks = cdiv(M, 256) * (N / 128);
  return blocks >= 200 && blocks <= 512;
}
// "this launch has the staged 256 x 256 tile": the bit of AOCR_HALO4_STAGED for its kind of output is on (1 fp32 tile of the data gradient, 2 of conv3 / conv5
// forward, 4 pooled tile) and the launch is not the 8-wave halo kernel's, which has no staged epilogue.  halo: the shape takes a halo-resident kernel
static bool staged256(int bit, bool halo) { return (knob::AOCR_HALO4_STAGED() & bit) != 0 && !(halo && knob::AOCR_HALO8()); }
template <class AL, class BL, class EP>
static void launch_dma(hipStream_t s, const AL& a, const BL& b, const EP& ep, int M, int N, int K, int tag = 0) {
  const int gx = N / 256, gy = cdiv(M, 256);
  const int opt = knob::AOCR_HALO4_STAGED();                 // the same switch as the halo kernel's: output tiles through LDS
  trace_launch("gemm_dma_bf16_kernel", tag ? "tag" : "", M, N, K);
  if (tag) hipLaunchKernelGGL((gemm_dma_bf16_kernel<AL, BL, EP, 0, 1>), dim3(gx * gy), dim3(512), 0, s, a, b, ep, K, gx, gy, zero_page(), opt);
  else hipLaunchKernelGGL((gemm_dma_bf16_kernel<AL, BL, EP>), dim3(gx * gy), dim3(512), 0, s, a, b, ep, K, gx, gy, zero_page(), opt);
}
// halo-resident 3 x 3 kernel (gemm_halo_bf16_kernel): the tile must be MT / W whole rows of one image
static bool halo_eligible(const LoadConvK& g, int N, int MT, int NT) {
  if (knob::AOCR_NO_HALO()) return false;                      // A/B runs, parity tests against the im2col kernels
  const int W = g.Wr;
  if (g.KW != 3 || g.W != g.Wr || g.H != g.Hr || (W != 32 && W != 64 && W != 128)) return false;
  const int R = MT / W;
  if (g.Hr % R || (g.pmode != 0 && (R & 1)) || g.C % 32 || N % NT || g.rows % MT || g.K != 9 * g.C) return false;
  return true;
}
// "this launch of the 4-wave halo kernel takes its SKIP form" (interleaved blocks per wave-row, the padding rows' dead blocks skipped): plain pixel order -- the
// pooled orders put a pool window's rows side by side, so no 32-pixel block lies in one map row (halo4_pool_skip_eligible below re-orders them) -- with blocks inside one map row (W % 32 == 0) and whole rows per
// tile (256 % W == 0; halo_eligible's widths all are).  Not with AOCR_BN_Y16's epilogue, whose fp32 column sums depend on which rows a lane holds.
// AOCR_NO_HALO4_SKIP=1: the first form everywhere (the parity reference and the A/B baseline)
template <class EP>
static bool halo4_skip_eligible(const LoadConvK& g, const EP& ep) {
  if (knob::AOCR_NO_HALO4_SKIP() || g.pmode != 0 || g.Wr % 32 || 256 % g.Wr) return false;
  if constexpr (std::is_same<EP, EpConv>::value) { if (ep.y16 && ep.bn_part) return false; }
  return true;
}
// "this (2,1)-pooled launch takes the SKIP form in its row-split order" (halo4_skip.h: a pool window's rows in acc[mi] and acc[mi + W / 64] of one lane): widths
// 64 and 128 -- at 32 the partner row belongs to the other wave-row -- and only where EVERY tile leaves through tile256_store_pooled (the kernel's own predicate,
// full tiles), the one epilogue that knows this order: an fp32 destination, a null idx or AOCR_HALO4_STAGED without bit 4 keep the first form and its quad epilogue.
// AOCR_NO_HALO4_POOL_SKIP=1: the first form for these launches only (the A/B switch); AOCR_NO_HALO4_SKIP=1 covers them too
template <class EP>
static bool halo4_pool_skip_eligible(const LoadConvK& g, const EP& ep, int opt) {
  if constexpr (std::is_same<EP, EpConv>::value) {
    if (knob::AOCR_NO_HALO4_SKIP() || knob::AOCR_NO_HALO4_POOL_SKIP() || g.pmode != 2 || !halo4_pool_width(g.Wr)) return false;
    return tile256_pooled_staged(ep, opt) && ep.rows % 256 == 0 && ep.Cout % 256 == 0;
  } else return false;
}
void kprobe_read(unsigned long long out[8]) { (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_kprobe), 64); }
template <int SGN, int MT, int NT, class EP>
static void launch_halo(hipStream_t s, const LoadConvKh& a, const LoadKh& b, const EP& ep, int M, int N, int tag = 0) {
  const int gx = N / NT, gy = M / MT;
  if constexpr (MT == 256 && NT == 256) {                 // four waves of 128 x 128 with hand-placed reads / DMA (AOCR_HALO8=1: the 8-wave kernel; bit-identical)
    if (!knob::AOCR_HALO8()) {
      const int opt = knob::AOCR_HALO4_STAGED();   // staged256's bits
      const bool pskip = SGN > 0 && halo4_pool_skip_eligible(a.g, ep, opt), skip = pskip || halo4_skip_eligible(a.g, ep);
      trace_launch("gemm_halo4_bf16_kernel", SGN > 0 ? "fwd" : "dgrad", M, N, 9LL * a.g.C, pskip ? "pskip" : skip ? "skip" : nullptr);
      if (skip && tag) hipLaunchKernelGGL((gemm_halo4_bf16_kernel<EP, SGN, 1, true>), dim3(gx * gy), dim3(256), 0, s, a, b, ep, gx, gy, zero_page(), opt);
      else if (skip) hipLaunchKernelGGL((gemm_halo4_bf16_kernel<EP, SGN, 0, true>), dim3(gx * gy), dim3(256), 0, s, a, b, ep, gx, gy, zero_page(), opt);
      else if (tag) hipLaunchKernelGGL((gemm_halo4_bf16_kernel<EP, SGN, 1>), dim3(gx * gy), dim3(256), 0, s, a, b, ep, gx, gy, zero_page(), opt);
      else hipLaunchKernelGGL((gemm_halo4_bf16_kernel<EP, SGN>), dim3(gx * gy), dim3(256), 0, s, a, b, ep, gx, gy, zero_page(), opt);
      return;
    }
  }
  trace_launch("gemm_halo_bf16_kernel", SGN > 0 ? "fwd" : "dgrad", M, N, 9LL * a.g.C);
  if (tag) hipLaunchKernelGGL((gemm_halo_bf16_kernel<EP, SGN, MT, NT, 1>), dim3(gx * gy), dim3(512), 0, s, a, b, ep, gx, gy, zero_page());
  else hipLaunchKernelGGL((gemm_halo_bf16_kernel<EP, SGN, MT, NT>), dim3(gx * gy), dim3(512), 0, s, a, b, ep, gx, gy, zero_page());
}
// (512 x 128 / 512 x 64 instantiations for the narrow layers -- conv2 forward, the data gradients of conv2 / conv3 -- were measured
// no faster than gemm_dma_narrow_kernel: 121 / 139 / 99 us against 103 / 137 / 102: with 8-16 MFMAs per wave and step those launches
// are bound by the per-step barrier + issue overhead and by their epilogues, which two workgroups per CU overlap, not by the im2col stream.)
// BK = 64 variant for bf16 K-contiguous operand pairs (conv forward / data gradient): half the barriers per FLOP
template <class AL, class BL, class EP>
[[maybe_unused]] static void launch_lds64(hipStream_t s, const AL& a, const BL& b, const EP& ep, int M, int N, int K) {
  if (M <= 0 || N <= 0) return;
  const int gx = cdiv(N, 128), gy = cdiv(M, 128);
  hipLaunchKernelGGL((gemm_lds_bf16_kernel<AL, BL, EP, 64>), dim3(gx * gy, 1, 1), dim3(256), 0, s, a, b, ep, K, cdiv(K, 64) * 64, gx, gy);
}
static bool f32t_ok(const LoadK& l) { return l.vec && l.K % 8 == 0 && (!l.p1 || l.K0 % 8 == 0); }
static bool f32t_ok(const LoadConvK& l) { return l.C % 8 == 0 && l.C >= 32 && l.K % 8 == 0 && (reinterpret_cast<uintptr_t>(l.src) & 15) == 0; }
template <class L> static bool f32t_ok(const L&) { return false; }
static bool f32w_ok(const LoadMN& l) { return l.vec && l.rows % 4 == 0; }
static bool f32w_ok(const LoadConvXcol& l) {
  const long long pixels = ((long long)l.K / ((long long)l.Ho * l.Wo) + 1) * l.H * l.W;          // K = B Ho Wo output pixels
  return l.Cin % 4 == 0 && l.N % 4 == 0 && l.Wo >= 8 && (reinterpret_cast<uintptr_t>(l.x) & 15) == 0 && pixels * l.Cin < (1ll << 31);
}
template <class L> static bool f32w_ok(const L&) { return false; }
template <class AL, class BL, class EP>
static void launch_big(hipStream_t s, bool bf16, const AL& a, const BL& b, const EP& ep, int M, int N, int K, int ksplit) {
  if (M <= 0 || N <= 0) return;
  if (bf16) { launch_lds(s, a, b, ep, M, N, K, ksplit); return; }
  // exact-fp32 mode: the LDS-tiled kernel for K-contiguous operand pairs (conv forward, conv data gradient over the re-laid taps,
  // nn.Linear forward) wherever a 128 x 128 tile is mostly full: C2 conv forward 1.86 -> 1.35 ms, data gradient 2.46 -> 1.98 ms per step.
  // The M/N-contiguous pairs (filter / weight gradients: transposing stagers, split-K) measured SLOWER on it (1.67 -> 1.85 ms) and keep
  // the fragment-from-global kernel.  AOCR_NO_LDS_F32=1 restores that kernel everywhere (bit-identical results).
  const bool no_lds32 = knob::AOCR_NO_LDS_F32();
  if constexpr (HasPtr8<AL>::v && HasPtr8<BL>::v) {
    // round 4: branch-free staging + tile shape by grid size (gemm_f32t_kernel); AOCR_NO_F32T=1 restores gemm_lds_f32_kernel (bit-identical)
    if (!no_lds32 && !knob::AOCR_NO_F32T() && M >= 96 && N >= 16 && K >= 32 && f32t_ok(a) && f32t_ok(b)) {      // (N < 64: the projector, 39 columns: rows past N stage zeros)
      int kp; split_k(K, 32, ksplit, kp);
      const int force = knob::AOCR_F32T_TILE();                        // A/B: 1 = 128 x 128, 2 = 64 x 128, 3 = 64 x 64
      auto wgs = [&](int bm, int bn) { return (long long)cdiv(M, bm) * cdiv(N, bn) * ksplit; };
      const int pick = force ? force : (N > 64 && wgs(128, 128) >= 512) ? 1 : (N > 64 && wgs(64, 128) >= 512) ? 2 : 3;
      trace_launch("gemm_f32t_kernel", pick == 1 ? "128x128" : pick == 2 ? "64x128" : "64x64", M, N, K);
      if (pick == 1) {
        const int gx = cdiv(N, 128), gy = cdiv(M, 128);
        hipLaunchKernelGGL((gemm_f32t_kernel<128, 128, AL, BL, EP>), dim3(gx * gy, 1, ksplit), dim3(256), 0, s, a, b, ep, K, kp, gx, gy);
      } else if (pick == 2) {
        const int gx = cdiv(N, 128), gy = cdiv(M, 64);
        hipLaunchKernelGGL((gemm_f32t_kernel<64, 128, AL, BL, EP>), dim3(gx * gy, 1, ksplit), dim3(256), 0, s, a, b, ep, K, kp, gx, gy);
      } else {
        const int gx = cdiv(N, 64), gy = cdiv(M, 64);
        hipLaunchKernelGGL((gemm_f32t_kernel<64, 64, AL, BL, EP>), dim3(gx * gy, 1, ksplit), dim3(256), 0, s, a, b, ep, K, kp, gx, gy);
      }
      return;
    }
  }
  if (KContig<AL>::v && KContig<BL>::v && !no_lds32 && M >= 96 && N >= 64 && K >= 32) {
    int kp; split_k(K, 32, ksplit, kp);
    const int gx = cdiv(N, 128), gy = cdiv(M, 128);
    trace_launch("gemm_lds_f32_kernel", "", M, N, K);
    hipLaunchKernelGGL((gemm_lds_f32_kernel<AL, BL, EP>), dim3(gx * gy, 1, ksplit), dim3(256), 0, s, a, b, ep, K, kp, gx, gy);
    return;
  }
  if constexpr (HasStagerW<AL>::v && HasStagerW<BL>::v) {
    // round 4: M/N-contiguous pairs (filter gradients, recurrent weight gradients) through a [k][m] LDS image (gemm_f32w_kernel);
    // AOCR_NO_F32W=1 restores the fragment-from-global kernel
    if (!knob::AOCR_NO_F32W() && M >= 64 && N >= 64 && K >= 64 && f32w_ok(a) && f32w_ok(b)) {
      // at least AOCR_F32W_MINK (default 192) of K per k range: the callers' split (pick_ksplit: 768 workgroups) gave the recurrent weight gradients at batch 64
      // (K = L B = 1536) 12-24 ranges of 64-128 rows -- 2-4 tiles of MFMA work under a 128 x 128 tile of memory-side atomics each (88 us, MFMA-busy 0.17).
      // Measured at C2 (ms per step, same box): 32 (the callers' split) 7.70, 128 7.62, 160 7.56, 192 7.51-7.57, 256 7.59, 384 7.66, 768 8.08.
      ksplit = std::min(ksplit, std::max(1, K / knob::AOCR_F32W_MINK()));
      int kp; split_k(K, 32, ksplit, kp);
      const int gx = cdiv(N, 128), gy = cdiv(M, 128);
      { char note[16]; snprintf(note, sizeof note, "%d", ksplit); trace_launch("gemm_f32w_kernel", "", M, N, K, note); }
      hipLaunchKernelGGL((gemm_f32w_kernel<AL, BL, EP>), dim3(gx * gy, 1, ksplit), dim3(256), 0, s, a, b, ep, K, kp, gx, gy);
      return;
    }
  }
  int kper; split_k(K, 8, ksplit, kper);
  trace_launch("gemm_big_kernel", "f32", M, N, K);
  hipLaunchKernelGGL((gemm_big_kernel<false, 2, 2, AL, BL, EP>), dim3(cdiv(N, 128), cdiv(M, 128), ksplit), dim3(256), 0, s, a, b, ep, K, kper);
}

void launch_big_kk(hipStream_t s, bool bf16, const LoadK& a, const LoadK& b, const EpStore& ep, int M, int N, int K, int ksplit) {
  const TraceScope ts("launch_big_kk");
  launch_big(s, bf16, a, b, ep, M, N, K, ksplit);
}
void launch_big_kmn(hipStream_t s, bool bf16, const LoadK& a, const LoadMN& b, const EpStore& ep, int M, int N, int K, int ksplit) {
  launch_big(s, bf16, a, b, ep, M, N, K, ksplit);
}
void launch_big_mnmn(hipStream_t s, bool bf16, const LoadMN& a, const LoadMN& b, const EpStore& ep, int M, int N, int K, int ksplit) {
  launch_big(s, bf16, a, b, ep, M, N, K, ksplit);
}
void launch_conv_fwd(hipStream_t s, bool bf16, const LoadConvK& a, const LoadK& b, const EpConv& ep, int M, int N, int K) {
  launch_big(s, bf16, a, b, ep, M, N, K, 1);
}
void launch_conv_dgrad(hipStream_t s, bool bf16, const LoadConvK& a, const LoadConvWT& b, const EpStore& ep, int M, int N, int K) {
  launch_big(s, bf16, a, b, ep, M, N, K, 1);
}
void launch_conv_wgrad(hipStream_t s, bool bf16, const LoadMN& a, const LoadConvXcol& b, const EpStore& ep, int M, int N, int K, int ksplit) {
  launch_big(s, bf16, a, b, ep, M, N, K, ksplit);
}

static bool quarter_gate_tiles(int H, int M, int nz) { return !knob::AOCR_NO_QUARTER_TILES() && H % 8 == 0 && (H / 32) * cdiv(M, 32) * nz < 128; }
template <int NT, bool GATES, class ARGS>
static void launch_small(hipStream_t s, bool bf16, int nz, const ARGS* z, int M, int ncols, int gate_stride) {
  if (M <= 0 || ncols <= 0) return;
  const TraceScope ts("launch_small");
  dim3 grid(GATES ? cdiv(ncols, 32) : cdiv(ncols, 32 * NT), cdiv(M, 32), nz);
  SmallArgs2<decltype(z[0].a), decltype(z[0].b), decltype(z[0].ep)> zz; zz.z[0] = z[0]; zz.z[1] = z[nz > 1 ? 1 : 0]; zz.z[2] = z[nz > 2 ? 2 : 0];
  if (bf16) {
    hipLaunchKernelGGL((gemm_small_kernel<true, NT, GATES, decltype(z[0].a), decltype(z[0].b), decltype(z[0].ep)>), grid, dim3(256), 0, s, zz,
                       gate_stride);
    return;
  }
  if constexpr (std::is_same<typename std::decay<decltype(z[0].a)>::type, LoadK>::value && std::is_same<typename std::decay<decltype(z[0].b)>::type, LoadK>::value &&
                ((GATES && NT == 4) || (!GATES && NT == 1))) {
    // round 4: wave-private LDS staging with whole-line loads for the exact-fp32 steps too (gemm_step_f32_kernel); AOCR_NO_STEP_F32=1: the
    // fragment-from-global kernels below
    bool ok = !knob::AOCR_NO_STEP_F32() && (GATES ? ncols % 8 == 0 : ncols % 32 == 0);
    for (int i = 0; i < nz && ok; ++i)
      ok = z[i].K > 0 && z[i].K % 32 == 0 && z[i].a.vec && z[i].b.vec && z[i].a.K == z[i].K && z[i].b.K == z[i].K &&
           (z[i].a.p1 ? z[i].a.K0 % 32 == 0 : z[i].a.K0 >= z[i].K) && (z[i].b.p1 ? z[i].b.K0 % 32 == 0 : z[i].b.K0 >= z[i].K);
    if (ok) {
      typedef typename std::decay<decltype(z[0].ep)>::type EPT;
      // AOCR_STEP_F32_W16=1: 16 waves (147 KB of LDS, one workgroup per CU) where K is deep and the launch covers less than half the chip (K = 4 Hd = 2048
      // of the decoder's d h products at batch 64: 32-96 workgroups x 8 chunks per wave).  Measured SLOWER (those launches 15.5-16.6 -> 17.5-18.2 us,
      // C2 7.67 -> 7.81 ms per step: the 1024-thread workgroup's launch and 16-way reduction cost more than the shorter K loop saves): opt-in.
      const int wgs = (GATES ? ncols / 8 : ncols / 32) * cdiv(M, 32) * nz;
      const bool deep = knob::AOCR_STEP_F32_W16() && z[0].K >= 2048 && wgs <= 128;
      trace_launch("gemm_step_f32_kernel", GATES ? "gates" : deep ? "plain,w16" : "plain,w8", M, ncols, z[0].K);
      if constexpr (GATES) hipLaunchKernelGGL((gemm_step_f32_kernel<true, EPT>), dim3(ncols / 8, cdiv(M, 32), nz), dim3(512), 0, s, zz, gate_stride);
      else if (deep) hipLaunchKernelGGL((gemm_step_f32_kernel<false, EPT, 16>), dim3(ncols / 32, cdiv(M, 32), nz), dim3(1024), 0, s, zz, gate_stride);
      else hipLaunchKernelGGL((gemm_step_f32_kernel<false, EPT>), dim3(ncols / 32, cdiv(M, 32), nz), dim3(512), 0, s, zz, gate_stride);
      return;
    }
  }
  if constexpr (GATES && NT == 4) {
    if (quarter_gate_tiles(ncols, M, nz)) {
      // small batch: 8 hidden units x 4 gates per workgroup (the A and B tiles are loaded straight from global memory here, so
      // the narrower tile costs nothing but a shuffle in the epilogue)
      trace_launch("gemm_small_kernel", "f32,quarter", M, ncols, z[0].K);
      hipLaunchKernelGGL((gemm_small_kernel<false, 1, true, decltype(z[0].a), decltype(z[0].b), decltype(z[0].ep), 8, true>),
                         dim3(ncols / 8, cdiv(M, 32), nz), dim3(512), 0, s, zz, gate_stride);
      return;
    }
  }
  // the fragment-from-global kernel's line: gemm_small_kernel[f32,<NT>,gates|plain,w8|w4]
  { char inst[32]; snprintf(inst, sizeof inst, "f32,%d,%s,%s", NT, GATES ? "gates" : "plain", knob::AOCR_STEP_WAVES4() ? "w4" : "w8");
    trace_launch("gemm_small_kernel", inst, M, ncols, z[0].K); }
  if (!knob::AOCR_STEP_WAVES4())
    hipLaunchKernelGGL((gemm_small_kernel<false, NT, GATES, decltype(z[0].a), decltype(z[0].b), decltype(z[0].ep), 8>), grid, dim3(512), 0, s,
                       zz, gate_stride);
  else
    hipLaunchKernelGGL((gemm_small_kernel<false, NT, GATES, decltype(z[0].a), decltype(z[0].b), decltype(z[0].ep)>), grid, dim3(256), 0, s,
                       zz, gate_stride);
}
void launch_small_gates_fwd(hipStream_t s, bool bf16, int nz, const GatesFwdArgs* z, int M, int H) {
  launch_small<4, true>(s, bf16, nz, z, M, H, H);
}
void launch_small_kk(hipStream_t s, bool bf16, int nz, const SmallKKArgs* z, int M, int N) {
  launch_small<1, false>(s, bf16, nz, z, M, N, 0);
}
void launch_small_kmn(hipStream_t s, bool bf16, int nz, const SmallKMNArgs* z, int M, int N) {
  launch_small<1, false>(s, bf16, nz, z, M, N, 0);
}
void launch_small_gates_bwd_kk(hipStream_t s, int nz, const GatesBwdKKArgs* z, int M, int H) { launch_small<1, false>(s, false, nz, z, M, H, 0); }
void launch_small_gates_bwd(hipStream_t s, bool bf16, int nz, const GatesBwdArgs* z, int M, int H) {
  launch_small<1, false>(s, bf16, nz, z, M, H, 0);
}

// half gate tiles (16 hidden units x 4 gates per workgroup) when the 32-unit grid would leave CUs idle; AOCR_NO_HALF_TILES=1 disables
static bool half_gate_tiles(int H, int M, int nz) {
  return !knob::AOCR_NO_HALF_TILES() && H % 16 == 0 && (H / 32) * cdiv(M, 32) * nz < knob::AOCR_HALF_TILES_MAXGRID();
}
// half gate tiles of the staged step kernel (callers: GATES && NT == 4, half_gate_tiles() holds)
template <class AL, class BL, class EP>
static void launch_step_half_gates(hipStream_t s, const SmallArgs2<AL, BL, EP>& zz, bool w8, int nz, int M, int ncols, int K, int gate_stride) {
  trace_step(2, 2, w8 ? 8 : 4, 1, M, ncols, K);
  if (w8)
    hipLaunchKernelGGL((gemm_step_kernel<2, 2, AL, EP, 8>), dim3(ncols / 16, cdiv(M, 32), nz), dim3(512), 0, s, zz, gate_stride);
  else
    hipLaunchKernelGGL((gemm_step_kernel<2, 2, AL, EP>), dim3(ncols / 16, cdiv(M, 32), nz), dim3(256), 0, s, zz, gate_stride);
}
// one 32-row tile per workgroup of the staged step kernel on the widest wave count allowed: 16 (NT = 1, K >= 1024), 8 (NT <= 2), else 4
template <int NT, bool GATES, class AL, class BL, class EP>
static void launch_step_by_waves(hipStream_t s, const SmallArgs2<AL, BL, EP>& zz, bool w8, bool w16, dim3 grid, int M, int ncols, int K, int gate_stride) {
  if constexpr (NT == 1) {
    if (w16 && K >= 1024) {                      // 147 KB of LDS; 64 k per wave at K = 1024
      trace_step(NT, GATES ? 1 : 0, 16, 1, M, ncols, K);
      hipLaunchKernelGGL((gemm_step_kernel<NT, GATES ? 1 : 0, AL, EP, 16>), grid, dim3(1024), 0, s, zz, gate_stride);
      return;
    }
  }
  if constexpr (NT <= 2) {
    if (w8) {
      trace_step(NT, GATES ? 1 : 0, 8, 1, M, ncols, K);
      hipLaunchKernelGGL((gemm_step_kernel<NT, GATES ? 1 : 0, AL, EP, 8>), grid, dim3(512), 0, s, zz, gate_stride);
      return;
    }
  }
  trace_step(NT, GATES ? 1 : 0, 4, 1, M, ncols, K);
  hipLaunchKernelGGL((gemm_step_kernel<NT, GATES ? 1 : 0, AL, EP>), grid, dim3(256), 0, s, zz, gate_stride);
}
template <int NT, bool GATES, class ARGS>
static void launch_small_bf16(hipStream_t s, int nz, const ARGS* z, int M, int ncols, int gate_stride) {
  if (M <= 0 || ncols <= 0) return;
  const TraceScope ts("launch_small_bf16");
  const bool w8 = !knob::AOCR_STEP_WAVES4(), w16 = w8 && knob::AOCR_STEP_WAVES16();
  dim3 grid(GATES ? cdiv(ncols, 32) : cdiv(ncols, 32 * NT), cdiv(M, 32), nz);
  SmallArgs2<decltype(z[0].a), decltype(z[0].b), decltype(z[0].ep)> zz; zz.z[0] = z[0]; zz.z[1] = z[nz > 1 ? 1 : 0]; zz.z[2] = z[nz > 2 ? 2 : 0];
  bool staged = ncols % 32 == 0;                              // wave-private-LDS kernel: full-line loads, needs 64-aligned K
  for (int i = 0; i < nz; ++i)
    staged = staged && z[i].K > 0 && z[i].K % 64 == 0 && z[i].a.K0 % 64 == 0 && z[i].a.vec && z[i].b.ld0 % 8 == 0 &&
             (!z[i].b.p1 || z[i].b.ld1 % 8 == 0);
  if (staged) {
    if constexpr (GATES && NT == 4) {
      if (half_gate_tiles(ncols, M, nz)) { launch_step_half_gates(s, zz, w8, nz, M, ncols, z[0].K, gate_stride); return; }
    }
    launch_step_by_waves<NT, GATES>(s, zz, w8, w16, grid, M, ncols, z[0].K, gate_stride);
    return;
  }
  trace_launch("gemm_small_kernel", NT == 4 ? (GATES ? "bf16,4,gates" : "bf16,4,plain") : (GATES ? "bf16,1,gates" : "bf16,1,plain"), M, ncols, z[0].K);
  hipLaunchKernelGGL((gemm_small_kernel<true, NT, GATES, decltype(z[0].a), decltype(z[0].b), decltype(z[0].ep)>), grid, dim3(256), 0, s,
                     zz, gate_stride);
}
// Large-batch form of the step products (stepl.h).  Shape conditions here; WHEN it is taken is decided per kind of launch from tools/ubench/step400.hip (M = 32 .. 1280,
// Hd = 512 / 1024, the library's own kernels side by side):
//   gate products: whenever the half-gate-tile grid of gemm_step_kernel<2, 2, ..., 8 waves> would be more than ONE round of the chip -- in one round that kernel wins
//     (Hd = 1024: 11.2 against 15.4 us at 128 rows), beyond it stepl.h does (192 rows: 19.2 / 15.9, 400 rows: 31.0 / 18.8; Hd = 512 at 400 rows: 13.9 / 11.6);
//   three plain products per launch: from 160 workgroups of 64 x 128 (400 rows x N = 1024: 38.8 / 30.8 us; at 256 rows the small tiles win);
//   one plain product: only at K >= 4096 and >= 160 workgroups (1280 rows: 37.3 / 28.4 us) -- below that its 416+ small workgroups beat every tile shape here.
// AOCR_NO_STEPL=1: off (A/B runs, parity tests); AOCR_STEPL_MIN_WGS=n: taken from n of its own workgroups, whatever the kind (tests force it at small batch).
template <class ARGS>
static bool stepl_eligible(const ARGS* z, int nz, int M) {
  if (knob::AOCR_NO_STEPL()) return false;
  for (int i = 0; i < nz; ++i) {
    const auto& a = z[i].a; const auto& b = z[i].b;
    if (z[i].K <= 0 || z[i].K % 128 || a.K0 % 64 || b.K0 != a.K0 || (a.p1 != nullptr) != (b.p1 != nullptr)) return false;
    if ((int64_t)M * std::max(a.ld0, a.ld1) >= (1ll << 31) || (int64_t)b.rows * std::max(b.ld0, b.ld1) >= (1ll << 31)) return false;      // 32-bit element offsets
    if (a.ld0 % 8 || (a.p1 && a.ld1 % 8) || b.ld0 % 8 || (b.p1 && b.ld1 % 8)) return false;                                              // 16-byte pieces
  }
  return true;
}
// both operands from bf16 shadows: only the staged kernel exists (callers check step_ok_hh first)
template <int NT, bool GATES, class ARGS>
static void launch_small_bf16_hh(hipStream_t s, int nz, const ARGS* z, int M, int ncols, int gate_stride) {
  if (M <= 0 || ncols <= 0) return;
  const TraceScope ts("launch_small_bf16_hh");
  const bool w8 = !knob::AOCR_STEP_WAVES4(), w16 = w8 && knob::AOCR_STEP_WAVES16();
  dim3 grid(GATES ? cdiv(ncols, 32) : cdiv(ncols, 32 * NT), cdiv(M, 32), nz);
  SmallArgs2<decltype(z[0].a), decltype(z[0].b), decltype(z[0].ep)> zz; zz.z[0] = z[0]; zz.z[1] = z[nz > 1 ? 1 : 0]; zz.z[2] = z[nz > 2 ? 2 : 0];
  if constexpr (GATES && NT == 4) {
    // large batch (round 6; the reference-default decoder: 400 rows x Hd = 1024): 64 x 128 gate tiles on the LDS-DMA ring, eight waves, four-unit epilogue (stepl.h)
    const int min_wgs = knob::AOCR_STEPL_MIN_WGS();
    if (stepl_eligible(z, nz, M) && (min_wgs >= 0 ? (ncols / 32) * cdiv(M, 64) * nz >= min_wgs : (ncols / 16) * cdiv(M, 32) * nz > 256)) {
      const int gx = ncols / 32, gy = cdiv(M, 64);
      trace_launch("gemm_stepl_kernel", "gates", M, ncols, z[0].K);
      hipLaunchKernelGGL((gemm_stepl_kernel<2, 4, 1, decltype(z[0].ep), 6, 2, 8, true>), dim3(gx * gy * nz), dim3(512), 0, s, zz, gate_stride, gx, gy);
      return;
    }
    if (half_gate_tiles(ncols, M, nz)) { launch_step_half_gates(s, zz, w8, nz, M, ncols, z[0].K, gate_stride); return; }
    // two row tiles per workgroup where the single-tile grid is more than a round of the chip anyway (reference default He = 512: M = 400, 32 x 13 workgroups):
    // the weight tile is streamed by half as many row blocks and every weight fragment feeds two MFMAs.  AOCR_NO_STEP_MT2=1: off
    if (!knob::AOCR_NO_STEP_MT2() && cdiv(ncols, 32) * cdiv(M, 64) * nz >= 200) {
      trace_step(NT, 1, 4, 2, M, ncols, z[0].K);
      hipLaunchKernelGGL((gemm_step_kernel<NT, 1, decltype(z[0].a), decltype(z[0].ep), 4, 2>), dim3(cdiv(ncols, 32), cdiv(M, 64), nz), dim3(256), 0, s, zz, gate_stride);
      return;
    }
  }
  if constexpr (!GATES && NT == 1) {
    // plain products at large batch (the backward step's d z W_h2h / input-feed group of three; single deep products from ~1280 rows): stepl.h, see stepl_eligible
    const int lw = ncols % 128 == 0 ? (ncols / 128) * cdiv(M, 64) * nz : 0;          // its workgroups
    const int min_wgs = knob::AOCR_STEPL_MIN_WGS();
    if (lw > 0 && stepl_eligible(z, nz, M) && (min_wgs >= 0 ? lw >= min_wgs : lw >= 160 && (nz == 3 || (nz == 1 && z[0].K >= 4096)))) {
      const int gx = ncols / 128, gy = cdiv(M, 64);
      trace_launch("gemm_stepl_kernel", "plain", M, ncols, z[0].K);
      hipLaunchKernelGGL((gemm_stepl_kernel<2, 4, 0, decltype(z[0].ep), 6, 2, 8, true>), dim3(gx * gy * nz), dim3(512), 0, s, zz, gate_stride, gx, gy);
      return;
    }
  }
  if constexpr (!GATES && NT == 1) {
    // ONE deep plain product at large batch (K >= 2048 at >= 320 rows: the backward step's d z_2 W_i2h in front of the lower cell, the out product): two row tiles per workgroup, 64 x 32
    // tiles on 224 workgroups of 8 waves -- 16.6 -> 14.8 us (tools/ubench/step400.hip; at K = 1024 and for three products per launch the 32 x 32 tiles win).  Same K
    // split and summation order as the one-tile form: bit-identical.  AOCR_NO_STEP_MT2=1: off
    // AOCR_STEP_MT2_MINK: the K from which the two-tile form is taken (A/B on the reference-default step: decoder 3.31 ms at 4096, 3.26 at 2048, 3.31 at 1024)
    if (!knob::AOCR_NO_STEP_MT2() && nz == 1 && z[0].K >= knob::AOCR_STEP_MT2_MINK() && M >= 320 && cdiv(ncols, 32) * cdiv(M, 64) >= 200 && w8) {
      trace_step(1, 0, 8, 2, M, ncols, z[0].K);
      hipLaunchKernelGGL((gemm_step_kernel<1, 0, decltype(z[0].a), decltype(z[0].ep), 8, 2>), dim3(cdiv(ncols, 32), cdiv(M, 64), nz), dim3(512), 0, s, zz, gate_stride);
      return;
    }
  }
  // (measured and dropped: 64 x 64 tiles -- NT = 2, MT = 2, eight waves -- for the plain step products of the backward pass at M = 400: 336 workgroups instead of
  //  1248, 350 MB instead of 640 MB per launch, decoder backward 2.27 -> 2.34 ms: there the many small workgroups are what hides the latency)
  launch_step_by_waves<NT, GATES>(s, zz, w8, w16, grid, M, ncols, z[0].K, gate_stride);
}
// ---- recurrent-step products at LARGE batch (round 5; the reference's default shape: 400 rows, Hd = 1024).  The step kernels above are built for latency at 32-256
// rows: 32-row tiles, every workgroup streams its own weight slice -- at 400 rows a gate launch re-reads its 16 MB of weights 13 times (41.5 us for 6.7 GFLOP =
// 0.06 of the MFMA peak, 18 % of that workload's step).  Here: 128 x 128 tiles on the LDS-DMA ring over the concatenated K range [x0 | x1] x [W0 | W1], fp32 tile
// out; the LSTM cell then runs as its own elementwise pass (gates_elem_fwd_kernel) on the SAME epilogue object (EpGatesFwd::elem), so every option of the
// fused epilogue (token table, dropout, shadows, saved gates) is the one code path.
static LoadKhCat cat_of(const LoadKh2& a) {
  LoadKhCat c; c.p0 = a.p0; c.ld0 = a.ld0; c.rows = a.rows; c.K = a.K;
  if (a.p1) { c.p1 = a.p1; c.ld1 = a.ld1; c.K0 = a.K0; } else { c.p1 = a.p0; c.ld1 = a.ld0; c.K0 = a.K; }
  return c;
}
bool big_step_eligible(int M, int N, int K) {
  // AOCR_BIG_STEP_MIN_ROWS (320): C3 / C4 launch-chain fallbacks (<= 256 rows) stay on the step kernels
  // MEASURED SLOWER, so opt-in (AOCR_BIG_STEP=1; tests/test_configs_gpu.py keeps its oracle test): at 400 rows x Hd = 1024 the 128 x 128 grid is 128 workgroups of 64 K steps, and
  // a workgroup's L2 -> LDS stream sustains ~32 GB/s (1 MB of operands in 32 us): gate product 32 us + 7 us for the cell pass against 41.5 us fused in the step kernel, the
  // N = 1024 products 19-25 us against 17 -- decoder 5.06 -> 5.82 ms per step of the reference-default workload.  Both forms are bound by what one compute unit pulls from L2.
  return knob::AOCR_BIG_STEP() && M >= knob::AOCR_BIG_STEP_MIN_ROWS() && N >= 1024 && dma128_eligible(M, N, K, 32);
}
static bool big_step_store_(hipStream_t s, const LoadKh2& a, const LoadKh2& b, const EpStore& ep, int M, int N) {       // (the caller holds the TraceScope)
  if (!big_step_eligible(M, N, a.K) || (a.p1 && a.K0 % 32) || (b.p1 && b.K0 % 32) || (a.p1 != nullptr) != (b.p1 != nullptr) || (a.p1 && a.K0 != b.K0)) return false;
  launch_dma128(s, cat_of(a), cat_of(b), ep, M, N, a.K);
  return true;
}
bool big_step_store(hipStream_t s, const LoadKh2& a, const LoadKh2& b, const EpStore& ep, int M, int N) {
  const TraceScope ts("big_step_store");
  return big_step_store_(s, a, b, ep, M, N);
}
__global__ __launch_bounds__(256) void gates_elem_fwd_kernel(const float* __restrict__ z, int64_t ldz, EpGatesFwd ep) {
  const int j = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
  if (j >= ep.H) return;
  EpGatesFwd::Pre pre = ep.prefetch(row, j);
  ep.prefetch_zx(pre, row, j);
  float v[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) v[g] = z[(int64_t)row * ldz + (int64_t)g * ep.H + j];
  ep.elem<4>(row, j, 0, v, pre);
}
// LSTM cell backward with NO product in front of it (d h comes entirely from the epilogue's own terms): one element per thread, operands by the loads-only prefetch
__global__ __launch_bounds__(256) void gates_elem_bwd_kernel(EpGatesBwd ep) {
  const int j = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
  if (j >= ep.H) return;
  const EpGatesBwd::Pre pre = ep.prefetch(row, j);
  const float v[1] = {0.f};
  ep.elem<1>(row, j, 0, v, pre);
}
void gates_elem_bwd(hipStream_t s, const EpGatesBwd& ep, int M, int H) {
  if (M <= 0 || H <= 0) return;
  const TraceScope ts("gates_elem_bwd");
  trace_launch("gates_elem_bwd_kernel", "", M, H, 0);
  hipLaunchKernelGGL(gates_elem_bwd_kernel, dim3(cdiv(H, 256), M), dim3(256), 0, s, ep);
}
bool big_step_gates_fwd(hipStream_t s, const LoadKh2& a, const LoadKh2& b, const EpGatesFwd& ep, int M, int H, float* zbuf, size_t zbuf_floats) {
  const TraceScope ts("big_step_gates_fwd");
  if (!zbuf || zbuf_floats < (size_t)M * 4 * H || !big_step_store_(s, a, b, make_store(zbuf, 4 * H, M, 4 * H, nullptr, nullptr, 0), M, 4 * H)) return false;
  trace_launch("gates_elem_fwd_kernel", "", M, H, 0);
  hipLaunchKernelGGL(gates_elem_fwd_kernel, dim3(cdiv(H, 256), M), dim3(256), 0, s, zbuf, (int64_t)4 * H, ep);
  return true;
}
void launch_small_gates_fwd_hh(hipStream_t s, int nz, const GatesFwdArgsHH* z, int M, int H) { launch_small_bf16_hh<4, true>(s, nz, z, M, H, H); }
void launch_small_hh(hipStream_t s, int nz, const SmallArgsHH* z, int M, int N) { launch_small_bf16_hh<1, false>(s, nz, z, M, N, 0); }
void launch_small_gates_bwd_hh(hipStream_t s, int nz, const GatesBwdArgsHH* z, int M, int H) { launch_small_bf16_hh<1, false>(s, nz, z, M, H, 0); }
void launch_small_gates_fwd_h(hipStream_t s, int nz, const GatesFwdArgsH* z, int M, int H) { launch_small_bf16<4, true>(s, nz, z, M, H, H); }
void launch_small_h(hipStream_t s, int nz, const SmallArgsH* z, int M, int N) { launch_small_bf16<1, false>(s, nz, z, M, N, 0); }
void launch_small_gates_bwd_h(hipStream_t s, int nz, const GatesBwdArgsH* z, int M, int H) { launch_small_bf16<1, false>(s, nz, z, M, H, 0); }

// number of K slices for an atomically accumulated contraction: fill ONE round of resident workgroups (256 CUs x 3 per CU)
// without spilling into a mostly empty second round
static int pick_ksplit(int M, int N, int K, bool bf16, int slots = 768) {
  int64_t tiles = (int64_t)cdiv(M, 128) * cdiv(N, 128);
  int chunk = bf16 ? 32 : 8;
  int ks = (int)(slots / tiles);
  int maxks = K / (chunk * 8); if (maxks < 1) maxks = 1;
  if (ks > maxks) ks = maxks;
  if (ks < 1) ks = 1;
  return ks;
}

int gemm(hipStream_t s, bool bf16, const float* A, int64_t lda, bool a_k, const float* B, int64_t ldb, bool b_k, float* C,
          int64_t ldc, int M, int N, int K, const float* bias, const float* bias2, int flags) {
  const TraceScope ts("gemm");
  EpStore ep = make_store(C, ldc, M, N, bias, bias2, flags);
  int ks = (flags & EP_ATOMIC) ? pick_ksplit(M, N, K, bf16) : 1;
  // skinny products (a 20- or 39-wide side: embedding part of the first decoder layer, projector and their backward): 128 x 128 tiles
  // give 48 workgroups for 6144 rows and pad N or K 3-6x; the 32 x 32 step kernel (K quartered over its waves) fills the chip
  // (only where K is a multiple of the step kernel's 16-deep chunk: its fragment loads have no K tail)
  const bool skinny = bf16 && M >= 1024 && N <= 64 && K % 16 == 0 && !knob::AOCR_NO_SKINNY();  // (an EP_ATOMIC epilogue stays atomic: one add per element, no split-K)
  if (skinny && a_k && b_k) { SmallKKArgs z; z.a = make_loadk(A, lda, M, K); z.b = make_loadk(B, ldb, N, K); z.ep = ep; z.K = K; launch_small_kk(s, true, 1, &z, M, N); }
  else if (skinny && a_k && !b_k) { SmallKMNArgs z; z.a = make_loadk(A, lda, M, K); z.b = make_loadmn(B, ldb, N, K); z.ep = ep; z.K = K; launch_small_kmn(s, true, 1, &z, M, N); }
  else if (a_k && b_k) launch_big_kk(s, bf16, make_loadk(A, lda, M, K), make_loadk(B, ldb, N, K), ep, M, N, K, ks);
  else if (a_k && !b_k) launch_big_kmn(s, bf16, make_loadk(A, lda, M, K), make_loadmn(B, ldb, N, K), ep, M, N, K, ks);
  else if (!a_k && !b_k) launch_big_mnmn(s, bf16, make_loadmn(A, lda, M, K), make_loadmn(B, ldb, N, K), ep, M, N, K, ks);
  else return -1;   // A^T * B^T never occurs on the hot path
  return 0;
}

// ---- Round 6: projector + criterion + projector data gradient as ONE launch (model.lua:594-612 forward, :648 backward; criterion.lua:3-9).
// Between the two whole-sequence decoder kernels a training step ran three dependent launches on a nearly idle chip -- logits = out W_o^T + b (39 columns),
// LogSoftMax + ClassNLL + d logits (one wave per row), d out = d logits W_o (K = 39) -- 14 + 8 + 28 us and their launch gaps at C3.  One workgroup per 32 rows does
// all three here, each with the arithmetic of the launch it replaces, in the same order (so every output is bit-identical to the three-launch form):
//   1. gemm_small_body (the skinny-product kernel's body: K quartered over the four waves, partial tiles summed through LDS in wave order), both 32-column tiles,
//      the epilogue adding the bias into an LDS tile instead of memory;
//   2. lsm_nll_wave_kernel's row: one wave per row, lane = class, butterfly maximum / sum; logits, NLL and d logits stored, d logits kept as bf16 in LDS;
//   3. d out tile = three chained v_mfma_f32_32x32x16_bf16 over k = 0..47 (classes past V are zero, as the 128 x 128 kernel pads), W_o fragments straight
//      from memory (80 KB, L2-resident; k-strided, lanes along Hd).
struct EpLogitTile {
  float* tile; const float* bias; int m0, N;
  template <int NT> __device__ __forceinline__ void quad(int m, int n, int nstep, const float (&v)[NT][4]) const {
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) {
      const int col = n + nstep * ni;
      if (col >= N) continue;
      float bb = 0.f;
      if (bias) bb = bias[col];
#pragma unroll
      for (int i = 0; i < 4; ++i) tile[(m - m0 + i) * 65 + col] = v[ni][i] + bb;
    }
  }
};
struct ProjLossArgs {
  LoadK a, b; const float* bias; const float* wo; int64_t ldw;
  float* logits; float* dlogits; int64_t ld; float* nll; float* dout; int64_t lddo;
  const int32_t* tgt; int64_t st, sb; int Bt, rows, V, K; float scale;
};
__device__ __forceinline__ float pl_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float pl_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__global__ __launch_bounds__(256) void project_loss_kernel(ProjLossArgs g) {
  __shared__ float red[4 * 2 * 16 * 64];
  __shared__ float tile[32 * 65];
  __shared__ __attribute__((aligned(16))) bf16_t dl[32][56];           // d logits as the product's A operand: k = class, padded to 48 (+ 8: rows 112 bytes apart)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m0 = blockIdx.y * 32;
  {
    SmallArgs<LoadK, LoadK, EpLogitTile> sa; sa.a = g.a; sa.b = g.b; sa.ep = EpLogitTile{tile, g.bias, m0, g.V}; sa.K = g.K;
    gemm_small_body<true, 2, false, 4, false>(sa, 0, red);
  }
  __syncthreads();
  const int V = g.V;
#pragma unroll 1
  for (int i = 0; i < 8; ++i) {
    const int row = wave * 8 + i;
    const int64_t r = (int64_t)m0 + row;
    float dv = 0.f;
    if (r < g.rows) {                                              // (wave-uniform)
      const float xv = lane < V ? tile[row * 65 + lane] : -INFINITY;
      const float mx = pl_wave_max(xv);
      const float sum = pl_wave_sum(lane < V ? expf(xv - mx) : 0.f);
      const float lse = mx + logf(sum);
      const int64_t t = r / g.Bt, b = r - t * g.Bt;
      const int y = g.tgt[t * g.st + b * g.sb] - 1;
      const float wy = (y == 0) ? 0.f : 1.f;                       // criterion.lua:5: weights[PAD] = 0
      if (lane < V) g.logits[r * g.ld + lane] = xv;
      if (lane == y) g.nll[r] = -wy * (xv - lse);
      const float gs = g.scale * wy;
      if (lane < V) { dv = gs * (expf(xv - lse) - (lane == y ? 1.f : 0.f)); g.dlogits[r * g.ld + lane] = dv; }
      for (int v = V + lane; v < g.ld; v += 64) g.dlogits[r * g.ld + v] = 0.f;
    }
    if (lane < 56) dl[row][lane] = (bf16_t)dv;
  }
  __syncthreads();
  const int r = lane & 31, h = lane >> 5;
  bf16x8 af[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) af[c] = *reinterpret_cast<const bf16x8*>(&dl[r][16 * c + 8 * h]);
  const int ntiles = g.K / 32;                                      // Hd / 32 column tiles of d out, wave w takes w, w + 4, ...
  for (int nt = wave; nt < ntiles; nt += 4) {
    const float* wcol = g.wo + 32 * nt + r;
    Frag<8> fb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 16 * c + 8 * h + j;
        const float w = wcol[(int64_t)min(k, V - 1) * g.ldw];
        fb[c].v[j] = k < V ? w : 0.f;
      }
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[c], to_bf16x8(fb[c]), acc, 0, 0, 0);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int64_t row = (int64_t)m0 + 8 * (e >> 2) + 4 * h + (e & 3);
      if (row < g.rows) g.dout[row * g.lddo + 32 * nt + r] = acc[e] + 0.f;
    }
  }
}
bool project_loss_ok(int rows, int V, int Hd) {
  return rows >= 1024 && V >= 2 && V <= 40 && Hd % 64 == 0 && !knob::AOCR_NO_SKINNY() && !knob::AOCR_NO_PROJ_FUSE();      // rows >= 1024: where gemm() takes the skinny kernel for the logits
}
void project_loss(hipStream_t s, const float* out, int64_t ldo, const float* wo, const float* bo, float* logits, float* dlogits, int64_t ld, float* nll, float* dout,
                  const int32_t* tgt, int64_t st, int64_t sb, int Bt, int rows, int V, int Hd, float scale) {
  ProjLossArgs g; g.a = make_loadk(out, ldo, rows, Hd); g.b = make_loadk(wo, Hd, V, Hd); g.bias = bo; g.wo = wo; g.ldw = Hd;
  g.logits = logits; g.dlogits = dlogits; g.ld = ld; g.nll = nll; g.dout = dout; g.lddo = Hd; g.tgt = tgt; g.st = st; g.sb = sb; g.Bt = Bt; g.rows = rows; g.V = V; g.K = Hd; g.scale = scale;
  hipLaunchKernelGGL(project_loss_kernel, dim3(1, cdiv(rows, 32)), dim3(256), 0, s, g);
}

// hoisted bf16 GEMMs with 256 x 128 tiles that fill the chip take the narrow LDS-DMA kernel (two workgroups per CU: one's epilogue under the other's 16-step K loop):
// hoisted GEMMs 0.739 -> 0.713 ms per C3 step (AOCR_NO_HH_NARROW: the 128 x 128 kernels).  A ragged last row tile is taken too unless AOCR_HH_NARROW_FULL_ONLY=1
static bool hh_narrow_ok(int M, int N, int K) {
  return !knob::AOCR_NO_HH_NARROW() && !knob::AOCR_NO_DMA() && (M % 256 == 0 || (M >= 256 && !knob::AOCR_HH_NARROW_FULL_ONLY())) && N % 128 == 0 && K % 32 == 0 && cdiv(M, 256) * (N / 128) >= 200;
}
void gemm_hh(hipStream_t s, const bf16_t* A, int64_t lda, const bf16_t* B, int64_t ldb, float* C, int64_t ldc, int M, int N, int K,
             const float* bias, const float* bias2, int flags) {
  const TraceScope ts("gemm_hh");
  LoadKh a; a.p = A; a.ld = lda; a.rows = M; a.K = K;
  LoadKh b; b.p = B; b.ld = ldb; b.rows = N; b.K = K;
  // (the 256 x 256 LDS-DMA kernel was measured slower here: K = 512 is only 16 tiles deep -- hoisted encoder projection at C3,
  // 63 x 4 workgroups: 56 / 47 us against 47 / 43 us; round 3: the BK = 64 form of the 128 x 128 kernel -- half the barriers and
  // staging round trips over the 16 tiles -- measured slower too: hoisted GEMMs 0.726 -> 0.745 ms per step)
  // (round 3, again with that kernel's output tile staged through LDS: hoisted GEMMs 0.750 -> 0.760 ms per step: still no faster)
  if (hh_narrow_ok(M, N, K)) { launch_dma_narrow(s, a, b, make_store(C, ldc, M, N, bias, bias2, flags), M, N, K); return; }
  if (dma128_eligible(M, N, K, 32)) { launch_dma128(s, a, b, make_store(C, ldc, M, N, bias, bias2, flags), M, N, K); return; }       // small / ragged M (32-64 lines per GPU)
  launch_lds(s, a, b, make_store(C, ldc, M, N, bias, bias2, flags), M, N, K, 1);
}

// C = [A0 | A1] . [B0 | B1]^T  (K = K0 + K1 over two buffer pairs; bf16, K-contiguous), one launch of the narrow LDS-DMA kernel.  Returns false when the
// shape does not take that kernel (the caller then runs two products).
bool gemm_hh_cat(hipStream_t s, const bf16_t* A0, const bf16_t* A1, int64_t lda, const bf16_t* B0, const bf16_t* B1, int64_t ldb, float* C, int64_t ldc, int M, int N, int K0, int K1) {
  if (K0 % 32 || K1 % 32 || !hh_narrow_ok(M, N, K0 + K1) || knob::AOCR_NO_HH_CAT()) return false;
  const TraceScope ts("gemm_hh_cat");
  LoadKhCat a; a.p0 = A0; a.p1 = A1; a.ld0 = a.ld1 = lda; a.rows = M; a.K0 = K0; a.K = K0 + K1;
  LoadKhCat b; b.p0 = B0; b.p1 = B1; b.ld0 = b.ld1 = ldb; b.rows = N; b.K0 = K0; b.K = K0 + K1;
  launch_dma_narrow(s, a, b, make_store(C, ldc, M, N, nullptr, nullptr, 0), M, N, K0 + K1);
  return true;
}

void gemm_hh_shadow(hipStream_t s, const bf16_t* A, int64_t lda, const bf16_t* B, int64_t ldb, float* C, int64_t ldc, bf16_t* Cb, int64_t ldcb,
                    int M, int N, int K) {
  const TraceScope ts("gemm_hh_shadow");
  LoadKh a; a.p = A; a.ld = lda; a.rows = M; a.K = K;
  LoadKh b; b.p = B; b.ld = ldb; b.rows = N; b.K = K;
  EpStore e = make_store(C, ldc, M, N, nullptr, nullptr, 0); e.Cb = Cb; e.ldcb = ldcb;
  if (hh_narrow_ok(M, N, K)) {
    if (!knob::AOCR_NO_NARROW_STAGED()) e.C = nullptr;     // every reader takes the bf16 copy (ctx W_a of the decoder kernels): the staged tile skips the fp32 store (33 MB per C3 step)
    launch_dma_narrow(s, a, b, e, M, N, K); return;
  }
  if (dma128_eligible(M, N, K, 32)) { launch_dma128(s, a, b, e, M, N, K); return; }
  launch_lds(s, a, b, e, M, N, K, 1);
}

template <class LD, class KERNEL>
static void grouped_launch(hipStream_t s, const WGradProblem* const* q, int cnt, int slots, bool shadows, KERNEL kernel) {
  int64_t tiles = 0;
  for (int i = 0; i < cnt; ++i) tiles += (int64_t)cdiv(q[i]->M, 128) * cdiv(q[i]->N, 128);
  int ks = (int)(slots / tiles); if (ks < 1) ks = 1;          // common split: fill one resident round
  GroupArgs<LD, LD, EpStore> g; g.n = cnt; int first = 0;
  for (int i = 0; i < cnt; ++i) {
    auto& P = g.p[i];
    int ksplit = ks, kper; split_k(q[i]->K, 32, ksplit, kper);
    if constexpr (std::is_same<LD, LoadMNh>::value) {
      P.a.p = q[i]->Ab; P.a.ld = q[i]->lda; P.a.rows = q[i]->M; P.a.K = q[i]->K;
      P.b.p = q[i]->Bb; P.b.ld = q[i]->ldb; P.b.rows = q[i]->N; P.b.K = q[i]->K;
    } else {
      P.a = make_loadmn(q[i]->A, q[i]->lda, q[i]->M, q[i]->K); P.b = make_loadmn(q[i]->B, q[i]->ldb, q[i]->N, q[i]->K);
    }
    P.ep = make_store(q[i]->C, q[i]->ldc, q[i]->M, q[i]->N, nullptr, nullptr, ksplit > 1 ? EP_ATOMIC : EP_ACCUM);
    P.K = q[i]->K; P.kper = kper; P.gx = cdiv(q[i]->N, 128); P.ksplit = ksplit; P.first = first;
    first += cdiv(q[i]->M, 128) * P.gx * ksplit;
  }
  g.total = first; (void)shadows;
  for (int i = 0; i < cnt; ++i) trace_launch(shadows ? "wgrad_tr_grouped_kernel" : "gemm_lds_grouped_kernel", "", q[i]->M, q[i]->N, q[i]->K);
  hipLaunchKernelGGL(kernel, dim3(first), dim3(256), 0, s, g);
}

// round 4: deep problems with full 256 x 256 tiles on the LDS-DMA skeleton (wgrad_dma_grouped_kernel), slabs in `part`; returns how many it took (the first `cnt` of q)
static int grouped_launch_dma(hipStream_t s, const WGradProblem* const* q, int cnt, float* part, size_t part_floats) {
  if (cnt <= 0 || !part) return 0;
  if (cnt > 8) cnt = 8;
  long long tiles = 0; int kmin = 1 << 30;
  for (int i = 0; i < cnt; ++i) { tiles += (long long)(q[i]->M / 256) * (q[i]->N / 256); kmin = std::min(kmin, q[i]->K); }
  int ks = (int)(knob::AOCR_WGRAD_DMA_WGS() / tiles); if (ks < 1) ks = 1;           // never more than one round of the 256 CUs (312 workgroups = a second round of 56: 120 instead of 75 us for the encoder's four problems)
  ks = std::min(ks, std::max(1, kmin / 768));                                 // at least 24 K steps per workgroup
  while (ks > 1 && (size_t)tiles * 65536 * ks > part_floats) --ks;
  if ((size_t)tiles * 65536 * ks > part_floats) return 0;
  WgDmaArgs g; g.n = cnt; int first = 0; long long f4 = 0; size_t off = 0;
  for (int i = 0; i < cnt; ++i) {
    WgDmaProblem& P = g.p[i];
    int ksplit = ks, kper; split_k(q[i]->K, 32, ksplit, kper);
    P.A = q[i]->Ab; P.B = q[i]->Bb; P.lda = q[i]->lda; P.ldb = q[i]->ldb; P.M = q[i]->M; P.N = q[i]->N; P.K = q[i]->K;
    P.gx = q[i]->N / 256; P.tiles = (q[i]->M / 256) * P.gx; P.ks = ksplit; P.kper = kper; P.first = first; first += P.tiles * ksplit;
    P.part = part + off; off += (size_t)P.M * P.N * ksplit;
    P.C = q[i]->C; P.ldc = q[i]->ldc; P.f4first = f4; f4 += (long long)P.M * (P.N / 4);
  }
  g.total = first; g.f4total = f4;
  for (int i = 0; i < cnt; ++i) trace_launch("wgrad_dma_grouped_kernel", "slab_reduce", q[i]->M, q[i]->N, q[i]->K);
  hipLaunchKernelGGL((wgrad_dma_grouped_kernel<0>), dim3(first), dim3(512), 0, s, g, zero_page());
  hipLaunchKernelGGL((wgrad_slab_reduce_kernel<0>), dim3((unsigned)((f4 + 255) / 256)), dim3(256), 0, s, g);
  return cnt;
}
void grouped_wgrad(hipStream_t s, bool bf16, const WGradProblem* p, int n, float* part, size_t part_floats) {
  const TraceScope ts("grouped_wgrad");
  if (!bf16) {                                                // fp32 mode: one launch per problem
    for (int i = 0; i < n; ++i)
      gemm(s, false, p[i].A, p[i].lda, false, p[i].B, p[i].ldb, false, p[i].C, p[i].ldc, p[i].M, p[i].N, p[i].K, nullptr, nullptr, EP_ATOMIC);
    return;
  }
  // problems whose operands both have bf16 shadows (16-byte pieces: M, N, lda, ldb multiples of 8) take the transposed-read kernel
  const WGradProblem* hs[16]; const WGradProblem* fs[16]; const WGradProblem* ds[16]; int nh = 0, nf = 0, nd = 0;
  const bool dma_ok = part && !knob::AOCR_NO_DMA() && !knob::AOCR_NO_WGRAD_DMA_GROUPED();
  const int dma_mink = knob::AOCR_WGRAD_DMA_MINK();      // smallest K (rows L B / T B) that takes the LDS-DMA kernel
  for (int i = 0; i < n && i < 16; ++i) {
    const bool ok = p[i].Ab && p[i].Bb && p[i].M % 8 == 0 && p[i].N % 8 == 0 && p[i].lda % 8 == 0 && p[i].ldb % 8 == 0;
    const bool deep = ok && dma_ok && p[i].M % 256 == 0 && p[i].N % 256 == 0 && p[i].K % 32 == 0 && p[i].K >= dma_mink &&
                      ((reinterpret_cast<uintptr_t>(p[i].Ab) | reinterpret_cast<uintptr_t>(p[i].Bb)) & 15) == 0;
    if (deep && nd < 8) ds[nd++] = &p[i]; else if (ok) hs[nh++] = &p[i]; else fs[nf++] = &p[i];
  }
  if (nd > 0 && grouped_launch_dma(s, ds, nd, part, part_floats) != nd)
    for (int i = 0; i < nd; ++i) hs[nh++] = ds[i];                             // no room for the slabs: the transposed-read kernel
  for (int base = 0; base < nh; base += 8)
    grouped_launch<LoadMNh>(s, hs + base, std::min(8, nh - base), 1024, true, wgrad_tr_grouped_kernel<EpStore>);
  for (int base = 0; base < nf; base += 8)
    grouped_launch<LoadMN>(s, fs + base, std::min(8, nf - base), 768, false, gemm_lds_grouped_kernel<LoadMN, LoadMN, EpStore>);
}

// ---------------------------------------------------------------------------------------------
// convolution layers, channels-last.  Output grid Ho = H + 2*pad - ks + 1 (stride 1).  When bf16 shadows of both
// operands are supplied the bf16-source loaders are used (half the L2->L1 bytes, no conversion in the kernel).
// ---------------------------------------------------------------------------------------------
static LoadConvK make_convk(const float* src, int B, int Hs, int Ws, int C, int ks, int sgn, int off, int Hr, int Wr, int pool) {
  LoadConvK a; a.src = src; a.H = Hs; a.W = Ws; a.C = C; a.KW = ks; a.sgn = sgn; a.off = off; a.Hr = Hr; a.Wr = Wr;
  a.pmode = pool; a.Hp = Hr / 2; a.Wp = Wr / 2;
  if (pool == 1) a.rows = B * a.Hp * a.Wp * 4; else if (pool == 2) a.rows = B * a.Hp * Wr * 2; else a.rows = B * Hr * Wr;
  a.K = ks * ks * C;
  return a;
}

void conv_forward(hipStream_t s, bool bf16, const float* x, const float* w, const float* bias, float* y, uint8_t* idx, int B,
                  int H, int W, int Cin, int Cout, int ks, int pad, int relu, int pool, const bf16_t* xb, const bf16_t* wb,
                  bf16_t* yb, int profile_tag, const float* bn_save, const float* bn_w, const float* bn_b, double* bn_part, int* bn_chunks, int* y_bf16) {
  const TraceScope ts("conv_forward");
  const int Ho = H + 2 * pad - ks + 1, Wo = W + 2 * pad - ks + 1;
  LoadConvK a = make_convk(x, B, H, W, Cin, ks, 1, -pad, Ho, Wo, pool);
  EpConv ep; ep.y = y; ep.idx = idx; ep.bias = bias; ep.Cout = Cout; ep.rows = a.rows; ep.pmode = pool; ep.relu = relu; ep.yb = yb;
  ep.bn_save = bn_save; ep.bn_w = bn_w; ep.bn_b = bn_b;
  if (bn_chunks) *bn_chunks = 0;
  if (y_bf16) *y_bf16 = 0;
  if (bf16 && xb && wb) {
    LoadConvKh ah; ah.src = xb; ah.g = a;
    LoadKh bh; bh.p = wb; bh.ld = a.K; bh.rows = Cout; bh.K = a.K;
    // BatchNorm statistics in the epilogue: only where EVERY tile of the launch takes tile256_store_f32 (full 256 x 256 tiles of a 256-wide LDS-DMA kernel with the
    // staged fp32 tile switched on; the 8-wave halo kernel has no staged epilogue), and the row tiles fit bn_relu_forward's chunk table (512)
    if (bn_part && bn_chunks && y && !yb && !bn_save && pool == 0 && dma_eligible(a.rows, Cout, a.K, Cin) && a.rows % 256 == 0 && a.rows / 256 <= 512 && !knob::AOCR_NO_BN_STATS_FUSE()) {
      if (staged256(2, pad == 1 && halo_eligible(a, Cout, 256, 256))) {
        ep.bn_part = bn_part; *bn_chunks = a.rows / 256;
        // The statistics come from the accumulators, so y itself could be stored as bf16 (AOCR_BN_Y16=1): -0.065 ms per C3 step (BatchNorm 0.49 -> 0.46 ms, conv forward
        // 0.83 -> 0.755) -- NOT the default: it is one more rounding than "bf16 contraction operands" (the model tests/test_configs_gpu.py holds the product to), and the
        // ReLU / arg-max decisions it flips take the conv-stack gradients from cosine 0.997 to 0.986 against the bf16-operand oracle (limit 0.995).
        if (y_bf16 && knob::AOCR_BN_Y16() && Cout % 4 == 0 && !knob::AOCR_BN_PARTIAL_OLD()) {   // only bn_partial4_kernel / bn_apply_relu_kernel read a bf16 x (xh): never with the 4-byte-access fallback
          ep.y16 = reinterpret_cast<bf16_t*>(y); ep.y = nullptr; *y_bf16 = 1; }
      }
    }
    // (conv3 -- K = 1152: 36 steps under an un-overlapped epilogue -- on 256 x 128 tiles of the narrow kernel instead: conv forward 0.79 -> 0.763 ms, but that kernel's
    // epilogue cannot leave the BatchNorm sums, which are worth more (0.04 ms for conv3): not taken)
    if (dma_eligible(a.rows, Cout, a.K, Cin) && pad == 1 && halo_eligible(a, Cout, 256, 256)) launch_halo<1, 256, 256>(s, ah, bh, ep, a.rows, Cout, profile_tag);
    else if (dma_eligible(a.rows, Cout, a.K, Cin)) launch_dma(s, ah, bh, ep, a.rows, Cout, a.K, profile_tag);
    else if (dma_narrow_eligible(a.rows, Cout, a.K, Cin) || dma_mid_eligible(a.rows, Cout, a.K, Cin)) launch_dma_narrow(s, ah, bh, ep, a.rows, Cout, a.K);
    else if (dma128_eligible(a.rows, Cout, a.K, Cin)) launch_dma128(s, ah, bh, ep, a.rows, Cout, a.K);
    else launch_lds(s, ah, bh, ep, a.rows, Cout, a.K, 1);       // (BK = 64 variant measured no faster: launch_lds64)
  } else {
    launch_conv_fwd(s, bf16, a, make_loadk(w, a.K, Cout, a.K), ep, a.rows, Cout, a.K);
  }
}

// the bf16 data gradient `a` leaves its map as bf16 (dx16: see conv_backward_data): opt-in, and only where every tile is a staged 256 x 256 one
static bool dgrad_bf16_out(const LoadConvK& a, int Cin, int Cout, int pad) {
  return dma_eligible(a.rows, Cin, a.K, Cout) && a.rows % 256 == 0 && Cin % 256 == 0 && knob::AOCR_DX16() && !knob::AOCR_BN_PARTIAL_OLD() && !knob::AOCR_UNPOOL4() &&   // (the generic forms of the two reader kernels take fp32 only)
         staged256(1, pad == 1 && halo_eligible(a, Cin, 256, 256));
}
bool conv_dgrad_bf16_out(int B, int H, int W, int Cin, int Cout, int ks, int pad) {
  const int Ho = H + 2 * pad - ks + 1, Wo = W + 2 * pad - ks + 1;
  return dgrad_bf16_out(make_convk(nullptr, B, Ho, Wo, Cout, ks, -1, pad, H, W, 0), Cin, Cout, pad);
}

void conv_backward_data(hipStream_t s, bool bf16, const float* dy, const float* w, float* dx, int B, int H, int W, int Cin,
                        int Cout, int ks, int pad, const bf16_t* dyb, const bf16_t* wtb, const float* wtf, int* dx16, const BnBwdFuse* bnb, int* bnb_chunks) {
  const TraceScope ts("conv_backward_data");
  const int Ho = H + 2 * pad - ks + 1, Wo = W + 2 * pad - ks + 1;
  LoadConvK a = make_convk(dy, B, Ho, Wo, Cout, ks, -1, pad, H, W, 0);
  EpStore ep = make_store(dx, Cin, a.rows, Cin);
  if (dx16) *dx16 = 0;
  if (bnb_chunks) *bnb_chunks = 0;
  if (bf16 && dyb && wtb) {
    LoadConvKh ah; ah.src = dyb; ah.g = a;
    LoadKh bh; bh.p = wtb; bh.ld = a.K; bh.rows = Cin; bh.K = a.K;          // wtb [Cin][tap][Cout]: K-contiguous over (tap, co)
    // Round 4: the data gradient as bf16 INTO THE SAME BUFFER (half of it) when the caller accepts that (dx16) -- its only readers are the BatchNorm backward /
    // un-pool passes, which round their own output to bf16 for the next contraction anyway, and the map is 2 of the 10-12 bytes per element those
    // HBM-bound passes move.  Only where the staged 256 x 256 tile exists (4-wave halo kernel / gemm_dma_bf16_kernel, full tiles).
    // OPT-IN (AOCR_DX16=1), not the default -- measured at C3: 5.463 -> 5.407 ms per step (BatchNorm 0.50 -> 0.48, data gradients 0.79 -> 0.77), but it is one more
    // rounding than "bf16 contraction operands", the model the parity tests hold the product to: with the GPU's decisions imposed on the bf16-operand oracle the
    // lowest gradient cosine falls from 0.99998 to 0.99983 (conv2.b; tests/test_configs_gpu.py requires 0.9999).  Parity first -- as for AOCR_BN_Y16.
    if (dx16 && dgrad_bf16_out(a, Cin, Cout, pad)) { ep.C = nullptr; ep.Cb = reinterpret_cast<bf16_t*>(dx); ep.ldcb = Cin; *dx16 = 1; }
    // Round 4: the sums pass of the BatchNorm backward that follows -- (sum d, sum d xhat) per channel, a re-read of this output (4 B), x (4 B) and the mask
    // (2 B) per element -- from the staged fp32 tile of the 256 x 256 kernels: the output values pass through a thread that keeps four fixed columns anyway
    // (as for the forward statistics, EpConv::bn_part), so only x and the mask are read, by the workgroup that has the tile's output in LDS.
    // Only where EVERY tile of the launch takes tile256_store_f32 (full tiles, staged fp32 tile on).
    // MEASURED, NOT THE DEFAULT (AOCR_BNB_FUSE=1 turns it on): at C3 the BatchNorm family drops 0.50 -> 0.365 ms per step, but the data gradients rise 0.767 -> 0.931 ms
    // -- the 201 MB of x / mask reads per layer land in an epilogue that nothing overlaps (one workgroup per CU, all of a round finishing together) -- net
    // 5.262 -> 5.280 ms per step, same box, two runs each.  The separate sums pass runs at 5.1 TB/s; it stays.
    if (bnb && bnb_chunks && ep.C && dma_eligible(a.rows, Cin, a.K, Cout) && a.rows % 256 == 0 && Cin % 256 == 0 && a.rows / 256 <= 512 && knob::AOCR_BNB_FUSE() &&
        staged256(1, pad == 1 && halo_eligible(a, Cin, 256, 256))) {
      ep.bnb_x = bnb->x; ep.bnb_yb = bnb->yb; ep.bnb_save = bnb->save; ep.bnb_part = bnb->part; *bnb_chunks = a.rows / 256;
    }
    if (dma_eligible(a.rows, Cin, a.K, Cout) && pad == 1 && halo_eligible(a, Cin, 256, 256)) launch_halo<-1, 256, 256>(s, ah, bh, ep, a.rows, Cin);
    else if (dma_eligible(a.rows, Cin, a.K, Cout)) launch_dma(s, ah, bh, ep, a.rows, Cin, a.K);
    else if (dma_narrow_eligible(a.rows, Cin, a.K, Cout)) launch_dma_narrow(s, ah, bh, ep, a.rows, Cin, a.K);
    else if (dma128_eligible(a.rows, Cin, a.K, Cout)) launch_dma128(s, ah, bh, ep, a.rows, Cin, a.K);
    else launch_lds(s, ah, bh, ep, a.rows, Cin, a.K, 1);
  } else if (wtf) {                                          // fp32 taps re-laid [Cin][tap][Cout]: K-contiguous dwordx4 loads
    launch_big(s, bf16, a, make_loadk(wtf, a.K, Cin, a.K), ep, a.rows, Cin, a.K, 1);
  } else {
    LoadConvWT b; b.w = w; b.Cin = Cin; b.Cout = Cout; b.KK = ks * ks; b.K = a.K;
    launch_conv_dgrad(s, bf16, a, b, ep, a.rows, Cin, a.K);
  }
}

void conv_backward_filter(hipStream_t s, bool bf16, const float* x, const float* dy, float* dw, float* dbias, int B, int H,
                          int W, int Cin, int Cout, int ks, int pad, const bf16_t* xb, const bf16_t* dyb, float* part, size_t part_floats, int profile_tag) {
  const TraceScope ts("conv_backward_filter");
  const int Ho = H + 2 * pad - ks + 1, Wo = W + 2 * pad - ks + 1;
  const int P = B * Ho * Wo, N = ks * ks * Cin;
  LoadConvXcol b; b.x = x; b.H = H; b.W = W; b.Cin = Cin; b.KW = ks; b.pad = pad; b.Ho = Ho; b.Wo = Wo; b.N = N; b.K = P;
  EpStore ep = make_store(dw, N, Cout, N, nullptr, nullptr, EP_ATOMIC);
  const int ksplit = pick_ksplit(Cout, N, P, bf16, (bf16 && xb && dyb) ? 1024 : 768);   // bf16-source kernel: 4 workgroups per CU
  if (bf16 && xb && dyb) {
    LoadMNh ah; ah.p = dyb; ah.ld = Cout; ah.rows = Cout; ah.K = P;
    LoadConvXcolh bh; bh.x = xb; bh.g = b;
    // 256 x 256 LDS-DMA kernel when Cout and N fill its tiles (measured on workload C3: conv4/5/6 249/239/427 -> 220/223/380 us;
    // conv7 (N = 2048) and conv3 (N = 1152) are no faster and stay on the 128 x 128 kernel)
    const int tiles = cdiv(N, 256) * (Cout / 256);
    // halo-resident kernel (conv_wgrad_halo_kernel, round 4): N tiles of nine taps x 32 input channels, the input map's halo staged once per 32-pixel row
    // segment -- 22.4 instead of 32 KB per K step through L2 -> LDS.  3 x 3 / pad 1 layers whose rows are whole 32-pixel segments; needs the slab scratch.
    // Same-box, same harness (tools/ubench/wgrad_halo.hip) at the C3 shapes: conv4 193 -> 166 us, conv5 180 -> 151 us, conv6 327 -> 276 us.
    // AOCR_NO_WGRAD_HALO=1: the one-tap-per-tile kernels below (the parity reference).
    const int hmt = Cout % 256 == 0 ? 256 : 128;            // tile rows: 256 output channels (eight waves), or 128 for conv2 (four waves)
    // (round 6: ragged rows too -- W % 32 != 0 pads every row to whole 32-pixel segments with zero slots; taken while at least 3/4 of the slots are pixels:
    //  the reference-default shape's 25- / 50-wide maps (0.78).  AOCR_WGRAD_HALO_RAGGED=0: whole segments only, as before)
    const int spr = (W + 31) / 32;
    const bool ragged_ok = W % 32 == 0 || (knob::AOCR_WGRAD_HALO_RAGGED() && W * 4 >= spr * 32 * 3);
    // AOCR_WGRAD_HALO_MINN (576): conv2 (64 -> 128) upwards; A/B at C3: 2304 -> 1152 (conv3 too) = 5.505 -> 5.455 ms per step, 1152 -> 576 (conv2 too, 128-channel tiles): see DESIGN.md
    if (ks == 3 && pad == 1 && ragged_ok && Cout % hmt == 0 && Cin % 32 == 0 && part && !knob::AOCR_NO_DMA() && !knob::AOCR_NO_WGRAD_HALO() && !knob::AOCR_WGRAD_ATOMIC() &&
        (knob::AOCR_FORCE_DMA() || (P >= 8192 && N >= knob::AOCR_WGRAD_HALO_MINN()))) {
      const int htiles = (Cin / 32) * (Cout / hmt), S = B * H * spr;
      int ksh = htiles >= 256 ? 1 : 256 / htiles; if (ksh > S) ksh = S;                   // one round of the 256 CUs
      { const int minsteps = knob::AOCR_WGRAD_HALO_MINSTEPS();       // A/B: at small P fewer, longer k ranges (less slab traffic) instead of a full round
        if (minsteps > 0 && S / ksh < minsteps) ksh = std::max(1, S / minsteps); }
      const int per = cdiv(S, ksh); ksh = cdiv(S, per);
      const size_t mn = (size_t)Cout * N;
      if (mn * ksh <= part_floats) {
        // (IM = !AOCR_NO_WGRAD_ISSUE_MID: MFMAs start behind their own k-half's reads, DMA issue between the halves -- mfma_gemm.h)
#define AOCR_WGH(TAGV, MGV, RGV, IMV, THREADS, MTV) hipLaunchKernelGGL((conv_wgrad_halo_kernel<TAGV, MGV, RGV, IMV>), dim3(htiles * ksh), dim3(THREADS), 0, s, dyb, xb, part, (long long)mn, B, H, W, Cin, Cout, Cin / 32, Cout / MTV, ksh, per, zero_page())
        const bool im = !knob::AOCR_NO_WGRAD_ISSUE_MID();
        { char inst[48]; snprintf(inst, sizeof inst, "%d,%s,%s", hmt, W % 32 ? "ragged" : "whole", im ? "issue_mid" : "no_issue_mid");
          trace_launch("conv_wgrad_halo_kernel", inst, Cout, N, P); }
        if (W % 32) {                                            // ragged rows: the form with the row-end pointer steps and the d y validity compare
          if (hmt == 128) { if (im) AOCR_WGH(0, 2, true, true, 256, 128); else AOCR_WGH(0, 2, true, false, 256, 128); }
          else { if (im) AOCR_WGH(0, 4, true, true, 512, 256); else AOCR_WGH(0, 4, true, false, 512, 256); }
        }
        else if (hmt == 128) { if (im) AOCR_WGH(0, 2, false, true, 256, 128); else AOCR_WGH(0, 2, false, false, 256, 128); }
        else if (profile_tag) { if (im) AOCR_WGH(1, 4, false, true, 512, 256); else AOCR_WGH(1, 4, false, false, 512, 256); }
        else { if (im) AOCR_WGH(0, 4, false, true, 512, 256); else AOCR_WGH(0, 4, false, false, 512, 256); }
#undef AOCR_WGH
        splitk_reduce(s, part, ksh, mn, dw);
        if (dbias) colsum_accum(s, dy, Cout, P, Cout, dbias);
        return;
      }
    }
    if (Cout % 256 == 0 && Cin % 8 == 0 && !knob::AOCR_NO_DMA() && (knob::AOCR_FORCE_DMA() || (P >= 8192 && tiles <= 256 && N % 256 == 0 && N >= 2304))) {
      int ks2 = tiles >= 128 ? (tiles >= 200 ? 1 : 2) : 256 / tiles, kper2; split_k(P, 32, ks2, kper2);      // one round of the 256 CUs
      const size_t mn = (size_t)Cout * N;
      float* const slab = (part && ks2 > 1 && mn * ks2 <= part_floats && !knob::AOCR_WGRAD_ATOMIC()) ? part : nullptr;
      trace_launch("conv_wgrad_dma_kernel", slab ? "slab" : "atomic", Cout, N, P);
      if (profile_tag)        // the same kernel under its own symbol (TAG 1): aocr_profile_kernel, per-kernel rocprofv3 / PMC rows
        hipLaunchKernelGGL((conv_wgrad_dma_kernel<EpStore, 0, 1>), dim3(tiles * ks2), dim3(512), 0, s, ah, bh, ep, P, kper2, cdiv(N, 256), Cout / 256, zero_page(), ks2, slab, (long long)mn);
      else
        hipLaunchKernelGGL((conv_wgrad_dma_kernel<EpStore>), dim3(tiles * ks2), dim3(512), 0, s, ah, bh, ep, P, kper2, cdiv(N, 256), Cout / 256, zero_page(), ks2, slab, (long long)mn);
      if (slab) splitk_reduce(s, slab, ks2, mn, dw);
      if (dbias) colsum_accum(s, dy, Cout, P, Cout, dbias);
      return;
    }
    int ks = ksplit, kper; split_k(P, 32, ks, kper);
    const int gx = cdiv(N, 128), gy = cdiv(Cout, 128);
    const size_t mn = (size_t)Cout * N;
    float* const slab = (part && ks > 1 && mn * ks <= part_floats && !knob::AOCR_WGRAD_ATOMIC()) ? part : nullptr;
    trace_launch("conv_wgrad_tr_kernel", slab ? "slab" : "atomic", Cout, N, P);
    hipLaunchKernelGGL((conv_wgrad_tr_kernel<EpStore>), dim3(gx * gy * ks), dim3(256), 0, s, ah, bh, ep, P, kper, gx, gy, ks, slab, (long long)mn);
    if (slab) splitk_reduce(s, slab, ks, mn, dw);
  } else {
    launch_conv_wgrad(s, bf16, make_loadmn(dy, Cout, Cout, P), b, ep, Cout, N, P, ksplit);
  }
  if (dbias) colsum_accum(s, dy, Cout, P, Cout, dbias);
}

}  // namespace aocr
