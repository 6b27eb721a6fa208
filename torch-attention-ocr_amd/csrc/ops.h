// ops.h -- host-side launchers of every kernel on the hot path (all enqueue on a stream, none synchronise).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "aocr.h"
#include "epilogues.h"
#include "mfma_gemm.h"
#include "knobs.h"

namespace aocr {

inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// ---- helpers to build loaders
inline LoadK make_loadk(const float* p, int64_t ld, int rows, int K) {
  LoadK l; l.p0 = p; l.ld0 = ld; l.K0 = K; l.p1 = nullptr; l.ld1 = 0; l.rows = rows; l.K = K;
  l.vec = (((uintptr_t)p & 15) == 0) && (ld % 4 == 0);
  return l;
}
inline LoadK make_loadk2(const float* p0, int64_t ld0, int K0, const float* p1, int64_t ld1, int K1, int rows) {
  LoadK l; l.p0 = p0; l.ld0 = ld0; l.K0 = K0; l.p1 = p1; l.ld1 = ld1; l.rows = rows; l.K = K0 + K1;
  l.vec = (((uintptr_t)p0 & 15) == 0) && (ld0 % 4 == 0) && (((uintptr_t)p1 & 15) == 0) && (ld1 % 4 == 0) && (K0 % 16 == 0);
  return l;
}
inline LoadMN make_loadmn(const float* p, int64_t ld, int rows, int K) {
  LoadMN l; l.p = p; l.ld = ld; l.rows = rows; l.K = K;
  l.vec = (((uintptr_t)p & 15) == 0) && (ld % 4 == 0);
  return l;
}
inline EpStore make_store(float* C, int64_t ldc, int M, int N, const float* bias = nullptr, const float* bias2 = nullptr,
                          int flags = 0) {
  EpStore e; e.C = C; e.ldc = ldc; e.M = M; e.N = N; e.bias = bias; e.bias2 = bias2; e.flags = flags;
  e.C1 = nullptr; e.ldc1 = 0; e.N0 = N; return e;
}

// ---- MFMA contractions (ops_gemm.hip)
// ksplit > 1 requires ep.flags & EP_ATOMIC.
void launch_big_kk(hipStream_t s, bool bf16, const LoadK& a, const LoadK& b, const EpStore& ep, int M, int N, int K, int ksplit);
void launch_big_kmn(hipStream_t s, bool bf16, const LoadK& a, const LoadMN& b, const EpStore& ep, int M, int N, int K, int ksplit);
void launch_big_mnmn(hipStream_t s, bool bf16, const LoadMN& a, const LoadMN& b, const EpStore& ep, int M, int N, int K, int ksplit);
void launch_conv_fwd(hipStream_t s, bool bf16, const LoadConvK& a, const LoadK& b, const EpConv& ep, int M, int N, int K);
void launch_conv_dgrad(hipStream_t s, bool bf16, const LoadConvK& a, const LoadConvWT& b, const EpStore& ep, int M, int N, int K);
void launch_conv_wgrad(hipStream_t s, bool bf16, const LoadMN& a, const LoadConvXcol& b, const EpStore& ep, int M, int N, int K, int ksplit);

typedef SmallArgs<LoadK, LoadK, EpGatesFwd> GatesFwdArgs;
typedef SmallArgs<LoadK, LoadK, EpStore> SmallKKArgs;
typedef SmallArgs<LoadK, LoadMN, EpStore> SmallKMNArgs;
typedef SmallArgs<LoadK, LoadMN, EpGatesBwd> GatesBwdArgs;
// nz = 1 or 2 argument sets (blockIdx.z); M rows, H (or N) columns.
void launch_small_gates_fwd(hipStream_t s, bool bf16, int nz, const GatesFwdArgs* z, int M, int H);
void launch_small_kk(hipStream_t s, bool bf16, int nz, const SmallKKArgs* z, int M, int N);
void launch_small_kmn(hipStream_t s, bool bf16, int nz, const SmallKMNArgs* z, int M, int N);
void launch_small_gates_bwd(hipStream_t s, bool bf16, int nz, const GatesBwdArgs* z, int M, int H);
typedef SmallArgs<LoadK, LoadK, EpGatesBwd> GatesBwdKKArgs;     // fp32 mode, B = fp32 transposed weights (K-contiguous)
void launch_small_gates_bwd_kk(hipStream_t s, int nz, const GatesBwdKKArgs* z, int M, int H);
// bf16 mode with bf16 weight shadows as the B operand (always K-contiguous: W for y = x W^T, W^T for y = x W)
typedef SmallArgs<LoadK, LoadKh2, EpGatesFwd> GatesFwdArgsH;
typedef SmallArgs<LoadK, LoadKh2, EpStore> SmallArgsH;
typedef SmallArgs<LoadK, LoadKh2, EpGatesBwd> GatesBwdArgsH;
typedef SmallArgs<LoadKh2, LoadKh2, EpGatesFwd> GatesFwdArgsHH;    // A read from its bf16 shadow as well
typedef SmallArgs<LoadKh2, LoadKh2, EpStore> SmallArgsHH;
typedef SmallArgs<LoadKh2, LoadKh2, EpGatesBwd> GatesBwdArgsHH;
void launch_small_gates_fwd_hh(hipStream_t s, int nz, const GatesFwdArgsHH* z, int M, int H);
// recurrent-step products at large batch (>= 320 rows, >= 1024 columns): 128 x 128 LDS-DMA tiles + an elementwise cell pass; false: shape not taken (ops_gemm.hip)
bool big_step_store(hipStream_t s, const LoadKh2& a, const LoadKh2& b, const EpStore& ep, int M, int N);
bool big_step_gates_fwd(hipStream_t s, const LoadKh2& a, const LoadKh2& b, const EpGatesFwd& ep, int M, int H, float* zbuf, size_t zbuf_floats);
void launch_small_hh(hipStream_t s, int nz, const SmallArgsHH* z, int M, int N);
void launch_small_gates_bwd_hh(hipStream_t s, int nz, const GatesBwdArgsHH* z, int M, int H);
void launch_small_gates_fwd_h(hipStream_t s, int nz, const GatesFwdArgsH* z, int M, int H);
void launch_small_h(hipStream_t s, int nz, const SmallArgsH* z, int M, int N);
void launch_small_gates_bwd_h(hipStream_t s, int nz, const GatesBwdArgsH* z, int M, int H);
inline LoadKh2 make_loadkh(const bf16_t* p, int64_t ld, int rows, int K) {
  LoadKh2 l; l.p0 = p; l.ld0 = ld; l.K0 = K; l.p1 = nullptr; l.ld1 = 0; l.rows = rows; l.K = K; return l;
}
inline LoadKh2 make_loadkh2(const bf16_t* p0, int64_t ld0, int K0, const bf16_t* p1, int64_t ld1, int K1, int rows) {
  LoadKh2 l; l.p0 = p0; l.ld0 = ld0; l.K0 = K0; l.p1 = p1; l.ld1 = ld1; l.rows = rows; l.K = K0 + K1; return l;
}
// wb [R][C] = bf16(w[r*ld + c]), wtb [C][R] = its transpose (dense)
void weight_shadows(hipStream_t s, const float* w, int64_t ld, int R, int C, bf16_t* wb, bf16_t* wtb);
void transpose_f32(hipStream_t s, const float* w, int64_t ld, int R, int C, float* wt);                    // wt [C][R]
void conv_weight_transpose_f32(hipStream_t s, const float* w, float* wt, int Cout, int KK, int Cin);     // wt [Cin][KK][Cout]

// generic GEMM used by the C ABI and the hoisted projections; picks ksplit when allowed (atomic accumulate).
// projector + LogSoftMax / ClassNLL + d logits + projector data gradient of all L B rows as one launch (ops_gemm.hip: project_loss_kernel; bf16 mode, V <= 40);
// every output bit-identical to gemm (skinny) + logsoftmax_nll + gemm (K = V)
bool project_loss_ok(int rows, int V, int Hd);
void project_loss(hipStream_t s, const float* out, int64_t ldo, const float* wo, const float* bo, float* logits, float* dlogits, int64_t ld, float* nll, float* dout,
                  const int32_t* tgt, int64_t st, int64_t sb, int Bt, int rows, int V, int Hd, float scale);
int gemm(hipStream_t s, bool bf16, const float* A, int64_t lda, bool a_kmajor, const float* B, int64_t ldb, bool b_kmajor,
          float* C, int64_t ldc, int M, int N, int K, const float* bias, const float* bias2, int flags);

// Grouped weight-gradient contractions C_i[M_i,N_i] += A_i^T B_i (A_i [K_i][M_i], B_i [K_i][N_i], all M/N-contiguous fp32):
// one launch for up to 8 problems; K is split only as far as needed to fill the chip once.
struct WGradProblem { const float* A; int64_t lda; const float* B; int64_t ldb; float* C; int64_t ldc; int M, N, K;
                      const bf16_t* Ab = nullptr; const bf16_t* Bb = nullptr; };     // optional bf16 shadows of A and B (same lda/ldb)
void grouped_wgrad(hipStream_t s, bool bf16, const WGradProblem* p, int n, float* part = nullptr, size_t part_floats = 0);     // part: split-K slab scratch (enables the LDS-DMA kernel for deep problems)
void kprobe_read(unsigned long long out[8]);   // debugging probe of the tagged halo kernels (mfma_gemm.h: g_kprobe)

// C = A B^T (+bias) with both operands read from K-contiguous bf16 shadows (A [M][K], B [N][K])
bool gemm_hh_cat(hipStream_t s, const bf16_t* A0, const bf16_t* A1, int64_t lda, const bf16_t* B0, const bf16_t* B1, int64_t ldb, float* C, int64_t ldc, int M, int N, int K0, int K1);   // C = [A0 | A1] . [B0 | B1]^T, one launch; false: shape not taken
void gemm_hh(hipStream_t s, const bf16_t* A, int64_t lda, const bf16_t* B, int64_t ldb, float* C, int64_t ldc, int M, int N, int K,
             const float* bias, const float* bias2, int flags);
// the same with a bf16 copy of C written beside it (plain stores)
void gemm_hh_shadow(hipStream_t s, const bf16_t* A, int64_t lda, const bf16_t* B, int64_t ldb, float* C, int64_t ldc, bf16_t* Cb, int64_t ldcb,
                    int M, int N, int K);

// ---- convolution layers (ops_gemm.hip)
// xb/wb/dyb/wtb: optional bf16 shadows of the operands (both of a contraction's operands must be given to take the
// bf16-source path); yb: optional bf16 shadow of the output to write.
void conv_forward(hipStream_t s, bool bf16, const float* x, const float* w, const float* bias, float* y, uint8_t* idx,
                  int B, int H, int W, int Cin, int Cout, int ks, int pad, int relu, int pool,
                  const bf16_t* xb = nullptr, const bf16_t* wb = nullptr, bf16_t* yb = nullptr, int profile_tag = 0,
                  const float* bn_save = nullptr, const float* bn_w = nullptr, const float* bn_b = nullptr,
                  double* bn_part = nullptr, int* bn_chunks = nullptr, int* y_bf16 = nullptr);
// bn_part / bn_chunks: scratch of the training-mode BatchNorm that follows (bn_relu_forward's `scratch`); when the launch taken stages its output tiles through
// LDS the per-tile column sums are written there and *bn_chunks = the number of row tiles (pass it to bn_relu_forward as stats_chunks), else *bn_chunks = 0.
// y_bf16 (with them): the caller accepts y written as bf16 INTO THE SAME BUFFER (half of it); *y_bf16 = 1 when that happened (only under AOCR_BN_Y16=1: see conv_forward)
// bn_save != nullptr: evaluation-mode BatchNorm + ReLU folded into the conv epilogue (bn_save from bn_eval_prepare)
void bn_eval_prepare(hipStream_t s, const float* rm, const float* rv, float* save, int C);
// profile_tag != 0: the same kernel under a distinct symbol (aocr_profile_kernel), so profilers list these launches separately
struct BnBwdFuse { const float* x; const bf16_t* yb; const float* save; double* part; };   // pre-BatchNorm map (fp32), post-ReLU bf16 shadow (mask), {mean, invstd}, bn_relu_backward's scratch
void conv_backward_data(hipStream_t s, bool bf16, const float* dy, const float* w, float* dx, int B, int H, int W, int Cin,
                        int Cout, int ks, int pad, const bf16_t* dyb = nullptr, const bf16_t* wtb = nullptr, const float* wtf = nullptr,
                        int* dx16 = nullptr /* the caller accepts dx written as bf16 into the first half of the same buffer; *dx16 = 1 when that happened */,
                        const struct BnBwdFuse* bnb = nullptr, int* bnb_chunks = nullptr /* the BatchNorm backward behind this data gradient: its partial sums from the conv epilogue; *bnb_chunks = row tiles written (pass to bn_relu_backward as sums_chunks), 0 = not taken */);
// what conv_backward_data puts in *dx16 for this shape in bf16 mode (shadows supplied, dx16 accepted) under the switches as they are now: aocr_profile_kernel asks the launcher's own predicate
bool conv_dgrad_bf16_out(int B, int H, int W, int Cin, int Cout, int ks, int pad);
void conv_backward_filter(hipStream_t s, bool bf16, const float* x, const float* dy, float* dw, float* dbias, int B, int H,
                          int W, int Cin, int Cout, int ks, int pad, const bf16_t* xb = nullptr, const bf16_t* dyb = nullptr,
                          float* part = nullptr, size_t part_floats = 0, int profile_tag = 0);   // part: scratch for the split-K slabs (else fp32 atomics)
void splitk_reduce(hipStream_t s, const float* part, int ks, size_t n, float* out);   // out[i] += sum_z part[z * n + i]  (n % 4 == 0)

// ---- everything that is not a contraction (ops_misc.hip)
// route (conv1_route_elems() uint16): the pooling/ReLU decision of every window, four 4-bit codes per word, for conv1_backward
void conv1_forward(hipStream_t s, const float* x, const float* w, const float* bias, float* y, int B, int H, int W,
                   bf16_t* yb = nullptr, uint16_t* route = nullptr);
size_t conv1_route_elems(int B, int H, int W);
void conv_weight_shadows(hipStream_t s, const float* w, bf16_t* wb, bf16_t* wtb, int Cout, int KK, int Cin);
struct ColsumJobs;
void conv1_backward(hipStream_t s, const float* x, const float* w, const float* bias, const float* dyp, float* dw, float* db,
                    int B, int H, int W, float* scratch = nullptr, ColsumJobs* defer = nullptr,
                    const uint16_t* route = nullptr /* conv1_forward's decisions for the SAME x, w, bias; null: re-evaluated here */);
// scratch (min(ceil(strips / 4), 2048) * 640 floats, strips = B * (H/2) * ceil((W/2) / 32)): one partial row per workgroup, finished by two column sums (else fp32 atomics)
void unpool_relu_backward(hipStream_t s, const float* dpooled, const float* pooled, const uint8_t* idx, float* dy, int B,
                          int Ho, int Wo, int C, int pool, bf16_t* dyb = nullptr, float* dbias = nullptr,
                          float* partial = nullptr, const bf16_t* pooledb = nullptr, ColsumJobs* defer = nullptr,
                          const bf16_t* dpooled16 = nullptr /* d(pooled) as bf16 instead of fp32 (bf16-mode 8-channel kernel only: conv_backward_data's dx16) */);
// defer: the column sum that finishes a partial slab is queued (colsum_flush) instead of launched -- the slab must then stay untouched until the flush
// dbias + partial (>= 2048*C floats scratch; min(ceil(windows*C/4 / 256), 2048) * C are written) + dyb: fused bias gradient where 256 % (C/4) == 0, dy may then be null
// (any other C: dy is required and dbias is left untouched); pooledb: bf16 shadow of pooled (mask source)
void bf16_to_f32(hipStream_t s, const bf16_t* src, float* dst, int64_t n);
size_t bn_scratch_bytes(int C);
// synchronised BatchNorm: sums `count` elements (dtype 1 = fp64) of a device buffer over the data-parallel ranks, on stream s
struct BnSync { int (*allreduce)(void* ctx, void* buf, int64_t count, int dtype, hipStream_t s); void* ctx; };
void bn_relu_forward(hipStream_t s, const float* x, float* y, const float* w, const float* b, float* rm, float* rv,
                     float* save, void* scratch, int64_t rows, int C, int training, int update_running, int tb_rows,
                     bf16_t* yb = nullptr, const BnSync* sync = nullptr, int stats_chunks = 0 /* > 0: scratch already holds that many chunks of partial sums (conv_forward's bn_part) */,
                     const bf16_t* xh = nullptr /* x as bf16 (conv_forward wrote it so: *y_bf16), read instead of x by the statistics and the apply pass */);
// xh (forward and backward) and dAh: where the launcher computes the sums itself (stats_chunks / sums_chunks == 0, training) they are legal only where the
// 16-byte partial-sum kernel runs -- C / 4 a power of two <= 256 and AOCR_BN_PARTIAL_OLD unset (the generic partial-sum kernel reads fp32 only); with the
// sums handed over, and in evaluation mode, only the apply kernels read them, for any C % 4 == 0
void bn_relu_backward(hipStream_t s, const float* x, const float* y, const float* dA, const float* w, const float* save,
                      float* dx, float* dw, float* db, void* scratch, int64_t rows, int C, int tb_rows, bf16_t* dxb = nullptr,
                      const bf16_t* yb = nullptr, float* conv_dbias = nullptr, float* partial = nullptr, const BnSync* sync = nullptr,
                      ColsumJobs* defer = nullptr, const bf16_t* xh = nullptr /* x as bf16 */,
                      const bf16_t* dAh = nullptr /* d A as bf16 instead of fp32 (bn_partial4 path only) */,
                      int sums_chunks = 0 /* > 0: scratch already holds that many chunks of (sum d, sum d xhat) (conv_backward_data's bnb_chunks) */);
// yb: bf16 shadow of y (ReLU mask source); conv_dbias + partial (min(ceil(rows*C/4 / 256), 2048) * 1024 floats) + dxb: fused bias gradient of the preceding conv
// where 256 % (C/4) == 0, dx may then be null (any other C: dx is required and conv_dbias is left untouched)
// ctx_div: rows r share context row r / ctx_div (beam search keeps one context per image, model.lua:373)
void attention_forward(hipStream_t s, const float* ctx, const float* q, float* a, float* c, int64_t ldc, int B, int T, int Hd,
                       int ctx_div = 1, bf16_t* cb = nullptr, int64_t ldcb = 0, const bf16_t* ctxb = nullptr);
void gates_elem_bwd(hipStream_t s, const EpGatesBwd& ep, int M, int H);       // LSTM cell backward without a product (ops_gemm.hip)
bool attention_dual_ok(int T, int Hd, const bf16_t* ctxb, const bf16_t* ctxab);     // scores against the pre-multiplied context (round 6, ops_misc.hip: attn_bf16_kernel<..., DUAL>)
void attention_forward_dual(hipStream_t s, const float* h_top, int64_t ldh, float* a, float* c, int64_t ldc, int B, int T, int ctx_div, bf16_t* cb, int64_t ldcb,
                            const bf16_t* ctxb, const bf16_t* ctxab);
void attention_backward_dual(hipStream_t s, const float* a, const float* dc, int64_t lddc, float* ds, float* dq, bf16_t* dqb, float* dh_attn, int B, int T,
                             const bf16_t* ctxb, const bf16_t* ctxab);
void attention_backward(hipStream_t s, const float* ctx, const float* q, const float* a, const float* dc, int64_t lddc,
                        float* ds, float* dq, int B, int T, int Hd, bf16_t* dqb = nullptr, const bf16_t* ctxb = nullptr,
                        const float* cfwd = nullptr, int64_t ldcf = 0);      // cfwd (optional): the forward pass's weighted context of the same rows -- the streamed kernel then makes ONE pass (ops_misc.hip)
// ctxb: bf16 shadow of ctx, read instead of ctx by the register-resident kernels (T <= 64, Hd in {256, 512})
// d(ctx)[b,t,:] = sum_l a[l,b,t]*dc[l,b,:] + ds[l,b,t]*q[l,b,:]   (dc row stride lddc)
void attention_dctx(hipStream_t s, const float* a_all, const float* ds_all, const float* dc_all, int64_t lddc,
                    const float* q_all, float* dctx, int L, int B, int T, int Hd);
void logsoftmax_nll(hipStream_t s, const float* logits, int64_t ld, const int32_t* tgt, int64_t tgt_stride_t,
                    int64_t tgt_stride_b, int Bt, float* logp, float* dlogits, float* nll_rows, int64_t rows, int V,
                    float grad_scale);
void sum_to_scalar(hipStream_t s, const float* x, int64_t n, float* out);                 // out[0] = sum x
void gold_scores(hipStream_t s, const float* nll_rows, float* gold, int L, int B);       // gold[b] = -sum_t nll[t,b]
struct ZeroList { void* p[16]; size_t bytes[16]; int n = 0;
  void add(void* q, size_t b) { if (q && b && n < 16) { p[n] = q; bytes[n] = b; ++n; } } };
void zero_many(hipStream_t s, const ZeroList& z);    // all listed regions (16-byte aligned) in one launch
void colsum_accum(hipStream_t s, const float* A, int64_t ld, int64_t rows, int N, float* out, float* out2 = nullptr);   // out[n] (and out2[n]) += sum_r A[r][n]
// deferred form: up to 8 column sums finished by ONE launch (each small sum is otherwise its own ~10 us dispatch on the step's critical path)
struct ColsumJob { const float* A; int64_t ld, rows; int N; float* out; float* out2; int first, nb, chunks; };
struct ColsumJobs { int n, total; ColsumJob j[8]; };
void colsum_defer(ColsumJobs& g, const float* A, int64_t ld, int64_t rows, int N, float* out, float* out2 = nullptr);
void colsum_flush(hipStream_t s, ColsumJobs& g);
void embedding_gather(hipStream_t s, const float* table, const int32_t* tok, int64_t stride_t, int64_t stride_b, float* out,
                      int L, int B, int E);
// S [V][ncols] = rows of dz summed by their token (zeroed here; index: segsum_index_ints(rows, V) ints of scratch); then db1 / db2 += the column
// totals, dlookup [V][E] += S W[:, :E] (W [ncols][ldw]) and dW [ncols][ldw] (first E columns) += S^T lookup
bool segsum_supported(int ncols, int V, int E);
size_t segsum_index_ints(int rows, int V);
void segsum_by_token(hipStream_t s, const float* dz, int64_t ld, const int32_t* tok, int64_t st, int64_t sb, int L, int B, int ncols, int V, float* S, int* index,
                     float* db1, float* db2, const float* W, int64_t ldw, const float* lookup, int E, float* dlookup, float* dW);
void embedding_scatter_accum(hipStream_t s, const float* demb, const int32_t* tok, int64_t stride_t, int64_t stride_b,
                             float* dtable, int L, int B, int E, int V);
void dpre_tanh(hipStream_t s, const float* g1, const float* g2, const float* out, float* dpre, int64_t n, bf16_t* dpreb = nullptr, const DropSpec* drop = nullptr);
void pointwise(hipStream_t s, int op, const float* a, const float* b, float* y, int64_t n);   // AOCR_PW_* of include/aocr.h
void u8_to_f32(hipStream_t s, const uint8_t* src, float* dst, int64_t n);
void dropout_apply(hipStream_t s, const float* src, float* dst, bf16_t* dstb, int64_t n, const DropSpec& drop);
void dropout_apply_b(hipStream_t s, const bf16_t* src, float* dst, bf16_t* dstb, int64_t n, const DropSpec& drop);  // (g1+g2)*(1-out^2)
void copy2d_bf16(hipStream_t s, const float* src, int64_t lds, bf16_t* dst, int64_t ldd, int rows, int cols);
void copy2d(hipStream_t s, const float* src, int64_t lds, float* dst, int64_t ldd, int rows, int cols);
void copy2d_pair(hipStream_t s, const float* s0, const float* s1, int64_t lds, float* d0, float* d1, int64_t ldd, int rows, int cols);
struct DecInitArgs { float* c0[4]; float* h0[4]; bf16_t* hb[4]; float* feed0; bf16_t* outb; const float *cfw, *cbw, *hfw, *hbw; int B, He, Hd, Ld, copy_h; };
void dec_init(hipStream_t s, const DecInitArgs& a);              // the decoder's initial state in one launch (ops_misc.hip)
void sgd_clip_update(hipStream_t s, float* params, float* grads, const int64_t* group_off /*6 host values*/, float lr,
                     float clip, float* norms_out, void* scratch, int* err = nullptr,
                     float* bn_state = nullptr, const float* bn_snap = nullptr, int bn_n = 0);   // err = the time-out word block (cl_err): err[0] != 0: no update, bn_state <- bn_snap (the step's move of the running statistics is taken back), and the code moves to err[CL_ERR_STICKY]
constexpr int CL_ERR_LATCH = 12, CL_ERR_STICKY = 13;              // words of the cl_err block (0: step in flight, 1..4 encoder diagnostics, 8..11 exchange scratch, 16..: trash slots)
void step_snapshot(hipStream_t s, const float* bn_state, float* bn_snap, int n, int* err);        // start of a training step (ops_misc.hip)
size_t sgd_scratch_bytes();
void adadelta_update(hipStream_t s, float* params, float* grads, float* var, float* acc, int64_t n, float rho, float eps, float wd, int* err = nullptr,
                     float* bn_state = nullptr, const float* bn_snap = nullptr, int bn_n = 0);
// AdamW on the flat vector (optim.hip; the arithmetic: include/aocr.h, aocr_adam_update).  state: {m | v | 32-byte tail}; skip: nullptr or one device word,
// non-zero = write nothing but norms_out (nullptr or 15 floats); scratch: adam_scratch_bytes().  grads is read only.
struct AdamHyper { float lr, beta1, beta2, eps, wd, clip; };
size_t adam_scratch_bytes();
void adam_update(hipStream_t s, float* params, const float* grads, void* state, const int64_t* group_off /*6 host values*/, const AdamHyper& h,
                 const int* skip, void* scratch, float* norms_out);
// the time-out half of an optimizer call whose update lives outside ops_misc.hip: the latch of the code (cl_err_latch) and, on a latched code, the restore of
// the BatchNorm running statistics -- the code sgd_update_kernel / adadelta_kernel run, not a copy of it (ops_misc.hip).  The update then reads err[CL_ERR_LATCH].
void optim_latch_restore(hipStream_t s, int* err, float* bn_state, const float* bn_snap, int bn_n);
// one 2-D piece of the per-step bf16 weight shadow refresh (shadow_jobs_kernel); tile0 = first 32x32 tile of the piece, tx = tiles per row
struct ShadowJob { const float* w; bf16_t* wb; bf16_t* wtb; int64_t ld, ldb, ldt; int R, C, tile0, tx; };
void shadow_jobs(hipStream_t s, const ShadowJob* jobs_dev, int njobs, int total_tiles, int tile_off = 0);      // tiles [tile_off, tile_off + total_tiles) of the table
// flat dictionary trie + the per-beam node ids of one decode step (mask == nullptr: unconstrained); needs V <= 64
struct TrieView { const unsigned long long* mask; const int32_t* base; const int32_t* child; const int32_t* loc_in; int32_t* loc_out; };
// sc_out (optional, recognition): a second copy of the kout new running scores, [B][kout] (the score history of aocr_recognize)
void beam_select(hipStream_t s, const float* logp, const int32_t* prev_tok, float* beam_scores, int32_t* tokens,
                 int32_t* parents, int B, int kin, int kout, int V, const float* logits = nullptr, int64_t ldl = 0,
                 const TrieView* tv = nullptr, float* sc_out = nullptr);
// logits != nullptr (and V <= 64): raw projector outputs, the LogSoftMax is applied inside (logp is then unused)
// projector + LogSoftMax + beam bookkeeping of one decode step in one launch (V <= 64, Hd % 4 == 0)
void project_select(hipStream_t s, const float* h, int64_t ldh, const float* wo, const float* bo, int Hd, const int32_t* prev_tok,
                    float* beam_scores, int32_t* tokens, int32_t* parents, int B, int kin, int kout, int V,
                    const TrieView* tv = nullptr, float* sc_out = nullptr);
void token_rows(hipStream_t s, const float* table, const int32_t* tok, int64_t stride, float* dst, int R, int width);   // dst[r] = table[tok[r*stride]-1]
// dst[b*kout+i][:] = src[(kin==1 ? b : b*kin + parents[b*kout+i])][:]
void gather_beam_rows_many(hipStream_t s, int n, const float* const* src, float* const* dst, int64_t ld, const int32_t* parents, int B, int kin, int kout, int width,
                           bf16_t* const* dstb = nullptr);      // dstb[i] (optional): bf16 copy of gathered tensor i
void gather_beam_rows(hipStream_t s, const float* src, int64_t lds, float* dst, int64_t ldd, const int32_t* parents, int B,
                      int kin, int kout, int width);
void beam_backtrace(hipStream_t s, const int32_t* hist_tok, const int32_t* hist_par, const float* beam_scores,
                    int32_t* labels, float* scores, int Lt, int B, int k);
// aocr_recognize's optional outputs from the search history: the winning hypothesis of each image (backtrace_kernel's rule; k = 1 / hist_par ==
// nullptr: greedy), walked back through hist_par [Lt][B][k]; char_logp [B][Lt] = score differences of sc_hist [Lt][B][k], attn [B][Lt][T] = its
// rows of attn_hist [Lt][B k][T] (row b kin + parent, kin = 1 at step 0).  Steps after the first EOS / PAD of labels are 0.  Either output may be nullptr.
void recognize_gather(hipStream_t s, const int32_t* labels, const int32_t* hist_par, const float* beam_scores, const float* sc_hist,
                      const float* attn_hist, float* char_logp, float* attn, int Lt, int B, int k, int T);
void fill_i32(hipStream_t s, int32_t* p, int32_t v, int64_t n);
// Levenshtein distance between two id rows cut at the first EOS (utils.lua:55-94 over the strings of utils.lua:136-168)
void edit_distance(hipStream_t s, const int32_t* labels, const int32_t* targets, int B, int L, int32_t* dist, int32_t* target_len);
// ---- lexicon snapping (lexicon.hip; include/aocr.h: aocr_lexicon_nearest): per label row cut at its first EOS, the word of
// words [n_words][stride] (ids 1..255, zero filled) in [row_begin[b], row_begin[b+1]) (nullptr: the whole list) at the smallest
// Levenshtein distance, lowest index on ties.  lexicon_slices: workgroups per row; scratch holds B * slices 64-bit keys when slices > 1.
int lexicon_slices(int n_words);
void lexicon_nearest(hipStream_t s, const int32_t* labels, int B, int L, const uint8_t* words, int n_words, int stride,
                     const int32_t* row_begin, void* scratch, int32_t* index, int32_t* dist);

// ---- whole-sequence encoder recurrence (rnn_seq.hip): one workgroup owns 16 batch rows of one direction for all T steps
struct EncSeqDir {
  const bf16_t* w;         // recurrent weight, bf16 [4He][He]
  const float* zx;         // pre-computed input part incl. both biases, fp32 [T][B][4He]
  float* hs; float* cs;    // state slots [(T+2)][B][He]: slot t+1 holds step t
  bf16_t* hsb;             // bf16 shadow of hs
  float* gates;            // saved post-activation gates [T][B][4He]
  float* ctx;              // context + dir*He (element (b,t,j) at ctx[(b*T + t)*Hd + j]) or nullptr below the top layer
  int reverse;             // 1: the direction that walks t = T-1 .. 0
};
struct EncSeqFwdArgs { EncSeqDir d[2]; int B, T, He, Hd; int abl = 0; unsigned long long* dbg = nullptr; };
struct EncSeqBwdDir {
  const bf16_t* wt;        // transposed recurrent weight, bf16 [He][4He]
  const float* dh1;        // d h(t) from above: element (row, t, j) at dh1[row*dh1_row + t*dh1_t + j]
  int64_t dh1_row, dh1_t;
  const float* dh2;        // extra d h for the FIRST processed step (decoder initial state), row stride dh2_row; or nullptr
  int64_t dh2_row;
  float* dc;               // [B][He]: in = d c entering the first processed step, out = d c leaving the last one
  const float* dc_in = nullptr; int64_t dc_in_row = 0;   // cluster kernels, first chunk: d c entering the first step read from here (row stride dc_in_row) instead of dc -- the decoder's [B][2 He] initial-state gradient without a split copy
  const float* gates;      // saved gates [T][B][4He]
  const float* cs;         // cell-state slots [(T+2)][B][He]
  float* dz; bf16_t* dzb;  // out: d z [T][B][4He], fp32 and bf16
  float* dbi = nullptr; float* dbh = nullptr;   // cluster kernels only: both bias gradients (+= sum of d z over rows and steps; no fp32 d z is written)
  int forward_dir;         // 1: the direction whose forward pass walked t = 0..T-1 (its BPTT walks T-1..0, c_prev = slot t)
};
struct EncSeqBwdArgs { EncSeqBwdDir d[2]; int B, T, He; };
bool enc_seq_supported(int B, int He, int blocks_limit);
// ---- the same recurrences on clusters of CUs with register-resident weights (rnn_cluster.hip)
struct EncClFwdArgs { EncSeqDir d[2]; int B, T, He, Hd, groups; unsigned epoch; unsigned long long* xbuf; int* err; int gid0 = 0, ngid = 0; unsigned long long* xtab = nullptr; int force_remote = 0; int it0 = 0, it1 = 0 /* iterations [it0, it1) of the T in this launch; it1 = 0: all */, gslot = 0 /* group-slot offset into xbuf / xtab (one set of slots per layer) */; int rh = 16 /* batch rows per 16-column tile: 16, or 8 (half tiles; set by enc_cluster_forward) */; };
struct EncClBwdArgs { EncSeqBwdDir d[2]; int B, T, He, groups; unsigned epoch; unsigned long long* pbuf; int* err; int gid0 = 0, ngid = 0; unsigned long long* xtab = nullptr; int force_remote = 0; int it0 = 0, it1 = 0, gslot = 0; int rh = 16 /* as EncClFwdArgs::rh; set by enc_cluster_backward */; };
bool enc_cluster_plan(int B, int He, int T, int cus, int& G, int& RT, int& groups);
size_t enc_cluster_xbuf_bytes(int B, int He);
size_t enc_cluster_pbuf_bytes(int B, int He);
void enc_cluster_forward(hipStream_t s, const EncClFwdArgs& a, int G, int RT, int reserve_cus = 0, int concurrent = 1);      // concurrent: launches of this size that run side by side (layer wavefront): half tiles only if they all fit
void enc_cluster_backward(hipStream_t s, const EncClBwdArgs& a, int G, int RT, int reserve_cus = 0, int concurrent = 1);
// teacher-forced decoder loop in one launch (dec_cluster.hip): Hd = 512, two layers, input feed, bf16 mode
struct DecClFwdArgs {
  int B, T, L; unsigned epoch; int group0 = 0, ngroups = 0, force_remote = 0; int no_early = 0;   /* greedy decode: do not leave the loop when every row of a group has finished (debugging aid) */
  const bf16_t *w1i, *w1h, *w2i, *w2h, *wc;           // bf16 shadows: [4 Hd][Hd] x 4, W_c [Hd][2 Hd]
  const float *b2i, *b2h;                              // layer-2 biases (layer 1's are inside zx1)
  const float* zx1;                                    // [L][B][4 Hd]: embedding part of layer 1 + both biases
  const bf16_t *ctxb, *ctxa;                           // [B][T][Hd]: encoder context and context . W_a
  float* cs[2]; bf16_t* hsb[2];                        // [L + 1][B][Hd], slot 0 = initial state (the fp32 h is not written: every reader takes the bf16 copy)
  float* gates[2];                                     // [L][B][Hd][4] post-activation (i, f, o, g INTERLEAVED per unit), or nullptr
  float *a_all, *out; bf16_t *cat_b, *out_b;           // [c ; h_top] only as its bf16 copy
  unsigned long long *xbuf, *xtab; int* err; unsigned long long* stamps = nullptr;
  // greedy decode (the kernel's DEC variant): zx1 is the per-token table [V][4 Hd]; tok0 = the GO tokens (row stride tok0_stride = the label width)
  const int32_t* tok0 = nullptr; int tok0_stride = 0; const float *wo = nullptr, *bo = nullptr; int V = 0;
  float* pbuf = nullptr; unsigned* tokx = nullptr; int32_t* labels = nullptr; float* scores = nullptr; int pgroups = 0;   /* dec_chain.hip: groups of the whole batch (the partial logits are kept per step parity) */
  const unsigned long long* trie_mask = nullptr; const int32_t* trie_base = nullptr; const int32_t* trie_child = nullptr;   // -use_dictionary (flat trie of include/aocr.h) or null
  // beam search on the chain kernel (dec_chain.hip, BEAM variant): k hypotheses per image, history [L][B][k] + final scores [B][k] for beam_backtrace
  int beam = 0, rows_slot = 0; int32_t *hist_tok = nullptr, *hist_par = nullptr; float* beam_scores = nullptr;
  // nn.Dropout(p) (training, LSTM.lua:68-69,116-118): masks of layer 2's input (site 2) and of the attention output (site 16), flat index
  // = step * B * Hd + row * Hd + unit added to .off = 0; hm_b [L][B][Hd]: the masked bf16 copy of h1 (operand of layer 2 and of its weight gradient)
  DropSpec drop_h, drop_out; bf16_t* hm_b = nullptr;
  // round 4, teacher-forced loop: zx1 as the per-token table [V][4 Hd] too (zx_tok = the input tokens, token of (step t, row b) = zx_tok[t zx_st + b zx_sb]):
  // no (L B, 4 Hd) gate-input tensor is written or read; V must be set
  const int32_t* zx_tok = nullptr; int64_t zx_st = 0, zx_sb = 0;
  // label-free recognition (aocr_recognize; the kernels' HIST variants only): cumulative score of every hypothesis after every step, [L][B][k]
  // (greedy: [L][B]); the attention rows go to a_all, [L][B k][T] with row image * kin + hypothesis (kin = 1 at step 0)
  float* sc_hist = nullptr;
};
// decoder BPTT in one launch (dec_cluster.hip); reads what the forward cluster kernel saved (interleaved gates)
struct DecClBwdArgs {
  int B, T, L; unsigned epoch; int group0 = 0, ngroups = 0, force_remote = 0;
  const bf16_t *w2i_t, *w2h_t, *w1h_t, *w1f_t;          // transposed bf16 shadows [Hd][4 Hd]: W2_i2h, W2_h2h, W1_h2h, W1_i2h[:, E:]
  const bf16_t *wc_t, *wa_t;                           // [2 Hd][Hd], [Hd][Hd]
  const float *dout_proj, *out;                        // [L][B][Hd] projector gradient; [L + 1][B][Hd] attention outputs
  const float* a_all; const bf16_t* ctxb;              // [L][B][T]; [B][T][Hd]
  const float* cs[2]; const float* gates[2];           // [L + 1][B][Hd]; [L][B][Hd][4] (interleaved)
  float* dpre; bf16_t* dpre_b;                         // [L][B][Hd]
  float* dcat;                                         // [L][B][2 Hd]: only the c half is written
  float* ds_all; float* dq; bf16_t* dq_b;              // [L][B][T]; [L][B][Hd]
  float* dz[2]; bf16_t* dzb[2];                        // [L][B][4 Hd]
  float* dc_st[2]; float* dh_rec[2]; float* dfeed;     // [B][Hd]: gradients of the initial state
  unsigned long long *xbuf, *xtab; int* err; unsigned long long* stamps = nullptr;
  DropSpec drop_h, drop_out;                           // as in DecClFwdArgs (the forward kernel stored the MASKED attention output)
};
// beam search (2 <= beam <= 8, V <= 40) as launches of dec_chain.hip's kernel: a.epoch = the first of dec_chain_beam_passes() consecutive epochs,
// a.pbuf / a.xtab sized for dec_chain_beam_group_cap() groups; four rolling step slots inside the [L + 1][B][Hd] buffers bound the groups of a launch (..._supported: at least one fits)
bool dec_chain_beam_supported(int B, int L, int beam, int V);
int dec_chain_beam_passes(int B, int L, int beam);
int dec_chain_beam_group_cap();
void dec_chain_beam_forward(hipStream_t s, const DecClFwdArgs& a);
bool dec_cluster_supported(int Hd, int Ld, int input_feed, int T, int L, int cus);
bool dec_cluster_bwd_supported(int Hd, int Ld, int input_feed, int T, int L, int cus);
size_t dec_cluster_bwd_xbuf_bytes(int B);
void dec_cluster_backward(hipStream_t s, const DecClBwdArgs& a);
size_t dec_cluster_xbuf_bytes(int B);
size_t dec_cluster_xtab_bytes(int B);
void dec_cluster_forward(hipStream_t s, const DecClFwdArgs& a, bool greedy_decode = false);
size_t dec_cluster_pbuf_bytes(int B);
void enc_seq_backward(hipStream_t s, const EncSeqBwdArgs& a);
void enc_seq_forward(hipStream_t s, const EncSeqFwdArgs& a);
// data path (data.hip): 255*rgb2y + image.scale to (out_h, out_w) for n images sharing out_w
void preprocess_lines(hipStream_t s, const uint8_t* src, const aocr_image_desc* desc, int n_images, int out_h, int out_w, float* out);
// training augmentation (data.hip): affine warp + gain / offset + counter-based noise of n (1,H,W) images, in != out
void augment_lines(hipStream_t s, const float* in, const aocr_warp* warp, int n_images, int H, int W, uint64_t seed, uint64_t counter,
                   float* out);
// scan degradation (degrade.hip; include/aocr.h: aocr_degrade_lines): elastic displacement, stroke weight and blur of n (1,H,W) images in one
// launch, in != out
void degrade_lines(hipStream_t s, const float* in, const aocr_degrade* rec, int n_images, int H, int W, uint64_t seed, uint64_t counter,
                   float* out);
// synthetic word lines (synth.hip; include/aocr.h: aocr_synth_lines): lexicon rows drawn from a glyph atlas into n (1,H,W) crops, and
// their targets / targets_eval rows (n, L) unless both are nullptr
void synth_lines(hipStream_t s, const aocr_lexicon& lex, const aocr_glyph_atlas& atlas, const aocr_synth_style* style, int n_images, int H,
                 int W, int L, float* out, int32_t* targets, int32_t* targets_eval);
// page segmentation (segment.hip; include/aocr.h: aocr_segment_page): word boxes of a pitched gray page by projection profiles
size_t segment_scratch_bytes(int H, int W, int max_boxes);
void segment_page(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_segment_params& p, void* scratch, int max_boxes,
                  aocr_box* boxes, int32_t* counts);
// the same with one word gap per band, estimated from the band's own gaps (include/aocr.h: aocr_segment_page_spaced); the scratch is
// segment_scratch_bytes; spacing_rows: max_lines rows of 8 words, or nullptr
void segment_page_spaced(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_segment_params& p,
                         const aocr_spacing_params& spacing, void* scratch, int max_boxes, aocr_box* boxes, int32_t* counts, int max_lines,
                         int32_t* spacing_rows);
// steps 1-2 of aocr_segment_page with Otsu (segment.hip): memset + histogram + Otsu; hist: 256 words, hdr[0] receives the threshold (-1: none)
void otsu_threshold(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, uint32_t* hist, int32_t* hdr);
// page deskew (skew.hip; include/aocr.h: aocr_estimate_skew, aocr_deskew_page): the sheared-profile sweep and the shear that removes the skew
size_t skew_scratch_bytes(int H, int W, int n_steps);
void estimate_skew(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_skew_params& p, void* scratch, int32_t* skew,
                   uint64_t* scores);
void deskew_page(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const int32_t* skew, int slope_q16, int fill, uint8_t* out,
                 int64_t out_pitch);
// the strip profiles of aocr_estimate_skew (skew.hip's strips_kernel, one launch): R[b * strip_rows(H) + y] = ink pixels of row y inside the
// 32-column strip b, uint8, for b < ceil(W / 32) and y < H; the other bytes of a strip's strip_rows(H) are not all written.  fixed >= 0 is
// the threshold, else hdr[0] is read on the device (otsu_threshold's; -1: nothing is ink)
int strip_rows(int H);
void strip_profiles(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, int light, int fixed, const int32_t* hdr, uint8_t* R);
// page dewarp (curl.hip; include/aocr.h: aocr_estimate_curl, aocr_dewarp_page): the row shift of every column group against the middle one
// from correlations of neighbouring groups' profiles, and the column-wise resample that takes the shifts out
int curl_groups(int W, int group);             // ng
size_t curl_scratch_bytes(int H, int W, int group, int max_shift);
void estimate_curl(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_curl_params& p, void* scratch, int32_t* curl,
                   int32_t* shifts, uint64_t* scores);
void dewarp_page(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, int group, const int32_t* shifts, int fill, uint8_t* out,
                 int64_t out_pitch);
// colour pages (colour.hip; include/aocr.h: aocr_estimate_page_colour, aocr_gray_page): the paper colour from three channel histograms, and the
// balanced gray page with the coloured pixels of chosen hue classes replaced by paper
size_t colour_scratch_bytes();
void estimate_page_colour(hipStream_t s, const uint8_t* rgb, int64_t pitch, int H, int W, const aocr_colour_params& p, void* scratch,
                          int32_t* colour);
void gray_page(hipStream_t s, const uint8_t* rgb, int64_t pitch, int H, int W, const aocr_colour_params& p, const int32_t* colour_in,
               int32_t* colour_out, uint8_t* out, int64_t out_pitch);
// page background flattening (flatten.hip; include/aocr.h: aocr_flatten_page): windowed max, windowed mean, division, on a pitched gray page
size_t flatten_scratch_bytes(int H, int W);
void flatten_page(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_flatten_params& p, void* scratch, uint8_t* out,
                  int64_t out_pitch);
// local adaptive binarisation (binarize.hip; include/aocr.h: aocr_binarize_page): a Sauvola threshold from the window sums of v and v^2, one
// fused launch; counts may be nullptr; the scratch is not used
size_t binarize_scratch_bytes(int H, int W, int radius);
void binarize_page(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_binarize_params& p, uint8_t* out, int64_t out_pitch,
                   int32_t* counts);
// page layout (layout.hip; include/aocr.h: aocr_ink_integral, aocr_layout_blocks): the summed-area table of the ink mask and the XY cut on it
size_t integral_scratch_bytes(int H, int W);
void ink_integral(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, int threshold, int light_text, void* scratch, uint32_t* sat,
                  int64_t sat_pitch, int32_t* info);
size_t layout_scratch_bytes(int max_blocks);
void layout_blocks(hipStream_t s, const uint32_t* sat, int64_t sat_pitch, int H, int W, const aocr_layout_params& p, void* scratch, int max_blocks,
                   aocr_box* blocks, int32_t* counts);
// connected components (components.hip; include/aocr.h: aocr_label_components, aocr_clean_page): canonical labels, area and box per component,
// and the page with its specks and rules painted over
size_t components_scratch_bytes(int H, int W);
void label_components(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, int threshold, int light_text, int connectivity,
                      void* scratch, int32_t* labels, int64_t labels_pitch, int max_components, aocr_box* comps, int32_t* info);
size_t clean_scratch_bytes(int H, int W);
void clean_page(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_clean_params& p, void* scratch, uint8_t* out,
                int64_t out_pitch, int32_t* counts);
// rule removal that keeps the text (rules.hip; include/aocr.h: aocr_remove_rules): run-length rules per pixel on bit planes of the ink; counts
// may be nullptr
size_t rules_scratch_bytes(int H, int W);
void remove_rules(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_rule_params& p, void* scratch, uint8_t* out,
                  int64_t out_pitch, int32_t* counts);
// reversed-out panels (panels.hip; include/aocr.h: aocr_invert_panels): the slabs among the components of components.hip, 255 - v inside their row
// spans; panels may be nullptr
size_t panels_scratch_bytes(int H, int W, int max_panels);
void invert_panels(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_panel_params& p, void* scratch, uint8_t* out,
                   int64_t out_pitch, int max_panels, int32_t* panels, int32_t* counts);
// where the launches of label_components leave every component's area (components.hip): the record of the component whose first pixel in
// raster order is (rx, ry) is the four words at rec + 4 * (ry * sw + (rx >> 1)): area, min x, max x, max y.  scratch: label_components' own
struct ComponentAreas { const int32_t* rec; int sw; };
ComponentAreas component_areas(int H, int W, void* scratch);
// page orientation (orient.hip; include/aocr.h: aocr_rotate_page, aocr_estimate_orientation): quarter turns of a pitched page, and the run-start
// counts that say which way the text lines run
void rotate_page(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const int32_t* orient, int quarter, uint8_t* out,
                 int64_t out_pitch);
size_t orient_scratch_bytes(int H, int W);
void estimate_orientation(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, int threshold, int light_text, void* scratch,
                          int32_t* orient);
// page rectification (rectify.hip; include/aocr.h: aocr_find_page_quad, aocr_rectify_plan, aocr_warp_page): the corners of the paper on a
// photograph, the output size and coefficients of the projective map (host only; 1 and a message in err_buf on error), and the resample
constexpr int RECTIFY_COORD_MAX = 1 << 20;
size_t quad_scratch_bytes(int H, int W);
void find_page_quad(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, int threshold, int dark_paper, void* scratch,
                    int32_t* quad);
int rectify_plan(const int32_t* quad, int Wo_in, int Ho_in, int32_t* size, double* coef, char* err_buf, size_t err_len);
void warp_page(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const double* coef, int fill, uint8_t* out, int64_t out_pitch,
               int Ho, int Wo);
// page scale normalisation (scale.hip; include/aocr.h: aocr_estimate_glyph_size, aocr_resize_page): the quartiles of min(w, h) over the
// components that can be glyphs, and exact pixel-area resampling to any size
constexpr int GLYPH_SIZE_MAX = 1024;           // the largest max_size: the histogram's bins
size_t glyph_scratch_bytes(int H, int W);
void estimate_glyph_size(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_glyph_params& p, void* scratch,
                         int32_t* glyph);
void resize_page(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, uint8_t* out, int64_t out_pitch, int Ho, int Wo);
// crops (data.hip; aocr_crop_lines): preprocess_lines' scaling of n box rectangles of a pitched page, n = min(n_boxes, count[0]) on the device
void crop_lines(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_box* boxes, const int32_t* count, int n_boxes,
                int out_h, int out_w, float* out);
// word slant (slant.hip; include/aocr.h: aocr_estimate_slant, aocr_crop_lines_slanted): one slant per box from a sweep of sheared column
// profiles, and crop_lines with every row of a box moved back along x (the scaling itself is resample.h's, shared with data.hip)
size_t slant_scratch_bytes(int n_boxes, int n_steps);
void estimate_slant(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_box* boxes, const int32_t* count, int n_boxes,
                    const aocr_slant_params& p, const int32_t* threshold, void* scratch, int32_t* slant, uint64_t* scores);
void crop_lines_slanted(hipStream_t s, const uint8_t* page, int64_t pitch, int H, int W, const aocr_box* boxes, const int32_t* count,
                        int n_boxes, const int32_t* slant, int fill, int out_h, int out_w, float* out);
}  // namespace aocr
