// tests/libkprobe.so: extern "C" wrappers around the host launchers of the bf16-source conv / GEMM paths, of the fused recurrent-step
// kernels, of the attention kernels, of the BatchNorm / un-pool / conv1 / column-sum kernels and of the loss, token-sum, optimizer, beam-search and small
// elementwise kernels, and of the whole-sequence encoder recurrences (csrc/ops.h), for tests/test_kernels_bf16_gpu.py, tests/test_step_kernels_bf16_gpu.py,
// tests/test_attention_kernels_gpu.py, tests/test_cnn_elementwise_kernels_gpu.py, tests/test_tail_kernels_gpu.py and tests/test_encoder_seq_kernels_gpu.py; and of
// the exact-fp32 (compute="f32") forms of the same launchers -- kp_conv_weight_transpose_f32, kp_conv_backward_data_f32 (the re-laid taps wtf), kp_big_kk_f32
// (two-segment LoadK operands, ksplit), kp_small_f32_gates_fwd / _kk / _kmn / _gates_bwd_kk / _gates_bwd -- for tests/test_kernels_f32_gpu.py and
// tests/test_step_kernels_f32_gpu.py (kp_conv_forward, kp_conv_backward_filter, kp_grouped_wgrad and kp_gemm take bf16 = 0 as they are).
// Test infrastructure: no kernels of its own, not part of the product's C ABI (include/aocr.h).
// Every wrapper enqueues on the given stream and returns hipGetLastError().  Pointers to bf16 data are passed as the raw addresses
// of torch.bfloat16 tensors (the same bit layout as bf16_t).
#include "ops.h"

using aocr::bf16_t;
#define H16(p) reinterpret_cast<const bf16_t*>(p)
#define W16(p) reinterpret_cast<bf16_t*>(p)

extern "C" {

int kp_conv_forward(hipStream_t s, int bf16, const float* x, const float* w, const float* bias, float* y, uint8_t* idx, int B, int H, int W,
                    int Cin, int Cout, int ks, int pad, int relu, int pool, const void* xb, const void* wb, void* yb,
                    const float* bn_save, const float* bn_w, const float* bn_b, double* bn_part, int* bn_chunks) {
  aocr::conv_forward(s, bf16 != 0, x, w, bias, y, idx, B, H, W, Cin, Cout, ks, pad, relu, pool, H16(xb), H16(wb), W16(yb), 0,
                     bn_save, bn_w, bn_b, bn_part, bn_chunks, nullptr);
  return (int)hipGetLastError();
}

int kp_conv_backward_data(hipStream_t s, int bf16, const float* dy, const float* w, float* dx, int B, int H, int W, int Cin, int Cout,
                          int ks, int pad, const void* dyb, const void* wtb, int* dx16) {
  aocr::conv_backward_data(s, bf16 != 0, dy, w, dx, B, H, W, Cin, Cout, ks, pad, H16(dyb), H16(wtb), nullptr, dx16, nullptr, nullptr);
  return (int)hipGetLastError();
}

// exact-fp32 mode as the model runs it: the taps re-laid [Cin][tap][Cout] (wtf, from kp_conv_weight_transpose_f32) -> LoadConvK x LoadK
int kp_conv_weight_transpose_f32(hipStream_t s, const float* w, float* wt, int Cout, int KK, int Cin) {
  aocr::conv_weight_transpose_f32(s, w, wt, Cout, KK, Cin);
  return (int)hipGetLastError();
}
int kp_conv_backward_data_f32(hipStream_t s, const float* dy, const float* w, const float* wtf, float* dx, int B, int H, int W, int Cin, int Cout, int ks, int pad) {
  aocr::conv_backward_data(s, false, dy, w, dx, B, H, W, Cin, Cout, ks, pad, nullptr, nullptr, wtf, nullptr, nullptr, nullptr);
  return (int)hipGetLastError();
}

int kp_conv_backward_filter(hipStream_t s, int bf16, const float* x, const float* dy, float* dw, float* dbias, int B, int H, int W,
                            int Cin, int Cout, int ks, int pad, const void* xb, const void* dyb, float* part, size_t part_floats) {
  aocr::conv_backward_filter(s, bf16 != 0, x, dy, dw, dbias, B, H, W, Cin, Cout, ks, pad, H16(xb), H16(dyb), part, part_floats, 0);
  return (int)hipGetLastError();
}

int kp_conv_weight_shadows(hipStream_t s, const float* w, void* wb, void* wtb, int Cout, int KK, int Cin) {
  aocr::conv_weight_shadows(s, w, W16(wb), W16(wtb), Cout, KK, Cin);
  return (int)hipGetLastError();
}

int kp_splitk_reduce(hipStream_t s, const float* part, int ks, size_t n, float* out) {
  aocr::splitk_reduce(s, part, ks, n, out);
  return (int)hipGetLastError();
}

int kp_gemm_hh(hipStream_t s, const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int64_t ldc, int M, int N, int K,
               const float* bias, const float* bias2, int flags) {
  aocr::gemm_hh(s, H16(A), lda, H16(B), ldb, C, ldc, M, N, K, bias, bias2, flags);
  return (int)hipGetLastError();
}

int kp_gemm_hh_shadow(hipStream_t s, const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int64_t ldc, void* Cb, int64_t ldcb,
                      int M, int N, int K) {
  aocr::gemm_hh_shadow(s, H16(A), lda, H16(B), ldb, C, ldc, W16(Cb), ldcb, M, N, K);
  return (int)hipGetLastError();
}

// *taken = 1 when the one-launch form ran (0: the shape is not taken and nothing was launched)
int kp_gemm_hh_cat(hipStream_t s, const void* A0, const void* A1, int64_t lda, const void* B0, const void* B1, int64_t ldb, float* C,
                   int64_t ldc, int M, int N, int K0, int K1, int* taken) {
  *taken = aocr::gemm_hh_cat(s, H16(A0), H16(A1), lda, H16(B0), H16(B1), ldb, C, ldc, M, N, K0, K1) ? 1 : 0;
  return (int)hipGetLastError();
}

// one problem per entry of the parallel arrays (Ab / Bb entries may be null: no shadow)
int kp_grouped_wgrad(hipStream_t s, int bf16, int n, const float* const* A, const int64_t* lda, const float* const* B, const int64_t* ldb,
                     float* const* C, const int64_t* ldc, const int* M, const int* N, const int* K, const void* const* Ab, const void* const* Bb,
                     float* part, size_t part_floats) {
  if (n < 0 || n > 16) return (int)hipErrorInvalidValue;
  aocr::WGradProblem p[16];
  for (int i = 0; i < n; ++i) {
    p[i].A = A[i]; p[i].lda = lda[i]; p[i].B = B[i]; p[i].ldb = ldb[i]; p[i].C = C[i]; p[i].ldc = ldc[i];
    p[i].M = M[i]; p[i].N = N[i]; p[i].K = K[i]; p[i].Ab = H16(Ab[i]); p[i].Bb = H16(Bb[i]);
  }
  aocr::grouped_wgrad(s, bf16 != 0, p, n, part, part_floats);
  return (int)hipGetLastError();
}

int kp_bn_relu_forward(hipStream_t s, const float* x, float* y, const float* w, const float* b, float* rm, float* rv, float* save,
                       void* scratch, int64_t rows, int C, int training, int update_running, int stats_chunks) {
  aocr::bn_relu_forward(s, x, y, w, b, rm, rv, save, scratch, rows, C, training, update_running, 0, nullptr, nullptr, stats_chunks, nullptr);
  return (int)hipGetLastError();
}

size_t kp_bn_scratch_bytes(int C) { return aocr::bn_scratch_bytes(C); }

int kp_bn_eval_prepare(hipStream_t s, const float* rm, const float* rv, float* save, int C) {
  aocr::bn_eval_prepare(s, rm, rv, save, C);
  return (int)hipGetLastError();
}

// ---- BatchNorm, un-pool, conv1 and the column sums (csrc/ops_misc.hip), for tests/test_cnn_elementwise_kernels_gpu.py: the launchers' full argument lists.
// sync != 0: a BnSync whose all-reduce is the one-rank identity below (the launcher then takes its synchronised branch: bn_sums_kernel + bn_fwd_stats_kernel /
// bn_bwd_scale_kernel).  defer != 0: the wrapper owns a ColsumJobs, hands it to the launcher and flushes it on the same stream before it returns.
static int kp_allreduce_identity(void*, void*, int64_t, int, hipStream_t) { return 0; }
static const aocr::BnSync kp_sync1 = {kp_allreduce_identity, nullptr};

int kp_bn_relu_forward2(hipStream_t s, const float* x, float* y, const float* w, const float* b, float* rm, float* rv, float* save, void* scratch,
                        int64_t rows, int C, int training, int update_running, int tb_rows, void* yb, int sync, int stats_chunks, const void* xh) {
  aocr::bn_relu_forward(s, x, y, w, b, rm, rv, save, scratch, rows, C, training, update_running, tb_rows, W16(yb), sync ? &kp_sync1 : nullptr, stats_chunks,
                        H16(xh));
  return (int)hipGetLastError();
}
int kp_bn_relu_backward(hipStream_t s, const float* x, const float* y, const float* dA, const float* w, const float* save, float* dx, float* dw, float* db,
                        void* scratch, int64_t rows, int C, int tb_rows, void* dxb, const void* yb, float* conv_dbias, float* partial, int sync, int defer,
                        const void* xh, const void* dAh, int sums_chunks) {
  aocr::ColsumJobs jobs = {};
  aocr::bn_relu_backward(s, x, y, dA, w, save, dx, dw, db, scratch, rows, C, tb_rows, W16(dxb), H16(yb), conv_dbias, partial, sync ? &kp_sync1 : nullptr,
                         defer ? &jobs : nullptr, H16(xh), H16(dAh), sums_chunks);
  if (defer) aocr::colsum_flush(s, jobs);
  return (int)hipGetLastError();
}
int kp_unpool_relu_backward(hipStream_t s, const float* dpooled, const float* pooled, const uint8_t* idx, float* dy, int B, int Ho, int Wo, int C, int pool,
                            void* dyb, float* dbias, float* partial, const void* pooledb, int defer, const void* dpooled16) {
  aocr::ColsumJobs jobs = {};
  aocr::unpool_relu_backward(s, dpooled, pooled, idx, dy, B, Ho, Wo, C, pool, W16(dyb), dbias, partial, H16(pooledb), defer ? &jobs : nullptr, H16(dpooled16));
  if (defer) aocr::colsum_flush(s, jobs);
  return (int)hipGetLastError();
}
int kp_conv1_forward(hipStream_t s, const float* x, const float* w, const float* bias, float* y, int B, int H, int W, void* yb, uint16_t* route) {
  aocr::conv1_forward(s, x, w, bias, y, B, H, W, W16(yb), route);
  return (int)hipGetLastError();
}
size_t kp_conv1_route_elems(int B, int H, int W) { return aocr::conv1_route_elems(B, H, W); }
int kp_conv1_backward(hipStream_t s, const float* x, const float* w, const float* bias, const float* dyp, float* dw, float* db, int B, int H, int W,
                      float* scratch, int defer, const uint16_t* route) {
  aocr::ColsumJobs jobs = {};
  aocr::conv1_backward(s, x, w, bias, dyp, dw, db, B, H, W, scratch, defer ? &jobs : nullptr, route);
  if (defer) aocr::colsum_flush(s, jobs);
  return (int)hipGetLastError();
}
int kp_colsum_accum(hipStream_t s, const float* A, int64_t ld, int64_t rows, int N, float* out, float* out2) {
  aocr::colsum_accum(s, A, ld, rows, N, out, out2);
  return (int)hipGetLastError();
}
// n jobs (parallel arrays; out2 entries may be null) deferred in order, then ONE flush.  *dropped = the jobs colsum_defer did not take (its table holds 8).
int kp_colsum_jobs(hipStream_t s, int n, const float* const* A, const int64_t* ld, const int64_t* rows, const int* N, float* const* out, float* const* out2,
                   int* dropped) {
  if (n < 0 || n > 16) return (int)hipErrorInvalidValue;
  aocr::ColsumJobs jobs = {};
  *dropped = 0;
  for (int i = 0; i < n; ++i) {
    const int before = jobs.n;
    aocr::colsum_defer(jobs, A[i], ld[i], rows[i], N[i], out[i], out2[i]);
    if (jobs.n == before) ++*dropped;
  }
  aocr::colsum_flush(s, jobs);
  return (int)hipGetLastError();
}

// ---- the attention launchers (csrc/ops_misc.hip), for tests/test_attention_kernels_gpu.py: the launchers' own signatures (the forward query has ldu = Hd and
// d q has ldo = Hd inside the launchers; no stride the product cannot pass is added here)
int kp_attention_forward(hipStream_t s, const float* ctx, const float* q, float* a, float* c, int64_t ldc, int B, int T, int Hd, int ctx_div, void* cb,
                         int64_t ldcb, const void* ctxb) {
  aocr::attention_forward(s, ctx, q, a, c, ldc, B, T, Hd, ctx_div, W16(cb), ldcb, H16(ctxb));
  return (int)hipGetLastError();
}
int kp_attention_backward(hipStream_t s, const float* ctx, const float* a, const float* dc, int64_t lddc, float* ds, float* dq, int B, int T, int Hd,
                          void* dqb, const void* ctxb, const float* cfwd, int64_t ldcf) {
  aocr::attention_backward(s, ctx, nullptr, a, dc, lddc, ds, dq, B, T, Hd, W16(dqb), H16(ctxb), cfwd, ldcf);
  return (int)hipGetLastError();
}
int kp_attention_forward_dual(hipStream_t s, const float* h_top, int64_t ldh, float* a, float* c, int64_t ldc, int B, int T, int ctx_div, void* cb,
                              int64_t ldcb, const void* ctxb, const void* ctxab) {
  aocr::attention_forward_dual(s, h_top, ldh, a, c, ldc, B, T, ctx_div, W16(cb), ldcb, H16(ctxb), H16(ctxab));
  return (int)hipGetLastError();
}
int kp_attention_backward_dual(hipStream_t s, const float* a, const float* dc, int64_t lddc, float* ds, float* dq, void* dqb, float* dh_attn, int B, int T,
                               const void* ctxb, const void* ctxab) {
  aocr::attention_backward_dual(s, a, dc, lddc, ds, dq, W16(dqb), dh_attn, B, T, H16(ctxb), H16(ctxab));
  return (int)hipGetLastError();
}
int kp_attention_dual_ok(int T, int Hd, const void* ctxb, const void* ctxab) { return aocr::attention_dual_ok(T, Hd, H16(ctxb), H16(ctxab)) ? 1 : 0; }
int kp_attention_dctx(hipStream_t s, const float* a_all, const float* ds_all, const float* dc_all, int64_t lddc, const float* q_all, float* dctx, int L, int B,
                      int T, int Hd) {
  aocr::attention_dctx(s, a_all, ds_all, dc_all, lddc, q_all, dctx, L, B, T, Hd);
  return (int)hipGetLastError();
}

// ---- the fused recurrent-step launchers.  One flat struct per problem (tests/test_step_kernels_bf16_gpu.py mirrors them as ctypes.Structure); a null pointer
// means "absent".  An operand is one K segment (p1 == null, K = K0) or two ([p0 | p1], K = K0 + K1) with a row stride each; the A side of an _hh wrapper is the
// bf16 shadow, of an _h wrapper the fp32 buffer (B is always a bf16 weight shadow).
struct KpOperand { const void* p0; int64_t ld0; int K0; const void* p1; int64_t ld1; int K1; int rows; };
struct KpDrop { unsigned long long base, thr; float scale; long long off; };
struct KpStore {
  KpOperand a, b;
  float* C; int64_t ldc; const float* bias; const float* bias2; int flags;
  float* C1; int64_t ldc1; int N0;
  void* Cb; int64_t ldcb;
  const float* dg; const float* dout; int64_t ldd;
};
struct KpGatesFwd {
  KpOperand a, b;
  const float* zx; int64_t ldzx; const float* b1; const float* b2;
  const float* c_prev; int64_t ldcp; float* c_out; int64_t ldc; float* h_out; int64_t ldh; float* h_out2; int64_t ldh2;
  float* gates; int64_t ldg; void* hb; int64_t ldhb; void* hb2; int64_t ldhb2;
  const int32_t* zx_tok; int64_t zx_tok_stride; KpDrop drop;
};
struct KpGatesBwd {
  KpOperand a, b;
  const float* dh1; int64_t ld1; const float* dh2; int64_t ld2; const float* dh3; int64_t ld3; const float* dc_in; int64_t lddc;
  const float* gates; int64_t ldg; const float* c_prev; int64_t ldcp; const float* c; int64_t ldcc;
  float* dz; int64_t lddz; float* dc_out; int64_t lddco; void* dzb; int64_t lddzb; KpDrop drop; int gil;
};

}  // extern "C"

namespace {
using namespace aocr;
LoadKh2 kh(const KpOperand& o) {
  return o.p1 ? make_loadkh2(H16(o.p0), o.ld0, o.K0, H16(o.p1), o.ld1, o.K1, o.rows) : make_loadkh(H16(o.p0), o.ld0, o.rows, o.K0);
}
LoadK kf(const KpOperand& o) {
  return o.p1 ? make_loadk2((const float*)o.p0, o.ld0, o.K0, (const float*)o.p1, o.ld1, o.K1, o.rows) : make_loadk((const float*)o.p0, o.ld0, o.rows, o.K0);
}
void load_a(LoadKh2& l, const KpOperand& o) { l = kh(o); }
void load_a(LoadK& l, const KpOperand& o) { l = kf(o); }
DropSpec drop_of(const KpDrop& d) { DropSpec s; s.base = d.base; s.thr = d.thr; s.scale = d.scale; s.off = d.off; return s; }
EpStore ep_of(const KpStore& p, int M, int N) {
  EpStore e = make_store(p.C, p.ldc, M, N, p.bias, p.bias2, p.flags);
  if (p.C1) { e.C1 = p.C1; e.ldc1 = p.ldc1; e.N0 = p.N0; }
  e.Cb = W16(p.Cb); e.ldcb = p.ldcb; e.dg = p.dg; e.dout = p.dout; e.ldd = p.ldd;
  return e;
}
EpGatesFwd ep_of(const KpGatesFwd& p, int M, int H) {
  EpGatesFwd e;
  e.zx = p.zx; e.ldzx = p.ldzx; e.b1 = p.b1; e.b2 = p.b2; e.c_prev = p.c_prev; e.ldcp = p.ldcp; e.c_out = p.c_out; e.ldc = p.ldc;
  e.h_out = p.h_out; e.ldh = p.ldh; e.h_out2 = p.h_out2; e.ldh2 = p.ldh2; e.gates = p.gates; e.ldg = p.ldg; e.M = M; e.H = H;
  e.hb = W16(p.hb); e.ldhb = p.ldhb; e.hb2 = W16(p.hb2); e.ldhb2 = p.ldhb2; e.zx_tok = p.zx_tok; e.zx_tok_stride = p.zx_tok_stride;
  e.drop = drop_of(p.drop);
  return e;
}
EpGatesBwd ep_of(const KpGatesBwd& p, int M, int H) {
  EpGatesBwd e;
  e.dh1 = p.dh1; e.ld1 = p.ld1; e.dh2 = p.dh2; e.ld2 = p.ld2; e.dh3 = p.dh3; e.ld3 = p.ld3; e.dc_in = p.dc_in; e.lddc = p.lddc;
  e.gates = p.gates; e.ldg = p.ldg; e.c_prev = p.c_prev; e.ldcp = p.ldcp; e.c = p.c; e.ldcc = p.ldcc; e.dz = p.dz; e.lddz = p.lddz;
  e.dc_out = p.dc_out; e.lddco = p.lddco; e.M = M; e.H = H; e.dzb = W16(p.dzb); e.lddzb = p.lddzb; e.drop = drop_of(p.drop); e.gil = p.gil != 0;
  return e;
}
// nz = 1..3 problems -> the launcher's argument sets (SmallArgs<A loader, LoadKh2, epilogue>)
template <class ARGS, class P> int fill(ARGS (&z)[3], int nz, const P* p, int M, int cols) {
  if (nz < 1 || nz > 3) return (int)hipErrorInvalidValue;
  for (int i = 0; i < nz; ++i) { load_a(z[i].a, p[i].a); z[i].b = kh(p[i].b); z[i].ep = ep_of(p[i], M, cols); z[i].K = z[i].a.K; }
  return 0;
}
// the exact-fp32 launchers' argument sets: A and B from fp32 buffers, B as its loader type says
void load_b(LoadK& l, const KpOperand& o) { l = kf(o); }
void load_b(LoadMN& l, const KpOperand& o) { l = make_loadmn((const float*)o.p0, o.ld0, o.rows, o.K0); }
template <class ARGS, class P> int fill_f32(ARGS (&z)[3], int nz, const P* p, int M, int cols) {
  if (nz < 1 || nz > 3) return (int)hipErrorInvalidValue;
  for (int i = 0; i < nz; ++i) { z[i].a = kf(p[i].a); load_b(z[i].b, p[i].b); z[i].ep = ep_of(p[i], M, cols); z[i].K = z[i].a.K; }
  return 0;
}
}  // namespace

extern "C" {

#define KP_SMALL(name, ARGS, P, launcher)                                        \
  int name(hipStream_t s, int nz, const P* p, int M, int cols) {                 \
    aocr::ARGS z[3];                                                             \
    if (int rc = fill(z, nz, p, M, cols)) return rc;                             \
    aocr::launcher(s, nz, z, M, cols);                                           \
    return (int)hipGetLastError();                                               \
  }
KP_SMALL(kp_small_gates_fwd_hh, GatesFwdArgsHH, KpGatesFwd, launch_small_gates_fwd_hh)
KP_SMALL(kp_small_gates_fwd_h, GatesFwdArgsH, KpGatesFwd, launch_small_gates_fwd_h)
KP_SMALL(kp_small_hh, SmallArgsHH, KpStore, launch_small_hh)
KP_SMALL(kp_small_h, SmallArgsH, KpStore, launch_small_h)
KP_SMALL(kp_small_gates_bwd_hh, GatesBwdArgsHH, KpGatesBwd, launch_small_gates_bwd_hh)
KP_SMALL(kp_small_gates_bwd_h, GatesBwdArgsH, KpGatesBwd, launch_small_gates_bwd_h)
#undef KP_SMALL

// ---- the exact-fp32 forms (tests/test_kernels_f32_gpu.py, tests/test_step_kernels_f32_gpu.py): both operands fp32.  A is K-contiguous (kf: one or two
// segments); B is K-contiguous too (LoadK, [cols][K]) or, for _kmn and _gates_bwd, M/N-contiguous (LoadMN: ONE segment, p0 [K0][rows] with row stride ld0).
int kp_big_kk_f32(hipStream_t s, const KpStore* p, int M, int N, int ksplit) {
  const aocr::LoadK a = kf(p->a), b = kf(p->b);
  aocr::launch_big_kk(s, false, a, b, ep_of(*p, M, N), M, N, a.K, ksplit);
  return (int)hipGetLastError();
}
int kp_small_f32_gates_fwd(hipStream_t s, int nz, const KpGatesFwd* p, int M, int cols) {
  aocr::GatesFwdArgs z[3];
  if (int rc = fill_f32(z, nz, p, M, cols)) return rc;
  aocr::launch_small_gates_fwd(s, false, nz, z, M, cols);
  return (int)hipGetLastError();
}
int kp_small_f32_kk(hipStream_t s, int nz, const KpStore* p, int M, int cols) {
  aocr::SmallKKArgs z[3];
  if (int rc = fill_f32(z, nz, p, M, cols)) return rc;
  aocr::launch_small_kk(s, false, nz, z, M, cols);
  return (int)hipGetLastError();
}
int kp_small_f32_kmn(hipStream_t s, int nz, const KpStore* p, int M, int cols) {
  aocr::SmallKMNArgs z[3];
  if (int rc = fill_f32(z, nz, p, M, cols)) return rc;
  aocr::launch_small_kmn(s, false, nz, z, M, cols);
  return (int)hipGetLastError();
}
int kp_small_f32_gates_bwd_kk(hipStream_t s, int nz, const KpGatesBwd* p, int M, int cols) {
  aocr::GatesBwdKKArgs z[3];
  if (int rc = fill_f32(z, nz, p, M, cols)) return rc;
  aocr::launch_small_gates_bwd_kk(s, nz, z, M, cols);
  return (int)hipGetLastError();
}
int kp_small_f32_gates_bwd(hipStream_t s, int nz, const KpGatesBwd* p, int M, int cols) {
  aocr::GatesBwdArgs z[3];
  if (int rc = fill_f32(z, nz, p, M, cols)) return rc;
  aocr::launch_small_gates_bwd(s, false, nz, z, M, cols);
  return (int)hipGetLastError();
}

// the cell backward without a product (the operands of *p are ignored)
int kp_gates_elem_bwd(hipStream_t s, const KpGatesBwd* p, int M, int H) {
  aocr::gates_elem_bwd(s, ep_of(*p, M, H), M, H);
  return (int)hipGetLastError();
}

// *taken = 1 when the 128 x 128 tiled form ran (0: the shape is not taken and nothing was launched)
int kp_big_step_store(hipStream_t s, const KpStore* p, int M, int N, int* taken) {
  *taken = aocr::big_step_store(s, kh(p->a), kh(p->b), ep_of(*p, M, N), M, N) ? 1 : 0;
  return (int)hipGetLastError();
}
int kp_big_step_gates_fwd(hipStream_t s, const KpGatesFwd* p, int M, int H, float* zbuf, size_t zbuf_floats, int* taken) {
  *taken = aocr::big_step_gates_fwd(s, kh(p->a), kh(p->b), ep_of(*p, M, H), M, H, zbuf, zbuf_floats) ? 1 : 0;
  return (int)hipGetLastError();
}

// ---- loss, sums by token, optimizer, weight shadows, beam search and the small elementwise kernels (csrc/ops_misc.hip; project_loss: csrc/ops_gemm.hip), for
// tests/test_tail_kernels_gpu.py: the launchers' own argument lists.  Structs passed by pointer mirror the C++ ones field by field (KpTrie = TrieView,
// KpDecInit = DecInitArgs, KpDrop = DropSpec; a null KpDrop pointer / a null KpTrie pointer = the launcher's default).
struct KpTrie { const unsigned long long* mask; const int32_t* base; const int32_t* child; const int32_t* loc_in; int32_t* loc_out; };
struct KpDecInit { float* c0[4]; float* h0[4]; void* hb[4]; float* feed0; void* outb; const float *cfw, *cbw, *hfw, *hbw; int B, He, Hd, Ld, copy_h; };

int kp_logsoftmax_nll(hipStream_t s, const float* logits, int64_t ld, const int32_t* tgt, int64_t st, int64_t sb, int Bt, float* logp, float* dlogits,
                      float* nll_rows, int64_t rows, int V, float grad_scale) {
  aocr::logsoftmax_nll(s, logits, ld, tgt, st, sb, Bt, logp, dlogits, nll_rows, rows, V, grad_scale);
  return (int)hipGetLastError();
}
int kp_project_loss_ok(int rows, int V, int Hd) { return aocr::project_loss_ok(rows, V, Hd) ? 1 : 0; }
int kp_project_loss(hipStream_t s, const float* out, int64_t ldo, const float* wo, const float* bo, float* logits, float* dlogits, int64_t ld, float* nll,
                    float* dout, const int32_t* tgt, int64_t st, int64_t sb, int Bt, int rows, int V, int Hd, float scale) {
  aocr::project_loss(s, out, ldo, wo, bo, logits, dlogits, ld, nll, dout, tgt, st, sb, Bt, rows, V, Hd, scale);
  return (int)hipGetLastError();
}
// the generic product project_loss documents itself against (*rc = gemm's own return value)
int kp_gemm(hipStream_t s, int bf16, const float* A, int64_t lda, int a_kmajor, const float* B, int64_t ldb, int b_kmajor, float* C, int64_t ldc, int M, int N,
            int K, const float* bias, const float* bias2, int flags, int* rc) {
  *rc = aocr::gemm(s, bf16 != 0, A, lda, a_kmajor != 0, B, ldb, b_kmajor != 0, C, ldc, M, N, K, bias, bias2, flags);
  return (int)hipGetLastError();
}
int kp_sum_to_scalar(hipStream_t s, const float* x, int64_t n, float* out) {
  aocr::sum_to_scalar(s, x, n, out);
  return (int)hipGetLastError();
}
int kp_gold_scores(hipStream_t s, const float* nll_rows, float* gold, int L, int B) {
  aocr::gold_scores(s, nll_rows, gold, L, B);
  return (int)hipGetLastError();
}

int kp_segsum_supported(int ncols, int V, int E) { return aocr::segsum_supported(ncols, V, E) ? 1 : 0; }
size_t kp_segsum_index_ints(int rows, int V) { return aocr::segsum_index_ints(rows, V); }
int kp_segsum_by_token(hipStream_t s, const float* dz, int64_t ld, const int32_t* tok, int64_t st, int64_t sb, int L, int B, int ncols, int V, float* S,
                       int* index, float* db1, float* db2, const float* W, int64_t ldw, const float* lookup, int E, float* dlookup, float* dW) {
  aocr::segsum_by_token(s, dz, ld, tok, st, sb, L, B, ncols, V, S, index, db1, db2, W, ldw, lookup, E, dlookup, dW);
  return (int)hipGetLastError();
}
int kp_embedding_gather(hipStream_t s, const float* table, const int32_t* tok, int64_t st, int64_t sb, float* out, int L, int B, int E) {
  aocr::embedding_gather(s, table, tok, st, sb, out, L, B, E);
  return (int)hipGetLastError();
}
int kp_embedding_scatter_accum(hipStream_t s, const float* demb, const int32_t* tok, int64_t st, int64_t sb, float* dtable, int L, int B, int E, int V) {
  aocr::embedding_scatter_accum(s, demb, tok, st, sb, dtable, L, B, E, V);
  return (int)hipGetLastError();
}

size_t kp_sgd_scratch_bytes() { return aocr::sgd_scratch_bytes(); }
int kp_cl_err_latch() { return aocr::CL_ERR_LATCH; }
int kp_cl_err_sticky() { return aocr::CL_ERR_STICKY; }
int kp_sgd_clip_update(hipStream_t s, float* params, float* grads, const int64_t* group_off, float lr, float clip, float* norms_out, void* scratch, int* err,
                       float* bn_state, const float* bn_snap, int bn_n) {
  aocr::sgd_clip_update(s, params, grads, group_off, lr, clip, norms_out, scratch, err, bn_state, bn_snap, bn_n);
  return (int)hipGetLastError();
}
int kp_adadelta_update(hipStream_t s, float* params, float* grads, float* var, float* acc, int64_t n, float rho, float eps, float wd, int* err, float* bn_state,
                       const float* bn_snap, int bn_n) {
  aocr::adadelta_update(s, params, grads, var, acc, n, rho, eps, wd, err, bn_state, bn_snap, bn_n);
  return (int)hipGetLastError();
}
int kp_step_snapshot(hipStream_t s, const float* bn_state, float* bn_snap, int n, int* err) {
  aocr::step_snapshot(s, bn_state, bn_snap, n, err);
  return (int)hipGetLastError();
}

// n pieces (parallel host arrays) -> the ShadowJob table as build_shadow_jobs lays it out (tile0 ascending, tx = tiles per row), copied to jobs_dev (n
// ShadowJob of device memory, kp_shadow_job_bytes() each) on the stream; then tiles [tile_off, tile_off + ntiles) are launched (ntiles < 0: all from tile_off).
// *total = the table's tile count.
size_t kp_shadow_job_bytes() { return sizeof(aocr::ShadowJob); }
int kp_shadow_jobs(hipStream_t s, int n, const float* const* w, void* const* wb, void* const* wtb, const int64_t* ld, const int64_t* ldb, const int64_t* ldt,
                   const int* R, const int* C, void* jobs_dev, int tile_off, int ntiles, int* total) {
  if (n < 1 || n > 16) return (int)hipErrorInvalidValue;
  aocr::ShadowJob j[16];
  int tiles = 0;
  for (int i = 0; i < n; ++i) {
    j[i] = aocr::ShadowJob{w[i], W16(wb[i]), W16(wtb[i]), ld[i], ldb[i], ldt[i], R[i], C[i], tiles, aocr::cdiv(C[i], 32)};
    tiles += aocr::cdiv(C[i], 32) * aocr::cdiv(R[i], 32);
  }
  *total = tiles;
  if (tile_off < 0 || tile_off > tiles) return (int)hipErrorInvalidValue;
  if (ntiles < 0) ntiles = tiles - tile_off;
  if (tile_off + ntiles > tiles) return (int)hipErrorInvalidValue;
  if (hipError_t e = hipMemcpyAsync(jobs_dev, j, n * sizeof(aocr::ShadowJob), hipMemcpyHostToDevice, s)) return (int)e;
  if (hipError_t e = hipStreamSynchronize(s)) return (int)e;      // (the table is on this stack frame)
  aocr::shadow_jobs(s, static_cast<const aocr::ShadowJob*>(jobs_dev), n, ntiles, tile_off);
  return (int)hipGetLastError();
}

static aocr::TrieView trie_of(const KpTrie& t) { aocr::TrieView v; v.mask = t.mask; v.base = t.base; v.child = t.child; v.loc_in = t.loc_in; v.loc_out = t.loc_out; return v; }
int kp_beam_select(hipStream_t s, const float* logp, const int32_t* prev_tok, float* beam_scores, int32_t* tokens, int32_t* parents, int B, int kin, int kout,
                   int V, const float* logits, int64_t ldl, const KpTrie* tv, float* sc_out) {
  aocr::TrieView v; if (tv) v = trie_of(*tv);
  aocr::beam_select(s, logp, prev_tok, beam_scores, tokens, parents, B, kin, kout, V, logits, ldl, tv ? &v : nullptr, sc_out);
  return (int)hipGetLastError();
}
int kp_project_select(hipStream_t s, const float* h, int64_t ldh, const float* wo, const float* bo, int Hd, const int32_t* prev_tok, float* beam_scores,
                      int32_t* tokens, int32_t* parents, int B, int kin, int kout, int V, const KpTrie* tv, float* sc_out) {
  aocr::TrieView v; if (tv) v = trie_of(*tv);
  aocr::project_select(s, h, ldh, wo, bo, Hd, prev_tok, beam_scores, tokens, parents, B, kin, kout, V, tv ? &v : nullptr, sc_out);
  return (int)hipGetLastError();
}
// n tensors (parallel host arrays of device pointers; dstb null or with null entries: no bf16 copy)
int kp_gather_beam_rows_many(hipStream_t s, int n, const float* const* src, float* const* dst, int64_t ld, const int32_t* parents, int B, int kin, int kout,
                             int width, void* const* dstb) {
  if (n < 0 || n > 16) return (int)hipErrorInvalidValue;
  aocr::bf16_t* db[16];
  for (int i = 0; i < n; ++i) db[i] = dstb ? W16(dstb[i]) : nullptr;
  aocr::gather_beam_rows_many(s, n, src, dst, ld, parents, B, kin, kout, width, dstb ? db : nullptr);
  return (int)hipGetLastError();
}
int kp_gather_beam_rows(hipStream_t s, const float* src, int64_t lds, float* dst, int64_t ldd, const int32_t* parents, int B, int kin, int kout, int width) {
  aocr::gather_beam_rows(s, src, lds, dst, ldd, parents, B, kin, kout, width);
  return (int)hipGetLastError();
}
int kp_token_rows(hipStream_t s, const float* table, const int32_t* tok, int64_t stride, float* dst, int R, int width) {
  aocr::token_rows(s, table, tok, stride, dst, R, width);
  return (int)hipGetLastError();
}
int kp_beam_backtrace(hipStream_t s, const int32_t* hist_tok, const int32_t* hist_par, const float* beam_scores, int32_t* labels, float* scores, int Lt, int B,
                      int k) {
  aocr::beam_backtrace(s, hist_tok, hist_par, beam_scores, labels, scores, Lt, B, k);
  return (int)hipGetLastError();
}
int kp_recognize_gather(hipStream_t s, const int32_t* labels, const int32_t* hist_par, const float* beam_scores, const float* sc_hist, const float* attn_hist,
                        float* char_logp, float* attn, int Lt, int B, int k, int T) {
  aocr::recognize_gather(s, labels, hist_par, beam_scores, sc_hist, attn_hist, char_logp, attn, Lt, B, k, T);
  return (int)hipGetLastError();
}

int kp_dec_init(hipStream_t s, const KpDecInit* p) {
  aocr::DecInitArgs a;
  for (int l = 0; l < 4; ++l) { a.c0[l] = p->c0[l]; a.h0[l] = p->h0[l]; a.hb[l] = W16(p->hb[l]); }
  a.feed0 = p->feed0; a.outb = W16(p->outb); a.cfw = p->cfw; a.cbw = p->cbw; a.hfw = p->hfw; a.hbw = p->hbw;
  a.B = p->B; a.He = p->He; a.Hd = p->Hd; a.Ld = p->Ld; a.copy_h = p->copy_h;
  aocr::dec_init(s, a);
  return (int)hipGetLastError();
}
int kp_dpre_tanh(hipStream_t s, const float* g1, const float* g2, const float* out, float* dpre, int64_t n, void* dpreb, const KpDrop* drop) {
  aocr::DropSpec d; if (drop) d = drop_of(*drop);
  aocr::dpre_tanh(s, g1, g2, out, dpre, n, W16(dpreb), drop ? &d : nullptr);
  return (int)hipGetLastError();
}
int kp_dropout_apply(hipStream_t s, const float* src, float* dst, void* dstb, int64_t n, const KpDrop* drop) {
  aocr::dropout_apply(s, src, dst, W16(dstb), n, drop_of(*drop));
  return (int)hipGetLastError();
}
int kp_dropout_apply_b(hipStream_t s, const void* src, float* dst, void* dstb, int64_t n, const KpDrop* drop) {
  aocr::dropout_apply_b(s, H16(src), dst, W16(dstb), n, drop_of(*drop));
  return (int)hipGetLastError();
}
// n regions (parallel host arrays) through ZeroList::add (which drops empty regions), one launch
int kp_zero_many(hipStream_t s, int n, void* const* p, const size_t* bytes) {
  if (n < 0 || n > 16) return (int)hipErrorInvalidValue;
  aocr::ZeroList z;
  for (int i = 0; i < n; ++i) z.add(p[i], bytes[i]);
  aocr::zero_many(s, z);
  return (int)hipGetLastError();
}
int kp_copy2d_bf16(hipStream_t s, const float* src, int64_t lds, void* dst, int64_t ldd, int rows, int cols) {
  aocr::copy2d_bf16(s, src, lds, W16(dst), ldd, rows, cols);
  return (int)hipGetLastError();
}
int kp_edit_distance(hipStream_t s, const int32_t* labels, const int32_t* targets, int B, int L, int32_t* dist, int32_t* target_len) {
  aocr::edit_distance(s, labels, targets, B, L, dist, target_len);
  return (int)hipGetLastError();
}

// ---- the whole-sequence encoder recurrences (csrc/rnn_seq.hip, csrc/rnn_cluster.hip), for tests/test_encoder_seq_kernels_gpu.py.  One flat struct per problem
// (mirrored there as ctypes.Structure): KpEncDir = EncSeqDir, KpEncBwdDir = EncSeqBwdDir field by field, then what the host sets of the launch arguments.
// A wrapper REFUSES -- returns one of the KP_ENC_* codes below (above every hipError_t) and launches nothing -- whatever the model would not launch either:
// the cluster kernels wait for each other, so every workgroup of a launch must be resident at once, which is what enc_cluster_plan decides.
struct KpEncDir { const void* w; const float* zx; float* hs; float* cs; void* hsb; float* gates; float* ctx; int reverse; };
struct KpEncBwdDir {
  const void* wt; const float* dh1; int64_t dh1_row, dh1_t; const float* dh2; int64_t dh2_row; float* dc; const float* dc_in; int64_t dc_in_row;
  const float* gates; const float* cs; float* dz; void* dzb; float* dbi; float* dbh; int forward_dir;
};
struct KpEncSeqFwd { KpEncDir d[2]; int B, T, He, Hd; };
struct KpEncSeqBwd { KpEncBwdDir d[2]; int B, T, He; };
// buf = xbuf (forward) / pbuf (backward); *_bytes / err_ints: what the caller allocated; layers: the sets of group slots the buffers were sized for (model.hip: Le)
struct KpEncCl {
  int B, T, He, Hd, groups; unsigned epoch; int it0, it1, gslot;
  unsigned long long* buf; size_t buf_bytes; unsigned long long* xtab; size_t xtab_bytes; int* err; size_t err_ints; int layers;
  int G, RT, reserve_cus, concurrent;
};
struct KpEncClFwd { KpEncDir d[2]; KpEncCl c; };
struct KpEncClBwd { KpEncBwdDir d[2]; KpEncCl c; };
enum { KP_ENC_UNSUPPORTED = 2001, KP_ENC_PLAN_MISMATCH = 2002, KP_ENC_BUF_SMALL = 2003, KP_ENC_XTAB_SMALL = 2004, KP_ENC_ERR_SMALL = 2005, KP_ENC_BAD_ARGS = 2006 };

}  // extern "C"

namespace {
int kp_cus() { int n = 0, dev = 0; (void)hipGetDevice(&dev); (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev); return n; }
aocr::EncSeqDir enc_dir(const KpEncDir& d) {
  aocr::EncSeqDir e; e.w = H16(d.w); e.zx = d.zx; e.hs = d.hs; e.cs = d.cs; e.hsb = W16(d.hsb); e.gates = d.gates; e.ctx = d.ctx; e.reverse = d.reverse;
  return e;
}
aocr::EncSeqBwdDir enc_bwd_dir(const KpEncBwdDir& d) {
  aocr::EncSeqBwdDir e; e.wt = H16(d.wt); e.dh1 = d.dh1; e.dh1_row = d.dh1_row; e.dh1_t = d.dh1_t; e.dh2 = d.dh2; e.dh2_row = d.dh2_row; e.dc = d.dc;
  e.dc_in = d.dc_in; e.dc_in_row = d.dc_in_row; e.gates = d.gates; e.cs = d.cs; e.dz = d.dz; e.dzb = W16(d.dzb); e.dbi = d.dbi; e.dbh = d.dbh;
  e.forward_dir = d.forward_dir;
  return e;
}
// What model.hip checks and allocates before it launches a cluster kernel, as refusals.  The sizes:
//   xbuf / pbuf  layers * enc_cluster_xbuf_bytes / enc_cluster_pbuf_bytes (model.hip: cl_xbytes, cl_pbytes: one set of group slots per layer)
//   xtab         (layers * 4 * ceil(B / 16) * 8 + 64) * 8 bytes (model.hip: cl_tbytes -- a layer's 8-row launches start at slot l * 4 * ceil(B / 16))
//   err          16 + 256 * 8 + 4096 ints (model.hip: cl_err): the error record, then the TRASH SLOTS the kernels' lanes of rows >= B store to
//                (p.err + 16, 256 lanes x 4 floats; the model leaves room for 8), then the debugging timeline of the stamps builds
// gslot is a layer's first slot, l * 2 * groups with l < layers (model.hip: encoder_forward_pipe).
int enc_cl_check(const KpEncCl& c, size_t layer_bytes) {
  if (c.reserve_cus < 0 || c.concurrent < 1 || c.layers < 1 || c.it0 < 0 || c.it1 < 0 || c.it1 > c.T || (c.it1 > 0 && c.it0 >= c.it1) || c.it0 >= c.T || c.epoch == 0 ||
      c.epoch >= (1u << 20))
    return KP_ENC_BAD_ARGS;
  int G = 0, RT = 0, groups = 0;
  if (!aocr::enc_cluster_plan(c.B, c.He, c.T, kp_cus() - c.reserve_cus, G, RT, groups)) return KP_ENC_UNSUPPORTED;
  if (G != c.G || RT != c.RT || groups != c.groups) return KP_ENC_PLAN_MISMATCH;
  if (c.gslot < 0 || c.gslot % (2 * groups) != 0 || c.gslot / (2 * groups) >= c.layers) return KP_ENC_BAD_ARGS;
  if (!c.buf || c.buf_bytes < (size_t)c.layers * layer_bytes) return KP_ENC_BUF_SMALL;
  if (!c.xtab || c.xtab_bytes < ((size_t)c.layers * 4 * ((c.B + 15) / 16) * 8 + 64) * 8) return KP_ENC_XTAB_SMALL;
  if (!c.err || c.err_ints < 16 + 256 * 8 + 4096) return KP_ENC_ERR_SMALL;
  return 0;
}
}  // namespace

extern "C" {

int kp_enc_seq_supported(int B, int He) { return aocr::enc_seq_supported(B, He, kp_cus()) ? 1 : 0; }       // (blocks_limit = the compute units, as model.hip passes it)
int kp_enc_seq_forward(hipStream_t s, const KpEncSeqFwd* p) {
  if (p->T < 1 || !aocr::enc_seq_supported(p->B, p->He, kp_cus())) return KP_ENC_UNSUPPORTED;
  aocr::EncSeqFwdArgs a; a.B = p->B; a.T = p->T; a.He = p->He; a.Hd = p->Hd;
  for (int dir = 0; dir < 2; ++dir) a.d[dir] = enc_dir(p->d[dir]);
  aocr::enc_seq_forward(s, a);
  return (int)hipGetLastError();
}
int kp_enc_seq_backward(hipStream_t s, const KpEncSeqBwd* p) {
  if (p->T < 1 || !aocr::enc_seq_supported(p->B, p->He, kp_cus())) return KP_ENC_UNSUPPORTED;
  aocr::EncSeqBwdArgs a; a.B = p->B; a.T = p->T; a.He = p->He;
  for (int dir = 0; dir < 2; ++dir) a.d[dir] = enc_bwd_dir(p->d[dir]);
  aocr::enc_seq_backward(s, a);
  return (int)hipGetLastError();
}

// -> 1 and *G, *RT, *groups when the cluster kernels take the shape on this device with reserve_cus compute units left out (0: they do not)
int kp_enc_cluster_plan(int B, int He, int T, int reserve_cus, int* G, int* RT, int* groups) {
  return reserve_cus >= 0 && aocr::enc_cluster_plan(B, He, T, kp_cus() - reserve_cus, *G, *RT, *groups) ? 1 : 0;
}
size_t kp_enc_cluster_xbuf_bytes(int B, int He) { return aocr::enc_cluster_xbuf_bytes(B, He); }
size_t kp_enc_cluster_pbuf_bytes(int B, int He) { return aocr::enc_cluster_pbuf_bytes(B, He); }
int kp_enc_cluster_forward(hipStream_t s, const KpEncClFwd* p) {
  const KpEncCl& c = p->c;
  if (int rc = enc_cl_check(c, aocr::enc_cluster_xbuf_bytes(c.B, c.He))) return rc;
  aocr::EncClFwdArgs a; a.B = c.B; a.T = c.T; a.He = c.He; a.Hd = c.Hd; a.groups = c.groups; a.epoch = c.epoch; a.xbuf = c.buf; a.err = c.err; a.xtab = c.xtab;
  a.it0 = c.it0; a.it1 = c.it1; a.gslot = c.gslot;
  for (int dir = 0; dir < 2; ++dir) a.d[dir] = enc_dir(p->d[dir]);
  aocr::enc_cluster_forward(s, a, c.G, c.RT, c.reserve_cus, c.concurrent);
  return (int)hipGetLastError();
}
int kp_enc_cluster_backward(hipStream_t s, const KpEncClBwd* p) {
  const KpEncCl& c = p->c;
  if (int rc = enc_cl_check(c, aocr::enc_cluster_pbuf_bytes(c.B, c.He))) return rc;
  aocr::EncClBwdArgs a; a.B = c.B; a.T = c.T; a.He = c.He; a.groups = c.groups; a.epoch = c.epoch; a.pbuf = c.buf; a.err = c.err; a.xtab = c.xtab;
  a.it0 = c.it0; a.it1 = c.it1; a.gslot = c.gslot;
  for (int dir = 0; dir < 2; ++dir) a.d[dir] = enc_bwd_dir(p->d[dir]);
  aocr::enc_cluster_backward(s, a, c.G, c.RT, c.reserve_cus, c.concurrent);
  return (int)hipGetLastError();
}

// ---- the whole-sequence decoder kernels (csrc/dec_cluster.hip, csrc/dec_chain.hip), for tests/test_decoder_seq_kernels_gpu.py.  One flat struct per problem
// (mirrored there as ctypes.Structure): the fields of DecClFwdArgs / DecClBwdArgs the model sets, plus what the caller allocated.  The wrappers call the PUBLIC
// launchers, so AOCR_NO_DEC_CHAINS* choose between the cluster and the chain kernels exactly as in the model.  Like the KP_ENC_* wrappers they REFUSE -- one of
// the KP_DEC_* codes, nothing launched -- what the model would not launch: the kernels of a launch wait for each other and index the buffers by group.
//   xbuf / pbuf / xtab  dec_cluster_xbuf_bytes / dec_cluster_bwd_xbuf_bytes, dec_cluster_pbuf_bytes (greedy only), dec_cluster_xtab_bytes of B
//   err                 16 + 256 * 8 + 4096 ints (model.hip: cl_err): the error record, the trash slots of the lanes of rows >= B, the stamps builds' timeline
struct KpDecFwd {
  int B, T, L, Hd; unsigned epoch; int greedy;
  const void *w1i, *w1h, *w2i, *w2h, *wc; const float *b2i, *b2h, *zx1; const void *ctxb, *ctxa;
  float* cs[2]; void* hsb[2]; float* gates[2]; float *a_all, *out; void *cat_b, *out_b;
  unsigned long long* xbuf; size_t xbuf_bytes; unsigned long long* xtab; size_t xtab_bytes; int* err; size_t err_ints;
  const int32_t* tok0; int tok0_stride; const float *wo, *bo; int V; float* pbuf; size_t pbuf_bytes; int32_t* labels; float* scores;
  const unsigned long long* trie_mask; const int32_t* trie_base; const int32_t* trie_child;
  KpDrop drop_h, drop_out; void* hm_b;
  const int32_t* zx_tok; int64_t zx_st, zx_sb; float* sc_hist;
};
struct KpDecBwd {
  int B, T, L, Hd; unsigned epoch;
  const void *w2i_t, *w2h_t, *w1h_t, *w1f_t, *wc_t, *wa_t; const float *dout_proj, *out, *a_all; const void* ctxb;
  const float* cs[2]; const float* gates[2];
  float* dpre; void* dpre_b; float* dcat; float* ds_all; float* dq; void* dq_b; float* dz[2]; void* dzb[2]; float* dc_st[2]; float* dh_rec[2]; float* dfeed;
  unsigned long long* xbuf; size_t xbuf_bytes; unsigned long long* xtab; size_t xtab_bytes; int* err; size_t err_ints;
  KpDrop drop_h, drop_out;
};
enum { KP_DEC_UNSUPPORTED = 2101, KP_DEC_XBUF_SMALL = 2102, KP_DEC_PBUF_SMALL = 2103, KP_DEC_XTAB_SMALL = 2104, KP_DEC_ERR_SMALL = 2105, KP_DEC_BAD_ARGS = 2106 };

int kp_dec_cluster_supported(int Hd, int Ld, int input_feed, int T, int L) { return aocr::dec_cluster_supported(Hd, Ld, input_feed, T, L, kp_cus()) ? 1 : 0; }
int kp_dec_cluster_bwd_supported(int Hd, int Ld, int input_feed, int T, int L) { return aocr::dec_cluster_bwd_supported(Hd, Ld, input_feed, T, L, kp_cus()) ? 1 : 0; }
size_t kp_dec_cluster_xbuf_bytes(int B) { return aocr::dec_cluster_xbuf_bytes(B); }
size_t kp_dec_cluster_bwd_xbuf_bytes(int B) { return aocr::dec_cluster_bwd_xbuf_bytes(B); }
size_t kp_dec_cluster_pbuf_bytes(int B) { return aocr::dec_cluster_pbuf_bytes(B); }
size_t kp_dec_cluster_xtab_bytes(int B) { return aocr::dec_cluster_xtab_bytes(B); }

int kp_dec_cluster_forward(hipStream_t s, const KpDecFwd* p) {
  if (p->B < 1 || p->L < 1 || p->epoch == 0 || p->epoch >= (1u << 20)) return KP_DEC_BAD_ARGS;
  if ((p->greedy || p->zx_tok) && (p->V < 1 || p->V > 40)) return KP_DEC_BAD_ARGS;
  if (p->greedy && (!p->tok0 || p->tok0_stride < p->L || !p->wo || !p->bo || !p->labels || !p->scores)) return KP_DEC_BAD_ARGS;
  if (!aocr::dec_cluster_supported(p->Hd, 2, 1, p->T, p->L, kp_cus())) return KP_DEC_UNSUPPORTED;
  if (!p->xbuf || p->xbuf_bytes < aocr::dec_cluster_xbuf_bytes(p->B)) return KP_DEC_XBUF_SMALL;
  if (p->greedy && (!p->pbuf || p->pbuf_bytes < aocr::dec_cluster_pbuf_bytes(p->B))) return KP_DEC_PBUF_SMALL;
  if (!p->xtab || p->xtab_bytes < aocr::dec_cluster_xtab_bytes(p->B)) return KP_DEC_XTAB_SMALL;
  if (!p->err || p->err_ints < 16 + 256 * 8 + 4096) return KP_DEC_ERR_SMALL;
  aocr::DecClFwdArgs a; a.B = p->B; a.T = p->T; a.L = p->L; a.epoch = p->epoch;
  a.w1i = H16(p->w1i); a.w1h = H16(p->w1h); a.w2i = H16(p->w2i); a.w2h = H16(p->w2h); a.wc = H16(p->wc);
  a.b2i = p->b2i; a.b2h = p->b2h; a.zx1 = p->zx1; a.ctxb = H16(p->ctxb); a.ctxa = H16(p->ctxa);
  for (int l = 0; l < 2; ++l) { a.cs[l] = p->cs[l]; a.hsb[l] = W16(p->hsb[l]); a.gates[l] = p->gates[l]; }
  a.a_all = p->a_all; a.out = p->out; a.cat_b = W16(p->cat_b); a.out_b = W16(p->out_b);
  a.xbuf = p->xbuf; a.xtab = p->xtab; a.err = p->err;
  a.tok0 = p->tok0; a.tok0_stride = p->tok0_stride; a.wo = p->wo; a.bo = p->bo; a.V = p->V; a.pbuf = p->pbuf; a.labels = p->labels; a.scores = p->scores;
  a.trie_mask = p->trie_mask; a.trie_base = p->trie_base; a.trie_child = p->trie_child;
  a.drop_h = drop_of(p->drop_h); a.drop_out = drop_of(p->drop_out); a.hm_b = W16(p->hm_b);
  a.zx_tok = p->zx_tok; a.zx_st = p->zx_st; a.zx_sb = p->zx_sb; a.sc_hist = p->sc_hist;
  aocr::dec_cluster_forward(s, a, p->greedy != 0);
  return (int)hipGetLastError();
}
int kp_dec_cluster_backward(hipStream_t s, const KpDecBwd* p) {
  if (p->B < 1 || p->L < 1 || p->epoch == 0 || p->epoch >= (1u << 20)) return KP_DEC_BAD_ARGS;
  if (!aocr::dec_cluster_bwd_supported(p->Hd, 2, 1, p->T, p->L, kp_cus())) return KP_DEC_UNSUPPORTED;
  if (!p->xbuf || p->xbuf_bytes < aocr::dec_cluster_bwd_xbuf_bytes(p->B)) return KP_DEC_XBUF_SMALL;
  if (!p->xtab || p->xtab_bytes < aocr::dec_cluster_xtab_bytes(p->B)) return KP_DEC_XTAB_SMALL;
  if (!p->err || p->err_ints < 16 + 256 * 8 + 4096) return KP_DEC_ERR_SMALL;
  aocr::DecClBwdArgs a; a.B = p->B; a.T = p->T; a.L = p->L; a.epoch = p->epoch;
  a.w2i_t = H16(p->w2i_t); a.w2h_t = H16(p->w2h_t); a.w1h_t = H16(p->w1h_t); a.w1f_t = H16(p->w1f_t); a.wc_t = H16(p->wc_t); a.wa_t = H16(p->wa_t);
  a.dout_proj = p->dout_proj; a.out = p->out; a.a_all = p->a_all; a.ctxb = H16(p->ctxb);
  for (int l = 0; l < 2; ++l) {
    a.cs[l] = p->cs[l]; a.gates[l] = p->gates[l]; a.dz[l] = p->dz[l]; a.dzb[l] = W16(p->dzb[l]); a.dc_st[l] = p->dc_st[l]; a.dh_rec[l] = p->dh_rec[l];
  }
  a.dpre = p->dpre; a.dpre_b = W16(p->dpre_b); a.dcat = p->dcat; a.ds_all = p->ds_all; a.dq = p->dq; a.dq_b = W16(p->dq_b); a.dfeed = p->dfeed;
  a.xbuf = p->xbuf; a.xtab = p->xtab; a.err = p->err; a.drop_h = drop_of(p->drop_h); a.drop_out = drop_of(p->drop_out);
  aocr::dec_cluster_backward(s, a);
  return (int)hipGetLastError();
}

// ---- beam search on the chain kernel (csrc/dec_chain.hip, the BEAM instantiations of dec_ch_fwd_kernel), for the beam tests of
// tests/test_decoder_seq_kernels_gpu.py.  f: what model.hip's decode function sets in the k > 1 branch (greedy, gates, out, the dropout and zx_tok fields are not read);
// a launch is dec_chain_beam_passes() kernels with consecutive epochs from f.epoch, each indexing pbuf / xtab by the group WITHIN the launch, so those two are
// sized -- as the model sizes them -- for max(B, 32 * dec_chain_beam_group_cap()) rows.  labels / scores are carried but not written: the model's back-trace fills them.
struct KpDecBeam { KpDecFwd f; int beam; int32_t* hist_tok; int32_t* hist_par; float* beam_scores; };

int kp_dec_chain_beam_supported(int B, int L, int k, int V) { return aocr::dec_chain_beam_supported(B, L, k, V) ? 1 : 0; }
int kp_dec_chain_beam_passes(int B, int L, int k) { return aocr::dec_chain_beam_passes(B, L, k); }
int kp_dec_chain_beam_group_cap() { return aocr::dec_chain_beam_group_cap(); }
int kp_dec_chain_beam_forward(hipStream_t s, const KpDecBeam* b) {
  const KpDecFwd* p = &b->f;
  if (p->V < 1 || !aocr::dec_chain_beam_supported(p->B, p->L, b->beam, p->V)) return KP_DEC_UNSUPPORTED;
  if (!aocr::dec_cluster_supported(p->Hd, 2, 1, p->T, p->L, kp_cus())) return KP_DEC_UNSUPPORTED;
  const unsigned passes = (unsigned)aocr::dec_chain_beam_passes(p->B, p->L, b->beam);
  if (p->epoch == 0 || p->epoch >= (1u << 20) || p->epoch + passes >= (1u << 20)) return KP_DEC_BAD_ARGS;
  if (!b->hist_tok || !b->hist_par || !b->beam_scores || (p->sc_hist && !p->a_all)) return KP_DEC_BAD_ARGS;      // (HIST stores the attention rows too)
  if (!p->tok0 || p->tok0_stride < p->L || !p->wo || !p->bo) return KP_DEC_BAD_ARGS;
  const int rows = std::max(p->B, 32 * aocr::dec_chain_beam_group_cap());
  if (!p->xbuf || p->xbuf_bytes < aocr::dec_cluster_xbuf_bytes(p->B)) return KP_DEC_XBUF_SMALL;
  if (!p->pbuf || p->pbuf_bytes < aocr::dec_cluster_pbuf_bytes(rows)) return KP_DEC_PBUF_SMALL;
  if (!p->xtab || p->xtab_bytes < aocr::dec_cluster_xtab_bytes(rows)) return KP_DEC_XTAB_SMALL;
  if (!p->err || p->err_ints < 16 + 256 * 8 + 4096) return KP_DEC_ERR_SMALL;
  aocr::DecClFwdArgs a; a.B = p->B; a.T = p->T; a.L = p->L; a.epoch = p->epoch;
  a.w1i = H16(p->w1i); a.w1h = H16(p->w1h); a.w2i = H16(p->w2i); a.w2h = H16(p->w2h); a.wc = H16(p->wc);
  a.b2i = p->b2i; a.b2h = p->b2h; a.zx1 = p->zx1; a.ctxb = H16(p->ctxb); a.ctxa = H16(p->ctxa);
  for (int l = 0; l < 2; ++l) { a.cs[l] = p->cs[l]; a.hsb[l] = W16(p->hsb[l]); a.gates[l] = nullptr; }
  a.a_all = p->a_all; a.sc_hist = p->sc_hist; a.out = p->out; a.cat_b = W16(p->cat_b); a.out_b = W16(p->out_b);
  a.xbuf = p->xbuf; a.xtab = p->xtab; a.err = p->err;
  a.tok0 = p->tok0; a.tok0_stride = p->tok0_stride; a.wo = p->wo; a.bo = p->bo; a.V = p->V; a.pbuf = p->pbuf; a.labels = p->labels; a.scores = p->scores;
  a.beam = b->beam; a.hist_tok = b->hist_tok; a.hist_par = b->hist_par; a.beam_scores = b->beam_scores;
  a.trie_mask = p->trie_mask; a.trie_base = p->trie_base; a.trie_child = p->trie_child;
  aocr::dec_chain_beam_forward(s, a);
  return (int)hipGetLastError();
}

}  // extern "C"
