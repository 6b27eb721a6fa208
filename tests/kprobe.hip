// tests/libkprobe.so: extern "C" wrappers around the host launchers of the bf16-source conv / GEMM paths (csrc/ops.h), for
// tests/test_kernels_bf16_gpu.py.  Test infrastructure: no kernels of its own, not part of the product's C ABI (include/aocr.h).
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

}  // extern "C"
