// resample.h -- image.scale's one-dimensional pass (torch/image generic/image.c: scaleLinear_rowcol; restated in oracle/data_oracle.py), what
// preprocess_kernel and crop_kernel (data.hip) and crop_slanted_kernel (slant.hip) share.  Every float operation is an explicitly rounded
// single-precision op in the order of the restatement: a translation unit that includes this is compiled with -ffp-contract=off (Makefile:
// FLAGS_data, FLAGS_slant), or hipcc contracts a*b+c into an FMA.
#pragma once
#include <hip/hip_runtime.h>

namespace aocr {

// element di of scaleLinear_rowcol(src[0..n), dst_len); F(i) yields src[i]
template <class F> __device__ __forceinline__ float scale_elem(const F& src, int n, int dst_len, int di) {
  if (dst_len == n) return src(di);
  if (dst_len > n) {
    if (n == 1) return src(0);
    if (di == dst_len - 1) return src(n - 1);
    const float scale = __fdiv_rn((float)(n - 1), (float)(dst_len - 1));
    const float sf = __fmul_rn((float)di, scale);
    const int si = (int)sf;
    const float fr = __fsub_rn(sf, (float)si);
    return __fadd_rn(__fmul_rn(__fsub_rn(1.0f, fr), src(si)), __fmul_rn(fr, src(si + 1)));
  }
  const float scale = __fdiv_rn((float)n, (float)dst_len);
  const float s0 = __fmul_rn((float)di, scale), s1 = __fmul_rn((float)(di + 1), scale);
  const int si0_i = (int)s0, si1_i = (int)s1;
  const float si0_f = __fsub_rn(s0, (float)si0_i), si1_f = __fsub_rn(s1, (float)si1_i);
  float acc = __fmul_rn(__fsub_rn(1.0f, si0_f), src(si0_i));
  float cnt = __fsub_rn(1.0f, si0_f);
  for (int si = si0_i + 1; si < si1_i; ++si) { acc = __fadd_rn(acc, src(si)); cnt = __fadd_rn(cnt, 1.0f); }
  if (si1_i < n) { acc = __fadd_rn(acc, __fmul_rn(si1_f, src(si1_i))); cnt = __fadd_rn(cnt, si1_f); }
  return __fdiv_rn(acc, cnt);
}

}  // namespace aocr
