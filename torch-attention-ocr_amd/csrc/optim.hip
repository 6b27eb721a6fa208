// optim.hip -- AdamW with decoupled weight decay on the flat parameter vector (include/aocr.h: aocr_adam_update), HBM-bound: a norm pass that reads
// w and g (8 bytes per parameter) and an update pass that reads w, g, m, v and writes w, m, v (28 bytes per parameter), with the per-group clip scales and
// the step bookkeeping in one small kernel between them.  Built with -ffp-contract=off (csrc/Makefile): tests/adam_ref.py restates the element arithmetic in
// numpy float32 operation for operation, so no product may be fused into a following sum; fp32 '/' and sqrtf stay the correctly rounded ones.
// All wave-width constants are 64 (gfx950).
#include "ops.h"

namespace aocr {

constexpr int ADAM_THREADS = 256;       // threads per workgroup of the two element passes
constexpr int ADAM_WGS_PER_CU = 8;      // their grid: this many workgroups per compute unit, grid-stride over the parameters (never sized from n) ...
constexpr int ADAM_MAX_WGS = 4096;      // ... and at most this many, which is what sizes the scratch block

// scratch: double part[10][ADAM_MAX_WGS] (row 2k: sum of w^2 of group k per workgroup, row 2k + 1: of g^2); float scal[8] = scale[5], c1, c2, unused
size_t adam_scratch_bytes() { return (size_t)10 * ADAM_MAX_WGS * sizeof(double) + 8 * sizeof(float); }

struct AdamOff { int64_t o[6]; };
// four consecutive floats at any 4-byte-aligned address: one global_load_dwordx4 / global_store_dwordx4 (gfx9 global memory instructions need dword
// alignment only).  The four arrays of a call are not aligned alike in general -- v sits n floats behind m, and n is odd for the model -- so the blocks are
// laid on the 16-byte grid of the PARAMETER vector (`phase`), which is also the grid of the gradient vector and of m for the model's buffers.
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// [b4, e4): the whole 16-byte blocks of group [beg, end); [beg, b4) and [e4, end) are its scalar head and tail (at most 3 elements each; an empty group
// or one inside a single block has b4 == e4)
__device__ __forceinline__ void adam_middle(int64_t beg, int64_t end, int phase, int64_t& b4, int64_t& e4) {
  b4 = min(end, beg + ((4 - (int)((phase + beg) & 3)) & 3));
  e4 = b4 + ((end - b4) & ~(int64_t)3);
}
// the edge element thread t < 8 of workgroup 0 owns: head element t, or tail element t - 4; -1: none
__device__ __forceinline__ int64_t adam_edge(int t, int64_t beg, int64_t end, int64_t b4, int64_t e4) {
  const int64_t i = t < 4 ? beg + t : e4 + (t - 4);
  return (t < 4 ? i < b4 : i < end) ? i : -1;
}

// pass 1: per workgroup and group, the sums of w^2 and g^2 in double (sgd_sumsq_kernel's scheme on a flat grid: no atomics, one slot per workgroup)
__global__ __launch_bounds__(ADAM_THREADS) void adam_sumsq_kernel(const float* __restrict__ p, const float* __restrict__ g, AdamOff go, int phase,
                                                                  double* __restrict__ part) {
  __shared__ double sh[10][ADAM_THREADS / 64];
  double acc[10];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int64_t beg = go.o[k], end = go.o[k + 1];
    int64_t b4, e4; adam_middle(beg, end, phase, b4, e4);
    double sp = 0, sg = 0;
    if (blockIdx.x == 0 && threadIdx.x < 8) {
      const int64_t i = adam_edge(threadIdx.x, beg, end, b4, e4);
      if (i >= 0) { const double a = p[i], b = g[i]; sp += a * a; sg += b * b; }
    }
    for (int64_t i = b4 + ((int64_t)blockIdx.x * ADAM_THREADS + threadIdx.x) * 4; i < e4; i += (int64_t)gridDim.x * ADAM_THREADS * 4) {
      const f32x4u a = *reinterpret_cast<const f32x4u*>(p + i), b = *reinterpret_cast<const f32x4u*>(g + i);
      sp += (double)a.x * a.x + (double)a.y * a.y + (double)a.z * a.z + (double)a.w * a.w;
      sg += (double)b.x * b.x + (double)b.y * b.y + (double)b.z * b.z + (double)b.w * b.w;
    }
    acc[2 * k] = sp; acc[2 * k + 1] = sg;
  }
#pragma unroll
  for (int j = 0; j < 10; ++j) {
    const double v = wave_sum_d(acc[j]);
    if ((threadIdx.x & 63) == 0) sh[j][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < 10) part[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = sh[threadIdx.x][0] + sh[threadIdx.x][1] + sh[threadIdx.x][2] + sh[threadIdx.x][3];
}

// between the passes, one wave per group: the fixed-order sum of the workgroups' partials, the norms and the clip scale; lane 0 of group 0 also keeps the
// books -- the 32-byte tail of the state {double p1, p2; int64 steps, reserved} is read and written by this one thread, a kernel boundary away from the
// element threads, which take c1 and c2 from scal[5], scal[6].  A non-zero skip word leaves the tail (and scal[5..6], which the update then does not read) alone.
__global__ __launch_bounds__(64) void adam_scale_kernel(const double* __restrict__ part, int nwg, float clip, float beta1, float beta2, char* tail,
                                                        const int* __restrict__ skip, float* __restrict__ scal, float* __restrict__ norms) {
  const int grp = blockIdx.x, lane = threadIdx.x;
  if (grp == 0 && lane == 0 && !(skip && *skip != 0)) {
    double* pp = reinterpret_cast<double*>(tail); long long* st = reinterpret_cast<long long*>(tail + 16);
    const long long steps = st[0];
    double p1 = steps == 0 ? 1.0 : pp[0], p2 = steps == 0 ? 1.0 : pp[1];        // all-zero state = a fresh optimizer
    p1 *= (double)beta1; p2 *= (double)beta2;                                   // running products beta^t, not pow
    pp[0] = p1; pp[1] = p2; st[0] = steps + 1;
    scal[5] = (float)(1.0 - p1); scal[6] = (float)(1.0 - p2);
  }
  double sp = 0, sg = 0;
  for (int i = lane; i < nwg; i += 64) { sp += part[(int64_t)(2 * grp) * nwg + i]; sg += part[(int64_t)(2 * grp + 1) * nwg + i]; }
  sp = wave_sum_d(sp); sg = wave_sum_d(sg);
  if (lane != 0) return;
  const double pn = sqrt(sp), gn = sqrt(sg);
  const float sc = (clip > 0.f && gn > (double)clip) ? (float)((double)clip / gn) : 1.f;
  scal[grp] = sc;
  if (norms) { norms[grp] = (float)pn; norms[5 + grp] = (float)gn; norms[10 + grp] = sc; }
}

struct AdamK { float lr, beta1, beta2, eps, wd; };
// one element, every operation rounded on its own (the order is the header's and tests/adam_ref.py's)
__device__ __forceinline__ void adam_elem(float& w, float g0, float& m, float& v, const AdamK& k, float omb1, float omb2, float sc, float c1, float c2) {
  const float g = g0 * sc;
  m = k.beta1 * m + omb1 * g;
  v = k.beta2 * v + omb2 * (g * g);
  const float u = (m / c1) / (sqrtf(v / c2) + k.eps);
  w = w - k.lr * (u + k.wd * w);
}

// pass 2: the update.  grads is read only.
__global__ __launch_bounds__(ADAM_THREADS) void adam_update_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                   float* __restrict__ v, AdamOff go, int phase, AdamK k,
                                                                   const float* __restrict__ scal, const int* __restrict__ skip) {
  if (skip && *skip != 0) return;           // nothing is written: not w, m, v (the tail: adam_scale_kernel)
  const float omb1 = 1.0f - k.beta1, omb2 = 1.0f - k.beta2, c1 = scal[5], c2 = scal[6];
#pragma unroll 1
  for (int grp = 0; grp < 5; ++grp) {
    const int64_t beg = go.o[grp], end = go.o[grp + 1];
    int64_t b4, e4; adam_middle(beg, end, phase, b4, e4);
    const float sc = scal[grp];
    if (blockIdx.x == 0 && threadIdx.x < 8) {
      const int64_t i = adam_edge(threadIdx.x, beg, end, b4, e4);
      if (i >= 0) { float w = p[i], mm = m[i], vv = v[i]; adam_elem(w, g[i], mm, vv, k, omb1, omb2, sc, c1, c2); p[i] = w; m[i] = mm; v[i] = vv; }
    }
    for (int64_t i = b4 + ((int64_t)blockIdx.x * ADAM_THREADS + threadIdx.x) * 4; i < e4; i += (int64_t)gridDim.x * ADAM_THREADS * 4) {
      f32x4u w = *reinterpret_cast<const f32x4u*>(p + i), mm = *reinterpret_cast<const f32x4u*>(m + i), vv = *reinterpret_cast<const f32x4u*>(v + i);
      const f32x4u gg = *reinterpret_cast<const f32x4u*>(g + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) { float wj = w[j], mj = mm[j], vj = vv[j]; adam_elem(wj, gg[j], mj, vj, k, omb1, omb2, sc, c1, c2); w[j] = wj; mm[j] = mj; vv[j] = vj; }
      *reinterpret_cast<f32x4u*>(p + i) = w; *reinterpret_cast<f32x4u*>(m + i) = mm; *reinterpret_cast<f32x4u*>(v + i) = vv;
    }
  }
}

void adam_update(hipStream_t s, float* params, const float* grads, void* state, const int64_t* group_off, const AdamHyper& h, const int* skip,
                 void* scratch, float* norms_out) {
  static const int cus = [] { int n = 0, dev = 0; (void)hipGetDevice(&dev); (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev); return n > 0 ? n : 256; }();
  const int nwg = cus * ADAM_WGS_PER_CU < ADAM_MAX_WGS ? cus * ADAM_WGS_PER_CU : ADAM_MAX_WGS;
  AdamOff go; for (int i = 0; i < 6; ++i) go.o[i] = group_off[i];
  const int64_t n = group_off[5];
  const int phase = (int)(((uintptr_t)params >> 2) & 3);
  double* part = (double*)scratch; float* scal = (float*)(part + 10 * ADAM_MAX_WGS);
  float* m = (float*)state; float* v = m + n; char* tail = (char*)state + 8 * n;
  const AdamK k = {h.lr, h.beta1, h.beta2, h.eps, h.wd};
  hipLaunchKernelGGL(adam_sumsq_kernel, dim3(nwg), dim3(ADAM_THREADS), 0, s, params, grads, go, phase, part);
  hipLaunchKernelGGL(adam_scale_kernel, dim3(5), dim3(64), 0, s, part, nwg, h.clip, h.beta1, h.beta2, tail, skip, scal, norms_out);
  hipLaunchKernelGGL(adam_update_kernel, dim3(nwg), dim3(ADAM_THREADS), 0, s, params, grads, m, v, go, phase, k, scal, skip);
}

}  // namespace aocr
