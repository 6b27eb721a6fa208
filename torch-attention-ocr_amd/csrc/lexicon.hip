// lexicon.hip -- lexicon snapping (include/aocr.h: aocr_lexicon_nearest): for every recognised row, the word of a device-resident list
// at the smallest Levenshtein distance (string.levenshtein, utils.lua:55-94, unit costs), lowest index on ties.
//
// The distance is Myers' bit-vector algorithm in Hyyro's formulation for GLOBAL distance: the row cut at its first EOS (length m <= 64) is
// the pattern, one bit per pattern position; the lexicon word is the text.  Per text character the column of vertical differences (pv: +1,
// mv: -1) advances with ~15 integer operations, and the distance D[m][j] is tracked at bit m - 1.  Three things that must be right:
//   * m = 64: the tracked bit is bit 63.  Nothing shifts by m or builds (1 << m) - 1: bits above m - 1 hold garbage, and since carries
//     and left shifts only move information upwards they never reach bit m - 1 or below.
//   * m = 0: the distance is the word's length; the recurrence is not run (word_length).
//   * the horizontal carry-in is +1 (ph = (ph << 1) | 1): row 0 of the DP is 0, 1, 2, ... for global distance, not the 0s of approximate search.
// m <= 32 runs the same recurrence on 32-bit columns (half the instructions; the usual case: words are short).
//
// One workgroup (256 threads) serves one row and one slice of that row's word range: it builds the row's match masks peq[id] (bit t set
// <=> pattern[t] == id) once in LDS, then every lane streams words with 16-byte loads (the fixed stride makes neighbouring lanes read
// neighbouring rows) and keeps its best (distance, index) as ONE packed 64-bit key, distance in the high half: "smallest distance, then
// lowest index" is a plain unsigned minimum.  Lanes -> wave (shuffles) -> workgroup (LDS) -> row (per-slice keys in scratch, a second
// kernel).  A minimum does not depend on the order of its operands, so the result is independent of the slicing and bit-identical from
// run to run; no atomics.  No word is pruned: every word of the range is scored.
#include <algorithm>
#include "ops.h"

namespace aocr {

namespace {

constexpr int LEX_THREADS = 256;            // also the number of peq entries: thread v builds peq[v]
constexpr int LEX_SLICE_WORDS = 4096;       // words of a full slice: 16 per lane
constexpr int LEX_MAX_SLICES = 64;
constexpr uint64_t LEX_NONE = ~0ull;        // key of an empty range (a real key has distance <= 255 in its high half)

// one text character: eq = match mask of the character against the pattern, top = bit m - 1
template <typename T> __host__ __device__ __forceinline__ void myers_step(T eq, T top, T& pv, T& mv, int& score) {
  const T xv = eq | mv;
  const T xh = (((eq & pv) + pv) ^ pv) | eq;
  T ph = mv | ~(xh | pv);
  T mh = pv & xh;
  score += (ph & top) ? 1 : 0;
  score -= (mh & top) ? 1 : 0;
  ph = (ph << 1) | 1;                       // global distance: D[0][j] - D[0][j-1] = +1
  mh <<= 1;
  pv = mh | ~(xv | ph);
  mv = ph & xv;
}

__host__ __device__ __forceinline__ uint32_t word_byte(const uint4& q, int j) {
  const uint32_t d = (j >> 2) == 0 ? q.x : (j >> 2) == 1 ? q.y : (j >> 2) == 2 ? q.z : q.w;
  return (d >> (8 * (j & 3))) & 0xffu;
}

// distance of the pattern (length m in 1..8*sizeof(T), masks peq) to the word at w (chunks * 16 bytes, ids then zeros)
template <typename T> __host__ __device__ __forceinline__ int word_distance(const uint4* __restrict__ w, int chunks, const uint64_t* peq, int m) {
  T pv = ~(T)0, mv = 0;
  const T top = (T)1 << (m - 1);
  int score = m;
  bool live = true;
  for (int k = 0; k < chunks; ++k) {
    const uint4 q = w[k];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint32_t c = word_byte(q, j);
      live = live && c != 0;                // the word ends at its first 0
      if (live) myers_step<T>((T)peq[c], top, pv, mv, score);
    }
    if (!live) break;
  }
  return score;
}

// m = 0: the distance to the empty pattern is the number of ids of the word
__host__ __device__ __forceinline__ int word_length(const uint4* __restrict__ w, int chunks) {
  int n = 0;
  bool live = true;
  for (int k = 0; k < chunks; ++k) {
    const uint4 q = w[k];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      live = live && word_byte(q, j) != 0;
      n += live ? 1 : 0;
    }
    if (!live) break;
  }
  return n;
}

// MODE 0: m = 0; 1: 1 <= m <= 32; 2: 33 <= m <= 64.  Words w0 + tid, w0 + tid + 256, ... < w1 of this lane.
template <int MODE> __device__ __forceinline__ uint64_t scan_slice(const uint8_t* __restrict__ words, int stride, int64_t w0, int64_t w1,
                                                                   const uint64_t* peq, int m) {
  uint64_t best = LEX_NONE;
  const int chunks = stride >> 4;
  for (int64_t w = w0 + threadIdx.x; w < w1; w += LEX_THREADS) {
    const uint4* p = reinterpret_cast<const uint4*>(words + w * stride);
    const int d = MODE == 0 ? word_length(p, chunks) : MODE == 1 ? word_distance<uint32_t>(p, chunks, peq, m) : word_distance<uint64_t>(p, chunks, peq, m);
    const uint64_t key = ((uint64_t)(uint32_t)d << 32) | (uint32_t)w;
    best = key < best ? key : best;
  }
  return best;
}

__device__ __forceinline__ void write_nearest(uint64_t key, int32_t* index, int32_t* dist) {
  const bool none = key == LEX_NONE;
  *index = none ? -1 : (int32_t)(uint32_t)key;
  *dist = none ? -1 : (int32_t)(key >> 32);
}

__global__ __launch_bounds__(LEX_THREADS) void lexicon_nearest_kernel(const int32_t* __restrict__ labels, int L, const uint8_t* __restrict__ words,
                                                                      int n_words, int stride, const int32_t* __restrict__ row_begin, int slices,
                                                                      uint64_t* __restrict__ partial, int32_t* __restrict__ index,
                                                                      int32_t* __restrict__ dist) {
  static_assert(LEX_THREADS == 256, "thread v builds peq[v], v = 0..255");
  __shared__ uint64_t peq[256];
  __shared__ uint64_t wave_best[LEX_THREADS / 64];
  __shared__ int32_t pat[64];
  __shared__ int pat_len;
  const int tid = threadIdx.x, b = blockIdx.x / slices, sl = blockIdx.x % slices;
  if (tid < 64) {                                                // wave 0: the row, cut at its first EOS (lanes past L count as EOS)
    const int32_t v = tid < L ? labels[(int64_t)b * L + tid] : 3;
    pat[tid] = v;
    const unsigned long long eos = __ballot(v == 3);
    if (tid == 0) pat_len = eos ? __builtin_ctzll(eos) : 64;
  }
  __syncthreads();
  const int m = pat_len;
  uint64_t e = 0;
  for (int t = 0; t < m; ++t) e |= (uint64_t)(pat[t] == tid) << t;  // ids outside 1..255 set no bit of any entry that is read (peq[0] never is)
  peq[tid] = e;
  __syncthreads();

  int lo = 0, hi = n_words;
  if (row_begin) {
    lo = min(max(row_begin[b], 0), n_words);
    hi = min(max(row_begin[b + 1], lo), n_words);
  }
  const int64_t per = ((int64_t)(hi - lo) + slices - 1) / slices;
  const int64_t w0 = lo + (int64_t)sl * per, w1 = min((int64_t)hi, w0 + per);
  uint64_t best = m == 0 ? scan_slice<0>(words, stride, w0, w1, peq, m)
                : m <= 32 ? scan_slice<1>(words, stride, w0, w1, peq, m) : scan_slice<2>(words, stride, w0, w1, peq, m);

  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t ohi = __shfl_xor((uint32_t)(best >> 32), o, 64), olo = __shfl_xor((uint32_t)best, o, 64);
    const uint64_t other = ((uint64_t)ohi << 32) | olo;
    best = other < best ? other : best;
  }
  if ((tid & 63) == 0) wave_best[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < LEX_THREADS / 64; ++i) best = wave_best[i] < best ? wave_best[i] : best;
    if (slices > 1) partial[(int64_t)b * slices + sl] = best;
    else write_nearest(best, index + b, dist + b);
  }
}

// the minimum over a row's slices; one thread per row
__global__ void lexicon_reduce_kernel(const uint64_t* __restrict__ partial, int B, int slices, int32_t* __restrict__ index, int32_t* __restrict__ dist) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  uint64_t best = LEX_NONE;
  for (int i = 0; i < slices; ++i) {
    const uint64_t k = partial[(int64_t)b * slices + i];
    best = k < best ? k : best;
  }
  write_nearest(best, index + b, dist + b);
}

}  // namespace

int lexicon_slices(int n_words) { return std::min(std::max(cdiv(n_words, LEX_SLICE_WORDS), 1), LEX_MAX_SLICES); }

void lexicon_nearest(hipStream_t s, const int32_t* labels, int B, int L, const uint8_t* words, int n_words, int stride, const int32_t* row_begin,
                     void* scratch, int32_t* index, int32_t* dist) {
  if (B <= 0) return;
  if (n_words <= 0) {                                            // every range is empty
    fill_i32(s, index, -1, B); fill_i32(s, dist, -1, B);
    return;
  }
  const int slices = lexicon_slices(n_words);
  hipLaunchKernelGGL(lexicon_nearest_kernel, dim3(B * slices), dim3(LEX_THREADS), 0, s, labels, L, words, n_words, stride, row_begin, slices,
                     (uint64_t*)scratch, index, dist);
  if (slices > 1) hipLaunchKernelGGL(lexicon_reduce_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, (const uint64_t*)scratch, B, slices, index, dist);
}

}  // namespace aocr
