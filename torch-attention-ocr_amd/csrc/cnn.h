// cnn.h -- the one description of the seven-layer CNN (cnn.lua:9-45): the static layer table, what follows from it (parameter
// offsets, map extents, BatchNorm state), the per-step view of layers 2..7 and one function per kind of launch (cnn.hip).
// The training step, the parity taps (aocr_get_tensor) and the kernel replays (aocr_profile_kernel) all run from these.
#pragma once
#include "model.h"

namespace aocr {

struct CnnLayer { int cin, cout, ks, pad, pool /* 0 / 1 = 2x2 / 2 = 2x1 (rows only) */, bn; };
constexpr int CNN_LAYERS = 7;
constexpr CnnLayer CNN[CNN_LAYERS + 1] = {{}, {1, 64, 3, 1, 1, 0}, {64, 128, 3, 1, 1, 0}, {128, 256, 3, 1, 0, 1}, {256, 256, 3, 1, 2, 0},
                                          {256, 512, 3, 1, 0, 1}, {512, 512, 3, 1, 2, 0}, {512, 512, 2, 0, 0, 1}};      // [1..7]

constexpr int64_t cnn_weight_floats(int i) { return (int64_t)CNN[i].cout * CNN[i].ks * CNN[i].ks * CNN[i].cin; }
// offset of cnn.conv<i>.w in the flat parameter / gradient vectors (build_layout's order: w, b, then the BatchNorm's w, b)
constexpr int64_t cnn_param_offset(int i) {
  int64_t off = 0;
  for (int j = 1; j < i; ++j) off += cnn_weight_floats(j) + CNN[j].cout * (CNN[j].bn ? 3 : 1);
  return off;
}
constexpr int CNN_SPLIT = 5;                                               // gradient bucket 2 is conv5 upwards, bucket 3 the rest (aocr_grad_buckets, grad_ev[2])
constexpr int64_t cnn_conv5_offset() { return cnn_param_offset(CNN_SPLIT); }
constexpr int64_t cnn_bn_state_floats() {                                  // running mean + variance of every BatchNorm
  int64_t n = 0;
  for (int i = 1; i <= CNN_LAYERS; ++i) if (CNN[i].bn) n += 2 * CNN[i].cout;
  return n;
}
// extents of layer i's output map after its pooling (i = 0: the image)
inline void cnn_map_extent(const Dims& d, int i, int& H, int& W) {
  H = d.H; W = d.W;
  for (int j = 1; j <= i; ++j) {
    H += 2 * CNN[j].pad - CNN[j].ks + 1; W += 2 * CNN[j].pad - CNN[j].ks + 1;
    if (CNN[j].pool) H /= 2;
    if (CNN[j].pool == 1) W /= 2;
  }
}
inline size_t cnn_map_elems(const Dims& d, int i) { int H, W; cnn_map_extent(d, i, H, W); return (size_t)d.B * H * W * CNN[i].cout; }
inline size_t cnn_gmax(const Dims& d) { int H, W; cnn_map_extent(d, 1, H, W); return (size_t)d.B * H * W * CNN[2].cout; }      // d(conv2's output before pooling): the largest gradient map

// Layer i (2..7) in one step: geometry, buffers, parameters, and the hand-overs between its launches.
struct CnnStage {
  int i, B;                       // layer number (CNN[i], m->conv[i], m->bn[i]); images
  int H, W, Ho, Wo;               // input map (= the conv's output before pooling, at pad 1) and output map after pooling
  int64_t rows;                   // B x pixels of the conv's output: the BatchNorm's rows
  float* x; bf16_t* xb;           // input map (layer i-1's output) and its bf16 shadow
  float* y; bf16_t* yb; uint8_t* idx;      // output map (pooled, or BatchNorm + ReLU; layer 7: X, time-major), shadow, arg-max of the pool
  float* pre;                     // BatchNorm layers: the conv's own output Y_i
  const ConvP* conv; const BnP* bn;        // bn == nullptr: conv + ReLU + pool
  bf16_t *wb, *wtb; float* wtf;   // weight shadows
  CnnStage* below;                // the stage that wrote x (nullptr: conv1)
  // --- what the table does not say in so many words
  bool epi_bn;                    // bn3 / bn5: the conv epilogue folds the evaluation-mode BatchNorm, or hands the training statistics over; conv7 writes Y7 and does neither
  int* y16;                       // epi_bn: "the conv left `pre` as bf16" (&m->y16[i]; a replay points it at a local), else nullptr
  int tb_rows;                    // bn7: B (its output is transposed to time-major), else 0
  bool dx16_ok;                   // the data gradient may leave d x as bf16: the pass that reads it (BatchNorm backward, (2,1) un-pool) takes bf16
  int slab;                       // partial-sum slab of the elementwise backward pass, in the order of the backward pass (cnn_slab)
  // --- hand-overs, written by one launch and read by the next
  int stats_chunks;               // conv forward -> BatchNorm forward: chunks of partial sums in bn_scratch (0: none)
  int dA16, sums_chunks;          // data gradient of layer i+1 -> this layer's elementwise backward: G1 holds bf16; BatchNorm backward sums in bn_scratch
  bool pre16() const { return y16 && *y16; }
};
void cnn_stages(aocr_model* m, const Dims& d, CnnStage st[CNN_LAYERS + 1]);      // fills st[2..7]

// bf16 mode: fp32 G0 is free during the backward pass, so the partial sums of the fused bias / conv1 gradients go there: slab k of eight
// when G0 holds eight and their column sums are deferred (cnn_backward), else its start
constexpr size_t CNN_SLAB = (size_t)4 << 20;                     // floats per slab: >= 2048 x 1024 (BatchNorm), 4096 x 640 (conv1)
inline bool cnn_slabs_apart(const aocr_model* m) { return m->bf16 && m->gmax >= 8 * CNN_SLAB && !knob::AOCR_NO_COLSUM_DEFER(); }
inline float* cnn_slab(const aocr_model* m, int k) { return cnn_slabs_apart(m) ? m->G0 + (size_t)k * CNN_SLAB : m->G0; }

// One function per kind of launch, on m->s unless a stream is given.  No profile marks, events or waits: those are the drivers'.
void cnn_conv1_fwd(aocr_model* m, const float* images, const Dims& d, bool route);
void cnn_conv_fwd(aocr_model* m, CnnStage& st, int training, bool fold, int profile_tag = 0);
void cnn_bn_fwd(aocr_model* m, const CnnStage& st, int training, int update_running, const BnSync* sync);
void cnn_wgrad(aocr_model* m, const CnnStage& st, hipStream_t s, const bf16_t* dyb, int profile_tag = 0, float* dw = nullptr /* null: the layer's gradient */);
void cnn_dgrad(aocr_model* m, const CnnStage& st, const bf16_t* dyb);
void cnn_elem_bwd(aocr_model* m, CnnStage& st, bf16_t* dyb, ColsumJobs* defer, const BnSync* sync);      // BatchNorm backward or un-pool: writes d(conv output) of the stage
void cnn_conv1_bwd(aocr_model* m, const float* images, const Dims& d, ColsumJobs* defer);

void cnn_forward(aocr_model* m, const float* images, const Dims& d, int training, int update_running);
bool cnn_wgrad_on_side(aocr_model* m);
void cnn_backward(aocr_model* m, const float* images, const Dims& d);

}  // namespace aocr
