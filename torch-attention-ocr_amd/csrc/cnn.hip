// cnn.hip -- the CNN drivers: the per-step view of the layer table (cnn.h), one function per kind of launch, and the forward /
// backward passes as loops over the stages.  aocr_get_tensor and aocr_profile_kernel (capi.hip) use the same view and functions.
#include "cnn.h"

namespace aocr {

void cnn_stages(aocr_model* m, const Dims& d, CnnStage st[CNN_LAYERS + 1]) {
  for (int i = 2; i <= CNN_LAYERS; ++i) {
    CnnStage& s = st[i]; const CnnLayer& L = CNN[i]; const bool last = i == CNN_LAYERS;
    s.i = i; s.B = d.B;
    cnn_map_extent(d, i - 1, s.H, s.W); cnn_map_extent(d, i, s.Ho, s.Wo);
    s.rows = (int64_t)d.B * (s.H + 2 * L.pad - L.ks + 1) * (s.W + 2 * L.pad - L.ks + 1);
    s.x = m->A[i - 1]; s.xb = m->Ab[i - 1];
    s.y = last ? m->X : m->A[i]; s.yb = last ? m->Xb : m->Ab[i]; s.idx = L.pool ? m->idx[i] : nullptr; s.pre = L.bn ? m->Y[i] : nullptr;
    s.conv = &m->conv[i]; s.bn = L.bn ? &m->bn[i] : nullptr;
    s.wb = m->wb[i]; s.wtb = m->wtb[i]; s.wtf = m->wtf[i];
    s.below = i > 2 ? &st[i - 1] : nullptr;
    s.epi_bn = L.bn && !last; s.y16 = s.epi_bn ? &m->y16[i] : nullptr; s.tb_rows = last ? d.B : 0;
    s.dx16_ok = CNN[i - 1].bn || CNN[i - 1].pool == 2;
    s.slab = CNN_LAYERS - i;
    s.stats_chunks = s.dA16 = s.sums_chunks = 0;
  }
}

// bf16 mode: the pooled conv outputs exist only as bf16 shadows (every consumer -- next conv, filter gradient, ReLU mask of the
// un-pool -- reads the shadow; aocr_get_tensor materialises fp32 on demand); X exists as both
static float* fwd_y32(const aocr_model* m, const CnnStage& st) { return (m->bf16 && !st.tb_rows) ? nullptr : st.y; }

void cnn_conv1_fwd(aocr_model* m, const float* images, const Dims& d, bool route) {
  conv1_forward(m->s, images, m->conv[1].w, m->conv[1].b, m->bf16 ? nullptr : m->A[1], d.B, d.H, d.W, m->Ab[1], route ? m->route1 : nullptr);
}

// A pooled stage writes y (and idx); a BatchNorm stage writes `pre`.  epi_bn stages: with fold (after bn_eval_prepare) the evaluation-mode BatchNorm + ReLU
// run in the conv epilogue, which then writes only the bf16 shadow of y; else, in training, the epilogue may leave the BatchNorm's partial sums in bn_scratch
// (st.stats_chunks > 0) and `pre` as bf16 (*st.y16).
void cnn_conv_fwd(aocr_model* m, CnnStage& st, int training, bool fold, int profile_tag) {
  const ConvP& c = *st.conv; const BnP* const fb = fold ? st.bn : nullptr; const bool hand = st.epi_bn && !fold;
  st.stats_chunks = 0;
  conv_forward(m->s, m->bf16, st.x, c.w, c.b, !st.bn ? fwd_y32(m, st) : fold ? nullptr : st.pre, st.idx, st.B, st.H, st.W, c.cin, c.cout, c.ks, c.pad, !st.bn, CNN[st.i].pool,
               st.xb, st.wb, (st.bn && !fold) ? nullptr : st.yb, profile_tag, fb ? fb->save : nullptr, fb ? fb->w : nullptr, fb ? fb->b : nullptr,
               (hand && training) ? (double*)m->bn_scratch : nullptr, hand ? &st.stats_chunks : nullptr, hand ? st.y16 : nullptr);
}

void cnn_bn_fwd(aocr_model* m, const CnnStage& st, int training, int update_running, const BnSync* sync) {
  const BnP& b = *st.bn;
  bn_relu_forward(m->s, st.pre, fwd_y32(m, st), b.w, b.b, b.rm, b.rv, b.save, m->bn_scratch, st.rows, b.C, training, update_running, st.tb_rows, st.yb, sync,
                  st.stats_chunks, st.pre16() ? reinterpret_cast<const bf16_t*>(st.pre) : nullptr);
}

// d(conv output) of the stage is in dyb (bf16 mode) / G0 (fp32 mode)
void cnn_wgrad(aocr_model* m, const CnnStage& st, hipStream_t s, const bf16_t* dyb, int profile_tag, float* dw) {
  const ConvP& c = *st.conv;
  conv_backward_filter(s, m->bf16, st.x, m->G0, dw ? dw : c.dw, (m->bf16 || dw) ? nullptr : c.db, st.B, st.H, st.W, c.cin, c.cout, c.ks, c.pad, st.xb, dyb, m->wg_part,
                       m->wg_part_floats, profile_tag);
}

// d x into G1, for the elementwise backward pass of the stage below (its dA16 / sums_chunks).  Above a BatchNorm whose `pre` is fp32 the
// epilogue is offered that BatchNorm's backward sums (BnBwdFuse).
void cnn_dgrad(aocr_model* m, const CnnStage& st, const bf16_t* dyb) {
  const ConvP& c = *st.conv; const bool bf = m->bf16; CnnStage* const lo = st.below;
  const bool over_bn = lo && lo->bn;
  const BnBwdFuse fuse{over_bn ? lo->pre : nullptr, st.xb, over_bn ? lo->bn->save : nullptr, (double*)m->bn_scratch};
  conv_backward_data(m->s, bf, m->G0, c.w, m->G1, st.B, st.H, st.W, c.cin, c.cout, c.ks, c.pad, dyb, st.wtb, st.wtf, (bf && st.dx16_ok) ? &lo->dA16 : nullptr,
                     (over_bn && bf && !lo->pre16()) ? &fuse : nullptr, over_bn ? &lo->sums_chunks : nullptr);
}

// bf16 mode: both passes write only the bf16 gradient map dyb, take the ReLU mask from the bf16 output shadow and accumulate the conv's bias
// gradient through a partial slab; fp32 mode: the map goes to G0
void cnn_elem_bwd(aocr_model* m, CnnStage& st, bf16_t* dyb, ColsumJobs* defer, const BnSync* sync) {
  const bool bf = m->bf16; float* const dy32 = bf ? nullptr : m->G0;
  float* const dbias = bf ? st.conv->db : nullptr; float* const part = bf ? cnn_slab(m, st.slab) : nullptr;
  const bf16_t* const dA16 = st.dA16 ? reinterpret_cast<const bf16_t*>(m->G1) : nullptr;
  if (st.bn) {                                                   // (bn7: d X is time-major, Y7 batch-major)
    const BnP& b = *st.bn;
    bn_relu_backward(m->s, st.pre, st.y, st.tb_rows ? m->dX : m->G1, b.w, b.save, dy32, b.dw, b.db, m->bn_scratch, st.rows, b.C, st.tb_rows, dyb, st.yb, dbias, part,
                     sync, defer, st.pre16() ? reinterpret_cast<const bf16_t*>(st.pre) : nullptr, dA16, st.sums_chunks);
    st.sums_chunks = 0;
  } else {
    unpool_relu_backward(m->s, m->G1, st.y, st.idx, dy32, st.B, st.H, st.W, st.conv->cout, CNN[st.i].pool, dyb, dbias, part, st.yb, defer, dA16);
  }
}

void cnn_conv1_bwd(aocr_model* m, const float* images, const Dims& d, ColsumJobs* defer) {
  const ConvP& c = m->conv[1];
  conv1_backward(m->s, images, c.w, c.b, m->G1, c.dw, c.db, d.B, d.H, d.W,
                 cnn_gmax(d) >= (size_t)4096 * 640 ? cnn_slab(m, CNN_LAYERS - 1) : nullptr, defer,      // G0 is free here: use it as the partial slab
                 m->route1_valid && !knob::AOCR_CONV1_RECOMPUTE() ? m->route1 : nullptr);       // the pooling/ReLU decisions of conv1_forward instead of re-evaluating the layer
}

// ------------------------------------------------------------------------------------------------
// CNN forward, cnn.lua:9-45.  Output X is time-major (T,B,512) (= cnn_output:transpose(1,2), model.lua:288).
// ------------------------------------------------------------------------------------------------
static int bn_sync_allreduce(void* ctx, void* buf, int64_t count, int dtype, hipStream_t s) { return comm_allreduce((aocr_model*)ctx, buf, count, dtype, s, 1); }

void cnn_forward(aocr_model* m, const float* images, const Dims& d, int training, int update_running) {
  hipStream_t s = m->s; const bool bf = m->bf16;
  for (int& f : m->y16) f = 0;                                    // only a training conv forward below sets them again: the evaluation / folded branch leaves Y3 / Y5 untouched, never "bf16 from an older step"
  const BnSync bsync_v{bn_sync_allreduce, m}; const BnSync* bsync = (training && sync_bn_on(m)) ? &bsync_v : nullptr;
  if (bf && !m->shadow_host.empty()) {                          // every bf16 shadow of the step in one launch
    if (!m->shadow_pending) shadow_jobs(s, m->shadow_dev, (int)m->shadow_host.size(), m->shadow_tiles);      // (pending: step_prologue put it on the side stream)
  } else {
    refresh_rnn_shadows(m);
    for (int i = 2; i <= CNN_LAYERS; ++i) {                     // refresh the re-laid weight copies (weights change every step)
      if (bf) conv_weight_shadows(s, m->conv[i].w, m->wb[i], m->wtb[i], m->conv[i].cout, m->conv[i].ks * m->conv[i].ks, m->conv[i].cin);
      else conv_weight_transpose_f32(s, m->conv[i].w, m->wtf[i], m->conv[i].cout, m->conv[i].ks * m->conv[i].ks, m->conv[i].cin);
    }
  }
  prof_mark(m, AOCR_PROF_POOL_CONV1); cnn_conv1_fwd(m, images, d, training);
  m->route1_valid = training;                                   // conv1_backward takes the pooling/ReLU decisions from here instead of re-evaluating the layer
  if (m->shadow_pending && m->shadow2_pending) { hipStreamWaitEvent(s, m->shadow2_done, 0); m->shadow2_pending = false; }       // conv1 reads no shadow; conv2 reads its own taps (the first part of the table)
  else if (m->shadow_pending) { hipStreamWaitEvent(s, m->shadow_done, 0); m->shadow_pending = false; }
  // evaluation mode, bf16: BatchNorm + ReLU of conv3 / conv5 are a per-channel affine map -> folded into the conv epilogue, which then writes only
  // the bf16 shadow (no fp32 map, no apply pass); conv7's BatchNorm also transposes to (T, B) and stays a pass of its own
  const bool fold = bf && !training && !knob::AOCR_NO_BN_FOLD();
  CnnStage S[CNN_LAYERS + 1]; cnn_stages(m, d, S);
  for (int i = 2; i <= CNN_LAYERS; ++i) {
    CnnStage& st = S[i]; const bool folded = fold && st.epi_bn;
    if (folded) { prof_mark(m, AOCR_PROF_BN); bn_eval_prepare(s, st.bn->rm, st.bn->rv, st.bn->save, st.bn->C); }
    prof_mark(m, AOCR_PROF_CONV_FWD); cnn_conv_fwd(m, st, training, folded);
    if (st.bn && !folded) { prof_mark(m, AOCR_PROF_BN); cnn_bn_fwd(m, st, training, update_running, bsync); }
    if (i == 2 && m->shadow_pending) { hipStreamWaitEvent(s, m->shadow_done, 0); m->shadow_pending = false; }       // the rest of the table (conv3 .. conv7, the recurrent matrices): refreshed under conv2
  }
}

// the filter gradients of the CNN backward pass run on the side stream (cnn_backward; backward_all asks too: the hoisted recurrent weight gradients then need no
// join in front of the CNN backward pass -- the filter gradients queue behind them on the same stream)
bool cnn_wgrad_on_side(aocr_model* m) {
  auto evok = [](hipEvent_t& e) { return e || hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess; };
  return m->bf16 && m->G2b && !knob::AOCR_DBG_STOP_SET() && !m->prof_on && m->side && m->side_done && !knob::AOCR_NO_SIDE_WGRAD() && !knob::AOCR_NO_CNN_WGRAD_SIDE() &&
         evok(m->cw_map[0]) && evok(m->cw_map[1]) && evok(m->cw_done[0]) && evok(m->cw_done[1]) && evok(m->cw_main);
}

void cnn_backward(aocr_model* m, const float* images, const Dims& d) {
  hipStream_t s = m->s;
  const BnSync bsync_v{bn_sync_allreduce, m}; const BnSync* bsync = sync_bn_on(m) ? &bsync_v : nullptr;
  // Round 4: the filter gradients on the side stream.  A stage is E_k (BatchNorm backward / un-pool: HBM-bound, writes the gradient map d Y_k) ->
  // { filter gradient k, data gradient k } (both MFMA-bound, both read d Y_k) -> E_(k-1).  On one stream the elementwise passes (0.5 ms of the
  // backward pass at C3) run with the MFMA pipes idle; with the filter gradient of stage k on the (low-priority) side stream it runs beside the data
  // gradient k and E_(k-1).  d Y alternates between two bf16 buffers so that E_(k-1) can write the next map while the filter gradient k still reads
  // its own; an event per buffer keeps E_(k-2) from overwriting it before that filter gradient is done.  AOCR_NO_CNN_WGRAD_SIDE=1: one stream.
  bf16_t* Gb[2] = {m->G0b, m->G2b}; int gp = 0;
  const int stop = knob::AOCR_DBG_STOP();                  // debugging aid: leave the gradient map of a stage in place (tap "g0"): 1 = bn7's, 2 = conv6's un-pool's
  const bool ws = !stop && cnn_wgrad_on_side(m);
  hipStream_t sw = ws ? m->side : s;
  const bool wg_after = ws && knob::AOCR_CNN_WGRAD_AFTER_DGRAD();      // A/B: start the filter gradient of a stage behind its data gradient (beside the next elementwise pass only)
  if (!ws) Gb[1] = Gb[0];
  auto map_ready = [&]() { if (ws) { hipEventRecord(m->cw_map[gp], s); hipStreamWaitEvent(sw, m->cw_map[gp], 0); } };        // d Y_k (Gb[gp]) is complete: the side stream may read it
  auto wgrad_done = [&]() { if (ws) hipEventRecord(m->cw_done[gp], sw); };
  auto next_map = [&]() { if (ws) { gp ^= 1; hipStreamWaitEvent(s, m->cw_done[gp], 0); } };                                    // the next E writes Gb[gp]: the filter gradient that read it two stages ago is done
  // with the slabs apart (cnn_slab) their column sums are finished by TWO launches (before the bucket event, at the end) instead of eight dependent ~10 us dispatches
  ColsumJobs cj; cj.n = 0; cj.total = 0;
  ColsumJobs* defer = cnn_slabs_apart(m) ? &cj : nullptr;
  CnnStage S[CNN_LAYERS + 1]; cnn_stages(m, d, S);
  for (int i = CNN_LAYERS; i >= 2; --i) {
    CnnStage& st = S[i];
    if (i < CNN_LAYERS) next_map();
    prof_mark(m, st.bn ? AOCR_PROF_BN : AOCR_PROF_POOL_CONV1); cnn_elem_bwd(m, st, Gb[gp], defer, bsync);
    if ((stop == 1 && i == 7) || (stop == 2 && i == 6)) { if (defer) colsum_flush(s, cj); return; }
    auto D = [&]() { prof_mark(m, AOCR_PROF_CONV_DGRAD); cnn_dgrad(m, st, Gb[gp]); };
    if (wg_after) D();
    map_ready(); prof_mark(m, AOCR_PROF_CONV_WGRAD); cnn_wgrad(m, st, sw, Gb[gp]); wgrad_done();
    if (i == CNN_SPLIT) {
      if (defer) colsum_flush(s, cj);                               // conv7.b, conv6.b, conv5.b
      if (ws) { hipEventRecord(m->cw_main, s); hipStreamWaitEvent(sw, m->cw_main, 0); hipEventRecord(m->grad_ev[2], sw); }      // (behind the filter gradient of conv5 on the side stream AND the bias sums on this one)
      else hipEventRecord(m->grad_ev[2], s);                        // every CNN gradient from conv5.w upwards is complete
    }
    if (!wg_after) D();
  }
  prof_mark(m, AOCR_PROF_POOL_CONV1); cnn_conv1_bwd(m, images, d, defer);
  if (defer) colsum_flush(s, cj);                               // conv4.b, conv3.b, conv2.b, conv1.w, conv1.b
  if (ws) { hipEventRecord(m->side_done, sw); hipStreamWaitEvent(s, m->side_done, 0); }
}

}  // namespace aocr
