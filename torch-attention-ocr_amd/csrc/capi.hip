// capi.hip -- the extern "C" surface declared in include/aocr.h.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include "cnn.h"

using namespace aocr;

static thread_local std::string g_err;
static int fail(const char* fmt, ...) {
  char buf[512]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  g_err = buf; return 1;
}
static int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail("%s: %s", what, hipGetErrorString(e));
  return 0;
}
#define REQUIRE(cond, ...) do { if (!(cond)) return fail(__VA_ARGS__); } while (0)

static int check_cfg(const aocr_config* c) {
  REQUIRE(c, "config is NULL");
  REQUIRE(c->batch_size >= 1 && c->img_h >= 32 && c->img_h % 16 == 0, "bad batch_size/img_h");
  REQUIRE(c->max_img_w >= 8, "max_img_w too small");
  REQUIRE(c->enc_hidden >= 16 && c->enc_hidden % 16 == 0, "enc_hidden must be a multiple of 16");
  REQUIRE(c->enc_layers >= 1 && c->enc_layers <= MAXL && c->dec_layers >= 1 && c->dec_layers <= MAXL, "layers must be 1..%d", MAXL);
  REQUIRE(c->vocab >= 4 && c->vocab <= LOGIT_LD, "vocab must be 4..%d", LOGIT_LD);
  REQUIRE(c->emb >= 1 && c->max_decoder_l >= 1 && c->max_beam >= 1, "bad emb/max_decoder_l/max_beam");
  REQUIRE(c->compute == AOCR_COMPUTE_F32 || c->compute == AOCR_COMPUTE_BF16, "bad compute type");
  return 0;
}

extern "C" {

const char* aocr_last_error(void) { return g_err.c_str(); }
int aocr_version(void) { return AOCR_VERSION; }

int aocr_param_counts(const aocr_config* cfg, int64_t counts[AOCR_NUM_GROUPS]) {
  if (check_cfg(cfg)) return 1;
  Layout L = build_layout(*cfg);
  for (int g = 0; g < AOCR_NUM_GROUPS; ++g) counts[g] = L.group_off[g + 1] - L.group_off[g];
  return 0;
}
int aocr_param_entry(const aocr_config* cfg, int32_t index, char name[64], int32_t* group, int64_t* offset, int32_t* ndim,
                     int64_t shape[4]) {
  if (check_cfg(cfg)) return -1;
  Layout L = build_layout(*cfg);
  if (index < 0 || index >= (int)L.e.size()) return 1;
  const ParamEntry& e = L.e[index];
  snprintf(name, 64, "%s", e.name.c_str()); *group = e.group; *offset = e.offset; *ndim = e.ndim;
  for (int i = 0; i < 4; ++i) shape[i] = e.shape[i];
  return 0;
}
int64_t aocr_bn_state_count(void) { return cnn_bn_state_floats(); }

static void bind_params(aocr_model* m) {
  auto find = [&](const std::string& n) -> int64_t {
    for (auto& e : m->layout.e) if (e.name == n) return e.offset;
    return -1;
  };
  float* bnst = m->bn_state; int bi = 0;
  for (int i = 1; i <= CNN_LAYERS; ++i) {
    char nm[64];
    ConvP& c = m->conv[i]; c.cin = CNN[i].cin; c.cout = CNN[i].cout; c.ks = CNN[i].ks; c.pad = CNN[i].pad;
    snprintf(nm, 64, "cnn.conv%d.w", i); int64_t o = find(nm); c.w = m->params + o; c.dw = m->grads + o;
    snprintf(nm, 64, "cnn.conv%d.b", i); o = find(nm); c.b = m->params + o; c.db = m->grads + o;
    if (CNN[i].bn) {
      BnP& b = m->bn[i]; b.C = c.cout;
      snprintf(nm, 64, "cnn.bn%d.w", i); o = find(nm); b.w = m->params + o; b.dw = m->grads + o;
      snprintf(nm, 64, "cnn.bn%d.b", i); o = find(nm); b.b = m->params + o; b.db = m->grads + o;
      b.rm = bnst; b.rv = bnst + b.C; bnst += 2 * b.C;
      b.save = m->bn_save + (size_t)bi * 1024; ++bi;
    }
  }
  auto lstm = [&](const char* prefix, LstmP* arr, int layers, int in0, int H) {
    for (int l = 1; l <= layers; ++l) {
      char nm[64]; LstmP& p = arr[l - 1]; p.in = l == 1 ? in0 : H; int64_t o;
      snprintf(nm, 64, "%s.l%d.i2h.w", prefix, l); o = find(nm); p.wi = m->params + o; p.dwi = m->grads + o;
      snprintf(nm, 64, "%s.l%d.i2h.b", prefix, l); o = find(nm); p.bi = m->params + o; p.dbi = m->grads + o;
      snprintf(nm, 64, "%s.l%d.h2h.w", prefix, l); o = find(nm); p.wh = m->params + o; p.dwh = m->grads + o;
      snprintf(nm, 64, "%s.l%d.h2h.b", prefix, l); o = find(nm); p.bh = m->params + o; p.dbh = m->grads + o;
      // recurrent-step views: the part of W_i2h that multiplies a hidden-size input (layer 1 of the decoder: the
      // input-feed columns [E, E+Hd)), and W_h2h
      const int skip = p.in - H;
      p.swi.w = p.wi + (skip > 0 ? skip : 0); p.swi.ld = p.in; p.swi.R = 4 * H; p.swi.C = H;
      if (in0 == 512 && l == 1) { p.swi.w = p.wi; p.swi.C = 512; }                  // encoder layer 1: the whole W_i2h (hoisted GEMMs)
      p.swh.w = p.wh; p.swh.ld = H; p.swh.R = 4 * H; p.swh.C = H;
    }
  };
  lstm("enc_fw", m->enc[0], m->Le, 512, m->He);
  lstm("enc_bw", m->enc[1], m->Le, 512, m->He);
  lstm("dec", m->dec, m->Ld, m->E + (m->cfg.input_feed ? m->Hd : 0), m->Hd);
  int64_t o = find("dec.lookup"); m->lookup = m->params + o; m->dlookup = m->grads + o;
  o = find("dec.attn.wa"); m->wa = m->params + o; m->dwa = m->grads + o;
  o = find("dec.attn.wc"); m->wc = m->params + o; m->dwc = m->grads + o;
  m->swa.w = m->wa; m->swa.ld = m->Hd; m->swa.R = m->Hd; m->swa.C = m->Hd;
  m->swc.w = m->wc; m->swc.ld = 2 * m->Hd; m->swc.R = m->Hd; m->swc.C = 2 * m->Hd;
  o = find("proj.w"); m->wo = m->params + o; m->dwo = m->grads + o;
  o = find("proj.b"); m->bo = m->params + o; m->dbo = m->grads + o;
}

static void init_model_fields(aocr_model* m, const aocr_config* cfg) {
  m->cfg = *cfg; m->bf16 = cfg->compute == AOCR_COMPUTE_BF16;
  m->He = cfg->enc_hidden; m->Hd = 2 * cfg->enc_hidden; m->Le = cfg->enc_layers; m->Ld = cfg->dec_layers;
  m->E = cfg->emb; m->V = cfg->vocab; m->last_valid = 0;
}

size_t aocr_workspace_bytes(const aocr_config* cfg) {
  if (check_cfg(cfg)) return 0;
  aocr_model* m = new (std::nothrow) aocr_model();
  if (!m) return 0;
  init_model_fields(m, cfg);
  size_t r = model_carve(m, nullptr, 0) == 0 ? m->ws_bytes : 0;
  delete m;
  return r;
}

int aocr_model_create(const aocr_config* cfg, float* params_dev, float* grads_dev, float* bn_state_dev, void* workspace_dev,
                      size_t workspace_bytes, void* stream, aocr_model** out) {
  if (check_cfg(cfg)) return 1;
  REQUIRE(params_dev && grads_dev && bn_state_dev && workspace_dev && out, "NULL pointer argument");
  REQUIRE(((uintptr_t)params_dev & 15) == 0 && ((uintptr_t)grads_dev & 15) == 0 && ((uintptr_t)workspace_dev & 255) == 0,
          "params/grads must be 16-byte and the workspace 256-byte aligned");
  aocr_model* m = new (std::nothrow) aocr_model();
  REQUIRE(m, "out of host memory");
  init_model_fields(m, cfg);
  m->s = (hipStream_t)stream; m->params = params_dev; m->grads = grads_dev; m->bn_state = bn_state_dev;
  m->layout = build_layout(*cfg);
  if (model_carve(m, workspace_dev, workspace_bytes) != 0) { delete m; return fail("workspace too small: need %zu bytes", aocr_workspace_bytes(cfg)); }
  bind_params(m);
  build_shadow_jobs(m);
  if (!m->shadow_host.empty() &&
      hipMemcpy(m->shadow_dev, m->shadow_host.data(), m->shadow_host.size() * sizeof(ShadowJob), hipMemcpyHostToDevice) != hipSuccess) {
    delete m; return fail("upload of the shadow job table failed");
  }
  if (m->cl_xbuf) {                                     // tags start at epoch 1: the exchange buffers must not hold a stale match
    hipMemsetAsync(m->cl_xbuf, 0, m->cl_xbytes, m->s); hipMemsetAsync(m->cl_pbuf, 0, m->cl_pbytes, m->s); hipMemsetAsync(m->cl_err, 0, 64, m->s);
    hipMemsetAsync(m->cl_xtab, 0, m->cl_tbytes, m->s);
    if (m->dc_xbuf) { hipMemsetAsync(m->dc_xbuf, 0, m->dc_xbytes, m->s); hipMemsetAsync(m->dc_xtab, 0, m->dc_tbytes, m->s); hipMemsetAsync(m->dc_bxbuf, 0, m->dc_bxbytes, m->s); }
  }
  for (int i = 0; i < 4; ++i)
  {
    const hipError_t e = hipEventCreateWithFlags(&m->grad_ev[i], hipEventDisableTiming);
    if (e != hipSuccess) { aocr_model_destroy(m); return fail("hipEventCreateWithFlags failed: %s", hipGetErrorString(e)); }
  }
  *out = m;
  return 0;
}
int aocr_model_destroy(aocr_model* m) {
  if (m) for (int i = 0; i < 4; ++i) if (m->grad_ev[i]) hipEventDestroy(m->grad_ev[i]);
  if (m && m->side) { hipStreamSynchronize(m->side); hipStreamDestroy(m->side); }
  if (m && m->side_go) hipEventDestroy(m->side_go);
  if (m && m->side_done) hipEventDestroy(m->side_done);
  if (m && m->side2_done) hipEventDestroy(m->side2_done);
  if (m && m->side2) hipStreamDestroy(m->side2);
  if (m) for (hipEvent_t e : {m->cw_map[0], m->cw_map[1], m->cw_done[0], m->cw_done[1], m->cw_main}) if (e) hipEventDestroy(e);
  if (m && m->tab_done) hipEventDestroy(m->tab_done);
  if (m && m->zero_done) hipEventDestroy(m->zero_done);
  if (m && m->shadow_done) hipEventDestroy(m->shadow_done);
  if (m && m->shadow2_done) hipEventDestroy(m->shadow2_done);
  if (m && m->q_go) hipEventDestroy(m->q_go);
  if (m && m->q_done) hipEventDestroy(m->q_done);
  if (m && m->enc_ev) hipEventDestroy(m->enc_ev);
  if (m) for (hipEvent_t e : m->prof_ev) hipEventDestroy(e);
  if (m) for (hipStream_t ls : m->lay_s) if (ls) { hipStreamSynchronize(ls); hipStreamDestroy(ls); }
  if (m) for (hipEvent_t e : m->lay_ev) hipEventDestroy(e);
  if (m) comm_destroy(m);
  delete m; return 0;
}
int aocr_comm_unique_id(char id[128]) {
  REQUIRE(id, "NULL argument");
  if (const char* e = comm_unique_id(id)) return fail("%s", e);
  return 0;
}
int aocr_comm_init_rank(aocr_model* m, const char id[128], int32_t nranks, int32_t rank, int32_t sync_bn) {
  REQUIRE(m && id && nranks >= 1 && rank >= 0 && rank < nranks, "bad arguments");
  REQUIRE(m->comm.provider == 0, "a communicator is already attached (aocr_comm_destroy first)");
  if (const char* e = comm_init_rccl(m, id, nranks, rank, sync_bn)) return fail("%s", e);
  return 0;
}
int aocr_comm_set_callback(aocr_model* m, aocr_allreduce_fn fn, void* user, int32_t nranks, int32_t sync_bn) {
  REQUIRE(m && fn && nranks >= 1, "bad arguments");
  REQUIRE(m->comm.provider == 0, "a communicator is already attached (aocr_comm_destroy first)");
  if (const char* e = comm_init_callback(m, fn, user, nranks, sync_bn)) return fail("%s", e);
  return 0;
}
int aocr_allreduce_grads(aocr_model* m, float* loss_dev) {
  REQUIRE(m, "NULL model");
  REQUIRE(m->comm.provider != 0, "no communicator attached (aocr_comm_init_rank / aocr_comm_set_callback)");
  REQUIRE(m->last_valid, "no train step has been enqueued yet");
  const int rc = comm_allreduce_grads(m, loss_dev);
  REQUIRE(rc == 0, rc == 2 ? "the all-reduce provider reported an error" : "stream / event error in the gradient exchange");
  return 0;
}
int aocr_comm_exposed_ms(aocr_model* m, float* ms) {
  REQUIRE(m && ms, "NULL argument");
  *ms = 0.f;
  if (!m->comm.timed) return 0;
  if (hipEventSynchronize(m->comm.wait1) != hipSuccess || hipEventElapsedTime(ms, m->comm.wait0, m->comm.wait1) != hipSuccess)
    return fail("aocr_comm_exposed_ms: %s", hipGetErrorString(hipGetLastError()));
  return 0;
}
int aocr_comm_destroy(aocr_model* m) { REQUIRE(m, "NULL model"); comm_destroy(m); return 0; }
int aocr_comm_info(aocr_model* m, int32_t* nranks, int32_t* sync_bn, int32_t* provider) {
  REQUIRE(m, "NULL model");
  if (nranks) *nranks = m->comm.provider ? m->comm.nranks : 1;
  if (sync_bn) *sync_bn = sync_bn_on(m) ? 1 : 0;
  if (provider) *provider = m->comm.provider;
  return 0;
}
int aocr_profile_enable(aocr_model* m, int32_t on) { REQUIRE(m, "NULL model"); m->prof_on = on != 0; m->prof_n = 0; return 0; }
int aocr_profile_read(aocr_model* m, float ms[AOCR_PROF_FAMILIES], int32_t* marks) {
  REQUIRE(m && ms, "NULL argument");
  for (int i = 0; i < AOCR_PROF_FAMILIES; ++i) ms[i] = 0.f;
  if (marks) *marks = (int32_t)m->prof_n;
  if (m->prof_n < 2) { m->prof_n = 0; return 0; }
  if (hipEventSynchronize(m->prof_ev[m->prof_n - 1]) != hipSuccess) return fail("hipEventSynchronize failed");
  for (size_t i = 0; i + 1 < m->prof_n; ++i) {
    const int tag = m->prof_tag[i];
    if (tag < 0) continue;                               // a closing mark: the gap to the next entry point is not kernel time
    float t = 0.f; if (hipEventElapsedTime(&t, m->prof_ev[i], m->prof_ev[i + 1]) == hipSuccess) ms[tag] += t;
  }
  m->prof_n = 0;
  return 0;
}
int aocr_model_set_stream(aocr_model* m, void* stream) { REQUIRE(m, "NULL model"); m->s = (hipStream_t)stream; return 0; }

static int step_dims(aocr_model* m, int32_t B, int32_t W, int32_t L, Dims& d) {
  REQUIRE(m, "NULL model");
  REQUIRE(B >= 1 && B <= m->cfg.batch_size, "B=%d outside 1..%d", B, m->cfg.batch_size);
  REQUIRE(W >= 8 && W <= m->cfg.max_img_w, "W=%d outside 8..%d", W, m->cfg.max_img_w);
  REQUIRE(L >= 1 && L <= m->cfg.max_decoder_l, "max_decoder_l (%d) < target_l (%d)!", m->cfg.max_decoder_l, L);   // model.lua:264
  REQUIRE(make_dims(m->cfg, B, W, L, d), "image too small for the CNN");
  return 0;
}

int aocr_cluster_status(aocr_model* m, int32_t* code) {
  REQUIRE(m && code, "NULL argument");
  *code = 0;
  if (!m->cl_err) return 0;
  int32_t w[16] = {0};           // word 0: a code no optimizer call has consumed yet (a decode call's, or feval without an update); CL_ERR_STICKY: the last code an optimizer call skipped its update on
  if (hipMemcpyAsync(w, m->cl_err, sizeof(w), hipMemcpyDeviceToHost, m->s) != hipSuccess || hipStreamSynchronize(m->s) != hipSuccess)
    return fail("aocr_cluster_status: %s", hipGetErrorString(hipGetLastError()));
  *code = w[CL_ERR_STICKY] != 0 ? w[CL_ERR_STICKY] : w[0];
  if (*code != 0) {
    hipMemsetAsync(m->cl_err, 0, sizeof(int32_t), m->s); hipMemsetAsync(m->cl_err + CL_ERR_LATCH, 0, 2 * sizeof(int32_t), m->s);      // read and clear: the next call reports the steps after this one
    // (the skipped step's move of the BatchNorm running statistics was taken back by the optimizer call that skipped the update --
    //  sgd_update_kernel / adadelta_kernel restore the snapshot of step_prologue -- so a repeat of the batch moves them exactly once,
    //  whenever the host polls)
  }
  return 0;
}

int aocr_set_dropout(aocr_model* m, double p, uint64_t seed, uint64_t train_step) {
  REQUIRE(m, "NULL model");
  REQUIRE(p >= 0.0 && p < 1.0, "dropout p=%g outside [0, 1)", p);
  m->drop_p = p; m->drop_seed = seed; m->drop_step = train_step;
  m->drop_thr = p > 0.0 ? (unsigned long long)ceil(p * 9007199254740992.0) : 0ull;       // keep <=> (r >> 11) >= p 2^53
  return 0;
}

int aocr_train_forward_backward(aocr_model* m, const float* images_dev, const int32_t* targets_dev, const int32_t* targets_eval_dev,
                                int32_t B, int32_t W, int32_t L, float grad_scale, float* loss_dev) {
  Dims d; if (step_dims(m, B, W, L, d)) return 1;
  REQUIRE(images_dev && targets_dev && targets_eval_dev, "NULL input");
  prof_mark(m, AOCR_PROF_OTHER);
  step_prologue(m, (size_t)m->layout.group_off[AOCR_NUM_GROUPS] * sizeof(float));      // model.lua:637-639 (zeroGradParameters) + the step's parameter-only work
  m->drop_on = m->drop_thr != 0;                                          // nn.Dropout is active in training() mode only (model.lua:284)
  cnn_forward(m, images_dev, d, 1, 1);
  encoder_forward(m, d);
  decoder_tf_forward(m, d, targets_dev, 1, L, true);
  loss_and_dlogits(m, d, targets_eval_dev, 1, L, grad_scale, true, loss_dev);
  backward_all(m, images_dev, targets_dev, d);
  m->drop_on = false;
  prof_mark(m, -1);
  m->last = d; m->last_valid = 1; m->last_images = images_dev; m->last_train = true; m->tab_valid = false;
  return check_launch("aocr_train_forward_backward");
}

int aocr_grad_buckets(const aocr_config* cfg, int64_t begin[AOCR_GRAD_BUCKETS], int64_t end[AOCR_GRAD_BUCKETS]) {
  if (check_cfg(cfg)) return 1;
  REQUIRE(begin && end, "NULL argument");
  const Layout l = build_layout(*cfg);
  const int64_t c5 = cnn_conv5_offset();
  begin[0] = l.group_off[3]; end[0] = l.group_off[AOCR_NUM_GROUPS];       // decoder + projector
  begin[1] = l.group_off[1]; end[1] = l.group_off[3];                     // both encoder directions
  begin[2] = c5;             end[2] = l.group_off[1];                     // CNN from conv5 upwards
  begin[3] = 0;              end[3] = c5;                                 // conv1 .. conv4 (+ bn3)
  return 0;
}
int aocr_stream_wait_grads(aocr_model* m, int32_t bucket, void* stream) {
  REQUIRE(m, "NULL model");
  REQUIRE(bucket >= 0 && bucket < AOCR_GRAD_BUCKETS, "bucket %d outside 0..%d", bucket, AOCR_GRAD_BUCKETS - 1);
  REQUIRE(m->last_valid, "no train step has been enqueued yet");
  if (hipStreamWaitEvent((hipStream_t)stream, m->grad_ev[bucket], 0) != hipSuccess) return fail("hipStreamWaitEvent failed");
  return 0;
}

int aocr_sgd_step(aocr_model* m, float lr, float clip, float* norms_dev) {
  REQUIRE(m, "NULL model");
  prof_mark(m, AOCR_PROF_SGD);
  sgd_clip_update(m->s, m->params, m->grads, m->layout.group_off, lr, clip, norms_dev, m->sgd_scratch, m->cl_err, m->bn_snap ? m->bn_state : nullptr, m->bn_snap, (int)aocr_bn_state_count());
  prof_mark(m, -1);
  return check_launch("aocr_sgd_step");
}

int aocr_adadelta_step(aocr_model* m, float rho, float eps, float weight_decay, float* state_dev) {
  REQUIRE(m && state_dev, "NULL argument");
  REQUIRE(rho >= 0.f && rho < 1.f && eps > 0.f, "rho=%g eps=%g out of range", rho, eps);
  const int64_t n = m->layout.group_off[AOCR_NUM_GROUPS];
  adadelta_update(m->s, m->params, m->grads, state_dev, state_dev + n, n, rho, eps, weight_decay, m->cl_err, m->bn_snap ? m->bn_state : nullptr, m->bn_snap, (int)aocr_bn_state_count());
  return check_launch("aocr_adadelta_step");
}

size_t aocr_adam_state_bytes(int64_t n) { return n < 0 ? 0 : (size_t)n * 8 + 32; }
size_t aocr_adam_scratch_bytes(void) { return adam_scratch_bytes(); }
static int check_adam_params(const aocr_adam_params* p) {
  REQUIRE(p, "NULL params");
  REQUIRE(std::isfinite(p->lr) && std::isfinite(p->beta1) && std::isfinite(p->beta2) && std::isfinite(p->eps) && std::isfinite(p->weight_decay) && std::isfinite(p->clip),
          "lr=%g beta1=%g beta2=%g eps=%g weight_decay=%g clip=%g: not finite", p->lr, p->beta1, p->beta2, p->eps, p->weight_decay, p->clip);
  REQUIRE(p->beta1 >= 0.f && p->beta1 < 1.f && p->beta2 >= 0.f && p->beta2 < 1.f, "beta1=%g beta2=%g outside [0, 1)", p->beta1, p->beta2);
  REQUIRE(p->eps > 0.f, "eps=%g must be > 0", p->eps);
  REQUIRE(p->lr >= 0.f && p->weight_decay >= 0.f && p->clip >= 0.f, "lr=%g weight_decay=%g clip=%g must be >= 0", p->lr, p->weight_decay, p->clip);
  REQUIRE(p->reserved[0] == 0 && p->reserved[1] == 0, "reserved words must be 0");
  return 0;
}
static int check_adam_state(const void* state_dev) {
  REQUIRE(state_dev, "NULL state");
  REQUIRE(((uintptr_t)state_dev & 7) == 0, "state_dev must be 8-byte aligned");
  return 0;
}
int aocr_adam_update(void* stream, float* params_dev, const float* grads_dev, void* state_dev, const int64_t group_off[6],
                     const aocr_adam_params* p, const int32_t* skip_dev, void* scratch_dev, float* norms_dev) {
  if (check_adam_params(p) || check_adam_state(state_dev)) return 1;
  REQUIRE(params_dev && grads_dev && group_off && scratch_dev, "NULL argument");
  REQUIRE(((uintptr_t)params_dev & 3) == 0 && ((uintptr_t)grads_dev & 3) == 0 && ((uintptr_t)scratch_dev & 7) == 0, "params / grads must be 4-byte aligned, scratch 8-byte aligned");
  REQUIRE(group_off[0] == 0, "group_off[0]=%lld must be 0", (long long)group_off[0]);
  for (int k = 0; k < AOCR_NUM_GROUPS; ++k) REQUIRE(group_off[k + 1] >= group_off[k], "group_off decreases at %d", k + 1);
  const AdamHyper h = {p->lr, p->beta1, p->beta2, p->eps, p->weight_decay, p->clip};
  adam_update((hipStream_t)stream, params_dev, grads_dev, state_dev, group_off, h, skip_dev, scratch_dev, norms_dev);
  return check_launch("aocr_adam_update");
}
int aocr_adam_step(aocr_model* m, const aocr_adam_params* p, void* state_dev, float* norms_dev) {
  REQUIRE(m, "NULL model");
  if (check_adam_params(p) || check_adam_state(state_dev)) return 1;
  // scratch: the BatchNorm layers' partial-sum block -- every kernel of the step that used it is in front of this call on the model's stream, and the
  // workspace keeps its size
  REQUIRE(bn_scratch_bytes(512) >= adam_scratch_bytes(), "the BatchNorm scratch block is smaller than aocr_adam_scratch_bytes()");
  prof_mark(m, AOCR_PROF_SGD);
  optim_latch_restore(m->s, m->cl_err, m->bn_snap ? m->bn_state : nullptr, m->bn_snap, (int)aocr_bn_state_count());
  const AdamHyper h = {p->lr, p->beta1, p->beta2, p->eps, p->weight_decay, p->clip};
  adam_update(m->s, m->params, m->grads, state_dev, m->layout.group_off, h, m->cl_err ? m->cl_err + CL_ERR_LATCH : nullptr, m->bn_scratch, norms_dev);
  prof_mark(m, -1);
  return check_launch("aocr_adam_step");
}

int aocr_forward_logits(aocr_model* m, const float* images_dev, const int32_t* targets_dev, const int32_t* targets_eval_dev,
                        int32_t B, int32_t W, int32_t L, int32_t training, float* logits_dev, float* loss_dev) {
  Dims d; if (step_dims(m, B, W, L, d)) return 1;
  REQUIRE(images_dev && targets_dev, "NULL input");
  m->tab_valid = false;                                                   // (the per-token table of an earlier call may be stale: the parameters may have moved)
  cnn_forward(m, images_dev, d, training, 0);
  encoder_forward(m, d);
  decoder_tf_forward(m, d, targets_dev, 1, L, false);
  if (targets_eval_dev) loss_and_dlogits(m, d, targets_eval_dev, 1, L, 0.f, false, loss_dev);
  if (logits_dev) copy2d(m->s, m->logits, LOGIT_LD, logits_dev, m->V, L * B, m->V);
  m->last = d; m->last_valid = 1; m->last_train = false;
  return check_launch("aocr_forward_logits");
}

__global__ void pad_targets_kernel(const int32_t* src, int32_t* dst, int B, int L, int Lt) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * Lt) return;
  int b = i / Lt, t = i - b * Lt;
  dst[i] = t < L ? src[b * L + t] : 1;                                    // model.lua:267-272: pad with PAD
}

int aocr_decode(aocr_model* m, const float* images_dev, const int32_t* targets_dev, const int32_t* targets_eval_dev, int32_t B,
                int32_t W, int32_t L, int32_t beam, int32_t* labels_dev, float* scores_dev, float* gold_scores_dev, float* loss_dev) {
  return aocr_decode_dict(m, images_dev, targets_dev, targets_eval_dev, B, W, L, beam, nullptr, labels_dev, scores_dev, gold_scores_dev,
                          loss_dev);
}
static int check_trie(const aocr_trie* t, int V) {
  REQUIRE(t->child_mask_dev && t->child_base_dev && (t->child_dev || t->n_edges == 0), "trie: NULL array");
  REQUIRE(t->n_nodes >= 1 && t->n_edges >= 0, "trie: n_nodes=%d n_edges=%d", t->n_nodes, t->n_edges);
  REQUIRE(V <= 64, "dictionary decoding needs target_vocab_size <= 64 (got %d)", V);
  return 0;
}
int aocr_decode_dict(aocr_model* m, const float* images_dev, const int32_t* targets_dev, const int32_t* targets_eval_dev, int32_t B,
                     int32_t W, int32_t L, int32_t beam, const aocr_trie* trie, int32_t* labels_dev, float* scores_dev,
                     float* gold_scores_dev, float* loss_dev) {
  Dims d; if (step_dims(m, B, W, L, d)) return 1;
  REQUIRE(images_dev && targets_dev && targets_eval_dev && labels_dev && scores_dev, "NULL argument");
  if (trie && check_trie(trie, m->V)) return 1;
  if (beam > m->V) beam = m->V;                                           // model.lua:229
  REQUIRE(beam >= 1 && beam <= m->cfg.max_beam, "beam=%d outside 1..%d", beam, m->cfg.max_beam);
  const int Lt = m->cfg.max_decoder_l;                                    // model.lua:273: always max_decoder_l steps (S8)
  hipLaunchKernelGGL(pad_targets_kernel, dim3(cdiv((int64_t)B * Lt, 256)), dim3(256), 0, m->s, targets_dev, m->tgt_pad, B, L, Lt);
  hipLaunchKernelGGL(pad_targets_kernel, dim3(cdiv((int64_t)B * Lt, 256)), dim3(256), 0, m->s, targets_eval_dev, m->tge_pad, B, L, Lt);
  d.L = Lt;
  prof_mark(m, AOCR_PROF_OTHER);
  m->tab_valid = false;                                                   // (a decode call keeps its weight shadows / token table in line: on the side stream they measured 2 % slower, 1.73 -> 1.76 ms per call)
  cnn_forward(m, images_dev, d, 0, 0);                                    // model.lua:280-281: evaluate()
  encoder_forward(m, d);
  prof_mark(m, AOCR_PROF_DECODE);
  decode_beam(m, d, m->tgt_pad, beam, labels_dev, scores_dev, trie);
  // gold pass, model.lua:589-627.  The reference runs it over all max_decoder_l steps of the PAD-filled target (model.lua:266-274); a step
  // whose targets are all PAD adds nothing to the loss (criterion weight 0, criterion.lua:4-5) nor to the gold scores (model.lua:614-618)
  // and no later code reads the decoder state, so the L steps the caller's targets span give identical outputs.
  d.L = L < Lt ? L : Lt;
  decoder_tf_forward(m, d, m->tgt_pad, 1, Lt, false);
  prof_mark(m, AOCR_PROF_OTHER);
  loss_and_dlogits(m, d, m->tge_pad, 1, Lt, 0.f, false, loss_dev);
  if (gold_scores_dev) gold_scores(m->s, m->nll_rows, gold_scores_dev, d.L, B);
  prof_mark(m, -1);
  m->last = d; m->last_valid = 1; m->last_train = false; m->tab_valid = false;
  return check_launch(trie ? "aocr_decode_dict" : "aocr_decode");
}

// Label-free recognition: the forward half of aocr_decode_dict without the gold pass.  GO (2) starts every row from tgt_pad, so that the search
// paths read their first tokens exactly as they do in a decode call; the optional outputs come from the search's own history (decode_beam).
int aocr_recognize(aocr_model* m, const float* images_dev, int32_t B, int32_t W, int32_t beam, const aocr_trie* trie, int32_t* labels_dev,
                   float* scores_dev, float* char_logp_dev, float* attn_dev) {
  REQUIRE(m, "NULL model");
  const int Lt = m->cfg.max_decoder_l;                                    // model.lua:273: always max_decoder_l steps (S8)
  Dims d; if (step_dims(m, B, W, Lt, d)) return 1;
  REQUIRE(images_dev && labels_dev && scores_dev, "NULL argument");
  if (trie && check_trie(trie, m->V)) return 1;
  if (beam > m->V) beam = m->V;                                           // model.lua:229
  REQUIRE(beam >= 1 && beam <= m->cfg.max_beam, "beam=%d outside 1..%d", beam, m->cfg.max_beam);
  const bool hist = char_logp_dev || attn_dev;
  fill_i32(m->s, m->tgt_pad, 2, (int64_t)B * Lt);                         // GO, model.lua:388 (the rest of the row is never read)
  prof_mark(m, AOCR_PROF_OTHER);
  m->tab_valid = false;
  cnn_forward(m, images_dev, d, 0, 0);                                    // model.lua:280-281: evaluate()
  encoder_forward(m, d);
  prof_mark(m, AOCR_PROF_DECODE);
  decode_beam(m, d, m->tgt_pad, beam, labels_dev, scores_dev, trie, hist ? m->attn_hist : nullptr, hist ? m->sc_hist : nullptr);
  if (hist) {
    // the greedy whole-sequence kernels select without a parent history (hist_par is then not written): k = 1 walks row b alone
    const bool greedy = beam == 1;
    recognize_gather(m->s, labels_dev, greedy ? nullptr : m->hist_par, greedy ? nullptr : m->beam_scores, m->sc_hist, m->attn_hist, char_logp_dev,
                     attn_dev, Lt, B, beam, d.T);
  }
  prof_mark(m, -1);
  m->ctxa_fresh = false;                                                  // (no gold pass consumes ctx W_a of this call)
  m->last = d; m->last_valid = 1; m->last_train = false; m->tab_valid = false;
  return check_launch("aocr_recognize");
}

int aocr_get_tensor(aocr_model* m, const char* name, const void** ptr_dev, int32_t* ndim, int64_t shape[4]) {
  REQUIRE(m && name && ptr_dev && ndim && shape, "NULL argument");
  REQUIRE(m->last_valid, "no step has run yet");
  const Dims& d = m->last; std::string n = name;
  for (int i = 0; i < 4; ++i) shape[i] = 1;
  CnnStage S[CNN_LAYERS + 1]; cnn_stages(m, d, S);
  const int li = n.empty() ? 0 : n.back() - '0';          // "conv<li>" / "idx<li>"
  const bool tap_conv = n.size() == 5 && n.compare(0, 4, "conv") == 0 && li >= 1 && li < CNN_LAYERS;
  const bool tap_idx = n.size() == 4 && n.compare(0, 3, "idx") == 0 && li >= 2 && li < CNN_LAYERS && CNN[li].pool;
  if (n == "feats") { *ptr_dev = m->X; *ndim = 3; shape[0] = d.T; shape[1] = d.B; shape[2] = 512; }
  else if (n == "dfeats") { *ptr_dev = m->dX; *ndim = 3; shape[0] = d.T; shape[1] = d.B; shape[2] = 512; }
  else if (n == "context") { *ptr_dev = m->context; *ndim = 3; shape[0] = d.B; shape[1] = d.T; shape[2] = m->Hd; }
  else if (n == "dcontext") { *ptr_dev = m->dctx; *ndim = 3; shape[0] = d.B; shape[1] = d.T; shape[2] = m->Hd; }
  else if (n == "logits") { *ptr_dev = m->logits; *ndim = 3; shape[0] = d.L; shape[1] = d.B; shape[2] = LOGIT_LD; }
  else if (n == "dlogits") { *ptr_dev = m->dlogits; *ndim = 3; shape[0] = d.L; shape[1] = d.B; shape[2] = LOGIT_LD; }      // (after a training step)
  else if (n == "dout_proj") { *ptr_dev = m->dout_proj; *ndim = 3; shape[0] = d.L; shape[1] = d.B; shape[2] = m->Hd; }
  else if (n == "outs") { *ptr_dev = m->out_all + (size_t)d.B * m->Hd; *ndim = 3; shape[0] = d.L; shape[1] = d.B; shape[2] = m->Hd; }
  else if (tap_conv) {                                    // conv1 .. conv6: the map layer li hands to layer li + 1 (bf16 mode: materialised from its shadow)
    const CnnStage& up = S[li + 1];
    if (m->bf16) bf16_to_f32(m->s, up.xb, up.x, (int64_t)cnn_map_elems(d, li));
    *ptr_dev = up.x; *ndim = 4; shape[0] = d.B; shape[1] = up.H; shape[2] = up.W; shape[3] = CNN[li].cout;
  }
  // parity aids: the max-pool DECISIONS of the forward pass (tests impose them on the fp64 oracle: tests/test_step_gpu.py)
  else if (tap_idx) { const CnnStage& st = S[li]; u8_to_f32(m->s, st.idx, m->G0, (int64_t)cnn_map_elems(d, li)); *ptr_dev = m->G0; *ndim = 4; shape[0] = d.B; shape[1] = st.Ho; shape[2] = st.Wo; shape[3] = CNN[li].cout; }
  else if (n == "enc_dz0" || n == "enc_dz1") {           // debugging aid: bf16 d z of the top encoder layer, direction 0 / 1
    const int dir = n == "enc_dz1"; const int64_t cnt = (int64_t)d.T * d.B * 4 * m->He;
    REQUIRE(m->edz_b[dir][m->Le - 1], "no bf16 d z in this mode");
    bf16_to_f32(m->s, m->edz_b[dir][m->Le - 1], m->G0, cnt);
    *ptr_dev = m->G0; *ndim = 3; shape[0] = d.T; shape[1] = d.B; shape[2] = 4 * m->He;
  }
  else if (n == "enc_cs0") { *ptr_dev = m->ecs[0][m->Le - 1]; *ndim = 3; shape[0] = d.T + 2; shape[1] = d.B; shape[2] = m->He; }
  else if (n == "enc_gates0") { *ptr_dev = m->egates[0][m->Le - 1]; *ndim = 3; shape[0] = d.T; shape[1] = d.B; shape[2] = 4 * m->He; }
  else if (n == "cl_err") { *ptr_dev = m->cl_err; *ndim = 1; shape[0] = 8; REQUIRE(m->cl_err, "no cluster kernels in this configuration"); }
  else if (n == "dc_stamps") { REQUIRE(m->dc_xtab, "no decoder cluster kernel in this configuration"); *ptr_dev = m->dc_xtab + (size_t)((d.B + 31) / 32) * 32; *ndim = 1; shape[0] = 32; }   // 16 x u64 cycle counters (AOCR_DC_STAMPS=1) viewed as 16 floats
  else if (n == "ds_all") { *ptr_dev = m->ds_all; *ndim = 3; shape[0] = d.L; shape[1] = d.B; shape[2] = d.T; }          // debugging aids: decoder BPTT intermediates
  else if (n == "dq_all") { *ptr_dev = m->dq_all; *ndim = 3; shape[0] = d.L; shape[1] = d.B; shape[2] = m->Hd; }
  else if (n == "dcat_all") { *ptr_dev = m->dcat_all; *ndim = 3; shape[0] = d.L; shape[1] = d.B; shape[2] = 2 * m->Hd; }
  else if (n == "dh_rec0" || n == "dh_rec1" || n == "dc_st0" || n == "dc_st1" || n == "dfeed0") {      // debugging aids: gradients of the decoder's initial state
    const int l = n.back() - '0'; *ptr_dev = n[1] == 'f' ? m->dfeed : (n[1] == 'h' ? m->dh_rec[l] : m->dc_st[l]); *ndim = 2; shape[0] = d.B; shape[1] = m->Hd; }
  else if (n == "dpre_all") { *ptr_dev = m->dpre_all; *ndim = 3; shape[0] = d.L; shape[1] = d.B; shape[2] = m->Hd; }
  else if (n == "dc_bstamps") { REQUIRE(m->dc_xtab, "no decoder cluster kernel in this configuration"); *ptr_dev = m->dc_xtab + (size_t)((d.B + 31) / 32) * 32 + 16; *ndim = 1; shape[0] = 32; }
  else if (n == "dc_times") { REQUIRE(m->cl_err, "no cluster kernels in this configuration"); *ptr_dev = m->cl_err + 16 + 2048; *ndim = 1; shape[0] = 32 * 4 * 16 * 2; }   // 32 members x 4 gathers x 16 x u64 (10 ns ticks)
  else if (n == "g0") {                                   // debugging aid (AOCR_DBG_STOP=1|2): the gradient map the CNN backward pass stopped at
    const int stop = knob::AOCR_DBG_STOP();
    const int64_t cnt = stop == 1 ? (int64_t)d.B * d.T * 512 : (int64_t)d.B * d.H4 * d.W2 * 512;
    if (m->bf16) bf16_to_f32(m->s, m->G0b, m->G0, cnt);
    *ptr_dev = m->G0; *ndim = 4; shape[0] = d.B; shape[1] = stop == 1 ? d.Ho7 : d.H4; shape[2] = stop == 1 ? d.Wo7 : d.W2; shape[3] = 512;
  }
  else return fail("unknown tensor '%s'", name);
  return 0;
}

int aocr_profile_kernel(aocr_model* m, int32_t which, int32_t iters, float* ms_per_launch, double* flops_per_launch) {
  REQUIRE(m && ms_per_launch && flops_per_launch, "NULL argument");
  REQUIRE(m->last_valid, "run a step first");
  REQUIRE(which >= 0 && which <= AOCR_PK_LAST, "unknown kernel id %d", which);
  REQUIRE(iters >= 1, "iters must be >= 1");
  REQUIRE(which < 2 || (m->bf16 && m->last_images && m->last_train), "the HBM-bound kernel ids replay the bf16 TRAINING step: run aocr_train_forward_backward in bf16 mode first");
  const Dims& d = m->last;
  const int64_t n5 = (int64_t)d.B * d.H4 * d.W2;            // pixels of the conv5 / conv6 maps (512 channels)
  // the replays write where the step writes: guard the buffers they assume
  REQUIRE((which != 1 && which != AOCR_PK_SPLITK) || (size_t)512 * 4608 <= m->gmax, "kernel id %d sums conv6's filter gradient (512 x 4608 floats) into the gradient-map scratch, which holds %zu floats in this configuration", which, m->gmax);
  REQUIRE((which != AOCR_PK_BN_FWD && which != AOCR_PK_BN_BWD && which != AOCR_PK_UNPOOL) || (n5 % 256 == 0 && n5 / 256 <= 512), "kernel id %d replays conv5's BatchNorm with the epilogue's 256-pixel statistics chunks: %lld pixels are not a multiple of 256 / more than 512 chunks", which, (long long)n5);
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  hipStream_t s = m->s; const int B = d.B;
  CnnStage S[CNN_LAYERS + 1]; cnn_stages(m, d, S);         // the step's own view and launch functions (cnn.h): a replay is the launch the step makes, partial-sum slabs (cnn_slab) included
  double bytes = 0.0;
  // bf16 data-gradient maps (conv_backward_data's dx16, round 4): what the step's BatchNorm backward / un-pool passes read when the switch is on
  // G1 as those two replays find it: conv6's data gradient in front of conv5's BatchNorm backward, conv7's in front of conv6's un-pool (cnn_backward's calls)
  const bool dx16 = which == AOCR_PK_BN_BWD ? conv_dgrad_bf16_out(B, d.H4, d.W2, 512, 512, 3, 1) : which == AOCR_PK_UNPOOL ? conv_dgrad_bf16_out(B, d.H6, d.W2, 512, 512, 2, 0) : false;
  S[5].dA16 = S[6].dA16 = dx16;
  // bn_scratch is shared by every BatchNorm of the step, forward and backward: conv5's statistics are put back by the step's own hand-over (untimed)
  if (which == AOCR_PK_BN_FWD) cnn_conv_fwd(m, S[5], 1, false);
  int y16 = 0; if (which == 0) S[3].y16 = S[5].y16 = &y16;   // the replay of a training conv forward leaves its flag here: m->y16[] stays as the step left it
  const double dab = dx16 ? 2.0 : 4.0;                    // bytes per element of d A / d(pooled)
  // ids >= 2: the bandwidth-bound kernels, each replayed on the buffers the last TRAINING step left, with the arguments cnn_forward /
  // cnn_backward / decoder_backward pass (bf16 mode).  Outputs land where the step puts them (activations, gradient maps, gradient
  // vector): the model's taps and gradients are UNDEFINED afterwards until the next step.  flops_per_launch returns ALGORITHMIC BYTES.
  auto run = [&]() {
    switch (which) {
    case 0:
      {
        const char* const pl = knob::AOCR_PROBE_LAYER();  // debugging aid (tools/debug/conv_probe.py): the tagged launch of conv3 / conv4 / conv5 forward instead, as cnn_forward makes it in training
        const int l = pl ? atoi(pl) : 0;
        cnn_conv_fwd(m, S[l >= 3 && l <= 5 ? l : 6], 1, false, 1);      // distinct symbol: TAG = 1
      }
      break;
    case 1:                                                 // conv6 filter gradient as backward_all launches it (split-K slabs + their sum), summed into scratch
      cnn_wgrad(m, S[6], s, m->G0b, 1, m->G1);
      break;
    case AOCR_PK_CONV1_FWD:                                 // R1 + R2: reads the image (fp32), writes the pooled 64-channel map as bf16
      cnn_conv1_fwd(m, m->last_images, d, m->route1_valid);
      bytes = (double)B * d.H * d.W * 4 + (double)B * d.H1 * d.W1 * 64 * 2 + (m->route1_valid ? (double)conv1_route_elems(B, d.H, d.W) * 2 : 0.0);
      break;
    case AOCR_PK_CONV1_BWD:                                 // reads the image and d(pooled map) (fp32, conv2's data gradient); writes 640 numbers
      cnn_conv1_bwd(m, m->last_images, d, nullptr);
      bytes = (double)B * d.H * d.W * 4 + (double)B * d.H1 * d.W1 * 64 * 4 + (m->route1_valid ? (double)conv1_route_elems(B, d.H, d.W) * 2 : 0.0);
      break;
    case AOCR_PK_BN_FWD:                                    // conv5's BatchNorm + ReLU as the step runs it: statistics from the conv epilogue -> finalize + ONE pass: fp32 y in, bf16 out
      cnn_bn_fwd(m, S[5], 1, 0, nullptr);
      bytes = (double)n5 * 512 * (4 + 2);
      break;
    case AOCR_PK_BN_BWD:                                    // conv5's BatchNorm backward: sums pass (x fp32, d A fp32, mask bf16) + apply pass (the same + bf16 d x out)
      cnn_elem_bwd(m, S[5], m->G0b, nullptr, nullptr);
      bytes = (double)n5 * 512 * ((4 + dab + 2) + (4 + dab + 2 + 2));
      break;
    case AOCR_PK_UNPOOL:                                    // (2,1) un-pool + ReLU backward of conv6: d(pooled) fp32 + arg-max (1 B) + pooled mask (bf16) in, bf16 gradient of the un-pooled map out
      cnn_elem_bwd(m, S[6], m->G0b, nullptr, nullptr);
      bytes = (double)B * d.H6 * d.W2 * 512 * (dab + 1 + 2) + (double)n5 * 512 * 2;
      break;
    case AOCR_PK_ATTN_DCTX:                                 // d(context) of all L steps in one pass (model.lua:652-653): a, d s (L,B,T), d c, q (L,B,Hd) in; (B,T,Hd) fp32 out
      attention_dctx(s, m->a_all, m->ds_all, m->dcat_all, 2 * m->Hd, m->q_all, m->dctx, d.L, B, d.T, m->Hd);
      bytes = (double)d.L * B * (2.0 * d.T + 2.0 * m->Hd) * 4 + (double)B * d.T * m->Hd * 4;
      break;
    case AOCR_PK_SPLITK:                                    // the sum of conv6's seven split-K slabs (512 x 4608 fp32 each) into the gradient
      {
        const int ksl = (int)std::min<size_t>(8, m->wg_part_floats / ((size_t)512 * 4608));       // 32 tiles of 256 x 288 on 256 units: 8 k ranges (conv_backward_filter, conv_wgrad_halo_kernel)
        if (ksl >= 1) splitk_reduce(s, m->wg_part, ksl, (size_t)512 * 4608, m->G1);
        bytes = (double)512 * 4608 * 4 * (ksl + 2);
      }
      break;
    }
  };
  run();
  hipEventRecord(e0, m->s);
  for (int i = 0; i < iters; ++i) run();
  hipEventRecord(e1, m->s);
  hipEventSynchronize(e1);
  float ms = 0.f; hipEventElapsedTime(&ms, e0, e1);
  hipEventDestroy(e0); hipEventDestroy(e1);
  *ms_per_launch = ms / iters;
  if (which == 0 && knob::AOCR_PROBE()) {
    unsigned long long pr[8] = {0}; kprobe_read(pr);
    if (knob::AOCR_PROBE_LAYER()) for (int k = 1; k >= 0; --k) if (pr[4 * k + 1]) fprintf(stderr, "[aocr] probe: workgroup %d of the tagged launch: start -> K loop %.1f us, K loop %.1f us (%llu cycles = %.2f GHz), whole workgroup (last store acknowledged) %.1f us\n", k ? 17 : 300, pr[4 * k + 2] / 100.0, pr[4 * k + 1] / 100.0, pr[4 * k], pr[4 * k] / (pr[4 * k + 1] * 10.0) , pr[4 * k + 3] / 100.0);
    for (int k = 0; k < 2; ++k) if (pr[4 * k + 1]) fprintf(stderr, "[aocr] probe (%s halo kernel, conv6 forward): K loop of one workgroup %llu shader cycles in %.1f us = %.2f GHz\n", k ? "4-wave" : "8-wave", pr[4 * k], pr[4 * k + 1] / 100.0, pr[4 * k] / (pr[4 * k + 1] * 10.0)), fprintf(stderr, "[aocr]   prologue %.1f us, whole workgroup %.1f us (stores acknowledged)\n", pr[4 * k + 2] / 100.0, pr[4 * k + 3] / 100.0);
  }
  *flops_per_launch = which < 2 ? 2.0 * (double)d.B * d.H4 * d.W2 * 512.0 * (9.0 * 512.0) : bytes;
  return check_launch("aocr_profile_kernel");
}

// ---------------------------------------------------------------------------------------------
// module-level entry points
// ---------------------------------------------------------------------------------------------
int aocr_gemm(void* stream, int32_t compute, const float* A_dev, int64_t lda, int32_t a_kmajor, const float* B_dev, int64_t ldb,
              int32_t b_kmajor, float* C_dev, int64_t ldc, int32_t M, int32_t N, int32_t K, const float* bias_dev, int32_t accumulate) {
  REQUIRE(A_dev && B_dev && C_dev && M >= 0 && N >= 0 && K >= 0, "bad gemm arguments");
  REQUIRE((accumulate & ~7) == 0, "unknown gemm flag bits %d", accumulate);
  const int fl = ((accumulate & AOCR_GEMM_ACCUMULATE) ? EP_ACCUM : 0) | ((accumulate & AOCR_GEMM_RELU) ? EP_RELU : 0) | ((accumulate & AOCR_GEMM_TANH) ? EP_TANH : 0);
  REQUIRE(!((fl & EP_ACCUM) && (fl & (EP_RELU | EP_TANH))), "an activation on an accumulating product is not a module of the path");
  int rc = gemm((hipStream_t)stream, compute == AOCR_COMPUTE_BF16, A_dev, lda, a_kmajor != 0, B_dev, ldb, b_kmajor != 0, C_dev, ldc,
                M, N, K, bias_dev, nullptr, fl);
  REQUIRE(rc == 0, "gemm: the (A column-major, B row-major-by-K) combination is not supported");
  return check_launch("aocr_gemm");
}
int aocr_pointwise(void* stream, int32_t op, const float* a_dev, const float* b_dev, float* y_dev, int64_t n) {
  REQUIRE(a_dev && y_dev && n >= 0 && op >= 0 && op <= 3 && (b_dev || op == AOCR_PW_RELU), "bad arguments");
  pointwise((hipStream_t)stream, op, a_dev, b_dev, y_dev, n);
  return check_launch("aocr_pointwise");
}
int aocr_lookup_forward(void* stream, const float* weight_dev, const int32_t* ids_dev, float* out_dev, int32_t n, int32_t E) {
  REQUIRE(weight_dev && ids_dev && out_dev && n >= 0 && E > 0, "bad arguments");
  embedding_gather((hipStream_t)stream, weight_dev, ids_dev, 0, 1, out_dev, 1, n, E);
  return check_launch("aocr_lookup_forward");
}
int aocr_lookup_backward(void* stream, const float* grad_out_dev, const int32_t* ids_dev, float* grad_weight_dev, int32_t n, int32_t E, int32_t V) {
  REQUIRE(grad_out_dev && ids_dev && grad_weight_dev && n >= 0 && E > 0 && E <= 256 && V > 0, "bad arguments");
  embedding_scatter_accum((hipStream_t)stream, grad_out_dev, ids_dev, 0, 1, grad_weight_dev, 1, n, E, V);
  return check_launch("aocr_lookup_backward");
}
int aocr_conv2d_forward(void* stream, int32_t compute, const float* x_dev, const float* w_dev, const float* bias_dev, float* y_dev,
                        uint8_t* idx_dev, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t ksize, int32_t pad,
                        int32_t relu, int32_t pool) {
  REQUIRE(x_dev && w_dev && y_dev, "NULL argument");
  REQUIRE(Cin % 16 == 0 && Cout % 16 == 0, "Cin and Cout must be multiples of 16 (the 1-channel first layer has its own entry point)");
  REQUIRE(pool >= 0 && pool <= 2 && (pool == 0 || idx_dev), "bad pool mode / missing idx");
  conv_forward((hipStream_t)stream, compute == AOCR_COMPUTE_BF16, x_dev, w_dev, bias_dev, y_dev, idx_dev, B, H, W, Cin, Cout, ksize, pad,
               relu, pool);
  return check_launch("aocr_conv2d_forward");
}
int aocr_conv2d_backward_data(void* stream, int32_t compute, const float* dy_dev, const float* w_dev, float* dx_dev, int32_t B, int32_t H,
                              int32_t W, int32_t Cin, int32_t Cout, int32_t ksize, int32_t pad) {
  REQUIRE(dy_dev && w_dev && dx_dev && Cin % 16 == 0 && Cout % 16 == 0, "bad arguments");
  conv_backward_data((hipStream_t)stream, compute == AOCR_COMPUTE_BF16, dy_dev, w_dev, dx_dev, B, H, W, Cin, Cout, ksize, pad);
  return check_launch("aocr_conv2d_backward_data");
}
int aocr_conv2d_backward_filter(void* stream, int32_t compute, const float* x_dev, const float* dy_dev, float* dw_dev, float* dbias_dev,
                                int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t ksize, int32_t pad) {
  REQUIRE(x_dev && dy_dev && dw_dev && Cin % 16 == 0 && Cout % 16 == 0, "bad arguments");
  conv_backward_filter((hipStream_t)stream, compute == AOCR_COMPUTE_BF16, x_dev, dy_dev, dw_dev, dbias_dev, B, H, W, Cin, Cout, ksize, pad);
  return check_launch("aocr_conv2d_backward_filter");
}
int aocr_unpool_relu_backward(void* stream, const float* dpooled_dev, const float* pooled_dev, const uint8_t* idx_dev, float* dy_dev,
                              int32_t B, int32_t Ho, int32_t Wo, int32_t C, int32_t pool) {
  REQUIRE(dpooled_dev && pooled_dev && idx_dev && dy_dev && (pool == 1 || pool == 2) && C % 4 == 0, "bad arguments");
  unpool_relu_backward((hipStream_t)stream, dpooled_dev, pooled_dev, idx_dev, dy_dev, B, Ho, Wo, C, pool);
  return check_launch("aocr_unpool_relu_backward");
}
int aocr_conv1_forward(void* stream, const float* x_dev, const float* w_dev, const float* bias_dev, float* y_dev, int32_t B, int32_t H,
                       int32_t W) {
  REQUIRE(x_dev && w_dev && bias_dev && y_dev, "NULL argument");
  conv1_forward((hipStream_t)stream, x_dev, w_dev, bias_dev, y_dev, B, H, W);
  return check_launch("aocr_conv1_forward");
}
int aocr_conv1_backward(void* stream, const float* x_dev, const float* w_dev, const float* bias_dev, const float* dy_pooled_dev,
                        float* dw_dev, float* dbias_dev, int32_t B, int32_t H, int32_t W) {
  REQUIRE(x_dev && w_dev && bias_dev && dy_pooled_dev && dw_dev && dbias_dev, "NULL argument");
  conv1_backward((hipStream_t)stream, x_dev, w_dev, bias_dev, dy_pooled_dev, dw_dev, dbias_dev, B, H, W);
  return check_launch("aocr_conv1_backward");
}
int aocr_batchnorm_relu_forward(void* stream, const float* x_dev, float* y_dev, const float* weight_dev, const float* bias_dev,
                                float* running_mean_dev, float* running_var_dev, float* save_dev, void* scratch_dev, int64_t rows,
                                int32_t C, int32_t training, int32_t update_running, int32_t tb_rows) {
  REQUIRE(x_dev && y_dev && weight_dev && bias_dev && running_mean_dev && running_var_dev && save_dev && scratch_dev, "NULL argument");
  REQUIRE(C % 4 == 0 && C <= 512, "C must be a multiple of 4 and <= 512");
  bn_relu_forward((hipStream_t)stream, x_dev, y_dev, weight_dev, bias_dev, running_mean_dev, running_var_dev, save_dev, scratch_dev, rows, C,
                  training, update_running, tb_rows);
  return check_launch("aocr_batchnorm_relu_forward");
}
int aocr_batchnorm_relu_backward(void* stream, const float* x_dev, const float* y_dev, const float* dA_dev, const float* weight_dev,
                                 const float* save_dev, float* dx_dev, float* dweight_dev, float* dbias_dev, void* scratch_dev,
                                 int64_t rows, int32_t C, int32_t tb_rows) {
  REQUIRE(x_dev && y_dev && dA_dev && weight_dev && save_dev && dx_dev && dweight_dev && dbias_dev && scratch_dev, "NULL argument");
  bn_relu_backward((hipStream_t)stream, x_dev, y_dev, dA_dev, weight_dev, save_dev, dx_dev, dweight_dev, dbias_dev, scratch_dev, rows, C,
                   tb_rows);
  return check_launch("aocr_batchnorm_relu_backward");
}
int aocr_lstm_cell_forward(void* stream, int32_t compute, const float* x_dev, int32_t in_size, const float* h_prev_dev,
                           const float* c_prev_dev, const float* w_i2h_dev, const float* b_i2h_dev, const float* w_h2h_dev,
                           const float* b_h2h_dev, float* c_dev, float* h_dev, float* gates_dev, int32_t B, int32_t H) {
  REQUIRE(x_dev && h_prev_dev && c_prev_dev && w_i2h_dev && b_i2h_dev && w_h2h_dev && b_h2h_dev && c_dev && h_dev, "NULL argument");
  REQUIRE(in_size % 16 == 0 && H % 16 == 0, "in_size and H must be multiples of 16");
  GatesFwdArgs z;
  z.a = make_loadk2(x_dev, in_size, in_size, h_prev_dev, H, H, B);
  z.b = make_loadk2(w_i2h_dev, in_size, in_size, w_h2h_dev, H, H, 4 * H);
  z.K = in_size + H;
  EpGatesFwd& e = z.ep; e.zx = nullptr; e.ldzx = 0; e.b1 = b_i2h_dev; e.b2 = b_h2h_dev; e.c_prev = c_prev_dev; e.ldcp = H;
  e.c_out = c_dev; e.ldc = H; e.h_out = h_dev; e.ldh = H; e.h_out2 = nullptr; e.ldh2 = 0; e.gates = gates_dev; e.ldg = 4 * H; e.M = B; e.H = H;
  launch_small_gates_fwd((hipStream_t)stream, compute == AOCR_COMPUTE_BF16, 1, &z, B, H);
  return check_launch("aocr_lstm_cell_forward");
}
int aocr_lstm_cell_forward_zx(void* stream, int32_t compute, const float* zx_dev, int64_t ldzx, const float* h_prev_dev, const float* c_prev_dev,
                              const float* w_h2h_dev, float* c_dev, float* h_dev, float* gates_dev, int32_t B, int32_t H) {
  REQUIRE(zx_dev && h_prev_dev && c_prev_dev && w_h2h_dev && c_dev && h_dev, "NULL argument");
  REQUIRE(H % 16 == 0 && ldzx >= 4 * (int64_t)H, "H must be a multiple of 16 and ldzx >= 4H");
  GatesFwdArgs z;
  z.a = make_loadk(h_prev_dev, H, B, H);
  z.b = make_loadk(w_h2h_dev, H, 4 * H, H);
  z.K = H;
  EpGatesFwd& e = z.ep; e.zx = zx_dev; e.ldzx = ldzx; e.b1 = nullptr; e.b2 = nullptr; e.c_prev = c_prev_dev; e.ldcp = H;
  e.c_out = c_dev; e.ldc = H; e.h_out = h_dev; e.ldh = H; e.h_out2 = nullptr; e.ldh2 = 0; e.gates = gates_dev; e.ldg = 4 * H; e.M = B; e.H = H;
  launch_small_gates_fwd((hipStream_t)stream, compute == AOCR_COMPUTE_BF16, 1, &z, B, H);
  return check_launch("aocr_lstm_cell_forward_zx");
}
int aocr_lstm_cell_backward(void* stream, const float* dc_dev, const float* dh_dev, const float* gates_dev, const float* c_prev_dev,
                            const float* c_dev, float* dz_dev, float* dc_prev_dev, int32_t B, int32_t H) {
  REQUIRE(dc_dev && dh_dev && gates_dev && c_prev_dev && c_dev && dz_dev && dc_prev_dev, "NULL argument");
  GatesBwdArgs z;
  z.a = make_loadk(dh_dev, H, B, 0); z.b = make_loadmn(dh_dev, H, H, 0); z.K = 0;     // no GEMM part: dh comes in through dh1
  EpGatesBwd& e = z.ep; e.dh1 = dh_dev; e.ld1 = H; e.dh2 = nullptr; e.ld2 = 0; e.dc_in = dc_dev; e.lddc = H; e.gates = gates_dev; e.ldg = 4 * H;
  e.c_prev = c_prev_dev; e.ldcp = H; e.c = c_dev; e.ldcc = H; e.dz = dz_dev; e.lddz = 4 * H; e.dc_out = dc_prev_dev; e.lddco = H; e.M = B; e.H = H;
  launch_small_gates_bwd((hipStream_t)stream, false, 1, &z, B, H);
  return check_launch("aocr_lstm_cell_backward");
}
int aocr_attention_forward(void* stream, const float* ctx_dev, const float* q_dev, float* a_dev, float* c_dev, int64_t ldc, int32_t B,
                           int32_t T, int32_t Hd) {
  REQUIRE(ctx_dev && q_dev && a_dev && c_dev && Hd % 4 == 0 && ldc % 4 == 0, "bad arguments");
  attention_forward((hipStream_t)stream, ctx_dev, q_dev, a_dev, c_dev, ldc, B, T, Hd, 1);
  return check_launch("aocr_attention_forward");
}
int aocr_attention_backward(void* stream, const float* ctx_dev, const float* q_dev, const float* a_dev, const float* dc_dev, int64_t lddc,
                            float* ds_dev, float* dq_dev, int32_t B, int32_t T, int32_t Hd) {
  REQUIRE(ctx_dev && a_dev && dc_dev && ds_dev && dq_dev && Hd % 4 == 0 && lddc % 4 == 0, "bad arguments");
  attention_backward((hipStream_t)stream, ctx_dev, q_dev, a_dev, dc_dev, lddc, ds_dev, dq_dev, B, T, Hd);
  return check_launch("aocr_attention_backward");
}
int aocr_logsoftmax_nll(void* stream, const float* logits_dev, int64_t ld, const int32_t* targets_dev, float* logp_dev, float* dlogits_dev,
                        float* nll_rows_dev, int64_t rows, int32_t V, float grad_scale) {
  REQUIRE(logits_dev && targets_dev && ld >= V, "bad arguments");
  logsoftmax_nll((hipStream_t)stream, logits_dev, ld, targets_dev, 0, 1, (int)rows, logp_dev, dlogits_dev, nll_rows_dev, rows, V, grad_scale);
  return check_launch("aocr_logsoftmax_nll");
}
int aocr_beam_select(void* stream, const float* logp_dev, const int32_t* prev_tok_dev, float* beam_scores_dev, int32_t* tokens_dev,
                     int32_t* parents_dev, int32_t B, int32_t kin, int32_t kout, int32_t V) {
  REQUIRE(logp_dev && beam_scores_dev && tokens_dev && parents_dev && kin >= 1 && kout >= 1 && kout <= kin * V, "bad arguments");
  beam_select((hipStream_t)stream, logp_dev, prev_tok_dev, beam_scores_dev, tokens_dev, parents_dev, B, kin, kout, V);
  return check_launch("aocr_beam_select");
}
int aocr_beam_select_dict(void* stream, const float* logp_dev, const int32_t* prev_tok_dev, float* beam_scores_dev, int32_t* tokens_dev,
                          int32_t* parents_dev, int32_t B, int32_t kin, int32_t kout, int32_t V, const aocr_trie* trie,
                          const int32_t* loc_in_dev, int32_t* loc_out_dev) {
  REQUIRE(logp_dev && beam_scores_dev && tokens_dev && parents_dev && kin >= 1 && kout >= 1 && kout <= kin * V, "bad arguments");
  REQUIRE(trie && loc_out_dev && (loc_in_dev || !prev_tok_dev) && loc_in_dev != loc_out_dev, "trie / node arrays missing or aliased");
  if (check_trie(trie, V)) return 1;
  TrieView tv{(const unsigned long long*)trie->child_mask_dev, trie->child_base_dev, trie->child_dev, loc_in_dev, loc_out_dev};
  beam_select((hipStream_t)stream, logp_dev, prev_tok_dev, beam_scores_dev, tokens_dev, parents_dev, B, kin, kout, V, nullptr, 0, &tv);
  return check_launch("aocr_beam_select_dict");
}
int aocr_edit_distance(void* stream, const int32_t* labels_dev, const int32_t* targets_dev, int32_t B, int32_t L, int32_t* dist_dev,
                       int32_t* target_len_dev) {
  REQUIRE(labels_dev && targets_dev && dist_dev, "NULL argument");
  REQUIRE(B >= 0 && L >= 1 && (size_t)(L + 1) * 256 <= 160 * 1024, "bad sizes: B=%d L=%d", B, L);
  if (B > 0) edit_distance((hipStream_t)stream, labels_dev, targets_dev, B, L, dist_dev, target_len_dev);
  return check_launch("aocr_edit_distance");
}

size_t aocr_lexicon_scratch_bytes(int32_t B, int32_t n_words) {
  if (B <= 0 || n_words <= 0) return 0;
  const int slices = lexicon_slices(n_words);
  return slices > 1 ? (size_t)B * slices * sizeof(uint64_t) : 0;           // one key per (row, slice); a single slice writes the result itself
}
int aocr_lexicon_nearest(void* stream, const int32_t* labels_dev, int32_t B, int32_t L, const aocr_lexicon* lex, const int32_t* row_begin_dev,
                         void* scratch_dev, int32_t* index_dev, int32_t* dist_dev) {
  REQUIRE(lex, "lexicon is NULL");
  REQUIRE(B >= 0 && L >= 1 && L <= 64, "bad sizes: B=%d L=%d (L must be 1..64)", B, L);
  REQUIRE(index_dev && dist_dev && (labels_dev || B == 0), "NULL argument");
  REQUIRE(lex->stride >= 16 && lex->stride <= 256 && lex->stride % 16 == 0, "bad stride %d: a multiple of 16 in 16..256", lex->stride);
  REQUIRE(lex->n_words >= 0 && (lex->n_words == 0 || lex->words_dev), "bad lexicon: n_words=%d words_dev=%p", lex->n_words, (const void*)lex->words_dev);
  REQUIRE(((uintptr_t)lex->words_dev & 15) == 0, "words_dev must be 16-byte aligned");
  REQUIRE((int64_t)B * lexicon_slices(lex->n_words) <= INT32_MAX, "B=%d rows against n_words=%d words: too many workgroups", B, lex->n_words);
  REQUIRE(scratch_dev || aocr_lexicon_scratch_bytes(B, lex->n_words) == 0, "scratch_dev is NULL: aocr_lexicon_scratch_bytes(%d, %d) bytes are needed",
          B, lex->n_words);
  REQUIRE(((uintptr_t)scratch_dev & 7) == 0, "scratch_dev must be 8-byte aligned");
  if (B == 0) return 0;
  lexicon_nearest((hipStream_t)stream, labels_dev, B, L, lex->words_dev, lex->n_words, lex->stride, row_begin_dev, scratch_dev, index_dev, dist_dev);
  return check_launch("aocr_lexicon_nearest");
}

int aocr_preprocess_lines(void* stream, const uint8_t* src_dev, const aocr_image_desc* desc_dev, int32_t n_images, int32_t out_h,
                          int32_t out_w, float* out_dev) {
  REQUIRE(src_dev && desc_dev && out_dev, "NULL argument");
  REQUIRE(n_images >= 0 && out_h >= 1 && out_w >= 1, "bad sizes: n_images=%d out_h=%d out_w=%d", n_images, out_h, out_w);
  preprocess_lines((hipStream_t)stream, src_dev, desc_dev, n_images, out_h, out_w, out_dev);
  return check_launch("aocr_preprocess_lines");
}

int aocr_augment_lines(void* stream, const float* in_dev, const aocr_warp* warp_dev, int32_t n_images, int32_t H, int32_t W, uint64_t seed,
                       uint64_t counter, float* out_dev) {
  REQUIRE(in_dev && warp_dev && out_dev, "NULL argument");
  REQUIRE(in_dev != out_dev, "in_dev and out_dev must not alias");
  REQUIRE(n_images >= 0 && H >= 1 && W >= 1 && (int64_t)H * W <= INT32_MAX, "bad sizes: n_images=%d H=%d W=%d", n_images, H, W);
  REQUIRE(n_images <= 65535, "n_images=%d: at most 65535 images per call", n_images);
  augment_lines((hipStream_t)stream, in_dev, warp_dev, n_images, H, W, seed, counter, out_dev);
  return check_launch("aocr_augment_lines");
}

int aocr_degrade_lines(void* stream, const float* in_dev, const aocr_degrade* rec_dev, int32_t n_images, int32_t H, int32_t W, uint64_t seed,
                       uint64_t counter, float* out_dev) {
  REQUIRE(in_dev && rec_dev && out_dev, "NULL argument");
  REQUIRE(in_dev != out_dev, "in_dev and out_dev must not alias");
  REQUIRE(n_images >= 0 && H >= 1 && W >= 1 && H <= 16384 && W <= 16384, "bad sizes: n_images=%d H=%d W=%d (H, W in 1..16384)", n_images, H, W);
  REQUIRE(n_images <= 65535, "n_images=%d: at most 65535 images per call", n_images);
  if (n_images == 0) return 0;
  degrade_lines((hipStream_t)stream, in_dev, rec_dev, n_images, H, W, seed, counter, out_dev);
  return check_launch("aocr_degrade_lines");
}

int aocr_synth_lines(void* stream, const aocr_lexicon* lex, const aocr_glyph_atlas* atlas, const aocr_synth_style* style_dev, int32_t n_images,
                     int32_t H, int32_t W, int32_t L, float* out_dev, int32_t* targets_dev, int32_t* targets_eval_dev) {
  REQUIRE(lex, "lexicon is NULL");
  REQUIRE(atlas, "atlas is NULL");
  REQUIRE(n_images >= 0 && H >= 1 && W >= 1 && L >= 1 && (int64_t)H * W <= INT32_MAX, "bad sizes: n_images=%d H=%d W=%d L=%d", n_images, H, W, L);
  REQUIRE(n_images <= 65535, "n_images=%d: at most 65535 images per call", n_images);
  REQUIRE(lex->stride >= 16 && lex->stride <= 256 && lex->stride % 16 == 0, "bad stride %d: a multiple of 16 in 16..256", lex->stride);
  REQUIRE(lex->n_words >= 0 && (lex->n_words == 0 || lex->words_dev), "bad lexicon: n_words=%d words_dev=%p", lex->n_words, (const void*)lex->words_dev);
  REQUIRE(((uintptr_t)lex->words_dev & 15) == 0, "words_dev must be 16-byte aligned");
  REQUIRE(atlas->n_faces >= 1 && atlas->n_glyphs >= 1 && atlas->n_glyphs <= 252 && atlas->gh >= 1 && atlas->gh <= 64 && atlas->gw >= 1 && atlas->gw <= 64,
          "bad atlas: n_faces=%d n_glyphs=%d (1..252) gh=%d gw=%d (1..64)", atlas->n_faces, atlas->n_glyphs, atlas->gh, atlas->gw);
  REQUIRE(atlas->pixels_dev && atlas->advance_dev, "bad atlas: pixels_dev or advance_dev is NULL");
  REQUIRE(style_dev && out_dev, "NULL argument");
  REQUIRE((targets_dev == nullptr) == (targets_eval_dev == nullptr), "targets_dev and targets_eval_dev must be given, or be NULL, together");
  if (n_images == 0) return 0;
  synth_lines((hipStream_t)stream, *lex, *atlas, style_dev, n_images, H, W, L, out_dev, targets_dev, targets_eval_dev);
  return check_launch("aocr_synth_lines");
}

// ---- the page stages: what every one of them checks ---------------------------------------------------------------------------------------

static bool page_size_ok(int64_t H, int64_t W) { return H >= 1 && W >= 1 && H <= 16384 && W <= 16384 && H * W <= ((int64_t)1 << 26); }

static int check_page(const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W) {
  REQUIRE(page_dev, "page_dev is NULL");
  REQUIRE(page_size_ok(H, W), "bad page size H=%d W=%d: 1..16384 each, H*W <= 2^26", H, W);
  REQUIRE(pitch >= W, "pitch=%lld is smaller than W=%d", (long long)pitch, W);
  return 0;
}

// for the aocr_*_scratch_bytes that take a page size only: they return 0 on failure
static bool scratch_size_ok(int32_t H, int32_t W) {
  if (!page_size_ok(H, W)) fail("bad sizes H=%d W=%d (1..16384 each, H*W <= 2^26)", H, W);
  return page_size_ok(H, W);
}

static int check_threshold(int32_t threshold) {
  REQUIRE(threshold >= -1 && threshold <= 254, "threshold=%d: 0..254, or -1 for Otsu", threshold);
  return 0;
}

// others: the call's other pointers that must not be NULL, reported together with scratch_dev
static int check_scratch(const void* scratch_dev, bool others) {
  REQUIRE(scratch_dev && others, "NULL argument");
  REQUIRE(((uintptr_t)scratch_dev & 15) == 0, "scratch_dev must be 16-byte aligned");
  return 0;
}

// the bytes of H rows of W elements, pitch elements apart; or of n bytes
struct Span { uintptr_t lo, hi; };
static Span span_rows(const void* p, int64_t pitch, int64_t H, int64_t W, size_t elem = 1) {
  return Span{(uintptr_t)p, (uintptr_t)p + ((uintptr_t)(H - 1) * pitch + W) * elem};
}
static Span span_bytes(const void* p, size_t n) { return Span{(uintptr_t)p, (uintptr_t)p + n}; }
static bool disjoint(Span a, Span b) { return a.hi <= b.lo || b.hi <= a.lo; }

// a stage that writes a few words: the scratch, the page and the words lie apart.  name_dev: the words' name in the messages
static int check_words(const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, const void* scratch_dev, size_t scratch_bytes,
                       const int32_t* words_dev, int n_words, const char* name_dev) {
  const Span page = span_rows(page_dev, pitch, H, W), scratch = span_bytes(scratch_dev, scratch_bytes);
  const Span words = span_bytes(words_dev, n_words * sizeof(int32_t));
  REQUIRE(disjoint(scratch, page), "scratch_dev overlaps the page");
  REQUIRE(disjoint(words, page), "%s overlaps the page", name_dev);
  REQUIRE(disjoint(words, scratch), "%s overlaps the scratch", name_dev);
  return 0;
}

// the output page of a stage, Ho x Wo (width: how the message names Wo).  between: the checks that the call reports after the pitch and
// before the overlap
static int check_out(const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, const uint8_t* out_dev, int64_t out_pitch, int32_t Ho, int32_t Wo,
                     const char* width = "W=", const std::function<int()>& between = nullptr) {
  REQUIRE(out_pitch >= Wo, "out_pitch=%lld is smaller than %s%d", (long long)out_pitch, width, Wo);
  if (between && between()) return 1;
  REQUIRE(disjoint(span_rows(out_dev, out_pitch, Ho, Wo), span_rows(page_dev, pitch, H, W)), "out_dev overlaps the page");
  return 0;
}

size_t aocr_segment_scratch_bytes(int32_t H, int32_t W, int32_t max_boxes) {
  if (!(page_size_ok(H, W) && max_boxes >= 1 && max_boxes <= 4096)) {
    fail("bad sizes H=%d W=%d (1..16384 each, H*W <= 2^26) max_boxes=%d (1..4096)", H, W, max_boxes);
    return 0;
  }
  return segment_scratch_bytes(H, W, max_boxes);
}

// what aocr_segment_page and aocr_segment_page_spaced check alike, in this order
static int check_segment(const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, const aocr_segment_params* params, const void* scratch_dev,
                         int32_t max_boxes, const aocr_box* boxes_dev, const int32_t* counts_dev) {
  if (check_page(page_dev, pitch, H, W)) return 1;
  if (check_scratch(scratch_dev, params && boxes_dev && counts_dev)) return 1;
  REQUIRE(max_boxes >= 1 && max_boxes <= 4096, "max_boxes=%d: 1..4096", max_boxes);
  if (check_threshold(params->threshold)) return 1;
  REQUIRE(params->min_row_ink >= 1 && params->min_line_h >= 1 && params->min_word_w >= 1, "min_row_ink=%d min_line_h=%d min_word_w=%d must be >= 1",
          params->min_row_ink, params->min_line_h, params->min_word_w);
  REQUIRE(params->merge_gap >= 0 && params->word_gap >= 0, "merge_gap=%d word_gap=%d must be >= 0", params->merge_gap, params->word_gap);
  REQUIRE(params->pad_x >= 0 && params->pad_y >= 0, "pad_x=%d pad_y=%d must be >= 0", params->pad_x, params->pad_y);
  return 0;
}

int aocr_segment_page(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, const aocr_segment_params* params,
                      void* scratch_dev, int32_t max_boxes, aocr_box* boxes_dev, int32_t counts_dev[4]) {
  if (check_segment(page_dev, pitch, H, W, params, scratch_dev, max_boxes, boxes_dev, counts_dev)) return 1;
  segment_page((hipStream_t)stream, page_dev, pitch, H, W, *params, scratch_dev, max_boxes, boxes_dev, counts_dev);
  return check_launch("aocr_segment_page");
}

size_t aocr_segment_spaced_scratch_bytes(int32_t H, int32_t W, int32_t max_boxes) {
  if (!(page_size_ok(H, W) && max_boxes >= 1 && max_boxes <= 4096)) {
    fail("bad sizes H=%d W=%d (1..16384 each, H*W <= 2^26) max_boxes=%d (1..4096)", H, W, max_boxes);
    return 0;
  }
  return segment_scratch_bytes(H, W, max_boxes);               // the estimate lives in LDS: the scratch of aocr_segment_page
}

int aocr_segment_page_spaced(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, const aocr_segment_params* params,
                             const aocr_spacing_params* spacing, void* scratch_dev, int32_t max_boxes, aocr_box* boxes_dev,
                             int32_t counts_dev[4], int32_t max_lines, int32_t* spacing_dev) {
  REQUIRE(spacing, "spacing is NULL");
  if (check_segment(page_dev, pitch, H, W, params, scratch_dev, max_boxes, boxes_dev, counts_dev)) return 1;
  REQUIRE(params->word_gap != 0, "word_gap=0 (one box per band) leaves nothing to estimate: call aocr_segment_page");
  REQUIRE(spacing->min_gaps >= 1, "min_gaps=%d must be >= 1", spacing->min_gaps);
  REQUIRE(1 <= spacing->lo_percent && spacing->lo_percent <= spacing->default_percent && spacing->default_percent <= spacing->hi_percent &&
              spacing->hi_percent <= 400,
          "lo_percent=%d default_percent=%d hi_percent=%d: 1 <= lo <= default <= hi <= 400", spacing->lo_percent, spacing->default_percent,
          spacing->hi_percent);
  REQUIRE(spacing->ratio_percent >= 100 && spacing->ratio_percent <= 100000, "ratio_percent=%d: 100..100000", spacing->ratio_percent);
  REQUIRE(spacing->reserved[0] == 0 && spacing->reserved[1] == 0 && spacing->reserved[2] == 0, "reserved words must be 0");
  REQUIRE(max_lines >= 0, "max_lines=%d must be >= 0", max_lines);
  REQUIRE(((uintptr_t)spacing_dev & 3) == 0, "spacing_dev must be 4-byte aligned");
  if (max_lines == 0) spacing_dev = nullptr;
  if (spacing_dev && check_words(page_dev, pitch, H, W, scratch_dev, segment_scratch_bytes(H, W, max_boxes), spacing_dev,
                                 8 * std::min(max_lines, (H + 1) / 2), "spacing_dev")) return 1;
  segment_page_spaced((hipStream_t)stream, page_dev, pitch, H, W, *params, *spacing, scratch_dev, max_boxes, boxes_dev, counts_dev, max_lines,
                      spacing_dev);
  return check_launch("aocr_segment_page_spaced");
}

int aocr_crop_lines(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, const aocr_box* boxes_dev,
                    const int32_t* count_dev, int32_t n_boxes, int32_t out_h, int32_t out_w, float* out_dev) {
  if (check_page(page_dev, pitch, H, W)) return 1;
  REQUIRE(n_boxes >= 0 && n_boxes <= 65535 && out_h >= 1 && out_w >= 1 && (int64_t)out_h * out_w <= INT32_MAX,
          "bad sizes: n_boxes=%d (0..65535) out_h=%d out_w=%d", n_boxes, out_h, out_w);
  if (n_boxes == 0) return 0;
  REQUIRE(boxes_dev && out_dev, "NULL argument");
  crop_lines((hipStream_t)stream, page_dev, pitch, H, W, boxes_dev, count_dev, n_boxes, out_h, out_w, out_dev);
  return check_launch("aocr_crop_lines");
}

static int check_skew_params(const aocr_skew_params* p) {
  REQUIRE(p, "params is NULL");
  if (check_threshold(p->threshold)) return 1;
  REQUIRE(p->step_q16 >= 1 && p->step_q16 <= 4096, "step_q16=%d: 1..4096", p->step_q16);
  REQUIRE(p->n_steps >= 0 && p->n_steps <= 256, "n_steps=%d: 0..256", p->n_steps);
  REQUIRE(p->n_steps * p->step_q16 <= 16384, "n_steps=%d * step_q16=%d exceeds 16384 (slope 0.25)", p->n_steps, p->step_q16);
  return 0;
}

size_t aocr_skew_scratch_bytes(int32_t H, int32_t W, int32_t n_steps) {
  if (!(page_size_ok(H, W) && n_steps >= 0 && n_steps <= 256)) {
    fail("bad sizes H=%d W=%d (1..16384 each, H*W <= 2^26) n_steps=%d (0..256)", H, W, n_steps);
    return 0;
  }
  return skew_scratch_bytes(H, W, n_steps);
}

int aocr_estimate_skew(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, const aocr_skew_params* params,
                       void* scratch_dev, int32_t skew_dev[4], uint64_t* scores_dev) {
  if (check_page(page_dev, pitch, H, W)) return 1;
  if (check_skew_params(params)) return 1;
  if (check_scratch(scratch_dev, skew_dev)) return 1;
  REQUIRE(((uintptr_t)scores_dev & 7) == 0, "scores_dev must be 8-byte aligned");
  estimate_skew((hipStream_t)stream, page_dev, pitch, H, W, *params, scratch_dev, skew_dev, scores_dev);
  return check_launch("aocr_estimate_skew");
}

int aocr_deskew_page(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, const int32_t* skew_dev, int32_t slope_q16,
                     int32_t fill, uint8_t* out_dev, int64_t out_pitch) {
  if (check_page(page_dev, pitch, H, W)) return 1;
  REQUIRE(out_dev, "out_dev is NULL");
  if (check_out(page_dev, pitch, H, W, out_dev, out_pitch, H, W, "W=", [&] { REQUIRE(fill >= 0 && fill <= 255, "fill=%d: 0..255", fill); return 0; }))
    return 1;
  deskew_page((hipStream_t)stream, page_dev, pitch, H, W, skew_dev, slope_q16, fill, out_dev, out_pitch);
  return check_launch("aocr_deskew_page");
}

size_t aocr_flatten_scratch_bytes(int32_t H, int32_t W, int32_t radius) {
  if (!(page_size_ok(H, W) && radius >= 1 && radius <= 127)) {
    fail("bad sizes H=%d W=%d (1..16384 each, H*W <= 2^26) radius=%d (1..127)", H, W, radius);
    return 0;
  }
  return flatten_scratch_bytes(H, W);
}

int aocr_flatten_page(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, const aocr_flatten_params* params,
                      void* scratch_dev, uint8_t* out_dev, int64_t out_pitch) {
  if (check_page(page_dev, pitch, H, W)) return 1;
  REQUIRE(params, "params is NULL");
  REQUIRE(params->radius >= 1 && params->radius <= 127, "radius=%d: 1..127", params->radius);
  REQUIRE(params->reserved[0] == 0 && params->reserved[1] == 0, "reserved words must be 0");
  if (check_scratch(scratch_dev, out_dev)) return 1;
  if (check_out(page_dev, pitch, H, W, out_dev, out_pitch, H, W)) return 1;
  flatten_page((hipStream_t)stream, page_dev, pitch, H, W, *params, scratch_dev, out_dev, out_pitch);
  return check_launch("aocr_flatten_page");
}

size_t aocr_binarize_scratch_bytes(int32_t H, int32_t W, int32_t radius) {
  if (!(page_size_ok(H, W) && radius >= 1 && radius <= 63)) {
    fail("bad sizes H=%d W=%d (1..16384 each, H*W <= 2^26) radius=%d (1..63)", H, W, radius);
    return 0;
  }
  return binarize_scratch_bytes(H, W, radius);
}

int aocr_binarize_page(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, const aocr_binarize_params* params,
                       void* scratch_dev, uint8_t* out_dev, int64_t out_pitch, int32_t counts_dev[4]) {
  if (check_page(page_dev, pitch, H, W)) return 1;
  REQUIRE(params, "params is NULL");
  REQUIRE(params->radius >= 1 && params->radius <= 63, "radius=%d: 1..63", params->radius);
  REQUIRE(params->k_q8 >= 0 && params->k_q8 <= 255, "k_q8=%d: 0..255", params->k_q8);
  REQUIRE(params->range >= 1 && params->range <= 255, "range=%d: 1..255", params->range);
  REQUIRE(params->reserved[0] == 0 && params->reserved[1] == 0 && params->reserved[2] == 0, "reserved words must be 0");
  if (check_scratch(scratch_dev, out_dev)) return 1;
  REQUIRE(((uintptr_t)counts_dev & 3) == 0, "counts_dev must be 4-byte aligned");
  if (check_out(page_dev, pitch, H, W, out_dev, out_pitch, H, W)) return 1;
  if (counts_dev) {
    const Span counts = span_bytes(counts_dev, 4 * sizeof(int32_t));
    REQUIRE(disjoint(counts, span_rows(page_dev, pitch, H, W)), "counts_dev overlaps the page");
    REQUIRE(disjoint(counts, span_rows(out_dev, out_pitch, H, W)), "counts_dev overlaps out_dev");
  }
  binarize_page((hipStream_t)stream, page_dev, pitch, H, W, *params, out_dev, out_pitch, counts_dev);
  return check_launch("aocr_binarize_page");
}

size_t aocr_integral_scratch_bytes(int32_t H, int32_t W) { return scratch_size_ok(H, W) ? integral_scratch_bytes(H, W) : 0; }

static int check_sat(const uint32_t* sat_dev, int64_t sat_pitch, int32_t H, int32_t W) {
  REQUIRE(sat_dev, "sat_dev is NULL");
  REQUIRE(page_size_ok(H, W), "bad page size H=%d W=%d: 1..16384 each, H*W <= 2^26", H, W);
  REQUIRE(sat_pitch >= (int64_t)W + 1, "sat_pitch=%lld is smaller than W+1=%d", (long long)sat_pitch, W + 1);
  REQUIRE(((uintptr_t)sat_dev & 3) == 0, "sat_dev must be 4-byte aligned");
  return 0;
}

int aocr_ink_integral(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, int32_t threshold, int32_t light_text,
                      void* scratch_dev, uint32_t* sat_dev, int64_t sat_pitch, int32_t info_dev[4]) {
  if (check_page(page_dev, pitch, H, W)) return 1;
  if (check_threshold(threshold)) return 1;
  if (check_scratch(scratch_dev, info_dev)) return 1;
  if (check_sat(sat_dev, sat_pitch, H, W)) return 1;
  const Span sat = span_rows(sat_dev, sat_pitch, H + 1, W + 1, sizeof(uint32_t));
  REQUIRE(disjoint(sat, span_rows(page_dev, pitch, H, W)), "sat_dev overlaps the page");
  REQUIRE(disjoint(sat, span_bytes(scratch_dev, integral_scratch_bytes(H, W))), "sat_dev overlaps the scratch");
  ink_integral((hipStream_t)stream, page_dev, pitch, H, W, threshold, light_text, scratch_dev, sat_dev, sat_pitch, info_dev);
  return check_launch("aocr_ink_integral");
}

size_t aocr_layout_scratch_bytes(int32_t H, int32_t W, int32_t max_blocks) {
  if (!(page_size_ok(H, W) && max_blocks >= 1 && max_blocks <= 1024)) {
    fail("bad sizes H=%d W=%d (1..16384 each, H*W <= 2^26) max_blocks=%d (1..1024)", H, W, max_blocks);
    return 0;
  }
  return layout_scratch_bytes(max_blocks);
}

int aocr_layout_blocks(void* stream, const uint32_t* sat_dev, int64_t sat_pitch, int32_t H, int32_t W, const aocr_layout_params* params,
                       void* scratch_dev, int32_t max_blocks, aocr_box* blocks_dev, int32_t counts_dev[4]) {
  if (check_sat(sat_dev, sat_pitch, H, W)) return 1;
  if (check_scratch(scratch_dev, params && blocks_dev && counts_dev)) return 1;
  REQUIRE(max_blocks >= 1 && max_blocks <= 1024, "max_blocks=%d: 1..1024", max_blocks);
  REQUIRE(params->min_ink >= 1 && params->gap_x >= 1 && params->gap_y >= 1, "min_ink=%d gap_x=%d gap_y=%d must be >= 1", params->min_ink,
          params->gap_x, params->gap_y);
  REQUIRE(params->max_depth >= 1 && params->max_depth <= 16, "max_depth=%d: 1..16", params->max_depth);
  REQUIRE(params->min_block_w >= 1 && params->min_block_h >= 1 && params->min_block_ink >= 1,
          "min_block_w=%d min_block_h=%d min_block_ink=%d must be >= 1", params->min_block_w, params->min_block_h, params->min_block_ink);
  REQUIRE(params->reserved == 0, "reserved word must be 0");
  REQUIRE(disjoint(span_rows(sat_dev, sat_pitch, H + 1, W + 1, sizeof(uint32_t)), span_bytes(scratch_dev, layout_scratch_bytes(max_blocks))),
          "sat_dev overlaps the scratch");
  layout_blocks((hipStream_t)stream, sat_dev, sat_pitch, H, W, *params, scratch_dev, max_blocks, blocks_dev, counts_dev);
  return check_launch("aocr_layout_blocks");
}

size_t aocr_components_scratch_bytes(int32_t H, int32_t W) { return scratch_size_ok(H, W) ? components_scratch_bytes(H, W) : 0; }

int aocr_label_components(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, int32_t threshold, int32_t light_text,
                          int32_t connectivity, void* scratch_dev, int32_t* labels_dev, int64_t labels_pitch, int32_t max_components,
                          aocr_box* comps_dev, int32_t info_dev[4]) {
  if (check_page(page_dev, pitch, H, W)) return 1;
  if (check_threshold(threshold)) return 1;
  REQUIRE(connectivity == 4 || connectivity == 8, "connectivity=%d: 4 or 8", connectivity);
  if (check_scratch(scratch_dev, labels_dev && info_dev)) return 1;
  REQUIRE(((uintptr_t)labels_dev & 3) == 0, "labels_dev must be 4-byte aligned");
  REQUIRE(labels_pitch >= W, "labels_pitch=%lld is smaller than W=%d", (long long)labels_pitch, W);
  REQUIRE(max_components >= 1 && max_components <= 65536, "max_components=%d: 1..65536", max_components);
  const Span labels = span_rows(labels_dev, labels_pitch, H, W, sizeof(int32_t));
  REQUIRE(disjoint(labels, span_rows(page_dev, pitch, H, W)), "labels_dev overlaps the page");
  REQUIRE(disjoint(labels, span_bytes(scratch_dev, components_scratch_bytes(H, W))), "labels_dev overlaps the scratch");
  label_components((hipStream_t)stream, page_dev, pitch, H, W, threshold, light_text, connectivity, scratch_dev, labels_dev, labels_pitch,
                   max_components, comps_dev, info_dev);
  return check_launch("aocr_label_components");
}

size_t aocr_clean_scratch_bytes(int32_t H, int32_t W) { return scratch_size_ok(H, W) ? clean_scratch_bytes(H, W) : 0; }

int aocr_clean_page(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, const aocr_clean_params* params,
                    void* scratch_dev, uint8_t* out_dev, int64_t out_pitch, int32_t counts_dev[8]) {
  if (check_page(page_dev, pitch, H, W)) return 1;
  REQUIRE(params, "params is NULL");
  if (check_threshold(params->threshold)) return 1;
  REQUIRE(params->connectivity == 4 || params->connectivity == 8, "connectivity=%d: 4 or 8", params->connectivity);
  REQUIRE(params->min_area >= 1, "min_area=%d must be >= 1", params->min_area);
  REQUIRE(params->max_w >= 0 && params->max_h >= 0, "max_w=%d max_h=%d must be >= 0", params->max_w, params->max_h);
  REQUIRE(params->reserved[0] == 0 && params->reserved[1] == 0, "reserved words must be 0");
  if (check_scratch(scratch_dev, out_dev && counts_dev)) return 1;
  REQUIRE(((uintptr_t)counts_dev & 3) == 0, "counts_dev must be 4-byte aligned");
  if (check_out(page_dev, pitch, H, W, out_dev, out_pitch, H, W)) return 1;
  REQUIRE(disjoint(span_rows(out_dev, out_pitch, H, W), span_bytes(scratch_dev, clean_scratch_bytes(H, W))), "out_dev overlaps the scratch");
  clean_page((hipStream_t)stream, page_dev, pitch, H, W, *params, scratch_dev, out_dev, out_pitch, counts_dev);
  return check_launch("aocr_clean_page");
}

size_t aocr_rules_scratch_bytes(int32_t H, int32_t W) { return scratch_size_ok(H, W) ? rules_scratch_bytes(H, W) : 0; }

int aocr_remove_rules(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, const aocr_rule_params* params,
                      void* scratch_dev, uint8_t* out_dev, int64_t out_pitch, int32_t counts_dev[8]) {
  if (check_page(page_dev, pitch, H, W)) return 1;
  REQUIRE(params, "params is NULL");
  if (check_threshold(params->threshold)) return 1;
  REQUIRE(params->axes >= 1 && params->axes <= 3, "axes=%d: 1 horizontal, 2 vertical, 3 both", params->axes);
  REQUIRE(params->max_thick >= 1 && params->max_thick <= 16, "max_thick=%d: 1..16", params->max_thick);
  REQUIRE(params->min_len > params->max_thick && params->min_len <= 16384, "min_len=%d: max_thick=%d < min_len <= 16384", params->min_len,
          params->max_thick);
  REQUIRE(params->edge >= 0 && params->edge <= 4, "edge=%d: 0..4", params->edge);
  REQUIRE(params->reserved[0] == 0 && params->reserved[1] == 0, "reserved words must be 0");
  if (check_scratch(scratch_dev, out_dev)) return 1;
  REQUIRE(((uintptr_t)counts_dev & 3) == 0, "counts_dev must be 4-byte aligned");
  if (check_out(page_dev, pitch, H, W, out_dev, out_pitch, H, W)) return 1;
  const Span page = span_rows(page_dev, pitch, H, W), out = span_rows(out_dev, out_pitch, H, W);
  const Span scratch = span_bytes(scratch_dev, rules_scratch_bytes(H, W));
  REQUIRE(disjoint(out, scratch), "out_dev overlaps the scratch");
  REQUIRE(disjoint(scratch, page), "scratch_dev overlaps the page");
  if (counts_dev) {
    const Span counts = span_bytes(counts_dev, 8 * sizeof(int32_t));
    REQUIRE(disjoint(counts, page), "counts_dev overlaps the page");
    REQUIRE(disjoint(counts, out), "counts_dev overlaps out_dev");
    REQUIRE(disjoint(counts, scratch), "counts_dev overlaps the scratch");
  }
  remove_rules((hipStream_t)stream, page_dev, pitch, H, W, *params, scratch_dev, out_dev, out_pitch, counts_dev);
  return check_launch("aocr_remove_rules");
}

static bool panels_size_ok(int32_t H, int32_t W, int32_t max_panels) { return page_size_ok(H, W) && max_panels >= 1 && max_panels <= 1024; }

size_t aocr_panels_scratch_bytes(int32_t H, int32_t W, int32_t max_panels) {
  if (!panels_size_ok(H, W, max_panels)) {
    fail("bad sizes H=%d W=%d (1..16384 each, H*W <= 2^26) max_panels=%d (1..1024)", H, W, max_panels);
    return 0;
  }
  return panels_scratch_bytes(H, W, max_panels);
}

int aocr_invert_panels(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, const aocr_panel_params* params,
                       void* scratch_dev, uint8_t* out_dev, int64_t out_pitch, int32_t max_panels, int32_t* panels_dev, int32_t counts_dev[8]) {
  if (check_page(page_dev, pitch, H, W)) return 1;
  REQUIRE(params, "params is NULL");
  if (check_threshold(params->threshold)) return 1;
  REQUIRE(params->connectivity == 4 || params->connectivity == 8, "connectivity=%d: 4 or 8", params->connectivity);
  REQUIRE(params->min_w >= 1 && params->min_h >= 1, "min_w=%d min_h=%d must be >= 1", params->min_w, params->min_h);
  REQUIRE(params->fill_percent >= 1 && params->fill_percent <= 100, "fill_percent=%d: 1..100", params->fill_percent);
  REQUIRE(params->min_inside_percent >= 0 && params->min_inside_percent <= 99, "min_inside_percent=%d: 0..99", params->min_inside_percent);
  REQUIRE(params->fill_percent + params->min_inside_percent <= 100, "fill_percent=%d + min_inside_percent=%d is more than 100", params->fill_percent,
          params->min_inside_percent);
  REQUIRE(params->reserved == 0, "the reserved word must be 0");
  REQUIRE(max_panels >= 1 && max_panels <= 1024, "max_panels=%d: 1..1024", max_panels);
  if (check_scratch(scratch_dev, out_dev && counts_dev)) return 1;
  REQUIRE(((uintptr_t)counts_dev & 3) == 0 && ((uintptr_t)panels_dev & 3) == 0, "counts_dev and panels_dev must be 4-byte aligned");
  if (check_out(page_dev, pitch, H, W, out_dev, out_pitch, H, W)) return 1;
  const Span page = span_rows(page_dev, pitch, H, W), out = span_rows(out_dev, out_pitch, H, W);
  const Span scratch = span_bytes(scratch_dev, panels_scratch_bytes(H, W, max_panels));
  REQUIRE(disjoint(out, scratch), "out_dev overlaps the scratch");
  REQUIRE(disjoint(scratch, page), "scratch_dev overlaps the page");
  const Span counts = span_bytes(counts_dev, 8 * sizeof(int32_t));
  REQUIRE(disjoint(counts, page), "counts_dev overlaps the page");
  REQUIRE(disjoint(counts, out), "counts_dev overlaps out_dev");
  REQUIRE(disjoint(counts, scratch), "counts_dev overlaps the scratch");
  if (panels_dev) {
    const Span panels = span_bytes(panels_dev, (size_t)max_panels * 8 * sizeof(int32_t));
    REQUIRE(disjoint(panels, page), "panels_dev overlaps the page");
    REQUIRE(disjoint(panels, out), "out_dev overlaps panels_dev");
    REQUIRE(disjoint(panels, scratch), "panels_dev overlaps the scratch");
    REQUIRE(disjoint(panels, counts), "panels_dev overlaps counts_dev");
  }
  invert_panels((hipStream_t)stream, page_dev, pitch, H, W, *params, scratch_dev, out_dev, out_pitch, max_panels, panels_dev, counts_dev);
  return check_launch("aocr_invert_panels");
}

int aocr_rotate_page(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, const int32_t* orient_dev, int32_t quarter,
                     uint8_t* out_dev, int64_t out_pitch) {
  if (check_page(page_dev, pitch, H, W)) return 1;
  REQUIRE(quarter >= 0 && quarter <= 3, "quarter=%d: 0..3", quarter);
  REQUIRE(out_dev, "out_dev is NULL");
  REQUIRE(((uintptr_t)orient_dev & 3) == 0, "orient_dev must be 4-byte aligned");
  const int32_t Ho = (quarter & 1) ? W : H, Wo = (quarter & 1) ? H : W;
  if (check_out(page_dev, pitch, H, W, out_dev, out_pitch, Ho, Wo, "the output's width ")) return 1;
  rotate_page((hipStream_t)stream, page_dev, pitch, H, W, orient_dev, quarter, out_dev, out_pitch);
  return check_launch("aocr_rotate_page");
}

size_t aocr_orient_scratch_bytes(int32_t H, int32_t W) { return scratch_size_ok(H, W) ? orient_scratch_bytes(H, W) : 0; }

int aocr_estimate_orientation(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, int32_t threshold, int32_t light_text,
                              void* scratch_dev, int32_t orient_dev[8]) {
  if (check_page(page_dev, pitch, H, W)) return 1;
  if (check_threshold(threshold)) return 1;
  if (check_scratch(scratch_dev, orient_dev)) return 1;
  REQUIRE(((uintptr_t)orient_dev & 3) == 0, "orient_dev must be 4-byte aligned");
  estimate_orientation((hipStream_t)stream, page_dev, pitch, H, W, threshold, light_text, scratch_dev, orient_dev);
  return check_launch("aocr_estimate_orientation");
}

size_t aocr_quad_scratch_bytes(int32_t H, int32_t W) { return scratch_size_ok(H, W) ? quad_scratch_bytes(H, W) : 0; }

int aocr_find_page_quad(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, int32_t threshold, int32_t dark_paper,
                        void* scratch_dev, int32_t quad_dev[16]) {
  if (check_page(page_dev, pitch, H, W)) return 1;
  if (check_threshold(threshold)) return 1;
  if (check_scratch(scratch_dev, quad_dev)) return 1;
  REQUIRE(((uintptr_t)quad_dev & 3) == 0, "quad_dev must be 4-byte aligned");
  if (check_words(page_dev, pitch, H, W, scratch_dev, quad_scratch_bytes(H, W), quad_dev, 16, "quad_dev")) return 1;
  find_page_quad((hipStream_t)stream, page_dev, pitch, H, W, threshold, dark_paper, scratch_dev, quad_dev);
  return check_launch("aocr_find_page_quad");
}

int aocr_rectify_plan(const int32_t quad[8], int32_t Wo_in, int32_t Ho_in, int32_t size[2], double coef[9]) {
  REQUIRE(quad && size && coef, "NULL argument");
  char msg[256] = "";
  int32_t sz[2];
  double c[9];
  if (rectify_plan(quad, Wo_in, Ho_in, sz, c, msg, sizeof msg)) return fail("%s", msg);
  size[0] = sz[0]; size[1] = sz[1];
  for (int i = 0; i < 9; ++i) coef[i] = c[i];
  return 0;
}

int aocr_warp_page(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, const double coef[9], int32_t fill,
                   uint8_t* out_dev, int64_t out_pitch, int32_t Ho, int32_t Wo) {
  if (check_page(page_dev, pitch, H, W)) return 1;
  REQUIRE(coef, "coef is NULL");
  REQUIRE(out_dev, "out_dev is NULL");
  REQUIRE(page_size_ok(Ho, Wo), "bad output size Ho=%d Wo=%d: 1..16384 each, Ho*Wo <= 2^26", Ho, Wo);
  if (check_out(page_dev, pitch, H, W, out_dev, out_pitch, Ho, Wo, "Wo=", [&] { REQUIRE(fill >= 0 && fill <= 255, "fill=%d: 0..255", fill); return 0; }))
    return 1;
  warp_page((hipStream_t)stream, page_dev, pitch, H, W, coef, fill, out_dev, out_pitch, Ho, Wo);
  return check_launch("aocr_warp_page");
}

size_t aocr_glyph_scratch_bytes(int32_t H, int32_t W) { return scratch_size_ok(H, W) ? glyph_scratch_bytes(H, W) : 0; }

int aocr_estimate_glyph_size(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, const aocr_glyph_params* params,
                             void* scratch_dev, int32_t glyph_dev[8]) {
  if (check_page(page_dev, pitch, H, W)) return 1;
  REQUIRE(params, "params is NULL");
  if (check_threshold(params->threshold)) return 1;
  REQUIRE(params->connectivity == 4 || params->connectivity == 8, "connectivity=%d: 4 or 8", params->connectivity);
  REQUIRE(params->min_size >= 1, "min_size=%d must be >= 1", params->min_size);
  REQUIRE(params->max_size >= params->min_size && params->max_size <= GLYPH_SIZE_MAX, "max_size=%d: min_size=%d..%d", params->max_size,
          params->min_size, GLYPH_SIZE_MAX);
  REQUIRE(params->max_aspect >= 1, "max_aspect=%d must be >= 1", params->max_aspect);
  REQUIRE(params->reserved[0] == 0 && params->reserved[1] == 0, "reserved words must be 0");
  if (check_scratch(scratch_dev, glyph_dev)) return 1;
  REQUIRE(((uintptr_t)glyph_dev & 3) == 0, "glyph_dev must be 4-byte aligned");
  if (check_words(page_dev, pitch, H, W, scratch_dev, glyph_scratch_bytes(H, W), glyph_dev, 8, "glyph_dev")) return 1;
  estimate_glyph_size((hipStream_t)stream, page_dev, pitch, H, W, *params, scratch_dev, glyph_dev);
  return check_launch("aocr_estimate_glyph_size");
}

int aocr_resize_page(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, uint8_t* out_dev, int64_t out_pitch,
                     int32_t Ho, int32_t Wo) {
  if (check_page(page_dev, pitch, H, W)) return 1;
  REQUIRE(out_dev, "out_dev is NULL");
  REQUIRE(page_size_ok(Ho, Wo), "bad output size Ho=%d Wo=%d: 1..16384 each, Ho*Wo <= 2^26", Ho, Wo);
  if (check_out(page_dev, pitch, H, W, out_dev, out_pitch, Ho, Wo, "Wo=", [&] {
        REQUIRE(W <= 8 * (int64_t)Wo && Wo <= 8 * (int64_t)W && H <= 8 * (int64_t)Ho && Ho <= 8 * (int64_t)H,
                "H=%d W=%d to Ho=%d Wo=%d: a ratio of at most 8 either way on each axis", H, W, Ho, Wo);
        return 0;
      }))
    return 1;
  resize_page((hipStream_t)stream, page_dev, pitch, H, W, out_dev, out_pitch, Ho, Wo);
  return check_launch("aocr_resize_page");
}

static bool curl_sizes_ok(int32_t group, int32_t max_shift) { return group >= 1 && group <= 16 && max_shift >= 0 && max_shift <= 64; }

size_t aocr_curl_scratch_bytes(int32_t H, int32_t W, int32_t group, int32_t max_shift) {
  if (!(page_size_ok(H, W) && curl_sizes_ok(group, max_shift))) {
    fail("bad sizes H=%d W=%d (1..16384 each, H*W <= 2^26) group=%d (1..16) max_shift=%d (0..64)", H, W, group, max_shift);
    return 0;
  }
  return curl_scratch_bytes(H, W, group, max_shift);
}

int aocr_estimate_curl(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, const aocr_curl_params* params,
                       void* scratch_dev, int32_t curl_dev[4], int32_t* shifts_dev, uint64_t* scores_dev) {
  if (check_page(page_dev, pitch, H, W)) return 1;
  REQUIRE(params, "params is NULL");
  if (check_threshold(params->threshold)) return 1;
  REQUIRE(params->group >= 1 && params->group <= 16, "group=%d: 1..16", params->group);
  REQUIRE(params->max_shift >= 0 && params->max_shift <= 64, "max_shift=%d: 0..64", params->max_shift);
  REQUIRE(params->min_ink >= 0 && params->min_ink <= (1 << 20), "min_ink=%d: 0..2^20", params->min_ink);
  REQUIRE(params->reserved[0] == 0 && params->reserved[1] == 0 && params->reserved[2] == 0, "reserved words must be 0");
  if (check_scratch(scratch_dev, curl_dev && shifts_dev)) return 1;
  REQUIRE(((uintptr_t)curl_dev & 3) == 0 && ((uintptr_t)shifts_dev & 3) == 0, "curl_dev and shifts_dev must be 4-byte aligned");
  REQUIRE(((uintptr_t)scores_dev & 7) == 0, "scores_dev must be 8-byte aligned");
  const int ng = curl_groups(W, params->group);
  const size_t scratch_bytes = curl_scratch_bytes(H, W, params->group, params->max_shift);
  if (check_words(page_dev, pitch, H, W, scratch_dev, scratch_bytes, curl_dev, 4, "curl_dev")) return 1;
  if (check_words(page_dev, pitch, H, W, scratch_dev, scratch_bytes, shifts_dev, ng, "shifts_dev")) return 1;
  if (scores_dev) {
    const Span scores = span_bytes(scores_dev, (size_t)(ng - 1) * (2 * params->max_shift + 1) * sizeof(uint64_t));
    REQUIRE(disjoint(scores, span_rows(page_dev, pitch, H, W)), "scores_dev overlaps the page");
    REQUIRE(disjoint(scores, span_bytes(scratch_dev, scratch_bytes)), "scores_dev overlaps the scratch");
  }
  estimate_curl((hipStream_t)stream, page_dev, pitch, H, W, *params, scratch_dev, curl_dev, shifts_dev, scores_dev);
  return check_launch("aocr_estimate_curl");
}

int aocr_dewarp_page(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, int32_t group, const int32_t* shifts_dev,
                     int32_t fill, uint8_t* out_dev, int64_t out_pitch) {
  if (check_page(page_dev, pitch, H, W)) return 1;
  REQUIRE(group >= 1 && group <= 16, "group=%d: 1..16", group);
  REQUIRE(shifts_dev, "shifts_dev is NULL");
  REQUIRE(((uintptr_t)shifts_dev & 3) == 0, "shifts_dev must be 4-byte aligned");
  REQUIRE(out_dev, "out_dev is NULL");
  if (check_out(page_dev, pitch, H, W, out_dev, out_pitch, H, W, "W=", [&] { REQUIRE(fill >= 0 && fill <= 255, "fill=%d: 0..255", fill); return 0; }))
    return 1;
  REQUIRE(disjoint(span_rows(out_dev, out_pitch, H, W), span_bytes(shifts_dev, curl_groups(W, group) * sizeof(int32_t))), "out_dev overlaps shifts_dev");
  dewarp_page((hipStream_t)stream, page_dev, pitch, H, W, group, shifts_dev, fill, out_dev, out_pitch);
  return check_launch("aocr_dewarp_page");
}

size_t aocr_colour_scratch_bytes(int32_t H, int32_t W) { return scratch_size_ok(H, W) ? colour_scratch_bytes() : 0; }

static int check_rgb(const uint8_t* rgb_dev, int64_t pitch, int32_t H, int32_t W) {
  REQUIRE(rgb_dev, "rgb_dev is NULL");
  REQUIRE(page_size_ok(H, W), "bad page size H=%d W=%d: 1..16384 each, H*W <= 2^26", H, W);
  REQUIRE(pitch >= 3 * (int64_t)W, "pitch=%lld is smaller than 3 * W=%d", (long long)pitch, W);
  return 0;
}

static int check_colour_params(const aocr_colour_params* p) {
  REQUIRE(p, "params is NULL");
  REQUIRE(p->weights[0] >= 0 && p->weights[1] >= 0 && p->weights[2] >= 0 && p->weights[0] + p->weights[1] + p->weights[2] == 256,
          "weights=%d %d %d: each >= 0 and 256 in sum", p->weights[0], p->weights[1], p->weights[2]);
  REQUIRE(p->mode == 0 || p->mode == 1, "mode=%d: 0 or 1", p->mode);
  REQUIRE(p->balance == 0 || p->balance == 1, "balance=%d: 0 or 1", p->balance);
  if (p->paper[0] >= 0)
    REQUIRE(p->paper[0] >= 1 && p->paper[0] <= 255 && p->paper[1] >= 1 && p->paper[1] <= 255 && p->paper[2] >= 1 && p->paper[2] <= 255,
            "paper=%d %d %d: 1..255 each, or paper[0] < 0 for an estimate", p->paper[0], p->paper[1], p->paper[2]);
  REQUIRE(p->paper_min >= 1 && p->paper_min <= 255, "paper_min=%d: 1..255", p->paper_min);
  REQUIRE(p->chroma_min >= 1 && p->chroma_min <= 255, "chroma_min=%d: 1..255", p->chroma_min);
  REQUIRE(p->drop >= 0 && p->drop <= 63, "drop=%d: 0..63", p->drop);
  REQUIRE(p->fill >= 0 && p->fill <= 255, "fill=%d: 0..255", p->fill);
  return 0;
}

int aocr_estimate_page_colour(void* stream, const uint8_t* rgb_dev, int64_t pitch, int32_t H, int32_t W, const aocr_colour_params* params,
                              void* scratch_dev, int32_t colour_dev[16]) {
  if (check_rgb(rgb_dev, pitch, H, W)) return 1;
  if (check_colour_params(params)) return 1;
  REQUIRE(scratch_dev, "scratch_dev is NULL");
  REQUIRE(colour_dev, "colour_dev is NULL");
  if (check_scratch(scratch_dev, true)) return 1;
  REQUIRE(((uintptr_t)colour_dev & 3) == 0, "colour_dev must be 4-byte aligned");
  if (check_words(rgb_dev, pitch, H, 3 * W, scratch_dev, colour_scratch_bytes(), colour_dev, 16, "colour_dev")) return 1;
  estimate_page_colour((hipStream_t)stream, rgb_dev, pitch, H, W, *params, scratch_dev, colour_dev);
  return check_launch("aocr_estimate_page_colour");
}

int aocr_gray_page(void* stream, const uint8_t* rgb_dev, int64_t pitch, int32_t H, int32_t W, const aocr_colour_params* params,
                   const int32_t* colour_in_dev, int32_t* colour_out_dev, uint8_t* out_dev, int64_t out_pitch) {
  if (check_rgb(rgb_dev, pitch, H, W)) return 1;
  if (check_colour_params(params)) return 1;
  REQUIRE(colour_in_dev || !params->balance || params->paper[0] >= 0, "colour_in_dev is NULL and params->paper asks for an estimate");
  REQUIRE(((uintptr_t)colour_in_dev & 3) == 0 && ((uintptr_t)colour_out_dev & 3) == 0, "colour_in_dev and colour_out_dev must be 4-byte aligned");
  REQUIRE(out_dev, "out_dev is NULL");
  REQUIRE(out_pitch >= W, "out_pitch=%lld is smaller than W=%d", (long long)out_pitch, W);
  const Span rgb = span_rows(rgb_dev, pitch, H, 3 * (int64_t)W), out = span_rows(out_dev, out_pitch, H, W);
  REQUIRE(disjoint(out, rgb), "out_dev overlaps the page");
  for (const int32_t* words : {colour_in_dev, (const int32_t*)colour_out_dev}) {
    if (!words) continue;
    const char* name = words == colour_in_dev ? "colour_in_dev" : "colour_out_dev";
    REQUIRE(disjoint(span_bytes(words, 16 * sizeof(int32_t)), rgb), "%s overlaps the page", name);
    REQUIRE(disjoint(span_bytes(words, 16 * sizeof(int32_t)), out), "out_dev overlaps %s", name);
  }
  REQUIRE(!colour_in_dev || !colour_out_dev || colour_in_dev == colour_out_dev ||
              disjoint(span_bytes(colour_in_dev, 16 * sizeof(int32_t)), span_bytes(colour_out_dev, 16 * sizeof(int32_t))),
          "colour_out_dev overlaps colour_in_dev without being equal to it");
  gray_page((hipStream_t)stream, rgb_dev, pitch, H, W, *params, colour_in_dev, colour_out_dev, out_dev, out_pitch);
  return check_launch("aocr_gray_page");
}

static bool slant_sizes_ok(int32_t n_boxes, int32_t n_steps) { return n_boxes >= 0 && n_boxes <= 65535 && n_steps >= 0 && n_steps <= 64; }

size_t aocr_slant_scratch_bytes(int32_t n_boxes, int32_t n_steps) {
  if (!slant_sizes_ok(n_boxes, n_steps)) {
    fail("bad sizes n_boxes=%d (0..65535) n_steps=%d (0..64)", n_boxes, n_steps);
    return 0;
  }
  return slant_scratch_bytes(n_boxes, n_steps);
}

int aocr_estimate_slant(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, const aocr_box* boxes_dev,
                        const int32_t* count_dev, int32_t n_boxes, const aocr_slant_params* params, const int32_t* threshold_dev,
                        void* scratch_dev, int32_t* slant_dev, uint64_t* scores_dev) {
  if (check_page(page_dev, pitch, H, W)) return 1;
  REQUIRE(n_boxes >= 0 && n_boxes <= 65535, "bad sizes: n_boxes=%d (0..65535)", n_boxes);
  REQUIRE(params, "params is NULL");
  if (check_threshold(params->threshold)) return 1;
  REQUIRE(params->step_q16 >= 1 && params->step_q16 <= 8192, "step_q16=%d: 1..8192", params->step_q16);
  REQUIRE(params->n_steps >= 0 && params->n_steps <= 64, "n_steps=%d: 0..64", params->n_steps);
  REQUIRE(params->n_steps * params->step_q16 <= 65536, "n_steps=%d * step_q16=%d exceeds 65536 (45 degrees)", params->n_steps, params->step_q16);
  REQUIRE(params->reserved[0] == 0 && params->reserved[1] == 0 && params->reserved[2] == 0 && params->reserved[3] == 0,
          "reserved words must be 0");
  REQUIRE(params->threshold >= 0 || threshold_dev, "threshold_dev is NULL and params->threshold asks for the device word");
  REQUIRE(((uintptr_t)threshold_dev & 3) == 0 && ((uintptr_t)count_dev & 3) == 0, "threshold_dev and count_dev must be 4-byte aligned");
  if (n_boxes == 0) return 0;
  REQUIRE(boxes_dev, "boxes_dev is NULL");
  REQUIRE(slant_dev, "slant_dev is NULL");
  if (check_scratch(scratch_dev, true)) return 1;
  REQUIRE(((uintptr_t)boxes_dev & 3) == 0 && ((uintptr_t)slant_dev & 3) == 0, "boxes_dev and slant_dev must be 4-byte aligned");
  REQUIRE(((uintptr_t)scores_dev & 7) == 0, "scores_dev must be 8-byte aligned");
  const size_t scratch_bytes = slant_scratch_bytes(n_boxes, params->n_steps);
  if (check_words(page_dev, pitch, H, W, scratch_dev, scratch_bytes, slant_dev, 4 * n_boxes, "slant_dev")) return 1;
  if (scores_dev) {
    const Span scores = span_bytes(scores_dev, (size_t)n_boxes * (2 * params->n_steps + 1) * sizeof(uint64_t));
    REQUIRE(disjoint(scores, span_rows(page_dev, pitch, H, W)), "scores_dev overlaps the page");
    REQUIRE(disjoint(scores, span_bytes(scratch_dev, scratch_bytes)), "scores_dev overlaps the scratch");
  }
  estimate_slant((hipStream_t)stream, page_dev, pitch, H, W, boxes_dev, count_dev, n_boxes, *params, threshold_dev, scratch_dev, slant_dev,
                 scores_dev);
  return check_launch("aocr_estimate_slant");
}

int aocr_crop_lines_slanted(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, const aocr_box* boxes_dev,
                            const int32_t* count_dev, int32_t n_boxes, const int32_t* slant_dev, int32_t fill, int32_t out_h, int32_t out_w,
                            float* out_dev) {
  if (check_page(page_dev, pitch, H, W)) return 1;
  REQUIRE(n_boxes >= 0 && n_boxes <= 65535 && out_h >= 1 && out_w >= 1 && (int64_t)out_h * out_w <= INT32_MAX,
          "bad sizes: n_boxes=%d (0..65535) out_h=%d out_w=%d", n_boxes, out_h, out_w);
  REQUIRE(fill >= 0 && fill <= 255, "fill=%d: 0..255", fill);
  REQUIRE(((uintptr_t)slant_dev & 3) == 0, "slant_dev must be 4-byte aligned");
  if (n_boxes == 0) return 0;
  REQUIRE(boxes_dev && out_dev, "NULL argument: boxes_dev or out_dev");
  crop_lines_slanted((hipStream_t)stream, page_dev, pitch, H, W, boxes_dev, count_dev, n_boxes, slant_dev, fill, out_h, out_w, out_dev);
  return check_launch("aocr_crop_lines_slanted");
}

}  // extern "C"
