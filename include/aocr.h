/* aocr.h -- C ABI of libaocr: the MI355X (gfx950) implementation of the
 * CNN -> BiLSTM -> attention-decoder train / decode step of
 * da03/torch-Attention-OCR.
 *
 * The reference has no FFI of its own: its hot path runs inside un-vendored
 * Torch7 packages that src/train.lua:4-9 and src/model/model.lua:3-7 only
 * `require`.  The entry points below are what a LuaJIT `ffi.cdef` (see
 * INTEGRATION.md) or a ctypes binding (torch-attention-ocr_amd/aocr/_lib.py)
 * binds instead; each one cites the reference code it replaces
 * (paths relative to the reference root).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; the message is
 *     available from aocr_last_error() (thread-local).  Nothing throws.
 *   - all pointers named *_dev are DEVICE pointers (HBM) owned by the caller;
 *     the library never allocates device memory: parameters, gradients and the
 *     workspace arena are handed in at aocr_model_create().
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every
 *     call only enqueues work on it and never synchronises.
 *   - activations are fp32, channels-last (B,H,W,C); token ids are 1-based int32
 *     (1 PAD, 2 GO, 3 EOS: src/train.lua:53).
 *   - the ABI is not re-entrant per aocr_model (Lua is single threaded).
 */
#ifndef AOCR_H
#define AOCR_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AOCR_VERSION 1
#define AOCR_NUM_GROUPS 5           /* cnn, enc_fw, enc_bw, decoder, projector: model.lua:150 */
#define AOCR_COMPUTE_F32 0          /* v_mfma_f32_32x32x2_f32, exact fp32 */
#define AOCR_COMPUTE_BF16 1         /* bf16 operands, fp32 accumulate */

typedef struct aocr_model aocr_model;

/* Hyper-parameters: src/train.lua:41-62, src/model/model.lua:83-96. */
typedef struct aocr_config {
  int32_t batch_size;       /* max rows per step                        (-batch_size) */
  int32_t img_h;            /* 32, src/data/data_gen.lua:16 */
  int32_t max_img_w;        /* widest crop the workspace is sized for */
  int32_t enc_hidden;       /* -encoder_num_hidden */
  int32_t enc_layers;       /* -encoder_num_layers */
  int32_t dec_layers;       /* -decoder_num_layers */
  int32_t vocab;            /* -target_vocab_size (39) */
  int32_t emb;              /* -target_embedding_size (20) */
  int32_t input_feed;       /* -input_feed */
  int32_t max_decoder_l;    /* -max_decoder_l (50) */
  int32_t max_beam;         /* largest -beam_size the workspace is sized for */
  int32_t compute;          /* AOCR_COMPUTE_* */
} aocr_config;

const char* aocr_last_error(void);
int aocr_version(void);

/* ---- parameter layout (replaces nn.Module:getParameters(), model.lua:163-168)
 * One flat fp32 buffer holds the 5 groups back to back; within a group the order
 * is Torch7's (module order, weight then bias).  Conv weights are stored
 * [Cout][kH][kW][Cin] (channels-last taps); everything else as in Torch7. */
int aocr_param_counts(const aocr_config* cfg, int64_t counts[AOCR_NUM_GROUPS]);
/* Enumerate named tensors: returns 0 and fills the outputs for index < n, 1 past the end.
 * offset is relative to the start of the flat buffer (not of the group). */
int aocr_param_entry(const aocr_config* cfg, int32_t index, char name[64], int32_t* group,
                     int64_t* offset, int32_t* ndim, int64_t shape[4]);
/* BatchNorm running statistics (not parameters): [rm3(256) rv3 rm5(512) rv5 rm7(512) rv7]. */
int64_t aocr_bn_state_count(void);

size_t aocr_workspace_bytes(const aocr_config* cfg);

/* ---- model handle (replaces Model:create/_build, model.lua:83-223) */
int aocr_model_create(const aocr_config* cfg, float* params_dev, float* grads_dev,
                      float* bn_state_dev, void* workspace_dev, size_t workspace_bytes,
                      void* stream, aocr_model** out);
int aocr_model_destroy(aocr_model* m);
int aocr_model_set_stream(aocr_model* m, void* stream);

/* ---- fused sequence-level entry points (what Model:step uses) */

/* Health of the whole-sequence ("cluster") kernels: the compute units that share a block of batch rows wait for each other with BOUNDED
 * spins; if a wait ever times out (it cannot unless another kernel keeps part of the chip busy for ~0.3 s) the kernel records a code,
 * finishes, and the step's results are invalid: aocr_sgd_step / aocr_adadelta_step then leave the parameters untouched (device-side
 * predicate on the same flag, no host sync).  The optimizer call CONSUMES the code (round 6): it moves it to a second word that waits for
 * the host, so exactly the step that timed out is skipped -- a host that polls this call only every N steps loses that one step, never its
 * weights and never the healthy steps behind it (before round 6 every step up to the poll was dropped).  A code raised by a call that has
 * no optimizer behind it (aocr_decode*) is moved aside the same way by the next aocr_train_forward_backward, so it cannot cancel that step.
 * *code = 0: healthy; otherwise the most recent code not yet reported; cleared by the call (read and clear).
 * Under data parallelism the code is a GLOBAL decision (round 4): aocr_allreduce_grads sums a time-out flag with the exchange, and a rank whose own
 * kernels were healthy while a peer's were not reads 0x7e -- so every rank's optimizer skips the update and every host repeats the step together.
 * The optimizer call that skips an update also restores the BatchNorm running statistics to their values at the start of that step (device side, round 5):
 * a skipped step leaves NO trace in the model, so the host may repeat the batch at once, later (whenever it polls) or never.
 * A caller that sums the gradient buckets itself (aocr_stream_wait_grads) must also take the MAX over ranks of the status word (tap "cl_err"[0]) before
 * aocr_sgd_step, as aocr_allreduce_grads does inside the library; the Python mirror does (Model._exchange_timeout_flag).
 * Synchronises the model's stream.  No reference counterpart.
 * These kernels need the device to themselves: a launch occupies every compute unit, so the steps of two models (or two processes)
 * must not run concurrently on ONE device -- AOCR_NO_CLUSTER=1 AOCR_NO_DEC_CLUSTER=1 selects the per-step launch chains for that case. */
int aocr_cluster_status(aocr_model* m, int32_t* code);

/* nn.Dropout(p) of LSTM.lua:68-69 (input of every LSTM layer above the first, encoder and decoder) and :116-118 (attention output),
 * active in the training step only (model.lua:284 `training()`; decode / forward_only run `evaluate()`).  The mask is a counter-based
 * function of (seed, train_step, site, element index) -- splitmix64, restated in oracle/oracle_torch.py::dropout_mask -- so a step is
 * reproducible and the oracle can replay it; kept activations are scaled by 1/(1-p) (nn.Dropout v2).  Call before every training
 * step with the step counter (the reference draws from torch's global generator instead: the mask VALUES cannot match, the
 * distribution does).  p = 0 (default) disables it.  (Round 3: the whole-sequence decoder kernels evaluate the same masks.) */
int aocr_set_dropout(aocr_model* m, double p, uint64_t seed, uint64_t train_step);

/* feval of model.lua:284-696 with forward_only=false: CNN forward (training-mode
 * BatchNorm, running stats updated), encoder fw/bw loops, teacher-forced decoder
 * loop, loss, hand-ordered BPTT, CNN backward.  Gradients are ZEROED then
 * accumulated into grads_dev with d(loss) scaled by grad_scale (= 1/batch_size in
 * the reference, model.lua:645-647; 1/global_batch under data parallelism).
 * loss_dev[0] = sum of NLL over the step (un-scaled, = loss*batch_size of :701).
 * images_dev (B,1,32,W) fp32 values 0..255; targets/targets_eval (B,L) int32
 * (src/data/data_gen.lua:107-117). */
int aocr_train_forward_backward(aocr_model* m, const float* images_dev, const int32_t* targets_dev,
                                const int32_t* targets_eval_dev, int32_t B, int32_t W, int32_t L,
                                float grad_scale, float* loss_dev);

/* Data-parallel overlap: the flat gradient vector completes back to front
 * during the backward pass -- bucket 0 = decoder + projector groups, 1 = both encoder groups,
 * 2 = the CNN from conv5 upwards, 3 = conv1..conv4 -- and an event marks each point.
 * aocr_grad_buckets gives the [begin, end) float ranges of the buckets inside grads_dev;
 * aocr_stream_wait_grads makes `stream` wait until bucket `bucket` of the LAST enqueued
 * aocr_train_forward_backward is complete, so that its all-reduce can run on a second stream
 * beside the rest of the backward pass.  The caller joins that stream before aocr_sgd_step. */
#define AOCR_GRAD_BUCKETS 4
int aocr_grad_buckets(const aocr_config* cfg, int64_t begin[AOCR_GRAD_BUCKETS], int64_t end[AOCR_GRAD_BUCKETS]);
int aocr_stream_wait_grads(aocr_model* m, int32_t bucket, void* stream);

/* ---- data parallelism inside the library: one process per GPU, ONE exchange step -- the sum over ranks of the flat
 * gradient vector between feval and the per-group clip (optim_sgd.lua:38 -> :40) -- plus, with sync_bn, the per-channel BatchNorm
 * sums of the three BatchNorm layers (cnn.lua:23,32,41) in the forward and the backward pass, so that N ranks on slices of a batch
 * compute what one GPU computes on the whole batch (training-mode statistics included; running statistics stay identical on all ranks).
 * Provider 1: RCCL over xGMI.  rank 0 calls aocr_comm_unique_id, the host hands the 128 bytes to the other ranks (file, socket, MPI:
 * its choice), every rank calls aocr_comm_init_rank (collective, like ncclCommInitRank).  librccl.so is bound at run time.
 * Provider 2: a host callback that sums `count` elements (dtype & 0xff: 0 = fp32, 1 = fp64) of a device buffer over the ranks in place,
 * enqueued on `stream` (the Python mirror routes torch.distributed through it; the tests use gloo).  dtype & AOCR_COMM_CHANNEL_BN
 * marks the BatchNorm sums: they are issued from inside the forward / backward pass while the gradient buckets are issued after it,
 * and a communicator runs its operations in issue order -- give that channel a communicator (process group) of its own, as provider 1
 * does (ncclCommSplit), or bucket 0 queues behind the last BatchNorm-backward sum and the overlap with the backward pass is lost.
 * aocr_allreduce_grads: after aocr_train_forward_backward and before aocr_sgd_step; the buckets of aocr_grad_buckets are summed on a
 * second stream as the backward pass completes them (overlap), loss_dev (optional, 1 float) is summed too, and the model's stream
 * waits for the last bucket.  Pass grad_scale = 1 / GLOBAL batch to aocr_train_forward_backward.
 * Exchange policy (round 4): no collective is in flight while a whole-sequence kernel runs -- with a communicator attached bucket 0 (decoder + projector)
 * is released behind the encoder BPTT (AOCR_COMM_EARLY_BUCKET0=1: as soon as it is complete; the encoder kernels then leave AOCR_COMM_RESERVE_CUS,
 * default 32, compute units free).  aocr_comm_init_rank fails if ncclCommSplit fails (AOCR_ONE_COMM=1 on every rank shares one communicator). */
#define AOCR_COMM_CHANNEL_BN 0x100
typedef int (*aocr_allreduce_fn)(void* user, void* buf_dev, int64_t count, int32_t dtype, void* stream);
int aocr_comm_unique_id(char id[128]);
int aocr_comm_init_rank(aocr_model* m, const char id[128], int32_t nranks, int32_t rank, int32_t sync_bn);
int aocr_comm_set_callback(aocr_model* m, aocr_allreduce_fn fn, void* user, int32_t nranks, int32_t sync_bn);
int aocr_allreduce_grads(aocr_model* m, float* loss_dev);
int aocr_comm_destroy(aocr_model* m);
/* What is attached: *nranks (1 without a communicator), *sync_bn (0 / 1), *provider (0 none, 1 RCCL, 2 host callback).  Any pointer may be NULL. */
int aocr_comm_info(aocr_model* m, int32_t* nranks, int32_t* sync_bn, int32_t* provider);
/* Measurement: milliseconds the model's stream waited for the exchange stream at the end of the LAST aocr_allreduce_grads -- the part
 * of the gradient exchange that the backward pass did not hide (0 without a communicator).  Synchronises that step. */
int aocr_comm_exposed_ms(aocr_model* m, float* ms);

/* optim.sgd_list, src/optim/optim_sgd.lua:38-95 with the options the reference
 * leaves at 0: per group, if ||g||_2 > clip then g *= clip/||g||_2; w -= lr*g.
 * norms_dev (optional, 2*5 floats): {param norm, grad norm} per group, as printed
 * by optim_sgd.lua:49.  A data-parallel all-reduce of grads_dev goes before this call. */
int aocr_sgd_step(aocr_model* m, float lr, float clip, float* norms_dev);

/* optim.adadelta_list, src/optim/optim_adadelta.lua:19-62 (the optimizer the reference ships
 * next to sgd_list), one fused pass over all parameters: var = rho*var + (1-rho)*g^2;
 * delta = sqrt(acc+eps)/sqrt(var+eps)*g; w -= delta; acc = rho*acc + (1-rho)*delta^2.
 * state_dev: 2*n floats {paramVariance | accDelta} (n = sum of aocr_param_counts), zeroed by
 * the caller before the first step and kept between steps.  weight_decay: g += wd*w first
 * (what optim_adadelta.lua:37 means; the line itself would raise).  No clipping (:31-57). */
int aocr_adadelta_step(aocr_model* m, float rho, float eps, float weight_decay, float* state_dev);

/* AdamW (Adam with decoupled weight decay) with a per-group gradient clip, on the device.  No reference counterpart: the reference ships
 * sgd_list and adadelta_list only.  aocr_adam_update is a model-free leaf like aocr_gemm / aocr_pointwise (explicit pointers, any 4-byte-aligned
 * params_dev / grads_dev); aocr_adam_step applies it to the model's parameters and gradients on the model's stream.
 * Groups: group_off[0..5], 0 = group_off[0] <= ... <= group_off[5] = n (the offsets aocr_param_counts sums to; a group may be empty).
 * Norms and clip, per group k: pn[k] = ||w_k||_2 and gn[k] = ||g_k||_2, squares summed in double (one partial per workgroup, then a
 *   fixed-order sum: no float atomics, the same bits on every run), the root taken in double;
 *   scale[k] = (clip > 0 && gn[k] > clip) ? (float)((double)clip / gn[k]) : 1.0f, compared in double.  An empty group: norms 0, scale 1.
 *   norms_dev (NULL or 15 floats) receives pn[5], gn[5] (each rounded to float once), scale[5].
 * State: state_dev holds 2n floats {m | v} and, at byte offset 8n, a 32-byte tail {double p1, double p2, int64 steps, int64 reserved};
 *   aocr_adam_state_bytes(n) = 8n + 32 bytes, 8-byte aligned, zeroed by the caller before the first step and kept between steps.
 *   All-zero state is a fresh optimizer: steps == 0 reads p1 = p2 = 1.0.  Per applied step, by one thread, ahead of the element update:
 *   p1 *= (double)beta1; p2 *= (double)beta2; steps += 1; c1 = (float)(1.0 - p1); c2 = (float)(1.0 - p2) -- running products, not pow.
 * Element i of group k, all fp32, every operation rounded on its own (no fused multiply-add; '/' and sqrtf correctly rounded), in this order:
 *   g  = grad[i] * scale[k]
 *   m' = beta1*m + (1.0f-beta1)*g
 *   v' = beta2*v + (1.0f-beta2)*(g*g)
 *   u  = (m'/c1) / (sqrtf(v'/c2) + eps)
 *   w' = w - lr*(u + wd*w)                 (decoupled decay; wd = 0 adds 0*w)
 *   w, m, v are written; grads_dev is NOT modified (aocr_sgd_step's clip rescales it in place), so the gradient taps stay readable.
 * skip_dev: NULL or one device int32; non-zero = nothing is written, not w, m, v nor the tail; norms_dev is still written.
 * scratch_dev: aocr_adam_scratch_bytes() bytes, 8-byte aligned, overwritten by the call; calls on one stream may share it.
 * Errors, all before anything is enqueued (non-zero return, aocr_last_error set, every output untouched): a params member that is not finite,
 *   beta1 or beta2 outside [0, 1), eps <= 0, lr < 0, weight_decay < 0, clip < 0, a non-zero reserved word, group_off[0] != 0 or decreasing
 *   offsets, state_dev not 8-byte aligned, a NULL pointer other than skip_dev / norms_dev.
 * aocr_adam_step: the skip word is the model's time-out latch (aocr_cluster_status), consumed as aocr_sgd_step consumes it; a skipped step also
 *   restores the BatchNorm running statistics from the step's snapshot.  A data-parallel all-reduce of the gradients goes before this call.
 *   The bf16 weight shadows are refreshed at the start of the next forward pass, as after the other optimizers.
 * No host sync in either call. */
typedef struct aocr_adam_params { float lr, beta1, beta2, eps, weight_decay, clip; int32_t reserved[2]; } aocr_adam_params;
size_t aocr_adam_state_bytes(int64_t n);
size_t aocr_adam_scratch_bytes(void);
int aocr_adam_update(void* stream, float* params_dev, const float* grads_dev, void* state_dev, const int64_t group_off[6],
                     const aocr_adam_params* p, const int32_t* skip_dev, void* scratch_dev, float* norms_dev);
int aocr_adam_step(aocr_model* m, const aocr_adam_params* p, void* state_dev, float* norms_dev);

/* Teacher-forced forward only (no gradients).  training!=0 uses batch statistics
 * in BatchNorm (without touching running stats); logits_dev (L,B,vocab) receives the
 * pre-LogSoftMax projector output (output_projector.lua:5), loss_dev[0] the NLL sum. */
int aocr_forward_logits(aocr_model* m, const float* images_dev, const int32_t* targets_dev,
                        const int32_t* targets_eval_dev, int32_t B, int32_t W, int32_t L,
                        int32_t training, float* logits_dev, float* loss_dev);

/* feval with forward_only=true (model.lua:321-536, 570-627): eval-mode CNN, encoder,
 * beam search over max_decoder_l steps (beam 1 = greedy), back-trace, then the
 * teacher-forced gold pass.  labels_dev (B,max_decoder_l) int32, scores_dev (B),
 * gold_scores_dev (B), loss_dev[0] = gold-pass NLL sum.  No dictionary (trie == nil). */
int aocr_decode(aocr_model* m, const float* images_dev, const int32_t* targets_dev,
                const int32_t* targets_eval_dev, int32_t B, int32_t W, int32_t L, int32_t beam,
                int32_t* labels_dev, float* scores_dev, float* gold_scores_dev, float* loss_dev);

/* The dictionary trie of loadDictionary (utils.lua:177-218) in flat, device-resident form.
 * Node 0 is the start symbol's node (trie[2]).  Node n has a child for vocab id v (1-based,
 * v <= 64) iff bit v-1 of child_mask_dev[n] is set; the children of n are
 * child_dev[child_base_dev[n] ...] in ascending v.  A node reached through EOS (3) is an
 * ordinary node (childless unless -allow_digit_prefix made it the root, utils.lua:193-198). */
typedef struct aocr_trie {
  const uint64_t* child_mask_dev;   /* [n_nodes] */
  const int32_t* child_base_dev;    /* [n_nodes] */
  const int32_t* child_dev;         /* [n_edges] */
  int32_t n_nodes, n_edges;
} aocr_trie;

/* aocr_decode with -use_dictionary (model.lua:380-387,405-445,460-513): at every step only
 * candidates whose token continues the beam's trie node are admissible (after the first step
 * PAD always is, :469); when fewer than `beam` candidates are admissible the best admissible one
 * fills the remaining beams (:419-433; the same rule replaces the broken fallback of :477-497).
 * trie == NULL is aocr_decode.  Needs target_vocab_size <= 64. */
int aocr_decode_dict(aocr_model* m, const float* images_dev, const int32_t* targets_dev,
                     const int32_t* targets_eval_dev, int32_t B, int32_t W, int32_t L, int32_t beam,
                     const aocr_trie* trie, int32_t* labels_dev, float* scores_dev,
                     float* gold_scores_dev, float* loss_dev);

/* Forward-only recognition without labels: eval-mode CNN, encoder, beam search over max_decoder_l
 * steps (beam 1 = greedy), back-trace.  There is no gold pass and no loss.  Every row starts from
 * GO (2).  trie may be NULL (no dictionary; otherwise as aocr_decode_dict).
 * labels_dev (B,max_decoder_l) int32 and scores_dev (B): what aocr_decode_dict returns for the
 * same images, bit for bit.  Optional (NULL = not wanted), along the winning hypothesis:
 *   char_logp_dev (B,max_decoder_l): log-probability of each emitted token at its step (the
 *     increase of the hypothesis' running score: sums to scores_dev up to rounding);
 *   attn_dev (B,max_decoder_l,T), T = W/4 - 1: the attention weights that produced each token.
 * Positions after the first EOS are 0 in both (the PAD-at-no-cost steps, model.lua:448-449;
 * a PAD emitted before any EOS ends a hypothesis the same way); that EOS itself is included. */
int aocr_recognize(aocr_model* m, const float* images_dev, int32_t B, int32_t W, int32_t beam,
                   const aocr_trie* trie, int32_t* labels_dev, float* scores_dev,
                   float* char_logp_dev, float* attn_dev);

/* Debug / parity taps: device pointer + shape of a named intermediate of the last
 * step ("feats" (T,B,512), "context" (B,T,2He), "logits" (L,B,40), "dfeats", "dcontext"). */
int aocr_get_tensor(aocr_model* m, const char* name, const void** ptr_dev, int32_t* ndim, int64_t shape[4]);

/* Times `iters` launches of one hot kernel of the LAST step's shape with HIP events
 * on the model's stream; which: 0 = conv6 forward implicit GEMM (largest layer), 1 = conv6 filter gradient (the split-K
 * kernel + the sum of its slabs, as the backward pass launches them; the result goes to scratch).
 * ms_per_launch and flops_per_launch are host outputs (this call synchronises).
 * which >= 2 (round 4): the BANDWIDTH-bound kernels of the bf16 training step, each replayed with the arguments and on the buffers of the last
 * aocr_train_forward_backward (whose image buffer must still be valid); *flops_per_launch then returns the ALGORITHMIC BYTES of one launch
 * (what the kernel must read and write once), so bytes / ms = the HBM rate to hold against ~6.3 TB/s achievable.
 * These replays overwrite activations / gradient maps / gradients: taps and gradients are undefined until the next step. */
#define AOCR_PK_CONV6_FWD 0
#define AOCR_PK_CONV6_WGRAD 1
#define AOCR_PK_CONV1_FWD 2      /* normalise + conv1 + ReLU + 2x2 pool (cnn.lua:9-15): image in, pooled bf16 map out */
#define AOCR_PK_CONV1_BWD 3      /* its filter / bias gradient (window recomputed; no d(image)) */
#define AOCR_PK_BN_FWD 4         /* conv5's BatchNorm + ReLU (cnn.lua:32-33): finalize + apply pass (the sums come from the conv epilogue) */
#define AOCR_PK_BN_BWD 5         /* its backward: sums pass + apply pass */
#define AOCR_PK_UNPOOL 6         /* conv6's (2,1) un-pool + ReLU backward (cnn.lua:37-38) */
#define AOCR_PK_ATTN_DCTX 7      /* d(context) summed over the L decoder steps (model.lua:652-653) */
#define AOCR_PK_SPLITK 8         /* sum of conv6's split-K filter-gradient slabs */
#define AOCR_PK_LAST 8
int aocr_profile_kernel(aocr_model* m, int32_t which, int32_t iters, float* ms_per_launch, double* flops_per_launch);

/* Per-family timing of the fused step with HIP events on the model's stream (measurement only).  After
 * aocr_profile_enable(m, 1) every fused entry point records an event wherever the work changes family; aocr_profile_read
 * synchronises the stream, returns the milliseconds accumulated per family since the last read (ms[AOCR_PROF_FAMILIES]) and the
 * number of marks, and clears the record.  Families: */
#define AOCR_PROF_OTHER 0        /* weight shadows, zero fills, copies, loss, embedding */
#define AOCR_PROF_CONV_FWD 1     /* conv2..conv7 forward implicit GEMMs (cnn.lua:17-41) */
#define AOCR_PROF_CONV_DGRAD 2   /* their data gradients */
#define AOCR_PROF_CONV_WGRAD 3   /* their filter gradients */
#define AOCR_PROF_BN 4           /* BatchNorm(+ReLU) forward and backward (cnn.lua:23,32,41) */
#define AOCR_PROF_POOL_CONV1 5   /* conv1 forward / backward and the un-pool passes */
#define AOCR_PROF_ENC_SEQ 6      /* the encoder recurrences, forward and BPTT (model.lua:294-316, 664-690) */
#define AOCR_PROF_RNN_GEMM 7     /* hoisted input projections, projector, every LSTM / attention weight gradient */
#define AOCR_PROF_DEC_FWD 8      /* decoder step chain forward (model.lua:553-568) */
#define AOCR_PROF_DEC_BWD 9      /* decoder step chain BPTT (model.lua:643-661) */
#define AOCR_PROF_SGD 10         /* clip + update (optim_sgd.lua:38-95) */
#define AOCR_PROF_DECODE 11      /* beam / greedy decode chain (model.lua:376-536) */
#define AOCR_PROF_FAMILIES 12
int aocr_profile_enable(aocr_model* m, int32_t on);
int aocr_profile_read(aocr_model* m, float ms[AOCR_PROF_FAMILIES], int32_t* marks);

/* ---- module-level entry points (the nn.Module surface of the files under src/model) ---- */

/* C[M,N] (ldc) = op(A) * op(B) (+bias[n]) ; a_kmajor: 1 = A stored [M][K] (lda), 0 = [K][M];
 * b_kmajor: 1 = B stored [N][K] (ldb), 0 = [K][N].  nn.Linear forward is (1,1) with bias
 * (LSTM.lua:79-88), its gradInput (1,0), its gradWeight (0,0).
 * accumulate: bit field -- 1: C += (instead of C =), 2: ReLU on the result, 4: tanh on the result (nn.Tanh fused behind
 * nn.LinearNoBias, LSTM.lua:155-157); 0 / 1 keep their round-1 meaning. */
#define AOCR_GEMM_ACCUMULATE 1
#define AOCR_GEMM_RELU 2
#define AOCR_GEMM_TANH 4
int aocr_gemm(void* stream, int32_t compute, const float* A_dev, int64_t lda, int32_t a_kmajor,
              const float* B_dev, int64_t ldb, int32_t b_kmajor, float* C_dev, int64_t ldc,
              int32_t M, int32_t N, int32_t K, const float* bias_dev, int32_t accumulate);

/* cudnn.SpatialConvolution + cudnn.ReLU + cudnn.SpatialMaxPooling (cnn.lua:12-42), fused.
 * x (B,H,W,Cin) channels-last; w [Cout][k][k][Cin]; stride 1.  pool: 0 none, 1 = 2x2/2, 2 = kH2 kW1 / (2,1).
 * relu applies before the pool.  y is (B,Ho',Wo',Cout); idx (same shape, uint8, may be NULL when pool=0)
 * records the arg-max position inside the window. */
int aocr_conv2d_forward(void* stream, int32_t compute, const float* x_dev, const float* w_dev, const float* bias_dev,
                        float* y_dev, uint8_t* idx_dev, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                        int32_t ksize, int32_t pad, int32_t relu, int32_t pool);
/* gradInput / gradWeight+gradBias of the same layer w.r.t. the PRE-pool, PRE-relu output gradient dy (B,Ho,Wo,Cout). */
int aocr_conv2d_backward_data(void* stream, int32_t compute, const float* dy_dev, const float* w_dev, float* dx_dev,
                              int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t ksize, int32_t pad);
int aocr_conv2d_backward_filter(void* stream, int32_t compute, const float* x_dev, const float* dy_dev, float* dw_dev,
                                float* dbias_dev, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                                int32_t ksize, int32_t pad);
/* Routes d(pooled) back through max-pool + ReLU: dy (B,Ho,Wo,C) from dpooled, idx and pooled (>0 test). */
int aocr_unpool_relu_backward(void* stream, const float* dpooled_dev, const float* pooled_dev, const uint8_t* idx_dev,
                              float* dy_dev, int32_t B, int32_t Ho, int32_t Wo, int32_t C, int32_t pool);

/* First layer, cnn.lua:9-15 fused: (x-128)/128, conv 1->64 3x3 p1, ReLU, maxpool 2x2. x (B,32,W) -> y (B,16,W/2,64). */
int aocr_conv1_forward(void* stream, const float* x_dev, const float* w_dev, const float* bias_dev, float* y_dev,
                       int32_t B, int32_t H, int32_t W);
int aocr_conv1_backward(void* stream, const float* x_dev, const float* w_dev, const float* bias_dev,
                        const float* dy_pooled_dev, float* dw_dev, float* dbias_dev, int32_t B, int32_t H, int32_t W);

/* nn.SpatialBatchNormalization (+ the ReLU that follows it in cnn.lua:23-24,32-33,41-42).
 * x,y (rows,C) channels-last.  training: batch stats (biased var, eps 1e-5), running stats updated with
 * momentum 0.1 and unbiased var when update_running; save_dev gets [mean(C), invstd(C)].
 * tb_rows>0 writes y transposed from (B,T,C) to (T,B,C) with B = tb_rows (cnn.lua:44-45 + model.lua:288).
 * scratch_dev: AOCR_BN_SCRATCH_BYTES of device memory the call may overwrite (partial sums), shared between calls on one stream. */
#define AOCR_BN_SCRATCH_BYTES (8u << 20)
int aocr_batchnorm_relu_forward(void* stream, const float* x_dev, float* y_dev, const float* weight_dev,
                                const float* bias_dev, float* running_mean_dev, float* running_var_dev,
                                float* save_dev, void* scratch_dev, int64_t rows, int32_t C, int32_t training,
                                int32_t update_running, int32_t tb_rows);
/* dy_out = d/dx of relu(bn(x)) given dA (gradient at the ReLU output) and y (the ReLU output).  dweight/dbias accumulate. */
int aocr_batchnorm_relu_backward(void* stream, const float* x_dev, const float* y_dev, const float* dA_dev,
                                 const float* weight_dev, const float* save_dev, float* dx_dev, float* dweight_dev,
                                 float* dbias_dev, void* scratch_dev, int64_t rows, int32_t C, int32_t tb_rows);

/* One LSTM cell, LSTM.lua:79-105 (gate order in,forget,out,g; two biases): z = W_i2h x + b_i2h + W_h2h h_prev + b_h2h.
 * x (B,in), in and H multiples of 16.  Outputs c,h (B,H) and gates (B,4H) post-activation. */
int aocr_lstm_cell_forward(void* stream, int32_t compute, const float* x_dev, int32_t in_size, const float* h_prev_dev,
                           const float* c_prev_dev, const float* w_i2h_dev, const float* b_i2h_dev,
                           const float* w_h2h_dev, const float* b_h2h_dev, float* c_dev, float* h_dev,
                           float* gates_dev, int32_t B, int32_t H);
/* The same cell with the input part pre-computed, as the fused path hoists it out of the time loops (and for input widths that are
 * not multiples of 16: the decoder's first layer sees E + Hd = 532 columns): zx (B,4H) row stride ldzx = W_i2h x + b_i2h + b_h2h
 * (aocr_gemm with the summed bias), the call adds W_h2h h_prev and applies the gates. */
int aocr_lstm_cell_forward_zx(void* stream, int32_t compute, const float* zx_dev, int64_t ldzx, const float* h_prev_dev,
                              const float* c_prev_dev, const float* w_h2h_dev, float* c_dev, float* h_dev, float* gates_dev,
                              int32_t B, int32_t H);
/* Backward of the cell given d(c_out), d(h_out): writes dz (B,4H), dc_prev; dx/dh_prev via aocr_gemm(dz, W). */
int aocr_lstm_cell_backward(void* stream, const float* dc_dev, const float* dh_dev, const float* gates_dev,
                            const float* c_prev_dev, const float* c_dev, float* dz_dev, float* dc_prev_dev,
                            int32_t B, int32_t H);

/* create_decoder_attn, LSTM.lua:124-162, the score/softmax/context core given q = W_a h_top:
 * a = softmax_T(ctx . q), c = a . ctx.  ctx (B,T,Hd), q (B,Hd) -> a (B,T), c written at c_dev with row stride ldc. */
int aocr_attention_forward(void* stream, const float* ctx_dev, const float* q_dev, float* a_dev, float* c_dev,
                           int64_t ldc, int32_t B, int32_t T, int32_t Hd);
/* given dc (row stride lddc): ds (B,T) = softmax-backward of the scores, dq (B,Hd). d(ctx) is assembled over all
 * decoder steps by the fused path. */
int aocr_attention_backward(void* stream, const float* ctx_dev, const float* q_dev, const float* a_dev,
                            const float* dc_dev, int64_t lddc, float* ds_dev, float* dq_dev, int32_t B, int32_t T,
                            int32_t Hd);

/* Element-wise helpers of the module-level surface (n fp32 elements; y may alias a or b):
 *   AOCR_PW_ADD        y = a + b                  nn.CAddTable (LSTM.lua:88), gradient fan-in of a shared input
 *   AOCR_PW_TANH_BWD   y = a * (1 - b^2)          nn.Tanh:updateGradInput (a = gradOutput, b = the tanh OUTPUT; LSTM.lua:157)
 *   AOCR_PW_RELU_BWD   y = a * (b > 0)            cudnn.ReLU:updateGradInput where no pool follows (b = the ReLU output)
 *   AOCR_PW_RELU       y = max(a, 0)              cudnn.ReLU:updateOutput on its own (b ignored, may be NULL) */
#define AOCR_PW_ADD 0
#define AOCR_PW_TANH_BWD 1
#define AOCR_PW_RELU_BWD 2
#define AOCR_PW_RELU 3
int aocr_pointwise(void* stream, int32_t op, const float* a_dev, const float* b_dev, float* y_dev, int64_t n);

/* nn.LookupTable (LSTM.lua:55-56): out (n, E) = weight[ids - 1] for n 1-based int32 ids; backward accumulates
 * gradWeight[ids - 1] += gradOutput rows (accGradParameters).  weight / gradWeight (V, E). */
int aocr_lookup_forward(void* stream, const float* weight_dev, const int32_t* ids_dev, float* out_dev, int32_t n, int32_t E);
int aocr_lookup_backward(void* stream, const float* grad_out_dev, const int32_t* ids_dev, float* grad_weight_dev, int32_t n, int32_t E, int32_t V);

/* nn.LogSoftMax + nn.ClassNLLCriterion(weights; PAD weight 0; sizeAverage=false): output_projector.lua:6,
 * criterion.lua:3-8, model.lua:644-648.  logits (rows, ld) ; targets (rows) 1-based.  logp (rows,V) optional,
 * dlogits (rows, ld) optional = grad_scale * w[y] * (softmax - onehot); nll_rows (rows) per-row weighted NLL. */
int aocr_logsoftmax_nll(void* stream, const float* logits_dev, int64_t ld, const int32_t* targets_dev, float* logp_dev,
                        float* dlogits_dev, float* nll_rows_dev, int64_t rows, int32_t V, float grad_scale);

/* topk over beam*V candidates + finished-beam PAD masking, model.lua:399-404,446-458,516.
 * logp (B*kin, V); beam_scores (B,kout) in/out; prev_tok (B*kin) or NULL at t=1 (kin=1).
 * Outputs tokens (B,kout) 1-based, parents (B,kout) 0-based source beam. */
int aocr_beam_select(void* stream, const float* logp_dev, const int32_t* prev_tok_dev, float* beam_scores_dev,
                     int32_t* tokens_dev, int32_t* parents_dev, int32_t B, int32_t kin, int32_t kout, int32_t V);

/* The same selection under the dictionary constraint (model.lua:405-445, 460-513):
 * loc_in_dev (B*kin) trie node of every input beam (ignored at t=1, prev_tok_dev == NULL: all
 * beams start at node 0), loc_out_dev (B,kout) node of every selected beam.  V <= 64. */
int aocr_beam_select_dict(void* stream, const float* logp_dev, const int32_t* prev_tok_dev, float* beam_scores_dev,
                          int32_t* tokens_dev, int32_t* parents_dev, int32_t B, int32_t kin, int32_t kout, int32_t V,
                          const aocr_trie* trie, const int32_t* loc_in_dev, int32_t* loc_out_dev);

/* evalWordErrRate's comparison (utils.lua:136-175) on device: both (B,L) id rows are cut at
 * their first EOS (3) and string.levenshtein (utils.lua:55-94) is taken between them.
 * dist_dev (B) edit distance (0 <=> the word is right, :168-171); target_len_dev (B) or NULL:
 * length of the cut target (the denominator of the edit-distance accuracy, :172, README.md:11). */
int aocr_edit_distance(void* stream, const int32_t* labels_dev, const int32_t* targets_dev, int32_t B, int32_t L,
                       int32_t* dist_dev, int32_t* target_len_dev);

/* Lexicon snapping, the lexicon-based recognition of the literature: every prediction is replaced by the word of a list at the smallest
 * edit distance.  A word list in device memory: row w holds the 1-based vocab ids (1..255) of word w, then 0 up to `stride`.
 * A word has at most stride-1 ids; an all-zero row is the empty word.  stride: a multiple of 16, 16..256; words_dev 16-byte aligned. */
typedef struct aocr_lexicon {
  const uint8_t* words_dev;    /* (n_words, stride) */
  int32_t n_words, stride;
} aocr_lexicon;

/* Bytes of device scratch aocr_lexicon_nearest needs for B rows against n_words words (0 for a list one workgroup per row covers). */
size_t aocr_lexicon_scratch_bytes(int32_t B, int32_t n_words);

/* For every row b of labels_dev (B, L) int32, cut at its first EOS (3) exactly as aocr_edit_distance cuts it:
 *   index_dev[b] = the word w in [row_begin[b], row_begin[b+1]) with the smallest string.levenshtein distance
 *                  (utils.lua:55-94, unit costs) to the cut row; ties go to the LOWEST w;
 *   dist_dev[b]  = that distance.
 * row_begin_dev (B+1) int32, non-decreasing: per-image lexicons (rows search disjoint or overlapping slices of one list);
 * NULL = every row searches [0, n_words).  An empty range gives index -1, dist -1.  The bounds read from row_begin_dev are
 * clamped to [0, n_words] on the device; a label id outside 1..255 before the EOS matches no lexicon id.
 * L <= 64.  B == 0 is a no-op.  Enqueues only, never synchronises; the result does not depend on launch geometry or run
 * (bit-identical between calls). */
int aocr_lexicon_nearest(void* stream, const int32_t* labels_dev, int32_t B, int32_t L, const aocr_lexicon* lex,
                         const int32_t* row_begin_dev, void* scratch_dev, int32_t* index_dev, int32_t* dist_dev);

/* ---- data path ----------------------------------------------------------------------------------
 * data_gen.lua:68-79: img = 255 * image.rgb2y(img); img = image.scale(img, imgW, 32) for every decoded image of a batch
 * (all images of a batch share imgW: the loader buckets by width, data_gen.lua:91-99).
 * src_dev: the decoded images back to back, uint8, interleaved HWC with 1 (already gray) or 3 (RGB) channels;
 * desc_dev[i]: where image i starts and its size; out_dev (n_images, 1, out_h, out_w) fp32 in 0..255.
 * Arithmetic: single precision, operation for operation that of torch/image's rgb2y and scaleBilinear (rows to out_w first,
 * then columns to out_h; enlarging interpolates with scale (src-1)/(dst-1), shrinking averages the covered source span). */
typedef struct aocr_image_desc {
  int64_t offset;      /* byte offset of the image inside src_dev */
  int32_t height, width, channels, reserved;
} aocr_image_desc;
int aocr_preprocess_lines(void* stream, const uint8_t* src_dev, const aocr_image_desc* desc_dev, int32_t n_images,
                          int32_t out_h, int32_t out_w, float* out_dev);

/* ---- training augmentation: affine warp, contrast / brightness, additive noise -----------------------------------------
 * in_dev, out_dev: (n_images, 1, H, W) fp32 in 0..255, the output layout of aocr_preprocess_lines; they must not alias.
 * warp_dev[i]: the record of image i.  Per output pixel (x, y), every operation one rounded single-precision op, in this order:
 *   sx = (m00*x + m01*y) + m02, sy = (m10*x + m11*y) + m12, clamped to [-1, W] and [-1, H] (NaN becomes -1);
 *   x0 = floor(sx), fx = sx - x0 (the same for y); the taps (x0,y0) (x0+1,y0) (x0,y0+1) (x0+1,y0+1) = a b c d read in_dev inside
 *   [0,W) x [0,H) and are `fill` elsewhere;  top = (1-fx)*a + fx*b, bot = (1-fx)*c + fx*d, s = (1-fy)*top + fy*bot;
 *   v = gain*s + offset;
 *   r = splitmix64(splitmix64(seed ^ counter*0xD1342543DE82EF95) + idx), idx = (i*H + y)*W + x (the construction of the dropout
 *   masks), u1 = (r >> 40) * 2^-24, u2 = ((r >> 16) & 0xFFFFFF) * 2^-24, v = v + noise*((u1 + u2) - 1): triangular on (-1, 1)
 *   times `noise`, variance noise^2 / 6;
 *   out = min(max(v, 0), 255).
 * The record (1,0,0, 0,1,0, 1,0, fill, 0) returns in_dev bit for bit; an integer translation returns shifted input and `fill`.
 * n_images <= 65535; n_images == 0 is a no-op.  The call only enqueues work. */
typedef struct aocr_warp {
  float m00, m01, m02;   /* source x = m00*x + m01*y + m02  (x, y: 0-based output pixel indices) */
  float m10, m11, m12;   /* source y = m10*x + m11*y + m12 */
  float gain, offset;    /* v = gain*s + offset (contrast g about mid-gray: offset = 128*(1-g) + brightness, folded on the host) */
  float fill;            /* value of the source outside the image, 0..255 */
  float noise;           /* amplitude of the additive triangular noise, 0 = none */
} aocr_warp;
int aocr_augment_lines(void* stream, const float* in_dev, const aocr_warp* warp_dev, int32_t n_images, int32_t H, int32_t W,
                       uint64_t seed, uint64_t counter, float* out_dev);

/* ---- scan degradation: elastic displacement, stroke weight, optical blur ---------------------------------------------------
 * What an affine map cannot do to a rendered glyph: wobble it locally, thicken or starve its strokes, soften its edges.  It runs before
 * aocr_augment_lines (ink, paper and optics come before the camera's map and the sensor's noise; a blur after the noise would remove it).
 * in_dev, out_dev: (n_images, 1, H, W) fp32 in 0..255, the layout of aocr_augment_lines; they must not alias.  rec_dev[i]: the record of
 * image i, composed by the host: the device computes no exp.  Three stages per output pixel (x, y) of image i, every float operation one
 * rounded single-precision op, in this order:
 *  1 elastic  nodes every `pitch` pixels, GX = (W-1)/pitch + 2 by GY = (H-1)/pitch + 2 of them (integer divisions); node (gx, gy) draws
 *             r = splitmix64(base_e + ((i*GY + gy)*GX + gx)), base_e = splitmix64(seed ^ counter*0xD1342543DE82EF95 ^ AOCR_DEGRADE_STREAM)
 *             (the constant keeps this stream apart from aocr_augment_lines' noise under the same seed and counter);
 *             u1 = (r >> 40) * 2^-24, u2 = ((r >> 16) & 0xFFFFFF) * 2^-24, dx = amp_x*((u1 + u1) - 1), dy = amp_y*((u2 + u2) - 1);
 *             gx = x / pitch, f = (float)(x - gx*pitch) * inv_pitch, ax = (f*f)*(3 - (f + f)) (smoothstep: no crease at a cell border); gy, ay
 *             from y alike; with p q r s = the dx of nodes (gx,gy) (gx+1,gy) (gx,gy+1) (gx+1,gy+1):
 *             top = (1-ax)*p + ax*q, bot = (1-ax)*r + ax*s, ex = (1-ay)*top + ay*bot; ey from the four dy alike;
 *             sx = x + ex, sy = y + ey, clamped to [-1, W] and [-1, H] (NaN becomes -1), then the four-tap bilinear rule of
 *             aocr_augment_lines on in_dev, taps outside the image reading `fill`: E(x, y);
 *  2 stroke   lo, hi = min, max of E over the 3x3 neighbourhood, coordinates clamped to the image;
 *             thick >= 0: t = thick, M = (1-t)*E + t*lo (ink is dark: the minimum spreads it);  else t = -thick, M = (1-t)*E + t*hi;
 *  3 blur     Bh(x,y) = w0*M(x,y), then for k = 1..4 in turn Bh = Bh + wk*(M(x-k,y) + M(x+k,y)), coordinates clamped to the image;
 *             Bv from Bh alike along y;  out = min(max(Bv, 0), 255).
 * The record (0, 0, pitch, 1/pitch, 0, {1,0,0,0,0}, fill) returns in_dev bit for bit; amp_x = amp_y = 0 switches stage 1 off at any pitch.
 * 1 <= H, W <= 16384; n_images <= 65535; n_images == 0 is a no-op.  Bad sizes, NULL or aliased pointers return an error before anything is
 * enqueued.  The records are device memory, which the call does not read: a record with pitch < 2 is rejected by the hosts that compose
 * records (aocr/degrade.py, lua/augment.lua) before they upload it, and the kernel leaves the image of such a record unwritten.
 * One launch; no intermediate image goes through HBM.  The call only enqueues; the result does not depend on launch geometry. */
#define AOCR_DEGRADE_STREAM 0x4445475241444531ull
typedef struct aocr_degrade {
  float amp_x, amp_y;    /* elastic amplitude in pixels, >= 0: a node moves its neighbourhood by up to this much */
  int32_t pitch;         /* spacing of the displacement nodes in pixels, >= 2 */
  float inv_pitch;       /* 1/pitch, computed on the host and cast to fp32 */
  float thick;           /* in [-1, 1]: > 0 darkens (thickens) strokes, < 0 lightens (thins) them */
  float taps[5];         /* w0..w4 of the symmetric 9-tap blur, normalised on the host in float64 (w0 + 2 (w1+..+w4) = 1) and cast to fp32 */
  float fill;            /* value of the source outside the image, 0..255 */
} aocr_degrade;
int aocr_degrade_lines(void* stream, const float* in_dev, const aocr_degrade* rec_dev, int32_t n_images, int32_t H, int32_t W,
                       uint64_t seed, uint64_t counter, float* out_dev);

/* ---- synthetic word lines: lexicon words rendered from a glyph atlas into a batch of line crops and its targets ---------
 * The reference's training set (train.lua:21) is rendered dictionary words stretched to 32 x 100; this renders such crops where the
 * train step reads them.  out_dev: (n_images, 1, H, W) fp32 in 0..255, the layout aocr_preprocess_lines writes and aocr_augment_lines
 * reads.  style_dev[i]: the record of image i, drawn by the host like aocr_warp.  Every float operation below is one rounded
 * single-precision op, in this order:
 *   word: the ids of lexicon row `word` up to its first 0 (n <= stride-1 ids); `word` outside [0, n_words) or `face` outside
 *         [0, n_faces) gives the empty word (paper only; its targets are those of the empty word);
 *   an id outside 4..n_glyphs+3 draws nothing and advances by 0 (it still appears in the targets);
 *   pens: sp = max(spacing, 0) (NaN -> 0); p_0 = 0, p_{k+1} = (p_k + adv_k) + sp, summed in this sequential order;
 *   per output pixel (x, y): u = (x - x0)*sx, v = (y - y0)*sy, each clamped to [-1, 16384] (NaN -> -1);
 *   glyph k = the largest k in [0, n) with p_k <= u (none if u < 0 or n = 0); lu = u - p_k;
 *   xi = floor(lu), fx = lu - xi, yi = floor(v), fy = v - yi; the taps (xi,yi) (xi+1,yi) (xi,yi+1) (xi+1,yi+1) = a b c d read glyph
 *   k's bitmap inside [0,gw) x [0,gh) and are 0 elsewhere or when there is no glyph;
 *   top = (1-fx)*a + fx*b, bot = (1-fx)*c + fx*d, s = (1-fy)*top + fy*bot (the order of aocr_augment_lines);
 *   out = min(max(bg + (fg - bg)*(s / 255), 0), 255), the division a true division: a 0/255 atlas blits exactly.
 * targets_dev, targets_eval_dev: (n_images, L) int32, the rows DataGen builds: targets[j] = GO(2) at j = 0, id_{j-1} while j-1 < n,
 * PAD(1) after; targets_eval[j] = id_j while j < n, EOS(3) at j = n, PAD after; a word longer than L-1 is cut by these rules.
 * Both may be NULL together: only the images are written.
 * n_images <= 65535; n_images == 0 is a no-op.  Enqueues only, never synchronises; the result does not depend on launch geometry. */
typedef struct aocr_glyph_atlas {
  const uint8_t* pixels_dev;    /* (n_faces, n_glyphs, gh, gw) ink coverage, 0 = paper, 255 = ink */
  const uint8_t* advance_dev;   /* (n_faces, n_glyphs) pen advance in atlas pixels, 0..gw */
  int32_t n_faces, n_glyphs, gh, gw;   /* glyph g draws vocab id g + 4; gh, gw in 1..64; n_glyphs in 1..252 */
} aocr_glyph_atlas;

typedef struct aocr_synth_style {      /* one per image, drawn by the host like aocr_warp */
  int32_t word, face;           /* lexicon row, atlas face */
  float spacing;                /* extra advance between glyphs, atlas pixels, >= 0 */
  float sx, sy;                 /* atlas pixels per output pixel, x and y */
  float x0, y0;                 /* output-pixel position of the text box's top-left corner */
  float fg, bg;                 /* ink and paper gray, 0..255 */
} aocr_synth_style;

int aocr_synth_lines(void* stream, const aocr_lexicon* lex, const aocr_glyph_atlas* atlas,
                     const aocr_synth_style* style_dev, int32_t n_images, int32_t H, int32_t W, int32_t L,
                     float* out_dev, int32_t* targets_dev, int32_t* targets_eval_dev);

/* ---- page segmentation: from a scanned page to the word crops aocr_recognize reads ---------------------------------------
 * The reference is fed cropped words (90kDICT32px); this finds them on a page by projection profiles and cuts them out, on the device.
 * It assumes horizontal lines in one column: a skewed page goes through aocr_estimate_skew and aocr_deskew_page (below) first; a multi-column
 * page is first cut into blocks by aocr_ink_integral and aocr_layout_blocks (further below), and each block is segmented on its own.
 * page_dev: gray uint8, H rows of W pixels, rows `pitch` bytes apart (pitch >= W); any base address and any pitch, nothing need be aligned.
 * 1 <= H, W <= 16384, H*W <= 2^26, 1 <= max_boxes <= 4096.  Steps, in order:
 *   1 histogram  h[v], 256 bins, of the page (only the Otsu threshold reads it);
 *   2 threshold  params.threshold when >= 0, else Otsu in double precision, every operation one rounded IEEE op: N = sum h, S = sum v*h[v]
 *                (int64); for t = 0..254 ascending: n0 += h[t], s0 += t*h[t] (integers), n1 = N - n0; t is skipped when n0 == 0 or n1 == 0;
 *                d = (double)s0*(double)n1 - (double)(S-s0)*(double)n0; score = (d*d) / ((double)n0*(double)n1); the first t with the strictly
 *                largest score wins.  No t qualifies (one gray value): the threshold is -1, nothing is ink, zero boxes;
 *                ink = (v <= threshold), or (v > threshold) with light_text;
 *   3 rows       row_ink[y] = ink pixels of row y;
 *   4 bands      maximal runs of rows with row_ink >= min_row_ink; neighbouring runs with <= merge_gap rows between them are one band (the gap
 *                is measured between the original runs; merging chains); bands lower than min_line_h are dropped; the rest, top to bottom,
 *                are lines 0, 1, ...;
 *   5 words      per band, col_ink[x] = ink pixels of column x inside the band's rows; columns with col_ink >= 1 form runs; word_gap == 0: one
 *                box from the band's first to its last ink column; else runs with fewer than word_gap empty columns between them are one
 *                word; words narrower than min_word_w are dropped (a band that loses all its words keeps its line number);
 *   6 boxes      a box spans its band's rows (not tightened per word: the words of a line keep their relative size and baseline); ink = the ink
 *                pixels inside the unpadded box; then x grows by pad_x and y by pad_y, clamped to the page.  Order: line, then x0.  The first
 *                max_boxes are written; rows of boxes_dev beyond them are untouched;
 *   7 counts     counts_dev[0] = boxes found (it may exceed max_boxes: that is how the caller sees truncation), [1] = lines, [2] = the
 *                threshold used, [3] = 0.
 * scratch_dev: aocr_segment_scratch_bytes(H, W, max_boxes) bytes, 16-byte aligned, overwritten by the call (0 and an error for bad sizes).
 * Enqueues only, never synchronises or allocates; the result does not depend on launch geometry, atomics order or run.  Invalid params or
 * sizes return an error before anything is enqueued. */
typedef struct aocr_segment_params {
  int32_t threshold;     /* 0..254: ink = (v <= threshold); -1: Otsu (above) */
  int32_t light_text;    /* 1: ink = (v > threshold) instead */
  int32_t min_row_ink;   /* >= 1: a row is a text row when its ink count >= this */
  int32_t merge_gap;     /* >= 0: text-row runs separated by <= merge_gap non-text rows are one band (0: never merges) */
  int32_t min_line_h;    /* >= 1: bands lower than this are dropped */
  int32_t word_gap;      /* 0: one box per band (first to last ink column); > 0: ink-column runs separated by fewer than
                            word_gap empty columns are one word */
  int32_t min_word_w;    /* >= 1: narrower words are dropped */
  int32_t pad_x, pad_y;  /* >= 0: every box grows by this much, clamped to the page */
  int32_t reserved;
} aocr_segment_params;

typedef struct aocr_box { int32_t x0, y0, x1, y1, line, ink; } aocr_box;   /* half-open [x0,x1) x [y0,y1) */

size_t aocr_segment_scratch_bytes(int32_t H, int32_t W, int32_t max_boxes);
int aocr_segment_page(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W,
                      const aocr_segment_params* params, void* scratch_dev, int32_t max_boxes,
                      aocr_box* boxes_dev, int32_t counts_dev[4]);

/* aocr_segment_page with one word gap per line, estimated from the line itself.  params.word_gap is one number for the whole page, and word
 * spacing is not: a headline above body text, a footnote or a caption under it, letter-spaced print and the blocks of a multi-column page set
 * in different sizes are wrongly cut by any single value.  Steps 1-4, 6 and 7 are those of aocr_segment_page, bit for bit; step 5 takes
 * gap_b in place of params.word_gap, for band b with rows [y0, y1), h = y1 - y0 (every division is a floor division of non-negative ints):
 *   runs      maximal runs r_0 .. r_m of columns with col_ink >= 1: nothing merged, min_word_w not applied yet (no ink column: m = 0);
 *   gaps      g_j = start(r_j) - end(r_(j-1)) for j = 1..m (ends are exclusive: the empty columns between two runs, >= 1); interior gaps only;
 *   bounds    lo = max(1, h * lo_percent / 100), hi = max(lo, h * hi_percent / 100), clip = min(hi, 255);
 *   histogram hist[min(g_j, clip)] += 1, 256 bins: a gutter or a tab cannot pull the classes apart (a gap of hi or more is a word gap whatever
 *             its size);
 *   split     t = the Otsu threshold of step 2 on hist, operation for operation (-1: no gap, or one distinct clipped length); with t >= 0,
 *             a = the largest occupied bin <= t, c = the smallest occupied bin > t, and est = (a + c + 1) >> 1, so a < est <= c; with
 *             t = -1, a = c = 0;
 *   decision  est is used when m >= min_gaps, t >= 0 and c * 100 >= a * ratio_percent; else est = max(1, h * default_percent / 100);
 *             gap_b = min(max(est, lo), hi);
 *   flags     0 estimated, 1 too few gaps (m < min_gaps), 2 one gap length (t = -1), 3 classes not separated (the ratio), the first that
 *             applies in this order; + 4 when the clamp changed the value (gap_b != est);
 *   words     runs with fewer than gap_b empty columns between them are one word; min_word_w, the boxes and the counts follow as in
 *             aocr_segment_page.
 * When every band ends with gap_b = G the boxes and counts are those of aocr_segment_page with word_gap = G.  The band height stands in for
 * the em.  Limits: h <= 16384 and the percents <= 400 keep h * percent below 2^23; a, c <= 255 and ratio_percent <= 100000 keep
 * a * ratio_percent below 2^25; m < 8192.
 * params: as for aocr_segment_page, but word_gap == 0 (one box per band) is an error; any other word_gap is not read.  boxes_dev and counts_dev
 * mean what they mean there, so aocr_crop_lines and aocr_estimate_slant take them unchanged.  spacing_dev: NULL, or max_lines >= 0 rows of 8
 * words, 4-byte aligned, disjoint from the page and the scratch: row b < min(lines, max_lines) = {gap_b, flags, m, a, c, h, 0, 0}; the other rows
 * are untouched.  scratch_dev: aocr_segment_spaced_scratch_bytes(H, W, max_boxes) bytes, 16-byte aligned.  The page is not read again: the
 * estimate works on the ink-column flags the words pass has staged.  Enqueues only, never synchronises or allocates; the result does not
 * depend on launch geometry, atomics order or run.  Invalid arguments return an error before anything is enqueued and leave the outputs
 * untouched. */
typedef struct aocr_spacing_params {
  int32_t min_gaps;        /* >= 1: a band with fewer interior gaps takes the default */
  int32_t lo_percent, hi_percent, default_percent;   /* of the band height; 1 <= lo <= default <= hi <= 400 */
  int32_t ratio_percent;   /* 100..100000: the word-gap class must start at ratio_percent / 100 times the end of the letter-gap class */
  int32_t reserved[3];     /* must be 0 */
} aocr_spacing_params;

size_t aocr_segment_spaced_scratch_bytes(int32_t H, int32_t W, int32_t max_boxes);
int aocr_segment_page_spaced(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W,
                             const aocr_segment_params* params, const aocr_spacing_params* spacing,
                             void* scratch_dev, int32_t max_boxes, aocr_box* boxes_dev, int32_t counts_dev[4],
                             int32_t max_lines, int32_t* spacing_dev);

/* The crops of a page: row i < n of out_dev (n_boxes, 1, out_h, out_w) fp32 is rectangle boxes_dev[i] of the page scaled to out_h x out_w with
 * the arithmetic of aocr_preprocess_lines on a one-channel image, operation for operation (rows to out_w first, then columns to out_h): the
 * result is bit-identical to aocr_preprocess_lines on a contiguous copy of the rectangle.  n = min(n_boxes, count_dev[0]) is read on the
 * device (count_dev = the counts of aocr_segment_page: no host sync in between); count_dev == NULL: n = n_boxes.  Box coordinates are
 * clamped to the page on the device before any read; a box that is empty after clamping gives a row of 255.0 (paper).  Rows >= n are
 * untouched.  n_boxes <= 65535; n_boxes == 0 is a no-op.  The page follows the rules of aocr_segment_page.  Enqueues only. */
int aocr_crop_lines(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W,
                    const aocr_box* boxes_dev, const int32_t* count_dev, int32_t n_boxes,
                    int32_t out_h, int32_t out_w, float* out_dev);

/* ---- page deskew: the slope of the text lines, and the shear that removes it, in front of aocr_segment_page ---------------------------
 * A scan is routinely off by a degree or two, and a skewed line smears its row profile into its neighbours.  aocr_estimate_skew finds the
 * slope by a sweep of sheared projection profiles, aocr_deskew_page removes it; both are integer arithmetic, specified exactly.  Every >>
 * is an arithmetic (floor) shift of a signed value; the limits keep every product inside int32.
 * The page follows the rules of aocr_segment_page: any base address, any pitch >= W, 1 <= H, W <= 16384, H*W <= 2^26.
 *   ink        the threshold is params.threshold when >= 0, else Otsu's: steps 1-2 of aocr_segment_page, bit for bit;
 *              ink = (v <= threshold), or (v > threshold) with light_text; an Otsu threshold of -1 (one gray value): nothing is ink;
 *   strips     columns in groups of 32: b = x >> 5, nb = ceil(W / 32) (the last strip may be narrower); R[b][y] = ink pixels of row y
 *              inside strip b, 0..32;
 *   offsets    candidates k = -K..K (K = n_steps), slope_k = k * step_q16 rows per column in Q16;  cx = W >> 1, c_b = 32*b + 16 (also for
 *              a narrow last strip);  off_k(b) = ((c_b - cx) * slope_k + 32768) >> 16;  D_k = max over b of |off_k(b)|;
 *   profile    P_k[r] = sum over b of R[b][r + off_k(b)] for r in [-D_k, H + D_k); a term whose row r + off_k(b) is outside [0, H) is 0:
 *              every ink pixel lands in exactly one r, all candidates see the same total;
 *   score      score_k = sum over r of P_k[r]^2, an exact unsigned 64-bit integer (at most about 2^43);
 *   winner     candidates in the order 0, -1, +1, -2, +2, ...: the first with the strictly largest score.  A page without ink, an Otsu
 *              threshold of -1 or K = 0 give k = 0;
 *   outputs    skew_dev = [k, k * step_q16, the threshold used, 0];  scores_dev[k + K] = score_k for all 2K+1 candidates when not NULL.
 * Limits: step_q16 in 1..4096, K in 0..256, K * step_q16 <= 16384 (slope 0.25, 14 degrees).
 * scratch_dev: aocr_skew_scratch_bytes(H, W, n_steps) bytes, 16-byte aligned, overwritten by the call (0 and an error for bad sizes).
 * Enqueues only, never synchronises or allocates; the result does not depend on launch geometry, atomics order or run (integer sums
 * only).  Invalid params or sizes return an error before anything is enqueued. */
typedef struct aocr_skew_params {
  int32_t threshold;     /* 0..254: ink = (v <= threshold); -1: Otsu, steps 1-2 of aocr_segment_page, bit for bit */
  int32_t light_text;    /* 1: ink = (v > threshold) instead */
  int32_t step_q16;      /* 1..4096: slope difference between neighbouring candidates, rows per column, Q16 */
  int32_t n_steps;       /* K in 0..256: candidates k = -K..K, slope_k = k*step_q16; K*step_q16 <= 16384 (slope 0.25) */
} aocr_skew_params;

size_t aocr_skew_scratch_bytes(int32_t H, int32_t W, int32_t n_steps);
int aocr_estimate_skew(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W,
                       const aocr_skew_params* params, void* scratch_dev, int32_t skew_dev[4], uint64_t* scores_dev);

/* The page with the slope s taken out: a combined vertical and horizontal shear with nearest-neighbour sampling, integers only.
 *   s = skew_dev[1], read on the device (skew_dev = the output of aocr_estimate_skew: no host read in between), or slope_q16 when skew_dev
 *   is NULL; clamped to [-16384, 16384] on the device;  cx = W >> 1, cy = H >> 1;
 *   per output pixel (x, y):  sy = y + (((x - cx) * s + 32768) >> 16),  sx = x - (((y - cy) * s + 32768) >> 16);
 *   out[y][x] = page[sy][sx] when (sx, sy) is inside the page, else fill (0..255).
 * s = 0 copies the page bit for bit.  out_dev: H rows of W bytes, out_pitch >= W apart, any alignment; bytes between W and out_pitch are
 * untouched; it must not overlap the page.  Enqueues only. */
int aocr_deskew_page(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W,
                     const int32_t* skew_dev, int32_t slope_q16, int32_t fill, uint8_t* out_dev, int64_t out_pitch);

/* ---- page background flattening: uneven lighting divided out, in front of aocr_estimate_skew and aocr_segment_page ----------------------
 * One global threshold (Otsu's or a fixed one) separates ink from paper only when the paper has one brightness.  A photographed page, a book
 * gutter or an open scanner lid gives paper that is darker on one side than the ink is on the other.  This estimates the paper brightness
 * near every pixel and divides it out.  Integer arithmetic only, specified exactly; every / is a floor division of non-negative integers.
 * The page and the output follow the rules of aocr_deskew_page: any base address, any pitch >= W, 1 <= H, W <= 16384, H*W <= 2^26; out_dev:
 * H rows of W bytes, out_pitch >= W apart, any alignment; bytes between W and out_pitch are untouched; it must not overlap the page.
 *   v           page[y][x], or 255 - page[y][x] with light_text: the paper is the bright side from here on;
 *   window      of (x, y), r = radius: [max(x-r,0), min(x+r,W-1)] x [max(y-r,0), min(y+r,H-1)], clipped to the page, n(x,y) pixels;
 *   background  M[y][x] = the max of v over the window: paper is the brightest thing near a pixel while the window is wider than a stroke;
 *   smoothing   B[y][x] = (the sum of M over the window + (n >> 1)) / n: the rounded mean (the sum is < 2^24);
 *   division    Bc = max(B, 1);  out = min(255, (v*255 + (Bc >> 1)) / Bc);  with light_text the byte written is 255 - out.
 * Consequences: a pixel whose B is 255 is copied unchanged ((v*255 + 127) / 255 = v), so a clean page with paper at 255 comes back bit for
 * bit; a constant page c >= 1 becomes 255 everywhere, c = 0 stays 0 (light_text: 255 - that); r larger than H or W is legal: the window is
 * the whole page along that axis.  Limits: a bright speck lifts the background within r of it; solid ink wider than 2r+1 is read as dark
 * paper; gray pages only; this divides out multiplicative shading, not an additive fog.
 * scratch_dev: aocr_flatten_scratch_bytes(H, W, radius) bytes, 16-byte aligned, overwritten by the call (0 and an error for bad sizes).
 * Enqueues only, never synchronises or allocates; the result does not depend on launch geometry or run (integer maxima and sums only, no
 * atomics).  Invalid params, sizes or overlap return an error before anything is enqueued and leave out_dev untouched. */
typedef struct aocr_flatten_params {
  int32_t radius;        /* r in 1..127: windows are (2r+1) x (2r+1), clipped to the page; it must exceed the stroke width */
  int32_t light_text;    /* 1: light ink on dark paper (the page is inverted, flattened, inverted back) */
  int32_t reserved[2];   /* must be 0 */
} aocr_flatten_params;

size_t aocr_flatten_scratch_bytes(int32_t H, int32_t W, int32_t radius);
int aocr_flatten_page(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W,
                      const aocr_flatten_params* params, void* scratch_dev, uint8_t* out_dev, int64_t out_pitch);

/* ---- local adaptive binarisation: a threshold per pixel (Sauvola and Pietikainen), behind aocr_flatten_page and in front of every stage that
 * separates ink from paper ----------------------------------------------------------------------------------------------------------------
 * Every other page stage separates ink from paper with ONE threshold, fixed or Otsu's.  Faded print beside strong print, stains and foxing,
 * show-through and carbon copies have no such threshold, even on evenly lit paper: where a stain's paper (say 140) is darker than faded ink
 * elsewhere (say 175), every global threshold loses one or swallows the other.  This call thresholds every pixel against the mean and the
 * standard deviation of the window around it, and writes a page on which the fixed threshold 127 is that local decision.  Integer
 * arithmetic only, specified exactly; every / is a floor division of non-negative integers.  The page and the output follow the rules of
 * aocr_flatten_page: any base address, any pitch >= W, 1 <= H, W <= 16384, H*W <= 2^26; out_dev: H rows of W bytes, out_pitch >= W apart, any
 * alignment; bytes between W and out_pitch are untouched; it must not overlap the page.
 *   v          page[y][x], or 255 - page[y][x] with light_text: the paper is the bright side from here on;
 *   window     of (x, y), r = radius: [max(x-r,0), min(x+r,W-1)] x [max(y-r,0), min(y+r,H-1)], clipped to the page, n pixels (n <= 127^2);
 *   sums       S1 = the sum of v over the window, S2 = the sum of v*v;
 *   deviation  D = n*S2 - S1*S1 (>= 0, < 2^43);  q = floor(sqrt(D)), the exact integer square root: q*q <= D < (q+1)*(q+1);
 *   threshold  T = ( S1 * ((256 - k_q8)*range*n + k_q8*q) ) / (256*range*n*n): Sauvola's m*(1 + k*(s/R - 1)) with the mean m = S1/n, the
 *              standard deviation s = q/n, k = k_q8/256 and R = range; the numerator is < 2^53;
 *   decision   the pixel is ink when v <= T;
 *   output     hard = 1: ink 0, paper 255.  hard = 0 (the recogniser reads gray crops, and this keeps the anti-aliasing):
 *              ink out = (v*127) / max(T, 1), which is <= 127;  paper out = min(255, 128 + ((v - T - 1)*127) / max(254 - T, 1));
 *              with light_text the byte written is 255 - out.
 *   counts_dev [ink pixels, the smallest T, the largest T, 0] over the page (integer atomics: the order does not matter); may be NULL.
 * Consequences: is_ink(out, 127, light_text) -- out <= 127, or out > 127 with light_text -- is the local decision at every pixel, in both
 * modes, so every later stage run with the fixed threshold 127 sees exactly the Sauvola ink map.  A constant page c has q = 0 and
 * T = (c*(256 - k_q8)) / 256 < c for c >= 1 and k_q8 >= 1: nothing on it is ink (c = 0: everything is).  k_q8 = 0: T is the floored local
 * mean.  r larger than H or W is legal: the window is the whole page along that axis.
 * Limits: a glyph stroke wider than the window is hollowed out (its inside has no contrast to its window); a sharp edge between paper and
 * a stain darker than about 0.8 of it leaves a rim of ink just inside the stain (the window's mean there is well above the stain: an edge
 * wider than the window leaves none); k and the radius are untuned defaults for 300 dpi; this handles local contrast and does not replace aocr_flatten_page for strong shading across the page: the two
 * compose, flatten first.
 * scratch_dev: aocr_binarize_scratch_bytes(H, W, radius) bytes, 16-byte aligned (0 and an error for bad sizes); the window sums live in
 * registers and LDS, so the size is a small constant and the call leaves those bytes alone.  Enqueues only, never synchronises or allocates; the result does not
 * depend on launch geometry or run (integer sums; the double sqrt and division are stepped to the exact integers).  Invalid params, sizes
 * or overlap return an error before anything is enqueued and leave out_dev and counts_dev untouched. */
typedef struct aocr_binarize_params {
  int32_t radius;        /* r in 1..63: windows are (2r+1) x (2r+1), clipped to the page */
  int32_t k_q8;          /* k*256, 0..255 (default 51: k = 0.2) */
  int32_t range;         /* R, 1..255 (default 128): the dynamic range of the standard deviation */
  int32_t light_text;    /* 1: light ink on dark paper (the page is inverted, binarised, inverted back) */
  int32_t hard;          /* 0: gray output (above); 1: ink 0, paper 255 */
  int32_t reserved[3];   /* must be 0 */
} aocr_binarize_params;

size_t aocr_binarize_scratch_bytes(int32_t H, int32_t W, int32_t radius);
int aocr_binarize_page(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W,
                       const aocr_binarize_params* params, void* scratch_dev, uint8_t* out_dev, int64_t out_pitch, int32_t counts_dev[4]);

/* ---- page layout: the blocks of a multi-column page, in reading order, in front of aocr_segment_page -------------------------------------
 * aocr_segment_page takes its row profiles across the whole width of the page: the lines of two columns fall into one band and their words
 * come back interleaved.  These two calls cut the page into blocks (headline, columns, paragraphs) by a recursive XY cut; every block is
 * then a one-column page for aocr_segment_page (a view: its row stride is the page's pitch).  Integer arithmetic only, specified exactly.
 *
 * aocr_ink_integral: the ink mask and its summed-area table.  The page follows the rules of aocr_segment_page: any base address, any
 * pitch >= W, 1 <= H, W <= 16384, H*W <= 2^26.  threshold: 0..254, or -1 for Otsu: steps 1-2 of aocr_segment_page, bit for bit;
 * ink = (v <= threshold), or (v > threshold) with light_text; an Otsu threshold of -1 (one gray value): nothing is ink.
 *   sat_dev   (H+1) rows of (W+1) uint32, sat_pitch elements apart (sat_pitch >= W+1; the base 4-byte aligned).  Row 0 and column 0 are
 *             zero; S[y+1][x+1] = the number of ink pixels in [0,x] x [0,y].  Elements between W+1 and sat_pitch are untouched.  It must
 *             not overlap the page or the scratch.
 *   info_dev  [the threshold used, the total ink (= S[H][W]), 0, 0].
 * scratch_dev: aocr_integral_scratch_bytes(H, W) bytes, 16-byte aligned, overwritten by the call (0 and an error for bad sizes).
 *
 * aocr_layout_blocks: the recursive XY cut.  All ink counts come from the table, four reads per rectangle: the ink of [x0,x1) x [y0,y1) is
 * S[y1][x1] - S[y0][x1] - S[y1][x0] + S[y0][x0].  For a region R = [x0,x1) x [y0,y1):
 *   profiles  c[x] = the ink of column x within R's rows, r[y] = the ink of row y within R's columns; a column or row is occupied when its
 *             count >= min_ink;
 *   pieces    along an axis: the maximal runs of occupied elements; runs with fewer than `gap` unoccupied elements between them are one
 *             piece (the gap is measured between the original runs; merging chains, as words are formed in step 5 of aocr_segment_page);
 *             unoccupied elements before the first run and after the last belong to no piece;
 *   tighten   first x0..x1 becomes the first to the last occupied column of R, then y0..y1 the first to the last occupied row of the
 *             narrowed region: one pass each, no iteration.  No occupied column, or then no occupied row: R is empty and is dropped;
 *   levels    L_0 = [tighten(page)] at depth 0, or the empty list.  For d = 0 .. max_depth-1 every region of L_d that is not yet a leaf is
 *             cut: its column pieces with gap_x -- two or more: the children are piece.x x R.y, left to right; otherwise its row pieces
 *             with gap_y over R's full columns -- two or more: the children are R.x x piece.y, top to bottom; otherwise R becomes a leaf
 *             and keeps its place and its depth.  Columns first: a grid of four rectangles reads column by column.  Children are tightened
 *             once, at creation; empty ones are dropped; the rest replace their parent in place at depth d+1, so the list is always in
 *             reading order, the preorder of the cut tree.  If the list after level d would hold more than max_blocks regions, that
 *             level's cuts are discarded, the list stays as it was before level d, counts[3] = 1 and cutting stops.  Cutting also stops
 *             after a level that cut nothing;
 *   output    every region of the final list with w >= min_block_w, h >= min_block_h and ink >= min_block_ink becomes, in list order, a
 *             row {x0, y0, x1, y1, line = depth, ink} of blocks_dev; the others are dropped.  Rows beyond the written ones are untouched;
 *   counts    counts_dev = [blocks written, levels in which something was cut and kept, regions dropped by size, overflow flag].
 * sat_dev, sat_pitch, H, W: the table of aocr_ink_integral (any table with these properties).  1 <= max_blocks <= 1024.
 * Limits: an XY cut cannot separate L-shaped or interleaved regions; a headline wider than one column but narrower than the page blocks
 * the gutter beneath it only as far as it reaches; aligned word gaps on a page of very few lines can look like a gutter (gap_x is the
 * control); paragraph gaps that line up across both columns are cut before the gutter is (the blocks then read row of paragraphs by row).
 * scratch_dev: aocr_layout_scratch_bytes(H, W, max_blocks) bytes, 16-byte aligned, overwritten by the call (0 and an error for bad sizes).
 * Both calls enqueue only, never synchronise or allocate; the results do not depend on launch geometry, atomics order or run.  Invalid
 * params, sizes, NULLs or overlap return an error before anything is enqueued and leave the outputs untouched. */
size_t aocr_integral_scratch_bytes(int32_t H, int32_t W);
int aocr_ink_integral(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W,
                      int32_t threshold, int32_t light_text, void* scratch_dev,
                      uint32_t* sat_dev, int64_t sat_pitch, int32_t info_dev[4]);

typedef struct aocr_layout_params {
  int32_t min_ink;      /* >= 1: a column (row) of a region is occupied when its ink inside the region >= this */
  int32_t gap_x;        /* >= 1: occupied-column runs with fewer than gap_x unoccupied columns between them are one piece */
  int32_t gap_y;        /* >= 1: the same for rows */
  int32_t max_depth;    /* 1..16 levels of cuts */
  int32_t min_block_w, min_block_h, min_block_ink;   /* >= 1: smaller leaves are dropped at the end */
  int32_t reserved;     /* must be 0 */
} aocr_layout_params;

size_t aocr_layout_scratch_bytes(int32_t H, int32_t W, int32_t max_blocks);
int aocr_layout_blocks(void* stream, const uint32_t* sat_dev, int64_t sat_pitch, int32_t H, int32_t W,
                       const aocr_layout_params* params, void* scratch_dev, int32_t max_blocks,
                       aocr_box* blocks_dev, int32_t counts_dev[4]);

/* ---- page cleaning: connected components of the ink; specks and rules painted over, in front of aocr_estimate_skew and aocr_segment_page --
 * Everything above reads projection profiles of the thresholded page, and a profile cannot tell a word from a speck or a ruled line: one
 * dark pixel makes a text row (min_row_ink = 1) and an occupied column (step 5), one vertical rule joins every line it passes into one band,
 * one underline joins the words of its line into one box.  These two calls label the ink, measure every component and delete the ones that
 * cannot be text.  Integer arithmetic only, specified exactly.
 *
 * aocr_label_components.  The page follows the rules of aocr_segment_page: any base address, any pitch >= W, 1 <= H, W <= 16384,
 * H*W <= 2^26.  threshold: 0..254, or -1 for Otsu: steps 1-2 of aocr_segment_page, bit for bit; ink = (v <= threshold), or (v > threshold)
 * with light_text; an Otsu threshold of -1 (one gray value): nothing is ink.
 *   neighbours  connectivity is 4 or 8: two ink pixels are neighbours when they differ by 1 in x or in y (4), or by at most 1 in both and
 *               are not the same pixel (8).  A component is a maximal set of ink pixels connected through neighbours;
 *   labels_dev  H rows of W int32, labels_pitch elements apart (labels_pitch >= W; the base 4-byte aligned); elements between W and
 *               labels_pitch are untouched.  Paper is -1; an ink pixel carries the smallest y*W + x of any pixel of its component: the
 *               component's first pixel in raster order (W, not the pitch: indices fit int32 because H*W <= 2^26).  It must not overlap
 *               the page or the scratch;
 *   comps_dev   may be NULL.  Otherwise the components in ascending label order (the raster order of their first pixels) as rows
 *               {x0, y0, x1, y1, line = label, ink = area}: the half-open tight box and the number of pixels.  Only the first
 *               max_components are written (1 <= max_components <= 65536); rows beyond them are untouched;
 *   info_dev    [the threshold used, the total ink, components found, 0].  Components found may exceed max_components: that is how the
 *               caller sees truncation.
 * scratch_dev: aocr_components_scratch_bytes(H, W) bytes, 16-byte aligned, overwritten by the call (0 and an error for bad sizes): about
 * 8 bytes per pixel (one 16-byte record per pixel pair), 516 MiB at H*W = 2^26, 67 MiB for A4 at 300 dpi.
 *
 * aocr_clean_page: the page with its specks and rules painted over.  Components as above (params.threshold, light_text, connectivity), each
 * with its area and its tight box of w x h pixels:
 *   speck       area < min_area (min_area = 1: nothing is a speck);
 *   rule        not a speck, and w > max_w or h > max_h (a limit of 0 switches that test off).  Specks are tested first: a short dash is a
 *               speck, never a rule;
 *   output      out[y][x] = fill when the pixel is ink and its component is a speck or a rule, fill = 255, or 0 with light_text; every
 *               other byte is copied bit for bit.  A page with nothing to remove comes back identical; an Otsu threshold of -1 copies it;
 *   counts      counts_dev = [components, specks removed, rules removed, the threshold used, the total ink, ink pixels removed, 0, 0]
 *               (4-byte aligned).
 * out_dev follows the rules of aocr_deskew_page: H rows of W bytes, out_pitch >= W apart, any alignment; bytes between W and out_pitch are
 * untouched; it must not overlap the page (or the scratch).  The labels live in the scratch; this call does not expose them.
 * Limits: a character that touches a rule goes with it (an underline through descenders takes them along); min_area above the area of an
 * i-dot or a full stop deletes those; a figure is one big component and is removed by max_w / max_h, which is intended: what is left is
 * what the recogniser can read.
 * scratch_dev: aocr_clean_scratch_bytes(H, W) bytes, 16-byte aligned, overwritten by the call (0 and an error for bad sizes): the above
 * plus the labels, about 12 bytes per pixel, 772 MiB at H*W = 2^26, 100 MiB for A4 at 300 dpi.
 * Both calls enqueue only, never synchronise or allocate; the results do not depend on launch geometry, atomics order or run (the labels
 * are canonical; sums, minima and maxima of integers).  Invalid params, sizes, NULLs, a bad connectivity or overlap return an error before
 * anything is enqueued and leave the outputs untouched. */
size_t aocr_components_scratch_bytes(int32_t H, int32_t W);
int aocr_label_components(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W,
                          int32_t threshold, int32_t light_text, int32_t connectivity, void* scratch_dev,
                          int32_t* labels_dev, int64_t labels_pitch,
                          int32_t max_components, aocr_box* comps_dev, int32_t info_dev[4]);

typedef struct aocr_clean_params {
  int32_t threshold;     /* 0..254: ink = (v <= threshold); -1: Otsu, steps 1-2 of aocr_segment_page, bit for bit */
  int32_t light_text;    /* 1: ink = (v > threshold) instead; removed pixels become 0 instead of 255 */
  int32_t connectivity;  /* 4 or 8 */
  int32_t min_area;      /* >= 1: a component with area < min_area is a speck (1: none is) */
  int32_t max_w, max_h;  /* >= 0: a component that is no speck and whose box is wider than max_w or higher than max_h is a rule
                            (0: that test is off) */
  int32_t reserved[2];   /* must be 0 */
} aocr_clean_params;

size_t aocr_clean_scratch_bytes(int32_t H, int32_t W);
int aocr_clean_page(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W,
                    const aocr_clean_params* params, void* scratch_dev, uint8_t* out_dev, int64_t out_pitch,
                    int32_t counts_dev[8]);

/* ---- rule removal that keeps the text: run-length rules per pixel, after aocr_deskew_page / aocr_dewarp_page, before layout and segmentation --
 * aocr_clean_page removes a rule only as a whole connected component, and a character that touches it goes with it: a word on its form
 * line, an underlined word with a g, p or y, every cell text that touches a table grid.  The rule and the glyph are one component, so the
 * decision is made per pixel, from run lengths: a rule is long one way and thin the other, and a stroke that crosses it is not thin.
 * Integer arithmetic only, specified exactly.
 *
 * The page and the output follow the rules of aocr_clean_page: any base address, any pitch >= W, 1 <= H, W <= 16384, H*W <= 2^26; out_dev
 * is H rows of W bytes, out_pitch >= W apart, bytes between W and out_pitch are untouched; the output, the page and the scratch must not
 * overlap; counts_dev may be NULL (else 8 int32, 4-byte aligned, apart from the three).
 *   ink         as everywhere: threshold 0..254, or -1 for Otsu (steps 1-2 of aocr_segment_page, bit for bit); ink = (v <= threshold), or
 *               (v > threshold) with light_text; an Otsu threshold of -1 (one gray value): nothing is ink and the page is copied;
 *   runs        for an ink pixel p = (y, x): its row run is the maximal run of ink in row y through p, columns [c, d); its column run the
 *               maximal run of ink in column x through p, rows [a, b).  Runs end at the page's edge;
 *   candidates  with L = min_len, T = max_thick, e = edge:  Hc(p): axes & 1, p is ink and d - c >= L;  Vc(p): axes & 2, p is ink and
 *               b - a >= L.  Hc is the opening of the ink by a 1 x L segment, Vc the opening by an L x 1 segment;
 *   erased      out[y][x] = fill (255, or 0 with light_text) when one of the following holds; every other byte is copied bit for bit:
 *                 cross  Hc(p) and Vc(p): where two rules cross, neither is thin;
 *                 byH    b - a <= T and some y' in [max(a, y - e), min(b - 1, y + e)] has Hc(y', x): a thin column run that belongs to a
 *                        long row run; with e > 0 that includes the ragged rows directly above and below the run;
 *                 byV    d - c <= T and some x' in [max(c, x - e), min(d - 1, x + e)] has Vc(y, x').
 *               Because L > T, Hc(p) excludes byV and Vc(p) excludes byH: the classes need no precedence beyond counting cross first, then
 *               byH, then byV.  A descender that crosses an underline has a column run longer than T, so every pixel of it stays, the
 *               ones inside the rule's rows included;
 *   counts      counts_dev = [the threshold used, the total ink, pixels erased, of them cross, of them byH and not cross, of them byV only,
 *               candidate pixels kept ((Hc or Vc) and not erased: the strokes that cross a rule), 0].
 * Limits: a rule thicker than T stays (all of it: none of its column runs is thin); dashed or dotted leaders are runs shorter than L; on
 * a page that was not deskewed a rule of thickness t at slope s has runs of only about t / s pixels; the bottoms of letters that sit on
 * a rule lose the rows within e of it; a headline stroke longer than L and no thicker than T is a rule.
 * scratch_dev: aocr_rules_scratch_bytes(H, W) bytes, 16-byte aligned, overwritten by the call (0 and an error for bad sizes): three bit
 * planes (ink, Hc, Vc: one uint64 per 64 columns of a row), one word per column and 64 rows, a histogram and a header: 7 / 16 of a byte
 * per pixel, 3.7 MiB for A4 at 300 dpi, 28 MiB at H*W = 2^26.
 * The call enqueues only, never synchronises or allocates; the result is a function of the page and the params alone (integer sums: no
 * dependence on launch geometry or atomics order).  Invalid params (L <= T, T outside 1..16, e outside 0..4, axes outside 1..3, non-zero
 * reserved), bad sizes, NULLs or overlap return an error before anything is enqueued and leave the outputs untouched.  A page with
 * nothing to erase comes back identical. */
typedef struct aocr_rule_params {
  int32_t threshold;    /* 0..254, or -1: Otsu, steps 1-2 of aocr_segment_page, bit for bit */
  int32_t light_text;   /* 1: ink = (v > threshold); erased pixels become 0 instead of 255 */
  int32_t axes;         /* 1 horizontal rules, 2 vertical rules, 3 both */
  int32_t min_len;      /* L: a run of at least L ink pixels is a rule candidate; max_thick < L <= 16384 */
  int32_t max_thick;    /* T in 1..16: a rule is at most T pixels thick */
  int32_t edge;         /* e in 0..4: ragged-edge pixels within e pixels of a candidate go with it */
  int32_t reserved[2];  /* must be 0 */
} aocr_rule_params;

size_t aocr_rules_scratch_bytes(int32_t H, int32_t W);
int aocr_remove_rules(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W,
                      const aocr_rule_params* params, void* scratch_dev, uint8_t* out_dev, int64_t out_pitch,
                      int32_t counts_dev[8]);

/* ---- reversed-out panels: find the dark slabs that carry light text and invert them, after aocr_resize_page, before aocr_clean_page ---------
 * light_text is one flag for the whole page, but a table header row, a form's section bar, a magazine banner or a sidebar box is white
 * text on a dark slab.  To aocr_segment_page the slab is one huge box that holds no readable crop; aocr_clean_page paints it over as a
 * figure (max_w / max_h), and the words on it go with it.  This stage finds the slabs among the connected components of the ink and
 * replaces the bytes inside them by 255 - v, so that every later stage sees dark text on light paper there too.  Integer arithmetic
 * only, specified exactly; every product that can pass 2^31 is formed in 64 bits.
 *
 * The page and the output follow the rules of aocr_clean_page: any base address, any pitch >= W, 1 <= H, W <= 16384, H*W <= 2^26; out_dev
 * is H rows of W bytes, out_pitch >= W apart, bytes between W and out_pitch are untouched; 1 <= max_panels <= 1024; counts_dev is 8
 * int32 and panels_dev, which may be NULL, max_panels rows of 8 int32, both 4-byte aligned; the page, the output, the scratch, panels_dev
 * and counts_dev must not overlap one another.
 *   ink, components  exactly those of aocr_label_components for threshold, light_text and connectivity (the same launches): threshold
 *               0..254, or -1 for Otsu (steps 1-2 of aocr_segment_page, bit for bit); ink = (v <= threshold), or (v > threshold) with
 *               light_text (the page is dark then and a panel is a light slab); a component's label is the raster index of its first pixel;
 *   candidate   a component whose tight box [x0, x1) x [y0, y1) has x1 - x0 >= min_w and y1 - y0 >= min_h.  Candidates are taken in
 *               ascending label order, the raster order of their first pixels, and only the first max_panels of them are examined;
 *   span        for an examined candidate c and a row y of its box, lo(y) is the smallest x whose label is c and hi(y) the largest such x
 *               plus one (a connected component has a pixel in every row of its box, so every row has a span);  hull = the sum over
 *               the rows of hi - lo.  The spans are the row-convex hull of the component: because the region is the hull and not the box,
 *               a rounded, elliptical or slightly rotated panel is not inverted outside itself;
 *   panel       an examined candidate with  area * 100 >= fill_percent * hull  and  (hull - area) * 100 >= min_inside_percent * hull.
 *               The first test keeps out glyphs, figures and blotchy photographs; the second keeps out solid bars with nothing written
 *               on them, which are left to aocr_clean_page and aocr_remove_rules; min_inside_percent = 0 switches the second test off;
 *   output      out[y][x] = 255 - page[y][x] when some panel has y in its box and lo(y) <= x < hi(y); every other byte is copied bit for
 *               bit.  A pixel inside the spans of two panels is inverted once, not twice: its source is always the page, never the
 *               output.  A page with no panel comes back identical; an Otsu threshold of -1 (one gray value) copies the page;
 *   panels_dev  one row of 8 int32 per examined candidate, in label order: {x0, y0, x1, y1, label, area, hull, accepted (1 or 0)}; rows
 *               beyond the examined candidates are untouched;
 *   counts_dev  [components, candidates found, candidates examined, panels inverted, the threshold used, the total ink, the sum of the
 *               inverted panels' hulls (capped at 2^31 - 1: hulls of nested rings can add up past it), 0].  candidates found >
 *               max_panels is how the caller sees that the list was cut short; later candidates are not inverted.
 * Limits: one level only -- a dark box inside a light box inside a panel comes out reversed; anti-aliased rim pixels of a panel that sit
 * above the threshold are not part of the component and stay gray, a thin gray frame around the inverted slab; a solid bar without text
 * is not a panel unless min_inside_percent is 0; a slab that touches other ink (a table grid drawn in the same dark) is one component
 * with it and is judged with it.  The defaults of the Python mirror (min_w 64, min_h 24, fill_percent 60, min_inside_percent 2) are a
 * judgement for text at 300 dpi and nobody has tuned them on real scans.
 * scratch_dev: aocr_panels_scratch_bytes(H, W, max_panels) bytes, 16-byte aligned, overwritten by the call (0 and an error for bad
 * sizes): the scratch of aocr_label_components, the label plane (4 bytes per pixel), one word per 64 columns of a row, and 8 bytes per
 * (candidate, row): max_panels * H spans.
 * The call enqueues only, never synchronises or allocates; the result is a function of the page and the params alone (integer sums,
 * minima and maxima: no dependence on launch geometry, atomics order or run).  Invalid params (connectivity other than 4 or 8, min_w or
 * min_h < 1, fill_percent outside 1..100, min_inside_percent outside 0..99, fill_percent + min_inside_percent > 100, non-zero
 * reserved), bad sizes, NULLs or overlap return an error before anything is enqueued and leave every output untouched. */
typedef struct aocr_panel_params {
  int32_t threshold;           /* 0..254, or -1: Otsu, steps 1-2 of aocr_segment_page, bit for bit */
  int32_t light_text;          /* 1: ink = (v > threshold): the page is dark, a panel is a light slab */
  int32_t connectivity;        /* 4 or 8 */
  int32_t min_w, min_h;        /* >= 1: a candidate's tight box is at least this wide and this high */
  int32_t fill_percent;        /* 1..100: a panel's ink fills at least this share of its hull */
  int32_t min_inside_percent;  /* 0..99, fill_percent + min_inside_percent <= 100: at least this share of the hull is not ink */
  int32_t reserved;            /* must be 0 */
} aocr_panel_params;

size_t aocr_panels_scratch_bytes(int32_t H, int32_t W, int32_t max_panels);
int aocr_invert_panels(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W,
                       const aocr_panel_params* params, void* scratch_dev, uint8_t* out_dev, int64_t out_pitch,
                       int32_t max_panels, int32_t* panels_dev, int32_t counts_dev[8]);

/* ---- page orientation: quarter turns, and which way the text lines run, in front of aocr_estimate_skew ------------------------------------
 * Every stage above reads row profiles and assumes that the lines run along x; aocr_estimate_skew sweeps slopes up to 0.25 only.  A page
 * fed sideways or upside down is turned here, on the device.  Integer arithmetic only, specified exactly.
 *
 * aocr_rotate_page: the page turned by q clockwise quarter turns, exactly numpy.rot90(page, -q):
 *   q        = (quarter + (orient_dev ? (orient_dev[0] & 2) : 0)) & 3.  quarter is 0..3: the host fixes the odd part, because it changes the
 *            output's shape; the device may add a half turn, which does not: orient_dev[0] is read on the device (no host read in
 *            between, as aocr_deskew_page reads skew_dev); its odd bit is ignored;
 *   shape    the output has Ho x Wo pixels, out_pitch >= Wo:  Ho, Wo = H, W for an even quarter, W, H for an odd one;
 *   q = 0    out[y][x] = page[y][x]                 q = 1    out[y][x] = page[H-1-x][y]
 *   q = 2    out[y][x] = page[H-1-y][W-1-x]         q = 3    out[y][x] = page[x][W-1-y]
 * The page follows the rules of aocr_deskew_page: any base address, any pitch >= W, 1 <= H, W <= 16384, H*W <= 2^26; out_dev: Ho rows of Wo
 * bytes, out_pitch >= Wo apart, any alignment; bytes between Wo and out_pitch are untouched; it must not overlap the page.  No scratch.
 * Enqueues only; the result does not depend on launch geometry.  Invalid sizes, NULLs, a quarter outside 0..3 or overlap return an error
 * before anything is enqueued.
 *
 * aocr_estimate_orientation: which way the lines run, from where ink runs start.
 *   ink      the threshold is `threshold` when 0..254, else (-1) Otsu's: steps 1-2 of aocr_segment_page, bit for bit; ink = (v <= threshold),
 *            or (v > threshold) with light_text; an Otsu threshold of -1 (one gray value): nothing is ink;
 *   N_h      the number of ink pixels whose left neighbour (x-1, y) is paper or off the page: the starts of the runs along x;
 *   N_v      the number of ink pixels whose upper neighbour (x, y-1) is paper or off the page: the starts of the runs along y;
 *   axis     1 when N_v > N_h, else 0 (a tie keeps the page): the clockwise quarter turns proposed.  Latin text is mostly vertical strokes: a
 *            stroke h rows high starts h runs along x and one along y, so N_h > N_v when the lines run along x;
 *   output   orient_dev = [axis, N_h, N_v, the threshold used, the total ink, 0, 0, 0] (4-byte aligned).
 * All sums are exact integers, at most 2^26.  A quarter turn of the page swaps N_h and N_v exactly, a half turn leaves both unchanged: the
 * call cannot tell an upright page from one upside down, and the caller chooses between axis and axis + 2 by other means (Model.recognize_page
 * in the Python host asks the recogniser).  Limits: the margin is thin -- on rendered lowercase text max(N_h, N_v) / min(N_h, N_v) goes down to
 * 1.03 -- and a page of digits alone decides wrongly (digits are round); N_h and N_v are returned so that a caller can reject a thin margin.
 * scratch_dev: aocr_orient_scratch_bytes(H, W) bytes, 16-byte aligned, overwritten by the call (0 and an error for bad sizes).
 * Enqueues only, never synchronises or allocates; the result does not depend on launch geometry, atomics order or run (integer sums
 * only).  Invalid sizes, a bad threshold or NULLs return an error before anything is enqueued. */
int aocr_rotate_page(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W,
                     const int32_t* orient_dev, int32_t quarter, uint8_t* out_dev, int64_t out_pitch);
size_t aocr_orient_scratch_bytes(int32_t H, int32_t W);
int aocr_estimate_orientation(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W,
                              int32_t threshold, int32_t light_text, void* scratch_dev, int32_t orient_dev[8]);

/* ---- page rectification: the paper's four corners on a photograph, and the projective warp to the upright page, in front of everything ------
 * A photographed page is a quadrilateral on a darker (or lighter) desk, seen in perspective: the lines converge (keystone), which no shear
 * removes, and aocr_flatten_page would divide the desk out to paper.  These three calls find the paper, plan the map and resample.  The
 * page follows the rules of aocr_segment_page: gray uint8, any base address, any pitch >= W, 1 <= H, W <= 16384, H*W <= 2^26.
 *
 * aocr_find_page_quad (device): the four corners of the paper.  Integer arithmetic only, specified exactly.
 *   threshold  `threshold` when 0..254, else (-1) Otsu's: steps 1-2 of aocr_segment_page, bit for bit;
 *   paper      (v > threshold), or (v <= threshold) with dark_paper; an Otsu threshold of -1 (one gray value): nothing is paper;
 *   sheet      the 8-connected components of the paper mask as aocr_label_components defines them (label = the smallest y*W + x); the sheet
 *              is the component of the largest area, a tie goes to the smallest label.  Text holes in the sheet do not matter;
 *   corners    over the sheet's pixels (x, y), exact integer keys with exact ties:
 *                TL minimises (x+y, then y);    TR maximises (x-y, then -y);
 *                BR maximises (x+y, then y);    BL minimises (x-y, then -y);
 *   valid      with P0..P3 = TL, TR, BR, BL: 1 when a sheet exists and all four cross products (P[i+1]-P[i]) x (P[i+2]-P[i+1]), indices
 *              mod 4, in int64, are > 0 (y points down: the order is clockwise); else 0;
 *   output     quad_dev = [x_tl, y_tl, x_tr, y_tr, x_br, y_br, x_bl, y_bl, the threshold used, the sheet's area, components found, valid,
 *              0, 0, 0, 0] (4-byte aligned); with no sheet the eight coordinates are 0.
 * Limits: the sheet must be turned by less than about 45 degrees, so that each corner is the extreme along its diagonal; rounded or
 * dog-eared corners move the estimate; a page that fills the frame yields the image corners, and rectifying it is then close to a copy; the
 * desk must fall on the other side of the threshold from the paper (a desk as bright as the paper joins the sheet).
 * scratch_dev: aocr_quad_scratch_bytes(H, W) bytes, 16-byte aligned, overwritten by the call (0 and an error for bad sizes): that of
 * aocr_clean_page, about 12 bytes per pixel.  It and quad_dev must not overlap the page or each other.
 *
 * aocr_rectify_plan (host only, plain C++, no device work): the output size and the warp coefficients of a quad x0 y0 .. x3 y3 = TL, TR,
 * BR, BL (host memory; every coordinate within +-2^20).
 *   checks     the quad must pass the valid test above, else an error;
 *   size       Wo = Wo_in when > 0, else isqrt(max(|TR-TL|^2, |BR-BL|^2)) + 1;  Ho = Ho_in when > 0, else
 *              isqrt(max(|BL-TL|^2, |BR-TR|^2)) + 1;  isqrt is the floor integer square root of an int64.  Wo or Ho > 16384, or
 *              Wo*Ho > 2^26, is an error naming the size: the caller passes a smaller one.  size = [Wo, Ho];
 *   map        Heckbert's square-to-quad map; it maps output to source, so no matrix is inverted.  Integers first, in int64:
 *                dx1 = x1-x2, dx2 = x3-x2, dx3 = x0-x1+x2-x3, the same for y;
 *                den = dx1*dy2 - dy1*dx2,  gn = dx3*dy2 - dy3*dx2,  hn = dx1*dy3 - dy1*dx3;
 *              then doubles, each operation rounded on its own, in this order:
 *                g = gn/den, h = hn/den;
 *                a = (x1-x0) + g*x1,  b = (x3-x0) + h*x3,  c = x0;    d = (y1-y0) + g*y1,  e = (y3-y0) + h*y3,  f = y0;
 *                U = max(Wo-1, 1), V = max(Ho-1, 1);
 *                coef = [a*V, b*U, c*(U*V), d*V, e*U, f*(U*V), g*V, h*U, U*V].
 * Consequence: the axis-aligned rectangle (x0,y0)..(x0+w, y0+h) with Wo = w+1, Ho = h+1 gives g = h = 0 and products that are exact
 * integers below 2^53: aocr_warp_page then maps (x, y) to (x+x0, y+y0) exactly and copies the rectangle bit for bit.
 *
 * aocr_warp_page (device): the projective resample, bilinear with 8 fractional bits.  coef is a HOST pointer, copied into the kernel's
 * arguments (the host has read the quad anyway, to learn the output's shape).  Per output pixel (x, y), in double, each operation
 * rounded on its own, left to right:
 *   nx = (c0*x + c1*y) + c2;   ny = (c3*x + c4*y) + c5;   dn = (c6*x + c7*y) + c8;
 *   the pixel is fill (0..255) when !(dn > 0), or X = nx/dn is not within [-1, W], or Y = ny/dn is not within [-1, H] (negated
 *   comparisons: a NaN falls to fill); otherwise
 *   qx = (int64)floor(X*256.0 + 0.5), ix = qx >> 8, fx = qx & 255 (arithmetic shift), the same for y;
 *   taps p00 = (ix,iy), p10 = (ix+1,iy), p01 = (ix,iy+1), p11 = (ix+1,iy+1); a tap off the page reads fill;
 *   top = p00*(256-fx) + p10*fx;   bot = p01*(256-fx) + p11*fx;   out = (top*(256-fy) + bot*fy + 32768) >> 16.
 * The divisions are correctly rounded.  out_dev follows the rules of aocr_deskew_page: Ho rows of Wo bytes (1 <= Ho, Wo <= 16384,
 * Ho*Wo <= 2^26), out_pitch >= Wo apart, any alignment; bytes between Wo and out_pitch are untouched; it must not overlap the page.  No
 * scratch.
 * The device calls enqueue only, never synchronise or allocate; the results do not depend on launch geometry, atomics order or run (integer
 * maxima; one thread per output byte).  Invalid sizes, a bad threshold or fill, NULLs or overlap return an error before anything is
 * enqueued and leave the outputs untouched. */
size_t aocr_quad_scratch_bytes(int32_t H, int32_t W);
int aocr_find_page_quad(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W,
                        int32_t threshold, int32_t dark_paper, void* scratch_dev, int32_t quad_dev[16]);
int aocr_rectify_plan(const int32_t quad[8], int32_t Wo_in, int32_t Ho_in, int32_t size[2], double coef[9]);
int aocr_warp_page(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W,
                   const double coef[9], int32_t fill, uint8_t* out_dev, int64_t out_pitch, int32_t Ho, int32_t Wo);

/* ---- page scale normalisation: the size of the glyphs, and exact area resampling, between aocr_flatten_page and aocr_clean_page ----------
 * Every stage above counts in pixels (min_line_h, word_gap, gap_x, min_area, radius ...), and every default is a judgement for text at
 * 300 dpi.  A page scanned at 150 or 600 dpi breaks them all at once.  These two calls measure how large the glyphs are and resample the
 * page so that the text has the size the defaults were written for.  Integer arithmetic only, specified exactly.  The page follows the
 * rules of aocr_segment_page: gray uint8, any base address, any pitch >= W, 1 <= H, W <= 16384, H*W <= 2^26.
 *
 * aocr_estimate_glyph_size (device): the quartiles of the glyph size.
 *   components as aocr_label_components defines them, with params.threshold (0..254, or -1 for Otsu: steps 1-2 of aocr_segment_page, bit
 *              for bit), light_text and connectivity (4 or 8); an Otsu threshold of -1 (one gray value): there are none;
 *   size       of a component with the tight box w x h: a = min(w, h), b = max(w, h).  The component qualifies when
 *              min_size <= a <= max_size and b <= max_aspect * a (in int64); a qualifying component adds one to hist[a];
 *   quartiles  with n the number of qualifying components, q_k (k = 1, 2, 3) is the element at index floor(k * (n - 1) / 4) of the
 *              ascending list of their a: the smallest s whose running sum hist[1] + .. + hist[s] exceeds that index;
 *   output     glyph_dev = [q_2 (the size), q_1, q_3, n, components found, the threshold used, the total ink, 0] (4-byte aligned); the three
 *              quartiles are 0 when n == 0.
 * min(w, h) does not change under quarter turns (the call may run before aocr_estimate_orientation) and ignores glyphs merged along the
 * line, whose box grows along one axis only; max_aspect drops rules and the stems of l and 1.
 * Limits: the size is a median of component boxes, not an x-height; all-caps text reads larger; touching or broken glyphs move it; below
 * about 4 pixels it is noise (read n and the quartiles before trusting it).
 * scratch_dev: aocr_glyph_scratch_bytes(H, W) bytes, 16-byte aligned, overwritten by the call (0 and an error for bad sizes): that of
 * aocr_clean_page plus a histogram, about 12 bytes per pixel.  It and glyph_dev must not overlap the page or each other.
 *
 * aocr_resize_page (device): exact pixel-area resampling of the H x W page to Ho x Wo.  Along x, source pixel x covers [x*Wo, (x+1)*Wo)
 * and output pixel X covers [X*W, (X+1)*W) on a common axis of W*Wo units:
 *   wx(x, X) = max(0, min((x+1)*Wo, (X+1)*W) - max(x*Wo, X*W)), which sums to W over x; wy(y, Y) likewise with H and Ho, summing to H;
 *   S        = sum over y, x of wy(y, Y) * wx(x, X) * page[y][x]                  (<= 255*H*W < 2^34: 64 bits);
 *   out[Y][X] = floor((S + floor(H*W / 2)) / (H*W)).
 * Consequences: equal sizes copy the page byte for byte; shrinking by an integer k gives the rounded mean of every k x k block; growing by
 * an integer k repeats every pixel k x k times; a constant page stays constant.
 * The page and the output each follow the size rules of aocr_deskew_page (1 <= Ho, Wo <= 16384, Ho*Wo <= 2^26, out_pitch >= Wo, any
 * alignment; bytes between Wo and out_pitch are untouched), and W <= 8*Wo, Wo <= 8*W, H <= 8*Ho, Ho <= 8*H: at most 9 taps per axis.  The
 * output must not overlap the page.  No scratch.
 * Both calls enqueue only, never synchronise or allocate; the results do not depend on launch geometry, atomics order or run (integer sums;
 * one thread per output byte).  Invalid params or sizes, non-zero reserved words, NULLs or overlap return an error before anything is
 * enqueued and leave the outputs untouched. */
typedef struct aocr_glyph_params {
  int32_t threshold;     /* 0..254: ink = (v <= threshold); -1: Otsu, steps 1-2 of aocr_segment_page, bit for bit */
  int32_t light_text;    /* 1: ink = (v > threshold) instead */
  int32_t connectivity;  /* 4 or 8 */
  int32_t min_size;      /* >= 1: a component whose min(w, h) is smaller does not count */
  int32_t max_size;      /* min_size..1024: nor one whose min(w, h) is larger */
  int32_t max_aspect;    /* >= 1: nor one with max(w, h) > max_aspect * min(w, h) */
  int32_t reserved[2];   /* must be 0 */
} aocr_glyph_params;

size_t aocr_glyph_scratch_bytes(int32_t H, int32_t W);
int aocr_estimate_glyph_size(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W,
                             const aocr_glyph_params* params, void* scratch_dev, int32_t glyph_dev[8]);
int aocr_resize_page(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W,
                     uint8_t* out_dev, int64_t out_pitch, int32_t Ho, int32_t Wo);

/* ---- page dewarp: the curl of the text lines, and the column shifts that remove it, after aocr_deskew_page and in front of aocr_segment_page --
 * On a book page bending into the gutter, or a sheet lifting at one edge, the text lines are curves.  aocr_deskew_page removes the best
 * single slope; what is left smears the whole-width row profiles of aocr_segment_page as skew did.  aocr_estimate_curl finds, for groups of
 * columns, how many rows the text of a group sits below that of the middle group; aocr_dewarp_page shifts every column back.  Both are
 * integer arithmetic, specified exactly.  The page follows the rules of aocr_segment_page: any base address, any pitch >= W,
 * 1 <= H, W <= 16384, H*W <= 2^26.
 *
 * aocr_estimate_curl (device):
 *   ink        the threshold is params.threshold when >= 0, else Otsu's: steps 1-2 of aocr_segment_page, bit for bit;
 *              ink = (v <= threshold), or (v > threshold) with light_text; an Otsu threshold of -1 (one gray value): nothing is ink;
 *   strips     R[b][y], b = x >> 5, nb = ceil(W / 32): exactly as in aocr_estimate_skew;
 *   groups     g = params.group strips each: ng = ceil(nb / g);  G[j][y] = sum of R[b][y] over b in [j*g, min((j+1)*g, nb)), at most 512;
 *              I_j = sum over y of G[j][y];
 *   scores     D = params.max_shift; for every pair j in [0, ng-1) and every d in [-D, D]:  C_j(d) = sum over y of G[j][y] * G[j+1][y+d];
 *              a term whose row y+d is outside [0, H) is 0; the sums are exact unsigned 64-bit integers.  D >= H is legal: those scores are 0;
 *   pair       delta_j = 0 when I_j < min_ink or I_{j+1} < min_ink; otherwise candidates in the order 0, -1, +1, -2, +2, ...: the first
 *              with the strictly largest score.  All scores 0 gives 0;
 *   chain      jc = ng >> 1, s[jc] = 0;  s[j+1] = s[j] + delta_j upward, s[j] = s[j+1] - delta_j downward: what is on row y of group jc
 *              is on row y + s[j] of group j;
 *   outputs    shifts_dev[j] = s[j] for j < ng;  curl_dev = [ng, max over j of |s[j]|, the threshold used, the number of pairs with
 *              delta_j != 0];  scores_dev[j*(2D+1) + d + D] = C_j(d) for every pair, gated ones included, when not NULL.
 * ng == 1 gives s = [0] and no scores; a page without ink, or an Otsu threshold of -1, gives all zeros.
 * Limits: D must stay below half the line pitch, or a pair locks onto the neighbouring line; the errors of the pairs add up along the
 * chain; a group in an empty margin (gated) continues its neighbour's shift flat.
 * scratch_dev: aocr_curl_scratch_bytes(H, W, group, max_shift) bytes, 16-byte aligned, overwritten by the call (0 and an error for bad
 * sizes).  curl_dev, shifts_dev (4-byte aligned) and scores_dev (8-byte aligned) must not overlap the page or the scratch.
 *
 * aocr_dewarp_page (device): every column resampled along y by its shift, linearly interpolated between the group centres.
 *   w = 32*group, h = 16*group, ng = ceil(ceil(W / 32) / group), c_j = j*w + h (also for a narrow last group);  s[j] = shifts_dev[j], read
 *   on the device (shifts_dev = the output of aocr_estimate_curl: no host read in between) and clamped to [-16384, 16384];
 *   shift      in Q8:  q(x) = 256*s[0] for x <= c_0;  q(x) = 256*s[ng-1] for x >= c_{ng-1};  otherwise j = (x - h) / w, t = x - c_j and
 *              q(x) = 256*s[j] + floor(((s[j+1] - s[j]) * t * 256 + h) / w): a floor division of a signed value, the product in 64 bits;
 *   pixel      p = 256*y + q(x), sy = p >> 8 (arithmetic shift), f = p & 255;  a = page[sy][x], b = page[sy+1][x], either one `fill`
 *              (0..255) when its row is outside [0, H);  out[y][x] = (a*(256 - f) + b*f + 128) >> 8.
 * All-zero shifts copy the page bit for bit; no read leaves the page.  Vertical displacement only: the foreshortening of the columns
 * toward a gutter stays.  out_dev follows the rules of aocr_deskew_page: H rows of W bytes, out_pitch >= W apart, any alignment; bytes
 * between W and out_pitch are untouched; it must not overlap the page (or shifts_dev).  No scratch.
 * All three calls enqueue only, never synchronise or allocate; the results do not depend on launch geometry, atomics order or run (integer
 * sums only).  Invalid params, sizes, non-zero reserved words, NULLs or overlap return an error before anything is enqueued and leave the
 * outputs untouched. */
typedef struct aocr_curl_params {
  int32_t threshold;     /* 0..254: ink = (v <= threshold); -1: Otsu, steps 1-2 of aocr_segment_page, bit for bit */
  int32_t light_text;    /* 1: ink = (v > threshold) instead */
  int32_t group;         /* g in 1..16: column groups of 32*g columns */
  int32_t max_shift;     /* D in 0..64: candidate row shifts -D..D between neighbouring groups */
  int32_t min_ink;       /* 0..2^20: a pair with a group holding fewer ink pixels than this gets shift 0 */
  int32_t reserved[3];   /* must be 0 */
} aocr_curl_params;

size_t aocr_curl_scratch_bytes(int32_t H, int32_t W, int32_t group, int32_t max_shift);
int aocr_estimate_curl(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W,
                       const aocr_curl_params* params, void* scratch_dev, int32_t curl_dev[4],
                       int32_t* shifts_dev, uint64_t* scores_dev);
int aocr_dewarp_page(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W, int32_t group,
                     const int32_t* shifts_dev, int32_t fill, uint8_t* out_dev, int64_t out_pitch);

/* ---- colour pages: the paper colour, and the gray page every other stage reads, in front of aocr_find_page_quad and aocr_flatten_page -----------
 * A colour scanner or a phone delivers interleaved RGB.  aocr_gray_page replaces the reduction to gray that a caller otherwise does on the
 * host (3 bytes per pixel read, 1 written, no host sync: the shape does not change), and keeps what that reduction throws away: a pixel's
 * chroma tells a red form rule, a yellow highlighter stroke or a blue stamp from black ink, so such pixels can be turned into paper before
 * any profile or threshold sees them.  aocr_estimate_page_colour replaces a host histogram of the page: it finds the colour of the paper, which
 * aocr_gray_page divides out so that yellowed paper or warm light costs no contrast.  Both are integer arithmetic, specified exactly.
 * The page: H rows of W pixels of 3 bytes, rows pitch >= 3*W bytes apart, any base address and any pitch (pitch % 3 != 0 included); byte
 * 3*x + c of a row is channel c (0 R, 1 G, 2 B) of pixel x.  1 <= H, W <= 16384, H*W <= 2^26, the limits of aocr_warp_page.
 *
 * aocr_estimate_page_colour (device):
 *   hist       hist_c[v] = the number of pixels whose channel c is v;
 *   window     S_c(v) = hist_c[v-2] + ... + hist_c[v+2], bins outside 0..255 counting as 0;
 *   paper      p_c = the v >= paper_min with the largest S_c(v), the larger v on a tie; 255 when no pixel has channel c >= paper_min;
 *   output     colour_dev = [p_R, p_G, p_B, 1, 0 x 12].
 * Only paper_min of params is used; the others must still be valid.  Limit: the mode is taken over the whole picture, so a desk that covers
 * more of a photograph than the sheet wins it: give the paper in params, or rely on aocr_warp_page and aocr_flatten_page afterwards.
 * scratch_dev: aocr_colour_scratch_bytes(H, W) bytes, 16-byte aligned, overwritten by the call (0 and an error containing "bad sizes" for
 * bad sizes).  colour_dev (4-byte aligned) must not overlap the page or the scratch.
 *
 * aocr_gray_page (device), for every pixel (r, g, b):
 *   paper      p = colour_in_dev[0..2] when colour_in_dev is not NULL, read on the device (the output of aocr_estimate_page_colour: no host
 *              read in between) and clamped to 1..255; otherwise params->paper, or (255, 255, 255) when params->balance is 0.  paper[0] < 0
 *              (estimate) with balance 1 and no colour_in_dev is an error;
 *   balance    r' = min(255, (r*255 + p_R/2) / p_R) with integer division, and likewise g', b': p = (255, 255, 255) is the identity;
 *   chroma     mx, mn = the largest and smallest of r', g', b';  c = mx - mn;  the pixel is coloured when c >= chroma_min;
 *   hue class  six classes centred on the primaries and secondaries (AOCR_HUE_*):
 *              mx == r':        2*(g'-b') >= c: YELLOW;  else 2*(b'-g') >  c: MAGENTA;  else RED;
 *              else mx == g':   2*(r'-b') >  c: YELLOW;  else 2*(b'-r') >= c: CYAN;     else GREEN;
 *              else:            2*(g'-r') >  c: CYAN;    else 2*(r'-g') >= c: MAGENTA;  else BLUE;
 *   output     a coloured pixel whose class bit (1 << class) is set in drop becomes fill; otherwise mode 0 gives
 *              (w_R*r' + w_G*g' + w_B*b' + 128) >> 8 and mode 1 gives mn (any coloured ink on white paper comes out dark);
 *   counts     colour_out_dev, when not NULL, is overwritten (not accumulated) with [p_R, p_G, p_B, estimated, n_RED, n_YELLOW, n_GREEN,
 *              n_CYAN, n_BLUE, n_MAGENTA, n_dropped, 0 x 5]: the paper used; estimated = (colour_in_dev[3] != 0), 0 without
 *              colour_in_dev; n_class = the coloured pixels of the class, dropped or not; n_dropped = the pixels replaced by fill.
 *              colour_out_dev may be colour_in_dev itself; otherwise the two must not overlap.
 * Limits: coloured text is dropped together with coloured marks of its class; below chroma_min the hue of a dark pixel is noise, which is
 * why such a pixel is never dropped.  The luma weights (77, 150, 29) stay within 1 gray level of round(255 * rgb2y): DESIGN.md section 21.
 * out_dev follows the rules of aocr_deskew_page: H rows of W bytes, out_pitch >= W apart, any alignment; bytes between W and out_pitch are
 * untouched; it must not overlap the page or the colour words.  No scratch.
 * All three calls enqueue only, never synchronise or allocate; the results do not depend on launch geometry, atomics order or run (integer
 * sums only).  NULL pointers, pitch < 3*W, out_pitch < W, weights that are negative or do not sum to 256, mode or balance outside {0, 1},
 * drop outside 0..63, chroma_min or paper_min outside 1..255, a given paper outside 1..255, fill outside 0..255 or an overlap return an
 * error that names the argument before anything is enqueued and leave the outputs untouched. */
#define AOCR_HUE_RED 0
#define AOCR_HUE_YELLOW 1
#define AOCR_HUE_GREEN 2
#define AOCR_HUE_CYAN 3
#define AOCR_HUE_BLUE 4
#define AOCR_HUE_MAGENTA 5

typedef struct aocr_colour_params {
  int32_t weights[3];    /* w_R, w_G, w_B: each >= 0, 256 in sum; (77, 150, 29) is luma, (256, 0, 0) reads the red channel */
  int32_t mode;          /* 0: the weighted sum; 1: the smallest balanced channel */
  int32_t balance;       /* 1: divide the paper colour out; 0: the paper is (255, 255, 255) */
  int32_t paper[3];      /* the paper colour, 1..255 each; paper[0] < 0: estimated (aocr_estimate_page_colour into colour_in_dev) */
  int32_t paper_min;     /* 1..255: the darkest value the estimate takes for paper */
  int32_t chroma_min;    /* 1..255: a pixel is coloured when max - min of its balanced channels reaches this */
  int32_t drop;          /* 0..63: bit (1 << AOCR_HUE_*) set: coloured pixels of that class become fill */
  int32_t fill;          /* 0..255 */
} aocr_colour_params;

size_t aocr_colour_scratch_bytes(int32_t H, int32_t W);
int aocr_estimate_page_colour(void* stream, const uint8_t* rgb_dev, int64_t pitch, int32_t H, int32_t W,
                              const aocr_colour_params* params, void* scratch_dev, int32_t colour_dev[16]);
int aocr_gray_page(void* stream, const uint8_t* rgb_dev, int64_t pitch, int32_t H, int32_t W,
                   const aocr_colour_params* params, const int32_t* colour_in_dev, int32_t* colour_out_dev,
                   uint8_t* out_dev, int64_t out_pitch);

/* ---- word slant: the lean of the writing inside every box, and crops with the lean taken out, between aocr_segment_page and the recogniser ----
 * Italic print and handwriting lean by 10 to 40 degrees: a horizontal shear of every word, which neither aocr_deskew_page (rows against
 * columns, up to slope 0.25) nor aocr_dewarp_page touches.  aocr_estimate_slant finds one slant per box by a sweep of sheared column
 * profiles; aocr_crop_lines_slanted is aocr_crop_lines with every row of a box moved back along x.  Integer arithmetic, specified exactly;
 * every >> is an arithmetic (floor) shift of a signed value.  The page follows the rules of aocr_segment_page: any base address,
 * pitch >= W, 1 <= H, W <= 16384, H*W <= 2^26.
 *
 * aocr_estimate_slant (device), for every box i < n, n = min(n_boxes, count_dev[0]) read on the device (count_dev == NULL: n = n_boxes):
 *   box        x0, y0, x1, y1 clamped to the page before any read;  h = y1 - y0, w = x1 - x0, cy = (y0 + y1) >> 1;
 *   ink        thr = params.threshold when >= 0, else threshold_dev[0], read on the device (the word aocr_segment_page wrote to counts_dev[2]:
 *              no host read in between);  I[y][x] = (v <= thr), or (v > thr) with light_text, for the pixels inside the clamped box and 0
 *              everywhere else: the ink of neighbouring words does not count.  thr == -1 (Otsu found one gray value): nothing is ink;
 *   candidates k = -K..K (K = n_steps), s_k = k * step_q16 columns per row in Q16;  off_k(y) = ((cy - y) * s_k + 32768) >> 16;
 *              D_k = max over y in [y0, y1) of |off_k(y)|.  Positive s: the strokes lean to the right, the top of a stroke is to the right
 *              of its foot;
 *   profile    P_k[c] = sum over y in [y0, y1) of I[y][c + off_k(y)] for c in [x0 - D_k, x1 + D_k): every ink pixel lands in exactly one c;
 *   score      score_k = sum over c of P_k[c]^2, an exact unsigned 64-bit integer;
 *   winner     candidates in the order 0, -1, +1, -2, +2, ...: the first with the strictly largest score.  K = 0 gives k = 0;
 *   outputs    slant_dev[4*i ..] = [k, k * step_q16, flag, the ink pixels of the box];  scores_dev[i*(2K+1) + k + K] = score_k when not NULL;
 *              flag 0: estimated;  flag 1: h > AOCR_SLANT_MAX_H, not estimated: k = 0, the ink word is still filled, the scores are 0;
 *              flag 2: the box is empty after clamping: [0, 0, 2, 0], the scores are 0.
 * Rows >= n of slant_dev and scores_dev are untouched.  n_boxes <= 65535; n_boxes == 0 is a no-op.
 * Limits: the sum of squares rewards any vertical alignment, not only strokes; a box of one round glyph has no slant to find; boxes taller
 * than AOCR_SLANT_MAX_H rows are skipped; the slant is one per box, not per character.
 * scratch_dev: aocr_slant_scratch_bytes(n_boxes, n_steps) bytes, 16-byte aligned, overwritten by the call (0 and an error containing "bad
 * sizes" for n_boxes outside 0..65535 or n_steps outside 0..64).  slant_dev (4-byte aligned) and scores_dev (8-byte aligned) must not
 * overlap the page or the scratch.
 *
 * aocr_crop_lines_slanted (device): row i < n of out_dev (n_boxes, 1, out_h, out_w) fp32, n as for aocr_crop_lines:
 *   slant      s = slant_dev[4*i + 1], read on the device (slant_dev = the output of aocr_estimate_slant: no host read in between) and clamped
 *              to [-65536, 65536];  slant_dev == NULL: s = 0;
 *   extent     off(y) = ((cy - y) * s + 32768) >> 16 with the clamped box's cy;  D = max(|off(y0)|, |off(y1 - 1)|);
 *   V          h rows, w + 2D columns:  V[r][c] = page[y0 + r][sx] with sx = x0 - D + c + off(y0 + r) when x0 <= sx < x1, else fill (0..255):
 *              the widening by D on each side loses no ink of the box, and reading inside the box only lets no neighbour's ink in;
 *   output     V scaled to out_h x out_w with the arithmetic of aocr_preprocess_lines, operation for operation: bit-identical to
 *              aocr_preprocess_lines on a contiguous copy of V.
 * With slant_dev == NULL, or every s == 0, the output equals that of aocr_crop_lines bit for bit.  A box that is empty after clamping gives
 * 255.0; rows >= n are untouched; n_boxes <= 65535; n_boxes == 0 is a no-op.  No scratch.
 * Both calls enqueue only, never synchronise or allocate; the results do not depend on launch geometry, atomics order or run (integer sums
 * only).  Invalid params, sizes, non-zero reserved words, NULL pointers, a -1 threshold with threshold_dev == NULL, fill outside 0..255 or
 * an overlap return an error that names the argument before anything is enqueued and leave the outputs untouched. */
#define AOCR_SLANT_MAX_H 256

typedef struct aocr_slant_params {
  int32_t threshold;     /* 0..254 fixed; -1: read threshold_dev[0] on the device (the word aocr_segment_page wrote to counts_dev[2]) */
  int32_t light_text;    /* 1: ink = (v > threshold) instead */
  int32_t step_q16;      /* 1..8192: difference between neighbouring candidates, columns per row, Q16 */
  int32_t n_steps;       /* K in 0..64, K * step_q16 <= 65536 (45 degrees) */
  int32_t reserved[4];   /* must be 0 */
} aocr_slant_params;

size_t aocr_slant_scratch_bytes(int32_t n_boxes, int32_t n_steps);
int aocr_estimate_slant(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W,
                        const aocr_box* boxes_dev, const int32_t* count_dev, int32_t n_boxes,
                        const aocr_slant_params* params, const int32_t* threshold_dev, void* scratch_dev,
                        int32_t* slant_dev, uint64_t* scores_dev);
int aocr_crop_lines_slanted(void* stream, const uint8_t* page_dev, int64_t pitch, int32_t H, int32_t W,
                            const aocr_box* boxes_dev, const int32_t* count_dev, int32_t n_boxes,
                            const int32_t* slant_dev, int32_t fill, int32_t out_h, int32_t out_w, float* out_dev);

#ifdef __cplusplus
}
#endif
#endif /* AOCR_H */
