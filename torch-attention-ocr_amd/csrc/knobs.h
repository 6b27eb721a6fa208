// knobs.h -- every AOCR_* environment switch that libaocr.so reads, declared once: name, read kind, default, effect.
// Host only, plain C++17 (a host compiler builds it alone: tests/knobs_main.cc).  DESIGN.md's "Dispatch switches" table lists
// these in the same order.  Each line makes one inline accessor knob::AOCR_<NAME>() that is a getenv of the name plus the compare
// of its kind -- the environment is read on EVERY call (tests and A/B runs toggle switches inside one process), nothing is cached.
//   SET   bool         the variable is present, whatever its value ("0" and "" included)
//   ON    bool         its first character is '1'
//   NOT0  bool         on unless its first character is '0' (a default-on switch)
//   INT   int          atoi of the value, the default when unset
//   RAW   const char*  the value itself (nullptr when unset) for the few call sites that parse it themselves
#pragma once
#include <cstdlib>

namespace aocr { namespace knob {
#define AOCR_KNOB_SET(FN, NAME, DEF)  inline bool FN() { return std::getenv(NAME) != nullptr; }
#define AOCR_KNOB_ON(FN, NAME, DEF)   inline bool FN() { const char* e = std::getenv(NAME); return e && e[0] == '1'; }
#define AOCR_KNOB_NOT0(FN, NAME, DEF) inline bool FN() { const char* e = std::getenv(NAME); return !(e && e[0] == '0'); }
#define AOCR_KNOB_INT(FN, NAME, DEF)  inline int FN() { const char* e = std::getenv(NAME); return e ? std::atoi(e) : (DEF); }
#define AOCR_KNOB_RAW(FN, NAME, DEF)  inline const char* FN() { return std::getenv(NAME); }
#define KNOB(NAME, KIND, DEF, EFFECT) AOCR_KNOB_##KIND(NAME, #NAME, DEF)
// KNOB_CLAMP: an INT whose value, when set, is clamped to [LO, HI] by the read.  KNOB_ALSO: a second accessor FN for a name that two call sites read with different kinds
#define KNOB_CLAMP(NAME, KIND, DEF, LO, HI, EFFECT) inline int NAME() { const char* e = std::getenv(#NAME); if (!e) return (DEF); const int n = std::atoi(e); return n < (LO) ? (LO) : n > (HI) ? (HI) : n; }
#define KNOB_ALSO(FN, NAME, KIND, DEF, EFFECT) AOCR_KNOB_##KIND(FN, #NAME, DEF)

// ---- diagnostics
KNOB(AOCR_TRACE,                 SET,  0,    "one stderr line per launch decision of the traced launchers")
KNOB(AOCR_PROBE,                 SET,  0,    "aocr_profile_kernel prints the in-kernel clock probe of the tagged conv launch")
KNOB(AOCR_PROBE_LAYER,           RAW,  0,    "3|4|5: aocr_profile_kernel id 0 replays that conv layer's tagged forward launch instead of conv6's")
KNOB(AOCR_DBG_STOP,              INT,  0,    "1|2: stop the CNN backward pass at that stage and leave its gradient map in place (tap g0)")
KNOB_ALSO(AOCR_DBG_STOP_SET, AOCR_DBG_STOP, SET, 0, "cnn_wgrad_on_side: any value keeps the CNN filter gradients off the side stream")
KNOB(AOCR_DC_STAMPS,             RAW,  0,    "cycle stamps of the decoder cluster / chain kernels (stamps build); a value starting with b: beam launches only")
KNOB(AOCR_SEQ_STAMP,             SET,  0,    "cycle stamps of the whole-sequence encoder forward kernel")
KNOB(AOCR_SEQ_ABL,               INT,  0,    "timing-only ablation bits of the whole-sequence encoder forward kernel")
KNOB(AOCR_CL_REMOTE,             SET,  0,    "cluster kernels exchange through write-through stores as if their members were not on one XCD")
// ---- bf16 convolutions and hoisted GEMMs (ops_gemm.hip)
KNOB(AOCR_NO_DMA,                ON,   0,    "no LDS-DMA kernels at all (the 128 x 128 LDS kernels)")
KNOB(AOCR_FORCE_DMA,             ON,   0,    "LDS-DMA kernels wherever their shape constraints hold, however the grid fills the chip")
KNOB(AOCR_NO_HALO,               ON,   0,    "no halo-resident 3 x 3 kernel (the im2col LDS-DMA kernel)")
KNOB(AOCR_HALO8,                 SET,  0,    "the 8-wave gemm_halo_bf16_kernel instead of the 4-wave gemm_halo4_bf16_kernel")
KNOB(AOCR_HALO4_STAGED,          INT,  7,    "bits: output tiles of the 256 x 256 kernels through LDS -- 1 fp32 data gradient, 2 fp32 conv forward, 4 pooled")
KNOB(AOCR_NO_HALO4_SKIP,         ON,   0,    "gemm_halo4_bf16_kernel with contiguous blocks per wave-row and no skipped padding-row MFMAs (its first form)")
KNOB(AOCR_NO_HALO4_POOL_SKIP,    ON,   0,    "the first form for the (2,1)-pooled launches of gemm_halo4_bf16_kernel only (conv4 / conv6 forward)")
KNOB(AOCR_NO_NARROW_WIDE,        SET,  0,    "conv7 forward on 128 x 128 tiles instead of 256 x 128 tiles of the narrow LDS-DMA kernel")
KNOB(AOCR_NO_NARROW_STAGED,      ON,   0,    "quad epilogue of the narrow LDS-DMA kernel instead of the staged tile")
KNOB(AOCR_NO_DMA128,             ON,   0,    "128 x 128 tiles on the register-staged kernel instead of gemm_dma128_kernel")
KNOB(AOCR_DMA128_W4,             ON,   0,    "gemm_dma128_kernel's 4-wave form at every grid size")
KNOB(AOCR_NO_HH_NARROW,          SET,  0,    "hoisted bf16 GEMMs on the 128 x 128 kernels instead of the narrow LDS-DMA kernel")
KNOB(AOCR_HH_NARROW_FULL_ONLY,   ON,   0,    "hoisted GEMMs take the narrow LDS-DMA kernel only when M is whole 256-row tiles")
KNOB(AOCR_NO_HH_CAT,             ON,   0,    "the encoder's d X as two products instead of one over the concatenated K range")
KNOB(AOCR_NO_SKINNY,             SET,  0,    "128 x 128 tiles for skinny products (N <= 64) instead of the step kernel; also turns project_loss_kernel off")
KNOB(AOCR_NO_PROJ_FUSE,          ON,   0,    "projector, criterion and projector data gradient as three launches instead of project_loss_kernel")
KNOB(AOCR_NO_BN_STATS_FUSE,      SET,  0,    "BatchNorm statistics of conv3 / conv5 by a pass over y instead of from the conv epilogue")
KNOB(AOCR_BN_Y16,                SET,  0,    "pre-BatchNorm maps stored as bf16 (outside the parity tolerance)")
KNOB(AOCR_DX16,                  ON,   0,    "bf16 data-gradient maps for the BatchNorm backward / un-pool passes (outside the parity tolerance)")
KNOB(AOCR_BNB_FUSE,              ON,   0,    "BatchNorm backward's sums pass from the data gradient's staged fp32 tile (measured slower)")
// ---- filter and weight gradients (ops_gemm.hip)
KNOB(AOCR_WGRAD_ATOMIC,          SET,  0,    "split-K filter gradients through fp32 atomics instead of slabs + splitk_reduce_kernel")
KNOB(AOCR_NO_WGRAD_HALO,         ON,   0,    "filter gradients on the one-tap-per-tile kernels instead of conv_wgrad_halo_kernel")
KNOB(AOCR_WGRAD_HALO_MINN,       INT,  576,  "smallest N = 9 Cin that takes conv_wgrad_halo_kernel (conv2 upwards)")
KNOB(AOCR_WGRAD_HALO_MINSTEPS,   INT,  0,    "> 0: at small P fewer, longer k ranges of at least n steps instead of a full round of the chip")
KNOB(AOCR_WGRAD_HALO_RAGGED,     NOT0, 1,    "0: conv_wgrad_halo_kernel only for rows of whole 32-pixel segments")
KNOB(AOCR_NO_WGRAD_ISSUE_MID,    ON,   0,    "conv_wgrad_halo_kernel issues the next DMA pieces before its first MFMA instead of between the k-halves")
KNOB(AOCR_NO_WGRAD_DMA_GROUPED,  ON,   0,    "recurrent weight gradients on wgrad_tr_grouped_kernel instead of wgrad_dma_grouped_kernel")
KNOB(AOCR_WGRAD_DMA_WGS,         INT,  256,  "workgroups wgrad_dma_grouped_kernel aims at per launch (one round)")
KNOB(AOCR_WGRAD_DMA_MINK,        INT,  2048, "smallest K (rows L B / T B) that takes wgrad_dma_grouped_kernel")
// ---- exact-fp32 GEMMs (ops_gemm.hip)
KNOB(AOCR_NO_LDS_F32,            SET,  0,    "fragment-from-global fp32 GEMM instead of the LDS-tiled kernels")
KNOB(AOCR_NO_F32T,               ON,   0,    "gemm_lds_f32_kernel instead of gemm_f32t_kernel")
KNOB(AOCR_F32T_TILE,             INT,  0,    "1|2|3: force gemm_f32t_kernel's tile (128 x 128 / 64 x 128 / 64 x 64)")
KNOB(AOCR_NO_F32W,               ON,   0,    "fragment-from-global kernel instead of gemm_f32w_kernel")
KNOB_CLAMP(AOCR_F32W_MINK,       INT,  192,  32, 0x7fffffff, "least K per k range of gemm_f32w_kernel's split (at least 32)")
KNOB(AOCR_NO_STEP_F32,           ON,   0,    "gemm_small_kernel<false> instead of gemm_step_f32_kernel")
KNOB(AOCR_STEP_F32_W16,          ON,   0,    "gemm_step_f32_kernel's 16-wave form for deep K on small grids (measured slower)")
// ---- recurrent-step products (ops_gemm.hip)
KNOB(AOCR_NO_QUARTER_TILES,      SET,  0,    "full gate tiles instead of 8-unit tiles at small batch (fp32 mode)")
KNOB(AOCR_NO_HALF_TILES,         ON,   0,    "32-unit gate tiles instead of half gate tiles on small grids")
KNOB(AOCR_HALF_TILES_MAXGRID,    INT,  200,  "the 32-unit grid size below which gate products take half tiles")
KNOB(AOCR_STEP_WAVES4,           SET,  0,    "4-wave gemm_step_kernel instead of 8 waves")
KNOB(AOCR_STEP_WAVES16,          SET,  0,    "16 waves for plain step products at K >= 1024 (measured slower)")
KNOB(AOCR_NO_STEP_MT2,           ON,   0,    "one 32-row tile per workgroup instead of two where the grid allows")
KNOB(AOCR_STEP_MT2_MINK,         INT,  2048, "the K from which one plain product takes two row tiles per workgroup")
KNOB(AOCR_NO_STEPL,              ON,   0,    "step products on gemm_step_kernel instead of stepl.h")
KNOB(AOCR_STEPL_MIN_WGS,         INT,  -1,   ">= 0: stepl.h from n of its own workgroups whatever the kind of launch")
KNOB(AOCR_BIG_STEP,              ON,   0,    "step products as 128 x 128 LDS-DMA tiles + an elementwise cell pass (measured slower)")
KNOB(AOCR_BIG_STEP_MIN_ROWS,     INT,  320,  "rows from which AOCR_BIG_STEP applies")
// ---- elementwise CNN kernels and attention (ops_misc.hip)
KNOB(AOCR_CONV1_SCALAR,          SET,  0,    "conv1's filter gradient on the scalar kernel instead of the packed one")
KNOB(AOCR_UNPOOL4,               SET,  0,    "un-pool on the 4-channel kernels instead of unpool8_kernel")
KNOB(AOCR_BN_PARTIAL_OLD,        SET,  0,    "4-byte-access BatchNorm partial sums instead of bn_partial4_kernel")
KNOB(AOCR_ATTN_BWD_TWO_PASS,     SET,  0,    "the streamed attention backward kernel in two passes over the context instead of one")
KNOB(AOCR_NO_ATTN_BF16,          SET,  0,    "fp32-context attention instead of the bf16-context kernels")
KNOB(AOCR_NO_ATTN_BEAM_GROUP,    SET,  0,    "beam decode at T > 64 with one attention workgroup per hypothesis instead of per image")
KNOB(AOCR_ATTN_NW16,             SET,  0,    "16-wave attention at T <= 32, Hd = 1024")
KNOB(AOCR_NO_CHAIN_CTXA,         SET,  0,    "the Hd = 1024 chain with a q = W_a h launch per step instead of scores against ctx W_a")
// ---- step orchestration (model.hip)
KNOB(AOCR_NO_BN_FOLD,            SET,  0,    "unfused evaluation-mode BatchNorm")
KNOB(AOCR_NO_SIDE_WGRAD,         SET,  0,    "no side stream: weight gradients on the main stream")
KNOB(AOCR_SIDE_PLAIN,            SET,  0,    "side stream at normal priority")
KNOB(AOCR_NO_SIDE_PROLOGUE,      ON,   0,    "gradient zeroing / weight shadows / token table on the main stream in front of conv1")
KNOB(AOCR_NO_SHADOW_SPLIT,       ON,   0,    "conv2 waits for the whole shadow table instead of its own taps")
KNOB(AOCR_NO_CNN_WGRAD_SIDE,     ON,   0,    "the CNN's filter gradients on the main stream")
KNOB(AOCR_CNN_WGRAD_AFTER_DGRAD, ON,   0,    "filter gradient of a stage started behind its data gradient (slower)")
KNOB(AOCR_NO_COLSUM_DEFER,       SET,  0,    "one column-sum launch per bias instead of two deferred ones")
KNOB(AOCR_CONV1_RECOMPUTE,       SET,  0,    "conv1's filter gradient re-evaluates the layer instead of reading the forward pass's routes")
KNOB(AOCR_NO_SEQ,                ON,   0,    "encoder: no whole-sequence kernels at all (per-step launches)")
KNOB(AOCR_NO_CLUSTER,            ON,   0,    "encoder: no cluster kernels (one-workgroup-per-16-rows whole-sequence kernels)")
KNOB(AOCR_NO_LAYER_PIPE,         SET,  0,    "stacked encoder layer after layer instead of the chunk wavefront")
KNOB(AOCR_LAYER_PIPE_CHUNKS,     RAW,  0,    "n: force the wavefront's chunk count")
KNOB(AOCR_ENC_DC_COPY,           ON,   0,    "split copy of the decoder's initial-state gradient in front of the encoder BPTT")
KNOB(AOCR_NO_ENC_WGRAD_SIDE,     ON,   0,    "the encoder's weight gradients on the main stream")
KNOB(AOCR_SIDE_GO_LATE,          ON,   0,    "side streams released behind d(context) instead of behind the decoder BPTT")
KNOB(AOCR_NO_SIDE2,              ON,   0,    "no second side stream")
KNOB(AOCR_JOIN_BEFORE_CNN_BWD,   ON,   0,    "the main stream joins the side stream in front of the CNN backward pass")
KNOB(AOCR_NO_Q_SIDE,             ON,   0,    "q of all steps on the main stream")
KNOB(AOCR_NO_EMB_TABLE,          ON,   0,    "first decoder layer's embedding part as a gathered tensor + product instead of the per-token table")
KNOB(AOCR_NO_EMB_TABLE_CHAIN,    ON,   0,    "the launch chain's first decoder layer without the per-token table")
KNOB(AOCR_NO_DEC_CLUSTER,        ON,   0,    "decoder: launch chain instead of the cluster kernels")
KNOB(AOCR_NO_DEC_CLUSTER_BWD,    ON,   0,    "decoder BPTT: launch chain instead of the cluster kernel")
KNOB(AOCR_NO_DEC_CLUSTER_DROP,   SET,  0,    "decoder under dropout: launch chain instead of the cluster kernels")
KNOB(AOCR_NO_DEC_GREEDY,         SET,  0,    "greedy decode on the launch chain instead of the cluster kernel")
KNOB(AOCR_NO_DECODE_SHADOWS,     ON,   0,    "the decode launch chain without bf16 shadows of its beam state")
// ---- whole-sequence decoder and encoder kernels (dec_cluster.hip, dec_chain.hip, rnn_cluster.hip)
KNOB(AOCR_NO_DEC_CHAINS,         ON,   0,    "dec_cluster.hip's one-chain kernels instead of dec_chain.hip")
KNOB(AOCR_NO_DEC_CHAINS_BWD,     SET,  0,    "the same for the decoder BPTT only")
KNOB(AOCR_NO_DEC_CHAINS_GREEDY,  SET,  0,    "the same for greedy decode only")
KNOB(AOCR_NO_DEC_CHAINS_BEAM,    SET,  0,    "beam search on the per-step launch chain")
KNOB(AOCR_CH_NO_RES,             SET,  0,    "the ctx W_a tile re-read per step instead of resident (T <= 64)")
KNOB(AOCR_NO_DEC_EARLY,          SET,  0,    "no early exit of the greedy kernel")
KNOB(AOCR_ENC_RT2,               ON,   0,    "two row tiles per encoder group although one fits the chip")
KNOB(AOCR_ENC_RH16,              ON,   0,    "encoder forward on 16-row groups")
KNOB(AOCR_ENC_BWD_RH,            RAW,  0,    "8|16: force 8- / 16-row groups in the encoder BPTT")
// ---- data parallelism (comm.hip, model.h)
KNOB(AOCR_ONE_COMM,              SET,  0,    "SyncBN on the gradient communicator (no ncclCommSplit)")
KNOB(AOCR_COMM_EARLY_BUCKET0,    ON,   0,    "release gradient bucket 0 before the encoder BPTT")
KNOB_CLAMP(AOCR_COMM_RESERVE_CUS, INT, 32,   0, 128, "compute units the encoder cluster launches then leave to the collective (0..128)")

#undef KNOB_ALSO
#undef KNOB_CLAMP
#undef KNOB
#undef AOCR_KNOB_RAW
#undef AOCR_KNOB_INT
#undef AOCR_KNOB_NOT0
#undef AOCR_KNOB_ON
#undef AOCR_KNOB_SET

}}  // namespace aocr::knob
