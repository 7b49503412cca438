// Declarations shared by the TopDown captioner's sequencer files: workspace layout and derived weight copies
// (topdown_layout.hip), feature prologue, attention step and the per-device side streams (topdown_features.hip), the pieces of a
// training step (struct Step, topdown_step.hip) that topdown_train.hip sequences, and the decode step (topdown_decode.hip).
#pragma once
#include "uic_common.h"
#include "uic_host.h"
#include "decode_internal.h"
#include "../../include/uic_hip.h"
#include <string.h>
#include <stdlib.h>

namespace topdown {

constexpr int WG_CHUNK = 4;     // decode steps per hand-off between the two streams of the fused training step
constexpr int BPTT_SPLIT = 4;   // K slices of the BPTT loop's d x GEMMs (Step::bptt_split)

struct Layout {
  // forward activations
  void* fcT; void* attT; int* row_len;
  float* ypre; float* amask_rep; int* row_len_rep;   // seq_per_img > 1: per-image relu(att_embed) (f32), att_masks / region counts per caption row
  void* fcp; void* attp; void* patt;
  void* eatt;                                  // bf16: e^{2 p_att}, what the persistent training recurrence's attention reads (rnn_persist.hip)
  void* ybn; float* bn_stat0; float* bn_stat4; float* bn_part; float* bn_red;   // use_bn: pre-BN4 activations, {mean, rstd}, scratch
  void* xt_all; float* gx; float* gfc;
  int64_t* tok_used;   // [N, T] inputs actually fed to the embedding (differs from labels under scheduled sampling)
  void* h_att; void* h_lang; float* c_att; float* c_lang;   // [(T+1), N, H]
  void* gates1; void* gates2;
  float* atth_all; float* alpha_all; void* ctx_all; void* hdrop_all;
  float* logits; void* dlogits; float* row_loss; float* scalars;
  int* cap_len;                                 // ... [N]: 1 + the last decode step at which the row has a live position (the BPTT steps behind it are zeros)
  int* live_inv;                                // ... and its inverse [T N]: position -> list index or -1 (the recurrence stores hdrop rows by it)
  int* live_map;                                // the live list made on the device (uic_topdown_batch.live_rows == NULL): [T N + 128]
  // the rows by caption length, longest first (uic_live_list_launch's UicLiveOrder): [N], its inverse [N], and per decode step the
  // number of rows whose caption has not ended [T + 1]; dG2 / dG1 of ONE decode step with the unfinished rows in that order
  // [N, 4H] -- the compact A operands of the BPTT loop's two d x GEMMs (Step::bwd_step)
  int* row_order; int* row_rank; int* unfinished; void* dg2c; void* dg1c;
  void* hc; float* dhc;                         // live-position logit layer (uic_topdown_batch.live_rows): the live rows of hdrop, operand dtype
                                                // [T N + 128, H]; their d hdrop, f32 [T N, H]
  void* lh[UIC_MAX_LOGIT_LAYERS - 1];       // logit_layers > 1: dropout(relu(hidden logit block l)) [T*N, H]
  void* dlh_pre[UIC_MAX_LOGIT_LAYERS - 1];  // its pre-activation gradient [T*N, H] (operand dtype), kept for the weight gradient
  float* dlh;                               // gradient flowing between the logit blocks [T*N, H] f32
  void* s_lh[UIC_MAX_LOGIT_LAYERS - 1];     // the same activations of one decode step [N, H]
  // backward
  float* dhdrop; float* dx2_all; float* dx1; float* dc_att; float* dc_lang;
  void* dg1_all; void* dg2_all; float* de_all; void* datth_all;
  void* dgfc; float* dfcp; void* dfcpre; float* dxt;
  float* d_att; void* d_patt; float* dwalpha_part; void* d_pre;
  void* tA; void* tB; float* colscratch; size_t colscratch_floats; float* small;
  float* slab; size_t slab_bytes;
  void* tLA; void* tLB; float* colscratchL;   // scratch of the logit-layer weight gradients (side stream)
  void* tSA; void* tSB; float* slab2;         // scratch of the per-chunk recurrent weight gradients (side stream)
  void* tTA; void* tTB; float* slab3;         // the same for the third stream (att_lstm / h2att share of a chunk)
  void* tUA; void* tUB; float* slab4;         // ... and the third stream's second set (default order: a chunk's att_lstm / h2att share)
  int* embed_scratch;                         // uic_embed_bwd_sorted_launch
  void* fcwT; void* attwT;                     // fc_embed / att_embed weights transposed ([Dfc, H], [D, H]): only for the optional input-feature gradients
  void* ones_blk; size_t ones_rows;           // [max(WG_CHUNK * N, N * R), 128] operand dtype, all ones: the "input" whose weight gradient is the bias gradient
  unsigned* rnn_sync; unsigned long long* rnn_dbg;   // persistent recurrence (rnn_persist.hip): sync block, optional time stamps
  float* bp_slab2[2]; float* bp_slab1;       // split-K partial slabs of the BPTT loop's d x2 (two generations) and d x1 GEMMs: [BPTT_SPLIT][N, 3H] / [N, 2H]
  unsigned* rnn_bwd_sync; size_t rnn_bwd_sync_bytes; unsigned long long* rnn_bwd_dbg;   // persistent BPTT (rnn_bwd_persist.hip): one sync block per launch of a step
  // sampling
  void* s_h_att[2]; void* s_h_lang[2]; float* s_c_att[2]; float* s_c_lang[2];
  void* s_xt; float* s_atth; float* s_alpha; void* s_ctx; void* s_hdrop; float* s_logits;
  SampleScratch smp;                         // input token, unfinished flags and counters [N], [N], step capacity T
  float* dec_part; int* dec_tok; void* dec_embed_relu;   // persistent decode (rnn_persist.hip): per-workgroup logit partials, exchanged tokens, relu(embed) in bf16
  BeamScratch beam;                          // beam search bookkeeping: N rows, a done_count entry per row, step capacity T
  size_t total;
};
Layout make_layout(const uic_topdown_dims& d, void* ws);

// operand-dtype and transposed weight copies
struct Derived {
  const void* embed_w;   // [V1, E] the embedding table in the operand dtype (the f32 master itself in f32 runs)
  const void* fc_w; const void* att_w; const void* ctx2att_w; const void* logit_w;
  const void* att_w_ih; const void* att_w_hh; const void* lang_w_ih; const void* lang_w_hh; const void* h2att_w;
  void* logit_wT;    // [H, V1p]
  void* w2T;         // [3H, 4H] = [lang_w_ih^T ; lang_w_hh^T]
  void* w1recT;      // [2H, 4H] = [att_w_ih[:, 0:H]^T ; att_w_hh^T]
  void* wxT;         // [E, 4H]  = att_w_ih[:, 2H:]^T
  void* wfcpT;       // [H, 4H]  = att_w_ih[:, H:2H]^T
  void* h2attT;      // [H, A]
  void* ctx2attT;    // [H, A]
  float* att_beff;   // use_bn: b' = att_b + att_w bn0_beta  [H]  (att_w then points at W' = att_w diag(bn0_gamma))
  const void* logit_h_w[UIC_MAX_LOGIT_LAYERS - 1];   // hidden logit blocks [H, H]
  void* logit_h_wT[UIC_MAX_LOGIT_LAYERS - 1];        // their transposes for the dX GEMMs
  size_t total;
};
Derived make_derived(const uic_topdown_dims& d, const uic_topdown_weights* w, void* base);
int check_dims(const uic_topdown_dims* d);

// _prepare_feature (P/models/AttModel.py:107-117) + operand casts.  part: 0 = everything; 1 = only the fc_embed branch
// (fc' = dropout(relu(fc_embed(fc)))), 2 = only the att_embed / ctx2att branch -- the two are independent, the fused
// training step runs them on its two streams.
int prepare_features(const uic_topdown_dims& d, const uic_topdown_weights* w, const Derived& dv, const uic_topdown_batch* b,
                     const Layout& L, int training, float drop_p, unsigned seed, const void** fc_in_out, const void** att_in_out,
                     hipStream_t s, int part = 0);
int attention_step(const uic_topdown_dims& d, const uic_topdown_weights* w, const Derived& dv, const uic_topdown_batch* b,
                   const Layout& L, const void* h_att, float* att_h, float* alpha, void* ctx, hipStream_t s);

// Side stream + events for the fused training step: the logit layer of finished decode steps (logit GEMM,
// log-softmax/criterion, dH GEMM, later dW_logit) runs beside the latency-bound recurrence on a second HIP stream.
constexpr int MAX_CHUNKS = 64;
struct SideStream {
  hipStream_t stream = nullptr;
  hipStream_t stream3 = nullptr;    // a chunk's att_lstm / h2att weight gradients beside its lang_lstm ones (independent GEMMs)
  hipEvent_t ev_s3 = nullptr;       // stream3 -> side: that share of every chunk so far is done
  hipEvent_t ev_prep = nullptr;     // side -> stream3: the embedding gradient's token bucketing is done
  hipEvent_t ev_den = nullptr, ev_done = nullptr;
  hipEvent_t ev_pro3 = nullptr;     // third stream: its branch of the forward prologue (fc_embed, Gfc, initial state) is through
  hipEvent_t ev_pro = nullptr;      // side: its branch of the forward prologue (fc_embed, embedding, batched input GEMM) is through
  hipEvent_t ev_logit = nullptr;    // side: the logit layer's gradients and the loss are final (start of the BPTT loop)
  hipEvent_t ev_lstm = nullptr;     // side: lang_lstm.weight_{ih,hh} and att_lstm.weight_hh are final (right after the BPTT loop)
  hipEvent_t ev_early = nullptr;    // main: every gradient except the late group (see uic_topdown_grad_ready_wait) is final
  bool early_recorded = false;
  hipEvent_t ev_embed = nullptr;    // the embedding table's gradient and the fc' columns of att_lstm.weight_ih are final (gradient group 3)
  bool embed_recorded = false;
  hipEvent_t ev_r0 = nullptr, ev_refresh = nullptr;   // uic_topdown_refresh_weights: main -> side, side -> consumers
  bool refresh_pending = false;
  // The refresh in two halves: the operand-dtype copies (all the forward pass needs; ev_cast) are enqueued by the call
  // itself, the transposes (backward pass only) by the first consumer -- the fused step puts its side-stream prologue branch
  // in front of them, everything else gets them through wait_refresh.
  hipEvent_t ev_cast = nullptr;
  bool cast_recorded = false, transposes_pending = false;
  // uic_topdown_refresh_weights_gathered (deferred form): the side stream's copies of gather group 2 (embedding table, fc_embed,
  // att_lstm.weight_ih) are done -- the fused step's third stream (fc_embed, Gfc) waits for it; cleared by every other refresh
  hipEvent_t ev_g2 = nullptr;
  bool g2_recorded = false;
  // ... and its late half: the copies of gather groups 1 and 0 (recurrent LSTM matrices, logit layer), the last bytes to arrive.
  // Deferred to the fused step, which enqueues them BEHIND its third stream's prologue branch -- in front of it they would hold
  // that branch back until the last all-gather is through; nothing before the recurrence reads them (ev_gl: they are done)
  bool gl_pending = false, gl_recorded = false;
  hipEvent_t ev_gl = nullptr;
  const void* gl_src[UIC_CAST_MULTI]; void* gl_dst[UIC_CAST_MULTI]; size_t gl_bytes[UIC_CAST_MULTI]; int gl_count = 0;
  void* gl_ready[2] = {nullptr, nullptr};
  uic_topdown_dims tp_d; uic_topdown_weights tp_w; void* tp_derived = nullptr;
  hipEvent_t ev_main[MAX_CHUNKS];   // main  -> side: decode steps of chunk c are finished
  hipEvent_t ev_side[MAX_CHUNKS];   // side  -> main: d hdrop of chunk c is ready
  bool ready = false;
  int compact_launches = 0;         // uic_topdown_compact_launches: of the last fused step
  // uic_topdown_step_marks: timing events of the last fused step (only recorded while marks_on)
  bool marks_on = false, marks_valid = false;
  hipEvent_t mark[UIC_STEP_MARKS];
};
// the calling device's instance (one per device, created on first use; topdown_features.hip holds them)
int get_side(SideStream** out);
// the late half of uic_topdown_refresh_weights_gathered (see SideStream::gl_pending), on `st`
int flush_gathered_late(SideStream* ss, hipStream_t st);
// the deferred half of uic_topdown_refresh_weights: the transposed copies the backward pass reads, on the side stream
int flush_transposes(SideStream* ss);
// every consumer of the derived weights first lets its stream wait for the side-stream part of the last refresh
int wait_refresh(hipStream_t s);

// One teacher-forced step of the captioner on one GPU, split into the pieces the public entry points
// (and the two-stream fused training step) sequence.
struct Step {
  uic_topdown_dims d;
  const uic_topdown_weights* w;
  const uic_topdown_batch* b;
  const uic_topdown_weights* G;
  Layout L;
  Derived dv;
  int dt, N, R, D, Dfc, H, E, A, V1, V1p, H4, ldih, t_run, Meff, Mp, Np, NR, NRp;
  size_t S, NH;
  float drop_p, inv_keep;
  unsigned seed;
  int training;          // bit 0: train mode; bit 1: keep the BatchNorm running statistics untouched
  const void* fc_in;
  const void* att_in;
  void init(const uic_topdown_dims* d_, const uic_topdown_weights* w_, const void* derived, const uic_topdown_batch* b_,
            int t_run_, int training_, unsigned seed_, void* workspace, const uic_topdown_weights* G_);
  // scheduled sampling (AttModel.py:130-143) is active in train mode only
  bool ss_on() const { return (training & 1) && b->ss_prob > 0.f; }
  bool embed_prepared = false;   // the fused step bucketed the tokens (uic_embed_bwd_sorted_prepare) while the side stream was idle
  // Live-position logit layer (round 6).  uic_topdown_batch.live_rows / live_count list the (step, row) positions whose mask is not
  // zero; positions behind a caption's end -- a quarter of the benchmark's, a third of COCO's -- have loss 0 and gradient 0, so the
  // logit layer (GEMM, criterion, d hdrop, its weight gradient) runs over the listed rows only: gathered into L.hc, logits / d
  // logits / d hdrop compact, d hdrop scattered back into the (zeroed) step-major buffer the BPTT loop reads.
  bool compact = false, build_live = false;
  const int32_t* live_rows = nullptr;
  int live_off[UIC_MAX_LIVE_STEPS + 1];
  int live_total() const { return live_off[t_run]; }
  int live_pad() const { return (live_total() + 127) & ~127; }
  void init_live();
  // fused_gather: the persistent recurrence stores every live row of hdrop into the compact operand itself (rnn_persist.hip, by the
  // list's inverse): no gather launches -- one of them sat on the main stream in front of the BPTT loop.  The list kernel clears the
  // operand's padding rows then.
  bool fused_gather = false;
  // have_len: L.cap_len holds every row's caption length (1 + the last decode step with a non-zero mask / gradient weight): the BPTT
  // loop's attention backward and the attention accumulation skip the steps behind it.  Made with the list, or -- a step that
  // computes every position with per-position weights (the self-critical step: a sampled caption's positions behind its end weigh
  // zero) -- by the list kernel alone.
  bool have_len = false;
  // rows_by_len (uic_topdown_batch.unfinished_count, with have_len on the split-K chain): the two d x GEMMs of a BPTT step whose
  // unfinished rows fill fewer 128-row tiles than the batch run over those rows only (compact_step), A from L.dg2c / L.dg1c --
  // the cell backward kernels store the unfinished rows there a second time, by rank -- and the slab rows placed by L.row_order,
  // so the slabs stay position-indexed; their consumers take zeros for the rows that were not written.  Every gradient of an
  // ended row is an exact zero and an output row of the GEMM depends on its own A row only: the results do not change.
  bool rows_by_len = false;
  int unf[UIC_MAX_LIVE_STEPS + 1];
  int compact_launches = 0;      // d x GEMM launches of this step that took the compact form
  void init_rows_by_len();
  bool compact_step(int t) const { return rows_by_len && unf[t] > 0 && (unf[t] + 127) / 128 < (N + 127) / 128; }
  int len_build(hipStream_t s);
  int live_build(hipStream_t s);
  int embed_split = 0;           // > 0: ... into the halves [0, embed_split) / [embed_split, t_run) of the decode steps (embed_grad)
  // d.recurrence & UIC_REC_EARLY_GRADS (fused step): the order of the gradient work a data-parallel caller may prefer -- see
  // uic_topdown_xe_train_step
  bool early_grads() const { return (d.recurrence & UIC_REC_EARLY_GRADS) != 0; }
  const int64_t* embed_tokens() const { return ss_on() ? L.tok_used : b->labels; }
  int embed_ldtok() const { return ss_on() ? d.T : b->ld_labels; }
  // gfc_separate: the persistent recurrence adds the caption row's fc' term (Gfc) itself, so the batched input GEMM (the long
  // pole of the prologue's side-stream branch) no longer queues behind cast -> fc_embed -> Gfc; the launch chain keeps Gfc
  // folded into Gx (one operand less per step).  Same f32 additions in the same order either way.
  bool gfc_separate() const { return persist_ok(); }
  int fwd_embed(hipStream_t s);
  int fwd_gx(hipStream_t s, bool with_gfc);
  int fwd_prologue(hipStream_t s, int part = 0);
  int fwd_step_inputs(int t, const int64_t* tok, int ld, hipStream_t s);
  int fwd_gfc(hipStream_t s, bool with_bias = false);
  void rnn_fwd_params(UicRnnFwdParams& p, int t0, int t1) const;
  bool decode_persist_ok(int sample_max, float temperature, int decoding_constraint) const {
    return !(d.recurrence & UIC_REC_FWD_CHAIN) && !decoding_constraint && (sample_max || temperature == 1.f) && d.logit_layers <= 1 &&
           uic_rnn_decode_persist_eligible(dt, N, H, A, R, E, V1);
  }
  int decode_persist(int Lsteps, int sample_max, const int64_t* forced, bool keep, int64_t* seq, float* seq_logp, hipStream_t s);
  int fwd_step(int t, hipStream_t s, bool inline_inputs = false);
  bool persist_ok() const {
    return !ss_on() && !(d.recurrence & UIC_REC_FWD_CHAIN) && uic_rnn_persist_eligible(dt, N, H, A, R);
  }
  int fwd_steps(int t0, int t1, hipStream_t s);
  int logits_rows(int t0, int t1, hipStream_t s);
  // logit_layers = n > 1 (AttModel.py:90-91): n - 1 blocks Linear(H, H) + ReLU + Dropout(0.5) in front of the vocabulary layer
  int nlh() const { return d.logit_layers > 1 ? d.logit_layers - 1 : 0; }
  const void* logit_in_all() const { return nlh() ? L.lh[nlh() - 1] : L.hdrop_all; }
  int live_begin(hipStream_t s) { return uic_zero4_launch(L.dhdrop, (size_t)Meff * H * 4, nullptr, 0, nullptr, 0, nullptr, 0, s); }
  int live_c0(int t0) const { return live_off[t0]; }
  int live_rows_of(int t0, int t1) const { return (t1 == t_run ? live_pad() : live_off[t1]) - live_off[t0]; }
  int logits_rows_live(int t0, int t1, hipStream_t s);
  int logits_rows_now(int t0, int t1, hipStream_t s);
  int xe_rows(int t0, int t1, const float* inv, float* logprobs_out, int with_loss, hipStream_t s);
  int dh_rows(int t0, int t1, hipStream_t s, bool side = false);
  int logit_weight_grads(hipStream_t s, UicWgPlace at);
  // with_fwd_sync (the fused step, whose third stream runs this beside the prologue): the forward recurrence's sync block is
  // cleared here too, so that no memset node sits between the prologue's join and the persistent launch on the main stream
  bool fwd_sync_clean = false;
  int bwd_begin(hipStream_t s, bool with_fwd_sync = false, bool with_live = false);
  bool bwd_persist_ok() const { return (d.recurrence & UIC_REC_BWD_PERSIST) && uic_rnn_bwd_persist_eligible(dt, N, H, A, R); }
  int bwd_launches = 0;
  int bwd_steps(int t_lo, int t_hi, hipStream_t s);
  // The two d x GEMMs of a BPTT step (640 x 1536 / 1024 outputs, K = 4H) run as BPTT_SPLIT K slices on the LDS-DMA kernel with
  // 128 x 128 tiles (half the operand traffic of the 64 x 64 skinny tiles, a quarter of the K rounds per workgroup); the slices
  // land in partial slabs and are summed by whoever reads them next -- the cell backward kernels and the attention backward
  // kernel (which leaves the summed d att_res where the deferred accumulation pass expects it): no reduction launch.
  // 15.2 -> 12.7 us and 14.5 -> 11.6 us per launch isolated (profiles/r03_v2_gemm_headroom.txt).  0: small problems, direct GEMMs.
  int bptt_split() const {
    const int rounds = H4 / (dt == UIC_BF16 ? 64 : 32);
    return (N >= 256 && H % 128 == 0 && uic_gemm_glds_eligible(dt, H4) && rounds % BPTT_SPLIT == 0 && rounds / BPTT_SPLIT >= 4) ? BPTT_SPLIT : 0;
  }
  int bwd_step(int t, hipStream_t s);
  int bwd_epilogue(hipStream_t s);
  // (at: where the weight gradients run, beside the BPTT chain or alone on the chip -- every method that issues them takes it
  // from its caller)
  int wgrad_group(float* slab, const void* A, int lda, int lrows, const UicGemmTnSeg* segs, int nseg, int rows, const WDest* dst,
                  int nd, hipStream_t s, bool accumulate, void* tA, void* tB, UicWgPlace at) {
    return ::wgrad_group(slab, L.slab_bytes, dt, A, lda, lrows, segs, nseg, rows, dst, nd, s, accumulate, tA, tB, at);
  }
  int wgrad_chunk(int t0, int t1, bool first, UicWgPlace at, hipStream_t s, bool third, hipStream_t sb = nullptr);
  // true when EVERY chunk's LSTM weight-gradient GEMM takes the direct transposing-read (TN) path with room for one more
  // 128-column segment: bf16, whole 64-row K rounds per decode step, 128-multiples everywhere
  bool bias_in_chunks() const {
    return dt == UIC_BF16 && N % 64 == 0 && H % 128 == 0 && E % 128 == 0 && (3 * H + 128) / 128 * (H4 / 128) >= 160 && (2 * H + E + 128) / 128 * (H4 / 128) >= 160;
  }
  int fc_cols_grad(hipStream_t s, float* slab, void* tA, void* tB, UicWgPlace at);
  int embed_grad(int half, hipStream_t s);
  int bias_hh_copies(hipStream_t s);
  int bwd_epilogue_early(hipStream_t s, UicWgPlace at, bool chunked = false, bool side = false, bool first_done = false, bool bias_copies = true);
  int bwd_epilogue_late(hipStream_t s, UicWgPlace at, bool chunked = false, int part = 0);
};

// the LSTM cells' GEMMs of a decode step (topdown_step.hip), shared by Step::fwd_step and decode_step
UicGemmParams att_lstm_gemm(const uic_topdown_dims& d, const uic_topdown_weights* w, const Derived& dv, const Layout& L,
                            const void* h_lang_prev, const void* h_att_prev, const float* c_prev, float* c_out, void* h_out, int t,
                            const void* xt_inline, bool store_gates);
UicGemmParams lang_lstm_gemm(const uic_topdown_dims& d, const uic_topdown_weights* w, const Derived& dv, const Layout& L, const void* ctx,
                             const void* h_att_new, const void* h_lang_prev, const float* c_prev, float* c_out, void* h_out,
                             void* h_drop, int t, float drop_p, unsigned seed, bool store_gates);
// One decode step of AttModel.get_logprobs_state (:158-165) on the sampling buffers: embedding of L.s_it, both LSTM cells,
// attention, logits into L.s_logits; recurrent state read from slot `cur`, written to slot `nxt`.
int decode_step(const uic_topdown_dims& d, const uic_topdown_weights* w, const Derived& dv, const uic_topdown_batch* b, const Layout& L,
                int cur, int nxt, int t, float drop_p, unsigned seed, hipStream_t s, bool train_mode = false, bool xt_ready = false);

}  // namespace topdown
