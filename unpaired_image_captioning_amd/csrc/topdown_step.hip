// The pieces of one teacher-forced step of the TopDown captioner (struct Step, topdown_internal.h): forward prologue and
// recurrence, logit layer, live-position list, BPTT, weight-gradient groups and epilogues.  topdown_train.hip sequences them.
#include "topdown_internal.h"

namespace topdown {

void Step::init(const uic_topdown_dims* d_, const uic_topdown_weights* w_, const void* derived, const uic_topdown_batch* b_,
          int t_run_, int training_, unsigned seed_, void* workspace, const uic_topdown_weights* G_) {
  d = *d_; w = w_; b = b_; G = G_;
  L = make_layout(d, workspace);
  dv = make_derived(d, w, (void*)derived);
  dt = d.dtype; N = d.N; R = d.R; D = d.D; Dfc = d.Dfc; H = d.H; E = d.E; A = d.A; V1 = d.V1;
  V1p = (int)vpad(V1); H4 = 4 * H; ldih = E + 2 * H; t_run = t_run_;
  Meff = t_run * N; Mp = (int)rup8(Meff); Np = (int)rup8(N); NR = N * R; NRp = (int)rup8(NR);
  S = uic_dtype_size(dt); NH = (size_t)N * H;
  training = training_;
  drop_p = (training & 1) ? d.drop_p : 0.f;
  inv_keep = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
  seed = seed_;
  fc_in = (dt == UIC_BF16 || d.seq_per_img > 1) ? L.fcT : (const void*)b->fc_feats;
  att_in = (dt == UIC_BF16 || d.use_bn) ? L.attT : (const void*)b->att_feats;   // per image when seq_per_img > 1
}

void Step::init_live() {
  compact = false;
  build_live = false;
  if (!b->live_count || !b->masks || t_run > UIC_MAX_LIVE_STEPS || ss_on() || b->grad_scale || nlh() != 0) return;
  if (((size_t)H * uic_dtype_size(dt)) % 16 != 0) return;     // (rows move as 16-byte pieces)
  live_off[0] = 0;
  for (int t = 0; t < t_run; ++t) {
    const int c = b->live_count[t];
    if (c < 0 || c > N) return;                       // (not a list of this batch: the plain path)
    live_off[t + 1] = live_off[t] + c;
  }
  // (no list from the caller: one small launch compacts the masks on the device, uic_live_list_launch -- the caller then
  // ships nothing but the counts it sizes the launches with)
  build_live = b->live_rows == nullptr;
  live_rows = build_live ? L.live_map : b->live_rows;
  compact = true;
}
// after init_live, before live_build.  The counts size launches and nothing else: whatever they hold, every launch stays inside its
// buffers (0 <= count <= N rows of an [N, 4H] operand; the map's entries are the device's own, each below N) -- counts that are not
// those of the masks are reported by the list kernel through the status word, never by a fault.
void Step::init_rows_by_len() {
  rows_by_len = false;
  compact_launches = 0;
  if (!b->unfinished_count || !compact || !build_live || !d.rnn_status || dt != UIC_BF16 || !bptt_split() || !uic_live_order_ok(N, t_run)) return;
  if ((size_t)N * H < 65536 || H % 32 != 0 || A % 128 != 0 || A > 512 || A == 384) return;   // (the two cell backward kernels that take row_len)
  for (int t = 0; t < t_run; ++t) {
    unf[t] = b->unfinished_count[t];
    if (unf[t] < 0 || unf[t] > N) return;
  }
  unf[t_run] = 0;
  rows_by_len = true;
}
int Step::len_build(hipStream_t s) {
  return uic_live_list_launch(b->grad_scale, b->ld_grad_scale, 0, N, t_run * N, L.live_map, 0, s, nullptr, nullptr, 0, L.cap_len);
}
int Step::live_build(hipStream_t s) {
  const size_t S = uic_dtype_size(dt);
  const UicLiveOrder ord{L.row_order, L.row_rank, L.unfinished, b->unfinished_count, d.rnn_status};
  return uic_live_list_launch(b->masks, b->ld_masks, 1, N, t_run * N, L.live_map, live_pad(), s, fused_gather ? L.live_inv : nullptr,
                              fused_gather ? offw(L.hc, (size_t)live_total() * H, dt) : nullptr,
                              fused_gather ? (size_t)(live_pad() - live_total()) * H * S : 0, L.cap_len, rows_by_len ? &ord : nullptr);
}

// ---------------------------------------------------------------- forward
int Step::fwd_embed(hipStream_t s) {
  // xt_t = dropout(relu(embed[labels[:, t]])) for all steps (AttModel.py:145,160)
  return uic_embed_fwd_t_launch(dt, dv.embed_w, dt, V1, E, b->labels, b->ld_labels, N, t_run, drop_p, seed, UIC_SITE_EMBED, 0, 1, L.xt_all, s);
}
int Step::fwd_gx(hipStream_t s, bool with_gfc) {
  // Gx = xt W_ih[:, 2H:]^T + b_ih + b_hh [+ Gfc (every step's rows get their caption row's fc' term)], all steps
  UicGemmParams g = gemm_base(dt, Meff, H4);
  add_seg(g, L.xt_all, E, off(dv.att_w_ih, 2 * H, dt), ldih, E);
  g.C = L.gx; g.ldc = H4; g.bias = w->att_lstm_b_ih; g.bias2 = w->att_lstm_b_hh; g.flags = UIC_GEMM_OUT_F32;
  if (with_gfc) { g.addend = L.gfc; g.add_mod = N; g.ld_add = H4; }
  return uic_gemm_launch(g, s);
}
// part: 0 = everything; 1 = the side stream's branch (embedding, batched input GEMM, fc_embed, Gfc, initial state); 2 = the
// main stream's (att_embed, ctx2att); with gfc_separate() the side branch splits again into 3 = embedding + batched input
// GEMM and 4 = fc_embed + Gfc + initial state (independent of each other: the fused step gives 4 to its third stream)
int Step::fwd_prologue(hipStream_t s, int part) {
  const void *f, *a;
  const bool sep = gfc_separate();
  UIC_REQUIRE(part < 3 || sep, "fwd_prologue: parts 3 / 4 need the separate Gfc");
  if (part != 2 && part != 4 && sep) {
    UIC_TRY(fwd_embed(s));
    UIC_TRY(fwd_gx(s, false));
  }
  if (part == 3) return UIC_OK;
  UIC_TRY(prepare_features(d, w, dv, b, L, training, drop_p, seed, &f, &a, s, part == 4 ? 1 : part));
  if (part == 2) return UIC_OK;
  if (!sep) UIC_TRY(fwd_embed(s));
  UIC_TRY(fwd_gfc(s));
  if (!sep) UIC_TRY(fwd_gx(s, true));
  if (ss_on()) UIC_TRY(uic_copy_tokens_launch(b->labels, b->ld_labels, N, t_run, L.tok_used, d.T, s));
  // init_hidden (AttModel.py:94-97): slot 0 of the four state buffers, one launch
  return uic_zero4_launch(L.h_att, NH * S, L.h_lang, NH * S, L.c_att, NH * 4, L.c_lang, NH * 4, s);
}

// step t's embedding row block and its slice of Gx from the tokens tok[n * ld] (the prologue made them from the labels)
int Step::fwd_step_inputs(int t, const int64_t* tok, int ld, hipStream_t s) {
  UIC_TRY(uic_embed_fwd_t_launch(dt, dv.embed_w, dt, V1, E, tok, ld, N, 1, drop_p, seed, UIC_SITE_EMBED,
                               (size_t)t * N * E, 1, offw(L.xt_all, (size_t)t * N * E, dt), s));
  UicGemmParams g = gemm_base(dt, N, H4);
  add_seg(g, off(L.xt_all, (size_t)t * N * E, dt), E, off(dv.att_w_ih, 2 * H, dt), ldih, E);
  g.C = L.gx + (size_t)t * N * H4; g.ldc = H4; g.bias = w->att_lstm_b_ih; g.bias2 = w->att_lstm_b_hh; g.flags = UIC_GEMM_OUT_F32;
  g.addend = L.gfc; g.add_mod = N; g.ld_add = H4;
  return uic_gemm_launch(g, s);
}
// Gfc = fc' W_ih[:, H:2H]^T, the caption row's share of every step's att_lstm pre-activations
int Step::fwd_gfc(hipStream_t s, bool with_bias) {
  UicGemmParams g = gemm_base(dt, N, H4);
  add_seg(g, L.fcp, H, off(dv.att_w_ih, H, dt), ldih, H);
  g.C = L.gfc; g.ldc = H4; g.flags = UIC_GEMM_OUT_F32;
  if (with_bias) { g.bias = w->att_lstm_b_ih; g.bias2 = w->att_lstm_b_hh; }
  return uic_gemm_launch(g, s);
}

// what the persistent recurrence's training launch (fwd_steps) and its decode launch (decode_persist) share
void Step::rnn_fwd_params(UicRnnFwdParams& p, int t0, int t1) const {
  memset(&p, 0, sizeof(p));
  p.dtype = dt; p.N = N; p.R = R; p.t0 = t0; p.t1 = t1;
  p.att_w_ih = dv.att_w_ih; p.ld_att_ih = ldih; p.att_w_hh = dv.att_w_hh;
  p.lang_w_ih = dv.lang_w_ih; p.lang_w_hh = dv.lang_w_hh;
  p.lang_b_ih = w->lang_lstm_b_ih; p.lang_b_hh = w->lang_lstm_b_hh;
  p.h2att_w = dv.h2att_w; p.h2att_b = w->h2att_b;
  p.w_alpha = w->alpha_w; p.b_alpha = w->alpha_b;
  p.p_att = L.patt; p.att = L.attp;
  p.mask = b->att_masks ? (d.seq_per_img > 1 ? L.amask_rep : b->att_masks) : nullptr; p.ldmask = R;
  p.h_att = L.h_att; p.h_lang = L.h_lang; p.c_att = L.c_att; p.c_lang = L.c_lang;
  p.att_h_all = L.atth_all; p.alpha_all = L.alpha_all; p.ctx_all = L.ctx_all; p.hdrop_all = L.hdrop_all;
  p.drop_p = drop_p; p.seed = seed;
  p.sync = L.rnn_sync;
  p.force_safe = (d.recurrence & UIC_REC_SAFE) != 0; p.status = d.rnn_status;
  p.dbg = (d.recurrence & UIC_REC_STAMPS) ? L.rnn_dbg : nullptr; p.dbg_T = d.T;
}

// ---------------------------------------------------------------- decode as one persistent launch
// AttModel._sample (P/models/AttModel.py:198-253) with beam_size = 1: all Lsteps decode steps -- embedding of the previous
// step's token, att_lstm, attention, lang_lstm, the logit layer and the greedy / multinomial choice -- in ONE launch of
// rnn_persist.hip's decode mode instead of six launches per step.  bf16, the default temperature, no decoding constraint,
// one logit layer; everything else keeps the per-step chain.  keep: the training layout's activations, the embedded inputs
// and every step's logits stay in the workspace for uic_topdown_xe_train_step(training | 4).
int Step::decode_persist(int Lsteps, int sample_max, const int64_t* forced, bool keep, int64_t* seq, float* seq_logp, hipStream_t s) {
  UIC_TRY(fwd_gfc(s, true));
  UIC_TRY(uic_rnn_decode_embed_relu_launch(dv.embed_w, dt, L.dec_embed_relu, V1, E, s));
  UIC_TRY(uic_fill_launch(L.dec_tok, 0, (size_t)N * 4, s));          // <bos> = 0 (AttModel.py:214-215)
  UicRnnFwdParams p;
  rnn_fwd_params(p, 0, Lsteps);
  p.gx = nullptr; p.gfc = L.gfc;
  p.gates1 = keep ? L.gates1 : nullptr; p.gates2 = keep ? L.gates2 : nullptr;
  p.dec = 1;
  p.dec_embed_relu = L.dec_embed_relu; p.dec_xw = off(dv.att_w_ih, 2 * H, dt); p.dec_ld_xw = ldih;
  p.dec_xt_drop = drop_p; p.dec_xt_all = keep ? L.xt_all : nullptr;
  p.dec_logit_w = dv.logit_w; p.dec_logit_b = w->logit_b; p.dec_V1 = V1; p.dec_V1p = V1p;
  p.dec_logits = keep ? L.logits : L.s_logits; p.dec_logits_step = keep ? (size_t)N * V1p : 0;
  p.dec_part = L.dec_part; p.dec_tok = L.dec_tok; p.dec_unf = L.smp.unfinished;
  p.dec_seq = seq; p.dec_seq_logp = seq_logp; p.dec_ld_out = Lsteps;
  p.dec_forced = sample_max ? nullptr : forced; p.dec_ld_forced = Lsteps;
  p.dec_sample_max = sample_max; p.dec_draw_seed = seed;
  UIC_TRY(uic_rnn_fwd_persist_launch(p, s));
  return uic_rnn_decode_finish_launch(seq, seq_logp, N, Lsteps, Lsteps, (const int*)d.rnn_status, s);
}

// The two LSTM cells of a decode step as one GEMM each with the cell in its epilogue, for the training layout (Step::fwd_step)
// and the sampling buffers (decode_step).  The order of the K segments is the GEMM's summation order: the same in both.
// att_lstm on cat([h_lang_prev, fc', xt]) (AttModel.py:431-434).  xt_inline: xt_t and fc' enter as K segments of their own (with
// both biases); nullptr: through step t's slice of the prologue's Gx (Gfc is already folded into it).  store_gates: into L.gates1.
UicGemmParams att_lstm_gemm(const uic_topdown_dims& d, const uic_topdown_weights* w, const Derived& dv, const Layout& L,
                            const void* h_lang_prev, const void* h_att_prev, const float* c_prev, float* c_out, void* h_out, int t,
                            const void* xt_inline, bool store_gates) {
  const int dt = d.dtype, N = d.N, H = d.H, E = d.E, H4 = 4 * H, ldih = E + 2 * H;
  UicGemmParams g = gemm_base(dt, N, H4);
  g.lstm = 1; g.H = H;
  add_seg(g, h_lang_prev, H, dv.att_w_ih, ldih, H);
  if (xt_inline) {
    add_seg(g, L.fcp, H, off(dv.att_w_ih, H, dt), ldih, H);
    add_seg(g, xt_inline, E, off(dv.att_w_ih, 2 * H, dt), ldih, E);
    g.bias = w->att_lstm_b_ih; g.bias2 = w->att_lstm_b_hh;
  } else {
    g.pre1 = L.gx + (size_t)t * N * H4; g.ldpre1 = H4;
  }
  add_seg(g, h_att_prev, H, dv.att_w_hh, H, H);
  g.c_prev = c_prev; g.c_out = c_out;
  g.h_out = h_out; g.ldh = H;
  if (store_gates) g.gates_out = offw(L.gates1, (size_t)t * N * H4, dt);
  return g;
}
// lang_lstm on cat([att_res, h_att]) (AttModel.py:438-441) + output dropout (:443): dropout(h_lang) feeds the logit layer
UicGemmParams lang_lstm_gemm(const uic_topdown_dims& d, const uic_topdown_weights* w, const Derived& dv, const Layout& L, const void* ctx,
                             const void* h_att_new, const void* h_lang_prev, const float* c_prev, float* c_out, void* h_out,
                             void* h_drop, int t, float drop_p, unsigned seed, bool store_gates) {
  const int dt = d.dtype, N = d.N, H = d.H, H4 = 4 * H;
  UicGemmParams g = gemm_base(dt, N, H4);
  g.lstm = 1; g.H = H;
  add_seg(g, ctx, H, dv.lang_w_ih, 2 * H, H);
  add_seg(g, h_att_new, H, off(dv.lang_w_ih, H, dt), 2 * H, H);
  add_seg(g, h_lang_prev, H, dv.lang_w_hh, H, H);
  g.bias = w->lang_lstm_b_ih; g.bias2 = w->lang_lstm_b_hh;
  g.c_prev = c_prev; g.c_out = c_out;
  g.h_out = h_out; g.ldh = H;
  g.h_drop = h_drop; g.ldhd = H;
  g.drop_p = drop_p; g.seed = seed; g.site = UIC_SITE_OUT0 + (unsigned)t;
  if (store_gates) g.gates_out = offw(L.gates2, (size_t)t * N * H4, dt);
  return g;
}

// inline_inputs: xt_t and fc' enter att_lstm's GEMM as K segments of their own (with both biases) instead of through the
// prologue's Gx -- the sampling pass, whose step-t embedding exists only once step t - 1 has drawn its tokens
int Step::fwd_step(int t, hipStream_t s, bool inline_inputs) {
  if (ss_on() && t >= 1) {
    // choose this step's input tokens from the previous step's distribution, then redo the step's embedding row block
    // and its slice of Gx (the prologue's teacher-forced values for the rows that keep their label are recomputed too)
    UIC_TRY(uic_ss_sample_launch(L.logits + (size_t)(t - 1) * N * V1p, N, V1, V1p, b->labels, b->ld_labels, t, b->ss_prob, seed,
                                 L.tok_used, d.T, s));
    UIC_TRY(fwd_step_inputs(t, L.tok_used + t, d.T, s));
  }
  const void* h_att_prev = off(L.h_att, t * NH, dt);
  void* h_att_new = offw(L.h_att, (t + 1) * NH, dt);
  const void* h_lang_prev = off(L.h_lang, t * NH, dt);
  void* h_lang_new = offw(L.h_lang, (t + 1) * NH, dt);
  UIC_TRY(uic_gemm_launch(att_lstm_gemm(d, w, dv, L, h_lang_prev, h_att_prev, L.c_att + t * NH, L.c_att + (t + 1) * NH, h_att_new, t,
                                        inline_inputs ? off(L.xt_all, (size_t)t * N * E, dt) : nullptr, true), s));
  UIC_TRY(attention_step(d, w, dv, b, L, h_att_new, L.atth_all + (size_t)t * N * A, L.alpha_all + (size_t)t * N * R,
                         offw(L.ctx_all, t * NH, dt), s));
  UIC_TRY(uic_gemm_launch(lang_lstm_gemm(d, w, dv, L, off(L.ctx_all, t * NH, dt), h_att_new, h_lang_prev, L.c_lang + t * NH,
                                         L.c_lang + (t + 1) * NH, h_lang_new, offw(L.hdrop_all, t * NH, dt), t, drop_p, seed, true), s));
  if (ss_on()) UIC_TRY(logits_rows_now(t, t + 1, s));   // the next step samples from this step's distribution
  return UIC_OK;
}

// decode steps [t0, t1) of the recurrence: one persistent launch (rnn_persist.hip) when the shapes allow, else the
// per-step chain.  Scheduled sampling needs the logits of step t - 1 on the host-sequenced path.
// The persistent kernel holds every CU (160 KB of LDS, the whole register file): inside the two-stream training step the
// logit layer cannot run beside it; it follows chunk by chunk, last chunk first, beside the BPTT loop (see
// uic_topdown_xe_train_step).  d.recurrence & UIC_REC_FWD_CHAIN keeps the per-step launches.
int Step::fwd_steps(int t0, int t1, hipStream_t s) {
  if (!persist_ok()) {
    for (int t = t0; t < t1; ++t) UIC_TRY(fwd_step(t, s));
    return UIC_OK;
  }
  UicRnnFwdParams p;
  rnn_fwd_params(p, t0, t1);
  p.gx = L.gx; p.gfc = gfc_separate() ? L.gfc : nullptr;
  p.e_att = L.eatt;
  p.gates1 = L.gates1; p.gates2 = L.gates2;
  if (fused_gather) { p.live_inv = L.live_inv; p.hdrop_live = L.hc; }
  p.sync_zeroed = fwd_sync_clean ? 1 : 0;
  fwd_sync_clean = false;            // (one launch's worth)
  return uic_rnn_fwd_persist_launch(p, s);
}

// logits of decode steps [t0, t1) (AttModel.py:163); under scheduled sampling every step already produced its own
int Step::logits_rows(int t0, int t1, hipStream_t s) {
  if (ss_on()) return UIC_OK;
  return logits_rows_now(t0, t1, s);
}
// rows [c0, c0 + rows) of the live list = the live positions of decode steps [t0, t1); the list's last chunk carries the padding
// rows up to a multiple of 128 (zero operand rows, zero gradient rows: the weight-gradient GEMM's K runs over whole tiles)
// d hdrop of the positions the list leaves out is zero: the whole buffer is cleared before the chunks scatter into it
int Step::logits_rows_live(int t0, int t1, hipStream_t s) {
  const int c0 = live_c0(t0), real = live_off[t1] - c0, rows = live_rows_of(t0, t1);
  if (!fused_gather) UIC_TRY(uic_gather_rows_launch(L.hdrop_all, live_rows + c0, Meff, offw(L.hc, (size_t)c0 * H, dt), real, rows, (size_t)H * uic_dtype_size(dt), s));
  if (rows == 0) return UIC_OK;
  UicGemmParams g = gemm_base(dt, rows, V1);
  add_seg(g, off(L.hc, (size_t)c0 * H, dt), H, dv.logit_w, H, H);
  g.C = L.logits + (size_t)c0 * V1p; g.ldc = V1p; g.bias = w->logit_b; g.flags = UIC_GEMM_OUT_F32;
  return uic_gemm_launch(g, s);
}
int Step::logits_rows_now(int t0, int t1, hipStream_t s) {
  if (compact) return logits_rows_live(t0, t1, s);
  const int rows = (t1 - t0) * N;
  for (int l = 0; l < nlh(); ++l) {
    UicGemmParams g = gemm_base(dt, rows, H);
    add_seg(g, off(l ? L.lh[l - 1] : L.hdrop_all, t0 * NH, dt), H, dv.logit_h_w[l], H, H);
    g.C = offw(L.lh[l], t0 * NH, dt); g.ldc = H; g.bias = w->logit_h_b[l]; g.flags = UIC_GEMM_RELU;
    if (training & 1) { g.drop_p = 0.5f; g.seed = seed; g.site = UIC_SITE_LOGIT_H0 + (unsigned)l; g.drop_row0 = t0 * N; }
    UIC_TRY(uic_gemm_launch(g, s));
  }
  UicGemmParams g = gemm_base(dt, rows, V1);
  add_seg(g, off(logit_in_all(), t0 * NH, dt), H, dv.logit_w, H, H);
  g.C = L.logits + (size_t)t0 * N * V1p; g.ldc = V1p; g.bias = w->logit_b; g.flags = UIC_GEMM_OUT_F32;
  return uic_gemm_launch(g, s);
}
// log-softmax + LanguageModelCriterion rows of steps [t0, t1): row losses and d logits
int Step::xe_rows(int t0, int t1, const float* inv, float* logprobs_out, int with_loss, hipStream_t s) {
  UicXeParams x;
  memset(&x, 0, sizeof(x));
  const size_t r0 = (size_t)t0 * N;
  x.dtype = dt; x.M = (t1 - t0) * N; x.V1 = V1; x.ldv = V1p; x.N = N;
  x.logits = L.logits + r0 * V1p;
  if (compact && with_loss) {
    // the live list's rows of these steps: logits / d logits / row losses are indexed by list position, labels and masks by the
    // (step, row) the list names (steps counted from 0: the column offsets below are those of step 0)
    const int c0 = live_c0(t0);
    x.M = live_rows_of(t0, t1);
    if (x.M == 0) return UIC_OK;
    x.row_map = live_rows + c0; x.row_map_limit = Meff;
    x.logits = L.logits + (size_t)c0 * V1p;
    x.dlogits = offw(L.dlogits, (size_t)c0 * V1p, dt);
    x.target = b->labels; x.ldtarget = b->ld_labels; x.target_col0 = 1;
    x.mask = b->masks; x.ldmask = b->ld_masks; x.mask_col0 = 1;
    x.inv_den = inv; x.row_loss = L.row_loss + c0; x.write_grad = 1;
    return uic_xe_launch(x, s);
  }
  if (with_loss) {
    x.dlogits = offw(L.dlogits, r0 * V1p, dt);
    x.target = b->labels; x.ldtarget = b->ld_labels; x.target_col0 = 1 + t0;
    x.mask = b->masks; x.ldmask = b->ld_masks; x.mask_col0 = 1 + t0;
    x.inv_den = inv; x.row_loss = L.row_loss + r0; x.write_grad = 1;
    x.grad_scale = b->grad_scale; x.ldscale = b->ld_grad_scale; x.scale_col0 = t0;
  }
  if (logprobs_out) {
    x.logprobs = logprobs_out + (size_t)t0 * V1; x.lp_step_stride = V1; x.lp_row_stride = (size_t)d.T * V1;
  }
  return uic_xe_launch(x, s);
}
// d hdrop rows of steps [t0, t1) = d logits W_logit
// (long K = V1, few output tiles: split-K over workgroups on the LDS-DMA GEMM when the shape allows; `side` picks
// the side stream's slab)
int Step::dh_rows(int t0, int t1, hipStream_t s, bool side) {
  if (compact) {
    const int c0 = live_c0(t0), real = live_off[t1] - c0;
    if (real == 0) return UIC_OK;
    const WDest dc{L.dhc + (size_t)c0 * H, H, 0, H};
    // (a chunk of a few rows -- the captions' last steps -- runs as one whole 128-row tile of the split-K kernel instead of the
    // generic one, 50 -> 17 us on the main stream in front of the BPTT loop: the rows behind the chunk's are the next chunk's or
    // padding, inside both buffers, and what they produce is not scattered)
    const int rows = real < 128 ? 128 : real;
    // (the split-K reduce places the rows itself; the direct GEMM -- shapes off the split-K path -- leaves compact rows to scatter)
    WRows wr{live_rows + c0, real, Meff, L.dhdrop, H, false};
    UIC_TRY(wgrad_multi(side ? L.slab2 : L.slab, L.slab_bytes, dt, off(L.dlogits, (size_t)c0 * V1p, dt), rows, dv.logit_wT, H, V1p, &dc, 1, s, false, &wr));
    if (wr.used) return UIC_OK;
    return uic_scatter_rows_launch(L.dhc + (size_t)c0 * H, live_rows + c0, L.dhdrop, Meff, real, (size_t)H * 4, s);
  }
  const size_t r0 = (size_t)t0 * N;
  const int rows = (t1 - t0) * N;
  const WDest d1{(nlh() ? L.dlh : L.dhdrop) + r0 * H, H, 0, H};
  UIC_TRY(wgrad_multi(side ? L.slab2 : L.slab, L.slab_bytes, dt, off(L.dlogits, r0 * V1p, dt), rows, dv.logit_wT, H, V1p, &d1, 1, s));
  // back through the hidden blocks: Dropout(0.5) + ReLU mask, then d x = d pre W
  for (int l = nlh() - 1; l >= 0; --l) {
    UIC_TRY(uic_relu_mask_bwd_launch(dt, L.dlh + r0 * H, off(L.lh[l], r0 * H, dt), (training & 1) ? 2.f : 1.f,
                                     offw(L.dlh_pre[l], r0 * H, dt), (size_t)rows * H, s));
    UicGemmParams g = gemm_base(dt, rows, H);
    add_seg(g, off(L.dlh_pre[l], r0 * H, dt), H, dv.logit_h_wT[l], H, H);
    g.C = (l ? L.dlh : L.dhdrop) + r0 * H; g.ldc = H; g.flags = UIC_GEMM_OUT_F32;
    UIC_TRY(uic_gemm_launch(g, s));
  }
  return UIC_OK;
}
// d W_logit, d b_logit over all executed steps (own scratch buffers; beside the BPTT loop: the side stream's slab)
int Step::logit_weight_grads(hipStream_t s, UicWgPlace at) {
  float* const slab = at == UIC_WG_ALONE ? L.slab : L.slab2;
  if (compact) {
    const int K = live_pad();
    if (K == 0) {
      // (a batch without a single live position: no gradient; plain memsets -- V1 need not be a multiple of four)
      UIC_TRY(uic_check_hip(hipMemsetAsync(G->logit_w, 0, (size_t)V1 * H * 4, s), "hipMemsetAsync(d logit.weight)"));
      return uic_check_hip(hipMemsetAsync(G->logit_b, 0, (size_t)V1 * 4, s), "hipMemsetAsync(d logit.bias)");
    }
    const UicGemmTnSeg seg{L.hc, H, H};
    const WDest d1{G->logit_w, H, 0, H};
    UIC_TRY(wgrad_group(slab, L.dlogits, V1p, V1, &seg, 1, K, &d1, 1, s, false, L.tLA, L.tLB, at));
    return uic_colsum_launch(dt, L.dlogits, K, V1, V1p, G->logit_b, L.colscratchL, L.colscratch_floats, s);
  }
  {
    const UicGemmTnSeg seg{logit_in_all(), H, H};
    const WDest d1{G->logit_w, H, 0, H};
    UIC_TRY(wgrad_group(slab, L.dlogits, V1p, V1, &seg, 1, Meff, &d1, 1, s, false, L.tLA, L.tLB, at));
  }
  for (int l = 0; l < nlh(); ++l) {
    UIC_REQUIRE(G->logit_h_w[l] && G->logit_h_b[l], "backward: logit_layers=%d needs gradient tensors for hidden block %d", d.logit_layers, l);
    const UicGemmTnSeg seg{l ? L.lh[l - 1] : L.hdrop_all, H, H};
    const WDest d1{G->logit_h_w[l], H, 0, H};
    UIC_TRY(wgrad_group(slab, L.dlh_pre[l], H, H, &seg, 1, Meff, &d1, 1, s, false, L.tLA, L.tLB, at));
    UIC_TRY(uic_colsum_launch(dt, L.dlh_pre[l], Meff, H, H, G->logit_h_b[l], L.colscratchL, L.colscratch_floats, s));
  }
  return uic_colsum_launch(dt, L.dlogits, Meff, V1, V1p, G->logit_b, L.colscratchL, L.colscratch_floats, s);
}

// with_live (the fused step over a live-position list, whose BPTT is the launch chain): d hdrop is cleared in the same launch --
// the positions the list leaves out have gradient zero, the chunks scatter the others into it
int Step::bwd_begin(hipStream_t s, bool with_fwd_sync, bool with_live) {
  if (bias_in_chunks()) UIC_TRY(uic_fill_value_launch(dt, L.ones_blk, L.ones_rows * 128, 1.f, s));
  bwd_launches = 0;
  fwd_sync_clean = with_fwd_sync;
  if (with_live && bwd_persist_ok()) { UIC_TRY(live_begin(s)); with_live = false; }      // (no free slot below)
  void* p2 = bwd_persist_ok() ? (void*)L.rnn_bwd_sync : with_live ? (void*)L.dhdrop : nullptr;
  const size_t b2 = bwd_persist_ok() ? L.rnn_bwd_sync_bytes : with_live ? (size_t)Meff * H * 4 : 0;
  return uic_zero4_launch(L.dc_att, NH * 4, L.dc_lang, NH * 4, p2, b2,
                          with_fwd_sync ? L.rnn_sync : nullptr, with_fwd_sync ? uic_rnn_persist_sync_bytes() : 0, s);
}

// BPTT of decode steps [t_lo, t_hi), latest first: ONE persistent launch (rnn_bwd_persist.hip) when the shapes allow, else
// the chain of five launches per step.  The choice is constant within a step (bwd_persist_ok depends on dims only), and it has
// to be: with bptt_split() > 0 the chain carries d h between decode steps in the split-K slabs (bp_slab1 / bp_slab2), not in
// L.dx1 / columns [H, 3H) of dx2_all where the persistent kernel keeps it -- a chunk of one cannot hand over to the other.
int Step::bwd_steps(int t_lo, int t_hi, hipStream_t s) {
  if (!bwd_persist_ok()) {
    for (int t = t_hi - 1; t >= t_lo; --t) UIC_TRY(bwd_step(t, s));
    return UIC_OK;
  }
  UicRnnBwdParams p;
  memset(&p, 0, sizeof(p));
  p.N = N; p.R = R; p.t_lo = t_lo; p.t_hi = t_hi; p.first = t_hi == t_run;
  p.w2T = dv.w2T; p.w1recT = dv.w1recT; p.h2attT = dv.h2attT; p.w_alpha = w->alpha_w;
  p.p_att = L.patt; p.att = L.attp;
  p.gates1 = L.gates1; p.gates2 = L.gates2; p.c_att = L.c_att; p.c_lang = L.c_lang;
  p.att_h_all = L.atth_all; p.alpha_all = L.alpha_all; p.dhdrop = L.dhdrop;
  p.drop_p = drop_p; p.seed = seed;
  p.dg1_all = L.dg1_all; p.dg2_all = L.dg2_all; p.dx2_all = L.dx2_all; p.dx1 = L.dx1;
  p.dc_att = L.dc_att; p.dc_lang = L.dc_lang; p.de_all = L.de_all; p.datth_all = L.datth_all;
  UIC_REQUIRE(bwd_launches < d.T, "backward: more BPTT launches than decode steps");
  p.sync = L.rnn_bwd_sync + (size_t)bwd_launches * (uic_rnn_persist_sync_bytes() / 4);
  p.sync_zeroed = 1;                 // (bwd_begin zeroed every launch's block of this step)
  ++bwd_launches;
  p.force_safe = (d.recurrence & UIC_REC_SAFE) != 0; p.status = d.rnn_status;
  p.dbg = (d.recurrence & UIC_REC_STAMPS) ? L.rnn_bwd_dbg : nullptr; p.dbg_T = d.T;
  return uic_rnn_bwd_persist_launch(p, s);
}


int Step::bwd_step(int t, hipStream_t s) {
  const bool last = t == t_run - 1;
  const int S = bptt_split();
  float* dx2 = L.dx2_all + (size_t)t * N * 3 * H;
  const float* dx2_next = L.dx2_all + (size_t)(t + 1) * N * 3 * H;
  float* slab2 = L.bp_slab2[t & 1];
  const float* slab2_next = L.bp_slab2[(t + 1) & 1];
  const size_t st2 = (size_t)N * 3 * H, st1 = (size_t)N * 2 * H;
  const bool cm = compact_step(t);       // this step's d x GEMMs run over the unfinished rows only
  {
    UicLstmBwdParams p;
    memset(&p, 0, sizeof(p));
    p.dtype = dt; p.M = N; p.H = H;
    p.dh0 = L.dhdrop + t * NH; p.lddh0 = H;
    p.drop_p = drop_p; p.seed = seed; p.site = UIC_SITE_OUT0 + (unsigned)t;
    if (!last && S) {
      p.slabA = slab2_next + 2 * H; p.ldA = 3 * H; p.nA = S; p.strideA = st2;
      p.slabB = L.bp_slab1; p.ldB = 2 * H; p.nB = S; p.strideB = st1;
    } else if (!last) { p.dh1 = dx2_next + 2 * H; p.lddh1 = 3 * H; p.dh2 = L.dx1; p.lddh2 = 2 * H; }
    p.dc = L.dc_lang; p.gates = off(L.gates2, (size_t)t * N * H4, dt);
    p.c_prev = L.c_lang + t * NH; p.c = L.c_lang + (t + 1) * NH;
    p.dgates = offw(L.dg2_all, (size_t)t * N * H4, dt);
    if (rows_by_len) { p.row_len = L.cap_len; p.rank = L.row_rank; p.step = t; p.dgates_c = cm ? L.dg2c : nullptr; }
    UIC_TRY(uic_lstm_bwd_launch(p, s));
  }
  {  // d[att_res | h_att | h_lang_prev] = dG2 [W_ih | W_hh]
    UicGemmParams g = gemm_base(dt, cm ? unf[t] : N, 3 * H);
    add_seg(g, cm ? L.dg2c : off(L.dg2_all, (size_t)t * N * H4, dt), H4, dv.w2T, H4, H4);
    if (cm) { g.slab_row_map = L.row_order; g.slab_rows = N; ++compact_launches; }
    if (S) { g.slab = slab2; g.splitk = S; }
    else { g.C = dx2; g.ldc = 3 * H; g.flags = UIC_GEMM_OUT_F32; }
    UIC_TRY(uic_gemm_launch(g, s));
  }
  {
    UicAttnParams a;
    memset(&a, 0, sizeof(a));
    a.dtype = dt; a.N = N; a.R = R; a.A = A; a.H = H;
    a.att_h = L.atth_all + (size_t)t * N * A; a.p_att = L.patt; a.att = L.attp; a.w_alpha = w->alpha_w;
    a.alpha = L.alpha_all + (size_t)t * N * R;
    a.dctx = S ? slab2 : dx2; a.lddctx = 3 * H;
    if (S) { a.dctx_nslab = S; a.dctx_slab_stride = st2; a.dctx_sum = dx2; a.ld_dctx_sum = 3 * H; }
    a.de = L.de_all + (size_t)t * N * R;
    a.d_att_h = offw(L.datth_all, (size_t)t * N * A, dt);
    if (have_len) { a.row_len = L.cap_len; a.step = t; }
    UIC_TRY(uic_attention_bwd_step_launch(a, s));
  }
  UicH2attCellParams hc;
  memset(&hc, 0, sizeof(hc));
  if (S) {   // d h_att = d_att_h W_h2att + the d x2 / d x1 slices, then the att_lstm cell backward: one launch (bptt_fused.hip)
    hc.dtype = dt; hc.N = N; hc.H = H; hc.A = A;
    hc.datth = off(L.datth_all, (size_t)t * N * A, dt); hc.h2attT = dv.h2attT;
    hc.slabA = slab2 + H; hc.ldA = 3 * H; hc.nA = S; hc.strideA = st2;
    if (!last) { hc.slabB = L.bp_slab1 + H; hc.ldB = 2 * H; hc.nB = S; hc.strideB = st1; }
    hc.dc = L.dc_att; hc.gates = off(L.gates1, (size_t)t * N * H4, dt);
    hc.c_prev = L.c_att + t * NH; hc.c = L.c_att + (t + 1) * NH;
    hc.dgates = offw(L.dg1_all, (size_t)t * N * H4, dt);
    if (rows_by_len) { hc.row_len = L.cap_len; hc.rank = L.row_rank; hc.step = t; hc.dgates_c = cm && t > 0 ? L.dg1c : nullptr; }
  }
  const bool fused_cell = S && uic_h2att_cell_bwd_eligible(hc);
  UIC_REQUIRE(fused_cell || !rows_by_len, "bwd_step: rows by length need the fused h2att + cell backward kernel");
  if (fused_cell) {
    UIC_TRY(uic_h2att_cell_bwd_launch(hc, s));
  } else {
  {  // dh_att += d_att_h W_h2att
    UicGemmParams g = gemm_base(dt, N, H);
    add_seg(g, off(L.datth_all, (size_t)t * N * A, dt), A, dv.h2attT, A, A);
    g.C = dx2 + H; g.ldc = 3 * H; g.flags = UIC_GEMM_OUT_F32 | (S ? 0 : UIC_GEMM_ACCUM);   // (split: the d x2 share is added by the cell backward below)
    UIC_TRY(uic_gemm_launch(g, s));
  }
  {
    UicLstmBwdParams p;
    memset(&p, 0, sizeof(p));
    p.dtype = dt; p.M = N; p.H = H;
    p.dh0 = dx2 + H; p.lddh0 = 3 * H;
    if (S) {
      p.slabA = slab2 + H; p.ldA = 3 * H; p.nA = S; p.strideA = st2;
      if (!last) { p.slabB = L.bp_slab1 + H; p.ldB = 2 * H; p.nB = S; p.strideB = st1; }
    } else if (!last) { p.dh1 = L.dx1 + H; p.lddh1 = 2 * H; }
    p.dc = L.dc_att; p.gates = off(L.gates1, (size_t)t * N * H4, dt);
    p.c_prev = L.c_att + t * NH; p.c = L.c_att + (t + 1) * NH;
    p.dgates = offw(L.dg1_all, (size_t)t * N * H4, dt);
    UIC_TRY(uic_lstm_bwd_launch(p, s));
  }
  }
  if (t > 0) {  // d[h_lang_prev | h_att_prev] = dG1 [W_ih[:, :H] | W_hh]
    UicGemmParams g = gemm_base(dt, cm ? unf[t] : N, 2 * H);
    add_seg(g, cm ? L.dg1c : off(L.dg1_all, (size_t)t * N * H4, dt), H4, dv.w1recT, H4, H4);
    if (cm) { g.slab_row_map = L.row_order; g.slab_rows = N; ++compact_launches; }
    if (S) { g.slab = L.bp_slab1; g.splitk = S; }
    else { g.C = L.dx1; g.ldc = 2 * H; g.flags = UIC_GEMM_OUT_F32; }
    UIC_TRY(uic_gemm_launch(g, s));
  }
  return UIC_OK;
}

// weight gradients of everything except the logit layer, over all executed steps; split in two so that a
// data-parallel caller can start exchanging the early group (LSTMs, embedding, fc_embed; with the logit layer
// > 85 % of the bytes) while the late group (h2att, alpha_net, ctx2att, att_embed) is still being computed
int Step::bwd_epilogue(hipStream_t s) {
  UIC_TRY(bwd_epilogue_early(s, UIC_WG_ALONE));
  return bwd_epilogue_late(s, UIC_WG_ALONE);
}

// recurrent weight gradients (both LSTMs' weights and h2att) restricted to decode steps [t0, t1): one chunk of the
// stacked-row GEMMs, accumulated into G unless `first`.  Used by the fused step on the side stream, chunk by chunk
// behind the BPTT loop, so that only the last chunk's share is left when the loop ends.
// third: `s` is the third stream (the default order of the fused step: the side stream keeps the logit layer), which runs both
// shares with its two scratch sets; else `s` is the side stream
// sb (optional, the early-gradient order): the third stream for the att_lstm / h2att share, with its scratch (the GEMMs are
// independent)
int Step::wgrad_chunk(int t0, int t1, bool first, UicWgPlace at, hipStream_t s, bool third, hipStream_t sb) {
  float* const slabA = third ? L.slab3 : L.slab2;
  void* const tAA = third ? L.tTA : L.tSA;
  void* const tAB = third ? L.tTB : L.tSB;
  float* const slabB = third ? L.slab4 : sb ? L.slab3 : L.slab2;
  void* const tBA = third ? L.tUA : sb ? L.tTA : L.tSA;
  void* const tBB = third ? L.tUB : sb ? L.tTB : L.tSB;
  if (!sb) sb = s;
  const int rows = (t1 - t0) * N;
  const size_t r0 = (size_t)t0 * N;
  const void* ctx = off(L.ctx_all, r0 * H, dt);
  const void* h_att_new = off(L.h_att, NH + r0 * H, dt);
  const void* h_att_prev = off(L.h_att, r0 * H, dt);
  const void* h_lang_prev = off(L.h_lang, r0 * H, dt);
  // bias_in_chunks(): the bias gradients (column sums of dG) ride in the same GEMMs: one more "input" segment of ones whose first
  // column's weight gradient IS the column sum -- one more column tile per row tile instead of two column-sum passes in the
  // tail.  The segment and its destination are the last entries below: `nb` more of each.
  const int nb = bias_in_chunks() ? 1 : 0, nbh = nb && A % 128 == 0 ? 1 : 0;
  {  // lang_lstm: dG2^T x [att_res | h_att | h_lang_prev | ones]
    const UicGemmTnSeg segs[4] = {{ctx, H, H}, {h_att_new, H, H}, {h_lang_prev, H, H}, {L.ones_blk, 128, 128}};
    const WDest dd[3] = {{G->lang_lstm_w_ih, 2 * H, 0, 2 * H}, {G->lang_lstm_w_hh, H, 2 * H, H}, {G->lang_lstm_b_ih, 1, 3 * H, 1}};
    UIC_TRY(wgrad_group(slabA, off(L.dg2_all, r0 * H4, dt), H4, H4, segs, 3 + nb, rows, dd, 2 + nb, s, !first, tAA, tAB, at));
  }
  {  // h2att: d_att_h^T x [h_att | ones]
    const UicGemmTnSeg segs[2] = {{h_att_new, H, H}, {L.ones_blk, 128, 128}};
    const WDest dd[2] = {{G->h2att_w, H, 0, H}, {G->h2att_b, 1, H, 1}};
    UIC_TRY(wgrad_group(slabB, off(L.datth_all, r0 * A, dt), A, A, segs, 1 + nbh, rows, dd, 1 + nbh, sb, !first, tBA, tBB, at));
  }
  {  // att_lstm: dG1^T x [h_lang_prev | xt | h_att_prev | ones]
    const UicGemmTnSeg segs[4] = {{h_lang_prev, H, H}, {off(L.xt_all, r0 * E, dt), E, E}, {h_att_prev, H, H}, {L.ones_blk, 128, 128}};
    const WDest dd[4] = {{G->att_lstm_w_ih, ldih, 0, H}, {G->att_lstm_w_ih + 2 * H, ldih, H, E}, {G->att_lstm_w_hh, H, H + E, H},
                         {G->att_lstm_b_ih, 1, 2 * H + E, 1}};
    UIC_TRY(wgrad_group(slabB, off(L.dg1_all, r0 * H4, dt), H4, H4, segs, 3 + nb, rows, dd, 3 + nb, sb, !first, tBA, tBB, at));
  }
  return UIC_OK;
}

// chunked == true: wgrad_chunk already produced the LSTM / h2att weight gradients
// side == true: runs on the fused step's side stream with that stream's own scratch buffers
// The two big tensors of the early group, on their own so that the fused step can finish them FIRST after the BPTT loop
// (with gradient group 1, uic_topdown_grad_ready_wait):
//   fc_cols_grad: dGfc = sum_t dG1_t (left in L.dgfc) -> the fc' columns of att_lstm.weight_ih, which completes that matrix;
//   embed_grad(half): d xt = dG1 Wx of the decode steps of one half of the bucketed position list (embed_split; 0: all
//                     steps at once) -> their share of the embedding table.
int Step::fc_cols_grad(hipStream_t s, float* slab, void* tA, void* tB, UicWgPlace at) {
  UIC_TRY(uic_sum_steps_launch(dt, L.dg1_all, t_run, (size_t)N * H4, L.dgfc, s));
  const UicGemmTnSeg seg{L.fcp, H, H};
  const WDest d1{G->att_lstm_w_ih + H, ldih, 0, H};
  return wgrad_group(slab, L.dgfc, H4, H4, &seg, 1, N, &d1, 1, s, false, tA, tB, at);
}
int Step::embed_grad(int half, hipStream_t s) {
  const int t0 = embed_split && half ? embed_split : 0, t1 = embed_split && !half ? embed_split : t_run;
  const size_t r0 = (size_t)t0 * N;
  UicGemmParams g = gemm_base(dt, (t1 - t0) * N, E);
  add_seg(g, off(L.dg1_all, r0 * H4, dt), H4, dv.wxT, H4, H4);
  g.C = L.dxt + r0 * E; g.ldc = E; g.flags = UIC_GEMM_OUT_F32;
  UIC_TRY(uic_gemm_launch(g, s));
  if (!embed_prepared) {
    UIC_REQUIRE(!embed_split, "embed_grad: the position list was not prepared for split=%d", embed_split);
    UIC_TRY(uic_embed_bwd_sorted_prepare(embed_tokens(), embed_ldtok(), N, t_run, V1, E, G->embed_w, L.embed_scratch, s));
    embed_prepared = true;
  }
  return uic_embed_bwd_sorted_gather(dt, L.dxt, L.xt_all, embed_tokens(), embed_ldtok(), N, t_run, V1, E, drop_p, -1, G->embed_w,
                                     L.embed_scratch, s, embed_split, half);
}
// first_done == true: the caller already ran fc_cols_grad and embed_grad (the fused step, right behind the last chunk)
// bias_copies == false: the caller copies bias_ih -> bias_hh of the two cells itself (the fused step's default order: the
// chunks' gradients -- the bias columns among them -- come from ANOTHER stream and are joined after this call)
int Step::bias_hh_copies(hipStream_t s) {
  UIC_TRY(uic_copy_launch(G->lang_lstm_b_hh, G->lang_lstm_b_ih, (size_t)H4 * 4, s));
  return uic_copy_launch(G->att_lstm_b_hh, G->att_lstm_b_ih, (size_t)H4 * 4, s);
}
int Step::bwd_epilogue_early(hipStream_t s, UicWgPlace at, bool chunked, bool side, bool first_done, bool bias_copies) {
  void* const tA = side ? L.tSA : L.tA;
  void* const tB = side ? L.tSB : L.tB;
  float* const colscratch = side ? L.colscratchL : L.colscratch;
  float* const slab = side ? L.slab2 : L.slab;
  if (chunked && !(bias_in_chunks() && A % 128 == 0))   // h2att.bias belongs to the early group then (its weight came from wgrad_chunk)
    UIC_TRY(uic_colsum_launch(dt, L.datth_all, Meff, A, A, G->h2att_b, colscratch, L.colscratch_floats, s));
  // per LSTM ONE GEMM dG^T [4H, T*N] x [stacked inputs]^T; lang_lstm inputs [att_res | h_att | h_lang_prev]
  if (!chunked) {
    const UicGemmTnSeg segs[3] = {{L.ctx_all, H, H}, {off(L.h_att, NH, dt), H, H}, {L.h_lang, H, H}};
    const WDest dd[2] = {{G->lang_lstm_w_ih, 2 * H, 0, 2 * H}, {G->lang_lstm_w_hh, H, 2 * H, H}};
    UIC_TRY(wgrad_group(slab, L.dg2_all, H4, H4, segs, 3, Meff, dd, 2, s, false, tA, tB, at));
  }
  if (!(chunked && bias_in_chunks()))
    UIC_TRY(uic_colsum_launch(dt, L.dg2_all, Meff, H4, H4, G->lang_lstm_b_ih, colscratch, L.colscratch_floats, s));
  if (bias_copies) UIC_TRY(uic_copy_launch(G->lang_lstm_b_hh, G->lang_lstm_b_ih, (size_t)H4 * 4, s));
  // att_lstm inputs [h_lang_prev | xt | h_att_prev]  (the fc' columns are handled below from dGfc)
  if (!chunked) {
    const UicGemmTnSeg segs[3] = {{L.h_lang, H, H}, {L.xt_all, E, E}, {L.h_att, H, H}};
    const WDest dd[3] = {{G->att_lstm_w_ih, ldih, 0, H}, {G->att_lstm_w_ih + 2 * H, ldih, H, E}, {G->att_lstm_w_hh, H, H + E, H}};
    UIC_TRY(wgrad_group(slab, L.dg1_all, H4, H4, segs, 3, Meff, dd, 3, s, false, tA, tB, at));
  }
  if (!(chunked && bias_in_chunks()))
    UIC_TRY(uic_colsum_launch(dt, L.dg1_all, Meff, H4, H4, G->att_lstm_b_ih, colscratch, L.colscratch_floats, s));
  if (bias_copies) UIC_TRY(uic_copy_launch(G->att_lstm_b_hh, G->att_lstm_b_ih, (size_t)H4 * 4, s));
  if (!first_done) {
    UIC_TRY(fc_cols_grad(s, slab, tA, tB, at));
    UIC_TRY(embed_grad(0, s));
  }
  {  // d fc' from dGfc (left in L.dgfc by fc_cols_grad)
    UicGemmParams g = gemm_base(dt, N, H);
    add_seg(g, L.dgfc, H4, dv.wfcpT, H4, H4);
    g.C = L.dfcp; g.ldc = H; g.flags = UIC_GEMM_OUT_F32;
    UIC_TRY(uic_gemm_launch(g, s));
  }
  UIC_TRY(uic_relu_mask_bwd_launch(dt, L.dfcp, L.fcp, inv_keep, L.dfcpre, NH, s));
  {
    const UicGemmTnSeg seg{fc_in, Dfc, Dfc};
    const WDest d1{G->fc_w, Dfc, 0, Dfc};
    UIC_TRY(wgrad_group(slab, L.dfcpre, H, H, &seg, 1, N, &d1, 1, s, false, tA, tB, at));
  }
  UIC_TRY(uic_colsum_launch(dt, L.dfcpre, N, H, H, G->fc_b, colscratch, L.colscratch_floats, s));
  if (b->d_fc_feats) {   // optional: d fc_feats = d fc_pre W_fc, the S caption rows of an image summed (row i S + k of d fc_pre: lda = S H)
    const int S = d.seq_per_img > 1 ? d.seq_per_img : 1;
    UIC_TRY(uic_transpose_launch(dt, dv.fc_w, H, Dfc, Dfc, L.fcwT, H, s));
    for (int k = 0; k < S; ++k) {
      UicGemmParams g = gemm_base(dt, N / S, Dfc);
      add_seg(g, off(L.dfcpre, (size_t)k * H, dt), S * H, L.fcwT, H, H);
      g.C = b->d_fc_feats; g.ldc = Dfc; g.flags = UIC_GEMM_OUT_F32 | (k ? UIC_GEMM_ACCUM : 0);
      UIC_TRY(uic_gemm_launch(g, s));
    }
  }
  return UIC_OK;
}
// part: 0 = everything, 1 = only the deferred attention accumulation, 2 = everything else.  (Measured: running the
// accumulation -- whole-CU workgroups -- before releasing the side stream's tail is 3 % SLOWER than letting both run.)
int Step::bwd_epilogue_late(hipStream_t s, UicWgPlace at, bool chunked, int part) {
  // h2att
  if (!chunked && part != 1) {
    const UicGemmTnSeg seg{off(L.h_att, NH, dt), H, H};
    const WDest d1{G->h2att_w, H, 0, H};
    UIC_TRY(wgrad_group(L.slab, L.datth_all, A, A, &seg, 1, Meff, &d1, 1, s, false, L.tA, L.tB, at));
    UIC_TRY(uic_colsum_launch(dt, L.datth_all, Meff, A, A, G->h2att_b, L.colscratch, L.colscratch_floats, s));
  }
  if (part != 2) {  // attention: deferred accumulation over steps
    UicAttnAccumParams a;
    memset(&a, 0, sizeof(a));
    a.dtype = dt; a.N = N; a.R = R; a.A = A; a.H = H; a.T = t_run;
    a.att_h_all = L.atth_all; a.alpha_all = L.alpha_all; a.de_all = L.de_all;
    a.dctx_all = L.dx2_all; a.lddctx = 3 * H; a.dctx_step_stride = (size_t)N * 3 * H;
    a.p_att = L.patt; a.w_alpha = w->alpha_w;
    a.d_att = L.d_att; a.d_p_att = L.d_patt; a.d_walpha_part = L.dwalpha_part;
    if (have_len) a.row_len = L.cap_len;     // (steps behind a caption's end add zeros)
    UIC_TRY(uic_attention_bwd_accum_launch(a, s));
    UIC_TRY(uic_colsum_small_launch(L.dwalpha_part, N, A + 1, A, G->alpha_w, G->alpha_b, s));
  }
  if (part == 1) return UIC_OK;
  // ctx2att (bias gradient as the ones segment's first column where the TN path takes it, else a column-sum pass)
  const bool ones_ok = bias_in_chunks() && A % 128 == 0 && NR % 64 == 0;
  if (ones_ok) {
    const UicGemmTnSeg segs[2] = {{L.attp, H, H}, {L.ones_blk, 128, 128}};
    const WDest dd[2] = {{G->ctx2att_w, H, 0, H}, {G->ctx2att_b, 1, H, 1}};
    UIC_TRY(wgrad_group(L.slab, L.d_patt, A, A, segs, 2, NR, dd, 2, s, false, L.tA, L.tB, at));
  } else {
    const UicGemmTnSeg seg{L.attp, H, H};
    const WDest d1{G->ctx2att_w, H, 0, H};
    UIC_TRY(wgrad_group(L.slab, L.d_patt, A, A, &seg, 1, NR, &d1, 1, s, false, L.tA, L.tB, at));
    UIC_TRY(uic_colsum_launch(dt, L.d_patt, NR, A, A, G->ctx2att_b, L.colscratch, L.colscratch_floats, s));
  }
  // d att' = (the attention's own share, in L.d_att) + d p_att W_ctx2att; without BatchNorm behind it and with one feature row
  // per caption row, the backward of att_embed's ReLU + dropout rides on this GEMM's epilogue: it writes L.d_pre (the weight
  // gradient's bf16 operand) directly instead of the f32 sum that a separate pass then masks (53 us of the main stream's tail)
  bool relu_fused = false;
  {
    UicGemmParams g = gemm_base(dt, NR, H);
    add_seg(g, L.d_patt, A, dv.ctx2attT, A, A);
    g.C = L.d_pre; g.ldc = H; g.acc_src = L.d_att; g.ld_acc_src = H; g.mask_act = L.attp; g.ld_mask_act = H; g.mask_scale = inv_keep;
    relu_fused = d.use_bn != 2 && d.seq_per_img <= 1 && dt == UIC_BF16 && uic_gemm_pp_eligible(g);
    if (!relu_fused) {
      g.C = L.d_att; g.flags = UIC_GEMM_OUT_F32 | UIC_GEMM_ACCUM;
      g.acc_src = nullptr; g.mask_act = nullptr;
    }
    UIC_TRY(uic_gemm_launch(g, s));
  }
  // att_embed (padded regions have att' = 0 -> zero gradient, as pack_wrapper never touched them)
  const void* act = L.attp;
  if (d.use_bn == 2) {   // through BatchNorm1d(H): d_att <- d y (in place), grads of its affine parameters
    UIC_REQUIRE(G->att_bn4_w && G->att_bn4_b, "backward: use_bn=2 needs gradient tensors for att_embed.4");
    UIC_TRY(uic_bn_bwd_launch(dt, L.d_att, L.ybn, NR, R, H, b->att_masks ? (d.seq_per_img > 1 ? L.row_len_rep : L.row_len) : nullptr, L.bn_stat4, w->att_bn4_w,
                              training & 1, L.bn_part, L.bn_red, G->att_bn4_w, G->att_bn4_b, s));
    act = L.ybn;
  }
  // seq_per_img > 1 without BN: the S caption rows of an image share the Linear's input, so their gradients are summed
  // first and the weight-gradient GEMM runs over the per-image rows
  const bool fold = d.seq_per_img > 1;
  const int NRa = fold ? NR / d.seq_per_img : NR;
  if (fold)
    UIC_TRY(uic_relu_mask_bwd_fold_launch(dt, L.d_att, act, inv_keep, L.d_pre, N / d.seq_per_img, d.seq_per_img, (size_t)R * H, s));
  else if (!relu_fused)
    UIC_TRY(uic_relu_mask_bwd_launch(dt, L.d_att, act, inv_keep, L.d_pre, (size_t)NR * H, s));
  if (ones_ok && D % 128 == 0 && NRa % 64 == 0) {
    const UicGemmTnSeg segs[2] = {{att_in, D, D}, {L.ones_blk, 128, 128}};
    const WDest dd[2] = {{G->att_w, D, 0, D}, {G->att_b, 1, D, 1}};
    UIC_TRY(wgrad_group(L.slab, L.d_pre, H, H, segs, 2, NRa, dd, 2, s, false, L.tA, L.tB, at));
  } else {
    const UicGemmTnSeg seg{att_in, D, D};
    const WDest d1{G->att_w, D, 0, D};
    UIC_TRY(wgrad_group(L.slab, L.d_pre, H, H, &seg, 1, NRa, &d1, 1, s, false, L.tA, L.tB, at));
    UIC_TRY(uic_colsum_launch(dt, L.d_pre, NRa, H, H, G->att_b, L.colscratch, L.colscratch_floats, s));
  }
  if (b->d_att_feats) {  // optional: d att_feats = d_pre W_att  (one row per image region; d_pre is already folded over seq_per_img)
    UIC_TRY(uic_transpose_launch(dt, dv.att_w, H, D, D, L.attwT, H, s));
    UicGemmParams g = gemm_base(dt, NRa, D);
    add_seg(g, L.d_pre, H, L.attwT, H, H);
    g.C = b->d_att_feats; g.ldc = D; g.flags = UIC_GEMM_OUT_F32;
    UIC_TRY(uic_gemm_launch(g, s));
  }
  if (d.use_bn) {        // G->att_w holds dW' = d_pre^T xhat: unfold the BatchNorm1d(D) affine part (batchnorm.hip)
    UIC_REQUIRE(G->att_bn0_w && G->att_bn0_b, "backward: use_bn needs gradient tensors for att_embed.0");
    UIC_TRY(uic_bn_fold_grad_launch(w->att_w, w->att_bn0_w, w->att_bn0_b, G->att_w, G->att_b, H, D, G->att_bn0_w, G->att_bn0_b, s));
  }
  return UIC_OK;
}

}  // namespace topdown
