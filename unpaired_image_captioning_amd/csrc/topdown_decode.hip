// Decoding with the TopDown captioner: the decode step on the sampling buffers, greedy / multinomial sampling (also in the
// training layout, for the self-critical step), one get_logprobs_state, beam search, and the ensemble of several captioners.
// The sampling and beam bookkeeping (how a pass starts, the beam loop, the done-list export) is decode_internal.h's; this file
// supplies the decode step, the recurrent state's clearing and gathering, and -- for the ensemble -- the loop over members.
#include "topdown_internal.h"

namespace topdown {

// One decode step of AttModel.get_logprobs_state (:158-165) on the sampling buffers: embedding of L.smp.it, both LSTM cells,
// attention, logits into L.s_logits; recurrent state read from slot `cur`, written to slot `nxt`.
int decode_step(const uic_topdown_dims& d, const uic_topdown_weights* w, const Derived& dv, const uic_topdown_batch* b, const Layout& L,
                int cur, int nxt, int t, float drop_p, unsigned seed, hipStream_t s, bool train_mode, bool xt_ready) {
  const int dt = d.dtype;
  const int N = d.N, H = d.H, E = d.E, V1 = d.V1;
  const int V1p = (int)vpad(V1);
  // (xt_ready: the sampling kernel of the previous step already wrote this step's embedding rows into L.s_xt)
  if (!xt_ready) UIC_TRY(uic_embed_fwd_t_launch(dt, dv.embed_w, dt, V1, E, L.smp.it, 1, N, 1, drop_p, seed, UIC_SITE_EMBED, (size_t)t * N * E, 1, L.s_xt, s));
  UIC_TRY(uic_gemm_launch(att_lstm_gemm(d, w, dv, L, L.s_h_lang[cur], L.s_h_att[cur], L.s_c_att[cur], L.s_c_att[nxt], L.s_h_att[nxt], t,
                                        L.s_xt, false), s));
  UIC_TRY(attention_step(d, w, dv, b, L, L.s_h_att[nxt], L.s_atth, L.s_alpha, L.s_ctx, s));
  UIC_TRY(uic_gemm_launch(lang_lstm_gemm(d, w, dv, L, L.s_ctx, L.s_h_att[nxt], L.s_h_lang[cur], L.s_c_lang[cur], L.s_c_lang[nxt],
                                         L.s_h_lang[nxt], L.s_hdrop, t, drop_p, seed, false), s));
  const void* x = L.s_hdrop;
  for (int l = 0; l + 1 < d.logit_layers; ++l) {      // hidden logit blocks (AttModel.py:90-91), same masks as a training pass of step t
    UicGemmParams g = gemm_base(dt, N, H);
    add_seg(g, x, H, dv.logit_h_w[l], H, H);
    g.C = L.s_lh[l]; g.ldc = H; g.bias = w->logit_h_b[l]; g.flags = UIC_GEMM_RELU;
    if (train_mode) { g.drop_p = 0.5f; g.seed = seed; g.site = UIC_SITE_LOGIT_H0 + (unsigned)l; g.drop_row0 = t * N; }
    UIC_TRY(uic_gemm_launch(g, s));
    x = L.s_lh[l];
  }
  UicGemmParams g = gemm_base(dt, N, V1);
  add_seg(g, x, H, dv.logit_w, H, H);
  g.C = L.s_logits; g.ldc = V1p; g.bias = w->logit_b; g.flags = UIC_GEMM_OUT_F32;
  return uic_gemm_launch(g, s);
}

}  // namespace topdown

using namespace topdown;

namespace {

// zero recurrent state in slot 0 of the sampling buffers (AttModel.py:214-215, :187); the first input <bos> = 0 is sample_begin's,
// or the beam drivers' own fill
int decode_state_zero(const Layout& L, size_t NH, size_t S, hipStream_t s) {
  UIC_TRY(uic_fill_launch(L.s_h_att[0], 0, NH * S, s));
  UIC_TRY(uic_fill_launch(L.s_h_lang[0], 0, NH * S, s));
  UIC_TRY(uic_fill_launch(L.s_c_att[0], 0, NH * 4, s));
  return uic_fill_launch(L.s_c_lang[0], 0, NH * 4, s);
}
// the next step's embedding rows ride in the sampling kernel (one launch less per step)
void sample_embeds_next(UicSampleParams& p, const uic_topdown_dims& d, const Derived& dv, float drop_p, void* xt_out) {
  p.embed_table = dv.embed_w; p.embed_table_dtype = d.dtype; p.embed_V1 = d.V1; p.embed_E = d.E; p.embed_drop_p = drop_p; p.embed_site = UIC_SITE_EMBED;
  p.embed_idx_base = (size_t)(p.t + 1) * d.N * d.E; p.xt_out = xt_out;
}
// the search over L's sampling buffers: N = images x beam_size rows, step capacity T
int topdown_beam_begin(const uic_topdown_dims& d, const Layout& L, int Lsteps, int beam_size, int decoding_constraint, int max_ppl,
                        UicBeamParams& p, hipStream_t s) {
  return beam_begin(L.beam, L.s_logits, (int)vpad(d.V1), L.smp.it, d.N / beam_size, beam_size, d.T, d.V1, Lsteps, decoding_constraint, max_ppl, p, s);
}

}  // namespace

extern "C" {

int uic_topdown_sample(const uic_topdown_dims* d, const uic_topdown_weights* w, const void* derived,
                       const uic_topdown_batch* b, int32_t Lsteps, int32_t sample_max, float temperature,
                       int32_t decoding_constraint, uint32_t seed, const int64_t* forced, int32_t training,
                       void* workspace, int64_t* seq, float* seq_logp, void* stream) {
  UIC_TRY(check_dims(d));
  UIC_REQUIRE(w && derived && b && workspace && seq && seq_logp, "sample: null pointer");
  UIC_REQUIRE(b->fc_feats && b->att_feats, "sample: batch needs fc_feats and att_feats");
  UIC_REQUIRE(Lsteps >= 1 && Lsteps <= d->T, "sample: L=%d outside [1,%d]", Lsteps, d->T);
  UIC_REQUIRE(temperature > 0.f, "sample: temperature must be positive");
  hipStream_t s = (hipStream_t)stream;
  const Layout L = make_layout(*d, workspace);
  const Derived dv = make_derived(*d, w, (void*)derived);
  const int dt = d->dtype;
  const int N = d->N, H = d->H, V1 = d->V1;
  const size_t S = uic_dtype_size(dt);
  const size_t NH = (size_t)N * H;
  const void *fc_in, *att_in;
  const float drop_p = (training & 1) ? d->drop_p : 0.f;
  UIC_TRY(prepare_features(*d, w, dv, b, L, training, drop_p, seed, &fc_in, &att_in, s));
  UIC_TRY(wait_refresh(s));
  {
    Step st;
    st.init(d, w, derived, b, Lsteps, training, seed, workspace, nullptr);
    if (st.decode_persist_ok(sample_max, temperature, decoding_constraint)) {
      UIC_TRY(uic_zero4_launch(L.h_att, NH * S, L.h_lang, NH * S, L.c_att, NH * 4, L.c_lang, NH * 4, s));
      return st.decode_persist(Lsteps, sample_max, forced, false, seq, seq_logp, s);
    }
  }
  UIC_TRY(decode_state_zero(L, NH, S, s));
  UIC_TRY(sample_begin(L.smp, N, d->T, nullptr, nullptr, 0, s));
  for (int t = 0; t < Lsteps; ++t) {
    const int cur = t & 1, nxt = cur ^ 1;
    UIC_TRY(decode_step(*d, w, dv, b, L, cur, nxt, t, drop_p, seed, s, (training & 1) != 0, t > 0));
    UicSampleParams p = sample_params(L.smp, dt, N, V1, t, Lsteps, L.s_logits, sample_max, temperature, decoding_constraint, seed, forced, seq, seq_logp);
    if (t + 1 < Lsteps) sample_embeds_next(p, *d, dv, drop_p, L.s_xt);
    UIC_TRY(uic_sample_step_launch(p, s));
  }
  return UIC_OK;
}

// The multinomial / greedy pass in the TRAINING layout: the per-step chain of uic_topdown_forward with each step's input
// tokens drawn from the previous step's distribution, so that every activation the backward pass reads (gates, states,
// attention weights, contexts, dropped outputs, logits) is left in the workspace -- uic_topdown_xe_train_step with
// training bit 2 (value 4) then starts at the criterion instead of replaying the sampled captions teacher-forced.
int uic_topdown_sample_train(const uic_topdown_dims* d, const uic_topdown_weights* w, const void* derived,
                             const uic_topdown_batch* b, int32_t Lsteps, int32_t sample_max, float temperature,
                             int32_t decoding_constraint, uint32_t seed, const int64_t* forced, int32_t training,
                             void* workspace, int64_t* seq, float* seq_logp, void* stream) {
  UIC_TRY(check_dims(d));
  UIC_REQUIRE(w && derived && b && workspace && seq && seq_logp, "sample_train: null pointer");
  UIC_REQUIRE(b->fc_feats && b->att_feats, "sample_train: batch needs fc_feats and att_feats");
  UIC_REQUIRE(Lsteps >= 1 && Lsteps <= d->T, "sample_train: L=%d outside [1,%d]", Lsteps, d->T);
  UIC_REQUIRE(temperature > 0.f, "sample_train: temperature must be positive");
  UIC_REQUIRE(!(b->ss_prob > 0.f), "sample_train: the pass draws every token itself (ss_prob must be 0)");
  hipStream_t s = (hipStream_t)stream;
  Step st;
  st.init(d, w, derived, b, Lsteps, training, seed, workspace, nullptr);
  const Layout& L = st.L;
  const int N = d->N;
  const void *f, *a;
  UIC_TRY(prepare_features(st.d, w, st.dv, b, L, training, st.drop_p, seed, &f, &a, s));
  UIC_TRY(uic_zero4_launch(L.h_att, st.NH * st.S, L.h_lang, st.NH * st.S, L.c_att, st.NH * 4, L.c_lang, st.NH * 4, s));
  UIC_TRY(wait_refresh(s));
  if (st.decode_persist_ok(sample_max, temperature, decoding_constraint))
    return st.decode_persist(Lsteps, sample_max, forced, true, seq, seq_logp, s);
  UIC_TRY(sample_begin(L.smp, N, d->T, nullptr, nullptr, 0, s));   // <bos> = 0 (AttModel.py:214-215)
  for (int t = 0; t < Lsteps; ++t) {
    if (t == 0)   // (later steps: written by the previous step's sampling kernel)
      UIC_TRY(uic_embed_fwd_t_launch(st.dt, st.dv.embed_w, st.dt, st.V1, st.E, L.smp.it, 1, N, 1, st.drop_p, seed, UIC_SITE_EMBED,
                                   (size_t)t * N * st.E, 1, offw(L.xt_all, (size_t)t * N * st.E, st.dt), s));
    UIC_TRY(st.fwd_step(t, s, true));
    UIC_TRY(st.logits_rows_now(t, t + 1, s));
    UicSampleParams p = sample_params(L.smp, st.dt, N, st.V1, t, Lsteps, L.logits + (size_t)t * N * st.V1p, sample_max, temperature, decoding_constraint,
                                      seed, forced, seq, seq_logp);
    if (t + 1 < Lsteps) sample_embeds_next(p, st.d, st.dv, st.drop_p, offw(L.xt_all, (size_t)(t + 1) * N * st.E, st.dt));
    UIC_TRY(uic_sample_step_launch(p, s));
  }
  return UIC_OK;
}

int uic_topdown_logprobs_state(const uic_topdown_dims* d, const uic_topdown_weights* w, const void* derived, const int64_t* it,
                               const float* fc, const float* att, const float* p_att, const float* att_masks,
                               const float* h_in, const float* c_in, int32_t t, int32_t training, uint32_t seed, void* workspace,
                               float* logprobs, float* h_out, float* c_out, void* stream) {
  UIC_TRY(check_dims(d));
  UIC_REQUIRE(w && derived && it && fc && att && p_att && h_in && c_in && workspace && logprobs && h_out && c_out, "logprobs_state: null pointer");
  UIC_REQUIRE(d->seq_per_img <= 1, "logprobs_state: the prepared features are per caption row (seq_per_img must be 0 or 1)");
  UIC_REQUIRE(t >= 0, "logprobs_state: t=%d", t);
  hipStream_t s = (hipStream_t)stream;
  const Layout L = make_layout(*d, workspace);
  const Derived dv = make_derived(*d, w, (void*)derived);
  const int dt = d->dtype;
  const size_t N = d->N, R = d->R, H = d->H, A = d->A, V1 = d->V1;
  UIC_TRY(wait_refresh(s));
  // the caller's prepared features and state become the step's operands (operand dtype) ...
  UIC_TRY(uic_cast_f32_launch(dt, fc, L.fcp, N * H, s));
  UIC_TRY(uic_cast_f32_launch(dt, att, L.attp, N * R * H, s));
  UIC_TRY(uic_cast_f32_launch(dt, p_att, L.patt, N * R * A, s));
  UIC_TRY(uic_cast_f32_launch(dt, h_in, L.s_h_att[0], N * H, s));
  UIC_TRY(uic_cast_f32_launch(dt, h_in + N * H, L.s_h_lang[0], N * H, s));
  UIC_TRY(uic_copy_launch(L.s_c_att[0], c_in, N * H * 4, s));
  UIC_TRY(uic_copy_launch(L.s_c_lang[0], c_in + N * H, N * H * 4, s));
  UIC_TRY(uic_copy_launch(L.smp.it, it, N * 8, s));
  uic_topdown_batch b;
  memset(&b, 0, sizeof(b));
  b.att_masks = att_masks;
  const float drop_p = (training & 1) ? d->drop_p : 0.f;
  // ... one get_logprobs_state (P/models/AttModel.py:158-165) ...
  UIC_TRY(decode_step(*d, w, dv, &b, L, 0, 1, t, drop_p, seed, s, (training & 1) != 0));
  // ... and its results go back out: log_softmax of the logits, the new (h, c) stacks [att_lstm, lang_lstm]
  UicXeParams x;
  memset(&x, 0, sizeof(x));
  x.dtype = dt; x.M = (int)N; x.V1 = (int)V1; x.ldv = (int)vpad(V1); x.N = (int)N;
  x.logits = L.s_logits; x.logprobs = logprobs; x.lp_step_stride = V1; x.lp_row_stride = V1;
  UIC_TRY(uic_xe_launch(x, s));
  UIC_TRY(uic_to_f32_launch(dt, L.s_h_att[1], h_out, N * H, s));
  UIC_TRY(uic_to_f32_launch(dt, L.s_h_lang[1], h_out + N * H, N * H, s));
  UIC_TRY(uic_copy_launch(c_out, L.s_c_att[1], N * H * 4, s));
  UIC_TRY(uic_copy_launch(c_out + N * H, L.s_c_lang[1], N * H * 4, s));
  return UIC_OK;
}

int uic_topdown_beam_done_lists(const uic_topdown_dims* d, void* workspace, int32_t Lsteps, int32_t beam_size, int32_t* done_count,
                                float* done_p, int64_t* done_seq, float* done_lp, void* stream) {
  UIC_TRY(check_dims(d));
  UIC_REQUIRE(workspace && done_count && done_p && done_seq && done_lp, "beam_done_lists: null pointer");
  UIC_REQUIRE(beam_size >= 1 && d->N % beam_size == 0 && Lsteps >= 1 && Lsteps <= d->T, "beam_done_lists: bad sizes");
  hipStream_t s = (hipStream_t)stream;
  const Layout L = make_layout(*d, workspace);
  return beam_done_lists(L.beam, (size_t)d->N / beam_size, Lsteps, beam_size, done_count, done_p, done_seq, done_lp, s);
}

int uic_topdown_sample_beam(const uic_topdown_dims* d, const uic_topdown_weights* w, const void* derived,
                            const uic_topdown_batch* b, int32_t Lsteps, int32_t beam_size, int32_t decoding_constraint,
                            int32_t max_ppl, void* workspace, int64_t* seq, float* seq_logp, void* stream) {
  UIC_TRY(check_dims(d));
  UIC_REQUIRE(w && derived && b && workspace && seq && seq_logp, "sample_beam: null pointer");
  UIC_REQUIRE(b->fc_feats && b->att_feats, "sample_beam: batch needs fc_feats and att_feats");
  UIC_REQUIRE(Lsteps >= 1 && Lsteps <= d->T, "sample_beam: L=%d outside [1,%d]", Lsteps, d->T);
  UIC_REQUIRE(beam_size >= 1 && beam_size <= UIC_BEAM_MAX && beam_size <= d->V1, "sample_beam: beam_size=%d outside [1, %d]", beam_size, UIC_BEAM_MAX);
  UIC_REQUIRE(d->N % beam_size == 0, "sample_beam: N=%d rows must be images x beam_size=%d (every image replicated beam_size times)", d->N, beam_size);
  hipStream_t s = (hipStream_t)stream;
  const Layout L = make_layout(*d, workspace);
  const Derived dv = make_derived(*d, w, (void*)derived);
  const int dt = d->dtype;
  const int N = d->N, H = d->H;
  const size_t S = uic_dtype_size(dt), NH = (size_t)N * H;
  const void *fc_in, *att_in;
  UIC_TRY(prepare_features(*d, w, dv, b, L, 0, 0.f, 0, &fc_in, &att_in, s));      // eval mode, like eval_utils.eval_split
  UIC_TRY(wait_refresh(s));
  UIC_TRY(decode_state_zero(L, NH, S, s));
  UIC_TRY(uic_fill_launch(L.smp.it, 0, (size_t)N * 8, s));     // <bos> for every beam row
  UicBeamParams p;
  UIC_TRY(topdown_beam_begin(*d, L, Lsteps, beam_size, decoding_constraint, max_ppl, p, s));
  UIC_TRY(decode_step(*d, w, dv, b, L, 0, 1, 0, 0.f, 0, s));   // logprobs after <bos> (AttModel.py:184-190)
  auto advance = [&](int t_next) -> int {
    UIC_TRY(uic_beam_gather_launch(dt, p.parent, N, beam_size, H, L.s_h_att[1], L.s_h_att[0], L.s_h_lang[1], L.s_h_lang[0],
                                   L.s_c_att[1], L.s_c_att[0], L.s_c_lang[1], L.s_c_lang[0], s));
    return decode_step(*d, w, dv, b, L, 0, 1, t_next, 0.f, 0, s);
  };
  return beam_search(p, Lsteps, advance, s, seq, seq_logp);
}

}  // extern "C"

// ---------------------------------------------------------------- ensemble of M captioners (P/models/AttEnsemble.py)
// Every member keeps its own dims / weights / derived copies / workspace and runs the decode step of the single-model chain on
// the caller's stream; ensemble_logmean_kernel (ensemble.hip) then folds the M rows of step logits into member 0's, and the
// single model's sampling / beam kernels go on from there as if member 0 had produced them.  The chosen token needs no copy:
// every member's embedding lookup reads member 0's token buffer.
namespace {

// L is make_layout() of the member's own workspace with ONE field patched: L.smp.it of every member is member 0's.  decode_step
// reads the input token from L.smp.it only (its embedding lookup; the ensemble path never passes xt_ready), and the sampling / beam
// kernels write it to member 0's: the members' own token buffers stay unused, and nothing else of a Layout may be shared.
struct Member {
  const uic_topdown_dims* d; const uic_topdown_weights* w; const uic_topdown_batch* b;
  Derived dv; Layout L;
};

int ensemble_members(const char* what, int M, const uic_topdown_dims* const* d, const uic_topdown_weights* const* w, const void* const* derived,
                     const uic_topdown_batch* const* b, void* const* workspace, int Lsteps, Member* mem) {
  UIC_REQUIRE(M >= 1 && M <= UIC_ENSEMBLE_MAX, "%s: %d members outside [1, %d]", what, M, UIC_ENSEMBLE_MAX);
  UIC_REQUIRE(d && w && derived && b && workspace, "%s: null pointer", what);
  for (int m = 0; m < M; ++m) {
    UIC_REQUIRE(d[m] && w[m] && derived[m] && b[m] && workspace[m], "%s: null pointer (member %d)", what, m);
    UIC_TRY(check_dims(d[m]));
    UIC_REQUIRE(b[m]->fc_feats && b[m]->att_feats, "%s: member %d's batch needs fc_feats and att_feats", what, m);
    UIC_REQUIRE(d[m]->N == d[0]->N && d[m]->V1 == d[0]->V1 && d[m]->R == d[0]->R && d[m]->T == d[0]->T,
                "%s: member %d has N=%d V1=%d R=%d T=%d, member 0 N=%d V1=%d R=%d T=%d (the members must share rows, vocabulary, regions and length)",
                what, m, d[m]->N, d[m]->V1, d[m]->R, d[m]->T, d[0]->N, d[0]->V1, d[0]->R, d[0]->T);
    UIC_REQUIRE((d[m]->seq_per_img > 1 ? d[m]->seq_per_img : 1) == (d[0]->seq_per_img > 1 ? d[0]->seq_per_img : 1),
                "%s: member %d replicates every image %d times, member 0 %d times", what, m, d[m]->seq_per_img, d[0]->seq_per_img);
    for (int k = 0; k < m; ++k)
      UIC_REQUIRE(workspace[k] != workspace[m], "%s: members %d and %d share a workspace", what, k, m);
  }
  UIC_REQUIRE(Lsteps >= 1 && Lsteps <= d[0]->T, "%s: L=%d outside [1,%d]", what, Lsteps, d[0]->T);
  for (int m = 0; m < M; ++m) {
    mem[m].d = d[m]; mem[m].w = w[m]; mem[m].b = b[m];
    mem[m].L = make_layout(*d[m], workspace[m]);
    mem[m].dv = make_derived(*d[m], w[m], (void*)derived[m]);
    mem[m].L.smp.it = mem[0].L.smp.it;
  }
  return UIC_OK;
}

// eval-mode features and the zero initial state of every member
int ensemble_begin(int M, Member* mem, hipStream_t s) {
  for (int m = 0; m < M; ++m) {
    const void *fc_in, *att_in;
    UIC_TRY(prepare_features(*mem[m].d, mem[m].w, mem[m].dv, mem[m].b, mem[m].L, 0, 0.f, 0, &fc_in, &att_in, s));
  }
  UIC_TRY(wait_refresh(s));      // (one side stream made every member's copies, in order: its last event covers them all)
  for (int m = 0; m < M; ++m) {
    const Layout& L = mem[m].L;
    const size_t NH = (size_t)mem[m].d->N * mem[m].d->H, S = uic_dtype_size(mem[m].d->dtype);
    UIC_TRY(uic_zero4_launch(L.s_h_att[0], NH * S, L.s_h_lang[0], NH * S, L.s_c_att[0], NH * 4, L.s_c_lang[0], NH * 4, s));
  }
  return UIC_OK;
}

// one get_logprobs_state of the ensemble (AttEnsemble.py:48-55): states slot `cur` -> `nxt`, combined log-probs into member 0's s_logits
int ensemble_step(int M, const Member* mem, int cur, int nxt, int t, hipStream_t s) {
  UicEnsembleParams e;
  memset(&e, 0, sizeof(e));
  e.M = M; e.N = mem[0].d->N; e.V1 = mem[0].d->V1;
  for (int m = 0; m < M; ++m) {
    UIC_TRY(decode_step(*mem[m].d, mem[m].w, mem[m].dv, mem[m].b, mem[m].L, cur, nxt, t, 0.f, 0, s));
    e.x[m] = mem[m].L.s_logits; e.ld[m] = (int)vpad(e.V1);
  }
  e.out = mem[0].L.s_logits; e.ld_out = (int)vpad(e.V1);
  return uic_ensemble_logmean_launch(e, s);
}

}  // namespace

extern "C" {

int uic_topdown_ensemble_sample(int32_t M, const uic_topdown_dims* const* d, const uic_topdown_weights* const* w, const void* const* derived,
                                const uic_topdown_batch* const* b, int32_t Lsteps, int32_t sample_max, float temperature,
                                int32_t decoding_constraint, uint32_t seed, const int64_t* forced, void* const* workspace,
                                int64_t* seq, float* seq_logp, void* stream) {
  Member mem[UIC_ENSEMBLE_MAX];
  UIC_TRY(ensemble_members("ensemble_sample", M, d, w, derived, b, workspace, Lsteps, mem));
  UIC_REQUIRE(seq && seq_logp, "ensemble_sample: null pointer");
  UIC_REQUIRE(temperature > 0.f, "ensemble_sample: temperature must be positive");
  hipStream_t s = (hipStream_t)stream;
  const Layout& L0 = mem[0].L;
  const int N = d[0]->N, V1 = d[0]->V1;
  bool all_bf16 = true;
  for (int m = 0; m < M; ++m) all_bf16 = all_bf16 && d[m]->dtype == UIC_BF16;
  UIC_TRY(ensemble_begin(M, mem, s));
  UIC_TRY(sample_begin(L0.smp, N, d[0]->T, nullptr, nullptr, 0, s));
  for (int t = 0; t < Lsteps; ++t) {
    const int cur = t & 1, nxt = cur ^ 1;
    UIC_TRY(ensemble_step(M, mem, cur, nxt, t, s));
    // (the hardware exponential of the bf16 sampling kernel only when no member is an f32 parity model)
    const UicSampleParams p = sample_params(L0.smp, all_bf16 ? UIC_BF16 : UIC_F32, N, V1, t, Lsteps, L0.s_logits, sample_max, temperature,
                                            decoding_constraint, seed, forced, seq, seq_logp);
    UIC_TRY(uic_sample_step_launch(p, s));
  }
  return UIC_OK;
}

int uic_topdown_ensemble_sample_beam(int32_t M, const uic_topdown_dims* const* d, const uic_topdown_weights* const* w,
                                     const void* const* derived, const uic_topdown_batch* const* b, int32_t Lsteps, int32_t beam_size,
                                     int32_t decoding_constraint, int32_t max_ppl, void* const* workspace, int64_t* seq,
                                     float* seq_logp, void* stream) {
  Member mem[UIC_ENSEMBLE_MAX];
  UIC_TRY(ensemble_members("ensemble_sample_beam", M, d, w, derived, b, workspace, Lsteps, mem));
  UIC_REQUIRE(seq && seq_logp, "ensemble_sample_beam: null pointer");
  UIC_REQUIRE(beam_size >= 1 && beam_size <= UIC_BEAM_MAX && beam_size <= d[0]->V1, "ensemble_sample_beam: beam_size=%d outside [1, %d]", beam_size, UIC_BEAM_MAX);
  UIC_REQUIRE(d[0]->N % beam_size == 0, "ensemble_sample_beam: N=%d rows must be images x beam_size=%d (every image replicated beam_size times)", d[0]->N, beam_size);
  hipStream_t s = (hipStream_t)stream;
  const Layout& L0 = mem[0].L;
  const int N = d[0]->N;
  UIC_TRY(ensemble_begin(M, mem, s));
  UIC_TRY(uic_fill_launch(L0.smp.it, 0, (size_t)N * 8, s));    // <bos> for every beam row
  UicBeamParams p;
  UIC_TRY(topdown_beam_begin(*d[0], L0, Lsteps, beam_size, decoding_constraint, max_ppl, p, s));
  UIC_TRY(ensemble_step(M, mem, 0, 1, 0, s));                  // logprobs after <bos> (AttEnsemble.py:88-89)
  auto advance = [&](int t_next) -> int {
    for (int m = 0; m < M; ++m) {                              // every member's states follow the surviving parents
      const Layout& L = mem[m].L;
      UIC_TRY(uic_beam_gather_launch(d[m]->dtype, p.parent, N, beam_size, d[m]->H, L.s_h_att[1], L.s_h_att[0], L.s_h_lang[1], L.s_h_lang[0],
                                     L.s_c_att[1], L.s_c_att[0], L.s_c_lang[1], L.s_c_lang[0], s));
    }
    return ensemble_step(M, mem, 0, 1, t_next, s);
  };
  return beam_search(p, Lsteps, advance, s, seq, seq_logp);
}

}  // extern "C"
