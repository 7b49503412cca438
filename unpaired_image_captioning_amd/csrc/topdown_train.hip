// Host-side sequencing of the TopDown captioner step on one MI355X: every launch of
// AttModel._forward / _sample, LanguageModelCriterion and their backward, enqueued on the
// caller's HIP stream with no host synchronisation.  (The fused training step also forks onto two library-owned side streams
// and joins them before returning.  Capturing it into a hipGraph is NOT supported: with every stream joined the capture itself
// goes through, but hipStreamEndCapture crashes inside the ROCm 7.2 runtime -- tools/graph_capture_probe.py; an un-joined stream
// is reported properly as hipErrorStreamCaptureUnjoined.  The step is GPU-bound with the host 2.5 ms ahead, so a graph would not
// shorten it.)
//
// Restructuring relative to the reference's per-step Python loop (P/models/AttModel.py:119-165):
//   * teacher forcing makes xt_t and fc' known up front, so their share of the att_lstm gate
//     GEMM is batched over all T steps (Gx, Gfc); only K = 2H stays in the recurrence;
//   * the logit GEMM, log_softmax and the criterion run once over all T*N rows, never
//     materialising [N,T,V1] log-probs unless the caller asks for them;
//   * in backward only dX GEMMs and the attention step stay in the BPTT loop; every weight
//     gradient is one GEMM over the T*N stacked rows afterwards, and the attention's [N,R,*]
//     gradients are produced by one deferred pass (attention.hip).
#include "topdown_internal.h"

using namespace topdown;

extern "C" {

int uic_topdown_forward(const uic_topdown_dims* d, const uic_topdown_weights* w, const void* derived,
                        const uic_topdown_batch* b, int32_t t_run, int32_t training, uint32_t seed,
                        void* workspace, float* logprobs_out, void* stream) {
  UIC_TRY(check_dims(d));
  UIC_REQUIRE(w && derived && b && workspace, "forward: null pointer");
  UIC_REQUIRE(b->fc_feats && b->att_feats && b->labels, "forward: batch needs fc_feats, att_feats and labels");
  UIC_REQUIRE(t_run >= 1 && t_run <= d->T, "forward: t_run=%d outside [1,%d]", t_run, d->T);
  UIC_REQUIRE(b->ld_labels >= t_run, "forward: labels have %d columns, need %d", b->ld_labels, t_run);
  hipStream_t s = (hipStream_t)stream;
  Step st;
  st.init(d, w, derived, b, t_run, training, seed, workspace, nullptr);
  UIC_TRY(wait_refresh(s));                           // (the embedding table's operand copy is made on the side stream)
  UIC_TRY(st.fwd_prologue(s));
  UIC_TRY(st.fwd_steps(0, t_run, s));
  UIC_TRY(st.logits_rows(0, t_run, s));
  if (logprobs_out) UIC_TRY(st.xe_rows(0, t_run, nullptr, logprobs_out, 0, s));
  return UIC_OK;
}

int uic_topdown_xe_loss(const uic_topdown_dims* d, const uic_topdown_batch* b, int32_t t_run, void* workspace,
                        const float* inv_den, float* loss_out, float* den_out, void* stream) {
  UIC_TRY(check_dims(d));
  UIC_REQUIRE(b && workspace && b->labels && b->masks && loss_out, "xe_loss: null pointer");
  UIC_REQUIRE(t_run >= 1 && t_run <= d->T, "xe_loss: t_run=%d outside [1,%d]", t_run, d->T);
  UIC_REQUIRE(b->ld_labels >= d->T + 1 && b->ld_masks >= d->T + 1, "xe_loss: labels/masks need %d columns", d->T + 1);
  hipStream_t s = (hipStream_t)stream;
  uic_topdown_weights none;
  memset(&none, 0, sizeof(none));
  Step st;
  st.init(d, &none, nullptr, b, t_run, 0, 0, workspace, nullptr);
  // denominator: sum of masks[:, 1:T+1] over ALL T columns (criterion.py:146-149), also after an early break
  UIC_TRY(uic_masked_sum_launch(b->masks, b->ld_masks, 1, d->N, d->T, st.L.scalars, st.L.scalars + 1, s));
  const float* inv = inv_den ? inv_den : st.L.scalars + 1;
  UIC_TRY(st.xe_rows(0, t_run, inv, nullptr, 1, s));
  UIC_TRY(uic_reduce_sum_launch(st.L.row_loss, (size_t)t_run * d->N, inv, loss_out, s));
  if (den_out) UIC_TRY(uic_copy_launch(den_out, st.L.scalars, 4, s));
  return UIC_OK;
}

int uic_topdown_backward(const uic_topdown_dims* d, const uic_topdown_weights* w, const void* derived,
                         const uic_topdown_batch* b, int32_t t_run, int32_t training, uint32_t seed,
                         void* workspace, const float* dlogprobs, const float* logprobs,
                         const uic_topdown_weights* G, void* stream) {
  UIC_TRY(check_dims(d));
  UIC_REQUIRE(w && derived && b && workspace && G, "backward: null pointer");
  UIC_REQUIRE(t_run >= 1 && t_run <= d->T, "backward: t_run=%d outside [1,%d]", t_run, d->T);
  UIC_REQUIRE(!dlogprobs || logprobs, "backward: dlogprobs needs the forward log-probs");
  UIC_REQUIRE(!b->d_att_feats || !d->use_bn, "backward: d_att_feats is not available through att_embed's BatchNorm (use_bn=%d)", d->use_bn);
  hipStream_t s = (hipStream_t)stream;
  Step st;
  st.init(d, w, derived, b, t_run, training, seed, workspace, G);
  UIC_TRY(wait_refresh(s));
  if (dlogprobs)
    UIC_TRY(uic_logsoftmax_bwd_launch(st.dt, st.L.dlogits, st.Meff, st.V1, st.V1p, st.N, dlogprobs, (size_t)st.V1,
                                      (size_t)d->T * st.V1, logprobs, s));
  UIC_TRY(st.dh_rows(0, t_run, s));
  UIC_TRY(st.logit_weight_grads(s, UIC_WG_ALONE));
  UIC_TRY(st.bwd_begin(s));
  UIC_TRY(st.bwd_steps(0, t_run, s));
  return st.bwd_epilogue(s);
}

int uic_topdown_xe_train_step(const uic_topdown_dims* d, const uic_topdown_weights* w, const void* derived,
                              const uic_topdown_batch* b, int32_t t_run, int32_t training, uint32_t seed,
                              void* workspace, const float* inv_den, float* loss_out, float* den_out,
                              const uic_topdown_weights* G, void* stream) {
  UIC_TRY(check_dims(d));
  UIC_REQUIRE(w && derived && b && workspace && G && loss_out, "xe_train_step: null pointer");
  UIC_REQUIRE(b->fc_feats && b->att_feats && b->labels && (b->masks || b->grad_scale), "xe_train_step: batch needs features, labels and masks (or grad_scale)");
  UIC_REQUIRE(t_run >= 1 && t_run <= d->T, "xe_train_step: t_run=%d outside [1,%d]", t_run, d->T);
  UIC_REQUIRE(b->ld_labels >= d->T + 1 && (!b->masks || b->ld_masks >= d->T + 1), "xe_train_step: labels/masks need %d columns", d->T + 1);
  UIC_REQUIRE(!b->grad_scale || b->ld_grad_scale >= t_run, "xe_train_step: grad_scale needs %d columns", t_run);
  UIC_REQUIRE(!b->d_att_feats || !d->use_bn, "xe_train_step: d_att_feats is not available through att_embed's BatchNorm (use_bn=%d)", d->use_bn);
  hipStream_t s = (hipStream_t)stream;
  SideStream* ss = nullptr;
  UIC_TRY(get_side(&ss));
  hipStream_t s2 = ss->stream;
  hipStream_t s3 = ss->stream3;
  Step st;
  st.init(d, w, derived, b, t_run, training, seed, workspace, G);
  // The fused step's BPTT is always the launch chain: the persistent BPTT kernel holds every CU, which serialises the side
  // stream's GEMMs behind it (measured 3.81 vs 3.48 ms, profiles/r03_v4_rnn_bwd_probe.txt); UIC_REC_BWD_PERSIST selects it for
  // the single-stream uic_topdown_backward call only, where nothing runs beside it.
  st.d.recurrence &= ~UIC_REC_BWD_PERSIST;
  st.init_live();
  st.init_rows_by_len();
  const bool early = st.early_grads();
  ss->embed_recorded = false;
  // UIC_REC_COMM_STREAM: a communication stream of the caller is busy beside this step (data parallel).  The chip dispatches
  // from THREE busy hardware queues at full speed; a fourth non-empty queue -- even one wave that only waits -- makes the BPTT
  // loop's 85 dependent launches 1.5-2.5x slower (tools/queue_probe.py, profiles/r05_*_queue_probe.txt).  So with the caller's
  // queue counted the step keeps to two of its own while the loop runs: the chunks' weight gradients go back to the side stream,
  // behind the logit layer (round 4's order), instead of stream 3.
  const bool comm = (d->recurrence & UIC_REC_COMM_STREAM) != 0;
  const int CH = WG_CHUNK;                            // decode steps per hand-off to the side stream
  // chunk c = decode steps [cb[c], cb[c + 1]): chunks of CH from step 0 (the last one -- the one the BPTT loop starts from -- is
  // t_run % CH steps long: ONE at the reference's 17 steps)
  int cb[MAX_CHUNKS + 1];
  int nchunk = 0;
  {
    UIC_REQUIRE((t_run + CH - 1) / CH + 2 <= MAX_CHUNKS, "xe_train_step: too many decode steps (%d)", t_run);
    cb[0] = 0;
    for (int t = 0; t < t_run;) {
      t += CH < t_run - t ? CH : t_run - t;
      cb[++nchunk] = t;
    }
  }
#define UIC_HIP(expr) UIC_TRY(uic_check_hip((expr), #expr))
#define UIC_MARK(i, strm) do { if (ss->marks_on) UIC_HIP(hipEventRecord(ss->mark[i], strm)); } while (0)

  UIC_MARK(0, s);
  // main: features, recurrence; hands each finished chunk of steps to the side stream.  ev_den: the step has begun (whatever
  // the caller enqueued on `s` before it is done) -- the side streams start from there.
  const float* inv = inv_den ? inv_den : st.L.scalars + 1;
  UIC_HIP(hipEventRecord(ss->ev_den, s));
  UIC_HIP(hipStreamWaitEvent(s2, ss->ev_den, 0));
  // side: the loss denominator (the criterion's first use of it is on this stream, after the recurrence).  First on its stream:
  // behind the branch below it would be dispatched beside the persistent recurrence and wait for a CU until that ends.
  // (A resumed step has no prologue after which the main stream waits for the side stream, and the loop's first logit chunk --
  // its criterion reads the denominator -- runs on the main stream: there the denominator is made on the main stream.)
  if (b->masks) UIC_TRY(uic_masked_sum_launch(b->masks, b->ld_masks, 1, d->N, d->T, st.L.scalars, st.L.scalars + 1,
                                              (training & 4) ? s : s2));
  // (the live list, when the caller left it to the library: on the side stream ahead of its prologue branch, whose event the main
  // stream waits for before the recurrence -- every logit chunk on either stream is ordered behind it)
  // (the whole recurrence as one launch of the weight-stationary kernel: it fills the compact operand itself)
  st.fused_gather = st.compact && st.build_live && !(training & 4) && st.persist_ok() && st.dt == UIC_BF16;
  if (st.compact && st.build_live) UIC_TRY(st.live_build((training & 4) ? s : s2));
  else if (b->grad_scale) UIC_TRY(st.len_build((training & 4) ? s : s2));
  // (not for a plain masked step without counts: it stays bit-equal to the three separate API calls, whose backward pass sums over
  // every step -- tests/test_gpu_topdown.py)
  st.have_len = (st.compact && st.build_live) || b->grad_scale;
  // the prologue's two independent branches side by side: att_embed + ctx2att here, fc_embed + embedding + the batched
  // input GEMM on the side stream (idle until the recurrence is through; its part of the weight refresh comes first there)
  // training bit 2: the workspace already holds this forward pass (uic_topdown_sample_train drew b->labels with these
  // weights, this seed and these dims): the step starts at the criterion
  const bool resume = (training & 4) != 0;
  bool bwd_begun = false, live_begun = false;
  UIC_REQUIRE(!resume || !st.ss_on(), "xe_train_step: a resumed step cannot use scheduled sampling");
  if (!resume) {
    // three branches: att_embed + ctx2att (main), embedding + batched input GEMM (side), fc_embed + Gfc + initial state (third
    // stream: two small latency-bound GEMMs that would otherwise sit behind the batched input GEMM on the side stream)
    // Enqueued longest branch first: the host has just come back from the previous step's loss read, so the GPU starts with an
    // empty queue and every launch ahead of att_embed's GEMM is ~5 us of its idle time.
    const bool split3 = st.gfc_separate() && !st.ss_on();
    UIC_TRY(st.fwd_prologue(s, 2));
    UIC_TRY(st.fwd_prologue(s2, split3 ? 3 : 1));
    if (!split3) UIC_TRY(flush_gathered_late(ss, s2));
    UIC_HIP(hipEventRecord(ss->ev_pro, s2));
    if (split3) {
      UIC_HIP(hipStreamWaitEvent(s3, ss->ev_den, 0));
      if (ss->g2_recorded) UIC_HIP(hipStreamWaitEvent(s3, ss->ev_g2, 0));   // (gathered refresh: fc_embed's operand copy was made on the side stream)
      UIC_TRY(st.fwd_prologue(s3, 4));
      // (the BPTT loop's zeroed carries and ones block -- nothing in the forward pass touches them -- and the live list's cleared
      // d hdrop.  On the main stream behind its own, shorter branch instead: no change per-caption, +0.02 ms with per-image features.)
      UIC_TRY(st.bwd_begin(s3, st.persist_ok(), st.compact));
      bwd_begun = true;
      live_begun = st.compact;
      UIC_TRY(flush_gathered_late(ss, s3));           // (gathered refresh: the recurrence's and the logit layer's operand copies, last to arrive)
      UIC_HIP(hipEventRecord(ss->ev_pro3, s3));
    }
    UIC_TRY(flush_transposes(ss));                    // (behind the branch: only the backward pass reads them)
    UIC_HIP(hipStreamWaitEvent(s, ss->ev_pro, 0));
    if (split3) UIC_HIP(hipStreamWaitEvent(s, ss->ev_pro3, 0));
    if (ss->cast_recorded) UIC_HIP(hipStreamWaitEvent(s, ss->ev_cast, 0));   // the recurrence reads copies made on the side stream
  }

  if (st.compact && !live_begun) UIC_TRY(st.live_begin(s));   // (every logit chunk, on either stream, is ordered behind this point of the main stream)
  UIC_MARK(1, s);
  // persistent mode 3: the whole recurrence as ONE launch (it holds every CU, nothing overlaps it); the logit layer follows
  // chunk by chunk on the side stream beside the BPTT loop
  const bool one_launch = resume || st.persist_ok();
  const bool first_on_main = one_launch && nchunk >= 2 && !st.ss_on();
  if (one_launch) { if (!resume) UIC_TRY(st.fwd_steps(0, t_run, s)); UIC_MARK(2, s); }
  for (int i = 0; i < nchunk; ++i) {
    // after a single launch every step is there at once: the logit layer then takes the chunks LAST FIRST, the order the
    // BPTT loop consumes them in, so that loop starts after one chunk instead of after all of them
    const int c = one_launch ? nchunk - 1 - i : i;
    const int t0 = cb[c], t1 = cb[c + 1];
    if (!one_launch) UIC_TRY(st.fwd_steps(t0, t1, s));
    if (first_on_main && i == 0) {
      // the chunk the BPTT loop starts from, on the MAIN stream itself (idle until that chunk is through anyway): no event hop to
      // the side stream and back in front of the loop; the side stream starts with the next chunk once this one is done
      UIC_TRY(wait_refresh(s));                       // (d hdrop = d logits W_logit reads the transposed copy the side stream made)
      if (!resume) UIC_TRY(st.logits_rows(t0, t1, s));
      UIC_TRY(st.xe_rows(t0, t1, inv, nullptr, 1, s));
      UIC_TRY(st.dh_rows(t0, t1, s, false));
      UIC_HIP(hipEventRecord(ss->ev_main[c], s));
      UIC_HIP(hipStreamWaitEvent(s2, ss->ev_main[c], 0));
      continue;
    }
    if (!one_launch || i == 0) UIC_HIP(hipEventRecord(ss->ev_main[c], s));
    // side: logit layer of the chunk, forward and backward-to-h (beside the next chunk's recurrence)
    if (!one_launch || i == 0) UIC_HIP(hipStreamWaitEvent(s2, ss->ev_main[c], 0));
    if (!resume) UIC_TRY(st.logits_rows(t0, t1, s2));
    UIC_TRY(st.xe_rows(t0, t1, inv, nullptr, 1, s2));
    UIC_TRY(st.dh_rows(t0, t1, s2, true));
    UIC_HIP(hipEventRecord(ss->ev_side[c], s2));
  }
  if (!one_launch) UIC_MARK(2, s);
  UIC_MARK(3, s2);                                    // side: the logit layer (forward, loss, d hdrop) is through
  // side: logit-layer weight gradients + loss reduction, beside the BPTT loop
  // (weight-gradient GEMMs that run beside the BPTT loop keep the 2-stage kernel: the 4-stage ring's 128 KB of LDS would
  // keep the loop's 74-KB workgroups off its CUs -- measured 3.89 -> 3.99 ms)
  // (data-parallel order: the chunks' gradients share the side stream with the logit layer, where the 128 x 128 kernel's short
  // launches serve the stream's latency better than 56-workgroup ones -- 3.84 vs 3.99 ms per step beside the stand-in exchange)
  const UicWgPlace beside = comm ? UIC_WG_BESIDE_TN128 : UIC_WG_BESIDE;
  UIC_TRY(st.logit_weight_grads(s2, beside));
  UIC_TRY(uic_reduce_sum_launch(st.L.row_loss, st.compact ? (size_t)st.live_total() : (size_t)t_run * d->N, inv, loss_out, s2));
  if (den_out) UIC_TRY(uic_copy_launch(den_out, st.L.scalars, 4, s2));
  UIC_HIP(hipEventRecord(ss->ev_logit, s2));          // gradient group 0 (logit layer) final: its exchange can start now
  UIC_MARK(10, s2);
  // main: BPTT, each step waits for the d hdrop rows of its chunk; side: the recurrent weight gradients of every
  // finished chunk (transposes + accumulating GEMMs), so only the last chunk's share outlives the loop
  UIC_TRY(wait_refresh(s));                           // the BPTT loop reads the transposed weight copies
  if (!bwd_begun) UIC_TRY(st.bwd_begin(s));
  {
    // The embedding gradient's token bucketing needs only the tokens (labels; under scheduled sampling the tokens the forward
    // pass fed, which the side stream has waited for): in the side stream's slack inside the BPTT window.  Two halves: the
    // share of decode steps [CH, t_run) is gathered while the BPTT loop works on its last chunk, only steps [0, CH) afterwards.
    st.embed_split = st.early_grads() && nchunk >= 2 ? cb[1] : 0;
    if (!st.ss_on() || st.early_grads()) {
      UIC_TRY(uic_embed_bwd_sorted_prepare(st.embed_tokens(), st.embed_ldtok(), d->N, t_run, d->V1, d->E, G->embed_w, st.L.embed_scratch, s2,
                                           st.embed_split));
      st.embed_prepared = true;
      UIC_HIP(hipEventRecord(ss->ev_prep, s2));
    }
  }
  // The tail after the BPTT loop is three independent pieces of throughput work: the last chunk's recurrent weight gradients
  // (side stream), the late group (main stream), and what completes att_lstm.weight_ih and the embedding table (sum over steps,
  // fc' columns, d xt GEMM, gather).  In the default order the third piece goes to the THIRD stream beside the other two
  // instead of behind the first (measured: the side stream's tail was the end of the step, 0.1 ms after the main stream's).
  const bool tail3 = !early && st.embed_prepared;
  for (int c = nchunk - 1; c >= 0; --c) {
    const int t0 = cb[c], t1 = cb[c + 1];
    if (!(first_on_main && c == nchunk - 1)) UIC_HIP(hipStreamWaitEvent(s, ss->ev_side[c], 0));
    if (c == nchunk - 1) UIC_MARK(4, s);              // main: BPTT starts
    UIC_TRY(st.bwd_steps(t0, t1, s));
    UIC_HIP(hipEventRecord(ss->ev_main[c], s));       // (the forward's use of ev_main[c] was consumed long ago)
    if (early) {
      UIC_HIP(hipStreamWaitEvent(s2, ss->ev_main[c], 0));
      UIC_HIP(hipStreamWaitEvent(s3, ss->ev_main[c], 0));
      UIC_TRY(st.wgrad_chunk(t0, t1, c == nchunk - 1, beside, s2, false, s3));
      if (c == 1) UIC_TRY(st.embed_grad(1, s2));      // d xt of steps [CH, t_run) is complete: their share of the embedding table
    } else if (comm) {
      UIC_HIP(hipStreamWaitEvent(s2, ss->ev_main[c], 0));
      UIC_TRY(st.wgrad_chunk(t0, t1, c == nchunk - 1, beside, s2, false));
    } else {
      // default order: the chunks' weight gradients on stream 3, one chunk after the other, both shares of a chunk in turn (the
      // 256 x 256 weight-gradient kernel runs a share on ~60 CUs: beside the side stream's logit layer they leave the BPTT chain
      // most of the chip; two streams of them slow the chain down again: 3.15 vs 3.08 ms, profiles/r05_v1_ab_knobs.txt), the side
      // stream stays with the logit layer.  The LAST chunk's, which start when the loop is over, are dispatched as alone on the chip.
      UIC_HIP(hipStreamWaitEvent(s3, ss->ev_main[c], 0));
      UIC_TRY(st.wgrad_chunk(t0, t1, c == nchunk - 1, c == 0 ? UIC_WG_ALONE : beside, s3, true));
    }
  }
  if (early) {
    // side: what completes att_lstm.weight_ih and the embedding table comes first, so that the two big tensors of the early
    // group are final with gradient group 1 (the fc_embed chain and the bias sums -- ~4 MB -- follow)
    UIC_TRY(st.fc_cols_grad(s2, st.L.slab2, st.L.tSA, st.L.tSB, beside));
    UIC_TRY(st.embed_grad(0, s2));
    UIC_HIP(hipEventRecord(ss->ev_embed, s2));
    ss->embed_recorded = true;
    UIC_HIP(hipEventRecord(ss->ev_s3, s3));
    UIC_HIP(hipStreamWaitEvent(s2, ss->ev_s3, 0));    // the third stream's share of the weight gradients
  } else if (comm) {
    if (tail3) {   // (round 4's tail: what completes att_lstm.weight_ih and the embedding table on stream 3 beside the last chunk's gradients)
      UIC_HIP(hipStreamWaitEvent(s3, ss->ev_main[0], 0));
      UIC_HIP(hipStreamWaitEvent(s3, ss->ev_prep, 0));
      UIC_TRY(st.fc_cols_grad(s3, st.L.slab3, st.L.tTA, st.L.tTB, beside));
      UIC_TRY(st.embed_grad(0, s3));
      UIC_HIP(hipEventRecord(ss->ev_s3, s3));
      UIC_HIP(hipEventRecord(ss->ev_embed, s3));
      ss->embed_recorded = true;
    }
  } else if (tail3) {
    UIC_HIP(hipStreamWaitEvent(s2, ss->ev_main[0], 0));     // the BPTT loop is through: dG1 of every step exists
    UIC_TRY(st.fc_cols_grad(s2, st.L.slab2, st.L.tSA, st.L.tSB, UIC_WG_ALONE));
    UIC_TRY(st.embed_grad(0, s2));
    UIC_HIP(hipEventRecord(ss->ev_embed, s2));
    ss->embed_recorded = true;
  }
  // side: the rest of the early gradient group (LSTM / h2att biases, embedding, fc_embed); main: the late group
  // (attention accumulation, ctx2att, att_embed).  ev_early: the early group, the logit layer and the loss are final.
  UIC_MARK(5, s);                                     // main: BPTT done
  hipStream_t s_lstm = (early || comm) ? s2 : s3;
  UIC_HIP(hipEventRecord(ss->ev_lstm, s_lstm));       // gradient group 1 final (uic_topdown_grad_ready_wait)
  UIC_MARK(6, s_lstm);                                // side: recurrent weight gradients done
  UIC_TRY(st.bwd_epilogue_late(s, UIC_WG_ALONE, true));   // (enqueued first: it is the longer of the two tails)
  UIC_MARK(7, s);
  if (!early && !tail3) UIC_HIP(hipStreamWaitEvent(s2, ss->ev_main[0], 0));
  if (comm && tail3) UIC_HIP(hipStreamWaitEvent(s2, ss->ev_s3, 0));      // (d fc' below reads the dGfc that fc_cols_grad left)
  const bool chunks_elsewhere = !early && !comm;      // the chunks' weight (and bias) gradients were made on stream 3
  UIC_TRY(st.bwd_epilogue_early(s2, UIC_WG_ALONE, true, true, early || tail3, !chunks_elsewhere));
  if (chunks_elsewhere) {
    UIC_HIP(hipStreamWaitEvent(s2, ss->ev_lstm, 0));  // the early group includes them; bias_hh = bias_ih needs the bias columns
    UIC_TRY(st.bias_hh_copies(s2));
  }
  UIC_HIP(hipEventRecord(ss->ev_early, s2));
  ss->early_recorded = true;
  UIC_MARK(8, s2);
  UIC_HIP(hipStreamWaitEvent(s, ss->ev_early, 0));    // join
  UIC_MARK(9, s);
  ss->compact_launches = st.compact_launches;
  ss->marks_valid = ss->marks_on;
#undef UIC_MARK
#undef UIC_HIP
  return UIC_OK;
}

int uic_topdown_step_marks(int32_t enable, float* ms_out) {
  SideStream* ss = nullptr;
  UIC_TRY(get_side(&ss));
  if (ms_out) {
    UIC_REQUIRE(ss->marks_valid, "step_marks: no fused step has run with the marks enabled");
    UIC_TRY(uic_check_hip(hipEventSynchronize(ss->mark[9]), "hipEventSynchronize"));   // (joined: every other mark precedes it)
    UIC_TRY(uic_check_hip(hipEventSynchronize(ss->mark[8]), "hipEventSynchronize"));
    ms_out[0] = 0.f;
    for (int i = 1; i < UIC_STEP_MARKS; ++i) UIC_TRY(uic_check_hip(hipEventElapsedTime(&ms_out[i], ss->mark[0], ss->mark[i]), "hipEventElapsedTime"));
  }
  ss->marks_on = enable != 0;
  if (!ss->marks_on) ss->marks_valid = false;
  return UIC_OK;
}

int uic_topdown_compact_launches(int32_t* out) {
  SideStream* ss = nullptr;
  UIC_TRY(get_side(&ss));
  UIC_REQUIRE(out, "compact_launches: null pointer");
  *out = ss->compact_launches;
  return UIC_OK;
}

int uic_topdown_grad_ready_wait(void* stream, int32_t group) {
  SideStream* ss = nullptr;
  UIC_TRY(get_side(&ss));
  UIC_REQUIRE(group >= 0 && group <= 4, "grad_ready_wait: group=%d must be 0 (logit layer), 1 (LSTM weights), 2 (early group), 3 (embedding table + att_lstm.weight_ih) or 4 (embedding table)", group);
  UIC_REQUIRE(ss->early_recorded, "grad_ready_wait: no uic_topdown_xe_train_step has run on this device yet");
  if (group == 4)   // embed.0.weight alone: its gather runs beside the last chunk's weight gradients and is through first
    return uic_check_hip(hipStreamWaitEvent((hipStream_t)stream, ss->embed_recorded ? ss->ev_embed : ss->ev_early, 0), "hipStreamWaitEvent");
  if (group == 3) {
    // embed.0.weight and core.att_lstm.weight_ih: the table's gather and the fc' columns (ev_embed) + the matrix's other columns,
    // which come with the recurrent weight gradients (ev_lstm).  A step that made them inside its early epilogue (scheduled
    // sampling without the early order) has no separate event: they are final with the early group
    if (!ss->embed_recorded) return uic_check_hip(hipStreamWaitEvent((hipStream_t)stream, ss->ev_early, 0), "hipStreamWaitEvent");
    UIC_TRY(uic_check_hip(hipStreamWaitEvent((hipStream_t)stream, ss->ev_embed, 0), "hipStreamWaitEvent"));
    return uic_check_hip(hipStreamWaitEvent((hipStream_t)stream, ss->ev_lstm, 0), "hipStreamWaitEvent");
  }
  hipEvent_t ev = group == 0 ? ss->ev_logit : group == 1 ? ss->ev_lstm : ss->ev_early;
  return uic_check_hip(hipStreamWaitEvent((hipStream_t)stream, ev, 0), "hipStreamWaitEvent");
}

}  // extern "C"
