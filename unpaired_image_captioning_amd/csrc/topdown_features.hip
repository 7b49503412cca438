// The TopDown captioner's feature prologue (_prepare_feature) and attention step, the per-device side streams of the fused training
// step, and the weight refresh: operand-dtype and transposed copies of the master weights, made on the caller's and the side stream.
#include "topdown_internal.h"
#include <mutex>

namespace {

__global__ void rowlen_kernel(const float* mask, int N, int R, int* out) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  int c = 0;
  for (int r = 0; r < R; ++r) c += mask[(size_t)n * R + r] != 0.f;
  out[n] = c;
}

}  // namespace

namespace topdown {

constexpr float BN_MOMENTUM = 0.1f, BN_EPS = 1e-5f;   // nn.BatchNorm1d defaults (AttModel.py:79,83)

// _prepare_feature (P/models/AttModel.py:107-117) + operand casts.  part: 0 = everything; 1 = only the fc_embed branch
// (fc' = dropout(relu(fc_embed(fc)))), 2 = only the att_embed / ctx2att branch -- the two are independent, the fused
// training step runs them on its two streams.
int prepare_features(const uic_topdown_dims& d, const uic_topdown_weights* w, const Derived& dv, const uic_topdown_batch* b,
                     const Layout& L, int training, float drop_p, unsigned seed, const void** fc_in_out, const void** att_in_out,
                     hipStream_t s, int part) {
  const int dt = d.dtype;
  const int N = d.N, R = d.R, H = d.H, A = d.A;
  const bool bn_train = (training & 1) != 0, bn_update = bn_train && !(training & 2);
  // seq_per_img = S > 1: fc_feats / att_feats / att_masks hold one row per IMAGE; caption row n belongs to image n / S
  const int S = d.seq_per_img > 1 ? d.seq_per_img : 1, Ni = N / S;
  const bool fold = S > 1;                  // att_embed's [BatchNorm +] Linear runs once per image; dropout is applied per caption row
  const float* att_src = b->att_feats;
  const float* amask = b->att_masks;        // per caption row
  const int Na = fold ? Ni : N;             // rows of att_src
  const int* row_len = b->att_masks ? L.row_len : nullptr;          // per row of att_src
  const int* row_len_cap = row_len;                                 // per caption row
  const bool do_fc = part != 2, do_att = part != 1;
  if (b->att_masks && !do_att) {       // (pointers only)
    if (fold) { amask = L.amask_rep; row_len_cap = L.row_len_rep; }
  } else if (b->att_masks) {
    hipLaunchKernelGGL(rowlen_kernel, dim3((Na + 255) / 256), dim3(256), 0, s, b->att_masks, Na, R, L.row_len);
    UIC_LAUNCH_CHECK("rowlen_kernel");
    if (fold) {
      UIC_TRY(uic_expand_rows_launch(UIC_F32, b->att_masks, L.amask_rep, Ni, S, (size_t)R, s));
      amask = L.amask_rep;
      hipLaunchKernelGGL(rowlen_kernel, dim3((N + 255) / 256), dim3(256), 0, s, amask, N, R, L.row_len_rep);
      UIC_LAUNCH_CHECK("rowlen_kernel");
      row_len_cap = L.row_len_rep;
    }
  }
  const void* fc_in = b->fc_feats;
  const void* att_in = att_src;
  if (S > 1) {
    if (do_fc) UIC_TRY(uic_expand_rows_launch(dt, b->fc_feats, L.fcT, Ni, S, (size_t)d.Dfc, s));
    fc_in = L.fcT;
  } else if (dt == UIC_BF16) {
    if (do_fc) UIC_TRY(uic_cast_f32_launch(dt, b->fc_feats, L.fcT, (size_t)N * d.Dfc, s));
    fc_in = L.fcT;
  }
  if (d.use_bn || dt == UIC_BF16) att_in = L.attT;
  // bf16 without BatchNorm in front: att_embed's GEMM takes the f32 features as they are, rounds them on their way to LDS and
  // leaves the bf16 image in L.attT for the weight gradient (gemm_pp.hip, f32 A operand) -- no separate 283 MB cast pass
  bool att_f32a = false;
  if (do_att && !d.use_bn && dt == UIC_BF16) {
    UicGemmParams g = gemm_base(dt, Na * R, H);
    add_seg(g, att_src, d.D, dv.att_w, d.D, d.D);
    g.C = L.attp; g.ldc = H; g.a_f32 = 1; g.a_copy = L.attT; g.ld_a_copy = d.D;
    att_f32a = uic_gemm_pp_eligible(g) && (size_t)Na * R >= 2048 && !(d.recurrence & UIC_REC_NO_F32A);
  }
  if (do_att && d.use_bn) {
    // BatchNorm1d(D) over the packed live regions; xhat goes to the GEMM, the affine part lives in W' / b'.  Features given
    // once per image stand for S identical caption rows each: same mean / biased variance, `rep` fixes the unbiased one.
    if (bn_train)
      UIC_TRY(uic_bn_stats_launch(UIC_F32, att_src, Na * R, R, d.D, row_len, L.bn_part, BN_MOMENTUM, BN_EPS, L.bn_stat0,
                                  bn_update ? w->att_bn0_rm : nullptr, bn_update ? w->att_bn0_rv : nullptr, s, (float)S));
    else
      UIC_TRY(uic_bn_stats_running_launch(w->att_bn0_rm, w->att_bn0_rv, d.D, BN_EPS, L.bn_stat0, s));
    UIC_TRY(uic_bn_apply_launch(UIC_F32, dt, att_src, Na * R, R, d.D, row_len, L.bn_stat0, nullptr, nullptr, 0, L.attT, s));
  } else if (do_att && dt == UIC_BF16 && !att_f32a) {
    UIC_TRY(uic_cast_f32_launch(dt, att_src, L.attT, (size_t)Na * R * d.D, s));
  }
  *fc_in_out = fc_in;
  *att_in_out = att_in;
  if (do_fc) {
    UicGemmParams g = gemm_base(dt, N, H);
    add_seg(g, fc_in, d.Dfc, dv.fc_w, d.Dfc, d.Dfc);
    g.C = L.fcp; g.ldc = H; g.bias = w->fc_b; g.flags = UIC_GEMM_RELU;
    g.drop_p = drop_p; g.seed = seed; g.site = UIC_SITE_FC;
    UIC_TRY(uic_gemm_launch(g, s));
  }
  if (!do_att) return UIC_OK;
  void* const att_out = d.use_bn == 2 ? L.ybn : L.attp;
  if (fold) {
    // relu(W att + b) once per image (f32), then S caption rows with their own dropout masks -- element for element
    // what the S-fold replicated GEMM epilogue writes
    UicGemmParams g = gemm_base(dt, Ni * R, H);
    add_seg(g, att_in, d.D, dv.att_w, d.D, d.D);
    if (att_f32a) { g.seg[0].A = att_src; g.a_f32 = 1; g.a_copy = L.attT; g.ld_a_copy = d.D; }
    g.C = L.ypre; g.ldc = H; g.bias = d.use_bn ? dv.att_beff : w->att_b; g.flags = UIC_GEMM_RELU | UIC_GEMM_OUT_F32;
    if (b->att_masks) { g.row_len = L.row_len; g.R = R; }
    UIC_TRY(uic_gemm_launch(g, s));
    UIC_TRY(uic_expand_drop_launch(dt, L.ypre, att_out, Ni, S, (size_t)R * H, drop_p, seed, UIC_SITE_ATT, s));
  } else {
    UicGemmParams g = gemm_base(dt, N * R, H);
    add_seg(g, att_in, d.D, dv.att_w, d.D, d.D);
    if (att_f32a) { g.seg[0].A = att_src; g.a_f32 = 1; g.a_copy = L.attT; g.ld_a_copy = d.D; }
    g.C = att_out; g.ldc = H; g.bias = d.use_bn ? dv.att_beff : w->att_b; g.flags = UIC_GEMM_RELU;
    if (b->att_masks) { g.row_len = L.row_len; g.R = R; }
    g.drop_p = drop_p; g.seed = seed; g.site = UIC_SITE_ATT;
    UIC_TRY(uic_gemm_launch(g, s));
  }
  if (d.use_bn == 2) {   // BatchNorm1d(H) after the Dropout; padded regions stay zero (pad_unsort_packed_sequence)
    if (bn_train)
      UIC_TRY(uic_bn_stats_launch(dt, L.ybn, N * R, R, H, row_len_cap, L.bn_part, BN_MOMENTUM, BN_EPS, L.bn_stat4,
                                  bn_update ? w->att_bn4_rm : nullptr, bn_update ? w->att_bn4_rv : nullptr, s));
    else
      UIC_TRY(uic_bn_stats_running_launch(w->att_bn4_rm, w->att_bn4_rv, H, BN_EPS, L.bn_stat4, s));
    UIC_TRY(uic_bn_apply_launch(dt, dt, L.ybn, N * R, R, H, row_len_cap, L.bn_stat4, w->att_bn4_w, w->att_bn4_b, 1, L.attp, s));
  }
  {
    UicGemmParams g = gemm_base(dt, N * R, A);
    add_seg(g, L.attp, H, dv.ctx2att_w, H, H);
    g.C = L.patt; g.ldc = A; g.bias = w->ctx2att_b;
    // e^{2 p_att} for the persistent recurrence's attention (rnn_persist.hip): from the ping-pong kernel's epilogue where that
    // kernel takes the problem, else one element-wise pass -- the same values either way
    g.C_exp2 = L.eatt;
    UIC_TRY(uic_gemm_launch(g, s));
  }
  return UIC_OK;
}

int attention_step(const uic_topdown_dims& d, const uic_topdown_weights* w, const Derived& dv, const uic_topdown_batch* b,
                   const Layout& L, const void* h_att, float* att_h, float* alpha, void* ctx, hipStream_t s) {
  UicGemmParams g = gemm_base(d.dtype, d.N, d.A);
  add_seg(g, h_att, d.H, dv.h2att_w, d.H, d.H);
  g.C = att_h; g.ldc = d.A; g.bias = w->h2att_b; g.flags = UIC_GEMM_OUT_F32;
  UIC_TRY(uic_gemm_launch(g, s));
  UicAttnParams a;
  memset(&a, 0, sizeof(a));
  a.dtype = d.dtype; a.N = d.N; a.R = d.R; a.A = d.A; a.H = d.H;
  a.att_h = att_h; a.p_att = L.patt; a.att = L.attp; a.w_alpha = w->alpha_w; a.b_alpha = w->alpha_b;
  a.mask = b->att_masks ? (d.seq_per_img > 1 ? L.amask_rep : b->att_masks) : nullptr; a.ldmask = d.R; a.alpha = alpha; a.ctx = ctx; a.ldctx = d.H;
  return uic_attention_fwd_launch(a, s);
}

// (the only instance: every other file reaches it through get_side)
SideStream g_side[16];
std::mutex g_side_mutex;   // guards the one-time creation of a device's streams / events (calls themselves are per device:
                           // one host thread drives a device at a time, as with any stream-ordered library state)

int get_side(SideStream** out) {
  int dev = 0;
  UIC_TRY(uic_check_hip(hipGetDevice(&dev), "hipGetDevice"));
  UIC_REQUIRE(dev >= 0 && dev < 16, "device index %d out of range", dev);
  SideStream& ss = g_side[dev];
  std::lock_guard<std::mutex> lock(g_side_mutex);
  if (!ss.ready) {
    // A plain second stream at the lowest priority.  Measured alternatives: confining it to a subset of the CUs
    // (hipExtStreamCreateWithCUMask, 64..224 CUs) makes the whole step 2x SLOWER; the priority itself is neutral.
    int least = 0, greatest = 0;
    UIC_TRY(uic_check_hip(hipDeviceGetStreamPriorityRange(&least, &greatest), "hipDeviceGetStreamPriorityRange"));
    UIC_TRY(uic_check_hip(hipStreamCreateWithPriority(&ss.stream, hipStreamNonBlocking, least), "hipStreamCreateWithPriority"));
    UIC_TRY(uic_check_hip(hipStreamCreateWithPriority(&ss.stream3, hipStreamNonBlocking, least), "hipStreamCreateWithPriority"));
    // NO fourth stream: a process gets full-speed dispatch from four HIP streams in all (tools/queue_probe.py: with the caller's
    // stream, these two and ONE more stream of the caller -- its communication stream -- a busy extra stream costs nothing; with a
    // fifth stream in existence, used or not, the same extra stream makes the step 0.7 ms longer).  The last chunk's second share
    // therefore runs behind the first on stream 3.
    hipEvent_t* const untimed[] = {&ss.ev_s3, &ss.ev_prep, &ss.ev_den, &ss.ev_done, &ss.ev_pro, &ss.ev_pro3, &ss.ev_early, &ss.ev_embed,
                                   &ss.ev_logit, &ss.ev_lstm, &ss.ev_r0, &ss.ev_refresh, &ss.ev_cast, &ss.ev_g2, &ss.ev_gl};
    for (hipEvent_t* ev : untimed) UIC_TRY(uic_check_hip(hipEventCreateWithFlags(ev, hipEventDisableTiming), "hipEventCreate"));
    for (int i = 0; i < UIC_STEP_MARKS; ++i) UIC_TRY(uic_check_hip(hipEventCreate(&ss.mark[i]), "hipEventCreate"));
    for (int i = 0; i < MAX_CHUNKS; ++i) {
      UIC_TRY(uic_check_hip(hipEventCreateWithFlags(&ss.ev_main[i], hipEventDisableTiming), "hipEventCreate"));
      UIC_TRY(uic_check_hip(hipEventCreateWithFlags(&ss.ev_side[i], hipEventDisableTiming), "hipEventCreate"));
    }
    ss.ready = true;
  }
  *out = &ss;
  return UIC_OK;
}

// the late half of uic_topdown_refresh_weights_gathered (see SideStream::gl_pending), on `st`
int flush_gathered_late(SideStream* ss, hipStream_t st) {
  if (!ss->gl_pending) return UIC_OK;
  ss->gl_pending = false;
  for (int i = 0; i < 2; ++i)
    if (ss->gl_ready[i]) UIC_TRY(uic_check_hip(hipStreamWaitEvent(st, (hipEvent_t)ss->gl_ready[i], 0), "hipStreamWaitEvent(gathered)"));
  UIC_TRY(uic_copy_multi_launch(ss->gl_count, ss->gl_src, ss->gl_dst, ss->gl_bytes, st));
  UIC_TRY(uic_check_hip(hipEventRecord(ss->ev_gl, st), "hipEventRecord"));
  ss->gl_recorded = true;
  return UIC_OK;
}

// the deferred half of uic_topdown_refresh_weights: the transposed copies the backward pass reads, on the side stream
int flush_transposes(SideStream* ss) {
  if (ss->gl_pending) UIC_TRY(flush_gathered_late(ss, ss->stream));
  if (!ss->transposes_pending) return UIC_OK;
  ss->transposes_pending = false;
  if (ss->gl_recorded) UIC_TRY(uic_check_hip(hipStreamWaitEvent(ss->stream, ss->ev_gl, 0), "hipStreamWaitEvent(gathered late)"));
  const uic_topdown_dims* d = &ss->tp_d;
  const Derived v = make_derived(*d, &ss->tp_w, ss->tp_derived);
  hipStream_t s2 = ss->stream;
  const int dt = d->dtype, H = d->H, E = d->E, A = d->A, V1 = d->V1;
  const int V1p = (int)vpad(V1), H4 = 4 * H, ldih = E + 2 * H;
  // one launch for all of them (the launches, not the 10 MB, are what the side stream would spend its time on)
  UicTransposeJob jobs[UIC_TRANSPOSE_MULTI];
  int nj = 0;
  auto job = [&](const void* src, int rows, int cols, int lds, void* dst, int ldd) { jobs[nj++] = UicTransposeJob{src, dst, rows, cols, lds, ldd}; };
  job(v.logit_w, V1, H, H, v.logit_wT, V1p);
  // w2T rows [0,2H) <- lang_w_ih^T, rows [2H,3H) <- lang_w_hh^T
  job(v.lang_w_ih, H4, 2 * H, 2 * H, v.w2T, H4);
  job(v.lang_w_hh, H4, H, H, offw(v.w2T, (size_t)2 * H * H4, dt), H4);
  job(v.att_w_ih, H4, H, ldih, v.w1recT, H4);
  job(v.att_w_hh, H4, H, H, offw(v.w1recT, (size_t)H * H4, dt), H4);
  job(off(v.att_w_ih, 2 * H, dt), H4, E, ldih, v.wxT, H4);
  job(off(v.att_w_ih, H, dt), H4, H, ldih, v.wfcpT, H4);
  job(v.h2att_w, A, H, H, v.h2attT, A);
  job(v.ctx2att_w, A, H, H, v.ctx2attT, A);
  for (int l = 0; l + 1 < d->logit_layers; ++l) job(v.logit_h_w[l], H, H, H, v.logit_h_wT[l], H);
  UIC_TRY(uic_transpose_multi_launch(dt, nj, jobs, s2));
  UIC_TRY(uic_check_hip(hipEventRecord(ss->ev_refresh, s2), "hipEventRecord"));
  ss->refresh_pending = true;
  return UIC_OK;
}

// every consumer of the derived weights first lets its stream wait for the side-stream part of the last refresh
int wait_refresh(hipStream_t s) {
  SideStream* ss = nullptr;
  UIC_TRY(get_side(&ss));
  UIC_TRY(flush_transposes(ss));
  if (ss->refresh_pending) UIC_TRY(uic_check_hip(hipStreamWaitEvent(s, ss->ev_refresh, 0), "hipStreamWaitEvent(refresh)"));
  return UIC_OK;
}

}  // namespace topdown

using namespace topdown;

extern "C" {

int uic_topdown_refresh_weights(const uic_topdown_dims* d, const uic_topdown_weights* w, void* derived, void* stream) {
  UIC_TRY(uic_topdown_refresh_weights_deferred(d, w, derived, stream));
  SideStream* ss = nullptr;
  UIC_TRY(get_side(&ss));
  return flush_transposes(ss);
}

int uic_topdown_refresh_weights_deferred(const uic_topdown_dims* d, const uic_topdown_weights* w, void* derived, void* stream) {
  UIC_TRY(check_dims(d));
  UIC_REQUIRE(w && derived, "refresh_weights: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const Derived v = make_derived(*d, w, derived);
  const int dt = d->dtype;
  const int D = d->D, Dfc = d->Dfc, H = d->H, E = d->E, A = d->A, V1 = d->V1;
  const int V1p = (int)vpad(V1);
  // The copies the feature projection and the batched input GEMMs need come first, on the caller's stream; everything
  // the recurrence, the logit layer and the backward pass need is produced on the side stream meanwhile (consumers
  // wait for ev_refresh, see wait_refresh), so a training step does not start with ~0.1 ms of serial weight shuffling.
  SideStream* ss = nullptr;
  UIC_TRY(get_side(&ss));
  hipStream_t s2 = ss->stream;
  if (ss->transposes_pending && ss->tp_derived != derived) UIC_TRY(flush_transposes(ss));   // another model's deferred half
  ss->g2_recorded = false;
  ss->gl_pending = false;                             // (a gathered refresh nobody consumed: this refresh rewrites every copy)
  ss->gl_recorded = false;
  UIC_TRY(uic_check_hip(hipEventRecord(ss->ev_r0, s), "hipEventRecord"));          // the master weights are final
  UIC_TRY(uic_check_hip(hipStreamWaitEvent(s2, ss->ev_r0, 0), "hipStreamWaitEvent"));
  if (dt == UIC_BF16) {   // one launch per stream (the step waits for launches here, not for bytes)
    {
      const float* src[4] = {w->fc_w, d->use_bn ? nullptr : w->att_w, w->ctx2att_w, w->att_lstm_w_ih};
      void* dst[4] = {(void*)v.fc_w, (void*)v.att_w, (void*)v.ctx2att_w, (void*)v.att_w_ih};
      const size_t n[4] = {(size_t)H * Dfc, d->use_bn ? 0 : (size_t)H * D, (size_t)A * H, (size_t)4 * H * (E + 2 * H)};
      UIC_TRY(uic_cast_f32_multi_launch(dt, 4, src, dst, n, s));
    }
    {
      // (the embedding table first: the side stream's branch of the fused step's prologue starts with the lookup)
      const float* src[6] = {w->embed_w, w->logit_w, w->att_lstm_w_hh, w->lang_lstm_w_ih, w->lang_lstm_w_hh, w->h2att_w};
      void* dst[6] = {(void*)v.embed_w, (void*)v.logit_w, (void*)v.att_w_hh, (void*)v.lang_w_ih, (void*)v.lang_w_hh, (void*)v.h2att_w};
      const size_t n[6] = {(size_t)V1 * E, (size_t)V1 * H, (size_t)4 * H * H, (size_t)4 * H * 2 * H, (size_t)4 * H * H, (size_t)A * H};
      UIC_TRY(uic_cast_f32_multi_launch(dt, 6, src, dst, n, s2));
    }
  }
  if (d->use_bn) {
    UIC_REQUIRE(w->att_bn0_w && w->att_bn0_b && w->att_bn0_rm && w->att_bn0_rv, "use_bn=%d needs the att_embed.0 BatchNorm tensors", d->use_bn);
    UIC_REQUIRE(d->use_bn < 2 || (w->att_bn4_w && w->att_bn4_b && w->att_bn4_rm && w->att_bn4_rv), "use_bn=2 needs the att_embed.4 BatchNorm tensors");
    UIC_TRY(uic_bn_fold_weight_launch(dt, w->att_w, w->att_bn0_w, w->att_bn0_b, w->att_b, H, D, (void*)v.att_w, v.att_beff, s));
  }
  // the side stream's later work (the transposes of att_w_ih among it) reads the copies made on `s` above
  UIC_TRY(uic_check_hip(hipEventRecord(ss->ev_r0, s), "hipEventRecord"));
  UIC_TRY(uic_check_hip(hipStreamWaitEvent(s2, ss->ev_r0, 0), "hipStreamWaitEvent"));
  for (int l = 0; l + 1 < d->logit_layers; ++l) {
    UIC_REQUIRE(w->logit_h_w[l] && w->logit_h_b[l], "logit_layers=%d needs the hidden logit block %d", d->logit_layers, l);
    if (dt == UIC_BF16) UIC_TRY(uic_cast_f32_launch(dt, w->logit_h_w[l], (void*)v.logit_h_w[l], (size_t)H * H, s2));
  }
  UIC_TRY(uic_check_hip(hipEventRecord(ss->ev_cast, s2), "hipEventRecord"));
  ss->cast_recorded = true;
  // the transposes (backward pass only) follow when the first consumer asks for them: flush_transposes
  ss->tp_d = *d; ss->tp_w = *w; ss->tp_derived = derived;
  ss->transposes_pending = true;
  return UIC_OK;
}

// The refresh of a data-parallel rank whose optimizer is sharded (reduce-scatter -> Adam on the rank's shard -> all-gather of the
// updated weights in the operand dtype): the operand copies are not cast from the f32 masters -- a rank's masters are current only
// inside its own shard -- but copied from the all-gathered operand-dtype arena (`g`), each gather group behind the event the
// caller recorded after that group's all-gather.  f32 operands: the gathered tensors ARE the masters (make_derived points at
// them); the call only orders the streams behind the events.
int uic_topdown_refresh_weights_gathered(const uic_topdown_dims* d, const uic_topdown_weights* w, const uic_topdown_gathered* g,
                                         void* derived, int32_t deferred, void* stream) {
  UIC_TRY(check_dims(d));
  UIC_REQUIRE(w && g && derived, "refresh_weights_gathered: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const Derived v = make_derived(*d, w, derived);
  const int dt = d->dtype;
  const size_t D = d->D, Dfc = d->Dfc, H = d->H, E = d->E, A = d->A, V1 = d->V1, S = uic_dtype_size(dt);
  SideStream* ss = nullptr;
  UIC_TRY(get_side(&ss));
  hipStream_t s2 = ss->stream;
  if (ss->transposes_pending && ss->tp_derived != derived) UIC_TRY(flush_transposes(ss));
  ss->gl_pending = false;                             // (a gathered refresh nobody consumed: this one rewrites every copy)
  ss->g2_recorded = false;
  ss->gl_recorded = false;
  auto wait_group = [&](hipStream_t st, int grp) -> int {
    if (g->ready[grp]) UIC_TRY(uic_check_hip(hipStreamWaitEvent(st, (hipEvent_t)g->ready[grp], 0), "hipStreamWaitEvent(gathered)"));
    return UIC_OK;
  };
  if (dt != UIC_BF16) {
    // f32 operands: nothing to copy; every consumer stream is ordered behind `s`, which waits for all four groups
    UIC_REQUIRE((!g->logit_w || g->logit_w == w->logit_w) && (!g->embed_w || g->embed_w == w->embed_w) && (!g->att_w || g->att_w == w->att_w),
                "refresh_weights_gathered: with f32 operands the gathered tensors must be the masters themselves");
    for (int grp = 3; grp >= 0; --grp) UIC_TRY(wait_group(s, grp));
    return deferred ? uic_topdown_refresh_weights_deferred(d, w, derived, stream) : uic_topdown_refresh_weights(d, w, derived, stream);
  }
  UIC_REQUIRE(g->embed_w && g->fc_w && g->logit_w && g->ctx2att_w && g->att_lstm_w_ih && g->att_lstm_w_hh && g->lang_lstm_w_ih &&
                  g->lang_lstm_w_hh && g->h2att_w && (g->att_w || d->use_bn),
              "refresh_weights_gathered: a gathered tensor is missing");
  UIC_TRY(uic_check_hip(hipEventRecord(ss->ev_r0, s), "hipEventRecord"));          // whatever the caller enqueued before (the replicated f32 tensors' update)
  UIC_TRY(uic_check_hip(hipStreamWaitEvent(s2, ss->ev_r0, 0), "hipStreamWaitEvent"));
  {   // gather group 3 on the caller's stream: all the main branch of the fused step's prologue reads (att_embed, ctx2att) + h2att
    UIC_TRY(wait_group(s, 3));
    const void* src[3] = {d->use_bn ? nullptr : g->att_w, g->ctx2att_w, g->h2att_w};
    void* dst[3] = {(void*)v.att_w, (void*)v.ctx2att_w, (void*)v.h2att_w};
    const size_t n[3] = {d->use_bn ? 0 : H * D * S, A * H * S, A * H * S};
    UIC_TRY(uic_copy_multi_launch(3, src, dst, n, s));
  }
  {   // group 2 on the side stream (its prologue branch -- embedding lookup, batched input GEMM -- follows there; the third stream's
      // fc_embed / Gfc wait for ev_g2), then the recurrence's and the logit layer's groups
    UIC_TRY(wait_group(s2, 2));
    const void* src[3] = {g->embed_w, g->fc_w, g->att_lstm_w_ih};
    void* dst[3] = {(void*)v.embed_w, (void*)v.fc_w, (void*)v.att_w_ih};
    const size_t n[3] = {V1 * E * S, H * Dfc * S, 4 * H * (E + 2 * H) * S};
    UIC_TRY(uic_copy_multi_launch(3, src, dst, n, s2));
    UIC_TRY(uic_check_hip(hipEventRecord(ss->ev_g2, s2), "hipEventRecord"));
    ss->g2_recorded = true;
  }
  {
    UIC_REQUIRE(d->logit_layers - 1 + 4 <= UIC_CAST_MULTI, "refresh_weights_gathered: too many logit layers (%d)", d->logit_layers);
    int k = 0;
    auto add = [&](const void* src, const void* dst, size_t bytes) { ss->gl_src[k] = src; ss->gl_dst[k] = (void*)dst; ss->gl_bytes[k] = bytes; ++k; };
    add(g->att_lstm_w_hh, v.att_w_hh, 4 * H * H * S);
    add(g->lang_lstm_w_ih, v.lang_w_ih, 4 * H * 2 * H * S);
    add(g->lang_lstm_w_hh, v.lang_w_hh, 4 * H * H * S);
    add(g->logit_w, v.logit_w, V1 * H * S);
    for (int l = 0; l + 1 < d->logit_layers; ++l) {
      UIC_REQUIRE(g->logit_h_w[l] && w->logit_h_b[l], "logit_layers=%d needs the hidden logit block %d", d->logit_layers, l);
      add(g->logit_h_w[l], v.logit_h_w[l], H * H * S);
    }
    ss->gl_count = k;
    ss->gl_ready[0] = g->ready[1]; ss->gl_ready[1] = g->ready[0];
    ss->gl_pending = true;
    ss->gl_recorded = false;
    if (!deferred) UIC_TRY(flush_gathered_late(ss, s2));
  }
  if (d->use_bn) {   // att_embed's Linear with the BatchNorm folded in needs the f32 master: the caller keeps that tensor replicated
    UIC_REQUIRE(w->att_bn0_w && w->att_bn0_b && w->att_bn0_rm && w->att_bn0_rv, "use_bn=%d needs the att_embed.0 BatchNorm tensors", d->use_bn);
    UIC_TRY(uic_bn_fold_weight_launch(dt, w->att_w, w->att_bn0_w, w->att_bn0_b, w->att_b, (int)H, (int)D, (void*)v.att_w, v.att_beff, s));
  }
  UIC_TRY(uic_check_hip(hipEventRecord(ss->ev_r0, s), "hipEventRecord"));          // the side stream's transposes read ctx2att / h2att copied on `s`
  UIC_TRY(uic_check_hip(hipStreamWaitEvent(s2, ss->ev_r0, 0), "hipStreamWaitEvent"));
  UIC_TRY(uic_check_hip(hipEventRecord(ss->ev_cast, s2), "hipEventRecord"));
  ss->cast_recorded = true;
  ss->tp_d = *d; ss->tp_w = *w; ss->tp_derived = derived;
  ss->transposes_pending = true;
  if (!deferred) {
    // any consumer may follow on `s` (decode passes, single calls): everything the side stream copied is ordered in front of it
    UIC_TRY(flush_transposes(ss));
    UIC_TRY(uic_check_hip(hipStreamWaitEvent(s, ss->ev_refresh, 0), "hipStreamWaitEvent(refresh)"));
  }
  return UIC_OK;
}

int uic_topdown_prepare_feature(const uic_topdown_dims* d, const uic_topdown_weights* w, const void* derived,
                                const uic_topdown_batch* b, int32_t training, uint32_t seed, void* workspace,
                                float* fc_out, float* att_out, float* p_att_out, void* stream) {
  UIC_TRY(check_dims(d));
  UIC_REQUIRE(w && derived && b && workspace && fc_out && att_out && p_att_out, "prepare_feature: null pointer");
  UIC_REQUIRE(b->fc_feats && b->att_feats, "prepare_feature: batch needs fc_feats and att_feats");
  hipStream_t s = (hipStream_t)stream;
  const Layout L = make_layout(*d, workspace);
  const Derived dv = make_derived(*d, w, (void*)derived);
  const void *fc_in, *att_in;
  const float drop_p = (training & 1) ? d->drop_p : 0.f;
  UIC_TRY(prepare_features(*d, w, dv, b, L, training, drop_p, seed, &fc_in, &att_in, s));
  const size_t N = d->N, R = d->R, H = d->H, A = d->A;
  UIC_TRY(uic_to_f32_launch(d->dtype, L.fcp, fc_out, N * H, s));
  UIC_TRY(uic_to_f32_launch(d->dtype, L.attp, att_out, N * R * H, s));
  return uic_to_f32_launch(d->dtype, L.patt, p_att_out, N * R * A, s);
}

}  // extern "C"
