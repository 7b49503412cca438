// The pivot NMT step's workspace layout and its size / pointer queries, the per-device side stream, and the parts of struct Nmt
// that prepare a step: init, the weight refresh (operand-dtype and transposed copies) and the zero-initialised buffers.
#include "nmt_internal.h"
#include <mutex>

namespace nmt {

NmtLayout nmt_layout(const uic_nmt_dims& d, const uic_nmt_weights* w, void* ws) {
  NmtLayout L;
  memset(&L, 0, sizeof(L));
  Bump b{(char*)ws, 0};
  const size_t Sz = uic_dtype_size(d.dtype);
  const size_t B = d.B, S = d.S, Td = d.T - 1, H = d.H, W = d.W, Hd = H / 2, NL = d.layers, Vt = d.Vt, Vtp = vpad(Vt);
  const bool bf = d.dtype == UIC_BF16;
  auto wcopy = [&](const float* master, size_t n, void** copy) -> const void* {
    *copy = b.take(n * Sz);
    return (bf || !w) ? *copy : (const void*)master;
  };
  L.enc_lin_w = wcopy(w ? w->enc_lin_w : nullptr, W * W, &L.c_enc_lin_w);
  for (size_t l = 0; l < NL; ++l) {
    const size_t in = l == 0 ? W : H, din = l == 0 ? W + H : H;
    for (int dd = 0; dd < 2; ++dd) {
      L.enc_w_ih[l][dd] = wcopy(w ? w->enc_w_ih[l][dd] : nullptr, 4 * Hd * in, &L.c_enc_w_ih[l][dd]);
      L.enc_w_hh[l][dd] = wcopy(w ? w->enc_w_hh[l][dd] : nullptr, 4 * Hd * Hd, &L.c_enc_w_hh[l][dd]);
      L.enc_w_ihT[l][dd] = b.take(in * 4 * Hd * Sz);
      L.enc_w_hhT[l][dd] = b.take(Hd * 4 * Hd * Sz);
    }
    L.dec_w_ih[l] = wcopy(w ? w->dec_w_ih[l] : nullptr, 4 * H * din, &L.c_dec_w_ih[l]);
    L.dec_w_hh[l] = wcopy(w ? w->dec_w_hh[l] : nullptr, 4 * H * H, &L.c_dec_w_hh[l]);
    L.dec_wT[l] = b.take((din + H) * 4 * H * Sz);
  }
  L.attn_in_w = wcopy(w ? w->attn_in_w : nullptr, H * H, &L.c_attn_in_w);
  L.attn_out_w = wcopy(w ? w->attn_out_w : nullptr, H * 2 * H, &L.c_attn_out_w);
  L.gen_w = wcopy(w ? w->gen_w : nullptr, Vt * H, &L.c_gen_w);
  L.enc_lin_wT = b.take(W * W * Sz);
  L.attn_in_wT = b.take(H * H * Sz);
  L.attn_out_wT = b.take(2 * H * H * Sz);
  L.gen_wT = b.take(H * Vtp * Sz);
  L.xe = b.take(S * B * W * Sz);
  for (size_t l = 0; l <= NL; ++l) L.xl[l] = b.take((S + 2) * B * (l == 0 ? W : H) * Sz);
  for (size_t l = 1; l < NL; ++l) L.xd[l] = b.take((S + 2) * B * H * Sz);
  for (size_t l = 0; l < NL; ++l)
    for (int dd = 0; dd < 2; ++dd) {
      L.gx_e[l][dd] = (float*)b.take(S * B * 4 * Hd * 4);
      L.c_e[l][dd] = (float*)b.take((S + 2) * B * Hd * 4);
      L.gates_e[l][dd] = b.take(S * B * 4 * Hd * Sz);
      L.dg_e[l][dd] = b.take(S * B * 4 * Hd * Sz);
    }
  L.target_bt = (int64_t*)b.take(B * Td * 8);
  L.mask_bt = (float*)b.take(B * Td * 4);
  L.tgt_in = (int64_t*)b.take(Td * B * 8);
  L.emb_d = b.take(Td * B * W * Sz);
  L.gx_d0 = (float*)b.take(Td * B * 4 * H * 4);
  for (size_t l = 0; l < NL; ++l) {
    L.hd[l] = b.take((Td + 1) * B * H * Sz);
    L.cd[l] = (float*)b.take((Td + 1) * B * H * 4);
    L.hdrop[l] = b.take(Td * B * H * Sz);
    L.gates_d[l] = b.take(Td * B * 4 * H * Sz);
    L.dg_d[l] = b.take(Td * B * 4 * H * Sz);
    L.dhrec_d[l] = (float*)b.take(B * H * 4);
    L.dcd[l] = (float*)b.take(B * H * 4);
  }
  L.ctxw = (float*)b.take(S * B * H * 4);
  L.dctxw = b.take(S * B * H * Sz);
  L.attn_all = (float*)b.take(Td * B * S * 4);
  L.cvec_all = b.take(Td * B * H * Sz);
  L.out_pre = b.take(Td * B * H * Sz);
  const size_t Mdp = nmt_gen_rows(Td * B);             // (the generator's rows with their zero padding)
  L.out_all = b.take(((Td + 1) * B + (Mdp - Td * B)) * H * Sz);
  L.logits = (float*)b.take(Mdp * Vtp * 4);            // (Mdp rows: the live-position list is padded to whole 128-row tiles)
  L.dlogits = b.take(Mdp * Vtp * Sz);
  L.out_live = b.take(Mdp * H * Sz);                   // uic_nmt_dims.tgt_live_rows: the listed rows of `out_all`, their d out
  L.d_out_live = (float*)b.take(Mdp * H * 4);
  L.live_map = (int*)b.take(Mdp * 4);                  // the list made on the device (tgt_live_rows == NULL)
  L.row_loss = (float*)b.take(Td * B * 4);
  L.scalars = (float*)b.take(64);
  L.stats = (int*)b.take(64);
  L.d_out_all = (float*)b.take(Td * B * H * 4);
  L.dfeed = (float*)b.take(B * 2 * H * 4);
  L.d_pre_all = b.take(Td * B * H * Sz);
  L.d_cq_all = (float*)b.take(Td * B * 2 * H * 4);
  L.dscore_all = (float*)b.take(Td * B * S * 4);
  L.dq = (float*)b.take(B * H * 4);
  for (int l = 0; l < ML; ++l) L.dx_lstm[l] = (float*)b.take(B * 2 * H * 4);
  L.d_lay = (float*)b.take(S * B * H * 4);
  L.dhrec_e = (float*)b.take(B * Hd * 4);
  L.dc_e = (float*)b.take(B * Hd * 4);
  L.dhrec_e1 = (float*)b.take(B * Hd * 4);
  L.dc_e1 = (float*)b.take(B * Hd * 4);
  L.dx_e = (float*)b.take(S * B * (W > H ? W : H) * 4);
  L.dpre_e = b.take(S * B * W * Sz);
  L.dxe = (float*)b.take(S * B * W * 4);
  L.demb_d = (float*)b.take(Td * B * W * 4);
  const size_t rows = rup8((S > Td ? S : Td) * B) > Mdp ? rup8((S > Td ? S : Td) * B) : Mdp;   // (the generator's padded rows: the transposing fallback of wgrad_group)
  L.tA = b.take((Vt > 4 * H ? Vt : 4 * H) * rows * Sz);
  L.tB = b.take((W + 2 * H) * rows * Sz);
  const size_t maxcols = Vtp > 4 * H ? Vtp : 4 * H;
  L.colscratch_floats = 128 * maxcols;
  L.colscratch = (float*)b.take(L.colscratch_floats * 4);
  L.slab_bytes = 4 * (4 * H) * (W + 2 * H) * 4;
  L.slab = (float*)b.take(L.slab_bytes);
  L.rnn_sync = (unsigned*)b.take((2 * NL + 2) * uic_rnn_persist_sync_bytes());   // one block per persistent launch of a step (sync_block)
  L.dfeed_x = (float*)b.take(Td * B * H * 4);
  L.dq_att_x = (float*)b.take(Td * B * H * 4);
  L.dec_bwd_dbg = (unsigned long long*)b.take((size_t)256 * Td * 16 * 8);
  L.dec_fwd_dbg = (unsigned long long*)b.take((size_t)256 * Td * 16 * 8);
  {
    const size_t es = uic_embed_bwd_sorted_scratch_ints((int)(S * B), 1, d.Vs, (int)W), ed = uic_embed_bwd_sorted_scratch_ints((int)(Td * B), 1, d.Vt, (int)W);
    L.embed_scratch = (int*)b.take((es > ed ? es : ed) * 4);
  }
  L.total = (b.off + 255) & ~(size_t)255;
  return L;
}

int nmt_check(const uic_nmt_dims* d) {
  UIC_REQUIRE(d != nullptr, "null dims");
  UIC_REQUIRE(d->dtype == UIC_F32 || d->dtype == UIC_BF16, "bad dtype %d", d->dtype);
  UIC_REQUIRE(d->B > 0 && d->S > 0 && d->S <= 4096 && d->T >= 2 && d->Vs > 1 && d->Vt > 1, "bad sizes B=%d S=%d T=%d", d->B, d->S, d->T);
  UIC_REQUIRE(d->layers >= 1 && d->layers <= ML, "layers=%d outside [1,%d]", d->layers, ML);
  UIC_REQUIRE(d->H % 16 == 0 && d->W % 8 == 0, "rnn_size=%d must be a multiple of 16, word_vec_size=%d of 8", d->H, d->W);
  UIC_REQUIRE(d->T - 1 < 256, "target length %d too long for the dropout site encoding", d->T);
  UIC_REQUIRE(d->drop_p >= 0.f && d->drop_p < 1.f, "dropout=%f outside [0,1)", (double)d->drop_p);
  return UIC_OK;
}

namespace {
NmtSide g_nmt_side[16];
std::mutex g_nmt_side_mutex;
}  // namespace
int nmt_side(NmtSide** out) {
  int dev = 0;
  UIC_TRY(uic_check_hip(hipGetDevice(&dev), "hipGetDevice"));
  UIC_REQUIRE(dev >= 0 && dev < 16, "device index %d out of range", dev);
  NmtSide& ss = g_nmt_side[dev];
  std::lock_guard<std::mutex> lock(g_nmt_side_mutex);
  if (!ss.ready) {
    UIC_TRY(uic_check_hip(hipStreamCreateWithFlags(&ss.stream, hipStreamNonBlocking), "hipStreamCreateWithFlags"));
    for (hipEvent_t* ev : {&ss.ev_go, &ss.ev_done, &ss.ev_r0, &ss.ev_gen, &ss.ev_grad_gen, &ss.ev_grad_dec})
      UIC_TRY(uic_check_hip(hipEventCreateWithFlags(ev, hipEventDisableTiming), "hipEventCreate"));
    ss.ready = true;
  }
  *out = &ss;
  return UIC_OK;
}

int Nmt::init(const uic_nmt_dims* d_, const uic_nmt_weights* w_, const int64_t* src_, const int32_t* lengths_host, const int64_t* tgt_,
              int training, unsigned seed_, void* ws, const uic_nmt_weights* G_) {
  d = *d_; w = w_; G = G_; src = src_; tgt = tgt_;
  L = nmt_layout(d, w, ws);
  dt = d.dtype; B = d.B; S = d.S; Td = d.T - 1; H = d.H; W = d.W; Hd = H / 2; NL = d.layers; Vs = d.Vs; Vt = d.Vt;
  Vtp = (int)vpad(Vt);
  Sz = uic_dtype_size(dt); BH = (size_t)B * H; BHd = (size_t)B * Hd;
  drop_p = training ? d.drop_p : 0.f;
  seed = seed_;
  live = d.tgt_live_count > 0 && d.tgt_live_count <= Td * B && ((size_t)H * Sz) % 16 == 0;
  live_n = live ? d.tgt_live_count : 0;
  live_pad = (live_n + 127) & ~127;
  live_rows = !live ? nullptr : d.tgt_live_rows ? d.tgt_live_rows : L.live_map;
  for (int b = 0; b < B; ++b) {
    UIC_REQUIRE(lengths_host[b] >= 1 && lengths_host[b] <= S, "lengths[%d]=%d outside [1,%d]", b, lengths_host[b], S);
    UIC_REQUIRE(b == 0 || lengths_host[b] <= lengths_host[b - 1], "lengths must be sorted in decreasing order (pack_padded_sequence)");
  }
  for (int st = 0; st < S; ++st) {
    int n = 0;
    while (n < B && lengths_host[n] > st) ++n;
    nb[st] = n;
  }
  return UIC_OK;
}

int Nmt::wait_gen(hipStream_t s) {
  if (!gen_pending) return UIC_OK;
  gen_pending = false;
  NmtSide* ss = nullptr;
  UIC_TRY(nmt_side(&ss));
  return uic_check_hip(hipStreamWaitEvent(s, ss->ev_gen, 0), "hipStreamWaitEvent(generator copies)");
}

int Nmt::refresh(hipStream_t s) {
  // operand-dtype copies and transposes of the weights, a handful of multi-tensor launches instead of one per tensor
  // (the step is a chain of small launches: 34 of them were this)
  {
    NmtSide* ss = nullptr;
    UIC_TRY(nmt_side(&ss));
    UIC_TRY(uic_check_hip(hipEventRecord(ss->ev_r0, s), "hipEventRecord"));            // the master weights are final
    UIC_TRY(uic_check_hip(hipStreamWaitEvent(ss->stream, ss->ev_r0, 0), "hipStreamWaitEvent"));
    if (dt == UIC_BF16) UIC_TRY(uic_cast_f32_launch(dt, w->gen_w, L.c_gen_w, (size_t)Vt * H, ss->stream));   // (25.6 M elements: a launch of its own)
    UIC_TRY(uic_transpose_launch(dt, L.gen_w, Vt, H, H, L.gen_wT, Vtp, ss->stream));
    UIC_TRY(uic_check_hip(hipEventRecord(ss->ev_gen, ss->stream), "hipEventRecord"));
    gen_pending = true;
  }
  if (dt == UIC_BF16) {
    const float* src[UIC_CAST_MULTI]; void* dst[UIC_CAST_MULTI]; size_t n[UIC_CAST_MULTI];
    int k = 0;
    auto flush = [&]() -> int { if (k) UIC_TRY(uic_cast_f32_multi_launch(dt, k, src, dst, n, s)); k = 0; return UIC_OK; };
    auto add = [&](const float* a, const void* b, size_t cnt) -> int {
      src[k] = a; dst[k] = (void*)b; n[k] = cnt;
      if (++k == UIC_CAST_MULTI) return flush();
      return UIC_OK;
    };
    UIC_TRY(add(w->enc_lin_w, L.c_enc_lin_w, (size_t)W * W));
    for (int l = 0; l < NL; ++l) {
      const int in = l == 0 ? W : H, din = l == 0 ? W + H : H;
      for (int dd = 0; dd < 2; ++dd) {
        UIC_TRY(add(w->enc_w_ih[l][dd], L.c_enc_w_ih[l][dd], (size_t)4 * Hd * in));
        UIC_TRY(add(w->enc_w_hh[l][dd], L.c_enc_w_hh[l][dd], (size_t)4 * Hd * Hd));
      }
      UIC_TRY(add(w->dec_w_ih[l], L.c_dec_w_ih[l], (size_t)4 * H * din));
      UIC_TRY(add(w->dec_w_hh[l], L.c_dec_w_hh[l], (size_t)4 * H * H));
    }
    UIC_TRY(add(w->attn_in_w, L.c_attn_in_w, (size_t)H * H));
    UIC_TRY(add(w->attn_out_w, L.c_attn_out_w, (size_t)H * 2 * H));
    UIC_TRY(flush());
  }
  {
    UicTransposeJob jobs[UIC_TRANSPOSE_MULTI];
    int k = 0;
    auto flush = [&]() -> int { if (k) UIC_TRY(uic_transpose_multi_launch(dt, k, jobs, s)); k = 0; return UIC_OK; };
    auto add = [&](const void* src, int rows, int cols, int lds, void* dst, int ldd) -> int {
      jobs[k] = UicTransposeJob{src, dst, rows, cols, lds, ldd};
      if (++k == UIC_TRANSPOSE_MULTI) return flush();
      return UIC_OK;
    };
    UIC_TRY(add(L.enc_lin_w, W, W, W, L.enc_lin_wT, W));
    for (int l = 0; l < NL; ++l) {
      const int in = l == 0 ? W : H, din = l == 0 ? W + H : H;
      for (int dd = 0; dd < 2; ++dd) {
        UIC_TRY(add(L.enc_w_ih[l][dd], 4 * Hd, in, in, L.enc_w_ihT[l][dd], 4 * Hd));
        UIC_TRY(add(L.enc_w_hh[l][dd], 4 * Hd, Hd, Hd, L.enc_w_hhT[l][dd], 4 * Hd));
      }
      UIC_TRY(add(L.dec_w_ih[l], 4 * H, din, din, L.dec_wT[l], 4 * H));
      UIC_TRY(add(L.dec_w_hh[l], 4 * H, H, H, offw(L.dec_wT[l], (size_t)din * 4 * H, dt), 4 * H));
    }
    UIC_TRY(add(L.attn_in_w, H, H, H, L.attn_in_wT, H));
    UIC_TRY(add(L.attn_out_w, H, 2 * H, 2 * H, L.attn_out_wT, H));
    UIC_TRY(flush());
  }
  return UIC_OK;
}

int Nmt::zero_forward_buffers(hipStream_t s) {
  void* ptr[4 * UIC_NMT_MAX_LAYERS + 4];
  size_t nbytes[4 * UIC_NMT_MAX_LAYERS + 4];
  int n = 0;
  auto add = [&](void* q, size_t by) { ptr[n] = q; nbytes[n] = (by + 15) & ~(size_t)15; ++n; };
  for (int l = 0; l < NL; ++l) {
    add(L.xl[l + 1], (size_t)(S + 2) * BH * Sz);
    for (int dd = 0; dd < 2; ++dd) add(L.c_e[l][dd], (size_t)(S + 2) * BHd * 4);
    if (l + 1 < NL && drop_p > 0.f) add(L.xd[l + 1], (size_t)(S + 2) * BH * Sz);
  }
  add(L.out_all, BH * Sz);                                         // init_input_feed: zeros (:454-458)
  add(sync_block(0), (size_t)(NL + 1) * uic_rnn_persist_sync_bytes());
  return uic_zero_list_launch(ptr, nbytes, n, s);
}

int Nmt::zero_backward_buffers(hipStream_t s) {
  void* ptr[2 * UIC_NMT_MAX_LAYERS + 5];
  size_t nbytes[2 * UIC_NMT_MAX_LAYERS + 5];
  int n = 0;
  if (live) { ptr[n] = L.d_out_all; nbytes[n] = (size_t)Td * B * H * 4; ++n; }
  for (int l = 0; l < NL; ++l)
    for (int dd = 0; dd < 2; ++dd) { ptr[n] = L.dg_e[l][dd]; nbytes[n] = ((size_t)S * B * 4 * Hd * Sz + 15) & ~(size_t)15; ++n; }
  ptr[n] = sync_block(NL + 1); nbytes[n] = (size_t)(NL + 1) * uic_rnn_persist_sync_bytes(); ++n;
  const size_t pad = gen_rows() - (size_t)Td * B;      // zero rows behind the generator weight gradient's operands (nmt_layout)
  if (pad) {
    ptr[n] = offw(L.dlogits, (size_t)Td * B * Vtp, dt); nbytes[n] = pad * Vtp * Sz; ++n;
    ptr[n] = offw(L.out_all, (size_t)(Td + 1) * B * H, dt); nbytes[n] = pad * H * Sz; ++n;
  }
  return uic_zero_list_launch(ptr, nbytes, n, s);
}

}  // namespace nmt

extern "C" {

size_t uic_nmt_workspace_bytes(const uic_nmt_dims* d) {
  if (nmt::nmt_check(d)) return 0;
  return nmt::nmt_layout(*d, nullptr, nullptr).total;
}

void* uic_nmt_workspace_ptr(const uic_nmt_dims* d, void* workspace, const char* name) {
  if (nmt::nmt_check(d) || !workspace || !name) return nullptr;
  const nmt::NmtLayout L = nmt::nmt_layout(*d, nullptr, workspace);
  struct { const char* n; void* p; } tab[] = {{"dec_bwd_dbg", L.dec_bwd_dbg}, {"dec_fwd_dbg", L.dec_fwd_dbg}, {"d_cq", L.d_cq_all}, {"dscore", L.dscore_all}, {"d_pre", L.d_pre_all}};
  for (auto& e : tab)
    if (!strcmp(e.n, name)) return e.p;
  return nullptr;
}

}  // extern "C"
