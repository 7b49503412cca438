// The pivot NMT training step: encoder, decoder and loss forward, the backward pass as a sequence of named steps, and the C entry
// points uic_nmt_forward_loss / uic_nmt_backward / uic_nmt_grad_ready_wait.  Each recurrence has two forms chosen by one
// predicate of Nmt: ONE persistent launch (nmt_persist.hip) or the launch chain.  No kernel here (nmt_kernels.hip).
#include "nmt_internal.h"

namespace nmt {

// W_ih x + b_ih + b_hh of encoder layer l, direction dd, for every (s, b)
UicGemmParams Nmt::enc_gx_gemm(int l, int dd) const {
  const int in = l == 0 ? W : H;
  UicGemmParams g = gemm_base(dt, S * B, 4 * Hd);
  add_seg(g, enc_in(l), in, L.enc_w_ih[l][dd], in, in);
  g.C = L.gx_e[l][dd]; g.ldc = 4 * Hd; g.bias = w->enc_b_ih[l][dd]; g.bias2 = w->enc_b_hh[l][dd]; g.flags = UIC_GEMM_OUT_F32;
  return g;
}

UicGemmParams Nmt::linear_out_gemm(const void* cvec, const void* q, void* out_pre, void* out, unsigned site) const {
  UicGemmParams g = gemm_base(dt, B, H);
  add_seg(g, cvec, H, L.attn_out_w, 2 * H, H);
  add_seg(g, q, H, off(L.attn_out_w, H, dt), 2 * H, H);
  if (out_pre) { g.C_pre = out_pre; g.ldc_pre = H; }
  g.C = out; g.ldc = H; g.flags = UIC_GEMM_TANH;
  g.drop_p = drop_p; g.seed = seed; g.site = site;
  return g;
}

UicGemmParams Nmt::generator_gemm(int rows, const void* x, float* logits) const {
  UicGemmParams g = gemm_base(dt, rows, Vt);
  add_seg(g, x, H, L.gen_w, H, H);
  g.C = logits; g.ldc = Vtp; g.bias = w->gen_b; g.flags = UIC_GEMM_OUT_F32;
  return g;
}

// what the forward and the backward persistent launch of encoder layer l share; `block`: the launch's sync block
void Nmt::enc_params(UicNmtEncParams& p, int l, int block) const {
  memset(&p, 0, sizeof(p));
  p.B = B; p.S = S;
  for (int st = 0; st < S; ++st) p.nb[st] = nb[st];
  for (int dd = 0; dd < 2; ++dd) { p.c[dd] = L.c_e[l][dd]; p.gates[dd] = L.gates_e[l][dd]; }
  persist_tail(p, block);
}

// both directions' S recurrent steps as ONE persistent launch (nmt_persist.hip) behind the two batched input GEMMs
int Nmt::enc_layer_persist(int l, hipStream_t s) {
  UicNmtEncParams p;
  enc_params(p, l, l);
  p.x_out = L.xl[l + 1];
  for (int dd = 0; dd < 2; ++dd) {
    UIC_TRY(uic_gemm_launch(enc_gx_gemm(l, dd), s));
    p.w_hh[dd] = L.enc_w_hh[l][dd]; p.gx[dd] = L.gx_e[l][dd];
  }
  return uic_nmt_enc_fwd_persist_launch(p, s);
}

int Nmt::enc_layer_chain(int l, hipStream_t s) {
  // the layer's input and the zeroed output buffer are ready: the backward direction runs on the side stream
  NmtSide* ss = nullptr;
  UIC_TRY(nmt_side(&ss));
  UIC_TRY(uic_check_hip(hipEventRecord(ss->ev_go, s), "hipEventRecord"));
  UIC_TRY(uic_check_hip(hipStreamWaitEvent(ss->stream, ss->ev_go, 0), "hipStreamWaitEvent"));
  for (int dd = 1; dd >= 0; --dd) {
    hipStream_t sd = dd == 1 ? ss->stream : s;
    UIC_TRY(uic_gemm_launch(enc_gx_gemm(l, dd), sd));
    for (int k = 0; k < S; ++k) {
      const int st = dd == 0 ? k : S - 1 - k;          // time step; its slot is st + 1
      const int prev = dd == 0 ? st : st + 2;          // slot of the previous state in this direction
      if (nb[st] == 0) continue;                       // S longer than the longest sentence
      UicGemmParams g = gemm_base(dt, nb[st], 4 * Hd);
      g.lstm = 1; g.H = Hd;
      add_seg(g, off(L.xl[l + 1], (size_t)prev * BH + dd * Hd, dt), H, L.enc_w_hh[l][dd], Hd, Hd);
      g.pre1 = L.gx_e[l][dd] + (size_t)st * B * 4 * Hd; g.ldpre1 = 4 * Hd;
      g.c_prev = L.c_e[l][dd] + (size_t)prev * BHd; g.c_out = L.c_e[l][dd] + (size_t)(st + 1) * BHd;
      g.h_out = offw(L.xl[l + 1], (size_t)(st + 1) * BH + dd * Hd, dt); g.ldh = H;
      g.gates_out = offw(L.gates_e[l][dd], (size_t)st * B * 4 * Hd, dt);
      UIC_TRY(uic_gemm_launch(g, sd));
    }
    if (dd == 1) UIC_TRY(uic_check_hip(hipEventRecord(ss->ev_done, sd), "hipEventRecord"));
  }
  return uic_check_hip(hipStreamWaitEvent(s, ss->ev_done, 0), "hipStreamWaitEvent");
}

int Nmt::encoder_fwd(const int32_t* lengths_dev, hipStream_t s) {
  UIC_TRY(zero_forward_buffers(s));
  // relu(linear(word_lut[src]))  (NMT_Models.py:63-67)
  UIC_TRY(uic_embed_fwd_launch(dt, w->enc_lut, Vs, W, src, 1, S * B, 1, 0.f, 0, 0, 0, 0, L.xe, s));
  {
    UicGemmParams g = gemm_base(dt, S * B, W);
    add_seg(g, L.xe, W, L.enc_lin_w, W, W);
    g.C = offw(L.xl[0], (size_t)B * W, dt); g.ldc = W; g.bias = w->enc_lin_b; g.flags = UIC_GEMM_RELU;
    UIC_TRY(uic_gemm_launch(g, s));
  }
  const bool persist = enc_persist();
  for (int l = 0; l < NL; ++l) {
    UIC_TRY(persist ? enc_layer_persist(l, s) : enc_layer_chain(l, s));
    if (l + 1 < NL && drop_p > 0.f)  // nn.LSTM's inter-layer dropout (element index over the [S*B, H] slots 1..S)
      UIC_TRY(nmt_dropout_apply_launch(dt, off(L.xl[l + 1], BH, dt), offw(L.xd[l + 1], BH, dt), (size_t)S * BH, drop_p, seed, SITE_NMT_ENC(l), s));
  }
  // decoder initial state (_fix_enc_hidden + init_decoder_state, :284-295): slot 0 of the decoder state buffers
  for (int l = 0; l < NL; ++l)
    UIC_TRY(nmt_enc_final_launch(dt, L.xl[l + 1], L.c_e[l][0], L.c_e[l][1], lengths_dev, B, H, Hd, L.hd[l], L.cd[l], s));
  return UIC_OK;
}

// the whole target-step loop as ONE persistent launch (nmt_persist.hip): same buffers, same dropout sites
int Nmt::decoder_persist(hipStream_t s) {
  UicNmtDecParams p;
  memset(&p, 0, sizeof(p));
  p.B = B; p.S = S; p.Td = Td; p.NL = NL;
  p.out_all = L.out_all; p.out_pre = L.out_pre; p.gx_d0 = L.gx_d0;
  for (int l = 0; l < NL; ++l) {
    p.hd[l] = L.hd[l]; p.cd[l] = L.cd[l]; p.hdrop[l] = L.hdrop[l]; p.gates_d[l] = L.gates_d[l];
    p.w_ih[l] = l == 0 ? off(L.dec_w_ih[0], W, dt) : L.dec_w_ih[l]; p.ld_ih[l] = l == 0 ? W + H : H;
    p.w_hh[l] = L.dec_w_hh[l];
    p.b_ih[l] = w->dec_b_ih[l]; p.b_hh[l] = w->dec_b_hh[l];
  }
  p.ctx = context(); p.ctxw = L.ctxw; p.attn_all = L.attn_all; p.cvec_all = L.cvec_all; p.attn_out_w = L.attn_out_w;
  p.drop_p = drop_p; p.seed = seed;
  persist_tail(p, NL);
  p.dbg = (d.recurrence & UIC_REC_STAMPS) ? L.dec_fwd_dbg : nullptr;
  return uic_nmt_dec_persist_launch(p, s);
}

int Nmt::decoder_chain(hipStream_t s) {
  const int H4 = 4 * H;
  for (int t = 0; t < Td; ++t) {
    const void* x = nullptr;
    for (int l = 0; l < NL; ++l) {                           // StackedLSTM.forward (StackedRNN.py:20-34)
      UicGemmParams g = gemm_base(dt, B, H4);
      g.lstm = 1; g.H = H;
      if (l == 0) {
        add_seg(g, off(L.out_all, (size_t)t * BH, dt), H, off(L.dec_w_ih[0], W, dt), W + H, H);   // input feed (:248-249)
        g.pre1 = L.gx_d0 + (size_t)t * B * H4; g.ldpre1 = H4;
      } else {
        add_seg(g, x, H, L.dec_w_ih[l], H, H);
        g.bias = w->dec_b_ih[l]; g.bias2 = w->dec_b_hh[l];
      }
      add_seg(g, off(L.hd[l], (size_t)t * BH, dt), H, L.dec_w_hh[l], H, H);
      g.c_prev = L.cd[l] + (size_t)t * BH; g.c_out = L.cd[l] + (size_t)(t + 1) * BH;
      g.h_out = offw(L.hd[l], (size_t)(t + 1) * BH, dt); g.ldh = H;
      g.gates_out = offw(L.gates_d[l], (size_t)t * B * H4, dt);
      if (l + 1 < NL) {                                      // dropout between layers only
        g.h_drop = offw(L.hdrop[l], (size_t)t * BH, dt); g.ldhd = H;
        g.drop_p = drop_p; g.seed = seed; g.site = SITE_NMT_DEC(l, t);
        x = g.h_drop;
      }
      UIC_TRY(uic_gemm_launch(g, s));
    }
    const void* q = off(L.hd[NL - 1], (size_t)(t + 1) * BH, dt);       // rnn_output = top layer's h
    // scores = context . linear_in(rnn_output) (GlobalAttention.py:114-116) = (context W_in) . rnn_output: L.ctxw was
    // made once before the loop, so no linear_in GEMM sits in the per-step chain
    UIC_TRY(nmt_gattn_fwd_launch(dt, context(), nullptr, S, B, H, L.attn_all + (size_t)t * B * S, offw(L.cvec_all, (size_t)t * BH, dt), nullptr,
                                 L.ctxw, q, s));
    // output = dropout(attn_output) = next step's input feed (NMT_Models.py:258-259): the epilogue writes both the
    // tanh output (kept for the backward pass) and its dropped copy
    UIC_TRY(uic_gemm_launch(linear_out_gemm(off(L.cvec_all, (size_t)t * BH, dt), q, offw(L.out_pre, (size_t)t * BH, dt),
                                            offw(L.out_all, (size_t)(t + 1) * BH, dt), SITE_NMT_OUT(t)), s));
  }
  return UIC_OK;
}

int Nmt::decoder_fwd(hipStream_t s) {
  UIC_TRY(nmt_prep_launch(tgt, Td + 1, B, L.target_bt, L.mask_bt, L.tgt_in, s));
  UIC_TRY(uic_embed_fwd_launch(dt, w->dec_lut, Vt, W, L.tgt_in, 1, Td * B, 1, 0.f, 0, 0, 0, 0, L.emb_d, s));
  {  // layer-0 input projection of the embedding part for all steps (the input-feed part stays in the loop)
    UicGemmParams g = gemm_base(dt, Td * B, 4 * H);
    add_seg(g, L.emb_d, W, L.dec_w_ih[0], W + H, W);
    g.C = L.gx_d0; g.ldc = 4 * H; g.bias = w->dec_b_ih[0]; g.bias2 = w->dec_b_hh[0]; g.flags = UIC_GEMM_OUT_F32;
    UIC_TRY(uic_gemm_launch(g, s));
  }
  {  // ctxw[s, b, :] = context[s, b, :] W_in, all source positions at once (see gattn_fwd_kernel)
    UicGemmParams g = gemm_base(dt, S * B, H);
    add_seg(g, context(), H, L.attn_in_wT, H, H);
    g.C = L.ctxw; g.ldc = H; g.flags = UIC_GEMM_OUT_F32;
    UIC_TRY(uic_gemm_launch(g, s));
  }
  return dec_persist() ? decoder_persist(s) : decoder_chain(s);
}

// generator + NMTCriterion + NMT_loss.score (criterion.py:126-136,175-184)
int Nmt::loss_fwd(float* loss_out, int32_t* stats_out, hipStream_t s) {
  UIC_TRY(wait_gen(s));
  if (live && !d.tgt_live_rows) UIC_TRY(uic_live_list_launch(L.mask_bt, Td, 0, B, Td * B, L.live_map, live_pad, s));   // (mask_bt: nmt_prep_kernel, this stream)
  if (live) UIC_TRY(uic_gather_rows_launch(off(L.out_all, BH, dt), live_rows, Td * B, L.out_live, live_n, live_pad, (size_t)H * Sz, s));
  if (!live || live_pad > 0)
    UIC_TRY(uic_gemm_launch(generator_gemm(live ? live_pad : Td * B, live ? L.out_live : off(L.out_all, BH, dt), L.logits), s));
  UIC_TRY(nmt_fill_f32_launch(L.scalars, 1.0f, 1, s));      // size_average=False: no denominator
  UicXeParams x;
  memset(&x, 0, sizeof(x));
  x.dtype = dt; x.M = Td * B; x.V1 = Vt; x.ldv = Vtp; x.logits = L.logits; x.dlogits = L.dlogits; x.N = B;
  x.target = L.target_bt; x.ldtarget = Td; x.target_col0 = 0;
  x.mask = L.mask_bt; x.ldmask = Td; x.mask_col0 = 0;             // weight[PAD] = 0
  x.inv_den = L.scalars; x.row_loss = L.row_loss; x.write_grad = 1;
  if (stats_out) {       // NMT_loss.score's counters ride on the criterion kernel's pass over the logits
    UIC_TRY(uic_fill_launch(L.stats, 0, 8, s));
    x.score_stats = L.stats;
  }
  if (live) { x.M = live_pad; x.row_map = live_rows; x.row_map_limit = Td * B; }   // (rows of logits / d logits / row_loss by list position)
  UIC_TRY(uic_xe_launch(x, s));
  UIC_TRY(uic_reduce_sum_launch(L.row_loss, live ? (size_t)live_n : (size_t)Td * B, nullptr, loss_out, s));
  if (stats_out) {
    UIC_TRY(uic_copy_launch(stats_out, L.stats, 8, s));
  }
  return UIC_OK;
}

// ---- generator: d out = d logits W_gen
int Nmt::bwd_gen_dout(hipStream_t s) {
  const int Md = Td * B;
  // [T B, H] outputs over K = the target vocabulary -- few tiles and a very long reduction: split-K over workgroups with the
  // deterministic slab reduction (wgrad_multi; one launch of 64 x 64 tiles walked all 50 048 columns in 347 us)
  const WDest d1{live ? L.d_out_live : L.d_out_all, (int)H, 0, (int)H};
  // (d out of the positions the list leaves out is zero: zero_backward_buffers cleared the buffer; the split-K reduce places
  // the listed rows itself, a direct GEMM leaves compact rows to scatter)
  WRows wr{live_rows, live_n, Md, L.d_out_all, (int)H, false};
  if (!live || live_pad > 0) UIC_TRY(wgrad_multi(L.slab, L.slab_bytes, dt, L.dlogits, live ? live_pad : Md, L.gen_wT, H, Vtp, &d1, 1, s, false, live ? &wr : nullptr));
  if (live && !wr.used) UIC_TRY(uic_scatter_rows_launch(L.d_out_live, live_rows, L.d_out_all, Md, live_n, (size_t)H * 4, s));
  return UIC_OK;
}

// The generator's weight / bias gradients (the largest GEMM of the backward pass, [Vt, H] over all target rows) need nothing
// from the BPTT loop and the loop -- ~6 dependent launches of 64 rows per step -- leaves the chip idle: they run on the side
// stream beside it and are joined (ev_done) before the main stream next touches the shared scratch buffers
int Nmt::bwd_gen_weights(NmtSide* ss, hipStream_t s) {
  UIC_TRY(uic_check_hip(hipEventRecord(ss->ev_go, s), "hipEventRecord"));
  UIC_TRY(uic_check_hip(hipStreamWaitEvent(ss->stream, ss->ev_go, 0), "hipStreamWaitEvent"));
  if (live && live_pad == 0) {
    // (a batch without a single target word: no gradient)
    UIC_TRY(uic_check_hip(hipMemsetAsync(G->gen_w, 0, (size_t)Vt * H * 4, ss->stream), "hipMemsetAsync(d generator.weight)"));
    UIC_TRY(uic_check_hip(hipMemsetAsync(G->gen_b, 0, (size_t)Vt * 4, ss->stream), "hipMemsetAsync(d generator.bias)"));
  } else {
    const UicGemmTnSeg seg{live ? L.out_live : off(L.out_all, BH, dt), H, H};
    const WDest d1{G->gen_w, H, 0, H};
    UIC_TRY(wgrad_group(L.slab, L.slab_bytes, dt, L.dlogits, Vtp, Vt, &seg, 1, live ? live_pad : (int)gen_rows(), &d1, 1, ss->stream, false, L.tA, L.tB));
    UIC_TRY(uic_colsum_launch(dt, L.dlogits, live ? live_pad : Td * B, Vt, Vtp, G->gen_b, L.colscratch, L.colscratch_floats, ss->stream));
  }
  UIC_TRY(uic_check_hip(hipEventRecord(ss->ev_done, ss->stream), "hipEventRecord"));
  return uic_check_hip(hipEventRecord(ss->ev_grad_gen, ss->stream), "hipEventRecord");   // gradient group 0: generator.*
}

// ---- decoder BPTT as ONE persistent launch (nmt_persist.hip) instead of 7 launches per step
int Nmt::bwd_dec_persist(hipStream_t s) {
  UicNmtDecBwdParams p;
  memset(&p, 0, sizeof(p));
  p.B = B; p.S = S; p.Td = Td;
  p.d_out_all = L.d_out_all; p.out_pre = L.out_pre; p.d_pre_all = L.d_pre_all; p.d_cq_all = L.d_cq_all;
  p.attn_all = L.attn_all; p.ctx = context(); p.ctxw = L.ctxw; p.dscore_all = L.dscore_all;
  for (int l = 0; l < 2; ++l) { p.gates_d[l] = L.gates_d[l]; p.cd[l] = L.cd[l]; p.dg_d[l] = L.dg_d[l]; p.dc_init[l] = L.dcd[l]; }
  p.woutT = L.attn_out_wT; p.w1T = L.dec_wT[1]; p.w0T = off(L.dec_wT[0], (size_t)W * 4 * H, dt);
  p.dfeed_x = L.dfeed_x; p.dq_att_x = L.dq_att_x;
  p.dh_init[0] = L.dfeed; p.dh_init[1] = L.dx_lstm[1];
  p.drop_p = drop_p; p.seed = seed;
  persist_tail(p, NL + 1);
  p.dbg = (d.recurrence & UIC_REC_STAMPS) ? L.dec_bwd_dbg : nullptr;
  return uic_nmt_dec_bwd_persist_launch(p, s);
}

// ---- decoder BPTT as the launch chain
int Nmt::bwd_dec_chain(hipStream_t s) {
  const int H4 = 4 * H;
  for (int l = 0; l < NL; ++l) {
    UIC_TRY(uic_fill_launch(L.dhrec_d[l], 0, BH * 4, s));
    UIC_TRY(uic_fill_launch(L.dcd[l], 0, BH * 4, s));
  }
  for (int t = Td - 1; t >= 0; --t) {
    const bool last = t == Td - 1;
    void* d_pre = offw(L.d_pre_all, (size_t)t * BH, dt);
    float* d_cq = L.d_cq_all + (size_t)t * B * 2 * H;
    UIC_TRY(nmt_tanh_drop_bwd_launch(dt, L.d_out_all + (size_t)t * BH, last ? nullptr : L.dfeed, 2 * H, H, off(L.out_pre, (size_t)t * BH, dt), (int)BH,
                                     drop_p, seed, SITE_NMT_OUT(t), d_pre, s));
    {  // d[c ; q] = d_pre W_out
      UicGemmParams g = gemm_base(dt, B, 2 * H);
      add_seg(g, d_pre, H, L.attn_out_wT, H, H);
      g.C = d_cq; g.ldc = 2 * H; g.flags = UIC_GEMM_OUT_F32;
      UIC_TRY(uic_gemm_launch(g, s));
    }
    // d q = d_cq[:, H:] (linear_out's share) + sum_s d_score[s] ctxw[s]: added by the attention kernel itself
    UIC_TRY(nmt_gattn_bwd_step_launch(dt, context(), L.attn_all + (size_t)t * B * S, d_cq, 2 * H, S, B, H, L.dscore_all + (size_t)t * B * S, L.ctxw,
                                      d_cq + H, 2 * H, s));
    for (int l = NL - 1; l >= 0; --l) {
      UicLstmBwdParams p;
      memset(&p, 0, sizeof(p));
      p.dtype = dt; p.M = B; p.H = H;
      if (l == NL - 1) { p.dh0 = d_cq + H; p.lddh0 = 2 * H; }
      else {                                               // gradient w.r.t. the dropped h of layer l (input of layer l+1)
        p.dh0 = L.dx_lstm[l + 1]; p.lddh0 = 2 * H;
        p.drop_p = drop_p; p.seed = seed; p.site = SITE_NMT_DEC(l, t);
      }
      if (!last) {       // d h_l(t) from step t + 1: layer 0 has its own buffer, layers > 0 read the second half of their dX
        if (l == 0) { p.dh1 = L.dfeed + H; p.lddh1 = 2 * H; }
        else { p.dh1 = L.dx_lstm[l] + H; p.lddh1 = 2 * H; }
      }
      p.dc = L.dcd[l]; p.gates = off(L.gates_d[l], (size_t)t * B * H4, dt);
      p.c_prev = L.cd[l] + (size_t)t * BH; p.c = L.cd[l] + (size_t)(t + 1) * BH;
      p.dgates = offw(L.dg_d[l], (size_t)t * B * H4, dt);
      UIC_TRY(uic_lstm_bwd_launch(p, s));
      // l > 0: d[x_l | h_l_prev] = dG [W_ih | W_hh].  Layer 0: d[feed | h_0_prev] = dG [W_ih[:, W:] | W_hh] in ONE GEMM (rows
      // W .. W + 2H of dec_wT[0] are contiguous; the embedding part is batched later): L.dfeed is [B, 2H] = [d feed | d h_0(t-1)]
      UicGemmParams g = gemm_base(dt, B, 2 * H);
      add_seg(g, p.dgates, H4, l > 0 ? L.dec_wT[l] : off(L.dec_wT[0], (size_t)W * H4, dt), H4, H4);
      g.C = l > 0 ? L.dx_lstm[l] : L.dfeed; g.ldc = 2 * H; g.flags = UIC_GEMM_OUT_F32;
      UIC_TRY(uic_gemm_launch(g, s));
    }
  }
  return UIC_OK;
}

// ---- decoder weights over all steps, decoder embeddings
int Nmt::bwd_dec_weights(hipStream_t s) {
  const int H4 = 4 * H, Md = Td * B;
  for (int l = 0; l < NL; ++l) {
    if (l == 0) {   // inputs [emb | feed_prev | h_prev]
      const UicGemmTnSeg segs[3] = {{L.emb_d, W, W}, {L.out_all, H, H}, {L.hd[0], H, H}};
      const WDest dd[2] = {{G->dec_w_ih[0], W + H, 0, W + H}, {G->dec_w_hh[0], H, W + H, H}};
      UIC_TRY(wgrad_group(L.slab, L.slab_bytes, dt, L.dg_d[0], H4, H4, segs, 3, Md, dd, 2, s, false, L.tA, L.tB));
    } else {        // inputs [dropped h of layer l-1 | h_prev]
      const UicGemmTnSeg segs[2] = {{L.hdrop[l - 1], H, H}, {L.hd[l], H, H}};
      const WDest dd[2] = {{G->dec_w_ih[l], H, 0, H}, {G->dec_w_hh[l], H, H, H}};
      UIC_TRY(wgrad_group(L.slab, L.slab_bytes, dt, L.dg_d[l], H4, H4, segs, 2, Md, dd, 2, s, false, L.tA, L.tB));
    }
    UIC_TRY(uic_colsum_launch(dt, L.dg_d[l], Md, H4, H4, G->dec_b_ih[l], L.colscratch, L.colscratch_floats, s));
    UIC_TRY(uic_copy_launch(G->dec_b_hh[l], G->dec_b_ih[l], (size_t)H4 * 4, s));
  }
  // decoder embeddings (padding_idx = PAD keeps that row's gradient at zero)
  UicGemmParams g = gemm_base(dt, Md, W);
  add_seg(g, L.dg_d[0], H4, L.dec_wT[0], H4, H4);
  g.C = L.demb_d; g.ldc = W; g.flags = UIC_GEMM_OUT_F32;
  UIC_TRY(uic_gemm_launch(g, s));
  // (bucketed by word, one owner per table row: bit-reproducible, no floating-point atomics -- csrc/embedding.hip)
  return uic_embed_bwd_sorted_launch(dt, L.demb_d, nullptr, L.tgt_in, 1, Md, 1, Vt, W, 0.f, 0, G->dec_lut, L.embed_scratch, s);
}

// ---- deferred attention gradients: d context (direct share, into L.d_lay) and d ctxw, then linear_in through ctxw = context W_in:
// dW_in = context^T d ctxw,  d context += d ctxw W_in^T; linear_out from (d_pre, [c | q])
int Nmt::bwd_attention(hipStream_t s) {
  const int Md = Td * B, Ms = S * B;
  UIC_TRY(nmt_gattn_bwd_accum_launch(dt, L.attn_all, L.dscore_all, L.d_cq_all, 2 * H, off(L.hd[NL - 1], BH, dt), Td, S, B, H, L.d_lay, L.dctxw, s));
  {
    const UicGemmTnSeg seg{L.dctxw, H, H};
    const WDest d1{G->attn_in_w, H, 0, H};
    UIC_TRY(wgrad_group(L.slab, L.slab_bytes, dt, context(), H, H, &seg, 1, Ms, &d1, 1, s, false, L.tA, L.tB));
    UicGemmParams g = gemm_base(dt, Ms, H);
    add_seg(g, L.dctxw, H, L.attn_in_w, H, H);
    g.C = L.d_lay; g.ldc = H; g.flags = UIC_GEMM_OUT_F32 | UIC_GEMM_ACCUM;
    UIC_TRY(uic_gemm_launch(g, s));
  }
  const UicGemmTnSeg segs[2] = {{L.cvec_all, H, H}, {off(L.hd[NL - 1], BH, dt), H, H}};
  const WDest d2{G->attn_out_w, 2 * H, 0, 2 * H};
  return wgrad_group(L.slab, L.slab_bytes, dt, L.d_pre_all, H, H, segs, 2, Md, &d2, 1, s, false, L.tA, L.tB);
}

// ---- encoder layer l's BPTT, both directions, as ONE persistent launch (nmt_persist.hip)
int Nmt::bwd_enc_layer_persist(int l, NmtSide* ss, hipStream_t s) {
  UicNmtEncParams p;
  enc_params(p, l, NL + 2 + l);
  for (int dd = 0; dd < 2; ++dd) { p.w_hh[dd] = L.enc_w_hhT[l][dd]; p.dgates[dd] = L.dg_e[l][dd]; }
  p.d_top = L.d_lay;
  p.dh_init = (l == 0 ? L.dfeed : L.dx_lstm[l]) + H; p.ld_dh_init = 2 * H;
  p.dc_init = L.dcd[l]; p.ld_dc_init = H;
  UIC_TRY(uic_nmt_enc_bwd_persist_launch(p, s));
  UIC_TRY(uic_check_hip(hipEventRecord(ss->ev_go, s), "hipEventRecord"));          // (the side stream falls in behind this layer, as in the chain)
  return uic_check_hip(hipStreamWaitEvent(ss->stream, ss->ev_go, 0), "hipStreamWaitEvent");
}

// ---- ... as the launch chain, the backward direction on the side stream
int Nmt::bwd_enc_layer_chain(int l, NmtSide* ss, hipStream_t s) {
  UIC_TRY(uic_check_hip(hipEventRecord(ss->ev_go, s), "hipEventRecord"));          // d_top of this layer is final
  UIC_TRY(uic_check_hip(hipStreamWaitEvent(ss->stream, ss->ev_go, 0), "hipStreamWaitEvent"));
  for (int dd = 1; dd >= 0; --dd) {
    hipStream_t sd = dd == 1 ? ss->stream : s;
    float* dhrec = dd == 1 ? L.dhrec_e1 : L.dhrec_e;
    float* dcc = dd == 1 ? L.dc_e1 : L.dc_e;
    // carried dh / dc start from the decoder-initial-state gradient halves (rows join the BPTT when they become active)
    // (d h_l(-1) of decoder layers > 0 sits in the second half of that layer's last dX)
    const float* dh_init = (l == 0 ? L.dfeed : L.dx_lstm[l]) + H;
    const size_t dh_pitch = (size_t)2 * H * 4;
    UIC_TRY(uic_check_hip(hipMemcpy2DAsync(dhrec, (size_t)Hd * 4, dh_init + dd * Hd, dh_pitch, (size_t)Hd * 4, B,
                                           hipMemcpyDeviceToDevice, sd), "memcpy2d dh0"));
    UIC_TRY(uic_check_hip(hipMemcpy2DAsync(dcc, (size_t)Hd * 4, L.dcd[l] + dd * Hd, (size_t)H * 4, (size_t)Hd * 4, B,
                                           hipMemcpyDeviceToDevice, sd), "memcpy2d dc0"));
    for (int k = S - 1; k >= 0; --k) {
      const int st = dd == 0 ? k : S - 1 - k;
      const int prev = dd == 0 ? st : st + 2;
      if (nb[st] == 0) continue;
      UicLstmBwdParams p;
      memset(&p, 0, sizeof(p));
      p.dtype = dt; p.M = nb[st]; p.H = Hd;
      p.dh0 = L.d_lay + (size_t)st * BH + dd * Hd; p.lddh0 = H;
      p.dh1 = dhrec; p.lddh1 = Hd;
      p.dc = dcc; p.gates = off(L.gates_e[l][dd], (size_t)st * B * 4 * Hd, dt);
      p.c_prev = L.c_e[l][dd] + (size_t)prev * BHd; p.c = L.c_e[l][dd] + (size_t)(st + 1) * BHd;
      p.dgates = offw(L.dg_e[l][dd], (size_t)st * B * 4 * Hd, dt);
      UIC_TRY(uic_lstm_bwd_launch(p, sd));
      UicGemmParams g = gemm_base(dt, nb[st], Hd);
      add_seg(g, p.dgates, 4 * Hd, L.enc_w_hhT[l][dd], 4 * Hd, 4 * Hd);
      g.C = dhrec; g.ldc = Hd; g.flags = UIC_GEMM_OUT_F32;
      UIC_TRY(uic_gemm_launch(g, sd));
    }
    if (dd == 1) UIC_TRY(uic_check_hip(hipEventRecord(ss->ev_done, sd), "hipEventRecord"));
  }
  return uic_check_hip(hipStreamWaitEvent(s, ss->ev_done, 0), "hipStreamWaitEvent");
}

// ---- encoder layer l: d context = deferred attention gradient (L.d_lay); d h0/c0 of the decoder enter at each row's final steps
int Nmt::bwd_enc_layer(int l, NmtSide* ss, hipStream_t s) {
  const int in = l == 0 ? W : H, Ms = S * B;
  UIC_TRY(enc_persist() ? bwd_enc_layer_persist(l, ss, s) : bwd_enc_layer_chain(l, ss, s));
  for (int dd = 0; dd < 2; ++dd) {
    // weights of this direction: dG^T [4Hd, S*B] x [x_l | h_prev]^T  (padded rows of dG are zero)
    const UicGemmTnSeg segs[2] = {{enc_in(l), in, in}, {off(L.xl[l + 1], (size_t)(dd == 0 ? 0 : 2) * BH + dd * Hd, dt), H, Hd}};
    const WDest dw[2] = {{G->enc_w_ih[l][dd], in, 0, in}, {G->enc_w_hh[l][dd], Hd, in, Hd}};
    UIC_TRY(wgrad_group(L.slab, L.slab_bytes, dt, L.dg_e[l][dd], 4 * Hd, 4 * Hd, segs, 2, Ms, dw, 2, s, false, L.tA, L.tB));
    UIC_TRY(uic_colsum_launch(dt, L.dg_e[l][dd], Ms, 4 * Hd, 4 * Hd, G->enc_b_ih[l][dd], L.colscratch, L.colscratch_floats, s));
    UIC_TRY(uic_copy_launch(G->enc_b_hh[l][dd], G->enc_b_ih[l][dd], (size_t)4 * Hd * 4, s));
  }
  {  // d input of layer l = sum over directions dG W_ih
    UicGemmParams g = gemm_base(dt, Ms, in);
    add_seg(g, L.dg_e[l][0], 4 * Hd, L.enc_w_ihT[l][0], 4 * Hd, 4 * Hd);
    add_seg(g, L.dg_e[l][1], 4 * Hd, L.enc_w_ihT[l][1], 4 * Hd, 4 * Hd);
    g.C = L.dx_e; g.ldc = in; g.flags = UIC_GEMM_OUT_F32;
    UIC_TRY(uic_gemm_launch(g, s));
  }
  if (l > 0) {   // the layer below takes it through the inter-layer dropout, in L.d_lay
    if (drop_p > 0.f) UIC_TRY(nmt_dropout_grad_launch(L.dx_e, (size_t)Ms * H, drop_p, seed, SITE_NMT_ENC(l - 1), s));
    UIC_TRY(uic_copy_launch(L.d_lay, L.dx_e, (size_t)Ms * H * 4, s));
  }
  return UIC_OK;
}

// ---- encoder embeddings: x0 = relu(linear(emb))
int Nmt::bwd_enc_embed(hipStream_t s) {
  const int Ms = S * B;
  UIC_TRY(uic_relu_mask_bwd_launch(dt, L.dx_e, off(L.xl[0], (size_t)B * W, dt), 1.f, L.dpre_e, (size_t)Ms * W, s));
  {
    const UicGemmTnSeg seg{L.xe, W, W};
    const WDest d1{G->enc_lin_w, W, 0, W};
    UIC_TRY(wgrad_group(L.slab, L.slab_bytes, dt, L.dpre_e, W, W, &seg, 1, Ms, &d1, 1, s, false, L.tA, L.tB));
  }
  UIC_TRY(uic_colsum_launch(dt, L.dpre_e, Ms, W, W, G->enc_lin_b, L.colscratch, L.colscratch_floats, s));
  {
    UicGemmParams g = gemm_base(dt, Ms, W);
    add_seg(g, L.dpre_e, W, L.enc_lin_wT, W, W);
    g.C = L.dxe; g.ldc = W; g.flags = UIC_GEMM_OUT_F32;
    UIC_TRY(uic_gemm_launch(g, s));
  }
  return uic_embed_bwd_sorted_launch(dt, L.dxe, nullptr, src, 1, Ms, 1, Vs, W, 0.f, 0, G->enc_lut, L.embed_scratch, s);
}

int Nmt::backward(hipStream_t s) {
  NmtSide* ss = nullptr;
  UIC_TRY(nmt_side(&ss));
  UIC_TRY(zero_backward_buffers(s));
  UIC_TRY(bwd_gen_dout(s));
  UIC_TRY(bwd_gen_weights(ss, s));
  if (bptt_persist()) {
    // the persistent launch needs every CU (one 160 KB workgroup each), so the generator's weight gradient cannot run beside it:
    // the main stream waits for the side stream first
    UIC_TRY(uic_check_hip(hipStreamWaitEvent(s, ss->ev_done, 0), "hipStreamWaitEvent"));
    UIC_TRY(bwd_dec_persist(s));
  } else {
    UIC_TRY(bwd_dec_chain(s));
  }
  UIC_TRY(uic_check_hip(hipStreamWaitEvent(s, ss->ev_done, 0), "hipStreamWaitEvent"));   // generator gradients done: scratch is free
  UIC_TRY(bwd_dec_weights(s));
  UIC_TRY(bwd_attention(s));
  // gradient group 1 (uic_nmt_grad_ready_wait): decoder LSTMs, decoder embeddings, linear_in, linear_out are final
  UIC_TRY(uic_check_hip(hipEventRecord(ss->ev_grad_dec, s), "hipEventRecord"));
  ss->grads_recorded = true;
  for (int l = NL - 1; l >= 0; --l) UIC_TRY(bwd_enc_layer(l, ss, s));
  return bwd_enc_embed(s);
}

}  // namespace nmt

using nmt::Nmt;

extern "C" {

int uic_nmt_forward_loss(const uic_nmt_dims* d, const uic_nmt_weights* w, const int64_t* src, const int32_t* lengths_host,
                         const int32_t* lengths_dev, const int64_t* tgt, int32_t training, uint32_t seed, void* workspace,
                         float* loss_out, int32_t* stats_out, float* outputs_out, float* attn_out, float* context_out,
                         void* stream) {
  UIC_TRY(nmt::nmt_check(d));
  UIC_REQUIRE(w && src && lengths_host && lengths_dev && tgt && workspace && loss_out, "nmt_forward_loss: null pointer");
  hipStream_t s = (hipStream_t)stream;
  static thread_local Nmt st;
  UIC_TRY(st.init(d, w, src, lengths_host, tgt, training, seed, workspace, nullptr));
  UIC_TRY(st.refresh(s));
  UIC_TRY(st.encoder_fwd(lengths_dev, s));
  UIC_TRY(st.decoder_fwd(s));
  UIC_TRY(st.loss_fwd(loss_out, stats_out, s));
  const int dt = st.dt;
  if (outputs_out) UIC_TRY(uic_to_f32_launch(dt, off(st.L.out_all, st.BH, dt), outputs_out, (size_t)st.Td * st.BH, s));
  if (attn_out) UIC_TRY(uic_copy_launch(attn_out, st.L.attn_all, (size_t)st.Td * st.B * st.S * 4, s));
  if (context_out) UIC_TRY(uic_to_f32_launch(dt, st.context(), context_out, (size_t)st.S * st.BH, s));
  return UIC_OK;
}

int uic_nmt_backward(const uic_nmt_dims* d, const uic_nmt_weights* w, const int64_t* src, const int32_t* lengths_host,
                     const int64_t* tgt, int32_t training, uint32_t seed, void* workspace, const uic_nmt_weights* grads,
                     void* stream) {
  UIC_TRY(nmt::nmt_check(d));
  UIC_REQUIRE(w && src && lengths_host && tgt && workspace && grads, "nmt_backward: null pointer");
  static thread_local Nmt st;
  UIC_TRY(st.init(d, w, src, lengths_host, tgt, training, seed, workspace, grads));
  return st.backward((hipStream_t)stream);
}

int uic_nmt_grad_ready_wait(void* stream, int32_t group) {
  nmt::NmtSide* ss = nullptr;
  UIC_TRY(nmt::nmt_side(&ss));
  UIC_REQUIRE(group == 0 || group == 1, "nmt_grad_ready_wait: group=%d must be 0 (generator) or 1 (decoder side)", group);
  UIC_REQUIRE(ss->grads_recorded, "nmt_grad_ready_wait: no uic_nmt_backward has run on this device yet");
  return uic_check_hip(hipStreamWaitEvent((hipStream_t)stream, group == 0 ? ss->ev_grad_gen : ss->ev_grad_dec, 0), "hipStreamWaitEvent");
}

}  // extern "C"
