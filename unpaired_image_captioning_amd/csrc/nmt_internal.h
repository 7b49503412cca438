// Declarations shared by the pivot NMT sequencer files: the dropout site numbers (also read by nmt_persist.hip), the launchers of
// the per-step kernels (nmt_kernels.hip), workspace layout and the per-device side stream (nmt_layout.hip), the pieces of a
// training step (struct Nmt: nmt_layout.hip, nmt_train.hip) and the translator's workspace (nmt_translate.hip).
#pragma once
#include "uic_common.h"
#include "uic_host.h"
#include "../../include/uic_hip.h"
#include <string.h>

// dropout sites of the pivot NMT step: between encoder layers, between decoder layers at step t, the decoder output of step t
#define SITE_NMT_ENC(l) (1000u + (unsigned)(l))
#define SITE_NMT_DEC(l, t) (2000u + (unsigned)(l) * 256u + (unsigned)(t))
#define SITE_NMT_OUT(t) (4000u + (unsigned)(t))

namespace nmt {

constexpr int NT = 256;
constexpr int ML = UIC_NMT_MAX_LAYERS;

// ---- nmt_kernels.hip: one launcher per kernel, each with its own dtype dispatch and launch check
int nmt_prep_launch(const int64_t* tgt, int T, int B, int64_t* target_bt, float* mask_bt, int64_t* tgt_in, hipStream_t s);
int nmt_dropout_apply_launch(int dt, const void* src, void* dst, size_t n, float p, unsigned seed, unsigned site, hipStream_t s);
int nmt_dropout_grad_launch(float* g, size_t n, float p, unsigned seed, unsigned site, hipStream_t s);
int nmt_enc_final_launch(int dt, const void* xl, const float* c_f, const float* c_b, const int* lens, int B, int H, int Hd, void* h0,
                         float* c0, hipStream_t s);
// source positions a wave of the register-resident attention kernels keeps (bf16, H = 512, S <= 4 waves x 8 or 16), 0: generic kernels
int nmt_gattn_maxr(int dt, int H, int S);
// one workgroup per row b < B.  Training: ctxw + q (target, mask null); translator: target + mask (ctxw, q null)
int nmt_gattn_fwd_launch(int dt, const void* ctx, const float* target, int S, int B, int H, float* attn, void* cvec, const int64_t* mask,
                         const float* ctxw, const void* q, hipStream_t s);
int nmt_gattn_bwd_step_launch(int dt, const void* ctx, const float* attn, const float* dcq, int lddcq, int S, int B, int H, float* dscore,
                              const float* ctxw, float* dq, int lddq, hipStream_t s);
int nmt_gattn_bwd_accum_launch(int dt, const float* attn_all, const float* dscore_all, const float* dcq_all, int lddcq, const void* q_all,
                               int Td, int S, int B, int H, float* dctx, void* dctxw, hipStream_t s);
int nmt_tanh_drop_bwd_launch(int dt, const float* d_out, const float* d_feed, int ld_feed, int H, const void* out_pre, int n, float p,
                             unsigned seed, unsigned site, void* d_pre, hipStream_t s);
int nmt_fill_f32_launch(float* p, float v, int n, hipStream_t s);

// ---- nmt_layout.hip
struct NmtLayout {
  // operand-dtype weight views (masters in f32 mode, copies in bf16 mode) and transposes for the dX GEMMs
  const void* enc_lin_w; const void* enc_w_ih[ML][2]; const void* enc_w_hh[ML][2];
  const void* dec_w_ih[ML]; const void* dec_w_hh[ML]; const void* attn_in_w; const void* attn_out_w; const void* gen_w;
  void* c_enc_lin_w; void* c_enc_w_ih[ML][2]; void* c_enc_w_hh[ML][2]; void* c_dec_w_ih[ML]; void* c_dec_w_hh[ML];
  void* c_attn_in_w; void* c_attn_out_w; void* c_gen_w;
  void* enc_lin_wT;            // [W, W]
  void* enc_w_ihT[ML][2];      // [in, 4Hd]
  void* enc_w_hhT[ML][2];      // [Hd, 4Hd]
  void* dec_wT[ML];            // [in_l + H, 4H] = [W_ih^T ; W_hh^T]
  void* attn_in_wT;            // [H, H]
  void* attn_out_wT;           // [2H, H]
  void* gen_wT;                // [H, Vtp]
  // encoder: xl[l] = input of layer l with one zero slot before and after the S steps: [(S+2), B, in_l]
  void* xe; void* xl[ML + 1]; void* xd[ML];
  float* gx_e[ML][2]; float* c_e[ML][2]; void* gates_e[ML][2]; void* dg_e[ML][2];
  // decoder
  int64_t* target_bt; float* mask_bt; int64_t* tgt_in;
  void* emb_d; float* gx_d0;
  void* hd[ML]; float* cd[ML]; void* hdrop[ML]; void* gates_d[ML]; void* dg_d[ML]; float* dhrec_d[ML]; float* dcd[ML];
  float* ctxw; void* dctxw; float* attn_all; void* cvec_all; void* out_pre; void* out_all;   // ctxw = context x W_in [S*B, H] f32
  float* logits; void* dlogits; float* row_loss; float* scalars; int* stats;
  void* out_live; float* d_out_live; int* live_map;
  // backward
  float* d_out_all; float* dfeed; void* d_pre_all; float* d_cq_all; float* dscore_all; float* dq;
  // dx_lstm[l]: d[x_l | h_l(t-1)] of decoder layer l > 0, one buffer per layer so that nothing has to be copied
  float* dx_lstm[ML]; float* d_lay; float* dhrec_e; float* dc_e; float* dhrec_e1; float* dc_e1; float* dx_e; void* dpre_e; float* dxe; float* demb_d;
  void* tA; void* tB; float* colscratch; size_t colscratch_floats; float* slab; size_t slab_bytes;
  unsigned* rnn_sync;          // nmt_persist.hip's registration / barrier counters
  int* embed_scratch;          // uic_embed_bwd_sorted_launch (both embedding tables, one after the other)
  float* dfeed_x; float* dq_att_x;   // [Td, B, H] f32: step-indexed exchange slabs of the persistent BPTT launch
  unsigned long long* dec_bwd_dbg;   // [256][Td][16] time stamps of the persistent BPTT launch (UIC_REC_STAMPS)
  unsigned long long* dec_fwd_dbg;   // the same of the persistent forward launch
  size_t total;
};
NmtLayout nmt_layout(const uic_nmt_dims& d, const uic_nmt_weights* w, void* ws);
int nmt_check(const uic_nmt_dims* d);
// The generator's weight gradient is one TN GEMM over the T B target rows: they are padded with zero rows to a multiple of 128, the
// K granularity of the 256 x 256 ping-pong kernel -- 190 -> 135 us at configs[2]'s 1984 rows; Nmt::backward clears the padding
inline size_t nmt_gen_rows(size_t rows) { return (rows + 127) & ~(size_t)127; }

// Second HIP stream for the backward-direction half of every encoder layer (the two directions of a bidirectional
// layer are independent chains of S latency-bound launches each).
struct NmtSide {
  hipStream_t stream = nullptr;
  hipEvent_t ev_go = nullptr, ev_done = nullptr;
  hipEvent_t ev_r0 = nullptr, ev_gen = nullptr;   // refresh: the caller's stream has reached it; the generator's copies are made
  // uic_nmt_grad_ready_wait: the generator's gradients (side stream) / the decoder-side gradients (caller's stream) of the last
  // uic_nmt_backward are final
  hipEvent_t ev_grad_gen = nullptr, ev_grad_dec = nullptr;
  bool grads_recorded = false;
  bool ready = false;
};
// the calling device's instance (one per device, created on first use; nmt_layout.hip holds them)
int nmt_side(NmtSide** out);

// One step of the pivot model on one GPU, split into the pieces the public entry points and the translator sequence.
struct Nmt {
  uic_nmt_dims d;
  const uic_nmt_weights* w;
  const uic_nmt_weights* G;
  NmtLayout L;
  int dt, B, S, Td, H, W, Hd, NL, Vs, Vt, Vtp;
  size_t Sz, BH, BHd;
  float drop_p;
  unsigned seed;
  const int64_t* src;
  const int64_t* tgt;
  int nb[4096];
  // uic_nmt_dims.tgt_live_rows: generator, criterion and their gradients over the non-PAD target positions only
  bool live = false;
  int live_n = 0, live_pad = 0;
  const int32_t* live_rows = nullptr;
  int init(const uic_nmt_dims* d_, const uic_nmt_weights* w_, const int64_t* src_, const int32_t* lengths_host, const int64_t* tgt_,
           int training, unsigned seed_, void* ws, const uic_nmt_weights* G_);
  // the generator's 25.6 M-element operand copy and its transpose (28 + 28 us) are not needed before the decoder is through: they
  // run on the side stream, and whoever reads them first waits for ev_gen (wait_gen)
  bool gen_pending = false;
  int wait_gen(hipStream_t s);
  int refresh(hipStream_t s);
  // input of encoder layer l as seen by its W_ih GEMM (slots 1..S): the dropped copy between layers in training
  const void* enc_in(int l) const { return off(l > 0 && drop_p > 0.f ? L.xd[l] : L.xl[l], (size_t)B * (l == 0 ? W : H), dt); }
  // the memory bank [S, B, H]: the top encoder layer's outputs, slot 1 onwards
  const void* context() const { return off(L.xl[NL], BH, dt); }
  // Each phase's recurrence as ONE persistent launch (nmt_persist.hip) where the shapes allow, else the launch chain
  bool chain() const { return (d.recurrence & UIC_REC_FWD_CHAIN) != 0; }
  bool enc_persist() const { return !chain() && uic_nmt_enc_persist_eligible(dt, B, S, H); }
  bool dec_persist() const { return !chain() && uic_nmt_dec_persist_eligible(dt, B, S, H, NL); }
  bool bptt_persist() const { return !chain() && uic_nmt_dec_bwd_persist_eligible(dt, B, S, H, NL); }
  // Persistent launch i of a step (encoder layers forward 0..NL-1, decoder forward NL, decoder BPTT NL+1, encoder layers backward
  // NL+2..) has a sync block of its own, so that one launch clears all of them together with the step's other zero-initialised
  // buffers (uic_zero_list_launch) instead of one memset per launch and per buffer.
  unsigned* sync_block(int i) const { return L.rnn_sync + (size_t)i * (uic_rnn_persist_sync_bytes() / 4); }
  // the fields every persistent launch's parameters end in (the one template here: the three parameter structs are unrelated types)
  template <typename P>
  void persist_tail(P& p, int i) const {
    p.sync = sync_block(i); p.sync_zeroed = 1; p.status = d.rnn_status; p.force_safe = (d.recurrence & UIC_REC_SAFE) != 0;
    p.row0 = 0; p.Nrows = B;
  }
  int zero_forward_buffers(hipStream_t s);
  int zero_backward_buffers(hipStream_t s);
  size_t gen_rows() const { return nmt_gen_rows((size_t)Td * B); }
  // ---- forward (nmt_train.hip)
  UicGemmParams enc_gx_gemm(int l, int dd) const;
  // tanh(linear_out([c ; q])) (GlobalAttention.py:165-167) of this step's B rows, for the training chain and the translator:
  // `out_pre` = the tanh output before dropout (kept for the backward pass) or null, `site` = the dropout site (0 with drop_p 0)
  UicGemmParams linear_out_gemm(const void* cvec, const void* q, void* out_pre, void* out, unsigned site) const;
  // logits [rows, Vt] (f32, ld Vtp) = x W_gen^T + b
  UicGemmParams generator_gemm(int rows, const void* x, float* logits) const;
  void enc_params(UicNmtEncParams& p, int l, int block) const;
  int enc_layer_persist(int l, hipStream_t s);
  int enc_layer_chain(int l, hipStream_t s);
  int encoder_fwd(const int32_t* lengths_dev, hipStream_t s);
  int decoder_persist(hipStream_t s);
  int decoder_chain(hipStream_t s);
  int decoder_fwd(hipStream_t s);
  int loss_fwd(float* loss_out, int32_t* stats_out, hipStream_t s);
  // ---- backward (nmt_train.hip), the steps of backward() in its order
  int bwd_gen_dout(hipStream_t s);
  int bwd_gen_weights(NmtSide* ss, hipStream_t s);
  int bwd_dec_persist(hipStream_t s);
  int bwd_dec_chain(hipStream_t s);
  int bwd_dec_weights(hipStream_t s);
  int bwd_attention(hipStream_t s);
  int bwd_enc_layer_persist(int l, NmtSide* ss, hipStream_t s);
  int bwd_enc_layer_chain(int l, NmtSide* ss, hipStream_t s);
  int bwd_enc_layer(int l, NmtSide* ss, hipStream_t s);
  int bwd_enc_embed(hipStream_t s);
  int backward(hipStream_t s);
};

// ---- nmt_translate.hip
struct TrLayout {
  int64_t* src_rep; int32_t* lens_dev;
  void* h[ML][2]; float* c[ML][2]; void* feed[2]; void* emb;
  float* targetq; float* attn; void* cvec; float* logits;
  float* cand_val; int* cand_idx; float* scores; int64_t* tok; int* prev_ks; int64_t* next_ys; float* attn_hist;
  int* done; int* flags;
  void* enc_ws; size_t enc_bytes;
  size_t total;
};

}  // namespace nmt
