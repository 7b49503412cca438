// Workspace layout and derived weight copies of the TopDown captioner: one bump allocation each over a caller-provided arena,
// the dims check, and the size / pointer queries of the C ABI.
#include "topdown_internal.h"

namespace topdown {

Layout make_layout(const uic_topdown_dims& d, void* ws) {
  Layout L;
  memset(&L, 0, sizeof(L));
  Bump b{(char*)ws, 0};
  const size_t S = uic_dtype_size(d.dtype);
  const size_t N = d.N, R = d.R, D = d.D, Dfc = d.Dfc, H = d.H, E = d.E, A = d.A, V1 = d.V1, T = d.T;
  const size_t M = T * N, Mp = rup8(M), Np = rup8(N), NR = N * R, NRp = rup8(NR), V1p = vpad(V1);
  L.fcT = b.take(N * Dfc * S);
  L.attT = b.take(NR * D * S);
  L.row_len = (int*)b.take(N * sizeof(int));
  if (d.seq_per_img > 1) {
    L.amask_rep = (float*)b.take(NR * 4);
    L.row_len_rep = (int*)b.take(N * sizeof(int));
    L.ypre = (float*)b.take(N / d.seq_per_img * R * H * 4);
  }
  L.fcp = b.take(N * H * S);
  L.attp = b.take(NR * H * S);
  L.patt = b.take(NR * A * S);
  L.eatt = d.dtype == UIC_BF16 ? b.take(NR * A * S) : nullptr;
  if (d.use_bn) {
    L.bn_stat0 = (float*)b.take(2 * D * 4);
    L.bn_stat4 = (float*)b.take(2 * H * 4);
    const size_t p0 = uic_bn_scratch_floats((int)NR, (int)D), p4 = uic_bn_scratch_floats((int)NR, (int)H);
    L.bn_part = (float*)b.take((p0 > p4 ? p0 : p4) * 4);
    L.bn_red = (float*)b.take(3 * (D > H ? D : H) * 4);
    if (d.use_bn == 2) L.ybn = b.take(NR * H * S);
  }
  L.tok_used = (int64_t*)b.take(N * T * 8);
  L.xt_all = b.take(M * E * S);
  L.gx = (float*)b.take(M * 4 * H * 4);
  L.gfc = (float*)b.take(N * 4 * H * 4);
  L.h_att = b.take((T + 1) * N * H * S);
  L.h_lang = b.take((T + 1) * N * H * S);
  L.c_att = (float*)b.take((T + 1) * N * H * 4);
  L.c_lang = (float*)b.take((T + 1) * N * H * 4);
  L.gates1 = b.take(M * 4 * H * S);
  L.gates2 = b.take(M * 4 * H * S);
  L.atth_all = (float*)b.take(M * A * 4);
  L.alpha_all = (float*)b.take(M * R * 4);
  L.ctx_all = b.take(M * H * S);
  L.hdrop_all = b.take(M * H * S);
  // (+128 rows: the live-position list is padded to whole 128-row tiles, uic_topdown_batch.live_rows)
  L.logits = (float*)b.take((M + 128) * V1p * 4);
  L.dlogits = b.take((M + 128) * V1p * S);
  L.row_loss = (float*)b.take(M * 4);
  for (int l = 0; l + 1 < d.logit_layers; ++l) {
    L.lh[l] = b.take(M * H * S);
    L.dlh_pre[l] = b.take(M * H * S);
    L.s_lh[l] = b.take(N * H * S);
  }
  if (d.logit_layers > 1) L.dlh = (float*)b.take(M * H * 4);
  L.scalars = (float*)b.take(64);
  L.dhdrop = (float*)b.take(M * H * 4);
  L.live_map = (int*)b.take((M + 128) * 4);
  L.live_inv = (int*)b.take(M * 4);
  L.cap_len = (int*)b.take(N * 4);
  L.hc = b.take((M + 128) * H * S);
  L.dhc = (float*)b.take((M + 128) * H * 4);
  L.dx2_all = (float*)b.take(M * 3 * H * 4);
  L.dx1 = (float*)b.take(N * 2 * H * 4);
  L.dc_att = (float*)b.take(N * H * 4);
  L.dc_lang = (float*)b.take(N * H * 4);
  L.dg1_all = b.take(M * 4 * H * S);
  L.dg2_all = b.take(M * 4 * H * S);
  L.de_all = (float*)b.take(M * R * 4);
  L.datth_all = b.take(M * A * S);
  L.dgfc = b.take(N * 4 * H * S);
  L.dfcp = (float*)b.take(N * H * 4);
  L.dfcpre = b.take(N * H * S);
  L.dxt = (float*)b.take(M * E * 4);
  L.d_att = (float*)b.take(NR * H * 4);
  L.d_patt = b.take(NR * A * S);
  L.dwalpha_part = (float*)b.take(N * (A + 1) * 4);
  L.d_pre = b.take(NR * H * S);
  size_t ta = 4 * H * Mp;
  if (A * Mp > ta) ta = A * Mp;
  if (A * NRp > ta) ta = A * NRp;
  if (H * NRp > ta) ta = H * NRp;
  if (4 * H * Np > ta) ta = 4 * H * Np;
  size_t tb = (2 * H + (E > H ? E : H)) * Mp;   // three stacked right operands of the merged LSTM weight-gradient GEMMs
  if ((H > D ? H : D) * NRp > tb) tb = (H > D ? H : D) * NRp;
  if ((H > Dfc ? H : Dfc) * Np > tb) tb = (H > Dfc ? H : Dfc) * Np;
  tb += 128 * (NRp > Mp ? NRp : Mp);            // + the ones segment of the bias gradients
  L.tA = b.take(ta * S);
  L.tB = b.take(tb * S);
  size_t maxcols = V1p;
  if (4 * H > maxcols) maxcols = 4 * H;
  if (A + 1 > maxcols) maxcols = A + 1;
  L.colscratch_floats = 128 * maxcols;
  L.colscratch = (float*)b.take(L.colscratch_floats * 4);
  L.small = (float*)b.take((A + 8) * 4);
  L.tLA = b.take((d.logit_layers > 1 && H > V1 ? H : V1) * (Mp + 128) * S);   // dlogits^T [V1, M]; hidden logit blocks: d pre^T [H, M]
  L.tLB = b.take(H * (Mp + 128) * S);
  L.colscratchL = (float*)b.take(L.colscratch_floats * 4);
  {
    const size_t Kc = rup8((size_t)WG_CHUNK * N);
    size_t rb = 2 * H + E + 128;                // att_lstm inputs [h_lang | xt | h_att]; lang_lstm inputs are 3H wide; + the ones block
    if (3 * H + 128 > rb) rb = 3 * H + 128;
    if (Dfc > rb) rb = Dfc;
    const size_t la = 4 * H > A ? 4 * H : A;    // left operands: dG [rows, 4H] of the LSTMs, d att_h [rows, A] of h2att
    L.tSA = b.take(la * Kc * S);
    L.tSB = b.take(rb * Kc * S);
    L.tTA = b.take(la * Kc * S);
    L.tTB = b.take(rb * Kc * S);
    L.tUA = b.take(la * Kc * S);
    L.tUB = b.take(rb * Kc * S);
  }
  {  // split-K partial slabs: room for 4 slices of the largest merged weight gradient [4H, 2H + E]
    size_t sl = 4 * (4 * H) * (2 * H + E) * 4;
    const size_t cap = (size_t)256 << 20;
    if (sl > cap) sl = cap;
    L.slab_bytes = sl;
    L.slab = (float*)b.take(sl);
    L.slab2 = (float*)b.take(sl);
    L.slab3 = (float*)b.take(sl);
    L.slab4 = (float*)b.take(sl);
  }
  L.embed_scratch = (int*)b.take(uic_embed_bwd_sorted_scratch_ints(N, T, V1, E) * 4);
  L.fcwT = b.take(Dfc * H * S);
  L.attwT = b.take(D * H * S);
  L.ones_rows = rup8((size_t)WG_CHUNK * N) > (size_t)N * R ? rup8((size_t)WG_CHUNK * N) : (size_t)N * R;
  L.ones_blk = b.take(L.ones_rows * 128 * S);
  L.rnn_sync = (unsigned*)b.take(uic_rnn_persist_sync_bytes());
  L.rnn_dbg = (unsigned long long*)b.take((size_t)256 * T * 16 * 8);
  for (int i = 0; i < 2; ++i) L.bp_slab2[i] = (float*)b.take((size_t)BPTT_SPLIT * N * 3 * H * 4);
  L.bp_slab1 = (float*)b.take((size_t)BPTT_SPLIT * N * 2 * H * 4);
  L.rnn_bwd_sync_bytes = T * uic_rnn_persist_sync_bytes();
  L.rnn_bwd_sync = (unsigned*)b.take(L.rnn_bwd_sync_bytes);
  L.rnn_bwd_dbg = (unsigned long long*)b.take((size_t)256 * T * 16 * 8);
  for (int i = 0; i < 2; ++i) {
    L.s_h_att[i] = b.take(N * H * S);
    L.s_h_lang[i] = b.take(N * H * S);
    L.s_c_att[i] = (float*)b.take(N * H * 4);
    L.s_c_lang[i] = (float*)b.take(N * H * 4);
  }
  L.s_xt = b.take(N * E * S);
  L.s_atth = (float*)b.take(N * A * 4);
  L.s_alpha = (float*)b.take(N * R * 4);
  L.s_ctx = b.take(N * H * S);
  L.s_hdrop = b.take(N * H * S);
  L.s_logits = (float*)b.take(N * V1p * 4);
  L.smp.carve(b, N, T);
  L.dec_part = (float*)b.take(uic_rnn_decode_part_floats((int)N) * 4);
  L.dec_tok = (int*)b.take(N * 4);
  L.dec_embed_relu = b.take(V1 * E * 2);
  L.beam.carve(b, N, N, T);
  L.row_order = (int*)b.take(N * 4);
  L.row_rank = (int*)b.take(N * 4);
  L.unfinished = (int*)b.take((T + 1) * 4);
  L.dg2c = b.take(N * 4 * H * S);
  L.dg1c = b.take(N * 4 * H * S);
  L.total = (b.off + 255) & ~(size_t)255;
  return L;
}

Derived make_derived(const uic_topdown_dims& d, const uic_topdown_weights* w, void* base) {
  Derived v;
  memset(&v, 0, sizeof(v));
  Bump b{(char*)base, 0};
  const size_t S = uic_dtype_size(d.dtype);
  const size_t D = d.D, Dfc = d.Dfc, H = d.H, E = d.E, A = d.A, V1 = d.V1, V1p = vpad(V1);
  const bool bf = d.dtype == UIC_BF16;
  auto copy = [&](const float* master, size_t n) -> const void* {
    if (!bf) return master;
    return b.take(n * S);
  };
  v.fc_w = copy(w ? w->fc_w : nullptr, H * Dfc);
  if (d.use_bn) {
    v.att_w = b.take(H * D * S);
    v.att_beff = (float*)b.take(H * 4);
  } else {
    v.att_w = copy(w ? w->att_w : nullptr, H * D);
  }
  v.ctx2att_w = copy(w ? w->ctx2att_w : nullptr, A * H);
  v.logit_w = copy(w ? w->logit_w : nullptr, V1 * H);
  v.att_w_ih = copy(w ? w->att_lstm_w_ih : nullptr, 4 * H * (E + 2 * H));
  v.att_w_hh = copy(w ? w->att_lstm_w_hh : nullptr, 4 * H * H);
  v.lang_w_ih = copy(w ? w->lang_lstm_w_ih : nullptr, 4 * H * 2 * H);
  v.lang_w_hh = copy(w ? w->lang_lstm_w_hh : nullptr, 4 * H * H);
  v.h2att_w = copy(w ? w->h2att_w : nullptr, A * H);
  v.embed_w = copy(w ? w->embed_w : nullptr, V1 * E);
  v.logit_wT = b.take(H * V1p * S);
  v.w2T = b.take(3 * H * 4 * H * S);
  v.w1recT = b.take(2 * H * 4 * H * S);
  v.wxT = b.take(E * 4 * H * S);
  v.wfcpT = b.take(H * 4 * H * S);
  v.h2attT = b.take(H * A * S);
  v.ctx2attT = b.take(H * A * S);
  for (int l = 0; l + 1 < d.logit_layers; ++l) {
    v.logit_h_w[l] = copy(w ? w->logit_h_w[l] : nullptr, H * H);
    v.logit_h_wT[l] = b.take(H * H * S);
  }
  v.total = (b.off + 255) & ~(size_t)255;
  return v;
}

int check_dims(const uic_topdown_dims* d) {
  UIC_REQUIRE(d != nullptr, "null dims");
  UIC_REQUIRE(d->dtype == UIC_F32 || d->dtype == UIC_BF16, "bad dtype %d", d->dtype);
  UIC_REQUIRE(d->N > 0 && d->R > 0 && d->T > 0 && d->V1 > 1, "bad sizes N=%d R=%d T=%d V1=%d", d->N, d->R, d->T, d->V1);
  UIC_REQUIRE(d->D % 8 == 0 && d->Dfc % 8 == 0 && d->H % 8 == 0 && d->E % 8 == 0 && d->A % 8 == 0,
              "D=%d Dfc=%d H=%d E=%d A=%d must all be multiples of 8", d->D, d->Dfc, d->H, d->E, d->A);
  UIC_REQUIRE(d->drop_p >= 0.f && d->drop_p < 1.f, "drop_p=%f outside [0,1)", (double)d->drop_p);
  UIC_REQUIRE(d->use_bn >= 0 && d->use_bn <= 2, "use_bn=%d outside {0,1,2}", d->use_bn);
  UIC_REQUIRE(d->logit_layers >= 0 && d->logit_layers <= UIC_MAX_LOGIT_LAYERS, "logit_layers=%d outside [0,%d]", d->logit_layers,
              UIC_MAX_LOGIT_LAYERS);
  UIC_REQUIRE(d->seq_per_img >= 0 && (d->seq_per_img <= 1 || d->N % d->seq_per_img == 0),
              "seq_per_img=%d must divide N=%d", d->seq_per_img, d->N);
  const int rec_known = UIC_REC_FWD_CHAIN | UIC_REC_BWD_PERSIST | UIC_REC_SAFE | UIC_REC_STAMPS | UIC_REC_EARLY_GRADS | UIC_REC_NO_F32A |
                        UIC_REC_COMM_STREAM;
  UIC_REQUIRE((d->recurrence & ~rec_known) == 0, "recurrence=0x%x: unknown bit(s) 0x%x (the UIC_REC_* flags of uic_hip.h)",
              (unsigned)d->recurrence, (unsigned)(d->recurrence & ~rec_known));
  return UIC_OK;
}

}  // namespace topdown

using namespace topdown;

extern "C" {

size_t uic_topdown_workspace_bytes(const uic_topdown_dims* d) {
  if (check_dims(d)) return 0;
  return make_layout(*d, nullptr).total;
}
size_t uic_topdown_derived_bytes(const uic_topdown_dims* d) {
  if (check_dims(d)) return 0;
  return make_derived(*d, nullptr, nullptr).total;
}

void* uic_topdown_workspace_ptr(const uic_topdown_dims* d, void* workspace, const char* name) {
  if (check_dims(d) || !workspace || !name) return nullptr;
  const Layout L = make_layout(*d, workspace);
  struct { const char* n; void* p; } tab[] = {
      {"tok_used", L.tok_used}, {"d_pre", L.d_pre}, {"fc_embed", L.fcp}, {"att_embed", L.attp}, {"p_att", L.patt}, {"e_att", L.eatt}, {"xt", L.xt_all}, {"gx", L.gx}, {"gfc", L.gfc},
      {"h_att", L.h_att}, {"h_lang", L.h_lang}, {"c_att", L.c_att}, {"c_lang", L.c_lang}, {"gates1", L.gates1},
      {"gates2", L.gates2}, {"att_h", L.atth_all}, {"alpha", L.alpha_all}, {"ctx", L.ctx_all}, {"hdrop", L.hdrop_all},
      {"logits", L.logits}, {"dlogits", L.dlogits}, {"row_loss", L.row_loss}, {"scalars", L.scalars},
      {"dhdrop", L.dhdrop}, {"dx2", L.dx2_all}, {"dg1", L.dg1_all}, {"dg2", L.dg2_all}, {"de", L.de_all},
      {"datth", L.datth_all}, {"d_att", L.d_att}, {"d_p_att", L.d_patt}, {"dxt", L.dxt}, {"rnn_dbg", L.rnn_dbg}, {"rnn_bwd_dbg", L.rnn_bwd_dbg},
      // ("dx1", and columns [H, 3H) of "dx2": written only when the d x GEMMs are not split-K, i.e. by the persistent BPTT kernel
      // or at shapes where bptt_split() == 0 -- the split chain keeps these sums in its slabs)
      {"dx1", L.dx1}, {"dc_att", L.dc_att}, {"dc_lang", L.dc_lang},
      {"cap_len", L.cap_len}, {"row_order", L.row_order}, {"row_rank", L.row_rank}, {"unfinished", L.unfinished}};
  for (auto& e : tab)
    if (!strcmp(e.n, name)) return e.p;
  return nullptr;
}

}  // extern "C"
