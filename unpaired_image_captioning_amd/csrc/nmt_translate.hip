// The pivot NMT translator (NMTModel.translateBatch, beam search): its bookkeeping kernels, workspace and uic_nmt_translate.  The
// encoder, the weight copies and the decode step's attention, linear_out and generator are the training path's (struct Nmt).
#include "nmt_internal.h"

namespace {

using nmt::NT;

// ---- translator bookkeeping (NMTModel.translateBatch + O/Beam.py); rows are sentence-major: row = b * K + k
// dst[s, b * K + k] = src[s, b]
__global__ void nmt_replicate_src_kernel(const int64_t* __restrict__ src, int S, int B, int K, int64_t* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S * B * K) return;
  const int s = i / (B * K), r = i - s * B * K;
  dst[i] = src[(size_t)s * B + r / K];
}
// Beam.__init__: every beam starts as [BOS, PAD, PAD, ...] with zero scores (O/Beam.py:28-38)
__global__ void nmt_beam_init_kernel(int B, int K, int64_t* tok, float* scores, int* done, int* flags) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B * K) { tok[i] = (i % K) == 0 ? 2 : 0; scores[i] = 0.f; }
  if (i < B) done[i] = 0;
  if (i < 4) flags[i] = 0;
}
// `if not active: break` (translateBatch :377-378) decided ON THE DEVICE, so the host loop need not wait for every step:
// before step `step` advances, flags[1] still holds the number of active sentences after step - 1.  None left: the search is
// frozen (flags[2]) -- the remaining, speculatively enqueued steps leave every beam tensor alone -- else flags[3] = the number
// of steps that really ran (the reference's loop count) and the counter is cleared for this step.
__global__ void nmt_beam_begin_kernel(int step, int* flags) {
  if (flags[2]) return;
  if (step > 0 && flags[1] == 0) { flags[2] = 1; return; }
  flags[3] = step + 1;
  flags[1] = 0;
}
// Beam.advance for every sentence (O/Beam.py:52-89): top K of the flattened beam x word scores -- the candidates are the
// per-row top K (cand_val / cand_idx from beam_topk), enumerated beam-major so that ties resolve to the lower flat index --
// back-pointers, next tokens; a sentence is done once its TOP hypothesis ends in EOS; flags[0] = all sentences done.
__global__ __launch_bounds__(64) void nmt_beam_advance_kernel(int B, int K, int step, const float* __restrict__ cand_val, const int* __restrict__ cand_idx,
                                        float* __restrict__ scores, int* __restrict__ prev_ks, int64_t* __restrict__ next_ys, int64_t* __restrict__ tok,
                                        int* __restrict__ done, int* __restrict__ flags) {
  // one wavefront per sentence: the rows x K candidates sit 4 to a lane, K rounds of a wave-wide arg-max
  constexpr int PER = (UIC_BEAM_MAX * UIC_BEAM_MAX + 63) / 64;
  const int b = blockIdx.x, lane = threadIdx.x;
  if (flags[2]) return;                                   // frozen: every sentence was done before this step (nmt_beam_begin_kernel)
  const int rows = step == 0 ? 1 : K, n = rows * K;
  float pj[PER];
  long flat[PER];
  bool used[PER];
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int id = lane + q * 64;
    used[q] = id >= n;
    pj[q] = 0.f;
    flat[q] = 0;
    if (id < n) {
      const int k = id / K;
      const size_t cr = (size_t)b * K * K + id;          // = ((b * K + k) * K + c)
      pj[q] = (step == 0 ? 0.f : scores[(size_t)b * K + k]) + cand_val[cr];
      flat[q] = (long)k * 0x40000000L + cand_idx[cr];
    }
  }
  __syncthreads();                                        // every lane has read the old scores before lane 0 overwrites them
  int first_word = -1;
  for (int j = 0; j < K; ++j) {
    float bp = 0.f;
    long bflat = 0x7fffffffffffffffL;
    int bid = -1;
#pragma unroll
    for (int q = 0; q < PER; ++q)
      if (!used[q] && (bid < 0 || pj[q] > bp || (pj[q] == bp && flat[q] < bflat))) { bp = pj[q]; bflat = flat[q]; bid = lane + q * 64; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float op = __shfl_xor(bp, o, 64);
      const long of = __shfl_xor(bflat, o, 64);
      const int oi = __shfl_xor(bid, o, 64);
      if (oi >= 0 && (bid < 0 || op > bp || (op == bp && of < bflat))) { bp = op; bflat = of; bid = oi; }
    }
#pragma unroll
    for (int q = 0; q < PER; ++q)
      if (bid == lane + q * 64) used[q] = true;
    const int k = bid / K;
    const int word = (int)(bflat - (long)k * 0x40000000L);
    if (j == 0) first_word = word;
    if (lane == 0) {
      prev_ks[((size_t)step * B + b) * K + j] = k;
      next_ys[((size_t)step * B + b) * K + j] = word;
      tok[(size_t)b * K + j] = word;
      scores[(size_t)b * K + j] = bp;
    }
  }
  if (lane == 0) {
    if (first_word == 3) done[b] = 1;
    if (!done[b]) atomicAdd(&flags[1], 1);       // flags[1]: active sentences of this step (zeroed by the host loop's memset)
  }
}
// read-out (translateBatch :384-392, Beam.getHyp :93-117): best final score (first maximum), walk the back-pointers; the
// attention of hypothesis position j is the one of the PARENT beam at step j, PAD source columns dropped (packed left)
__global__ void nmt_beam_readout_kernel(int B, int K, int S, int n_iter, int ld_out, const float* __restrict__ scores, const int* __restrict__ prev_ks,
                                        const int64_t* __restrict__ next_ys, const float* __restrict__ attn_hist, const int64_t* __restrict__ src,
                                        int64_t* __restrict__ hyp, float* __restrict__ score_out, float* __restrict__ attn_out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int k = 0;
  for (int j = 1; j < K; ++j)
    if (scores[(size_t)b * K + j] > scores[(size_t)b * K + k]) k = j;
  score_out[b] = scores[(size_t)b * K + k];
  for (int j = n_iter - 1; j >= 0; --j) {
    hyp[(size_t)b * ld_out + j] = next_ys[((size_t)j * B + b) * K + k];
    const int parent = prev_ks[((size_t)j * B + b) * K + k];
    if (attn_out) {
      const float* a = attn_hist + ((size_t)j * B * K + (size_t)b * K + parent) * S;
      float* o = attn_out + ((size_t)b * ld_out + j) * S;
      int n = 0;
      for (int s2 = 0; s2 < S; ++s2)
        if (src[(size_t)s2 * B + b] != 0) o[n++] = a[s2];
      for (; n < S; ++n) o[n] = 0.f;
    }
    k = parent;
  }
}

}  // namespace

namespace nmt {

TrLayout tr_layout(const uic_nmt_dims& d, int K, int max_steps, void* ws) {
  TrLayout T;
  memset(&T, 0, sizeof(T));
  Bump b{(char*)ws, 0};
  const size_t Sz = uic_dtype_size(d.dtype);
  const size_t B = d.B, R = B * K, S = d.S, H = d.H, W = d.W, NL = d.layers, Vtp = vpad(d.Vt);
  T.src_rep = (int64_t*)b.take(S * R * 8);
  T.lens_dev = (int32_t*)b.take(R * 4);
  for (size_t l = 0; l < NL; ++l)
    for (int i = 0; i < 2; ++i) {
      T.h[l][i] = b.take(R * H * Sz);
      T.c[l][i] = (float*)b.take(R * H * 4);
    }
  for (int i = 0; i < 2; ++i) T.feed[i] = b.take(R * H * Sz);
  T.emb = b.take(R * W * Sz);
  T.targetq = (float*)b.take(R * H * 4);
  T.attn = (float*)b.take(R * S * 4);
  T.cvec = b.take(R * H * Sz);
  T.logits = (float*)b.take(R * Vtp * 4);
  T.cand_val = (float*)b.take(R * UIC_BEAM_MAX * 4);
  T.cand_idx = (int*)b.take(R * UIC_BEAM_MAX * 4);
  T.scores = (float*)b.take(R * 4);
  T.tok = (int64_t*)b.take(R * 8);
  T.prev_ks = (int*)b.take((size_t)max_steps * R * 4);
  T.next_ys = (int64_t*)b.take((size_t)max_steps * R * 8);
  T.attn_hist = (float*)b.take((size_t)max_steps * R * S * 4);
  T.done = (int*)b.take(B * 4);
  T.flags = (int*)b.take(64);
  // the encoder (and the weight copies) run through the training path's workspace on the replicated batch
  uic_nmt_dims d2 = d;
  d2.B = (int)R; d2.T = 2;
  T.enc_bytes = nmt_layout(d2, nullptr, nullptr).total;
  T.enc_ws = b.take(T.enc_bytes);
  T.total = (b.off + 255) & ~(size_t)255;
  return T;
}

// the search's four flag words (nmt_beam_begin_kernel) on the host; waits for the stream
static int read_flags(const int* flags_dev, int fl[4], hipStream_t s) {
  UIC_TRY(uic_check_hip(hipMemcpyAsync(fl, flags_dev, 16, hipMemcpyDeviceToHost, s), "memcpy flags"));
  return uic_check_hip(hipStreamSynchronize(s), "hipStreamSynchronize");
}

}  // namespace nmt

using namespace nmt;

extern "C" {

size_t uic_nmt_translate_workspace_bytes(const uic_nmt_dims* d, int32_t beam_size, int32_t max_steps) {
  if (nmt_check(d) || beam_size < 1 || beam_size > UIC_BEAM_MAX || max_steps < 1) return 0;
  return tr_layout(*d, beam_size, max_steps, nullptr).total;
}

int uic_nmt_translate(const uic_nmt_dims* d, const uic_nmt_weights* w, const int64_t* src, int32_t beam_size, int32_t max_steps,
                      void* workspace, int64_t* hyp_out, float* score_out, float* attn_out, int32_t* n_iter_out, void* stream) {
  UIC_TRY(nmt_check(d));
  UIC_REQUIRE(w && src && workspace && hyp_out && score_out && n_iter_out, "nmt_translate: null pointer");
  UIC_REQUIRE(beam_size >= 1 && beam_size <= UIC_BEAM_MAX && beam_size <= d->Vt, "nmt_translate: beam_size=%d outside [1, %d]", beam_size, UIC_BEAM_MAX);
  UIC_REQUIRE(max_steps >= 1, "nmt_translate: max_steps=%d", max_steps);
  hipStream_t s = (hipStream_t)stream;
  const int K = beam_size, B = d->B, R = B * K, S = d->S, H = d->H, W = d->W, NL = d->layers, Vt = d->Vt, dt = d->dtype;
  const size_t Sz = uic_dtype_size(dt), RH = (size_t)R * H;
  const TrLayout T = tr_layout(*d, K, max_steps, workspace);
  // (1) encoder on the replicated batch, WITHOUT lengths: every position of every row is processed (translateBatch :327)
  hipLaunchKernelGGL(nmt_replicate_src_kernel, dim3(uic_grid_for((size_t)S * R, NT)), dim3(NT), 0, s, src, S, B, K, T.src_rep);
  UIC_LAUNCH_CHECK("nmt_replicate_src_kernel");
  uic_nmt_dims d2 = *d;
  d2.B = R; d2.T = 2; d2.drop_p = 0.f;
  static thread_local Nmt st;           // (its B is the R replicated rows, no dropout)
  {
    static thread_local int32_t lens_host[4096 * UIC_BEAM_MAX];
    UIC_REQUIRE(R <= 4096 * UIC_BEAM_MAX, "nmt_translate: too many rows (%d)", R);
    for (int i = 0; i < R; ++i) lens_host[i] = S;
    UIC_TRY(st.init(&d2, w, T.src_rep, lens_host, nullptr, 0, 0, T.enc_ws, nullptr));
    UIC_TRY(uic_check_hip(hipMemcpyAsync(T.lens_dev, lens_host, (size_t)R * 4, hipMemcpyHostToDevice, s), "memcpy lengths"));
  }
  UIC_TRY(st.refresh(s));
  UIC_TRY(st.encoder_fwd(T.lens_dev, s));
  UIC_TRY(st.wait_gen(s));                  // the generator's copies (side stream) are read from the first decode step on
  const NmtLayout& L = st.L;
  // (2) decoder state = encoder final states (slot 0 of the training path's state buffers), zero input feed
  for (int l = 0; l < NL; ++l) {
    UIC_TRY(uic_copy_launch(T.h[l][0], L.hd[l], RH * Sz, s));
    UIC_TRY(uic_copy_launch(T.c[l][0], L.cd[l], RH * 4, s));
  }
  UIC_TRY(uic_fill_launch(T.feed[0], 0, RH * Sz, s));
  hipLaunchKernelGGL(nmt_beam_init_kernel, dim3(uic_grid_for((size_t)R, NT)), dim3(NT), 0, s, B, K, T.tok, T.scores, T.done, T.flags);
  UIC_LAUNCH_CHECK("nmt_beam_init_kernel");
  UIC_TRY(uic_fill_launch(T.prev_ks, 0, (size_t)max_steps * R * 4, s));   // (speculative steps of a frozen search gather parent 0)
  UicBeamParams bp;
  memset(&bp, 0, sizeof(bp));
  bp.n_img = B; bp.B = K; bp.L = max_steps; bp.V1 = Vt; bp.ldv = st.Vtp; bp.plain = 1;
  bp.logits = T.logits; bp.cand_val = T.cand_val; bp.cand_idx = T.cand_idx;
  int fl[4] = {0, 0, 0, 0};
  // (3) the main loop (:349-378): state slot 0 -> 1, then re-threaded back into slot 0 by the back-pointers
  for (int step = 0; step < max_steps; ++step) {
    UIC_TRY(uic_embed_fwd_launch(dt, w->dec_lut, Vt, W, T.tok, 1, R, 1, 0.f, 0, 0, 0, 0, T.emb, s));
    const void* x = nullptr;
    for (int l = 0; l < NL; ++l) {
      UicGemmParams g = gemm_base(dt, R, 4 * H);
      g.lstm = 1; g.H = H;
      if (l == 0) {
        add_seg(g, T.emb, W, L.dec_w_ih[0], W + H, W);
        add_seg(g, T.feed[0], H, off(L.dec_w_ih[0], W, dt), W + H, H);
      } else {
        add_seg(g, x, H, L.dec_w_ih[l], H, H);
      }
      add_seg(g, T.h[l][0], H, L.dec_w_hh[l], H, H);
      g.bias = w->dec_b_ih[l]; g.bias2 = w->dec_b_hh[l];
      g.c_prev = T.c[l][0]; g.c_out = T.c[l][1]; g.h_out = T.h[l][1]; g.ldh = H;
      UIC_TRY(uic_gemm_launch(g, s));
      x = T.h[l][1];
    }
    {
      UicGemmParams g = gemm_base(dt, R, H);
      add_seg(g, x, H, L.attn_in_w, H, H);
      g.C = T.targetq; g.ldc = H; g.flags = UIC_GEMM_OUT_F32;
      UIC_TRY(uic_gemm_launch(g, s));
    }
    // the memory bank [S, R, H] against linear_in(rnn_output), source padding masked (GlobalAttention.applyMask, :345,352)
    UIC_TRY(nmt_gattn_fwd_launch(dt, st.context(), T.targetq, S, R, H, T.attn_hist + (size_t)step * R * S, T.cvec, T.src_rep, nullptr, nullptr, s));
    UIC_TRY(uic_gemm_launch(st.linear_out_gemm(T.cvec, x, nullptr, T.feed[1], 0), s));
    UIC_TRY(uic_gemm_launch(st.generator_gemm(R, T.feed[1], T.logits), s));
    bp.t = step;
    UIC_TRY(uic_beam_topk_launch(bp, s));
    hipLaunchKernelGGL(nmt_beam_begin_kernel, dim3(1), dim3(1), 0, s, step, T.flags);
    UIC_LAUNCH_CHECK("nmt_beam_begin_kernel");
    hipLaunchKernelGGL(nmt_beam_advance_kernel, dim3(B), dim3(64), 0, s, B, K, step, T.cand_val, T.cand_idx, T.scores,
                       T.prev_ks, T.next_ys, T.tok, T.done, T.flags);
    UIC_LAUNCH_CHECK("nmt_beam_advance_kernel");
    // decStates.beamUpdate_ (:376): re-thread every state tensor of every sentence to the surviving parents
    const int* parents = T.prev_ks + (size_t)step * R;
    for (int l = 0; l < NL; ++l)
      UIC_TRY(uic_beam_gather_launch(dt, parents, R, K, H, T.h[l][1], T.h[l][0], nullptr, nullptr, T.c[l][1], T.c[l][0], nullptr, nullptr, s));
    UIC_TRY(uic_beam_gather_launch(dt, parents, R, K, H, T.feed[1], T.feed[0], nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, s));
    // `if not active: break` (:377-378): the device freezes the search by itself (nmt_beam_begin_kernel); the host looks at the
    // flags every SYNC_EVERY steps only -- at most SYNC_EVERY - 1 speculative steps run on a finished search, and the GPU no
    // longer idles through a host round trip + 13 launches after every step
    constexpr int SYNC_EVERY = 4;
    if ((step + 1) % SYNC_EVERY == 0 && step + 1 < max_steps) {
      UIC_TRY(read_flags(T.flags, fl, s));
      if (fl[2] || fl[1] == 0) break;                    // frozen already, or this very step finished the last sentence
    }
  }
  // steps that really ran: flags[3] (a search that never froze ran them all)
  UIC_TRY(read_flags(T.flags, fl, s));
  const int n_iter = fl[3];
  *n_iter_out = n_iter;
  // (4) read-out
  hipLaunchKernelGGL(nmt_beam_readout_kernel, dim3((B + 63) / 64), dim3(64), 0, s, B, K, S, n_iter, max_steps, T.scores, T.prev_ks, T.next_ys,
                     T.attn_hist, src, hyp_out, score_out, attn_out);
  UIC_LAUNCH_CHECK("nmt_beam_readout_kernel");
  return UIC_OK;
}

}  // extern "C"
