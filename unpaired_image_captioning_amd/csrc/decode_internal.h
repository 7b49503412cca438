// The host side of decoding that every captioner shares (TopDown and its ensemble, FC, Transformer, AdaAtt): the buffers of the
// beam kernels (beam.hip) and of the sampling kernel (sampling.hip), how a search or a sampling pass starts, the beam loop, and
// the export of the finished-beam lists.  The rules of those buffers -- their shapes, which history generation a step reads, one
// done_count entry per image -- are written here once; a model supplies its logits, its token buffer and its step.
#pragma once
#include "uic_common.h"
#include "uic_host.h"
#include <string.h>

namespace {

// ---------------------------------------------------------------- beam search bookkeeping (rows = (image, beam))
struct BeamScratch {
  float* bm_cand_val; int* bm_cand_idx;          // [rows, UIC_BEAM_MAX]
  int64_t* bm_seq[2]; float* bm_lp[2];           // [rows, cap] x 2 generations (a step reads t & 1, writes the other)
  float* bm_sum; int* bm_parent;                 // [rows]
  // the done lists, contiguous from bm_done_count to the end of bm_done_lp (done_bytes, alignment gaps included)
  int* bm_done_count;                            // [n_count]; the kernels use one entry per image
  float* bm_done_p;                              // [rows, cap]      of which the kernels use [n_img, L*B]
  int64_t* bm_done_seq; float* bm_done_lp;       // [rows, cap, cap] of which the kernels use [n_img, L*B, L]
  size_t done_bytes;
  // cap: the step capacity (the longest search).  n_count: TopDown and FC give every row a done_count entry, the Transformer and
  // AdaAtt every image.
  void carve(Bump& b, size_t rows, size_t n_count, size_t cap) {
    bm_cand_val = (float*)b.take(rows * UIC_BEAM_MAX * 4);
    bm_cand_idx = (int*)b.take(rows * UIC_BEAM_MAX * 4);
    for (int i = 0; i < 2; ++i) {
      bm_seq[i] = (int64_t*)b.take(rows * cap * 8);
      bm_lp[i] = (float*)b.take(rows * cap * 4);
    }
    bm_sum = (float*)b.take(rows * 4);
    bm_parent = (int*)b.take(rows * 4);
    bm_done_count = (int*)b.take(n_count * 4);
    const size_t done0 = b.off - n_count * 4;
    bm_done_p = (float*)b.take(rows * cap * 4);
    bm_done_seq = (int64_t*)b.take(rows * cap * cap * 8);
    bm_done_lp = (float*)b.take(rows * cap * cap * 4);
    done_bytes = b.off - done0;
  }
};

// The bookkeeping cleared (both history generations whole, the sums, the done lists) and the beam kernels' parameters over it.
// The kernels write an image's first done_count entries only and beam_done_lists copies whole arrays: one fill over the counts
// AND the three lists behind them, so that what the export hands out behind an image's count is zeros, not an earlier search's
// beams.  logits [n_img * B, ldv] and it [n_img * B] are the model's; cap is what carve() was given.
inline int beam_begin(const BeamScratch& bs, const float* logits, int ldv, int64_t* it, int n_img, int B, int cap, int V1, int Lsteps,
                      int decoding_constraint, int max_ppl, UicBeamParams& p, hipStream_t s) {
  const size_t rows = (size_t)n_img * B;
  for (int i = 0; i < 2; ++i) {
    UIC_TRY(uic_fill_launch(bs.bm_seq[i], 0, rows * cap * 8, s));
    UIC_TRY(uic_fill_launch(bs.bm_lp[i], 0, rows * cap * 4, s));
  }
  UIC_TRY(uic_fill_launch(bs.bm_sum, 0, rows * 4, s));
  UIC_TRY(uic_fill_launch(bs.bm_done_count, 0, bs.done_bytes, s));
  memset(&p, 0, sizeof(p));
  p.n_img = n_img; p.B = B; p.L = Lsteps; p.V1 = V1; p.ldv = ldv;
  p.decoding_constraint = decoding_constraint; p.max_ppl = max_ppl;
  p.logits = logits; p.cand_val = bs.bm_cand_val; p.cand_idx = bs.bm_cand_idx;
  p.beam_seq_hist[0] = bs.bm_seq[0]; p.beam_seq_hist[1] = bs.bm_seq[1]; p.beam_lp_hist[0] = bs.bm_lp[0]; p.beam_lp_hist[1] = bs.bm_lp[1];
  p.beam_sum = bs.bm_sum; p.parent = bs.bm_parent; p.it = it;
  p.done_count = bs.bm_done_count; p.done_p = bs.bm_done_p; p.done_seq = bs.bm_done_seq; p.done_lp = bs.bm_done_lp;
  return UIC_OK;
}

// CaptionModel.beam_search's loop (P/models/CaptionModel.py:56-120) over p.logits, which hold the log-probs after <bos> on entry.
// advance(t_next) is the model's: its states follow the surviving parents (p.parent, CaptionModel.py:90-92), then its
// get_logprobs_state of p.it for step t_next leaves the next logits.
template <typename Advance>
inline int beam_search(UicBeamParams& p, int Lsteps, Advance advance, hipStream_t s, int64_t* seq, float* seq_logp) {
  for (int t = 0; t < Lsteps; ++t) {
    p.t = t;
    UIC_TRY(uic_beam_step_launch(p, s));
    if (t + 1 == Lsteps) break;                                // (the reference's last get_logprobs_state is never used)
    UIC_TRY(advance(t + 1));
  }
  return uic_beam_final_launch(p, seq, seq_logp, s);
}

// the finished beams of the last search: done_count [n_img], done_p [n_img, L*B], done_seq / done_lp [n_img, L*B, L]; zeros behind
// an image's count
inline int beam_done_lists(const BeamScratch& bs, size_t n_img, size_t Lsteps, size_t B, int32_t* done_count, float* done_p, int64_t* done_seq,
                           float* done_lp, hipStream_t s) {
  const size_t LB = Lsteps * B;
  UIC_TRY(uic_copy_launch(done_count, bs.bm_done_count, n_img * 4, s));
  UIC_TRY(uic_copy_launch(done_p, bs.bm_done_p, n_img * LB * 4, s));
  UIC_TRY(uic_copy_launch(done_seq, bs.bm_done_seq, n_img * LB * Lsteps * 8, s));
  return uic_copy_launch(done_lp, bs.bm_done_lp, n_img * LB * Lsteps * 4, s);
}

// ---------------------------------------------------------------- the sampling kernel's token, flags and counters
struct SampleScratch {
  int64_t* it;          // [rows] next input token
  int* unfinished;      // [rows]
  int* n_unfinished;    // [(cap + 2) * UIC_NUNF_STRIPES] live-row counters per step, striped
  void carve(Bump& b, size_t rows, size_t cap) {
    it = (int64_t*)b.take(rows * 8);
    unfinished = (int*)b.take(rows * 4);
    n_unfinished = (int*)b.take((cap + 2) * UIC_NUNF_STRIPES * 4);
  }
};

// <bos> = 0 as the first input of `rows` rows, the flags and all counters cleared; seq / seq_logp [n_out] too where the model's
// kernels do not write every element (seq == null: the caller's buffers stay as they are)
inline int sample_begin(const SampleScratch& sc, size_t rows, size_t cap, int64_t* seq, float* seq_logp, size_t n_out, hipStream_t s) {
  UIC_TRY(uic_fill_launch(sc.it, 0, rows * 8, s));
  UIC_TRY(uic_fill_launch(sc.unfinished, 0, rows * 4, s));
  UIC_TRY(uic_fill_launch(sc.n_unfinished, 0, (cap + 2) * UIC_NUNF_STRIPES * 4, s));
  if (!seq) return UIC_OK;
  UIC_TRY(uic_fill_launch(seq, 0, n_out * 8, s));
  return uic_fill_launch(seq_logp, 0, n_out * 4, s);
}

// step t of a sampling pass over `logits` [N, vpad(V1)]
inline UicSampleParams sample_params(const SampleScratch& sc, int dtype, int N, int V1, int t, int Lsteps, const float* logits, int sample_max,
                                     float temperature, int decoding_constraint, unsigned seed, const int64_t* forced, int64_t* seq,
                                     float* seq_logp) {
  UicSampleParams p;
  memset(&p, 0, sizeof(p));
  p.dtype = dtype; p.N = N; p.V1 = V1; p.ldv = (int)vpad(V1); p.t = t; p.L = Lsteps;
  p.logits = logits; p.sample_max = sample_max; p.temperature = temperature; p.seed = seed;
  p.decoding_constraint = decoding_constraint;
  p.seq = seq; p.seq_logp = seq_logp; p.it = sc.it; p.unfinished = sc.unfinished; p.n_unfinished = sc.n_unfinished;
  p.forced = forced;
  return p;
}

}  // namespace
