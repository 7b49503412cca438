// The glue of the unpaired validation chain (P/eval_utils.py:329-473, eval_split_coco_unpaired), on token ids:
//
//   captioner rows  --uic_pivot_source-->  translator source batch  --uic_nmt_translate-->  hypotheses + attention
//                   --uic_pivot_target-->  caption rows in the scored vocabulary  --uic_langeval_*-->  coco_lang_stats
//
// uic_pivot_source replaces utils.decode_sequence + str.split + onmt.Dict.convertToIdx (O/Dict.py:116-132) + the padding of
// onmt.Dataset._batchify; uic_pivot_target replaces NMTModel.buildTargetTokens (P/models/NMT_Models.py:312-320) + the word
// lookup of the scorer.  The word <-> id work is done once, on the host, as three int32 tables (misc/pivot.py).
//
// No sort by length: onmt.Dataset sorts a batch for pack_padded_sequence only, and translateBatch encodes WITHOUT lengths
// (:327), so a sentence's translation depends on the padded width of its batch and not on the order of the batch's columns.
// Deviation: an empty caption becomes the one-token sentence [UNK]; the reference's readSrcLine / Dataset crash on an empty
// source line.
//
// Integer and gather work only: no floating-point atomics (max_len is an integer atomicMax, order-free), every index is
// clamped before the load that uses it, plain vector stores.
#include "uic_common.h"
#include "../../include/uic_hip.h"

namespace {

constexpr int PAD = 0, UNK = 1, EOS = 3;       // onmt.Constants
constexpr int WAVE = 64;

// one thread per caption; lanes of a wave hold neighbouring captions, so the time-major stores are coalesced
__global__ __launch_bounds__(WAVE) void pivot_source_kernel(const int64_t* __restrict__ seq, int ld_seq, int B, int L,
                                                            const int32_t* __restrict__ table, int V1, int64_t* __restrict__ src,
                                                            int32_t* __restrict__ lengths, int32_t* __restrict__ max_len) {
  const int b = blockIdx.x * WAVE + threadIdx.x;
  int len = 0;
  if (b < B) {
    const int64_t* row = seq + (size_t)b * ld_seq;
    bool ended = false;
    for (int t = 0; t < L; ++t) {
      const int64_t tok = row[t];
      ended = ended || tok <= 0;                 // 0 ends a caption; a timed-out decode leaves -1
      int64_t v = PAD;
      if (!ended) {
        v = tok < V1 ? (int64_t)table[tok] : (int64_t)UNK;
        len = t + 1;
      }
      src[(size_t)t * B + b] = v;
    }
    if (len == 0) {                              // the empty caption: [UNK]
      src[b] = UNK;
      len = 1;
    }
    lengths[b] = len;
  }
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) len = max(len, __shfl_xor(len, o, WAVE));
  if (threadIdx.x == 0) atomicMax(max_len, len);
}

// one wave per sentence
__global__ __launch_bounds__(WAVE) void pivot_target_kernel(const int64_t* __restrict__ hyp, int ld_hyp, int n_steps,
                                                            const float* __restrict__ attn, int attn_ld, int S,
                                                            const int32_t* __restrict__ src_len, const int64_t* __restrict__ seq,
                                                            int ld_seq, const int32_t* __restrict__ tgt_table, int Vt,
                                                            const int32_t* __restrict__ copy_table, int V1, int L_out,
                                                            int64_t* __restrict__ out, int32_t* __restrict__ out_len,
                                                            int32_t* __restrict__ repl) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int64_t* h = hyp + (size_t)b * ld_hyp;
  int m = n_steps;                               // first EOS column
  for (int i = lane; i < n_steps; i += WAVE)
    if (h[i] == EOS) { m = i; break; }
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o, WAVE));
  // convertToLabels(pred, EOS)[:-1]: up to and including EOS, then the last label dropped -- EOS or not
  int n = m < n_steps ? m : n_steps - 1;
  n = min(max(n, 0), L_out);
  const int sl = min(max(src_len[b], 0), min(S, ld_seq));
  for (int i = lane; i < L_out; i += WAVE) {
    int64_t o = 0;
    int r = -1;
    if (i < n) {
      const int64_t tok = h[i];
      if (tok == UNK) {
        const float* a = attn + ((size_t)b * attn_ld + i) * S;
        int j = 0;
        for (int s = 1; s < sl; ++s)
          if (a[s] > a[j]) j = s;                // lowest index on ties
        int64_t c = seq[(size_t)b * ld_seq + j];
        if (c < 0 || c >= V1) c = 0;
        o = copy_table[c];
        r = j;
      } else {
        o = tgt_table[tok >= 0 && tok < Vt ? tok : UNK];
      }
    }
    out[(size_t)b * L_out + i] = o;
    repl[(size_t)b * L_out + i] = r;
  }
  if (lane == 0) out_len[b] = n;
}

}  // namespace

extern "C" {

int uic_pivot_source(const int64_t* seq, int32_t ld_seq, int32_t B, int32_t L, const int32_t* table, int32_t V1, int64_t* src,
                     int32_t* lengths, int32_t* max_len, void* stream) {
  UIC_REQUIRE(B >= 0, "pivot_source: B=%d must be >= 0", B);
  UIC_REQUIRE(L >= 1, "pivot_source: L=%d must be >= 1", L);
  UIC_REQUIRE(ld_seq >= L, "pivot_source: ld_seq=%d must be >= L=%d", ld_seq, L);
  UIC_REQUIRE(V1 >= 1, "pivot_source: V1=%d must be >= 1", V1);
  UIC_REQUIRE(seq, "pivot_source: seq is null");
  UIC_REQUIRE(table, "pivot_source: table is null");
  UIC_REQUIRE(src, "pivot_source: src is null");
  UIC_REQUIRE(lengths, "pivot_source: lengths is null");
  UIC_REQUIRE(max_len, "pivot_source: max_len is null");
  if (B == 0) return UIC_OK;
  hipStream_t s = (hipStream_t)stream;
  UIC_TRY(uic_check_hip(hipMemsetAsync(max_len, 0, sizeof(int32_t), s), "pivot_source: memset max_len"));
  hipLaunchKernelGGL(pivot_source_kernel, dim3((B + WAVE - 1) / WAVE), dim3(WAVE), 0, s, seq, ld_seq, B, L, table, V1, src, lengths, max_len);
  UIC_LAUNCH_CHECK("pivot_source_kernel");
  return UIC_OK;
}

int uic_pivot_target(const int64_t* hyp, int32_t ld_hyp, int32_t n_steps, const float* attn, int32_t attn_ld, int32_t S,
                     const int32_t* src_len, const int64_t* seq, int32_t ld_seq, int32_t B, const int32_t* tgt_table, int32_t Vt,
                     const int32_t* copy_table, int32_t V1, int32_t L_out, int64_t* out, int32_t* out_len, int32_t* repl, void* stream) {
  UIC_REQUIRE(B >= 0, "pivot_target: B=%d must be >= 0", B);
  UIC_REQUIRE(n_steps >= 1, "pivot_target: n_steps=%d must be >= 1", n_steps);
  UIC_REQUIRE(ld_hyp >= n_steps, "pivot_target: ld_hyp=%d must be >= n_steps=%d", ld_hyp, n_steps);
  UIC_REQUIRE(attn_ld >= n_steps, "pivot_target: attn_ld=%d must be >= n_steps=%d", attn_ld, n_steps);
  UIC_REQUIRE(S >= 1, "pivot_target: S=%d must be >= 1", S);
  UIC_REQUIRE(ld_seq >= 1, "pivot_target: ld_seq=%d must be >= 1", ld_seq);
  UIC_REQUIRE(Vt >= 2, "pivot_target: Vt=%d must be >= 2 (UNK = 1 is looked up)", Vt);
  UIC_REQUIRE(V1 >= 1, "pivot_target: V1=%d must be >= 1", V1);
  UIC_REQUIRE(L_out >= 1, "pivot_target: L_out=%d must be >= 1", L_out);
  UIC_REQUIRE(hyp, "pivot_target: hyp is null");
  UIC_REQUIRE(attn, "pivot_target: attn is null");
  UIC_REQUIRE(src_len, "pivot_target: src_len is null");
  UIC_REQUIRE(seq, "pivot_target: seq is null");
  UIC_REQUIRE(tgt_table, "pivot_target: tgt_table is null");
  UIC_REQUIRE(copy_table, "pivot_target: copy_table is null");
  UIC_REQUIRE(out, "pivot_target: out is null");
  UIC_REQUIRE(out_len, "pivot_target: out_len is null");
  UIC_REQUIRE(repl, "pivot_target: repl is null");
  if (B == 0) return UIC_OK;
  hipLaunchKernelGGL(pivot_target_kernel, dim3(B), dim3(WAVE), 0, (hipStream_t)stream, hyp, ld_hyp, n_steps, attn, attn_ld, S, src_len,
                     seq, ld_seq, tgt_table, Vt, copy_table, V1, L_out, out, out_len, repl);
  UIC_LAUNCH_CHECK("pivot_target_kernel");
  return UIC_OK;
}

}  // extern "C"
