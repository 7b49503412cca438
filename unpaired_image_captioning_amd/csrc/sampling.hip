// Token draws on the device (gfx950): the scheduled-sampling draw of the training loop (P/models/AttModel.py:130-143), one
// decode step of AttModel._sample (P/models/AttModel.py:216-251) with its finished-row bookkeeping, and the clean-up of
// FCModel_NMT._sample's early break (P/models/FCModel_NMT.py:203-206).  No host sync anywhere: the reference's
// `unfinished.sum() == 0` is a device counter per step.
#include "uic_common.h"
#include "../../include/uic_hip.h"

namespace {

constexpr int NT = 256;

// ------------------------------------------------------------------ scheduled sampling (AttModel.py:130-143)
// One block per caption row: rows whose uniform falls under ss_prob take an inverse-CDF draw from
// softmax(previous step's logits) (= exp(outputs[:, i-1]), torch.multinomial's distribution); the others keep seq[:, i].
__global__ __launch_bounds__(NT) void ss_sample_kernel(const float* __restrict__ logits, int V1, int ldv,
                                                       const int64_t* __restrict__ labels, int ld_labels, int t, float ss_prob,
                                                       unsigned seed, int64_t* __restrict__ used, int ld_used) {
  __shared__ float s_buf[NT / 64];
  __shared__ float s_val[NT];
  const int n = blockIdx.x;
  if (!(uic_uniform(seed, UIC_SITE_SS_MASK0 + (unsigned)t, (unsigned)n) < ss_prob)) {
    if (threadIdx.x == 0) used[(size_t)n * ld_used + t] = labels[(size_t)n * ld_labels + t];
    return;
  }
  const float* row = logits + (size_t)n * ldv;
  float mx = -INFINITY;
  for (int v = threadIdx.x; v < V1; v += NT) mx = fmaxf(mx, row[v]);
  mx = uic_block_max<NT>(mx, s_buf);
  const int per = (V1 + NT - 1) / NT;
  const int v_lo = threadIdx.x * per, v_hi = min(V1, v_lo + per);
  float part = 0.f;
  for (int v = v_lo; v < v_hi; ++v) part += expf(row[v] - mx);
  s_val[threadIdx.x] = part;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int i = 0; i < NT; ++i) tot += s_val[i];
    const float target = uic_uniform(seed, UIC_SITE_SS_DRAW0 + (unsigned)t, (unsigned)n) * tot;
    float cum = 0.f;
    int seg = NT - 1;
    for (int i = 0; i < NT; ++i) {
      if (cum + s_val[i] > target) { seg = i; break; }
      cum += s_val[i];
    }
    int pick = -1;
    const int lo = seg * per, hi = min(V1, lo + per);
    for (int v = lo; v < hi; ++v) {
      const float pr = expf(row[v] - mx);
      if (pr > 0.f) pick = v;
      cum += pr;
      if (cum > target && pr > 0.f) break;
    }
    if (pick < 0) pick = 0;
    used[(size_t)n * ld_used + t] = pick;
  }
}
__global__ void copy_tokens_kernel(const int64_t* __restrict__ src, int ld_src, int N, int T, int64_t* __restrict__ dst, int ld_dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * T) return;
  const int n = i / T, t = i - n * T;
  dst[(size_t)n * ld_dst + t] = src[(size_t)n * ld_src + t];
}

// ------------------------------------------------------------------ one decode step of AttModel._sample
// (P/models/AttModel.py:216-251): log_softmax, optional decoding constraint, greedy max (lowest index on
// ties) or multinomial draw, finished-row bookkeeping.  The reference's host-side early break
// (`unfinished.sum() == 0`) becomes a device counter per step, so no host sync is needed.
// STAGED: the logits row is copied into LDS once (16-byte loads) and every pass below reads it from there; rows too long
// for 64 KB of LDS are read from memory by each pass.  Same arithmetic in the same order either way.
// FAST (bf16 models): hardware exp; the f32 parity path keeps libm's
template <bool STAGED, bool FAST>
__global__ __launch_bounds__(NT) void sample_step_kernel(const UicSampleParams p) {
  auto ex = [](float x) { return FAST ? __expf(x) : expf(x); };
  __shared__ float s_buf[NT / 64];
  __shared__ float s_val[NT];
  __shared__ int s_idx[NT];
  extern __shared__ __attribute__((aligned(16))) float s_row[];
  const int n = blockIdx.x;
  const int t = p.t;
  const float* grow = (const float*)p.logits + (size_t)n * p.ldv;
  const float* row = grow;
  if constexpr (STAGED) {
    const int n4 = p.V1 >> 2;
    for (int i = threadIdx.x; i < n4; i += NT) *(float4*)(s_row + 4 * i) = *(const float4*)(grow + 4 * i);
    for (int v = (n4 << 2) + threadIdx.x; v < p.V1; v += NT) s_row[v] = grow[v];
    __syncthreads();
    row = s_row;
  }
  bool dead = false;                                                       // every row had finished: the reference broke out
  if (!p.fc_mode && t > 0) {
    int live = threadIdx.x < UIC_NUNF_STRIPES ? p.n_unfinished[(t - 1) * UIC_NUNF_STRIPES + threadIdx.x] : 0;
    dead = __syncthreads_or(live) == 0;
  }
  long banned = -1;
  const int ldo = p.ld_out > 0 ? p.ld_out : p.L;
  if (p.decoding_constraint && t > 0) banned = p.seq[(size_t)n * ldo + t - 1];

  float mx = -INFINITY;
  for (int v = threadIdx.x; v < p.V1; v += NT) mx = fmaxf(mx, row[v]);
  mx = uic_block_max<NT>(mx, s_buf);
  float sum = 0.f;
  for (int v = threadIdx.x; v < p.V1; v += NT) sum += ex(row[v] - mx);
  sum = uic_block_sum<NT>(sum, s_buf);
  const float lse = mx + logf(sum);
  if (p.logprobs_out)
    for (int v = threadIdx.x; v < p.V1; v += NT) p.logprobs_out[(size_t)n * p.V1 + v] = row[v] - lse;

  int choice = 0;
  if (p.sample_max) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int v = threadIdx.x; v < p.V1; v += NT) {
      const float x = (v == banned) ? -INFINITY : row[v];
      if (x > bv || (x == bv && v < bi)) { bv = x; bi = v; }
    }
    uic_block_argmax<NT>(bv, bi, s_val, s_idx);      // (value descending, lowest index on ties)
    choice = bi;
  } else if (p.forced) {
    choice = (int)p.forced[(size_t)n * p.L + t];
  } else {
    // inverse-CDF draw from softmax(logprobs / temperature) with the banned token removed.  Thread i owns the contiguous
    // vocabulary segment [i * per, (i + 1) * per); an inclusive scan of the segment masses (wave shuffles + one LDS exchange
    // between the waves) finds the segment the uniform number falls into, and only that segment's owner walks its <= per
    // entries.  (The first version summed and searched the NT segment masses on thread 0: two serial loops of NT LDS reads,
    // ~14 us of the kernel's 32.)
    const float invT = 1.f / p.temperature;
    float part = 0.f;
    const int per = (p.V1 + NT - 1) / NT;
    const int v_lo = threadIdx.x * per, v_hi = min(p.V1, v_lo + per);
    for (int v = v_lo; v < v_hi; ++v) part += (v == banned) ? 0.f : ex((row[v] - lse) * invT);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float incl = part;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    __syncthreads();                                   // s_buf was last read by uic_block_sum
    if (lane == 63) s_buf[wv] = incl;
    __syncthreads();
    float woff = 0.f, tot = 0.f;
#pragma unroll
    for (int w2 = 0; w2 < NT / 64; ++w2) {
      if (w2 < wv) woff += s_buf[w2];
      tot += s_buf[w2];
    }
    incl += woff;
    s_val[threadIdx.x] = incl;
    if (threadIdx.x == 0) s_idx[0] = -1;
    __syncthreads();
    unsigned x = (unsigned)n * 0x9E3779B1u ^ (p.seed + (unsigned)t * 0x85EBCA77u);
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    const float target = (float)(x >> 8) * (1.0f / 16777216.0f) * tot;
    const float below = threadIdx.x > 0 ? s_val[threadIdx.x - 1] : 0.f;
    // the owner: the first segment whose inclusive mass exceeds the target (the last one if rounding leaves none)
    const bool owner = (incl > target && !(below > target)) || (threadIdx.x == NT - 1 && !(incl > target));
    if (owner) {
      float cum = below;
      int pick = -1;
      for (int v = v_lo; v < v_hi; ++v) {
        const float pr = (v == banned) ? 0.f : ex((row[v] - lse) * invT);
        if (pr > 0.f) pick = v;
        cum += pr;
        if (cum > target && pr > 0.f) break;
      }
      s_idx[0] = pick;
    }
    __syncthreads();
    if (s_idx[0] < 0) {
      // rounding left the target at or beyond the total mass and the last segment is empty: the last token that has mass (rare)
      if (threadIdx.x == 0) {
        int pick = 0;
        for (int v = p.V1 - 1; v >= 0; --v)
          if (v != banned && ex((row[v] - lse) * invT) > 0.f) { pick = v; break; }
        s_idx[0] = pick;
      }
      __syncthreads();
    }
    choice = s_idx[0];
  }
  if (threadIdx.x == 0) {
    if (dead) {
      p.seq[(size_t)n * ldo + t] = 0;
      p.seq_logp[(size_t)n * ldo + t] = 0.f;
      p.it[n] = 0;
    } else {
      const float lp = row[choice] - lse;
      int unf = choice > 0;
      if (t > 0) unf = unf && p.unfinished[n];
      p.unfinished[n] = unf;
      const long tok = unf ? choice : 0;
      p.it[n] = p.fc_mode ? (long)choice : tok;      // FCModel_NMT feeds the RAW sampled token to the next step (:199)
      p.seq[(size_t)n * ldo + t] = tok;
      p.seq_logp[(size_t)n * ldo + t] = lp;
      if (unf) atomicAdd(&p.n_unfinished[t * UIC_NUNF_STRIPES + (n % UIC_NUNF_STRIPES)], 1);
    }
  }
  if (p.xt_out) {   // the next step's input embedding of this row (embed_fwd_kernel's arithmetic)
    __syncthreads();                                   // (s_idx[0] was read by everybody above)
    if (threadIdx.x == 0) s_idx[0] = (int)p.it[n];
    __syncthreads();
    long tok = s_idx[0];
    if (tok < 0 || tok >= p.embed_V1) tok = 0;
    const int E = p.embed_E;
    const float inv_keep = p.embed_drop_p > 0.f ? 1.f / (1.f - p.embed_drop_p) : 1.f;
    for (int c = threadIdx.x * 4; c < E; c += NT * 4) {
      float f[4];
      if (p.embed_table_dtype == UIC_BF16) uic_table_load4((const bf16_t*)p.embed_table + (size_t)tok * E + c, f);
      else uic_table_load4((const float*)p.embed_table + (size_t)tok * E + c, f);
#pragma unroll
      for (int j = 0; j < 4; ++j) f[j] = fmaxf(f[j], 0.f);
      if (p.embed_drop_p > 0.f) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          f[j] *= uic_drop_scale(p.seed, p.embed_site, (unsigned)(p.embed_idx_base + (size_t)n * E + c + j), p.embed_drop_p, inv_keep);
      }
      if (p.dtype == UIC_BF16) {
        bf16_t* o = (bf16_t*)p.xt_out + (size_t)n * E + c;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (bf16_t)f[j];
      } else {
        *(float4*)((float*)p.xt_out + (size_t)n * E + c) = make_float4(f[0], f[1], f[2], f[3]);
      }
    }
  }
}

// FCModel_NMT._sample breaks BEFORE writing the step at which every row has finished (:203-206): zero that
// column and everything after it.
__global__ void sample_fixup_kernel(int N, int L, int ld, const int* n_unfinished, int64_t* seq, float* seq_logp) {
  int first = L;
  for (int t = 0; t < L; ++t) {
    int live = 0;
    for (int k = 0; k < UIC_NUNF_STRIPES; ++k) live += n_unfinished[t * UIC_NUNF_STRIPES + k];
    if (live == 0) { first = t; break; }
  }
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N * ld; i += gridDim.x * blockDim.x) {
    const int t = i % ld;
    if (t >= first) { seq[i] = 0; seq_logp[i] = 0.f; }
  }
}

// The gradient weights of a kept FCModel_NMT sampling pass (uic_fc_reward_backward): d logits[t, n, :] =
// dlogp[n, t] (onehot - softmax) = (softmax - onehot) * scale[n, t] with scale = -dlogp for the steps the pass ran.  The
// reference never wrote the column at which every row had finished, nor anything behind it (:203-206) -- seqLogprobs is a
// constant 0 there -- so those columns weigh +0, like every position whose dlogp is 0 (behind a caption's end).
__global__ void sample_reward_scale_kernel(int N, int L, int ld, const int* n_unfinished, const float* dlogp, float* scale) {
  int first = L;
  for (int t = 0; t < L; ++t) {
    int live = 0;
    for (int k = 0; k < UIC_NUNF_STRIPES; ++k) live += n_unfinished[t * UIC_NUNF_STRIPES + k];
    if (live == 0) { first = t; break; }
  }
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N * ld; i += gridDim.x * blockDim.x) {
    const float g = dlogp[i];
    scale[i] = (i % ld >= first || g == 0.f) ? 0.f : -g;
  }
}

}  // namespace

int uic_ss_sample_launch(const float* logits_prev, int N, int V1, int ldv, const int64_t* labels, int ld_labels, int t,
                         float ss_prob, unsigned seed, int64_t* used, int ld_used, hipStream_t s) {
  UIC_REQUIRE(logits_prev && labels && used && t >= 1 && t < 256, "ss_sample: bad arguments (t=%d)", t);
  if (N == 0) return UIC_OK;
  hipLaunchKernelGGL(ss_sample_kernel, dim3(N), dim3(NT), 0, s, logits_prev, V1, ldv, labels, ld_labels, t, ss_prob, seed, used, ld_used);
  UIC_LAUNCH_CHECK("ss_sample");
  return UIC_OK;
}
int uic_copy_tokens_launch(const int64_t* src, int ld_src, int N, int T, int64_t* dst, int ld_dst, hipStream_t s) {
  if (N * T == 0) return UIC_OK;
  hipLaunchKernelGGL(copy_tokens_kernel, dim3((N * T + NT - 1) / NT), dim3(NT), 0, s, src, ld_src, N, T, dst, ld_dst);
  UIC_LAUNCH_CHECK("copy_tokens");
  return UIC_OK;
}
int uic_sample_step_launch(const UicSampleParams& p, hipStream_t s) {
  UIC_REQUIRE(p.logits && p.seq && p.seq_logp && p.it && p.unfinished && p.n_unfinished, "sample_step: null pointer");
  UIC_REQUIRE(p.t >= 0 && p.t < p.L, "sample_step: t=%d outside [0,%d)", p.t, p.L);
  if (p.N == 0) return UIC_OK;
  const size_t row_bytes = ((size_t)p.V1 * 4 + 15) & ~(size_t)15;
  const bool staged = row_bytes <= 60 * 1024 && p.ldv % 4 == 0 && ((uintptr_t)p.logits & 15) == 0;
  const bool fast = p.dtype == UIC_BF16;
  if (staged && fast) hipLaunchKernelGGL((sample_step_kernel<true, true>), dim3(p.N), dim3(NT), row_bytes, s, p);
  else if (staged) hipLaunchKernelGGL((sample_step_kernel<true, false>), dim3(p.N), dim3(NT), row_bytes, s, p);
  else if (fast) hipLaunchKernelGGL((sample_step_kernel<false, true>), dim3(p.N), dim3(NT), 0, s, p);
  else hipLaunchKernelGGL((sample_step_kernel<false, false>), dim3(p.N), dim3(NT), 0, s, p);
  UIC_LAUNCH_CHECK("sample_step");
  return UIC_OK;
}
int uic_sample_fixup_launch(int N, int L, int ld, const int* n_unfinished, int64_t* seq, float* seq_logp, hipStream_t s) {
  hipLaunchKernelGGL(sample_fixup_kernel, dim3(8), dim3(NT), 0, s, N, L, ld, n_unfinished, seq, seq_logp);
  UIC_LAUNCH_CHECK("sample_fixup");
  return UIC_OK;
}
int uic_sample_reward_scale_launch(int N, int L, int ld, const int* n_unfinished, const float* dlogp, float* scale, hipStream_t s) {
  UIC_REQUIRE(n_unfinished && dlogp && scale && L <= ld, "sample_reward_scale: bad arguments");
  hipLaunchKernelGGL(sample_reward_scale_kernel, dim3(8), dim3(NT), 0, s, N, L, ld, n_unfinished, dlogp, scale);
  UIC_LAUNCH_CHECK("sample_reward_scale");
  return UIC_OK;
}
