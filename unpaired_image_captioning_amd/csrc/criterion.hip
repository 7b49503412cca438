// log_softmax over the vocabulary (AttModel.py:163) fused with the masked NLL and its gradient (LanguageModelCriterion,
// criterion.py:143-150: d logits = (softmax - onehot) * mask / sum(mask)), one workgroup per (t, n) row of logits (gfx950).
// Five kernels for five row lengths / outputs (uic_xe_launch picks); what they share -- the position of a row, its target and
// mask, the accuracy counters, the gradient weight, the 4-wide gradient store, the log-prob row -- is written once, below.
// Behind them the two criteria on materialised log-probs of the single-operator API: LanguageModelCriterion
// (criterion.py:143-150) and RewardCriterion (criterion.py:117-124).
#include "uic_common.h"
#include "../../include/uic_hip.h"

namespace {

constexpr int NT = 256;

// ------------------------------------------------------------------ the shared pieces
// (They take UicXeParams BY VALUE, as the kernels do: behind a reference hipcc allocated two more registers in xe_reg_kernel
// and spilled four more in xe_reg_wide_kernel, which sits on the 128-register limit of a 1024-thread workgroup.)
// The position (t, n) of the logits row of this workgroup.  row_map: the rows are a compacted list of (step, row) positions;
// -1 (or out of range) = a padding row: zero gradient, no loss entry (it reads position 0's target and mask slots, unused).
struct XePos { int m; bool pad; int t, n; };
__device__ __forceinline__ XePos xe_pos(const UicXeParams p) {
  XePos q;
  q.m = blockIdx.x;
  const int mr = p.row_map ? p.row_map[q.m] : q.m;
  q.pad = p.row_map && (unsigned)mr >= (unsigned)p.row_map_limit;
  const int mo = q.pad ? 0 : mr;
  q.t = mo / p.N;
  q.n = mo - q.t * p.N;
  return q;
}

// Target and mask of a position (p.target != null): y0 the raw target (0 for a padding row), y the one that is scored
// (0 when y0 is outside [0, V1)), mk the mask (0 for a padding row or without a mask).
struct XeTarget { long y0, y; float mk; };
__device__ __forceinline__ XeTarget xe_target(const UicXeParams p, const XePos q) {
  XeTarget g;
  g.y0 = q.pad ? 0 : p.target[(size_t)q.n * p.ldtarget + p.target_col0 + q.t];
  g.mk = p.mask && !q.pad ? p.mask[(size_t)q.n * p.ldmask + p.mask_col0 + q.t] : 0.f;
  g.y = g.y0 < 0 || g.y0 >= p.V1 ? 0 : g.y0;
  return g;
}

// The accuracy counters of NMT_loss.score (criterion.py:175-184): [1] counts the rows whose raw target is not 0, [0] those
// whose arg-max (lowest index on ties) is that target; the mask plays no part.  One thread of the workgroup adds.
__device__ __forceinline__ void xe_count(const UicXeParams p, long y0, int argmax) {
  if (threadIdx.x == 0 && p.score_stats && y0 != 0) {
    atomicAdd(&p.score_stats[1], 1);
    if (argmax == (int)y0) atomicAdd(&p.score_stats[0], 1);
  }
}

// The weight of a position's gradient: the self-critical weight if given, else mask / sum(mask).
__device__ __forceinline__ float xe_weight(const UicXeParams p, const XePos q, float mk) {
  return p.grad_scale ? p.grad_scale[(size_t)q.n * p.ldscale + p.scale_col0 + q.t] : mk * p.inv_den[0];
}

// Four consecutive gradient columns in one store (8 bytes of bf16 or 16 of f32), and the all-zero row of a position that has
// no gradient, by the same stores.
template <typename T>
__device__ __forceinline__ void xe_store4(T* d, float g0, float g1, float g2, float g3) {
  if constexpr (sizeof(T) == 2) {
    *(uint2*)d = make_uint2(uic_pack_bf16x2(g0, g1), uic_pack_bf16x2(g2, g3));
  } else {
    *(float4*)d = make_float4(g0, g1, g2, g3);
  }
}
template <typename T, int NTH>
__device__ __forceinline__ void xe_zero_row(T* d, int ldv) {
  for (int v = threadIdx.x * 4; v < ldv; v += NTH * 4) {
    if constexpr (sizeof(T) == 2) *(uint2*)(d + v) = make_uint2(0u, 0u);
    else *(float4*)(d + v) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
// columns v .. v + 3 of (softmax - onehot(y)) * sc from the logits x[0..3] and the row's log-sum-exp (hardware exp; the
// padding columns [V1, ldv) get zeros)
template <typename T>
__device__ __forceinline__ void xe_grad4(T* d, const float* x, int v, long y, int V1, float lse, float sc) {
  float g[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int vv = v + j;
    g[j] = vv < V1 ? (__expf(x[j] - lse) - (vv == y ? 1.f : 0.f)) * sc : 0.f;
  }
  xe_store4(d + v, g[0], g[1], g[2], g[3]);
}

// The log-probabilities of a row, logprobs[n][t][v]; `src` (the logits row) may be LDS or global.
__device__ __forceinline__ void xe_write_logprobs(const UicXeParams p, const XePos q, const float* src, float lse) {
  float* lp = p.logprobs + (size_t)q.n * p.lp_row_stride + (size_t)q.t * p.lp_step_stride;
  for (int v = threadIdx.x; v < p.V1; v += NT) lp[v] = src[v] - lse;
}

// arg-max of a row (lowest index on ties) for the accuracy counters; `src` may be LDS or global
__device__ __forceinline__ int xe_row_argmax(const float* src, int V1, float* s_bv, int* s_bi) {
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int v = threadIdx.x; v < V1; v += NT) {
    const float x = src[v];
    if (x > bv || (x == bv && v < bi)) { bv = x; bi = v; }
  }
  uic_block_argmax<NT>(bv, bi, s_bv, s_bi);
  return bi;
}

// What the three kernels that hold the row in memory (`src`: LDS or global) do once they know its log-sum-exp: the loss entry,
// the accuracy counters, the log-probabilities.  Returns the scored target and the mask for the gradient pass.
// FIND_ARGMAX: the arg-max is not known yet and costs one more pass over the row when the counters are wanted.
template <bool FIND_ARGMAX>
__device__ __forceinline__ XeTarget xe_loss_and_outputs(const UicXeParams p, const XePos q, const float* src, float lse, int argmax) {
  XeTarget g = {0, 0, 0.f};
  if (p.target) {
    g = xe_target(p, q);
    if (p.score_stats) {
      if constexpr (FIND_ARGMAX) {
        __shared__ float s_bv[NT / 64];
        __shared__ int s_bi[NT / 64];
        argmax = xe_row_argmax(src, p.V1, s_bv, s_bi);
      }
      xe_count(p, g.y0, argmax);
    }
    if (threadIdx.x == 0 && !q.pad) p.row_loss[q.m] = -(src[g.y] - lse) * g.mk;
  }
  if (p.logprobs) xe_write_logprobs(p, q, src, lse);
  return g;
}

// ------------------------------------------------------------------ any dtype, any ldv
// Three passes over the row in global memory, libm exp (the f32 parity path).
template <typename T>
__global__ __launch_bounds__(NT) void xe_kernel(const UicXeParams p, const float* __restrict__ logits, T* __restrict__ dlogits) {
  __shared__ float s_buf[NT / 64];
  const XePos q = xe_pos(p);
  const float* row = logits + (size_t)q.m * p.ldv;
  float mx = -INFINITY;
  for (int v = threadIdx.x; v < p.V1; v += NT) mx = fmaxf(mx, row[v]);
  mx = uic_block_max<NT>(mx, s_buf);
  float sum = 0.f;
  for (int v = threadIdx.x; v < p.V1; v += NT) sum += expf(row[v] - mx);
  sum = uic_block_sum<NT>(sum, s_buf);
  const float lse = mx + logf(sum);
  const XeTarget g = xe_loss_and_outputs<true>(p, q, row, lse, 0);
  if (p.write_grad) {
    const float sc = xe_weight(p, q, g.mk);
    T* d = dlogits + (size_t)q.m * p.ldv;
    for (int v = threadIdx.x; v < p.ldv; v += NT) {
      float gr = 0.f;
      if (v < p.V1) gr = (expf(row[v] - lse) - (v == g.y ? 1.f : 0.f)) * sc;
      d[v] = uic_from_f<T>(gr);
    }
  }
}

// ------------------------------------------------------------------ bf16, rows of any length
// Rows too long for LDS (the 50 004-word NMT generator: 200 KB per row): TWO passes over the row instead of three --
// pass 1 keeps a running (max, sum of exp) per thread (rescaled when the max moves) together with the arg-max, pass 2
// writes the gradient -- with 16-byte loads.  The arg-max feeds the accuracy counters, which otherwise cost a third pass.
template <typename T>
__global__ __launch_bounds__(NT) void xe_big_kernel(const UicXeParams p, const float* __restrict__ logits, T* __restrict__ dlogits) {
  __shared__ float s_m[NT / 64], s_s[NT / 64], s_bv[NT / 64];
  __shared__ int s_bi[NT / 64];
  const XePos q = xe_pos(p);
  const float* row = logits + (size_t)q.m * p.ldv;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float mx = -INFINITY, sum = 0.f, bv = -INFINITY;
  int bi = 0x7fffffff;
  auto take = [&](float x, int v) {
    if (x > bv || (x == bv && v < bi)) { bv = x; bi = v; }
    if (x > mx) { sum = sum * __expf(mx - x) + 1.f; mx = x; }
    else if (mx != -INFINITY) sum += __expf(x - mx);          // (x = mx = -inf contributes nothing)
  };
  for (int v = threadIdx.x * 4; v < p.V1; v += NT * 4) {
    const float4 x = *(const float4*)(row + v);            // ldv is a multiple of 4 and >= V1: in bounds
    take(x.x, v);
    if (v + 1 < p.V1) take(x.y, v + 1);
    if (v + 2 < p.V1) take(x.z, v + 2);
    if (v + 3 < p.V1) take(x.w, v + 3);
  }
  // the combined merge of two partial (max, rescaled sum, arg-max) triples: not one of uic_common.h's workgroup reductions
  auto merge = [&](float om, float os, float ov, int oi) {
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    const float nm = fmaxf(mx, om);
    if (nm != -INFINITY) sum = sum * __expf(mx - nm) + os * __expf(om - nm);
    mx = nm;
  };
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    merge(__shfl_xor(mx, o, 64), __shfl_xor(sum, o, 64), __shfl_xor(bv, o, 64), __shfl_xor(bi, o, 64));
  if (lane == 0) { s_m[wave] = mx; s_s[wave] = sum; s_bv[wave] = bv; s_bi[wave] = bi; }
  __syncthreads();
  mx = s_m[0]; sum = s_s[0]; bv = s_bv[0]; bi = s_bi[0];
#pragma unroll
  for (int w2 = 1; w2 < NT / 64; ++w2) merge(s_m[w2], s_s[w2], s_bv[w2], s_bi[w2]);
  const float lse = mx + logf(sum);
  const XeTarget g = xe_loss_and_outputs<false>(p, q, row, lse, bi);
  if (p.write_grad) {
    const float sc = xe_weight(p, q, g.mk);
    T* d = dlogits + (size_t)q.m * p.ldv;
    for (int v = threadIdx.x * 4; v < p.ldv; v += NT * 4) {
      const float4 x = *(const float4*)(row + v);
      const float xs[4] = {x.x, x.y, x.z, x.w};
      xe_grad4(d, xs, v, g.y, p.V1, lse, sc);
    }
  }
}

// ------------------------------------------------------------------ bf16, rows up to 64 KB, every output
// The logits row staged once in LDS: one HBM read of the 413 MB logits tensor instead of three.
template <typename T>
__global__ __launch_bounds__(NT) void xe_lds_kernel(const UicXeParams p, const float* __restrict__ logits, T* __restrict__ dlogits) {
  extern __shared__ __attribute__((aligned(16))) float s_row[];
  __shared__ float s_buf[NT / 64];
  const XePos q = xe_pos(p);
  const float* row = logits + (size_t)q.m * p.ldv;
  float mx = -INFINITY;
  for (int v = threadIdx.x * 4; v < p.ldv; v += NT * 4) {
    const float4 x = *(const float4*)(row + v);
    *(float4*)(s_row + v) = x;
    if (v < p.V1) mx = fmaxf(mx, x.x);
    if (v + 1 < p.V1) mx = fmaxf(mx, x.y);
    if (v + 2 < p.V1) mx = fmaxf(mx, x.z);
    if (v + 3 < p.V1) mx = fmaxf(mx, x.w);
  }
  mx = uic_block_max<NT>(mx, s_buf);
  float sum = 0.f;
  for (int v = threadIdx.x; v < p.V1; v += NT) sum += __expf(s_row[v] - mx);
  sum = uic_block_sum<NT>(sum, s_buf);
  const float lse = mx + logf(sum);
  const XeTarget g = xe_loss_and_outputs<true>(p, q, s_row, lse, 0);
  if (p.write_grad) {
    const float sc = xe_weight(p, q, g.mk);
    T* d = dlogits + (size_t)q.m * p.ldv;
    for (int v = threadIdx.x * 4; v < p.ldv; v += NT * 4) xe_grad4(d, s_row + v, v, g.y, p.V1, lse, sc);
  }
}

// ------------------------------------------------------------------ bf16, the training path: the row in registers
// Loss + d logits, no log-prob output: the row lives in REGISTERS (CH float4 per thread of NTH), one HBM read, one exp per
// element (the e^{x - max} of the normaliser pass is reused for the gradient), no LDS staging.
//   256 threads x 10 chunks (rows up to 10 240 columns): 8 instead of the LDS kernel's 4 workgroups per CU keep more loads in
//     flight on the HBM-bound pass over the logits.
//   1024 threads x 13 chunks (up to 53 248 columns, ARGMAX) for rows too long for 256 threads' registers -- the pivot NMT's
//     generator, 50 004 words = 200 KB per row: the criterion reads the 397 MB of logits ONCE (xe_big_kernel: twice) and keeps
//     the arg-max for the accuracy counters on the way; the row's maximum IS the arg-max's value.  (512 threads x 26 float4
//     at two workgroups per CU: 128 registers per lane, 307 spilled -- 427 us.)
constexpr int XE_RCH = 10;
constexpr int XE_WTH = 1024, XE_WCH = 13;
template <typename T, int NTH, int CH, bool ARGMAX>
__device__ __forceinline__ void xe_reg_body(const UicXeParams p, const float* __restrict__ logits, T* __restrict__ dlogits) {
  __shared__ float s_f[NTH / 64];
  __shared__ float s_y;
  const XePos q = xe_pos(p);
  const float* row = logits + (size_t)q.m * p.ldv;
  const XeTarget g = xe_target(p, q);
  const long y = g.y;
  if (g.mk == 0.f && !p.grad_scale && !(ARGMAX && p.score_stats && g.y0 != 0)) {      // (a row that is counted is read)
    // a position behind its caption's end (a quarter of the benchmark's, a third of COCO's): loss 0 x (.), d logits = 0 x softmax - 0 --
    // exact zeros whatever the logits are, so the row is not read (uniform over the workgroup).  Every padding row ends here.
    if (threadIdx.x == 0 && !q.pad) p.row_loss[q.m] = 0.f;
    xe_zero_row<T, NTH>(dlogits + (size_t)q.m * p.ldv, p.ldv);
    return;
  }
  float4 x[CH];
  // Every chunk of the row requested before the first is used, from a clamped address: behind `if (v < p.ldv)` hipcc waited
  // for each load at its branch's join -- a thread's ten loads were ten HBM round trips in a row.
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int v = (threadIdx.x + i * NTH) * 4;
    x[i] = *(const float4*)(row + (v < p.ldv ? v : p.ldv - 4));
  }
  float mx = -INFINITY;
  int bi = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int v = (threadIdx.x + i * NTH) * 4;
    const float4 r = x[i];
    const bool in = v < p.ldv;
    // -inf in the slots out of the row or past V1 (-> e = 0 below); the target's logit from the value as loaded
    x[i].x = in && v < p.V1 ? r.x : -INFINITY; x[i].y = in && v + 1 < p.V1 ? r.y : -INFINITY;
    x[i].z = in && v + 2 < p.V1 ? r.z : -INFINITY; x[i].w = in && v + 3 < p.V1 ? r.w : -INFINITY;
    if (in && (long)v <= y && y < (long)v + 4) s_y = y == v ? r.x : y == v + 1 ? r.y : y == v + 2 ? r.z : r.w;
    if constexpr (ARGMAX) {
      // (ascending index inside the thread: a later equal value does not replace the arg-max)
      if (x[i].x > mx) { mx = x[i].x; bi = v; }
      if (x[i].y > mx) { mx = x[i].y; bi = v + 1; }
      if (x[i].z > mx) { mx = x[i].z; bi = v + 2; }
      if (x[i].w > mx) { mx = x[i].w; bi = v + 3; }
    } else {
      mx = fmaxf(mx, fmaxf(fmaxf(x[i].x, x[i].y), fmaxf(x[i].z, x[i].w)));
    }
  }
  if constexpr (ARGMAX) {
    __shared__ float s_bv[NTH / 64];
    __shared__ int s_bi[NTH / 64];
    uic_block_argmax<NTH>(mx, bi, s_bv, s_bi);
  } else {
    mx = uic_block_max<NTH>(mx, s_f);
  }
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    x[i].x = __expf(x[i].x - mx); x[i].y = __expf(x[i].y - mx); x[i].z = __expf(x[i].z - mx); x[i].w = __expf(x[i].w - mx);
    sum += (x[i].x + x[i].y) + (x[i].z + x[i].w);
  }
  sum = uic_block_sum<NTH>(sum, s_f);       // (its barriers also publish s_y)
  const float lse = mx + logf(sum);
  if (threadIdx.x == 0 && !q.pad) p.row_loss[q.m] = -(s_y - lse) * g.mk;
  if constexpr (ARGMAX) xe_count(p, g.y0, bi);
  const float sc = xe_weight(p, q, g.mk);
  const float k = sc / sum;                 // softmax * sc = e^{x - max} * k
  T* d = dlogits + (size_t)q.m * p.ldv;
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int v = (threadIdx.x + i * NTH) * 4;
    if (v >= p.ldv) continue;
    float gr[4] = {x[i].x * k, x[i].y * k, x[i].z * k, x[i].w * k};
    const long j = y - (long)v;             // (the one-hot without a dynamic index into gr[], which would put it in scratch)
    gr[0] -= j == 0 ? sc : 0.f; gr[1] -= j == 1 ? sc : 0.f; gr[2] -= j == 2 ? sc : 0.f; gr[3] -= j == 3 ? sc : 0.f;
    xe_store4(d + v, gr[0], gr[1], gr[2], gr[3]);
  }
}
template <typename T>
__global__ __launch_bounds__(NT) void xe_reg_kernel(const UicXeParams p, const float* __restrict__ logits, T* __restrict__ dlogits) {
  xe_reg_body<T, NT, XE_RCH, false>(p, logits, dlogits);
}
template <typename T>
__global__ __launch_bounds__(XE_WTH) void xe_reg_wide_kernel(const UicXeParams p, const float* __restrict__ logits, T* __restrict__ dlogits) {
  xe_reg_body<T, XE_WTH, XE_WCH, true>(p, logits, dlogits);
}

// ------------------------------------------------------------------ log-softmax backward
// API-compat backward: upstream grad g wrt log-probs [n][t][v]; d logits = g - softmax * sum_v g
template <typename T>
__global__ __launch_bounds__(NT) void logsoftmax_bwd_kernel(T* __restrict__ dlogits, int V1, int ldv, int N, const float* __restrict__ g,
                                                            size_t g_step, size_t g_row, const float* __restrict__ logprobs) {
  __shared__ float s_buf[NT / 64];
  const int m = blockIdx.x;
  const int t = m / N, n = m - t * N;
  const float* gr = g + (size_t)n * g_row + (size_t)t * g_step;
  const float* lp = logprobs + (size_t)n * g_row + (size_t)t * g_step;
  float sum = 0.f;
  for (int v = threadIdx.x; v < V1; v += NT) sum += gr[v];
  sum = uic_block_sum<NT>(sum, s_buf);
  T* d = dlogits + (size_t)m * ldv;
  for (int v = threadIdx.x; v < ldv; v += NT) {
    float x = 0.f;
    if (v < V1) x = gr[v] - expf(lp[v]) * sum;
    d[v] = uic_from_f<T>(x);
  }
}

// ------------------------------------------------------------------ the criteria on materialised log-probs
// LanguageModelCriterion on materialised log-probs (P/misc/criterion.py:143-150)
__global__ void lm_crit_rows_kernel(int N, int T, int V1, const float* logp, const int64_t* target, int ldt,
                                    const float* mask, int ldm, float* row_loss, float* row_mask) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * T) return;
  const int n = i / T, t = i - n * T;
  long y = target[(size_t)n * ldt + t];
  if (y < 0 || y >= V1) y = 0;
  const float m = mask[(size_t)n * ldm + t];
  row_loss[i] = -logp[((size_t)n * T + t) * V1 + y] * m;
  row_mask[i] = m;
}
__global__ void lm_crit_final_kernel(const float* row_loss, const float* row_mask, int n, float* out) {
  __shared__ float s_a[256], s_b[256];
  float a = 0.f, b = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) { a += row_loss[i]; b += row_mask[i]; }
  s_a[threadIdx.x] = a; s_b[threadIdx.x] = b;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { s_a[threadIdx.x] += s_a[threadIdx.x + o]; s_b[threadIdx.x] += s_b[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[0] = s_a[0] / s_b[0]; out[1] = s_b[0]; }
}
__global__ void lm_crit_bwd_kernel(int N, int T, int V1, const int64_t* target, int ldt, const float* mask, int ldm,
                                   const float* loss_den, float grad_out, float* dlogp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * T) return;
  const int n = i / T, t = i - n * T;
  long y = target[(size_t)n * ldt + t];
  if (y < 0 || y >= V1) y = 0;
  dlogp[((size_t)n * T + t) * V1 + y] = -mask[(size_t)n * ldm + t] / loss_den[1] * grad_out;
}
// RewardCriterion (P/misc/criterion.py:117-124), one block
__global__ void reward_crit_kernel(int N, int L, const float* logp, const int64_t* seq, const float* reward, float* loss_out, float* dlogp) {
  // One workgroup (the sums are small and their order is part of the result).  Eight elements per thread in flight: with one
  // element per trip the 40 trips of a 640 x 16 step were 40 memory latencies in a row (40 us between the reward and the backward
  // pass of the self-critical step).  The per-thread sums still run over i = tid, tid + 256, ... in that order.
  __shared__ float s_a[256], s_b[256];
  const int total = N * L;
  float a = 0.f, b = 0.f;
  for (int i0 = threadIdx.x; i0 < total; i0 += 256 * 8) {
    float lp[8], rw[8], m[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u * 256;
      const bool in = i < total;
      const int n = in ? i / L : 0, t = in ? i - n * L : 0;
      lp[u] = in ? logp[i] : 0.f;
      rw[u] = in ? reward[i] : 0.f;
      m[u] = !in ? 0.f : (t == 0 || seq[(size_t)n * L + t - 1] > 0) ? 1.f : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (i0 + u * 256 < total) { a += -lp[u] * rw[u] * m[u]; b += m[u]; }
  }
  s_a[threadIdx.x] = a; s_b[threadIdx.x] = b;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { s_a[threadIdx.x] += s_a[threadIdx.x + o]; s_b[threadIdx.x] += s_b[threadIdx.x + o]; }
    __syncthreads();
  }
  const float den = s_b[0];
  if (threadIdx.x == 0) loss_out[0] = s_a[0] / den;
  if (dlogp)
    for (int i0 = threadIdx.x; i0 < total; i0 += 256 * 8) {
      float rw[8], m[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = i0 + u * 256;
        const bool in = i < total;
        const int n = in ? i / L : 0, t = in ? i - n * L : 0;
        rw[u] = in ? reward[i] : 0.f;
        m[u] = !in ? 0.f : (t == 0 || seq[(size_t)n * L + t - 1] > 0) ? 1.f : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (i0 + u * 256 < total) dlogp[i0 + u * 256] = -rw[u] * m[u] / den;
    }
}

// Which kernel takes a launch of uic_xe_launch.  The four bf16 kernels load 16 bytes at a time; everything else -- f32, a row stride that is
// not a multiple of 4, logits that are not 16-byte aligned -- goes to the generic kernel.
int xe_choose(const UicXeParams& p) {
  if (!(p.dtype == UIC_BF16 && p.ldv % 4 == 0 && ((uintptr_t)p.logits & 15) == 0)) return UIC_XE_GENERIC;
  const bool d8 = ((uintptr_t)p.dlogits & 7) == 0;          // the 8-byte gradient stores (true for a null dlogits)
  if (p.ldv <= XE_RCH * NT * 4 && p.write_grad && p.target && !p.logprobs && !p.score_stats && d8) return UIC_XE_REG;
  if (p.ldv > XE_RCH * NT * 4 && p.ldv <= XE_WCH * XE_WTH * 4 && p.write_grad && p.target && !p.logprobs && d8) return UIC_XE_REG_WIDE;
  // (no test of d8 here, although the kernel stores 8 bytes at a time like the others: looks like an oversight, kept as it is)
  if ((size_t)p.ldv * 4 <= 64 * 1024) return UIC_XE_LDS;
  // (`!p.dlogits ||` adds nothing to d8; kept as it was written)
  if (!p.dlogits || d8) return UIC_XE_BIG;
  return UIC_XE_GENERIC;
}

}  // namespace

int uic_xe_launch(const UicXeParams& p, hipStream_t s, int32_t* kernel_id) {
  UIC_REQUIRE(p.logits && p.N > 0, "xe: null logits or N=0");
  UIC_REQUIRE(!p.write_grad || (p.target && ((p.mask && p.inv_den) || p.grad_scale)), "xe: gradient needs target and mask+inv_den or grad_scale");
  UIC_REQUIRE(!p.write_grad || p.dlogits, "xe: null dlogits");
  UIC_REQUIRE(!p.target || p.row_loss, "xe: null row_loss");
  UIC_REQUIRE(!p.row_map || (p.write_grad && p.mask && !p.grad_scale && !p.logprobs),
              "xe: a row list goes with the masked criterion only (target, mask, gradient; no per-position scale or log-probabilities)");
  if (p.M == 0) return UIC_OK;
  const int id = xe_choose(p);
  bf16_t* const d16 = (bf16_t*)p.dlogits;
  switch (id) {
    case UIC_XE_REG:
      hipLaunchKernelGGL(xe_reg_kernel<bf16_t>, dim3(p.M), dim3(NT), 0, s, p, p.logits, d16);
      break;
    case UIC_XE_REG_WIDE:
      hipLaunchKernelGGL(xe_reg_wide_kernel<bf16_t>, dim3(p.M), dim3(XE_WTH), 0, s, p, p.logits, d16);
      break;
    case UIC_XE_LDS:          // (dynamic LDS: the row)
      hipLaunchKernelGGL(xe_lds_kernel<bf16_t>, dim3(p.M), dim3(NT), (size_t)p.ldv * 4, s, p, p.logits, d16);
      break;
    case UIC_XE_BIG:
      hipLaunchKernelGGL(xe_big_kernel<bf16_t>, dim3(p.M), dim3(NT), 0, s, p, p.logits, d16);
      break;
    default:
      if (p.dtype == UIC_BF16) hipLaunchKernelGGL(xe_kernel<bf16_t>, dim3(p.M), dim3(NT), 0, s, p, p.logits, d16);
      else hipLaunchKernelGGL(xe_kernel<float>, dim3(p.M), dim3(NT), 0, s, p, p.logits, (float*)p.dlogits);
  }
  static const char* const names[] = {"xe_kernel", "xe_lds_kernel", "xe_reg_kernel", "xe_reg_wide_kernel", "xe_big_kernel"};
  UIC_LAUNCH_CHECK(names[id]);
  if (kernel_id) *kernel_id = id;
  return UIC_OK;
}

int uic_logsoftmax_bwd_launch(int dtype, void* dlogits, int M, int V1, int ldv, int N, const float* g,
                              size_t g_step_stride, size_t g_row_stride, const float* logprobs, hipStream_t s) {
  UIC_REQUIRE(dlogits && g && logprobs && N > 0, "logsoftmax_bwd: null pointer");
  if (M == 0) return UIC_OK;
  if (dtype == UIC_BF16) hipLaunchKernelGGL(logsoftmax_bwd_kernel<bf16_t>, dim3(M), dim3(NT), 0, s, (bf16_t*)dlogits, V1, ldv, N, g, g_step_stride, g_row_stride, logprobs);
  else hipLaunchKernelGGL(logsoftmax_bwd_kernel<float>, dim3(M), dim3(NT), 0, s, (float*)dlogits, V1, ldv, N, g, g_step_stride, g_row_stride, logprobs);
  UIC_LAUNCH_CHECK("logsoftmax_bwd");
  return UIC_OK;
}

// scratch: row_loss [N T] | row_mask [N T] | {loss, den}
int uic_lm_crit_launch(int N, int T, int V1, const float* logp, const int64_t* target, int ld_target, const float* mask, int ld_mask,
                       float* loss_out, float* scratch, float* dlogp, float grad_out, hipStream_t s) {
  const int n = N * T;
  if (n == 0) return UIC_OK;
  float* row_loss = scratch;
  float* row_mask = scratch + n;
  float* fin = scratch + 2 * (size_t)n;   // {loss, den}
  hipLaunchKernelGGL(lm_crit_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, s, N, T, V1, logp, target, ld_target, mask, ld_mask, row_loss, row_mask);
  UIC_LAUNCH_CHECK("lm_crit_rows");
  hipLaunchKernelGGL(lm_crit_final_kernel, dim3(1), dim3(256), 0, s, row_loss, row_mask, n, fin);
  UIC_LAUNCH_CHECK("lm_crit_final");
  UIC_TRY(uic_copy_launch(loss_out, fin, 4, s));
  if (dlogp) {
    UIC_TRY(uic_fill_launch(dlogp, 0, (size_t)n * V1 * 4, s));
    hipLaunchKernelGGL(lm_crit_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, s, N, T, V1, target, ld_target, mask, ld_mask, fin, grad_out, dlogp);
    UIC_LAUNCH_CHECK("lm_crit_bwd");
  }
  return UIC_OK;
}

int uic_reward_crit_launch(int N, int L, const float* logp, const int64_t* seq, const float* reward, float* loss_out, float* dlogp,
                           hipStream_t s) {
  hipLaunchKernelGGL(reward_crit_kernel, dim3(1), dim3(256), 0, s, N, L, logp, seq, reward, loss_out, dlogp);
  UIC_LAUNCH_CHECK("reward_crit_kernel");
  return UIC_OK;
}
