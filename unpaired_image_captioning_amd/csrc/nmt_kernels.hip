// Pivot NMT step (zh -> en teacher) on one MI355X: SURVEY.md section 8a rows 12-15.
//
// Replaces NMTModel.forward (P/models/NMT_Models.py:414-420) = Embeddings + packed bi-LSTM Encoder (:27-135),
// _fix_enc_hidden / init_decoder_state (:284-295), input-feed Decoder over StackedLSTM + dot GlobalAttention
// (:183-271, O/modules/StackedRNN.py:20-34, O/modules/GlobalAttention.py:112-167), the generator +
// NMTCriterion with the NMT_loss.score counters (P/misc/criterion.py:126-136,175-184), and their backward.
// This file: the kernels of the launch chain and one host launcher for each (nmt_internal.h); the sequencers are nmt_layout.hip,
// nmt_train.hip and nmt_translate.hip, the persistent forms of the recurrences nmt_persist.hip.
//
// Layout: time-major like the reference ([S,B,*], [T,B,*]).  pack_padded_sequence semantics without packing: the
// batch is length-sorted (descending), so the rows alive at source step s are the prefix [0, nb(s)) and every
// recurrent GEMM simply runs on that many rows; state buffers carry one zero slot before and after the S steps, so
// "previous state" of both directions is a plain view and padded positions stay exactly zero (unpack's padding).
// Input projections (W_ih x) are batched over all steps; only W_hh (and the input-feed part) stays in the loops.
// Like the reference, attention is NOT masked over padded source positions (GlobalAttention.mask is never set in
// training): their context vectors are zero, their scores are 0, and they take part in the softmax.
#include "nmt_internal.h"

namespace {

using nmt::NT;

// tgt [T,B] -> target_bt [B,T-1] (= tgt[1:]), mask_bt [B,T-1] (target != PAD), tgt_in [(T-1)*B] (= tgt[:-1], flat)
__global__ void nmt_prep_kernel(const int64_t* tgt, int T, int B, int64_t* target_bt, float* mask_bt, int64_t* tgt_in) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (T - 1) * B) return;
  const int t = i / B, b = i - t * B;
  const long y = tgt[(size_t)(t + 1) * B + b];
  target_bt[(size_t)b * (T - 1) + t] = y;
  mask_bt[(size_t)b * (T - 1) + t] = y != 0 ? 1.f : 0.f;
  tgt_in[i] = tgt[i];
}

template <typename T>
__global__ void dropout_apply_kernel(const void* src_, void* dst_, size_t n, float p, unsigned seed, unsigned site) {
  const T* src = (const T*)src_;
  T* dst = (T*)dst_;
  const float inv_keep = 1.f / (1.f - p);
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    dst[i] = uic_from_f<T>(uic_to_f(src[i]) * uic_drop_scale(seed, site, (unsigned)i, p, inv_keep));
}
// g[i] *= mask (f32 gradient through a dropout site)
__global__ void dropout_grad_kernel(float* g, size_t n, float p, unsigned seed, unsigned site) {
  const float inv_keep = 1.f / (1.f - p);
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    g[i] *= uic_drop_scale(seed, site, (unsigned)i, p, inv_keep);
}

// _fix_enc_hidden (NMT_Models.py:284-287): decoder initial state of layer l, row b = [fwd final | bwd final]; the
// forward direction ends at the row's last valid step (slot len), the backward one at step 0 (slot 1).
template <typename T>
__global__ void enc_final_kernel(const void* xl_, const float* c_f, const float* c_b, const int* lens, int B, int H, int Hd,
                                 void* h0_, float* c0) {
  const T* xl = (const T*)xl_;
  T* h0 = (T*)h0_;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * H) return;
  const int b = i / H, j = i - b * H;
  const int d = j >= Hd;
  const int slot = d ? 1 : lens[b];
  h0[i] = xl[((size_t)slot * B + b) * H + j];
  c0[i] = (d ? c_b : c_f)[((size_t)slot * B + b) * Hd + (j - d * Hd)];
}

// sum_j row[j] * vec[j] over one wavefront, 16-byte loads (H is a multiple of the vector width)
template <typename T>
__device__ __forceinline__ float row_dot(const T* __restrict__ row, const float* __restrict__ vec, int H, int lane) {
  constexpr int VEC = uic_vec<T>::N;
  float p = 0.f;
  for (int c = lane; c < H / VEC; c += 64) {
    float f[VEC];
    uic_unpack<T>(*(const uint4*)(row + c * VEC), f);
#pragma unroll
    for (int k = 0; k < VEC; ++k) p += f[k] * vec[c * VEC + k];
  }
  return uic_wave_sum(p);
}
// s_red[wave][:] = sum over this wave's source positions s of coef[s] * ctx[s, b, :]
template <typename T>
__device__ __forceinline__ void weighted_rows(const T* __restrict__ ctx, const float* __restrict__ coef, int S, int B, int H, int b,
                                              int lane, int wave, float* __restrict__ s_red) {
  constexpr int VEC = uic_vec<T>::N;
  for (int c = lane; c < H / VEC; c += 64) {
    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    for (int s = wave; s < S; s += 4) {
      float f[VEC];
      uic_unpack<T>(*(const uint4*)(ctx + ((size_t)s * B + b) * H + c * VEC), f);
      const float a = coef[s];
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc[k] += a * f[k];
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) s_red[wave * H + c * VEC + k] = acc[k];
  }
}

// ---- dot GlobalAttention (O/modules/GlobalAttention.py:112-116,152,160-162), one workgroup per batch row
template <typename T>
// Training path: `ctxw` = context x W_in (f32, made once per batch) and `qvec` = the decoder's rnn_output, so that
// score[s] = ctxw[s, b, :] . q -- the same number as context[s, b, :] . linear_in(q) without a linear_in GEMM per step.
__global__ __launch_bounds__(NT) void gattn_fwd_kernel(const void* ctx_, const float* target, int S, int B, int H, float* attn,
                                                       void* cvec_, const int64_t* mask_src = nullptr, const float* ctxw = nullptr,
                                                       const void* qvec_ = nullptr) {
  const T* ctx = (const T*)ctx_;
  T* cvec = (T*)cvec_;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* s_t = sm;            // [H]
  float* s_a = s_t + H;       // [S]
  float* s_red = s_a + S;     // [4][H]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int j = tid; j < H; j += NT) s_t[j] = ctxw ? uic_to_f(((const T*)qvec_)[(size_t)b * H + j]) : target[(size_t)b * H + j];
  __syncthreads();
  for (int s = wave; s < S; s += 4) {
    float p = ctxw ? row_dot<float>(ctxw + ((size_t)s * B + b) * H, s_t, H, lane)
                   : row_dot<T>(ctx + ((size_t)s * B + b) * H, s_t, H, lane);
    // translator only: source padding is masked (GlobalAttention.applyMask, NMT_Models.py:345,352)
    if (mask_src && mask_src[(size_t)s * B + b] == 0) p = -INFINITY;
    if (lane == 0) s_a[s] = p;
  }
  __syncthreads();
  float mx = -INFINITY;
  for (int s = 0; s < S; ++s) mx = fmaxf(mx, s_a[s]);
  float sum = 0.f;
  for (int s = 0; s < S; ++s) sum += expf(s_a[s] - mx);
  const float inv = 1.f / sum;
  __syncthreads();
  for (int s = tid; s < S; s += NT) {
    const float a = expf(s_a[s] - mx) * inv;
    s_a[s] = a;
    attn[(size_t)b * S + s] = a;
  }
  __syncthreads();
  weighted_rows<T>(ctx, s_a, S, B, H, b, lane, wave, s_red);
  __syncthreads();
  for (int j = tid; j < H; j += NT)
    cvec[(size_t)b * H + j] = uic_from_f<T>(s_red[j] + s_red[H + j] + s_red[2 * H + j] + s_red[3 * H + j]);
}

// backward of one decode step: d_a = d_c . ctx[s]; d_score = a (d_a - sum a d_a); with the hoisted linear_in the
// query's gradient is direct: d q += sum_s d_score[s] ctxw[s, b, :] (added to `dq`, which already holds the linear_out share)
template <typename T>
__global__ __launch_bounds__(NT) void gattn_bwd_step_kernel(const void* ctx_, const float* attn, const float* dcq, int lddcq,
                                                            int S, int B, int H, float* dscore, const float* ctxw, float* dq, int lddq) {
  const T* ctx = (const T*)ctx_;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* s_dc = sm;           // [H]
  float* s_a = s_dc + H;      // [S]
  float* s_da = s_a + S;      // [S]
  float* s_red = s_da + S;    // [4][H]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int j = tid; j < H; j += NT) s_dc[j] = dcq[(size_t)b * lddcq + j];
  for (int s = tid; s < S; s += NT) s_a[s] = attn[(size_t)b * S + s];
  __syncthreads();
  for (int s = wave; s < S; s += 4) {
    const float p = row_dot<T>(ctx + ((size_t)s * B + b) * H, s_dc, H, lane);
    if (lane == 0) s_da[s] = p;
  }
  __syncthreads();
  float wbar = 0.f;
  for (int s = 0; s < S; ++s) wbar += s_a[s] * s_da[s];
  __syncthreads();
  for (int s = tid; s < S; s += NT) {
    const float ds = s_a[s] * (s_da[s] - wbar);
    s_da[s] = ds;
    dscore[(size_t)b * S + s] = ds;
  }
  __syncthreads();
  weighted_rows<float>(ctxw, s_da, S, B, H, b, lane, wave, s_red);
  __syncthreads();
  for (int j = tid; j < H; j += NT)
    dq[(size_t)b * lddq + j] += s_red[j] + s_red[H + j] + s_red[2 * H + j] + s_red[3 * H + j];
}

// The same two kernels for bf16 rows of H = 512 and S <= 4 * MAXR source positions, with EVERY global load of the launch issued
// at its top: a wave keeps its <= MAXR context rows (16 B per lane) and, where scores or gradients go through ctxw, those f32
// rows (2 x 16 B per lane) in registers.  The generic kernels above pay a memory latency per phase (query, score rows,
// weighted rows); at batch 64 the launch IS those latencies.  Same arithmetic in the same order: bit-identical results.
template <int MAXR>
__global__ __launch_bounds__(NT) void gattn_fwd_fast_kernel(const bf16_t* __restrict__ ctx, const float* __restrict__ target, int S, int B,
                                                            float* __restrict__ attn, bf16_t* __restrict__ cvec,
                                                            const int64_t* __restrict__ mask_src, const float* __restrict__ ctxw,
                                                            const bf16_t* __restrict__ qvec) {
  constexpr int H = 512;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* s_t = sm;            // [H]
  float* s_a = s_t + H;       // [S]
  float* s_red = s_a + S;     // [4][H]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint4 cr[MAXR];
  float4 wr[MAXR][2];
  long mk[MAXR];
#pragma unroll
  for (int u = 0; u < MAXR; ++u) {
    const int sp = wave + 4 * u;
    const size_t r = ((size_t)(sp < S ? sp : S - 1) * B + b) * H;
    cr[u] = *(const uint4*)(ctx + r + lane * 8);
    if (ctxw) { wr[u][0] = *(const float4*)(ctxw + r + lane * 4); wr[u][1] = *(const float4*)(ctxw + r + (lane + 64) * 4); }
    mk[u] = mask_src ? mask_src[(size_t)(sp < S ? sp : S - 1) * B + b] : 1;
  }
  for (int j = tid; j < H; j += NT) s_t[j] = ctxw ? uic_to_f(qvec[(size_t)b * H + j]) : target[(size_t)b * H + j];
  __syncthreads();
#pragma unroll
  for (int u = 0; u < MAXR; ++u) {
    const int sp = wave + 4 * u;
    if (sp >= S) break;
    float p = 0.f;
    if (ctxw) {                                           // row_dot<float>: chunks lane, lane + 64 of four floats
      const float* v0 = s_t + lane * 4; const float* v1 = s_t + (lane + 64) * 4;
      p += wr[u][0].x * v0[0]; p += wr[u][0].y * v0[1]; p += wr[u][0].z * v0[2]; p += wr[u][0].w * v0[3];
      p += wr[u][1].x * v1[0]; p += wr[u][1].y * v1[1]; p += wr[u][1].z * v1[2]; p += wr[u][1].w * v1[3];
    } else {                                              // row_dot<bf16>: chunk lane of eight
      float f[8];
      uic_unpack<bf16_t>(cr[u], f);
#pragma unroll
      for (int k = 0; k < 8; ++k) p += f[k] * s_t[lane * 8 + k];
    }
    p = uic_wave_sum(p);
    if (mk[u] == 0) p = -INFINITY;
    if (lane == 0) s_a[sp] = p;
  }
  __syncthreads();
  float mx = -INFINITY;
  for (int sp = 0; sp < S; ++sp) mx = fmaxf(mx, s_a[sp]);
  float sum = 0.f;
  for (int sp = 0; sp < S; ++sp) sum += expf(s_a[sp] - mx);
  const float inv = 1.f / sum;
  __syncthreads();
  for (int sp = tid; sp < S; sp += NT) {
    const float a = expf(s_a[sp] - mx) * inv;
    s_a[sp] = a;
    attn[(size_t)b * S + sp] = a;
  }
  __syncthreads();
  float acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
#pragma unroll
  for (int u = 0; u < MAXR; ++u) {
    const int sp = wave + 4 * u;
    if (sp >= S) break;
    float f[8];
    uic_unpack<bf16_t>(cr[u], f);
    const float a = s_a[sp];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] += a * f[k];
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) s_red[wave * H + lane * 8 + k] = acc[k];
  __syncthreads();
  for (int j = tid; j < H; j += NT) cvec[(size_t)b * H + j] = (bf16_t)(s_red[j] + s_red[H + j] + s_red[2 * H + j] + s_red[3 * H + j]);
}

template <int MAXR>
__global__ __launch_bounds__(NT) void gattn_bwd_step_fast_kernel(const bf16_t* __restrict__ ctx, const float* __restrict__ attn,
                                                                 const float* __restrict__ dcq, int lddcq, int S, int B,
                                                                 float* __restrict__ dscore, const float* __restrict__ ctxw,
                                                                 float* __restrict__ dq, int lddq) {
  constexpr int H = 512;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* s_dc = sm;           // [H]
  float* s_a = s_dc + H;      // [S]
  float* s_da = s_a + S;      // [S]
  float* s_red = s_da + S;    // [4][H]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint4 cr[MAXR];
  float4 wr[MAXR][2];
#pragma unroll
  for (int u = 0; u < MAXR; ++u) {
    const int sp = wave + 4 * u;
    const size_t r = ((size_t)(sp < S ? sp : S - 1) * B + b) * H;
    cr[u] = *(const uint4*)(ctx + r + lane * 8);
    wr[u][0] = *(const float4*)(ctxw + r + lane * 4);
    wr[u][1] = *(const float4*)(ctxw + r + (lane + 64) * 4);
  }
  const float dq0 = dq[(size_t)b * lddq + tid], dq1 = dq[(size_t)b * lddq + tid + NT];      // (H = 2 NT)
  for (int j = tid; j < H; j += NT) s_dc[j] = dcq[(size_t)b * lddcq + j];
  for (int sp = tid; sp < S; sp += NT) s_a[sp] = attn[(size_t)b * S + sp];
  __syncthreads();
#pragma unroll
  for (int u = 0; u < MAXR; ++u) {
    const int sp = wave + 4 * u;
    if (sp >= S) break;
    float f[8];
    uic_unpack<bf16_t>(cr[u], f);
    float p = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) p += f[k] * s_dc[lane * 8 + k];
    p = uic_wave_sum(p);
    if (lane == 0) s_da[sp] = p;
  }
  __syncthreads();
  float wbar = 0.f;
  for (int sp = 0; sp < S; ++sp) wbar += s_a[sp] * s_da[sp];
  __syncthreads();
  for (int sp = tid; sp < S; sp += NT) {
    const float ds = s_a[sp] * (s_da[sp] - wbar);
    s_da[sp] = ds;
    dscore[(size_t)b * S + sp] = ds;
  }
  __syncthreads();
  // weighted_rows<float>(ctxw, s_da): chunks lane, lane + 64 of four floats
  float a0[4] = {0.f, 0.f, 0.f, 0.f}, a1[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < MAXR; ++u) {
    const int sp = wave + 4 * u;
    if (sp >= S) break;
    const float a = s_da[sp];
    a0[0] += a * wr[u][0].x; a0[1] += a * wr[u][0].y; a0[2] += a * wr[u][0].z; a0[3] += a * wr[u][0].w;
    a1[0] += a * wr[u][1].x; a1[1] += a * wr[u][1].y; a1[2] += a * wr[u][1].z; a1[3] += a * wr[u][1].w;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) { s_red[wave * H + lane * 4 + k] = a0[k]; s_red[wave * H + (lane + 64) * 4 + k] = a1[k]; }
  __syncthreads();
  dq[(size_t)b * lddq + tid] = dq0 + (s_red[tid] + s_red[H + tid] + s_red[2 * H + tid] + s_red[3 * H + tid]);
  dq[(size_t)b * lddq + tid + NT] = dq1 + (s_red[tid + NT] + s_red[H + tid + NT] + s_red[2 * H + tid + NT] + s_red[3 * H + tid + NT]);
}

// deferred over decode steps: d ctx[s,b,:] = sum_t a_t[b,s] d_c_t[b,:]  and  d ctxw[s,b,:] = sum_t d_score_t[b,s] q_t[b,:]
template <typename T>
__global__ void gattn_bwd_accum_kernel(const float* attn_all, const float* dscore_all, const float* dcq_all, int lddcq,
                                       const void* q_all_, int Td, int S, int B, int H, float* dctx, void* dctxw_) {
  const T* q_all = (const T*)q_all_;
  T* dctxw = (T*)dctxw_;
  const size_t total = (size_t)S * B * H;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int j = (int)(i % H);
    const size_t sb = i / H;
    const int b = (int)(sb % B), s = (int)(sb / B);
    float acc = 0.f, accw = 0.f;
    for (int t = 0; t < Td; ++t) {
      const size_t tb = (size_t)t * B + b;
      acc += attn_all[tb * S + s] * dcq_all[tb * lddcq + j];
      accw += dscore_all[tb * S + s] * uic_to_f(q_all[tb * H + j]);
    }
    dctx[i] = acc;
    dctxw[i] = uic_from_f<T>(accw);
  }
}

// d_pre = (d_out + d_feed) * dropout_mask * (1 - out_pre^2): backward of out = dropout(tanh(.))
template <typename T>
__global__ void tanh_drop_bwd_kernel(const float* d_out, const float* d_feed, int ld_feed, int H, const void* out_pre_, int n, float p,
                                     unsigned seed, unsigned site, void* d_pre_) {
  const T* out_pre = (const T*)out_pre_;
  T* d_pre = (T*)d_pre_;
  const float inv_keep = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float g = d_out[i] + (d_feed ? d_feed[(size_t)(i / H) * ld_feed + (i % H)] : 0.f);
  if (p > 0.f) g *= uic_drop_scale(seed, site, (unsigned)i, p, inv_keep);
  const float o = uic_to_f(out_pre[i]);
  d_pre[i] = uic_from_f<T>(g * (1.f - o * o));
}

// (NMT_loss.score's counters, criterion.py:175-179, are computed by the criterion kernel: UicXeParams.score_stats)
__global__ void fill_f32_kernel(float* p, float v, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

}  // namespace

namespace nmt {

int nmt_prep_launch(const int64_t* tgt, int T, int B, int64_t* target_bt, float* mask_bt, int64_t* tgt_in, hipStream_t s) {
  hipLaunchKernelGGL(nmt_prep_kernel, dim3(uic_grid_for((size_t)(T - 1) * B, NT)), dim3(NT), 0, s, tgt, T, B, target_bt, mask_bt, tgt_in);
  UIC_LAUNCH_CHECK("nmt_prep_kernel");
  return UIC_OK;
}

int nmt_dropout_apply_launch(int dt, const void* src, void* dst, size_t n, float p, unsigned seed, unsigned site, hipStream_t s) {
  const dim3 grid(uic_grid_for(n, NT));
  UIC_DISPATCH_T(dt, hipLaunchKernelGGL(dropout_apply_kernel<bf16_t>, grid, dim3(NT), 0, s, src, dst, n, p, seed, site),
                 hipLaunchKernelGGL(dropout_apply_kernel<float>, grid, dim3(NT), 0, s, src, dst, n, p, seed, site));
  UIC_LAUNCH_CHECK("dropout_apply_kernel");
  return UIC_OK;
}

int nmt_dropout_grad_launch(float* g, size_t n, float p, unsigned seed, unsigned site, hipStream_t s) {
  hipLaunchKernelGGL(dropout_grad_kernel, dim3(uic_grid_for(n, NT)), dim3(NT), 0, s, g, n, p, seed, site);
  UIC_LAUNCH_CHECK("dropout_grad_kernel");
  return UIC_OK;
}

int nmt_enc_final_launch(int dt, const void* xl, const float* c_f, const float* c_b, const int* lens, int B, int H, int Hd, void* h0,
                         float* c0, hipStream_t s) {
  const dim3 grid(uic_grid_for((size_t)B * H, NT));
  UIC_DISPATCH_T(dt, hipLaunchKernelGGL(enc_final_kernel<bf16_t>, grid, dim3(NT), 0, s, xl, c_f, c_b, lens, B, H, Hd, h0, c0),
                 hipLaunchKernelGGL(enc_final_kernel<float>, grid, dim3(NT), 0, s, xl, c_f, c_b, lens, B, H, Hd, h0, c0));
  UIC_LAUNCH_CHECK("enc_final_kernel");
  return UIC_OK;
}

// the register-resident fast kernels take bf16, H = 512, S <= 64 (NT = 256 threads = 4 waves of 8 or 16 rows), else generic
int nmt_gattn_maxr(int dt, int H, int S) { return dt == UIC_BF16 && H == 512 && S <= 64 ? (S <= 32 ? 8 : 16) : 0; }

int nmt_gattn_fwd_launch(int dt, const void* ctx, const float* target, int S, int B, int H, float* attn, void* cvec, const int64_t* mask,
                         const float* ctxw, const void* q, hipStream_t s) {
  const size_t lds = sizeof(float) * ((size_t)H + S + 4 * (size_t)H);   // s_t [H], s_a [S], s_red [4][H]
  const int maxr = nmt_gattn_maxr(dt, H, S);
  if (maxr == 8)
    hipLaunchKernelGGL(gattn_fwd_fast_kernel<8>, dim3(B), dim3(NT), lds, s, (const bf16_t*)ctx, target, S, B, attn, (bf16_t*)cvec, mask, ctxw,
                       (const bf16_t*)q);
  else if (maxr == 16)
    hipLaunchKernelGGL(gattn_fwd_fast_kernel<16>, dim3(B), dim3(NT), lds, s, (const bf16_t*)ctx, target, S, B, attn, (bf16_t*)cvec, mask, ctxw,
                       (const bf16_t*)q);
  else
    UIC_DISPATCH_T(dt, hipLaunchKernelGGL(gattn_fwd_kernel<bf16_t>, dim3(B), dim3(NT), lds, s, ctx, target, S, B, H, attn, cvec, mask, ctxw, q),
                   hipLaunchKernelGGL(gattn_fwd_kernel<float>, dim3(B), dim3(NT), lds, s, ctx, target, S, B, H, attn, cvec, mask, ctxw, q));
  UIC_LAUNCH_CHECK("gattn_fwd_kernel");
  return UIC_OK;
}

int nmt_gattn_bwd_step_launch(int dt, const void* ctx, const float* attn, const float* dcq, int lddcq, int S, int B, int H, float* dscore,
                              const float* ctxw, float* dq, int lddq, hipStream_t s) {
  const size_t lds = sizeof(float) * ((size_t)H + 2 * (size_t)S + 4 * (size_t)H);   // s_dc [H], s_a [S], s_da [S], s_red [4][H]
  const int maxr = nmt_gattn_maxr(dt, H, S);
  if (maxr == 8)
    hipLaunchKernelGGL(gattn_bwd_step_fast_kernel<8>, dim3(B), dim3(NT), lds, s, (const bf16_t*)ctx, attn, dcq, lddcq, S, B, dscore, ctxw, dq, lddq);
  else if (maxr == 16)
    hipLaunchKernelGGL(gattn_bwd_step_fast_kernel<16>, dim3(B), dim3(NT), lds, s, (const bf16_t*)ctx, attn, dcq, lddcq, S, B, dscore, ctxw, dq, lddq);
  else
    UIC_DISPATCH_T(dt, hipLaunchKernelGGL(gattn_bwd_step_kernel<bf16_t>, dim3(B), dim3(NT), lds, s, ctx, attn, dcq, lddcq, S, B, H, dscore, ctxw, dq, lddq),
                   hipLaunchKernelGGL(gattn_bwd_step_kernel<float>, dim3(B), dim3(NT), lds, s, ctx, attn, dcq, lddcq, S, B, H, dscore, ctxw, dq, lddq));
  UIC_LAUNCH_CHECK("gattn_bwd_step_kernel");
  return UIC_OK;
}

int nmt_gattn_bwd_accum_launch(int dt, const float* attn_all, const float* dscore_all, const float* dcq_all, int lddcq, const void* q_all,
                               int Td, int S, int B, int H, float* dctx, void* dctxw, hipStream_t s) {
  const dim3 grid(uic_grid_for((size_t)S * B * H, NT));
  UIC_DISPATCH_T(dt, hipLaunchKernelGGL(gattn_bwd_accum_kernel<bf16_t>, grid, dim3(NT), 0, s, attn_all, dscore_all, dcq_all, lddcq, q_all, Td, S, B, H, dctx, dctxw),
                 hipLaunchKernelGGL(gattn_bwd_accum_kernel<float>, grid, dim3(NT), 0, s, attn_all, dscore_all, dcq_all, lddcq, q_all, Td, S, B, H, dctx, dctxw));
  UIC_LAUNCH_CHECK("gattn_bwd_accum_kernel");
  return UIC_OK;
}

int nmt_tanh_drop_bwd_launch(int dt, const float* d_out, const float* d_feed, int ld_feed, int H, const void* out_pre, int n, float p,
                             unsigned seed, unsigned site, void* d_pre, hipStream_t s) {
  const dim3 grid(uic_grid_for((size_t)n, NT));
  UIC_DISPATCH_T(dt, hipLaunchKernelGGL(tanh_drop_bwd_kernel<bf16_t>, grid, dim3(NT), 0, s, d_out, d_feed, ld_feed, H, out_pre, n, p, seed, site, d_pre),
                 hipLaunchKernelGGL(tanh_drop_bwd_kernel<float>, grid, dim3(NT), 0, s, d_out, d_feed, ld_feed, H, out_pre, n, p, seed, site, d_pre));
  UIC_LAUNCH_CHECK("tanh_drop_bwd_kernel");
  return UIC_OK;
}

int nmt_fill_f32_launch(float* p, float v, int n, hipStream_t s) {
  hipLaunchKernelGGL(fill_f32_kernel, dim3((n + 63) / 64), dim3(64), 0, s, p, v, n);
  UIC_LAUNCH_CHECK("fill_f32_kernel");
  return UIC_OK;
}

}  // namespace nmt
