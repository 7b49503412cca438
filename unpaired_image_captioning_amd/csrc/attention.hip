// Additive attention over the R region features of one caption row, gfx950.
//
// Replaces Attention.forward (P/models/AttModel.py:538-558): the reference runs
// linear / expand+add / tanh / linear / softmax / mul+div / bmm as seven kernels that
// round-trip [N,R,A] intermediates through HBM.  Here one workgroup per caption row
// streams p_att[n] and att[n] exactly once with 16-byte coalesced loads, keeps
// att_h / w_alpha / scores in LDS, reduces each region's score across a 64-lane
// wavefront, normalises the R scores in LDS and accumulates the weighted sum per wave.
//
// Backward is split so the BPTT loop stays read-only on the big tensors:
//   * bwd_step  (inside the loop): d alpha, softmax backward, d att_h   -- reads att, p_att once
//   * bwd_accum (after the loop):  d att'[n,r,:]  = sum_t alpha_t[r] dctx_t
//                                  d p_att[n,r,a] = sum_t de_t[r] w_a (1 - tanh^2(p_att + att_h_t))
//     one pass, no read-modify-write of [N,R,*] accumulators per decode step.
#include "uic_common.h"
#include "../../include/uic_hip.h"

namespace {

constexpr int NTHREADS = 256;
constexpr int NWAVES = 4;
constexpr int UB = 9;   // regions a wave keeps in flight per batch (R = 36 -> one batch per wave)
constexpr int UIC_ATT_FAST_R = UB * NWAVES;   // regions the fast kernels cover

template <typename T>
__global__ __launch_bounds__(NTHREADS) void attn_fwd_kernel(const UicAttnParams p) {
  constexpr int VEC = uic_vec<T>::N;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int A = p.A, H = p.H, R = p.R;
  float* s_atth = sm;
  float* s_w = s_atth + A;
  float* s_e = s_w + A;
  float* s_red = s_e + ((R + 3) & ~3);
  const int n = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  for (int a = tid; a < A; a += NTHREADS) {
    s_atth[a] = p.att_h[(size_t)n * A + a];
    s_w[a] = p.w_alpha[a];
  }
  __syncthreads();

  // ---- scores e_r = w . tanh(p_att[r] + att_h) + b   (AttModel.py:543-549)
  const T* pa = (const T*)p.p_att + (size_t)n * R * A;
  const int ncA = A / VEC;
  const float b_alpha = p.b_alpha ? p.b_alpha[0] : 0.f;
  for (int r0 = wave; r0 < R; r0 += UB * NWAVES) {
    float part[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) part[u] = 0.f;
    for (int c = lane; c < ncA; c += 64) {
      uint4 v[UB];
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int r = r0 + u * NWAVES;
        v[u] = r < R ? *(const uint4*)(pa + (size_t)r * A + c * VEC) : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        float f[VEC];
        uic_unpack<T>(v[u], f);
#pragma unroll
        for (int j = 0; j < VEC; ++j) part[u] += s_w[c * VEC + j] * uic_tanh<T>(f[j] + s_atth[c * VEC + j]);
      }
    }
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int r = r0 + u * NWAVES;
      const float s = uic_wave_sum(part[u]);
      if (lane == 0 && r < R) s_e[r] = s + b_alpha;
    }
  }
  __syncthreads();

  // ---- softmax over R, then mask-renormalise (AttModel.py:551-554)
  float mx = -INFINITY;
  for (int r = 0; r < R; ++r) mx = fmaxf(mx, s_e[r]);
  float sum = 0.f;
  for (int r = 0; r < R; ++r) sum += expf(s_e[r] - mx);
  const float inv = 1.f / sum;
  float usum = 1.f;
  const float* mk = p.mask ? p.mask + (size_t)n * p.ldmask : nullptr;
  if (mk) {
    usum = 0.f;
    for (int r = 0; r < R; ++r) usum += expf(s_e[r] - mx) * inv * mk[r];
  }
  __syncthreads();
  for (int r = tid; r < R; r += NTHREADS) {
    float w = expf(s_e[r] - mx) * inv;
    if (mk) w = w * mk[r] / usum;
    s_e[r] = w;
    p.alpha[(size_t)n * R + r] = w;
  }
  __syncthreads();

  // ---- ctx = sum_r alpha_r att[r]   (AttModel.py:555-556)
  const T* pt = (const T*)p.att + (size_t)n * R * H;
  const int ncH = H / VEC;
  for (int c = lane; c < ncH; c += 64) {
    float acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
    for (int r0 = wave; r0 < R; r0 += UB * NWAVES) {
      uint4 v[UB];
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int r = r0 + u * NWAVES;
        v[u] = r < R ? *(const uint4*)(pt + (size_t)r * H + c * VEC) : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int r = r0 + u * NWAVES;
        float f[VEC];
        uic_unpack<T>(v[u], f);
        const float al = r < R ? s_e[r] : 0.f;
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[j] += al * f[j];
      }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) s_red[wave * H + c * VEC + j] = acc[j];
  }
  __syncthreads();
  T* ctx = (T*)p.ctx + (size_t)n * p.ldctx;
  for (int h = tid; h < H; h += NTHREADS)
    ctx[h] = uic_from_f<T>(s_red[h] + s_red[H + h] + s_red[2 * H + h] + s_red[3 * H + h]);
}

template <typename T>
__global__ __launch_bounds__(NTHREADS) void attn_bwd_step_kernel(const UicAttnParams p) {
  constexpr int VEC = uic_vec<T>::N;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int A = p.A, H = p.H, R = p.R;
  const int Rp = (R + 3) & ~3;
  float* s_atth = sm;
  float* s_w = s_atth + A;
  float* s_dctx = s_w + A;
  float* s_al = s_dctx + H;
  float* s_da = s_al + Rp;
  float* s_red = s_da + Rp;
  const int n = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (p.row_len && p.step >= p.row_len[n]) {
    // a caption that ended before this decode step: exact zeros, no operand read (the same exit as attn_bwd_step_fast_kernel, so
    // that what such a row gets does not depend on which kernel the launcher picks)
    if (p.dctx_sum) for (int h = tid; h < H; h += NTHREADS) p.dctx_sum[(size_t)n * p.ld_dctx_sum + h] = 0.f;
    for (int r = tid; r < R; r += NTHREADS) p.de[(size_t)n * R + r] = 0.f;
    T* out0 = (T*)p.d_att_h + (size_t)n * A;
    for (int a = tid; a < A; a += NTHREADS) out0[a] = uic_from_f<T>(0.f);
    return;
  }

  for (int a = tid; a < A; a += NTHREADS) {
    s_atth[a] = p.att_h[(size_t)n * A + a];
    s_w[a] = p.w_alpha[a];
  }
  for (int h = tid; h < H; h += NTHREADS) {
    float v = p.dctx[(size_t)n * p.lddctx + h];
    for (int z = 1; z < p.dctx_nslab; ++z) v += p.dctx[(size_t)z * p.dctx_slab_stride + (size_t)n * p.lddctx + h];
    s_dctx[h] = v;
    if (p.dctx_sum) p.dctx_sum[(size_t)n * p.ld_dctx_sum + h] = v;
  }
  for (int r = tid; r < R; r += NTHREADS) s_al[r] = p.alpha[(size_t)n * R + r];
  __syncthreads();

  // d alpha_r = dctx . att[r]
  const T* pt = (const T*)p.att + (size_t)n * R * H;
  const int ncH = H / VEC;
  for (int r0 = wave; r0 < R; r0 += UB * NWAVES) {
    float part[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) part[u] = 0.f;
    for (int c = lane; c < ncH; c += 64) {
      uint4 v[UB];
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int r = r0 + u * NWAVES;
        v[u] = r < R ? *(const uint4*)(pt + (size_t)r * H + c * VEC) : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        float f[VEC];
        uic_unpack<T>(v[u], f);
#pragma unroll
        for (int j = 0; j < VEC; ++j) part[u] += s_dctx[c * VEC + j] * f[j];
      }
    }
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int r = r0 + u * NWAVES;
      const float s = uic_wave_sum(part[u]);
      if (lane == 0 && r < R) s_da[r] = s;
    }
  }
  __syncthreads();
  // backward of softmax (+ mask renormalisation): de_r = alpha_r (dalpha_r - sum_j alpha_j dalpha_j)
  float wbar = 0.f;
  for (int r = 0; r < R; ++r) wbar += s_al[r] * s_da[r];
  __syncthreads();
  for (int r = tid; r < R; r += NTHREADS) {
    const float de = s_al[r] * (s_da[r] - wbar);
    s_da[r] = de;
    p.de[(size_t)n * R + r] = de;
  }
  __syncthreads();
  // d att_h[a] = w_a sum_r de_r (1 - tanh^2(p_att[r,a] + att_h[a]))
  const T* pa = (const T*)p.p_att + (size_t)n * R * A;
  const int ncA = A / VEC;
  for (int c = lane; c < ncA; c += 64) {
    float acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
    for (int r0 = wave; r0 < R; r0 += UB * NWAVES) {
      uint4 v[UB];
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int r = r0 + u * NWAVES;
        v[u] = r < R ? *(const uint4*)(pa + (size_t)r * A + c * VEC) : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int r = r0 + u * NWAVES;
        float f[VEC];
        uic_unpack<T>(v[u], f);
        const float de = r < R ? s_da[r] : 0.f;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const float th = uic_tanh<T>(f[j] + s_atth[c * VEC + j]);
          acc[j] += de * (1.f - th * th);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) s_red[wave * A + c * VEC + j] = acc[j] * s_w[c * VEC + j];
  }
  __syncthreads();
  T* out = (T*)p.d_att_h + (size_t)n * A;
  for (int a = tid; a < A; a += NTHREADS)
    out[a] = uic_from_f<T>(s_red[a] + s_red[A + a] + s_red[2 * A + a] + s_red[3 * A + a]);
}


// ---------------------------------------------------------------------------------------------------
// Fast path (R <= UB * NWAVES regions, A and H at most 64 16-byte chunks: the BASELINE shapes in bf16).
// Every lane issues ALL of its p_att and att loads (2 x UB x 16 B) before the first use, so a
// workgroup exposes one memory latency instead of one per phase, and the only LDS traffic is the
// R scores and the 4-wave reduction of the context vector.
template <typename T>
__device__ __forceinline__ void load_chunk_f32(const float* src, int c, bool ok, float* out) {
  constexpr int VEC = uic_vec<T>::N;
#pragma unroll
  for (int q = 0; q < VEC / 4; ++q) {
    float4 v = ok ? *(const float4*)(src + c * VEC + q * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    out[q * 4 + 0] = v.x; out[q * 4 + 1] = v.y; out[q * 4 + 2] = v.z; out[q * 4 + 3] = v.w;
  }
}

// NW waves per caption row, each keeping UBX = ceil(36 / NW) regions in flight (NW = 8: more waves to hide the HBM latency of
// the one-shot load burst and half the per-wave tanh / reduction work; measured against NW = 4 on MI355X)
// FULL (att_hid_size = rnn_size = 64 lanes x VEC): no lane predicates -- see attn_bwd_step_fast_kernel.  Requests in the order of
// use: att_h and w_alpha (the scores' other operands) FIRST, then the p_att rows, then the att' rows, which keep arriving while the
// scores are computed.  (Before round 6 the two small vectors were requested last, behind a lane predicate: the first score then
// waited for all 2 x UB row loads of the wave.)
template <typename T, int NW, bool FULL>
__global__ __launch_bounds__(NW * 64) void attn_fwd_fast_kernel(const UicAttnParams p) {
  constexpr int NWAVES = NW, NTHREADS = NW * 64, UB = (UIC_ATT_FAST_R + NW - 1) / NW;
  constexpr int VEC = uic_vec<T>::N;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int A = p.A, H = p.H, R = p.R;
  float* s_e = sm;                    // [R][4] row-of-16 partial scores
  float* s_red = s_e + 4 * R;
  const int n = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool la = FULL ? true : lane < A / VEC, lh = FULL ? true : lane < H / VEC;
  // indices are clamped instead of predicated (no exec-mask branches around the 18 loads); out-of-range
  // regions / lanes read valid memory and are neutralised by zero weights below
  const T* pa = (const T*)p.p_att + (size_t)n * R * A + (la ? lane : 0) * VEC;
  const T* pt = (const T*)p.att + (size_t)n * R * H + (lh ? lane : 0) * VEC;
  float ah[VEC], w[VEC];
  load_chunk_f32<T>(p.att_h + (size_t)n * A, lane, la, ah);
  load_chunk_f32<T>(p.w_alpha, lane, la, w);
  // (the region mask value of this lane's region: requested here, without a branch -- no mask: any readable word, ignored below)
  const float* mkp = p.mask ? p.mask + (size_t)n * p.ldmask : p.w_alpha;
  const float mkv = mkp[lane < R ? lane : 0];
  __builtin_amdgcn_sched_barrier(0);                  // (or hipcc issues the row loads first and these arrive behind them)
  uint4 vp[UB], va[UB];
#pragma unroll
  for (int u = 0; u < UB; ++u) vp[u] = *(const uint4*)(pa + (size_t)min(wave + u * NWAVES, R - 1) * A);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int u = 0; u < UB; ++u) va[u] = *(const uint4*)(pt + (size_t)min(wave + u * NWAVES, R - 1) * H);
  __builtin_amdgcn_sched_barrier(0);
  const float b_alpha = p.b_alpha ? p.b_alpha[0] : 0.f;
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    const int r = wave + u * NWAVES;
    float f[VEC];
    uic_unpack<T>(vp[u], f);
    float part = 0.f;
#pragma unroll
    for (int j = 0; j < VEC; ++j) part += w[j] * uic_tanh<T>(f[j] + ah[j]);
    part = uic_row16_sum(part);                       // 4 row sums per region, added when the scores are read
    if ((lane & 15) == 0 && r < R) s_e[r * 4 + (lane >> 4)] = part;
  }
  __syncthreads();
  // every wave normalises the R <= 64 scores with one lane per region (softmax, then mask-renormalise)
  float e = -INFINITY;
  if (lane < R) {
    const float4 q = *(const float4*)(s_e + lane * 4);
    e = (q.x + q.y) + (q.z + q.w) + b_alpha;
  }
  const float mx = uic_wave_max(e);
  // (bf16 path: one v_exp_f32 / v_rcp_f32 instead of libm's exp and an IEEE division -- this kernel is made of instruction issue)
  const float ex = lane < R ? (sizeof(T) == 2 ? __builtin_amdgcn_exp2f((e - mx) * 1.4426950408889634f) : expf(e - mx)) : 0.f;
  float wgt = ex * (sizeof(T) == 2 ? __builtin_amdgcn_rcpf(uic_wave_sum(ex)) : 1.f / uic_wave_sum(ex));
  if (p.mask) {
    wgt *= lane < R ? mkv : 0.f;
    wgt = wgt / uic_wave_sum(wgt);
  }
  if (wave == 0 && lane < R) p.alpha[(size_t)n * R + lane] = wgt;
  float acc[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    const int r = wave + u * NWAVES;
    float al = __shfl(wgt, r < R ? r : 0, 64);
    if (r >= R) al = 0.f;
    float f[VEC];
    uic_unpack<T>(va[u], f);
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] += al * f[j];
  }
  if (lh) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) s_red[wave * H + lane * VEC + j] = acc[j];
  }
  __syncthreads();
  T* ctx = (T*)p.ctx + (size_t)n * p.ldctx;
  for (int h = tid; h < H; h += NTHREADS)
  {
    float acc = 0.f;
#pragma unroll
    for (int wv = 0; wv < NWAVES; ++wv) acc += s_red[wv * H + h];
    ctx[h] = uic_from_f<T>(acc);
  }
}

// FULL: att_hid_size = rnn_size = 64 lanes x VEC (512 in bf16, the reference's sizes): every lane holds a chunk of every vector, so
// no load sits behind a lane predicate.  That matters beyond the branch itself: hipcc waits for a predicated load at the JOIN of
// its branch (s_waitcnt vmcnt(1) one instruction behind the request), and with loads returning in order that wait is for every
// load issued before it -- the kernel then ran "request 36 region rows, wait for all of them, request the small vectors, wait,
// request d ctx, wait, request its slabs, wait": three to four serial memory round trips behind the burst (round 6).  Order of
// the requests now = order of use: d ctx (+ slabs) and the att' rows (first pass), att_h, w_alpha and the p_att rows (second pass,
// still arriving while the first pass computes).
template <typename T, bool FULL>
__global__ __launch_bounds__(NTHREADS) void attn_bwd_step_fast_kernel(const UicAttnParams p) {
  constexpr int VEC = uic_vec<T>::N;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int A = p.A, H = p.H, R = p.R;
  const int Rp = (R + 3) & ~3;
  float* s_al = sm;
  float* s_da4 = s_al + Rp;           // [R][4] row-of-16 partial d alpha
  float* s_red = s_da4 + 4 * Rp;
  const int n = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (p.row_len && p.step >= p.row_len[n]) {
    // a caption that ended before this decode step: d ctx is all zero, so is everything this workgroup would compute -- written
    // without a single operand read (one scalar load decides; a third of a real batch's (step, row) pairs)
    if (p.dctx_sum) for (int h = tid; h < H; h += NTHREADS) p.dctx_sum[(size_t)n * p.ld_dctx_sum + h] = 0.f;
    for (int r = tid; r < R; r += NTHREADS) p.de[(size_t)n * R + r] = 0.f;
    T* out0 = (T*)p.d_att_h + (size_t)n * A;
    for (int a = tid; a < A; a += NTHREADS) out0[a] = uic_from_f<T>(0.f);
    return;
  }
  const bool la = FULL ? true : lane < A / VEC, lh = FULL ? true : lane < H / VEC;
  const T* pa = (const T*)p.p_att + (size_t)n * R * A + (la ? lane : 0) * VEC;
  const T* pt = (const T*)p.att + (size_t)n * R * H + (lh ? lane : 0) * VEC;
  float ah[VEC], w[VEC], dc[VEC];
  float dz[3][VEC];
  load_chunk_f32<T>(p.dctx + (size_t)n * p.lddctx, lane, lh, dc);
  // d ctx may arrive as split-K partial slabs, summed here in a fixed order (the sum is left for the accumulation pass).  The
  // first three extra slabs are requested whether or not they exist (a slab that does not is the last one again, and dropped).
  const int ns = p.dctx_nslab > 1 ? p.dctx_nslab : 1;
#pragma unroll
  for (int z = 0; z < 3; ++z) load_chunk_f32<T>(p.dctx + (size_t)min(z + 1, ns - 1) * p.dctx_slab_stride + (size_t)n * p.lddctx, lane, lh, dz[z]);
  const float al_mine = p.alpha[(size_t)n * R + (tid < R ? tid : 0)];       // (R <= 64 < NTHREADS in the fast path)
  // (scheduling barriers: left alone hipcc issues the 2 x UB row loads first -- their addresses are ready first -- and everything
  // above would again arrive behind them)
  __builtin_amdgcn_sched_barrier(0);
  uint4 vp[UB], va[UB];
#pragma unroll
  for (int u = 0; u < UB; ++u) va[u] = *(const uint4*)(pt + (size_t)min(wave + u * NWAVES, R - 1) * H);
  __builtin_amdgcn_sched_barrier(0);
  load_chunk_f32<T>(p.att_h + (size_t)n * A, lane, la, ah);
  load_chunk_f32<T>(p.w_alpha, lane, la, w);
#pragma unroll
  for (int u = 0; u < UB; ++u) vp[u] = *(const uint4*)(pa + (size_t)min(wave + u * NWAVES, R - 1) * A);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int z = 0; z < 3; ++z) {
    const bool use = z + 1 < ns;
#pragma unroll
    for (int j = 0; j < VEC; ++j) dc[j] += use ? dz[z][j] : 0.f;
  }
  for (int z = 4; z < ns; ++z) {
    float dw[VEC];
    load_chunk_f32<T>(p.dctx + (size_t)z * p.dctx_slab_stride + (size_t)n * p.lddctx, lane, lh, dw);
#pragma unroll
    for (int j = 0; j < VEC; ++j) dc[j] += dw[j];
  }
  if (p.dctx_sum && lh && wave == 0) {
#pragma unroll
    for (int q = 0; q < VEC / 4; ++q)
      *(float4*)(p.dctx_sum + (size_t)n * p.ld_dctx_sum + lane * VEC + q * 4) = make_float4(dc[q * 4], dc[q * 4 + 1], dc[q * 4 + 2], dc[q * 4 + 3]);
  }
  if (tid < R) s_al[tid] = al_mine;
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    const int r = wave + u * NWAVES;
    float f[VEC];
    uic_unpack<T>(va[u], f);
    float part = 0.f;
#pragma unroll
    for (int j = 0; j < VEC; ++j) part += dc[j] * f[j];
    part = uic_row16_sum(part);
    if ((lane & 15) == 0 && r < R) s_da4[r * 4 + (lane >> 4)] = part;
  }
  __syncthreads();
  // one lane per region: d alpha_r, then wbar = sum_r alpha_r d alpha_r by a wave reduction (every wave redundantly)
  float da_l = 0.f, al_l = 0.f;
  if (lane < R) {
    const float4 q = *(const float4*)(s_da4 + lane * 4);
    da_l = (q.x + q.y) + (q.z + q.w);
    al_l = s_al[lane];
  }
  const float wbar = uic_wave_sum(al_l * da_l);
  const float de_l = al_l * (da_l - wbar);
  if (wave == 0 && lane < R) p.de[(size_t)n * R + lane] = de_l;
  float acc[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
#pragma unroll
  for (int u = 0; u < UB; ++u) {
    const int r = wave + u * NWAVES;
    float de = __shfl(de_l, r < R ? r : 0, 64);
    if (r >= R) de = 0.f;
    float f[VEC];
    uic_unpack<T>(vp[u], f);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const float th = uic_tanh<T>(f[j] + ah[j]);
      acc[j] += de * (1.f - th * th);
    }
  }
  if (la) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) s_red[wave * A + lane * VEC + j] = acc[j] * w[j];
  }
  __syncthreads();
  T* out = (T*)p.d_att_h + (size_t)n * A;
  for (int a = tid; a < A; a += NTHREADS)
    out[a] = uic_from_f<T>(s_red[a] + s_red[A + a] + s_red[2 * A + a] + s_red[3 * A + a]);
}

inline bool al16(const void* q) { return ((uintptr_t)q & 15) == 0; }
// The fast kernels read att_h and w_alpha 16 bytes at a time (the step kernel d ctx and its slabs too, and it stores dctx_sum
// that way); the generic kernels touch those operands one word at a time, so a call that fails a condition here is theirs.
inline bool fast_ok(const UicAttnParams& p, bool step) {
  const int vec = p.dtype == UIC_BF16 ? 8 : 4;
  bool ok = p.R <= UB * NWAVES && p.A / vec <= 64 && p.H / vec <= 64 && al16(p.att_h) && al16(p.w_alpha);
  if (step) {
    ok = ok && p.lddctx % 4 == 0 && al16(p.dctx) && (p.dctx_nslab <= 1 || p.dctx_slab_stride % 4 == 0);
    ok = ok && (!p.dctx_sum || (al16(p.dctx_sum) && p.ld_dctx_sum % 4 == 0));
  }
  return ok;
}

// PART 1: d att' only (stages alpha, dctx);  PART 2: d p_att and d w_alpha only (stages att_h, de).  Two launches of
// 256-thread workgroups with < 50 KB of LDS each instead of one 1024-thread / > 100 KB workgroup per row: the small
// workgroups interleave with whatever else is resident (the fused step's other stream) instead of waiting for whole CUs.
template <typename T, int PART>
__global__ __launch_bounds__(512) void attn_bwd_accum_kernel(const UicAttnAccumParams p) {
  constexpr int VEC = uic_vec<T>::N;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int A = p.A, H = p.H, R = p.R, N = p.N;
  const int Rp = (R + 3) & ~3;
  const int nthreads = blockDim.x, nw = blockDim.x >> 6;
  const int n = blockIdx.x;
  // (the steps behind the caption's end are left out, as in the round-6 kernels; no step at all: the loops below write zeros)
  const int TS = p.row_len ? max(0, min(p.T, p.row_len[n])) : p.T;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  if constexpr (PART == 1) {
    float* s_dctx = sm;                 // [TS][H]
    float* s_al = s_dctx + TS * H;      // [TS][Rp]
    for (int h = tid; h < H; h += nthreads) {
#pragma unroll 8
      for (int t = 0; t < TS; ++t) s_dctx[t * H + h] = p.dctx_all[(size_t)t * p.dctx_step_stride + (size_t)n * p.lddctx + h];
    }
    for (int r = tid; r < R; r += nthreads) {
#pragma unroll 8
      for (int t = 0; t < TS; ++t) s_al[t * Rp + r] = p.alpha_all[((size_t)t * N + n) * R + r];
    }
    __syncthreads();
    // d att'[n,r,:] = sum_t alpha_t[r] dctx_t   (backward of the bmm, AttModel.py:555-556)
    float* dat = p.d_att + (size_t)n * R * H;
    const int nc4 = H / 4;
    for (int r = wave; r < R; r += nw) {
      for (int c = lane; c < nc4; c += 64) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int t = 0; t < TS; ++t) {
          const float al = s_al[t * Rp + r];
          const float4 d = *(const float4*)(s_dctx + t * H + c * 4);
          acc.x += al * d.x; acc.y += al * d.y; acc.z += al * d.z; acc.w += al * d.w;
        }
        *(float4*)(dat + (size_t)r * H + c * 4) = acc;
      }
    }
  } else {
    float* s_atth = sm;                 // [TS][A]
    float* s_de = s_atth + TS * A;      // [TS][Rp]
    float* s_w = s_de + TS * Rp;        // [A]
    float* s_red = s_w + A;             // [nw][A]
    // bf16 path: e^{2(p + h)} = e^{2p} e^{2h}, so the T x R x A tanh evaluations need ONE transcendental each (the
    // reciprocal) instead of two: e^{2h} is staged once per (t, a) and e^{2p} computed once per (r, a).  Exact products
    // need |2p|, |2h| <= EXP_LIM (no overflow / 0 * inf); anything larger -- never seen with trained or initial
    // weights -- takes the direct form below.
    constexpr bool FACTORED = sizeof(T) == 2;
    constexpr float EXP_LIM = 40.f, LOG2E2 = 2.8853900817779268f;
    int bad_h = 0;
    // staging, step by step (no division per element) and eight steps' loads in flight at a time: the flat loop ran TS * A /
    // nthreads dependent trips of one load each
    for (int a = tid; a < A; a += nthreads) {
#pragma unroll 8
      for (int t = 0; t < TS; ++t) {
        const float v = p.att_h_all[((size_t)t * N + n) * A + a];
        if constexpr (FACTORED) {
          bad_h |= !(fabsf(v) * 2.f <= EXP_LIM);
          s_atth[t * A + a] = __builtin_amdgcn_exp2f(v * LOG2E2);
        } else {
          s_atth[t * A + a] = v;
        }
      }
    }
    for (int r = tid; r < R; r += nthreads) {
#pragma unroll 8
      for (int t = 0; t < TS; ++t) s_de[t * Rp + r] = p.de_all[((size_t)t * N + n) * R + r];
    }
    for (int a = tid; a < A; a += nthreads) s_w[a] = p.w_alpha[a];
    for (int i = tid; i < nw * A; i += nthreads) s_red[i] = 0.f;
    const bool wg_direct = __syncthreads_or(bad_h) != 0;
    // d p_att[n,r,a] = w_a sum_t de_t[r] (1 - tanh^2(.)) ;  d w_alpha[a] += sum_{t,r} de_t[r] tanh(.)
    const T* pa = (const T*)p.p_att + (size_t)n * R * A;
    T* dpa = (T*)p.d_p_att + (size_t)n * R * A;
    const int ncA = A / VEC;
    for (int c = lane; c < ncA; c += 64) {
      float dwacc[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) dwacc[j] = 0.f;
      // (the next row's chunk is requested before this row's arithmetic: one exposed memory latency instead of one per row)
      uint4 vnext = *(const uint4*)(pa + (size_t)(wave < R ? wave : 0) * A + c * VEC);
      for (int r = wave; r < R; r += nw) {
        const uint4 v = vnext;
        if (r + nw < R) vnext = *(const uint4*)(pa + (size_t)(r + nw) * A + c * VEC);
        float f[VEC], acc[VEC];
        uic_unpack<T>(v, f);
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
        bool direct = !FACTORED;
        if constexpr (FACTORED) {
          direct = wg_direct;
#pragma unroll
          for (int j = 0; j < VEC; ++j) direct |= !(fabsf(f[j]) * 2.f <= EXP_LIM);
        }
        if (!direct) {
          float ep[VEC];
#pragma unroll
          for (int j = 0; j < VEC; ++j) ep[j] = __builtin_amdgcn_exp2f(f[j] * LOG2E2);
#pragma unroll 8
          for (int t = 0; t < TS; ++t) {
            const float de = s_de[t * Rp + r];
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
              // rc = 1 / (1 + e^{2x});  tanh x = 1 - 2 rc;  1 - tanh^2 x = 4 rc (1 - rc)
              const float rc = __builtin_amdgcn_rcpf(fmaf(ep[j], s_atth[t * A + c * VEC + j], 1.f));
              acc[j] = fmaf(de * 4.f, rc - rc * rc, acc[j]);
              dwacc[j] = fmaf(de, fmaf(-2.f, rc, 1.f), dwacc[j]);
            }
          }
        } else {
          for (int t = 0; t < TS; ++t) {
            const float de = s_de[t * Rp + r];
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
              const float h = FACTORED ? p.att_h_all[((size_t)t * N + n) * A + c * VEC + j] : s_atth[t * A + c * VEC + j];
              const float th = uic_tanh<T>(f[j] + h);
              acc[j] += de * (1.f - th * th);
              dwacc[j] += de * th;
            }
          }
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[j] *= s_w[c * VEC + j];
        *(uint4*)(dpa + (size_t)r * A + c * VEC) = uic_pack<T>(acc);
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) s_red[wave * A + c * VEC + j] = dwacc[j];
    }
    __syncthreads();
    float* part = p.d_walpha_part + (size_t)n * (A + 1);
    for (int a = tid; a < A; a += nthreads) {
      float sacc = 0.f;
      for (int wv = 0; wv < nw; ++wv) sacc += s_red[wv * A + a];
      part[a] = sacc;
    }
    if (tid == 0) {
      float s = 0.f;
      for (int t = 0; t < TS; ++t)
        for (int r = 0; r < R; ++r) s += s_de[t * Rp + r];
      part[A] = s;
    }
  }
}

// ---- round 6: the two accumulation passes rewritten for instruction count (they head the step's tail, where three streams
// compete for CU time: every VALU / LDS instruction saved here is step time).
//
// PART 1, any dtype (its operands are f32): a lane keeps the d ctx values of its four columns for SIX decode steps in registers
// and nine region accumulators, so the inner loop is FMAs fed by one wave-uniform LDS word each -- the first form re-read every
// d ctx value from LDS for every region (R x T 16-byte LDS reads per lane).  8 waves: two column halves x four region groups.
constexpr int P1_TCH = 6, P1_RU = 9;
__global__ __launch_bounds__(512) void attn_bwd_accum_p1_kernel(const UicAttnAccumParams p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int H = p.H, R = p.R, N = p.N;
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  // (the steps behind the caption's end add exact zeros: d ctx = 0 there)
  const int TS = p.row_len ? min(p.T, p.row_len[n]) : p.T;
  if (TS <= 0) {                        // a row without a live position: d att' = 0
    float4* o = (float4*)(p.d_att + (size_t)n * R * H);
    for (int i = tid; i < R * H / 4; i += 512) o[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const int TSp = (TS + P1_TCH - 1) / P1_TCH * P1_TCH;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* s_al = sm;                     // [R][TSp]: a region's weights over the steps, zero behind step TS
  for (int i = tid; i < R * TSp; i += 512) {
    const int r = i / TSp, t = i - r * TSp;
    s_al[i] = t < TS ? p.alpha_all[((size_t)t * N + n) * R + r] : 0.f;
  }
  __syncthreads();
  const int nc4 = H >> 2;
  const int rg = wave >> 1;
  float* dat = p.d_att + (size_t)n * R * H;
  const float* dc = p.dctx_all + (size_t)n * p.lddctx;
  for (int c = (wave & 1) * 64 + lane; c < nc4; c += 128) {
    for (int rb = 0; rb < R; rb += 4 * P1_RU) {
      float4 acc[P1_RU];
#pragma unroll
      for (int k = 0; k < P1_RU; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int t0 = 0; t0 < TS; t0 += P1_TCH) {
        float4 d[P1_TCH];
#pragma unroll
        for (int u = 0; u < P1_TCH; ++u) {       // (steps behind TS: a valid address, weight zero)
          const int t = t0 + u < TS ? t0 + u : TS - 1;
          d[u] = *(const float4*)(dc + (size_t)t * p.dctx_step_stride + c * 4);
        }
#pragma unroll
        for (int k = 0; k < P1_RU; ++k) {
          int r = rb + rg + 4 * k;
          r = r < R ? r : R - 1;
          const float* al = s_al + r * TSp + t0;
#pragma unroll
          for (int u = 0; u < P1_TCH; ++u) {
            const float a = al[u];
            acc[k].x = fmaf(a, d[u].x, acc[k].x); acc[k].y = fmaf(a, d[u].y, acc[k].y);
            acc[k].z = fmaf(a, d[u].z, acc[k].z); acc[k].w = fmaf(a, d[u].w, acc[k].w);
          }
        }
      }
#pragma unroll
      for (int k = 0; k < P1_RU; ++k) {
        const int r = rb + rg + 4 * k;
        if (r < R) *(float4*)(dat + (size_t)r * H + c * 4) = acc[k];
      }
    }
  }
}

// PART 2, bf16: one workgroup per (caption row, HALF of A) -- 2 N workgroups of four waves spread evenly over the 256 CUs where N
// of them left every other CU a third workgroup -- and per (region, column, step) three packed FMA-class instructions and HALF a
// reciprocal:
//   rc_t = 1 / (1 + e^{2p} e^{2h_t});   1 - tanh^2 = 4 (rc - rc^2);   tanh = 1 - 2 rc
//   d p_att = 4 w (S1 - S2),  d w_alpha = sum de - 2 sum S1   with S1 = sum_t de_t rc_t, S2 = sum_t de_t rc_t^2
//   two steps share one reciprocal: 1 / (x0 x1), rc_0 = x1 / (x0 x1), rc_1 = x0 / (x0 x1)
// Products stay finite for |2p|, |2h| <= P2_LIM (x <= 1 + e^{43}); larger values -- never seen with initial or trained weights --
// take the direct tanh form for the whole workgroup.
typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr float P2_LIM = 21.5f;
__global__ __launch_bounds__(256) void attn_bwd_accum_p2_bf16_kernel(const UicAttnAccumParams p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr float LOG2E2 = 2.8853900817779268f;
  const int A = p.A, R = p.R, N = p.N;
  const int Ah = A >> 1, nc = Ah >> 2;
  const int Rp = (R + 3) & ~3;
  const int n = blockIdx.x, a0 = blockIdx.y * Ah;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // (the steps behind the caption's end add exact zeros: d e = 0 there)
  const int TS = p.row_len ? min(p.T, p.row_len[n]) : p.T;
  if (TS <= 0) {                        // a row without a live position: d p_att = 0, no share of d w_alpha
    uint2* o = (uint2*)((bf16_t*)p.d_p_att + (size_t)n * R * A + a0);
    for (int i = tid; i < R * nc; i += 256) { const int r = i / nc, c = i - r * nc; o[(size_t)r * (A / 4) + c] = make_uint2(0u, 0u); }
    float* part0 = p.d_walpha_part + (size_t)n * (A + 1);
    for (int a = tid; a < Ah; a += 256) part0[a0 + a] = 0.f;
    if (tid == 0 && blockIdx.y == 0) part0[A] = 0.f;
    return;
  }
  float* s_eh = sm;                     // [TS][Ah]  e^{2 h_t[a]} (the direct form: h_t[a])
  float* s_de = s_eh + TS * Ah;         // [TS][Rp]
  float* s_red = s_de + TS * Rp;        // [4][Ah]
  float* s_tot = s_red + 4 * Ah;        // [4]
  // ---- staging: every load of a thread requested before the first use
  int bad = 0;
  {
    const int total = TS * nc;
    for (int i0 = tid; i0 < total; i0 += 256 * 8) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        int i = i0 + u * 256;
        i = i < total ? i : total - 1;
        const int t = i / nc, c = i - t * nc;
        v[u] = *(const float4*)(p.att_h_all + ((size_t)t * N + n) * A + a0 + c * 4);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = i0 + u * 256;
        if (i < total) {
          bad |= !(fabsf(v[u].x) * 2.f <= P2_LIM) | !(fabsf(v[u].y) * 2.f <= P2_LIM) | !(fabsf(v[u].z) * 2.f <= P2_LIM) | !(fabsf(v[u].w) * 2.f <= P2_LIM);
          *(float4*)(s_eh + (size_t)i * 4) = v[u];          // (t * Ah + c * 4 == i * 4)
        }
      }
    }
    const int nde = TS * R;
    float dsum = 0.f;
    for (int i0 = tid; i0 < nde; i0 += 256 * 4) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        int i = i0 + u * 256;
        i = i < nde ? i : nde - 1;
        const int t = i / R, r = i - t * R;
        v[u] = p.de_all[((size_t)t * N + n) * R + r];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * 256;
        if (i < nde) { const int t = i / R, r = i - t * R; s_de[t * Rp + r] = v[u]; dsum += v[u]; }
      }
    }
    dsum = uic_wave_sum(dsum);
    if (lane == 0) s_tot[wave] = dsum;
  }
  const bf16_t* pa = (const bf16_t*)p.p_att + (size_t)n * R * A + a0;
  bf16_t* dpa = (bf16_t*)p.d_p_att + (size_t)n * R * A + a0;
  const bool direct = __syncthreads_or(bad) != 0;
  if (!direct) {         // e^{2h} in place (each thread the entries it staged itself would do, but the barrier is behind us anyway)
    for (int i = tid; i < TS * Ah; i += 256) s_eh[i] = __builtin_amdgcn_exp2f(s_eh[i] * LOG2E2);
    __syncthreads();
  }
  for (int c = lane; c < nc; c += 64) {
    const float4 w4 = *(const float4*)(p.w_alpha + a0 + c * 4);
    f32x2 dw0 = {0.f, 0.f}, dw1 = {0.f, 0.f};            // sum over this wave's regions of S1 (direct form: of de tanh)
    {
      // (the next region's chunk is requested before this region's arithmetic -- ~1.5 us of it: the latency is covered)
      uint2 vnext = *(const uint2*)(pa + (size_t)(wave < R ? wave : R - 1) * A + c * 4);
#pragma clang loop unroll(disable)
      for (int r = wave; r < R; r += 4) {
        const uint2 pvk = vnext;
        vnext = *(const uint2*)(pa + (size_t)(r + 4 < R ? r + 4 : R - 1) * A + c * 4);
        const float f0 = __uint_as_float(pvk.x << 16), f1 = __uint_as_float(pvk.x & 0xffff0000u);
        const float f2 = __uint_as_float(pvk.y << 16), f3 = __uint_as_float(pvk.y & 0xffff0000u);
        float o[4];
        const bool big = !(fabsf(f0) * 2.f <= P2_LIM) | !(fabsf(f1) * 2.f <= P2_LIM) | !(fabsf(f2) * 2.f <= P2_LIM) | !(fabsf(f3) * 2.f <= P2_LIM);
        if (!direct && !__any(big)) {
          const f32x2 ep0 = {__builtin_amdgcn_exp2f(f0 * LOG2E2), __builtin_amdgcn_exp2f(f1 * LOG2E2)};
          const f32x2 ep1 = {__builtin_amdgcn_exp2f(f2 * LOG2E2), __builtin_amdgcn_exp2f(f3 * LOG2E2)};
          const f32x2 one = {1.f, 1.f};
          f32x2 s1a = {0.f, 0.f}, s1b = {0.f, 0.f}, s2a = {0.f, 0.f}, s2b = {0.f, 0.f};
          const float* eh = s_eh + c * 4;
          const float* de = s_de + r;
          int t = 0;
#pragma unroll 2
          for (; t + 1 < TS; t += 2) {
            const float4 e0 = *(const float4*)(eh + t * Ah), e1 = *(const float4*)(eh + (t + 1) * Ah);
            const float d0 = de[t * Rp], d1 = de[(t + 1) * Rp];
            const f32x2 d0v = {d0, d0}, d1v = {d1, d1};
            {
              const f32x2 x0 = __builtin_elementwise_fma(ep0, (f32x2){e0.x, e0.y}, one), x1 = __builtin_elementwise_fma(ep0, (f32x2){e1.x, e1.y}, one);
              const f32x2 pr = x0 * x1;
              const f32x2 inv = {__builtin_amdgcn_rcpf(pr.x), __builtin_amdgcn_rcpf(pr.y)};
              const f32x2 rc0 = inv * x1, rc1 = inv * x0;
              s1a = __builtin_elementwise_fma(d0v, rc0, s1a); s2a = __builtin_elementwise_fma(d0v * rc0, rc0, s2a);
              s1a = __builtin_elementwise_fma(d1v, rc1, s1a); s2a = __builtin_elementwise_fma(d1v * rc1, rc1, s2a);
            }
            {
              const f32x2 x0 = __builtin_elementwise_fma(ep1, (f32x2){e0.z, e0.w}, one), x1 = __builtin_elementwise_fma(ep1, (f32x2){e1.z, e1.w}, one);
              const f32x2 pr = x0 * x1;
              const f32x2 inv = {__builtin_amdgcn_rcpf(pr.x), __builtin_amdgcn_rcpf(pr.y)};
              const f32x2 rc0 = inv * x1, rc1 = inv * x0;
              s1b = __builtin_elementwise_fma(d0v, rc0, s1b); s2b = __builtin_elementwise_fma(d0v * rc0, rc0, s2b);
              s1b = __builtin_elementwise_fma(d1v, rc1, s1b); s2b = __builtin_elementwise_fma(d1v * rc1, rc1, s2b);
            }
          }
          if (t < TS) {
            const float4 e0 = *(const float4*)(eh + t * Ah);
            const float d0 = de[t * Rp];
            const f32x2 d0v = {d0, d0};
            const f32x2 x0 = __builtin_elementwise_fma(ep0, (f32x2){e0.x, e0.y}, one), x1 = __builtin_elementwise_fma(ep1, (f32x2){e0.z, e0.w}, one);
            const f32x2 rc0 = {__builtin_amdgcn_rcpf(x0.x), __builtin_amdgcn_rcpf(x0.y)}, rc1 = {__builtin_amdgcn_rcpf(x1.x), __builtin_amdgcn_rcpf(x1.y)};
            s1a = __builtin_elementwise_fma(d0v, rc0, s1a); s2a = __builtin_elementwise_fma(d0v * rc0, rc0, s2a);
            s1b = __builtin_elementwise_fma(d0v, rc1, s1b); s2b = __builtin_elementwise_fma(d0v * rc1, rc1, s2b);
          }
          dw0 += s1a; dw1 += s1b;
          o[0] = 4.f * (s1a.x - s2a.x) * w4.x; o[1] = 4.f * (s1a.y - s2a.y) * w4.y;
          o[2] = 4.f * (s1b.x - s2b.x) * w4.z; o[3] = 4.f * (s1b.y - s2b.y) * w4.w;
        } else {
          // direct form (s_eh holds h when the whole workgroup is direct, e^{2h} otherwise: h is re-read from memory then)
          const float f[4] = {f0, f1, f2, f3};
          const float w[4] = {w4.x, w4.y, w4.z, w4.w};
          float accd[4] = {0.f, 0.f, 0.f, 0.f}, dwd[4] = {0.f, 0.f, 0.f, 0.f};
          for (int t = 0; t < TS; ++t) {
            const float d0 = s_de[t * Rp + r];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float h = direct ? s_eh[t * Ah + c * 4 + j] : p.att_h_all[((size_t)t * N + n) * A + a0 + c * 4 + j];
              const float th = uic_tanh<bf16_t>(f[j] + h);
              accd[j] += d0 * (1.f - th * th);
              dwd[j] += d0 * th;
            }
          }
          // (the epilogue below computes sum de - 2 sum S1: hand it S1-equivalents, (sum_t de - sum_t de tanh) / 2)
          float dsr = 0.f;
          for (int t = 0; t < TS; ++t) dsr += s_de[t * Rp + r];
          dw0.x += 0.5f * (dsr - dwd[0]); dw0.y += 0.5f * (dsr - dwd[1]); dw1.x += 0.5f * (dsr - dwd[2]); dw1.y += 0.5f * (dsr - dwd[3]);
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = accd[j] * w[j];
        }
        uint2 st;
        st.x = uic_pack_bf16x2(o[0], o[1]); st.y = uic_pack_bf16x2(o[2], o[3]);
        *(uint2*)(dpa + (size_t)r * A + c * 4) = st;
      }
    }
    *(float4*)(s_red + wave * Ah + c * 4) = make_float4(dw0.x, dw0.y, dw1.x, dw1.y);
  }
  __syncthreads();
  const float tot = (s_tot[0] + s_tot[1]) + (s_tot[2] + s_tot[3]);
  float* part = p.d_walpha_part + (size_t)n * (A + 1);
  for (int a = tid; a < Ah; a += 256)
    part[a0 + a] = tot - 2.f * ((s_red[a] + s_red[Ah + a]) + (s_red[2 * Ah + a] + s_red[3 * Ah + a]));
  if (tid == 0 && blockIdx.y == 0) part[A] = tot;
}

int check_common(const char* who, int dtype, int N, int R, int A, int H) {
  const int vec = dtype == UIC_BF16 ? 8 : 4;
  UIC_REQUIRE(dtype == UIC_F32 || dtype == UIC_BF16, "%s: bad dtype %d", who, dtype);
  UIC_REQUIRE(N >= 0 && R > 0 && A > 0 && H > 0, "%s: bad sizes N=%d R=%d A=%d H=%d", who, N, R, A, H);
  UIC_REQUIRE(A % vec == 0 && H % vec == 0, "%s: A=%d and H=%d must be multiples of %d", who, A, H, vec);
  return UIC_OK;
}

// (more than 64 KB of dynamic LDS has to be asked for per kernel, up to the 160 KB of a CU)
template <typename K>
int launch_attn(K kernel, const UicAttnParams& p, int nthreads, size_t lds, hipStream_t s, const char* what) {
  if (lds > 64 * 1024)
    UIC_TRY(uic_check_hip(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "hipFuncSetAttribute"));
  hipLaunchKernelGGL(kernel, dim3(p.N), dim3(nthreads), lds, s, p);
  UIC_LAUNCH_CHECK(what);
  return UIC_OK;
}

}  // namespace

int uic_attention_fwd_launch(const UicAttnParams& p, hipStream_t s, int* kernel_id) {
  UIC_TRY(check_common("attention_fwd", p.dtype, p.N, p.R, p.A, p.H));
  UIC_REQUIRE(p.att_h && p.p_att && p.att && p.w_alpha && p.alpha && p.ctx, "attention_fwd: null pointer");
  UIC_REQUIRE(p.ldctx >= p.H && (!p.mask || p.ldmask >= p.R), "attention_fwd: ld_ctx=%d < H=%d or ld_mask=%d < R=%d", p.ldctx, p.H, p.ldmask, p.R);
  UIC_REQUIRE(al16(p.p_att) && al16(p.att), "attention_fwd: p_att and att must be 16-byte aligned (every kernel reads them 16 bytes at a time)");
  const size_t lds = sizeof(float) * (2 * (size_t)p.A + 4 * (size_t)p.R + 4 + NWAVES * (size_t)p.H);
  UIC_REQUIRE(lds <= 160 * 1024, "attention_fwd: needs %zu B of LDS", lds);
  const int vec = p.dtype == UIC_BF16 ? 8 : 4;
  const bool fast = fast_ok(p, false), full = fast && p.A == 64 * vec && p.H == 64 * vec;
  if (kernel_id) *kernel_id = full ? UIC_ATTN_FAST_FULL : fast ? UIC_ATTN_FAST : UIC_ATTN_GENERIC;
  if (p.N == 0) return UIC_OK;
  if (fast) {
    // waves per caption row, measured at N = 640 (bf16; 3 alternating passes each): 4 -> 12.1 us cache-resident / 13.5 us
    // HBM-cold, 8 -> 11.8-12.5 / 12.9-13.1, 9 -> 12.3 / 13.1, 6 -> 12.4 / 13.4, 12 -> 11.7 / 12.8-12.9 (3 regions per wave).
    // 12 costs the two-stream training step 0.4 % (a 768-thread workgroup leaves the side stream fewer free slots) and is
    // taken for the steadier, faster kernel.
    const size_t lds8 = sizeof(float) * (4 * (size_t)p.R + 4 + 8 * (size_t)p.H);
    const size_t lds12 = sizeof(float) * (4 * (size_t)p.R + 4 + 12 * (size_t)p.H);
    if (p.dtype == UIC_BF16) {
      if (full) hipLaunchKernelGGL((attn_fwd_fast_kernel<bf16_t, 12, true>), dim3(p.N), dim3(768), lds12, s, p);
      else hipLaunchKernelGGL((attn_fwd_fast_kernel<bf16_t, 12, false>), dim3(p.N), dim3(768), lds12, s, p);
    } else {
      if (full) hipLaunchKernelGGL((attn_fwd_fast_kernel<float, 8, true>), dim3(p.N), dim3(512), lds8, s, p);
      else hipLaunchKernelGGL((attn_fwd_fast_kernel<float, 8, false>), dim3(p.N), dim3(512), lds8, s, p);
    }
    UIC_LAUNCH_CHECK("attn_fwd_fast_kernel");
    return UIC_OK;
  }
  if (p.dtype == UIC_BF16) return launch_attn(attn_fwd_kernel<bf16_t>, p, NTHREADS, lds, s, "attn_fwd_kernel");
  return launch_attn(attn_fwd_kernel<float>, p, NTHREADS, lds, s, "attn_fwd_kernel");
}

int uic_attention_bwd_step_launch(const UicAttnParams& p, hipStream_t s, int* kernel_id) {
  UIC_TRY(check_common("attention_bwd_step", p.dtype, p.N, p.R, p.A, p.H));
  UIC_REQUIRE(p.att_h && p.p_att && p.att && p.w_alpha && p.alpha && p.dctx && p.de && p.d_att_h,
              "attention_bwd_step: null pointer");
  UIC_REQUIRE(p.lddctx >= p.H && p.dctx_nslab >= 0 && (!p.dctx_sum || p.ld_dctx_sum >= p.H),
              "attention_bwd_step: lddctx=%d or ld_dctx_sum=%d < H=%d, or nslab=%d < 0", p.lddctx, p.ld_dctx_sum, p.H, p.dctx_nslab);
  UIC_REQUIRE(!p.row_len || p.step >= 0, "attention_bwd_step: step=%d with a row_len", p.step);
  UIC_REQUIRE(al16(p.p_att) && al16(p.att), "attention_bwd_step: p_att and att must be 16-byte aligned (every kernel reads them 16 bytes at a time)");
  const size_t lds = sizeof(float) * (2 * (size_t)p.A + p.H + 5 * ((p.R + 3) & ~3) + NWAVES * (size_t)p.A);
  UIC_REQUIRE(lds <= 160 * 1024, "attention_bwd_step: needs %zu B of LDS", lds);
  const int vec = p.dtype == UIC_BF16 ? 8 : 4;
  const bool fast = fast_ok(p, true), full = fast && p.A == 64 * vec && p.H == 64 * vec;
  if (kernel_id) *kernel_id = full ? UIC_ATTN_FAST_FULL : fast ? UIC_ATTN_FAST : UIC_ATTN_GENERIC;
  if (p.N == 0) return UIC_OK;
  const char* what = "attn_bwd_step_kernel";
  if (fast) {
    if (p.dtype == UIC_BF16) return full ? launch_attn(attn_bwd_step_fast_kernel<bf16_t, true>, p, NTHREADS, lds, s, what)
                                         : launch_attn(attn_bwd_step_fast_kernel<bf16_t, false>, p, NTHREADS, lds, s, what);
    return full ? launch_attn(attn_bwd_step_fast_kernel<float, true>, p, NTHREADS, lds, s, what)
                : launch_attn(attn_bwd_step_fast_kernel<float, false>, p, NTHREADS, lds, s, what);
  }
  if (p.dtype == UIC_BF16) return launch_attn(attn_bwd_step_kernel<bf16_t>, p, NTHREADS, lds, s, what);
  return launch_attn(attn_bwd_step_kernel<float>, p, NTHREADS, lds, s, what);
}

int uic_attention_bwd_accum_launch(const UicAttnAccumParams& p, hipStream_t s, int* kernel_id) {
  UIC_TRY(check_common("attention_bwd_accum", p.dtype, p.N, p.R, p.A, p.H));
  UIC_REQUIRE(p.T > 0, "attention_bwd_accum: T=%d", p.T);
  UIC_REQUIRE(p.att_h_all && p.alpha_all && p.de_all && p.dctx_all && p.p_att && p.w_alpha && p.d_att && p.d_p_att &&
                  p.d_walpha_part, "attention_bwd_accum: null pointer");
  UIC_REQUIRE(p.lddctx >= p.H, "attention_bwd_accum: lddctx=%d < H=%d", p.lddctx, p.H);
  const int Rp = (p.R + 3) & ~3;
  // measured at the benchmark shapes: PART 1 (f32 FMAs over LDS-staged rows) 42 -> 32 us with 8 waves per workgroup, PART 2
  // (one reciprocal per element) 110 us with 4 waves, 118 with 8
  // round 6 forms (above): PART 2 for bf16 with an even split of A into 4-column chunks, PART 1 wherever a lane's 16-byte loads
  // and stores are aligned
  const bool p1_new = p.H % 4 == 0 && p.lddctx % 4 == 0 && p.dctx_step_stride % 4 == 0 && al16(p.dctx_all);
  const bool p2_new = p.dtype == UIC_BF16 && p.A % 8 == 0 && al16(p.att_h_all) && al16(p.w_alpha) &&
                      ((uintptr_t)p.p_att & 7) == 0 && ((uintptr_t)p.d_p_att & 7) == 0;
  // what no kernel honours: both PART 1 kernels store d att' 16 bytes at a time, and the first PART 2 kernel reads p_att and writes
  // d p_att 16 bytes at a time (the round-6 one 8).  att_h_all, w_alpha and d ctx are read one word at a time by the first forms.
  UIC_REQUIRE(al16(p.d_att), "attention_bwd_accum: d_att must be 16-byte aligned");
  UIC_REQUIRE(p2_new || (al16(p.p_att) && al16(p.d_p_att)), "attention_bwd_accum: p_att and d_p_att must be 16-byte aligned (8-byte for the bf16 kernel)");
  const size_t lds1n = sizeof(float) * (size_t)p.R * ((p.T + P1_TCH - 1) / P1_TCH * P1_TCH);
  const size_t lds2n = sizeof(float) * ((size_t)p.T * (p.A / 2 + Rp) + 4 * (size_t)(p.A / 2) + 4);
  UIC_REQUIRE(lds1n <= 160 * 1024 && lds2n <= 160 * 1024, "attention_bwd_accum: needs %zu B of LDS (T=%d)", lds1n > lds2n ? lds1n : lds2n, p.T);
  const int nthreads1 = 512, nthreads2 = 256;
  const size_t lds1 = sizeof(float) * ((size_t)p.T * (p.H + Rp));
  const size_t lds2 = sizeof(float) * ((size_t)p.T * (p.A + Rp) + p.A + (nthreads2 / 64) * (size_t)p.A);
  UIC_REQUIRE(lds1 <= 160 * 1024 && lds2 <= 160 * 1024, "attention_bwd_accum: needs %zu B of LDS (T=%d)", lds1 > lds2 ? lds1 : lds2, p.T);
  if (kernel_id) *kernel_id = (p1_new ? UIC_ATTN_ACCUM_P1_R6 : 0) | (p2_new ? UIC_ATTN_ACCUM_P2_R6 : 0);
  if (p.N == 0) return UIC_OK;
  if (p2_new) {
    if (lds2n > 64 * 1024) UIC_TRY(uic_check_hip(hipFuncSetAttribute((const void*)attn_bwd_accum_p2_bf16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2n), "hipFuncSetAttribute"));
    hipLaunchKernelGGL(attn_bwd_accum_p2_bf16_kernel, dim3(p.N, 2), dim3(256), lds2n, s, p);
  }
  if (p1_new) {
    if (lds1n > 64 * 1024) UIC_TRY(uic_check_hip(hipFuncSetAttribute((const void*)attn_bwd_accum_p1_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1n), "hipFuncSetAttribute"));
    hipLaunchKernelGGL(attn_bwd_accum_p1_kernel, dim3(p.N), dim3(512), lds1n, s, p);
  }
#define ACCUM_LAUNCH(TT)                                                                                                          \
  do {                                                                                                                            \
    if (!p1_new && lds1 > 64 * 1024) UIC_TRY(uic_check_hip(hipFuncSetAttribute((const void*)attn_bwd_accum_kernel<TT, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1), "hipFuncSetAttribute")); \
    if (!p2_new && lds2 > 64 * 1024) UIC_TRY(uic_check_hip(hipFuncSetAttribute((const void*)attn_bwd_accum_kernel<TT, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2), "hipFuncSetAttribute")); \
    if (!p2_new) hipLaunchKernelGGL((attn_bwd_accum_kernel<TT, 2>), dim3(p.N), dim3(nthreads2), lds2, s, p);                        \
    if (!p1_new) hipLaunchKernelGGL((attn_bwd_accum_kernel<TT, 1>), dim3(p.N), dim3(nthreads1), lds1, s, p);                        \
  } while (0)
  if (p.dtype == UIC_BF16) ACCUM_LAUNCH(bf16_t); else ACCUM_LAUNCH(float);
#undef ACCUM_LAUNCH
  UIC_LAUNCH_CHECK("attn_bwd_accum_kernel");
  return UIC_OK;
}
