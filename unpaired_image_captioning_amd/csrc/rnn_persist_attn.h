// The attention phase of the persistent recurrence kernels (Attention.forward behind h2att, P/models/AttModel.py:544-556):
// attn_phase, all waves of the workgroup per caption row (the generic kernel and the decode kernel), and attn_phase_wave, one
// wave per caption row (the weight-stationary training kernel).
#pragma once
#include "rnn_persist_common.h"

namespace {

// Attention.forward after h2att (P/models/AttModel.py:544-556), all 8 waves per caption row (attention.hip's
// attn_fwd_fast_kernel with the row's att_h read past the L1).  A workgroup has up to three rows per step; their loads are
// software-pipelined through three register slots of 5 x 16 B per lane (p_att of a row, att' of a row), so that two
// slots' worth of loads are always in flight while the third is being consumed.
template <typename T> struct AttnCfg {
  static constexpr int VEC = 16 / (int)sizeof(T);
  static constexpr int CH = HH / VEC / 64;        // 16-byte chunks of a 512-wide row per lane (bf16: 1, f32: 2)
};
template <typename T, int NW> struct AttnSlot { uint4 v[ATT_R / NW][AttnCfg<T>::CH]; };
template <typename T> struct AttnHead { u32x4 ah[AttnCfg<T>::CH][AttnCfg<T>::VEC / 4]; };

// STREAM: the load is non-temporal (does not stay in the XCD's L2).  A workgroup re-reads the SAME rows of p_att and att'
// every decode step: 5.9 MB per XCD and step against a 4 MB L2, so with one policy for both the L2 thrashes; streaming att'
// lets the 2.95 MB of p_att rows stay resident.
template <typename T, int NW, bool STREAM>
__device__ __forceinline__ void attn_load_slot(const Ctx& c, int R, const T* base, AttnSlot<T, NW>& q) {
  constexpr int VEC = AttnCfg<T>::VEC, CH = AttnCfg<T>::CH;
#pragma unroll
  for (int u = 0; u < ATT_R / NW; ++u) {
    const int r = min(c.wave + u * NW, R - 1);
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const u32x4* src = (const u32x4*)(base + (unsigned)(r * HH + (c.lane + 64 * k) * VEC));
      const u32x4 v = *src;
      q.v[u][k] = make_uint4(v.x, v.y, v.z, v.w);
    }
  }
}
template <typename T>
__device__ __forceinline__ void attn_load_head(const Ctx& c, const float* att_h_row, AttnHead<T>& q) {
  constexpr int VEC = AttnCfg<T>::VEC, CH = AttnCfg<T>::CH;
  const __amdgpu_buffer_rsrc_t rh = rsrc_of(att_h_row);
#pragma unroll
  for (int k = 0; k < CH; ++k)
#pragma unroll
    for (int v = 0; v < VEC / 4; ++v) q.ah[k][v] = bload<true>(rh, (unsigned)(((c.lane + 64 * k) * VEC + v * 4) * 4), 0);
}
// scores + softmax (+ mask renormalisation) of row n; returns this lane's weight (lane r < R holds alpha_r)
template <typename T, int NW>
__device__ __forceinline__ float attn_scores(const Ctx& c, const UicRnnFwdParams& p, int n, const AttnSlot<T, NW>& vp, const AttnHead<T>& hd,
                                             float* alpha) {
  constexpr int VEC = AttnCfg<T>::VEC, CH = AttnCfg<T>::CH;
  const int R = p.R;
  float* s_e = (float*)c.smem + 64;               // [R][4] row-of-16 partial scores (word 0 of smem is the barrier flag)
  float ah[CH][VEC], w[CH][VEC];
#pragma unroll
  for (int k = 0; k < CH; ++k)
#pragma unroll
    for (int v = 0; v < VEC / 4; ++v) {
      ah[k][v * 4 + 0] = __uint_as_float(hd.ah[k][v].x); ah[k][v * 4 + 1] = __uint_as_float(hd.ah[k][v].y);
      ah[k][v * 4 + 2] = __uint_as_float(hd.ah[k][v].z); ah[k][v * 4 + 3] = __uint_as_float(hd.ah[k][v].w);
      const float4 ww = *(const float4*)(p.w_alpha + (c.lane + 64 * k) * VEC + v * 4);
      w[k][v * 4 + 0] = ww.x; w[k][v * 4 + 1] = ww.y; w[k][v * 4 + 2] = ww.z; w[k][v * 4 + 3] = ww.w;
    }
  const float b_alpha = p.b_alpha ? p.b_alpha[0] : 0.f;
#pragma unroll
  for (int u = 0; u < ATT_R / NW; ++u) {
    const int r = c.wave + u * NW;
    float part = 0.f;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      float f[VEC];
      uic_unpack<T>(vp.v[u][k], f);
#pragma unroll
      for (int j = 0; j < VEC; ++j) part += w[k][j] * uic_tanh<T>(f[j] + ah[k][j]);
    }
    part = uic_row16_sum(part);
    if (c.l15 == 0 && r < R) s_e[r * 4 + c.lq] = part;
  }
  __syncthreads();
  const float* mk = p.mask ? p.mask + (size_t)n * p.ldmask : nullptr;
  float e = -INFINITY;
  if (c.lane < R) {
    const float4 qq = *(const float4*)(s_e + c.lane * 4);
    e = (qq.x + qq.y) + (qq.z + qq.w) + b_alpha;
  }
  const float mx = uic_wave_max(e);
  // (bf16 path: one v_exp_f32 / v_rcp_f32 instead of libm's exp and an IEEE division -- this kernel is made of instruction issue)
  const float ex = c.lane < R ? (sizeof(T) == 2 ? __builtin_amdgcn_exp2f((e - mx) * 1.4426950408889634f) : expf(e - mx)) : 0.f;
  float wgt = ex * (sizeof(T) == 2 ? __builtin_amdgcn_rcpf(uic_wave_sum(ex)) : 1.f / uic_wave_sum(ex));
  if (mk) {
    wgt *= c.lane < R ? mk[c.lane] : 0.f;
    wgt = wgt / uic_wave_sum(wgt);
  }
  if (c.wave == 0 && c.lane < R) alpha[(unsigned)(n * R + c.lane)] = wgt;
  return wgt;
}
template <typename T, bool SAFE, int NW>
__device__ __forceinline__ void attn_context(const Ctx& c, const UicRnnFwdParams& p, int n, const AttnSlot<T, NW>& va, float wgt, T* ctx) {
  constexpr int VEC = AttnCfg<T>::VEC, CH = AttnCfg<T>::CH;
  const int R = p.R;
  float* s_red = (float*)c.smem + 64 + 4 * ((R + 3) & ~3);        // [NW][HH]
  float acc[CH][VEC];
#pragma unroll
  for (int k = 0; k < CH; ++k)
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[k][j] = 0.f;
#pragma unroll
  for (int u = 0; u < ATT_R / NW; ++u) {
    const int r = c.wave + u * NW;
    float al = __shfl(wgt, r < R ? r : 0, 64);
    if (r >= R) al = 0.f;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      float f[VEC];
      uic_unpack<T>(va.v[u][k], f);
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc[k][j] += al * f[j];
    }
  }
#pragma unroll
  for (int k = 0; k < CH; ++k)
#pragma unroll
    for (int j = 0; j < VEC; ++j) s_red[c.wave * HH + (c.lane + 64 * k) * VEC + j] = acc[k][j];
  __syncthreads();
#pragma unroll
  for (int h = c.tid; h < HH; h += NW * 64) {
    float sacc = 0.f;
#pragma unroll
    for (int wv = 0; wv < NW; ++wv) sacc += s_red[wv * HH + h];
    st_x<SAFE>(ctx + (unsigned)(n * HH + h), sacc);
  }
  __syncthreads();
}
// the attention phase of one workgroup: rows rank, rank + 32, rank + 64 of the group (<= 3).  SLOTS = 3: p_att and att' of
// a row plus p_att of the next one in flight; SLOTS = 2 (the weight-stationary kernel, whose registers hold weights):
// one slot in flight while the other is consumed.
template <typename T, bool SAFE, int NW, int SLOTS>
__device__ __forceinline__ void attn_phase(const Ctx& c, const UicRnnFwdParams& p, const float* att_h, float* alpha, T* ctx) {
  const int R = p.R;
  const int r0 = c.rank, r1 = c.rank + PW, r2 = c.rank + 2 * PW;
  if (r0 >= c.nrow) return;
  const bool has1 = r1 < c.nrow, has2 = r2 < c.nrow;
  const int n0 = c.rbegin + r0, n1 = c.rbegin + r1, n2 = c.rbegin + r2;
  const T* P = (const T*)p.p_att;
  const T* V = (const T*)p.att;
  AttnHead<T> h0, h1;
  if constexpr (SLOTS == 3) {
    AttnSlot<T, NW> s0, s1, s2;
    attn_load_head<T>(c, att_h + (size_t)n0 * HH, h0);
    attn_load_slot<T, NW, false>(c, R, P + (size_t)n0 * R * HH, s0);
    attn_load_slot<T, NW, true>(c, R, V + (size_t)n0 * R * HH, s1);
    if (has1) {
      attn_load_head<T>(c, att_h + (size_t)n1 * HH, h1);
      attn_load_slot<T, NW, false>(c, R, P + (size_t)n1 * R * HH, s2);
    }
    float wgt = attn_scores<T, NW>(c, p, n0, s0, h0, alpha);
    if (has1) attn_load_slot<T, NW, true>(c, R, V + (size_t)n1 * R * HH, s0);
    attn_context<T, SAFE, NW>(c, p, n0, s1, wgt, ctx);
    if (has2) {
      attn_load_head<T>(c, att_h + (size_t)n2 * HH, h0);
      attn_load_slot<T, NW, false>(c, R, P + (size_t)n2 * R * HH, s1);
    }
    if (has1) {
      wgt = attn_scores<T, NW>(c, p, n1, s2, h1, alpha);
      if (has2) attn_load_slot<T, NW, true>(c, R, V + (size_t)n2 * R * HH, s2);
      attn_context<T, SAFE, NW>(c, p, n1, s0, wgt, ctx);
    }
    if (has2) {
      wgt = attn_scores<T, NW>(c, p, n2, s1, h0, alpha);
      attn_context<T, SAFE, NW>(c, p, n2, s2, wgt, ctx);
    }
  } else {
    AttnSlot<T, NW> s0, s1;
    attn_load_head<T>(c, att_h + (size_t)n0 * HH, h0);
    attn_load_slot<T, NW, false>(c, R, P + (size_t)n0 * R * HH, s0);
    attn_load_slot<T, NW, true>(c, R, V + (size_t)n0 * R * HH, s1);
    float wgt = attn_scores<T, NW>(c, p, n0, s0, h0, alpha);
    if (has1) {
      attn_load_head<T>(c, att_h + (size_t)n1 * HH, h1);
      attn_load_slot<T, NW, false>(c, R, P + (size_t)n1 * R * HH, s0);
    }
    attn_context<T, SAFE, NW>(c, p, n0, s1, wgt, ctx);
    if (has1) {
      attn_load_slot<T, NW, true>(c, R, V + (size_t)n1 * R * HH, s1);
      wgt = attn_scores<T, NW>(c, p, n1, s0, h1, alpha);
      if (has2) {
        attn_load_head<T>(c, att_h + (size_t)n2 * HH, h0);
        attn_load_slot<T, NW, false>(c, R, P + (size_t)n2 * R * HH, s0);
      }
      attn_context<T, SAFE, NW>(c, p, n1, s1, wgt, ctx);
    }
    if (has2) {
      attn_load_slot<T, NW, true>(c, R, V + (size_t)n2 * R * HH, s1);
      wgt = attn_scores<T, NW>(c, p, n2, s0, h0, alpha);
      attn_context<T, SAFE, NW>(c, p, n2, s1, wgt, ctx);
    }
  }
}

// Round 5: the attention phase of the weight-stationary TRAINING kernel with ONE WAVE PER CAPTION ROW.  The four-waves-per-row form
// above is a chain of dependent stages per row (head load, two workgroup barriers, an LDS reduction between the waves, the
// softmax, another barrier, the context reduction): ~4 us of latency per row beside 2 us of arithmetic, three rows in a row for
// half of the workgroups (17.4 us) and two for the others, who then wait in the group barrier.  Here wave w of workgroup `rank`
// takes row rank + 32 w of the group by itself (waves 0..2; 80 rows on 96 of the group's 128 waves): no workgroup barrier, no
// cross-wave reduction, every wave one row -- the phase is one row's arithmetic on one SIMD (~8 us, 4.8 of it v_exp / v_rcp) and
// the same length for every workgroup.  Region rows arrive in chunks of 10 through two register buffers; att's first chunk is
// requested before the scores so that the context starts without a load latency.  The context is one running sum over the
// regions instead of four partial sums.
constexpr int AW_CR = 10;                             // regions per chunk of attn_phase_wave
// the first chunk of the wave's p_att rows: requested between the two halves of the group barrier in front of the phase
__device__ __forceinline__ void attn_wave_preload(const Ctx& c, const UicRnnFwdParams& p, uint4 (&q)[AW_CR]) {
  const int r = c.rank + PW * c.wave;
  if (r >= c.nrow) return;
  const bf16_t* P = (const bf16_t*)p.e_att + (size_t)(c.rbegin + r) * p.R * HH + c.lane * 8;
#pragma unroll
  for (int u = 0; u < AW_CR; ++u) {
    const u32x4 v = *(const u32x4*)(P + (unsigned)(min(u, p.R - 1) * HH));
    q[u] = make_uint4(v.x, v.y, v.z, v.w);
  }
}
template <bool SAFE>
__device__ __forceinline__ void attn_phase_wave(const Ctx& c, const UicRnnFwdParams& p, const float* att_h, float* alpha, bf16_t* ctx,
                                                const uint4 (&pre)[AW_CR]) {
  typedef bf16_t T;
  const int R = p.R;
  const int r = c.rank + PW * c.wave;                 // this wave's row of the group (uniform per wave)
  if (r >= c.nrow) return;
  const int n = c.rbegin + r;
  constexpr int CR = AW_CR, NCH = ATT_R / CR;
  static_assert(NCH * CR == ATT_R, "chunks cover the region slots");
  const T* P = (const T*)p.e_att + (size_t)n * R * HH + c.lane * 8;      // e^{2 p_att} (round 6, below)
  const T* V = (const T*)p.att + (size_t)n * R * HH + c.lane * 8;
  float* s_e = (float*)c.smem + 64 + c.wave * (4 * ATT_R);      // [R][4] row-of-16 partial scores of this wave's row (word 0: barrier flag)
  auto load_chunk = [&](const T* base, int ch, uint4 (&q)[CR]) {
#pragma unroll
    for (int u = 0; u < CR; ++u) {
      const int rr = min(ch * CR + u, R - 1);
      const u32x4 v = *(const u32x4*)(base + (unsigned)(rr * HH));
      q[u] = make_uint4(v.x, v.y, v.z, v.w);
    }
  };
  const __amdgpu_buffer_rsrc_t rh = rsrc_of(att_h + (size_t)n * HH);
  const u32x4 h0 = bload<true>(rh, (unsigned)(c.lane * 32), 0), h1 = bload<true>(rh, (unsigned)(c.lane * 32 + 16), 0);
  // the region mask of this lane's region, requested HERE and without a branch (no mask: any readable word, ignored below): read
  // where it is used, under `if (mask)`, it was a load behind a run-time branch followed by s_waitcnt vmcnt(0) -- an exposed L2
  // round trip between the softmax and the context, with the context's first chunks held up behind it
  const float* mkp = p.mask ? p.mask + (size_t)n * p.ldmask : p.w_alpha;
  const float mkv = mkp[c.lane < R ? c.lane : 0];
  uint4 pa[2][CR], va[2][CR];
#pragma unroll
  for (int u = 0; u < CR; ++u) pa[0][u] = pre[u];
  load_chunk(P, 1, pa[1]);
  load_chunk(V, 0, va[0]);
  float ah[8], w[8];
  ah[0] = __uint_as_float(h0.x); ah[1] = __uint_as_float(h0.y); ah[2] = __uint_as_float(h0.z); ah[3] = __uint_as_float(h0.w);
  ah[4] = __uint_as_float(h1.x); ah[5] = __uint_as_float(h1.y); ah[6] = __uint_as_float(h1.z); ah[7] = __uint_as_float(h1.w);
  {
    const float4 w0 = *(const float4*)(p.w_alpha + c.lane * 8), w1 = *(const float4*)(p.w_alpha + c.lane * 8 + 4);
    w[0] = w0.x; w[1] = w0.y; w[2] = w0.z; w[3] = w0.w; w[4] = w1.x; w[5] = w1.y; w[6] = w1.z; w[7] = w1.w;
  }
  const float b_alpha = p.b_alpha ? p.b_alpha[0] : 0.f;
  // Round 6: w tanh(p + h) = w - 2 w rc,  rc = 1 / (1 + e^{2p} e^{2h}).  e^{2p} comes from memory (uic_exp2x2_launch, once per
  // training step), e^{2h} is eight v_exp per lane and step, and TWO regions share one reciprocal: rc_0 = x_1 / (x_0 x_1),
  // rc_1 = x_0 / (x_0 x_1) -- per element 0.5 v_rcp and three packed / plain VALU instructions where the direct form spent
  // v_exp + v_rcp + four (the phase is one row's arithmetic on one SIMD: 288 elements per lane).  Both factors are clamped to
  // 2^+-60 where they are made, so x <= 2^120 + 1 is finite; a product beyond f32 gives rc = 0 for both, which is what
  // tanh = 1 means (the partner's own x would have to be < 2^8 against 2^120 for that to matter).
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  f32x2 eh[8], wm2[8];
  float wsum = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float e = __builtin_amdgcn_exp2f(fminf(fmaxf(ah[j] * 2.8853900817779268f, -UIC_E2_CLAMP), UIC_E2_CLAMP));
    eh[j] = (f32x2){e, e};
    wm2[j] = (f32x2){-2.f * w[j], -2.f * w[j]};
    wsum += w[j];
  }
  const f32x2 one2 = {1.f, 1.f};
  static_assert(CR % 2 == 0, "regions are taken in pairs");
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
    for (int u = 0; u < CR; u += 2) {
      const int rr = ch * CR + u;
      float f0[8], f1[8];
      uic_unpack<T>(pa[ch & 1][u], f0);
      uic_unpack<T>(pa[ch & 1][u + 1], f1);
      f32x2 part = {wsum, wsum};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const f32x2 x = __builtin_elementwise_fma((f32x2){f0[j], f1[j]}, eh[j], one2);
        const float inv = __builtin_amdgcn_rcpf(x.x * x.y);
        part = __builtin_elementwise_fma(wm2[j], (f32x2){inv, inv} * x.yx, part);
      }
      const float p0 = uic_row16_sum(part.x), p1 = uic_row16_sum(part.y);
      if (c.l15 == 0 && rr < R) s_e[rr * 4 + c.lq] = p0;
      if (c.l15 == 0 && rr + 1 < R) s_e[(rr + 1) * 4 + c.lq] = p1;
    }
    if (ch + 2 < NCH) load_chunk(P, ch + 2, pa[ch & 1]);
    // (no four-buffer form with att' chunks 2 / 3 in the score buffers: it takes the last free registers, then any foreign wave blocks residency)
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's LDS writes are done (LDS serves a wave's requests in order)
  float e = -INFINITY;
  if (c.lane < R) {
    const float4 qq = *(const float4*)(s_e + c.lane * 4);
    e = (qq.x + qq.y) + (qq.z + qq.w) + b_alpha;
  }
  const float mx = uic_wave_max(e);
  const float ex = c.lane < R ? __builtin_amdgcn_exp2f((e - mx) * 1.4426950408889634f) : 0.f;
  float wgt = ex * __builtin_amdgcn_rcpf(uic_wave_sum(ex));
  if (p.mask) {                                       // (wave-uniform; the value has been here since the top of the phase)
    wgt *= c.lane < R ? mkv : 0.f;
    wgt = wgt / uic_wave_sum(wgt);
  }
  if (c.lane < R) alpha[(unsigned)(n * R + c.lane)] = wgt;
  load_chunk(V, 1, va[1]);
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
#pragma unroll
    for (int u = 0; u < CR; ++u) {
      const int rr = ch * CR + u;
      float al = __shfl(wgt, rr < ATT_R ? (rr < 64 ? rr : 0) : 0, 64);
      if (rr >= R) al = 0.f;
      float f[8];
      uic_unpack<T>(va[ch & 1][u], f);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(al, f[j], acc[j]);   // (explicit: the SAFE and the XCD-local instantiation must round alike)
    }
    if (ch + 2 < NCH) load_chunk(V, ch + 2, va[ch & 1]);
  }
  T* o = ctx + (unsigned)(n * HH + c.lane * 8);
  if (!SAFE) {
    *(uint4*)o = uic_pack<T>(acc);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) st_x<SAFE>(o + j, acc[j]);
  }
}

}  // namespace
