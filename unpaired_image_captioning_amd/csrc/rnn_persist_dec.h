// Decode mode of the weight-stationary kernel (rnn_persist_ws.hip): the three pieces of a decode step that the teacher-forced
// loop does not have.
#pragma once
#include "rnn_persist_internal.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// Decode mode of the weight-stationary kernel (AttModel._sample, P/models/AttModel.py:198-253: greedy or multinomial, the
// sampling pass and the greedy baseline of the self-critical step, P/trainer.py:167-171): a step's input token exists only
// once the previous step has picked it, so three more pieces run inside the launch, all per row group:
//   dec_xt_gemm   the token's share of att_lstm's gates, dropout(relu(embed[token])) W_x^T, for the rows whose cell update
//                 this wave finishes -- A fragments built straight from the f32 embedding table, the result stays in the
//                 registers the cell update reads (the teacher-forced kernel gets it from the batched input GEMM);
//   dec_logits    logits of the group's rows for this workgroup's 1/32 of the vocabulary (W_logit streamed from L2 / the
//                 Infinity Cache, A = the rows' dropped h_lang), written out, plus per-row (max, sum exp, arg max) partials;
//   dec_sample    after a group barrier: every workgroup combines the 32 partials of every row (same order everywhere, so
//                 all agree); greedy: the arg max; multinomial: the workgroup whose vocabulary range holds the inverse-CDF
//                 target scans its <= 320 logits of that row.  The row's writer stores token, log-prob and finished flag.
// Three more group barriers per step than the teacher-forced loop.

template <bool SAFE> __device__ __forceinline__ void st_xi(int* p, int v) {
  if (SAFE) __hip_atomic_store(p, v, RLX_AGENT);
  else *p = v;
}
__device__ __forceinline__ int ld_xi(const int* p) { return __hip_atomic_load(p, RLX_AGENT); }       // (past the vector L1)
__device__ __forceinline__ float ld_xf(const float* p) { return __hip_atomic_load(p, RLX_AGENT); }

// (m, s, a) <- the combination of two partial (max, sum of exp(x - max), arg max) triples; `o` lies at HIGHER column indices
__device__ __forceinline__ void dec_merge(float& m, float& s, int& a, float om, float os, int oa) {
  const float m2 = fmaxf(m, om);
  const float e1 = m > -INFINITY ? __expf(m - m2) : 0.f, e2 = om > -INFINITY ? __expf(om - m2) : 0.f;
  s = s * e1 + os * e2;
  if (om > m || (om == m && oa < a)) a = oa;
  m = m2;
}

// xg[r][g] / xg5[g]: the input token's share of att_lstm's gate pre-activations of step `t`, in the layout ws_cell reads
// (own tile: rows 16 wave + 4 lq + r; fifth tile: row 64 + 4 lq + wave), unit u0 + l15, gate g.
// K is split over the waves (wave w: k-steps 4w .. 4w+3 of EVERY row tile), so a lane requests its 16 W_x fragments and its
// <= 20 embedding-row fragments all at once -- the table (relu(embed) in bf16, 10 MB, random rows) comes from the Infinity
// Cache, W_x from L2,
// one round trip each -- and the partial tiles are summed through LDS, one row tile per pass (as lang_lstm does).
__device__ __forceinline__ void dec_xt_gemm(const UicRnnFwdParams& p, const Ctx& c, int t, float (&xg)[4][4], float (&xg5)[4], const int* tok_lds = nullptr) {
  const float dp = p.dec_xt_drop, inv_keep = dp > 0.f ? 1.f / (1.f - dp) : 1.f;
  const __amdgpu_buffer_rsrc_t r_xw = rsrc_of(p.dec_xw);
  u32x4 fb[4][4];                                  // [k-step of this wave][gate]
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      fb[k][g] = bload<false>(r_xw, (unsigned)(((g * HH + c.u0 + c.l15) * p.dec_ld_xw + c.lq * 8) * 2), (unsigned)((4 * c.wave + k) * 64));
  // (tok_lds: the group's tokens as dec_sample left them in LDS -- greedy / forced, where every workgroup knows them all)
  int tok[MT_MAX], rowi[MT_MAX];
#pragma unroll
  for (int i = 0; i < MT_MAX; ++i) {
    int r = 16 * i + c.l15;
    r = r < c.nrow ? r : c.nrow - 1;
    rowi[i] = r;
    int tk = i < c.MT ? (tok_lds ? tok_lds[r] : ld_xi(p.dec_tok + c.rbegin + r)) : 0;
    tok[i] = tk < 0 || tk >= p.dec_V1 ? 0 : tk;
  }
  if (tok_lds) __syncthreads();                    // (the token list lives in the scratch the partial tiles go to: every wave has read it)
  const unsigned ko = (unsigned)(c.wave * 128 + c.lq * 8);          // first K element of this lane's fragments
  // every fragment of the lane (<= 20 x 16 bytes of relu(embed) in bf16, made once per launch by the host side) in flight at once
  u32x4 fa[MT_MAX][4];
  const bf16_t* er = (const bf16_t*)p.dec_embed_relu;
#pragma unroll
  for (int i = 0; i < MT_MAX; ++i)
    if (i < c.MT) {
#pragma unroll
      for (int k = 0; k < 4; ++k) fa[i][k] = *(const u32x4*)(er + (size_t)tok[i] * HH + ko + k * 32);
    }
  bf16_t* xo = (bf16_t*)p.dec_xt_all;
  if (dp > 0.f || xo) {
#pragma unroll
    for (int i = 0; i < MT_MAX; ++i)
      if (i < c.MT) {
        // dropout index of element e of row n at step t: (t N + n) E + e, the index uic_embed_fwd_launch uses for the training layout
        const unsigned idx = (unsigned)(((size_t)t * p.N + c.rbegin + rowi[i]) * HH) + ko;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (dp > 0.f) {
            float f[8];
            uic_unpack<bf16_t>(__builtin_bit_cast(uint4, fa[i][k]), f);
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] *= uic_drop_scale(p.seed, UIC_SITE_EMBED, idx + (unsigned)(k * 32 + j), dp, inv_keep);
            fa[i][k] = u32x4{uic_pack_bf16x2(f[0], f[1]), uic_pack_bf16x2(f[2], f[3]), uic_pack_bf16x2(f[4], f[5]), uic_pack_bf16x2(f[6], f[7])};
          }
          // the embedded inputs, for a backward pass: workgroup `rank` writes k-step `rank` (of the 16) of every row
          if (xo && c.rank == 4 * c.wave + k && 16 * i + c.l15 < c.nrow)
            *(u32x4*)(xo + ((size_t)t * p.N + c.rbegin + rowi[i]) * HH + ko + k * 32) = fa[i][k];
        }
      }
  }
  f32x4* scr = (f32x4*)c.smem;                     // two 16 KB halves, as in the lang_lstm phase
#pragma unroll
  for (int i = 0; i < MT_MAX; ++i)
    if (i < c.MT) {
      f32x4 acc[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = Mma<bf16_t>::run(fa[i][k], fb[k][g], acc[g]);
      f32x4* half = scr + (i & 1) * (WS_NW * 4 * 64);
#pragma unroll
      for (int g = 0; g < 4; ++g) half[(c.wave * 4 + g) * 64 + c.lane] = acc[g];
      __syncthreads();
      if (i < WS_NW) {
        if (c.wave == i) {                         // the tile's owner: all four accumulator components of its lanes
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            f32x4 v = half[(0 * 4 + g) * 64 + c.lane];
#pragma unroll
            for (int w = 1; w < WS_NW; ++w) v += half[(w * 4 + g) * 64 + c.lane];
#pragma unroll
            for (int r = 0; r < 4; ++r) xg[r][g] = v[r];
          }
        }
      } else {                                     // the fifth tile: wave w finishes row 4 lq + w
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float v = 0.f;
#pragma unroll
          for (int w = 0; w < WS_NW; ++w) v += ((const float*)(half + (w * 4 + g) * 64 + c.lane))[c.wave];
          xg5[g] = v;
        }
      }
    }
  __syncthreads();                                 // (the scratch is the barrier flag's home, and the next pass's)
}

// LDS layout of the decode tail inside the 32 KB scratch (word 0 is the barrier flag)
constexpr int DEC_OFF_PM = 256, DEC_OFF_PS = DEC_OFF_PM + WS_NW * 80 * 4, DEC_OFF_PA = DEC_OFF_PS + WS_NW * 80 * 4;
constexpr int DEC_OFF_CNT = DEC_OFF_PA + WS_NW * 80 * 4, DEC_OFF_LIST = DEC_OFF_CNT + 16;   // list: 80 x {row, rt, M, lse}

// The group's dropped h_lang rows (80 x 512 bf16 = 80 KB) are every wave's A operand: they are staged ONCE per step into LDS
// as MFMA fragments, over the first 80 KB of att_lstm's weight image (k-steps 0..19), which is reloaded from L2 afterwards --
// the weights of W_logit, the operand that comes from the Infinity Cache, can then be requested DEC_LD k-steps ahead.
constexpr int DEC_LD = 3;
// arrived: the caller has ARRIVED at the group barrier behind lang_lstm but not waited yet -- W_logit's first fragments are
// requested before the wait (they do not depend on the exchange).  Returns false after a barrier timeout.
template <bool SAFE>
__device__ __forceinline__ bool dec_logits(const UicRnnFwdParams& p, Ctx& c, int t, char* lds) {
  const int V1 = p.dec_V1;
  const int ntile_all = (V1 + 15) >> 4, per = (ntile_all + PW - 1) / PW;
  const int tile0 = c.rank * per;
  const int ntile = min(per, max(0, ntile_all - tile0));
  const bf16_t* hd = (const bf16_t*)p.hdrop_all + ((size_t)t * p.N + c.rbegin) * HH;
  const __amdgpu_buffer_rsrc_t r_a = rsrc_of(hd), r_w = rsrc_of(p.dec_logit_w);
  u32x4* la = (u32x4*)lds;                         // [k-step 16][row tile 5][lane 64]
  unsigned woff[DEC_NJ];
  int col0[DEC_NJ];                                // first column of the wave's tile j (>= V1: no tile)
#pragma unroll
  for (int j = 0; j < DEC_NJ; ++j) {
    const bool tv = c.wave + WS_NW * j < ntile;
    col0[j] = tv ? 16 * (tile0 + c.wave + WS_NW * j) : V1;
    const int wr = col0[j] + c.l15 < V1 ? col0[j] + c.l15 : V1 - 1;
    woff[j] = (unsigned)((wr * HH + c.lq * 8) * 2);
  }
  u32x4 fb[DEC_LD][DEC_NJ];
  auto loadb = [&](int buf, int ks) {
#pragma unroll
    for (int j = 0; j < DEC_NJ; ++j) fb[buf][j] = bload<false>(r_w, woff[j], (unsigned)(ks * 64));
  };
  const int ks0 = c.rank & 15;                     // de-phased walk over K, as in the recurrence's GEMMs
#pragma unroll
  for (int q = 0; q < DEC_LD - 1; ++q) loadb(q, (q + ks0) & 15);
  if (!group_wait(c, (int*)c.smem)) return false;
  if (c.dbg && c.tid == 0) c.dbg[15] = __builtin_amdgcn_s_memrealtime();
  {
    // fragment f = ks * 5 + i is staged by wave f & 3: 20 loads per lane, all in flight
    u32x4 st[20];
#pragma unroll
    for (int q = 0; q < 20; ++q) {
      const int f = c.wave + 4 * q, ks = f / MT_MAX, i = f - ks * MT_MAX;
      int r = 16 * i + c.l15;
      r = r < c.nrow ? r : c.nrow - 1;
      st[q] = bload<true>(r_a, (unsigned)((r * HH + c.lq * 8) * 2), (unsigned)(ks * 64));
    }
#pragma unroll
    for (int q = 0; q < 20; ++q) la[(c.wave + 4 * q) * 64 + c.lane] = st[q];
  }
  float4 bias[DEC_NJ];
#pragma unroll
  for (int j = 0; j < DEC_NJ; ++j) {
    const int cb = col0[j] + 4 * c.lq;
    bias[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.dec_logit_b && cb < V1) {
      if (cb + 3 < V1) bias[j] = *(const float4*)(p.dec_logit_b + cb);
      else { bias[j].x = p.dec_logit_b[cb]; bias[j].y = cb + 1 < V1 ? p.dec_logit_b[cb + 1] : 0.f; bias[j].z = cb + 2 < V1 ? p.dec_logit_b[cb + 2] : 0.f; }
    }
  }
  f32x4 acc[MT_MAX][DEC_NJ];
#pragma unroll
  for (int i = 0; i < MT_MAX; ++i)
#pragma unroll
    for (int j = 0; j < DEC_NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();                                 // the A image is complete
  if (c.dbg && c.tid == 0) c.dbg[11] = __builtin_amdgcn_s_memrealtime();
  // W_logit's fragment is the MFMA's FIRST operand: the lane then holds 4 consecutive vocabulary columns (4 lq + r) of ONE
  // caption row (l15) per tile -- one 16-byte store per tile, and a row's maximum / sum are mostly in-lane
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int ks = (q + ks0) & 15;
    if (q + DEC_LD - 1 < 16) loadb((q + DEC_LD - 1) % DEC_LD, (q + DEC_LD - 1 + ks0) & 15);
    u32x4 fa[MT_MAX];
#pragma unroll
    for (int i = 0; i < MT_MAX; ++i)
      if (i < c.MT) fa[i] = la[(ks * MT_MAX + i) * 64 + c.lane];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < MT_MAX; ++i)
      if (i < c.MT) {
#pragma unroll
        for (int j = 0; j < DEC_NJ; ++j) acc[i][j] = Mma<bf16_t>::run(fb[q % DEC_LD][j], fa[i], acc[i][j]);
      }
    __builtin_amdgcn_sched_barrier(0);
  }
  if (c.dbg && c.tid == 0) c.dbg[12] = __builtin_amdgcn_s_memrealtime();
  // bias, store, per-row partials
  const bool store = p.dec_logits_step != 0 || !p.dec_sample_max;     // kept for a backward pass, or read back by the draw
  float* lg = p.dec_logits + (size_t)t * p.dec_logits_step;
  float* pm = (float*)(c.smem + DEC_OFF_PM);
  float* ps = (float*)(c.smem + DEC_OFF_PS);
  int* pa = (int*)(c.smem + DEC_OFF_PA);
#pragma unroll
  for (int i = 0; i < MT_MAX; ++i)
    if (i < c.MT) {
      const int row = 16 * i + c.l15;
      const bool rv = row < c.nrow;
      float m = -INFINITY;
      int a = 0x7fffffff;
      float v[DEC_NJ][4];
#pragma unroll
      for (int j = 0; j < DEC_NJ; ++j) {
        const int cb = col0[j] + 4 * c.lq;
        v[j][0] = acc[i][j][0] + bias[j].x; v[j][1] = acc[i][j][1] + bias[j].y;
        v[j][2] = acc[i][j][2] + bias[j].z; v[j][3] = acc[i][j][3] + bias[j].w;
        if (store && rv && cb < V1) {
          float* o = lg + (size_t)(c.rbegin + row) * p.dec_V1p + cb;
          if (!SAFE && cb + 3 < V1) *(float4*)o = make_float4(v[j][0], v[j][1], v[j][2], v[j][3]);
          else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (cb + r < V1) st_x<SAFE>(o + r, v[j][r]);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (cb + r >= V1) v[j][r] = -INFINITY;
          if (v[j][r] > m) { m = v[j][r]; a = cb + r; }           // (columns ascend with j and r inside a lane)
        }
      }
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < DEC_NJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) sum += v[j][r] > -INFINITY ? __expf(v[j][r] - m) : 0.f;
      // the other three column quarters of the same tiles live in lanes l15 + 16, + 32, + 48
#pragma unroll
      for (int o = 16; o < 64; o <<= 1) {
        const float om = __shfl_xor(m, o, 64), os = __shfl_xor(sum, o, 64);
        const int oa = __shfl_xor(a, o, 64);
        dec_merge(m, sum, a, om, os, oa);
      }
      if (c.lq == 0 && rv) { pm[c.wave * 80 + row] = m; ps[c.wave * 80 + row] = sum; pa[c.wave * 80 + row] = a; }
    }
  if (c.dbg && c.tid == 0) c.dbg[14] = __builtin_amdgcn_s_memrealtime();
  __syncthreads();                                 // partials in LDS; every wave is through with the A image
  if (c.tid < c.nrow) {
    const int row = c.tid;
    float m = pm[row], sum = ps[row];
    int a = pa[row];
#pragma unroll
    for (int w = 1; w < WS_NW; ++w) dec_merge(m, sum, a, pm[w * 80 + row], ps[w * 80 + row], pa[w * 80 + row]);
    float* o = p.dec_part + ((size_t)(c.rbegin + row) * PW + c.rank) * 4;
    st_x<SAFE>(o, m); st_x<SAFE>(o + 1, sum); st_x<SAFE>(o + 2, __int_as_float(a));
  }
  return true;
}

template <bool SAFE>
__device__ __forceinline__ void dec_sample(const UicRnnFwdParams& p, const Ctx& c, int t, char* lds) {
  const int V1 = p.dec_V1;
  const int ntile_all = (V1 + 15) >> 4, per = (ntile_all + PW - 1) / PW;
  int* s_cnt = (int*)(c.smem + DEC_OFF_CNT);
  float* s_list = (float*)(c.smem + DEC_OFF_LIST);
  const float* lg = p.dec_logits + (size_t)t * p.dec_logits_step;
  if (c.tid == 0) *s_cnt = 0;
  __syncthreads();
  // att_lstm's weight fragments of k-steps 0..19 go back into the LDS image dec_logits borrowed (from L2): by the two waves
  // that have no row to combine below (a group has at most 80 rows = threads 0..79), beside the two that do
  if (c.wave >= 2) {
    const unsigned bl = (unsigned)(c.lq * 8);
    const __amdgpu_buffer_rsrc_t r_a_ih = rsrc_of(p.att_w_ih), r_a_hh = rsrc_of(p.att_w_hh);
    u32x4 v[40];                                   // all in flight: one L2 round trip
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int vw = c.wave - 2 * half;            // the wave whose share of the image this is
#pragma unroll
      for (int jj = 0; jj < 5; ++jj) {
        const unsigned kk = (unsigned)(((vw + 4 * jj) & 15) * 32);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const unsigned row = (unsigned)(g * HH + c.u0 + c.l15);
          v[half * 20 + jj * 4 + g] = jj < 4 ? bload<false>(r_a_ih, (row * (unsigned)p.ld_att_ih + kk + bl) * 2u, 0)
                                             : bload<false>(r_a_hh, (row * (unsigned)HH + kk + bl) * 2u, 0);
        }
      }
    }
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int jj = 0; jj < 5; ++jj)
#pragma unroll
        for (int g = 0; g < 4; ++g) ((u32x4*)lds)[((c.wave - 2 * half + 4 * jj) * 4 + g) * 64 + c.lane] = v[half * 20 + jj * 4 + g];
  }
  auto finish = [&](int n, int choice, float lp) {   // the row's writer (AttModel.py:240-249)
    int unf = choice > 0;
    if (t > p.t0) unf = unf && ld_xi(p.dec_unf + n) != 0;
    const int tok = unf ? choice : 0;
    st_xi<SAFE>(p.dec_unf + n, unf);
    st_xi<SAFE>(p.dec_tok + n, tok);
    p.dec_seq[(size_t)n * p.dec_ld_out + t] = tok;
    p.dec_seq_logp[(size_t)n * p.dec_ld_out + t] = lp;
  };
  if (c.tid < c.nrow) {
    const int row = c.tid, n = c.rbegin + row;
    const __amdgpu_buffer_rsrc_t r_p = rsrc_of(p.dec_part);       // (one descriptor for the wave: the row is the lane offset)
    const unsigned poff = (unsigned)n * (unsigned)(PW * 16);
    float M = -INFINITY;
    int best = 0;
    u32x4 q[PW];
#pragma unroll
    for (int w = 0; w < PW; ++w) q[w] = bload<true>(r_p, poff, (unsigned)(w * 16));
#pragma unroll
    for (int w = 0; w < PW; ++w) {
      const float mw = __uint_as_float(q[w].x);
      if (mw > M) { M = mw; best = (int)q[w].z; }       // ranks own increasing column ranges: the first maximum is the lowest index
    }
    float Z = 0.f;
#pragma unroll
    for (int w = 0; w < PW; ++w) {
      const float mw = __uint_as_float(q[w].x);
      Z += mw > -INFINITY ? __uint_as_float(q[w].y) * __expf(mw - M) : 0.f;
    }
    const float lse = M + __logf(Z);
    const bool writer = (row & (PW - 1)) == c.rank;
    if (p.dec_sample_max || p.dec_forced) {
      // every workgroup knows the choice of every row of the group: the next step's tokens go to LDS (no exchange, no barrier)
      int ch = best;
      if (!p.dec_sample_max) {
        ch = (int)p.dec_forced[(size_t)n * p.dec_ld_forced + t];
        ch = ch < 0 || ch >= V1 ? 0 : ch;
      }
      int unf = ch > 0;
      if (t > p.t0) unf = unf && ld_xi(p.dec_unf + n) != 0;       // (written by the row's writer one step -- several barriers -- ago)
      ((int*)s_list)[row] = unf ? ch : 0;
      if (writer) finish(n, ch, p.dec_sample_max ? M - lse : ld_xf(lg + (size_t)n * p.dec_V1p + ch) - lse);
    } else {
      // inverse-CDF target in units of exp(. - M); the owner is the first workgroup whose cumulative mass exceeds it
      unsigned x = (unsigned)n * 0x9E3779B1u ^ (p.dec_draw_seed + (unsigned)t * 0x85EBCA77u);
      x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
      const float target = (float)(x >> 8) * (1.0f / 16777216.0f) * Z;
      float cum = 0.f, rt = INFINITY;
      int owner = -1, lastmass = 0;
#pragma unroll
      for (int w = 0; w < PW; ++w) {
        const float mw = __uint_as_float(q[w].x);
        const float sw = mw > -INFINITY ? __uint_as_float(q[w].y) * __expf(mw - M) : 0.f;
        if (sw > 0.f) lastmass = w;
        if (owner < 0) {
          if (cum + sw > target) { owner = w; rt = target - cum; }
          else cum += sw;
        }
      }
      if (owner < 0) owner = lastmass;                // rounding left the target at or beyond the total mass: the last token with mass
      if (owner == c.rank) {
        const int k = atomicAdd(s_cnt, 1);
        s_list[4 * k] = __int_as_float(row); s_list[4 * k + 1] = rt; s_list[4 * k + 2] = M; s_list[4 * k + 3] = lse;
      }
    }
  }
  if (p.dec_sample_max || p.dec_forced) return;
  __syncthreads();
  const int cnt = *s_cnt;
  const int c_lo = 16 * c.rank * per, c_hi = min(V1, c_lo + 16 * per);
  for (int k = c.wave; k < cnt; k += WS_NW) {          // one wave per owned row: its <= 320 logits, 64 per round
    const int row = __float_as_int(s_list[4 * k]), n = c.rbegin + row;
    const float rt = s_list[4 * k + 1], M = s_list[4 * k + 2], lse = s_list[4 * k + 3];
    const float* lr = lg + (size_t)n * p.dec_V1p;
    float lv[DEC_NJ];
#pragma unroll
    for (int j = 0; j < DEC_NJ; ++j) {
      const int v = c_lo + 64 * j + c.lane;
      lv[j] = v < c_hi ? ld_xf(lr + v) : -INFINITY;
    }
    float cum = 0.f, lp = 0.f;
    int pick = -1, last = -1;
    float lastl = 0.f;
#pragma unroll
    for (int j = 0; j < DEC_NJ; ++j) {
      const float e = lv[j] > -INFINITY ? __expf(lv[j] - M) : 0.f;
      float incl = e;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const float up = __shfl_up(incl, o, 64);
        if (c.lane >= o) incl += up;
      }
      const unsigned long long hit = __ballot(pick < 0 && cum + incl > rt && e > 0.f);
      const unsigned long long mass = __ballot(e > 0.f);
      if (mass) {
        const int hl = 63 - __clzll((long long)mass);
        last = c_lo + 64 * j + hl;
        lastl = __shfl(lv[j], hl, 64);
      }
      if (hit && pick < 0) {
        const int fl = __ffsll((long long)hit) - 1;
        pick = c_lo + 64 * j + fl;
        lp = __shfl(lv[j], fl, 64) - lse;
      }
      cum += __shfl(incl, 63, 64);
    }
    if (pick < 0) { pick = last < 0 ? 0 : last; lp = (last < 0 ? ld_xf(lr) : lastl) - lse; }
    if (c.lane == 0) finish(n, pick, lp);
  }
}

}  // namespace
