// The weight-stationary bf16 kernels of the persistent recurrence (rnn_persist.hip's header comment: decomposition, visibility):
// the teacher-forced training loop and the decode loop, two instantiations of ws_run in one translation unit.
#include "rnn_persist_internal.h"
#include "rnn_persist_attn.h"
#include "rnn_persist_dec.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// Weight-stationary bf16 variant.  A workgroup's slice of the recurrent weights is 336 KB in bf16 (64 gate columns of
// att_lstm x K 1024, 64 of lang_lstm x K 1536, 16 columns of h2att x K 512): streamed from the Infinity Cache every step
// it is 10.7 MB per XCD and step, as much as the activations.  Here the two LSTM slices are loaded ONCE per launch by a
// workgroup of FOUR waves with the whole 512-entry register file of their SIMD each:
//   * att_lstm's slice (128 KB) lives in LDS as MFMA B fragments [k-step][gate][lane][16 B]; wave w owns the 16-row tile w
//     of the group and walks all 32 k-steps itself, so the four gate accumulators of a (row, unit) end up in one lane and
//     the cell update needs no cross-wave reduction (the fifth tile of an 80-row group is split over the waves by K and
//     summed through LDS);
//   * lang_lstm's slice (192 KB) lives in REGISTERS, K split over the 4 waves (wave w holds k-steps w, w+4, ...: 48
//     fragments = 192 registers, MFMA operands only); the partial tiles are summed through two 16 KB LDS buffers, one
//     row tile per pass and one workgroup barrier per pass;
//   * h2att's slice (16 KB) is re-read every step beside the activations (4 MB per step chip-wide).
// The c state of both cells stays in the registers of the lanes that update it.
constexpr int WS_NTH = WS_NW * 64;
constexpr int WS_W1_BYTES = 32 * 4 * 1024;
constexpr int WS_SCR_BYTES = 32 * 1024;
constexpr int WS_LDS_BYTES = WS_W1_BYTES + WS_SCR_BYTES;

// nn.LSTMCell's pointwise part for the 4 rows x 1 unit a lane holds in the D layout of four gate accumulators
template <bool SAFE>
__device__ __forceinline__ void ws_cell(const Ctx& c, int tile, const f32x4 (&s)[4], const float (&pv)[4][4], float (&cst)[4],
                                        float* c_out, bf16_t* h_out, bf16_t* gates_out) {
  const unsigned u = (unsigned)(c.u0 + c.l15);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int rr = 16 * tile + 4 * c.lq + r;
    const float gi = uic_sigmoid_t<bf16_t>(s[0][r] + pv[r][0]);
    const float gf = uic_sigmoid_t<bf16_t>(s[1][r] + pv[r][1]);
    const float gg = uic_tanh<bf16_t>(s[2][r] + pv[r][2]);
    const float go = uic_sigmoid_t<bf16_t>(s[3][r] + pv[r][3]);
    const float cn = gf * cst[r] + gi * gg;
    const float h = go * uic_tanh<bf16_t>(cn);
    cst[r] = cn;
    if (rr < c.nrow) {
      const unsigned nn = (unsigned)((c.rbegin + rr) * HH);
      const unsigned o = nn + u;
      c_out[o] = cn;
      st_x<SAFE>(h_out + o, h);
      if (gates_out) {
        const unsigned og = 4u * nn + u;
        __builtin_nontemporal_store((bf16_t)gi, gates_out + og);
        __builtin_nontemporal_store((bf16_t)gf, gates_out + og + HH);
        __builtin_nontemporal_store((bf16_t)gg, gates_out + og + 2 * HH);
        __builtin_nontemporal_store((bf16_t)go, gates_out + og + 3 * HH);
      }
    }
  }
}

// att_lstm's B fragments of k-steps wave + 4 jj, jj in [jj0, jj1), into the LDS image (the launch's one-time load, and the
// reload of the part dec_logits borrows)
// (vwave: the wave whose share of the image this wave loads -- normally its own)
__device__ __forceinline__ void ws_load_w1(const UicRnnFwdParams& p, const Ctx& c, char* lds, int jj0, int jj1, int vwave) {
  const unsigned bl = (unsigned)(c.lq * 8);
  const __amdgpu_buffer_rsrc_t r_a_ih = rsrc_of(p.att_w_ih), r_a_hh = rsrc_of(p.att_w_hh);
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) {
    if (jj < jj0 || jj >= jj1) continue;
    const int s = vwave + 4 * jj;                 // k-step of [h_lang_prev | h_att_prev]
    const unsigned kk = (unsigned)((s & 15) * 32);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const unsigned row = (unsigned)(g * HH + c.u0 + c.l15);
      const u32x4 v = jj < 4 ? bload<false>(r_a_ih, (row * (unsigned)p.ld_att_ih + kk + bl) * 2u, 0)
                             : bload<false>(r_a_hh, (row * (unsigned)HH + kk + bl) * 2u, 0);
      ((u32x4*)lds)[(s * 4 + g) * 64 + c.lane] = v;
    }
  }
}

// The step loop of both kernels, every phase written in place.  Both kernels sit at the register limit: a phase moved verbatim
// into a function of its own (att_lstm, lang_lstm, lstm1_early, the one-row cell tails, the time stamps) changes the wait / branch /
// register counts of at least one of them, and the two moves that keep those counts (h2att; tile_of / aoff_of as functions) put the
// decode kernel's time outside the parent's own spread (tools/isa_profile.py on every variant; figures in profiles/LOG.md).
template <bool SAFE, bool DEC>
__device__ __forceinline__ void ws_run(const UicRnnFwdParams& p, Ctx& c, char* lds) {
  typedef bf16_t T;
  const int N = p.N;
  const size_t NH = (size_t)N * HH;
  const size_t rb = (size_t)c.rbegin * HH;
  const u32x4* w1 = (const u32x4*)lds;             // [k-step 32][gate 4][lane 64]
  f32x4* scr = (f32x4*)c.smem;                     // 32 KB: two 16 KB halves
  // ---- one-time weight load
  // De-phasing: all 32 workgroups of a group read the SAME activation rows in every GEMM phase.  Walking them in the same
  // order at the same time puts every request of the XCD on the same few L2 channels, so each workgroup starts its walk
  // over K (and over the row tiles) at an offset of its own, `rank`; the stationary fragments are laid out to match.
  const int j0 = __builtin_amdgcn_readfirstlane(c.rank % 12);
  const int tr = __builtin_amdgcn_readfirstlane(c.rank % c.MT);   // the row tiles are walked starting at tile tr
  u32x4 w2[12][4];                                 // slot j: k-step wave + 4 m of [att_res | h_att | h_lang_prev], m as below
  {
    const unsigned bl = (unsigned)(c.lq * 8);
    // (one descriptor for weight_ih and weight_hh of lang_lstm: which of them slot j reads is a select of a 32-bit offset)
    const char* wlo = (const char*)p.lang_w_ih < (const char*)p.lang_w_hh ? (const char*)p.lang_w_ih : (const char*)p.lang_w_hh;
    const __amdgpu_buffer_rsrc_t r_w = __builtin_amdgcn_make_buffer_rsrc((void*)wlo, 0, -1, 0x00020000);
    const unsigned o_ih = (unsigned)((const char*)p.lang_w_ih - wlo), o_hh = (unsigned)((const char*)p.lang_w_hh - wlo);
#pragma unroll
    for (int j = 0; j < 12; ++j) {
      // slots 0-3: h_att, 4-7: h_lang_prev, 8-11: att_res -- the segment that the attention phase produces comes LAST, so that a
      // row tile's first eight fragments can be requested (and multiplied) before the group barrier behind the attention is through;
      // inside a segment the four k-steps are walked from an offset of the workgroup's own (j0)
      const int sg = (j >> 2) == 2 ? 0 : (j >> 2) + 1;   // 0: att_res, 1: h_att, 2: h_lang_prev   (16 k-steps each)
      const int m = sg * 4 + ((j + j0) & 3);
      const unsigned kk = (unsigned)(((m & 3) * 4 + c.wave) * 32);
      const unsigned ld = sg < 2 ? 2u * HH : (unsigned)HH;
      const unsigned so = (sg < 2 ? o_ih + (unsigned)(sg * HH) * 2u : o_hh) + kk * 2u;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const unsigned row = (unsigned)(g * HH + c.u0 + c.l15);
        w2[j][g] = bload<false>(r_w, (row * ld + bl) * 2u, so);
      }
    }
    ws_load_w1(p, c, lds, 0, 8, c.wave);
  }
  // lang_lstm's bias for the unit of this lane (tile owners: wave w owns row tile w, wave 0 also tile 4)
  float pb[4][4];
  {
    const unsigned u = (unsigned)(c.u0 + c.l15);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float b = (p.lang_b_ih ? p.lang_b_ih[g * HH + u] : 0.f) + (p.lang_b_hh ? p.lang_b_hh[g * HH + u] : 0.f);
#pragma unroll
      for (int r = 0; r < 4; ++r) pb[r][g] = b;
    }
  }
  // The recurrence-independent share of att_lstm's gate pre-activations (xt and fc' terms and both biases, one f32 tensor
  // made by the batched input GEMM) and the cell state of step `ts`, for the 4 rows x 1 unit this lane finishes in row tile
  // `tile`.  They come from HBM / the Infinity Cache.
  // The caption row's fc' share (Gfc, when the host keeps it out of gx) is the same at every step: read once, kept in registers.
  float gfo[4][4], gf5[4];
  {
    const unsigned u = (unsigned)(c.u0 + c.l15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = 16 * c.wave + 4 * c.lq + r;
      const unsigned n1 = (unsigned)((c.rbegin + (rr < c.nrow ? rr : c.nrow - 1)) * HH);
#pragma unroll
      for (int g = 0; g < 4; ++g) gfo[r][g] = p.gfc ? p.gfc[4u * n1 + (unsigned)(g * HH) + u] : 0.f;
    }
    const int rr = 16 * WS_NW + 4 * c.lq + c.wave;
    const unsigned n1 = (unsigned)((c.rbegin + (rr < c.nrow ? rr : c.nrow - 1)) * HH);
#pragma unroll
    for (int g = 0; g < 4; ++g) gf5[g] = p.gfc ? p.gfc[4u * n1 + (unsigned)(g * HH) + u] : 0.f;
  }
  // decode mode: the input token's share of att_lstm's gates of the coming step, made by dec_xt_gemm (the teacher-forced loop
  // reads it from gx)
  float xg[4][4], xg5[4];
  if (DEC) dec_xt_gemm(p, c, p.t0, xg, xg5);
  auto load_pre = [&](int ts, int tile, float (&pv)[4][4], float (&cp)[4]) {     // (tile == this wave's own tile)
    const float* gx = p.gx + (size_t)ts * N * 4 * HH;
    const float* c_prev = p.c_att + (size_t)ts * NH;
    const unsigned u = (unsigned)(c.u0 + c.l15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = 16 * tile + 4 * c.lq + r;
      const unsigned n1 = (unsigned)((c.rbegin + (rr < c.nrow ? rr : c.nrow - 1)) * HH);
      cp[r] = c_prev[n1 + u];
#pragma unroll
      for (int g = 0; g < 4; ++g) pv[r][g] = DEC ? xg[r][g] : gx[4u * n1 + (unsigned)(g * HH) + u];
    }
  };
  // fifth tile: its cell update is shared by the four waves, wave w takes row 4 lq + w of every 4-row group
  auto load_pre5 = [&](int ts, float (&pv)[4], float& cp) {
    const float* gx = p.gx + (size_t)ts * N * 4 * HH;
    const unsigned u = (unsigned)(c.u0 + c.l15);
    const int rr = 16 * WS_NW + 4 * c.lq + c.wave;
    const unsigned n1 = (unsigned)((c.rbegin + (rr < c.nrow ? rr : c.nrow - 1)) * HH);
    cp = p.c_att[(size_t)ts * NH + n1 + u];
#pragma unroll
    for (int g = 0; g < 4; ++g) pv[g] = DEC ? xg5[g] : gx[4u * n1 + (unsigned)(g * HH) + u];
  };
  __syncthreads();                                  // the W1 image is complete
  // att_lstm's gate accumulators of this wave's own row tile, and the half of its K that needs no exchange at the step boundary:
  // h_att_prev of step t + 1 is step t's h_att_new, which every workgroup has had since the barrier behind att_lstm -- so its 16
  // k-steps are multiplied between the two halves of the step's LAST group barrier (after this workgroup's arrival, before it
  // looks for the others'), i.e. in time that was idle; what is left behind the barrier is the h_lang_prev half.
  f32x4 acc1[4];
  const __amdgpu_buffer_rsrc_t rx0 = __builtin_amdgcn_make_buffer_rsrc((void*)p.xbase, 0, -1, 0x00020000);
  auto lstm1_early = [&](unsigned o_hap_t) {
#pragma unroll
    for (int g = 0; g < 4; ++g) acc1[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (c.wave < c.MT) {
      int ar = 16 * c.wave + c.l15;
      ar = ar < c.nrow ? ar : c.nrow - 1;
      const unsigned aoff = (unsigned)((ar * HH + c.lq * 8) * 2);
      const int h0 = c.rank & 15;                   // each workgroup starts its walk over the half at an offset of its own
      u32x4 fa[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) fa[q] = bload<true>(rx0, aoff, o_hap_t + (unsigned)(((q + h0) & 15) * 64));
      u32x4 fb[2][4];
#pragma unroll
      for (int g = 0; g < 4; ++g) fb[0][g] = w1[((16 + h0) * 4 + g) * 64 + c.lane];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int sn = 16 + ((q + 1 + h0) & 15);    // (the last prefetch wraps and is unused)
#pragma unroll
        for (int g = 0; g < 4; ++g) fb[(q + 1) & 1][g] = w1[(sn * 4 + g) * 64 + c.lane];
#pragma unroll
        for (int g = 0; g < 4; ++g) acc1[g] = Mma<bf16_t>::run(fa[q], fb[q & 1][g], acc1[g]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  unsigned long long* dbg = p.dbg ? p.dbg + ((size_t)blockIdx.x * p.dbg_T + p.t0) * 16 : nullptr;
  for (int t = p.t0; t < p.t1; ++t) {
    asm volatile("" : "+v"(c.lane), "+v"(c.l15), "+v"(c.lq), "+v"(c.tid));
    asm volatile("" : "+s"(c.wave), "+s"(c.u0), "+s"(c.rbegin), "+s"(c.nrow), "+s"(c.MT));
    T* h_att_prev = (T*)p.h_att + (size_t)t * NH;
    T* h_att_new = h_att_prev + NH;
    T* h_lang_prev = (T*)p.h_lang + (size_t)t * NH;
    T* h_lang_new = h_lang_prev + NH;
    float* att_h = p.att_h_all + (size_t)t * NH;
    T* ctx = (T*)p.ctx_all + (size_t)t * NH;
    c.dbg = dbg;
    // every exchanged slab is addressed through ONE buffer descriptor (base = lowest of their addresses, from the host) plus
    // a 32-bit byte offset: which slab a k-step comes from is then a scalar select of an offset, not of a pointer
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.xbase, 0, -1, 0x00020000);
    const unsigned o_hlp = (unsigned)((const char*)(h_lang_prev + rb) - (const char*)p.xbase);
    const unsigned o_hap = (unsigned)((const char*)(h_att_prev + rb) - (const char*)p.xbase);
    const unsigned o_han = (unsigned)((const char*)(h_att_new + rb) - (const char*)p.xbase);
    const unsigned o_ctx = (unsigned)((const char*)(ctx + rb) - (const char*)p.xbase);
    if (dbg && c.tid == 0) dbg[0] = __builtin_amdgcn_s_memrealtime();
    // ---- att_lstm (:431-434): wave w = row tile w (all 32 k-steps, B fragments from LDS); tile 4: k-steps w, w+4, ...
    // The h_att_prev half of K (k-steps 16..31) has been multiplied already (lstm1_early: at the top of the first step, else
    // inside the previous step's last group barrier); here the h_lang_prev half, which that barrier exchanged.
    if (DEC || t == p.t0) lstm1_early(o_hap);
    {
      // k-step s of [h_lang_prev | h_att_prev]: its slab and its byte offset inside a row
      auto a_soff = [&](int s) { return ((s >> 4) ? o_hap : o_hlp) + (unsigned)((s & 15) * 64); };
      const int s0 = c.rank;                        // (fifth tile: this workgroup walks its k-steps starting at s0)
      float pv5[4], cp5 = 0.f;
      const bool split5 = c.MT > WS_NW;             // an 80-row group: a fifth tile, shared by the waves (then every wave has a tile of its own too)
      if (c.wave < c.MT) {
        const int i = c.wave;
        int ar = 16 * i + c.l15;
        ar = ar < c.nrow ? ar : c.nrow - 1;
        const unsigned aoff = (unsigned)((ar * HH + c.lq * 8) * 2);
        int ar5 = 16 * WS_NW + c.l15;
        ar5 = ar5 < c.nrow ? ar5 : c.nrow - 1;
        const unsigned aoff5 = (unsigned)((ar5 * HH + c.lq * 8) * 2);
        const int h0 = c.rank & 15;                 // de-phased walk over the half, as lstm1_early's
        // the whole half of the tile's activations in flight: the L2 latency is paid once and the MFMAs run as the fragments
        // arrive (loads return in order); then the cell update's own operands
        u32x4 fa[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) fa[q] = bload<true>(rx, aoff, o_hlp + (unsigned)(((q + h0) & 15) * 64));
        float pvn[4][4], cpn[4];
        load_pre(t, i, pvn, cpn);
        // B fragments of k-step q + 1 are read from LDS while the MFMAs of k-step q run (left alone hipcc emits
        // read - wait - MFMA per fragment: an LDS round trip per MFMA, 7 us for the 128 of a tile)
        u32x4 fb[2][4];
#pragma unroll
        for (int g = 0; g < 4; ++g) fb[0][g] = w1[(h0 * 4 + g) * 64 + c.lane];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int sn = (q + 1 + h0) & 15;         // (the last prefetch wraps to k-step h0 and is unused)
#pragma unroll
          for (int g = 0; g < 4; ++g) fb[(q + 1) & 1][g] = w1[(sn * 4 + g) * 64 + c.lane];
#pragma unroll
          for (int g = 0; g < 4; ++g) acc1[g] = Mma<bf16_t>::run(fa[q], fb[q & 1][g], acc1[g]);
          if (q == 7 && (DEC ? split5 : true)) {
            // the registers that have just been consumed take this wave's share of tile 4: k-steps wave, wave + 4, ...
            // (training kernel: requested whether or not the group has a fifth tile -- the row index is clamped --, so that the
            // waits of the remaining k-steps are counted exactly; see the note at mfma_range)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
              const int sr = c.wave + 4 * ((k + s0) & 7);
              fa[k] = bload<true>(rx, aoff5, a_soff(sr));
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        u32x4 (&f5)[16] = fa;
        if (dbg && c.tid == 0) dbg[8] = __builtin_amdgcn_s_memrealtime();
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int g = 0; g < 4; ++g) pvn[r][g] += gfo[r][g];
        ws_cell<SAFE>(c, i, acc1, pvn, cpn, p.c_att + (size_t)(t + 1) * NH, h_att_new,
                      p.gates1 ? (T*)p.gates1 + (size_t)t * N * 4 * HH : nullptr);
        if (dbg && c.tid == 0) dbg[9] = __builtin_amdgcn_s_memrealtime();
        if (split5) {
          f32x4 acc[4];
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int g = 0; g < 4; ++g) fb[0][g] = w1[((c.wave + 4 * (s0 & 7)) * 4 + g) * 64 + c.lane];
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const int sn = c.wave + 4 * ((q + 1 + s0) & 7);
#pragma unroll
            for (int g = 0; g < 4; ++g) fb[(q + 1) & 1][g] = w1[(sn * 4 + g) * 64 + c.lane];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = Mma<bf16_t>::run(f5[q], fb[q & 1][g], acc[g]);
          }
#pragma unroll
          for (int g = 0; g < 4; ++g) scr[(c.wave * 4 + g) * 64 + c.lane] = acc[g];
          load_pre5(t, pv5, cp5);
          __syncthreads();                          // (split5 => MT == 5 => all four waves are here)
          {
            float sg4[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              float v = 0.f;
#pragma unroll
              for (int w = 0; w < WS_NW; ++w) v += ((const float*)(scr + (w * 4 + g) * 64 + c.lane))[c.wave];
              sg4[g] = v;
            }
            const int rr = 16 * WS_NW + 4 * c.lq + c.wave;
            const unsigned u = (unsigned)(c.u0 + c.l15);
            const float gi = uic_sigmoid_t<bf16_t>(sg4[0] + (pv5[0] + gf5[0]));
            const float gf = uic_sigmoid_t<bf16_t>(sg4[1] + (pv5[1] + gf5[1]));
            const float gg = uic_tanh<bf16_t>(sg4[2] + (pv5[2] + gf5[2]));
            const float go = uic_sigmoid_t<bf16_t>(sg4[3] + (pv5[3] + gf5[3]));
            const float cn = gf * cp5 + gi * gg;
            const float h = go * uic_tanh<bf16_t>(cn);
            if (rr < c.nrow) {
              const unsigned nn = (unsigned)((c.rbegin + rr) * HH);
              const unsigned o = nn + u;
              p.c_att[(size_t)(t + 1) * NH + o] = cn;
              st_x<SAFE>(h_att_new + o, h);
              if (p.gates1) {
                T* G = (T*)p.gates1 + (size_t)t * N * 4 * HH + 4u * nn + u;
                __builtin_nontemporal_store((bf16_t)gi, G);
                __builtin_nontemporal_store((bf16_t)gf, G + HH);
                __builtin_nontemporal_store((bf16_t)gg, G + 2 * HH);
                __builtin_nontemporal_store((bf16_t)go, G + 3 * HH);
              }
            }
          }
        }
      }
    }
    if (dbg && c.tid == 0) dbg[1] = __builtin_amdgcn_s_memrealtime();
    if (!group_barrier(c)) return;
    if (dbg && c.tid == 0) dbg[2] = __builtin_amdgcn_s_memrealtime();
    asm volatile("" : "+v"(c.lane), "+v"(c.l15), "+v"(c.lq), "+v"(c.tid));   // keep this phase's lane-derived values out of the others' live ranges
    // ---- h2att (:543): the waves split K, wave w (and wave 0 for tile 4) reduces its row tile
    {
      const __amdgpu_buffer_rsrc_t r_h2 = rsrc_of(p.h2att_w);
      constexpr int P2D = 2;                         // row tiles of activations in flight
      u32x4 wh[4], fa[P2D][4];
      auto tile_of = [&](int i) { const int x = i + tr; return x >= c.MT ? x - c.MT : x; };
      auto load_tile = [&](int buf, int i) {
        int ar = 16 * tile_of(i) + c.l15;
        ar = ar < c.nrow ? ar : c.nrow - 1;
        const unsigned aoff = (unsigned)((ar * HH + c.lq * 8) * 2);
#pragma unroll
        for (int j = 0; j < 4; ++j) fa[buf][j] = bload<true>(rx, aoff, o_han + (unsigned)((c.wave + 4 * ((j + c.rank) & 3)) * 64));
      };
#pragma unroll
      for (int j = 0; j < 4; ++j)
        wh[j] = bload<false>(r_h2, (unsigned)(((c.u0 + c.l15) * HH + c.lq * 8) * 2), (unsigned)((c.wave + 4 * ((j + c.rank) & 3)) * 64));
      // (requests without run-time conditions -- a tile the group does not have is its last real tile again -- and an early exit
      // instead of skipped blocks: the waits in front of every tile's MFMAs are then counted exactly; see the note at mfma_range)
      auto clamp_tile = [&](int i) { return i < c.MT ? i : c.MT - 1; };
#pragma unroll
      for (int i = 0; i < P2D - 1; ++i) load_tile(i, clamp_tile(i));
#pragma unroll
      for (int i = 0; i < MT_MAX; ++i) {
        if (i >= c.MT) break;
        {
          if (i + P2D - 1 < MT_MAX) load_tile((i + P2D - 1) % P2D, DEC ? (i + P2D - 1 < c.MT ? i + P2D - 1 : i) : clamp_tile(i + P2D - 1));
          __builtin_amdgcn_sched_barrier(0);
          f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int j = 0; j < 4; ++j) a = Mma<bf16_t>::run(fa[i % P2D][j], wh[j], a);
          scr[(c.wave * MT_MAX + tile_of(i)) * 64 + c.lane] = a;
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      __syncthreads();
      const int a = c.u0 + c.l15;
      const float bias = p.h2att_b ? p.h2att_b[a] : 0.f;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int i = c.wave + WS_NW * k;
        if (i < c.MT && (k == 0 || c.wave == 0)) {
          f32x4 sum = scr[(0 * MT_MAX + i) * 64 + c.lane];
#pragma unroll
          for (int w = 1; w < WS_NW; ++w) sum += scr[(w * MT_MAX + i) * 64 + c.lane];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int rr = 16 * i + 4 * c.lq + r;
            if (rr < c.nrow) st_x<SAFE>(att_h + (unsigned)((c.rbegin + rr) * HH + a), sum[r] + bias);
          }
        }
      }
    }
    if (dbg && c.tid == 0) dbg[3] = __builtin_amdgcn_s_memrealtime();
    // ---- attention (:544-556)
    if constexpr (!DEC) {
      group_arrive(c);
      asm volatile("" : "+v"(c.lane), "+v"(c.l15), "+v"(c.lq), "+v"(c.tid));
      uint4 apre[AW_CR];
      attn_wave_preload(c, p, apre);                  // (not exchanged data: its latency passes while the workgroup waits for the others)
      if (!group_wait(c, (int*)c.smem)) return;
      if (dbg && c.tid == 0) dbg[4] = __builtin_amdgcn_s_memrealtime();
      attn_phase_wave<SAFE>(c, p, att_h, p.alpha_all + (size_t)t * N * p.R, ctx, apre);
    } else {                                          // (the decode kernel has no registers to spare)
      if (!group_barrier(c)) return;
      if (dbg && c.tid == 0) dbg[4] = __builtin_amdgcn_s_memrealtime();
      asm volatile("" : "+v"(c.lane), "+v"(c.l15), "+v"(c.lq), "+v"(c.tid));   // keep this phase's lane-derived values out of the others' live ranges
      attn_phase<T, SAFE, WS_NW, 2>(c, p, att_h, p.alpha_all + (size_t)t * N * p.R, ctx);
    }
    if (dbg && c.tid == 0) dbg[5] = __builtin_amdgcn_s_memrealtime();
    group_arrive(c);                                // (the wait is inside the block below, behind the requests that need no exchange)
    asm volatile("" : "+v"(c.lane), "+v"(c.l15), "+v"(c.lq), "+v"(c.tid));   // keep this phase's lane-derived values out of the others' live ranges
    // ---- lang_lstm (:438-441) + output dropout (:443): K split over the waves (stationary fragments in registers), one row
    // tile per pass; pass i writes its partial tiles to LDS half i & 1, ONE barrier, then the tile's owner sums and finishes
    // it while the other waves already multiply tile i + 1 (whose partials go to the other half)
    {
      auto tile_of = [&](int i) { const int x = i + tr; return x >= c.MT ? x - c.MT : x; };
      // The cell update of a tile is shared by the four waves: wave w takes accumulator component w, i.e. row 4 lq + w of
      // every 4-row group, so a pass costs a quarter of the transcendental work on its critical path.
      float cl[MT_MAX];                            // c_lang of (tile i, row 4 lq + wave, unit u0 + l15)
      {
        const float* c_prev = p.c_lang + (size_t)t * NH;
        const unsigned u = (unsigned)(c.u0 + c.l15);
#pragma unroll
        for (int i = 0; i < MT_MAX; ++i) {
          const int rr = 16 * i + 4 * c.lq + c.wave;
          cl[i] = c_prev[(unsigned)((c.rbegin + (rr < c.nrow ? rr : c.nrow - 1)) * HH) + u];
        }
      }
      // One register set of 12 activation fragments: fragment j of the NEXT row tile is requested right after the MFMAs that
      // consumed fragment j of this one, so a whole pass (MFMAs, barrier, the owner's cell update) covers its latency.
      u32x4 fa[12];
      auto aoff_of = [&](int i) {
        int ar = 16 * i + c.l15;
        ar = ar < c.nrow ? ar : c.nrow - 1;
        return (unsigned)((ar * HH + c.lq * 8) * 2);
      };
      auto load_frag = [&](int j, unsigned aoff) {
        const int m = ((j >> 2) == 2 ? 0 : (j >> 2) + 1) * 4 + ((j + j0) & 3);     // (as the stationary fragments' slots)
        // (two independent selects: a three-way select chain becomes a table in private memory, and with it everything
        // this lambda captures)
        const unsigned so = o_ctx + (m >= 4 ? o_han - o_ctx : 0u) + (m >= 8 ? o_hlp - o_han : 0u);
        fa[j] = bload<true>(rx, aoff, so + (unsigned)(((m & 3) * 4 + c.wave) * 64));
      };
      {
        // the first row tile's h_att / h_lang_prev fragments (exchanged one and three barriers ago) are requested before this
        // workgroup looks for the others' arrival at the barrier behind the attention; att_res's four behind it
        const unsigned a0 = aoff_of(tile_of(0));
#pragma unroll
        for (int j = 0; j < 8; ++j) load_frag(j, a0);
      }
      // ... and multiplied too (the first tile's eight k-fragments that need no exchange): in the time between this workgroup's
      // arrival and its first look at the barrier.  mfma_range: slots [jlo, jhi) of a pass (see the note on the inline asm below).
      f32x4 acc0[4];
      // `more` is a COMPILE-TIME fact (is there a later pass in the unrolled loop at all); whether the group really has that tile
      // only picks the address (the last real tile's again).  A load under a run-time branch here makes hipcc's s_waitcnt
      // insertion assume it may NOT have been issued, and every later slot of the pass then waits with vmcnt(4) .. vmcnt(0) --
      // i.e. for the loads this very pass has just issued, an L2 round trip per pass (round 6: 1.46 us of a pass's 2.26 were this).
      auto mfma_range = [&](f32x4 (&acc)[4], int jlo, int jhi, bool more, unsigned an) {
#pragma unroll
        for (int j = 0; j < 12; ++j) {
          if (j < jlo || j >= jhi) continue;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            if (j == 0) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=&v"(acc[g]) : "v"(fa[0]), "a"(w2[0][g]));
            else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc[g]) : "v"(fa[j]), "a"(w2[j][g]));
          }
          if (more) load_frag(j, an);
        }
      };
      {
        constexpr bool more0 = 1 < MT_MAX;
        if constexpr (!DEC) mfma_range(acc0, 0, 8, more0, aoff_of(tile_of(1 < c.MT ? 1 : 0)));   // (not the decode kernel: it spills as it is)
        if (!group_wait(c, (int*)c.smem)) return;
        if (dbg && c.tid == 0) dbg[6] = __builtin_amdgcn_s_memrealtime();
        const unsigned a0 = aoff_of(tile_of(0));
#pragma unroll
        for (int j = 8; j < 12; ++j) load_frag(j, a0);
      }
#pragma unroll
      for (int i = 0; i < MT_MAX; ++i) {
        if (i >= c.MT) break;                       // (an early exit, not a skipped block: pass i + 1 is reachable through pass i only)
        {
          const bool more = DEC ? (i + 1 < MT_MAX && i + 1 < c.MT) : i + 1 < MT_MAX;      // training kernel: compile-time (see mfma_range)
          const int tile = tile_of(i);
          const unsigned an = aoff_of(tile_of(i + 1 < MT_MAX && i + 1 < c.MT ? i + 1 : i));
          // (live-position logit layer: where this lane's row of the tile goes in the compact operand -- requested now, used in the
          // epilogue behind the MFMAs; a valid address whatever the row)
          int live_ci = -1;
          if constexpr (!DEC) {
            if (p.live_inv) {
              const int rq = 16 * tile + 4 * c.lq + c.wave;
              live_ci = p.live_inv[t * N + c.rbegin + (rq < c.nrow ? rq : 0)];
            }
          }
          // The stationary B fragments are named as ACCUMULATOR-file operands ("a"), which is what keeps them there for the
          // whole launch: left to itself hipcc parks them in AGPRs but copies each one back (4 x v_accvgpr_read) in front of
          // every MFMA.  Inline-asm MFMAs get no hazard padding from the compiler: gate g's chain is re-entered only after
          // the three other gates' MFMAs (the matrix pipe is in order), and the nops below cover MFMA result -> LDS store.
          f32x4 acc[4];
          if constexpr (!DEC) {
            if (i == 0) {
#pragma unroll
              for (int g = 0; g < 4; ++g) acc[g] = acc0[g];
              mfma_range(acc, 8, 12, more, an);
            } else {
              mfma_range(acc, 0, 12, more, an);
            }
          } else {
            // (mfma_range(acc, 0, 12, more, an) written out: called through the lambda the decode kernel, which spills as it is, comes
            // out with other waits and exec-mask saves and four more SGPR spills -- measured on the assembly, profiles/LOG.md)
#pragma unroll
            for (int j = 0; j < 12; ++j) {
#pragma unroll
              for (int g = 0; g < 4; ++g) {
                if (j == 0) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=&v"(acc[g]) : "v"(fa[0]), "a"(w2[0][g]));
                else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc[g]) : "v"(fa[j]), "a"(w2[j][g]));
              }
              if (more) load_frag(j, an);
            }
          }
          asm volatile("s_nop 7\n\ts_nop 7" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]));
          f32x4* half = scr + (i & 1) * (WS_NW * 4 * 64);
#pragma unroll
          for (int g = 0; g < 4; ++g) half[(c.wave * 4 + g) * 64 + c.lane] = acc[g];
          __syncthreads();
          if (dbg && c.tid == 0) dbg[11 + i] = __builtin_amdgcn_s_memrealtime();
          {
            // every wave sums component `wave` of the four partial tiles (fixed order: deterministic) and finishes that row
            float sg4[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              float v = 0.f;
#pragma unroll
              for (int w = 0; w < WS_NW; ++w) v += ((const float*)(half + (w * 4 + g) * 64 + c.lane))[c.wave];
              sg4[g] = v;
            }
            float cst = cl[0];
#pragma unroll
            for (int k = 1; k < MT_MAX; ++k) cst = tile == k ? cl[k] : cst;
            const int rr = 16 * tile + 4 * c.lq + c.wave;
            const unsigned u = (unsigned)(c.u0 + c.l15);
            const float gi = uic_sigmoid_t<bf16_t>(sg4[0] + pb[0][0]);
            const float gf = uic_sigmoid_t<bf16_t>(sg4[1] + pb[0][1]);
            const float gg = uic_tanh<bf16_t>(sg4[2] + pb[0][2]);
            const float go = uic_sigmoid_t<bf16_t>(sg4[3] + pb[0][3]);
            const float cn = gf * cst + gi * gg;
            const float h = go * uic_tanh<bf16_t>(cn);
            if (rr < c.nrow) {
              const unsigned nn = (unsigned)((c.rbegin + rr) * HH);
              const unsigned o = nn + u;
              p.c_lang[(size_t)(t + 1) * NH + o] = cn;
              st_x<SAFE>(h_lang_new + o, h);
              if (p.hdrop_all) {
                float hd = h;
                if (p.drop_p > 0.f) hd *= uic_drop_scale(p.seed, UIC_SITE_OUT0 + (unsigned)t, o, p.drop_p, 1.f / (1.f - p.drop_p));
                // (decode mode: the logit phase of every workgroup of the group reads these rows -- exchanged data)
                if (DEC) st_x<SAFE>((T*)p.hdrop_all + (size_t)t * NH + o, hd);
                else {
                  ((T*)p.hdrop_all)[(size_t)t * NH + o] = (bf16_t)hd;
                  // (live-position logit layer: the row also goes to its place in the compact operand -- no gather launches)
                  if (live_ci >= 0) ((T*)p.hdrop_live)[(size_t)live_ci * HH + u] = (bf16_t)hd;
                }
              }
              if (p.gates2) {
                T* G = (T*)p.gates2 + (size_t)t * N * 4 * HH + 4u * nn + u;
                __builtin_nontemporal_store((bf16_t)gi, G);
                __builtin_nontemporal_store((bf16_t)gf, G + HH);
                __builtin_nontemporal_store((bf16_t)gg, G + 2 * HH);
                __builtin_nontemporal_store((bf16_t)go, G + 3 * HH);
              }
            }
          }
        }
      }
      __syncthreads();                              // the scratch halves are free again (barrier flag, next step)
    }
    if (dbg && c.tid == 0) dbg[7] = __builtin_amdgcn_s_memrealtime();
    if (!DEC) {
      group_arrive(c);
      if (t + 1 < p.t1) lstm1_early(o_han);         // (step t + 1's h_att_prev = this step's h_att_new)
      if (!group_wait(c, (int*)c.smem)) return;
    } else {
      group_arrive(c);
      asm volatile("" : "+v"(c.lane), "+v"(c.l15), "+v"(c.lq), "+v"(c.tid));
      if (!dec_logits<SAFE>(p, c, t, lds)) return;
      if (dbg && c.tid == 0) dbg[8] = __builtin_amdgcn_s_memrealtime();
      if (!group_barrier(c)) return;
      asm volatile("" : "+v"(c.lane), "+v"(c.l15), "+v"(c.lq), "+v"(c.tid));
      dec_sample<SAFE>(p, c, t, lds);
      if (dbg && c.tid == 0) dbg[9] = __builtin_amdgcn_s_memrealtime();
      const bool tok_in_lds = p.dec_sample_max || p.dec_forced;      // greedy / forced: dec_sample left the group's tokens in LDS
      if (tok_in_lds) __syncthreads();
      else if (!group_barrier(c)) return;
      asm volatile("" : "+v"(c.lane), "+v"(c.l15), "+v"(c.lq), "+v"(c.tid));
      if (t + 1 < p.t1) dec_xt_gemm(p, c, t + 1, xg, xg5, tok_in_lds ? (const int*)(c.smem + DEC_OFF_LIST) : nullptr);
      if (dbg && c.tid == 0) dbg[10] = __builtin_amdgcn_s_memrealtime();
    }
    if (dbg) dbg += 16;
  }
}

__global__ __launch_bounds__(WS_NTH) void rnn_fwd_persist_ws_kernel(const UicRnnFwdParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Ctx c;
  const int mode = setup_ctx(p, smem + WS_W1_BYTES, c);
  if (mode == 0) return;
  if (mode == 2) ws_run<true, false>(p, c, smem);
  else ws_run<false, false>(p, c, smem);
}
__global__ __launch_bounds__(WS_NTH) void rnn_dec_persist_ws_kernel(const UicRnnFwdParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Ctx c;
  const int mode = setup_ctx(p, smem + WS_W1_BYTES, c);
  if (mode == 0) return;
  if (mode == 2) ws_run<true, true>(p, c, smem);
  else ws_run<false, true>(p, c, smem);
}

}  // namespace

int rnn_persist::ws_train_launch(const UicRnnFwdParams& p, hipStream_t s) {
  UIC_REQUIRE(p.e_att, "rnn_fwd_persist: the weight-stationary training kernel reads e_att = e^{2 p_att} (uic_exp2x2_launch)");
  static bool configured = false;
  if (!configured) {
    UIC_TRY(uic_check_hip(hipFuncSetAttribute((const void*)rnn_fwd_persist_ws_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, WS_LDS_BYTES), "hipFuncSetAttribute(rnn persist ws)"));
    configured = true;
  }
  hipLaunchKernelGGL(rnn_fwd_persist_ws_kernel, dim3(8 * PW), dim3(WS_NTH), WS_LDS_BYTES, s, p);
  UIC_LAUNCH_CHECK("rnn_fwd_persist_ws_kernel");
  return UIC_OK;
}

int rnn_persist::ws_decode_launch(const UicRnnFwdParams& p, hipStream_t s) {
  static bool configured = false;
  if (!configured) {
    UIC_TRY(uic_check_hip(hipFuncSetAttribute((const void*)rnn_dec_persist_ws_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, WS_LDS_BYTES), "hipFuncSetAttribute(rnn decode persist)"));
    configured = true;
  }
  hipLaunchKernelGGL(rnn_dec_persist_ws_kernel, dim3(8 * PW), dim3(WS_NTH), WS_LDS_BYTES, s, p);
  UIC_LAUNCH_CHECK("rnn_dec_persist_ws_kernel");
  return UIC_OK;
}
