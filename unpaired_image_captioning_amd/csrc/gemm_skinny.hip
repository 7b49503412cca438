// NT MFMA GEMM, register-staged form (gemm.hip's file comment describes the staging, the K segments and the LSTM mode): the
// per-decode-step "skinny" GEMMs with an in-block K split, the LSTM / maxout cell epilogues, and the problems the LDS-DMA kernels
// do not take (K segments, K not a whole 128-byte round, a pre-dropout copy).  gemm::skinny_launch picks the tile.
#include "gemm_internal.h"

namespace {

constexpr int LDS_STRIDE = 144;   // 128-B K slice + 16-B pad

// KS > 1: KS groups of WM x WN waves each take one 128-byte K slice of a (KS * 128)-byte K step for the
// SAME output tile and are summed through LDS at the end.  The skinny per-decode-step GEMMs (M = 640)
// are latency chains of K/BK dependent load->LDS->MFMA rounds; KS = 4 makes the chain 4x shorter and
// puts 4x the bytes in flight per round.
// PF: K rounds kept in flight in registers (global -> VGPR) ahead of the round being multiplied.  With PF rounds
// outstanding the chain is one load latency plus the LDS/MFMA rounds instead of one load latency PER round.
template <typename T, int TM, int TN, int WM, int WN, int KS, bool LSTM, int PF>
__global__ __launch_bounds__(64 * WM * WN * KS) void uic_gemm_kernel(const UicGemmParams p) {
  constexpr int NT = 64 * WM * WN * KS;
  constexpr int BM = 32 * TM * WM;
  constexpr int BN = 32 * TN * WN;
  constexpr int VEC = 16 / (int)sizeof(T);
  constexpr int BK = KS * 128 / (int)sizeof(T);   // K elements per round
  constexpr int CPR = 8 * KS;                      // 16-byte chunks per tile row per round
  constexpr int A_CH = BM * CPR / NT;
  constexpr int B_CH = BN * CPR / NT;
  static_assert(BM * CPR % NT == 0 && BN * CPR % NT == 0, "tile/threads mismatch");
  static_assert(!LSTM || TN == 4 || TN == 5, "LSTM mode keeps the 4 (nn.LSTMCell) or 5 (maxout LSTMCore) gate chunks in the N tiles of a wave");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sA = smem;
  char* sB = smem + KS * BM * LDS_STRIDE;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int ks_id = wave / (WM * WN);
  const int wmn = wave % (WM * WN);
  const int wm = wmn / WN;
  const int wn = wmn % WN;
  const int half = lane >> 5;
  const int r32 = lane & 31;
  // XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs (each with a private 4 MB L2), so
  // give every XCD a contiguous run of tiles, M fastest: the tiles of one XCD share a few B (weight) tiles and
  // walk A once, which keeps the re-reads of both operands inside that XCD's L2.  (bijective for any grid)
  int bm, bn;
  {
    const int gx = gridDim.x, nblk = gx * gridDim.y;
    const int lin = blockIdx.x + gx * blockIdx.y;
    const int lp = gemm::xcd_run(lin, nblk);
    bm = lp % gx;
    bn = lp / gx;
  }
  const int m0 = bm * BM;
  const int n0 = bn * (LSTM ? 32 * WN : BN);   // LSTM: first hidden unit of the block

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[i][j][k] = 0.f;

  int ntiles = 0;
  for (int s = 0; s < p.nseg; ++s) ntiles += (p.seg[s].K + BK - 1) / BK;

  uint4 rra[PF][A_CH], rrb[PF][B_CH];
  int seg = 0, k0 = 0;        // K position of the NEXT round to load

  auto load_tile = [&](uint4* ra, uint4* rb) {
    const UicGemmSeg sg = p.seg[seg];
    const char* Ab = (const char*)sg.A;
    const char* Bb = (const char*)sg.B;
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
      const int c = tid + i * NT;
      const int row = c / CPR;
      const int k = k0 + (c % CPR) * VEC;
      const int gm = m0 + row;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (gm < p.M && k < sg.K) v = *(const uint4*)(Ab + ((size_t)gm * sg.lda + k) * sizeof(T));
      ra[i] = v;
    }
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
      const int c = tid + i * NT;
      const int row = c / CPR;
      const int k = k0 + (c % CPR) * VEC;
      int grow;
      bool ok;
      if (LSTM) {
        const int u = n0 + (row / (TN * 32)) * 32 + (row & 31);
        grow = ((row % (TN * 32)) >> 5) * p.H + u;
        ok = u < p.H;
      } else {
        grow = n0 + row;
        ok = grow < p.N;
      }
      uint4 v = make_uint4(0, 0, 0, 0);
      if (ok && k < sg.K) v = *(const uint4*)(Bb + ((size_t)grow * sg.ldb + k) * sizeof(T));
      rb[i] = v;
    }
    k0 += BK;
    if (k0 >= sg.K) { ++seg; k0 = 0; }
  };
  auto store_tile = [&](const uint4* ra, const uint4* rb) {
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
      const int c = tid + i * NT;
      const int kc = c % CPR;
      *(uint4*)(sA + ((kc >> 3) * BM + c / CPR) * LDS_STRIDE + (kc & 7) * 16) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
      const int c = tid + i * NT;
      const int kc = c % CPR;
      *(uint4*)(sB + ((kc >> 3) * BN + c / CPR) * LDS_STRIDE + (kc & 7) * 16) = rb[i];
    }
  };

  // LSTM epilogue operands of the (row, unit) pairs this lane will finish -- the gate pre-activations made elsewhere, the
  // previous cell state, the biases: requested NOW, so that their latency passes under the K rounds instead of after them
  // (these launches are a few microseconds of dependent latencies each; the NMT step is 256 of them)
  constexpr int RPG0 = 16 / KS;
  float pf_pre[LSTM ? TM : 1][LSTM ? RPG0 : 1][LSTM ? TN : 1], pf_c[LSTM ? TM : 1][LSTM ? RPG0 : 1], pf_b[LSTM ? TN : 1];
  float pf_pre2[LSTM ? TM : 1][LSTM ? RPG0 : 1][LSTM ? TN : 1], pf_b2[LSTM ? TN : 1];
  if constexpr (LSTM) {
    // Round 6: none of these requests sits behind a condition any more.  An optional operand that is absent is read from a valid
    // stand-in word (c_out[0]) and dropped by a select; lanes / rows beyond the problem read a clamped index.  hipcc waits for a
    // load under a branch at the join of that branch: the two biases were eight serial memory round trips at the top of every
    // launch, and `pre2`, read in the epilogue under `if (p.pre2)`, four more per output row -- in launches that are a few
    // microseconds of dependent latencies in the first place.
    const int u = n0 + wn * 32 + r32;
    const int uc = u < p.H ? u : p.H - 1;
    const float* b1 = p.bias ? p.bias : p.c_out;
    const float* b2 = p.bias2 ? p.bias2 : p.c_out;
    float l1[TN], l2[TN];
#pragma unroll
    for (int g = 0; g < TN; ++g) {
      l1[g] = b1[p.bias ? g * p.H + uc : 0];
      l2[g] = b2[p.bias2 ? g * p.H + uc : 0];
    }
    const float* cpp = p.c_prev ? p.c_prev : p.c_out;
    const float* p1 = p.pre1 ? p.pre1 : p.c_out;
    const float* p2 = p.pre2 ? p.pre2 : p.c_out;
    float lc[TM][RPG0], lp1[TM][RPG0][TN], lp2[TM][RPG0][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int q = 0; q < RPG0; ++q) {
        const int reg = ks_id * RPG0 + q;
        const int row = m0 + (wm * TM + i) * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * half;   // (written out: reg is not a constant here, and gemm::c32_row changed the shifts)
        const int rc = row < p.M ? row : p.M - 1;
        lc[i][q] = cpp[p.c_prev ? (size_t)rc * p.H + uc : 0];
#pragma unroll
        for (int g = 0; g < TN; ++g) {
          lp1[i][q][g] = p1[p.pre1 ? (size_t)rc * p.ldpre1 + g * p.H + uc : 0];
          lp2[i][q][g] = p2[p.pre2 ? (size_t)rc * p.ldpre2 + g * p.H + uc : 0];
        }
      }
    // (the raw values stay in registers through the K rounds; the selects that drop the stand-ins are applied in the epilogue --
    // here they would be the first use of the loads and bring their wait to the top of the launch)
#pragma unroll
    for (int g = 0; g < TN; ++g) { pf_b[g] = l1[g]; pf_b2[g] = l2[g]; }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int q = 0; q < RPG0; ++q) {
        pf_c[i][q] = lc[i][q];
#pragma unroll
        for (int g = 0; g < TN; ++g) { pf_pre[i][q][g] = lp1[i][q][g]; pf_pre2[i][q][g] = lp2[i][q][g]; }
      }
  }
  // likewise the values an accumulating skinny GEMM adds to (f32 C += A B^T: the per-step `h2att` term of the BPTT loop)
  constexpr bool PFA = !LSTM && KS > 1;
  float pf_acc[PFA ? TM : 1][PFA ? TN : 1][PFA ? RPG0 : 1];
  const bool pf_accum = PFA && (p.flags & UIC_GEMM_ACCUM) && ((p.flags & UIC_GEMM_OUT_F32) || sizeof(T) == 4);
  if constexpr (PFA) {
    if (pf_accum) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int col = n0 + (wn * TN + j) * 32 + r32;
#pragma unroll
          for (int q = 0; q < RPG0; ++q) {
            const int reg = ks_id * RPG0 + q;
            const int row = m0 + (wm * TM + i) * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * half;   // (written out, as above)
            pf_acc[i][j][q] = (row < p.M && col < p.N) ? ((const float*)p.C)[(size_t)row * p.ldc + col] : 0.f;
          }
        }
    }
  }
#pragma unroll
  for (int j = 0; j < PF; ++j)
    if (j < ntiles) load_tile(rra[j], rrb[j]);
  for (int it0 = 0; it0 < ntiles; it0 += PF) {
#pragma unroll
  for (int j = 0; j < PF; ++j) {
    const int it = it0 + j;
    if (it >= ntiles) break;
    store_tile(rra[j], rrb[j]);
    __syncthreads();
    if (it + PF < ntiles) load_tile(rra[j], rrb[j]);
    const char* pa = sA + (ks_id * BM + wm * 32 * TM + r32) * LDS_STRIDE + half * 64;
    const char* pb = sB + (ks_id * BN + wn * 32 * TN + r32) * LDS_STRIDE + half * 64;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      uint4 fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[i] = *(const uint4*)(pa + i * 32 * LDS_STRIDE + ks * 16);
#pragma unroll
      for (int j = 0; j < TN; ++j) fb[j] = *(const uint4*)(pb + j * 32 * LDS_STRIDE + ks * 16);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          if constexpr (sizeof(T) == 2) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                __builtin_bit_cast(bf16x8, fa[i]), __builtin_bit_cast(bf16x8, fb[j]), acc[i][j], 0, 0, 0);
          } else {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(fa[i].x), __uint_as_float(fb[j].x), acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(fa[i].y), __uint_as_float(fb[j].y), acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(fa[i].z), __uint_as_float(fb[j].z), acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(fa[i].w), __uint_as_float(fb[j].w), acc[i][j], 0, 0, 0);
          }
        }
    }
    __syncthreads();
  }
  }

  // ---- reduce-scatter over the KS wave groups: group q ends up with the complete sums of accumulator
  // registers [q*RPG, (q+1)*RPG) of every tile (= 8-row bands of the output), so ALL waves share the epilogue.
  constexpr int RPG = 16 / KS;
  if constexpr (KS > 1) {
    float* red = (float*)smem;    // [dst group][src slot][wmn][tile][RPG][64]; staging buffers are free now
    constexpr int TILE = TM * TN;
#pragma unroll
    for (int q = 0; q < KS; ++q) {
      if (q != ks_id) {
        const int slot = ks_id < q ? ks_id : ks_id - 1;
        float* dst = red + (size_t)(((q * (KS - 1) + slot) * WM * WN + wmn) * TILE) * RPG * 64 + lane;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int rr = 0; rr < RPG; ++rr) dst[((i * TN + j) * RPG + rr) * 64] = acc[i][j][q * RPG + rr];
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < KS; ++q) {
      if (q == ks_id) {
#pragma unroll
        for (int slot = 0; slot < KS - 1; ++slot) {
          const float* src = red + (size_t)(((q * (KS - 1) + slot) * WM * WN + wmn) * TILE) * RPG * 64 + lane;
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
              for (int rr = 0; rr < RPG; ++rr) acc[i][j][q * RPG + rr] += src[((i * TN + j) * RPG + rr) * 64];
        }
      }
    }
  }

  // ------------------------------------------------------------------ epilogue
  // C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
  const float inv_keep = p.drop_p > 0.f ? 1.f / (1.f - p.drop_p) : 1.f;
  auto epilogue = [&](auto r0c) {
    constexpr int R0 = decltype(r0c)::value;
    if constexpr (!LSTM) {
      const bool out_f32 = (p.flags & UIC_GEMM_OUT_F32) || sizeof(T) == 4;
      int arow[TM][RPG];                 // addend row of every output row this lane holds (row % add_mod, once per row)
      if (p.addend) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int q = 0; q < RPG; ++q) {
            const int reg = R0 + q;
            arow[i][q] = (m0 + (wm * TM + i) * 32 + gemm::c32_row(reg, half)) % p.add_mod;
          }
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int col = n0 + (wn * TN + j) * 32 + r32;
          if (col >= p.N) continue;
          float b = 0.f;
          if (p.bias) b += p.bias[col];
          if (p.bias2) b += p.bias2[col];
#pragma unroll
          for (int reg = R0; reg < R0 + RPG; ++reg) {
            const int row = m0 + (wm * TM + i) * 32 + gemm::c32_row(reg, half);
            if (row >= p.M) continue;
            float v = acc[i][j][reg] + b;
            if (p.addend) v += p.addend[(size_t)arow[i][reg - R0] * p.ld_add + col];
            if (p.flags & UIC_GEMM_RELU) v = fmaxf(v, 0.f);
            if (p.flags & UIC_GEMM_TANH) v = uic_tanh<T>(v);
            if (p.row_len) {
              const int n = row / p.R;
              if (row - n * p.R >= p.row_len[n]) v = 0.f;
            }
            if (p.C_pre) ((T*)p.C_pre)[(size_t)row * p.ldc_pre + col] = uic_from_f<T>(v);
            if (p.drop_p > 0.f) v *= uic_drop_scale(p.seed, p.site, (unsigned)(row + p.drop_row0) * (unsigned)p.N + (unsigned)col, p.drop_p, inv_keep);
            const size_t o = (size_t)row * p.ldc + col;
            if (out_f32) {
              float* C = (float*)p.C;
              if constexpr (PFA) {
                if (p.flags & UIC_GEMM_ACCUM) v += pf_accum ? pf_acc[i][j][reg - R0] : C[o];   // (requested before the K rounds)
              } else {
                if (p.flags & UIC_GEMM_ACCUM) v += C[o];
              }
              C[o] = v;
            } else {
              T* C = (T*)p.C;
              if (p.flags & UIC_GEMM_ACCUM) v += uic_to_f(C[o]);
              C[o] = uic_from_f<T>(v);
            }
          }
        }
    } else {
      const int H = p.H;
      const int u = n0 + wn * 32 + r32;
      if (u < H) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int reg = R0; reg < R0 + RPG; ++reg) {
            const int row = m0 + (wm * TM + i) * 32 + gemm::c32_row(reg, half);
            if (row >= p.M) continue;
            float g4[TN];
#pragma unroll
            for (int g = 0; g < TN; ++g) {
              float v = acc[i][g][reg] + ((p.bias ? pf_b[g] : 0.f) + (p.bias2 ? pf_b2[g] : 0.f));
              if (p.pre1) v += pf_pre[i][reg - R0][g];             // (requested before the K rounds)
              if (p.pre2) v += pf_pre2[i][reg - R0][g];
              g4[g] = v;
            }
            const float cp = p.c_prev ? pf_c[i][reg - R0] : 0.f;
            if constexpr (TN == 4) {
              // nn.LSTMCell: chunks (i, f, g, o)
              const float gi = uic_sigmoid_t<T>(g4[0]);
              const float gf = uic_sigmoid_t<T>(g4[1]);
              const float gg = uic_tanh<T>(g4[2]);
              const float go = uic_sigmoid_t<T>(g4[3]);
              const float c = gf * cp + gi * gg;
              const float h = go * uic_tanh<T>(c);
              p.c_out[(size_t)row * H + u] = c;
              ((T*)p.h_out)[(size_t)row * p.ldh + u] = uic_from_f<T>(h);
              if (p.h_drop) {
                float hd = h;
                if (p.drop_p > 0.f) hd *= uic_drop_scale(p.seed, p.site, (unsigned)row * (unsigned)H + (unsigned)u, p.drop_p, inv_keep);
                ((T*)p.h_drop)[(size_t)row * p.ldhd + u] = uic_from_f<T>(hd);
              }
              if (p.gates_out) {
                T* G = (T*)p.gates_out + (size_t)row * 4 * H + u;      // read again only in the backward pass
                __builtin_nontemporal_store(uic_from_f<T>(gi), G);
                __builtin_nontemporal_store(uic_from_f<T>(gf), G + H);
                __builtin_nontemporal_store(uic_from_f<T>(gg), G + 2 * H);
                __builtin_nontemporal_store(uic_from_f<T>(go), G + 3 * H);
              }
            } else {
              // maxout LSTMCore (P/models/FCModel_NMT.py:32-50): chunks (in, forget, out, a, b); g = max(a, b);
              // the DROPPED next_h is both the output and the recurrent state (:47-50)
              const float gi = uic_sigmoid_t<T>(g4[0]);
              const float gf = uic_sigmoid_t<T>(g4[1]);
              const float go = uic_sigmoid_t<T>(g4[2]);
              const bool first = g4[3] >= g4[4];
              const float gg = first ? g4[3] : g4[4];
              const float c = gf * cp + gi * gg;
              float h = go * uic_tanh<T>(c);
              if (p.drop_p > 0.f) h *= uic_drop_scale(p.seed, p.site, (unsigned)row * (unsigned)H + (unsigned)u, p.drop_p, inv_keep);
              p.c_out[(size_t)row * H + u] = c;
              ((T*)p.h_out)[(size_t)row * p.ldh + u] = uic_from_f<T>(h);
              if (p.gates_out) {
                T* G = (T*)p.gates_out + (size_t)row * 5 * H + u;
                G[0] = uic_from_f<T>(gi);
                G[H] = uic_from_f<T>(gf);
                G[2 * H] = uic_from_f<T>(go);
                G[3 * H] = uic_from_f<T>(gg);
                G[4 * H] = uic_from_f<T>(first ? 1.f : 0.f);
              }
            }
          }
      }
    }
  };
  if constexpr (KS == 1) {
    epilogue(std::integral_constant<int, 0>{});
  } else {
    static_assert(KS == 4 || KS == 8, "epilogue dispatch is written for KS = 4 or 8");
    if (ks_id == 0) epilogue(std::integral_constant<int, 0>{});
    else if (ks_id == 1) epilogue(std::integral_constant<int, RPG>{});
    else if (ks_id == 2) epilogue(std::integral_constant<int, 2 * RPG>{});
    else if (ks_id == 3) epilogue(std::integral_constant<int, 3 * RPG>{});
    else if constexpr (KS == 8) {
      if (ks_id == 4) epilogue(std::integral_constant<int, 4 * RPG>{});
      else if (ks_id == 5) epilogue(std::integral_constant<int, 5 * RPG>{});
      else if (ks_id == 6) epilogue(std::integral_constant<int, 6 * RPG>{});
      else epilogue(std::integral_constant<int, 7 * RPG>{});
    }
  }
}

template <typename T, int TM, int TN, int WM, int WN, int KS, bool LSTM, int PF = 1>
int launch_cfg(const UicGemmParams& p, hipStream_t s) {
  constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
  constexpr int stage_bytes = KS * (BM + BN) * LDS_STRIDE;
  constexpr int red_bytes = KS * (KS - 1) * WM * WN * TM * TN * (16 / KS) * 64 * 4;
  constexpr int lds = stage_bytes > red_bytes ? stage_bytes : red_bytes;
  static bool configured = false;
  if (!configured) {
    if (lds > 64 * 1024)
      UIC_TRY(uic_check_hip(hipFuncSetAttribute((const void*)uic_gemm_kernel<T, TM, TN, WM, WN, KS, LSTM, PF>,
                                                hipFuncAttributeMaxDynamicSharedMemorySize, lds), "hipFuncSetAttribute(gemm)"));
    configured = true;
  }
  dim3 grid((p.M + BM - 1) / BM, LSTM ? (p.H + 32 * WN - 1) / (32 * WN) : (p.N + BN - 1) / BN);
  hipLaunchKernelGGL((uic_gemm_kernel<T, TM, TN, WM, WN, KS, LSTM, PF>), grid, dim3(64 * WM * WN * KS), lds, s, p);
  UIC_LAUNCH_CHECK("uic_gemm_kernel");
  return UIC_OK;
}

template <typename T>
int launch_skinny(const UicGemmParams& p, hipStream_t s) {
  // skinny problems (the per-decode-step GEMMs, M = rows of one step): 64-row tiles with a 4-way in-block K split
  // PF (register prefetch depth) stays 1: measured on MI355X, PF = 2 / 4 do not shorten these launches (their time is
  // launch + epilogue overhead plus ~0.9 us per K round, not exposed load latency) and PF = 4 slows the dX GEMMs.
  if (p.lstm == 2) return launch_cfg<T, 1, 5, 2, 1, 4, true>(p, s);
  if (p.lstm) return launch_cfg<T, 1, 4, 2, 1, 4, true>(p, s);
  if (gemm::many_tiles(p)) return launch_cfg<T, 1 + 1, 2, 2, 2, 1, false>(p, s);
  // one row tile (M <= 64: the pivot NMT's per-step GEMMs at batch 64) with a long reduction: 8-way in-block K split on a
  // 64 x 32 tile -- the chain of dependent K rounds is what such a launch takes, and twice as many workgroups share the columns
  if (p.M <= 64) {
    int ktot = 0;
    for (int i = 0; i < p.nseg; ++i) ktot += p.seg[i].K;
    if (ktot * (int)sizeof(T) >= 2048) return launch_cfg<T, 1, 1, 2, 1, 8, false>(p, s);   // (K = 512 launches: no gain measured)
  }
  return launch_cfg<T, 1, 1, 2, 2, 4, false>(p, s);
}

}  // namespace

int gemm::skinny_launch(const UicGemmParams& p, hipStream_t s) {
  return p.dtype == UIC_BF16 ? launch_skinny<bf16_t>(p, s) : launch_skinny<float>(p, s);
}
