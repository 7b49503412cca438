// NT MFMA GEMM, LDS-DMA form (operands and epilogue options: gemm.hip's file comment).
#include "gemm_internal.h"

namespace {

using gemm::u32x4;

// Large-GEMM path: 128x128 tile, 4 waves (2x2, 64x64 each), K rounds of 128 bytes staged global -> LDS
// directly (global_load_lds_dwordx4, no VGPR round trip) into two LDS buffers, one barrier per round.
// LDS rows are the bare 128-byte K slices (an LDS-DMA wave instruction writes 1 KiB = 8 rows linearly),
// so the bank-conflict fix is an XOR swizzle applied to the per-lane SOURCE address and again on the
// fragment read: 16-byte chunk c of tile row r lives at chunk c ^ ((r >> 1) & 7), which makes the 16-lane
// groups of ds_read_b128 hit 16 distinct 16-byte slots of the 256-byte bank row.
// Requires one K segment with K a multiple of the round (64 bf16 / 32 f32 elements).
// STAGES (round 6): 2 = two LDS buffers, the next round's DMA issued at the top of a round and waited for at the top of the next
// -- one L2 / Infinity Cache latency (~0.8 us) per 64-deep K round whatever the MFMA time (0.2 us), hidden only by the CU's second
// workgroup; 3 = a ring of three buffers (96 KB: one workgroup per CU), two rounds in flight.  For launches that put at most one
// workgroup on a CU anyway -- the BPTT loop's split-K d x GEMMs: 160 / 240 workgroups of 8 rounds -- the ring is what hides the latency.
// MAPPED (UicGemmParams.slab_row_map, split-K slabs only): the map entries of the tile's rows are requested before the first K round
// and used in the epilogue only -- nothing is loaded between the K loop and the stores.  (First form: every lane requested the 32
// entries of the rows it holds, 32 loads in front of the first LDS-DMA round: + 1 us per launch, which made the compact d x1 launch
// slower than the full one, 10.5 against 9.5 us.)
template <typename T, int STAGES = 2, bool MAPPED = false>
__global__ __launch_bounds__(256, 2) void uic_gemm_glds_kernel(const UicGemmParams p) {   // (2 waves per SIMD = two workgroups per CU: <= 256 registers)
  constexpr int BM = 128, BN = 128;
  constexpr int BK = 128 / (int)sizeof(T);
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [2][A 16 KB | B 16 KB]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int half = lane >> 5, r32 = lane & 31;

  // XCD-aware + grouped tile order: each XCD takes a contiguous run of tiles; inside it tiles advance over
  // GM = 8 row-tiles before moving to the next column tile, so one XCD's L2 holds an 8-tile A band while
  // B tiles stream through once per band.
  // Split-K launches (round 6): the run is taken over the whole 3-D grid in dispatch order (x fastest, z slowest), K slice
  // slowest in the tile order -- an XCD then works on ONE K slice (two at most) of a few column tiles: at the BPTT loop's
  // 5 x 12 x 4 grid it reads 0.66 MB of A and 0.79 MB of B instead of all 2.6 MB of A and B tiles of every K slice, and its B
  // tiles are the same ones every decode step.  (gz = 1: the order above, unchanged)
  int bm, bn, bz;
  {
    const int gx = gridDim.x, gy = gridDim.y, nxy = gx * gy, nblk = nxy * gridDim.z;
    const int lin = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
    const int lp3 = gemm::xcd_run(lin, nblk);
    bz = lp3 / nxy;
    gemm::grouped_tile(lp3 - bz * nxy, gx, gy, bm, bn);
  }
  const int m0 = bm * BM, n0 = bn * BN;

  // MAPPED: a wave's output rows are the 64 rows m0 + 64 wm ...: ONE request per lane, for the row of its own number (clamped to
  // the last row, dropped below by a select: not a load under a condition); the epilogue hands the entries round by lane shuffles
  int mval = -1;
  if constexpr (MAPPED) {
    const int row = m0 + wm * 64 + lane;
    const int v = p.slab_row_map[min(row, p.M - 1)];
    mval = row < p.M ? v : -1;
  }

  const UicGemmSeg sg = p.seg[0];
  // per-lane source pointers of this wave's 4 A and 4 B LDS-DMA instructions per round
  const int slot = lane & 7;
  const char* srcA[4];
  const char* srcB[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (wave * 4 + i) * 8 + (lane >> 3);
    const int chunk = slot ^ ((row >> 1) & 7);
    const int gm = min(m0 + row, p.M - 1);
    const int gn = min(n0 + row, p.N - 1);
    srcA[i] = (const char*)sg.A + (size_t)gm * sg.lda * sizeof(T) + chunk * 16;
    srcB[i] = (const char*)sg.B + (size_t)gn * sg.ldb * sizeof(T) + chunk * 16;
  }
  auto stage = [&](int kt, int buf) {
    char* dA = smem + buf * 32768 + wave * 4096;
    char* dB = dA + 16384;
    const size_t koff = (size_t)kt * 128;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      gemm::dma16(srcA[i] + koff, dA + i * 1024);
      gemm::dma16(srcB[i] + koff, dB + i * 1024);
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[i][j][k] = 0.f;

  // K rounds of this workgroup: all of them, or slice blockIdx.z of a split-K launch
  int kt0 = 0, nt = sg.K / BK;
  gemm::splitk_slice(p.splitk, bz, kt0, nt);
  // LDS byte addresses of this lane's fragment chunks (buffer 0, first 32-row sub-tile), one per K step
  const int sw = (r32 >> 1) & 7;
  const unsigned lds0 = (unsigned)(size_t)((__attribute__((address_space(3))) char*)smem);
  unsigned adA[4], adB[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const unsigned pc = (unsigned)(((half * 4 + ks) ^ sw) * 16);
    adA[ks] = lds0 + (unsigned)((wm * 64 + r32) * 128) + pc;
    adB[ks] = lds0 + 16384u + (unsigned)((wn * 64 + r32) * 128) + pc;
  }
  // The fragment reads are inline asm on purpose: hipcc cannot tell the LDS-DMA writes of the NEXT round's
  // buffer from these reads and would drain vmcnt(0) before the first ds_read of every round, serialising
  // load and MFMA.  Ordering is by hand: vmcnt(0) + barrier at the top of a round covers the RAW on this
  // round's buffer and the WAR on the other one; counted lgkmcnt waits name their destination registers.
#define UIC_DSR(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))
#define UIC_MFMA4(A0, A1, B0, B1)                                                                         \
  do {                                                                                                   \
    if constexpr (sizeof(T) == 2) {                                                                      \
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A0), __builtin_bit_cast(bf16x8, B0), acc[0][0], 0, 0, 0); \
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A0), __builtin_bit_cast(bf16x8, B1), acc[0][1], 0, 0, 0); \
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A1), __builtin_bit_cast(bf16x8, B0), acc[1][0], 0, 0, 0); \
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A1), __builtin_bit_cast(bf16x8, B1), acc[1][1], 0, 0, 0); \
    } else {                                                                                             \
      const u32x4 aa[2] = {A0, A1}, bb[2] = {B0, B1};                                                    \
      _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j) {      \
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(aa[i].x), __uint_as_float(bb[j].x), acc[i][j], 0, 0, 0); \
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(aa[i].y), __uint_as_float(bb[j].y), acc[i][j], 0, 0, 0); \
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(aa[i].z), __uint_as_float(bb[j].z), acc[i][j], 0, 0, 0); \
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(aa[i].w), __uint_as_float(bb[j].w), acc[i][j], 0, 0, 0); \
      }                                                                                                  \
    }                                                                                                    \
  } while (0)
#define UIC_ISSUE(A0, A1, B0, B1, KS) \
  UIC_DSR(A0, aA[KS], 0); UIC_DSR(A1, aA[KS], 4096); UIC_DSR(B0, aB[KS], 0); UIC_DSR(B1, aB[KS], 4096)
#define UIC_WAIT(N, A0, A1, B0, B1)                                                           \
  asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(A0), "+v"(A1), "+v"(B0), "+v"(B1));         \
  __builtin_amdgcn_sched_barrier(0)
  auto compute = [&](unsigned bo) {                    // bo = byte offset of the round's buffer (uniform)
    unsigned aA[4], aB[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) { aA[ks] = adA[ks] + bo; aB[ks] = adB[ks] + bo; }
    u32x4 a00, a01, b00, b01, a10, a11, b10, b11;     // two register sets: K step ks uses set ks & 1
    UIC_ISSUE(a00, a01, b00, b01, 0);
    UIC_ISSUE(a10, a11, b10, b11, 1);
    UIC_WAIT(4, a00, a01, b00, b01);
    UIC_MFMA4(a00, a01, b00, b01);
    UIC_ISSUE(a00, a01, b00, b01, 2);
    UIC_WAIT(4, a10, a11, b10, b11);
    UIC_MFMA4(a10, a11, b10, b11);
    UIC_ISSUE(a10, a11, b10, b11, 3);
    UIC_WAIT(4, a00, a01, b00, b01);
    UIC_MFMA4(a00, a01, b00, b01);
    UIC_WAIT(0, a10, a11, b10, b11);
    UIC_MFMA4(a10, a11, b10, b11);
  };
#undef UIC_WAIT
#undef UIC_ISSUE
#undef UIC_MFMA4
#undef UIC_DSR
  if constexpr (STAGES == 2) {
    if (nt > 0) stage(kt0, 0);
    for (int t = 0; t < nt; t += 2) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (t + 1 < nt) stage(kt0 + t + 1, 1);
      compute(0u);
      if (t + 1 < nt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (t + 2 < nt) stage(kt0 + t + 2, 0);
        compute(32768u);
      }
    }
  } else {
    // ring: rounds t .. t + STAGES - 2 are in flight at the top of round t.  A wave's DMA instructions complete in order, 8 per round:
    // round t's have landed once at most 8 x (newer rounds) are outstanding; the barrier behind the wait makes every wave's share
    // of round t visible and says that buffer (t - 1) % STAGES -- which the next DMA overwrites -- has been read by all.
    for (int i = 0; i < STAGES - 1 && i < nt; ++i) stage(kt0 + i, i);
    int buf = 0;
    for (int t = 0; t < nt; ++t) {
      const int newer = min(STAGES - 2, nt - 1 - t);
      if (newer >= 2) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
      else if (newer == 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (t + STAGES - 1 < nt) stage(kt0 + t + STAGES - 1, buf == 0 ? STAGES - 1 : buf - 1);
      compute((unsigned)buf * 32768u);
      buf = buf + 1 == STAGES ? 0 : buf + 1;
    }
  }

  if constexpr (MAPPED) {   // raw partial tile -> rows slab_row_map[row] of slab[z] (32-bit offsets: the launcher checked the size)
    float* slab = p.slab + (size_t)bz * p.slab_rows * p.N;
    int mrow[2][16];                     // the slab row of every output row this lane holds (every lane takes part: no test before)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) mrow[i][reg] = __shfl(mval, i * 32 + gemm::c32_row(reg, half));
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = n0 + (wn * 2 + j) * 32 + r32;
        if (col >= p.N) continue;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int mr = mrow[i][reg];
          if ((unsigned)mr < (unsigned)p.slab_rows) slab[(unsigned)mr * (unsigned)p.N + (unsigned)col] = acc[i][j][reg];
        }
      }
    return;
  }
  if (p.slab) {   // raw partial tile -> slab[z]  (the same text ends uic_gemm_tn_kernel, gemm_tn.hip: as one function it changed both kernels' branches)
    float* slab = p.slab + (size_t)bz * p.M * p.N;
    if (m0 + BM <= p.M && n0 + BN <= p.N && (size_t)p.M * (size_t)p.N < ((size_t)1 << 31)) {   // whole tile: no tests, 32-bit offsets
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const unsigned ro = (unsigned)(m0 + (wm * 2 + i) * 32 + gemm::c32_row(reg, half)) * (unsigned)p.N + (unsigned)(n0 + wn * 64 + r32);
          slab[ro] = acc[i][0][reg];
          slab[ro + 32] = acc[i][1][reg];
        }
      return;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = n0 + (wn * 2 + j) * 32 + r32;
        if (col >= p.N) continue;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int row = m0 + (wm * 2 + i) * 32 + gemm::c32_row(reg, half);
          if (row < p.M) slab[(size_t)row * p.N + col] = acc[i][j][reg];
        }
      }
    return;
  }

  const float inv_keep = p.drop_p > 0.f ? 1.f / (1.f - p.drop_p) : 1.f;
  const bool out_f32 = (p.flags & UIC_GEMM_OUT_F32) || sizeof(T) == 4;
  // Fast epilogue (everything but tanh): ReLU / dropout / output type / whole-tile are decided ONCE (16 specialised bodies), the
  // rarer options (addend, region mask) cost a uniform test per row, offsets are 32-bit, whole tiles skip the bounds tests.  Measured: the general
  // epilogue below, which tests its eight options per element, was ~14 us per wave of tiles -- 43 of the 62 us of a logit chunk.
  if (!(p.flags & UIC_GEMM_TANH) && (size_t)p.M * (size_t)p.ldc < ((size_t)1 << 31)) {
    const bool full = m0 + BM <= p.M && n0 + BN <= p.N;
    const bool relu = (p.flags & UIC_GEMM_RELU) != 0, drop = p.drop_p > 0.f, accum = (p.flags & UIC_GEMM_ACCUM) != 0;
    float bj[2];
    unsigned cj[2];
    bool cok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + (wn * 2 + j) * 32 + r32;
      cj[j] = (unsigned)col; cok[j] = col < p.N; bj[j] = 0.f;
      if (cok[j]) { if (p.bias) bj[j] += p.bias[col]; if (p.bias2) bj[j] += p.bias2[col]; }
    }
    auto body = [&](auto relu_c, auto drop_c, auto f32_c, auto full_c) {
      constexpr bool RELU = decltype(relu_c)::value, DROP = decltype(drop_c)::value, F32 = decltype(f32_c)::value, FULL = decltype(full_c)::value;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int row = m0 + (wm * 2 + i) * 32 + gemm::c32_row(reg, half);
          if (!FULL && row >= p.M) continue;
          const unsigned ro = (unsigned)row * (unsigned)p.ldc;
          const unsigned dro = (unsigned)(row + p.drop_row0) * (unsigned)p.N;
          // per-row work of the rarer options (uniform tests): the addend's row, the region mask of pack_wrapper
          const float* ad = p.addend ? p.addend + (size_t)(row % p.add_mod) * p.ld_add : nullptr;
          bool live = true;
          if (p.row_len) { const int n = row / p.R; live = row - n * p.R < p.row_len[n]; }
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            if (!FULL && !cok[j]) continue;
            float v = acc[i][j][reg] + bj[j];
            if (ad) v += ad[cj[j]];
            if (RELU) v = fmaxf(v, 0.f);
            if (!live) v = 0.f;
            if (DROP) v *= uic_drop_scale(p.seed, p.site, dro + cj[j], p.drop_p, inv_keep);
            if (F32) {
              float* o = (float*)p.C + (ro + cj[j]);
              if (accum) v += *o;
              *o = v;
            } else {
              T* o = (T*)p.C + (ro + cj[j]);
              if (accum) v += uic_to_f(*o);
              *o = uic_from_f<T>(v);
            }
          }
        }
    };
    using TT = std::true_type; using FF = std::false_type;
#define UIC_EPI(R, D)                                                                              \
    do {                                                                                           \
      if (out_f32) { if (full) body(R{}, D{}, TT{}, TT{}); else body(R{}, D{}, TT{}, FF{}); }      \
      else { if (full) body(R{}, D{}, FF{}, TT{}); else body(R{}, D{}, FF{}, FF{}); }              \
    } while (0)
    if (relu && drop) UIC_EPI(TT, TT);
    else if (relu) UIC_EPI(TT, FF);
    else if (drop) UIC_EPI(FF, TT);
    else UIC_EPI(FF, FF);
#undef UIC_EPI
    return;
  }
  int arow[2][16];                       // addend row of every output row this lane holds (row % add_mod, once per row)
  if (p.addend) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) arow[i][reg] = (m0 + (wm * 2 + i) * 32 + gemm::c32_row(reg, half)) % p.add_mod;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + (wn * 2 + j) * 32 + r32;
      if (col >= p.N) continue;
      float b = 0.f;
      if (p.bias) b += p.bias[col];
      if (p.bias2) b += p.bias2[col];
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int row = m0 + (wm * 2 + i) * 32 + gemm::c32_row(reg, half);
        if (row >= p.M) continue;
        float v = acc[i][j][reg] + b;
        if (p.addend) v += p.addend[(size_t)arow[i][reg] * p.ld_add + col];
        if (p.flags & UIC_GEMM_RELU) v = fmaxf(v, 0.f);
        if (p.flags & UIC_GEMM_TANH) v = uic_tanh<T>(v);
        if (p.row_len) {
          const int n = row / p.R;
          if (row - n * p.R >= p.row_len[n]) v = 0.f;
        }
        if (p.drop_p > 0.f) v *= uic_drop_scale(p.seed, p.site, (unsigned)(row + p.drop_row0) * (unsigned)p.N + (unsigned)col, p.drop_p, inv_keep);
        const size_t o = (size_t)row * p.ldc + col;
        if (out_f32) {
          float* C = (float*)p.C;
          if (p.flags & UIC_GEMM_ACCUM) v += C[o];
          C[o] = v;
        } else {
          T* C = (T*)p.C;
          if (p.flags & UIC_GEMM_ACCUM) v += uic_to_f(C[o]);
          C[o] = uic_from_f<T>(v);
        }
      }
    }
}

template <typename T>
int launch_glds(const UicGemmParams& p, hipStream_t s) {
  static bool configured = false;
  if (!configured) {
    UIC_TRY(uic_check_hip(hipFuncSetAttribute((const void*)uic_gemm_glds_kernel<T, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536),
                          "hipFuncSetAttribute(gemm glds)"));
    UIC_TRY(uic_check_hip(hipFuncSetAttribute((const void*)uic_gemm_glds_kernel<T, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, 98304),
                          "hipFuncSetAttribute(gemm glds ring)"));
    configured = true;
  }
  dim3 grid((p.M + 127) / 128, (p.N + 127) / 128, p.splitk > 1 ? p.splitk : 1);
  // the three-buffer ring where the launch is well under one workgroup per CU and the K loop has rounds to overlap.  Measured in the
  // training step (rocprofv3, median): the first logit chunk's d h (5 x 4 x 8 workgroups, 18 rounds) 22.7 -> 17.6 us, the BPTT loop's
  // d x1 (5 x 8 x 4, 8 rounds) 10.1 -> 9.8; its d x2 (5 x 12 x 4 = 240 workgroups) 13.2 -> 15.6: at 96 KB a CU takes ONE of them where
  // it took two 64-KB ones, and beside the side streams' 128-KB workgroups the launch then waits for 240 free CUs instead of 120 --
  // so the ring stops at 192 workgroups.  Alone on the chip it makes a K round cost 0.3 us instead of 0.8 (tools/gemm_headroom.py).
  const int rounds = p.seg[0].K / (128 / (int)sizeof(T)) / (p.splitk > 1 ? p.splitk : 1);
  const long wgs = (long)grid.x * grid.y * grid.z;
  const bool ring = ((wgs <= 192 && rounds >= 3) || (wgs <= 256 && rounds >= 32)) && !(p.flags & UIC_GEMM_NO_RING);   // (long K loops: also at one workgroup per CU)
  if (p.slab_row_map) {
    if constexpr (sizeof(T) == 2) {
      static bool configured_map = false;
      if (!configured_map) {
        UIC_TRY(uic_check_hip(hipFuncSetAttribute((const void*)uic_gemm_glds_kernel<T, 2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536),
                              "hipFuncSetAttribute(gemm glds, row map)"));
        UIC_TRY(uic_check_hip(hipFuncSetAttribute((const void*)uic_gemm_glds_kernel<T, 3, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 98304),
                              "hipFuncSetAttribute(gemm glds ring, row map)"));
        configured_map = true;
      }
      if (ring) hipLaunchKernelGGL((uic_gemm_glds_kernel<T, 3, true>), grid, dim3(256), 98304, s, p);
      else hipLaunchKernelGGL((uic_gemm_glds_kernel<T, 2, true>), grid, dim3(256), 65536, s, p);
      UIC_LAUNCH_CHECK("uic_gemm_glds_kernel (row map)");
      return UIC_OK;
    }
  }
  if (ring) hipLaunchKernelGGL((uic_gemm_glds_kernel<T, 3>), grid, dim3(256), 98304, s, p);
  else hipLaunchKernelGGL((uic_gemm_glds_kernel<T, 2>), grid, dim3(256), 65536, s, p);
  UIC_LAUNCH_CHECK("uic_gemm_glds_kernel");
  return UIC_OK;
}

}  // namespace

int gemm::glds_launch(const UicGemmParams& p, hipStream_t s) {
  return p.dtype == UIC_BF16 ? launch_glds<bf16_t>(p, s) : launch_glds<float>(p, s);
}
