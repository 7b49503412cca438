// Word embedding of the captioners and the pivot NMT (gfx950): nn.Embedding + ReLU + Dropout for all T steps at once
// (P/models/AttModel.py:73-75,160) and its gradient with the positions bucketed by token -- a stable counting sort in four
// launches, then a gather in two -- so that every table row has one owner and no floating-point atomic is needed.
// The C entries uic_embedding_* (api.hip) check the arguments; the launchers below do the work.
#include "uic_common.h"
#include "uic_host.h"
#include <type_traits>

namespace {

constexpr int NT = 256;

// ------------------------------------------------------------------ forward
// self.embed = Embedding + ReLU + Dropout (P/models/AttModel.py:73-75,160), all T steps at once:
// out[(t*N+n), :] = dropout(relu(table[tokens[n, t]]))
// (the table comes as f32 masters or in the operand dtype: bf16 runs of the captioner gather from the bf16 copy of the table that
// the weight refresh keeps beside the other operand copies -- the copy a data-parallel rank receives from the all-gather)
template <typename T, typename TT>
__global__ void embed_fwd_kernel(const TT* __restrict__ table, int V1, int E, const int64_t* __restrict__ tokens,
                                 int ldtok, int N, int TS, float drop_p, unsigned seed, unsigned site, size_t idx_base, int relu, T* __restrict__ out) {
  const int e4 = E / 4;
  const size_t total = (size_t)TS * N * e4;
  const float inv_keep = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const size_t row = i / e4;
    const int c = (int)(i - row * e4) * 4;
    const int t = (int)(row / N), n = (int)(row - (size_t)t * N);
    long tok = tokens[(size_t)n * ldtok + t];
    if (tok < 0 || tok >= V1) tok = 0;
    float f[4];
    uic_table_load4(table + (size_t)tok * E + c, f);
    if (relu) {
#pragma unroll
      for (int j = 0; j < 4; ++j) f[j] = fmaxf(f[j], 0.f);
    }
    if (drop_p > 0.f) {
#pragma unroll
      for (int j = 0; j < 4; ++j) f[j] *= uic_drop_scale(seed, site, (unsigned)(idx_base + row * E + c + j), drop_p, inv_keep);
    }
    T* o = out + row * E + c;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = uic_from_f<T>(f[j]);
  }
}
// The same for bf16 outputs with E % 8 == 0: one WAVE per embedded row (the token is read once per wave, not once per lane;
// no 64-bit divisions), a lane takes 8 consecutive elements -- two 16-byte loads, ONE 16-byte store (the element-wise form
// above stores four 2-byte values per lane and ran at 0.7 TB/s: 48 us for the step's 10880 rows).  Same values, same dropout
// decisions (the hash is per element index).
template <typename TT>
__global__ __launch_bounds__(256) void embed_fwd_rows_bf16_kernel(const TT* __restrict__ table, int V1, int E, const int64_t* __restrict__ tokens,
                                                                  int ldtok, int N, int rows, float drop_p, unsigned seed, unsigned site, size_t idx_base,
                                                                  int relu, bf16_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const float inv_keep = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
  const int e8 = E >> 3;
  for (int row = blockIdx.x * 4 + wave; row < rows; row += gridDim.x * 4) {
    const int t = row / N, n = row - t * N;
    long tok = tokens[(size_t)n * ldtok + t];
    if (tok < 0 || tok >= V1) tok = 0;
    const TT* src = table + (size_t)tok * E;
    bf16_t* dst = out + (size_t)row * E;
    for (int c = lane; c < e8; c += 64) {
      float f[8];
      uic_table_load8(src + c * 8, f);
      if (relu) {
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = fmaxf(f[j], 0.f);
      }
      if (drop_p > 0.f) {
        const unsigned base = (unsigned)(idx_base + (size_t)row * E + c * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] *= uic_drop_scale(seed, site, base + (unsigned)j, drop_p, inv_keep);
      }
      *(uint4*)(dst + c * 8) = uic_pack<bf16_t>(f);
    }
  }
}

// ------------------------------------------------------------------ backward
// The gradient with the T*N positions first bucketed by token -- a STABLE counting sort (positions of one token stay in
// position order), so that every run of the repository is bit for bit the same: histogram per block of EMB_BLK positions ->
// per-token prefix over the blocks -> exclusive scan over the tokens -> fill (slot = bucket start + entries of earlier blocks +
// rank inside the block, counted in LDS).  Equal tokens become neighbours, so embed_gather_kernel can sum them in registers, and
// every table row has ONE owner that stores it (no floating-point atomics anywhere).
// Wave-aggregated counting: a token shared by many lanes of a wave (the padding token at late decode steps, frequent words)
// costs ONE atomic per wave instead of one per lane -- plain per-lane atomics on cnt[0] serialise ~1000 deep.  Two aggregation
// rounds (the tokens of the first two still-active lanes) catch the hot tokens; the remaining lanes use plain atomics.
// (integer adds whose old value nobody reads: the totals do not depend on arrival order)
__device__ __forceinline__ void wave_token_add(int* base, int tok, bool active) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    const unsigned long long todo = __ballot(active);
    if (todo == 0) break;
    const int leader = __ffsll((long long)todo) - 1;
    const int t0 = __shfl(tok, leader, 64);
    const unsigned long long m = __ballot(active && tok == t0);
    if (lane == leader) atomicAdd(base + t0, __popcll(m));
    if (active && tok == t0) active = false;
  }
  if (active) atomicAdd(base + tok, 1);
}
constexpr int EMB_BLK = 1024;                     // positions per histogram block (one workgroup)
// split > 0: the bucket key is (t >= split) * V1 + token -- the positions of decode steps [0, split) are entries [0, split N) of the
// list, those of [split, T) the rest, and each half can be gathered on its own (the later steps' half while BPTT still runs)
__device__ __forceinline__ int embed_key(const int64_t* __restrict__ tokens, int ldtok, int N, int V1, int split, int i) {
  const int t = i / N, n = i - t * N;
  long tok = tokens[(size_t)n * ldtok + t];
  if (tok < 0 || tok >= V1) tok = 0;
  if (split && t >= split) tok += V1;
  return (int)tok;
}
// cntb[b, key] = how many of block b's positions carry `key`
__global__ __launch_bounds__(EMB_BLK) void embed_hist_kernel(const int64_t* __restrict__ tokens, int ldtok, int N, int TS, int V1, int split,
                                                             int nkeys, int* __restrict__ cntb) {
  const int i = blockIdx.x * EMB_BLK + threadIdx.x;          // whole waves enter the aggregation together
  const bool ok = i < TS * N;
  const int key = ok ? embed_key(tokens, ldtok, N, V1, split, i) : 0;
  wave_token_add(cntb + (size_t)blockIdx.x * nkeys, key, ok);
}
// per key: cntb[b, key] <- entries of blocks < b (exclusive prefix over the blocks), cnt[key] <- the key's total
__global__ void embed_block_prefix_kernel(int* __restrict__ cntb, int nkeys, int nblk, int* __restrict__ cnt) {
  const int key = blockIdx.x * blockDim.x + threadIdx.x;
  if (key >= nkeys) return;
  int run = 0;
  for (int b = 0; b < nblk; ++b) {
    const int v = cntb[(size_t)b * nkeys + key];
    cntb[(size_t)b * nkeys + key] = run;
    run += v;
  }
  cnt[key] = run;
}
// single workgroup: off[v] = exclusive prefix of cnt, off[V1] = total.  Rows of 1024 consecutive keys (coalesced loads), each
// scanned by wave shuffles + one LDS hop, with the running total carried from row to row (a thread that walked its own run of
// ~50 consecutive keys -- strided loads, one at a time -- took 72 us on the pivot NMT's 100 008 keys).
__global__ __launch_bounds__(1024) void embed_scan_kernel(const int* __restrict__ cnt, int V1, int* __restrict__ off) {
  // four consecutive keys per thread and trip (one 16-byte load): 4096 keys per trip, 13 trips for the pivot NMT's 50 005 keys
  // (one key per thread: 49 trips of shuffle scan + LDS hop + barrier = 40 us)
  __shared__ int s_wave[2][16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int carry = 0;
  auto load4 = [&](int v0, int (&x)[4]) {
    if (v0 + 3 < V1) {
      const int4 q = *(const int4*)(cnt + v0);          // (cnt is 16-byte aligned and v0 a multiple of 4)
      x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) x[k] = v0 + k < V1 ? cnt[v0 + k] : 0;
    }
  };
  int nxt[4];
  load4((int)threadIdx.x * 4, nxt);
  for (int base = 0, it = 0; base < V1; base += 4096, ++it) {
    const int v0 = base + (int)threadIdx.x * 4;
    const int x[4] = {nxt[0], nxt[1], nxt[2], nxt[3]};
    if (base + 4096 < V1) load4(v0 + 4096, nxt);          // (the next trip's load passes behind this trip's scan)
    const int t4 = (x[0] + x[1]) + (x[2] + x[3]);
    int incl = t4;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    int* sw = s_wave[it & 1];
    if (lane == 63) sw[wv] = incl;
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int t = sw[k];
      if (k < wv) woff += t;
      tot += t;
    }
    int run = carry + woff + incl - t4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (v0 + k < V1) off[v0 + k] = run;
      run += x[k];
    }
    carry += tot;
  }
  if (threadIdx.x == 0) off[V1] = carry;
}
// perm[off[key] + (entries of earlier blocks) + (earlier entries of this block with the same key)] = position
__global__ __launch_bounds__(EMB_BLK) void embed_fill_kernel(const int64_t* __restrict__ tokens, int ldtok, int N, int TS, int V1, int split,
                                                             int nkeys, const int* __restrict__ off, const int* __restrict__ cntb,
                                                             int* __restrict__ perm) {
  __shared__ __attribute__((aligned(16))) int s_key[EMB_BLK];
  const int i = blockIdx.x * EMB_BLK + threadIdx.x;
  const bool ok = i < TS * N;
  const int key = ok ? embed_key(tokens, ldtok, N, V1, split, i) : -1;
  s_key[threadIdx.x] = key;
  __syncthreads();
  if (!ok) return;
  int rank = 0;
  const int full = threadIdx.x >> 2;
  for (int q = 0; q < full; ++q) {                 // (LDS broadcast reads: every lane of a wave asks for the same 16 bytes)
    const int4 v = ((const int4*)s_key)[q];
    rank += (v.x == key) + (v.y == key) + (v.z == key) + (v.w == key);
  }
  for (int j = full * 4; j < (int)threadIdx.x; ++j) rank += s_key[j] == key;
  perm[off[key] + cntb[(size_t)blockIdx.x * nkeys + key] + rank] = i;
}
// One workgroup per CH consecutive entries of the token-bucketed position list: it loads its CH rows up front and sums runs of
// equal tokens in registers.  A bucket that lies wholly inside the workgroup's entries (most tokens occur once or twice) is
// stored straight into the table.  A bucket that straddles workgroups (a hot token -- the padding token 0 owns thousands of
// positions) leaves one partial row per workgroup in `part` ([2, nchunks, E]: plane 0 = the bucket began in an earlier
// workgroup, plane 1 = it begins here and goes on), and embed_gather_finish_kernel lets the workgroup in which the bucket begins
// add them up in list order: one owner per table row, a fixed summation order.
constexpr int EMB_CH = 16;
template <typename T>
__global__ __launch_bounds__(128) void embed_gather_kernel(const float* __restrict__ dxt, const T* __restrict__ xt, const int64_t* __restrict__ tokens,
                                                           int ldtok, int N, int V1, const int* __restrict__ off, const int* __restrict__ perm, int total,
                                                           int E, float inv_keep, long skip_token, float* __restrict__ dtable, int base, int keybase,
                                                           int accum, float* __restrict__ part, int chunk0, size_t plane) {
  // entries [base, total) of the list; keybase = this chunk's first bucket key; accum: the table already holds earlier chunks' sums
  const int start = base + blockIdx.x * EMB_CH;
  const int cnt = min(EMB_CH, total - start);
  __shared__ int s_pos[EMB_CH];
  __shared__ int s_tok[EMB_CH];
  __shared__ int s_b0[EMB_CH], s_b1[EMB_CH];          // the bucket bounds of entry j's token (round 6: fetched here, by the thread that
                                                      // has the token, instead of one dependent load pair per run in the loop below)
  if (threadIdx.x < cnt) {
    const int pos = perm[start + threadIdx.x];
    const int t = pos / N, n = pos - t * N;
    long tok = tokens[(size_t)n * ldtok + t];
    if (tok < 0 || tok >= V1) tok = 0;
    s_pos[threadIdx.x] = pos;
    s_tok[threadIdx.x] = (int)tok;
    s_b0[threadIdx.x] = off[keybase + (int)tok];
    s_b1[threadIdx.x] = off[keybase + (int)tok + 1];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < E / 4; c += blockDim.x) {
    // All 2 x EMB_CH loads of the lane requested before the first is used (round 6): entries behind `cnt` re-read the last valid
    // row and are dropped by a select, the ReLU mask comes from a stand-in (the gradient itself) when there is no xt -- behind
    // `if (j < cnt)` / `if (xt)` hipcc waited for every load at its branch's join: 32 dependent HBM round trips per workgroup.
    float4 g[EMB_CH];
    typename std::conditional<sizeof(T) == 2, uint2, float4>::type a[EMB_CH];
    const char* const xsrc = xt ? (const char*)xt : (const char*)dxt;
    const size_t xscale = xt ? sizeof(T) : sizeof(float);
#pragma unroll
    for (int j = 0; j < EMB_CH; ++j) {
      const size_t o = (size_t)s_pos[j < cnt ? j : cnt - 1] * E + c * 4;
      g[j] = *(const float4*)(dxt + o);
      if constexpr (sizeof(T) == 2) a[j] = *(const uint2*)(xsrc + o * xscale);        // 4 bf16 in one 8-byte load
      else a[j] = *(const float4*)(xsrc + o * xscale);
    }
#pragma unroll
    for (int j = 0; j < EMB_CH; ++j) {
      float a4[4];
      if constexpr (sizeof(T) == 2) {
        a4[0] = __uint_as_float(a[j].x << 16); a4[1] = __uint_as_float(a[j].x & 0xffff0000u);
        a4[2] = __uint_as_float(a[j].y << 16); a4[3] = __uint_as_float(a[j].y & 0xffff0000u);
      } else {
        a4[0] = a[j].x; a4[1] = a[j].y; a4[2] = a[j].z; a4[3] = a[j].w;
      }
      const bool live = j < cnt, relu = xt != nullptr;
      g[j].x = live && !(relu && !(a4[0] > 0.f)) ? g[j].x : 0.f;
      g[j].y = live && !(relu && !(a4[1] > 0.f)) ? g[j].y : 0.f;
      g[j].z = live && !(relu && !(a4[2] > 0.f)) ? g[j].z : 0.f;
      g[j].w = live && !(relu && !(a4[3] > 0.f)) ? g[j].w : 0.f;
    }
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < EMB_CH; ++j) {
      if (j < cnt) {
        acc.x += g[j].x; acc.y += g[j].y; acc.z += g[j].z; acc.w += g[j].w;
        const bool last = j + 1 == cnt || s_tok[j + 1] != s_tok[j];       // uniform over the workgroup
        if (last) {
          if (s_tok[j] != skip_token) {
            const int b0 = s_b0[j], b1 = s_b1[j];
            if (b0 >= start && b1 <= start + cnt) {                        // the whole bucket: this workgroup owns the table row
              float* o = dtable + (size_t)s_tok[j] * E + c * 4;
              float4 v = make_float4(acc.x * inv_keep, acc.y * inv_keep, acc.z * inv_keep, acc.w * inv_keep);
              if (accum) { const float4 q = *(const float4*)o; v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w; }
              *(float4*)o = v;
            } else {
              *(float4*)(part + (b0 >= start ? plane : 0) + (size_t)(chunk0 + blockIdx.x) * E + c * 4) = acc;
            }
          }
          acc = make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
    }
  }
}
// the owner of a straddling bucket (the workgroup whose entries hold the bucket's first position) adds the partial rows and
// stores the table row.  A hot bucket spans hundreds of workgroups (the padding token: ~190 partial rows), so the sum is split
// over EMB_FG groups of 128 threads -- group g takes the partial rows k = g, g + EMB_FG, ... in that order, the groups' sums are
// added in group order through LDS: a fixed summation tree, whatever the timing (one thread walking all rows took 33 us).
constexpr int EMB_FG = 8;
__global__ __launch_bounds__(128 * EMB_FG) void embed_gather_finish_kernel(const int64_t* __restrict__ tokens, int ldtok, int N, int V1,
                                                                           const int* __restrict__ off, const int* __restrict__ perm, int total, int E,
                                                                           float inv_keep, long skip_token, float* __restrict__ dtable, int base, int keybase,
                                                                           int accum, const float* __restrict__ part, int chunk0, size_t plane) {
  __shared__ float4 s_sum[EMB_FG][128];
  const int start = base + blockIdx.x * EMB_CH;
  const int cnt = min(EMB_CH, total - start);
  const int pos = perm[start + cnt - 1];                      // the workgroup's last entry
  const int t = pos / N, n = pos - t * N;
  long tok = tokens[(size_t)n * ldtok + t];
  if (tok < 0 || tok >= V1) tok = 0;
  if (tok == skip_token) return;
  const int b0 = off[keybase + tok], b1 = off[keybase + tok + 1];
  if (b0 < start || b1 <= start + cnt) return;                // began earlier (somebody else's), or ends here (stored by the gather)
  const int c_last = (b1 - 1 - base) / EMB_CH;                // the workgroup that holds the bucket's last entry
  const int g = threadIdx.x >> 7, lt = threadIdx.x & 127;
  for (int c0 = 0; c0 < E / 4; c0 += 128) {
    const int c = c0 + lt;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < E / 4) {
      if (g == 0) acc = *(const float4*)(part + plane + (size_t)(chunk0 + blockIdx.x) * E + c * 4);   // the owner's own tail run
#pragma unroll 8
      for (int k = blockIdx.x + 1 + g; k <= c_last; k += EMB_FG) {
        const float4 q = *(const float4*)(part + (size_t)(chunk0 + k) * E + c * 4);
        acc.x += q.x; acc.y += q.y; acc.z += q.z; acc.w += q.w;
      }
    }
    s_sum[g][lt] = acc;
    __syncthreads();
    if (g == 0 && c < E / 4) {
#pragma unroll
      for (int j = 1; j < EMB_FG; ++j) { const float4 q = s_sum[j][lt]; acc.x += q.x; acc.y += q.y; acc.z += q.z; acc.w += q.w; }
      float* o = dtable + (size_t)tok * E + c * 4;
      float4 v = make_float4(acc.x * inv_keep, acc.y * inv_keep, acc.z * inv_keep, acc.w * inv_keep);
      if (accum) { const float4 q = *(const float4*)o; v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w; }
      *(float4*)o = v;
    }
    __syncthreads();
  }
}

// scratch layout (ints): cnt [nkeys + 1] | off [nkeys + 1] | (unused) [nkeys + 1] | perm [N T] ... then, at offsets that do not
// depend on `split`: cntb [nblk, 2 V1] | part [2, nchunks, E] f32
inline size_t emb_fixed_ints(int N, int T, int V1) { return ((3 * ((size_t)2 * V1 + 1) + (size_t)N * T + 64) + 63) & ~(size_t)63; }
inline int emb_blocks(int total) { return (total + EMB_BLK - 1) / EMB_BLK; }
inline size_t emb_cntb_ints(int N, int T, int V1) { return ((size_t)emb_blocks(N * T) * 2 * V1 + 63) & ~(size_t)63; }
inline size_t emb_chunks(int N, int T) { return (size_t)(N * T) / EMB_CH + 2; }           // two halves, each rounded up

}  // namespace

int uic_embed_fwd_t_launch(int dtype, const void* table, int table_dtype, int V1, int E, const int64_t* tokens, int ldtok, int N, int T,
                           float drop_p, unsigned seed, unsigned site, size_t idx_base, int relu, void* out, hipStream_t s) {
  UIC_REQUIRE(E % 4 == 0, "embed: E=%d must be a multiple of 4", E);
  UIC_REQUIRE(table_dtype == UIC_F32 || (table_dtype == UIC_BF16 && dtype == UIC_BF16), "embed: a bf16 table needs bf16 outputs");
  if (N == 0 || T == 0) return UIC_OK;
  const bool t16 = table_dtype == UIC_BF16;
  if (dtype == UIC_BF16 && E % 8 == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)table & 15) == 0 && (size_t)T * N < ((size_t)1 << 30)) {
    const int rows = T * N;
    int gw = (rows + 3) / 4;
    if (gw > 8192) gw = 8192;
    if (t16) hipLaunchKernelGGL(embed_fwd_rows_bf16_kernel<bf16_t>, dim3(gw), dim3(256), 0, s, (const bf16_t*)table, V1, E, tokens, ldtok, N, rows, drop_p, seed, site, idx_base, relu, (bf16_t*)out);
    else hipLaunchKernelGGL(embed_fwd_rows_bf16_kernel<float>, dim3(gw), dim3(256), 0, s, (const float*)table, V1, E, tokens, ldtok, N, rows, drop_p, seed, site, idx_base, relu, (bf16_t*)out);
    UIC_LAUNCH_CHECK("embed_fwd_rows");
    return UIC_OK;
  }
  const int g = uic_grid_for((size_t)T * N * (E / 4), NT);
  if (t16) {
    hipLaunchKernelGGL((embed_fwd_kernel<bf16_t, bf16_t>), dim3(g), dim3(NT), 0, s, (const bf16_t*)table, V1, E, tokens, ldtok, N, T, drop_p, seed, site, idx_base, relu, (bf16_t*)out);
  } else {
    UIC_DISPATCH_T(dtype,
                   hipLaunchKernelGGL((embed_fwd_kernel<bf16_t, float>), dim3(g), dim3(NT), 0, s, (const float*)table, V1, E, tokens, ldtok, N, T, drop_p, seed, site, idx_base, relu, (bf16_t*)out),
                   hipLaunchKernelGGL((embed_fwd_kernel<float, float>), dim3(g), dim3(NT), 0, s, (const float*)table, V1, E, tokens, ldtok, N, T, drop_p, seed, site, idx_base, relu, (float*)out));
  }
  UIC_LAUNCH_CHECK("embed_fwd");
  return UIC_OK;
}
int uic_embed_fwd_launch(int dtype, const float* table, int V1, int E, const int64_t* tokens, int ldtok, int N, int T,
                         float drop_p, unsigned seed, unsigned site, size_t idx_base, int relu, void* out, hipStream_t s) {
  return uic_embed_fwd_t_launch(dtype, table, UIC_F32, V1, E, tokens, ldtok, N, T, drop_p, seed, site, idx_base, relu, out, s);
}

size_t uic_embed_bwd_sorted_scratch_ints(int N, int T, int V1, int E) {
  return emb_fixed_ints(N, T, V1) + emb_cntb_ints(N, T, V1) + 2 * emb_chunks(N, T) * (size_t)E;
}
// Two halves, so that a caller can do the token bucketing (which needs only the tokens) long before the gradients exist:
//   prepare: zero dtable, histogram -> prefixes -> fill of the position list into `scratch`;   gather: the sums.
// split > 0 (< T): the list holds the positions of decode steps [0, split) first, then those of [split, T); gather then takes one
// of the two halves per call (half = 0 / 1) and adds into the table, so the later steps' share can be gathered before the
// earlier steps' d xt exists.  Both calls must get the same `split` (and the same N, T, V1).
int uic_embed_bwd_sorted_prepare(const int64_t* tokens, int ldtok, int N, int T, int V1, int E, float* dtable, int* scratch, hipStream_t s, int split) {
  UIC_REQUIRE(E % 4 == 0 && scratch, "embed_bwd_sorted: E=%d must be a multiple of 4", E);
  UIC_REQUIRE(split >= 0 && split < (T > 0 ? T : 1), "embed_bwd_sorted: split=%d outside [0, %d)", split, T);
  if (V1 == 0) return UIC_OK;
  const int nkeys = (split > 0 ? 2 : 1) * V1;
  int* cnt = scratch;
  int* off = cnt + (nkeys + 1);
  int* perm = scratch + 3 * (nkeys + 1);
  int* cntb = scratch + emb_fixed_ints(N, T, V1);
  const int total = N * T;
  UIC_TRY(uic_fill_launch(dtable, 0, (size_t)V1 * E * 4, s));
  if (total == 0) return UIC_OK;
  const int nblk = emb_blocks(total);
  UIC_TRY(uic_fill_launch(cntb, 0, (size_t)nblk * nkeys * 4, s));
  hipLaunchKernelGGL(embed_hist_kernel, dim3(nblk), dim3(EMB_BLK), 0, s, tokens, ldtok, N, T, V1, split, nkeys, cntb);
  UIC_LAUNCH_CHECK("embed_hist");
  hipLaunchKernelGGL(embed_block_prefix_kernel, dim3((nkeys + NT - 1) / NT), dim3(NT), 0, s, cntb, nkeys, nblk, cnt);
  UIC_LAUNCH_CHECK("embed_block_prefix");
  hipLaunchKernelGGL(embed_scan_kernel, dim3(1), dim3(1024), 0, s, (const int*)cnt, nkeys, off);
  UIC_LAUNCH_CHECK("embed_scan");
  hipLaunchKernelGGL(embed_fill_kernel, dim3(nblk), dim3(EMB_BLK), 0, s, tokens, ldtok, N, T, V1, split, nkeys, (const int*)off, (const int*)cntb, perm);
  UIC_LAUNCH_CHECK("embed_fill");
  return UIC_OK;
}
int uic_embed_bwd_sorted_gather(int dtype, const float* dxt, const void* xt, const int64_t* tokens, int ldtok, int N, int T,
                                int V1, int E, float drop_p, long skip_token, float* dtable, int* scratch, hipStream_t s,
                                int split, int half) {
  if (V1 == 0 || N * T == 0) return UIC_OK;
  int base = 0, total = N * T, keybase = 0, nkeys = V1, chunk0 = 0;
  if (split > 0) {
    UIC_REQUIRE(split < T && (half == 0 || half == 1), "embed_bwd_sorted_gather: split=%d half=%d (T=%d)", split, half, T);
    nkeys = 2 * V1;
    base = half ? split * N : 0; total = half ? T * N : split * N; keybase = half ? V1 : 0;
    chunk0 = half ? (split * N + EMB_CH - 1) / EMB_CH : 0;
  }
  const int* off = scratch + (nkeys + 1);
  const int* perm = scratch + 3 * (nkeys + 1);
  float* part = (float*)(scratch + emb_fixed_ints(N, T, V1) + emb_cntb_ints(N, T, V1));
  const size_t plane = emb_chunks(N, T) * (size_t)E;
  const float inv_keep = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
  const int gw = (total - base + EMB_CH - 1) / EMB_CH;
  const int accum = split > 0;     // (the table was zeroed by prepare; every bucket has one owner per launch)
  UIC_DISPATCH_T(dtype,
                 hipLaunchKernelGGL(embed_gather_kernel<bf16_t>, dim3(gw), dim3(128), 0, s, dxt, (const bf16_t*)xt, tokens, ldtok, N, V1, off, perm, total, E, inv_keep, skip_token, dtable, base, keybase, accum, part, chunk0, plane),
                 hipLaunchKernelGGL(embed_gather_kernel<float>, dim3(gw), dim3(128), 0, s, dxt, (const float*)xt, tokens, ldtok, N, V1, off, perm, total, E, inv_keep, skip_token, dtable, base, keybase, accum, part, chunk0, plane));
  UIC_LAUNCH_CHECK("embed_gather");
  hipLaunchKernelGGL(embed_gather_finish_kernel, dim3(gw), dim3(128 * EMB_FG), 0, s, tokens, ldtok, N, V1, off, perm, total, E, inv_keep, skip_token, dtable, base, keybase, accum, (const float*)part, chunk0, plane);
  UIC_LAUNCH_CHECK("embed_gather_finish");
  return UIC_OK;
}
// dtable [V1, E] is overwritten.  scratch: uic_embed_bwd_sorted_scratch_ints ints.
int uic_embed_bwd_sorted_launch(int dtype, const float* dxt, const void* xt, const int64_t* tokens, int ldtok, int N, int T,
                                int V1, int E, float drop_p, long skip_token, float* dtable, int* scratch, hipStream_t s) {
  UIC_TRY(uic_embed_bwd_sorted_prepare(tokens, ldtok, N, T, V1, E, dtable, scratch, s, 0));
  return uic_embed_bwd_sorted_gather(dtype, dxt, xt, tokens, ldtok, N, T, V1, E, drop_p, skip_token, dtable, scratch, s, 0, 0);
}
