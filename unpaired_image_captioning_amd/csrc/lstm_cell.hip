// Backward of the LSTM cells' gate math, the element-wise part between two GEMMs of a BPTT step (gfx950): nn.LSTMCell
// (P/models/AttModel.py:434,441) in a scalar and a four-units-per-lane form, and the maxout LSTMCore of the FC model
// (P/models/FCModel_NMT.py:32-50).  The C entries uic_lstm_cell_bwd* / uic_maxout_lstm_cell_bwd (api.hip) fill
// UicLstmBwdParams; the launchers below check it and pick the kernel.
#include "uic_common.h"
#include "uic_host.h"
#include "../../include/uic_hip.h"

namespace {

constexpr int NT = 256;

// Backward of nn.LSTMCell's gate math (P/models/AttModel.py:434,441): gates are stored activated.
template <typename T>
__global__ void lstm_bwd_kernel(const UicLstmBwdParams p) {
  const int H = p.H;
  const size_t total = (size_t)p.M * H;
  const float inv_keep = p.drop_p > 0.f ? 1.f / (1.f - p.drop_p) : 1.f;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
    const int m = (int)(idx / H), u = (int)(idx - (size_t)m * H);
    float dh = 0.f;
    if (p.dh0) {
      float v = p.dh0[(size_t)m * p.lddh0 + u];
      if (p.drop_p > 0.f) v *= uic_drop_scale(p.seed, p.site, (unsigned)idx, p.drop_p, inv_keep);
      dh += v;
    }
    if (p.dh1) dh += p.dh1[(size_t)m * p.lddh1 + u];
    if (p.dh2) dh += p.dh2[(size_t)m * p.lddh2 + u];
    for (int z = 0; z < p.nA; ++z) dh += p.slabA[(size_t)z * p.strideA + (size_t)m * p.ldA + u];
    for (int z = 0; z < p.nB; ++z) dh += p.slabB[(size_t)z * p.strideB + (size_t)m * p.ldB + u];
    const T* G = (const T*)p.gates + (size_t)m * 4 * H + u;
    const float gi = uic_to_f(G[0]), gf = uic_to_f(G[H]), gg = uic_to_f(G[2 * H]), go = uic_to_f(G[3 * H]);
    const float c = p.c[idx];
    const float cp = p.c_prev ? p.c_prev[idx] : 0.f;
    const float tc = uic_tanh<T>(c);                 // (the forward's own tanh: hardware exp on the bf16 path, libm on f32)
    const float dc = p.dc[idx] + dh * go * (1.f - tc * tc);
    const float d_o = dh * tc;
    T* D = (T*)p.dgates + (size_t)m * 4 * H + u;
    D[0] = uic_from_f<T>(dc * gg * gi * (1.f - gi));
    D[H] = uic_from_f<T>(dc * cp * gf * (1.f - gf));
    D[2 * H] = uic_from_f<T>(dc * gi * (1.f - gg * gg));
    D[3 * H] = uic_from_f<T>(d_o * go * (1.f - go));
    p.dc[idx] = dc * gf;
  }
}

// The same for H % 4 == 0 and 16-byte aligned rows: FOUR hidden units per lane, one 16-byte (f32) / 8-byte (bf16) access per
// tensor and gate instead of four scalar ones -- the kernel sits in the BPTT chain 34 times per step and is made of memory
// latency and instruction issue, not of bytes (captioner step 3.775 -> 3.757 ms over six alternations).  Same formulas per element.
// SIMPLE: dh0 and c_prev present, dh1 / dh2 absent -- the two calls of the split BPTT chain (topdown_step.hip); then no load has an
// optional address at all, only the slab stand-ins below.
// LIVE (SIMPLE only; UicLstmBwdParams.row_len): the row's caption length and rank are requested with the operands -- the row is the
// workgroup's, so they are two scalar loads -- and decide, uniformly per workgroup: a row that ended at or before this step writes
// its zero row and leaves; a row whose last step this is drops both slab sums by a select (its slab rows were not written this
// time: the words there may be anything, NaN included -- never a multiply); every other row stores its result twice.
template <typename T, bool SIMPLE, bool LIVE = false>
__global__ __launch_bounds__(NT) void lstm_bwd_vec4_kernel(const UicLstmBwdParams p) {
  const int H = p.H, H4 = H >> 2;
  const int m = blockIdx.y, u4 = blockIdx.x * blockDim.x + threadIdx.x;      // (row from the grid: no division per lane)
  if (u4 >= H4) return;
  const int u = u4 * 4;
  const size_t idx = (size_t)m * H + u;
  int len = 0x7fffffff, rk = 0;
  if constexpr (LIVE) { len = p.row_len[m]; rk = p.rank ? p.rank[m] : 0; }
  const float inv_keep = p.drop_p > 0.f ? 1.f / (1.f - p.drop_p) : 1.f;
  // Every load first, and NONE behind a run-time condition (round 6): an optional source that is absent is read from a valid
  // stand-in address (the d c row) and dropped by a select below.  hipcc waits for a predicated load at the join of its branch --
  // s_waitcnt vmcnt(0) right behind the first optional slab --, which made this link of the BPTT chain two to three serial memory
  // round trips instead of one.  The loads are raw buffer loads: a plain float4 load hipcc is free to split (it made one of them
  // a dwordx3 plus a dword under the dropout branch, with a full drain behind it) or to fold into another one of the same address.
  auto ld4 = [](const float* base, size_t elem) -> float4 {
    const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
        __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0x7fffffff, 0x00020000), (unsigned)(elem * 4), 0, 0));
    return make_float4(v[0], v[1], v[2], v[3]);
  };
  const bool has0 = SIMPLE || p.dh0 != nullptr, has1 = !SIMPLE && p.dh1 != nullptr, has2 = !SIMPLE && p.dh2 != nullptr;
  const bool hascp = SIMPLE || p.c_prev != nullptr;
  const float4 c4 = ld4(p.c, idx);
  const float4 dc4 = ld4(p.dc, idx);
  const float4 d0r = has0 ? ld4(p.dh0, (size_t)m * p.lddh0 + u) : dc4;
  float4 d1r = make_float4(0.f, 0.f, 0.f, 0.f), d2r = d1r;
  if constexpr (!SIMPLE) {
    d1r = ld4(p.dh1 ? p.dh1 : p.dc, p.dh1 ? (size_t)m * p.lddh1 + u : idx);
    d2r = ld4(p.dh2 ? p.dh2 : p.dc, p.dh2 ? (size_t)m * p.lddh2 + u : idx);
  }
  const float4 cpr = ld4(hascp ? p.c_prev : p.c, idx);
  float4 sv[8];
  const int nA = p.nA < 4 ? p.nA : 4, nB = p.nB < 4 ? p.nB : 4;
  {
    const float* bA = nA > 0 ? p.slabA : p.dc;
    const float* bB = nB > 0 ? p.slabB : p.dc;
    const size_t oA = nA > 0 ? (size_t)m * p.ldA + u : idx, oB = nB > 0 ? (size_t)m * p.ldB + u : idx;
    const size_t sA = nA > 0 ? p.strideA : 0, sB = nB > 0 ? p.strideB : 0;
    const int mA = nA > 0 ? nA - 1 : 0, mB = nB > 0 ? nB - 1 : 0;
#pragma unroll
    for (int z = 0; z < 4; ++z) sv[z] = ld4(bA, (size_t)min(z, mA) * sA + oA);
#pragma unroll
    for (int z = 0; z < 4; ++z) sv[4 + z] = ld4(bB, (size_t)min(z, mB) * sB + oB);
  }
  if constexpr (LIVE) {
    if (len <= p.step) {
      // the caption ended before this step: d h, the carried d c (cleared at the loop's start, never written by a row that has not
      // begun: this exit is what keeps it so) and with them the whole row are zero
      T* Z = (T*)p.dgates + (size_t)m * 4 * H + u;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if constexpr (sizeof(T) == 2) *(uint2*)(Z + q * H) = make_uint2(0u, 0u);
        else *(float4*)(Z + q * H) = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      return;
    }
  }
  const bool slabs_on = !LIVE || len > p.step + 1;
  float g[4][4];
  const T* G = (const T*)p.gates + (size_t)m * 4 * H + u;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if constexpr (sizeof(T) == 2) {
      const uint2 w = *(const uint2*)(G + q * H);
      g[q][0] = __uint_as_float(w.x << 16); g[q][1] = __uint_as_float(w.x & 0xffff0000u);
      g[q][2] = __uint_as_float(w.y << 16); g[q][3] = __uint_as_float(w.y & 0xffff0000u);
    } else {
      const float4 w = *(const float4*)(G + q * H);
      g[q][0] = w.x; g[q][1] = w.y; g[q][2] = w.z; g[q][3] = w.w;
    }
  }
  float4 ds = make_float4(0.f, 0.f, 0.f, 0.f);       // split-K partial slabs of two more sources, summed in a fixed order
#pragma unroll
  for (int z = 0; z < 8; ++z) {
    const bool use = (z < 4 ? z < nA : z - 4 < nB) && slabs_on;
    ds.x += use ? sv[z].x : 0.f; ds.y += use ? sv[z].y : 0.f; ds.z += use ? sv[z].z : 0.f; ds.w += use ? sv[z].w : 0.f;
  }
  const float4 cp = hascp ? cpr : make_float4(0.f, 0.f, 0.f, 0.f);
  const float dh0[4] = {d0r.x, d0r.y, d0r.z, d0r.w}, dh1[4] = {d1r.x, d1r.y, d1r.z, d1r.w}, dh2[4] = {d2r.x, d2r.y, d2r.z, d2r.w}, dsl[4] = {ds.x, ds.y, ds.z, ds.w};
  const float cc[4] = {c4.x, c4.y, c4.z, c4.w}, cpv[4] = {cp.x, cp.y, cp.z, cp.w}, dcv[4] = {dc4.x, dc4.y, dc4.z, dc4.w};
  float o[4][4], dcn[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float dh = 0.f;
    if (has0) {
      float v = dh0[k];
      if (p.drop_p > 0.f) v *= uic_drop_scale(p.seed, p.site, (unsigned)(idx + k), p.drop_p, inv_keep);
      dh += v;
    }
    if (has1) dh += dh1[k];
    if (has2) dh += dh2[k];
    dh += dsl[k];
    const float gi = g[0][k], gf = g[1][k], gg = g[2][k], go = g[3][k];
    const float tc = uic_tanh<T>(cc[k]);
    const float dc = dcv[k] + dh * go * (1.f - tc * tc);
    const float d_o = dh * tc;
    o[0][k] = dc * gg * gi * (1.f - gi);
    o[1][k] = dc * cpv[k] * gf * (1.f - gf);
    o[2][k] = dc * gi * (1.f - gg * gg);
    o[3][k] = d_o * go * (1.f - go);
    dcn[k] = dc * gf;
  }
  T* D = (T*)p.dgates + (size_t)m * 4 * H + u;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if constexpr (sizeof(T) == 2) *(uint2*)(D + q * H) = make_uint2(uic_pack_bf16x2(o[q][0], o[q][1]), uic_pack_bf16x2(o[q][2], o[q][3]));
    else *(float4*)(D + q * H) = make_float4(o[q][0], o[q][1], o[q][2], o[q][3]);
  }
  if constexpr (LIVE && sizeof(T) == 2) {
    if (p.dgates_c) {                                  // the same row again, where the step's d x GEMM reads its A operand
      T* Dc = (T*)p.dgates_c + (size_t)rk * 4 * H + u;
#pragma unroll
      for (int q = 0; q < 4; ++q) *(uint2*)(Dc + q * H) = make_uint2(uic_pack_bf16x2(o[q][0], o[q][1]), uic_pack_bf16x2(o[q][2], o[q][3]));
    }
  }
  *(float4*)(p.dc + idx) = make_float4(dcn[0], dcn[1], dcn[2], dcn[3]);
}

// Backward of the maxout LSTMCore gate math (P/models/FCModel_NMT.py:32-50).  gates = (in, forget, out, g, first)
// as stored by the forward GEMM epilogue; the dropout mask applies to the SUM of the incoming dh because the dropped
// next_h is both the output and the recurrent state.
template <typename T>
__global__ void maxout_lstm_bwd_kernel(const UicLstmBwdParams p) {
  const int H = p.H;
  const size_t total = (size_t)p.M * H;
  const float inv_keep = p.drop_p > 0.f ? 1.f / (1.f - p.drop_p) : 1.f;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
    const int m = (int)(idx / H), u = (int)(idx - (size_t)m * H);
    float dh = 0.f;
    if (p.dh0) dh += p.dh0[(size_t)m * p.lddh0 + u];
    if (p.dh1) dh += p.dh1[(size_t)m * p.lddh1 + u];
    if (p.drop_p > 0.f) dh *= uic_drop_scale(p.seed, p.site, (unsigned)idx, p.drop_p, inv_keep);
    const T* G = (const T*)p.gates + (size_t)m * 5 * H + u;
    const float gi = uic_to_f(G[0]), gf = uic_to_f(G[H]), go = uic_to_f(G[2 * H]), gg = uic_to_f(G[3 * H]);
    const bool first = uic_to_f(G[4 * H]) > 0.5f;
    const float c = p.c[idx];
    const float cp = p.c_prev ? p.c_prev[idx] : 0.f;
    const float tc = tanhf(c);
    const float dc = p.dc[idx] + dh * go * (1.f - tc * tc);
    const float dg = dc * gi;
    T* D = (T*)p.dgates + (size_t)m * 5 * H + u;
    D[0] = uic_from_f<T>(dc * gg * gi * (1.f - gi));
    D[H] = uic_from_f<T>(dc * cp * gf * (1.f - gf));
    D[2 * H] = uic_from_f<T>(dh * tc * go * (1.f - go));
    D[3 * H] = uic_from_f<T>(first ? dg : 0.f);
    D[4 * H] = uic_from_f<T>(first ? 0.f : dg);
    p.dc[idx] = dc * gf;
  }
}

}  // namespace

// What both cell-backward launchers check before anything is launched (the kernels take all of it on trust).
static int lstm_bwd_check(const UicLstmBwdParams& p, const char* who) {
  UIC_REQUIRE(p.dc && p.gates && p.c && p.dgates, "%s: null pointer", who);
  UIC_REQUIRE(p.M >= 0 && p.H > 0, "%s: M=%d must be >= 0 and H=%d > 0", who, p.M, p.H);
  UIC_REQUIRE((!p.nA || p.slabA) && (!p.nB || p.slabB) && p.nA >= 0 && p.nB >= 0, "%s: slab sources", who);
  UIC_REQUIRE((!p.dh0 || p.lddh0 >= p.H) && (!p.dh1 || p.lddh1 >= p.H) && (!p.dh2 || p.lddh2 >= p.H) && (!p.nA || p.ldA >= p.H) &&
              (!p.nB || p.ldB >= p.H), "%s: a leading dimension below H=%d (lddh %d %d %d, ldA %d, ldB %d)", who, p.H, p.lddh0, p.lddh1,
              p.lddh2, p.ldA, p.ldB);
  UIC_REQUIRE(p.drop_p >= 0.f && p.drop_p < 1.f, "%s: drop_p=%f outside [0, 1)", who, (double)p.drop_p);
  UIC_REQUIRE(p.row_len || (!p.rank && !p.dgates_c), "%s: rank / dgates_c without row_len", who);
  UIC_REQUIRE(!p.row_len || (p.step >= 0 && (!p.dgates_c || p.rank)), "%s: row_len needs step=%d >= 0, dgates_c needs rank", who, p.step);
  return UIC_OK;
}
int uic_lstm_bwd_launch(const UicLstmBwdParams& p, hipStream_t s, int32_t* kernel_id) {
  UIC_TRY(lstm_bwd_check(p, "lstm_bwd"));
  if (kernel_id) *kernel_id = UIC_LSTM_BWD_SCALAR;
  if (p.M == 0) return UIC_OK;
  auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
  // (small problems -- the pivot NMT's 64 rows -- keep one unit per lane: four times the workgroups, measured faster there)
  const bool vec = (size_t)p.M * p.H >= 65536 && p.H % 4 == 0 && al16(p.dc) && al16(p.c) && (!p.c_prev || al16(p.c_prev)) &&
                   ((uintptr_t)p.gates & 7) == 0 && ((uintptr_t)p.dgates & 7) == 0 && (p.dtype == UIC_BF16 || (al16(p.gates) && al16(p.dgates))) &&
                   (!p.dh0 || (al16(p.dh0) && p.lddh0 % 4 == 0)) && (!p.dh1 || (al16(p.dh1) && p.lddh1 % 4 == 0)) &&
                   (!p.dh2 || (al16(p.dh2) && p.lddh2 % 4 == 0)) && p.M <= 65535 &&
                   p.nA <= 4 && p.nB <= 4 && (!p.nA || (al16(p.slabA) && p.ldA % 4 == 0 && p.strideA % 4 == 0)) &&
                   (!p.nB || (al16(p.slabB) && p.ldB % 4 == 0 && p.strideB % 4 == 0));
  // The vec4 kernel's f32 loads are raw buffer loads: 0x7fffffff records and a 32-bit BYTE offset, so a source whose last byte
  // lies at 2^31 or beyond would be read as zeros (and past 2^32 from a wrapped address).  Such a source keeps the scalar
  // kernel, which addresses with 64 bits.  span: floats from a source's base to the end of its last row (of its last slice).
  auto span = [&](int ld, int n, size_t stride) { return (size_t)(n - 1) * stride + (size_t)(p.M - 1) * (size_t)ld + (size_t)p.H; };
  auto fits = [](size_t floats) { return floats <= (((size_t)1 << 31) - 16) / 4; };
  const bool near = fits((size_t)p.M * p.H) && (!p.dh0 || fits(span(p.lddh0, 1, 0))) && (!p.dh1 || fits(span(p.lddh1, 1, 0))) &&
                    (!p.dh2 || fits(span(p.lddh2, 1, 0))) && (!p.nA || fits(span(p.ldA, p.nA, p.strideA))) &&
                    (!p.nB || fits(span(p.ldB, p.nB, p.strideB)));
  if (vec && near) {
    const int h4 = p.H / 4;
    const int bt = h4 >= NT ? NT : ((h4 + 63) / 64) * 64;
    const dim3 g4((unsigned)((h4 + bt - 1) / bt), (unsigned)p.M);
    const bool simple = p.dh0 && !p.dh1 && !p.dh2 && p.c_prev;
    if (kernel_id) *kernel_id = simple ? UIC_LSTM_BWD_VEC4_SIMPLE : UIC_LSTM_BWD_VEC4;
    UIC_REQUIRE(!p.row_len || (simple && p.dtype == UIC_BF16 && (!p.dgates_c || ((uintptr_t)p.dgates_c & 7) == 0)),
                "lstm_bwd: row_len is taken by the bf16 four-units-per-lane kernel with dh0 and c_prev only");
    if (p.row_len) {
      hipLaunchKernelGGL((lstm_bwd_vec4_kernel<bf16_t, true, true>), g4, dim3(bt), 0, s, p);
    } else if (simple) {
      UIC_DISPATCH_T(p.dtype, hipLaunchKernelGGL((lstm_bwd_vec4_kernel<bf16_t, true>), g4, dim3(bt), 0, s, p),
                     hipLaunchKernelGGL((lstm_bwd_vec4_kernel<float, true>), g4, dim3(bt), 0, s, p));
    } else {
      UIC_DISPATCH_T(p.dtype, hipLaunchKernelGGL((lstm_bwd_vec4_kernel<bf16_t, false>), g4, dim3(bt), 0, s, p),
                     hipLaunchKernelGGL((lstm_bwd_vec4_kernel<float, false>), g4, dim3(bt), 0, s, p));
    }
    UIC_LAUNCH_CHECK("lstm_bwd_vec4");
    return UIC_OK;
  }
  UIC_REQUIRE(!p.row_len, "lstm_bwd: row_len needs the four-units-per-lane kernel (M H >= 65536, H %% 4 == 0, aligned operands below 2^31 bytes)");
  const int g = uic_grid_for((size_t)p.M * p.H, NT);
  UIC_DISPATCH_T(p.dtype, hipLaunchKernelGGL(lstm_bwd_kernel<bf16_t>, dim3(g), dim3(NT), 0, s, p),
                 hipLaunchKernelGGL(lstm_bwd_kernel<float>, dim3(g), dim3(NT), 0, s, p));
  UIC_LAUNCH_CHECK("lstm_bwd");
  return UIC_OK;
}
int uic_maxout_lstm_bwd_launch(const UicLstmBwdParams& p, hipStream_t s) {
  UIC_TRY(lstm_bwd_check(p, "maxout_lstm_bwd"));
  UIC_REQUIRE(!p.dh2 && !p.nA && !p.nB && !p.row_len, "maxout_lstm_bwd: takes dh0 and dh1 only");
  if (p.M == 0) return UIC_OK;
  const int g = uic_grid_for((size_t)p.M * p.H, NT);
  UIC_DISPATCH_T(p.dtype, hipLaunchKernelGGL(maxout_lstm_bwd_kernel<bf16_t>, dim3(g), dim3(NT), 0, s, p),
                 hipLaunchKernelGGL(maxout_lstm_bwd_kernel<float>, dim3(g), dim3(NT), 0, s, p));
  UIC_LAUNCH_CHECK("maxout_lstm_bwd");
  return UIC_OK;
}
