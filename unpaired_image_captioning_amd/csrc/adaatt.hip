// The adaptive-attention captioners (the `adaatt` / `adaattmo` caption models: AdaAtt_lstm, AdaAtt_attention, AdaAttCore,
// AdaAttModel, AdaAttMOModel of P/models/AttModel.py:256-418, 657-667) in eval mode on one MI355X: the teacher-forced forward
// pass (validation loss) and decoding (greedy, sampled, beam).  Training is not built.
//
// Two kernels of their own, each behind a C-ABI operator:
//   adaatt_cell_kernel       the pointwise part of AdaAtt_lstm.forward for one layer (:304-329): gates, tanh or maxout transform,
//                            next_c, next_h and -- on the last layer -- the sentinel sigmoid(n5) tanh(next_c).
//   adaatt_attention_kernel  AdaAtt_attention.forward between its linears (:383-402): scores of the R + 1 slots (slot 0 = the
//                            sentinel), softmax, the mask rule cat([m[:, :1], m]), PI . [fr ; att] + h_out_linear.  One workgroup
//                            owns a row: no atomics, one fixed order of operations.
// Everything else is the project's GEMM (every nn.Linear), its BatchNorm operators (att_embed), embedding.hip, sampling.hip and
// beam.hip -- the last two through decode_internal.h, which owns their buffers, the start of a pass and the beam loop; the beam
// driver here supplies the step and gathers the (h, c) stacks by the surviving parents.  input_encoding_size == rnn_size == att_hid_size == H (the reference's view / cat need it, :385-386).
//
// Per decode step: embedding; ONE GEMM [xt | h_prev] x [w2h ; r_w2h | h2h ; r_h2h]^T (+ the per-row img_fc projection and the
// summed biases, made once per call) -> [rows, (4 + maxout + 1) H]; the cell; fr_linear, fr_embed, ho_linear, ho_embed; the
// attention; tanh(att2h); the logit layer(s).  The beams of an image share its p_att / att (row_div).
#include "uic_common.h"
#include "uic_host.h"
#include "decode_internal.h"
#include "../../include/uic_hip.h"
#include <math.h>
#include <string.h>

namespace {

constexpr int NT = 256;
constexpr float BN_EPS = 1e-5f;                  // nn.BatchNorm1d default
constexpr size_t LDS_MAX = 160 * 1024;

// ------------------------------------------------------------------ the cell (AdaAtt_lstm.forward, :304-329)
struct CellParams {
  int N, H, maxout;
  const float* sums; int ld_sums;
  const float* n5; int ld_n5;
  const float* c_prev; float* c_out;
  void* h_out; int ld_h;
  void* fake_out; int ld_fake;
};

__device__ __forceinline__ void store4(float* p, const float* v) { *(float4*)p = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void store4(bf16_t* p, const float* v) { *(uint2*)p = make_uint2(uic_pack_bf16x2(v[0], v[1]), uic_pack_bf16x2(v[2], v[3])); }
__device__ __forceinline__ void load4(const float* p, float* v) { const float4 x = *(const float4*)p; v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w; }

// Four columns of a row per thread.  Optional operands are read from a clamped address (the `sums` row itself) and dropped by a
// select, so every load is unconditional.
template <typename T>
__global__ __launch_bounds__(NT) void adaatt_cell_kernel(const CellParams p) {
  const int H = p.H, hq = H >> 2;
  const size_t total = (size_t)p.N * hq, stride = (size_t)gridDim.x * NT;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += stride) {
    const size_t n = i / hq;
    const int j = (int)(i - n * hq) * 4;
    const float* s = p.sums + n * p.ld_sums + j;
    float gi[4], gf[4], go[4], ga[4], gb[4], cp[4], q[4];
    load4(s, gi); load4(s + H, gf); load4(s + 2 * H, go); load4(s + 3 * H, ga);
    load4(p.maxout ? s + 4 * H : s + 3 * H, gb);
    load4(p.c_prev ? p.c_prev + n * H + j : s, cp);
    load4(p.n5 ? p.n5 + n * p.ld_n5 + j : s, q);
    float c[4], h[4], f[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float in_gate = uic_sigmoid_t<T>(gi[e]), forget_gate = uic_sigmoid_t<T>(gf[e]), out_gate = uic_sigmoid_t<T>(go[e]);
      const float tr = p.maxout ? fmaxf(ga[e], gb[e]) : uic_tanh<T>(ga[e]);
      c[e] = forget_gate * (p.c_prev ? cp[e] : 0.f) + in_gate * tr;
      const float tc = uic_tanh<T>(c[e]);
      h[e] = out_gate * tc;
      f[e] = uic_sigmoid_t<T>(q[e]) * tc;
    }
    store4(p.c_out + n * H + j, c);
    store4((T*)p.h_out + n * p.ld_h + j, h);
    if (p.fake_out) store4((T*)p.fake_out + n * p.ld_fake + j, f);
  }
}

int cell_launch(int dtype, const CellParams& p, hipStream_t s) {
  UIC_REQUIRE(dtype == UIC_F32 || dtype == UIC_BF16, "adaatt_cell_fwd: bad dtype %d", dtype);
  UIC_REQUIRE(p.N >= 0 && p.H > 0 && p.H % 4 == 0, "adaatt_cell_fwd: N=%d H=%d (H a positive multiple of 4)", p.N, p.H);
  UIC_REQUIRE(p.maxout == 0 || p.maxout == 1, "adaatt_cell_fwd: maxout=%d must be 0 or 1", p.maxout);
  UIC_REQUIRE(p.sums && p.c_out && p.h_out, "adaatt_cell_fwd: null pointer");
  UIC_REQUIRE((p.n5 != nullptr) == (p.fake_out != nullptr), "adaatt_cell_fwd: n5 and fake_out come together (the last layer) or not at all");
  UIC_REQUIRE(p.ld_sums >= (4 + p.maxout) * p.H && p.ld_sums % 4 == 0, "adaatt_cell_fwd: ld_sums=%d below (4 + maxout) H = %d or no multiple of 4",
              p.ld_sums, (4 + p.maxout) * p.H);
  UIC_REQUIRE(p.ld_h >= p.H && p.ld_h % 4 == 0, "adaatt_cell_fwd: ld_h=%d below H=%d or no multiple of 4", p.ld_h, p.H);
  UIC_REQUIRE(!p.n5 || (p.ld_n5 >= p.H && p.ld_n5 % 4 == 0 && p.ld_fake >= p.H && p.ld_fake % 4 == 0),
              "adaatt_cell_fwd: ld_n5=%d / ld_fake=%d below H=%d or no multiple of 4", p.ld_n5, p.ld_fake, p.H);
  const uintptr_t oa = dtype == UIC_BF16 ? 7 : 15;
  UIC_REQUIRE(!((uintptr_t)p.sums & 15) && !((uintptr_t)p.n5 & 15) && !((uintptr_t)p.c_prev & 15) && !((uintptr_t)p.c_out & 15) &&
              !((uintptr_t)p.h_out & oa) && !((uintptr_t)p.fake_out & oa),
              "adaatt_cell_fwd: operands are read and written four elements at a time (f32 16-byte, bf16 8-byte aligned)");
  if (p.N == 0) return UIC_OK;
  const int g = uic_grid_for((size_t)p.N * (p.H / 4), NT);
  if (dtype == UIC_BF16) hipLaunchKernelGGL(adaatt_cell_kernel<bf16_t>, dim3(g), dim3(NT), 0, s, p);
  else hipLaunchKernelGGL(adaatt_cell_kernel<float>, dim3(g), dim3(NT), 0, s, p);
  UIC_LAUNCH_CHECK("adaatt_cell");
  return UIC_OK;
}

// ------------------------------------------------------------------ the attention (AdaAtt_attention.forward, :383-402)
struct AttParams {
  int N, R, A, H, div;
  const float* fr_e; const float* hl_e; int ld_q;
  const void* fr; const void* hl; int ld_x;
  const void* p_att; const void* att;
  const float* w; const float* b;
  const float* mask; int ld_mask;
  float* PI; void* out; int ld_out;
};
__host__ __device__ inline size_t att_slots_padded(int R) { return ((size_t)R + 1 + 3) & ~(size_t)3; }
inline size_t att_lds_bytes(int R, int A, int H) { return (3 * (size_t)A + att_slots_padded(R) + (NT / 64) * (size_t)H) * 4; }

// grid (N).  LDS: hl_e [A], fr_e [A], w [A], the R + 1 scores / weights, and per wave a partial output row [H].
//   scores   wave v takes slots v, v + 4, ...; its lanes stride over A in 16-byte pieces of the p_att row (slot 0 reads row 0 too
//            -- a clamped address -- and selects fr_e instead), one wave reduction per slot.
//   softmax  wave 0 alone: maximum, sum, the mask and its renormalisation -- one order of operations.
//   output   wave v sums PI_r att[r] over r = v, v + 4, ... for the row pieces its lanes hold; the four partial rows are added in
//            the order 0, 1, 2, 3 with PI_0 fr and hl.
template <typename T>
__global__ __launch_bounds__(NT) void adaatt_attention_kernel(const AttParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int VN = uic_vec<T>::N;
  const int R = p.R, A = p.A, H = p.H;
  float* sH = smem;
  float* sF = sH + A;
  float* sW = sF + A;
  float* sE = sW + A;
  float* sAcc = sE + att_slots_padded(R);
  const int n = blockIdx.x, img = n / p.div;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int a = tid; a < A; a += NT) {
    sH[a] = p.hl_e[(size_t)n * p.ld_q + a];
    sF[a] = p.fr_e[(size_t)n * p.ld_q + a];
    sW[a] = p.w[a];
  }
  __syncthreads();
  const float bias = p.b[0];
  const T* pa = (const T*)p.p_att + (size_t)img * R * A;
  for (int s = wave; s <= R; s += NT / 64) {
    const T* row = pa + (size_t)(s > 0 ? s - 1 : 0) * A;
    float acc = 0.f;
    for (int c = lane; c < A / VN; c += 64) {
      float f[8];
      uic_unpack<T>(*(const uint4*)(row + c * VN), f);
#pragma unroll
      for (int e = 0; e < VN; ++e) {
        const int a = c * VN + e;
        acc += sW[a] * uic_tanh<T>((s == 0 ? sF[a] : f[e]) + sH[a]);
      }
    }
    acc = uic_wave_sum(acc);
    if (lane == 0) sE[s] = acc + bias;
  }
  __syncthreads();
  if (wave == 0) {
    float mx = -INFINITY;
    for (int s = lane; s <= R; s += 64) mx = fmaxf(mx, sE[s]);
    mx = uic_wave_max(mx);
    float sum = 0.f;
    for (int s = lane; s <= R; s += 64) sum += expf(sE[s] - mx);
    sum = uic_wave_sum(sum);
    // PI = softmax; with a mask PI * cat([m[:, :1], m]) / its sum (:394-397): slot 0 and slot 1 both take m_0
    const float* mrow = p.mask ? p.mask + (size_t)img * p.ld_mask : nullptr;
    float msum = 0.f;
    for (int s = lane; s <= R; s += 64) {
      float v = expf(sE[s] - mx) / sum;
      if (mrow) v *= mrow[s > 0 ? s - 1 : 0];
      sE[s] = v;
      msum += v;
    }
    msum = uic_wave_sum(msum);
    for (int s = lane; s <= R; s += 64) {
      const float v = mrow ? sE[s] / msum : sE[s];
      sE[s] = v;
      p.PI[(size_t)n * (R + 1) + s] = v;
    }
  }
  __syncthreads();
  const T* av = (const T*)p.att + (size_t)img * R * H;
  for (int c = lane; c < H / VN; c += 64) {
    float acc[VN];
#pragma unroll
    for (int e = 0; e < VN; ++e) acc[e] = 0.f;
    for (int r = wave; r < R; r += NT / 64) {
      const float pi = sE[r + 1];
      float f[8];
      uic_unpack<T>(*(const uint4*)(av + (size_t)r * H + c * VN), f);
#pragma unroll
      for (int e = 0; e < VN; ++e) acc[e] += pi * f[e];
    }
#pragma unroll
    for (int e = 0; e < VN; ++e) sAcc[wave * H + c * VN + e] = acc[e];
  }
  __syncthreads();
  const float pi0 = sE[0];
  const T* fr = (const T*)p.fr + (size_t)n * p.ld_x;
  const T* hl = (const T*)p.hl + (size_t)n * p.ld_x;
  T* out = (T*)p.out + (size_t)n * p.ld_out;
  for (int c = tid; c < H / VN; c += NT) {
    float f[8], g[8], o[8];
    uic_unpack<T>(*(const uint4*)(fr + c * VN), f);
    uic_unpack<T>(*(const uint4*)(hl + c * VN), g);
#pragma unroll
    for (int e = 0; e < VN; ++e) {
      const int j = c * VN + e;
      float v = pi0 * f[e];
#pragma unroll
      for (int k = 0; k < NT / 64; ++k) v += sAcc[k * H + j];
      o[e] = v + g[e];
    }
    *(uint4*)(out + c * VN) = uic_pack<T>(o);
  }
}

int attention_launch(int dtype, const AttParams& p, hipStream_t s) {
  UIC_REQUIRE(dtype == UIC_F32 || dtype == UIC_BF16, "adaatt_attention_fwd: bad dtype %d", dtype);
  const int vec = dtype == UIC_BF16 ? 8 : 4;
  UIC_REQUIRE(p.N >= 0 && p.R >= 1 && p.A >= 1 && p.H >= 1, "adaatt_attention_fwd: bad sizes N=%d R=%d A=%d H=%d", p.N, p.R, p.A, p.H);
  UIC_REQUIRE(p.A % vec == 0 && p.H % vec == 0, "adaatt_attention_fwd: A=%d and H=%d must be multiples of %d", p.A, p.H, vec);
  UIC_REQUIRE(p.div >= 1 && p.N % p.div == 0, "adaatt_attention_fwd: row_div=%d does not divide N=%d", p.div, p.N);
  UIC_REQUIRE(p.fr_e && p.hl_e && p.fr && p.hl && p.p_att && p.att && p.w && p.b && p.PI && p.out, "adaatt_attention_fwd: null pointer");
  UIC_REQUIRE(p.ld_q >= p.A && p.ld_x >= p.H && p.ld_out >= p.H && (!p.mask || p.ld_mask >= p.R),
              "adaatt_attention_fwd: a leading dimension is below its width (ld_q=%d A=%d, ld_x=%d ld_out=%d H=%d, ld_mask=%d R=%d)", p.ld_q, p.A,
              p.ld_x, p.ld_out, p.H, p.ld_mask, p.R);
  UIC_REQUIRE(p.ld_x % vec == 0 && p.ld_out % vec == 0 && !((uintptr_t)p.fr & 15) && !((uintptr_t)p.hl & 15) && !((uintptr_t)p.out & 15) &&
              !((uintptr_t)p.p_att & 15) && !((uintptr_t)p.att & 15),
              "adaatt_attention_fwd: p_att, att, fr, hl and out are read and written 16 bytes at a time (16-byte aligned, ld_x / ld_out multiples of %d)", vec);
  const size_t lds = att_lds_bytes(p.R, p.A, p.H);
  UIC_REQUIRE(lds <= LDS_MAX, "adaatt_attention_fwd: %zu B of LDS (4 (3A + R + 1 + 4H)) exceed 160 KB", lds);
  if (p.N == 0) return UIC_OK;
  static bool configured = false;
  if (!configured) {
    UIC_TRY(uic_check_hip(hipFuncSetAttribute((const void*)adaatt_attention_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX),
                          "hipFuncSetAttribute(adaatt_attention f32)"));
    UIC_TRY(uic_check_hip(hipFuncSetAttribute((const void*)adaatt_attention_kernel<bf16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX),
                          "hipFuncSetAttribute(adaatt_attention bf16)"));
    configured = true;
  }
  if (dtype == UIC_BF16) hipLaunchKernelGGL(adaatt_attention_kernel<bf16_t>, dim3(p.N), dim3(NT), lds, s, p);
  else hipLaunchKernelGGL(adaatt_attention_kernel<float>, dim3(p.N), dim3(NT), lds, s, p);
  UIC_LAUNCH_CHECK("adaatt_attention");
  return UIC_OK;
}

// ------------------------------------------------------------------ small kernels of the sequencers
// pack_wrapper's lengths (AttModel.py:44-53: att_masks.sum(1))
__global__ void row_len_kernel(const float* __restrict__ att_masks, int N, int R, int* __restrict__ row_len) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  int len = 0;
  for (int r = 0; r < R; ++r) len += (int)att_masks[(size_t)n * R + r];
  row_len[n] = len;
}
// out[i] = a[i] + b[i] + c[i] (b, c optional): the bias rows of the stacked gate GEMMs
__global__ void bias_sum_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c, int n, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = a[i] + (b ? b[i] : 0.f) + (c ? c[i] : 0.f);
}
int bias_sum(const float* a, const float* b, const float* c, int n, float* out, hipStream_t s) {
  hipLaunchKernelGGL(bias_sum_kernel, dim3((n + NT - 1) / NT), dim3(NT), 0, s, a, b, c, n, out);
  UIC_LAUNCH_CHECK("adaatt_bias_sum");
  return UIC_OK;
}

// C = act(A[M, K] W[N, K]^T + bias)
int lin(int dt, int M, int N, int K, const void* A, const void* W, void* C, int ldc, const float* bias, int flags, hipStream_t s) {
  UicGemmParams g = gemm_base(dt, M, N);
  add_seg(g, A, K, W, K, K);
  g.C = C; g.ldc = ldc; g.bias = bias; g.flags = flags;
  return uic_gemm_launch(g, s);
}

struct Layout {
  // operand-dtype weight copies, rebuilt by every call (the f32 masters themselves in f32 runs where no stacking is needed)
  const void* fc_w; const void* att_w; const void* ctx_w; const void* frl_w; const void* fre_w; const void* hol_w; const void* hoe_w;
  const void* a2h_w; const void* logit_w; const void* logit_h_w[UIC_MAX_LOGIT_LAYERS - 1];
  void* c_fc_w; void* c_att_w; void* c_ctx_w; void* c_frl_w; void* c_fre_w; void* c_hol_w; void* c_hoe_w; void* c_a2h_w; void* c_logit_w;
  void* c_logit_h_w[UIC_MAX_LOGIT_LAYERS - 1];
  float* att_beff;                    // use_bn: b' = att_b + att_w bn0_beta
  void* Wx[UIC_ADAATT_MAX_LAYERS];    // layer 0 [rows_0, H] = [w2h ; r_w2h], layer 1 [rows_1, H] = [i2h.0 ; r_i2h]
  void* Wh[UIC_ADAATT_MAX_LAYERS];    // [rows_l, H] = [h2h.l ; r_h2h]; rows_l = (4 + maxout) H, + H on the last layer
  void* Wv;                           // [rows_0, H] = [v2h ; r_v2h]
  float* bsum[UIC_ADAATT_MAX_LAYERS]; // the summed biases of a layer's stacked rows
  // features
  int* row_len; float* bn_stat0; float* bn_stat4; void* xhat; float* ybn; void* fcT;
  void* fcp; void* attp; void* patt;  // fc' [N, H], att' [N R, H], p_att [N R, H]
  float* fcproj; float* fcproj_rows;  // [N, rows_0] = fc' Wv^T + bsum_0, and its copy per decode row (beam > 1)
  // one step over `rows` rows
  void* xt; float* sums; void* h[2][UIC_ADAATT_MAX_LAYERS]; float* c[2][UIC_ADAATT_MAX_LAYERS];
  void* fake; void* fr; void* hl; float* fr_e; float* hl_e; float* PI; void* aout; void* ah; void* lh[UIC_MAX_LOGIT_LAYERS - 1];
  float* logits;                      // [max(rows, (S - 1) N), V1p]
  SampleScratch smp;                  // rows = N beam, step capacity S
  BeamScratch beam;                   // the same rows, a done_count entry per image, step capacity S
  size_t total;
};

inline int gate_rows(const uic_adaatt_dims& d, int l) { return (4 + d.maxout + (l == d.layers - 1 ? 1 : 0)) * d.H; }

Layout make_layout(const uic_adaatt_dims& d, const uic_adaatt_weights* w, void* ws) {
  Layout L;
  memset(&L, 0, sizeof(L));
  Bump b{(char*)ws, 0};
  const size_t Sz = uic_dtype_size(d.dtype), N = d.N, R = d.R, H = d.H, D = d.D, Dfc = d.Dfc, V1 = d.V1, V1p = vpad(V1), S = d.S;
  const size_t rows = N * (size_t)d.beam, NR = N * R, G1 = (4 + d.maxout + 1) * H;
  const bool bf = d.dtype == UIC_BF16;
  L.c_fc_w = b.take(H * Dfc * Sz); L.c_att_w = b.take(H * D * Sz); L.c_ctx_w = b.take(H * H * Sz);
  L.c_frl_w = b.take(H * H * Sz); L.c_fre_w = b.take(H * H * Sz); L.c_hol_w = b.take(H * H * Sz); L.c_hoe_w = b.take(H * H * Sz);
  L.c_a2h_w = b.take(H * H * Sz); L.c_logit_w = b.take(V1 * H * Sz);
  for (int l = 0; l + 1 < d.logit_layers; ++l) L.c_logit_h_w[l] = b.take(H * H * Sz);
  L.att_beff = (float*)b.take(H * 4);
  for (int l = 0; l < d.layers; ++l) {
    L.Wx[l] = b.take(G1 * H * Sz);
    L.Wh[l] = b.take(G1 * H * Sz);
    L.bsum[l] = (float*)b.take(G1 * 4);
  }
  L.Wv = b.take(G1 * H * Sz);
  const bool own = bf || !w;            // (w == null: a size query)
  L.fc_w = own ? L.c_fc_w : (const void*)w->fc_w;
  L.att_w = own || d.use_bn ? L.c_att_w : (const void*)w->att_w;
  L.ctx_w = own ? L.c_ctx_w : (const void*)w->ctx2att_w;
  L.frl_w = own ? L.c_frl_w : (const void*)w->fr_linear_w;
  L.fre_w = own ? L.c_fre_w : (const void*)w->fr_embed_w;
  L.hol_w = own ? L.c_hol_w : (const void*)w->ho_linear_w;
  L.hoe_w = own ? L.c_hoe_w : (const void*)w->ho_embed_w;
  L.a2h_w = own ? L.c_a2h_w : (const void*)w->att2h_w;
  L.logit_w = own ? L.c_logit_w : (const void*)w->logit_w;
  for (int l = 0; l + 1 < d.logit_layers; ++l) L.logit_h_w[l] = own ? L.c_logit_h_w[l] : (const void*)w->logit_h_w[l];
  L.row_len = (int*)b.take(N * 4);
  L.bn_stat0 = (float*)b.take(2 * D * 4);
  L.bn_stat4 = (float*)b.take(2 * H * 4);
  L.xhat = b.take(NR * D * Sz);
  L.ybn = (float*)b.take(d.use_bn == 2 ? NR * H * 4 : 0);
  L.fcT = b.take(N * Dfc * Sz);
  L.fcp = b.take(N * H * Sz);
  L.attp = b.take(NR * H * Sz);
  L.patt = b.take(NR * H * Sz);
  L.fcproj = (float*)b.take(N * G1 * 4);
  L.fcproj_rows = (float*)b.take(rows * G1 * 4);
  L.xt = b.take(rows * H * Sz);
  L.sums = (float*)b.take(rows * G1 * 4);
  for (int i = 0; i < 2; ++i)
    for (int l = 0; l < d.layers; ++l) {
      L.h[i][l] = b.take(rows * H * Sz);
      L.c[i][l] = (float*)b.take(rows * H * 4);
    }
  L.fake = b.take(rows * H * Sz); L.fr = b.take(rows * H * Sz); L.hl = b.take(rows * H * Sz);
  L.fr_e = (float*)b.take(rows * H * 4); L.hl_e = (float*)b.take(rows * H * 4);
  L.PI = (float*)b.take(rows * (R + 1) * 4);
  L.aout = b.take(rows * H * Sz); L.ah = b.take(rows * H * Sz);
  for (int l = 0; l + 1 < d.logit_layers; ++l) L.lh[l] = b.take(rows * H * Sz);
  const size_t lrows = rows > (S - 1) * N ? rows : (S - 1) * N;
  L.logits = (float*)b.take(lrows * V1p * 4);
  L.smp.carve(b, rows, S);
  L.beam.carve(b, rows, N, S);
  L.total = (b.off + 255) & ~(size_t)255;
  return L;
}

int check_dims(const uic_adaatt_dims* d) {
  UIC_REQUIRE(d != nullptr, "adaatt: null dims");
  UIC_REQUIRE(d->dtype == UIC_F32 || d->dtype == UIC_BF16, "adaatt: bad dtype %d", d->dtype);
  UIC_REQUIRE(d->N > 0 && d->R > 0 && d->S >= 2 && d->V1 > 1, "adaatt: bad sizes N=%d R=%d S=%d V1=%d", d->N, d->R, d->S, d->V1);
  UIC_REQUIRE(d->D > 0 && d->D % 8 == 0 && d->Dfc > 0 && d->Dfc % 8 == 0 && d->H > 0 && d->H % 8 == 0, "adaatt: D=%d Dfc=%d H=%d must be multiples of 8",
              d->D, d->Dfc, d->H);
  UIC_REQUIRE(d->layers >= 1 && d->layers <= UIC_ADAATT_MAX_LAYERS, "adaatt: %d layers (1..%d)", d->layers, UIC_ADAATT_MAX_LAYERS);
  UIC_REQUIRE(d->maxout == 0 || d->maxout == 1, "adaatt: maxout=%d must be 0 (adaatt) or 1 (adaattmo)", d->maxout);
  UIC_REQUIRE(d->logit_layers >= 1 && d->logit_layers <= UIC_MAX_LOGIT_LAYERS, "adaatt: logit_layers=%d outside [1, %d]", d->logit_layers, UIC_MAX_LOGIT_LAYERS);
  UIC_REQUIRE(d->use_bn >= 0 && d->use_bn <= 2, "adaatt: use_bn=%d", d->use_bn);
  UIC_REQUIRE(d->beam >= 1 && d->beam <= UIC_BEAM_MAX, "adaatt: beam=%d outside [1, %d]", d->beam, UIC_BEAM_MAX);
  UIC_REQUIRE(att_lds_bytes(d->R, d->H, d->H) <= LDS_MAX, "adaatt: R=%d regions at H=%d need more than 160 KB of LDS in the attention", d->R, d->H);
  return UIC_OK;
}

int check_call(const uic_adaatt_dims* d, const uic_adaatt_weights* w, const void* ws, const char* who) {
  UIC_TRY(check_dims(d));
  UIC_REQUIRE(w && ws, "%s: null pointer", who);
  UIC_REQUIRE(w->embed_w && w->fc_w && w->fc_b && w->att_w && w->att_b && w->logit_w && w->logit_b && w->ctx2att_w && w->ctx2att_b && w->w2h_w &&
              w->w2h_b && w->v2h_w && w->v2h_b && w->r_h2h_w && w->r_h2h_b && w->fr_linear_w && w->fr_linear_b && w->fr_embed_w && w->fr_embed_b &&
              w->ho_linear_w && w->ho_linear_b && w->ho_embed_w && w->ho_embed_b && w->alpha_w && w->alpha_b && w->att2h_w && w->att2h_b,
              "%s: null weight", who);
  for (int l = 0; l < d->layers; ++l) UIC_REQUIRE(w->h2h_w[l] && w->h2h_b[l], "%s: null h2h.%d", who, l);
  for (int l = 0; l + 1 < d->layers; ++l) UIC_REQUIRE(w->i2h_w[l] && w->i2h_b[l], "%s: null i2h.%d", who, l);
  if (d->layers == 1) UIC_REQUIRE(w->r_w2h_w && w->r_w2h_b && w->r_v2h_w && w->r_v2h_b, "%s: one layer needs r_w2h and r_v2h", who);
  else UIC_REQUIRE(w->r_i2h_w && w->r_i2h_b, "%s: %d layers need r_i2h", who, d->layers);
  for (int l = 0; l + 1 < d->logit_layers; ++l) UIC_REQUIRE(w->logit_h_w[l] && w->logit_h_b[l], "%s: null hidden logit block %d", who, l);
  if (d->use_bn) UIC_REQUIRE(w->att_bn0_w && w->att_bn0_b && w->att_bn0_rm && w->att_bn0_rv, "%s: use_bn=%d needs the att_embed.0 BatchNorm tensors", who, d->use_bn);
  if (d->use_bn == 2) UIC_REQUIRE(w->att_bn4_w && w->att_bn4_b && w->att_bn4_rm && w->att_bn4_rv, "%s: use_bn=2 needs the att_embed.4 BatchNorm tensors", who);
  return UIC_OK;
}

struct Ada {
  const uic_adaatt_dims& d; const uic_adaatt_weights* w; Layout L; hipStream_t s;
  int dt, N, R, H, V1, V1p, GH;
  size_t Sz;
  Ada(const uic_adaatt_dims& d_, const uic_adaatt_weights* w_, void* ws, hipStream_t s_) : d(d_), w(w_), L(make_layout(d_, w_, ws)), s(s_) {
    dt = d.dtype; N = d.N; R = d.R; H = d.H; V1 = d.V1; V1p = (int)vpad(d.V1); GH = (4 + d.maxout) * d.H; Sz = uic_dtype_size(dt);
  }
  int cast(const float* src, void* dst, size_t n) const { return uic_cast_f32_launch(dt, src, dst, n, s); }

  // the operand-dtype copies, the stacked gate matrices and their summed biases
  int refresh() const {
    const size_t HH = (size_t)H * H, GHH = (size_t)GH * H;
    if (d.use_bn) UIC_TRY(uic_bn_fold_weight_launch(dt, w->att_w, w->att_bn0_w, w->att_bn0_b, w->att_b, H, d.D, L.c_att_w, L.att_beff, s));
    else if (dt == UIC_BF16) UIC_TRY(cast(w->att_w, L.c_att_w, (size_t)H * d.D));
    if (dt == UIC_BF16) {
      UIC_TRY(cast(w->fc_w, L.c_fc_w, (size_t)H * d.Dfc));
      UIC_TRY(cast(w->ctx2att_w, L.c_ctx_w, HH));
      UIC_TRY(cast(w->fr_linear_w, L.c_frl_w, HH));
      UIC_TRY(cast(w->fr_embed_w, L.c_fre_w, HH));
      UIC_TRY(cast(w->ho_linear_w, L.c_hol_w, HH));
      UIC_TRY(cast(w->ho_embed_w, L.c_hoe_w, HH));
      UIC_TRY(cast(w->att2h_w, L.c_a2h_w, HH));
      UIC_TRY(cast(w->logit_w, L.c_logit_w, (size_t)V1 * H));
      for (int l = 0; l + 1 < d.logit_layers; ++l) UIC_TRY(cast(w->logit_h_w[l], L.c_logit_h_w[l], HH));
    }
    const int last = d.layers - 1;
    // layer 0: [w2h ; r_w2h], [h2h.0 ; r_h2h], [v2h ; r_v2h]; the r_ rows only when it is the last layer (:323-328)
    UIC_TRY(cast(w->w2h_w, L.Wx[0], GHH));
    UIC_TRY(cast(w->h2h_w[0], L.Wh[0], GHH));
    UIC_TRY(cast(w->v2h_w, L.Wv, GHH));
    UIC_TRY(bias_sum(w->w2h_b, w->v2h_b, w->h2h_b[0], GH, L.bsum[0], s));
    if (last == 0) {
      UIC_TRY(cast(w->r_w2h_w, offw(L.Wx[0], GHH, dt), HH));
      UIC_TRY(cast(w->r_h2h_w, offw(L.Wh[0], GHH, dt), HH));
      UIC_TRY(cast(w->r_v2h_w, offw(L.Wv, GHH, dt), HH));
      UIC_TRY(bias_sum(w->r_w2h_b, w->r_v2h_b, w->r_h2h_b, H, L.bsum[0] + GH, s));
    }
    for (int l = 1; l < d.layers; ++l) {
      UIC_TRY(cast(w->i2h_w[l - 1], L.Wx[l], GHH));
      UIC_TRY(cast(w->h2h_w[l], L.Wh[l], GHH));
      UIC_TRY(bias_sum(w->i2h_b[l - 1], w->h2h_b[l], nullptr, GH, L.bsum[l], s));
      if (l == last) {
        UIC_TRY(cast(w->r_i2h_w, offw(L.Wx[l], GHH, dt), HH));
        UIC_TRY(cast(w->r_h2h_w, offw(L.Wh[l], GHH, dt), HH));
        UIC_TRY(bias_sum(w->r_i2h_b, w->r_h2h_b, nullptr, H, L.bsum[l] + GH, s));
      }
    }
    return UIC_OK;
  }

  // layer 0's share of img_fc, once per call: fcproj = fc' [v2h ; r_v2h]^T + the summed biases, one row per decode row
  int fc_projection(const void* fcp, int n_rows, int rep) const {
    const int r0 = gate_rows(d, 0);
    UIC_TRY(lin(dt, n_rows, r0, H, fcp, L.Wv, L.fcproj, r0, L.bsum[0], UIC_GEMM_OUT_F32, s));
    if (rep > 1) UIC_TRY(uic_expand_rows_launch(UIC_F32, L.fcproj, L.fcproj_rows, n_rows, rep, (size_t)r0, s));
    return UIC_OK;
  }

  // _prepare_feature (AttModel.py:107-117) in eval mode: fc' = relu(fc_embed(fc)), att' = att_embed on the valid regions (padded
  // regions exact zeros, as pack_wrapper leaves them), p_att = ctx2att(att')
  int prepare(const float* fc_feats, const float* att_feats, const float* att_masks) const {
    const int NR = N * R, D = d.D;
    const int* row_len = nullptr;
    if (att_masks) {
      hipLaunchKernelGGL(row_len_kernel, dim3((N + 63) / 64), dim3(64), 0, s, att_masks, N, R, L.row_len);
      UIC_LAUNCH_CHECK("adaatt_row_len");
      row_len = L.row_len;
    }
    const void* fc_in = fc_feats;
    if (dt == UIC_BF16) {
      UIC_TRY(cast(fc_feats, L.fcT, (size_t)N * d.Dfc));
      fc_in = L.fcT;
    }
    UIC_TRY(lin(dt, N, H, d.Dfc, fc_in, L.fc_w, L.fcp, H, w->fc_b, UIC_GEMM_RELU, s));
    const void* att_in = att_feats;
    if (d.use_bn) {   // BatchNorm1d(D), running statistics; its affine part is folded into the Linear's copy (refresh)
      UIC_TRY(uic_bn_stats_running_launch(w->att_bn0_rm, w->att_bn0_rv, D, BN_EPS, L.bn_stat0, s));
      UIC_TRY(uic_bn_apply_launch(UIC_F32, dt, att_feats, NR, R, D, row_len, L.bn_stat0, nullptr, nullptr, 0, L.xhat, s));
      att_in = L.xhat;
    } else if (dt == UIC_BF16) {
      UIC_TRY(cast(att_feats, L.xhat, (size_t)NR * D));
      att_in = L.xhat;
    }
    {
      UicGemmParams g = gemm_base(dt, NR, H);
      add_seg(g, att_in, D, L.att_w, D, D);
      g.C = d.use_bn == 2 ? (void*)L.ybn : L.attp; g.ldc = H; g.bias = d.use_bn ? L.att_beff : w->att_b;
      g.flags = UIC_GEMM_RELU | (d.use_bn == 2 ? UIC_GEMM_OUT_F32 : 0);
      if (row_len) { g.row_len = row_len; g.R = R; }
      UIC_TRY(uic_gemm_launch(g, s));
    }
    if (d.use_bn == 2) {
      UIC_TRY(uic_bn_stats_running_launch(w->att_bn4_rm, w->att_bn4_rv, H, BN_EPS, L.bn_stat4, s));
      UIC_TRY(uic_bn_apply_launch(UIC_F32, dt, L.ybn, NR, R, H, row_len, L.bn_stat4, w->att_bn4_w, w->att_bn4_b, 1, L.attp, s));
    }
    UIC_TRY(lin(dt, NR, H, H, L.attp, L.ctx_w, L.patt, H, w->ctx2att_b, 0, s));
    return fc_projection(L.fcp, N, d.beam);
  }

  int state_zero(int rows) const {
    for (int l = 0; l < d.layers; ++l) {
      UIC_TRY(uic_fill_launch(L.h[0][l], 0, (size_t)rows * H * Sz, s));
      UIC_TRY(uic_fill_launch(L.c[0][l], 0, (size_t)rows * H * 4, s));
    }
    return UIC_OK;
  }

  // One get_logprobs_state (AttModel.py:158-165) over `rows` rows: the embedding of tok[n * ld_tok], AdaAttCore (:415-418), the logit
  // layer(s) into `logits` [rows, V1p] f32.  State slot cur -> nxt; the rows of image k are k div .. k div + div - 1.
  int step(int rows, int div, const int64_t* tok, int ld_tok, const float* mask, int cur, int nxt, float* logits) const {
    UIC_TRY(uic_embed_fwd_launch(dt, w->embed_w, V1, H, tok, ld_tok, rows, 1, 0.f, 0, 0, 0, 1, L.xt, s));
    const float* fcproj = div > 1 ? L.fcproj_rows : L.fcproj;
    const int last = d.layers - 1;
    for (int l = 0; l < d.layers; ++l) {
      const int rl = gate_rows(d, l);
      UicGemmParams g = gemm_base(dt, rows, rl);
      add_seg(g, l == 0 ? L.xt : L.h[nxt][l - 1], H, L.Wx[l], H, H);
      add_seg(g, L.h[cur][l], H, L.Wh[l], H, H);
      g.C = L.sums; g.ldc = rl; g.flags = UIC_GEMM_OUT_F32;
      if (l == 0) { g.addend = fcproj; g.add_mod = rows; g.ld_add = rl; }
      else g.bias = L.bsum[l];
      UIC_TRY(uic_gemm_launch(g, s));
      CellParams c;
      memset(&c, 0, sizeof(c));
      c.N = rows; c.H = H; c.maxout = d.maxout; c.sums = L.sums; c.ld_sums = rl;
      c.c_prev = L.c[cur][l]; c.c_out = L.c[nxt][l]; c.h_out = L.h[nxt][l]; c.ld_h = H;
      if (l == last) { c.n5 = L.sums + GH; c.ld_n5 = rl; c.fake_out = L.fake; c.ld_fake = H; }
      UIC_TRY(cell_launch(dt, c, s));
    }
    // AdaAtt_attention (:377-381): fr = relu(fr_linear(fake)), fr_e = fr_embed(fr), hl = tanh(ho_linear(h)), hl_e = ho_embed(hl)
    UIC_TRY(lin(dt, rows, H, H, L.fake, L.frl_w, L.fr, H, w->fr_linear_b, UIC_GEMM_RELU, s));
    UIC_TRY(lin(dt, rows, H, H, L.fr, L.fre_w, L.fr_e, H, w->fr_embed_b, UIC_GEMM_OUT_F32, s));
    UIC_TRY(lin(dt, rows, H, H, L.h[nxt][last], L.hol_w, L.hl, H, w->ho_linear_b, UIC_GEMM_TANH, s));
    UIC_TRY(lin(dt, rows, H, H, L.hl, L.hoe_w, L.hl_e, H, w->ho_embed_b, UIC_GEMM_OUT_F32, s));
    AttParams a;
    memset(&a, 0, sizeof(a));
    a.N = rows; a.R = R; a.A = H; a.H = H; a.div = div;
    a.fr_e = L.fr_e; a.hl_e = L.hl_e; a.ld_q = H; a.fr = L.fr; a.hl = L.hl; a.ld_x = H;
    a.p_att = L.patt; a.att = L.attp; a.w = w->alpha_w; a.b = w->alpha_b; a.mask = mask; a.ld_mask = R;
    a.PI = L.PI; a.out = L.aout; a.ld_out = H;
    UIC_TRY(attention_launch(dt, a, s));
    UIC_TRY(lin(dt, rows, H, H, L.aout, L.a2h_w, L.ah, H, w->att2h_b, UIC_GEMM_TANH, s));
    const void* x = L.ah;
    for (int l = 0; l + 1 < d.logit_layers; ++l) {     // hidden logit blocks (AttModel.py:90-91); Dropout is the identity in eval mode
      UIC_TRY(lin(dt, rows, H, H, x, L.logit_h_w[l], L.lh[l], H, w->logit_h_b[l], UIC_GEMM_RELU, s));
      x = L.lh[l];
    }
    return lin(dt, rows, V1, H, x, L.logit_w, logits, V1p, w->logit_b, UIC_GEMM_OUT_F32, s);
  }

  int log_softmax(const float* logits, int steps, int rows, float* out, size_t step_stride, size_t row_stride) const {
    UicXeParams x;
    memset(&x, 0, sizeof(x));
    x.dtype = dt; x.M = steps * rows; x.V1 = V1; x.ldv = V1p; x.logits = logits; x.N = rows;
    x.logprobs = out; x.lp_step_stride = step_stride; x.lp_row_stride = row_stride;
    return uic_xe_launch(x, s);
  }
};

}  // namespace

extern "C" {

int uic_adaatt_cell_fwd(int32_t dtype, int32_t N, int32_t H, int32_t maxout, const float* sums, int32_t ld_sums, const float* n5,
                        int32_t ld_n5, const float* c_prev, float* c_out, void* h_out, int32_t ld_h, void* fake_out, int32_t ld_fake,
                        void* stream) {
  CellParams p;
  memset(&p, 0, sizeof(p));
  p.N = N; p.H = H; p.maxout = maxout; p.sums = sums; p.ld_sums = ld_sums; p.n5 = n5; p.ld_n5 = ld_n5;
  p.c_prev = c_prev; p.c_out = c_out; p.h_out = h_out; p.ld_h = ld_h; p.fake_out = fake_out; p.ld_fake = ld_fake;
  return cell_launch(dtype, p, (hipStream_t)stream);
}

int uic_adaatt_attention_fwd(int32_t dtype, int32_t N, int32_t R, int32_t A, int32_t H, int32_t row_div, const float* fr_e,
                             const float* hl_e, int32_t ld_q, const void* fr, const void* hl, int32_t ld_x, const void* p_att,
                             const void* att, const float* w_alpha, const float* b_alpha, const float* mask, int32_t ld_mask, float* PI,
                             void* out, int32_t ld_out, void* stream) {
  AttParams p;
  memset(&p, 0, sizeof(p));
  p.N = N; p.R = R; p.A = A; p.H = H; p.div = row_div; p.fr_e = fr_e; p.hl_e = hl_e; p.ld_q = ld_q; p.fr = fr; p.hl = hl; p.ld_x = ld_x;
  p.p_att = p_att; p.att = att; p.w = w_alpha; p.b = b_alpha; p.mask = mask; p.ld_mask = ld_mask; p.PI = PI; p.out = out; p.ld_out = ld_out;
  return attention_launch(dtype, p, (hipStream_t)stream);
}

size_t uic_adaatt_workspace_bytes(const uic_adaatt_dims* d) {
  if (check_dims(d)) return 0;
  return make_layout(*d, nullptr, nullptr).total;
}

int uic_adaatt_prepare_feature(const uic_adaatt_dims* d, const uic_adaatt_weights* w, const float* fc_feats, const float* att_feats,
                               const float* att_masks, void* workspace, float* fc_out, float* att_out, float* p_att_out, void* stream) {
  UIC_TRY(check_call(d, w, workspace, "adaatt_prepare_feature"));
  UIC_REQUIRE(fc_feats && att_feats && fc_out && att_out && p_att_out, "adaatt_prepare_feature: null pointer");
  const Ada m(*d, w, workspace, (hipStream_t)stream);
  UIC_TRY(m.refresh());
  UIC_TRY(m.prepare(fc_feats, att_feats, att_masks));
  const size_t NR = (size_t)d->N * d->R;
  UIC_TRY(uic_to_f32_launch(m.dt, m.L.fcp, fc_out, (size_t)d->N * d->H, m.s));
  UIC_TRY(uic_to_f32_launch(m.dt, m.L.attp, att_out, NR * d->H, m.s));
  return uic_to_f32_launch(m.dt, m.L.patt, p_att_out, NR * d->H, m.s);
}

int uic_adaatt_forward(const uic_adaatt_dims* d, const uic_adaatt_weights* w, const float* fc_feats, const float* att_feats,
                       const float* att_masks, const int64_t* seq, int32_t ld_seq, int32_t Tq, int32_t s_run, void* workspace,
                       float* logprobs_out, void* stream) {
  UIC_TRY(check_call(d, w, workspace, "adaatt_forward"));
  UIC_REQUIRE(fc_feats && att_feats && seq && logprobs_out, "adaatt_forward: null pointer");
  UIC_REQUIRE(d->beam == 1, "adaatt_forward: dims.beam=%d (one row per caption)", d->beam);
  UIC_REQUIRE(Tq >= 1 && Tq <= d->S - 1 && ld_seq >= Tq, "adaatt_forward: Tq=%d outside [1, S - 1 = %d] or ld_seq=%d shorter", Tq, d->S - 1, ld_seq);
  UIC_REQUIRE(s_run >= 1 && s_run <= Tq, "adaatt_forward: s_run=%d outside [1, Tq = %d]", s_run, Tq);
  const Ada m(*d, w, workspace, (hipStream_t)stream);
  const int N = d->N;
  UIC_TRY(m.refresh());
  UIC_TRY(m.prepare(fc_feats, att_feats, att_masks));
  UIC_TRY(m.state_zero(N));
  for (int i = 0; i < s_run; ++i)
    UIC_TRY(m.step(N, 1, seq + i, ld_seq, att_masks, i & 1, (i & 1) ^ 1, m.L.logits + (size_t)i * N * m.V1p));
  // (the steps behind the early break keep the caller's zeros, as `outputs` does, AttModel.py:123)
  return m.log_softmax(m.L.logits, s_run, N, logprobs_out, (size_t)d->V1, (size_t)Tq * d->V1);
}

int uic_adaatt_logprobs_state(const uic_adaatt_dims* d, const uic_adaatt_weights* w, const int64_t* it, const float* fc, const float* att,
                              const float* p_att, const float* att_masks, const float* h_in, const float* c_in, void* workspace,
                              float* logprobs, float* h_out, float* c_out, void* stream) {
  UIC_TRY(check_call(d, w, workspace, "adaatt_logprobs_state"));
  UIC_REQUIRE(it && fc && att && p_att && h_in && c_in && logprobs && h_out && c_out, "adaatt_logprobs_state: null pointer");
  UIC_REQUIRE(d->beam == 1, "adaatt_logprobs_state: dims.beam=%d (the prepared features are per row)", d->beam);
  const Ada m(*d, w, workspace, (hipStream_t)stream);
  const Layout& L = m.L;
  hipStream_t s = m.s;
  const size_t N = d->N, NH = N * d->H, NRH = N * d->R * d->H;
  UIC_TRY(m.refresh());
  // the caller's prepared features and state become the step's operands (operand dtype) ...
  UIC_TRY(m.cast(fc, L.fcp, NH));
  UIC_TRY(m.cast(att, L.attp, NRH));
  UIC_TRY(m.cast(p_att, L.patt, NRH));
  UIC_TRY(m.fc_projection(L.fcp, (int)N, 1));
  for (int l = 0; l < d->layers; ++l) {
    UIC_TRY(m.cast(h_in + l * NH, L.h[0][l], NH));
    UIC_TRY(uic_copy_launch(L.c[0][l], c_in + l * NH, NH * 4, s));
  }
  UIC_TRY(m.step((int)N, 1, it, 1, att_masks, 0, 1, L.logits));
  // ... and its results go back out: log_softmax of the logits, the new (h, c) stacks [num_layers, N, H]
  UIC_TRY(m.log_softmax(L.logits, 1, (int)N, logprobs, (size_t)d->V1, (size_t)d->V1));
  for (int l = 0; l < d->layers; ++l) {
    UIC_TRY(uic_to_f32_launch(m.dt, L.h[1][l], h_out + l * NH, NH, s));
    UIC_TRY(uic_copy_launch(c_out + l * NH, L.c[1][l], NH * 4, s));
  }
  return UIC_OK;
}

int uic_adaatt_sample(const uic_adaatt_dims* d, const uic_adaatt_weights* w, const float* fc_feats, const float* att_feats,
                      const float* att_masks, int32_t Lsteps, int32_t sample_max, float temperature, int32_t decoding_constraint,
                      uint32_t seed, void* workspace, int64_t* seq, float* seq_logp, void* stream) {
  UIC_TRY(check_call(d, w, workspace, "adaatt_sample"));
  UIC_REQUIRE(fc_feats && att_feats && seq && seq_logp, "adaatt_sample: null pointer");
  UIC_REQUIRE(d->beam == 1, "adaatt_sample: dims.beam=%d (one row per image)", d->beam);
  UIC_REQUIRE(Lsteps >= 1 && Lsteps <= d->S, "adaatt_sample: L=%d outside [1, S = %d]", Lsteps, d->S);
  UIC_REQUIRE(temperature > 0.f, "adaatt_sample: temperature must be positive");
  const Ada m(*d, w, workspace, (hipStream_t)stream);
  const Layout& L = m.L;
  hipStream_t s = m.s;
  const int N = d->N;
  UIC_TRY(m.refresh());
  UIC_TRY(m.prepare(fc_feats, att_feats, att_masks));
  UIC_TRY(m.state_zero(N));
  UIC_TRY(sample_begin(L.smp, N, d->S, seq, seq_logp, (size_t)N * Lsteps, s));   // <bos> = 0 (AttModel.py:214-216)
  for (int t = 0; t < Lsteps; ++t) {
    UIC_TRY(m.step(N, 1, L.smp.it, 1, att_masks, t & 1, (t & 1) ^ 1, L.logits));
    UIC_TRY(uic_sample_step_launch(sample_params(L.smp, m.dt, N, d->V1, t, Lsteps, L.logits, sample_max, temperature, decoding_constraint, seed, nullptr,
                                                 seq, seq_logp), s));
  }
  return UIC_OK;
}

int uic_adaatt_sample_beam(const uic_adaatt_dims* d, const uic_adaatt_weights* w, const float* fc_feats, const float* att_feats,
                           const float* att_masks, int32_t Lsteps, int32_t beam_size, int32_t decoding_constraint, int32_t max_ppl,
                           void* workspace, int64_t* seq, float* seq_logp, void* stream) {
  UIC_TRY(check_call(d, w, workspace, "adaatt_sample_beam"));
  UIC_REQUIRE(fc_feats && att_feats && seq && seq_logp, "adaatt_sample_beam: null pointer");
  UIC_REQUIRE(Lsteps >= 1 && Lsteps <= d->S, "adaatt_sample_beam: L=%d outside [1, S = %d]", Lsteps, d->S);
  UIC_REQUIRE(beam_size >= 1 && beam_size == d->beam && beam_size <= d->V1, "adaatt_sample_beam: beam_size=%d must equal dims.beam=%d (<= V1)",
              beam_size, d->beam);
  const Ada m(*d, w, workspace, (hipStream_t)stream);
  const Layout& L = m.L;
  hipStream_t s = m.s;
  const int N = d->N, B = beam_size, rows = N * B, S = d->S, H = d->H;
  UIC_TRY(m.refresh());
  UIC_TRY(m.prepare(fc_feats, att_feats, att_masks));
  UIC_TRY(m.state_zero(rows));
  UIC_TRY(uic_fill_launch(L.smp.it, 0, (size_t)rows * 8, s));          // <bos> on every beam (AttModel.py:187-188)
  UicBeamParams p;
  UIC_TRY(beam_begin(L.beam, L.logits, m.V1p, L.smp.it, N, B, S, d->V1, Lsteps, decoding_constraint, max_ppl, p, s));
  UIC_TRY(m.step(rows, B, L.smp.it, 1, att_masks, 0, 1, L.logits));       // logprobs after <bos> (AttModel.py:190)
  const bool two = d->layers > 1;
  auto advance = [&](int) -> int {
    // the states follow the surviving parents (CaptionModel.py:90-92): slot 1 -> slot 0
    UIC_TRY(uic_beam_gather_launch(m.dt, p.parent, rows, B, H, L.h[1][0], L.h[0][0], two ? L.h[1][1] : nullptr, two ? L.h[0][1] : nullptr,
                                   L.c[1][0], L.c[0][0], two ? L.c[1][1] : nullptr, two ? L.c[0][1] : nullptr, s));
    return m.step(rows, B, L.smp.it, 1, att_masks, 0, 1, L.logits);
  };
  return beam_search(p, Lsteps, advance, s, seq, seq_logp);
}

int uic_adaatt_beam_done_lists(const uic_adaatt_dims* d, void* workspace, int32_t Lsteps, int32_t beam_size, int32_t* done_count,
                               float* done_p, int64_t* done_seq, float* done_lp, void* stream) {
  UIC_TRY(check_dims(d));
  UIC_REQUIRE(workspace && done_count && done_p && done_seq && done_lp, "adaatt_beam_done_lists: null pointer");
  UIC_REQUIRE(beam_size >= 1 && beam_size == d->beam && Lsteps >= 1 && Lsteps <= d->S, "adaatt_beam_done_lists: bad sizes");
  hipStream_t s = (hipStream_t)stream;
  const Layout L = make_layout(*d, nullptr, workspace);
  return beam_done_lists(L.beam, d->N, Lsteps, beam_size, done_count, done_p, done_seq, done_lp, s);
}

}  // extern "C"
