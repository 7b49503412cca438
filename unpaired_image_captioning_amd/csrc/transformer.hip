// The Transformer captioner (the `transformer` caption model, P/models/TransformerModel.py) in eval mode on one MI355X:
// the teacher-forced forward pass (validation loss) and decoding (greedy, sampled, beam).  Training is not built.
//
// Two kernels of their own, each behind a C-ABI operator:
//   layernorm_std_kernel  the reference's LayerNorm (:91-103): a_2 (x - mean) / (std + eps) + b_2 with the UNBIASED std and eps
//                         added to the std -- not nn.LayerNorm.  One wave per row, the row read once into registers.
//   mha_fwd_kernel        MultiHeadedAttention's `attention` (:178-188) for short sequences: one workgroup per (row, head),
//                         that head's whole K and V in LDS as f32, scores / softmax in f32, no [B, h, Sq, Sk] tensor in memory.
// Everything else is the project's GEMM (every nn.Linear), its BatchNorm operators (att_embed), sampling.hip and beam.hip -- the
// last two through decode_internal.h, which owns their buffers, the start of a pass and the beam loop; the beam driver here
// supplies the step and re-threads the K/V cache by the surviving parents.
//
// Layout of the sequencers: the residual stream x stays f32; LayerNorm writes the GEMM operand (operand dtype); the output
// projections of attention and of the FFN accumulate into x (UIC_GEMM_ACCUM | UIC_GEMM_OUT_F32).  The three input projections
// of an attention are ONE GEMM against the stacked [3 d_model, d_model] copy of linears.0-2.  d_ff is zero-padded to a multiple
// of 8 in the derived copies of w_1 / w_2 (opts.py's default 1300 is none, and the bf16 GEMM needs K % 8 == 0).
// Decoding keeps, per decoder layer, the q | k | v rows of every position so far (the K/V cache: [row][layer][T][3 d_model]);
// a step computes only the new position.  The source-attention K / V of each layer are projected once per call.
#include "uic_common.h"
#include "uic_host.h"
#include "decode_internal.h"
#include "../../include/uic_hip.h"
#include <math.h>
#include <string.h>

namespace {

constexpr int NT = 256;
constexpr int LN_PER = 16;                       // row elements per lane: d <= 64 * LN_PER
constexpr int MHA_MAX_SK = 128, MHA_MAX_DK = 128;
constexpr int HEADS = UIC_TRANSFORMER_HEADS;
constexpr float LN_EPS = 1e-6f;                  // LayerNorm(features, eps=1e-6) (:94)
constexpr float BN_EPS = 1e-5f;                  // nn.BatchNorm1d default

// ------------------------------------------------------------------ LayerNorm (P/models/TransformerModel.py:91-103)
// One wave per row.  The statistics are taken of x - x[0]: the subtraction is exact for rows whose spread is small against
// their offset, so a row of 1e4 + O(1) loses nothing to cancellation; mean first, then the centred squares (no E[x^2] - E[x]^2).
template <typename TI, typename TO>
__global__ __launch_bounds__(NT) void layernorm_std_kernel(const TI* __restrict__ x, int ldx, int rows, int d, const float* __restrict__ a,
                                                           const float* __restrict__ b, float eps, TO* __restrict__ y, int ldy) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;                       // (whole waves leave; the kernel has no workgroup barrier)
  const TI* xr = x + (size_t)row * ldx;
  const float x0 = uic_to_f(xr[0]);
  float v[LN_PER];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < LN_PER; ++k) {
    const int i = lane + 64 * k;
    v[k] = i < d ? uic_to_f(xr[i]) - x0 : 0.f;
    s += v[k];
  }
  const float mean = uic_wave_sum(s) / (float)d;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < LN_PER; ++k) {
    const int i = lane + 64 * k;
    const float c = v[k] - mean;
    if (i < d) q += c * c;
  }
  const float sd = sqrtf(uic_wave_sum(q) / (float)(d - 1));
  const float den = sd + eps;
  TO* yr = y + (size_t)row * ldy;
#pragma unroll
  for (int k = 0; k < LN_PER; ++k) {
    const int i = lane + 64 * k;
    if (i < d) yr[i] = uic_from_f<TO>(a[i] * (v[k] - mean) / den + b[i]);
  }
}

// ------------------------------------------------------------------ multi-head attention (:178-222)
struct MhaParams {
  int B, Sq, Sk, dk, div, causal, q_off;
  const void* Q; const void* K; const void* V; void* O;
  long long q_bs, k_bs, v_bs, o_bs;             // batch strides, elements
  int ldq, ldk, ldv, ldo;                       // row strides, elements
  const unsigned char* mask; int ldmask;        // [B, Sk] or null
};
inline size_t mha_lds_bytes(int Sk, int dk) { return ((size_t)Sk * (dk + 1) + (size_t)Sk * dk + (NT / 64) * (size_t)(Sk + dk)) * 4; }

// grid (heads, B).  LDS: K [Sk][dk + 1] (odd row stride: lane j reads row j without bank conflicts), V [Sk][dk], and per wave the
// probabilities [Sk] and the query row [dk].  A wave owns query rows wave, wave + 4, ...: lane j scores keys j and j + 64, the
// softmax is two wave reductions, lane d then sums p[j] V[j][d].
template <typename T>
__global__ __launch_bounds__(NT) void mha_fwd_kernel(const MhaParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Sk = p.Sk, dk = p.dk, kst = dk + 1;
  float* sK = smem;
  float* sV = sK + (size_t)Sk * kst;
  float* sP = sV + (size_t)Sk * dk;
  float* sQ = sP + (NT / 64) * Sk;
  const int head = blockIdx.x, b = blockIdx.y, bk = b / p.div;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int VN = uic_vec<T>::N;
  const T* Kb = (const T*)p.K + (size_t)bk * p.k_bs + (size_t)head * dk;
  const T* Vb = (const T*)p.V + (size_t)bk * p.v_bs + (size_t)head * dk;
  const int cpr = dk / VN;
  for (int c = tid; c < Sk * cpr; c += NT) {
    const int j = c / cpr, d0 = (c - j * cpr) * VN;
    float f[8];
    uic_unpack<T>(*(const uint4*)(Kb + (size_t)j * p.ldk + d0), f);
#pragma unroll
    for (int e = 0; e < VN; ++e) sK[j * kst + d0 + e] = f[e];
    uic_unpack<T>(*(const uint4*)(Vb + (size_t)j * p.ldv + d0), f);
#pragma unroll
    for (int e = 0; e < VN; ++e) sV[j * dk + d0 + e] = f[e];
  }
  const float rdk = sqrtf((float)dk);
  const unsigned char* mrow = p.mask ? p.mask + (size_t)b * p.ldmask : nullptr;
  float* myP = sP + wave * Sk;
  float* myQ = sQ + wave * dk;
  for (int i0 = 0; i0 < p.Sq; i0 += NT / 64) {    // (uniform trip count: the barriers below are workgroup barriers)
    const int i = i0 + wave;
    const bool live = i < p.Sq;
    if (live) {
      const T* q = (const T*)p.Q + (size_t)b * p.q_bs + (size_t)i * p.ldq + (size_t)head * dk;
      for (int d = lane; d < dk; d += 64) myQ[d] = uic_to_f(q[d]);
    }
    __syncthreads();                              // K / V staged (first trip), the query row visible to the wave
    if (live) {
      float sc[2];
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int j = lane + 64 * jj;
        sc[jj] = -INFINITY;
        if (j < Sk) {
          float acc = 0.f;
          const float* kr = sK + j * kst;
          for (int d = 0; d < dk; ++d) acc += myQ[d] * kr[d];
          acc = acc / rdk;
          // masked_fill(mask == 0, -1e9) (:184): finite, so a fully masked row comes out uniform
          if ((mrow && mrow[j] == 0) || (p.causal && j > p.q_off + i)) acc = -1e9f;
          sc[jj] = acc;
        }
      }
      const float mx = uic_wave_max(fmaxf(sc[0], sc[1]));
      const float e0 = lane < Sk ? expf(sc[0] - mx) : 0.f;
      const float e1 = lane + 64 < Sk ? expf(sc[1] - mx) : 0.f;
      const float sum = uic_wave_sum(e0 + e1);
      if (lane < Sk) myP[lane] = e0 / sum;
      if (lane + 64 < Sk) myP[lane + 64] = e1 / sum;
    }
    __syncthreads();
    if (live) {
      T* o = (T*)p.O + (size_t)b * p.o_bs + (size_t)i * p.ldo + (size_t)head * dk;
      for (int d = lane; d < dk; d += 64) {
        float acc = 0.f;
        for (int j = 0; j < Sk; ++j) acc += myP[j] * sV[j * dk + d];
        o[d] = uic_from_f<T>(acc);
      }
    }
    __syncthreads();                              // the next trip overwrites the wave's query row and probabilities
  }
}

// ------------------------------------------------------------------ small kernels of the sequencers
// dst[r, c] (r < rows_dst, c < ldd) = r < rows and c < cols ? src[r * cols + c] : 0 -- the operand-dtype copy of a weight, with
// the zero padding of d_ff
template <typename T>
__global__ void pad_cast_kernel(const float* __restrict__ src, int rows, int cols, T* __restrict__ dst, int rows_dst, int ldd) {
  const size_t total = (size_t)rows_dst * ldd, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const size_t r = i / ldd;
    const int c = (int)(i - r * ldd);
    dst[i] = uic_from_f<T>(r < (size_t)rows && c < cols ? src[r * cols + c] : 0.f);
  }
}

// pack_wrapper's lengths (AttModel.py:44-53: att_masks.sum(1)) and the key mask of every decode row (image n, repeated `rep`
// times); att_masks == null: all regions
__global__ void region_mask_kernel(const float* __restrict__ att_masks, int N, int R, int rep, int* __restrict__ row_len,
                                   unsigned char* __restrict__ kmask, unsigned char* __restrict__ kmask_rep) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  int len = 0;
  for (int r = 0; r < R; ++r) {
    const float m = att_masks ? att_masks[(size_t)n * R + r] : 1.f;
    len += (int)m;
    const unsigned char on = m != 0.f;
    kmask[(size_t)n * R + r] = on;
    if (kmask_rep)
      for (int k = 0; k < rep; ++k) kmask_rep[((size_t)n * rep + k) * R + r] = on;
  }
  row_len[n] = len;
}

// the target key mask of _prepare_feature (:375-382): (seq > 0) with column 0 forced on
__global__ void target_mask_kernel(const int64_t* __restrict__ seq, int ld_seq, int N, int Tq, unsigned char* __restrict__ tmask) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * Tq) return;
  const int n = i / Tq, t = i - n * Tq;
  tmask[i] = t == 0 || seq[(size_t)n * ld_seq + t] > 0;
}

// tgt_embed (:238-267): x[n, t] = lut[tok[n, t]] * sqrt(d_model) + pe[pos0 + t]; a token outside the table reads row 0
__global__ void target_embed_kernel(const float* __restrict__ lut, const float* __restrict__ pe, const int64_t* __restrict__ tok, int ld_tok,
                                    int Tq, int pos0, int V1, int dm, float scale, float* __restrict__ x) {
  const int row = blockIdx.x, n = row / Tq, t = row - n * Tq;
  long v = tok[(size_t)n * ld_tok + t];
  if (v < 0 || v >= V1) v = 0;
  for (int c = threadIdx.x; c < dm; c += blockDim.x)
    x[(size_t)row * dm + c] = lut[(size_t)v * dm + c] * scale + pe[(size_t)(pos0 + t) * dm + c];
}

int layernorm_launch(int in_dtype, int out_dtype, const void* x, int ldx, int rows, int d, const float* a, const float* b, float eps,
                     void* y, int ldy, hipStream_t s) {
  if (rows == 0) return UIC_OK;
  const dim3 grid((rows + NT / 64 - 1) / (NT / 64)), block(NT);
#define UIC_LN_CASE(TI, TO) \
  hipLaunchKernelGGL((layernorm_std_kernel<TI, TO>), grid, block, 0, s, (const TI*)x, ldx, rows, d, a, b, eps, (TO*)y, ldy)
  if (in_dtype == UIC_F32 && out_dtype == UIC_F32) UIC_LN_CASE(float, float);
  else if (in_dtype == UIC_F32) UIC_LN_CASE(float, bf16_t);
  else if (out_dtype == UIC_F32) UIC_LN_CASE(bf16_t, float);
  else UIC_LN_CASE(bf16_t, bf16_t);
#undef UIC_LN_CASE
  UIC_LAUNCH_CHECK("layernorm_std");
  return UIC_OK;
}

int mha_launch(int dtype, const MhaParams& p, hipStream_t s) {
  const int vec = dtype == UIC_BF16 ? 8 : 4;
  UIC_REQUIRE(p.B > 0 && p.Sq > 0 && p.B <= 65535, "mha_fwd: B=%d Sq=%d (B in [1, 65535], Sq >= 1)", p.B, p.Sq);
  UIC_REQUIRE(p.Sk >= 1 && p.Sk <= MHA_MAX_SK, "mha_fwd: Sk=%d outside [1, %d] (a head's whole K and V live in LDS)", p.Sk, MHA_MAX_SK);
  UIC_REQUIRE(p.dk >= 8 && p.dk <= MHA_MAX_DK && p.dk % 8 == 0, "mha_fwd: d_k=%d must be a multiple of 8 in [8, %d]", p.dk, MHA_MAX_DK);
  UIC_REQUIRE(p.div >= 1 && p.B % p.div == 0, "mha_fwd: row divisor %d does not divide B=%d", p.div, p.B);
  UIC_REQUIRE(p.Q && p.K && p.V && p.O, "mha_fwd: null pointer");
  UIC_REQUIRE(p.ldk % vec == 0 && p.ldv % vec == 0 && p.k_bs % vec == 0 && p.v_bs % vec == 0 && ((uintptr_t)p.K & 15) == 0 && ((uintptr_t)p.V & 15) == 0,
              "mha_fwd: K / V rows are read in 16-byte pieces (strides multiples of %d elements, 16-byte aligned)", vec);
  UIC_REQUIRE(p.ldq >= HEADS * p.dk && p.ldk >= HEADS * p.dk && p.ldv >= HEADS * p.dk && p.ldo >= HEADS * p.dk,
              "mha_fwd: a row stride is shorter than heads * d_k = %d", HEADS * p.dk);
  UIC_REQUIRE(!p.mask || p.ldmask >= p.Sk, "mha_fwd: mask rows of %d bytes for Sk=%d", p.ldmask, p.Sk);
  UIC_REQUIRE(p.q_off >= 0, "mha_fwd: negative query offset");
  const size_t lds = mha_lds_bytes(p.Sk, p.dk);
  static bool configured = false;
  if (!configured) {
    const int most = (int)mha_lds_bytes(MHA_MAX_SK, MHA_MAX_DK);
    UIC_TRY(uic_check_hip(hipFuncSetAttribute((const void*)mha_fwd_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, most), "hipFuncSetAttribute(mha f32)"));
    UIC_TRY(uic_check_hip(hipFuncSetAttribute((const void*)mha_fwd_kernel<bf16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, most), "hipFuncSetAttribute(mha bf16)"));
    configured = true;
  }
  const dim3 grid(HEADS, p.B), block(NT);
  if (dtype == UIC_BF16) hipLaunchKernelGGL(mha_fwd_kernel<bf16_t>, grid, block, lds, s, p);
  else hipLaunchKernelGGL(mha_fwd_kernel<float>, grid, block, lds, s, p);
  UIC_LAUNCH_CHECK("mha_fwd");
  return UIC_OK;
}

int pad_cast(int dt, const float* src, int rows, int cols, void* dst, int rows_dst, int ldd, hipStream_t s) {
  const size_t total = (size_t)rows_dst * ldd;
  if (total == 0) return UIC_OK;
  const int g = uic_grid_for(total, NT);
  if (dt == UIC_BF16) hipLaunchKernelGGL(pad_cast_kernel<bf16_t>, dim3(g), dim3(NT), 0, s, src, rows, cols, (bf16_t*)dst, rows_dst, ldd);
  else hipLaunchKernelGGL(pad_cast_kernel<float>, dim3(g), dim3(NT), 0, s, src, rows, cols, (float*)dst, rows_dst, ldd);
  UIC_LAUNCH_CHECK("pad_cast");
  return UIC_OK;
}

// indices into uic_transformer_weights.enc[l] / .dec[l] (include/uic_hip.h)
enum { E_LN0A, E_LN0B, E_LN1A, E_LN1B, E_QW, E_QB, E_KW, E_KB, E_VW, E_VB, E_OW, E_OB, E_W1W, E_W1B, E_W2W, E_W2B };
enum { D_LN0A, D_LN0B, D_LN1A, D_LN1B, D_LN2A, D_LN2B, D_QW, D_QB, D_KW, D_KB, D_VW, D_VB, D_OW, D_OB,
       D_SQW, D_SQB, D_SKW, D_SKB, D_SVW, D_SVB, D_SOW, D_SOB, D_W1W, D_W1B, D_W2W, D_W2B };

struct AttnW { void* qkv; float* bqkv; void* o; };           // [3 dm, dm] stacked linears.0-2, their biases, linears.3
struct FfnW { void* w1; float* b1; void* w2; };               // [dffp, dm], [dffp], [dm, dffp]
struct TfDerived {
  void* att_w; float* att_beff;
  AttnW enc_attn[UIC_TRANSFORMER_MAX_LAYERS]; FfnW enc_ffn[UIC_TRANSFORMER_MAX_LAYERS];
  AttnW dec_self[UIC_TRANSFORMER_MAX_LAYERS]; AttnW dec_src[UIC_TRANSFORMER_MAX_LAYERS]; FfnW dec_ffn[UIC_TRANSFORMER_MAX_LAYERS];
  void* gen_w;
  size_t total;
};

TfDerived tf_derived(const uic_transformer_dims& d, void* base) {
  TfDerived v;
  memset(&v, 0, sizeof(v));
  Bump b{(char*)base, 0};
  const size_t Sz = uic_dtype_size(d.dtype), dm = d.d_model, dffp = rup8(d.d_ff);
  v.att_w = b.take(dm * d.D * Sz);
  v.att_beff = (float*)b.take(dm * 4);
  auto attn = [&](AttnW& a) { a.qkv = b.take(3 * dm * dm * Sz); a.bqkv = (float*)b.take(3 * dm * 4); a.o = b.take(dm * dm * Sz); };
  auto ffn = [&](FfnW& f) { f.w1 = b.take(dffp * dm * Sz); f.b1 = (float*)b.take(dffp * 4); f.w2 = b.take(dm * dffp * Sz); };
  for (int l = 0; l < d.layers; ++l) {
    attn(v.enc_attn[l]); ffn(v.enc_ffn[l]);
    attn(v.dec_self[l]); attn(v.dec_src[l]); ffn(v.dec_ffn[l]);
  }
  v.gen_w = b.take((size_t)d.V1 * dm * Sz);
  v.total = (b.off + 255) & ~(size_t)255;
  return v;
}

struct TfLayout {
  int* row_len; unsigned char* kmask; unsigned char* kmask_rep; unsigned char* tmask;
  float* bn_stat0; float* bn_stat4; void* xhat; float* ybn;
  float* x_enc;      // [N R, dm] the encoder's residual stream
  void* xn;          // [M, dm] LayerNorm output = GEMM operand
  void* qkv;         // [M, 3 dm]
  void* ctx;         // [M, dm]
  void* hff;         // [M, dffp]
  void* mem;         // [N R, dm] encoder memory
  void* memkv[UIC_TRANSFORMER_MAX_LAYERS];   // [N R, 2 dm] source-attention K | V of decoder layer l
  float* x_dec;      // [rows T, dm]
  float* logits;     // [rows T, V1p]
  void* cache[2];    // [rows][layers][T][3 dm] q | k | v of every decoded position (two generations for the beam re-threading)
  SampleScratch smp; // rows = N beam, step capacity T
  BeamScratch beam;  // the same rows, a done_count entry per image, step capacity T
  size_t total;
};

TfLayout tf_layout(const uic_transformer_dims& d, void* ws) {
  TfLayout L;
  memset(&L, 0, sizeof(L));
  Bump b{(char*)ws, 0};
  const size_t Sz = uic_dtype_size(d.dtype), N = d.N, R = d.R, dm = d.d_model, dffp = rup8(d.d_ff), T = d.T, B = d.beam;
  const size_t rows = N * B, NR = N * R, V1p = vpad(d.V1);
  const size_t Md = rows * T > N * T ? rows * T : N * T;
  const size_t M = NR > Md ? NR : Md;
  L.row_len = (int*)b.take(N * 4);
  L.kmask = (unsigned char*)b.take(NR);
  L.kmask_rep = (unsigned char*)b.take(rows * R);
  L.tmask = (unsigned char*)b.take(N * T);
  L.bn_stat0 = (float*)b.take(2 * (size_t)d.D * 4);
  L.bn_stat4 = (float*)b.take(2 * dm * 4);
  L.xhat = b.take(NR * d.D * Sz);
  L.ybn = (float*)b.take(d.use_bn == 2 ? NR * dm * 4 : 0);
  L.x_enc = (float*)b.take(NR * dm * 4);
  L.xn = b.take(M * dm * Sz);
  L.qkv = b.take(M * 3 * dm * Sz);
  L.ctx = b.take(M * dm * Sz);
  L.hff = b.take(M * dffp * Sz);
  L.mem = b.take(NR * dm * Sz);
  for (int l = 0; l < d.layers; ++l) L.memkv[l] = b.take(NR * 2 * dm * Sz);
  L.x_dec = (float*)b.take(Md * dm * 4);
  L.logits = (float*)b.take(Md * V1p * 4);
  for (int i = 0; i < 2; ++i) L.cache[i] = b.take(rows * d.layers * T * 3 * dm * Sz);
  L.smp.carve(b, rows, T);
  L.beam.carve(b, rows, N, T);
  L.total = (b.off + 255) & ~(size_t)255;
  return L;
}

int tf_check(const uic_transformer_dims* d) {
  UIC_REQUIRE(d != nullptr, "transformer: null dims");
  UIC_REQUIRE(d->dtype == UIC_F32 || d->dtype == UIC_BF16, "transformer: bad dtype %d", d->dtype);
  UIC_REQUIRE(d->N > 0 && d->T >= 1 && d->V1 > 1, "transformer: bad sizes N=%d T=%d V1=%d", d->N, d->T, d->V1);
  UIC_REQUIRE(d->R >= 1 && d->R <= MHA_MAX_SK, "transformer: R=%d regions outside [1, %d]", d->R, MHA_MAX_SK);
  UIC_REQUIRE(d->T <= MHA_MAX_SK, "transformer: T=%d target positions (max %d)", d->T, MHA_MAX_SK);
  UIC_REQUIRE(d->D > 0 && d->D % 8 == 0, "transformer: att_feat_size D=%d must be a multiple of 8", d->D);
  UIC_REQUIRE(d->d_model >= 8 * HEADS && d->d_model % (8 * HEADS) == 0 && d->d_model / HEADS <= MHA_MAX_DK && d->d_model <= 64 * LN_PER,
              "transformer: d_model=%d must be a multiple of %d in [%d, %d] (h = %d heads, d_k a multiple of 8)", d->d_model, 8 * HEADS,
              8 * HEADS, 64 * LN_PER, HEADS);
  UIC_REQUIRE(d->d_ff >= 1, "transformer: d_ff=%d", d->d_ff);
  UIC_REQUIRE(d->layers >= 1 && d->layers <= UIC_TRANSFORMER_MAX_LAYERS, "transformer: %d layers (1..%d)", d->layers, UIC_TRANSFORMER_MAX_LAYERS);
  UIC_REQUIRE(d->beam >= 1 && d->beam <= UIC_BEAM_MAX, "transformer: beam=%d outside [1, %d]", d->beam, UIC_BEAM_MAX);
  UIC_REQUIRE(d->use_bn >= 0 && d->use_bn <= 2, "transformer: use_bn=%d", d->use_bn);
  return UIC_OK;
}

// C (+)= A[M, K] W[N, K]^T + bias
int lin(int dt, int M, int N, int K, const void* A, int lda, const void* W, int ldw, void* C, int ldc, const float* bias, int flags,
        hipStream_t s) {
  UicGemmParams g = gemm_base(dt, M, N);
  add_seg(g, A, lda, W, ldw, K);
  g.C = C; g.ldc = ldc; g.bias = bias; g.flags = flags;
  return uic_gemm_launch(g, s);
}

struct Tf {
  const uic_transformer_dims& d; const uic_transformer_weights* w; TfDerived v; TfLayout L; hipStream_t s;
  int dt, dm, dk, dffp, V1p;
  size_t Sz;
  Tf(const uic_transformer_dims& d_, const uic_transformer_weights* w_, const void* derived, void* ws, hipStream_t s_)
      : d(d_), w(w_), v(tf_derived(d_, (void*)derived)), L(tf_layout(d_, ws)), s(s_) {
    dt = d.dtype; dm = d.d_model; dk = dm / HEADS; dffp = (int)rup8(d.d_ff); V1p = (int)vpad(d.V1); Sz = uic_dtype_size(dt);
  }
  int ln(const float* x, int rows, const float* a, const float* b, void* y, int out_dtype) const {
    return layernorm_launch(UIC_F32, out_dtype, x, dm, rows, dm, a, b, LN_EPS, y, dm, s);
  }
  // x += w_2 relu(w_1 norm(x))   (SublayerConnection over PositionwiseFeedForward, :106-119, :225-235)
  int ffn(float* x, int M, const float* na, const float* nb, const FfnW& f, const float* b2) const {
    UIC_TRY(ln(x, M, na, nb, L.xn, dt));
    UIC_TRY(lin(dt, M, dffp, dm, L.xn, dm, f.w1, dm, L.hff, dffp, f.b1, UIC_GEMM_RELU, s));
    return lin(dt, M, dm, dffp, L.hff, dffp, f.w2, dffp, x, dm, b2, UIC_GEMM_ACCUM | UIC_GEMM_OUT_F32, s);
  }
  MhaParams mha_base(int B, int Sq, int Sk) const {
    MhaParams p;
    memset(&p, 0, sizeof(p));
    p.B = B; p.Sq = Sq; p.Sk = Sk; p.dk = dk; p.div = 1;
    return p;
  }

  // _prepare_feature's source side + model.encode (:366-373, :53-54): memory [N R, dm] in L.mem
  int encode(const float* att_feats, const float* att_masks, float* memory_out) const {
    const int N = d.N, R = d.R, NR = N * R, D = d.D;
    hipLaunchKernelGGL(region_mask_kernel, dim3((N + 63) / 64), dim3(64), 0, s, att_masks, N, R, d.beam, L.row_len, L.kmask,
                       d.beam > 1 ? L.kmask_rep : nullptr);
    UIC_LAUNCH_CHECK("region_mask");
    const int* row_len = att_masks ? L.row_len : nullptr;
    const void* att_in = att_feats;
    if (d.use_bn) {   // BatchNorm1d(D), running statistics; its affine part is folded into the Linear's copy (refresh)
      UIC_TRY(uic_bn_stats_running_launch(w->att_bn0_rm, w->att_bn0_rv, D, BN_EPS, L.bn_stat0, s));
      UIC_TRY(uic_bn_apply_launch(UIC_F32, dt, att_feats, NR, R, D, row_len, L.bn_stat0, nullptr, nullptr, 0, L.xhat, s));
      att_in = L.xhat;
    } else if (dt == UIC_BF16) {
      UIC_TRY(uic_cast_f32_launch(dt, att_feats, L.xhat, (size_t)NR * D, s));
      att_in = L.xhat;
    }
    {  // Linear + ReLU (Dropout is the identity in eval mode); pack_wrapper leaves the padded regions exact zeros
      UicGemmParams g = gemm_base(dt, NR, dm);
      add_seg(g, att_in, D, v.att_w, D, D);
      g.C = d.use_bn == 2 ? L.ybn : L.x_enc; g.ldc = dm; g.bias = d.use_bn ? v.att_beff : w->att_b;
      g.flags = UIC_GEMM_RELU | UIC_GEMM_OUT_F32;
      if (row_len) { g.row_len = row_len; g.R = R; }
      UIC_TRY(uic_gemm_launch(g, s));
    }
    if (d.use_bn == 2) {
      UIC_TRY(uic_bn_stats_running_launch(w->att_bn4_rm, w->att_bn4_rv, dm, BN_EPS, L.bn_stat4, s));
      UIC_TRY(uic_bn_apply_launch(UIC_F32, UIC_F32, L.ybn, NR, R, dm, row_len, L.bn_stat4, w->att_bn4_w, w->att_bn4_b, 1, L.x_enc, s));
    }
    for (int l = 0; l < d.layers; ++l) {
      const float* const* e = w->enc[l];
      UIC_TRY(ln(L.x_enc, NR, e[E_LN0A], e[E_LN0B], L.xn, dt));
      UIC_TRY(lin(dt, NR, 3 * dm, dm, L.xn, dm, v.enc_attn[l].qkv, dm, L.qkv, 3 * dm, v.enc_attn[l].bqkv, 0, s));
      MhaParams p = mha_base(N, R, R);
      p.Q = L.qkv; p.K = off(L.qkv, dm, dt); p.V = off(L.qkv, 2 * dm, dt); p.O = L.ctx;
      p.ldq = p.ldk = p.ldv = 3 * dm; p.q_bs = p.k_bs = p.v_bs = (long long)R * 3 * dm;
      p.ldo = dm; p.o_bs = (long long)R * dm;
      p.mask = L.kmask; p.ldmask = R;
      UIC_TRY(mha_launch(dt, p, s));
      UIC_TRY(lin(dt, NR, dm, dm, L.ctx, dm, v.enc_attn[l].o, dm, L.x_enc, dm, e[E_OB], UIC_GEMM_ACCUM | UIC_GEMM_OUT_F32, s));
      UIC_TRY(ffn(L.x_enc, NR, e[E_LN1A], e[E_LN1B], v.enc_ffn[l], e[E_W2B]));
    }
    UIC_TRY(ln(L.x_enc, NR, w->enc_norm_a, w->enc_norm_b, L.mem, dt));
    if (memory_out) UIC_TRY(ln(L.x_enc, NR, w->enc_norm_a, w->enc_norm_b, memory_out, UIC_F32));
    // every decoder layer's source-attention K | V, once per call
    for (int l = 0; l < d.layers; ++l)
      UIC_TRY(lin(dt, NR, 2 * dm, dm, L.mem, dm, off(v.dec_src[l].qkv, (size_t)dm * dm, dt), dm, L.memkv[l], 2 * dm, v.dec_src[l].bqkv + dm, 0, s));
    return UIC_OK;
  }

  // The decoder stack over `rows` sequences of Sq new positions each (x = L.x_dec [rows Sq, dm]), positions pos0 .. pos0 + Sq - 1.
  //   cache == null (teacher forcing): keys are the Sq positions themselves, masked by tmask and causally;
  //   cache != null (decoding, Sq = 1): the new q | k | v row goes to the cache, keys are positions 0 .. pos0.
  // src_div: rows per image (the beams of an image share its memory K / V).  Leaves norm(x) in L.xn.
  int decoder(int rows, int Sq, int pos0, void* cache, const unsigned char* tmask, const unsigned char* kmask_rows, int src_div) const {
    const int M = rows * Sq, R = d.R, T = d.T;
    const long long crow = (long long)d.layers * T * 3 * dm;     // cache elements per row
    for (int l = 0; l < d.layers; ++l) {
      const float* const* e = w->dec[l];
      UIC_TRY(ln(L.x_dec, M, e[D_LN0A], e[D_LN0B], L.xn, dt));
      MhaParams p = mha_base(rows, Sq, cache ? pos0 + 1 : Sq);
      if (cache) {
        const void* cl = off(cache, (size_t)l * T * 3 * dm, dt);
        void* at = offw(cache, ((size_t)l * T + pos0) * 3 * dm, dt);
        UIC_TRY(lin(dt, rows, 3 * dm, dm, L.xn, dm, v.dec_self[l].qkv, dm, at, (int)crow, v.dec_self[l].bqkv, 0, s));
        p.Q = at; p.K = off(cl, dm, dt); p.V = off(cl, 2 * dm, dt);
        p.q_bs = p.k_bs = p.v_bs = crow;
      } else {
        UIC_TRY(lin(dt, M, 3 * dm, dm, L.xn, dm, v.dec_self[l].qkv, dm, L.qkv, 3 * dm, v.dec_self[l].bqkv, 0, s));
        p.Q = L.qkv; p.K = off(L.qkv, dm, dt); p.V = off(L.qkv, 2 * dm, dt);
        p.q_bs = p.k_bs = p.v_bs = (long long)Sq * 3 * dm;
        p.mask = tmask; p.ldmask = Sq; p.causal = 1;
      }
      p.ldq = p.ldk = p.ldv = 3 * dm; p.O = L.ctx; p.ldo = dm; p.o_bs = (long long)Sq * dm;
      UIC_TRY(mha_launch(dt, p, s));
      UIC_TRY(lin(dt, M, dm, dm, L.ctx, dm, v.dec_self[l].o, dm, L.x_dec, dm, e[D_OB], UIC_GEMM_ACCUM | UIC_GEMM_OUT_F32, s));
      // source attention over the memory
      UIC_TRY(ln(L.x_dec, M, e[D_LN1A], e[D_LN1B], L.xn, dt));
      UIC_TRY(lin(dt, M, dm, dm, L.xn, dm, v.dec_src[l].qkv, dm, L.qkv, dm, v.dec_src[l].bqkv, 0, s));
      MhaParams q = mha_base(rows, Sq, R);
      q.Q = L.qkv; q.ldq = dm; q.q_bs = (long long)Sq * dm;
      q.K = L.memkv[l]; q.V = off(L.memkv[l], dm, dt); q.ldk = q.ldv = 2 * dm; q.k_bs = q.v_bs = (long long)R * 2 * dm;
      q.O = L.ctx; q.ldo = dm; q.o_bs = (long long)Sq * dm;
      q.mask = kmask_rows; q.ldmask = R; q.div = src_div;
      UIC_TRY(mha_launch(dt, q, s));
      UIC_TRY(lin(dt, M, dm, dm, L.ctx, dm, v.dec_src[l].o, dm, L.x_dec, dm, e[D_SOB], UIC_GEMM_ACCUM | UIC_GEMM_OUT_F32, s));
      UIC_TRY(ffn(L.x_dec, M, e[D_LN2A], e[D_LN2B], v.dec_ffn[l], e[D_W2B]));
    }
    return ln(L.x_dec, M, w->dec_norm_a, w->dec_norm_b, L.xn, dt);
  }
  int embed(const int64_t* tok, int ld_tok, int rows, int Tq, int pos0) const {
    hipLaunchKernelGGL(target_embed_kernel, dim3(rows * Tq), dim3(dm < NT ? 64 : NT), 0, s, w->lut, w->pe, tok, ld_tok, Tq, pos0, d.V1, dm,
                       sqrtf((float)dm), L.x_dec);
    UIC_LAUNCH_CHECK("target_embed");
    return UIC_OK;
  }
  int generator(int M) const {   // Generator.proj (:60-68); the log-softmax is the consumer's
    return lin(dt, M, d.V1, dm, L.xn, dm, v.gen_w, dm, L.logits, V1p, w->gen_b, UIC_GEMM_OUT_F32, s);
  }
  // one decoding step: embed the rows' input tokens (L.smp.it) at position t, the stack against the cache, the logits
  int step(int rows, int t, void* cache, const unsigned char* kmask_rows, int src_div) const {
    UIC_TRY(embed(L.smp.it, 1, rows, 1, t));
    UIC_TRY(decoder(rows, 1, t, cache, nullptr, kmask_rows, src_div));
    return generator(rows);
  }
};

int tf_check_call(const uic_transformer_dims* d, const uic_transformer_weights* w, const void* derived, const void* ws, const char* who) {
  UIC_TRY(tf_check(d));
  UIC_REQUIRE(w && derived && ws, "%s: null pointer", who);
  UIC_REQUIRE(w->att_w && w->att_b && w->lut && w->pe && w->gen_w && w->gen_b && w->enc_norm_a && w->enc_norm_b && w->dec_norm_a && w->dec_norm_b,
              "%s: null weight", who);
  if (d->use_bn) UIC_REQUIRE(w->att_bn0_w && w->att_bn0_b && w->att_bn0_rm && w->att_bn0_rv, "%s: use_bn=%d needs the att_embed.0 BatchNorm tensors", who, d->use_bn);
  if (d->use_bn == 2) UIC_REQUIRE(w->att_bn4_w && w->att_bn4_b && w->att_bn4_rm && w->att_bn4_rv, "%s: use_bn=2 needs the att_embed.4 BatchNorm tensors", who);
  for (int l = 0; l < d->layers; ++l) {
    for (int i = 0; i < 16; ++i) UIC_REQUIRE(w->enc[l][i], "%s: null encoder weight %d of layer %d", who, i, l);
    for (int i = 0; i < 26; ++i) UIC_REQUIRE(w->dec[l][i], "%s: null decoder weight %d of layer %d", who, i, l);
  }
  return UIC_OK;
}

}  // namespace

extern "C" {

int uic_layernorm_std(int32_t in_dtype, int32_t out_dtype, const void* x, int32_t ldx, int32_t rows, int32_t d, const float* a_2,
                      const float* b_2, float eps, void* y, int32_t ldy, void* stream) {
  UIC_REQUIRE((in_dtype == UIC_F32 || in_dtype == UIC_BF16) && (out_dtype == UIC_F32 || out_dtype == UIC_BF16), "layernorm_std: bad dtype %d / %d",
              in_dtype, out_dtype);
  UIC_REQUIRE(x && a_2 && b_2 && y, "layernorm_std: null pointer");
  UIC_REQUIRE(rows >= 0 && d >= 2 && d <= 64 * LN_PER, "layernorm_std: rows=%d d=%d (d in [2, %d]: the unbiased std needs two elements, a row lives in one wave's registers)",
              rows, d, 64 * LN_PER);
  UIC_REQUIRE(ldx >= d && ldy >= d, "layernorm_std: ldx=%d ldy=%d shorter than d=%d", ldx, ldy, d);
  return layernorm_launch(in_dtype, out_dtype, x, ldx, rows, d, a_2, b_2, eps, y, ldy, (hipStream_t)stream);
}

int uic_mha_fwd(int32_t dtype, int32_t B, int32_t Sq, int32_t Sk, int32_t d_k, const void* Q, int32_t ldq, int64_t q_batch_stride,
                const void* K, int32_t ldk, int64_t k_batch_stride, const void* V, int32_t ldv, int64_t v_batch_stride, void* O, int32_t ldo,
                int64_t o_batch_stride, const uint8_t* key_mask, int32_t ld_mask, int32_t causal, int32_t q_offset, int32_t row_div,
                void* stream) {
  UIC_REQUIRE(dtype == UIC_F32 || dtype == UIC_BF16, "mha_fwd: bad dtype %d", dtype);
  MhaParams p;
  memset(&p, 0, sizeof(p));
  p.B = B; p.Sq = Sq; p.Sk = Sk; p.dk = d_k; p.div = row_div; p.causal = causal != 0; p.q_off = q_offset;
  p.Q = Q; p.K = K; p.V = V; p.O = O;
  p.q_bs = q_batch_stride; p.k_bs = k_batch_stride; p.v_bs = v_batch_stride; p.o_bs = o_batch_stride;
  p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo;
  p.mask = key_mask; p.ldmask = ld_mask;
  return mha_launch(dtype, p, (hipStream_t)stream);
}

size_t uic_transformer_workspace_bytes(const uic_transformer_dims* d) {
  if (tf_check(d)) return 0;
  return tf_layout(*d, nullptr).total;
}

size_t uic_transformer_derived_bytes(const uic_transformer_dims* d) {
  if (tf_check(d)) return 0;
  return tf_derived(*d, nullptr).total;
}

int uic_transformer_refresh_weights(const uic_transformer_dims* d, const uic_transformer_weights* w, void* derived, void* stream) {
  UIC_TRY(tf_check_call(d, w, derived, derived, "transformer_refresh_weights"));
  hipStream_t s = (hipStream_t)stream;
  const TfDerived v = tf_derived(*d, derived);
  const int dt = d->dtype, dm = d->d_model, dff = d->d_ff, dffp = (int)rup8(dff);
  if (d->use_bn) UIC_TRY(uic_bn_fold_weight_launch(dt, w->att_w, w->att_bn0_w, w->att_bn0_b, w->att_b, dm, d->D, v.att_w, v.att_beff, s));
  else UIC_TRY(pad_cast(dt, w->att_w, dm, d->D, v.att_w, dm, d->D, s));
  auto attn = [&](const AttnW& a, const float* const* p, int q0) -> int {   // p[q0 ..]: q_w q_b k_w k_b v_w v_b o_w o_b
    for (int i = 0; i < 3; ++i) {
      UIC_TRY(pad_cast(dt, p[q0 + 2 * i], dm, dm, offw(a.qkv, (size_t)i * dm * dm, dt), dm, dm, s));
      UIC_TRY(pad_cast(UIC_F32, p[q0 + 2 * i + 1], 1, dm, a.bqkv + (size_t)i * dm, 1, dm, s));
    }
    return pad_cast(dt, p[q0 + 6], dm, dm, a.o, dm, dm, s);
  };
  auto ffn = [&](const FfnW& f, const float* const* p, int w0) -> int {     // p[w0 ..]: w1_w w1_b w2_w w2_b
    UIC_TRY(pad_cast(dt, p[w0], dff, dm, f.w1, dffp, dm, s));
    UIC_TRY(pad_cast(UIC_F32, p[w0 + 1], 1, dff, f.b1, 1, dffp, s));
    return pad_cast(dt, p[w0 + 2], dm, dff, f.w2, dm, dffp, s);
  };
  for (int l = 0; l < d->layers; ++l) {
    UIC_TRY(attn(v.enc_attn[l], w->enc[l], E_QW));
    UIC_TRY(ffn(v.enc_ffn[l], w->enc[l], E_W1W));
    UIC_TRY(attn(v.dec_self[l], w->dec[l], D_QW));
    UIC_TRY(attn(v.dec_src[l], w->dec[l], D_SQW));
    UIC_TRY(ffn(v.dec_ffn[l], w->dec[l], D_W1W));
  }
  return pad_cast(dt, w->gen_w, d->V1, dm, v.gen_w, d->V1, dm, s);
}

int uic_transformer_encode(const uic_transformer_dims* d, const uic_transformer_weights* w, const void* derived, const float* att_feats,
                           const float* att_masks, void* workspace, float* memory_out, void* stream) {
  UIC_TRY(tf_check_call(d, w, derived, workspace, "transformer_encode"));
  UIC_REQUIRE(att_feats, "transformer_encode: null att_feats");
  const Tf tf(*d, w, derived, workspace, (hipStream_t)stream);
  return tf.encode(att_feats, att_masks, memory_out);
}

int uic_transformer_forward(const uic_transformer_dims* d, const uic_transformer_weights* w, const void* derived, const float* att_feats,
                            const float* att_masks, const int64_t* seq, int32_t ld_seq, int32_t Tq, void* workspace, float* logprobs_out,
                            void* stream) {
  UIC_TRY(tf_check_call(d, w, derived, workspace, "transformer_forward"));
  UIC_REQUIRE(att_feats && seq && logprobs_out, "transformer_forward: null pointer");
  UIC_REQUIRE(Tq >= 1 && Tq <= d->T && ld_seq >= Tq, "transformer_forward: Tq=%d outside [1, T = %d] or ld_seq=%d shorter", Tq, d->T, ld_seq);
  const Tf tf(*d, w, derived, workspace, (hipStream_t)stream);
  hipStream_t s = tf.s;
  const int N = d->N, M = N * Tq;
  UIC_TRY(tf.encode(att_feats, att_masks, nullptr));
  hipLaunchKernelGGL(target_mask_kernel, dim3((M + NT - 1) / NT), dim3(NT), 0, s, seq, ld_seq, N, Tq, tf.L.tmask);
  UIC_LAUNCH_CHECK("target_mask");
  UIC_TRY(tf.embed(seq, ld_seq, N, Tq, 0));
  UIC_TRY(tf.decoder(N, Tq, 0, nullptr, tf.L.tmask, tf.L.kmask, 1));
  UIC_TRY(tf.generator(M));
  UicXeParams x;                    // log_softmax, rows in (n, t) order: one "caption row", M "steps"
  memset(&x, 0, sizeof(x));
  x.dtype = d->dtype; x.M = M; x.V1 = d->V1; x.ldv = tf.V1p; x.logits = tf.L.logits; x.N = 1;
  x.logprobs = logprobs_out; x.lp_step_stride = (size_t)d->V1; x.lp_row_stride = 0;
  return uic_xe_launch(x, s);
}

int uic_transformer_sample(const uic_transformer_dims* d, const uic_transformer_weights* w, const void* derived, const float* att_feats,
                           const float* att_masks, int32_t Lsteps, int32_t sample_max, float temperature, uint32_t seed, void* workspace,
                           int64_t* seq, float* seq_logp, void* stream) {
  UIC_TRY(tf_check_call(d, w, derived, workspace, "transformer_sample"));
  UIC_REQUIRE(att_feats && seq && seq_logp, "transformer_sample: null pointer");
  UIC_REQUIRE(Lsteps >= 1 && Lsteps <= d->T, "transformer_sample: L=%d outside [1, T = %d]", Lsteps, d->T);
  UIC_REQUIRE(temperature > 0.f, "transformer_sample: temperature must be positive");
  const Tf tf(*d, w, derived, workspace, (hipStream_t)stream);
  hipStream_t s = tf.s;
  const TfLayout& L = tf.L;
  const int N = d->N;
  UIC_TRY(tf.encode(att_feats, att_masks, nullptr));
  UIC_TRY(sample_begin(L.smp, N, d->T, seq, seq_logp, (size_t)N * Lsteps, s));   // <bos> = 0 (:539-540)
  for (int t = 0; t < Lsteps; ++t) {
    UIC_TRY(tf.step(N, t, L.cache[0], L.kmask, 1));
    UIC_TRY(uic_sample_step_launch(sample_params(L.smp, d->dtype, N, d->V1, t, Lsteps, L.logits, sample_max, temperature, 0, seed, nullptr, seq, seq_logp), s));
  }
  return UIC_OK;
}

int uic_transformer_sample_beam(const uic_transformer_dims* d, const uic_transformer_weights* w, const void* derived, const float* att_feats,
                                const float* att_masks, int32_t Lsteps, int32_t beam_size, int32_t decoding_constraint, int32_t max_ppl,
                                void* workspace, int64_t* seq, float* seq_logp, void* stream) {
  UIC_TRY(tf_check_call(d, w, derived, workspace, "transformer_sample_beam"));
  UIC_REQUIRE(att_feats && seq && seq_logp, "transformer_sample_beam: null pointer");
  UIC_REQUIRE(Lsteps >= 1 && Lsteps <= d->T, "transformer_sample_beam: L=%d outside [1, T = %d]", Lsteps, d->T);
  UIC_REQUIRE(beam_size >= 1 && beam_size == d->beam && beam_size <= d->V1, "transformer_sample_beam: beam_size=%d must equal dims.beam=%d (<= V1)",
              beam_size, d->beam);
  const Tf tf(*d, w, derived, workspace, (hipStream_t)stream);
  hipStream_t s = tf.s;
  const TfLayout& L = tf.L;
  const int N = d->N, B = beam_size, rows = N * B, T = d->T;
  UIC_TRY(tf.encode(att_feats, att_masks, nullptr));
  const unsigned char* kmask_rows = B > 1 ? L.kmask_rep : L.kmask;
  UIC_TRY(uic_fill_launch(L.smp.it, 0, (size_t)rows * 8, s));          // <bos> on every beam (:464)
  UicBeamParams p;
  UIC_TRY(beam_begin(L.beam, L.logits, tf.V1p, L.smp.it, N, B, T, d->V1, Lsteps, decoding_constraint, max_ppl, p, s));
  int cur = 0;
  UIC_TRY(tf.step(rows, 0, L.cache[cur], kmask_rows, B));              // get_logprobs_state(<bos>) (:466)
  const long long crow = (long long)d->layers * T * 3 * tf.dm;
  auto advance = [&](int t_next) -> int {
    // state = [ys]: the surviving parents' histories (CaptionModel.py:90-92) -- here their cached q | k | v rows
    UIC_TRY(uic_beam_gather_launch(d->dtype, p.parent, rows, B, (int)crow, L.cache[cur], L.cache[cur ^ 1], nullptr, nullptr, nullptr, nullptr,
                                   nullptr, nullptr, s));
    cur ^= 1;
    return tf.step(rows, t_next, L.cache[cur], kmask_rows, B);
  };
  return beam_search(p, Lsteps, advance, s, seq, seq_logp);
}

int uic_transformer_beam_done_lists(const uic_transformer_dims* d, void* workspace, int32_t Lsteps, int32_t beam_size, int32_t* done_count,
                                    float* done_p, int64_t* done_seq, float* done_lp, void* stream) {
  UIC_TRY(tf_check(d));
  UIC_REQUIRE(workspace && done_count && done_p && done_seq && done_lp, "transformer_beam_done_lists: null pointer");
  UIC_REQUIRE(beam_size >= 1 && beam_size == d->beam && Lsteps >= 1 && Lsteps <= d->T, "transformer_beam_done_lists: bad sizes");
  hipStream_t s = (hipStream_t)stream;
  const TfLayout L = tf_layout(*d, workspace);
  return beam_done_lists(L.beam, d->N, Lsteps, beam_size, done_count, done_p, done_seq, done_lp, s);
}

}  // extern "C"
