// extern "C" surface of libuic_hip.so for the single operators + error reporting.
#include "uic_common.h"
#include "uic_host.h"
#include "../../include/uic_hip.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <math.h>

static thread_local char g_err[512] = "";

void uic_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
int uic_check_hip(hipError_t e, const char* what) {
  if (e == hipSuccess) return UIC_OK;
  uic_set_error("%s: %s", what, hipGetErrorString(e));
  return (int)e > 0 ? (int)e : 1;
}

// UicOptimParams of one optimizer step; Adam's bias corrections 1 - beta^step in double, as torch.optim.Adam computes them.
// `what` names the C entry in the error text.  A method's unused state pointers are dropped here, so no kernel can see them.
static int optim_params(const char* what, const uic_optim_config* c, float* p, const float* g, float* s0, float* s1, size_t n,
                        UicOptimParams* out) {
  UIC_REQUIRE(c, "%s: null config", what);
  const int states = uic_optim_state_count(c->method);
  UIC_REQUIRE(states >= 0, "%s: unknown method %d", what, c->method);
  UIC_REQUIRE(p && g && (states < 1 || s0) && (states < 2 || s1), "%s: null pointer", what);
  UIC_REQUIRE(c->step >= 1, "%s: step=%d must be >= 1", what, c->step);
  UIC_REQUIRE((c->max_norm > 0.f) == (c->sqnorm != nullptr), "%s: max_norm and sqnorm go together", what);
  UIC_REQUIRE(c->weight_decay >= 0.f, "%s: weight_decay=%f must be >= 0", what, (double)c->weight_decay);
  UicOptimParams a;
  a.method = c->method;
  a.p = p; a.g = g; a.s0 = states >= 1 ? s0 : nullptr; a.s1 = states >= 2 ? s1 : nullptr; a.n = n;
  a.lr = c->lr; a.alpha = c->alpha; a.beta = c->beta; a.eps = c->eps; a.weight_decay = c->weight_decay;
  a.bc1 = a.bc2 = 1.f;
  if (c->method == UIC_OPTIM_ADAM) {
    a.bc1 = (float)(1.0 - pow((double)c->alpha, (double)c->step));
    a.bc2 = (float)(1.0 - pow((double)c->beta, (double)c->step));
  }
  a.grad_scale = c->grad_scale;
  a.max_norm = c->max_norm; a.sqnorm = c->sqnorm; a.guard = c->skip_if_nonzero;
  *out = a;
  return UIC_OK;
}
static int optim_step(const char* what, const uic_optim_config* c, float* p, const float* g, float* s0, float* s1, size_t n, void* stream) {
  UicOptimParams a;
  const int rc = optim_params(what, c, p, g, s0, s1, n, &a);
  return rc ? rc : uic_optim_launch(a, (hipStream_t)stream);
}
static int optim_step_ranges(const char* what, const uic_optim_config* c, float* p, const float* g, float* s0, float* s1, int32_t n_ranges,
                             const uint64_t* lo, const uint64_t* hi, void* w_out, int32_t w_dtype, void* stream) {
  UicOptimParams a;
  const int rc = optim_params(what, c, p, g, s0, s1, 0, &a);
  if (rc) return rc;
  UIC_REQUIRE(n_ranges == 0 || (lo && hi), "%s: null pointer", what);
  UIC_REQUIRE(n_ranges >= 0 && n_ranges <= UIC_OPTIM_RANGES, "%s: %d ranges (max %d)", what, n_ranges, UIC_OPTIM_RANGES);
  UIC_REQUIRE(!w_out || w_dtype == UIC_F32 || w_dtype == UIC_BF16, "%s: bad w_dtype %d", what, w_dtype);
  UicOptimRanges r;
  memset(&r, 0, sizeof(r));
  for (int i = 0; i < n_ranges; ++i) {
    UIC_REQUIRE(hi[i] >= lo[i], "%s: range %d is [%llu, %llu)", what, i, (unsigned long long)lo[i], (unsigned long long)hi[i]);
    if (hi[i] == lo[i]) continue;
    r.lo[r.count] = (size_t)lo[i]; r.start[r.count] = r.total; r.total += (size_t)(hi[i] - lo[i]); ++r.count;
  }
  return uic_optim_ranges_launch(a, r, w_out, w_dtype, (hipStream_t)stream);
}
// the uic_adam_* entries' arguments as a config (no weight decay: their bits are those of before uic_optim_step existed)
static uic_optim_config adam_config(float lr, float beta1, float beta2, float eps, int32_t step, float grad_scale, float max_norm,
                                    const float* sqnorm, const int32_t* guard) {
  uic_optim_config c;
  c.method = UIC_OPTIM_ADAM; c.lr = lr; c.alpha = beta1; c.beta = beta2; c.eps = eps; c.weight_decay = 0.f; c.step = step;
  c.grad_scale = grad_scale; c.max_norm = max_norm; c.sqnorm = sqnorm; c.skip_if_nonzero = guard;
  return c;
}

extern "C" {

const char* uic_last_error_string(void) { return g_err; }
int uic_version(void) { return 100; }

int uic_linear(int32_t dtype, int32_t M, int32_t N, int32_t K, const void* A, int32_t lda, const void* B, int32_t ldb,
               void* C, int32_t ldc, const float* bias, int32_t flags, void* stream) {
  UicGemmParams g;
  memset(&g, 0, sizeof(g));
  g.dtype = dtype; g.M = M; g.N = N; g.nseg = 1;
  g.seg[0].A = A; g.seg[0].B = B; g.seg[0].K = K; g.seg[0].lda = lda; g.seg[0].ldb = ldb;
  g.C = C; g.ldc = ldc; g.bias = bias; g.flags = flags;
  return uic_gemm_launch(g, (hipStream_t)stream);
}

int uic_linear_f32a(int32_t M, int32_t N, int32_t K, const float* A, int32_t lda, const void* B, int32_t ldb,
                    void* C, int32_t ldc, const float* bias, int32_t flags, void* a_bf16, int32_t ld_a_bf16, void* stream) {
  UIC_REQUIRE(A && B && C, "linear_f32a: null pointer");
  UicGemmParams g;
  memset(&g, 0, sizeof(g));
  g.dtype = UIC_BF16; g.M = M; g.N = N; g.nseg = 1;
  g.seg[0].A = A; g.seg[0].B = B; g.seg[0].K = K; g.seg[0].lda = lda; g.seg[0].ldb = ldb;
  g.C = C; g.ldc = ldc; g.bias = bias; g.flags = flags;
  g.a_f32 = 1; g.a_copy = a_bf16; g.ld_a_copy = ld_a_bf16;
  UIC_REQUIRE(uic_gemm_pp_eligible(g), "linear_f32a: needs K %% 128 == 0, N %% 4 == 0, lda %% 4 == 0, 16-byte aligned operands, "
              "ld_a_bf16 %% 8 == 0 and >= K, A below 4 GB (M=%d N=%d K=%d lda=%d)", M, N, K, lda);
  return uic_gemm_launch(g, (hipStream_t)stream);
}

int uic_linear_partials(int32_t dtype, int32_t M, int32_t N, int32_t K, const void* A, int32_t lda, const void* B, int32_t ldb,
                        float* slab, int32_t splitk, void* stream) {
  UIC_REQUIRE(slab && splitk >= 1 && splitk <= 16, "linear_partials: slab / splitk=%d", splitk);
  UIC_REQUIRE(uic_gemm_glds_eligible(dtype, K), "linear_partials: K=%d must be a multiple of one 128-byte round", K);
  UicGemmParams g;
  memset(&g, 0, sizeof(g));
  g.dtype = dtype; g.M = M; g.N = N; g.nseg = 1;
  g.seg[0].A = A; g.seg[0].B = B; g.seg[0].K = K; g.seg[0].lda = lda; g.seg[0].ldb = ldb;
  g.slab = slab; g.splitk = splitk;
  return uic_gemm_launch(g, (hipStream_t)stream);
}

int uic_linear_partials_rows(int32_t dtype, int32_t M, int32_t N, int32_t K, const void* A, int32_t lda, const void* B, int32_t ldb,
                             float* slab, int32_t splitk, const int32_t* row_map, int32_t slab_rows, void* stream) {
  if (!row_map) return uic_linear_partials(dtype, M, N, K, A, lda, B, ldb, slab, splitk, stream);
  UIC_REQUIRE(slab && splitk >= 1 && splitk <= 16, "linear_partials_rows: slab / splitk=%d", splitk);
  UIC_REQUIRE(uic_gemm_glds_eligible(dtype, K), "linear_partials_rows: K=%d must be a multiple of one 128-byte round", K);
  UIC_REQUIRE(M >= 1 && slab_rows >= M, "linear_partials_rows: M=%d must be in [1, slab_rows=%d]", M, slab_rows);
  UicGemmParams g;
  memset(&g, 0, sizeof(g));
  g.dtype = dtype; g.M = M; g.N = N; g.nseg = 1;
  g.seg[0].A = A; g.seg[0].B = B; g.seg[0].K = K; g.seg[0].lda = lda; g.seg[0].ldb = ldb;
  g.slab = slab; g.splitk = splitk; g.slab_row_map = row_map; g.slab_rows = slab_rows;
  return uic_gemm_launch(g, (hipStream_t)stream);
}

int uic_linear_wgrad(int32_t dtype, int32_t M, int32_t N, int32_t K, const void* dY, int32_t ldy, const void* X, int32_t ldx,
                     float* dW, int32_t ldw, void* workspace, size_t workspace_bytes, int32_t accumulate, void* stream) {
  UIC_REQUIRE(dY && X && dW && workspace, "linear_wgrad: null pointer");
  UIC_REQUIRE(dtype == UIC_BF16, "linear_wgrad: the transposing-read kernel is bf16 only (dtype=%d)", dtype);
  const WDest d1{dW, ldw, 0, N};
  const UicGemmTnSeg seg{X, ldx, N};
  bool done = false;
  UIC_TRY(wgrad_tn((float*)workspace, workspace_bytes, dtype, dY, ldy, M, &seg, 1, K, &d1, 1, (hipStream_t)stream, (accumulate & 1) != 0, &done,
                   accumulate & (UIC_TN_FORCE_128 | UIC_TN_FORCE_256 | UIC_TN_SPLITK(0xff))));
  UIC_REQUIRE(done, "linear_wgrad: shape M=%d N=%d K=%d not eligible (needs M >= 128, M %% 8 == 0, N %% 128 == 0, K %% 64 == 0, "
                    "16-byte aligned rows) or workspace of %zu bytes too small", M, N, K, workspace_bytes);
  return UIC_OK;
}

int uic_lstm_cell_fwd(int32_t dtype, int32_t M, int32_t H, int32_t nx, const void* const* x, const int32_t* Kx,
                      const void* const* Wx, const int32_t* ldw, const void* h, const void* W_hh,
                      const float* b_ih, const float* b_hh, const float* c_prev, float* c_out, void* h_out,
                      void* gates_out, void* stream) {
  UIC_REQUIRE(nx >= 0 && nx <= 3, "lstm_cell_fwd: nx=%d outside [0,3]", nx);
  UicGemmParams g;
  memset(&g, 0, sizeof(g));
  g.dtype = dtype; g.M = M; g.N = 4 * H; g.lstm = 1; g.H = H;
  for (int i = 0; i < nx; ++i) {
    UicGemmSeg& s = g.seg[g.nseg++];
    s.A = x[i]; s.B = Wx[i]; s.K = Kx[i]; s.lda = Kx[i]; s.ldb = ldw[i];
  }
  if (h) {
    UicGemmSeg& s = g.seg[g.nseg++];
    s.A = h; s.B = W_hh; s.K = H; s.lda = H; s.ldb = H;
  }
  g.bias = b_ih; g.bias2 = b_hh; g.c_prev = c_prev; g.c_out = c_out; g.h_out = h_out; g.ldh = H; g.gates_out = gates_out;
  return uic_gemm_launch(g, (hipStream_t)stream);
}

int uic_lstm_cell_bwd_sources(int32_t dtype, int32_t M, int32_t H, const float* dh0, int32_t lddh0, float drop_p, uint32_t seed,
                              uint32_t site, const float* dh1, int32_t lddh1, const float* dh2, int32_t lddh2,
                              const float* slabA, int32_t ldA, int32_t nA, size_t strideA,
                              const float* slabB, int32_t ldB, int32_t nB, size_t strideB,
                              float* dc, const void* gates, const float* c_prev, const float* c, void* dgates,
                              int32_t* kernel_id, void* stream) {
  UIC_REQUIRE(dtype == UIC_F32 || dtype == UIC_BF16, "lstm_cell_bwd_sources: dtype=%d", dtype);
  UicLstmBwdParams p;
  memset(&p, 0, sizeof(p));
  p.dtype = dtype; p.M = M; p.H = H;
  p.dh0 = dh0; p.lddh0 = lddh0; p.drop_p = drop_p; p.seed = seed; p.site = site;
  p.dh1 = dh1; p.lddh1 = lddh1; p.dh2 = dh2; p.lddh2 = lddh2;
  p.slabA = slabA; p.ldA = ldA; p.nA = nA; p.strideA = strideA;
  p.slabB = slabB; p.ldB = ldB; p.nB = nB; p.strideB = strideB;
  p.dc = dc; p.gates = gates; p.c_prev = c_prev; p.c = c; p.dgates = dgates;
  return uic_lstm_bwd_launch(p, (hipStream_t)stream, kernel_id);
}

int uic_lstm_cell_bwd(int32_t dtype, int32_t M, int32_t H, const float* dh, float* dc, const void* gates,
                      const float* c_prev, const float* c, void* dgates, void* stream) {
  return uic_lstm_cell_bwd_sources(dtype, M, H, dh, H, 0.f, 0, 0, nullptr, 0, nullptr, 0, nullptr, 0, 0, 0, nullptr, 0, 0, 0, dc, gates,
                                   c_prev, c, dgates, nullptr, stream);
}

int uic_maxout_lstm_cell_bwd(int32_t dtype, int32_t M, int32_t H, const float* dh0, int32_t lddh0, const float* dh1, int32_t lddh1,
                             float drop_p, uint32_t seed, uint32_t site, float* dc, const void* gates, const float* c_prev,
                             const float* c, void* dgates, void* stream) {
  UIC_REQUIRE(dtype == UIC_F32 || dtype == UIC_BF16, "maxout_lstm_cell_bwd: dtype=%d", dtype);
  UicLstmBwdParams p;
  memset(&p, 0, sizeof(p));
  p.dtype = dtype; p.M = M; p.H = H;
  p.dh0 = dh0; p.lddh0 = lddh0; p.dh1 = dh1; p.lddh1 = lddh1; p.drop_p = drop_p; p.seed = seed; p.site = site;
  p.dc = dc; p.gates = gates; p.c_prev = c_prev; p.c = c; p.dgates = dgates;
  return uic_maxout_lstm_bwd_launch(p, (hipStream_t)stream);
}

int uic_h2att_cell_bwd(int32_t dtype, int32_t N, int32_t H, int32_t A, const void* datth, const void* h2attT,
                       const float* slabA, int32_t ldA, int32_t nA, size_t strideA,
                       const float* slabB, int32_t ldB, int32_t nB, size_t strideB,
                       float* dc, const void* gates, const float* c_prev, const float* c, void* dgates, void* stream) {
  UicH2attCellParams p;
  memset(&p, 0, sizeof(p));
  p.dtype = dtype; p.N = N; p.H = H; p.A = A; p.datth = datth; p.h2attT = h2attT;
  p.slabA = slabA; p.ldA = ldA; p.nA = nA; p.strideA = strideA;
  p.slabB = slabB; p.ldB = ldB; p.nB = nB; p.strideB = strideB;
  p.dc = dc; p.gates = gates; p.c_prev = c_prev; p.c = c; p.dgates = dgates;
  return uic_h2att_cell_bwd_launch(p, (hipStream_t)stream);
}

int uic_lstm_cell_bwd_live(int32_t M, int32_t H, const float* dh0, int32_t lddh0, float drop_p, uint32_t seed, uint32_t site,
                           const float* slabA, int32_t ldA, int32_t nA, size_t strideA,
                           const float* slabB, int32_t ldB, int32_t nB, size_t strideB,
                           float* dc, const void* gates, const float* c_prev, const float* c, void* dgates,
                           const int32_t* row_len, const int32_t* rank, int32_t step, void* dgates_c, void* stream) {
  UicLstmBwdParams p;
  memset(&p, 0, sizeof(p));
  p.dtype = UIC_BF16; p.M = M; p.H = H;
  p.dh0 = dh0; p.lddh0 = lddh0; p.drop_p = drop_p; p.seed = seed; p.site = site;
  p.slabA = slabA; p.ldA = ldA; p.nA = nA; p.strideA = strideA;
  p.slabB = slabB; p.ldB = ldB; p.nB = nB; p.strideB = strideB;
  p.dc = dc; p.gates = gates; p.c_prev = c_prev; p.c = c; p.dgates = dgates;
  p.row_len = row_len; p.rank = rank; p.step = step; p.dgates_c = dgates_c;
  return uic_lstm_bwd_launch(p, (hipStream_t)stream);
}

int uic_h2att_cell_bwd_live(int32_t N, int32_t H, int32_t A, const void* datth, const void* h2attT,
                            const float* slabA, int32_t ldA, int32_t nA, size_t strideA,
                            const float* slabB, int32_t ldB, int32_t nB, size_t strideB,
                            float* dc, const void* gates, const float* c_prev, const float* c, void* dgates,
                            const int32_t* row_len, const int32_t* rank, int32_t step, void* dgates_c, void* stream) {
  UicH2attCellParams p;
  memset(&p, 0, sizeof(p));
  p.dtype = UIC_BF16; p.N = N; p.H = H; p.A = A; p.datth = datth; p.h2attT = h2attT;
  p.slabA = slabA; p.ldA = ldA; p.nA = nA; p.strideA = strideA;
  p.slabB = slabB; p.ldB = ldB; p.nB = nB; p.strideB = strideB;
  p.dc = dc; p.gates = gates; p.c_prev = c_prev; p.c = c; p.dgates = dgates;
  p.row_len = row_len; p.rank = rank; p.step = step; p.dgates_c = dgates_c;
  return uic_h2att_cell_bwd_launch(p, (hipStream_t)stream);
}

int uic_live_order(const float* masks, int32_t ld, int32_t col0, int32_t N, int32_t T, int32_t* row_len, int32_t* order, int32_t* rank,
                   int32_t* unfinished, const int32_t* expect, uint32_t* status, void* stream) {
  UIC_REQUIRE(masks && row_len && order && rank && unfinished && ld >= col0 + T && col0 >= 0, "live_order: null pointer or ld=%d < col0 + T", ld);
  UIC_REQUIRE(uic_live_order_ok(N, T), "live_order: N=%d outside [1, 4096] or T=%d outside [1, %d]", N, T, UIC_MAX_LIVE_STEPS);
  const UicLiveOrder ord{order, rank, unfinished, expect, status};
  // (the list itself is not wanted: out_len = 0 writes nothing through `out`)
  return uic_live_list_launch(masks, ld, col0, N, T * N, order, 0, (hipStream_t)stream, nullptr, nullptr, 0, row_len, &ord);
}

int uic_attention_fwd_strided(int32_t dtype, int32_t N, int32_t R, int32_t A, int32_t H, const float* att_h, const void* p_att,
                              const void* att, const float* w_alpha, const float* b_alpha, const float* mask, int32_t ld_mask,
                              float* alpha, void* ctx, int32_t ld_ctx, int32_t* kernel_id, void* stream) {
  UicAttnParams a;
  memset(&a, 0, sizeof(a));
  a.dtype = dtype; a.N = N; a.R = R; a.A = A; a.H = H; a.att_h = att_h; a.p_att = p_att; a.att = att;
  a.w_alpha = w_alpha; a.b_alpha = b_alpha; a.mask = mask; a.ldmask = ld_mask; a.alpha = alpha; a.ctx = ctx; a.ldctx = ld_ctx;
  return uic_attention_fwd_launch(a, (hipStream_t)stream, kernel_id);
}
int uic_attention_fwd(int32_t dtype, int32_t N, int32_t R, int32_t A, int32_t H, const float* att_h, const void* p_att,
                      const void* att, const float* w_alpha, const float* b_alpha, const float* mask, float* alpha,
                      void* ctx, void* stream) {
  return uic_attention_fwd_strided(dtype, N, R, A, H, att_h, p_att, att, w_alpha, b_alpha, mask, R, alpha, ctx, H, nullptr, stream);
}
int uic_attention_bwd_step_sources(int32_t dtype, int32_t N, int32_t R, int32_t A, int32_t H, const float* att_h,
                                   const void* p_att, const void* att, const float* w_alpha, const float* alpha,
                                   const float* dctx, int32_t lddctx, int32_t nslab, size_t slab_stride,
                                   float* dctx_sum, int32_t ld_dctx_sum, const int32_t* row_len, int32_t step,
                                   float* de, void* d_att_h, int32_t* kernel_id, void* stream) {
  UicAttnParams a;
  memset(&a, 0, sizeof(a));
  a.dtype = dtype; a.N = N; a.R = R; a.A = A; a.H = H; a.att_h = att_h; a.p_att = p_att; a.att = att;
  a.w_alpha = w_alpha; a.alpha = (float*)alpha; a.dctx = dctx; a.lddctx = lddctx; a.dctx_nslab = nslab; a.dctx_slab_stride = slab_stride;
  a.dctx_sum = dctx_sum; a.ld_dctx_sum = ld_dctx_sum; a.row_len = row_len; a.step = step; a.de = de; a.d_att_h = d_att_h;
  return uic_attention_bwd_step_launch(a, (hipStream_t)stream, kernel_id);
}
int uic_attention_bwd_step(int32_t dtype, int32_t N, int32_t R, int32_t A, int32_t H, const float* att_h,
                           const void* p_att, const void* att, const float* w_alpha, const float* alpha,
                           const float* dctx, float* de, void* d_att_h, void* stream) {
  return uic_attention_bwd_step_sources(dtype, N, R, A, H, att_h, p_att, att, w_alpha, alpha, dctx, H, 0, 0, nullptr, 0, nullptr, 0,
                                        de, d_att_h, nullptr, stream);
}
int uic_attention_bwd_accum_strided(int32_t dtype, int32_t N, int32_t R, int32_t A, int32_t H, int32_t T,
                                    const float* att_h_all, const float* alpha_all, const float* de_all, const float* dctx_all,
                                    int32_t lddctx, size_t dctx_step_stride, const int32_t* row_len,
                                    const void* p_att, const float* w_alpha, float* d_att, void* d_p_att, float* d_walpha_part,
                                    int32_t* kernel_id, void* stream) {
  UicAttnAccumParams a;
  memset(&a, 0, sizeof(a));
  a.dtype = dtype; a.N = N; a.R = R; a.A = A; a.H = H; a.T = T;
  a.att_h_all = att_h_all; a.alpha_all = alpha_all; a.de_all = de_all;
  a.dctx_all = dctx_all; a.lddctx = lddctx; a.dctx_step_stride = dctx_step_stride; a.row_len = row_len;
  a.p_att = p_att; a.w_alpha = w_alpha; a.d_att = d_att; a.d_p_att = d_p_att; a.d_walpha_part = d_walpha_part;
  return uic_attention_bwd_accum_launch(a, (hipStream_t)stream, kernel_id);
}
int uic_attention_bwd_accum(int32_t dtype, int32_t N, int32_t R, int32_t A, int32_t H, int32_t T,
                            const float* att_h_all, const float* alpha_all, const float* de_all, const float* dctx_all,
                            const void* p_att, const float* w_alpha, float* d_att, void* d_p_att, float* d_walpha_part,
                            void* stream) {
  return uic_attention_bwd_accum_strided(dtype, N, R, A, H, T, att_h_all, alpha_all, de_all, dctx_all, H, (size_t)(N > 0 ? N : 0) * H,
                                         nullptr, p_att, w_alpha, d_att, d_p_att, d_walpha_part, nullptr, stream);
}

int uic_optim_states(int32_t method) { return uic_optim_state_count(method); }

int uic_optim_step(const uic_optim_config* cfg, float* p, const float* g, float* s0, float* s1, size_t n, void* stream) {
  return optim_step("optim_step", cfg, p, g, s0, s1, n, stream);
}

int uic_optim_step_ranges(const uic_optim_config* cfg, float* p, const float* g, float* s0, float* s1, int32_t n_ranges,
                          const uint64_t* lo, const uint64_t* hi, void* w_out, int32_t w_dtype, void* stream) {
  return optim_step_ranges("optim_step_ranges", cfg, p, g, s0, s1, n_ranges, lo, hi, w_out, w_dtype, stream);
}

int uic_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                  float eps, int32_t step, float grad_scale, void* stream) {
  const uic_optim_config c = adam_config(lr, beta1, beta2, eps, step, grad_scale, 0.f, nullptr, nullptr);
  return optim_step("adam_step", &c, p, g, m, v, n, stream);
}

int uic_adam_step_guarded(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                          float eps, int32_t step, float grad_scale, const int32_t* skip_if_nonzero, void* stream) {
  const uic_optim_config c = adam_config(lr, beta1, beta2, eps, step, grad_scale, 0.f, nullptr, skip_if_nonzero);
  return optim_step("adam_step_guarded", &c, p, g, m, v, n, stream);
}

int uic_grad_sqnorm(const float* g, size_t n, float* scratch, float* out, void* stream) {
  return uic_sqnorm_launch(g, n, scratch, out, (hipStream_t)stream);
}

int uic_grad_sqnorm_f64(const float* g, size_t n, float* scratch, float* out, void* stream) {
  return uic_sqnorm_f64_launch(g, n, scratch, out, (hipStream_t)stream);
}

int uic_adam_step_clip(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                       float eps, int32_t step, float grad_scale, float max_norm, const float* sqnorm, void* stream) {
  UIC_REQUIRE(sqnorm && max_norm > 0.f, "adam_step_clip: sqnorm must be given and max_norm=%f > 0", (double)max_norm);
  const uic_optim_config c = adam_config(lr, beta1, beta2, eps, step, grad_scale, max_norm, sqnorm, nullptr);
  return optim_step("adam_step_clip", &c, p, g, m, v, n, stream);
}

int uic_adam_step_clip_guarded(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                               float eps, int32_t step, float grad_scale, float max_norm, const float* sqnorm,
                               const int32_t* skip_if_nonzero, void* stream) {
  UIC_REQUIRE(sqnorm && max_norm > 0.f, "adam_step_clip_guarded: sqnorm must be given and max_norm=%f > 0", (double)max_norm);
  const uic_optim_config c = adam_config(lr, beta1, beta2, eps, step, grad_scale, max_norm, sqnorm, skip_if_nonzero);
  return optim_step("adam_step_clip_guarded", &c, p, g, m, v, n, stream);
}

int uic_adam_step_ranges(float* p, const float* g, float* m, float* v, int32_t n_ranges, const uint64_t* lo, const uint64_t* hi,
                         float lr, float beta1, float beta2, float eps, int32_t step, float grad_scale, float max_norm,
                         const float* sqnorm, const int32_t* skip_if_nonzero, void* w_out, int32_t w_dtype, void* stream) {
  const uic_optim_config c = adam_config(lr, beta1, beta2, eps, step, grad_scale, max_norm, sqnorm, skip_if_nonzero);
  return optim_step_ranges("adam_step_ranges", &c, p, g, m, v, n_ranges, lo, hi, w_out, w_dtype, stream);
}

int uic_lm_criterion(int32_t N, int32_t T, int32_t V1, const float* logp, const int64_t* target, int32_t ld_target,
                     const float* mask, int32_t ld_mask, float* loss_out, float* scratch, float* dlogp, float grad_out,
                     void* stream) {
  UIC_REQUIRE(logp && target && mask && loss_out && scratch, "lm_criterion: null pointer");
  return uic_lm_crit_launch(N, T, V1, logp, target, ld_target, mask, ld_mask, loss_out, scratch, dlogp, grad_out, (hipStream_t)stream);
}

int uic_reward_criterion(int32_t N, int32_t L, const float* logp, const int64_t* seq, const float* reward, float* loss_out,
                         float* dlogp, void* stream) {
  UIC_REQUIRE(logp && seq && reward && loss_out, "reward_criterion: null pointer");
  UIC_REQUIRE(N > 0 && L > 0, "reward_criterion: empty input");
  return uic_reward_crit_launch(N, L, logp, seq, reward, loss_out, dlogp, (hipStream_t)stream);
}

int uic_xe_criterion(int32_t dtype, int32_t M, int32_t N, int32_t V1, int32_t ldv, const float* logits, void* dlogits,
                     const int64_t* target, int32_t ld_target, int32_t target_col0,
                     const float* mask, int32_t ld_mask, int32_t mask_col0, const float* inv_den,
                     const float* grad_scale, int32_t ld_scale, int32_t scale_col0,
                     float* row_loss, float* logprobs, size_t lp_step_stride, size_t lp_row_stride, int32_t* score_stats,
                     const int32_t* row_map, int32_t row_map_limit, int32_t* kernel_id, void* stream) {
  UIC_REQUIRE(dtype == UIC_F32 || dtype == UIC_BF16, "xe_criterion: bad dtype %d", dtype);
  UIC_REQUIRE(M >= 0 && N > 0 && V1 > 0 && ldv >= V1, "xe_criterion: M=%d N=%d V1=%d ldv=%d", M, N, V1, ldv);
  UIC_REQUIRE(target || logprobs, "xe_criterion: nothing to compute (no target, no logprobs)");
  UicXeParams x;
  memset(&x, 0, sizeof(x));
  x.dtype = dtype; x.M = M; x.N = N; x.V1 = V1; x.ldv = ldv; x.logits = logits; x.dlogits = dlogits; x.write_grad = dlogits != nullptr;
  x.target = target; x.ldtarget = ld_target; x.target_col0 = target_col0;
  x.mask = mask; x.ldmask = ld_mask; x.mask_col0 = mask_col0; x.inv_den = inv_den;
  x.grad_scale = grad_scale; x.ldscale = ld_scale; x.scale_col0 = scale_col0;
  x.row_loss = row_loss; x.logprobs = logprobs; x.lp_step_stride = lp_step_stride; x.lp_row_stride = lp_row_stride;
  x.score_stats = score_stats; x.row_map = row_map; x.row_map_limit = row_map_limit;
  return uic_xe_launch(x, (hipStream_t)stream, kernel_id);
}

// BatchNorm1d of att_embed on its own: argument checks here, the launchers of csrc/batchnorm.hip do the work
#define UIC_BN_DTYPE(dt, who) UIC_REQUIRE((dt) == UIC_F32 || (dt) == UIC_BF16, who ": bad dtype %d", (int)(dt))
#define UIC_BN_SHAPE(who)                                                                                        \
  UIC_REQUIRE(NR > 0 && C > 0 && C % 4 == 0, who ": NR=%d C=%d (NR > 0, C a positive multiple of 4)", NR, C);   \
  UIC_REQUIRE(!row_len || R > 0, who ": R=%d with a row_len", R)

size_t uic_batchnorm_scratch_floats(int32_t NR, int32_t C) {
  if (NR <= 0 || C <= 0 || C % 4 != 0) {
    uic_set_error("batchnorm_scratch_floats: NR=%d C=%d (NR > 0, C a positive multiple of 4)", NR, C);
    return 0;
  }
  return uic_bn_scratch_floats(NR, C);
}

int uic_batchnorm_stats(int32_t in_dtype, const void* x, int32_t NR, int32_t R, int32_t C, const int32_t* row_len, float* part,
                        float momentum, float eps, int32_t rep, float* stat, float* run_mean, float* run_var, void* stream) {
  UIC_BN_DTYPE(in_dtype, "batchnorm_stats");
  UIC_REQUIRE(x && part && stat, "batchnorm_stats: null pointer");
  UIC_BN_SHAPE("batchnorm_stats");
  UIC_REQUIRE(rep >= 1, "batchnorm_stats: rep=%d must be >= 1", rep);
  return uic_bn_stats_launch(in_dtype, x, NR, R, C, row_len, part, momentum, eps, stat, run_mean, run_var, (hipStream_t)stream, (float)rep);
}

int uic_batchnorm_stats_running(const float* run_mean, const float* run_var, int32_t C, float eps, float* stat, void* stream) {
  UIC_REQUIRE(run_mean && run_var && stat, "batchnorm_stats_running: null pointer");
  UIC_REQUIRE(C > 0 && C % 4 == 0, "batchnorm_stats_running: C=%d must be a positive multiple of 4", C);
  return uic_bn_stats_running_launch(run_mean, run_var, C, eps, stat, (hipStream_t)stream);
}

int uic_batchnorm_apply(int32_t in_dtype, int32_t out_dtype, const void* x, int32_t NR, int32_t R, int32_t C, const int32_t* row_len,
                        const float* stat, const float* gamma, const float* beta, int32_t zero_padded, void* out, void* stream) {
  UIC_BN_DTYPE(in_dtype, "batchnorm_apply");
  UIC_BN_DTYPE(out_dtype, "batchnorm_apply");
  UIC_REQUIRE(x && stat && out, "batchnorm_apply: null pointer");
  UIC_BN_SHAPE("batchnorm_apply");
  return uic_bn_apply_launch(in_dtype, out_dtype, x, NR, R, C, row_len, stat, gamma, beta, zero_padded, out, (hipStream_t)stream);
}

int uic_batchnorm_backward(int32_t dtype, float* d, const void* y, int32_t NR, int32_t R, int32_t C, const int32_t* row_len,
                           const float* stat, const float* gamma, int32_t training, float* part, float* red, float* dgamma,
                           float* dbeta, void* stream) {
  UIC_BN_DTYPE(dtype, "batchnorm_backward");
  UIC_REQUIRE(d && y && stat && gamma && part && red, "batchnorm_backward: null pointer");
  UIC_BN_SHAPE("batchnorm_backward");
  return uic_bn_bwd_launch(dtype, d, y, NR, R, C, row_len, stat, gamma, training, part, red, dgamma, dbeta, (hipStream_t)stream);
}

int uic_batchnorm_fold_weight(int32_t dtype, const float* W, const float* gamma, const float* beta, const float* b, int32_t H,
                              int32_t D, void* Weff, float* beff, void* stream) {
  UIC_BN_DTYPE(dtype, "batchnorm_fold_weight");
  UIC_REQUIRE(W && gamma && beta && b && Weff && beff, "batchnorm_fold_weight: null pointer");
  UIC_REQUIRE(H > 0 && D > 0, "batchnorm_fold_weight: H=%d D=%d", H, D);
  return uic_bn_fold_weight_launch(dtype, W, gamma, beta, b, H, D, Weff, beff, (hipStream_t)stream);
}

int uic_batchnorm_fold_grad(const float* W, const float* gamma, const float* beta, float* dW, const float* db, int32_t H, int32_t D,
                            float* dgamma, float* dbeta, void* stream) {
  UIC_REQUIRE(W && gamma && beta && dW && db && dgamma && dbeta, "batchnorm_fold_grad: null pointer");
  UIC_REQUIRE(H > 0 && D > 0, "batchnorm_fold_grad: H=%d D=%d", H, D);
  return uic_bn_fold_grad_launch(W, gamma, beta, dW, db, H, D, dgamma, dbeta, (hipStream_t)stream);
}
#undef UIC_BN_DTYPE
#undef UIC_BN_SHAPE

// nn.Embedding (+ ReLU + Dropout) forward and its bucketed backward on their own: argument checks here, the launchers of
// csrc/embedding.hip do the work.  The alignments are those of the kernels' vector loads: f32 rows are read and stored as float4,
// a bf16 table and a bf16 xt as uint2; scratch holds the int4 loads of the scan and the float4 partial rows.
#define UIC_EMB_DTYPE(dt, who) UIC_REQUIRE((dt) == UIC_F32 || (dt) == UIC_BF16, who ": bad dtype %d", (int)(dt))
#define UIC_EMB_ALIGNED(p, bytes, who, name) \
  UIC_REQUIRE(((uintptr_t)(p) & (uintptr_t)((bytes) - 1)) == 0, who ": " name " must be %d-byte aligned", (int)(bytes))
#define UIC_EMB_SHAPE(who)                                                                                              \
  UIC_REQUIRE(E > 0 && E % 4 == 0 && V1 > 0, who ": E=%d V1=%d (E a positive multiple of 4, V1 > 0)", E, V1);            \
  UIC_REQUIRE(N >= 0 && T >= 0 && ld_tokens >= T, who ": N=%d T=%d ld_tokens=%d (N, T >= 0, ld_tokens >= T)", N, T, ld_tokens); \
  UIC_REQUIRE((int64_t)N * T < ((int64_t)1 << 30), who ": N * T = %lld positions (< 2^30)", (long long)N * T)
#define UIC_EMB_SPLIT(who) UIC_REQUIRE(split >= 0 && (split == 0 || split < T), who ": split=%d outside [0, T = %d)", split, T)

size_t uic_embedding_scratch_ints(int32_t N, int32_t T, int32_t V1, int32_t E) {
  if (N < 0 || T < 0 || V1 <= 0 || E <= 0 || E % 4 != 0 || (int64_t)N * T >= ((int64_t)1 << 30)) {
    uic_set_error("embedding_scratch_ints: N=%d T=%d V1=%d E=%d (N, T >= 0, N * T < 2^30, V1 > 0, E a positive multiple of 4)", N, T, V1, E);
    return 0;
  }
  return uic_embed_bwd_sorted_scratch_ints(N, T, V1, E);
}

int uic_embedding_forward(int32_t out_dtype, const void* table, int32_t table_dtype, int32_t V1, int32_t E, const int64_t* tokens,
                          int32_t ld_tokens, int32_t N, int32_t T, float drop_p, uint32_t seed, uint32_t site, size_t idx_base,
                          int32_t relu, void* out, void* stream) {
  UIC_EMB_DTYPE(out_dtype, "embedding_forward");
  UIC_EMB_DTYPE(table_dtype, "embedding_forward");
  UIC_REQUIRE(!(table_dtype == UIC_BF16 && out_dtype == UIC_F32), "embedding_forward: a bf16 table needs bf16 outputs");
  UIC_REQUIRE(table && tokens && out, "embedding_forward: null pointer");
  UIC_EMB_SHAPE("embedding_forward");
  UIC_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "embedding_forward: drop_p=%g outside [0, 1)", (double)drop_p);
  UIC_EMB_ALIGNED(table, table_dtype == UIC_BF16 ? 8 : 16, "embedding_forward", "table");
  UIC_EMB_ALIGNED(out, out_dtype == UIC_BF16 ? 2 : 4, "embedding_forward", "out");
  return uic_embed_fwd_t_launch(out_dtype, table, table_dtype, V1, E, tokens, ld_tokens, N, T, drop_p, seed, site, idx_base, relu, out,
                                (hipStream_t)stream);
}

int uic_embedding_backward_prepare(const int64_t* tokens, int32_t ld_tokens, int32_t N, int32_t T, int32_t V1, int32_t E, float* dtable,
                                   int32_t* scratch, int32_t split, void* stream) {
  UIC_REQUIRE(tokens && dtable && scratch, "embedding_backward_prepare: null pointer");
  UIC_EMB_SHAPE("embedding_backward_prepare");
  UIC_EMB_SPLIT("embedding_backward_prepare");
  UIC_EMB_ALIGNED(dtable, 16, "embedding_backward_prepare", "dtable");
  UIC_EMB_ALIGNED(scratch, 16, "embedding_backward_prepare", "scratch");
  return uic_embed_bwd_sorted_prepare(tokens, ld_tokens, N, T, V1, E, dtable, scratch, (hipStream_t)stream, split);
}

int uic_embedding_backward_gather(int32_t dtype, const float* dxt, const void* xt, const int64_t* tokens, int32_t ld_tokens, int32_t N,
                                  int32_t T, int32_t V1, int32_t E, float drop_p, int64_t skip_token, float* dtable, int32_t* scratch,
                                  int32_t split, int32_t half, void* stream) {
  UIC_EMB_DTYPE(dtype, "embedding_backward_gather");
  UIC_REQUIRE(dxt && tokens && dtable && scratch, "embedding_backward_gather: null pointer");
  UIC_EMB_SHAPE("embedding_backward_gather");
  UIC_EMB_SPLIT("embedding_backward_gather");
  UIC_REQUIRE((half == 0 || half == 1) && !(half && split == 0), "embedding_backward_gather: half=%d with split=%d (0 or 1; 1 only with a split)",
              half, split);
  UIC_REQUIRE(skip_token < V1, "embedding_backward_gather: skip_token=%lld outside the table (V1=%d; < 0 = none)", (long long)skip_token, V1);
  UIC_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "embedding_backward_gather: drop_p=%g outside [0, 1)", (double)drop_p);
  UIC_EMB_ALIGNED(dxt, 16, "embedding_backward_gather", "dxt");
  UIC_EMB_ALIGNED(xt, dtype == UIC_BF16 ? 8 : 16, "embedding_backward_gather", "xt");
  UIC_EMB_ALIGNED(dtable, 16, "embedding_backward_gather", "dtable");
  UIC_EMB_ALIGNED(scratch, 16, "embedding_backward_gather", "scratch");
  return uic_embed_bwd_sorted_gather(dtype, dxt, xt, tokens, ld_tokens, N, T, V1, E, drop_p, (long)skip_token, dtable, scratch,
                                     (hipStream_t)stream, split, half);
}

int uic_embedding_backward(int32_t dtype, const float* dxt, const void* xt, const int64_t* tokens, int32_t ld_tokens, int32_t N, int32_t T,
                           int32_t V1, int32_t E, float drop_p, int64_t skip_token, float* dtable, int32_t* scratch, void* stream) {
  // (every check before the first launch: a refused call leaves dtable as it was)
  UIC_EMB_DTYPE(dtype, "embedding_backward");
  UIC_REQUIRE(dxt && tokens && dtable && scratch, "embedding_backward: null pointer");
  UIC_EMB_SHAPE("embedding_backward");
  UIC_REQUIRE(skip_token < V1, "embedding_backward: skip_token=%lld outside the table (V1=%d; < 0 = none)", (long long)skip_token, V1);
  UIC_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "embedding_backward: drop_p=%g outside [0, 1)", (double)drop_p);
  UIC_EMB_ALIGNED(dxt, 16, "embedding_backward", "dxt");
  UIC_EMB_ALIGNED(xt, dtype == UIC_BF16 ? 8 : 16, "embedding_backward", "xt");
  UIC_EMB_ALIGNED(dtable, 16, "embedding_backward", "dtable");
  UIC_EMB_ALIGNED(scratch, 16, "embedding_backward", "scratch");
  return uic_embed_bwd_sorted_launch(dtype, dxt, xt, tokens, ld_tokens, N, T, V1, E, drop_p, (long)skip_token, dtable, scratch,
                                     (hipStream_t)stream);
}
#undef UIC_EMB_DTYPE
#undef UIC_EMB_ALIGNED
#undef UIC_EMB_SHAPE
#undef UIC_EMB_SPLIT

int uic_cast_from_f32(int32_t dtype, const float* src, void* dst, size_t n, void* stream) {
  return uic_cast_f32_launch(dtype, src, dst, n, (hipStream_t)stream);
}
int uic_cast_to_f32(int32_t dtype, const void* src, float* dst, size_t n, void* stream) {
  return uic_to_f32_launch(dtype, src, dst, n, (hipStream_t)stream);
}
int uic_transpose(int32_t dtype, const void* src, int32_t rows, int32_t cols, int32_t ld_src, void* dst, int32_t ld_dst, void* stream) {
  return uic_transpose_launch(dtype, src, rows, cols, ld_src, dst, ld_dst, (hipStream_t)stream);
}
int uic_dropout_mask(float* out, size_t n, float p, uint32_t seed, uint32_t site, size_t base, void* stream) {
  return uic_dropout_mask_launch(out, n, p, seed, site, base, (hipStream_t)stream);
}

}  // extern "C"
