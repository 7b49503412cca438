// The generic persistent recurrence kernel (rnn_persist.hip's header comment: decomposition, visibility, GEMM phases): eight
// waves, weights re-read from L2 every step.  f32 -- the parity path -- is its one instantiation.
#include "rnn_persist_internal.h"
#include "rnn_persist_attn.h"

namespace {

// att_h = h2att(h_att) (P/models/AttModel.py:543): 16 columns of the group's rows
template <typename T, bool SAFE>
__device__ __forceinline__ void h2att_phase(Ctx& c, const T* h_att_new, const T* w, const float* b, float* att_h) {
  const bool owner = c.wave < c.MT;
  const int a = c.u0 + c.l15;
  const float bias = owner && b ? b[a] : 0.f;
  f32x4 acc[MT_MAX][1];
  zero_acc<1>(acc);
  const void* const As[1] = {h_att_new};
  const void* const Bs[1] = {w};
  const int ldb[1] = {HH};
  gemm_ksplit<T, 1, 1, false>(c, acc, As, Bs, ldb);
  f32x4* red = (f32x4*)c.smem;      // [wave][tile][lane]
#pragma unroll
  for (int i = 0; i < MT_MAX; ++i)
    if (i < c.MT) red[(c.wave * MT_MAX + i) * 64 + c.lane] = acc[i][0];
  __syncthreads();
  if (owner) {
    f32x4 s = red[(0 * MT_MAX + c.wave) * 64 + c.lane];
#pragma unroll
    for (int w2 = 1; w2 < NWAVE; ++w2) s += red[(w2 * MT_MAX + c.wave) * 64 + c.lane];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = 16 * c.wave + 4 * c.lq + r;
      if (rr < c.nrow) st_x<SAFE>(att_h + (unsigned)((c.rbegin + rr) * HH + a), s[r] + bias);
    }
  }
  __syncthreads();
}

template <typename T, bool SAFE>
__device__ __forceinline__ void run_steps(const UicRnnFwdParams& p, Ctx& c) {
  const int N = p.N;
  const size_t NH = (size_t)N * HH;
  const size_t rb = (size_t)c.rbegin * HH;
  const T* att_w_ih = (const T*)p.att_w_ih;
  const T* lang_w_ih = (const T*)p.lang_w_ih;
  unsigned long long* dbg = p.dbg ? p.dbg + ((size_t)blockIdx.x * p.dbg_T + p.t0) * 16 : nullptr;
  for (int t = p.t0; t < p.t1; ++t) {
    T* h_att_prev = (T*)p.h_att + (size_t)t * NH;
    T* h_att_new = h_att_prev + NH;
    T* h_lang_prev = (T*)p.h_lang + (size_t)t * NH;
    T* h_lang_new = h_lang_prev + NH;
    // hipcc hoists every step-invariant per-lane value (row offsets, dropout hashes, 64-bit addresses of all four phases)
    // out of this loop and then spills them; making the lane coordinates opaque once per step keeps them recomputed instead
    asm volatile("" : "+v"(c.lane), "+v"(c.l15), "+v"(c.lq), "+v"(c.tid));
    asm volatile("" : "+s"(c.wave), "+s"(c.u0), "+s"(c.rbegin), "+s"(c.nrow), "+s"(c.MT));
    c.dbg = dbg;
    if (dbg && c.tid == 0) dbg[0] = __builtin_amdgcn_s_memrealtime();
    {  // att_lstm on cat([h_lang_prev, fc', xt]) with the fc' / xt share precomputed in gx / gfc (:431-434)
      const void* const As[2] = {h_lang_prev + rb, h_att_prev + rb};
      const void* const Bs[2] = {att_w_ih, p.att_w_hh};
      const int ldb[2] = {p.ld_att_ih, HH};
      const float* gx = p.gx + (size_t)t * N * 4 * HH;
      const float* gfc = p.gfc;
      auto pre = [&](unsigned idx4, unsigned) { return gx[idx4] + (gfc ? gfc[idx4] : 0.f); };
      lstm_phase<T, SAFE, 2>(c, As, Bs, ldb, pre, p.c_att + (size_t)t * NH, p.c_att + (size_t)(t + 1) * NH, h_att_new,
                             (T*)nullptr, p.gates1 ? (T*)p.gates1 + (size_t)t * N * 4 * HH : nullptr, N, 0.f, 0u, 0u);
    }
    if (dbg && c.tid == 0) dbg[1] = __builtin_amdgcn_s_memrealtime();
    if (!group_barrier(c)) return;
    if (dbg && c.tid == 0) dbg[2] = __builtin_amdgcn_s_memrealtime();
    float* att_h = p.att_h_all + (size_t)t * NH;
    h2att_phase<T, SAFE>(c, h_att_new + rb, (const T*)p.h2att_w, p.h2att_b, att_h);
    if (dbg && c.tid == 0) dbg[3] = __builtin_amdgcn_s_memrealtime();
    if (!group_barrier(c)) return;
    if (dbg && c.tid == 0) dbg[4] = __builtin_amdgcn_s_memrealtime();
    T* ctx = (T*)p.ctx_all + (size_t)t * NH;
    attn_phase<T, SAFE, NWAVE, 3>(c, p, att_h, p.alpha_all + (size_t)t * N * p.R, ctx);
    if (dbg && c.tid == 0) dbg[5] = __builtin_amdgcn_s_memrealtime();
    if (!group_barrier(c)) return;
    if (dbg && c.tid == 0) dbg[6] = __builtin_amdgcn_s_memrealtime();
    {  // lang_lstm on cat([att_res, h_att]) (:438-441) + the output dropout (:443)
      const void* const As[3] = {ctx + rb, h_att_new + rb, h_lang_prev + rb};
      const void* const Bs[3] = {lang_w_ih, lang_w_ih + HH, p.lang_w_hh};
      const int ldb[3] = {2 * HH, 2 * HH, HH};
      const float* b1 = p.lang_b_ih;
      const float* b2 = p.lang_b_hh;
      auto pre = [&](unsigned, unsigned col) { return (b1 ? b1[col] : 0.f) + (b2 ? b2[col] : 0.f); };
      lstm_phase<T, SAFE, 3>(c, As, Bs, ldb, pre, p.c_lang + (size_t)t * NH, p.c_lang + (size_t)(t + 1) * NH, h_lang_new,
                             p.hdrop_all ? (T*)p.hdrop_all + (size_t)t * NH : nullptr,
                             p.gates2 ? (T*)p.gates2 + (size_t)t * N * 4 * HH : nullptr, N, p.drop_p, p.seed,
                             UIC_SITE_OUT0 + (unsigned)t);
    }
    if (dbg && c.tid == 0) dbg[7] = __builtin_amdgcn_s_memrealtime();
    if (!group_barrier(c)) return;
    if (dbg) dbg += 16;
  }
}

template <typename T>
__global__ __launch_bounds__(NTH) void rnn_fwd_persist_kernel(const UicRnnFwdParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Ctx c;
  const int mode = setup_ctx(p, smem, c);
  if (mode == 0) return;
  if (mode == 2) run_steps<T, true>(p, c);
  else run_steps<T, false>(p, c);
}

}  // namespace

int rnn_persist::generic_f32_launch(const UicRnnFwdParams& p, hipStream_t s) {
  static bool configured = false;
  if (!configured) {
    UIC_TRY(uic_check_hip(hipFuncSetAttribute((const void*)rnn_fwd_persist_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES), "hipFuncSetAttribute(rnn persist)"));
    configured = true;
  }
  hipLaunchKernelGGL(rnn_fwd_persist_kernel<float>, dim3(8 * PW), dim3(NTH), LDS_BYTES, s, p);
  UIC_LAUNCH_CHECK("rnn_fwd_persist_kernel");
  return UIC_OK;
}
