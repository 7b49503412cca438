// Persistent, step-fused recurrence of the TopDown captioner for gfx950 (MI355X): ONE launch runs decode steps
// [t0, t1) of AttModel._forward's loop body (P/models/AttModel.py:129-154 -> TopDownCore.forward :430-446 ->
// Attention.forward :538-558) -- att_lstm GEMM + cell, h2att, attention, lang_lstm GEMM + cell + output dropout --
// instead of four dependent launches per step.
//
// Why it can be split: every caption row's recurrence is independent of every other row's, only the weights are
// shared.  So the chip is cut into row GROUPS, one per XCD (32 CUs behind one 4 MB L2): group g owns caption rows
// [g*Rg, (g+1)*Rg) for all steps and never talks to another group.  Inside a group workgroup `rank` (one per CU) owns
// 16 hidden units = 64 gate columns of both LSTMs and 16 columns of h2att for all of the group's rows, and between 2
// and 3 of the group's rows in the attention phase; the only exchanged data are the rows' h_att / att_h / ctx /
// h_lang vectors (<= 80 rows x 512), which stay in that XCD's L2.  Phases are separated by a GROUP barrier (32
// arrivals on one counter) instead of a kernel boundary or a grid barrier.
//
// Visibility (MI355X_MICROARCH.md, inter-workgroup visibility): a CU's vector L1 is never refreshed by another CU's
// stores, the L2 of one XCD is shared by its CUs, the L2s of different XCDs are not coherent.  Groups are formed from
// the hardware's own XCC_ID register (never from blockIdx), so in the normal case all members of a group sit behind
// one L2: exchanged data are written with plain stores (they land in that L2), every storing wave drains vmcnt(0)
// before the workgroup arrives at the barrier, and EVERY load of exchanged data is an `sc1` load (bypasses the
// reader's L1).  If the dispatcher ever places the grid differently (an XCD with != 32 workgroups) the kernel runs in
// SAFE mode: groups by arrival ticket, exchanged data stored write-through (`sc1`) as well -- slower, still correct,
// so results never depend on placement.  Every spin is bounded; a timeout sets sync[SY_ERR] and the launch ends.
//
// GEMM phases: an output tile [<=80 rows] x [64 gate columns] per workgroup, K split over the 8 waves (wave w takes
// k-steps w, w+8, ...), operands go global -> VGPR directly in MFMA 16x16 fragment layout (no LDS staging: every
// operand byte is used by exactly one wave), the 8 partial tiles are summed through LDS and the cell update runs on
// the wave that owns the 16-row tile.  bf16 operands -> v_mfma_f32_16x16x32_bf16, f32 -> v_mfma_f32_16x16x4_f32.
//
// Files: this one holds the host side (the persist gate, the eligibility checks, uic_rnn_fwd_persist_launch and the three small
// kernels of the decode mode); rnn_persist_generic.hip the generic kernel (f32), rnn_persist_ws.hip the two weight-stationary bf16
// kernels, rnn_persist_attn.h the attention phases of both, rnn_persist_dec.h the decode pieces, rnn_persist_internal.h the
// launcher of each kernel, rnn_persist_common.h the protocol (shared with rnn_bwd_persist.hip and nmt_persist.hip).
#include "rnn_persist_internal.h"
#include <mutex>

namespace {

// relu(embed) in bf16: what every decode step gathers its input rows from (dropout, where the pass has it, is applied to the
// gathered values; with the reference's p = 0.5 that is exactly dropout(relu(embed)) rounded once, otherwise within one bf16 ulp)
__global__ void dec_embed_relu_kernel(const float* __restrict__ w, bf16_t* __restrict__ out, size_t n4) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 v = *(const float4*)(w + 4 * i);
    *(uint2*)(out + 4 * i) = make_uint2(uic_pack_bf16x2(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f)), uic_pack_bf16x2(fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)));
  }
}
// the same from the bf16 copy of the table (relu of a bf16 value: clear the halves whose sign bit is set)
__global__ void dec_embed_relu16_kernel(const uint2* __restrict__ w, uint2* __restrict__ out, size_t n4) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    uint2 v = w[i];
    if (v.x & 0x8000u) v.x &= 0xFFFF0000u;
    if (v.x & 0x80000000u) v.x &= 0x0000FFFFu;
    if (v.y & 0x8000u) v.y &= 0xFFFF0000u;
    if (v.y & 0x80000000u) v.y &= 0x0000FFFFu;
    out[i] = v;
  }
}

// the reference stops decoding once every row has finished (AttModel.py:236-238): entries after that step stay zero.
// status[0] != 0: a persistent launch gave up waiting for its workgroups (bounded spin) and left its outputs partly unwritten --
// the captions are then POISONED (token -1, log-prob NaN) so that no caller can score or print them as if they were results.
__global__ void dec_finish_kernel(int64_t* __restrict__ seq, float* __restrict__ seq_logp, int N, int L, int ld, const int* __restrict__ status) {
  __shared__ int s_max;
  if (status && status[0] != 0) {
    for (int i = threadIdx.x; i < N * L; i += blockDim.x) {
      const int n = i / L, t = i - n * L;
      seq[(size_t)n * ld + t] = -1;
      seq_logp[(size_t)n * ld + t] = __int_as_float(0x7fc00000);
    }
    return;
  }
  if (threadIdx.x == 0) s_max = 0;
  __syncthreads();
  int mx = 0;
  for (int n = threadIdx.x; n < N; n += blockDim.x) {
    int f = L;                                   // first step at which the row emitted token 0
    for (int t = 0; t < L; ++t)
      if (seq[(size_t)n * ld + t] == 0) { f = t; break; }
    mx = max(mx, f);
  }
  atomicMax(&s_max, mx);
  __syncthreads();
  const int t_dead = s_max + 1;                  // every row had finished before this step
  for (int i = threadIdx.x; i < N * L; i += blockDim.x) {
    const int n = i / L, t = i - n * L;
    if (t >= t_dead) seq_logp[(size_t)n * ld + t] = 0.f;
  }
}

}  // namespace

// Two persistent launches must not be on the chip at once (each holds every CU while it waits, bounded, for its own
// workgroups to become resident): inside one process every persistent launch therefore waits for the previous one on its
// device, whatever stream that ran on.  (Across processes the caller has to choose: UIC_REC_FWD_CHAIN.)
// enter .. leave is ONE critical section per device (host threads call in through ctypes without the GIL): the lock taken by
// enter is held until leave has recorded the launch's event -- or until abandon, on an error path (UicPersistGateScope).
namespace {
struct PersistGate { hipEvent_t ev = nullptr; bool recorded = false; std::mutex mu; };
PersistGate g_gate[16];
int gate_device(hipStream_t s, int* dev) {
  // the STREAM's device, not the calling thread's current one (the default stream belongs to the current device)
  if (s) return uic_check_hip(hipStreamGetDevice(s, dev), "hipStreamGetDevice");
  return uic_check_hip(hipGetDevice(dev), "hipGetDevice");
}
}
int uic_persist_gate_enter(hipStream_t s, int* dev_out) {
  int dev = 0;
  UIC_TRY(gate_device(s, &dev));
  UIC_REQUIRE(dev >= 0 && dev < 16, "device index %d out of range", dev);
  PersistGate& g = g_gate[dev];
  g.mu.lock();
  int rc = UIC_OK;
  if (!g.ev) rc = uic_check_hip(hipEventCreateWithFlags(&g.ev, hipEventDisableTiming), "hipEventCreate");
  if (rc == UIC_OK && g.recorded) rc = uic_check_hip(hipStreamWaitEvent(s, g.ev, 0), "hipStreamWaitEvent(persistent gate)");
  if (rc != UIC_OK) { g.mu.unlock(); return rc; }
  *dev_out = dev;
  return UIC_OK;
}
int uic_persist_gate_leave(hipStream_t s, int dev) {
  PersistGate& g = g_gate[dev];
  const int rc = uic_check_hip(hipEventRecord(g.ev, s), "hipEventRecord(persistent gate)");
  if (rc == UIC_OK) g.recorded = true;
  g.mu.unlock();
  return rc;
}
void uic_persist_gate_abandon(int dev) { g_gate[dev].mu.unlock(); }

constexpr int MAX_SLABS = 8;       // launches of <= 640 caption rows each
size_t uic_rnn_persist_sync_bytes() { return (size_t)MAX_SLABS * SY_WORDS * 4; }

bool uic_rnn_persist_eligible(int dtype, int N, int H, int A, int R) {
  if (dtype != UIC_BF16 && dtype != UIC_F32) return false;
  if (H != HH || A != HH || R < 1 || R > ATT_R || N < 1 || N > MAX_SLABS * 8 * 16 * MT_MAX) return false;
  static int cus = -1;
  if (cus < 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return false;
    cus = prop.multiProcessorCount;
  }
  return cus == 8 * PW;        // one workgroup per CU, 32 per XCD
}

int uic_rnn_fwd_persist_launch(const UicRnnFwdParams& p0, hipStream_t s) {
  UIC_REQUIRE(p0.sync && p0.t1 > p0.t0 && p0.N > 0, "rnn_fwd_persist: bad arguments");
  UIC_REQUIRE(!p0.dec || (p0.dtype == UIC_BF16 && p0.gfc && p0.dec_embed_relu && p0.dec_xw && p0.dec_logit_w && p0.dec_logits && p0.dec_part &&
                          p0.dec_tok && p0.dec_unf && p0.dec_seq && p0.dec_seq_logp && p0.hdrop_all && p0.dec_V1 >= 2 &&
                          p0.dec_V1 <= PW * WS_NW * DEC_NJ * 16),
              "rnn_fwd_persist: decode mode needs bf16, gfc, the embedding / logit operands and its exchange buffers (V1 <= %d)", PW * WS_NW * DEC_NJ * 16);
  const int G = 8, cap = G * 16 * MT_MAX;     // caption rows one launch covers
  UicPersistGateScope gate;
  UIC_TRY(gate.enter(s));
  for (int r0 = 0; r0 < p0.N; r0 += cap) {
    UicRnnFwdParams p = p0;
    p.row0 = r0;
    p.Nrows = p0.N - r0 < cap ? p0.N - r0 : cap;
    {
      const char* lo = (const char*)p.h_att;
      if ((const char*)p.h_lang < lo) lo = (const char*)p.h_lang;
      if ((const char*)p.ctx_all < lo) lo = (const char*)p.ctx_all;
      const char* ends[3] = {(const char*)p.h_att, (const char*)p.h_lang, (const char*)p.ctx_all};
      for (int k = 0; k < 3; ++k)
        UIC_REQUIRE((size_t)(ends[k] - lo) + (size_t)(p.t1 + 1) * p.N * HH * 4 < ((size_t)1 << 32), "rnn_fwd_persist: the state slabs must lie within 4 GB of each other");
      p.xbase = lo;
    }
    p.sync = p0.sync + (size_t)(r0 / cap) * SY_WORDS;
    if (!(p0.sync_zeroed && r0 == 0)) UIC_TRY(uic_check_hip(hipMemsetAsync(p.sync, 0, (size_t)SY_WORDS * 4, s), "hipMemsetAsync(rnn sync)"));
    // bf16: the weight-stationary kernels; f32 (the parity path): the generic one, weights re-read from L2 every step
    if (p.dec) UIC_TRY(rnn_persist::ws_decode_launch(p, s));
    else if (p.dtype == UIC_BF16) UIC_TRY(rnn_persist::ws_train_launch(p, s));
    else UIC_TRY(rnn_persist::generic_f32_launch(p, s));
  }
  return gate.leave();
}

bool uic_rnn_decode_persist_eligible(int dtype, int N, int H, int A, int R, int E, int V1) {
  return dtype == UIC_BF16 && E == HH && V1 >= 2 && V1 <= PW * WS_NW * DEC_NJ * 16 && uic_rnn_persist_eligible(dtype, N, H, A, R);
}
size_t uic_rnn_decode_part_floats(int N) { return (size_t)N * PW * 4; }
int uic_rnn_decode_finish_launch(int64_t* seq, float* seq_logp, int N, int L, int ld, const int* status, hipStream_t s) {
  UIC_REQUIRE(seq && seq_logp && N > 0 && L > 0 && ld >= L, "rnn_decode_finish: bad arguments");
  hipLaunchKernelGGL(dec_finish_kernel, dim3(1), dim3(1024), 0, s, seq, seq_logp, N, L, ld, status);
  UIC_LAUNCH_CHECK("dec_finish_kernel");
  return UIC_OK;
}
int uic_rnn_decode_embed_relu_launch(const void* embed_w, int table_dtype, void* out_bf16, int V1, int E, hipStream_t s) {
  UIC_REQUIRE(embed_w && out_bf16 && V1 > 0 && E % 4 == 0, "rnn_decode_embed_relu: bad arguments");
  const size_t n4 = (size_t)V1 * E / 4;
  const dim3 grid((unsigned)((n4 + 255) / 256 > 4096 ? 4096 : (n4 + 255) / 256));
  if (table_dtype == UIC_BF16) hipLaunchKernelGGL(dec_embed_relu16_kernel, grid, dim3(256), 0, s, (const uint2*)embed_w, (uint2*)out_bf16, n4);
  else hipLaunchKernelGGL(dec_embed_relu_kernel, grid, dim3(256), 0, s, (const float*)embed_w, (bf16_t*)out_bf16, n4);
  UIC_LAUNCH_CHECK("dec_embed_relu_kernel");
  return UIC_OK;
}
