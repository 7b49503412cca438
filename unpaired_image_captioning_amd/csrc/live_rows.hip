// The live rows of a training step (gfx950): the ascending list of the (step, row) positions whose mask is set, built on the
// device in one workgroup so that it never crosses PCIe, and the gather / scatter of 16-byte-chunked rows by such a list
// (the position-indexed operands of the step run over the listed rows only).
#include "uic_common.h"
#include "uic_host.h"
#include "../../include/uic_hip.h"
#include <string.h>

namespace {

// row_len[n] = 1 + the last t < T with mask[n * ld + col0 + t] != 0 (0: none): a thread per row walks its T consecutive words (the
// list kernels have just read them: cache hits) -- no atomics
__device__ inline void live_row_len(const float* __restrict__ mask, int ld, int col0, int N, int T, int* __restrict__ row_len, int tid) {
  for (int n = tid; n < N; n += 1024) {
    const float* m = mask + (size_t)n * ld + col0;
    int len = 0;
    for (int t = 0; t < T; ++t) len = m[t] != 0.f ? t + 1 : len;
    row_len[n] = len;
  }
}
// The rows ordered by their length, longest first (UicLiveOrder, uic_common.h): a stable counting sort with the T + 1 lengths as
// buckets, in the list kernels' own workgroup behind live_row_len.  Wave w of the row space (rows 64 w ... 64 w + 63) counts its rows
// of every length with one ballot each; the counts meet in LDS as cnt[(T - len) * W + w] -- the order of the sorted output --, one
// wave scans them, and a row's place is its (length, wave) offset + the rows of that length below it in its wave.  No atomics: the
// same lengths give the same order.  unfinished[t] = the offset of bucket t = the number of rows with a greater length.
constexpr int LO_MAX_WAVES = 64;                       // rows / 64 the order covers (uic_live_order_ok)
constexpr int LO_MAX_ENT = LO_MAX_WAVES * (UIC_MAX_LIVE_STEPS + 1);
struct LiveOrderArgs {
  int* order; int* rank; int* unfinished; unsigned* status;
  int has_expect;
  int expect[UIC_MAX_LIVE_STEPS];
};
__device__ inline void live_order(const int* __restrict__ row_len, int N, int T, const LiveOrderArgs& o, int* s_ent, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  const int W = (N + 63) >> 6, E = (T + 1) * W;
  __syncthreads();                                     // (row_len was written by this workgroup)
  for (int w = wave; w < W; w += 16) {
    const int n = w * 64 + lane;
    const int len = n < N ? row_len[n] : -1;
    for (int v = 0; v <= T; ++v) {
      const unsigned long long b = __ballot(len == v);
      if (lane == 0) s_ent[(T - v) * W + w] = __popcll(b);
    }
  }
  __syncthreads();
  if (wave == 0) {                                     // exclusive prefix of the E counts, in place: a run per lane + a wave scan
    const int per = (E + 63) >> 6, e0 = lane * per, e1 = min(E, e0 + per);
    int sum = 0;
    for (int e = e0; e < e1; ++e) sum += s_ent[e];
    int incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int up = __shfl_up(incl, d); if (lane >= d) incl += up; }
    int run = incl - sum;
    for (int e = e0; e < e1; ++e) { const int c = s_ent[e]; s_ent[e] = run; run += c; }
  }
  __syncthreads();
  for (int w = wave; w < W; w += 16) {
    const int n = w * 64 + lane;
    const int len = n < N ? row_len[n] : -1;
    int at = 0;
    for (int v = 0; v <= T; ++v) {
      const unsigned long long b = __ballot(len == v);
      if (len == v) at = s_ent[(T - v) * W + w] + __popcll(b & ((1ull << lane) - 1ull));
    }
    if (n < N) { o.rank[n] = at; o.order[at] = n; }
  }
  // unfinished[t] = #{n : row_len[n] > t} (unfinished[T] = 0); against the counts the caller sized its launches with
  if (tid <= T) o.unfinished[tid] = tid < T ? s_ent[(T - tid) * W] : 0;
  if (tid == 0 && o.has_expect && o.status) {
    for (int t = 0; t < T; ++t)
      if (o.expect[t] != s_ent[(T - t) * W]) { o.status[0] = (unsigned)UIC_STATUS_UNFINISHED_COUNT | (unsigned)t; break; }
  }
}

// out = the positions p = t * N + n, ascending, whose mask[n * ld + col0 + t] is not zero; entries behind them up to out_len: -1.
// ONE workgroup: an ordered compaction of ~1e4 positions in chunks of 1024 (ballot + wave prefix + one running offset), a few
// microseconds beside the prologue -- the list never crosses PCIe.
// inv (optional, [M]): the inverse -- inv[p] = the list index of position p, or -1; zero16 (optional): n16 16-byte words cleared on
// the way (the padding rows of the compact operand the list's consumer fills by itself, rnn_persist.hip)
__global__ __launch_bounds__(1024) void live_list_kernel(const float* __restrict__ mask, int ld, int col0, int N, int M, int* __restrict__ out, int out_len,
                                                         int* __restrict__ inv, uint4* __restrict__ zero16, int n16, int* __restrict__ row_len, const LiveOrderArgs ord) {
  __shared__ int s_ent[LO_MAX_ENT];
  __shared__ int s_wave[16];
  __shared__ int s_base;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_base = 0;
  __syncthreads();
  for (int p0 = 0; p0 < M; p0 += 1024) {
    const int p = p0 + tid;
    bool on = false;
    if (p < M) {
      const int t = p / N, n = p - t * N;
      on = mask[(size_t)n * ld + col0 + t] != 0.f;
    }
    const unsigned long long b = __ballot(on);
    const int before = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wave] = __popcll(b);
    __syncthreads();
    int off = s_base;
    for (int w2 = 0; w2 < wave; ++w2) off += s_wave[w2];
    if (on && off + before < out_len) out[off + before] = p;
    if (inv && p < M) inv[p] = on && off + before < out_len ? off + before : -1;
    __syncthreads();
    if (tid == 0) { int tot = 0; for (int w2 = 0; w2 < 16; ++w2) tot += s_wave[w2]; s_base += tot; }
    __syncthreads();
  }
  for (int i = s_base + tid; i < out_len; i += 1024) out[i] = -1;
  for (int i = tid; i < n16; i += 1024) zero16[i] = make_uint4(0u, 0u, 0u, 0u);
  if (row_len) live_row_len(mask, ld, col0, N, M / N, row_len, tid);
  if (ord.order) live_order(row_len, N, M / N, ord, s_ent, tid);       // (uniform: a kernel argument)
}
// the same for M <= 16 x 1024 positions (the captioner's 10 880, the NMT step's ~2 000) with ONE round trip to memory: every
// thread requests its <= 16 mask words at once, the per-(round, wave) counts meet in LDS, one wave scans the 256 of them
// (19 -> 4 us: the first form paid a memory latency and three barriers per 1024 positions)
constexpr int LL_R = 16;
__global__ __launch_bounds__(1024) void live_list_burst_kernel(const float* __restrict__ mask, int ld, int col0, int N, int M, int* __restrict__ out, int out_len,
                                                               int* __restrict__ inv, uint4* __restrict__ zero16, int n16, int* __restrict__ row_len, const LiveOrderArgs ord) {
  __shared__ int s_ent[LO_MAX_ENT];
  __shared__ int s_cnt[LL_R * 16];
  __shared__ int s_off[LL_R * 16 + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float v[LL_R];
#pragma unroll
  for (int i = 0; i < LL_R; ++i) {
    int p = i * 1024 + tid;
    p = p < M ? p : 0;                                  // (a valid address; the test below drops it)
    const int t = p / N, n = p - t * N;
    v[i] = mask[(size_t)n * ld + col0 + t];
  }
  unsigned bits = 0;
#pragma unroll
  for (int i = 0; i < LL_R; ++i) {
    const bool on = i * 1024 + tid < M && v[i] != 0.f;
    bits |= on ? 1u << i : 0u;
    const unsigned long long b = __ballot(on);
    if (lane == 0) s_cnt[i * 16 + wave] = __popcll(b);
  }
  __syncthreads();
  if (wave == 0) {                                      // exclusive prefix of the 256 counts: 4 per lane + a wave scan
    int c[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { c[j] = s_cnt[lane * 4 + j]; sum += c[j]; }
    int incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d); if (lane >= d) incl += o; }
    int run = incl - sum;
#pragma unroll
    for (int j = 0; j < 4; ++j) { s_off[lane * 4 + j] = run; run += c[j]; }
    if (lane == 63) s_off[LL_R * 16] = run;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < LL_R; ++i) {
    const bool on = (bits >> i) & 1u;
    const unsigned long long b = __ballot(on);
    const int at = s_off[i * 16 + wave] + __popcll(b & ((1ull << lane) - 1ull));
    if (on && at < out_len) out[at] = i * 1024 + tid;
    if (inv && i * 1024 + tid < M) inv[i * 1024 + tid] = on && at < out_len ? at : -1;
  }
  for (int i = s_off[LL_R * 16] + tid; i < out_len; i += 1024) out[i] = -1;
  for (int i = tid; i < n16; i += 1024) zero16[i] = make_uint4(0u, 0u, 0u, 0u);
  if (row_len) live_row_len(mask, ld, col0, N, M / N, row_len, tid);
  if (ord.order) live_order(row_len, N, M / N, ord, s_ent, tid);       // (uniform: a kernel argument)
}

// out[m, :] = src[map[m], :] (rows of `chunks` 16-byte pieces) for m < M; rows [M, Mpad) of out are cleared
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint4* __restrict__ src, const int* __restrict__ map, uint4* __restrict__ out, int M, int Mpad,
                                                          int chunks, int limit) {
  const size_t total = (size_t)Mpad * chunks, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int m = (int)(i / chunks), c = (int)(i - (size_t)m * chunks);
    const int r = m < M ? map[m] : -1;
    out[i] = (unsigned)r < (unsigned)limit ? src[(size_t)r * chunks + c] : make_uint4(0u, 0u, 0u, 0u);
  }
}
// dst[map[m], :] = src[m, :] for m < M
__global__ __launch_bounds__(256) void scatter_rows_kernel(const uint4* __restrict__ src, const int* __restrict__ map, uint4* __restrict__ dst, int M, int chunks, int limit) {
  const size_t total = (size_t)M * chunks, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int m = (int)(i / chunks), c = (int)(i - (size_t)m * chunks);
    const int r = map[m];
    if ((unsigned)r < (unsigned)limit) dst[(size_t)r * chunks + c] = src[i];
  }
}

}  // namespace

bool uic_live_order_ok(int N, int T) { return N >= 1 && N <= 64 * LO_MAX_WAVES && T >= 1 && T <= UIC_MAX_LIVE_STEPS; }
int uic_live_list_launch(const float* mask, int ld, int col0, int N, int M, int* out, int out_len, hipStream_t s, int* inv, void* zero, size_t zero_bytes,
                         int* row_len, const UicLiveOrder* order) {
  UIC_REQUIRE(mask && out && N > 0 && M >= 0 && out_len >= 0, "live_list: bad arguments");
  LiveOrderArgs ord;
  memset(&ord, 0, sizeof(ord));
  if (order) {
    UIC_REQUIRE(row_len && order->order && order->rank && order->unfinished && M % N == 0 && uic_live_order_ok(N, M / N),
                "live_list: the row order needs row_len and its three outputs, N=%d <= %d rows and M / N = %d <= %d steps", N,
                64 * LO_MAX_WAVES, M / N, UIC_MAX_LIVE_STEPS);
    ord.order = order->order; ord.rank = order->rank; ord.unfinished = order->unfinished; ord.status = order->status;
    ord.has_expect = order->expect != nullptr;
    if (order->expect) memcpy(ord.expect, order->expect, (size_t)(M / N) * sizeof(int));
  }
  UIC_REQUIRE(zero_bytes == 0 || (zero && ((uintptr_t)zero & 15) == 0 && zero_bytes % 16 == 0 && zero_bytes < ((size_t)1 << 30)), "live_list: the cleared region must be 16-byte aligned / sized");
  if (out_len == 0 && !inv && !row_len) return UIC_OK;
  const int n16 = (int)(zero_bytes / 16);
  if (M <= LL_R * 1024 && M > 0) hipLaunchKernelGGL(live_list_burst_kernel, dim3(1), dim3(1024), 0, s, mask, ld, col0, N, M, out, out_len, inv, (uint4*)zero, n16, row_len, ord);
  else hipLaunchKernelGGL(live_list_kernel, dim3(1), dim3(1024), 0, s, mask, ld, col0, N, M, out, out_len, inv, (uint4*)zero, n16, row_len, ord);
  UIC_LAUNCH_CHECK("live_list");
  return UIC_OK;
}
int uic_gather_rows_launch(const void* src, const int* map, int src_rows, void* out, int M, int Mpad, size_t row_bytes, hipStream_t s) {
  UIC_REQUIRE(row_bytes % 16 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)out & 15) == 0 && Mpad >= M && M >= 0, "gather_rows: bad arguments");
  if (Mpad == 0) return UIC_OK;
  const int chunks = (int)(row_bytes / 16);
  hipLaunchKernelGGL(gather_rows_kernel, dim3(uic_grid_for((size_t)Mpad * chunks, 256)), dim3(256), 0, s, (const uint4*)src, map, (uint4*)out, M, Mpad, chunks, src_rows);
  UIC_LAUNCH_CHECK("gather_rows");
  return UIC_OK;
}
int uic_scatter_rows_launch(const void* src, const int* map, void* dst, int dst_rows, int M, size_t row_bytes, hipStream_t s) {
  UIC_REQUIRE(row_bytes % 16 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0 && M >= 0, "scatter_rows: bad arguments");
  if (M == 0) return UIC_OK;
  const int chunks = (int)(row_bytes / 16);
  hipLaunchKernelGGL(scatter_rows_kernel, dim3(uic_grid_for((size_t)M * chunks, 256)), dim3(256), 0, s, (const uint4*)src, map, (uint4*)dst, M, chunks, dst_rows);
  UIC_LAUNCH_CHECK("scatter_rows");
  return UIC_OK;
}
