// The ensemble's word distribution (P/models/AttEnsemble.py:53): softmax of every member's logits, mean over the members,
// log.  One decode step of M members -> one row of combined log-probs per caption row:
//
//   out[v] = log( (1/M) sum_m exp(x_m[v] - lse_m) ),   lse_m = max_m + log sum_v exp(x_m[v] - max_m)
//
// ensemble_logmean_kernel: one workgroup of 256 threads per row, two sweeps over the M member rows (a 9 488-word row is 38 KB:
// the M rows are expected to stay in the L2 between the sweeps, as beam_topk3_kernel relies on for its three -- expected, not
// measured: no timing or counter run of this kernel exists yet, see profiles/LOG.md "Ensemble decode").
//   sweep 1: per member, running maximum and the sum of exponentials rescaled to it (per thread, then merged over the wave by
//            shuffles and over the four waves through LDS);
//   sweep 2: a_m = x_m[v] - lse_m, out[v] = max_m a_m + log sum_m exp(a_m - max_m a_m) - log M.  The same number as the formula
//            above, but no term underflows before the logarithm: the row stays finite wherever one member's log-prob is (the
//            reference's exp -> mean -> log gives -inf once every member's probability is below 2^-149), and M = 1 is
//            x - lse to the bit, i.e. log_softmax.
// f32 arithmetic with expf / logf throughout (the reference does this step in f32; greedy / beam token ids of the f32 parity
// path depend on it).
// Loads: every sweep asks for the M members' 16 bytes of a trip first, unconditionally, from a clamped group index; whether a
// word is inside the row is applied to the VALUE (requests first, conditions late).  Rows whose base or leading dimension is
// not a multiple of 16 bytes take four clamped 4-byte loads per group instead.
// Columns [V1, ld_out) of `out` are left alone: the logit GEMM of decode_step does not write them either (they hold whatever
// the workspace held), and neither uic_sample_step_launch nor uic_beam_step_launch reads past V1 -- there is no value the
// consumers expect there, so none is written.
// `out` may be one of the members' rows (the sequencers combine into member 0's step logits): a word is read and written by
// the same thread in the same trip of sweep 2, after sweep 1 is through for the whole workgroup.
#include "uic_common.h"
#include "../../include/uic_hip.h"
#include <stdint.h>

namespace {

constexpr int NT = 256;
constexpr int NW = NT / 64;

// (mx, sum) <- merge with (omx, osum): sum of exponentials relative to the common maximum.  Nothing seen yet is (-inf, 0).
__device__ __forceinline__ void merge(float& mx, float& sum, float omx, float osum) {
  const float nm = fmaxf(mx, omx);
  const float s = sum * expf(mx - nm) + osum * expf(omx - nm);
  sum = nm > -INFINITY ? s : 0.f;      // (-inf) - (-inf) is NaN: a row part of -inf only contributes nothing
  mx = nm;
}

// the four words of group g of row x: one 16-byte load, or four 4-byte loads from clamped addresses
template <bool VEC>
__device__ __forceinline__ void load4(const float* x, int g, int V1, float* q) {
  if (VEC) {
    const float4 f = *(const float4*)(x + 4 * (size_t)g);
    q[0] = f.x; q[1] = f.y; q[2] = f.z; q[3] = f.w;
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) q[c] = x[min(4 * g + c, V1 - 1)];
  }
}

template <int M, bool VEC>
__global__ __launch_bounds__(NT) void ensemble_logmean_kernel(const UicEnsembleParams p) {
  __shared__ float s_mx[M][NW];
  __shared__ float s_sum[M][NW];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V1 = p.V1;
  const int G = (V1 + 3) >> 2;                    // groups of four words; the last one may reach into the row's padding (VEC: ld % 4 == 0)
  const int trips = (G + NT - 1) / NT;
  const float* x[M];
#pragma unroll
  for (int m = 0; m < M; ++m) x[m] = p.x[m] + (size_t)row * p.ld[m];
  float* out = p.out + (size_t)row * p.ld_out;

  float mx[M], sum[M];
#pragma unroll
  for (int m = 0; m < M; ++m) { mx[m] = -INFINITY; sum[m] = 0.f; }
  for (int i = 0; i < trips; ++i) {
    const int g = i * NT + tid, gc = min(g, G - 1);
    float q[M][4];
#pragma unroll
    for (int m = 0; m < M; ++m) load4<VEC>(x[m], gc, V1, q[m]);
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        // one word folded into the running (maximum, rescaled sum): ONE expf -- of -|x - mx|, which rescales the sum when the
        // word is the new maximum and is the word's own term otherwise.  Words outside the row (whatever the padding holds,
        // NaN included) and words at -inf change nothing: the predicate selects between finished VALUES.
        const float xv = q[m][c];
        const float dlt = xv - mx[m];
        const float e = expf(-fabsf(dlt));
        const float ns = dlt > 0.f ? sum[m] * e + 1.f : sum[m] + e;
        const bool use = 4 * g + c < V1 && xv > -INFINITY;
        sum[m] = use ? ns : sum[m];
        mx[m] = use ? fmaxf(mx[m], xv) : mx[m];
      }
  }
#pragma unroll
  for (int m = 0; m < M; ++m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) merge(mx[m], sum[m], __shfl_xor(mx[m], o, 64), __shfl_xor(sum[m], o, 64));
    if (lane == 0) { s_mx[m][wave] = mx[m]; s_sum[m][wave] = sum[m]; }
  }
  __syncthreads();
  float lse[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    float a = s_mx[m][0], b = s_sum[m][0];
#pragma unroll
    for (int w = 1; w < NW; ++w) merge(a, b, s_mx[m][w], s_sum[m][w]);
    lse[m] = a + logf(b);
  }

  const float log_m = logf((float)M);
  for (int i = 0; i < trips; ++i) {
    const int g = i * NT + tid, gc = min(g, G - 1);
    float q[M][4];
#pragma unroll
    for (int m = 0; m < M; ++m) load4<VEC>(x[m], gc, V1, q[m]);
    float r[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float a[M];
      float am = -INFINITY;
#pragma unroll
      for (int m = 0; m < M; ++m) { a[m] = q[m][c] - lse[m]; am = fmaxf(am, a[m]); }
      if (M == 1) { r[c] = a[0]; continue; }
      float s = 0.f;
#pragma unroll
      for (int m = 0; m < M; ++m) s += expf(a[m] - am);
      // (every member at -inf: the word has probability 0 in the ensemble too)
      r[c] = am > -INFINITY ? am + logf(s) - log_m : am;
    }
    if (VEC && 4 * g + 3 < V1) {
      *(float4*)(out + 4 * (size_t)g) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (4 * g + c < V1) out[4 * g + c] = r[c];
    }
  }
}

template <int M>
void launch_m(const UicEnsembleParams& p, bool vec, hipStream_t s) {
  if (vec) hipLaunchKernelGGL((ensemble_logmean_kernel<M, true>), dim3(p.N), dim3(NT), 0, s, p);
  else hipLaunchKernelGGL((ensemble_logmean_kernel<M, false>), dim3(p.N), dim3(NT), 0, s, p);
}

}  // namespace

int uic_ensemble_logmean_launch(const UicEnsembleParams& p, hipStream_t s) {
  UIC_REQUIRE(p.M >= 1 && p.M <= UIC_ENSEMBLE_MAX, "ensemble: %d members outside [1, %d]", p.M, UIC_ENSEMBLE_MAX);
  UIC_REQUIRE(p.N >= 0 && p.V1 >= 1 && p.V1 <= (1 << 28), "ensemble: bad sizes N=%d V1=%d", p.N, p.V1);
  UIC_REQUIRE(p.out && p.ld_out >= p.V1, "ensemble: output needs a leading dimension >= V1=%d (got %d)", p.V1, p.ld_out);
  bool vec = p.ld_out % 4 == 0 && ((uintptr_t)p.out & 15) == 0;
  for (int m = 0; m < p.M; ++m) {
    UIC_REQUIRE(p.x[m] && p.ld[m] >= p.V1, "ensemble: member %d needs logits with a leading dimension >= V1=%d (got %d)", m, p.V1, p.ld[m]);
    vec = vec && p.ld[m] % 4 == 0 && ((uintptr_t)p.x[m] & 15) == 0;
  }
  if (p.N == 0) return UIC_OK;
  switch (p.M) {
    case 1: launch_m<1>(p, vec, s); break;
    case 2: launch_m<2>(p, vec, s); break;
    case 3: launch_m<3>(p, vec, s); break;
    case 4: launch_m<4>(p, vec, s); break;
    case 5: launch_m<5>(p, vec, s); break;
    case 6: launch_m<6>(p, vec, s); break;
    case 7: launch_m<7>(p, vec, s); break;
    default: launch_m<8>(p, vec, s); break;
  }
  UIC_LAUNCH_CHECK("ensemble_logmean");
  return UIC_OK;
}

extern "C" int uic_ensemble_logprobs(int32_t M, int32_t N, int32_t V1, const float* const* logits, const int32_t* ld, float* out,
                                     int32_t ld_out, void* stream) {
  UIC_REQUIRE(logits && ld && out, "ensemble_logprobs: null pointer");
  UIC_REQUIRE(M >= 1 && M <= UIC_ENSEMBLE_MAX, "ensemble_logprobs: %d members outside [1, %d]", M, UIC_ENSEMBLE_MAX);
  UicEnsembleParams p;
  p.M = M; p.N = N; p.V1 = V1; p.out = out; p.ld_out = ld_out;
  for (int m = 0; m < UIC_ENSEMBLE_MAX; ++m) { p.x[m] = m < M ? logits[m] : nullptr; p.ld[m] = m < M ? ld[m] : 0; }
  return uic_ensemble_logmean_launch(p, (hipStream_t)stream);
}
