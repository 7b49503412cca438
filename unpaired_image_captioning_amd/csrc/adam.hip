// Adam (torch.optim.Adam, P/misc/optimizer.py:70) over the parameter arena and the squared gradient norm that
// clip_grad_norm needs (P/misc/optimizer.py:99), read on the device (gfx950).  The C entries uic_adam_step* and
// uic_grad_sqnorm (api.hip) fill UicAdamParams; the launchers below do the work.
#include "uic_common.h"
#include "uic_host.h"

namespace {

constexpr int NT = 256;

// (16 bytes per lane and four independent partial sums in flight: the scalar form read the pivot NMT's 360 MB of gradients at
// 2.7 TB/s, one dependent add per load)
__global__ __launch_bounds__(NT) void sqnorm_part_kernel(const float* __restrict__ g, size_t n, float* __restrict__ part) {
  __shared__ float s_buf[NT / 64];
  const size_t n4 = ((uintptr_t)g & 15) == 0 ? n / 4 : 0;
  const size_t stride = (size_t)gridDim.x * NT;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  const f32x4* g4 = (const f32x4*)g;
  for (; i + 3 * stride < n4; i += 4 * stride) {
    const f32x4 a = __builtin_nontemporal_load(g4 + i), b = __builtin_nontemporal_load(g4 + i + stride);
    const f32x4 c = __builtin_nontemporal_load(g4 + i + 2 * stride), d = __builtin_nontemporal_load(g4 + i + 3 * stride);
    s0 += (a[0] * a[0] + a[1] * a[1]) + (a[2] * a[2] + a[3] * a[3]);
    s1 += (b[0] * b[0] + b[1] * b[1]) + (b[2] * b[2] + b[3] * b[3]);
    s2 += (c[0] * c[0] + c[1] * c[1]) + (c[2] * c[2] + c[3] * c[3]);
    s3 += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
  }
  for (; i < n4; i += stride) {
    const f32x4 a = g4[i];
    s0 += (a[0] * a[0] + a[1] * a[1]) + (a[2] * a[2] + a[3] * a[3]);
  }
  for (size_t j = n4 * 4 + (size_t)blockIdx.x * NT + threadIdx.x; j < n; j += stride) s1 += g[j] * g[j];
  float s = uic_block_sum<NT>((s0 + s1) + (s2 + s3), s_buf);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
// ONE definition of the element update for both Adam kernels, with floating-point contraction off: the whole-arena kernel and the
// ranges kernel of the sharded exchange must produce the same bits from the same inputs (tests/test_gpu_dp2.py compares the two
// exchanges bit for bit), whatever fused multiply-adds the optimizer would pick for each loop shape.
__device__ __forceinline__ float uic_adam_update(float p, float& m, float& v, float g, float beta1, float beta2, float step_size,
                                                 float inv_sqrt_bc2, float eps) {
#pragma clang fp contract(off)
  m = beta1 * m + (1.f - beta1) * g;
  v = beta2 * v + (1.f - beta2) * g * g;
  const float denom = sqrtf(v) * inv_sqrt_bc2 + eps;
  return p - step_size * (m / denom);
}
__device__ __forceinline__ float uic_adam_grad_scale(const UicAdamParams& a) {
#pragma clang fp contract(off)
  float gs = a.grad_scale;
  if (a.sqnorm) {
    const float coef = a.max_norm / (fabsf(a.grad_scale) * sqrtf(a.sqnorm[0]) + 1e-6f);
    if (coef < 1.f) gs *= coef;
  }
  return gs;
}
__global__ void adam_kernel(const UicAdamParams a) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const float step_size = a.lr / a.bc1;
  const float inv_sqrt_bc2 = 1.f / sqrtf(a.bc2);
  if (a.guard && a.guard[0] != 0) return;          // (uniform over the launch: the step's gradients are invalid, keep the weights)
  const float gs = uic_adam_grad_scale(a);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
    // gradient and moments are touched once per step, by this kernel only: streamed past the caches (the parameters are
    // re-read right after by the operand-copy refresh and stay cacheable)
    const float g = __builtin_nontemporal_load(a.g + i) * gs;
    float m = __builtin_nontemporal_load(a.m + i), v = __builtin_nontemporal_load(a.v + i);
    const float pn = uic_adam_update(a.p[i], m, v, g, a.beta1, a.beta2, step_size, inv_sqrt_bc2, a.eps);
    __builtin_nontemporal_store(m, a.m + i);
    __builtin_nontemporal_store(v, a.v + i);
    a.p[i] = pn;
  }
}

// The same update on up to UIC_ADAM_RANGES index ranges of the arena in ONE launch -- the ranges a data-parallel rank owns after
// the reduce-scatter (one per gradient piece) plus the replicated tail -- optionally leaving the updated parameters of those
// ranges in the operand dtype in `w_out` (same element index), which is what the all-gather then distributes.
template <typename WT>
__global__ void adam_ranges_kernel(const UicAdamParams a, const UicAdamRanges r, WT* __restrict__ w_out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const float step_size = a.lr / a.bc1;
  const float inv_sqrt_bc2 = 1.f / sqrtf(a.bc2);
  if (a.guard && a.guard[0] != 0) return;
  const float gs = uic_adam_grad_scale(a);
  for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < r.total; j += stride) {
    int k = 0;
    while (k + 1 < r.count && j >= r.start[k + 1]) ++k;       // start[k]: position of range k in the concatenation
    const size_t i = r.lo[k] + (j - r.start[k]);
    const float g = __builtin_nontemporal_load(a.g + i) * gs;
    float m = __builtin_nontemporal_load(a.m + i), v = __builtin_nontemporal_load(a.v + i);
    const float pn = uic_adam_update(a.p[i], m, v, g, a.beta1, a.beta2, step_size, inv_sqrt_bc2, a.eps);
    __builtin_nontemporal_store(m, a.m + i);
    __builtin_nontemporal_store(v, a.v + i);
    a.p[i] = pn;
    if (w_out) w_out[i] = uic_from_f<WT>(pn);
  }
}

}  // namespace

// out[0] = sum_i g[i]^2: per-workgroup partials into scratch, then the one-workgroup sum of pointwise.hip
int uic_sqnorm_launch(const float* g, size_t n, float* scratch, float* out, hipStream_t s) {
  UIC_REQUIRE(g && scratch && out, "sqnorm: null pointer");
  const int blocks = (int)(n / (NT * 8) > 1024 ? 1024 : (n / (NT * 8) ? n / (NT * 8) : 1));
  hipLaunchKernelGGL(sqnorm_part_kernel, dim3(blocks), dim3(NT), 0, s, g, n, scratch);
  UIC_LAUNCH_CHECK("sqnorm_part");
  return uic_reduce_sum_launch(scratch, (size_t)blocks, nullptr, out, s);
}
int uic_adam_launch(const UicAdamParams& a, hipStream_t s) {
  if (a.n == 0) return UIC_OK;
  hipLaunchKernelGGL(adam_kernel, dim3(uic_grid_for(a.n, NT)), dim3(NT), 0, s, a);
  UIC_LAUNCH_CHECK("adam");
  return UIC_OK;
}
int uic_adam_ranges_launch(const UicAdamParams& a, const UicAdamRanges& r, void* w_out, int w_dtype, hipStream_t s) {
  if (r.total == 0) return UIC_OK;
  const int g = uic_grid_for(r.total, NT);
  if (w_out && w_dtype == UIC_BF16) hipLaunchKernelGGL(adam_ranges_kernel<bf16_t>, dim3(g), dim3(NT), 0, s, a, r, (bf16_t*)w_out);
  else hipLaunchKernelGGL(adam_ranges_kernel<float>, dim3(g), dim3(NT), 0, s, a, r, (float*)nullptr);   // (f32 operands ARE the masters)
  UIC_LAUNCH_CHECK("adam_ranges");
  return UIC_OK;
}
