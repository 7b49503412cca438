// The optimizer step of every --i2t_optim / --nmt_optim method (torch.optim.{Adam,SGD,RMSprop,Adagrad} as
// P/misc/optimizer.py:59-74 constructs them) over the parameter arena and the squared gradient norm that clip_grad_norm needs
// (P/misc/optimizer.py:99), read on the device (gfx950).  The C entries uic_optim_step*, uic_adam_step* and uic_grad_sqnorm
// (api.hip) fill UicOptimParams; the launchers below do the work.
#include "uic_common.h"
#include "uic_host.h"
#include "../../include/uic_hip.h"
#include <type_traits>

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
// The same sum accumulated in double and left as a PAIR of floats, out[0] + out[1] (the rounded sum and what the rounding dropped):
// the norm under the clip of a step WITH weight decay, whose coefficient uic_optim_grad_scale_d forms in double.  One float is not
// enough there: where clip * g and wd * p cancel to 3e-5 of their size (measured on the pivot model's first step) the 1e-8 of a
// float's last bit is 1e-3 of what is left.  (Scalar loads: this path reads the gradient at a lower rate than the form above.)
constexpr int SQ64_BLOCKS = 512;          // partials in the caller's scratch of >= 1024 floats
__device__ __forceinline__ double block_sum_f64(double s, double* s_buf) {
  s_buf[threadIdx.x] = s;
  __syncthreads();
  for (int w = NT / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s_buf[threadIdx.x] += s_buf[threadIdx.x + w];
    __syncthreads();
  }
  return s_buf[0];
}
__global__ __launch_bounds__(NT) void sqnorm_part_f64_kernel(const float* __restrict__ g, size_t n, double* __restrict__ part) {
  __shared__ double s_buf[NT];
  const size_t stride = (size_t)gridDim.x * NT;
  double s = 0.0;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += stride) {
    const double x = (double)__builtin_nontemporal_load(g + i);
    s += x * x;
  }
  s = block_sum_f64(s, s_buf);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(NT) void sqnorm_final_f64_kernel(const double* __restrict__ part, int count, float* __restrict__ out) {
  __shared__ double s_buf[NT];
  double s = 0.0;
  for (int i = threadIdx.x; i < count; i += NT) s += part[i];
  s = block_sum_f64(s, s_buf);
  if (threadIdx.x == 0) {
    const float hi = (float)s;
    out[0] = hi;
    out[1] = (float)(s - (double)hi);
  }
}
// ONE definition of each method's element update for both kernels, with floating-point contraction off: the whole-arena kernel
// and the ranges kernel of the sharded exchange must produce the same bits from the same inputs (tests/test_gpu_dp2.py compares
// the two exchanges bit for bit), whatever fused multiply-adds the optimizer would pick for each loop shape.  Each returns the
// new parameter and updates its state in place; g is the gradient after grad_scale, the clip and the weight decay.
__device__ __forceinline__ float uic_adam_update(float p, float& m, float& v, float g, float beta1, float beta2, float step_size,
                                                 float inv_sqrt_bc2, float eps) {
#pragma clang fp contract(off)
  m = beta1 * m + (1.f - beta1) * g;
  v = beta2 * v + (1.f - beta2) * g * g;
  const float denom = sqrtf(v) * inv_sqrt_bc2 + eps;
  return p - step_size * (m / denom);
}
__device__ __forceinline__ float uic_sgd_update(float p, float g, float lr) {
#pragma clang fp contract(off)
  return p - lr * g;
}
// SGD(momentum=alpha[, nesterov=True]), dampening 0: a zero buffer gives buf = g on the first step, as torch's clone does
template <bool NESTEROV>
__device__ __forceinline__ float uic_momentum_update(float p, float& buf, float g, float alpha, float lr) {
#pragma clang fp contract(off)
  buf = alpha * buf + g;
  return p - lr * (NESTEROV ? g + alpha * buf : buf);
}
__device__ __forceinline__ float uic_rmsprop_update(float p, float& sq, float g, float alpha, float lr, float eps) {
#pragma clang fp contract(off)
  sq = alpha * sq + (1.f - alpha) * g * g;
  return p - lr * (g / (sqrtf(sq) + eps));
}
__device__ __forceinline__ float uic_adagrad_update(float p, float& sum, float g, float lr, float eps) {
#pragma clang fp contract(off)
  sum = sum + g * g;
  return p - lr * (g / (sqrtf(sum) + eps));
}
// The gradient with torch's coupled L2 term, gs * g + wd * p: the decay is added AFTER grad_scale and the clip coefficient
// (clip_grad_norm, then optimizer.step()) and is not scaled by them.  Formed in double -- both products are exact there -- and
// rounded ONCE: where gs * g and wd * p nearly cancel (weights of 0.1 under a decay of 1e-2 meet gradients of 1e-3), the float
// roundings of the two terms would be a large share of what is left, and RMSprop and Adagrad divide by the size of what is left.
__device__ __forceinline__ float uic_decayed_grad(float g, double gs, float wd, float p) {
  return (float)((double)g * gs + (double)wd * (double)p);
}
__device__ __forceinline__ float uic_optim_grad_scale(const UicOptimParams& a) {
#pragma clang fp contract(off)
  float gs = a.grad_scale;
  if (a.sqnorm) {
    const float coef = a.max_norm / (fabsf(a.grad_scale) * sqrtf(a.sqnorm[0]) + 1e-6f);
    if (coef < 1.f) gs *= coef;
  }
  return gs;
}
// The same scale in double for uic_decayed_grad, from the norm as the float pair sqnorm[0] + sqnorm[1] (uic_sqnorm_f64_launch): a
// float coefficient's last bit is a visible share of gs * g + wd * p once the two terms have nearly cancelled.  (The scale of the
// launches without decay stays the float one, from sqnorm[0] alone: Adam's bits are those of before.)
__device__ __forceinline__ double uic_optim_grad_scale_d(const UicOptimParams& a) {
  double gs = (double)a.grad_scale;
  if (a.sqnorm) {
    const double coef = (double)a.max_norm / (fabs(gs) * sqrt((double)a.sqnorm[0] + (double)a.sqnorm[1]) + 1e-6);
    if (coef < 1.0) gs *= coef;
  }
  return gs;
}
constexpr int optim_states(int method) { return method == UIC_OPTIM_ADAM ? 2 : method == UIC_OPTIM_SGD ? 0 : 1; }

// What a launch computes once per lane, in front of its loop.  `skip`: the guard word is set (uniform over the launch: the
// step's gradients are invalid, keep the weights).
struct OptimCoef { float gs, step_size, inv_sqrt_bc2; double gs_d; bool skip; };
template <int METHOD, bool WD>
__device__ __forceinline__ OptimCoef optim_coef(const UicOptimParams& a) {
  OptimCoef c;
  c.step_size = METHOD == UIC_OPTIM_ADAM ? a.lr / a.bc1 : a.lr;
  c.inv_sqrt_bc2 = METHOD == UIC_OPTIM_ADAM ? 1.f / sqrtf(a.bc2) : 1.f;
  c.skip = a.guard && a.guard[0] != 0;
  c.gs = c.skip || WD ? 0.f : uic_optim_grad_scale(a);
  c.gs_d = c.skip || !WD ? 0.0 : uic_optim_grad_scale_d(a);
  return c;
}
// Element i of the arena: loads, the method's update, stores; returns the new parameter.  A method touches only the arrays it
// has (optim_states); WD = false never forms gs * g + 0 * p.
template <int METHOD, bool WD>
__device__ __forceinline__ float optim_element(const UicOptimParams& a, const OptimCoef& c, size_t i) {
  // gradient and state are touched once per step, by this kernel only: streamed past the caches (the parameters are
  // re-read right after by the operand-copy refresh and stay cacheable)
  float g = __builtin_nontemporal_load(a.g + i);
  if (!WD) g *= c.gs;
  float s0 = 0.f, s1 = 0.f;
  if (optim_states(METHOD) > 0) s0 = __builtin_nontemporal_load(a.s0 + i);
  if (optim_states(METHOD) > 1) s1 = __builtin_nontemporal_load(a.s1 + i);
  const float p = a.p[i];
  if (WD) g = uic_decayed_grad(g, c.gs_d, a.weight_decay, p);
  float pn;
  if (METHOD == UIC_OPTIM_ADAM) pn = uic_adam_update(p, s0, s1, g, a.alpha, a.beta, c.step_size, c.inv_sqrt_bc2, a.eps);
  else if (METHOD == UIC_OPTIM_SGD) pn = uic_sgd_update(p, g, c.step_size);
  else if (METHOD == UIC_OPTIM_SGDM) pn = uic_momentum_update<false>(p, s0, g, a.alpha, c.step_size);
  else if (METHOD == UIC_OPTIM_SGDMOM) pn = uic_momentum_update<true>(p, s0, g, a.alpha, c.step_size);
  else if (METHOD == UIC_OPTIM_RMSPROP) pn = uic_rmsprop_update(p, s0, g, a.alpha, c.step_size, a.eps);
  else pn = uic_adagrad_update(p, s0, g, c.step_size, a.eps);
  if (optim_states(METHOD) > 0) __builtin_nontemporal_store(s0, a.s0 + i);
  if (optim_states(METHOD) > 1) __builtin_nontemporal_store(s1, a.s1 + i);
  a.p[i] = pn;
  return pn;
}
// (adam_* for every method: the trace tools under tools/ find the end of a training step by these kernel names)
template <int METHOD, bool WD>
__global__ void adam_kernel(const UicOptimParams a) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const OptimCoef c = optim_coef<METHOD, WD>(a);
  if (c.skip) return;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) optim_element<METHOD, WD>(a, c, i);
}

// The same update on up to UIC_OPTIM_RANGES index ranges of the arena in ONE launch -- the ranges a data-parallel rank owns after
// the reduce-scatter (one per gradient piece) plus the replicated tail -- optionally leaving the updated parameters of those
// ranges in the operand dtype in `w_out` (same element index), which is what the all-gather then distributes.
template <int METHOD, bool WD, typename WT>
__global__ void adam_ranges_kernel(const UicOptimParams a, const UicOptimRanges r, WT* __restrict__ w_out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const OptimCoef c = optim_coef<METHOD, WD>(a);
  if (c.skip) return;
  for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < r.total; j += stride) {
    int k = 0;
    while (k + 1 < r.count && j >= r.start[k + 1]) ++k;       // start[k]: position of range k in the concatenation
    const size_t i = r.lo[k] + (j - r.start[k]);
    const float pn = optim_element<METHOD, WD>(a, c, i);
    if (w_out) w_out[i] = uic_from_f<WT>(pn);
  }
}

// f(method, weight decay present) with both as compile-time constants
template <int METHOD, typename F>
int with_decay(bool wd, F&& f) {
  return wd ? f(std::integral_constant<int, METHOD>{}, std::true_type{}) : f(std::integral_constant<int, METHOD>{}, std::false_type{});
}
template <typename F>
int with_method(const UicOptimParams& a, F&& f) {
  const bool wd = a.weight_decay != 0.f;
  switch (a.method) {
    case UIC_OPTIM_ADAM: return with_decay<UIC_OPTIM_ADAM>(wd, f);
    case UIC_OPTIM_SGD: return with_decay<UIC_OPTIM_SGD>(wd, f);
    case UIC_OPTIM_SGDM: return with_decay<UIC_OPTIM_SGDM>(wd, f);
    case UIC_OPTIM_SGDMOM: return with_decay<UIC_OPTIM_SGDMOM>(wd, f);
    case UIC_OPTIM_RMSPROP: return with_decay<UIC_OPTIM_RMSPROP>(wd, f);
    case UIC_OPTIM_ADAGRAD: return with_decay<UIC_OPTIM_ADAGRAD>(wd, f);
  }
  uic_set_error("optim: unknown method %d", a.method);
  return UIC_EARG;
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
int uic_sqnorm_f64_launch(const float* g, size_t n, float* scratch, float* out, hipStream_t s) {
  UIC_REQUIRE(g && scratch && out, "sqnorm_f64: null pointer");
  UIC_REQUIRE(((uintptr_t)scratch & 7) == 0, "sqnorm_f64: scratch must be 8-byte aligned");
  const size_t want = (n + NT * 8 - 1) / (NT * 8);
  const int blocks = (int)(want > SQ64_BLOCKS ? SQ64_BLOCKS : (want ? want : 1));
  hipLaunchKernelGGL(sqnorm_part_f64_kernel, dim3(blocks), dim3(NT), 0, s, g, n, (double*)scratch);
  UIC_LAUNCH_CHECK("sqnorm_part_f64");
  hipLaunchKernelGGL(sqnorm_final_f64_kernel, dim3(1), dim3(NT), 0, s, (const double*)scratch, blocks, out);
  UIC_LAUNCH_CHECK("sqnorm_final_f64");
  return UIC_OK;
}
int uic_optim_state_count(int method) { return method < 0 || method >= UIC_OPTIM_METHODS ? -1 : optim_states(method); }
int uic_optim_launch(const UicOptimParams& a, hipStream_t s) {
  if (a.n == 0) return UIC_OK;
  return with_method(a, [&](auto method, auto wd) {
    hipLaunchKernelGGL((adam_kernel<method.value, wd.value>), dim3(uic_grid_for(a.n, NT)), dim3(NT), 0, s, a);
    UIC_LAUNCH_CHECK("optim");
    return (int)UIC_OK;
  });
}
int uic_optim_ranges_launch(const UicOptimParams& a, const UicOptimRanges& r, void* w_out, int w_dtype, hipStream_t s) {
  if (r.total == 0) return UIC_OK;
  const int g = uic_grid_for(r.total, NT);
  return with_method(a, [&](auto method, auto wd) {
    constexpr int M = method.value;
    constexpr bool WD = wd.value;
    if (w_out && w_dtype == UIC_BF16) hipLaunchKernelGGL((adam_ranges_kernel<M, WD, bf16_t>), dim3(g), dim3(NT), 0, s, a, r, (bf16_t*)w_out);
    else hipLaunchKernelGGL((adam_ranges_kernel<M, WD, float>), dim3(g), dim3(NT), 0, s, a, r, (float*)nullptr);   // (f32 operands ARE the masters)
    UIC_LAUNCH_CHECK("optim_ranges");
    return (int)UIC_OK;
  });
}
