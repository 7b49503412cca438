// General HBM-bound helper kernels shared by every model's sequencer (gfx950): casts, copies, fills, transposes, column
// sums, the seq_per_img expansion, ReLU-mask gradients, one-workgroup sums, the factored tanh's exponentials and the
// exported dropout mask.  Each group of kernels is followed by its launchers.  (The operators with a file of their own:
// embedding.hip, lstm_cell.hip, adam.hip, sampling.hip, live_rows.hip, criterion.hip, batchnorm.hip.)
#include "uic_common.h"
#include "uic_host.h"
#include <string.h>

namespace {
constexpr int NT = 256;
}  // namespace

// ------------------------------------------------------------------ casts
namespace {
template <typename T>
__global__ void cast_from_f32_kernel(const float* __restrict__ src, T* __restrict__ dst, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
  for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 3 < n) {
      // the f32 source (master parameters, the loader's features) is not read again this step: streamed
      const float4 v = make_float4(__builtin_nontemporal_load(src + i), __builtin_nontemporal_load(src + i + 1),
                                   __builtin_nontemporal_load(src + i + 2), __builtin_nontemporal_load(src + i + 3));
      if constexpr (sizeof(T) == 2) {
        *(uint2*)(dst + i) = make_uint2(uic_pack_bf16x2(v.x, v.y), uic_pack_bf16x2(v.z, v.w));
      } else {
        *(float4*)(dst + i) = v;
      }
    } else {
      for (size_t j = i; j < n; ++j) dst[j] = uic_from_f<T>(src[j]);
    }
  }
}
template <typename T>
__global__ void cast_to_f32_kernel(const T* __restrict__ src, float* __restrict__ dst, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = uic_to_f(src[i]);
}
// up to UIC_CAST_MULTI tensors in ONE launch (blockIdx.y picks the tensor): the weight refresh of a training step is a handful
// of small casts whose launches, not their bytes, are what the step waits for
struct CastMulti { const float* src[UIC_CAST_MULTI]; void* dst[UIC_CAST_MULTI]; size_t n[UIC_CAST_MULTI]; };
template <typename T>
__global__ void cast_multi_kernel(const CastMulti c) {
  const int k = blockIdx.y;
  const float* src = k == 0 ? c.src[0] : k == 1 ? c.src[1] : k == 2 ? c.src[2] : k == 3 ? c.src[3] : k == 4 ? c.src[4] : c.src[5];
  T* dst = (T*)(k == 0 ? c.dst[0] : k == 1 ? c.dst[1] : k == 2 ? c.dst[2] : k == 3 ? c.dst[3] : k == 4 ? c.dst[4] : c.dst[5]);
  const size_t n = k == 0 ? c.n[0] : k == 1 ? c.n[1] : k == 2 ? c.n[2] : k == 3 ? c.n[3] : k == 4 ? c.n[4] : c.n[5];
  const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
  for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 3 < n) {
      const float4 v = make_float4(__builtin_nontemporal_load(src + i), __builtin_nontemporal_load(src + i + 1),
                                   __builtin_nontemporal_load(src + i + 2), __builtin_nontemporal_load(src + i + 3));
      if constexpr (sizeof(T) == 2) *(uint2*)(dst + i) = make_uint2(uic_pack_bf16x2(v.x, v.y), uic_pack_bf16x2(v.z, v.w));
      else *(float4*)(dst + i) = v;
    } else {
      for (size_t j = i; j < n; ++j) dst[j] = uic_from_f<T>(src[j]);
    }
  }
}
}  // namespace
int uic_cast_f32_launch(int dtype, const float* src, void* dst, size_t n, hipStream_t s) {
  if (n == 0) return UIC_OK;
  const int g = uic_grid_for(n, NT * 4);
  UIC_DISPATCH_T(dtype, hipLaunchKernelGGL(cast_from_f32_kernel<bf16_t>, dim3(g), dim3(NT), 0, s, src, (bf16_t*)dst, n),
                 hipLaunchKernelGGL(cast_from_f32_kernel<float>, dim3(g), dim3(NT), 0, s, src, (float*)dst, n));
  UIC_LAUNCH_CHECK("cast_from_f32");
  return UIC_OK;
}
int uic_cast_f32_multi_launch(int dtype, int count, const float* const* src, void* const* dst, const size_t* n, hipStream_t s) {
  UIC_REQUIRE(count >= 0 && count <= UIC_CAST_MULTI, "cast_multi: %d tensors (max %d)", count, UIC_CAST_MULTI);
  CastMulti c;
  memset(&c, 0, sizeof(c));
  size_t most = 0;
  int m = 0;
  for (int i = 0; i < count; ++i) {
    if (n[i] == 0) continue;
    UIC_REQUIRE(src[i] && dst[i] && (((uintptr_t)src[i] | (uintptr_t)dst[i]) & 15) == 0, "cast_multi: tensor %d must be 16-byte aligned", i);
    c.src[m] = src[i]; c.dst[m] = dst[i]; c.n[m] = n[i];
    if (n[i] > most) most = n[i];
    ++m;
  }
  if (m == 0) return UIC_OK;
  const int g = uic_grid_for(most, NT * 4);
  UIC_DISPATCH_T(dtype, hipLaunchKernelGGL(cast_multi_kernel<bf16_t>, dim3(g, m), dim3(NT), 0, s, c),
                 hipLaunchKernelGGL(cast_multi_kernel<float>, dim3(g, m), dim3(NT), 0, s, c));
  UIC_LAUNCH_CHECK("cast_multi");
  return UIC_OK;
}
int uic_to_f32_launch(int dtype, const void* src, float* dst, size_t n, hipStream_t s) {
  if (n == 0) return UIC_OK;
  const int g = uic_grid_for(n, NT);
  UIC_DISPATCH_T(dtype, hipLaunchKernelGGL(cast_to_f32_kernel<bf16_t>, dim3(g), dim3(NT), 0, s, (const bf16_t*)src, dst, n),
                 hipLaunchKernelGGL(cast_to_f32_kernel<float>, dim3(g), dim3(NT), 0, s, (const float*)src, dst, n));
  UIC_LAUNCH_CHECK("cast_to_f32");
  return UIC_OK;
}

// ------------------------------------------------------------------ copies
namespace {
typedef __attribute__((ext_vector_type(4))) unsigned u32x4m;
struct CopyMulti { const u32x4m* src[UIC_CAST_MULTI]; u32x4m* dst[UIC_CAST_MULTI]; size_t n16[UIC_CAST_MULTI]; };
__global__ __launch_bounds__(NT) void copy_multi_kernel(const CopyMulti c) {
  const int k = blockIdx.y;
  const u32x4m* src = c.src[k];
  u32x4m* dst = c.dst[k];
  const size_t n = c.n16[k], stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = __builtin_nontemporal_load(src + i);
}
// device-to-device copy as an ordinary kernel: hipMemcpyAsync(DeviceToDevice) holds the calling host thread until the stream
// has drained up to the copy (measured: the other stream's launches behind it were enqueued ~0.2 ms late in the fused step)
__global__ void copy_words_kernel(const unsigned* __restrict__ src, unsigned* __restrict__ dst, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = src[i];
}
}  // namespace
// up to UIC_CAST_MULTI device-to-device copies in ONE launch (sizes in bytes, multiples of 16; 16-byte aligned pointers)
int uic_copy_multi_launch(int count, const void* const* src, void* const* dst, const size_t* bytes, hipStream_t s) {
  UIC_REQUIRE(count >= 0 && count <= UIC_CAST_MULTI, "copy_multi: %d tensors (max %d)", count, UIC_CAST_MULTI);
  CopyMulti c;
  memset(&c, 0, sizeof(c));
  size_t most = 0;
  int m = 0;
  for (int i = 0; i < count; ++i) {
    if (bytes[i] == 0) continue;
    UIC_REQUIRE(src[i] && dst[i] && (((uintptr_t)src[i] | (uintptr_t)dst[i] | bytes[i]) & 15) == 0, "copy_multi: tensor %d must be 16-byte aligned", i);
    c.src[m] = (const u32x4m*)src[i]; c.dst[m] = (u32x4m*)dst[i]; c.n16[m] = bytes[i] / 16;
    if (c.n16[m] > most) most = c.n16[m];
    ++m;
  }
  if (m == 0) return UIC_OK;
  hipLaunchKernelGGL(copy_multi_kernel, dim3(uic_grid_for(most, NT * 2), m), dim3(NT), 0, s, c);
  UIC_LAUNCH_CHECK("copy_multi");
  return UIC_OK;
}
int uic_copy_launch(void* dst, const void* src, size_t bytes, hipStream_t s) {
  if (bytes == 0) return UIC_OK;
  UIC_REQUIRE(bytes % 4 == 0 && ((uintptr_t)dst & 3) == 0 && ((uintptr_t)src & 3) == 0, "copy: %zu bytes / pointers must be 4-byte aligned", bytes);
  const size_t n = bytes / 4;
  const int g = uic_grid_for(n, NT);
  hipLaunchKernelGGL(copy_words_kernel, dim3(g), dim3(NT), 0, s, (const unsigned*)src, (unsigned*)dst, n);
  UIC_LAUNCH_CHECK("copy_words");
  return UIC_OK;
}

// ------------------------------------------------------------------ fills and zeroing
namespace {
template <typename T>
__global__ void fill_value_kernel(T* __restrict__ dst, size_t n, float value) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = uic_from_f<T>(value);
}
struct UicZero4 { uint4* p[4]; size_t n[4]; };     // n in 16-byte units
__global__ void zero4_kernel(const UicZero4 z) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const uint4 zero = make_uint4(0, 0, 0, 0);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < z.n[k]; i += stride) z.p[k][i] = zero;
}
// up to UIC_ZERO_LIST buffers in ONE launch (blockIdx.y picks the buffer): a step of the pivot NMT cleared 18 small buffers with
// 18 memsets of ~6 us each on its only stream
struct UicZeroList { uint4* p[UIC_ZERO_LIST]; size_t n[UIC_ZERO_LIST]; };     // n in 16-byte units
__global__ void zero_list_kernel(const UicZeroList z) {
  uint4* p = nullptr;
  size_t n = 0;
#pragma unroll
  for (int k = 0; k < UIC_ZERO_LIST; ++k)
    if (k == (int)blockIdx.y) { p = z.p[k]; n = z.n[k]; }
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const uint4 zero = make_uint4(0, 0, 0, 0);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = zero;
}
}  // namespace
int uic_fill_launch(void* dst, int value_byte, size_t bytes, hipStream_t s) {
  if (bytes == 0) return UIC_OK;
  return uic_check_hip(hipMemsetAsync(dst, value_byte, bytes, s), "hipMemsetAsync");
}
int uic_fill_value_launch(int dtype, void* dst, size_t n, float value, hipStream_t s) {
  if (n == 0) return UIC_OK;
  const int g = uic_grid_for(n, NT);
  UIC_DISPATCH_T(dtype, hipLaunchKernelGGL(fill_value_kernel<bf16_t>, dim3(g), dim3(NT), 0, s, (bf16_t*)dst, n, value),
                 hipLaunchKernelGGL(fill_value_kernel<float>, dim3(g), dim3(NT), 0, s, (float*)dst, n, value));
  UIC_LAUNCH_CHECK("fill_value");
  return UIC_OK;
}
int uic_zero4_launch(void* p0, size_t b0, void* p1, size_t b1, void* p2, size_t b2, void* p3, size_t b3, hipStream_t s) {
  void* ps[4] = {p0, p1, p2, p3};
  const size_t bs[4] = {b0, b1, b2, b3};
  UicZero4 z;
  size_t most = 0;
  for (int k = 0; k < 4; ++k) {
    UIC_REQUIRE(bs[k] == 0 || (ps[k] && ((uintptr_t)ps[k] & 15) == 0 && bs[k] % 16 == 0), "zero4: buffer %d must be 16-byte aligned / sized", k);
    z.p[k] = (uint4*)ps[k];
    z.n[k] = bs[k] / 16;
    if (z.n[k] > most) most = z.n[k];
  }
  if (most == 0) return UIC_OK;
  hipLaunchKernelGGL(zero4_kernel, dim3(uic_grid_for(most, NT)), dim3(NT), 0, s, z);
  UIC_LAUNCH_CHECK("zero4");
  return UIC_OK;
}
int uic_zero_list_launch(void* const* ptrs, const size_t* bytes, int n, hipStream_t s) {
  for (int k0 = 0; k0 < n; k0 += UIC_ZERO_LIST) {
    UicZeroList z;
    memset(&z, 0, sizeof(z));
    size_t most = 0;
    int m = 0;
    for (int k = k0; k < n && k < k0 + UIC_ZERO_LIST; ++k) {
      if (bytes[k] == 0) continue;
      UIC_REQUIRE(ptrs[k] && ((uintptr_t)ptrs[k] & 15) == 0 && bytes[k] % 16 == 0, "zero_list: buffer %d must be 16-byte aligned / sized", k);
      z.p[m] = (uint4*)ptrs[k];
      z.n[m] = bytes[k] / 16;
      if (z.n[m] > most) most = z.n[m];
      ++m;
    }
    if (m == 0) continue;
    int gx = uic_grid_for(most, NT);
    if (gx > 512) gx = 512;
    hipLaunchKernelGGL(zero_list_kernel, dim3(gx, m), dim3(NT), 0, s, z);
    UIC_LAUNCH_CHECK("zero_list");
  }
  return UIC_OK;
}

// ------------------------------------------------------------------ transposes
namespace {
template <typename T>
__global__ __launch_bounds__(NT) void transpose_kernel(const T* __restrict__ src, int rows, int cols, int lds,
                                                       T* __restrict__ dst, int ldd) {
  __shared__ T tile[64][66];
  const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int r = r0 + ty + 4 * i, c = c0 + tx;
    T v = uic_from_f<T>(0.f);
    if (r < rows && c < cols) v = src[(size_t)r * lds + c];
    tile[ty + 4 * i][tx] = v;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = c0 + ty + 4 * i, r = r0 + tx;
    if (c < cols && r < ldd) dst[(size_t)c * ldd + r] = tile[tx][ty + 4 * i];
  }
}

// several transposes in one launch (blockIdx.z picks the job; every field by a uniform select -- indexing the by-value
// table would put it in private memory): the weight refresh's transposes are launch-bound, not byte-bound
struct TransposeMulti { UicTransposeJob j[UIC_TRANSPOSE_MULTI]; int start[UIC_TRANSPOSE_MULTI + 1]; };   // start[k]: first 64 x 64 tile of job k
#define UIC_TSEL2(f) (k == 0 ? c.f[0] : k == 1 ? c.f[1] : k == 2 ? c.f[2] : k == 3 ? c.f[3] : k == 4 ? c.f[4] : k == 5 ? c.f[5] : \
                      k == 6 ? c.f[6] : k == 7 ? c.f[7] : k == 8 ? c.f[8] : k == 9 ? c.f[9] : k == 10 ? c.f[10] : c.f[11])
#define UIC_TSEL(f) (k == 0 ? c.j[0].f : k == 1 ? c.j[1].f : k == 2 ? c.j[2].f : k == 3 ? c.j[3].f : k == 4 ? c.j[4].f : k == 5 ? c.j[5].f : \
                     k == 6 ? c.j[6].f : k == 7 ? c.j[7].f : k == 8 ? c.j[8].f : k == 9 ? c.j[9].f : k == 10 ? c.j[10].f : c.j[11].f)
template <typename T>
__global__ __launch_bounds__(NT) void transpose_multi_kernel(const TransposeMulti c) {
  __shared__ T tile[64][66];
  // the job of this tile: the grid is the concatenation of the jobs' tile lists (one block per 64 x 64 tile, none idle)
  int k = 0;
#pragma unroll
  for (int q = 1; q < UIC_TRANSPOSE_MULTI; ++q) k += (int)blockIdx.x >= c.start[q] ? 1 : 0;
  const T* __restrict__ src = (const T*)UIC_TSEL(src);
  T* __restrict__ dst = (T*)UIC_TSEL(dst);
  const int rows = UIC_TSEL(rows), cols = UIC_TSEL(cols), lds = UIC_TSEL(lds), ldd = UIC_TSEL(ldd);
  const int t = blockIdx.x - UIC_TSEL2(start), tx_n = (ldd + 63) / 64;
  const int r0 = (t % tx_n) * 64, c0 = (t / tx_n) * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int r = r0 + ty + 4 * i, cc = c0 + tx;
    T v = uic_from_f<T>(0.f);
    if (r < rows && cc < cols) v = src[(size_t)r * lds + cc];
    tile[ty + 4 * i][tx] = v;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int cc = c0 + ty + 4 * i, r = r0 + tx;
    if (cc < cols && r < ldd) dst[(size_t)cc * ldd + r] = tile[tx][ty + 4 * i];
  }
}
#undef UIC_TSEL
#undef UIC_TSEL2
}  // namespace
int uic_transpose_launch(int dtype, const void* src, int rows, int cols, int lds, void* dst, int ldd, hipStream_t s) {
  UIC_REQUIRE(ldd >= rows && lds >= cols, "transpose: ldd=%d < rows=%d or lds=%d < cols=%d", ldd, rows, lds, cols);
  if (rows == 0 || cols == 0) return UIC_OK;
  dim3 grid((ldd + 63) / 64, (cols + 63) / 64);
  UIC_DISPATCH_T(dtype,
                 hipLaunchKernelGGL(transpose_kernel<bf16_t>, grid, dim3(NT), 0, s, (const bf16_t*)src, rows, cols, lds, (bf16_t*)dst, ldd),
                 hipLaunchKernelGGL(transpose_kernel<float>, grid, dim3(NT), 0, s, (const float*)src, rows, cols, lds, (float*)dst, ldd));
  UIC_LAUNCH_CHECK("transpose");
  return UIC_OK;
}
int uic_transpose_multi_launch(int dtype, int count, const UicTransposeJob* jobs, hipStream_t s) {
  UIC_REQUIRE(count >= 0 && count <= UIC_TRANSPOSE_MULTI, "transpose_multi: %d jobs (max %d)", count, UIC_TRANSPOSE_MULTI);
  TransposeMulti c;
  memset(&c, 0, sizeof(c));
  int m = 0, tiles = 0;
  for (int i = 0; i < count; ++i) {
    if (jobs[i].rows == 0 || jobs[i].cols == 0) continue;
    c.start[m] = tiles;
    c.j[m++] = jobs[i];
    tiles += ((jobs[i].ldd + 63) / 64) * ((jobs[i].cols + 63) / 64);
  }
  if (m == 0) return UIC_OK;
  for (int i = m; i <= UIC_TRANSPOSE_MULTI; ++i) c.start[i] = 0x7fffffff;     // (never reached by a block index)
  UIC_DISPATCH_T(dtype, hipLaunchKernelGGL(transpose_multi_kernel<bf16_t>, dim3(tiles), dim3(NT), 0, s, c),
                 hipLaunchKernelGGL(transpose_multi_kernel<float>, dim3(tiles), dim3(NT), 0, s, c));
  UIC_LAUNCH_CHECK("transpose_multi");
  return UIC_OK;
}

// ------------------------------------------------------------------ column sums (bias gradients) and sums over the steps
namespace {
// stage 1: a block sums `rows_per_block` rows of a 64-column strip; its 4 waves take rows r, r+4, ...
template <typename T>
__global__ __launch_bounds__(NT) void colsum_stage1(const T* __restrict__ src, int rows, int cols, int lds,
                                                    int rows_per_block, float* __restrict__ part) {
  __shared__ float s_part[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int rb = blockIdx.y;
  const int r_lo = rb * rows_per_block;
  const int r_hi = min(rows, r_lo + rows_per_block);
  float s = 0.f;
  if (c < cols) {
#pragma unroll 4
    for (int r = r_lo + wave; r < r_hi; r += 4) s += uic_to_f(src[(size_t)r * lds + c]);
  }
  s_part[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && c < cols) part[(size_t)rb * cols + c] = s_part[0][lane] + s_part[1][lane] + s_part[2][lane] + s_part[3][lane];
}
// stage 2: 64 columns per block; the 4 waves split the row-block partials (fixed order -> deterministic)
__global__ __launch_bounds__(NT) void colsum_stage2(const float* __restrict__ part, int nrb, int cols, float* __restrict__ out) {
  __shared__ float s_part[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  float s = 0.f;
  if (c < cols) {
#pragma unroll 4
    for (int rb = wave; rb < nrb; rb += 4) s += part[(size_t)rb * cols + c];
  }
  s_part[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && c < cols) out[c] = (s_part[0][lane] + s_part[1][lane]) + (s_part[2][lane] + s_part[3][lane]);
}
// out[c] = sum_n part[n, c] for the ncols <= 1024 columns of a small [rows, ncols] f32 matrix, split over two destinations
// (columns [0, n0) -> out0, the rest -> out1): d w_alpha / d b_alpha from the attention accumulation's per-row partials in ONE
// launch instead of a two-stage column sum and two copies.
__global__ __launch_bounds__(1024) void colsum_small_kernel(const float* __restrict__ part, int rows, int ncols, int n0, float* __restrict__ out0,
                                                            float* __restrict__ out1) {
  __shared__ float s_acc[16][64];
  const int lc = threadIdx.x & 63, g = threadIdx.x >> 6;          // 64 columns x 16 row groups per workgroup
  const int c = blockIdx.x * 64 + lc;
  float acc = 0.f;
  if (c < ncols) {
#pragma unroll 8
    for (int r = g; r < rows; r += 16) acc += part[(size_t)r * ncols + c];
  }
  s_acc[g][lc] = acc;
  __syncthreads();
  if (g == 0 && c < ncols) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) v += s_acc[k][lc];
    if (c < n0) out0[c] = v; else out1[c - n0] = v;
  }
}
template <typename T>
__global__ void sum_steps_kernel(const T* __restrict__ src, int TS, size_t step, T* __restrict__ dst) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < step; i += stride) {
    float s = 0.f;
    for (int t = 0; t < TS; ++t) s += uic_to_f(src[(size_t)t * step + i]);
    dst[i] = uic_from_f<T>(s);
  }
}
// 16-byte chunks (step_elems a multiple of the vector width, 16-byte aligned pointers): one load instruction per step
template <typename T>
__global__ void sum_steps_vec_kernel(const T* __restrict__ src, int TS, size_t step, T* __restrict__ dst) {
  constexpr int VEC = uic_vec<T>::N;
  const size_t nch = step / VEC;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c < nch; c += stride) {
    float acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
#pragma unroll 4
    for (int t = 0; t < TS; ++t) {
      const uint4 v = *(const uint4*)(src + (size_t)t * step + c * VEC);
      float f[VEC];
      uic_unpack<T>(v, f);
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc[j] += f[j];
    }
    *(uint4*)(dst + c * VEC) = uic_pack<T>(acc);
  }
}
}  // namespace
int uic_colsum_launch(int src_dtype, const void* src, int rows, int cols, int lds, float* out, float* scratch,
                      size_t scratch_floats, hipStream_t s) {
  if (cols == 0) return UIC_OK;
  int nrb = (rows + 63) / 64;
  if (nrb > 32) nrb = 32;
  if (nrb < 1) nrb = 1;
  while (nrb > 1 && (size_t)nrb * cols > scratch_floats) nrb /= 2;
  UIC_REQUIRE((size_t)nrb * cols <= scratch_floats, "colsum: scratch too small (%zu floats for %d cols)", scratch_floats, cols);
  const int rpb = (rows + nrb - 1) / nrb;
  dim3 grid((cols + 63) / 64, nrb);
  UIC_DISPATCH_T(src_dtype,
                 hipLaunchKernelGGL(colsum_stage1<bf16_t>, grid, dim3(NT), 0, s, (const bf16_t*)src, rows, cols, lds, rpb, scratch),
                 hipLaunchKernelGGL(colsum_stage1<float>, grid, dim3(NT), 0, s, (const float*)src, rows, cols, lds, rpb, scratch));
  UIC_LAUNCH_CHECK("colsum_stage1");
  hipLaunchKernelGGL(colsum_stage2, dim3((cols + 63) / 64), dim3(NT), 0, s, scratch, nrb, cols, out);
  UIC_LAUNCH_CHECK("colsum_stage2");
  return UIC_OK;
}
int uic_colsum_small_launch(const float* part, int rows, int ncols, int n0, float* out0, float* out1, hipStream_t s) {
  if (ncols == 0) return UIC_OK;
  hipLaunchKernelGGL(colsum_small_kernel, dim3((ncols + 63) / 64), dim3(1024), 0, s, part, rows, ncols, n0, out0, out1);
  UIC_LAUNCH_CHECK("colsum_small");
  return UIC_OK;
}
int uic_sum_steps_launch(int dtype, const void* src, int T, size_t step_elems, void* dst, hipStream_t s) {
  if (step_elems == 0) return UIC_OK;
  const size_t vec = dtype == UIC_BF16 ? 8 : 4;
  if (step_elems % vec == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
    const int gv = uic_grid_for(step_elems / vec, NT);
    UIC_DISPATCH_T(dtype, hipLaunchKernelGGL(sum_steps_vec_kernel<bf16_t>, dim3(gv), dim3(NT), 0, s, (const bf16_t*)src, T, step_elems, (bf16_t*)dst),
                   hipLaunchKernelGGL(sum_steps_vec_kernel<float>, dim3(gv), dim3(NT), 0, s, (const float*)src, T, step_elems, (float*)dst));
    UIC_LAUNCH_CHECK("sum_steps_vec");
    return UIC_OK;
  }
  const int g = uic_grid_for(step_elems, NT);
  UIC_DISPATCH_T(dtype, hipLaunchKernelGGL(sum_steps_kernel<bf16_t>, dim3(g), dim3(NT), 0, s, (const bf16_t*)src, T, step_elems, (bf16_t*)dst),
                 hipLaunchKernelGGL(sum_steps_kernel<float>, dim3(g), dim3(NT), 0, s, (const float*)src, T, step_elems, (float*)dst));
  UIC_LAUNCH_CHECK("sum_steps");
  return UIC_OK;
}

// ------------------------------------------------------------------ seq_per_img > 1: per-image features -> caption rows
// (the loader's S-fold replication, P/misc/dataloader/dataloader.py:270-277, done on the device instead of the host),
// and the ReLU-mask gradients of the embedded features, plain and folded back over the S captions of an image
namespace {
template <typename T>
__global__ void expand_rows_kernel(const float* __restrict__ src, T* __restrict__ dst, int S, size_t row, size_t total) {
  const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
  for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < total; i += stride) {   // i indexes src; row % 4 == 0
    const size_t img = i / row, e = i - img * row;
    const float4 v = *(const float4*)(src + i);
    for (int j = 0; j < S; ++j) {
      T* o = dst + (img * S + j) * row + e;
      if constexpr (sizeof(T) == 2) *(uint2*)o = make_uint2(uic_pack_bf16x2(v.x, v.y), uic_pack_bf16x2(v.z, v.w));
      else *(float4*)o = v;
    }
  }
}
template <typename T>
__global__ void expand_rows_scalar_kernel(const float* __restrict__ src, T* __restrict__ dst, int S, size_t row, size_t total) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const size_t img = i / row, e = i - img * row;
    for (int j = 0; j < S; ++j) dst[(img * S + j) * row + e] = uic_from_f<T>(src[i]);
  }
}
template <typename T>
__global__ void expand_drop_kernel(const float* __restrict__ y, T* __restrict__ out, int S, size_t row, size_t total,
                                   float drop_p, unsigned seed, unsigned site) {
  const float inv_keep = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
  const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
  for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < total; i += stride) {
    const size_t img = i / row, e = i - img * row;
    const float4 v = *(const float4*)(y + i);
    const float f[4] = {v.x, v.y, v.z, v.w};
    for (int j = 0; j < S; ++j) {
      const size_t o = (img * S + j) * row + e;
      float g[4];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        g[q] = drop_p > 0.f ? f[q] * uic_drop_scale(seed, site, (unsigned)(o + q), drop_p, inv_keep) : f[q];
      if constexpr (sizeof(T) == 2) *(uint2*)(out + o) = make_uint2(uic_pack_bf16x2(g[0], g[1]), uic_pack_bf16x2(g[2], g[3]));
      else *(float4*)(out + o) = make_float4(g[0], g[1], g[2], g[3]);
    }
  }
}
template <typename T>
__global__ void relu_mask_bwd_kernel(const float* __restrict__ g, const T* __restrict__ act, float scale,
                                     T* __restrict__ dst, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    dst[i] = uic_from_f<T>(uic_to_f(act[i]) > 0.f ? g[i] * scale : 0.f);
}
template <typename T>
__global__ void relu_mask_bwd_fold_kernel(const float* __restrict__ g, const T* __restrict__ act, float scale,
                                          T* __restrict__ dst, int S, size_t row, size_t total) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const size_t img = i / row, e = i - img * row;
    float acc = 0.f;
    for (int j = 0; j < S; ++j) {
      const size_t o = (img * S + j) * row + e;
      acc += uic_to_f(act[o]) > 0.f ? g[o] * scale : 0.f;
    }
    dst[i] = uic_from_f<T>(acc);
  }
}
}  // namespace
int uic_expand_rows_launch(int dtype_out, const float* src, void* dst, int n_img, int S, size_t row, hipStream_t s) {
  UIC_REQUIRE(src && dst && S >= 1, "expand_rows: bad arguments");
  const size_t total = (size_t)n_img * row;
  if (total == 0) return UIC_OK;
  if (row % 4 != 0) {     // short odd rows (att_masks [n_img, R])
    const int g1 = uic_grid_for(total, NT);
    UIC_DISPATCH_T(dtype_out, hipLaunchKernelGGL(expand_rows_scalar_kernel<bf16_t>, dim3(g1), dim3(NT), 0, s, src, (bf16_t*)dst, S, row, total),
                   hipLaunchKernelGGL(expand_rows_scalar_kernel<float>, dim3(g1), dim3(NT), 0, s, src, (float*)dst, S, row, total));
    UIC_LAUNCH_CHECK("expand_rows_scalar");
    return UIC_OK;
  }
  const int g = uic_grid_for(total / 4, NT);
  UIC_DISPATCH_T(dtype_out, hipLaunchKernelGGL(expand_rows_kernel<bf16_t>, dim3(g), dim3(NT), 0, s, src, (bf16_t*)dst, S, row, total),
                 hipLaunchKernelGGL(expand_rows_kernel<float>, dim3(g), dim3(NT), 0, s, src, (float*)dst, S, row, total));
  UIC_LAUNCH_CHECK("expand_rows");
  return UIC_OK;
}
int uic_expand_drop_launch(int dtype, const float* y, void* out, int n_img, int S, size_t row, float drop_p, unsigned seed,
                           unsigned site, hipStream_t s) {
  UIC_REQUIRE(y && out && S >= 1 && row % 4 == 0, "expand_drop: bad arguments");
  const size_t total = (size_t)n_img * row;
  if (total == 0) return UIC_OK;
  const int g = uic_grid_for(total / 4, NT);
  UIC_DISPATCH_T(dtype, hipLaunchKernelGGL(expand_drop_kernel<bf16_t>, dim3(g), dim3(NT), 0, s, y, (bf16_t*)out, S, row, total, drop_p, seed, site),
                 hipLaunchKernelGGL(expand_drop_kernel<float>, dim3(g), dim3(NT), 0, s, y, (float*)out, S, row, total, drop_p, seed, site));
  UIC_LAUNCH_CHECK("expand_drop");
  return UIC_OK;
}
int uic_relu_mask_bwd_launch(int dtype, const float* grad, const void* act, float scale, void* dst, size_t n, hipStream_t s) {
  if (n == 0) return UIC_OK;
  const int g = uic_grid_for(n, NT);
  UIC_DISPATCH_T(dtype, hipLaunchKernelGGL(relu_mask_bwd_kernel<bf16_t>, dim3(g), dim3(NT), 0, s, grad, (const bf16_t*)act, scale, (bf16_t*)dst, n),
                 hipLaunchKernelGGL(relu_mask_bwd_kernel<float>, dim3(g), dim3(NT), 0, s, grad, (const float*)act, scale, (float*)dst, n));
  UIC_LAUNCH_CHECK("relu_mask_bwd");
  return UIC_OK;
}
int uic_relu_mask_bwd_fold_launch(int dtype, const float* grad, const void* act, float scale, void* dst, int n_img, int S,
                                  size_t row, hipStream_t s) {
  UIC_REQUIRE(grad && act && dst && S >= 1, "relu_mask_bwd_fold: bad arguments");
  const size_t total = (size_t)n_img * row;
  if (total == 0) return UIC_OK;
  const int g = uic_grid_for(total, NT);
  UIC_DISPATCH_T(dtype, hipLaunchKernelGGL(relu_mask_bwd_fold_kernel<bf16_t>, dim3(g), dim3(NT), 0, s, grad, (const bf16_t*)act, scale, (bf16_t*)dst, S, row, total),
                 hipLaunchKernelGGL(relu_mask_bwd_fold_kernel<float>, dim3(g), dim3(NT), 0, s, grad, (const float*)act, scale, (float*)dst, S, row, total));
  UIC_LAUNCH_CHECK("relu_mask_bwd_fold");
  return UIC_OK;
}

// ------------------------------------------------------------------ one-workgroup sums (the criterion kernels: criterion.hip)
namespace {
constexpr int MS_NT = 1024, MS_U = 16;
__global__ __launch_bounds__(MS_NT) void masked_sum_kernel(const float* __restrict__ mask, int ldmask, int col0, int N, int TS,
                                                           float* out_sum, float* out_inv) {
  __shared__ float s_buf[MS_NT / 64];
  // One workgroup (the sum is one number and must not depend on a grid), but ONE round trip: 1024 threads x 16 unconditional
  // loads from clamped addresses cover the reference's 640 x 17 mask in a single pass (round 6; 256 threads x 8 loads at a time
  // took six dependent passes -- 12-19 us at the head of the step's side stream)
  float s = 0.f;
  const int total = N * TS;
  for (int i0 = threadIdx.x; i0 < total; i0 += MS_NT * MS_U) {
    float v[MS_U];
#pragma unroll
    for (int u = 0; u < MS_U; ++u) {
      int i = i0 + u * MS_NT;
      i = i < total ? i : total - 1;
      const int n = i / TS, t = i - n * TS;
      v[u] = mask[(size_t)n * ldmask + col0 + t];
    }
#pragma unroll
    for (int u = 0; u < MS_U; ++u) s += i0 + u * MS_NT < total ? v[u] : 0.f;
  }
  s = uic_wave_sum(s);
  if ((threadIdx.x & 63) == 0) s_buf[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
#pragma unroll
    for (int k = 0; k < MS_NT / 64; ++k) tot += s_buf[k];
    if (out_sum) out_sum[0] = tot;
    if (out_inv) out_inv[0] = 1.f / tot;
  }
}

__global__ __launch_bounds__(NT) void reduce_sum_kernel(const float* __restrict__ x, size_t n, const float* scale, float* out) {
  __shared__ float s_buf[NT / 64];
  float s = 0.f;
  for (size_t i0 = threadIdx.x; i0 < n; i0 += (size_t)NT * 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = i0 + (size_t)u * NT < n ? x[i0 + (size_t)u * NT] : 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  s = uic_block_sum<NT>(s, s_buf);
  if (threadIdx.x == 0) out[0] = scale ? s * scale[0] : s;
}
}  // namespace
int uic_masked_sum_launch(const float* mask, int ldmask, int col0, int N, int T, float* out_sum, float* out_inv, hipStream_t s) {
  hipLaunchKernelGGL(masked_sum_kernel, dim3(1), dim3(MS_NT), 0, s, mask, ldmask, col0, N, T, out_sum, out_inv);
  UIC_LAUNCH_CHECK("masked_sum");
  return UIC_OK;
}
int uic_reduce_sum_launch(const float* x, size_t n, const float* scale, float* out, hipStream_t s) {
  hipLaunchKernelGGL(reduce_sum_kernel, dim3(1), dim3(NT), 0, s, x, n, scale, out);
  UIC_LAUNCH_CHECK("reduce_sum");
  return UIC_OK;
}

// ------------------------------------------------------------------ e^{2x} of the factored tanh (uic_common.h: UIC_E2_CLAMP)
namespace {
__global__ __launch_bounds__(256) void exp2x2_bf16_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n8) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
    float f[8];
    uic_unpack<bf16_t>(src[i], f);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      f[j] = __builtin_amdgcn_exp2f(fminf(fmaxf(f[j] * 2.8853900817779268f, -UIC_E2_CLAMP), UIC_E2_CLAMP));
    dst[i] = uic_pack<bf16_t>(f);
  }
}
}  // namespace
int uic_exp2x2_launch(const void* src, void* dst, size_t n, hipStream_t s) {
  UIC_REQUIRE(n % 8 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0, "exp2x2: n %% 8 and 16-byte alignment");
  if (n == 0) return UIC_OK;
  hipLaunchKernelGGL(exp2x2_bf16_kernel, dim3(uic_grid_for(n / 8, 256)), dim3(256), 0, s, (const uint4*)src, (uint4*)dst, n / 8);
  UIC_LAUNCH_CHECK("exp2x2");
  return UIC_OK;
}

// ------------------------------------------------------------------ the dropout mask of a site, for tests and exports
namespace {
__global__ void dropout_mask_kernel(float* out, size_t n, float pdrop, unsigned seed, unsigned site, size_t base) {
  const float inv_keep = pdrop > 0.f ? 1.f / (1.f - pdrop) : 1.f;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    out[i] = pdrop > 0.f ? uic_drop_scale(seed, site, (unsigned)(base + i), pdrop, inv_keep) : 1.f;
}
}  // namespace
int uic_dropout_mask_launch(float* out, size_t n, float p, unsigned seed, unsigned site, size_t base, hipStream_t s) {
  if (n == 0) return UIC_OK;
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(uic_grid_for(n, NT)), dim3(NT), 0, s, out, n, p, seed, site, base);
  UIC_LAUNCH_CHECK("dropout_mask");
  return UIC_OK;
}
