// The second pass of every split-K GEMM of the family: slice z of the launch left its raw f32 partial tile in slab[z][M][N], and
// these kernels sum the slices in a fixed order (deterministic) into the destination(s).  One destination (the NT kernels of
// gemm_glds.hip / gemm_pp.hip), one destination with its rows placed by a list, or up to four column ranges of the slab going to
// four matrices (the weight gradients of gemm_tn.hip / gemm_tn_pp.hip).
#include "uic_common.h"

// ---- one destination
namespace {
__global__ void splitk_reduce_kernel(const float* __restrict__ slab, int splitk, int M, int N, int col0, int ncols,
                                     float* __restrict__ C, int ldc, int accumulate) {
  const size_t total = (size_t)M * ncols;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int row = (int)(i / ncols), c = (int)(i - (size_t)row * ncols);
    const float* src = slab + (size_t)row * N + col0 + c;
    float v = 0.f;
    for (int z = 0; z < splitk; ++z) v += src[(size_t)z * M * N];
    if (accumulate) v += C[(size_t)row * ldc + c];
    C[(size_t)row * ldc + c] = v;
  }
}
// four columns per lane, the row from the grid (see splitk_reduce_multi_vec_kernel below)
__global__ void splitk_reduce_vec_kernel(const float* __restrict__ slab, int splitk, int M, int N, int col0, int ncols,
                                         float* __restrict__ C, int ldc, int accumulate) {
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (c >= ncols) return;
  const size_t MN = (size_t)M * N;
  for (int row = blockIdx.y; row < M; row += gridDim.y) {
    const float* src = slab + (size_t)row * N + col0 + c;
    float4 v = *(const float4*)src;
    for (int z = 1; z < splitk; ++z) {
      const float4 w = *(const float4*)(src + (size_t)z * MN);
      v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
    }
    float4* o = (float4*)(C + (size_t)row * ldc + c);
    if (accumulate) { const float4 w = *o; v.x = w.x + v.x; v.y = w.y + v.y; v.z = w.z + v.z; v.w = w.w + v.w; }
    *o = v;
  }
}
// the same sum with the output rows placed by a list: row r < map_rows of the slab goes to row map[r] of C (entries outside
// [0, map_limit) -- a list's -1 padding -- and rows >= map_rows are dropped).  The live-position logit layer's d hdrop (topdown_step.hip).
__global__ void splitk_reduce_rows_kernel(const float* __restrict__ slab, int splitk, int M, int N, const int* __restrict__ map, int map_rows,
                                          int map_limit, float* __restrict__ C, int ldc) {
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (c >= N) return;
  const size_t MN = (size_t)M * N;
  for (int row = blockIdx.y; row < map_rows; row += gridDim.y) {
    const int orow = map[row];
    const float* src = slab + (size_t)row * N + c;
    float4 v = *(const float4*)src;
    for (int z = 1; z < splitk; ++z) {
      const float4 w = *(const float4*)(src + (size_t)z * MN);
      v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
    }
    if ((unsigned)orow < (unsigned)map_limit) *(float4*)(C + (size_t)orow * ldc + c) = v;
  }
}
}  // namespace

bool uic_splitk_reduce_rows_ok(const float* slab, int M, int N, const float* C, int ldc) {
  return N % 4 == 0 && ldc % 4 == 0 && ((uintptr_t)slab & 15) == 0 && ((uintptr_t)C & 15) == 0 && ((size_t)M * N) % 4 == 0;
}
int uic_splitk_reduce_rows_launch(const float* slab, int splitk, int M, int N, const int* map, int map_rows, int map_limit, float* C, int ldc,
                                  hipStream_t s) {
  UIC_REQUIRE(map && map_rows <= M && uic_splitk_reduce_rows_ok(slab, M, N, C, ldc), "splitk_reduce_rows: bad arguments");
  if (map_rows <= 0) return UIC_OK;
  const int bt = N / 4 >= 256 ? 256 : ((N / 4 + 63) / 64) * 64;
  hipLaunchKernelGGL(splitk_reduce_rows_kernel, dim3((unsigned)((N / 4 + bt - 1) / bt), (unsigned)(map_rows > 65535 ? 65535 : map_rows)), dim3(bt), 0, s,
                     slab, splitk, M, N, map, map_rows, map_limit, C, ldc);
  UIC_LAUNCH_CHECK("splitk_reduce_rows");
  return UIC_OK;
}

int uic_splitk_reduce_launch(const float* slab, int splitk, int M, int N, int col0, int ncols, float* C, int ldc, hipStream_t s,
                             int accumulate) {
  if (M == 0 || ncols == 0) return UIC_OK;
  if (N % 4 == 0 && ncols % 4 == 0 && col0 % 4 == 0 && ldc % 4 == 0 && ((uintptr_t)slab & 15) == 0 && ((uintptr_t)C & 15) == 0 && ((size_t)M * N) % 4 == 0) {
    const int bt = ncols / 4 >= 256 ? 256 : ((ncols / 4 + 63) / 64) * 64;
    hipLaunchKernelGGL(splitk_reduce_vec_kernel, dim3((unsigned)((ncols / 4 + bt - 1) / bt), (unsigned)(M > 65535 ? 65535 : M)), dim3(bt), 0, s,
                       slab, splitk, M, N, col0, ncols, C, ldc, accumulate);
    UIC_LAUNCH_CHECK("splitk_reduce_vec");
    return UIC_OK;
  }
  size_t g = ((size_t)M * ncols + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)g), dim3(256), 0, s, slab, splitk, M, N, col0, ncols, C, ldc, accumulate);
  UIC_LAUNCH_CHECK("splitk_reduce");
  return UIC_OK;
}

// ---- up to four destinations
namespace {
// blockIdx.y picks the destination (a uniform select: indexing an array of the by-value structs would put it in scratch)
__global__ void splitk_reduce_multi_kernel(const float* __restrict__ slab, int splitk, int M, int N, UicSlabDest d0, UicSlabDest d1,
                                           UicSlabDest d2, UicSlabDest d3, int accumulate) {
  const int k = blockIdx.y;
  float* const C = k == 0 ? d0.C : k == 1 ? d1.C : k == 2 ? d2.C : d3.C;
  const int ldc = k == 0 ? d0.ldc : k == 1 ? d1.ldc : k == 2 ? d2.ldc : d3.ldc;
  const int col0 = k == 0 ? d0.col0 : k == 1 ? d1.col0 : k == 2 ? d2.col0 : d3.col0;
  const int ncols = k == 0 ? d0.ncols : k == 1 ? d1.ncols : k == 2 ? d2.ncols : d3.ncols;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t total = (size_t)M * ncols;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int row = (int)(i / ncols), c = (int)(i - (size_t)row * ncols);
    const float* src = slab + (size_t)row * N + col0 + c;
    float v = 0.f;
    for (int z = 0; z < splitk; ++z) v += src[(size_t)z * M * N];
    float* o = C + (size_t)row * ldc + c;
    *o = accumulate ? *o + v : v;
  }
}

// the same, four columns per lane and the row from the grid (no division, 16-byte accesses): every extent and leading dimension
// a multiple of 4 and 16-byte aligned pointers
__global__ void splitk_reduce_multi_vec_kernel(const float* __restrict__ slab, int splitk, int M, int N, UicSlabDest d0, UicSlabDest d1,
                                               UicSlabDest d2, UicSlabDest d3, int accumulate) {
  const int k = blockIdx.y;
  float* const C = k == 0 ? d0.C : k == 1 ? d1.C : k == 2 ? d2.C : d3.C;
  const int ldc = k == 0 ? d0.ldc : k == 1 ? d1.ldc : k == 2 ? d2.ldc : d3.ldc;
  const int col0 = k == 0 ? d0.col0 : k == 1 ? d1.col0 : k == 2 ? d2.col0 : d3.col0;
  const int ncols = k == 0 ? d0.ncols : k == 1 ? d1.ncols : k == 2 ? d2.ncols : d3.ncols;
  const size_t MN = (size_t)M * N;
  if (ncols % 4 || col0 % 4 || ldc % 4 || ((size_t)C & 15)) {      // a destination that cannot take 16-byte accesses (a bias column): one column per lane
    const int c1 = blockIdx.x * blockDim.x + threadIdx.x;
    if (c1 >= ncols) return;
    for (int row = blockIdx.z; row < M; row += gridDim.z) {
      const float* src = slab + (size_t)row * N + col0 + c1;
      float v = 0.f;
      for (int z = 0; z < splitk; ++z) v += src[(size_t)z * MN];
      float* o = C + (size_t)row * ldc + c1;
      *o = accumulate ? *o + v : v;
    }
    return;
  }
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (c >= ncols) return;
  for (int row = blockIdx.z; row < M; row += gridDim.z) {
    const float* src = slab + (size_t)row * N + col0 + c;
    float4 v = *(const float4*)src;
    for (int z = 1; z < splitk; ++z) {
      const float4 w = *(const float4*)(src + (size_t)z * MN);
      v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
    }
    float4* o = (float4*)(C + (size_t)row * ldc + c);
    if (accumulate) { const float4 w = *o; v.x = w.x + v.x; v.y = w.y + v.y; v.z = w.z + v.z; v.w = w.w + v.w; }
    *o = v;
  }
}

}  // namespace

int uic_splitk_reduce_multi_launch(const float* slab, int splitk, int M, int N, const UicSlabDest* dst, int nd, int accumulate, hipStream_t s) {
  UIC_REQUIRE(nd >= 1 && nd <= 4, "splitk_reduce_multi: %d destinations", nd);
  UicSlabDest d[4] = {dst[0], dst[nd > 1 ? 1 : 0], dst[nd > 2 ? 2 : 0], dst[nd > 3 ? 3 : 0]};
  size_t cols = 0;
  for (int i = 0; i < nd; ++i) cols += dst[i].ncols;
  const bool vec = N % 4 == 0 && ((uintptr_t)slab & 15) == 0 && ((size_t)M * N) % 4 == 0;
  int maxt = 0;      // lanes a destination needs along its columns: ncols / 4, or ncols where it takes the one-column path
  for (int i = 0; i < nd; ++i) {
    const bool v4 = dst[i].ncols % 4 == 0 && dst[i].col0 % 4 == 0 && dst[i].ldc % 4 == 0 && ((uintptr_t)dst[i].C & 15) == 0;
    const int t = v4 ? dst[i].ncols / 4 : dst[i].ncols;
    maxt = t > maxt ? t : maxt;
  }
  if (vec && M > 0 && maxt > 0) {
    const int bt = maxt >= 256 ? 256 : ((maxt + 63) / 64) * 64;
    const unsigned gz = (unsigned)(M > 65535 ? 65535 : M);
    hipLaunchKernelGGL(splitk_reduce_multi_vec_kernel, dim3((unsigned)((maxt + bt - 1) / bt), (unsigned)nd, gz), dim3(bt), 0, s, slab, splitk, M, N,
                       d[0], d[1], d[2], d[3], accumulate);
    UIC_LAUNCH_CHECK("splitk_reduce_multi_vec");
    return UIC_OK;
  }
  size_t g = ((size_t)M * cols / nd + 255) / 256;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  hipLaunchKernelGGL(splitk_reduce_multi_kernel, dim3((unsigned)g, (unsigned)nd), dim3(256), 0, s, slab, splitk, M, N, d[0], d[1], d[2], d[3], accumulate);
  UIC_LAUNCH_CHECK("splitk_reduce_multi");
  return UIC_OK;
}
