// Host-side helpers shared by the launchers and the model-level sequencers (topdown_*.hip, fcmodel.hip, nmt_*.hip).
#pragma once
#include "uic_common.h"
#include <string.h>

// one launch per operand dtype
#define UIC_DISPATCH_T(dtype, CALL_BF16, CALL_F32) \
  do {                                             \
    if ((dtype) == UIC_BF16) { CALL_BF16; } else { CALL_F32; } \
  } while (0)

namespace {

// workgroups of a grid-stride kernel: n elements, per_block of them per workgroup and trip
inline int uic_grid_for(size_t n, int per_block) {
  size_t g = (n + per_block - 1) / per_block;
  if (g > 65536) g = 65536;   // grid-stride beyond that
  if (g == 0) g = 1;
  return (int)g;
}

// bump allocator over a caller-provided arena (base == nullptr: size query)
struct Bump {
  char* base;
  size_t off;
  void* take(size_t bytes) {
    off = (off + 255) & ~(size_t)255;
    void* p = base ? base + off : nullptr;
    off += bytes;
    return p;
  }
};

inline size_t rup8(size_t x) { return (x + 7) & ~(size_t)7; }
// padded vocabulary width (leading dimension of logits / dlogits): a multiple of 64 for real vocabularies so the
// K = V1 backward GEMM runs on the 128-byte-round LDS-DMA path, a multiple of 8 for toy sizes
inline size_t vpad(size_t v1) { return v1 >= 1024 ? (v1 + 63) & ~(size_t)63 : rup8(v1); }

inline const char* off(const void* p, size_t elems, int dtype) { return (const char*)p + elems * uic_dtype_size(dtype); }
inline char* offw(void* p, size_t elems, int dtype) { return (char*)p + elems * uic_dtype_size(dtype); }

inline UicGemmParams gemm_base(int dtype, int M, int N) {
  UicGemmParams g;
  memset(&g, 0, sizeof(g));
  g.dtype = dtype; g.M = M; g.N = N;
  return g;
}
inline void add_seg(UicGemmParams& g, const void* A, int lda, const void* B, int ldb, int K) {
  UicGemmSeg& s = g.seg[g.nseg++];
  s.A = A; s.B = B; s.K = K; s.lda = lda; s.ldb = ldb;
}

}  // namespace
