// Shared by the GEMM family (gemm.hip, gemm_skinny.hip, gemm_glds.hip, gemm_pp.hip, gemm_tn.hip, gemm_tn_pp.hip): the launchers
// behind uic_gemm_launch's dispatch, and the one copy of every tile rule that more than one of the kernels follows.  No host state.
#pragma once
#include "uic_common.h"
#include <type_traits>

namespace gemm {

// ---- one launcher per NT kernel (gemm_skinny.hip, gemm_glds.hip; the ping-pong kernel's is uic_gemm_pp_launch), each with its
// own dtype dispatch, dynamic-LDS attribute and launch check
int skinny_launch(const UicGemmParams& p, hipStream_t s);
int glds_launch(const UicGemmParams& p, hipStream_t s);

// a problem of at least 200 tiles of 128 x 128: the throughput kernels (the LDS-DMA kernel, or the 128 x 128 register-staged tile
// where that one is not eligible) instead of the 64-row in-block K split
inline bool many_tiles(const UicGemmParams& p) { return (long)((p.M + 127) / 128) * ((p.N + 127) / 128) >= 200; }

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

// C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
__device__ __forceinline__ int c32_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

// XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs (each with a private 4 MB L2), so workgroup `lin` of
// `nblk` takes position xcd_run() of a tile order in which every XCD owns one contiguous run.  (bijective for any grid)
__device__ __forceinline__ int xcd_run(int lin, int nblk) {
  const int q = nblk >> 3, r = nblk & 7, xcd = lin & 7, idx = lin >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// grouped order inside a run: position lp of a gx x gy grid advances over GM = 8 row tiles before moving to the next column
// tile, so one XCD's L2 holds an 8-tile A band while B tiles stream through once per band
__device__ __forceinline__ void grouped_tile(int lp, int gx, int gy, int& bm, int& bn) {
  constexpr int GM = 8;
  const int width = GM * gy;
  const int first = (lp / width) * GM;
  const int gsz = min(gx - first, GM);
  const int rem = lp % width;
  bm = first + rem % gsz;
  bn = rem / gsz;
}

// K rounds [kt0, kt0 + nt) of slice z of a split-K launch, from all nt of them: ceil(nt / splitk) each, the last ones fewer or
// none.  (The ping-pong kernels take exactly nt / splitk, checked by their launchers, and keep that form written out: as a
// function it changed every instruction stream of uic_gemm_pp_kernel.)
__device__ __forceinline__ void splitk_slice(int splitk, int z, int& kt0, int& nt) {
  if (splitk > 1) {
    const int tps = (nt + splitk - 1) / splitk;
    kt0 = z * tps;
    nt = max(0, min(nt - kt0, tps));
  }
}

// one LDS-DMA wave instruction (global_load_lds_dwordx4): 16 bytes per lane from `src`, written lane-linearly from `lds` on
__device__ __forceinline__ void dma16(const void* src, void* lds) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)lds, 16, 0, 0);
}

}  // namespace gemm
