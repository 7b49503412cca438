// Weight-gradient dispatch (host code only): which GEMM kernel and which split over K a weight gradient gets, and the launches
// of that choice.  Every call first makes a WgPlan -- a function of the shape, the number of destinations, the slab's size, `how`,
// `at` and the kernels' *_eligible predicates, nothing else -- and then executes it.  Declared in uic_common.h.
#include "uic_host.h"

namespace {

enum WgPath {
  WG_NOT_ELIGIBLE,   // wgrad_tn: the caller transposes and uses wgrad_multi
  WG_REFUSED_256,    // wgrad_tn: UIC_TN_FORCE_256 on a problem the 256 x 256 kernel does not take (an error)
  WG_TNPP_256,       // the 256 x 256 ping-pong TN kernel (gemm_tn_pp.hip)
  WG_TN_128,         // the 128 x 128 TN kernel (gemm_tn.hip)
  WG_NT_SPLITK,      // the LDS-DMA NT GEMM split over K, deterministic slab reduction
  WG_NT_DIRECT,      // one NT GEMM per destination
};
struct WgPlan {
  WgPath path;
  int splitk;        // K slices of the launch
  bool direct;       // the GEMM's epilogue writes the destinations itself: no slab, no reduction launch
};

WgPlan plan_nt(int dt, int lrows, int rrows, int K, int nd, bool accumulate, size_t slab_bytes, UicWgPlace at) {
  const long blocks = (long)((lrows + 127) / 128) * ((rrows + 127) / 128);
  if (uic_gemm_glds_eligible(dt, K) && lrows >= 128 && rrows >= 128) {
    const int nt = K / (dt == UIC_BF16 ? 64 : 32);
    int sk = (int)((384 + blocks - 1) / blocks);
    if (sk > 8) sk = 8;
    if (sk > nt / 4) sk = nt / 4 > 0 ? nt / 4 : 1;
    // alone on the chip with a long reduction (the NMT generator's d out: 64 tiles x 782 rounds): one workgroup per CU, so that the
    // launch takes the 128 x 128 kernel's three-buffer ring (a K round then costs 0.3 us instead of 0.8: 87 -> 65 us)
    if (at == UIC_WG_ALONE && blocks <= 128 && nt >= 128) {
      int one_per_cu = (int)(256 / blocks);
      if (one_per_cu > 8) one_per_cu = 8;
      if (one_per_cu >= 2 && nt / one_per_cu >= 32) sk = one_per_cu;
    }
    while (sk > 1 && (size_t)sk * lrows * rrows * 4 > slab_bytes) --sk;
    if ((size_t)sk * lrows * rrows * 4 <= slab_bytes && (sk > 1 || nd > 1 || accumulate)) return {WG_NT_SPLITK, sk, false};
  }
  return {WG_NT_DIRECT, 1, true};
}

// K slices of a 256 x 256 launch.  Cost model fitted to tools/tn_bench.py (profiles/r05_*_tn_bench.txt): one workgroup per CU,
// so ceil(workgroups / 256) rounds of (K tiles per slice x 1.05 us + 8 us), plus the slab traffic of a split launch (partials
// written, read back, destination written) at 4 TB/s.  Slices hold a whole, even number of K tiles.
double tnpp_cost_us(long tiles, int nt, int sk, size_t out_bytes) {
  const long wgs = tiles * sk;
  const double body = (double)((wgs + 255) / 256) * ((double)(nt / sk) * 1.05 + 8.0);
  const double slab = sk > 1 ? ((double)out_bytes * (2.0 * sk + 1.0)) / 4.0e6 + 3.0 : (double)out_bytes / 4.0e6;
  return body + slab;
}
int tnpp_splitk(long tiles, int nt, size_t out_bytes, size_t slab_bytes, bool beside) {
  int best = 1;
  if (beside) {
    // as few workgroups as the problem has tiles; split only a problem of a handful of tiles, until ~24 CUs work on it
    if (tiles >= 24) return 1;
    for (int sk = 2; sk <= 64; ++sk) {
      if (nt % (2 * sk) != 0 || nt / sk < 4) continue;
      if ((size_t)sk * out_bytes > slab_bytes) break;
      best = sk;
      if (tiles * sk >= 24) break;
    }
    return best;
  }
  double best_cost = tnpp_cost_us(tiles, nt, 1, out_bytes);
  for (int sk = 2; sk <= 64; ++sk) {
    if (nt % (2 * sk) != 0 || nt / sk < 4) continue;
    if ((size_t)sk * out_bytes > slab_bytes || tiles * sk > 1024) break;
    const double c = tnpp_cost_us(tiles, nt, sk, out_bytes);
    if (c < best_cost) { best_cost = c; best = sk; }
  }
  return best;
}

void set_dst(UicGemmTnParams& p, const WDest* dst, int nd, bool accumulate) {
  p.ndst = nd; p.accumulate = accumulate ? 1 : 0;
  for (int i = 0; i < nd; ++i) { p.dst[i].C = dst[i].C; p.dst[i].ldc = dst[i].ldc; p.dst[i].col0 = dst[i].col0; p.dst[i].ncols = dst[i].ncols; }
}

// Two TN kernels.  The 256 x 256 ping-pong form takes every problem with whole pairs of K tiles and >= 1024 reduction rows: it
// needs a quarter of the 128 x 128 kernel's workgroups for the same flops and half its LDS traffic.  How many workgroups a
// launch should have depends on where it runs (`at`, passed by the caller):
//   * beside the BPTT chain (CU-time-bound window): as FEW workgroups as the problem has 256 x 256 tiles -- the chain's kernels
//     need the other CUs --, split over K only until ~48 CUs work on it;
//   * alone on the chip (the step's tail, every stand-alone call): split over K until one workgroup per CU, slices of >= 4 K tiles.
// p: operands, shape and slab of the problem (uic_gemm_tn_eligible).
WgPlan plan_tn(const UicGemmTnParams& p, const WDest* dst, int nd, bool accumulate, size_t slab_bytes, int how, UicWgPlace at) {
  const int lrows = p.M, rrows = p.N, K = p.K, nt = K / 64;
  const int sk_forced = (how >> 16) & 0xff;
  const size_t out_bytes = (size_t)lrows * rrows * 4;
  if (!(how & UIC_TN_FORCE_128)) {
    const bool beside = at != UIC_WG_ALONE;
    const long t256 = (long)((lrows + 255) / 256) * ((rrows + 255) / 256);
    const int sk = sk_forced ? sk_forced : tnpp_splitk(t256, nt, out_bytes, slab_bytes, beside);
    // beside the BPTT chain every problem with a real K loop; alone on the chip the 128 x 128 kernel's many small workgroups
    // finish a small problem sooner (tools/tn_bench.py: LSTM chunk 31 vs 45 us, ctx2att 36 vs 45; logit 181 vs 146, att_embed 79 vs 70)
    bool wanted = (how & UIC_TN_FORCE_256) || (lrows >= 256 && (beside ? K >= 1024 : 2.0 * lrows * rrows * K >= 3.0e10));
    if (at == UIC_WG_BESIDE_TN128 && !(how & UIC_TN_FORCE_256) && K <= 8192) wanted = false;
    const bool direct = sk == 1 && nd <= UIC_GEMM_TN_MAX_SEG;
    UicGemmTnParams q = p;
    q.splitk = sk;
    if (direct) set_dst(q, dst, nd, accumulate);
    if (wanted && (direct || (size_t)sk * out_bytes <= slab_bytes) && uic_gemm_tnpp_eligible(q)) return {WG_TNPP_256, sk, direct};
    if (how & UIC_TN_FORCE_256) return {WG_REFUSED_256, sk, direct};
  }
  const long blocks = (long)((lrows + 127) / 128) * ((rrows + 127) / 128);
  int sk = blocks >= 160 ? 1 : (int)((384 + blocks - 1) / blocks);   // >= 160 tiles fill the 256 CUs well enough: no slab pass
  if (sk > 8) sk = 8;
  if (sk > nt / 4) sk = nt / 4 > 0 ? nt / 4 : 1;
  if (sk_forced) sk = sk_forced;
  while (sk > 1 && (size_t)sk * out_bytes > slab_bytes) --sk;
  const bool direct = sk == 1 && nd <= UIC_GEMM_TN_MAX_SEG;
  if (!direct && (size_t)sk * out_bytes > slab_bytes) return {WG_NOT_ELIGIBLE, sk, false};
  return {WG_TN_128, sk, direct};
}

}  // namespace

int wgrad_multi(float* slab, size_t slab_bytes, int dt, const void* left, int lrows, const void* right, int rrows, int K,
                const WDest* dst, int nd, hipStream_t s, bool accumulate, WRows* rows, UicWgPlace at) {
  if (rows) rows->used = false;
  const WgPlan plan = plan_nt(dt, lrows, rrows, K, nd, accumulate, slab_bytes, at);
  if (plan.path == WG_NT_SPLITK) {
    const int sk = plan.splitk;
    UicGemmParams g = gemm_base(dt, lrows, rrows);
    add_seg(g, left, K, right, K, K);
    g.splitk = sk; g.slab = slab;
    UIC_TRY(uic_gemm_launch(g, s));
    if (rows && nd == 1 && !accumulate && dst[0].col0 == 0 && dst[0].ncols == rrows && rows->n <= lrows &&
        uic_splitk_reduce_rows_ok(slab, lrows, rrows, rows->C, rows->ldc)) {
      rows->used = true;
      return uic_splitk_reduce_rows_launch(slab, sk, lrows, rrows, rows->map, rows->n, rows->limit, rows->C, rows->ldc, s);
    }
    for (int i = 0; i < nd; ++i)
      UIC_TRY(uic_splitk_reduce_launch(slab, sk, lrows, rrows, dst[i].col0, dst[i].ncols, dst[i].C, dst[i].ldc, s, accumulate ? 1 : 0));
    return UIC_OK;
  }
  for (int i = 0; i < nd; ++i) {
    UicGemmParams g = gemm_base(dt, lrows, dst[i].ncols);
    add_seg(g, left, K, (const char*)right + (size_t)dst[i].col0 * K * uic_dtype_size(dt), K, K);
    g.C = dst[i].C; g.ldc = dst[i].ldc; g.flags = UIC_GEMM_OUT_F32 | (accumulate ? UIC_GEMM_ACCUM : 0);
    UIC_TRY(uic_gemm_launch(g, s));
  }
  return UIC_OK;
}

int wgrad_tn(float* slab, size_t slab_bytes, int dt, const void* A, int lda, int lrows, const UicGemmTnSeg* segs, int nseg,
             int K, const WDest* dst, int nd, hipStream_t s, bool accumulate, bool* done, int how, UicWgPlace at) {
  *done = false;
  if (dt != UIC_BF16 || nseg > UIC_GEMM_TN_MAX_SEG) return UIC_OK;
  UicGemmTnParams p;
  memset(&p, 0, sizeof(p));
  p.A = A; p.lda = lda; p.M = lrows; p.K = K; p.nseg = nseg;
  int rrows = 0;
  for (int i = 0; i < nseg; ++i) { p.seg[i] = segs[i]; rrows += segs[i].ncols; }
  p.N = rrows;
  if (!uic_gemm_tn_eligible(p)) return UIC_OK;
  p.slab = slab;
  const WgPlan plan = plan_tn(p, dst, nd, accumulate, slab_bytes, how, at);
  UIC_REQUIRE(plan.path != WG_REFUSED_256, "wgrad_tn: M=%d N=%d K=%d splitk=%d is not a problem of the 256 x 256 kernel (K %% (128 splitk), slab of %zu bytes)",
              lrows, rrows, K, plan.splitk, slab_bytes);
  if (plan.path == WG_NOT_ELIGIBLE) return UIC_OK;
  p.splitk = plan.splitk;
  if (plan.direct) set_dst(p, dst, nd, accumulate);
  if (plan.path == WG_TNPP_256) UIC_TRY(uic_gemm_tnpp_launch(p, s));
  else UIC_TRY(uic_gemm_tn_launch(p, s, at));
  if (!plan.direct) {
    UicSlabDest sd[4];
    for (int i0 = 0; i0 < nd; i0 += 4) {
      const int n = nd - i0 < 4 ? nd - i0 : 4;
      for (int i = 0; i < n; ++i) sd[i] = UicSlabDest{dst[i0 + i].C, dst[i0 + i].ldc, dst[i0 + i].col0, dst[i0 + i].ncols};
      UIC_TRY(uic_splitk_reduce_multi_launch(slab, plan.splitk, lrows, rrows, sd, n, accumulate ? 1 : 0, s));
    }
  }
  *done = true;
  return UIC_OK;
}

int wgrad_group(float* slab, size_t slab_bytes, int dt, const void* A, int lda, int lrows, const UicGemmTnSeg* segs, int nseg,
                int rows, const WDest* dst, int nd, hipStream_t s, bool accumulate, void* tA, void* tB, UicWgPlace at) {
  bool done = false;
  UIC_TRY(wgrad_tn(slab, slab_bytes, dt, A, lda, lrows, segs, nseg, rows, dst, nd, s, accumulate, &done, 0, at));
  if (done) return UIC_OK;
  const int Kp = (int)rup8(rows);
  UIC_TRY(uic_transpose_launch(dt, A, rows, lrows, lda, tA, Kp, s));
  int col = 0;
  for (int i = 0; i < nseg; ++i) {
    UIC_TRY(uic_transpose_launch(dt, segs[i].B, rows, segs[i].ncols, segs[i].ldb, offw(tB, (size_t)col * Kp, dt), Kp, s));
    col += segs[i].ncols;
  }
  return wgrad_multi(slab, slab_bytes, dt, tA, lrows, tB, col, Kp, dst, nd, s, accumulate, nullptr, at);
}
