// MFMA GEMM for gfx950:  C[M,N] = sum_seg A_s[M,K_s] * B_s[N,K_s]^T  (+ epilogue)
//
// Replaces the nn.Linear / nn.LSTMCell GEMM call sites of the reference hot path
// (P/models/AttModel.py:76-92 fc_embed/att_embed/logit/ctx2att, :426-427,434,441 the two
// LSTMCells, :543 h2att).  Both operands are K-contiguous ("NT"), which is how nn.Linear
// stores its weight; transposed weight/activation copies make every backward GEMM NT too.
//
//  * bf16 operands -> v_mfma_f32_32x32x16_bf16, f32 operands -> v_mfma_f32_32x32x2_f32
//    (exact-f32 MFMA, the parity path); accumulation is always f32.
//  * A block stages a [BM x 128 B] A tile and a [BN x 128 B] B tile per K step through LDS
//    (row stride 144 B => the 16-lane groups of ds_read_b128 hit 16 distinct 16-B slots).
//    Each lane half owns 64 contiguous bytes of the 128-B K slice, so fragments are plain
//    16-B LDS reads; the K order inside a tile is permuted identically for A and B.
//  * K segments: the concatenations torch.cat([prev_h, fc, xt]) / cat([att, h_att]) of
//    TopDownCore.forward (AttModel.py:432,438) are never materialised.
//  * LSTM mode: a wave owns the 4 gates (i,f,g,o) of 32 hidden units for 32 rows in four
//    32x32 accumulators with identical lane layout, so the cell update
//    c' = s(f) c + s(i) tanh(g), h' = s(o) tanh(c') runs in the epilogue on registers.
//
// This file is the host side of the NT family: uic_gemm_launch checks the arguments, gemm::choose names the kernel and a switch
// launches it.  The kernels: gemm_skinny.hip (uic_gemm_kernel: register-staged tiles, in-block K split, LSTM epilogue),
// gemm_glds.hip (uic_gemm_glds_kernel: 128 x 128 LDS-DMA tile), gemm_pp.hip (uic_gemm_pp_kernel: 256-column ping-pong tile);
// splitk_reduce.hip sums the slabs of a split-K launch.
#include "gemm_internal.h"

namespace {

// Where the ping-pong kernel (gemm_pp.hip) is the faster of the two large-GEMM kernels.  It holds one workgroup per CU, so it needs
// enough tiles of its best height (uic_gemm_pp_rows) to cover most of the 256 CUs; measured (profiles/r04_*_gemm_headroom.txt,
// us, 128 x 128 kernel -> ping-pong): att_embed 23040 x 512 x 2048 66 -> 47.5 (192 rows), ctx2att 23040 x 512 x 512 29 -> 23,
// Gx 10880 x 2048 x 1024 70 -> 57, d xt 10880 x 512 x 2048 42 -> 32 (128 rows), logit chunk 2560 x 9488 x 512 50 -> 49; the
// BPTT loop's 640-row GEMMs (18-36 tiles) lose 2-3x and stay on the 128 x 128 / skinny kernels.
inline bool uic_gemm_pp_wins(const UicGemmParams& p) {
  if (!uic_gemm_pp_eligible(p) || p.seg[0].K < 512) return false;
  const int rows = uic_gemm_pp_rows(p.M, p.N, 256, p.seg[0].K / (p.splitk > 1 ? p.splitk : 1));
  const long tiles = (long)((p.M + rows - 1) / rows) * ((p.N + 255) / 256) * (p.splitk > 1 ? p.splitk : 1);
  return tiles >= 160;
}

// one K segment of whole LDS-DMA rounds (128 bytes): what the 128 x 128 LDS-DMA kernel needs
bool glds_ok(const UicGemmParams& p) { return p.nseg == 1 && p.seg[0].K % (128 / (int)uic_dtype_size(p.dtype)) == 0; }

}  // namespace

namespace gemm {

enum Kernel { SKINNY, GLDS, PP };
struct Choice {
  Kernel kernel;
  int pp_rows;     // PP: the tile height, 256 / 192 / 128 (0 = uic_gemm_pp_rows' choice)
};

// The kernel of a problem, one rule per line, first match.  Launches nothing and refuses nothing: what a kernel cannot take is
// refused where it is launched (launch_chosen, uic_gemm_pp_launch).
Choice choose(const UicGemmParams& p) {
  // the LSTM epilogues exist in the skinny kernel only
  if (p.lstm) return {SKINNY, 0};
  // must go to the ping-pong kernel: it alone rounds an f32 A operand and has the fused backward-of-ReLU epilogue (callers test
  // uic_gemm_pp_eligible first)
  if (p.a_f32 || p.acc_src || p.mask_act) return {PP, 0};
  // told to, with the tile height
  if (p.flags & UIC_GEMM_FORCE_256) return {PP, 256};
  if (p.flags & UIC_GEMM_FORCE_192) return {PP, 192};
  if (p.flags & UIC_GEMM_FORCE_PP128) return {PP, 128};
  // may go there: where it is the faster one (the row-mapped slab store exists in the LDS-DMA kernel only)
  if (!(p.flags & UIC_GEMM_FORCE_128) && !p.slab_row_map && uic_gemm_pp_wins(p)) return {PP, 0};
  // raw split-K partial tiles: the LDS-DMA kernel
  if (p.slab) return {GLDS, 0};
  // throughput problems it is eligible for (it has no pre-dropout copy); the skinny launcher takes the others, large or small
  if (many_tiles(p) && glds_ok(p) && !p.C_pre) return {GLDS, 0};
  return {SKINNY, 0};
}

}  // namespace gemm

namespace {

int launch_chosen(const UicGemmParams& p, gemm::Choice c, hipStream_t s) {
  const bool bf16 = p.dtype == UIC_BF16;
  switch (c.kernel) {
    case gemm::PP:
      if (p.a_f32)
        UIC_REQUIRE(bf16 && uic_gemm_pp_eligible(p), "gemm: an f32 A operand needs the ping-pong kernel (bf16, one K segment of whole 128-element rounds, < 4 GB)");
      else if (p.acc_src || p.mask_act)
        UIC_REQUIRE(bf16 && !p.slab && uic_gemm_pp_eligible(p), "gemm: acc_src / mask_act need the ping-pong kernel (bf16, one K segment of whole 128-element rounds)");
      return uic_gemm_pp_launch(p, c.pp_rows, s);
    case gemm::GLDS:
      if (p.slab) {
        UIC_REQUIRE(glds_ok(p) && !p.lstm, "gemm: slab output needs one K segment that is a multiple of 128 bytes");
        UIC_REQUIRE(!p.slab_row_map || (bf16 && p.slab_rows >= p.M && (size_t)p.slab_rows * (size_t)p.N < ((size_t)1 << 31)),
                    "gemm: slab_row_map needs bf16, slab_rows=%d >= M=%d and a slab slice below 2^31 elements", p.slab_rows, p.M);
      }
      return gemm::glds_launch(p, s);
    default:
      return gemm::skinny_launch(p, s);
  }
}

// second output e^{2 C}: the ping-pong kernel's epilogue, or one element-wise pass behind any other kernel
int launch_with_exp2(const UicGemmParams& p, hipStream_t s) {
  UIC_REQUIRE(p.dtype == UIC_BF16 && !(p.flags & UIC_GEMM_OUT_F32) && p.C && p.ldc == p.N && ((size_t)p.M * p.N) % 8 == 0 && !p.slab,
              "gemm: C_exp2 needs a contiguous bf16 output");
  const gemm::Choice c = gemm::choose(p);
  if (c.kernel == gemm::PP && uic_gemm_pp_eligible(p)) return launch_chosen(p, c, s);
  UicGemmParams q = p;
  q.C_exp2 = nullptr;
  UIC_TRY(launch_chosen(q, gemm::choose(q), s));
  return uic_exp2x2_launch(p.C, p.C_exp2, (size_t)p.M * p.N, s);
}

}  // namespace

bool uic_gemm_glds_eligible(int dtype, int K) { return K > 0 && K % (dtype == UIC_BF16 ? 64 : 32) == 0; }

int uic_gemm_launch(const UicGemmParams& p, hipStream_t s) {
  UIC_REQUIRE(p.dtype == UIC_F32 || p.dtype == UIC_BF16, "gemm: bad dtype %d", p.dtype);
  UIC_REQUIRE(p.M >= 0 && p.N >= 0, "gemm: negative size");
  UIC_REQUIRE(p.nseg >= 1 && p.nseg <= UIC_GEMM_MAX_SEG, "gemm: nseg %d out of range", p.nseg);
  const int vec = p.dtype == UIC_BF16 ? 8 : 4;
  for (int i = 0; i < p.nseg; ++i) {
    const UicGemmSeg& g = p.seg[i];
    UIC_REQUIRE(g.A && g.B, "gemm: null operand in segment %d", i);
    // (an f32 A operand of the bf16 ping-pong kernel -- uic_linear_f32a -- is read in 16-byte pieces of FOUR floats: lda % 4)
    const int veca = p.a_f32 ? 4 : vec;
    UIC_REQUIRE(g.K > 0 && g.K % vec == 0 && g.lda % veca == 0 && g.ldb % vec == 0,
                "gemm: segment %d K=%d lda=%d ldb=%d must be multiples of %d elements (lda: %d)", i, g.K, g.lda, g.ldb, vec, veca);
    UIC_REQUIRE(((uintptr_t)g.A & 15) == 0 && ((uintptr_t)g.B & 15) == 0, "gemm: segment %d operands must be 16-byte aligned", i);
  }
  if (p.lstm) {
    UIC_REQUIRE(p.H > 0 && p.N == (p.lstm == 2 ? 5 : 4) * p.H, "gemm(lstm): N=%d must equal %d*H (H=%d)", p.N, p.lstm == 2 ? 5 : 4, p.H);
    UIC_REQUIRE(p.c_out && p.h_out, "gemm(lstm): c_out and h_out are required");
  } else {
    UIC_REQUIRE(p.C != nullptr || p.slab != nullptr, "gemm: null C");
  }
  if (p.M == 0 || p.N == 0) return UIC_OK;
  if (p.C_exp2 && !p.lstm) return launch_with_exp2(p, s);
  return launch_chosen(p, gemm::choose(p), s);
}
