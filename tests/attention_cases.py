"""Cases, float64 references, per-element bounds and the launchers' kernel choice for the additive attention (csrc/attention.hip: nine
kernels behind uic_attention_fwd_strided, uic_attention_bwd_step_sources and uic_attention_bwd_accum_strided) -- shared by
tests/test_attention_cases_host.py (the list reaches every kernel and both sides of every condition; a float32 restatement of the
kernels' formulas stays inside a quarter of the bound) and tests/test_gpu_attention.py (the kernels themselves).  No GPU, no torch.

References, float64, on the operands AS STORED (p_att and att rounded to bf16 where the call is bf16):
    forward  e_r = w . tanh(p_r + h) + b;  s = softmax_R(e);  alpha_r = s_r m_r / sum_j s_j m_j;  ctx = sum_r alpha_r att_r
    step     dctx = slab_0 + slab_1 + ... (in order);  da_r = dctx . att_r;  de_r = alpha_r (da_r - sum_j alpha_j da_j);
             d_att_h[a] = w_a sum_r de_r (1 - tanh^2(p_ra + h_a));   rows with step >= row_len[n]: zeros
    accum    d_att[r] = sum_{t<TS} alpha_t[r] dctx_t;  d_p_att[r,a] = w_a sum_{t<TS} de_t[r] (1 - tanh^2(p_ra + h_ta));
             part[a] = sum_{t<TS,r} de_t[r] tanh(p_ra + h_ta);  part[A] = sum_{t<TS,r} de_t[r];  TS = min(T, max(row_len[n], 0))

Bounds: per element, u = 2^-24 times (a count of roundings) times (the sum of the magnitudes of the terms that enter the element),
floor 2^-126 (smaller results may be flushed), plus 2^-8 |ref| where the result is stored in bf16.  The count is not one constant C
chosen in advance: it is written out below per output, one unit per rounding of relative size u on a quantity no larger than the
magnitude sum, a serial chain of n additions counting n.  The cancelling factor 1 - tanh^2 counts as 1 (near saturation its
ABSOLUTE error survives), tanh as 1.

  tanh(p + h)                      C_TANH = 8: the sum p + h (its error times 1 - tanh^2 <= 0.45 |x| u ... 1), then on the bf16 path
                                   1 - 2 rcp(1 + exp2(k x)): the product k x (1), v_exp_f32 (1 ulp = 2), + 1 (1), v_rcp_f32 (2), 1 - 2 rc (1);
                                   tanhf of the f32 path (<= 2 ulp) is covered by the same 8
  1 - tanh^2                       counting gives 2 C_TANH + 2 = 18 (the square doubles the error of tanh, + its rounding, + the subtraction),
                                   nearly met where tanh -> -1 (rc -> 1: the roundings of 1 + e, rcp and 1 - 2 rc all survive); the float32
                                   restatement reaches 5.8 units there on a one-step row, so C_G = 24 keeps it inside a quarter
  factored form (bf16 accum)       rc = 1 / (1 + e^{2p} e^{2h}), 1 - tanh^2 = 4 (rc - rc^2), tanh = 1 - 2 rc.  The arguments 2p k and 2h k
                                   are rounded SEPARATELY: relative error (|2p| + |2h|) u in e^{2p} e^{2h}, which moves 1 - tanh^2 by
                                   |tanh (1 - tanh^2)| <= 0.385 times that and tanh by (1 - tanh^2) / 2 times that: ARG = 0.77 (|p| + |h|)
                                   for 1 - tanh^2 and |p| + |h| for tanh, per element (up to 31 / 40 at |2p| = |2h| = 40).  Then 26, C_GF = 32 as for C_G:
                                   two exp2 and the fma (5 x 0.385 ... 2), the SHARED reciprocal of the PART 2 kernel -- x0 x1 (1), rcp (2),
                                   times x1 (1), each acting on rc, where d(4 rc (1 - rc)) <= 4 d rc ... 16 -- and rc^2, rc - rc^2 (2 x 4 = 8)
  a dot product over n elements    chain(n) = vec ceil(n / (64 vec)) + 6: a lane's serial chain, then the six levels across the wave
  forward score e                  U_E = C_TANH + 1 (w tanh) + chain(A) + 1 (b):  |d e| <= U_E u (sum |w_a| + |b|) = DE
  forward exp(e_r - max)           relative REL1_r = DE + 3 u |e_r - max| + 2 u (the subtraction and, on the bf16 path, the product with
                                   log2 e scale with the argument; exp itself 2)
  alpha_r                          relative REL1_r + sum_j alpha_j REL1_j (the denominator) + (2 R + 8) u (two serial sums over R, the
                                   reciprocal or division twice, the products);  exact 0 where the mask is 0
  ctx[h]                           sum_r tol(alpha_r) |att_rh| + (1 + 9 ceil(R / 36) + 12) u sum_r alpha_r |att_rh|  (a wave's regions, up to 12 waves)
  step dctx[h]                     4 nslab u sum_z |slab_z[h]|  (sums of two or three terms MEET their worst case, so the count carries the
                                   factor 4 that the restatement test leaves);  dctx_sum moreover equals the sequential float32 sum bit for bit
  step da_r                        sum_h tol(dctx_h) |att_rh| + (1 + chain(H)) u sum_h |dctx_h att_rh|
  step de_r                        alpha_r (tol(da_r) + tol(wbar) + 2 u (|da_r| + |wbar|)),  tol(wbar) = sum_j alpha_j tol(da_j) + (1 + R) u sum_j alpha_j |da_j|
  step d_att_h[a]                  |w_a| (sum_r tol(de_r) + (C_G + 9 ceil(R / 36) + 4 + 2) u sum_r |de_r|)
  accum d_att[r,h]                 (4 TS + 4) u sum_t |alpha_t[r] dctx_t[h]|  (a product and an addition a step in the first form; doubled, see dctx)
  accum d_p_att[r,a]               |w_a| u sum_t |de_t[r]| (G + K TS + 2):  f32  G = C_G, K = 3 (de g, the accumulation);  bf16  G = C_GF + ARG,
                                   K = 24: S1 = sum de rc and S2 = sum de rc^2 are subtracted AFTER the sums, 3 roundings a step, times 4 -- and on rows
                                   of two or three steps the restatement comes within half of that worst case, hence doubled (see dctx)
  accum part[a]                    u sum_{t,r} |de_t[r]| (TH + TS ceil(R / 4) + 2 (TS + ceil(R / 4) + 5) + 12):  TH = C_TANH (f32), C_TANH + ARG
                                   (bf16);  a wave's serial chain over its regions and steps (first form), or sum de - 2 sum S1 (round 6)
  accum part[A]                    (TS R + 8) u sum |de|  (one thread's serial loop in the first form)
The float32 restatement (restated_f32: correctly rounded tanh, the exp2 / reciprocal form, the factored form with both limits and the
shared reciprocal) stays below a quarter of these on every case; tests/test_attention_cases_host.py holds that and records the maxima.

Every operand is a view into a larger buffer of NaN canaries (layout()); rows behind a caption's end hold NaN as well.
"""
import functools
import zlib

import numpy as np

F32, BF16 = 0, 1
EPS = 2.0 ** -24
TINY = 2.0 ** -126
PAD = 64                                    # canary elements in front of and behind every view (a multiple of 16 bytes)
GENERIC, FAST, FAST_FULL = 0, 1, 2          # UIC_ATTN_*
P1_R6, P2_R6 = 1, 2                         # UIC_ATTN_ACCUM_* bits
FAST_R = 36                                 # regions the fast kernels cover
P1_TCH, P1_RU = 6, 9
EXP_LIM, P2_LIM = 40.0, 21.5                # |2p|, |2h| up to which attn_bwd_accum_kernel<bf16, 2> / the round-6 PART 2 kernel factor
LDS_MAX, LDS_DEFAULT = 160 * 1024, 64 * 1024
C_TANH, C_G, C_GF = 8.0, 24.0, 32.0
LOG2E2 = np.float32(2.8853900817779268)
DT_NAMES = ("f32", "bf16")
OPS = ("fwd", "step", "accum")
OP_NAMES = {"fwd": "attention_fwd", "step": "attention_bwd_step", "accum": "attention_bwd_accum"}     # what the error text names


def vec(dt):
    return 8 if dt == BF16 else 4


def round_bf16(x):
    """float32 values that bf16 holds exactly (round to nearest even; finite inputs)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def round_to(x, dt):
    return round_bf16(x) if dt == BF16 else np.asarray(x, dtype=np.float32)


class Case:
    """One call.  A and H are given in 16-byte chunks (Av, Hv: the same case sits at the same edge in both dtypes) or in elements."""

    def __init__(self, name, op, N=3, R=5, Av=2, Hv=3, A=None, H=None, T=1, mask=None, ld_mask=0, ld_ctx=(1, 0), lddctx=(1, 0), col=0,
                 nslab=0, stride_extra=0, dsum=False, ld_sum=(3, 0), row_len=None, step=2, shift=None, values="normal", bias=True,
                 poison=False, dtypes=(F32, BF16), data=None):
        assert op in OPS
        self.name, self.op, self.N, self.R, self.T = name, op, N, R, T
        self._A, self._H, self.Av, self.Hv = A, H, Av, Hv
        self.mask, self.ld_mask_extra, self._ld_ctx, self._lddctx, self.col = mask, ld_mask, ld_ctx, lddctx, col
        self.nslab, self.stride_extra, self.dsum, self._ld_sum = nslab, stride_extra, dsum, ld_sum
        self.row_len, self.step = None if row_len is None else tuple(row_len), step
        self.shift = dict(shift or {})                                      # tensor -> bytes off 16-byte alignment
        self.values, self.bias, self.poison, self.dtypes = values, bias, poison, tuple(dtypes)
        self.seed = zlib.crc32((data or name).encode()) % (2 ** 31)         # (two cases with the same `data` hold the same numbers)
        assert row_len is None or len(row_len) == N

    def A(self, dt):
        return self._A if self._A is not None else self.Av * vec(dt)

    def H(self, dt):
        return self._H if self._H is not None else self.Hv * vec(dt)

    def _ld(self, l, dt):
        return l[0] * self.H(dt) + l[1]

    def ld_ctx(self, dt):
        return self._ld(self._ld_ctx, dt)

    def lddctx(self, dt):
        return self._ld(self._lddctx, dt)

    def ld_sum(self, dt):
        return self._ld(self._ld_sum, dt)

    def ld_mask(self):
        return self.R + self.ld_mask_extra

    def stride(self, dt):
        """Slab stride (step) / step stride (accum) of d ctx."""
        return self.N * self.lddctx(dt) + self.stride_extra

    def ts(self):
        """Live steps of every row of an accumulation."""
        if self.row_len is None:
            return np.full(self.N, self.T)
        return np.clip(np.asarray(self.row_len), 0, self.T)

    def live_rows(self):
        """Rows of a step call that are computed (not behind their caption's end)."""
        if self.row_len is None:
            return np.ones(self.N, dtype=bool)
        return self.step < np.asarray(self.row_len)

    def __repr__(self):
        return "Case(%s)" % self.name


OUTPUTS = {"fwd": ("alpha", "ctx"), "step": ("de", "d_att_h", "dctx_sum"), "accum": ("d_att", "d_p_att", "part")}
REQUIRED = {"fwd": ("att_h", "p_att", "att", "w_alpha", "alpha", "ctx"),
            "step": ("att_h", "p_att", "att", "w_alpha", "alpha", "dctx", "de", "d_att_h"),
            "accum": ("att_h_all", "alpha_all", "de_all", "dctx_all", "p_att", "w_alpha", "d_att", "d_p_att", "part")}


def esize(tensor, dt):
    return 2 if dt == BF16 and tensor in ("p_att", "att", "ctx", "d_att_h", "d_p_att") else 4


def layout(case, dt):
    """tensor -> dict(elems, start, shape, strides) in elements of the tensor's type; outputs are those of OUTPUTS[case.op]."""
    c, N, R, T = case, case.N, case.R, case.T
    A, H = c.A(dt), c.H(dt)
    out = {}

    def put(name, shape, strides=None, col=0):
        if strides is None:
            strides = tuple(int(np.prod(shape[i + 1:])) for i in range(len(shape)))
        sh = c.shift.get(name, 0) // esize(name, dt)
        last = sum((n - 1) * s for n, s in zip(shape, strides))
        whole = shape[0] * strides[0] if len(shape) > 1 else 0             # whole rows of the wider buffer
        out[name] = dict(elems=PAD + sh + max(col + last + 1, whole) + PAD, start=PAD + sh + col, shape=tuple(shape), strides=tuple(strides))
    put("p_att", (N, R, A))
    put("w_alpha", (A,))
    if c.row_len is not None:
        put("row_len", (N,))
    if c.op != "accum":
        put("att_h", (N, A))
        put("att", (N, R, H))
        put("alpha", (N, R))
    if c.op == "fwd":
        if c.bias:
            put("b_alpha", (1,))
        if c.mask:
            put("mask", (N, R), (c.ld_mask(), 1))
        put("ctx", (N, H), (c.ld_ctx(dt), 1))
    elif c.op == "step":
        put("dctx", (max(c.nslab, 1), N, H), (c.stride(dt), c.lddctx(dt), 1), c.col)
        if c.dsum:
            put("dctx_sum", (N, H), (c.ld_sum(dt), 1))
        put("de", (N, R))
        put("d_att_h", (N, A))
    else:
        put("att_h_all", (T, N, A))
        put("alpha_all", (T, N, R))
        put("de_all", (T, N, R))
        put("dctx_all", (T, N, H), (c.stride(dt), c.lddctx(dt), 1), c.col)
        put("d_att", (N, R, H))
        put("d_p_att", (N, R, A))
        put("part", (N, A + 1))
    return out


def lds_bytes(case, dt):
    """Dynamic LDS the forward / step launcher asks for (the generic kernel's; the fast forward kernels need less)."""
    A, H, R = case.A(dt), case.H(dt), case.R
    if case.op == "fwd":
        return 4 * (2 * A + 4 * R + 4 + 4 * H)
    if case.op == "step":
        return 4 * (6 * A + H + 5 * ((R + 3) & ~3))
    Rp, T = (R + 3) & ~3, case.T
    return max(4 * R * (-(-T // P1_TCH) * P1_TCH), 4 * (T * (A // 2 + Rp) + 2 * A + 4), 4 * T * (H + Rp), 4 * (T * (A + Rp) + 5 * A))


# ---- which kernel the launchers pick (csrc/attention.hip: fast_ok, uic_attention_bwd_accum_launch), and what they refuse ----
CONDITIONS = {"fwd": ("R", "A", "H", "att_h_al", "w_alpha_al"),
              "step": ("R", "A", "H", "att_h_al", "w_alpha_al", "lddctx", "dctx_al", "slab_stride", "sum_al", "sum_ld"),
              "p1": ("lddctx", "step_stride", "dctx_al"),
              "p2": ("dtype", "att_h_al", "w_alpha_al", "p_att_al8", "d_p_att_al8")}
REFUSALS_ASKED = ("dtype", "vec", "null", "p_att_al", "att_al", "d_att_al", "d_p_att_al", "lds")


def _al(lay, name, dt, k=16):
    return (lay[name]["start"] * esize(name, dt)) % k == 0


def broken_conditions(case, dt, part=None):
    """The conditions of the fast (fwd, step) or round-6 (accum: part "p1" / "p2") choice that do NOT hold for this call."""
    c, lay = case, layout(case, dt)
    A, H, v = c.A(dt), c.H(dt), vec(dt)
    bad = set()
    if c.op in ("fwd", "step"):
        if c.R > FAST_R:
            bad.add("R")
        if A // v > 64:
            bad.add("A")
        if H // v > 64:
            bad.add("H")
        for t in ("att_h", "w_alpha"):
            if not _al(lay, t, dt):
                bad.add(t + "_al")
        if c.op == "step":
            if c.lddctx(dt) % 4:
                bad.add("lddctx")
            if not _al(lay, "dctx", dt):
                bad.add("dctx_al")
            if c.nslab > 1 and c.stride(dt) % 4:
                bad.add("slab_stride")
            if c.dsum and not _al(lay, "dctx_sum", dt):
                bad.add("sum_al")
            if c.dsum and c.ld_sum(dt) % 4:
                bad.add("sum_ld")
    elif part == "p1":
        if c.lddctx(dt) % 4:
            bad.add("lddctx")
        if c.stride(dt) % 4:
            bad.add("step_stride")
        if not _al(lay, "dctx_all", dt):
            bad.add("dctx_al")
    else:
        assert part == "p2"
        if dt != BF16:
            bad.add("dtype")
        for t in ("att_h_all", "w_alpha"):
            if not _al(lay, t, dt):
                bad.add(t.replace("_all", "") + "_al")
        for t in ("p_att", "d_p_att"):
            if not _al(lay, t, dt, 8):
                bad.add(t + "_al8")
    return bad


def classify(case, dt):
    """UIC_ATTN_* (fwd, step) or the UIC_ATTN_ACCUM_* bits (accum) of an accepted call."""
    if case.op == "accum":
        return (0 if broken_conditions(case, dt, "p1") else P1_R6) | (0 if broken_conditions(case, dt, "p2") else P2_R6)
    if broken_conditions(case, dt):
        return GENERIC
    v = vec(dt)
    return FAST_FULL if case.A(dt) == 64 * v and case.H(dt) == 64 * v else FAST


def refusal(case, dt):
    """Why the launcher refuses the call (a name of REFUSALS_ASKED), or None."""
    c = case
    if dt not in (F32, BF16):
        return "dtype"
    if c.A(dt) % vec(dt) or c.H(dt) % vec(dt):
        return "vec"
    lay = layout(c, dt)
    if c.op in ("fwd", "step"):
        for t in ("p_att", "att"):
            if not _al(lay, t, dt):
                return t + "_al"
    else:
        if not _al(lay, "d_att", dt):
            return "d_att_al"
        if broken_conditions(c, dt, "p2"):
            for t in ("p_att", "d_p_att"):
                if not _al(lay, t, dt):
                    return t + "_al"
    if lds_bytes(c, dt) > LDS_MAX:
        return "lds"
    return None


KERNEL_NAMES = {("fwd", GENERIC): "attn_fwd_kernel", ("fwd", FAST): "attn_fwd_fast_kernel<FULL=0>", ("fwd", FAST_FULL): "attn_fwd_fast_kernel<FULL=1>",
                ("step", GENERIC): "attn_bwd_step_kernel", ("step", FAST): "attn_bwd_step_fast_kernel<FULL=0>",
                ("step", FAST_FULL): "attn_bwd_step_fast_kernel<FULL=1>"}


def kernel_of(case, dt, output):
    """Name of the kernel that writes `output` of an accepted call."""
    k = classify(case, dt)
    if case.op != "accum":
        return KERNEL_NAMES[(case.op, k)]
    if output == "d_att":
        return "attn_bwd_accum_p1_kernel" if k & P1_R6 else "attn_bwd_accum_kernel<PART=1>"
    return "attn_bwd_accum_p2_bf16_kernel" if k & P2_R6 else "attn_bwd_accum_kernel<PART=2>"


# ---- inputs ----
class Inputs:
    pass


def mask_of(kind, N, R, rng):
    m = np.ones((N, R), dtype=np.float32)
    if kind is None:
        return None
    for n in range(N):
        if kind == "prefix":
            m[n, max(1, (R * (n + 1)) // (N + 1)):] = 0
        elif kind == "holes":
            m[n, 1:-1] = (rng.random(max(R - 2, 0)) < 0.5)
            if R > 2:
                m[n, 1 + n % (R - 2)] = 0
        else:
            live = {"one-first": 0, "one-mid": R // 2, "one-last": R - 1}[kind]
            m[n] = 0
            m[n, live] = 1
    return m


def inputs(case, dt):
    """The tensors of a call, compact, as float32 arrays of what is stored (p_att, att: rounded to the operand dtype)."""
    c, N, R, T = case, case.N, case.R, case.T
    A, H = c.A(dt), c.H(dt)
    rng = np.random.default_rng(c.seed)
    f = np.float32
    x = Inputs()
    x.case, x.dt, x.op, x.N, x.R, x.A, x.H, x.T = c, dt, c.op, N, R, A, H, T
    nh = T if c.op == "accum" else 1
    v = c.values
    if v.startswith("wide"):
        lim = float(v[4:] or 25)
        p = rng.uniform(-lim, lim, (N, R, A))
        h = rng.uniform(-lim, lim, (nh, N, A))
        p[:, 0, :] = -h[0] + rng.standard_normal((N, A)) * 0.5              # opposite signs, a small sum
        if R > 2:
            p[:, 2, ::2] = -h[-1][:, ::2] + rng.standard_normal((N, (A + 1) // 2)) * 0.05
    else:
        p = rng.standard_normal((N, R, A))
        h = rng.standard_normal((nh, N, A))
    if v.startswith("limit"):                                               # exactly at (or one bf16 step beyond) a factoring limit
        lim = float(v[5:])
        p[:, :, 1], h[:, :, 1] = lim, lim                                   # every pair of adjacent steps: x0 x1 = (1 + e^{4 lim})^2
        p[:, :, 2], h[:, :, 2] = lim, -lim
        p[:, :, 3], h[:, :, 3] = -lim, -lim
        p[:, R // 2, 5] = -lim                                              # one region alone
        h[nh // 2, :, 6] = lim                                              # one step alone
    w = rng.standard_normal(A) * 3.0 / np.sqrt(A)
    x.p_att = round_to(p, dt)
    x.att_h = h.astype(f) if c.op == "accum" else h[0].astype(f)
    x.b_alpha = f(0.3) if (c.bias and c.op == "fwd") else None
    x.mask = mask_of(c.mask, N, R, rng)
    att = rng.standard_normal((N, R, H))
    if v.startswith("spread"):                                              # scores of a row spread over `spread` (> 104: weights underflow to 0)
        e = np.tanh(x.p_att.astype(np.float64) + x.att_h.astype(np.float64)[:, None, :]) @ w
        w = w * float(v[6:]) / (e.max(1) - e.min(1)).min()
        if x.mask is not None:                                              # the largest score stays live: the reference's own f32 limits
            for n in range(N):
                hi, live = int(np.argmax(e[n])), int(np.argmax(x.mask[n]))
                x.p_att[n, [hi, live]] = x.p_att[n, [live, hi]]
    x.w_alpha = w.astype(f)
    if c.op != "accum":
        if c.poison and x.mask is not None:
            att = np.where(x.mask[:, :, None] > 0, att, 1e30)               # finite: 0 x 1e30 = 0
        x.att = round_to(att, dt)
    if c.op == "step":
        fw = Inputs()
        fw.__dict__.update(x.__dict__)
        fw.op, fw.b_alpha = "fwd", None
        x.alpha = reference(fw)[0]["alpha"].astype(f)                       # (masked regions: exact zeros)
        ns = max(c.nslab, 1)
        x.dctx = np.stack([rng.standard_normal((N, H)) * 0.3 * 10.0 ** -z for z in range(ns)]).astype(f)
    if c.op == "accum":
        s = rng.standard_normal((T, N, R)) * 2
        s = np.exp(s - s.max(-1, keepdims=True))
        x.alpha_all = (s / s.sum(-1, keepdims=True)).astype(f)
        x.de_all = (rng.standard_normal((T, N, R)) * 0.1).astype(f)
        x.dctx_all = rng.standard_normal((T, N, H)).astype(f)
    x.row_len = None if c.row_len is None else np.asarray(c.row_len, dtype=np.int32)
    return x


# ---- the references and their bounds ----
def chain(n, dt):
    return vec(dt) * -(-n // (64 * vec(dt))) + 6


def _fin(ref, tol, bf16=False, exact=None):
    tol = tol + (2.0 ** -8 * np.abs(ref) if bf16 else 0.0)
    tol = np.maximum(tol, TINY)
    return np.where(exact, 0.0, tol) if exact is not None else tol


def _arg_units(p, h, dt, k):
    """ARG of the module docstring, [.., N, R, A]: the separately rounded arguments of the factored form (bf16, both within EXP_LIM)."""
    if dt != BF16:
        return 0.0
    fact = (2 * np.abs(p) <= EXP_LIM) & (2 * np.abs(h) <= EXP_LIM)
    return np.where(fact, k * (np.abs(p) + np.abs(h)), 0.0)


def reference(x, out_bf16=None):
    """(ref, tol): dicts of float64 arrays, keys = OUTPUTS[op] (dctx_sum only where the case has one), plus for the step "dctx".
    out_bf16 (default: the call is bf16): the bound has room for the rounding of ctx / d_att_h / d_p_att to bf16."""
    f = np.float64
    dt, N, R, A, H = x.dt, x.N, x.R, x.A, x.H
    bf = dt == BF16
    obf = bf if out_bf16 is None else out_bf16
    p, w = x.p_att.astype(f), x.w_alpha.astype(f)
    ref, tol = {}, {}
    if x.op == "fwd":
        h, att = x.att_h.astype(f), x.att.astype(f)
        b = 0.0 if x.b_alpha is None else f(x.b_alpha)
        e = np.tanh(p + h[:, None, :]) @ w + b
        de_abs = (C_TANH + 1 + chain(A, dt) + 1) * EPS * (np.abs(w).sum() + abs(b))
        mx = e.max(1, keepdims=True)
        ex = np.exp(e - mx)
        rel1 = de_abs + EPS * (3 * np.abs(e - mx) + 2)
        m = np.ones((N, R)) if x.mask is None else x.mask.astype(f)
        al = ex * m / (ex * m).sum(1, keepdims=True)
        rel = rel1 + (al * rel1).sum(1, keepdims=True) + (2 * R + 8) * EPS
        if x.mask is not None:                                              # (the softmax over all regions comes first)
            s = ex / ex.sum(1, keepdims=True)
            rel = rel + (s * rel1).sum(1, keepdims=True)
        ref["alpha"], tol["alpha"] = al, _fin(al, al * rel, exact=m == 0)
        ta = np.where(m == 0, 0.0, tol["alpha"])
        ref["ctx"] = np.einsum("nr,nrh->nh", al, att)
        mag = np.einsum("nr,nrh->nh", al, np.abs(att))
        tol["ctx"] = _fin(ref["ctx"], np.einsum("nr,nrh->nh", ta, np.abs(att)) + (1 + 9 * -(-R // 36) + 12) * EPS * mag, obf)
    elif x.op == "step":
        h, att, al = x.att_h.astype(f), x.att.astype(f), x.alpha.astype(f)
        live = x.case.live_rows()
        slabs = x.dctx.astype(f)
        dctx = slabs.sum(0)
        t_dc = 4 * len(slabs) * EPS * np.abs(slabs).sum(0) * (len(slabs) > 1)
        da = np.einsum("nh,nrh->nr", dctx, att)
        t_da = np.einsum("nh,nrh->nr", t_dc, np.abs(att)) + (1 + chain(H, dt)) * EPS * np.einsum("nh,nrh->nr", np.abs(dctx), np.abs(att))
        wbar = (al * da).sum(1, keepdims=True)
        t_wbar = (al * t_da).sum(1, keepdims=True) + (1 + R) * EPS * (al * np.abs(da)).sum(1, keepdims=True)
        de = al * (da - wbar)
        t_de = al * (t_da + t_wbar + 2 * EPS * (np.abs(da) + np.abs(wbar)))
        g = 1.0 - np.tanh(p + h[:, None, :]) ** 2
        dah = w * np.einsum("nr,nra->na", de, g)
        t_dah = np.abs(w) * (t_de.sum(1, keepdims=True) + (C_G + 9 * -(-R // 36) + 6) * EPS * np.abs(de).sum(1, keepdims=True))
        dead = ~live[:, None]
        z = lambda a: np.where(dead, 0.0, a)
        ref["de"], tol["de"] = z(de), _fin(de, t_de, exact=dead | (al == 0))
        ref["d_att_h"], tol["d_att_h"] = z(dah), _fin(dah, t_dah, obf, exact=dead | np.zeros_like(dah, dtype=bool))
        ref["dctx"], tol["dctx"] = z(dctx), _fin(dctx, t_dc, exact=dead | np.zeros_like(dctx, dtype=bool))
        if x.case.dsum:
            ref["dctx_sum"], tol["dctx_sum"] = ref["dctx"], tol["dctx"]
    else:
        T = x.T
        ts = x.case.ts()
        L = (np.arange(T)[:, None] < ts[None, :]).astype(f)                 # [T, N]
        h = x.att_h.astype(f)
        al, de, dc = x.alpha_all.astype(f) * L[:, :, None], x.de_all.astype(f) * L[:, :, None], x.dctx_all.astype(f) * L[:, :, None]
        tsn = ts.astype(f)
        ref["d_att"] = np.einsum("tnr,tnh->nrh", al, dc)
        tol["d_att"] = _fin(ref["d_att"], (4 * tsn + 4)[:, None, None] * EPS * np.einsum("tnr,tnh->nrh", al, np.abs(dc)))
        th = np.tanh(p[None] + h[:, :, None, :])                            # [T, N, R, A]
        ade = np.abs(de)
        ref["d_p_att"] = w * np.einsum("tnr,tnra->nra", de, 1.0 - th * th)
        G = (C_GF if bf else C_G) + _arg_units(p[None], h[:, :, None, :], dt, 0.77)
        K = 24.0 if bf else 3.0
        t = np.einsum("tnr,tnra->nra", ade, G + np.zeros_like(th)) + (K * tsn + 2)[:, None, None] * ade.sum(0)[:, :, None]
        tol["d_p_att"] = _fin(ref["d_p_att"], np.abs(w) * EPS * t, obf)
        r4 = -(-R // 4)
        TH = C_TANH + _arg_units(p[None], h[:, :, None, :], dt, 1.0)
        part = np.concatenate([np.einsum("tnr,tnra->na", de, th), de.sum((0, 2))[:, None]], axis=1)
        sde = ade.sum((0, 2))
        t_a = np.einsum("tnr,tnra->na", ade, TH + np.zeros_like(th)) + ((tsn * r4 + 2 * (tsn + r4 + 5) + 12) * sde)[:, None]
        t_b = (tsn * R + 8) * sde
        ref["part"], tol["part"] = part, _fin(part, EPS * np.concatenate([t_a, t_b[:, None]], axis=1))
    return ref, tol


def worst_ratio(got, ref, tol):
    """max over the elements of |got - ref| / tol (inf where got is not finite or a result that must be exact is not)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    err = np.where(np.isfinite(err), err, np.inf)
    r = np.where(err == 0, 0.0, err / np.where(tol > 0, tol, TINY * TINY))
    return float(r.max()) if r.size else 0.0


def dctx_sum_f32(x):
    """The sequential float32 sum of the slabs, which both step kernels must reproduce bit for bit (zeros on dead rows)."""
    s = x.dctx[0].copy()
    for z in range(1, len(x.dctx)):
        s = s + x.dctx[z]
    return np.where(x.case.live_rows()[:, None], s, np.float32(0))


# ---- the kernels' formulas in float32 ----
FORMS = {"fwd": ("tanhf", "exp"), "step": ("tanhf", "exp"), "accum": ("tanhf", "exp", "factored-40", "factored-21.5-shared")}


def _tanh32(s, form):
    f = np.float32
    if form == "tanhf":
        return np.tanh(s.astype(np.float64)).astype(f)
    e = np.exp2(s * LOG2E2)
    return f(1) - f(2) * (f(1) / (e + f(1)))


def restated_f32(x, form):
    """One rounding per operation, the kernels' order of operations where it matters (the slabs, the steps of an accumulation); wide
    sums in numpy's pairwise order.  form: "tanhf" (correctly rounded tanh), "exp" (1 - 2 / (1 + 2^(kx)) and exp2 / reciprocal in the
    softmax: the bf16 path), "factored-40" (rc = 1 / (1 + e^{2p} e^{2h}) where |2p|, |2h| <= 40, attn_bwd_accum_kernel<bf16, 2>),
    "factored-21.5-shared" (S1 / S2 sums and one reciprocal for two steps, the round-6 PART 2 kernel).  Results before the rounding
    to the operand dtype."""
    f = np.float32
    out = {}
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        p, w = x.p_att, x.w_alpha
        if x.op == "fwd":
            th = _tanh32(p + x.att_h[:, None, :], form)
            e = (w * th).sum(-1, dtype=f) + (f(0) if x.b_alpha is None else x.b_alpha)
            mx = e.max(1, keepdims=True)
            if form == "exp":
                ex = np.exp2((e - mx) * f(1.4426950408889634))
                al = ex * (f(1) / ex.sum(1, keepdims=True, dtype=f))
            else:
                ex = np.exp(e - mx)
                al = ex * (f(1) / ex.sum(1, keepdims=True, dtype=f))
            if x.mask is not None:
                al = al * x.mask
                al = al / al.sum(1, keepdims=True, dtype=f)
            out["alpha"] = al
            out["ctx"] = (al[:, :, None] * x.att).sum(1, dtype=f)
        elif x.op == "step":
            live = x.case.live_rows()[:, None]
            dctx = dctx_sum_f32(x)
            da = (dctx[:, None, :] * x.att).sum(-1, dtype=f)
            wbar = (x.alpha * da).sum(1, keepdims=True, dtype=f)
            de = x.alpha * (da - wbar)
            th = _tanh32(p + x.att_h[:, None, :], form)
            dah = (de[:, :, None] * (f(1) - th * th)).sum(1, dtype=f) * w
            out["de"], out["d_att_h"], out["dctx"] = np.where(live, de, f(0)), np.where(live, dah, f(0)), dctx
            if x.case.dsum:
                out["dctx_sum"] = dctx
        else:
            T, N, R, A = x.T, x.N, x.R, x.A
            ts = x.case.ts()
            d_att = np.zeros((N, R, x.H), dtype=f)
            acc = np.zeros((N, R, A), dtype=f)                              # sum de (1 - tanh^2)
            dw = np.zeros((N, R, A), dtype=f)                               # sum de tanh
            s1, s2 = np.zeros((N, R, A), dtype=f), np.zeros((N, R, A), dtype=f)
            anydirect = np.zeros((N, R, A), dtype=bool)
            tot = np.zeros((N, R), dtype=f)
            lim = {"factored-40": EXP_LIM, "factored-21.5-shared": P2_LIM}.get(form)
            shared = form.endswith("shared")
            if lim is not None:
                ep = np.exp2(p * LOG2E2)
                okp = np.abs(p) * f(2) <= f(lim)
                xs = [ep * np.exp2(x.att_h[t] * LOG2E2)[:, None, :] + f(1) for t in range(T)]
                # (one h beyond the limit in a live step sends the whole workgroup, here the whole row, to the direct form)
                okh = np.array([all((np.abs(x.att_h[t, n]) * f(2) <= f(lim)).all() for t in range(int(ts[n]))) for n in range(N)])
            for t in range(T):
                lv = (t < ts).astype(f)
                de = x.de_all[t] * lv[:, None]
                d_att = d_att + (x.alpha_all[t] * lv[:, None])[:, :, None] * x.dctx_all[t][:, None, :]
                tot = tot + de
                th = _tanh32(p + x.att_h[t][:, None, :], "exp" if lim is not None else form)
                g = f(1) - th * th
                if lim is not None:
                    ok = okp & okh[:, None, None]
                    rc = f(1) / xs[t]
                    if shared:
                        t0 = t & ~1
                        pair = (t0 + 1 < ts)[:, None, None] & (t0 + 1 < T)
                        if t0 + 1 < T:
                            inv = f(1) / (xs[t0] * xs[t0 + 1])
                            rc = np.where(pair, inv * xs[t0 + 1 if t == t0 else t0], rc)
                        live3 = (lv > 0)[:, None, None]
                        anydirect |= ~ok & live3
                        dl = de[:, :, None]
                        s1 = s1 + np.where(ok, dl * rc, f(0))
                        s2 = s2 + np.where(ok, (dl * rc) * rc, f(0))
                    else:
                        g = np.where(ok, f(4) * (rc - rc * rc), g)
                        th = np.where(ok, f(1) - f(2) * rc, th)
                acc = acc + de[:, :, None] * g
                dw = dw + de[:, :, None] * th
            if shared:
                # (a region with an element beyond the limit takes the direct form as a whole wave; per element here)
                acc = np.where(anydirect, acc, f(4) * (s1 - s2))
                dw = np.where(anydirect, dw, tot[:, :, None] - f(2) * s1)
            out["d_att"] = d_att
            out["d_p_att"] = acc * w
            out["part"] = np.concatenate([dw.sum(1, dtype=f), tot.sum(1, dtype=f)[:, None]], axis=1)
    return out


# ---- the cases ----
SHAPES_ALL_R = ((64, 64), (2, 3))                                            # (A, H) in 16-byte chunks, at every R
SHAPES_EDGE_R = ((64, 63), (63, 64), (65, 64), (64, 65), (1, 1), (63, 63), (1, 64), (65, 65))      # at R = 36 | 37
CHOICE_R = (1, 3, 35, 36, 37, 40)
LDDCTX = ((1, 0), (3, 0), (1, 2))                                            # H, 3H (Step::bwd_step), H + 2
MASKS = (None, "prefix", "holes", "one-first", "one-mid", "one-last")
STEP_NSLAB = (0, 1, 2, 3, 4, 5, 7)
ACCUM_T = (1, 2, 5, 6, 7, 12, 13)
ACCUM_R = (1, 3, 4, 36, 37, 72, 73)
ACCUM_A = (8, 72, 512)
ACCUM_H = (8, 40, 512)
LIMITS = ("10.75", "10.8125", "20", "20.125")


def _choice(op, cs):
    for R in CHOICE_R:
        for Av, Hv in SHAPES_ALL_R:
            cs.append(Case("%s-R%d-%dx%d" % (op, R, Av, Hv), op, R=R, Av=Av, Hv=Hv, lddctx=(3, 0)))
    for R in (36, 37):
        for Av, Hv in SHAPES_EDGE_R:
            cs.append(Case("%s-R%d-%dx%d" % (op, R, Av, Hv), op, R=R, Av=Av, Hv=Hv, lddctx=(3, 0)))


@functools.lru_cache(maxsize=None)
def fwd_cases():
    cs = []
    _choice("fwd", cs)

    def add(name, **kw):
        cs.append(Case("fwd-" + name, "fwd", **kw))
    for R, Av, Hv in ((36, 64, 64), (37, 2, 3), (5, 2, 3)):                   # fast-full, generic, fast
        for m in MASKS[1:]:
            add("mask-%s-R%d" % (m, R), R=R, Av=Av, Hv=Hv, mask=m, poison=True, ld_mask=0 if m == "holes" else 3, N=4)
    add("ldctx-3H", R=36, Av=64, Hv=64, ld_ctx=(3, 0))
    add("ldctx-H+3", R=7, ld_ctx=(1, 3))
    add("ldctx-generic", R=37, ld_ctx=(2, 1), mask="prefix", ld_mask=1)
    add("nobias", R=36, Av=64, Hv=64, bias=False)
    add("nobias-generic", R=40, bias=False)
    for R, Av, Hv in ((36, 64, 64), (37, 2, 3), (9, 5, 2)):
        add("wide-R%d" % R, R=R, Av=Av, Hv=Hv, values="wide")
        add("spread110-R%d" % R, R=R, Av=Av, Hv=Hv, values="spread110")
        add("spread90-R%d" % R, R=R, Av=Av, Hv=Hv, values="spread90")
        add("spread90-prefix-R%d" % R, R=R, Av=Av, Hv=Hv, values="spread90", mask="prefix", poison=True)
    add("mis-att_h", R=36, Av=64, Hv=64, shift={"att_h": 4})                 # honest fallbacks: the generic kernel reads them by the word
    add("mis-w_alpha", R=36, Av=64, Hv=64, shift={"w_alpha": 4})
    add("mis-att_h-8", R=5, shift={"att_h": 8})
    add("N1", N=1, R=36, Av=64, Hv=64)
    # the LDS bound: 64 KB (what a launch gets unasked) and 160 KB (what the launcher admits), on both sides
    for H in (4088, 4096, 10232):
        add("lds-H%d" % H, N=1, R=1, A=8, H=H, dtypes=(F32,) if H % 8 or H > 5000 else (F32, BF16))
    assert len({c.name for c in cs}) == len(cs)
    return tuple(cs)


@functools.lru_cache(maxsize=None)
def step_cases():
    cs = []
    _choice("step", cs)

    def add(name, **kw):
        cs.append(Case("step-" + name, "step", **kw))
    for Av, Hv, R in ((64, 64, 36), (2, 3, 36), (2, 3, 37)):
        for l in LDDCTX:
            add("lddctx-%d-%d-R%d-%dx%d" % (l + (R, Av, Hv)), R=R, Av=Av, Hv=Hv, lddctx=l, col=0 if l[0] == 1 else 2 * Hv * 4,
                data="step-lddctx-R%d-%dx%d" % (R, Av, Hv), nslab=3, dsum=True)
    for ns in STEP_NSLAB:
        for tag, kw in (("full", dict(R=36, Av=64, Hv=64)), ("fast", dict(R=5)), ("generic", dict(R=37))):
            add("nslab%d-%s" % (ns, tag), nslab=ns, lddctx=(3, 0), dsum=ns % 2 == 0 or ns == 7, N=2, **kw)
    add("nslab4-nosum", nslab=4, lddctx=(3, 0), R=36, Av=64, Hv=64)
    add("nslab5-sum-generic-ld", nslab=5, lddctx=(1, 2), dsum=True, R=7)
    for tag, kw in (("full", dict(R=36, Av=64, Hv=64)), ("fast", dict(R=5)), ("generic", dict(R=37)), ("generic-ld", dict(R=5, lddctx=(1, 2)))):
        for ns, dsum in ((0, False), (3, True), (5, True)):
            kw2 = dict(dict(lddctx=(3, 0)), **kw)
            add("rowlen-%s-s%d" % (tag, ns), N=4, row_len=(3, 2, 0, 7), step=2, nslab=ns, dsum=dsum, **kw2)
    add("rowlen-all-dead", N=3, row_len=(0, 1, 2), step=2, R=36, Av=64, Hv=64, dsum=True, nslab=2)
    add("rowlen-all-live", N=3, row_len=(1, 5, 2), step=0, R=37, dsum=True, nslab=2)
    for m in ("holes", "one-mid", "one-last", "prefix"):                     # alpha holds exact zeros
        add("mask-%s-full" % m, R=36, Av=64, Hv=64, mask=m, poison=True)
        add("mask-%s-generic" % m, R=37, mask=m, poison=True)
    for R, Av, Hv in ((36, 64, 64), (37, 2, 3), (9, 5, 2)):
        add("wide-R%d" % R, R=R, Av=Av, Hv=Hv, values="wide", nslab=2)
        add("spread90-R%d" % R, R=R, Av=Av, Hv=Hv, values="spread90")
    # each condition of the fast choice broken alone, on the shape of the benchmarked step (nslab = 2, dctx_sum at 3H)
    base = dict(R=36, Av=64, Hv=64, nslab=2, dsum=True, lddctx=(3, 0))
    add("base", **base)
    for t in ("att_h", "w_alpha", "dctx", "dctx_sum"):
        add("mis-" + t, shift={t: 4}, **base)
    add("mis-slab-stride", stride_extra=2, **base)
    add("mis-slab-stride-one-slab", stride_extra=2, **dict(base, nslab=1))   # (a stride nobody uses)
    add("mis-ld-sum", ld_sum=(3, 2), **base)
    add("mis-lddctx", **dict(base, lddctx=(3, 2)))
    for A in (2724, 2728, 6820):
        add("lds-A%d" % A, N=1, R=1, A=A, H=8, dtypes=(F32,) if A % 8 else (F32, BF16))
    assert len({c.name for c in cs}) == len(cs)
    return tuple(cs)


@functools.lru_cache(maxsize=None)
def accum_cases():
    cs = []

    def add(name, **kw):
        kw = dict(dict(lddctx=(3, 0), N=2), **kw)
        cs.append(Case("accum-" + name, "accum", **kw))
    for i, T in enumerate(ACCUM_T):
        for j in (0, 3):
            R, A, H = ACCUM_R[(i + j) % 7], ACCUM_A[(i + j) % 3], ACCUM_H[(i + 2 * j + 1) % 3]
            add("T%d-R%d-A%d-H%d" % (T, R, A, H), T=T, R=R, A=A, H=H)
    for R in ACCUM_R:
        add("R%d-T7" % R, T=7, R=R, A=72, H=40, N=3)
    add("big", T=13, R=73, A=512, H=512)
    add("ld-H", T=6, R=4, A=72, H=40, lddctx=(1, 0))
    for k, rl in enumerate(((0, 1, 6, 7), (10, 0, 1, 6), (7, 6, 1, 10))):
        for T, R, A, H in ((7, 37, 72, 40), (7, 4, 512, 8)):
            add("rowlen%d-R%d" % (k, R), T=T, R=R, A=A, H=H, N=4, row_len=rl)
    add("rowlen-all-dead", T=5, R=5, A=8, H=8, N=2, row_len=(0, -1))
    base = dict(T=7, R=37, A=72, H=40, N=3, row_len=(7, 3, 9))
    add("base", **base)
    for t in ("att_h_all", "w_alpha", "dctx_all"):                           # honest fallbacks: the first kernels read them by the word
        add("mis-" + t, shift={t: 4}, **base)
    add("mis-both-parts", shift={"w_alpha": 4, "dctx_all": 4}, **base)        # both first forms in bf16 too
    add("mis-step-stride", stride_extra=2, **base)
    add("mis-lddctx", stride_extra=2, **dict(base, lddctx=(3, 2)))                # (3 (3H + 2) + 2: the step stride stays a multiple of 4)
    add("mis-patt-8", shift={"p_att": 8}, dtypes=(BF16,), **base)            # the round-6 PART 2 kernel reads 8 bytes at a time
    add("mis-dpatt-8", shift={"d_p_att": 8}, dtypes=(BF16,), **base)
    for v in ("wide", "wide20", "wide10") + tuple("limit" + l for l in LIMITS):
        for T in (2, 5):
            add("%s-T%d" % (v, T), T=T, R=5, A=16, H=8, values=v)
            add("%s-T%d-first" % (v, T), T=T, R=5, A=16, H=8, values=v, shift={"att_h_all": 4})      # attn_bwd_accum_kernel<bf16, 2>: EXP_LIM
    add("limit10.75-T12-R37", T=12, R=37, A=72, H=8, values="limit10.75", N=3, row_len=(12, 11, 2))
    assert len({c.name for c in cs}) == len(cs)
    return tuple(cs)


def all_cases():
    return fwd_cases() + step_cases() + accum_cases()


@functools.lru_cache(maxsize=None)
def refused_cases():
    """Calls the launchers must refuse: (case, dtype passed, null operand or None, the name of REFUSALS_ASKED).  A case with a dtype
    outside the two is laid out as f32."""
    out = []

    def add(name, op, dts, why, null=None, **kw):
        c = Case("refuse-%s-%s" % (op, name), op, dtypes=dts, **kw)
        for dt in dts:
            out.append((c, dt, null, why))
    for op in OPS:
        kw = dict(T=3, lddctx=(3, 0)) if op == "accum" else dict(lddctx=(3, 0), nslab=2, dsum=op == "step")
        add("dtype7", op, (7,), "dtype", **kw)
        add("dtype-1", op, (-1,), "dtype", **kw)
        add("A6", op, (F32,), "vec", A=6, H=8, **kw)
        add("H6", op, (F32,), "vec", A=8, H=6, **kw)
        add("A12", op, (BF16,), "vec", A=12, H=8, **kw)
        add("H12", op, (BF16,), "vec", A=8, H=12, **kw)
        for name in REQUIRED[op]:
            add("null-" + name, op, (F32, BF16), "null", null=name, **kw)
    for op in ("fwd", "step"):
        for t in ("p_att", "att"):
            for sh in (4, 8):
                add("mis-%s-%d" % (t, sh), op, (F32, BF16), t + "_al", shift={t: sh}, R=36, Av=64, Hv=64)
            add("mis-%s-2" % t, op, (BF16,), t + "_al", shift={t: 2}, R=37)
    for sh in (4, 8):
        add("mis-d_att-%d" % sh, "accum", (F32, BF16), "d_att_al", shift={"d_att": sh}, T=3, lddctx=(3, 0))
    for t in ("p_att", "d_p_att"):
        add("mis-%s-4" % t, "accum", (F32, BF16), t + "_al", shift={t: 4}, T=3, lddctx=(3, 0))
        add("mis-%s-8" % t, "accum", (F32,), t + "_al", shift={t: 8}, T=3, lddctx=(3, 0))
        add("mis-%s-8-first" % t, "accum", (BF16,), t + "_al", shift={t: 8, "w_alpha": 4}, T=3, lddctx=(3, 0))      # no round-6 kernel to take it
    add("lds-H10240", "fwd", (F32, BF16), "lds", N=1, R=1, A=8, H=10240)
    add("lds-A6824", "step", (F32, BF16), "lds", N=1, R=1, A=6824, H=8)
    add("lds-T", "accum", (F32, BF16), "lds", N=1, R=4, A=512, H=8, T=80, lddctx=(1, 0))
    return tuple(out)
