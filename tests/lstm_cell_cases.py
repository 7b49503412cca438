"""Cases, float64 reference, per-element bound and kernel-choice classifier for the LSTM cell backward kernels (csrc/lstm_cell.hip:
lstm_bwd_kernel, lstm_bwd_vec4_kernel<T, SIMPLE>, maxout_lstm_bwd_kernel; csrc/bptt_fused.hip: h2att_cell_bwd_kernel<KS>) behind
uic_lstm_cell_bwd_sources, uic_maxout_lstm_cell_bwd and uic_h2att_cell_bwd -- shared by tests/test_lstm_cell_cases_host.py (the cases
reach every kernel and both sides of every condition of the choice; a float32 restatement of the kernels' formulas stays inside a
quarter of the bound) and tests/test_gpu_lstm_cell.py (the kernels themselves).

The reference works on the STORED activated gates, in float64, without logit / atanh and without autograd:
    dh  = drop(dh0) + dh1 + dh2 + sum_z slabA[z] + sum_z slabB[z]           (maxout: drop(dh0 + dh1); fused: datth h2attT^T + slabs)
    tc  = tanh(c);   dc = dc_in + dh go (1 - tc^2)
    d_i = dc gg gi (1 - gi);  d_f = dc c_prev gf (1 - gf);  d_g = dc gi (1 - gg^2);  d_o = dh tc go (1 - go);  dc_out = dc gf
(maxout, P/models/FCModel_NMT.py:32-50: g = max(a, b) is stored as it is, so d_g = dc gi, routed to a where `first` is set, else to b).

The bound is per element, eps = 2^-24, C = 32:   S = sum |every term added into dh|,   Mag_dc = |dc_in| + S |go|
    d_i: C eps Mag_dc |gg| gi (1 - gi)      d_f: C eps Mag_dc |c_prev| gf (1 - gf)      d_g: C eps Mag_dc gi
    d_o: C eps S go (1 - go)                dc_out: C eps Mag_dc gf
The cancelling factors 1 - tc^2 and 1 - gg^2 count as 1: at saturation it is their ABSOLUTE error that survives.  bf16 outputs add
2^-8 |ref| for the rounding of the result.  For the fused operator the terms added into dh are the A products a_k b_k of the GEMM and
the slab entries, so S = sum_k |a_k b_k| + sum |slab entries|, to which A eps sum_k |a_k b_k| is added for the accumulation on the
matrix cores.  Every tolerance has a floor of 2^-126 (results below the smallest normal f32 may be flushed).
C = 32: counting roundings gives about 36 in the worst case (up to 11 additions in dh, about 18 for 1 - tc^2 through the exp / rcp
form, the rest for the products); the float32 restatement below, in both tanh forms, stays below C / 4 on every case
(tests/test_lstm_cell_cases_host.py holds that and records the measured maximum).

Every strided source is a view into a larger buffer that holds a NaN canary everywhere else (layout()): a kernel that reads beside
its view poisons its output, one that writes beside its outputs changes a canary.
"""
import functools
import zlib

import numpy as np

F32, BF16 = 0, 1
EPS = 2.0 ** -24
C_BOUND = 32.0
TINY = 2.0 ** -126
SPARSE_FROM = 2 ** 28                      # buffers of more elements are allocated uninitialised: only their view is written
PAD = 64                                   # canary elements in front of and behind every view (a multiple of 16 bytes)
SCALAR, VEC4, VEC4_SIMPLE = 0, 1, 2        # UIC_LSTM_BWD_*
VEC_MIN = 65536                            # the vec4 kernel from M * H >= this
NT = 256
FT = 32                                    # the fused kernel's tile: FT rows x FT units
SITE_OUT0 = 16
DH_MAG = (1.0, 1e-2, 1e-4)                 # dh0, dh1, dh2
SLAB_MAG = {"A": 3e-1, "B": 5e-2}          # slice z: this times 10^-z


class Case:
    """One call.  Leading dimensions and columns are given as (multiple of H, extra elements); nothing is modified afterwards."""

    def __init__(self, name, op="cell", M=128, H=512, A=0, dh0=((1, 0), (0, 0)), dh1=None, dh2=None, nA=0, layA=((3, 0), (2, 0)), strideA=None,
                 nB=0, layB=((2, 0), (0, 0)), strideB=None, drop_p=0.0, site=0, cprev="yes", gscale=1.0, cscale=1.0, shift=None, far=False,
                 dtypes=(F32, BF16)):
        self.name, self.op, self.M, self.H, self.A = name, op, M, H, A

        def lay(l):
            return None if l is None else (l[0][0] * H + l[0][1], l[1][0] * H + l[1][1])          # (ld, first column)
        self.dh = [lay(dh0) if op != "fused" else None, lay(dh1), lay(dh2)]
        self.nA, self.nB = nA, nB
        self.layA, self.layB = lay(layA), lay(layB)
        self.strideA = M * self.layA[0] if strideA is None else strideA
        self.strideB = M * self.layB[0] if strideB is None else strideB
        self.drop_p, self.site, self.cprev, self.gscale, self.cscale = drop_p, site, cprev, gscale, cscale
        self.shift = dict(shift or {})                                                            # tensor -> bytes off 16-byte alignment
        self.far, self.dtypes = far, dtypes
        self.seed = zlib.crc32(name.encode()) % (2 ** 31)
        self.G = 5 if op == "maxout" else 4

    def __repr__(self):
        return "Case(%s)" % self.name


def esize(tensor, dtype):
    return 2 if dtype == BF16 and tensor in ("gates", "dgates", "datth", "h2attT") else 4


def layout(case, dtype):
    """tensor -> dict(elems: buffer length, start: first element of the view, shape, strides) in elements of the tensor's type.  The
    outputs of the fused operator are allocated up to a whole tile of rows: rows >= N belong to the canary."""
    c, M, H = case, case.M, case.H
    out = {}

    def put(name, shape, strides, col=0, rows_alloc=None):
        sh = c.shift.get(name, 0) // esize(name, dtype)
        start = PAD + sh + col
        last = sum((n - 1) * s for n, s in zip(shape, strides))             # the view's last element, from its first
        rows = shape[-2] if rows_alloc is None else rows_alloc
        whole = (shape[0] - 1) * strides[0] * (len(shape) == 3) + rows * strides[-2]      # whole rows of the wider buffer
        elems = PAD + sh + max(col + last + 1, whole) + PAD
        out[name] = dict(elems=elems, start=start, shape=tuple(shape), strides=tuple(strides), sparse=elems > SPARSE_FROM)
    for i, l in enumerate(c.dh):
        if l is not None:
            put("dh%d" % i, (M, H), (l[0], 1), l[1])
    if c.nA:
        put("slabA", (c.nA, M, H), (c.strideA, c.layA[0], 1), c.layA[1])
    if c.nB:
        put("slabB", (c.nB, M, H), (c.strideB, c.layB[0], 1), c.layB[1])
    rows = -(-M // FT) * FT if c.op == "fused" else None
    put("dc", (M, H), (H, 1), rows_alloc=rows)
    put("c", (M, H), (H, 1))
    if c.cprev != "no":
        put("c_prev", (M, H), (H, 1))
    put("gates", (M, c.G * H), (c.G * H, 1))
    put("dgates", (M, c.G * H), (c.G * H, 1), rows_alloc=rows)
    if c.op == "fused":
        put("datth", (M, c.A), (c.A, 1))
        put("h2attT", (H, c.A), (c.A, 1))
    return out


# ---- which kernel the launcher picks (csrc/lstm_cell.hip uic_lstm_bwd_launch; csrc/bptt_fused.hip uic_h2att_cell_bwd_eligible) ----
CELL_CONDITIONS = ("size", "h4", "rows", "nA", "nB", "near", "dc_al", "c_al", "c_prev_al", "gates_al", "dgates_al",
                   "dh0_al", "dh0_ld", "dh1_al", "dh1_ld", "dh2_al", "dh2_ld", "slabA_al", "slabA_ld", "slabA_stride", "slabB_al", "slabB_ld",
                   "slabB_stride")
FUSED_CONDITIONS = ("dtype", "rows", "H32", "A", "nA", "nB", "dc_al", "c_al", "c_prev_al", "datth_al", "h2attT_al", "gates_al", "dgates_al",
                    "slabA_al", "slabA_ld", "slabA_stride", "slabB_al", "slabB_ld", "slabB_stride")
FUSED_REFUSALS_ASKED = ("A", "H32", "dtype", "nA", "dc_al")       # what the refused calls must at least cover


def _al(lay, name, dtype, k=16):
    return (lay[name]["start"] * esize(name, dtype)) % k == 0


def broken_conditions(case, dtype):
    """The conditions of the vec4 choice that do NOT hold for this call (empty: a vec4 kernel runs)."""
    c, M, H, lay = case, case.M, case.H, layout(case, dtype)
    bad = set()
    if M * H < VEC_MIN:
        bad.add("size")
    if H % 4:
        bad.add("h4")
    if M > 65535:
        bad.add("rows")
    if c.nA > 4:
        bad.add("nA")
    if c.nB > 4:
        bad.add("nB")
    for t in ("dc", "c", "c_prev"):
        if t in lay and not _al(lay, t, dtype):
            bad.add(t + "_al")
    for t in ("gates", "dgates"):
        if not _al(lay, t, dtype, 8 if dtype == BF16 else 16):
            bad.add(t + "_al")
    limit = (2 ** 31 - 16) // 4                                        # floats a 32-bit buffer offset reaches
    far = M * H > limit
    for i, l in enumerate(c.dh):
        if l is not None:
            t = "dh%d" % i
            if not _al(lay, t, dtype):
                bad.add(t + "_al")
            if l[0] % 4:
                bad.add(t + "_ld")
            far |= (M - 1) * l[0] + H > limit
    for t, n, l, st in (("slabA", c.nA, c.layA, c.strideA), ("slabB", c.nB, c.layB, c.strideB)):
        if n:
            if not _al(lay, t, dtype):
                bad.add(t + "_al")
            if l[0] % 4:
                bad.add(t + "_ld")
            if st % 4:
                bad.add(t + "_stride")
            far |= (n - 1) * st + (M - 1) * l[0] + H > limit
    if far:
        bad.add("near")
    return bad


def classify(case, dtype):
    """UIC_LSTM_BWD_* of a `cell` case."""
    if broken_conditions(case, dtype):
        return SCALAR
    simple = case.dh[0] is not None and case.dh[1] is None and case.dh[2] is None and case.cprev != "no"
    return VEC4_SIMPLE if simple else VEC4


def vec4_geometry(H):
    """(threads per workgroup, workgroups in x, live lanes of the last workgroup) of the vec4 launch."""
    h4 = H // 4
    bt = NT if h4 >= NT else (h4 + 63) // 64 * 64
    gx = -(-h4 // bt)
    return bt, gx, h4 - (gx - 1) * bt


def fused_broken(case, dtype):
    """The conditions of uic_h2att_cell_bwd_eligible that do not hold (empty: the fused kernel runs, KS = A / 128) -- the whole
    predicate; FUSED_CONDITIONS lists every name this can return."""
    c, lay = case, layout(case, dtype)
    bad = set()
    if dtype != BF16:
        bad.add("dtype")
    if c.M < 1:
        bad.add("rows")
    if c.H % FT:
        bad.add("H32")
    if c.A not in (128, 256, 512):
        bad.add("A")
    if c.nA > 4:
        bad.add("nA")
    if c.nB > 4:
        bad.add("nB")
    for t in ("dc", "c", "c_prev", "datth", "h2attT"):
        if t in lay and not _al(lay, t, dtype):
            bad.add(t + "_al")
    for t in ("gates", "dgates"):
        if not _al(lay, t, dtype, 8):
            bad.add(t + "_al")
    for t, n, l, st in (("slabA", c.nA, c.layA, c.strideA), ("slabB", c.nB, c.layB, c.strideB)):
        if n:
            if not _al(lay, t, dtype):
                bad.add(t + "_al")
            if l[0] % 4:
                bad.add(t + "_ld")
            if st % 4:
                bad.add(t + "_stride")
    return bad


# ---- inputs ----
def round_to(x, dtype):
    """float32 values that the operand dtype holds exactly."""
    x = np.asarray(x, dtype=np.float32)
    if dtype != BF16:
        return x
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).bfloat16().float().numpy()


def _sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


class Inputs:
    pass


def inputs(case, dtype):
    """The tensors of a call, compact (no strides), float32 values; gates / datth / h2attT hold what `dtype` stores.  At gscale 8 many
    bf16 gates are exactly 0, 1 or +-1; at cscale 6 tanh(c) is 1 to within an ulp for an eighth of the cells."""
    c, M, H = case, case.M, case.H
    rng = np.random.default_rng(c.seed)
    x = Inputs()
    x.M, x.H, x.op, x.dtype = M, H, c.op, dtype
    z = rng.standard_normal((M, c.G, H)) * c.gscale
    if c.op == "maxout":
        a, b = z[:, 3], z[:, 4]
        g = np.stack([_sigmoid(z[:, 0]), _sigmoid(z[:, 1]), _sigmoid(z[:, 2]), np.maximum(a, b), (a >= b).astype(np.float64)], axis=1)
    else:
        g = np.stack([_sigmoid(z[:, 0]), _sigmoid(z[:, 1]), np.tanh(z[:, 2]), _sigmoid(z[:, 3])], axis=1)
    x.gates = round_to(g, dtype)                                               # [M, G, H]
    x.c = (rng.standard_normal((M, H)) * c.cscale).astype(np.float32)
    x.c_prev = None if c.cprev == "no" else (rng.standard_normal((M, H)) * (1e-3 if c.cprev == "small" else c.cscale)).astype(np.float32)
    x.dc = rng.standard_normal((M, H)).astype(np.float32)
    x.dh = [None if l is None else (rng.standard_normal((M, H)) * DH_MAG[i]).astype(np.float32) for i, l in enumerate(c.dh)]
    x.slabA = np.stack([rng.standard_normal((M, H)) * SLAB_MAG["A"] * 10.0 ** -k for k in range(c.nA)]).astype(np.float32) if c.nA else None
    x.slabB = np.stack([rng.standard_normal((M, H)) * SLAB_MAG["B"] * 10.0 ** -k for k in range(c.nB)]).astype(np.float32) if c.nB else None
    x.datth = x.h2attT = None
    if c.op == "fused":
        x.datth = round_to(rng.standard_normal((M, c.A)), BF16)
        x.h2attT = round_to(rng.standard_normal((H, c.A)) / np.sqrt(c.A), BF16)
    return x


def drop_keep(n, p, seed, site, base=0):
    """uic_drop_scale's keep decision (csrc/uic_common.h), restated in uint32; tests/test_gpu_embedding.py pins it against the library."""
    from embedding_cases import drop_keep as k
    return k(n, p, seed, site, base)


def host_mask(case):
    """The dropout factor of every element [M, H] (float64), from the restated hash; None without dropout."""
    if case.drop_p <= 0:
        return None
    keep = drop_keep(case.M * case.H, case.drop_p, case.seed, case.site)
    scale = np.float64(np.float32(1.0) / (np.float32(1.0) - np.float32(case.drop_p)))
    return np.where(keep, scale, 0.0).reshape(case.M, case.H)


# ---- the reference and its bound ----
def dh_terms(x, mask):
    """Every term added into dh as float64 [M, H] arrays, and S = the sum of their magnitudes."""
    f = np.float64
    m = 1.0 if mask is None else mask
    terms = []
    for i, d in enumerate(x.dh):
        if d is not None:
            terms.append(d.astype(f) * (m if (i == 0 or x.op == "maxout") else 1.0))
    for s in (x.slabA, x.slabB):
        if s is not None:
            terms += [t.astype(f) for t in s]
    S = sum((np.abs(t) for t in terms), np.zeros((x.M, x.H)))
    if x.datth is not None:
        a, b = x.datth.astype(f), x.h2attT.astype(f)
        terms.append(a @ b.T)
        sumabs = np.abs(a) @ np.abs(b).T
        S = S + sumabs + a.shape[1] * EPS * sumabs
    return terms, S


def reference(x, mask=None, out_bf16=None):
    """(ref, tol): dicts of float64 [M, H] arrays.  Keys in the order of the gate blocks of dgates, then "dc".  out_bf16 (default: the
    inputs' dtype is bf16): dgates is rounded to bf16."""
    f = np.float64
    out_bf16 = x.dtype == BF16 if out_bf16 is None else out_bf16
    terms, S = dh_terms(x, mask)
    dh = sum(terms, np.zeros((x.M, x.H)))
    g = x.gates.astype(f)
    c = x.c.astype(f)
    cp = np.zeros_like(c) if x.c_prev is None else x.c_prev.astype(f)
    dc_in = x.dc.astype(f)
    tc = np.tanh(c)
    if x.op == "maxout":
        gi, gf, go, gg, first = g[:, 0], g[:, 1], g[:, 2], g[:, 3], g[:, 4] > 0.5
    else:
        gi, gf, gg, go, first = g[:, 0], g[:, 1], g[:, 2], g[:, 3], np.ones((x.M, x.H), dtype=bool)
    dc = dc_in + dh * go * (1.0 - tc * tc)
    mag = np.abs(dc_in) + S * np.abs(go)
    k = C_BOUND * EPS
    ref, tol = {}, {}
    ref["d_i"], tol["d_i"] = dc * gg * gi * (1 - gi), k * mag * np.abs(gg) * gi * (1 - gi)
    ref["d_f"], tol["d_f"] = dc * cp * gf * (1 - gf), k * mag * np.abs(cp) * gf * (1 - gf)
    d_o, t_o = dh * tc * go * (1 - go), k * S * go * (1 - go)
    if x.op == "maxout":
        ref["d_o"], tol["d_o"] = d_o, t_o
        dg, tg = dc * gi, k * mag * gi
        ref["d_g1"], tol["d_g1"] = np.where(first, dg, 0.0), np.where(first, tg, 0.0)
        ref["d_g2"], tol["d_g2"] = np.where(first, 0.0, dg), np.where(first, 0.0, tg)
    else:
        ref["d_g"], tol["d_g"] = dc * gi * (1 - gg * gg), k * mag * gi
        ref["d_o"], tol["d_o"] = d_o, t_o
    ref["dc"], tol["dc"] = dc * gf, k * mag * gf
    for n in tol:
        if n != "dc" and out_bf16:
            tol[n] = tol[n] + 2.0 ** -8 * np.abs(ref[n])
        live = np.ones_like(first) if n not in ("d_g1", "d_g2") else (first if n == "d_g1" else ~first)
        tol[n] = np.where(live, np.maximum(tol[n], TINY), 0.0)              # (the gate block `first` does not pick is exactly 0)
    return ref, tol


def worst_ratio(got, ref, tol):
    """max over the elements of |got - ref| / tol (inf where got is not finite)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    err = np.where(np.isfinite(err), err, np.inf)
    r = np.where(err == 0, 0.0, err / np.where(tol > 0, tol, TINY * TINY))
    return float(r.max()) if r.size else 0.0


def restated_f32(x, mask, form):
    """The kernels' formulas in float32, one rounding per operation, in the order the vec4 kernel applies them.  form "tanhf": a
    correctly rounded tanh; "exp": 1 - 2 / (1 + 2^(c * 2 log2 e)), the bf16 path.  Results before the rounding to the operand dtype."""
    f = np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        m = None if mask is None else mask.astype(f)
        dh = np.zeros((x.M, x.H), dtype=f)
        if x.op == "maxout":
            for d in x.dh[:2]:
                if d is not None:
                    dh = dh + d
            if m is not None:
                dh = dh * m
        else:
            for i, d in enumerate(x.dh):
                if d is not None:
                    dh = dh + (d * m if (i == 0 and m is not None) else d)
        ds = np.zeros((x.M, x.H), dtype=f)
        for s in (x.slabA, x.slabB):
            if s is not None:
                for t in s:
                    ds = ds + t
        if x.datth is not None:
            dh = x.datth @ x.h2attT.T                      # (f32 accumulation, in numpy's order)
        dh = dh + ds
        c = x.c
        if form == "tanhf" or x.op == "maxout":
            tc = np.tanh(c.astype(np.float64)).astype(f)
        else:
            e = np.exp2(c * f(2.8853900817779268))
            tc = f(1) - f(2) * (f(1) / (e + f(1)))
        g = x.gates
        cp = np.zeros_like(c) if x.c_prev is None else x.c_prev
        if x.op == "maxout":
            gi, gf, go, gg, first = g[:, 0], g[:, 1], g[:, 2], g[:, 3], g[:, 4] > 0.5
        else:
            gi, gf, gg, go = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
        dc = x.dc + dh * go * (f(1) - tc * tc)
        out = {"d_i": dc * gg * gi * (f(1) - gi), "d_f": dc * cp * gf * (f(1) - gf)}
        d_o = dh * tc * go * (f(1) - go)
        if x.op == "maxout":
            dg = dc * gi
            out.update(d_o=d_o, d_g1=np.where(first, dg, f(0)), d_g2=np.where(first, f(0), dg))
        else:
            out.update(d_g=dc * gi * (f(1) - gg * gg), d_o=d_o)
        out["dc"] = dc * gf
    return out


# ---- the cases ----
_MIS4 = ("dh0", "dh1", "dh2", "dc", "c", "c_prev", "slabA", "slabB")
GEN = dict(dh1=((3, 0), (2, 0)), dh2=((2, 0), (0, 0)))                         # lddh1 = 3H from column 2H, lddh2 = 2H (Step::bwd_step)


@functools.lru_cache(maxsize=None)
def cell_cases():
    cs = []

    def add(name, **kw):
        cs.append(Case(name, **kw))
    # launch-geometry edges, each with dh0 alone (simple) and with every kind of source (general)
    for M, H in ((128, 512), (127, 512), (512, 128), (128, 516), (64, 1028), (64, 1030), (65536, 4), (65535, 4), (6, 32), (33, 96)):
        add("shape-%dx%d-simple" % (M, H), M=M, H=H)
        add("shape-%dx%d-general" % (M, H), M=M, H=H, nA=2, nB=3, **GEN)
    add("shape-64x1030-ld1032", M=64, H=1030, dh0=((1, 2), (0, 0)))              # H % 4 != 0 alone: the rows of dh0 keep their alignment
    # source combinations at the first vec4 size
    add("src-dh012", **GEN)
    add("src-no-dh0", dh0=None, dh1=((1, 0), (0, 0)))                          # the t = 0 shape of call: the recurrent source alone
    add("src-no-cprev", cprev="no")
    add("src-none", dh0=None)                                                  # d c alone
    for nA in (1, 2, 4):
        for nB in (0, 3, 4):
            add("slab-%d-%d" % (nA, nB), nA=nA, nB=nB)
    add("slab-att-cell", dh0=((3, 0), (1, 0)), nA=4, layA=((3, 0), (1, 0)), nB=4, layB=((2, 0), (1, 0)))      # the unfused att cell of bwd_step
    add("slab-B-only", nB=2)
    add("slab-general", nA=4, nB=4, **GEN)
    add("slab-nA5", nA=5)
    add("slab-nB5", nB=5, nA=1)
    add("drop-simple", drop_p=0.5, site=SITE_OUT0 + 3)
    add("drop-general", drop_p=0.5, site=SITE_OUT0 + 7, nA=2, **GEN)
    add("drop-strided", drop_p=0.5, site=SITE_OUT0 + 1, dh0=((3, 0), (1, 0)), M=33, H=96)
    # every alignment condition broken alone
    full = dict(nA=2, nB=2, **GEN)
    for t in _MIS4:
        add("mis-%s" % t, shift={t: 4}, **full)
    add("mis-lddh0", dh0=((1, 2), (0, 0)), **full)
    add("mis-lddh1", nA=2, nB=2, dh1=((3, 2), (2, 0)), dh2=GEN["dh2"])
    add("mis-lddh2", nA=2, nB=2, dh1=GEN["dh1"], dh2=((2, 2), (0, 0)))
    add("mis-ldA", layA=((3, 2), (2, 0)), nA=2, nB=2, **GEN)
    add("mis-ldB", layB=((2, 2), (0, 0)), nA=2, nB=2, **GEN)
    add("mis-strideA", strideA=128 * 3 * 512 + 2, nA=2, nB=2, **GEN)
    add("mis-strideB", strideB=128 * 2 * 512 + 2, nA=2, nB=2, **GEN)
    add("mis-gates8", shift={"gates": 8})                                      # bf16 stays vec4, f32 goes scalar
    add("mis-dgates8", shift={"dgates": 8})
    add("mis-gates8-both", shift={"gates": 8, "dgates": 8}, **full)
    add("mis-gates4", shift={"gates": 4})
    add("mis-dgates4", shift={"dgates": 4})
    # saturated gates and cell states; a forget-gate gradient a whole-tensor norm would hide
    add("sat-simple", gscale=8.0, cscale=6.0)
    add("sat-general", gscale=8.0, cscale=6.0, nA=4, nB=4, **GEN)
    add("sat-scalar", gscale=8.0, cscale=6.0, M=33, H=96, nA=2, **GEN)
    add("smallcp-simple", cprev="small")
    add("smallcp-general", cprev="small", nA=2, nB=3, **GEN)
    add("smallcp-scalar", cprev="small", M=33, H=96)
    # slice 1 of slabA begins at byte offset 2^31: beyond what the vec4 kernel's 32-bit buffer offsets reach
    add("far-slabA", nA=2, strideA=2 ** 29, far=True)
    # ... and the same for the other kinds of source: the last of 128 rows begins beyond 2^31 bytes, or the last slice does
    wide = (2 ** 29 // 127 + 4) // 4 * 4
    add("far-dh0", dh0=((0, wide), (0, 0)), far=True)
    add("far-dh1", dh1=((0, wide), (0, 0)), far=True)
    add("far-dh2", dh1=GEN["dh1"], dh2=((0, wide), (0, 0)), far=True)
    add("far-slabB", nA=1, nB=4, strideB=(2 ** 29 + 8) // 3 // 4 * 4 + 4, far=True)
    assert len({c.name for c in cs}) == len(cs)
    return tuple(cs)


@functools.lru_cache(maxsize=None)
def maxout_cases():
    cs = []
    one = ((1, 0), (0, 0))
    for M, H in ((5, 40), (128, 512), (33, 96)):
        cs.append(Case("maxout-%dx%d" % (M, H), op="maxout", M=M, H=H, dh1=one, drop_p=0.5, site=SITE_OUT0 + 2))
    for h0 in (True, False):
        for h1 in (True, False):
            for p in (0.0, 0.5):
                cs.append(Case("maxout-dh%d%d-p%d" % (h0, h1, p * 10), op="maxout", M=33, H=96, dh0=one if h0 else None, dh1=one if h1 else None,
                               drop_p=p, site=SITE_OUT0 + 5))
    cs.append(Case("maxout-no-cprev", op="maxout", M=33, H=96, dh0=None, dh1=one, cprev="no", drop_p=0.5, site=SITE_OUT0))
    cs.append(Case("maxout-sat", op="maxout", M=33, H=96, dh1=one, gscale=8.0, cscale=6.0))
    cs.append(Case("maxout-strided", op="maxout", M=33, H=96, dh0=((3, 0), (1, 0)), dh1=((2, 0), (1, 0)), drop_p=0.5, site=SITE_OUT0 + 9))
    return tuple(cs)


FUSED_N = (1, 31, 32, 33, 65)
FUSED_A = (128, 256, 512)
FUSED_H = (32, 96, 512)
FUSED_SLABS = ((4, 4), (4, 0), (1, 2), (0, 0))
_FUSED_LAY = dict(layA=((3, 0), (1, 0)), layB=((2, 0), (1, 0)))                # slab2 + H at 3H, bp_slab1 + H at 2H (Step::bwd_step)


@functools.lru_cache(maxsize=None)
def fused_cases():
    cs = []

    def add(name, N, H, A, nA, nB, **kw):
        kw = dict(_FUSED_LAY, **kw)
        cs.append(Case(name, op="fused", M=N, H=H, A=A, nA=nA, nB=nB, dtypes=(BF16,), **kw))
    i = 0
    for A in FUSED_A:
        for N in FUSED_N:
            nA, nB = FUSED_SLABS[i % 4]
            add("fused-A%d-N%d" % (A, N), N, FUSED_H[i % 3], A, nA, nB)
            i += 1
    for H in FUSED_H:
        for nA, nB in FUSED_SLABS:
            add("fused-H%d-s%d%d" % (H, nA, nB), 33, H, 512, nA, nB)
    add("fused-no-cprev", 33, 96, 256, 4, 4, cprev="no")
    add("fused-no-cprev-no-slabs", 31, 32, 128, 0, 0, cprev="no")
    add("fused-sat", 65, 96, 512, 4, 4, gscale=8.0, cscale=6.0)
    add("fused-sat-A128", 33, 32, 128, 1, 2, gscale=8.0, cscale=6.0)
    add("fused-smallcp", 65, 96, 256, 4, 0, cprev="small")
    return tuple(cs)


@functools.lru_cache(maxsize=None)
def fused_refused():
    """Calls uic_h2att_cell_bwd must refuse: (case, dtype, the one condition that fails)."""
    def mk(name, N=33, H=96, A=256, nA=2, nB=2, **kw):
        return Case(name, op="fused", M=N, H=H, A=A, nA=nA, nB=nB, **dict(_FUSED_LAY, **kw))
    more = [(mk("refuse-" + t, shift={t: 4}), BF16, t + "_al") for t in ("c", "c_prev", "datth", "h2attT", "gates", "dgates", "slabA", "slabB")]
    more += [(mk("refuse-ldA", layA=((3, 2), (1, 0)), strideA=34 * 290), BF16, "slabA_ld"), (mk("refuse-ldB", layB=((2, 2), (1, 0)), strideB=34 * 194), BF16, "slabB_ld"),
             (mk("refuse-strideA", strideA=33 * 3 * 96 + 2), BF16, "slabA_stride"), (mk("refuse-strideB", strideB=33 * 2 * 96 + 2), BF16, "slabB_stride")]
    return ((mk("refuse-A384", A=384), BF16, "A"), (mk("refuse-A64", A=64), BF16, "A"), (mk("refuse-H48", H=48), BF16, "H32"),
            (mk("refuse-f32"), F32, "dtype"), (mk("refuse-nA5", nA=5), BF16, "nA"), (mk("refuse-nB5", nB=5), BF16, "nB"),
            (mk("refuse-dc", shift={"dc": 4}), BF16, "dc_al")) + tuple(more)


def all_cases():
    return cell_cases() + maxout_cases() + fused_cases()
