"""The nine batch-norm kernels behind uic_batchnorm_* (csrc/batchnorm.hip: bn_stats_part / _final / _running, bn_apply, bn_bwd_part /
_final / _apply, bn_fold_weight, bn_fold_grad) against float64, at the row and column counts where the launch geometry changes and
on the columns the shifted sums and the Chan merge were written for.

Columns cycle through eight profiles (PROFILES): N(0,1); mean 1e3 with std 1e-2 (cancellation); constant 0.75 and constant 0 (the
zero-padded feature columns: variance exactly 0); scale 1e4; mean -7 with std 1e-3; N(0,1) whose first live row is 1000 (the shift K
of its chunk is an outlier); mean 3e2 with std 1.  Dead rows of x, y and d hold NaN and +-inf.  Row counts run over one chunk, the four
waves of the final kernels holding 0 / 1 / 2 chunks, and 32768 | 32769 rows (the last count with 64 rows per chunk, the first with
128); live-row patterns (PATTERNS) put a whole dead chunk, chunks whose first rows are dead, one live row and no live row in front of
them.  Column counts run over the 64-column groups of the final kernels and the second blockIdx.x of the part kernels, and one case
each of apply and backward passes the 65536-workgroup cap of the element-wise grids.

References: statistics in float64 numpy; backward and the folds by torch float64 AUTOGRAD (F.batch_norm on the live rows, a double
Linear for the folds), so the hand-derived backward formulas are not restated; `rep` by replicating the rows; bf16 operands are
rounded to bf16 first, so both sides see the same numbers.  The backward tests take `stat` from the float64 reference rounded to
f32, not from the forward kernel.  One test chains stats -> apply -> fold_weight -> backward -> fold_grad against the autograd of
Linear(BatchNorm1d(x)).

Tolerances come from the arithmetic, not from the kernels.  U = 2^-23, so one rounding is U / 2 of its result.  k roundings of
quantities of size s accumulate to at most g(k) s, g(k) = min(k / 2, 2 sqrt(k)) U: the worst case up to k = 16, beyond it the
square-root law of independent roundings at four standard deviations (Higham & Mary's probabilistic bound with lambda = 4) -- the
roundings of a running sum are relative to a partial sum that grows to the total, and the low bits of squares of bf16 numbers are
not independent, so nothing tighter holds up: the float32 restatement in tests/test_batchnorm_bounds_host.py reaches 0.31 of it.
With rpc rows per chunk, nch chunks and m = ceil(nch / 4) + 3 merges on the longest path of the final kernel, per column:
  mean   g(m + 2) max|x| + g(rpc) max|x - mean|: every merge and the chunk mean K + s1 / cnt round a number of the size of the
         mean once; the shifted sum s1 is rpc additions of terms no larger than 2 max|x - mean|, divided by cnt.
  var    g(rpc + m + 4) S2 / n + 2 dm sb + dm^2, with S2 = sum over chunks of sum (x - K)^2, K the chunk's first live row -- the sum
         of positive terms that M2 is cancelled out of, so an outlier K (profile g) widens the bound of its own column only --,
         dm the mean bound above, which enters every between-chunk term n_a n_b / (n_a + n_b) (mean_b - mean_a)^2, and sb the
         standard deviation of the chunk means (Cauchy-Schwarz on the cross term).
  rstd   relative: var bound / (2 (var + eps)) + 2 U (the division and the reciprocal square root).
  running statistics: momentum times the bound of the batch value, plus 3 U of the two terms of the update.
  out    apply reads stat as given, so against the float64 evaluation with the SAME f32 stat: U (3 |gamma xhat| + |out|).
  xhat   with stat rounded to f32: e_x = |f32(mean) - mean| rstd + |xhat| (|f32(rstd) - rstd| / rstd + 2 U).
  dbeta  g(rpc + m) sum |d|;   dgamma  sum |d| e_x + g(rpc + m + 1) sum |d xhat| -- relative to the sum of magnitudes reduced.
  dx     |gamma| rstd ((dbeta bound + (|xhat| + e_x) dgamma bound + e_x |dgamma|) / n) + (rstd rounding + 4 U) |gamma| rstd (|d| +
         (|dbeta| + |xhat dgamma|) / n); eval mode: (rstd rounding + 2 U) |dx|.  The product of the two errors is kept: with two
         live rows of profile b dx is a cancellation to 1e-3 of its terms and the f32 rounding of the mean alone comes to 0.9997
         of this bound.
  folds  Weff U |ref|; beff g(ceil(D / 256) + 11) (|b| + sum_c |W beta|); dgamma g(ceil(H / 4) + 4) sum_h |W dW'| (signed weights:
         the sum cancels, the bound does not follow it); dbeta the same over |W db|; dW 3 U (|dW' gamma| + |db beta|).
  bf16 outputs: one round-to-nearest, 2^-8 |ref|, more.
Constant columns are held exactly: the mean is the constant, bit for bit, and every constant column has the same rstd bits.
tests/test_batchnorm_bounds_host.py evaluates a float32 restatement of the chunked algorithm on the CPU against these bounds (it
stays within half of each) and shows that a plain f32 E[x^2] - E[x]^2 exceeds them on the cancellation profiles.

The worst observed error / bound per kernel and quantity is printed at the end of the module (run with -s; 1.0 would be the bound).
Measured on an MI355X (profiles/LOG.md, "Batch-norm kernels as uic_batchnorm_*"), 210 cases in 5.5 s: bn_stats mean 0.36, rstd 0.44,
run_mean 0.34, run_var 0.44 (f32 input; bf16 0.26 / 0.29 / 0.34 / 0.31); bn_stats_running rstd 0.38; bn_apply 0.49 to f32 (0.50 past
the grid cap), 0.996 to bf16 (the bf16 rounding term); bn_bwd dbeta 0.14, dgamma 0.41 and dx 0.60 with bf16 y, dx in eval mode
0.56, past the grid cap 0.002 / 0.044 / 0.85; with f32 y dgamma and dx reach 1.000 of the bound in the two-row cases, where the
bound is the f32 rounding of `stat` alone, known exactly; bn_fold_weight Weff 0.50 (bf16 0.996), beff 0.08; bn_fold_grad dgamma
0.41, dbeta 0.41, dW 0.31; the chain pre 0.03, dx 0.13, dW 0.19, dbeta 0.15, dgamma 0.003.  The float32 restatement on the CPU:
mean 0.25, rstd 0.28, run_mean 0.28, run_var 0.31.
"""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
BF = 2.0 ** -8
EPS = float(np.float32(1e-5))
MOM = float(np.float32(0.1))
F32, BF16 = 0, 1
PROFILES = "abcdefgh"
NT = 256                       # threads per workgroup in csrc/batchnorm.hip
GRID_CAP = 65536               # workgroups of the element-wise kernels

ROW_EDGES = (1, 2, 63, 64, 65, 255, 256, 257, 32768, 32769)
PATTERNS = (None, "full", "cyc7", "first_dead", "one_live", "dead_chunk")
COL_EDGES = (4, 60, 64, 68, 1024, 1028, 2052)
ROW_CASES = [(nr, p) for nr in ROW_EDGES for p in PATTERNS if p != "dead_chunk" or nr >= 255]
BIG = (32769, 2052)            # NR C / 4 just above 65536 * 256

WORST = {}                     # kernel -> {quantity: worst error / bound}


def _note(kernel, what, ratio):
    d = WORST.setdefault(kernel, {})
    d[what] = max(d.get(what, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print("\n[batchnorm] %-22s worst error / bound: %s" % (k, ", ".join("%s %.3f" % kv for kv in sorted(WORST[k].items()))))


def _L():
    from unpaired_image_captioning_amd import _lib
    return _lib


# ---- the launch geometry of csrc/batchnorm.hip, restated (the chunk count is checked against uic_batchnorm_scratch_floats) ----
def chunks_for(NR):
    rpc = 64
    n = -(-NR // rpc)
    while n > 512:
        rpc *= 2
        n = -(-NR // rpc)
    return n, rpc


def grid_blocks(NR, C):
    return min(GRID_CAP, max(1, -(-(NR * (C // 4)) // NT)))


def row_pattern(NR, pattern):
    """(R, row_len or None) of a live-row pattern; row n * R + r is live iff r < row_len[n]."""
    if pattern is None:
        return 1, None
    R = {"full": 7, "cyc7": 7, "one_live": 7, "first_dead": 3, "dead_chunk": 36}[pattern]
    n_img = -(-NR // R)
    i = np.arange(n_img)
    if pattern == "full":
        rl = np.full(n_img, R)
    elif pattern == "cyc7":
        rl = (i + 3) % 8                                   # 3, 4, ..., 7, 0, 1, 2, ...: every length 0...7
    elif pattern == "first_dead":
        rl = np.array([0, 1, 3, 2])[i % 4]                 # rows 0..2 dead: chunk 0 starts dead
    elif pattern == "one_live":
        rl = np.zeros(n_img)
        rl[n_img // 2] = 1
    else:
        rl = 1 + (i * 5) % R                               # 1...36
        rpc = chunks_for(NR)[1]
        for first in (0, 9 * rpc):                         # chunk 0 and chunk 9: 9 * 64 = 16 * 36, 9 * 128 = 32 * 36
            k = first // R
            n_dead = -(-(rpc + first - k * R) // R)        # the neighbouring images that cover the chunk: 2 (4 with 128 rows)
            if (k + n_dead) * R <= NR:
                rl[k:k + n_dead] = 0
    return R, rl.astype(np.int32)


def live_mask(NR, R, row_len):
    if row_len is None:
        return np.ones(NR, dtype=bool)
    r = np.arange(NR)
    return (r % R) < row_len[r // R]


def profile_columns(rng, rows, C):
    """[rows, C] float64 draws, column c of profile PROFILES[c % 8]."""
    z = rng.standard_normal((rows, C))
    x = np.empty((rows, C))
    for c in range(C):
        p = PROFILES[c % 8]
        x[:, c] = {"a": z[:, c], "b": 1e3 + 1e-2 * z[:, c], "c": 0.75, "d": 0.0, "e": 1e4 * z[:, c], "f": -7 + 1e-3 * z[:, c],
                   "g": z[:, c], "h": 3e2 + z[:, c]}[p]
    return x


def round_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def poison(a, dead):
    """Dead rows hold NaN, +inf and -inf."""
    rows = np.nonzero(dead)[0]
    if rows.size:
        bad = np.array([np.nan, np.inf, -np.inf], dtype=a.dtype)
        a[rows] = bad[(rows[:, None] + np.arange(a.shape[1])[None, :]) % 3]
    return a


class Case:
    """Inputs of one (NR, C, live-row pattern, operand dtype) and their float64 references; built once and never modified."""

    def __init__(self, NR, C, pattern, bf16=False):
        rng = np.random.default_rng(NR * 131 + C * 7 + PATTERNS.index(pattern) + (1000003 if bf16 else 0))
        self.NR, self.C, self.pattern, self.bf16 = NR, C, pattern, bf16
        self.R, self.row_len = row_pattern(NR, pattern)
        self.live = live_mask(NR, self.R, self.row_len)
        self.rows = np.nonzero(self.live)[0]
        self.n = n = int(self.rows.size)
        self.nch, self.rpc = chunks_for(NR)
        self.merges = -(-self.nch // 4) + 3
        x = profile_columns(rng, NR, C).astype(np.float32)
        if n:
            x[self.rows[0], 6::8] = 1000.0                 # profile g: the first live row, the shift K of its chunk, is an outlier
        if bf16:
            x = round_bf16(x)
        self.x = poison(x, ~self.live)                     # f32 values (bf16-representable when bf16)
        xl = self.xl = x[self.rows].astype(np.float64)
        # float64 statistics of the live rows
        self.mean = xl.mean(0) if n else np.zeros(C)
        self.M2 = ((xl - self.mean) ** 2).sum(0) if n else np.zeros(C)
        self.var = self.M2 / max(n, 1)
        self.rstd = 1.0 / np.sqrt(self.var + EPS)
        self.maxabs = np.abs(xl).max(0) if n else np.zeros(C)
        self.dev = np.abs(xl - self.mean).max(0) if n else np.zeros(C)
        # what the bounds need of the chunks: sum (x - K)^2 with K the chunk's first live row, and the spread of the chunk means
        self.chunk_live = np.bincount(self.rows // self.rpc, minlength=self.nch)
        if n:
            _, first, inv, cnt = np.unique(self.rows // self.rpc, return_index=True, return_inverse=True, return_counts=True)
            self.S2 = ((xl - xl[first][inv]) ** 2).sum(0)
            mb = np.add.reduceat(xl, first, axis=0) / cnt[:, None]
            self.sigma_b = np.sqrt((cnt[:, None] * (mb - self.mean) ** 2).sum(0) / n)
        else:
            self.S2 = self.sigma_b = np.zeros(C)
        self.constant = self.dev == 0                      # profiles c and d, and every column when one row is live
        # d out, gamma, beta and the running statistics the tests start from
        self.gamma = (rng.standard_normal(C) + np.where(np.arange(C) % 2, 1.5, -1.5)).astype(np.float32)        # both signs
        self.beta = rng.standard_normal(C).astype(np.float32)
        self.rm0 = (3 * rng.standard_normal(C)).astype(np.float32)
        self.rv0 = (0.5 + rng.random(C)).astype(np.float32)
        d = (rng.standard_normal((NR, C)) * (0.1 + np.arange(C) % 3)).astype(np.float32)
        self.d = poison(d, ~self.live)
        self.stat32 = np.concatenate([self.mean, self.rstd]).astype(np.float32)

    def var_unbiased(self, rep):
        """The variance nn.BatchNorm1d feeds its running_var when every row is there `rep` times; biased when n rep <= 1."""
        return self.M2 * rep / (self.n * rep - 1) if self.n * rep > 1 else self.var

    def dev_x(self):
        t = torch.from_numpy(self.x).cuda()
        return t.bfloat16() if self.bf16 else t

    def dev_row_len(self):
        return None if self.row_len is None else torch.from_numpy(self.row_len).cuda()


@functools.lru_cache(maxsize=None)
def case(NR, C, pattern, bf16=False):
    return Case(NR, C, pattern, bf16)


# ---- bounds (module docstring); arrays may be numpy or torch ----
def g(k):
    return min(k / 2.0, 2.0 * math.sqrt(k)) * U


def mean_tol(c):
    return g(c.merges + 2) * c.maxabs + g(min(c.rpc, c.NR)) * c.dev


def var_tol(c):
    dm = mean_tol(c)
    return g(min(c.rpc, c.NR) + c.merges + 4) * c.S2 / max(c.n, 1) + 2 * dm * c.sigma_b + dm * dm


def rstd_rtol(c):
    return 0.5 * var_tol(c) / (c.var + EPS) + 2 * U


def run_mean_tol(c):
    return MOM * mean_tol(c) + 3 * U * (abs((1 - MOM) * c.rm0) + MOM * abs(c.mean))


def run_var_tol(c, rep):
    nr = c.n * rep
    return MOM * var_tol(c) * (nr / (nr - 1.0) if nr > 1 else 1.0) + 3 * U * (abs((1 - MOM) * c.rv0) + MOM * c.var_unbiased(rep))


def apply_tol(gxh, ref, bf16_out):
    return U * (3 * abs(gxh) + abs(ref)) + (BF * abs(ref) if bf16_out else 0.0)


def xhat_err(xhat, rstd, e_mean, e_rstd):
    return e_mean * rstd * (1 + e_rstd + 2 * U) + abs(xhat) * (e_rstd + 2 * U)


def bwd_tols(d, xhat, rstd, e_mean, e_rstd, gamma, n, rpc, merges, dbeta, dgamma):
    """(dbeta, dgamma, dx in training, dx in eval) bounds; d and xhat are the live rows, the rest per column."""
    ex = xhat_err(xhat, rstd, e_mean, e_rstd)
    t_db = g(rpc + merges) * abs(d).sum(0)
    t_dg = (abs(d) * ex).sum(0) + g(rpc + merges + 1) * abs(d * xhat).sum(0)
    s = abs(gamma) * rstd
    t_dx = s * (t_db + (abs(xhat) + ex) * t_dg + ex * abs(dgamma)) / n + (e_rstd + 4 * U) * s * (abs(d) + (abs(dbeta) + abs(xhat * dgamma)) / n)
    t_ev = (e_rstd + 2 * U) * s * abs(d)
    return t_db, t_dg, t_dx, t_ev


def fold_tols(W, gamma, beta, b, dWp, db):
    """float64 torch tensors -> bounds of (Weff, beff, dgamma, dbeta, dW)."""
    H, D = W.shape
    return (U * (W * gamma).abs(), g(-(-D // NT) + 11) * (b.abs() + (W * beta).abs().sum(1)),
            g(-(-H // 4) + 4) * (W * dWp).abs().sum(0), g(-(-H // 4) + 4) * (W * db[:, None]).abs().sum(0),
            3 * U * ((dWp * gamma).abs() + (db[:, None] * beta).abs()))


def _ratio(err, tol):
    """max err / tol over the entries (0 / 0 counts as 0: an exact value with a zero bound)."""
    err, tol = np.asarray(err, dtype=np.float64), np.broadcast_to(np.asarray(tol, dtype=np.float64), np.shape(err))
    if err.size == 0:
        return 0.0
    assert not np.isnan(err).any()
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / tol)
    return float(r.max())


def _hold(kernel, what, got, ref, tol, ctx=()):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.isfinite(got).all(), (kernel, what) + tuple(ctx)
    r = _ratio(np.abs(got - ref), tol)
    _note(kernel, what, r)
    if r > 1.0:
        err = np.abs(got - ref) / np.maximum(np.broadcast_to(tol, got.shape), 1e-300)
        w = np.unravel_index(int(np.argmax(err)), got.shape)
        raise AssertionError((kernel, what, r, w, float(got[w]), float(ref[w])) + tuple(ctx))


# ---- launches: fresh outputs every time, every launch twice (bit-equal) ----
def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def scratch_floats(NR, C):
    return int(_L().load().uic_batchnorm_scratch_floats(NR, C))


def launch_stats(c, x, rl, rep=1, running=True):
    L = _L()
    part = torch.full((scratch_floats(c.NR, c.C),), float("nan"), device="cuda")
    stat = torch.full((2 * c.C,), -77.0, device="cuda")
    rm, rv = (_t(c.rm0), _t(c.rv0)) if running else (None, None)
    L.check(L.load().uic_batchnorm_stats(BF16 if c.bf16 else F32, L.ptr(x), c.NR, c.R, c.C, L.ptr(rl), L.ptr(part), MOM, EPS, rep, L.ptr(stat),
                                         L.ptr(rm), L.ptr(rv), L.stream()), "batchnorm_stats")
    torch.cuda.synchronize()
    return {"stat": stat.cpu().numpy(), "rm": rm.cpu().numpy() if running else None, "rv": rv.cpu().numpy() if running else None}


def launch_apply(c, x, rl, stat, gamma, beta, zero_padded, out_bf16):
    L = _L()
    out = torch.full((c.NR, c.C), 7.0, device="cuda", dtype=torch.bfloat16 if out_bf16 else torch.float32)
    L.check(L.load().uic_batchnorm_apply(BF16 if c.bf16 else F32, BF16 if out_bf16 else F32, L.ptr(x), c.NR, c.R, c.C, L.ptr(rl), L.ptr(stat),
                                         L.ptr(gamma), L.ptr(beta), zero_padded, L.ptr(out), L.stream()), "batchnorm_apply")
    torch.cuda.synchronize()
    return {"out": out}


def launch_backward(c, d0, y, rl, stat, gamma, training, want_grads=True):
    L = _L()
    d = d0.clone()
    part = torch.full((scratch_floats(c.NR, c.C),), float("nan"), device="cuda")
    red = torch.full((3 * c.C,), -77.0, device="cuda")
    dg = torch.full((c.C,), -77.0, device="cuda") if want_grads else None
    db = torch.full((c.C,), -77.0, device="cuda") if want_grads else None
    L.check(L.load().uic_batchnorm_backward(BF16 if c.bf16 else F32, L.ptr(d), L.ptr(y), c.NR, c.R, c.C, L.ptr(rl), L.ptr(stat), L.ptr(gamma),
                                            training, L.ptr(part), L.ptr(red), L.ptr(dg), L.ptr(db), L.stream()), "batchnorm_backward")
    torch.cuda.synchronize()
    return {"d": d, "red": red, "dgamma": dg, "dbeta": db}


def twice(fn, *a, **k):
    """Every launch is repeated once on fresh outputs: the results must be bit-equal (NaN-free outputs; raw bits compared)."""
    one, two = fn(*a, **k), fn(*a, **k)
    for key, v in one.items():
        if v is None:
            continue
        if isinstance(v, np.ndarray):
            assert v.tobytes() == two[key].tobytes(), (fn.__name__, key)
        else:
            bits = torch.int16 if v.dtype == torch.bfloat16 else torch.int32
            assert torch.equal(v.view(bits), two[key].view(bits)), (fn.__name__, key)
    return one


# ---- the edges are reached ----
def test_the_cases_reach_every_branch_of_the_launch_geometry():
    assert chunks_for(32768) == (512, 64) and chunks_for(32769) == (257, 128)          # the last count with 64 rows per chunk, the first with 128
    assert [chunks_for(n)[0] for n in (1, 64, 65, 255, 256, 257)] == [1, 1, 2, 4, 4, 5]  # the final kernel's waves get 0, 1 and 2 chunks
    for NR, C in [(nr, 8) for nr in ROW_EDGES] + [(130, cc) for cc in COL_EDGES] + [BIG]:
        assert scratch_floats(NR, C) == chunks_for(NR)[0] * 3 * C, (NR, C)              # (the library's own chunk count)
    assert grid_blocks(*BIG) == GRID_CAP and BIG[0] * BIG[1] // 4 > GRID_CAP * NT        # the grid-stride loops take a second trip
    assert grid_blocks(32769, 16) < GRID_CAP
    assert max(COL_EDGES) // 4 > 2 * NT and 1028 // 4 > NT >= 1024 // 4                 # 1, 2 and 3 blockIdx.x of the part kernels
    assert {cc % 64 for cc in COL_EDGES} >= {0, 4, 60}                                  # the final kernels' 64-column groups


@pytest.mark.parametrize("NR", [n for n in ROW_EDGES if n >= 255])
def test_the_dead_chunk_pattern_holds_a_dead_chunk(NR):
    c = case(NR, 8, "dead_chunk")
    assert c.R == 36
    dead = np.nonzero(c.chunk_live == 0)[0]
    assert 0 in dead, dead                                              # wave 0 starts from n = 0 and meets n_b = 0
    assert NR < 10 * c.rpc + 2 * 36 or 9 in dead, dead                  # ... and again in the middle of wave 1's chunks
    zero = np.nonzero(c.row_len == 0)[0]
    assert (np.diff(zero) == 1).any()                                   # neighbouring images of length 0
    first_rows = np.arange(c.nch) * c.rpc
    assert ((~c.live[first_rows]) & (c.chunk_live > 0)).any()           # a chunk whose first rows are dead but which has live rows
    assert 0 < c.n < NR


def test_the_other_patterns_are_what_they_say():
    for NR in ROW_EDGES:
        c = case(NR, 8, "cyc7")
        assert set(c.row_len.tolist()) == set(range(8)) or NR < 56
        assert case(NR, 8, "one_live").n == 1
        assert case(NR, 8, "full").n == NR and case(NR, 8, None).n == NR
        f = case(NR, 8, "first_dead")
        assert not f.live[0] and (f.n > 0 or NR <= 3)
    assert case(1, 8, "first_dead").n == 0 and case(2, 8, "cyc7").n == 2          # no live row at all; a partial last image


# ---- statistics ----
def check_stats(c, out, rep, running):
    k = "bn_stats[%s]" % ("bf16" if c.bf16 else "f32")
    C_ = c.C
    mean, rstd = out["stat"][:C_], out["stat"][C_:]
    ctx = (c.NR, c.C, c.pattern, rep)
    if c.n == 0:
        assert (mean == 0).all() and (rstd == rstd[0]).all(), ctx
    # constant columns: the mean is the constant bit for bit, and the variance is exactly 0 (every such column has the same rstd bits)
    cc = c.constant
    assert (mean[cc].astype(np.float64) == c.mean[cc]).all(), ctx + ("constant mean",)
    assert np.unique(rstd[cc].view(np.int32)).size <= 1, ctx + ("constant rstd",)
    _hold(k, "mean", mean, c.mean, mean_tol(c), ctx)
    _hold(k, "rstd", rstd, c.rstd, rstd_rtol(c) * c.rstd, ctx)
    if running:
        _hold(k, "run_mean", out["rm"], (1 - MOM) * c.rm0.astype(np.float64) + MOM * c.mean, run_mean_tol(c), ctx)
        _hold(k, "run_var", out["rv"], (1 - MOM) * c.rv0.astype(np.float64) + MOM * c.var_unbiased(rep), run_var_tol(c, rep), ctx)


def run_stats_case(NR, C_, pattern):
    for bf16 in (False, True):
        c = case(NR, C_, pattern, bf16)
        x, rl = c.dev_x(), c.dev_row_len()
        base = None
        for rep, running in ((1, True), (5, True), (1, False)):
            out = twice(launch_stats, c, x, rl, rep, running)
            check_stats(c, out, rep, running)
            if base is None:
                base = out
            assert out["stat"].tobytes() == base["stat"].tobytes()                # rep and the running pointers do not touch stat
        if pattern == "full":
            none = twice(launch_stats, c, x, None, 1, True)                        # row_len all equal to R == no row_len, bit for bit
            for key in ("stat", "rm", "rv"):
                assert none[key].tobytes() == base[key].tobytes(), key


@pytest.mark.parametrize("NR,pattern", ROW_CASES, ids=["%d-%s" % c for c in ROW_CASES])
def test_stats_row_edges_against_float64(NR, pattern):
    run_stats_case(NR, 8, pattern)


@pytest.mark.parametrize("C_", COL_EDGES)
def test_stats_column_edges_against_float64(C_):
    run_stats_case(130, C_, "cyc7")
    run_stats_case(130, C_, None)


def test_rep_is_what_replicated_rows_give():
    """rep = 5 against nn.BatchNorm1d-style statistics of the rows replicated five times, in float64."""
    c = case(65, 8, "cyc7")
    x5 = np.repeat(c.xl, 5, axis=0)
    np.testing.assert_allclose(x5.mean(0), c.mean, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(x5.var(0, ddof=1), c.var_unbiased(5), rtol=1e-9, atol=1e-18)
    np.testing.assert_allclose(x5.var(0), c.var, rtol=1e-9, atol=1e-18)
    t = torch.from_numpy(x5)
    rv = torch.ones(c.C, dtype=torch.float64)
    torch.nn.functional.batch_norm(t, torch.zeros(c.C, dtype=torch.float64), rv, training=True, momentum=1.0, eps=EPS)
    np.testing.assert_allclose(rv.numpy(), c.var_unbiased(5), rtol=1e-9, atol=1e-18)
    out = twice(launch_stats, c, c.dev_x(), c.dev_row_len(), 5, True)
    check_stats(c, out, 5, True)


def test_one_live_row_follows_the_stated_contract():
    """nn.BatchNorm1d refuses one value per channel in training; include/uic_hip.h says: mean = the row, variance 0, and run_var takes
    the biased variance (0) when n rep <= 1, the unbiased one (also 0) otherwise."""
    c = case(257, 8, "one_live")
    assert c.n == 1 and c.constant.all()
    for rep in (1, 5):
        out = twice(launch_stats, c, c.dev_x(), c.dev_row_len(), rep, True)
        assert (out["stat"][:c.C].astype(np.float64) == c.xl[0]).all()
        assert np.abs(out["stat"][c.C:] / EPS ** -0.5 - 1).max() <= 2 * U
        _hold("bn_stats[f32]", "run_var", out["rv"], (1 - MOM) * c.rv0.astype(np.float64), 3 * U * c.rv0)


def test_stats_running_against_float64():
    for C_ in (4, 260, 1028):
        rng = np.random.default_rng(C_)
        rm, rv = rng.standard_normal(C_).astype(np.float32), (rng.random(C_) * np.where(np.arange(C_) % 3, 1.0, 0.0)).astype(np.float32)
        L = _L()

        def launch():
            stat, drm, drv = torch.full((2 * C_,), -77.0, device="cuda"), _t(rm), _t(rv)
            L.check(L.load().uic_batchnorm_stats_running(L.ptr(drm), L.ptr(drv), C_, EPS, L.ptr(stat), L.stream()), "stats_running")
            return {"stat": stat.cpu().numpy()}
        out = twice(launch)["stat"]
        assert (out[:C_] == rm).all()
        ref = 1 / np.sqrt(rv.astype(np.float64) + EPS)
        _hold("bn_stats_running", "rstd", out[C_:], ref, 2 * U * ref)


# ---- apply ----
def run_apply_case(NR, C_, pattern, combos=((False, False), (False, True), (True, False), (True, True))):
    for in_bf16, out_bf16 in combos:
        c = case(NR, C_, pattern, in_bf16)
        x, rl, stat = c.dev_x(), c.dev_row_len(), _t(c.stat32)
        m, r = c.stat32[:C_].astype(np.float64), c.stat32[C_:].astype(np.float64)
        xh = (c.xl - m) * r
        k = "bn_apply[%s->%s]" % ("bf16" if in_bf16 else "f32", "bf16" if out_bf16 else "f32")
        for affine, zero_padded in ((True, 1), (False, 1), (True, 0)):
            ga, be = (c.gamma, c.beta) if affine else (None, None)
            out = twice(launch_apply, c, x, rl, stat, _t(ga), _t(be), zero_padded, out_bf16)["out"].float().cpu().numpy()
            gxh = xh * ga if affine else xh
            ref = gxh + be if affine else gxh
            _hold(k, "out", out[c.rows], ref, apply_tol(gxh, ref, out_bf16), (NR, C_, pattern, affine, zero_padded))
            if zero_padded:
                assert (out[~c.live] == 0).all(), (NR, C_, pattern)                # dead rows are written as zeros, never read
            if not affine:
                assert (out[c.rows][:, c.constant] == 0).all()                     # xhat of a constant column is exactly 0


@pytest.mark.parametrize("NR,pattern", ROW_CASES, ids=["%d-%s" % c for c in ROW_CASES])
def test_apply_row_edges_against_float64(NR, pattern):
    run_apply_case(NR, 8, pattern)


@pytest.mark.parametrize("C_", COL_EDGES)
def test_apply_column_edges_against_float64(C_):
    run_apply_case(130, C_, "cyc7", combos=((False, True), (True, False)))


# ---- backward ----
def autograd_bn(xl, dl, gamma, beta, training, mean=None, var=None):
    """dx, dgamma, dbeta of F.batch_norm in float64 on the live rows (torch tensors, any device)."""
    x = xl.clone().requires_grad_(True)
    ga, be = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    if training:
        out = torch.nn.functional.batch_norm(x, None, None, ga, be, training=True, eps=EPS)
    else:
        out = torch.nn.functional.batch_norm(x, mean, var, ga, be, training=False, eps=EPS)
    out.backward(dl)
    return x.grad, ga.grad, be.grad


def contract_bn(xl, dl, gamma, mean, rstd, n):
    """The header's formula in float64, for the batch F.batch_norm refuses (one live row)."""
    xhat = (xl - mean) * rstd
    dbeta, dgamma = dl.sum(0), (dl * xhat).sum(0)
    return gamma * rstd * (dl - (dbeta + xhat * dgamma) / n), dgamma, dbeta


def run_backward_case(NR, C_, pattern):
    for bf16 in (False, True):
        c = case(NR, C_, pattern, bf16)
        k = "bn_bwd[%s]" % ("bf16" if bf16 else "f32")
        y, rl, stat, d0, gamma = c.dev_x(), c.dev_row_len(), _t(c.stat32), _t(c.d), _t(c.gamma)
        dl = c.d[c.rows].astype(np.float64)
        m32, r32 = c.stat32[:C_].astype(np.float64), c.stat32[C_:].astype(np.float64)
        e_mean, e_rstd = np.abs(m32 - c.mean), np.abs(r32 - c.rstd) / c.rstd
        xhat = (c.xl - c.mean) * c.rstd
        ga64 = c.gamma.astype(np.float64)
        for training in (1, 0):
            out = twice(launch_backward, c, d0, y, rl, stat, gamma, training)
            dx = out["d"].cpu().numpy()
            assert (dx[~c.live] == 0).all(), (NR, C_, pattern)                       # dead rows of d are written as zeros
            red = out["red"].cpu().numpy()
            assert (red[:C_] == c.n).all()
            assert red[C_:2 * C_].tobytes() == out["dbeta"].cpu().numpy().tobytes() and red[2 * C_:].tobytes() == out["dgamma"].cpu().numpy().tobytes()
            if c.n == 0:
                assert (red == 0).all()
                continue
            T = torch.from_numpy
            if training and c.n == 1:
                rdx, rdg, rdb = contract_bn(c.xl, dl, ga64, c.mean, c.rstd, 1)
            else:
                rdx, rdg, rdb = (t.numpy() for t in autograd_bn(T(c.xl), T(dl), T(ga64), T(c.beta.astype(np.float64)), bool(training),
                                                                 T(c.mean), T(c.var)))
            t_db, t_dg, t_dx, t_ev = bwd_tols(dl, xhat, c.rstd, e_mean, e_rstd, ga64, c.n, min(c.rpc, NR), c.merges, rdb, rdg)
            ctx = (NR, C_, pattern, training)
            _hold(k, "dbeta", red[C_:2 * C_], rdb, t_db, ctx)
            _hold(k, "dgamma", red[2 * C_:], rdg, t_dg, ctx)
            _hold(k, "dx" if training else "dx(eval)", dx[c.rows], rdx, t_dx if training else t_ev, ctx)
            assert (red[2 * C_:][c.constant & (e_mean == 0)] == 0).all()             # xhat exactly 0 -> dgamma exactly 0
        a = twice(launch_backward, c, d0, y, rl, stat, gamma, 1, want_grads=False)         # dgamma / dbeta may be null
        assert a["red"].cpu().numpy().tobytes() == red.tobytes()                           # (red does not depend on `training`)
        if pattern == "full":
            b = launch_backward(c, d0, y, None, stat, gamma, 1)                            # row_len all R == no row_len, bit for bit
            for key in ("d", "red"):
                assert torch.equal(a[key], b[key]), key


@pytest.mark.parametrize("NR,pattern", ROW_CASES, ids=["%d-%s" % c for c in ROW_CASES])
def test_backward_row_edges_against_float64_autograd(NR, pattern):
    run_backward_case(NR, 8, pattern)


@pytest.mark.parametrize("C_", COL_EDGES)
def test_backward_column_edges_against_float64_autograd(C_):
    run_backward_case(130, C_, "cyc7")


# ---- the grid cap: NR C / 4 > 65536 * 256, references in float64 on the device ----
@functools.lru_cache(maxsize=1)
def big_case():
    NR, C_ = BIG
    R, row_len = row_pattern(NR, "dead_chunk")
    live = live_mask(NR, R, row_len)
    gen = torch.Generator(device="cuda").manual_seed(11)
    z = torch.randn(NR, C_, device="cuda", generator=gen)
    col = torch.arange(C_, device="cuda") % 8
    scale = torch.tensor([1, 1e-2, 0, 0, 1e4, 1e-3, 1, 1], device="cuda")[col]
    shift = torch.tensor([0, 1e3, 0.75, 0, 0, -7, 0, 3e2], device="cuda")[col]
    x = z * scale + shift
    rows = torch.from_numpy(np.nonzero(live)[0]).cuda()
    x[rows[0], 6::8] = 1000.0
    d = torch.randn(NR, C_, device="cuda", generator=gen) * (0.1 + (torch.arange(C_, device="cuda") % 3))
    dead = torch.from_numpy(np.nonzero(~live)[0]).cuda()
    x[dead] = float("nan")
    x[dead[1::2]] = float("inf")
    d[dead] = float("-inf")
    d[dead[::3]] = float("nan")
    xl = x[rows].double()
    mean = xl.mean(0)
    var = ((xl - mean) ** 2).mean(0)
    rstd = (var + EPS).rsqrt()
    gamma = torch.randn(C_, device="cuda", generator=gen) + torch.where(col % 2 == 1, 1.5, -1.5)
    beta = torch.randn(C_, device="cuda", generator=gen)
    return dict(NR=NR, C=C_, R=R, rl=torch.from_numpy(row_len).cuda(), live=torch.from_numpy(live).cuda(), rows=rows, x=x, d=d, mean=mean,
                var=var, rstd=rstd, stat=torch.cat([mean, rstd]).float(), gamma=gamma, beta=beta, n=int(rows.numel()))


class _Shape:
    def __init__(self, b):
        self.NR, self.C, self.R, self.bf16 = b["NR"], b["C"], b["R"], False


def _hold_dev(kernel, what, got, ref, tol):
    assert torch.isfinite(got).all(), (kernel, what)
    err = (got.double() - ref).abs()
    r = float(torch.where(err == 0, torch.zeros_like(err), err / tol).max())
    _note(kernel, what, r)
    assert r <= 1.0, (kernel, what, r)


def test_apply_past_the_grid_cap():
    b = big_case()
    assert grid_blocks(b["NR"], b["C"]) == GRID_CAP < -(-(b["NR"] * b["C"] // 4) // NT)
    out = twice(launch_apply, _Shape(b), b["x"], b["rl"], b["stat"], b["gamma"], b["beta"], 1, False)["out"]
    assert (out[~b["live"]] == 0).all()
    m, r = b["stat"][:b["C"]].double(), b["stat"][b["C"]:].double()
    gxh = (b["x"][b["rows"]].double() - m) * r * b["gamma"].double()
    ref = gxh + b["beta"].double()
    _hold_dev("bn_apply[f32->f32]", "out (grid cap)", out[b["rows"]], ref, apply_tol(gxh, ref, False))


def test_backward_past_the_grid_cap():
    b = big_case()
    C_, n = b["C"], b["n"]
    nch, rpc = chunks_for(b["NR"])
    assert grid_blocks(b["NR"], C_) == GRID_CAP < -(-(b["NR"] * C_ // 4) // NT) and (nch, rpc) == (257, 128)
    out = twice(launch_backward, _Shape(b), b["d"], b["x"], b["rl"], b["stat"], b["gamma"], 1)
    assert (out["d"][~b["live"]] == 0).all()
    xl, dl = b["x"][b["rows"]].double(), b["d"][b["rows"]].double()
    rdx, rdg, rdb = autograd_bn(xl, dl, b["gamma"].double(), b["beta"].double(), True)
    e_mean = (b["stat"][:C_].double() - b["mean"]).abs()
    e_rstd = (b["stat"][C_:].double() - b["rstd"]).abs() / b["rstd"]
    xhat = (xl - b["mean"]) * b["rstd"]
    t_db, t_dg, t_dx, _ = bwd_tols(dl, xhat, b["rstd"], e_mean, e_rstd, b["gamma"].double(), n, rpc, -(-nch // 4) + 3, rdb, rdg)
    k = "bn_bwd[f32]"
    _hold_dev(k, "dbeta (grid cap)", out["red"][C_:2 * C_], rdb, t_db)
    _hold_dev(k, "dgamma (grid cap)", out["red"][2 * C_:], rdg, t_dg)
    _hold_dev(k, "dx (grid cap)", out["d"][b["rows"]], rdx, t_dx)


# ---- the folds ----
FOLD_SHAPES = [(1, 1), (3, 63), (4, 64), (5, 65), (512, 63), (512, 261), (3, 2053), (5, 2053), (1, 261), (4, 1)]


def fold_inputs(H, D):
    gen = torch.Generator().manual_seed(H * 4099 + D)
    r = lambda *s: torch.randn(*s, generator=gen)                                         # noqa: E731
    return dict(W=r(H, D), gamma=r(D) + 0.5, beta=r(D), b=r(H), dWp=r(H, D) * 3, db=r(H))     # signed: sum_h W dW' cancels


def fold_reference(f):
    """Autograd in float64 through the fold itself: L = <Weff, dW'> + <beff, db> has dL/dWeff = dW', dL/dbeff = db."""
    W, gamma, beta = (f[k].double().requires_grad_(True) for k in ("W", "gamma", "beta"))
    b, dWp, db = f["b"].double(), f["dWp"].double(), f["db"].double()
    Weff, beff = W * gamma, b + torch.nn.functional.linear(beta, W)
    ((Weff * dWp).sum() + (beff * db).sum()).backward()
    return Weff.detach(), beff.detach(), gamma.grad, beta.grad, W.grad


@pytest.mark.parametrize("H,D", FOLD_SHAPES)
def test_folds_against_float64_autograd(H, D):
    L = _L()
    f = fold_inputs(H, D)
    dev = {k: v.cuda() for k, v in f.items()}
    rWeff, rbeff, rdg, rdb, rdW = fold_reference(f)
    t_W, t_b, t_dg, t_db, t_dW = fold_tols(*(f[k].double() for k in ("W", "gamma", "beta", "b", "dWp", "db")))
    for bf16 in (False, True):
        def launch_w():
            Weff = torch.full((H, D), 7.0, device="cuda", dtype=torch.bfloat16 if bf16 else torch.float32)
            beff = torch.full((H,), -77.0, device="cuda")
            L.check(L.load().uic_batchnorm_fold_weight(BF16 if bf16 else F32, L.ptr(dev["W"]), L.ptr(dev["gamma"]), L.ptr(dev["beta"]), L.ptr(dev["b"]),
                                                       H, D, L.ptr(Weff), L.ptr(beff), L.stream()), "fold_weight")
            torch.cuda.synchronize()
            return {"Weff": Weff, "beff": beff}
        out = twice(launch_w)
        k = "bn_fold_weight[%s]" % ("bf16" if bf16 else "f32")
        _hold(k, "Weff", out["Weff"].float().cpu(), rWeff, t_W + (BF * rWeff.abs() if bf16 else 0), (H, D))
        _hold(k, "beff", out["beff"].cpu(), rbeff, t_b, (H, D))

    def launch_g():
        dW = dev["dWp"].clone()
        dg, db = torch.full((D,), -77.0, device="cuda"), torch.full((D,), -77.0, device="cuda")
        L.check(L.load().uic_batchnorm_fold_grad(L.ptr(dev["W"]), L.ptr(dev["gamma"]), L.ptr(dev["beta"]), L.ptr(dW), L.ptr(dev["db"]), H, D,
                                                 L.ptr(dg), L.ptr(db), L.stream()), "fold_grad")
        torch.cuda.synchronize()
        return {"dW": dW, "dgamma": dg, "dbeta": db}
    out = twice(launch_g)
    _hold("bn_fold_grad", "dgamma", out["dgamma"].cpu(), rdg, t_dg, (H, D))
    _hold("bn_fold_grad", "dbeta", out["dbeta"].cpu(), rdb, t_db, (H, D))
    _hold("bn_fold_grad", "dW", out["dW"].cpu(), rdW, t_dW, (H, D))
    if H >= 512:
        assert float((rdg.abs() / (f["W"].double() * f["dWp"].double()).abs().sum(0)).min()) < 0.05     # dgamma really cancels somewhere


# ---- the chain: Linear(BatchNorm1d(x)) with the affine part folded into the Linear, no extra GEMM ----
def test_chain_matches_autograd_of_linear_of_batchnorm():
    """stats -> apply (xhat, no affine) -> fold_weight -> [pre = xhat Weff^T + beff and its three GEMMs, in float64 on the kernels'
    outputs] -> backward (gamma = 1: the affine part lives in Weff) -> fold_grad, against autograd of Linear(BatchNorm1d(x)) on the
    live rows.  Bounds: the statistics' bounds propagated to first order (e_x = mean bound * rstd + |xhat| rstd bound), the
    per-kernel bounds of this module on top."""
    L = _L()
    NR, C_, H = 130, 8, 5
    c = case(NR, C_, "cyc7")
    gen = torch.Generator().manual_seed(3)
    W, b, G = torch.randn(H, C_, generator=gen), torch.randn(H, generator=gen), torch.randn(c.n, H, generator=gen)
    gamma, beta = torch.from_numpy(c.gamma), torch.from_numpy(c.beta)
    # reference
    x64 = torch.from_numpy(c.xl).requires_grad_(True)
    p64 = [t.double().requires_grad_(True) for t in (gamma, beta, W, b)]
    pre = torch.nn.functional.linear(torch.nn.functional.batch_norm(x64, None, None, p64[0], p64[1], training=True, eps=EPS), p64[2], p64[3])
    (pre * G.double()).sum().backward()
    # the kernels
    x, rl = c.dev_x(), c.dev_row_len()
    stat = torch.from_numpy(twice(launch_stats, c, x, rl, 1, False)["stat"]).cuda()
    xhat = twice(launch_apply, c, x, rl, stat, None, None, 1, False)["out"]
    Weff, beff = torch.empty(H, C_, device="cuda"), torch.empty(H, device="cuda")
    dv = [t.cuda() for t in (W, gamma, beta, b)]
    L.check(L.load().uic_batchnorm_fold_weight(F32, L.ptr(dv[0]), L.ptr(dv[1]), L.ptr(dv[2]), L.ptr(dv[3]), H, C_, L.ptr(Weff), L.ptr(beff),
                                               L.stream()), "fold_weight")
    xh_l = xhat.cpu().double()[c.rows]
    pre_k = xh_l @ Weff.cpu().double().T + beff.cpu().double()
    dWp, db, dxh = G.double().T @ xh_l, G.double().sum(0), G.double() @ Weff.cpu().double()
    d = torch.from_numpy(poison(np.zeros((NR, C_), dtype=np.float32), ~c.live))
    d[c.rows] = dxh.float()
    ones = torch.ones(C_, device="cuda")
    dx = twice(launch_backward, c, d.cuda(), x, rl, stat, ones, 1)["d"].cpu().double()[c.rows]
    dW, db32 = dWp.float().cuda(), db.float().cuda()
    dg, dbt = torch.empty(C_, device="cuda"), torch.empty(C_, device="cuda")
    L.check(L.load().uic_batchnorm_fold_grad(L.ptr(dv[0]), L.ptr(dv[1]), L.ptr(dv[2]), L.ptr(dW), L.ptr(db32), H, C_, L.ptr(dg),
                                             L.ptr(dbt), L.stream()), "fold_grad")
    torch.cuda.synchronize()
    # bounds
    T = torch.from_numpy
    rstd, xh64 = T(c.rstd), (T(c.xl) - T(c.mean)) * T(c.rstd)
    ex = T(mean_tol(c)) * rstd + xh64.abs() * (T(rstd_rtol(c)) + 2 * U)                 # xhat, with the statistics' own bounds
    Wd, Gd, ga, be = W.double(), G.double(), gamma.double(), beta.double()
    t_pre = ex @ (Wd * ga).abs().T + 4 * U * (xh64.abs() @ (Wd * ga).abs().T + (b.double().abs() + (Wd * be).abs().sum(1)))
    _hold("chain", "pre", pre_k, pre.detach(), t_pre)
    t_dWp = Gd.abs().T @ ex + U * (Gd.abs().T @ xh64.abs())
    rdWp = Gd.T @ xh64
    _, _, f_dg, f_db, f_dW = fold_tols(Wd, ga, be, b.double(), rdWp, db)
    _hold("chain", "dgamma", dg.cpu(), p64[0].grad, (Wd.abs() * t_dWp).sum(0) + f_dg + U * (Wd * rdWp).abs().sum(0))     # (+ the f32 cast of dW')
    _hold("chain", "dbeta", dbt.cpu(), p64[1].grad, f_db + U * (Wd * db[:, None]).abs().sum(0))
    _hold("chain", "dW", dW.cpu(), p64[2].grad, t_dWp * ga.abs() + f_dW + U * p64[2].grad.abs())
    np.testing.assert_allclose(db.numpy(), p64[3].grad.numpy(), rtol=1e-12, atol=1e-12)
    dxh64 = Gd @ (Wd * ga)
    e_mean, e_rstd = T(mean_tol(c)), T(rstd_rtol(c))
    one = torch.ones(C_, dtype=torch.float64)
    _, _, t_dx, _ = bwd_tols(dxh64, xh64, rstd, e_mean, e_rstd, one, c.n, c.rpc, c.merges, dxh64.sum(0), (dxh64 * xh64).sum(0))
    dd = 2 * U * dxh64.abs()                                                             # d xhat as the kernel got it: Weff and the cast round it
    _hold("chain", "dx", dx, x64.grad, t_dx + rstd * (dd + dd.mean(0) + xh64.abs() * (dd * xh64.abs()).mean(0)))


# ---- argument errors: refused, and nothing written ----
def test_argument_errors_are_refused_and_write_nothing():
    L = _L()
    lib = L.load()
    NR, C_, R = 10, 8, 5
    x = torch.randn(NR, C_, device="cuda")
    rl = torch.tensor([5, 3], dtype=torch.int32, device="cuda")
    canary = lambda n: torch.full((n,), -77.0, device="cuda")                              # noqa: E731
    part, stat, rm, rv, out, red, dg, db = canary(3 * C_), canary(2 * C_), canary(C_), canary(C_), canary(NR * C_), canary(3 * C_), canary(C_), canary(C_)
    d = canary(NR * C_)
    gamma = torch.ones(C_, device="cuda")
    s, P = L.stream(), L.ptr
    X, RL, PT, ST, O, D_, RD, GA = P(x), P(rl), P(part), P(stat), P(out), P(d), P(red), P(gamma)

    def stats(dt=F32, x=X, NR=NR, R=R, C_=C_, rl=RL, part=PT, rep=1, stat=ST):
        return lib.uic_batchnorm_stats(dt, x, NR, R, C_, rl, part, MOM, EPS, rep, stat, P(rm), P(rv), s)

    def apply(di=F32, do=F32, x=X, NR=NR, R=R, C_=C_, rl=RL, stat=ST, out=O):
        return lib.uic_batchnorm_apply(di, do, x, NR, R, C_, rl, stat, None, None, 1, out, s)

    def bwd(dt=F32, d=D_, y=X, NR=NR, R=R, C_=C_, rl=RL, stat=ST, gamma=GA, part=PT, red=RD):
        return lib.uic_batchnorm_backward(dt, d, y, NR, R, C_, rl, stat, gamma, 1, part, red, P(dg), P(db), s)

    bad = [stats(x=None), stats(part=None), stats(stat=None), stats(NR=0), stats(NR=-3), stats(C_=0), stats(C_=6), stats(C_=-4), stats(R=0),
           stats(R=-1), stats(rep=0), stats(rep=-2), stats(dt=2), stats(dt=-1),
           apply(x=None), apply(stat=None), apply(out=None), apply(NR=0), apply(C_=0), apply(C_=7), apply(R=0), apply(di=3), apply(do=3),
           bwd(d=None), bwd(y=None), bwd(stat=None), bwd(gamma=None), bwd(part=None), bwd(red=None), bwd(NR=0), bwd(C_=0), bwd(C_=2), bwd(R=0),
           bwd(dt=5),
           lib.uic_batchnorm_stats_running(None, P(rv), C_, EPS, ST, s), lib.uic_batchnorm_stats_running(P(rm), None, C_, EPS, ST, s),
           lib.uic_batchnorm_stats_running(P(rm), P(rv), C_, EPS, None, s), lib.uic_batchnorm_stats_running(P(rm), P(rv), 0, EPS, ST, s),
           lib.uic_batchnorm_stats_running(P(rm), P(rv), 6, EPS, ST, s)]
    W, b, Weff, beff = canary(3 * C_), canary(3), canary(3 * C_), canary(3)
    fw = lambda dt=F32, W=P(W), g_=GA, be=GA, b=P(b), H=3, D=C_, We=P(Weff), bf=P(beff): lib.uic_batchnorm_fold_weight(dt, W, g_, be, b, H, D, We, bf, s)   # noqa: E731
    fg = lambda W=P(W), g_=GA, be=GA, dW=P(Weff), db_=P(b), H=3, D=C_, dg_=P(dg), dbt=P(db): lib.uic_batchnorm_fold_grad(W, g_, be, dW, db_, H, D, dg_, dbt, s)   # noqa: E731
    bad += [fw(dt=2), fw(W=None), fw(g_=None), fw(be=None), fw(b=None), fw(We=None), fw(bf=None), fw(H=0), fw(D=0), fw(D=-1),
            fg(W=None), fg(g_=None), fg(be=None), fg(dW=None), fg(db_=None), fg(dg_=None), fg(dbt=None), fg(H=0), fg(D=0)]
    assert all(rc != 0 for rc in bad), bad
    assert lib.uic_last_error_string()
    for bad_size in ((0, 8), (-1, 8), (10, 0), (10, 6)):
        assert lib.uic_batchnorm_scratch_floats(*bad_size) == 0
    torch.cuda.synchronize()
    for t in (part, stat, rm, rv, out, red, dg, db, d, W, b, Weff, beff):
        assert (t == -77.0).all()
    # R is not looked at without a row_len
    assert stats(R=0, rl=None) == 0 and apply(R=-5, rl=None) == 0
    torch.cuda.synchronize()
