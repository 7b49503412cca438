"""The five log-softmax + masked-NLL kernels behind uic_xe_criterion (csrc/criterion.hip: xe_kernel, xe_lds_kernel, xe_reg_kernel,
xe_reg_wide_kernel, xe_big_kernel) against a float64 log_softmax, at the row lengths where uic_xe_launch changes kernel and where a
kernel's last chunk is full, holds one live float4, or holds a single live column.

A model step with random weights spreads the probability flat over the vocabulary, so a kernel that misplaced the last columns of
a long row would move the loss by 1e-4.  Here each row carries a +12 spike on one of the boundary columns (0, 3, 4, 1023, 1024, 4095,
4096, 10239, 10240, V1-5, V1-4, V1-2, V1-1) and the targets cycle through the same columns, so those columns ARE the loss and the
gradient.  Row 1 is scaled to |x| ~ 1e4, row 2 is constant, row 3 holds -inf in a third of its columns, and the padding columns
[V1, ldv) hold NaN and +inf, which the contract says are ignored.

Tolerances come from the arithmetic, not from the kernels: an f32 `max + log(sum)` and the hardware exp's argument rounding give
2e-5 + 4 * 2^-23 * max|finite x_row| per row on log-probabilities and losses, the same bound relative to the probability plus 1e-7
on probabilities, and one round-to-nearest (2^-8 |ref|) more on bf16 gradients.

The worst observed error / bound per kernel and quantity is printed at the end of the module (run with -s; 1.0 would be the
bound).  Measured on an MI355X (profiles/LOG.md, "Criterion kernels moved to csrc/criterion.hip"): d logits 0.95-0.98 of the
bound in every kernel (the bf16 rounding term), log-probabilities 0.23, losses 0.05-0.11.  A float32 evaluation of the same
inputs on the CPU (max, exp, sum, log in f32) stays within 0.24 of the bounds at every shape.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, T = 3, 4
M = N * T
INF = float("inf")
GENERIC, LDS, REG, REG_WIDE, BIG = 0, 1, 2, 3, 4
NAMES = ("xe_kernel", "xe_lds_kernel", "xe_reg_kernel", "xe_reg_wide_kernel", "xe_big_kernel")

REG_SHAPES = [(5, 8), (1021, 1024), (1024, 1024), (1025, 1028), (4093, 4096), (10237, 10240), (10240, 10240)]
WIDE_SHAPES = [(10241, 10244), (12288, 12288), (12289, 12292), (50004, 50048), (53245, 53248), (53248, 53248)]
LONG_SHAPES = [(53249, 53252)]
# log-probabilities wanted: the LDS kernel while the row fits 64 KB (ldv <= 16384), the two-pass kernel beyond
LOGPROB_SHAPES = [((1000, 1000), LDS), ((16381, 16384), LDS), ((16384, 16384), LDS), ((16385, 16388), BIG)]
UNALIGNED_SHAPES = [(1001, 1001), (50, 51)]          # bf16 with ldv % 4 != 0: the generic kernel

# (dtype, (V1, ldv), kernel of the gradient launches, kernel of the log-prob launches or None), the two dtypes of a shape side by side
CASES = []
for _shape in REG_SHAPES:
    CASES += [(1, _shape, REG, None), (0, _shape, GENERIC, None)]
for _shape in WIDE_SHAPES:
    CASES += [(1, _shape, REG_WIDE, None), (0, _shape, GENERIC, None)]
for _shape in LONG_SHAPES:
    CASES += [(1, _shape, BIG, None), (0, _shape, GENERIC, None)]
for _shape, _k in LOGPROB_SHAPES:
    # (the gradient-only launches of these shapes: ldv <= 10240 -> registers, <= 53248 -> wide)
    CASES += [(1, _shape, REG if _shape[1] <= 10240 else REG_WIDE, _k), (0, _shape, GENERIC, GENERIC)]
for _shape in UNALIGNED_SHAPES:
    CASES += [(1, _shape, GENERIC, GENERIC)]


def _case_id(c):
    return "%s-%dx%d-%s" % ("bf16" if c[0] else "f32", c[1][0], c[1][1], NAMES[c[2]] + ("+" + NAMES[c[3]] if c[3] is not None else ""))


WORST = {}          # kernel id -> {quantity: worst error / bound}


def _note(kid, what, ratio):
    d = WORST.setdefault(kid, {})
    d[what] = max(d.get(what, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for kid in sorted(WORST):
        print("\n[criterion] %-20s worst error / bound: %s" % (NAMES[kid], ", ".join("%s %.3f" % kv for kv in sorted(WORST[kid].items()))))


def _L():
    from unpaired_image_captioning_amd import _lib
    return _lib


def boundary_columns(V1):
    """The boundary columns inside [0, V1), highest first (so V1-1 is the first to carry a spike and a target)."""
    s = {0, 3, 4, 1023, 1024, 4095, 4096, 10239, 10240, V1 - 5, V1 - 4, V1 - 2, V1 - 1}
    return sorted((c for c in s if 0 <= c < V1), reverse=True)


class Case:
    """Inputs of one (V1, ldv) and their float64 reference; built once per shape and never modified."""

    def __init__(self, V1, ldv, ties=False):
        g = torch.Generator().manual_seed(V1 * 7 + ldv)
        x = torch.randn(M, V1, generator=g) * 3
        cols = boundary_columns(V1)
        k = len(cols)
        tgt = []
        for m in range(M):
            x[m, cols[m % k]] += 12                 # one boundary column carries almost all of the row's mass
            tgt.append(cols[m % k] if m % 2 == 0 else cols[(7 * m + 3) % k])        # on the spike / somewhere else on the boundary
        x[1] *= 3000
        x[2] = 0.75
        x[3, 1::3] = -INF
        tgt[3] = max(c for c in cols if c % 3 == 0)
        if ties:
            # an exact tie of the maximum between two columns in different chunks, threads and waves: the lowest index wins
            for m, (a, b) in ((4, (3, 4)), (7, (4095, 4096)), (9, (1023, V1 - 1)), (11, (3, 4))):
                if a < V1 and b < V1 and a != b:
                    x[m, a] = x[m, b] = 40.0
                    tgt[m] = a if m != 11 else b     # row 11 aims at the HIGHER column of the tie: not a hit
            tgt[0] = 0                               # (not counted at all)
        raw = list(tgt)
        raw[6], raw[8] = -1, V1                      # outside [0, V1): scored as target 0
        self.V1, self.ldv, self.x = V1, ldv, x
        self.raw = torch.tensor(raw)
        self.eff = torch.tensor([t if 0 <= t < V1 else 0 for t in raw])
        self.mask = torch.ones(M)
        self.mask[5] = self.mask[10] = 0
        self.inv_den = 1.0 / float(self.mask.sum())
        self.scale = torch.tensor([(-1.0) ** m * (0.05 + 0.01 * m) for m in range(M)])      # the self-critical weight, both signs
        full = torch.empty(M, ldv)
        full[:, :V1] = x
        full[:, V1::2] = float("nan")
        full[:, V1 + 1::2] = INF
        self.logits = full
        xd = x.double()
        self.lp = torch.log_softmax(xd, 1)
        self.p = self.lp.exp()
        finite = torch.where(torch.isfinite(x), x.abs(), torch.zeros(())).max(1).values.double()
        self.tol = 2e-5 + 4 * 2.0 ** -23 * finite                                         # per row
        self.row_loss = -self.lp[torch.arange(M), self.eff] * self.mask.double()
        self.onehot = torch.zeros(M, V1, dtype=torch.float64)
        self.onehot[torch.arange(M), self.eff] = 1.0

    def by_position(self, v, ld, col0, fill):
        """[M] values laid out as the library reads them: v[n * ld + col0 + t] for row m = t * N + n."""
        out = torch.full((N, ld), fill, dtype=v.dtype)
        for m in range(M):
            out[m % N, col0 + m // N] = v[m]
        return out


@functools.lru_cache(maxsize=2)
def case(V1, ldv):
    return Case(V1, ldv)


LD_T, COL_T, LD_M, COL_M, LD_S, COL_S, LP_PAD = T + 2, 1, T + 3, 2, T + 1, 1, 3


def launch(c, dtype, grad=True, scale=False, logprobs=False, stats=False, row_map=None, logits=None):
    """One uic_xe_criterion launch on fresh, canary-filled outputs.  Returns (kernel id, outputs on the host).
    `logits`: other rows than the case's; a tensor that is already on the device is passed as it lies (its address included)."""
    L = _L()
    lib = L.load()
    V1, ldv = c.V1, c.ldv
    lg = c.logits if logits is None else logits
    if not lg.is_cuda:
        lg = lg.cuda()
    rows = lg.shape[0]
    tgt = c.by_position(c.raw, LD_T, COL_T, V1 + 99).cuda()
    msk = c.by_position(c.mask, LD_M, COL_M, 1.0).cuda()
    scl = c.by_position(c.scale, LD_S, COL_S, 9.0).cuda() if scale else None
    inv = torch.tensor([c.inv_den], device="cuda")
    d = torch.full((rows, ldv), 7.0, device="cuda", dtype=torch.bfloat16 if dtype else torch.float32) if grad else None
    row_loss = torch.full((rows,), -77.0, device="cuda")
    lp = torch.full((N, T, V1 + LP_PAD), -55.0, device="cuda") if logprobs else None
    st = torch.zeros(2, dtype=torch.int32, device="cuda") if stats else None             # (zeroed before each launch)
    rm = torch.tensor(row_map, dtype=torch.int32, device="cuda") if row_map is not None else None
    kid = C.c_int32(-1)
    L.check(lib.uic_xe_criterion(dtype, rows, N, V1, ldv, L.ptr(lg), L.ptr(d), L.ptr(tgt), LD_T, COL_T, L.ptr(msk), LD_M, COL_M, L.ptr(inv),
                                 L.ptr(scl), LD_S, COL_S, L.ptr(row_loss), L.ptr(lp), V1 + LP_PAD, T * (V1 + LP_PAD), L.ptr(st),
                                 L.ptr(rm), M, C.byref(kid), L.stream()), "xe_criterion")
    torch.cuda.synchronize()
    out = {"row_loss": row_loss.cpu()}
    if grad:
        out["dlogits"] = d.cpu()
    if logprobs:
        out["logprobs"] = lp.cpu()
    if stats:
        out["stats"] = st.cpu()
    return kid.value, out


def launch_twice(*a, **k):
    """Every launch is repeated once: the results must be bit-equal."""
    kid, out = launch(*a, **k)
    kid2, out2 = launch(*a, **k)
    assert kid2 == kid
    for key in out:
        assert torch.equal(out[key], out2[key]), (NAMES[kid], key)
    return kid, out


def check_loss(c, kid, out):
    got = out["row_loss"].double()
    ref, tol, mask = c.row_loss, c.tol, c.mask.double()
    assert not torch.isnan(got).any()
    assert (got[mask == 0] == 0).all(), got                                   # exact zeros behind the mask
    err = (got - ref).abs()
    _note(kid, "row_loss", (err / tol).max())
    assert (err <= tol * mask).all(), (NAMES[kid], err.tolist(), tol.tolist())
    total = abs(float(got.sum()) - float(ref.sum()))
    assert total <= float((tol * mask).sum()), (NAMES[kid], total)
    _note(kid, "summed loss", total / float((tol * mask).sum()))


def check_grad(c, kid, out, w, bf16):
    """dlogits = (softmax - onehot) * w: probabilities within tol * p + 1e-7 (times |w|), one bf16 rounding more for bf16."""
    got = out["dlogits"].double()
    assert not torch.isnan(got).any() and not torch.isinf(got).any(), NAMES[kid]
    assert (got[:, c.V1:] == 0).all(), NAMES[kid]                           # the padding columns are written, as zeros
    got = got[:, :c.V1]
    w = w.double()
    assert (got[w == 0] == 0).all(), NAMES[kid]                             # all-zero gradient rows behind the mask
    ref = (c.p - c.onehot) * w[:, None]
    bound = w.abs()[:, None] * (c.tol[:, None] * c.p + 1e-7)
    if bf16:
        bound = bound + 2.0 ** -8 * ref.abs()
    err = (got - ref).abs()
    live = w != 0
    ratio = (err[live] / bound[live]).max()
    _note(kid, "dlogits", ratio)
    worst = int((err - bound).argmax())
    assert ratio <= 1.0, (NAMES[kid], float(ratio), divmod(worst, c.V1), float(got.flatten()[worst]), float(ref.flatten()[worst]))


def check_logprobs(c, kid, out):
    got = out["logprobs"]
    assert (got[:, :, c.V1:] == -55.0).all(), NAMES[kid]                     # nothing written past V1
    got = got[:, :, :c.V1].permute(1, 0, 2).reshape(M, c.V1).double()       # [n][t][v] -> row m = t * N + n
    assert not torch.isnan(got).any(), NAMES[kid]
    dead = torch.isinf(c.lp)
    assert (got[dead] == -INF).all(), NAMES[kid]
    err = torch.where(dead, torch.zeros((), dtype=torch.float64), (got - c.lp).abs())
    ratio = (err / c.tol[:, None]).max()
    _note(kid, "logprobs", ratio)
    worst = int((err / c.tol[:, None]).argmax())
    assert ratio <= 1.0, (NAMES[kid], float(ratio), divmod(worst, c.V1))


def test_the_cases_reach_all_five_kernels():
    want = {k for _, _, a, b in CASES for k in (a, b) if k is not None}
    assert want == {GENERIC, LDS, REG, REG_WIDE, BIG}
    L = _L()
    assert (L.XE_GENERIC, L.XE_LDS, L.XE_REG, L.XE_REG_WIDE, L.XE_BIG) == (GENERIC, LDS, REG, REG_WIDE, BIG)
    assert L.XE_KERNEL_NAMES == NAMES


@pytest.mark.parametrize("dtype,shape,grad_kernel,lp_kernel", CASES, ids=[_case_id(c) for c in CASES])
def test_criterion_kernels_against_float64(dtype, shape, grad_kernel, lp_kernel):
    c = case(*shape)
    # the masked criterion: d logits = (softmax - onehot) * mask / sum(mask)
    kid, out = launch_twice(c, dtype)
    assert kid == grad_kernel, (NAMES[kid], NAMES[grad_kernel])
    check_loss(c, kid, out)
    check_grad(c, kid, out, c.mask * c.inv_den, dtype == 1)
    # the self-critical form: a weight per position, either sign, instead of mask / sum(mask)
    kid, out = launch_twice(c, dtype, scale=True)
    assert kid == grad_kernel, (NAMES[kid], NAMES[grad_kernel])
    check_loss(c, kid, out)
    check_grad(c, kid, out, c.scale, dtype == 1)
    if lp_kernel is None:
        return
    # log-probabilities out, gradient off and on
    for grad in (False, True):
        kid, out = launch_twice(c, dtype, grad=grad, logprobs=True)
        assert kid == lp_kernel, (NAMES[kid], NAMES[lp_kernel], grad)
        check_loss(c, kid, out)
        check_logprobs(c, kid, out)
        if grad:
            check_grad(c, kid, out, c.mask * c.inv_den, dtype == 1)


def test_logits_off_a_16_byte_boundary_take_the_generic_kernel():
    """bf16 logits that start 4 bytes into a device buffer -- aligned for a float, not for the 16-byte loads of the four bf16
    kernels: the dispatcher must pick the generic kernel, which is held to the same bounds."""
    c = case(1024, 1024)
    buf = torch.empty(M * c.ldv + 1, device="cuda")
    lg = buf[1:].view(M, c.ldv)
    lg.copy_(c.logits)
    assert lg.is_contiguous() and lg.data_ptr() % 16 == 4
    kid, out = launch_twice(c, 1, logits=lg)
    assert kid == GENERIC, NAMES[kid]
    check_loss(c, kid, out)
    check_grad(c, kid, out, c.mask * c.inv_den, True)


ROW_MAP_CASES = [(1, (1025, 1028), REG, False), (1, (10241, 10244), REG_WIDE, False), (1, (53249, 53252), BIG, False),
                 (1, (1025, 1028), LDS, True),          # (with the accuracy counters the short bf16 row goes through LDS)
                 (0, (1025, 1028), GENERIC, False), (0, (10241, 10244), GENERIC, False), (0, (53249, 53252), GENERIC, False)]


@pytest.mark.parametrize("dtype,shape,kernel,stats", ROW_MAP_CASES,
                         ids=["%s-%dx%d-%s" % ("bf16" if d else "f32", s[0], s[1], NAMES[k]) for d, s, k, _ in ROW_MAP_CASES])
def test_row_map_lists_the_live_positions(dtype, shape, kernel, stats):
    """A compacted, shuffled list of the mask-live positions, padded with -1 and one entry >= row_map_limit: the listed rows are
    bit for bit the rows of the unlisted launch at those positions, padding rows get a zero gradient and no loss entry."""
    c = case(*shape)
    kid0, plain = launch(c, dtype, stats=stats)
    assert kid0 == kernel
    check_grad(c, kid0, plain, c.mask * c.inv_den, dtype == 1)
    live = [m for m in range(M) if c.mask[m] != 0]
    order = torch.randperm(len(live), generator=torch.Generator().manual_seed(5)).tolist()
    row_map = [live[order[0]], -1] + [live[i] for i in order[1:6]] + [M + 3] + [live[i] for i in order[6:]] + [-1, -1]
    rows = len(row_map)
    src = [p if 0 <= p < M else 0 for p in row_map]                  # (padding rows: finite logits of some other row)
    logits = c.logits[src].clone()
    kid, out = launch_twice(c, dtype, row_map=row_map, logits=logits, stats=stats)
    assert kid == kernel, (NAMES[kid], NAMES[kernel])
    for j, p in enumerate(row_map):
        if 0 <= p < M:
            assert torch.equal(out["dlogits"][j], plain["dlogits"][p]), (j, p)
            assert torch.equal(out["row_loss"][j], plain["row_loss"][p]), (j, p)
        else:
            assert (out["dlogits"][j] == 0).all(), j
            assert out["row_loss"][j] == -77.0, j                     # the canary
    assert rows == len(live) + 4
    if stats:
        # padding rows count nothing, and the masked-out positions are not listed
        am, raw = np.argmax(c.x.numpy(), axis=1), c.raw.numpy()
        listed = np.isin(np.arange(M), live)
        want = [int((listed & (raw != 0) & (am == raw)).sum()), int((listed & (raw != 0)).sum())]
        assert want[1] > 0 and out["stats"].tolist() == want, (out["stats"].tolist(), want)


STATS_CASES = [(1, (1000, 1000), LDS), (1, (50004, 50048), REG_WIDE), (1, (53249, 53252), BIG),
               (0, (1000, 1000), GENERIC), (0, (50004, 50048), GENERIC), (0, (53249, 53252), GENERIC)]


@pytest.mark.parametrize("dtype,shape,kernel", STATS_CASES,
                         ids=["%s-%dx%d-%s" % ("bf16" if d else "f32", s[0], s[1], NAMES[k]) for d, s, k in STATS_CASES])
def test_score_stats_count_by_the_raw_target_and_the_lowest_arg_max(dtype, shape, kernel):
    """NMT_loss.score's counters: [1] = rows whose raw target is not 0 (the mask plays no part), [0] = those whose arg-max is the
    raw target, with the LOWEST index winning an exact tie between columns held by different chunks, threads and waves."""
    c = Case(*shape, ties=True)
    am = np.argmax(c.x.numpy(), axis=1)                      # (first occurrence: the lowest index)
    raw = c.raw.numpy()
    want = [int(((raw != 0) & (am == raw)).sum()), int((raw != 0).sum())]
    for m, (a, b) in ((4, (3, 4)), (7, (4095, 4096)), (9, (1023, c.V1 - 1))):
        if b < c.V1 and a < c.V1:
            assert am[m] == a and c.x[m, a] == c.x[m, b]
    assert 0 < want[0] < want[1] < M                         # hits, misses and uncounted rows are all present
    assert raw[11] == 4 and am[11] == 3                      # the row that aims at the higher column of a tie is a miss
    assert c.mask[10] == 0 and raw[10] != 0                  # a masked-out position with a target still counts
    kid, out = launch_twice(c, dtype, stats=True)
    assert kid == kernel, (NAMES[kid], NAMES[kernel])
    assert out["stats"].tolist() == want, (NAMES[kid], out["stats"].tolist(), want)
    check_loss(c, kid, out)
    check_grad(c, kid, out, c.mask * c.inv_den, dtype == 1)
