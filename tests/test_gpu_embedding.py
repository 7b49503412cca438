"""The embedding kernels behind uic_embedding_* (csrc/embedding.hip: embed_fwd_kernel, embed_fwd_rows_bf16_kernel, and the backward
pipeline embed_hist -> embed_block_prefix -> embed_scan -> embed_fill -> embed_gather -> embed_gather_finish) on their own, through
raw pointers, on token sets shaped like captions: hot buckets of 17 to 200 and more entries back to back in the sorted list.

Backward is compared EXACTLY.  Gradients are integers in [-8, 8] and 1 / (1 - drop_p) is 1, 2 or 4, so every partial sum is an
integer below 2^24 and the f32 result must equal zeros(V1, E, float64).index_add_(0, token of the row, masked gradient) * inv_keep
whatever the order of the additions; a dropped partial row, a bucket with two owners or none, a wrong mask or a missing inv_keep
changes an integer.  dtable holds NaN before every call and rows that no position selects must come back as 0.  The cases and the
classes of launch geometry they reach (buckets inside a workgroup, straddling two, straddling more than ten, beginning or ending on
a workgroup boundary, both planes of a chunk written, key 0 / key V1 - 1 / the padding index straddling, a short last workgroup,
several histogram blocks, the plain-atomic fallback of the wave aggregation, every one of those in the second half of a split
list) are in tests/embedding_cases.py; tests/test_embedding_cases_host.py asserts on the CPU that no class is left out.

Every case runs on zero-filled scratch, and again right after a larger case whose gradients are all 2^20 -- same bits: stale
entries of that run are in-range indices and huge partial rows, so a slot that is read without having been written shows up as a
wrong sum.  With a split, the table after gather(half = 1) alone is the share of steps >= split, and after gather(half = 0) the
whole gradient, bit-equal to the split = 0 result.

One Zipf case has randn gradients: per entry |got - ref64| <= n 2^-24 sum|terms| + ulp(result) (n the bucket size; the bound of n
f32 additions in any order, and one rounding for inv_keep), three runs bit-equal.  Measured on an MI355X (profiles/LOG.md,
"Embedding kernels as uic_embedding_*"): worst error / bound 0.375 over the 154 800 entries, the largest bucket 583 entries; the
87 cases of this module take 2.5 s.

Forward: torch.equal against (relu?(table[token]) * mask).to(out dtype), mask from uic_dropout_mask with base = idx_base -- E = 4 /
8 / 12 / 520, 1 / 3 / 4 / 5 / 8192 * 4 + 1 rows (past the row kernel's grid cap), f32 and bf16 tables, an index base that wraps
2^32 inside the tensor, and an output 8 bytes off 16-byte alignment, where the element-wise kernel must give the bits of the row
kernel.  The dropout hash itself is pinned against a numpy uint32 restatement.
"""
import functools

import numpy as np
import pytest
import torch

import embedding_cases as EC

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
SITE_EMBED = 3
CASES = EC.backward_cases()
NAN = float("nan")
WORST = {}


def _L():
    from unpaired_image_captioning_amd import _lib
    return _lib


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print("\n[embedding] %-28s worst error / bound: %.4f" % (k, WORST[k]))


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class Buffers:
    """scratch, dxt, xt, tokens and dtable, allocated once at the size of the largest case (the dirty one) and shared by every run."""

    def __init__(self):
        d = EC.dirty_case()
        every = CASES + (d,)
        dev = "cuda"
        self.scratch = torch.zeros(max(EC.scratch_ints(c.N, c.T, c.V1, c.E) for c in every), dtype=torch.int32, device=dev)
        self.dxt = torch.zeros(d.positions * d.E, device=dev)
        self.xt = torch.zeros(d.positions * d.E, device=dev)
        self.tokens = torch.zeros(max(c.N * c.ld for c in every), dtype=torch.int64, device=dev)
        self.dtable = torch.zeros(d.V1 * d.E, device=dev)
        self.dirty_g = torch.full((d.positions * d.E,), 2.0 ** 20, device=dev)


@pytest.fixture(scope="module")
def B():
    return Buffers()


HAND = (1.0, 0.0, -0.0, -2.5, NAN, 0.5, 3.0, -0.0078125, 2.0, 0.0, 7.0)       # only the positive ones pass


def forward(out_dtype, table, tokens, ld, N, T, drop_p, seed, site, idx_base, relu, out):
    L = _L()
    V1, E = table.shape
    L.check(L.load().uic_embedding_forward(out_dtype, L.ptr(table), BF16 if table.dtype == torch.bfloat16 else F32, V1, E, L.ptr(tokens), ld, N, T,
                                           drop_p, seed, site, idx_base, relu, out.data_ptr(), L.stream()), "embedding_forward")


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(gradient [P, E] f32, xt or None, the mask xt > 0) of a case, on the CPU; built once."""
    c = EC.case_by_name(name) if name != "dirty" else EC.dirty_case()
    g = torch.from_numpy(c.grad())
    P, E = c.positions, c.E
    if c.xt == "none":
        return g, None, np.ones((P, E), dtype=bool)
    bf16 = c.xt.endswith("bf16")
    if c.xt.startswith("hand"):
        xt = torch.tensor(HAND, dtype=torch.float32)[torch.arange(P * E) % len(HAND)].view(P, E)
        xt = xt.bfloat16() if bf16 else xt
    else:                                        # the forward output itself: relu and the dropped elements are one mask
        gen = torch.Generator().manual_seed(c.seed)
        table = torch.randn(c.V1, E, generator=gen).cuda()
        out = torch.full((P, E), NAN, device="cuda", dtype=torch.bfloat16 if bf16 else torch.float32)
        forward(BF16 if bf16 else F32, table, torch.from_numpy(c.tokens).cuda(), c.ld, c.N, c.T, c.drop_p, c.seed, SITE_EMBED, 0, 1, out)
        xt = out.cpu()
        assert not torch.isnan(xt.float()).any()
        kept = float((xt.float() > 0).float().mean())
        assert 0 < kept < 1 or P * E < 200, (name, kept)                  # (the mask masks, and not everything)
    return g, xt, (xt.float() > 0).numpy()


def launch(B, c, g, xt, split, one_call=False, dirty=False):
    """One backward pass of case c in the shared buffers, dtable NaN before it.  Returns (dtable, dtable after half 1 alone or None)."""
    L = _L()
    lib, P = L.load(), L.ptr
    n = c.positions * c.E
    tok = B.tokens[:c.N * c.ld]
    tok.copy_(torch.from_numpy(c.tokens).view(-1))
    dxt = B.dxt[:n]
    dxt.copy_(B.dirty_g[:n] if dirty else g.view(-1))
    if xt is None or dirty:
        xp, dt = None, (BF16 if c.seed % 2 else F32)                      # (the dtype only picks the kernel's instantiation)
    elif xt.dtype == torch.bfloat16:
        xv = B.xt.view(torch.bfloat16)[:n]
        xv.copy_(xt.view(-1))
        xp, dt = P(xv), BF16
    else:
        xv = B.xt[:n]
        xv.copy_(xt.view(-1))
        xp, dt = P(xv), F32
    table = B.dtable[:c.V1 * c.E]
    table.fill_(NAN)
    s = L.stream()
    shape = (c.ld, c.N, c.T, c.V1, c.E)
    drop_p = 0.0 if dirty else c.drop_p
    half1 = None
    if one_call:
        assert split == 0
        L.check(lib.uic_embedding_backward(dt, P(dxt), xp, P(tok), *shape, drop_p, c.skip, P(table), P(B.scratch), s), "embedding_backward")
    else:
        L.check(lib.uic_embedding_backward_prepare(P(tok), *shape, P(table), P(B.scratch), split, s), "embedding_backward_prepare")
        if split:
            L.check(lib.uic_embedding_backward_gather(dt, P(dxt), xp, P(tok), *shape, drop_p, c.skip, P(table), P(B.scratch), split, 1, s), "gather 1")
            half1 = table.clone().view(c.V1, c.E)
        L.check(lib.uic_embedding_backward_gather(dt, P(dxt), xp, P(tok), *shape, drop_p, c.skip, P(table), P(B.scratch), split, 0, s), "gather 0")
    torch.cuda.synchronize()
    return table.clone().view(c.V1, c.E), half1


def run_dirty(B):
    d = EC.dirty_case()
    return launch(B, d, None, None, 0, one_call=True, dirty=True)[0]


def exact(got, ref, c, what):
    got = got.cpu()
    if not torch.equal(got.double(), ref):
        bad = (got.double() != ref) | torch.isnan(got.double())
        rows = torch.nonzero(bad.any(1)).view(-1).tolist()
        r = rows[0]
        col = int(torch.nonzero(bad[r]).view(-1)[0])
        raise AssertionError("%s %s: %d table rows differ (first: row %d col %d got %r want %r; bucket sizes of the wrong rows %s)" % (
            c.name, what, len(rows), r, col, float(got[r, col]), float(ref[r, col]), np.bincount(c.row_token(), minlength=c.V1)[rows[:8]].tolist()))


# ---- the restated geometry is the library's ----
def test_scratch_size_is_the_restated_formula():
    """If this fails a constant of the kernels has moved: move the edges of tests/embedding_cases.py with it."""
    lib = _L().load()
    shapes = [(c.N, c.T, c.V1, c.E) for c in CASES + (EC.dirty_case(),)] + [(0, 5, 3, 4), (5, 0, 3, 4), (1, 1, 1, 4), (10, 20, 9488, 512), (80, 17, 50004, 512)]
    for s in shapes:
        assert lib.uic_embedding_scratch_ints(*s) == EC.scratch_ints(*s), s
    for bad in ((-1, 5, 3, 4), (5, -1, 3, 4), (5, 5, 0, 4), (5, 5, -2, 4), (5, 5, 3, 0), (5, 5, 3, 6), (5, 5, 3, -4), (2 ** 15, 2 ** 15, 3, 4)):
        assert lib.uic_embedding_scratch_ints(*bad) == 0, bad
    assert EC.fwd_row_kernel_trips(EC.FWD_GRID_CAP * EC.FWD_ROWS_PER_WG + 1, 8) == (2, 1) and EC.fwd_row_kernel_trips(5, 520) == (1, 2)
    assert EC.fwd_row_kernel_trips(EC.FWD_GRID_CAP * EC.FWD_ROWS_PER_WG, 512) == (1, 1)


# ---- backward ----
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_backward_is_exact_and_does_not_depend_on_what_the_scratch_held(B, c):
    g, xt, mask = inputs(c.name)
    gm = np.where(mask, g.numpy(), 0.0).astype(np.float64)
    assert float(np.abs(gm).sum(0).max()) * c.inv_keep < 2 ** 24
    ref = EC.reference(c, gm)
    B.scratch.zero_()
    got, half1 = launch(B, c, g, xt, c.split, one_call=not c.split)
    exact(got, ref, c, "on clean scratch")
    absent = np.ones(c.V1, dtype=bool)
    absent[c.row_token()] = False
    if c.skip >= 0:
        absent[c.skip] = True
    assert (got.cpu()[torch.from_numpy(absent)] == 0).all()
    if c.split:
        exact(half1, EC.reference(c, gm, halves=(1,)), c, "after half 1 alone")
    other, _ = launch(B, c, g, xt, 0, one_call=bool(c.split))              # split = 0 by the other entry point: the same bits
    assert torch.equal(bits(other), bits(got)), (c.name, "split / two-call form")
    run_dirty(B)
    again, half1_again = launch(B, c, g, xt, c.split, one_call=not c.split)
    exact(again, ref, c, "on dirty scratch")
    assert torch.equal(bits(again), bits(got)), c.name
    if c.split:
        assert torch.equal(bits(half1_again), bits(half1)), c.name


def test_the_dirty_run_itself_is_exact(B):
    d = EC.dirty_case()
    B.scratch.zero_()
    got = run_dirty(B)
    count = torch.from_numpy(np.bincount(d.row_token(), minlength=d.V1)).double()
    assert count.max() * 2.0 ** 20 < 2.0 ** 53 and count.max() < 2 ** 12                # a multiple of 2^20 below 2^32: exact in f32
    assert torch.equal(got.cpu().double(), (count * 2.0 ** 20)[:, None].expand(d.V1, d.E))


def test_float_gradients_hold_the_bound_of_any_summation_order(B):
    """n additions of f32 numbers in any order: |error| <= n 2^-24 sum |terms|; inv_keep = 2 is exact, one ulp is granted for it."""
    c = EC.case_by_name("zipf")
    assert c.drop_p == 0.5 and c.xt == "fwd_bf16"
    _, xt, mask = inputs(c.name)
    g = torch.randn(c.positions, c.E, generator=torch.Generator().manual_seed(77))
    gm = np.where(mask, g.numpy(), 0.0).astype(np.float64)
    ref = EC.reference(c, gm)
    mag = EC.reference(c, np.abs(gm))
    size = torch.from_numpy(np.bincount(c.row_token(), minlength=c.V1)).double()[:, None]
    ulp = torch.from_numpy(np.spacing(np.abs(ref.numpy()).astype(np.float32)).astype(np.float64))
    bound = size * 2.0 ** -24 * mag + ulp
    B.scratch.zero_()
    got, _ = launch(B, c, g, xt, 0, one_call=True)
    for _ in range(2):
        again, _ = launch(B, c, g, xt, 0, one_call=True)
        assert torch.equal(bits(again), bits(got))
    err = (got.cpu().double() - ref).abs()
    assert not torch.isnan(err).any()
    ratio = float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())
    WORST["backward, randn gradients"] = ratio
    print("\n[embedding] float case: worst error / bound %.4f over %d entries, largest bucket %d" % (ratio, err.numel(), int(size.max())))
    assert ratio <= 1.0, ratio
    assert int(size.max()) >= 200 and float(err.max()) > 0            # the sums do round: the case is not exact by accident


# ---- forward ----
FWD_SHAPES = [(1, 1, 8), (3, 1, 8), (2, 2, 8), (5, 1, 8), (3641, 9, 8), (1, 1, 4), (3, 5, 4), (3, 5, 12), (7, 3, 520)]
FWD_V1 = 11


@functools.lru_cache(maxsize=None)
def fwd_tokens(N, T):
    ld = T + 3
    rng = np.random.default_rng(N * 31 + T)
    tok = rng.integers(0, FWD_V1, size=(N, ld)).astype(np.int64)
    if N * T >= 5:
        flat = rng.permutation(N * T)[:4]
        for i, v in zip(flat, (-1, FWD_V1, 2 ** 40, EC.INT64_MIN)):
            tok[i % N, i // N] = v
    live = tok[:, :T]
    rows = np.where((live < 0) | (live >= FWD_V1), 0, live).T.reshape(-1)          # time-major
    return tok, ld, torch.from_numpy(rows)


def dropout_mask(n, p, seed, site, base):
    L = _L()
    out = torch.full((n,), NAN, device="cuda")
    L.check(L.load().uic_dropout_mask(L.ptr(out), n, p, seed, site, base, L.stream()), "dropout_mask")
    return out.cpu()


@pytest.mark.parametrize("N,T,E", FWD_SHAPES, ids=["%dx%dx%d" % s for s in FWD_SHAPES])
def test_forward_equals_table_rows_times_the_exported_mask(N, T, E):
    rows = N * T
    assert rows in (1, 3, 4, 5, 15, 21, EC.FWD_GRID_CAP * EC.FWD_ROWS_PER_WG + 1)
    tok, ld, row_tok = fwd_tokens(N, T)
    tok_d = torch.from_numpy(tok).cuda()
    table = torch.randn(FWD_V1, E, generator=torch.Generator().manual_seed(E + rows))
    table[1, :] = table[1, :].abs()
    table[2, :] = -table[2, :].abs()
    tables = {F32: table, BF16: table.bfloat16()}
    n = rows * E
    seed = 1234567 + rows
    for drop_p in (0.0, 0.25, 0.5):
        for idx_base in (0, 7 * N * E, 2 ** 32 - 5 * E):
            mask = dropout_mask(n, drop_p, seed, SITE_EMBED, idx_base).view(rows, E)
            if drop_p > 0 and n >= 60:
                assert 0 < int((mask == 0).sum()) < n
            for tdt, odt in ((F32, F32), (F32, BF16), (BF16, BF16)):
                tab = tables[tdt]
                tab_d = tab.cuda()
                tdtype = torch.bfloat16 if odt == BF16 else torch.float32
                for relu in (0, 1):
                    v = tab.float()[row_tok]
                    ref = ((torch.relu(v) if relu else v) * mask).to(tdtype)
                    buf = torch.full((n + 64,), NAN, device="cuda", dtype=tdtype)
                    forward(odt, tab_d, tok_d, ld, N, T, drop_p, seed, SITE_EMBED, idx_base, relu, buf)
                    torch.cuda.synchronize()
                    out = buf.cpu()
                    ctx = (N, T, E, drop_p, idx_base, tdt, odt, relu)
                    assert torch.equal(out[:n].view(rows, E), ref), ctx
                    assert torch.isnan(out[n:].float()).all(), ctx                                  # nothing behind the last row
                    if odt == BF16 and E % 8 == 0:
                        # 8 bytes off 16-byte alignment (out, then the bf16 table): the element-wise kernel, the same bits
                        buf2 = torch.full((n + 64,), NAN, device="cuda", dtype=tdtype)
                        off_out = buf2[4:]
                        assert off_out.data_ptr() % 16 == 8
                        forward(odt, tab_d, tok_d, ld, N, T, drop_p, seed, SITE_EMBED, idx_base, relu, off_out)
                        assert torch.equal(bits(off_out[:n]), bits(buf[:n])), ctx + ("out + 8 bytes",)
                        assert torch.isnan(buf2[:4].float()).all() and torch.isnan(off_out[n:].float()).all(), ctx
                        if tdt == BF16:
                            tbuf = torch.zeros(FWD_V1 * E + 4, device="cuda", dtype=torch.bfloat16)
                            off_tab = tbuf[4:].view(FWD_V1, E)
                            off_tab.copy_(tab_d)
                            assert off_tab.data_ptr() % 16 == 8
                            buf3 = torch.full((n + 64,), NAN, device="cuda", dtype=tdtype)
                            forward(odt, off_tab, tok_d, ld, N, T, drop_p, seed, SITE_EMBED, idx_base, relu, buf3)
                            assert torch.equal(bits(buf3[:n]), bits(buf[:n])), ctx + ("table + 8 bytes",)


def test_forward_index_wraps_inside_the_tensor():
    """idx_base = 2^32 - 5 E: row 5 starts again at element index 0 -- the mask of rows 5... is the mask of base 0."""
    E, rows = 8, 21
    wrapped = dropout_mask(rows * E, 0.5, 99, SITE_EMBED, 2 ** 32 - 5 * E)
    assert torch.equal(wrapped[5 * E:], dropout_mask((rows - 5) * E, 0.5, 99, SITE_EMBED, 0))


# ---- the dropout hash: checkpoint resume relies on it never drifting ----
@pytest.mark.parametrize("seed,site", [(1, SITE_EMBED), (0x9E3779B9, 4001)])
def test_dropout_hash_is_the_restated_one(seed, site):
    n, base = 100003, 2 ** 32 - 50000
    for p in (0.25, 0.5):
        mask = dropout_mask(n, p, seed, site, base).numpy()
        keep = EC.drop_keep(n, p, seed, site, base)
        assert ((mask != 0) == keep).all(), (seed, site, p, int(((mask != 0) != keep).sum()))
        assert (mask[keep] == np.float32(1.0) / (np.float32(1.0) - np.float32(p))).all()
        assert abs(keep.mean() - (1 - p)) < 0.01
    assert (dropout_mask(1000, 0.0, seed, site, base).numpy() == 1).all()


# ---- argument errors: refused with a message, nothing launched ----
def test_argument_errors_are_refused_and_write_nothing():
    L = _L()
    lib, P, s = L.load(), L.ptr, L.stream()
    N, T, ld, V1, E = 5, 4, 6, 7, 8
    canary = lambda n, dt=torch.float32: torch.full((n,), NAN, device="cuda", dtype=dt)          # noqa: E731
    table, table16 = torch.randn(V1, E, device="cuda"), torch.randn(V1, E, device="cuda").bfloat16()
    tok = torch.randint(0, V1, (N, ld), device="cuda")
    out, out16, dtable = canary(N * T * E + 8), canary(N * T * E + 8, torch.bfloat16), canary(V1 * E + 8)
    dxt, xt, xt16 = torch.ones(N * T * E + 8, device="cuda"), torch.ones(N * T * E + 8, device="cuda"), torch.ones(N * T * E + 8, device="cuda").bfloat16()
    scratch = torch.zeros(lib.uic_embedding_scratch_ints(N, T, V1, E) + 8, dtype=torch.int32, device="cuda")
    TB, TB16, TK, O, O16, DT, DX, XT, XT16, SC = P(table), P(table16), P(tok), P(out), P(out16), P(dtable), P(dxt), P(xt), P(xt16), P(scratch)

    def fwd(odt=F32, table=TB, tdt=F32, V1=V1, E=E, tok=TK, ld=ld, N=N, T=T, p=0.5, out=O):
        return lib.uic_embedding_forward(odt, table, tdt, V1, E, tok, ld, N, T, p, 1, SITE_EMBED, 0, 1, out, s)

    def prep(tok=TK, ld=ld, N=N, T=T, V1=V1, E=E, dtable=DT, scratch=SC, split=0):
        return lib.uic_embedding_backward_prepare(tok, ld, N, T, V1, E, dtable, scratch, split, s)

    def gather(dt=F32, dxt=DX, xt=XT, tok=TK, ld=ld, N=N, T=T, V1=V1, E=E, p=0.5, skip=-1, dtable=DT, scratch=SC, split=0, half=0):
        return lib.uic_embedding_backward_gather(dt, dxt, xt, tok, ld, N, T, V1, E, p, skip, dtable, scratch, split, half, s)

    def bwd(dt=F32, dxt=DX, xt=XT, tok=TK, ld=ld, N=N, T=T, V1=V1, E=E, p=0.5, skip=-1, dtable=DT, scratch=SC):
        return lib.uic_embedding_backward(dt, dxt, xt, tok, ld, N, T, V1, E, p, skip, dtable, scratch, s)

    bad = {}

    def refuse(what, call, **kw):
        rc = call(**kw)
        msg = lib.uic_last_error_string()
        bad[what + " " + repr(sorted(kw))] = (rc, msg)
        assert rc != 0 and msg and b"embedding" in msg, (what, kw, rc, msg)

    nan = float("nan")
    for kw in (dict(table=None), dict(tok=None), dict(out=None), dict(odt=2), dict(odt=-1), dict(tdt=2), dict(tdt=-1), dict(E=0), dict(E=6), dict(E=-4),
               dict(V1=0), dict(V1=-1), dict(N=-1), dict(T=-1), dict(ld=T - 1), dict(table=TB16, tdt=BF16, odt=F32), dict(p=-0.1), dict(p=1.0), dict(p=1.5),
               dict(p=nan), dict(table=TB + 8), dict(table=TB + 4), dict(table=TB16 + 4, tdt=BF16, odt=BF16, out=O16), dict(out=O + 2),
               dict(out=O16 + 1, odt=BF16), dict(N=2 ** 15, T=2 ** 15, ld=2 ** 15)):
        refuse("forward", fwd, **kw)
    for kw in (dict(tok=None), dict(dtable=None), dict(scratch=None), dict(E=0), dict(E=10), dict(V1=0), dict(V1=-3), dict(N=-1), dict(T=-1), dict(ld=T - 1),
               dict(split=-1), dict(split=T), dict(split=T + 3), dict(dtable=DT + 8), dict(dtable=DT + 4), dict(scratch=SC + 4), dict(scratch=SC + 8)):
        refuse("prepare", prep, **kw)
    common = (dict(dt=2), dict(dt=-1), dict(dxt=None), dict(tok=None), dict(dtable=None), dict(scratch=None), dict(E=0), dict(E=10), dict(V1=0), dict(N=-1),
              dict(T=-1), dict(ld=T - 1), dict(skip=V1), dict(skip=V1 + 5), dict(skip=2 ** 40), dict(p=-0.5), dict(p=1.0), dict(p=nan), dict(dxt=DX + 8),
              dict(xt=XT + 8), dict(xt=XT16 + 4, dt=BF16), dict(xt=XT16 + 2, dt=BF16), dict(dtable=DT + 8), dict(scratch=SC + 4))
    for kw in common:
        refuse("gather", gather, **kw)
        refuse("backward", bwd, **kw)
    for kw in (dict(split=-1), dict(split=T), dict(half=2), dict(half=-1), dict(half=1), dict(half=1, split=0), dict(split=2, half=2)):
        refuse("gather", gather, **kw)
    torch.cuda.synchronize()
    for t in (out, out16, dtable):
        assert torch.isnan(t.float()).all()
    # an 8-byte aligned bf16 xt and an f32 output 4 bytes into a buffer are fine; so is no xt at all
    assert fwd(out=O + 4) == 0 and fwd(odt=BF16, out=O16 + 2) == 0
    assert prep() == 0 and gather(dt=BF16, xt=XT16 + 8) == 0 and gather(xt=None) == 0 and bwd(xt=None, skip=V1 - 1) == 0
    torch.cuda.synchronize()
    # N == 0 or T == 0: a successful no-op, except that prepare (and the one-call form) still zero dtable
    out.fill_(NAN)
    for kw in (dict(N=0), dict(T=0, ld=0), dict(T=0)):
        dtable.fill_(NAN)
        assert fwd(**kw) == 0 and gather(**kw) == 0
        torch.cuda.synchronize()
        assert torch.isnan(out).all() and torch.isnan(dtable).all(), kw
        assert prep(**kw) == 0
        torch.cuda.synchronize()
        assert (dtable[:V1 * E] == 0).all() and torch.isnan(dtable[V1 * E:]).all(), kw
        dtable.fill_(NAN)
        assert bwd(**kw) == 0
        torch.cuda.synchronize()
        assert (dtable[:V1 * E] == 0).all(), kw
