"""The operators behind uic_topdown_batch.unfinished_count, each on its own and exact -- a GEMM row's result does not depend on where
the row sits, and a value that is dropped by a select leaves no trace, so every comparison here is bit for bit:
  * uic_live_order (csrc/live_rows.hip): caption lengths, their stable descending order, its inverse and the per-step counts
    against numpy, and the status word for counts that are not the masks';
  * uic_linear_partials_rows (csrc/gemm_glds.hip, the slab epilogue with a row map): a compact A operand whose tile tail holds NaN, the
    written slab rows against the unmapped launch, the others against a sentinel;
  * uic_lstm_cell_bwd_live / uic_h2att_cell_bwd_live (csrc/lstm_cell.hip, csrc/bptt_fused.hip): slab rows of ended captions filled
    with NaN against the same rows zeroed, against the operators without row_len, and the compact copy against the rows by order."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 17
SENTINEL = -12345.678


def _lib():
    from unpaired_image_captioning_amd import _lib as L_
    return L_


def _masks_from_lengths(lengths):
    m = torch.zeros(len(lengths), T + 1)
    for n, k in enumerate(lengths):
        m[n, :1 + int(k)] = 1.0
    return m


def _live_order(masks, expect=None, status=None):
    """(row_len, order, rank, unfinished) of masks [N, T + 1] (device), as numpy."""
    L = _lib()
    N = masks.shape[0]
    out = [torch.full((n,), -7, dtype=torch.int32, device="cuda") for n in (N, N, N, T + 1)]
    ex = None if expect is None else np.ascontiguousarray(expect, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    L.check(L.load().uic_live_order(L.ptr(masks), T + 1, 1, N, T, *[L.ptr(o) for o in out], ex, L.ptr(status), L.stream()), "live_order")
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _lengths(pattern, N, rng):
    if pattern == "equal":
        return np.full(N, 11)
    if pattern == "one_longer":
        k = rng.integers(1, 9, N)
        k[N // 2] = 16
        return k
    return rng.integers(0, T + 1, N)


@pytest.mark.parametrize("N", [1, 4, 85, 129, 640, 1050])
@pytest.mark.parametrize("pattern", ["equal", "one_longer", "ragged", "holes"])
def test_live_order_is_the_stable_descending_sort_of_the_lengths(N, pattern):
    rng = np.random.default_rng(N)
    if pattern == "holes":
        m = (torch.from_numpy(rng.random((N, T + 1))) < 0.4).float() * 0.5
        m[:, 1 + 4] = 0.0
        m[N // 3, :] = 0.0
    else:
        m = _masks_from_lengths(_lengths(pattern, N, rng))
    on = m[:, 1:].numpy() != 0
    want_len = np.where(on.any(1), T - np.argmax(on[:, ::-1], axis=1), 0)
    want_unf = [(want_len > t).sum() for t in range(T)] + [0]
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    row_len, order, rank, unf = _live_order(m.cuda(), expect=want_unf[:T], status=status)
    assert row_len.tolist() == want_len.tolist()
    assert order.tolist() == np.argsort(-want_len, kind="stable").tolist()
    assert rank[order].tolist() == list(range(N))
    assert unf.tolist() == want_unf
    for t in range(T):                                # the rows with a longer caption are a prefix of the order, for every t
        assert set(order[:unf[t]].tolist()) == set(np.flatnonzero(want_len > t).tolist())
    assert status.cpu().tolist() == [0, 0, 0, 0]
    # the same masks again: the same order (no atomics)
    again = _live_order(m.cuda())
    assert again[1].tolist() == order.tolist() and again[2].tolist() == rank.tolist()


def test_live_order_reports_counts_that_are_not_the_masks():
    L = _lib()
    rng = np.random.default_rng(5)
    m = _masks_from_lengths(rng.integers(0, T + 1, 300))
    _, _, _, unf = _live_order(m.cuda())
    for t_bad, delta in ((9, -1), (0, 1)):
        expect = unf[:T].copy()
        expect[t_bad] += delta
        expect[T - 1] += 3                            # (the FIRST step that differs is named)
        status = torch.zeros(4, dtype=torch.int32, device="cuda")
        got = _live_order(m.cuda(), expect=expect, status=status)
        assert got[3].tolist() == unf.tolist()        # the outputs are the masks' whatever the caller expected
        assert status.cpu().tolist() == [L.STATUS_UNFINISHED_COUNT | t_bad, 0, 0, 0]


@pytest.mark.parametrize("S", [2, 4])
def test_linear_partials_rows_writes_the_mapped_rows_of_the_full_product_and_nothing_else(S):
    L = _lib()
    lib = L.load()
    N, K, NC = 300, 2048, 384
    g = torch.Generator(device="cuda").manual_seed(S)
    A = (torch.randn(N, K, device="cuda", generator=g) * 0.5).bfloat16()
    B = (torch.randn(NC, K, device="cuda", generator=g) * 0.5).bfloat16()
    full = torch.full((S, N, NC), float("nan"), device="cuda")
    L.check(lib.uic_linear_partials(L.BF16, N, NC, K, L.ptr(A), K, L.ptr(B), K, L.ptr(full), S, L.stream()))
    assert not torch.isnan(full).any()
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(11))
    nan_bits = torch.tensor([0x7FC0, 0xFFC1, 0x7F81, 0x7FFF], dtype=torch.int32).to(torch.int16)
    for M in (1, 127, 128, 129, 257, 300):
        rows = perm[:M].cuda()
        pad = (M + 127) // 128 * 128
        Ac = nan_bits.repeat(pad * K // 4).view(torch.bfloat16).view(pad, K).cuda().contiguous()   # stale rows [M, tile end): NaN patterns
        Ac[:M] = A[rows]
        assert torch.isnan(Ac[M:].float()).all()
        slab = torch.full((S, N, NC), SENTINEL, device="cuda")
        L.check(lib.uic_linear_partials_rows(L.BF16, M, NC, K, L.ptr(Ac), K, L.ptr(B), K, L.ptr(slab), S, L.ptr(rows.int()), N, L.stream()),
                "linear_partials_rows M=%d" % M)
        torch.cuda.synchronize()
        assert not torch.isnan(slab).any(), M
        assert torch.equal(slab[:, rows], full[:, rows]), M
        rest = torch.ones(N, dtype=torch.bool)
        rest[perm[:M]] = False
        assert (slab[:, rest.cuda()] == SENTINEL).all(), M
    # an entry outside [0, slab_rows) drops its row
    rows = perm[:5].clone().int()
    rows[2] = -1
    rows[4] = N
    slab = torch.full((S, N, NC), SENTINEL, device="cuda")
    L.check(lib.uic_linear_partials_rows(L.BF16, 5, NC, K, L.ptr(A[perm[:5].cuda()].contiguous()), K, L.ptr(B), K, L.ptr(slab), S, L.ptr(rows.cuda()), N,
                                         L.stream()))
    torch.cuda.synchronize()
    kept = perm[[0, 1, 3]].cuda()
    assert torch.equal(slab[:, kept], full[:, kept])
    assert int((slab != SENTINEL).any(2).sum()) == 3 * S


def _cell_inputs(M, H, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    gates = torch.cat([torch.sigmoid(r(M, H)), torch.sigmoid(r(M, H)), torch.tanh(r(M, H)), torch.sigmoid(r(M, H))], 1).bfloat16().contiguous()
    return dict(gates=gates, c_prev=r(M, H), c=r(M, H), dc=r(M, H) * 0.1, r=r)


def _row_lengths(M, t):
    return np.resize(np.array([0, t, t + 1, t + 2, T]), M)


def _poison(slab, rows):
    out = slab.clone()
    out[:, rows] = float("nan")
    return out


def test_lang_cell_backward_drops_the_slab_rows_of_ended_captions_and_stores_the_unfinished_rows_compactly():
    L = _lib()
    lib = L.load()
    M, H, t = 160, 512, 5
    x = _cell_inputs(M, H, 3)
    lens = _row_lengths(M, t)
    row_len, order, rank, unf = _live_order(_masks_from_lengths(lens).cuda())
    assert row_len.tolist() == lens.tolist()
    dh0 = x["r"](M, H)
    slabA0, slabB0 = x["r"](4, M, 3 * H), x["r"](4, M, 2 * H)
    dead_next = torch.from_numpy(lens <= t + 1).cuda()
    d_len, d_rank = torch.from_numpy(row_len).cuda(), torch.from_numpy(rank).cuda()

    def run(slabA, slabB, live=True):
        dc, dg = x["dc"].clone(), torch.full((M, 4 * H), SENTINEL, device="cuda").bfloat16()
        dgc = torch.full((M, 4 * H), SENTINEL, device="cuda").bfloat16()
        a = (L.ptr(slabA.view(-1)[2 * H:]), 3 * H, 4, M * 3 * H, L.ptr(slabB), 2 * H, 4, M * 2 * H)
        tail = (L.ptr(dc), L.ptr(x["gates"]), L.ptr(x["c_prev"]), L.ptr(x["c"]), L.ptr(dg))
        if live:
            L.check(lib.uic_lstm_cell_bwd_live(M, H, L.ptr(dh0), H, 0.5, 77, 9, *a, *tail, L.ptr(d_len), L.ptr(d_rank), t, L.ptr(dgc), L.stream()), "live")
        else:
            kid = C.c_int32(-1)
            L.check(lib.uic_lstm_cell_bwd_sources(L.BF16, M, H, L.ptr(dh0), H, 0.5, 77, 9, None, 0, None, 0, *a, *tail, C.byref(kid), L.stream()))
            assert kid.value == L.LSTM_BWD_VEC4_SIMPLE
        torch.cuda.synchronize()
        return dc, dg.view(torch.int16), dgc.view(torch.int16)

    zA, zB = slabA0.clone(), slabB0.clone()
    zA[:, dead_next] = 0.0
    zB[:, dead_next] = 0.0
    got = run(_poison(slabA0, dead_next), _poison(slabB0, dead_next))
    ref = run(zA, zB)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    assert not torch.isnan(got[0]).any() and not torch.isnan(got[1].view(torch.bfloat16).float()).any()
    # rows whose caption is unfinished: the operator without row_len on the zeroed slabs; ended rows: a zero row, d c untouched
    old = run(zA, zB, live=False)
    on = torch.from_numpy(lens > t).cuda()
    assert torch.equal(got[0][on], old[0][on]) and torch.equal(got[1][on], old[1][on])
    assert (got[1][~on] == 0).all() and torch.equal(got[0][~on], x["dc"][~on])
    # the compact copy: the unfinished rows in the order of their rank; nothing behind them
    n_on = int(unf[t])
    assert n_on == int(on.sum())
    assert torch.equal(got[2][:n_on], got[1][torch.from_numpy(order[:n_on]).long().cuda()])
    assert torch.equal(got[2][n_on:], torch.full((M - n_on, 4 * H), SENTINEL, device="cuda").bfloat16().view(torch.int16))


def test_h2att_cell_backward_drops_the_slab_rows_of_ended_captions_and_stores_the_unfinished_rows_compactly():
    L = _lib()
    lib = L.load()
    N, H, A, t = 150, 512, 512, 5
    x = _cell_inputs(N, H, 4)
    lens = _row_lengths(N, t)
    row_len, order, rank, unf = _live_order(_masks_from_lengths(lens).cuda())
    datth = (x["r"](N, A) * 0.1).bfloat16()
    h2attT = (x["r"](H, A) * 0.1).bfloat16()
    slabA0, slabB0 = x["r"](4, N, 3 * H), x["r"](4, N, 2 * H)
    dead_now, dead_next = torch.from_numpy(lens <= t).cuda(), torch.from_numpy(lens <= t + 1).cuda()
    d_len, d_rank = torch.from_numpy(row_len).cuda(), torch.from_numpy(rank).cuda()

    def run(slabA, slabB, live=True):
        dc, dg = x["dc"].clone(), torch.full((N, 4 * H), SENTINEL, device="cuda").bfloat16()
        dgc = torch.full((N, 4 * H), SENTINEL, device="cuda").bfloat16()
        a = (L.ptr(slabA.view(-1)[H:]), 3 * H, 4, N * 3 * H, L.ptr(slabB.view(-1)[H:]), 2 * H, 4, N * 2 * H)
        tail = (L.ptr(dc), L.ptr(x["gates"]), L.ptr(x["c_prev"]), L.ptr(x["c"]), L.ptr(dg))
        if live:
            L.check(lib.uic_h2att_cell_bwd_live(N, H, A, L.ptr(datth), L.ptr(h2attT), *a, *tail, L.ptr(d_len), L.ptr(d_rank), t, L.ptr(dgc), L.stream()), "live")
        else:
            L.check(lib.uic_h2att_cell_bwd(L.BF16, N, H, A, L.ptr(datth), L.ptr(h2attT), *a, *tail, L.stream()))
        torch.cuda.synchronize()
        return dc, dg.view(torch.int16), dgc.view(torch.int16)

    zA, zB = slabA0.clone(), slabB0.clone()
    zA[:, dead_now] = 0.0                             # this step's d x2: no rows for the captions that ended before it
    zB[:, dead_next] = 0.0                            # the next step's d x1
    got = run(_poison(slabA0, dead_now), _poison(slabB0, dead_next))
    ref = run(zA, zB)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    assert not torch.isnan(got[0]).any() and not torch.isnan(got[1].view(torch.bfloat16).float()).any()
    old = run(zA, zB, live=False)
    assert torch.equal(got[0], old[0]) and torch.equal(got[1], old[1])
    n_on = int(unf[t])
    assert n_on == int((lens > t).sum())
    assert torch.equal(got[2][:n_on], got[1][torch.from_numpy(order[:n_on]).long().cuda()])
    assert torch.equal(got[2][n_on:], torch.full((N - n_on, 4 * H), SENTINEL, device="cuda").bfloat16().view(torch.int16))
