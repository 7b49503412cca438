"""The cases of tests/lstm_cell_cases.py on the CPU (a condition: an edge nobody reaches is a hole in tests/test_gpu_lstm_cell.py).

* The case list reaches the three kernels of uic_lstm_cell_bwd_sources, and for every condition of the vec4 choice a case where
  that condition ALONE fails (the scalar kernel) beside cases where it holds; the shapes are the smallest that reach their edge.
* A float32 restatement of the kernels' formulas, with a correctly rounded tanh and with the bf16 path's 1 - 2 / (1 + 2^(kx)), stays
  within C / 4 = 8 units of eps x the element's magnitude on the inputs of EVERY GPU case -- room for the hardware's exp / rcp and
  another contraction, none for a wrong term.  Measured maximum over all cases and both dtypes: 6.50 in the exp form (d_o of
  shape-65536x4-general) and 5.43 with tanhf (d_i of mis-strideB); the maxout cell 4.05, the fused operator 2.66.
* The reference equals float64 autograd through sigmoid / tanh of pre-activations on an unsaturated cell, which ties it to the
  reference of tests/test_gpu_ops.py::test_lstm_cell_fwd_bwd; the maxout reference equals autograd through torch.max.
* Each planted mistake of a source, a slice, the dropout index or c_prev leaves the bound by orders of magnitude.
"""
import numpy as np
import pytest
import torch

import lstm_cell_cases as LC

CELL, MAXOUT, FUSED = LC.cell_cases(), LC.maxout_cases(), LC.fused_cases()
EVERY = [(c, dt) for c in LC.all_cases() for dt in c.dtypes]
WORST = {}


def test_the_cases_reach_every_kernel_and_both_sides_of_every_condition():
    kinds = {(LC.classify(c, dt), dt) for c in CELL for dt in c.dtypes}
    assert kinds == {(k, dt) for k in (LC.SCALAR, LC.VEC4, LC.VEC4_SIMPLE) for dt in (LC.F32, LC.BF16)}
    for dt in (LC.F32, LC.BF16):
        alone = {}
        for c in CELL:
            bad = LC.broken_conditions(c, dt)
            if len(bad) == 1:
                alone.setdefault(next(iter(bad)), []).append(c.name)
        missing = [k for k in LC.CELL_CONDITIONS if k not in alone]
        assert not missing, (dt, missing)
        # ... and the same configuration with the condition in place runs vec4: every scalar-by-one-condition case at the first vec4
        # size differs from a vec4 case only in what its name says
        assert LC.classify(LC.Case("x", nA=2, nB=2, **LC.GEN), dt) == LC.VEC4
    by = {c.name: c for c in CELL}
    # gates and dgates 8 bytes off: bf16 reads them as 8-byte pairs, f32 needs 16
    for n in ("mis-gates8", "mis-dgates8"):
        assert LC.classify(by[n], LC.BF16) == LC.VEC4_SIMPLE and LC.classify(by[n], LC.F32) == LC.SCALAR
    assert LC.classify(by["mis-gates8-both"], LC.BF16) == LC.VEC4 and LC.classify(by["mis-gates8-both"], LC.F32) == LC.SCALAR
    for n in ("mis-gates4", "mis-dgates4"):
        assert LC.classify(by[n], LC.BF16) == LC.classify(by[n], LC.F32) == LC.SCALAR
    # the variants
    expect = {"shape-128x512-simple": LC.VEC4_SIMPLE, "src-dh012": LC.VEC4, "src-no-dh0": LC.VEC4, "src-no-cprev": LC.VEC4, "src-none": LC.VEC4,
              "slab-att-cell": LC.VEC4_SIMPLE, "slab-general": LC.VEC4, "slab-nA5": LC.SCALAR, "slab-nB5": LC.SCALAR, "drop-simple": LC.VEC4_SIMPLE,
              "drop-general": LC.VEC4, "sat-simple": LC.VEC4_SIMPLE, "sat-general": LC.VEC4, "smallcp-simple": LC.VEC4_SIMPLE,
              "smallcp-general": LC.VEC4, "far-slabA": LC.SCALAR, "far-dh0": LC.SCALAR, "far-dh1": LC.SCALAR, "far-dh2": LC.SCALAR, "far-slabB": LC.SCALAR, "sat-scalar": LC.SCALAR, "smallcp-scalar": LC.SCALAR}
    for nA in (1, 2, 4):
        for nB in (0, 3, 4):
            expect["slab-%d-%d" % (nA, nB)] = LC.VEC4_SIMPLE
    for n, k in expect.items():
        for dt in (LC.F32, LC.BF16):
            assert LC.classify(by[n], dt) == k, (n, dt)
    for n in ("far-slabA", "far-dh0", "far-dh1", "far-dh2", "far-slabB"):          # each kind of source beyond 2^31 bytes, nothing else wrong
        for dt in (LC.F32, LC.BF16):
            assert LC.broken_conditions(by[n], dt) == {"near"} and by[n].far, n
        big = [t for t, l in LC.layout(by[n], LC.F32).items() if l["sparse"]]
        assert big == [n[4:]], (n, big)
    lay = LC.layout(by["far-slabA"], LC.F32)["slabA"]
    assert lay["strides"][0] * 4 == 2 ** 31 and lay["elems"] * 4 < 2 ** 31 + 2 ** 22       # slice 1 at byte 2^31; just over 2 GiB
    # drop_p on both sides, with the site of a decode step; strided sources as Step::bwd_step passes them
    assert {c.drop_p for c in CELL} == {0.0, 0.5} and all(c.site >= LC.SITE_OUT0 for c in CELL if c.drop_p)
    assert by["src-dh012"].dh[1] == (3 * 512, 2 * 512) and by["src-dh012"].dh[2] == (2 * 512, 0)
    assert by["slab-1-0"].layA == (3 * 512, 2 * 512) and by["slab-1-3"].layB == (2 * 512, 0)


def test_the_shapes_are_the_smallest_that_reach_their_edge():
    shapes = {(c.M, c.H): c for c in CELL if c.name.startswith("shape-") and c.name.endswith("-simple")}
    kind = {k: LC.classify(c, LC.BF16) for k, c in shapes.items()}
    assert 128 * 512 == LC.VEC_MIN and kind[(128, 512)] == LC.VEC4_SIMPLE             # the first vec4 size ...
    assert 127 * 512 == LC.VEC_MIN - 512 and kind[(127, 512)] == LC.SCALAR            # ... and one row less
    assert LC.vec4_geometry(128) == (64, 1, 32) and kind[(512, 128)] == LC.VEC4_SIMPLE        # a 64-thread workgroup, half of it live
    assert LC.vec4_geometry(512) == (128, 1, 128)
    assert LC.vec4_geometry(516) == (192, 1, 129) and kind[(128, 516)] == LC.VEC4_SIMPLE      # one lane into the third wave
    assert LC.vec4_geometry(1028) == (256, 2, 1) and kind[(64, 1028)] == LC.VEC4_SIMPLE       # a second workgroup in x, one live lane
    assert 64 * 1028 >= LC.VEC_MIN > 63 * 1028
    assert 64 * 1030 >= LC.VEC_MIN and LC.broken_conditions(shapes[(64, 1030)], LC.BF16) == {"h4", "dh0_ld"}
    assert LC.broken_conditions(shapes[(65536, 4)], LC.BF16) == {"rows"} and kind[(65535, 4)] == LC.VEC4_SIMPLE
    assert LC.broken_conditions(shapes[(6, 32)], LC.F32) == {"size"} and LC.broken_conditions(shapes[(33, 96)], LC.F32) == {"size"}
    for (M, H), c in shapes.items():
        g = next(x for x in CELL if x.name == "shape-%dx%d-general" % (M, H))
        assert LC.classify(g, LC.BF16) == (LC.VEC4 if kind[(M, H)] != LC.SCALAR else LC.SCALAR)


def test_the_fused_cases_reach_every_k_split_every_tail_and_every_refusal():
    assert {c.A // 128 for c in FUSED} == {1, 2, 4}
    assert {(c.A, c.M) for c in FUSED} >= {(A, N) for A in LC.FUSED_A for N in LC.FUSED_N}
    assert sorted({-c.M % LC.FT for c in FUSED if c.M in LC.FUSED_N}) == [0, 1, 31] and [-n % LC.FT for n in LC.FUSED_N] == [31, 1, 0, 31, 31]
    assert {(c.H, c.nA, c.nB) for c in FUSED} >= {(H, a, b) for H in LC.FUSED_H for a, b in LC.FUSED_SLABS}
    for A in LC.FUSED_A:                                                     # every K split with and without each slab source
        assert {(c.nA > 0, c.nB > 0) for c in FUSED if c.A == A} >= {(True, True), (True, False), (False, False)}
    assert any(c.cprev == "no" for c in FUSED) and any(c.gscale == 8 for c in FUSED)
    for c in FUSED:
        assert not LC.fused_broken(c, LC.BF16), c
        lay = LC.layout(c, LC.BF16)
        assert lay["dgates"]["elems"] - lay["dgates"]["start"] - LC.PAD == -(-c.M // LC.FT) * LC.FT * 4 * c.H     # whole tiles of rows
    reasons = []
    for c, dt, why in LC.fused_refused():
        assert LC.fused_broken(c, dt) == {why}, (c, LC.fused_broken(c, dt))
        reasons.append(why)
    assert set(LC.FUSED_REFUSALS_ASKED) <= set(reasons) and set(reasons) == set(LC.FUSED_CONDITIONS) - {"rows"}      # (N = 0 is a no-op, N < 0 an argument error)


def test_the_maxout_cases():
    assert {(c.M, c.H) for c in MAXOUT} == {(5, 40), (128, 512), (33, 96)}
    assert {(c.dh[0] is not None, c.dh[1] is not None, c.drop_p) for c in MAXOUT} >= {(a, b, p) for a in (True, False) for b in (True, False)
                                                                                    for p in (0.0, 0.5)}
    assert any(c.cprev == "no" for c in MAXOUT)
    for c in MAXOUT:
        first = LC.inputs(c, LC.BF16).gates[:, 4]
        assert set(np.unique(first)) == {0.0, 1.0}                           # both sides of the flag within one call


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print("\n[lstm cell, host] %-8s %-6s worst error in units of eps x magnitude: %.3f (%s, %s)" % (k + WORST[k]))


def _unit_ratio(got, ref, tol_f32):
    """error in units of eps x magnitude: C times the share of the f32 tolerance."""
    return LC.C_BOUND * LC.worst_ratio(got, ref, tol_f32)


@pytest.mark.parametrize("c,dt", EVERY, ids=["%s-%s" % (c.name, ("f32", "bf16")[dt]) for c, dt in EVERY])
def test_float32_restatement_stays_within_a_quarter_of_the_bound(c, dt):
    x = LC.inputs(c, dt)
    mask = LC.host_mask(c)
    ref, tol = LC.reference(x, mask, out_bf16=False)
    for form in ("tanhf", "exp"):
        got = LC.restated_f32(x, mask, form)
        assert list(got) == list(ref)
        for n in ref:
            r = _unit_ratio(got[n], ref[n], tol[n])
            WORST[(c.op, form)] = max(WORST.get((c.op, form), (0.0,)), (r, c.name, n))
            assert r <= LC.C_BOUND / 4, (c.name, form, n, r)


def test_saturated_inputs_are_saturated():
    by = {c.name: c for c in CELL}
    x = LC.inputs(by["sat-simple"], LC.BF16)
    g = x.gates
    for q, vals in ((0, (1.0,)), (1, (1.0,)), (2, (-1.0, 1.0)), (3, (1.0,))):
        for v in vals:
            assert (g[:, q] == v).mean() > 0.02, (q, v)                      # stored gates exactly 1 or -1: gi (1 - gi) and 1 - gg^2 are 0
    tc = np.tanh(x.c.astype(np.float64))
    assert (1 - tc * tc < 2.0 ** -24).mean() > 0.1                            # 1 - tc^2 is pure cancellation there
    s = LC.inputs(by["smallcp-simple"], LC.F32)
    assert np.abs(s.c_prev).max() < 1e-2 and np.abs(s.c_prev).mean() > 1e-4


def _planted(x, mask, what):
    import copy
    y = copy.copy(x)
    if what == "drop dh2":
        y.dh = [x.dh[0], x.dh[1], None]
    elif what == "last slice of A dropped":
        y.slabA = x.slabA[:-1]
    elif what == "double dh1":
        y.dh = [x.dh[0], 2 * x.dh[1], x.dh[2]]
    elif what == "c for c_prev":
        y.c_prev = x.c
    elif what == "last slice of B dropped":
        y.slabB = x.slabB[:-1]
    return LC.reference(y, mask)[0]


@pytest.mark.parametrize("what", ["drop dh2", "last slice of A dropped", "double dh1", "c for c_prev", "last slice of B dropped"])
def test_a_planted_mistake_leaves_the_bound(what):
    c = next(c for c in CELL if c.name == "slab-general")
    for dt in (LC.F32, LC.BF16):
        x = LC.inputs(c, dt)
        ref, tol = LC.reference(x, None)
        wrong = _planted(x, None, what)
        assert max(LC.worst_ratio(wrong[n], ref[n], tol[n]) for n in ref) > 10, (what, dt)
    sm = next(c for c in CELL if c.name == "smallcp-simple")               # the forget-gate gradient under a small c_prev
    x = LC.inputs(sm, LC.BF16)
    ref, tol = LC.reference(x, None)
    wrong = _planted(x, None, "c for c_prev")
    assert LC.worst_ratio(wrong["d_f"], ref["d_f"], tol["d_f"]) > 100
    whole = np.abs(np.stack([wrong[n] - ref[n] for n in ("d_i", "d_f", "d_g", "d_o")])).max() / np.abs(np.stack([ref[n] for n in ("d_i", "d_f", "d_g", "d_o")])).max()
    assert whole < 1.0                                                        # (a whole-tensor norm sees it only as a share of the largest element)


def test_a_wrong_dropout_index_leaves_the_bound():
    c = next(c for c in CELL if c.name == "drop-simple")
    x = LC.inputs(c, LC.F32)
    mask = LC.host_mask(c)
    assert 0.4 < (mask == 0).mean() < 0.6 and set(np.unique(mask)) == {0.0, 2.0}
    ref, tol = LC.reference(x, mask)
    wrong = LC.reference(x, np.broadcast_to(mask[0], mask.shape))[0]        # the unit for the element index: every row gets row 0's mask
    assert LC.worst_ratio(wrong["dc"], ref["dc"], tol["dc"]) > 100


def test_reference_equals_float64_autograd_through_preactivations():
    rng = np.random.default_rng(3)
    M, H = 7, 12
    z = torch.from_numpy(rng.standard_normal((M, 4, H))).requires_grad_()
    cp = torch.from_numpy(rng.standard_normal((M, H))).requires_grad_()
    gi, gf, gg, go = torch.sigmoid(z[:, 0]), torch.sigmoid(z[:, 1]), torch.tanh(z[:, 2]), torch.sigmoid(z[:, 3])
    c = gf * cp + gi * gg
    h = go * torch.tanh(c)
    x = LC.Inputs()
    x.M, x.H, x.op, x.dtype = M, H, "cell", LC.F32
    x.dh = [rng.standard_normal((M, H)), rng.standard_normal((M, H)) * 1e-2, None]
    x.slabA = rng.standard_normal((2, M, H))
    x.slabB, x.datth, x.h2attT = None, None, None
    x.dc = rng.standard_normal((M, H))
    x.gates = torch.stack([gi, gf, gg, go], 1).detach().numpy()
    x.c, x.c_prev = c.detach().numpy(), cp.detach().numpy()
    dh = x.dh[0] + x.dh[1] + x.slabA.sum(0)
    ((h * torch.from_numpy(dh)).sum() + (c * torch.from_numpy(x.dc)).sum()).backward()
    ref, _ = LC.reference(x, None)
    for q, n in enumerate(("d_i", "d_f", "d_g", "d_o")):
        np.testing.assert_allclose(ref[n], z.grad[:, q].numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(ref["dc"], cp.grad.numpy(), rtol=1e-12, atol=1e-14)


def test_maxout_reference_equals_float64_autograd():
    rng = np.random.default_rng(4)
    M, H = 6, 10
    z = torch.from_numpy(rng.standard_normal((M, 5, H))).requires_grad_()
    cp = torch.from_numpy(rng.standard_normal((M, H))).requires_grad_()
    gi, gf, go = torch.sigmoid(z[:, 0]), torch.sigmoid(z[:, 1]), torch.sigmoid(z[:, 2])
    g = torch.max(z[:, 3], z[:, 4])                                          # P/models/FCModel_NMT.py:41-43
    c = gf * cp + gi * g
    keep = torch.from_numpy(np.where(rng.random((M, H)) < 0.5, 0.0, 2.0))
    h = go * torch.tanh(c) * keep                                            # :45-47, the dropped next_h is output and state
    x = LC.Inputs()
    x.M, x.H, x.op, x.dtype = M, H, "maxout", LC.F32
    x.dh = [rng.standard_normal((M, H)), rng.standard_normal((M, H)) * 1e-2, None]
    x.slabA = x.slabB = x.datth = x.h2attT = None
    x.dc = rng.standard_normal((M, H))
    x.gates = torch.stack([gi, gf, go, g, (z[:, 3] >= z[:, 4]).double()], 1).detach().numpy()
    x.c, x.c_prev = c.detach().numpy(), cp.detach().numpy()
    ((h * torch.from_numpy(x.dh[0] + x.dh[1])).sum() + (c * torch.from_numpy(x.dc)).sum()).backward()
    ref, _ = LC.reference(x, keep.numpy())
    for q, n in enumerate(("d_i", "d_f", "d_o", "d_g1", "d_g2")):
        np.testing.assert_allclose(ref[n], z.grad[:, q].numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(ref["dc"], cp.grad.numpy(), rtol=1e-12, atol=1e-14)


def test_fused_reference_is_the_gemm_plus_the_slabs():
    c = next(c for c in FUSED if c.name == "fused-H96-s12")
    x = LC.inputs(c, LC.BF16)
    terms, S = LC.dh_terms(x, None)
    a, b = x.datth.astype(np.float64), x.h2attT.astype(np.float64)
    np.testing.assert_allclose(sum(terms), a @ b.T + x.slabA.astype(np.float64).sum(0) + x.slabB.astype(np.float64).sum(0), rtol=1e-13, atol=1e-15)
    assert (S >= np.abs(sum(terms))).all()
    assert (x.datth == LC.round_to(x.datth, LC.BF16)).all() and (x.gates == LC.round_to(x.gates, LC.BF16)).all()
