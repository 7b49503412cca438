"""Full-size parity of BASELINE.json configs[1] (128 images x 5 captions = 640 caption rows, R = 36, D = 2048, H = E = A = 512,
vocabulary 9487 + 1, 17 decode steps) against the CPU oracle -- not properties, the oracle's own numbers: log-probs, loss,
the norm of every gradient tensor and three gradient tensors entry by entry -- and of the persistent recurrence kernels
(csrc/rnn_persist.hip: the decode loop, csrc/rnn_bwd_persist.hip: its BPTT) against the per-step launch chains they replace,
under both of their exchange protocols.
The step that bench.py times -- the list of live positions made on the device, training-mode dropout 0.5, and in bf16 the
persistent kernel's own store of the live hdrop rows into the compact logit operand (Step::fused_gather, csrc/topdown_step.hip) -- is
compared with the oracle here as well: test_configs1_full_size_step_over_live_positions_vs_oracle and
test_full_size_benchmark_dropout_step_vs_oracle (tests/test_gpu_live_persist.py holds the edges at 512 hidden units).
Tolerances (north_star): log-probs 1e-3 (f32) / 1e-2 (bf16)."""
import numpy as np
import pytest
import torch

from conftest import poison_workspaces

from oracle import topdown as O
from test_gpu_topdown import build_model

pytestmark = pytest.mark.gpu

V, E, H, A, D, L, R = 9487, 512, 512, 512, 2048, 16, 36
CFG = dict(V=V, E=E, H=H, A=A, D=D, L=L)
LOGP_TOL = {"f32": 1e-3, "bf16": 1e-2}
# Gradients: L2 error of every tensor relative to max(|oracle tensor|_2, floor), floor = 1e-3 x the largest tensor norm of the
# model (h2att / alpha_net gradients are cancellations of size 1e-10 at random initialisation and are compared at the model's
# scale, not their own).  Measured on MI355X at these shapes: f32 1.2e-6, bf16 6.0e-3; the bounds are ~3x that.
GRAD_TOL = {"f32": 4e-6, "bf16": 2e-2}
FULL_TENSORS = ["core.att_lstm.weight_hh", "core.attention.h2att.weight", "ctx2att.weight"]


def _lib():
    from unpaired_image_captioning_amd import _lib as L_
    return L_


def seed_after(counter):
    """The seed model.next_seed() draws when model._seed_counter == counter (models/AttModel.py)."""
    return (counter * 1103515245 + 12345) & 0x7FFFFFFF


def kernel_dropout_masks(seed, N, R, T, H, E, p=0.5):
    """The masks the kernels themselves apply under `seed` (uic_dropout_mask: a hash of seed, site and element index -- not of
    the dtype, the list of live positions or the way the recurrence is launched), in the layout the oracle's `drop` takes."""
    Lb = _lib()
    lib = Lb.load()

    def mask(n, site):
        out = torch.empty(n, device="cuda")
        Lb.check(lib.uic_dropout_mask(Lb.ptr(out), n, p, seed, site, 0, Lb.stream()))
        return out.cpu()

    return dict(fc=mask(N * H, Lb.SITE_FC).view(N, H), att=mask(N * R * H, Lb.SITE_ATT).view(N, R, H),
                embed=mask(T * N * E, Lb.SITE_EMBED).view(T, N, E),
                out=torch.stack([mask(N * H, Lb.SITE_OUT0 + t).view(N, H) for t in range(T)]))


def with_live(batch, live):
    """The batch as xe_step takes it: live = None (every position), "rows" (the caller's own list, live_positions) or
    "device" (counts only, the way Trainer.attach_live does it: the step compacts the masks itself)."""
    from unpaired_image_captioning_amd.topdown_engine import live_positions
    from unpaired_image_captioning_amd.trainer import Trainer
    b = {k: v for k, v in batch.items() if not k.startswith("live_")}
    if live == "rows":
        b["live_rows"], b["live_count"] = live_positions(b["masks"])
    elif live == "device":
        Trainer.attach_live(b)
        assert "live_rows" not in b
    else:
        assert live is None, live
    return b


def grad_errors(grads, ref_grads):
    """{tensor: L2 error relative to max(|oracle tensor|_2, 1e-3 x the largest tensor norm of the model)} (see GRAD_TOL)."""
    floor = 1e-3 * max(float(v.norm()) for v in ref_grads.values())
    return {k: ((grads[k].float().cpu().double() - r.double()).norm() / max(r.double().norm().item(), floor)).item() for k, r in ref_grads.items()}


def assert_step_vs_oracle(tag, loss, grads, ref_loss, ref_grads, dtype):
    """Loss, every per-tensor gradient norm, every tensor in L2 and the three FULL_TENSORS by their worst entry."""
    assert abs(loss - ref_loss) < LOGP_TOL[dtype], (tag, loss, ref_loss)
    floor = 1e-3 * max(float(v.norm()) for v in ref_grads.values())
    worst = max(grad_errors(grads, ref_grads).values())
    print("%s: loss %.6f (oracle %.6f), worst per-tensor L2 gradient error %.3e" % (tag, loss, ref_loss, worst))
    for k, r in ref_grads.items():
        g = grads[k].float().cpu().double()
        r = r.double()
        # per-tensor gradient norm
        assert abs(g.norm().item() - r.norm().item()) <= GRAD_TOL[dtype] * max(r.norm().item(), floor), (k, g.norm().item(), r.norm().item())
    # every tensor entry by entry (L2), three of them also by their worst entry on the f32 path
    for k, r in ref_grads.items():
        g = grads[k].float().cpu().double()
        r = r.double()
        assert ((g - r).norm() / max(r.norm().item(), floor)).item() < GRAD_TOL[dtype], k
    efloor = 1e-3 * max(float(v.abs().max()) for v in ref_grads.values())
    for k in FULL_TENSORS:
        g = grads[k].float().cpu().double()
        r = ref_grads[k].double()
        err = ((g - r).abs().max() / max(r.abs().max().item(), efloor)).item()
        print("   %s: worst entry error %.3e" % (k, err))
        assert err < (2e-5 if dtype == "f32" else 5e-2), k


@pytest.fixture(scope="module")
def case():
    """Weights, the 640-row batch, and the oracle's forward + loss + backward on it (CPU, ~10 s)."""
    torch.manual_seed(0)
    W = O.init_weights(V + 1, E, H, A, D, D, seed=7)
    b = O.synthetic_batch(128, 5, R, D, V, L, seed=1234, ragged_regions=True)
    nt = torch.get_num_threads()
    torch.set_num_threads(min(16, nt))
    loss, grads, logp = O.xe_loss_and_grads(W, b["fc_feats"], b["att_feats"], b["labels"], b["masks"], b["att_masks"])
    torch.set_num_threads(nt)
    return W, b, float(loss), grads, logp


# uic_topdown_dims.recurrence: per-step launches everywhere / the default (persistent forward recurrence) / the same with
# the SAFE exchange protocol / UIC_REC_EARLY_GRADS (three streams, the embedding gradient in two halves).  (The persistent BPTT
# kernel serves the single-stream backward call only -- test_persistent_bptt_equals_the_launch_chain -- the fused step ignores
# UIC_REC_BWD_PERSIST.)
REC_MODES = {"chain": 1, "default": 0, "safe": 4, "early": 16}


@pytest.mark.parametrize("mode", list(REC_MODES))
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_configs1_full_size_vs_oracle(case, dtype, mode):
    """Forward call, fused training step (loss, every gradient) at BASELINE configs[1] size against the oracle, in every
    way the library can launch the recurrence (REC_MODES)."""
    from unpaired_image_captioning_amd.trainer import xe_step
    Lb = _lib()
    W, b, ref_loss, ref_grads, ref_logp = case
    batch = {k: v.cuda() for k, v in b.items()}
    model = build_model(CFG, W, dtype)
    model.train()                                    # drop_prob_lm = 0: deterministic
    model.engine.recurrence = REC_MODES[mode]
    poison_workspaces(model.engine)                  # no mode may live on what an earlier, identical run left in memory
    before = Lb.persistent_status()
    try:
        logp = model(batch["fc_feats"], None, batch["att_feats"], batch["labels"], batch["att_masks"])
        t_run = model._steps_to_run(batch["labels"])
        # log-probs: every row and step on a strided subset of the vocabulary, and the target entries
        cols = torch.arange(0, V + 1, 37)
        got = logp[:, :t_run][:, :, cols.cuda()].float().cpu()
        assert (got - ref_logp[:, :t_run][:, :, cols]).abs().max().item() < LOGP_TOL[dtype]
        tgt = batch["labels"][:, 1:t_run + 1]
        got_t = logp[:, :t_run].gather(2, tgt.unsqueeze(2)).float().cpu()
        assert (got_t - ref_logp[:, :t_run].gather(2, b["labels"][:, 1:t_run + 1].unsqueeze(2))).abs().max().item() < LOGP_TOL[dtype]
        loss, grads = xe_step(model, batch)
        assert abs(loss.item() - ref_loss) < LOGP_TOL[dtype]
        st = Lb.persistent_status()
    finally:
        model.engine.recurrence = 0
    assert st[0] == 0
    launches = (st[1] - before[1], st[2] - before[2])            # (XCD-local, SAFE) persistent launches of this test
    want = {"chain": (0, 0), "default": (2, 0), "safe": (0, 2), "early": (2, 0)}[mode]
    assert launches == want, (mode, launches, want)
    assert_step_vs_oracle("full size %s mode %s" % (dtype, mode), loss.item(), grads, ref_loss, ref_grads, dtype)


@pytest.mark.parametrize("mode", ["default", "chain", "early"])
@pytest.mark.parametrize("live", ["device", "rows"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_configs1_full_size_step_over_live_positions_vs_oracle(case, dtype, live, mode):
    """The same 640-row batch and oracle run as test_configs1_full_size_vs_oracle, the fused step handed the list of live
    positions -- made on the device from the counts (what bench.py times; in bf16 with the persistent kernel the recurrence then
    stores the live hdrop rows into the compact logit operand itself) or the caller's own list -- under the same bounds.  The
    persistent launches each mode implies are counted: a silent fall-back to the launch chain does not pass."""
    from unpaired_image_captioning_amd.trainer import xe_step
    Lb = _lib()
    W, b, ref_loss, ref_grads, _ = case
    batch = with_live({k: v.cuda() for k, v in b.items()}, live)
    assert int(batch["live_count"].sum()) < b["masks"][:, 1:].numel()         # (the list leaves positions out)
    model = build_model(CFG, W, dtype)
    model.train()                                    # drop_prob_lm = 0: deterministic
    model.engine.recurrence = REC_MODES[mode]
    poison_workspaces(model.engine)
    before = Lb.persistent_status()
    try:
        loss, grads = xe_step(model, batch)
        st = Lb.persistent_status()
    finally:
        model.engine.recurrence = 0
    assert st[0] == 0
    launches = (st[1] - before[1], st[2] - before[2])            # (XCD-local, SAFE) persistent launches of this test
    want = {"chain": (0, 0), "default": (1, 0), "early": (1, 0)}[mode]
    assert launches == want, (mode, launches, want)
    assert_step_vs_oracle("full size %s, list: %s, mode %s" % (dtype, live, mode), loss.item(), grads, ref_loss, ref_grads, dtype)


DROP_SEED_COUNTER = 640512            # model._seed_counter in front of the dropout step below: one set of masks for both dtypes


@pytest.fixture(scope="module")
def case_drop(case):
    """The oracle on the 640-row batch of `case` under the dropout masks (p = 0.5) the kernels apply for the seed that follows
    DROP_SEED_COUNTER (CPU, ~15 s)."""
    W, b, *_ = case
    seed = seed_after(DROP_SEED_COUNTER)
    drop = kernel_dropout_masks(seed, b["labels"].shape[0], R, L + 1, H, E)
    keep = drop["out"].flatten()
    assert 0.45 < (keep > 0).float().mean().item() < 0.55 and set(keep.unique().tolist()) <= {0.0, 2.0}
    nt = torch.get_num_threads()
    torch.set_num_threads(min(16, nt))
    loss, grads, _ = O.xe_loss_and_grads(W, b["fc_feats"], b["att_feats"], b["labels"], b["masks"], b["att_masks"], drop)
    torch.set_num_threads(nt)
    return seed, float(loss), grads


# Gradients of the 640-row step under dropout 0.5 (L2 per tensor, floors as GRAD_TOL): GRAD_TOL's own bounds hold.  Measured on an
# MI355X against the oracle, worst tensor: f32 1.34e-6 (launch chain over every position 1.39e-6); bf16 8.75e-3 (launch chain
# 8.71e-3, fc_embed.0.weight) -- against 6.0e-3 at drop 0, so 2e-2 stands and no 3 x launch-chain bound is needed.


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_full_size_benchmark_dropout_step_vs_oracle(case, case_drop, dtype):
    """What bench.py times, against the oracle: 640 caption rows with ragged region counts, model.train() with drop_prob_lm =
    0.5, the list made on the device (Trainer.attach_live), the default recurrence -- in bf16 that is Step::fused_gather.  The
    oracle is fed the kernels' own masks.  Beside it the oldest path -- the per-step launch chain over every position, with
    neither the persistent kernel nor the list -- on the same batch and seed: the step over the live positions agrees with it
    within tests/test_live_positions.py's bounds."""
    from test_live_positions import _same
    from unpaired_image_captioning_amd.trainer import xe_step
    Lb = _lib()
    W, b, *_ = case
    seed, ref_loss, ref_grads = case_drop
    batch = {k: v.cuda() for k, v in b.items()}
    model = build_model(CFG, W, dtype, drop=0.5)
    model.train()
    poison_workspaces(model.engine)
    out = {}
    try:
        for name, rec, live, want in (("chain, every position", Lb.REC_FWD_CHAIN, None, (0, 0)), ("list made on the device", 0, "device", (1, 0))):
            model.engine.recurrence = rec
            model._seed_counter = DROP_SEED_COUNTER
            before = Lb.persistent_status()
            loss, grads, got_seed = xe_step(model, with_live(batch, live), return_seed=True)
            st = Lb.persistent_status()
            assert got_seed == seed
            assert st[0] == 0 and (st[1] - before[1], st[2] - before[2]) == want, (name, before, st)
            errs = grad_errors(grads, ref_grads)
            worst = max(errs, key=errs.get)
            print("full size %s, dropout 0.5, %s: loss %.6f (oracle %.6f), worst per-tensor L2 gradient error %.3e (%s)" %
                  (dtype, name, loss.item(), ref_loss, errs[worst], worst))
            out[name] = (loss.item(), {k: g.detach().clone() for k, g in grads.items()}, errs)
    finally:
        model.engine.recurrence = 0
    (l0, g0, e0), (l1, g1, e1) = out["chain, every position"], out["list made on the device"]
    assert abs(l1 - ref_loss) < LOGP_TOL[dtype], (l1, ref_loss)
    for k, err in e1.items():
        assert err < GRAD_TOL[dtype], (k, err, e0[k])
    _same(g1, g0, 2e-5 if dtype == "f32" else 2e-3)


@pytest.mark.parametrize("mode", ["default", "chain", "early"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_training_step_is_bit_reproducible(case, dtype, mode):
    """The same 640-row step three times with training-mode dropout (fixed seed): the loss and EVERY gradient tensor bit for
    bit -- incl. `embed.0.weight`, the backward of nn.Embedding (P/models/AttModel.py:73-75,160), which is a stable counting sort
    of the token positions with one owner per table row (csrc/embedding.hip), not floating-point atomics.  The padding token 0
    owns thousands of positions here (a bucket that straddles many gather workgroups) and most words one or two."""
    from unpaired_image_captioning_amd.trainer import xe_step
    W, b, *_ = case
    batch = {k: v.cuda() for k, v in b.items()}
    assert int((b["labels"][:, 1:] == 0).sum()) > 1000
    model = build_model(CFG, W, dtype, drop=0.5)
    model.train()
    model.engine.recurrence = REC_MODES[mode]
    runs = []
    try:
        for rep in range(3):
            model._seed_counter = 77
            model.zero_grad()
            poison_workspaces(model.engine)
            loss, grads = xe_step(model, batch)
            runs.append((loss.item(), {k: g.detach().clone() for k, g in grads.items()}))
    finally:
        model.engine.recurrence = 0
    for loss, grads in runs[1:]:
        assert loss == runs[0][0]
        for k, g in grads.items():
            assert torch.equal(g, runs[0][1][k]), (k, (g.double() - runs[0][1][k].double()).abs().max().item())
    assert float(runs[0][1]["embed.0.weight"].abs().max()) > 0


def test_training_step_reproduces_beside_busy_neighbours(case):
    """The default bf16 step 40 times while an HBM-bound copy and an MFMA-bound GEMM run on another stream: the timing inside
    every kernel changes from run to run, the bits must not (a counted wait one short, a hand-off without its fence or store
    data overwritten early shows up exactly here -- tools/step_repro_soak.py is the long form, tools/gemm_f32a_soak.py found
    such a bug in the first f32-A GEMM)."""
    from unpaired_image_captioning_amd.trainer import xe_step
    W, b, *_ = case
    batch = {k: v.cuda() for k, v in b.items()}
    model = build_model(CFG, W, "bf16", drop=0.5)
    model.train()
    side = torch.cuda.Stream()
    hog_a = torch.randn(32 << 20, device="cuda")
    hog_b = torch.empty_like(hog_a)
    X = torch.randn(4096, 4096, device="cuda").bfloat16()
    ref = None
    for it in range(40):
        with torch.cuda.stream(side):
            if it % 2 == 0:
                hog_b.copy_(hog_a)
            if it % 3 != 0:
                torch.matmul(X, X)
        model._seed_counter = 4242
        loss, grads = xe_step(model, batch)
        torch.cuda.synchronize()
        if ref is None:
            ref = (loss.clone(), {k: g.clone() for k, g in grads.items()})
            continue
        assert torch.equal(loss, ref[0]), it
        for k, g in grads.items():
            assert torch.equal(g, ref[1][k]), (it, k)


def test_step_without_the_f32a_gemm_is_bit_identical(case):
    """UIC_REC_NO_F32A (include/uic_hip.h): att_embed as cast + bf16 GEMM instead of the GEMM that rounds its f32 A operand in
    flight -- the fallback for that kernel's hand-counted register loads.  Both forms round the same values
    the same way and accumulate in the same order: every gradient must be the same bits."""
    from unpaired_image_captioning_amd import _lib as Lb
    from unpaired_image_captioning_amd.trainer import xe_step
    W, b, *_ = case
    batch = {k: v.cuda() for k, v in b.items()}
    model = build_model(CFG, W, "bf16", drop=0.5)
    model.train()
    out = []
    for rec in (0, Lb.REC_NO_F32A):
        model.engine.recurrence = rec
        model._seed_counter = 77
        loss, grads = xe_step(model, batch)
        torch.cuda.synchronize()
        out.append((loss.clone(), {k: g.clone() for k, g in grads.items()}))
    model.engine.recurrence = 0
    assert torch.equal(out[0][0], out[1][0])
    for k in out[0][1]:
        assert torch.equal(out[0][1][k], out[1][1][k]), k


@pytest.mark.parametrize("M,N,K", [(23040, 512, 2048), (4608, 512, 2048), (1000, 1028, 640), (2880, 512, 384)])
def test_linear_f32a_beside_busy_neighbours_is_bit_exact(M, N, K):
    """The short form of tools/gemm_f32a_soak.py in the suite: uic_linear_f32a (csrc/gemm_pp.hip: A loaded by inline-asm register
    loads, committed four phases later behind a hand-counted vmcnt) beside an HBM-bound and an MFMA-bound neighbour, output and
    bf16 image compared bit for bit with cast + GEMM at every launch.  Its first form failed exactly this way: 32-64 wrong
    elements in 1 % of the launches, only with a busy neighbour."""
    from unpaired_image_captioning_amd import _lib as L
    lib = L.load()
    torch.manual_seed(1)
    A = torch.randn(M, K, device="cuda") * 3
    Ab = A.bfloat16()
    B = (torch.randn(N, K, device="cuda") / K ** 0.5).bfloat16()
    bias = torch.randn(N, device="cuda")
    ref = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    L.check(lib.uic_linear(1, M, N, K, L.ptr(Ab), K, L.ptr(B), K, L.ptr(ref), N, L.ptr(bias), 1 | 0x400, L.stream()))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    hog_a = torch.randn(32 << 20, device="cuda")
    hog_b = torch.empty_like(hog_a)
    X = torch.randn(4096, 4096, device="cuda").bfloat16()
    for it in range(60 if M > 10000 else 120):
        mode = it % 4
        with torch.cuda.stream(side):
            if mode in (1, 3):
                hog_b.copy_(hog_a)
            if mode in (2, 3):
                torch.matmul(X, X)
        C = torch.full((M, N), 7.0, device="cuda", dtype=torch.bfloat16)
        img = torch.full((M, K), 7.0, device="cuda", dtype=torch.bfloat16)
        L.check(lib.uic_linear_f32a(M, N, K, L.ptr(A), K, L.ptr(B), K, L.ptr(C), N, L.ptr(bias), 1, L.ptr(img), K, L.stream()))
        torch.cuda.synchronize()
        assert torch.equal(C, ref), (it, mode, int((C != ref).sum()))
        assert torch.equal(img, Ab), (it, mode, int((img != Ab).sum()))


NAMES = lambda T, N, td: [("h_att", (T + 1, N, H), td), ("h_lang", (T + 1, N, H), td), ("c_att", (T + 1, N, H), torch.float32),
                          ("c_lang", (T + 1, N, H), torch.float32), ("att_h", (T, N, H), torch.float32), ("alpha", (T, N, R), torch.float32),
                          ("ctx", (T, N, H), td), ("hdrop", (T, N, H), td), ("gates1", (T, N, 4 * H), td), ("gates2", (T, N, 4 * H), td)]


@pytest.mark.parametrize("n_img,S", [(1, 4), (17, 5), (128, 5), (140, 5), (129, 1)])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_persistent_recurrence_equals_the_launch_chain(dtype, n_img, S):
    """Every activation the recurrence leaves for the backward pass, every decode step, persistent kernel vs per-step
    launches: 4 rows (most row groups empty), 85 rows (11 per group: ragged 16-row tiles), 640 (the benchmark), 700 (two
    launches of <= 640 rows), 129 -- with ragged region counts (att_masks), training-mode dropout, and both exchange
    protocols; results must not depend on the protocol and must repeat bit for bit."""
    Lb = _lib()
    lib = Lb.load()
    W = O.init_weights(V + 1, E, H, A, D, D, seed=11)
    b = O.synthetic_batch(n_img, S, R, D, V, L, seed=77, ragged_regions=True)
    batch = {k: v.cuda() for k, v in b.items()}
    model = build_model(CFG, W, dtype, drop=0.5)
    model.train()
    eng = model.engine
    N, T = n_img * S, L + 1
    t_run = model._steps_to_run(batch["labels"])
    pd = {k: v.detach() for k, v in model.param_dict().items()}
    td = torch.float32 if dtype == "f32" else torch.bfloat16

    def run(rec):
        eng.recurrence = rec
        logp, ws, _ = eng.forward(pd, batch["fc_feats"], batch["att_feats"], batch["att_masks"], batch["labels"], t_run, True, 99)
        out = {n: eng.workspace_tensor(ws, n, shp, dt)[: (t_run + 1 if shp[0] == T + 1 else t_run)].float().clone() for n, shp, dt in NAMES(T, N, td)}
        out["logp"] = logp[:, :t_run].clone()
        torch.cuda.synchronize()
        eng.release(ws)
        return out
    try:
        before = Lb.persistent_status()
        ref = run(Lb.REC_FWD_CHAIN)
        got1, got1b, got2 = run(0), run(0), run(Lb.REC_SAFE)
        after = Lb.persistent_status()
    finally:
        eng.recurrence = 0
    assert after[0] == 0
    n_launch = (N + 639) // 640
    assert after[1] - before[1] == 2 * n_launch and after[2] - before[2] == n_launch      # XCD-local twice, SAFE once
    tol = 2e-5 if dtype == "f32" else 1.6e-2          # bf16: one rounding step of a value <= 2 (h, gates) is 2^-7
    for k in ref:
        assert torch.equal(got1[k], got1b[k]), k                         # bit-repeatable
        assert torch.equal(got1[k], got2[k]), k                          # independent of the protocol / placement
        assert (got1[k] - ref[k]).abs().max().item() < tol, (k, (got1[k] - ref[k]).abs().max().item())
    assert (got1["logp"] - ref["logp"]).abs().max().item() < (2e-4 if dtype == "f32" else 1e-2)


@pytest.mark.parametrize("n_img,S", [(1, 4), (17, 5), (128, 5)])
def test_e_att_is_exp_of_twice_the_stored_p_att(n_img, S):
    """The persistent training recurrence's attention reads e_att = e^{2 p_att} (tanh(p + h) = 1 - 2 / (1 + e^{2p} e^{2h}),
    csrc/rnn_persist.hip).  It is made from the ROUNDED bf16 p_att -- by the ctx2att GEMM's epilogue at the large shapes, by an
    element-wise pass behind the small ones -- so both forms must give bf16(2^(2 log2(e) p)) of the stored p_att: within one bf16
    step of torch's exp (v_exp_f32 is not correctly rounded), and identical between two runs."""
    Lb = _lib()
    W = O.init_weights(V + 1, E, H, A, D, D, seed=11)
    b = O.synthetic_batch(n_img, S, R, D, V, L, seed=78, ragged_regions=True)
    batch = {k: v.cuda() for k, v in b.items()}
    model = build_model(CFG, W, "bf16", drop=0.5)
    model.train()
    eng = model.engine
    N = n_img * S
    t_run = model._steps_to_run(batch["labels"])
    pd = {k: v.detach() for k, v in model.param_dict().items()}
    outs = []
    for _ in range(2):
        logp, ws, _ = eng.forward(pd, batch["fc_feats"], batch["att_feats"], batch["att_masks"], batch["labels"], t_run, True, 99)
        p_att = eng.workspace_tensor(ws, "p_att", (N, R, A), torch.bfloat16).float().clone()
        e_att = eng.workspace_tensor(ws, "e_att", (N, R, A), torch.bfloat16).float().clone()
        torch.cuda.synchronize()
        eng.release(ws)
        outs.append((p_att, e_att))
    p_att, e_att = outs[0]
    assert torch.equal(e_att, outs[1][1]) and torch.equal(p_att, outs[1][0])
    ref = torch.exp(2.0 * p_att.double()).float()
    assert p_att.abs().max().item() < 20.0                      # (far inside the clamp at 2^+-60)
    assert ((e_att - ref).abs() / ref).max().item() <= 2.0 ** -7 * 1.01
    assert ((e_att - ref).abs() / ref).mean().item() < 2.0 ** -9


BNAMES = lambda T, N: [("dg1", (T, N, 4 * H), torch.bfloat16), ("dg2", (T, N, 4 * H), torch.bfloat16), ("datth", (T, N, H), torch.bfloat16),
                       ("de", (T, N, R), torch.float32), ("dx2", (T, N, 3 * H), torch.float32)]


@pytest.mark.parametrize("n_img,S", [(1, 4), (17, 5), (128, 5), (140, 5), (129, 1)])
def test_persistent_bptt_equals_the_launch_chain(n_img, S):
    """Everything the BPTT loop leaves behind -- both cells' gate gradients, d att_h, the attention score gradients and d att_res
    of every decode step, and every gradient tensor of the model -- persistent kernel (csrc/rnn_bwd_persist.hip, one launch for
    all steps) vs six launches per step, on the same forward pass: 4 rows (most row groups empty), 85 rows (11 per group:
    ragged 16-row tiles), 640 (the benchmark), 700 (two launches of <= 640 rows), 129; ragged region counts, training-mode
    dropout; both exchange protocols must agree bit for bit and repeat bit for bit."""
    Lb = _lib()
    W = O.init_weights(V + 1, E, H, A, D, D, seed=11)
    b = O.synthetic_batch(n_img, S, R, D, V, L, seed=77, ragged_regions=True)
    batch = {k: v.cuda() for k, v in b.items()}
    model = build_model(CFG, W, "bf16", drop=0.5)
    model.train()
    eng = model.engine
    N, T = n_img * S, L + 1
    t_run = model._steps_to_run(batch["labels"])
    pd = {k: v.detach() for k, v in model.param_dict().items()}

    def run(rec):
        eng.recurrence = 0
        _, ws, (d, w, bs) = eng.forward(pd, batch["fc_feats"], batch["att_feats"], batch["att_masks"], batch["labels"], t_run, True, 99,
                                        want_logprobs=False, masks=batch["masks"])
        eng.xe_loss(ws, d, bs, t_run)
        eng.recurrence = rec
        d = eng.dims(N, R, T)
        grads = {k: torch.zeros_like(v) for k, v in pd.items()}
        eng.backward(ws, d, w, bs, t_run, True, 99, grads)
        torch.cuda.synchronize()
        out = {n: eng.workspace_tensor(ws, n, shp, dt)[:t_run].float().clone() for n, shp, dt in BNAMES(T, N)}
        out["dx2"] = out["dx2"][:, :, :H].contiguous()            # the d att_res columns are what outlives the loop
        out.update({"grad:" + k: g.float().clone() for k, g in grads.items()})
        eng.release(ws)
        return out
    try:
        before = Lb.persistent_status()
        ref = run(0)
        got1, got1b, got2 = run(Lb.REC_BWD_PERSIST), run(Lb.REC_BWD_PERSIST), run(Lb.REC_BWD_PERSIST | Lb.REC_SAFE)
        after = Lb.persistent_status()
    finally:
        eng.recurrence = 0
    assert after[0] == 0
    n_launch = (N + 639) // 640
    # (each run's forward pass is one XCD-local launch per 640 rows as well)
    assert after[1] - before[1] == 4 * n_launch + 2 * n_launch and after[2] - before[2] == n_launch
    floor = 1e-3 * max(float(v.norm()) for k, v in ref.items() if k.startswith("grad:"))
    for k in ref:
        assert torch.equal(got1[k], got1b[k]), k                         # bit-repeatable (the embedding gradient included)
        assert torch.equal(got1[k], got2[k]), k                          # independent of the protocol / placement
        den = max(float(ref[k].norm()), floor if k.startswith("grad:") else 1e-30)
        err = float((got1[k] - ref[k]).norm()) / den
        # measured at 640 rows: per-step buffers 3e-4 .. 9e-4 (bf16 rounding of the gate gradients after a different f32
        # summation order), gradient tensors <= 6e-4
        assert err < 5e-3, (k, err)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_reference_default_feature_config_full_size_vs_oracle(dtype):
    """The reference's DEFAULT feature configuration at configs[1] size (P/opts.py: use_bn = 1, use_box = 1): BatchNorm1d in
    front of att_embed's Linear (batch statistics over the packed live regions, running statistics updated) and 2053-wide region
    features (2048 + 5 box features, no multiple of 8), 640 caption rows with ragged region counts, default persistent mode --
    loss, log-probs of the targets, every gradient tensor (L2) and the updated running statistics against the oracle."""
    from unpaired_image_captioning_amd.trainer import xe_step
    Lb = _lib()
    Dbox = 2053
    cfg = dict(V=V, E=E, H=H, A=A, D=Dbox, Dfc=D, L=L, use_bn=1)
    torch.manual_seed(0)
    W = O.init_weights(V + 1, E, H, A, Dbox, D, seed=17, use_bn=1)
    g = torch.Generator().manual_seed(3)
    W["att_embed.0.weight"] = 0.5 + torch.rand(Dbox, generator=g)            # non-trivial BatchNorm affine parameters
    W["att_embed.0.bias"] = 0.1 * torch.randn(Dbox, generator=g)
    b = O.synthetic_batch(128, 5, R, Dbox, V, L, seed=4321, ragged_regions=True)
    b["fc_feats"] = b["fc_feats"][:, :D].contiguous()
    nt = torch.get_num_threads()
    torch.set_num_threads(min(16, nt))
    Wo = {k: v.clone() for k, v in W.items()}
    ref_loss, ref_grads, ref_logp = O.xe_loss_and_grads(Wo, b["fc_feats"], b["att_feats"], b["labels"], b["masks"], b["att_masks"], use_bn=1)
    torch.set_num_threads(nt)
    batch = {k: v.cuda() for k, v in b.items()}
    model = build_model(cfg, W, dtype)
    model.train()
    loss, grads = xe_step(model, batch)
    assert Lb.persistent_status()[0] == 0
    assert abs(loss.item() - float(ref_loss)) < LOGP_TOL[dtype]
    floor = 1e-3 * max(float(v.norm()) for v in ref_grads.values())
    worst, worst_k = 0.0, ""
    for k, r in ref_grads.items():
        err = ((grads[k].float().cpu().double() - r.double()).norm() / max(r.double().norm().item(), floor)).item()
        if err > worst:
            worst, worst_k = err, k
        # measured: f32 7.0e-6; bf16 3.8e-2 on the BatchNorm affine gradients (sums of bf16-rounded products over 2053 x 512
        # weights), 7e-3 on every other tensor
        assert err < ({"f32": 2e-5, "bf16": 6e-2} if k.startswith("att_embed.0.") else GRAD_TOL)[dtype], (k, err)
    print("reference-default features, full size %s: loss %.6f (oracle %.6f), worst per-tensor L2 gradient error %.3e (%s)" %
          (dtype, loss.item(), float(ref_loss), worst, worst_k))
    sd = model.state_dict()
    for k in ("att_embed.0.running_mean", "att_embed.0.running_var"):
        assert (sd[k].cpu() - Wo[k]).abs().max().item() < (1e-5 if dtype == "f32" else 2e-3) * max(1.0, float(Wo[k].abs().max())), k
