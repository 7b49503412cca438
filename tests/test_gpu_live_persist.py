"""The step over the live positions at 512 hidden units -- where the persistent recurrence kernel runs (uic_rnn_persist_eligible:
H == A == 512) and, in bf16 with the list made on the device, stores every live hdrop row into the compact logit operand itself
(Step::fused_gather, csrc/topdown_step.hip; rnn_persist.hip: live_inv / hdrop_live) -- against the CPU oracle, with training-mode
dropout 0.5 (the oracle is fed the kernels' own masks), at the row counts and masks where that store, the list and the
captions' lengths (cap_len) can go wrong: a handful of rows, ragged 16-row tiles, two launches of <= 640 rows, more positions
than the list kernel's single round trip, early breaks, holes, empty decode steps, fractional weights, dead rows.  And the
benchmark's own loop: Trainer.train_device_batch on a resident batch, three steps, against the oracle's Adam trajectory.
The region features are narrow (D = 256) and the vocabulary small and odd (1000 + 1) so that an oracle run takes a second."""
import argparse

import pytest
import torch

from conftest import poison_workspaces

from oracle import topdown as O
from test_gpu_fullsize import GRAD_TOL, LOGP_TOL, grad_errors, kernel_dropout_masks, seed_after, with_live
from test_gpu_topdown import build_model
from test_live_positions import _same

pytestmark = pytest.mark.gpu

V, E, H, A, D, L = 1000, 512, 512, 512, 256, 16
CFG = dict(V=V, E=E, H=H, A=A, D=D, L=L)
T = L + 1
IMAGES = {4: (1, 4), 85: (17, 5), 129: (129, 1), 700: (140, 5), 1050: (210, 5)}     # caption rows: (images, captions per image)
SEED_COUNTER = 512085


def _lib():
    from unpaired_image_captioning_amd import _lib as L_
    return L_


def make_batch(rows, R, pattern, Datt=D, seed=41):
    """pattern "lengths": the captions' own lengths (8 .. 16 tokens); "short": every caption at most 11 tokens, so that the decode
    loop breaks early; "holes": the masks of test_arbitrary_masks_holes_empty_steps_and_fractional_weights -- random holes with
    fractional weights, decode steps 4 and 5 without a live row, one row without a live position, one live row at the last step."""
    n_img, S = IMAGES[rows]
    b = O.synthetic_batch(n_img, S, R, Datt, V, L, seed=seed, ragged_regions=True)
    if pattern == "short":
        keep = L - 5
        b["labels"][:, 1 + keep:] = 0
        b["masks"][:, 2 + keep:] = 0.0
    elif pattern == "holes":
        g = torch.Generator().manual_seed(4)
        m = (torch.rand(b["masks"].shape, generator=g) < 0.6).float() * (0.25 + torch.rand(b["masks"].shape, generator=g))
        dead, last = (7, 3) if rows > 8 else (rows - 1, 1)
        m[:, 1 + 4] = 0.0                                     # decode step 4: nothing live
        m[:, 1 + 5] = 0.0                                     # ... nor step 5
        m[dead, :] = 0.0                                      # a row that contributes nothing
        m[:, 1 + T - 1] = 0.0
        m[last, 1 + T - 1] = 1.0                              # the last step: one live row
        b["labels"][last, 1:] = torch.randint(1, V, (T,), generator=g)      # (so that every step is run: no early break)
        b["masks"] = m
    else:
        assert pattern == "lengths", pattern
    return b


def oracle_step(W, b, drop, use_bn=0):
    nt = torch.get_num_threads()
    torch.set_num_threads(min(16, nt))
    try:
        loss, grads, _ = O.xe_loss_and_grads(W, b["fc_feats"], b["att_feats"], b["labels"], b["masks"], b["att_masks"], drop, use_bn, True)
    finally:
        torch.set_num_threads(nt)
    return float(loss), grads


def check_case(tag, cfg, W, b, dtype, tol, pattern="lengths", device_batch=None, use_bn=0, forms=(None, "rows", "device")):
    """One batch through the fused step in every form of `forms` (see with_live), the device form twice, and through the per-step
    launch chain over every position; everything against the oracle under the step's own dropout masks.  Every gradient tensor
    is held to `tol` (test_gpu_fullsize.GRAD_TOL, or the case's entry of CASE_TOL).  Returns BatchNorm's
    running statistics as the first of these steps left them."""
    from unpaired_image_captioning_amd.trainer import xe_step
    Lb = _lib()
    rows, R = b["labels"].shape[0], b["att_feats"].shape[1]
    batch = device_batch if device_batch is not None else {k: v.cuda() for k, v in b.items()}
    model = build_model(cfg, W, dtype, drop=0.5)
    model.train()
    poison_workspaces(model.engine)
    t_run = model._steps_to_run(batch["labels"])
    if pattern == "short":
        assert t_run < T, t_run                               # an early break: the decode loop stops in front of step T
    elif pattern == "holes":
        assert t_run == T
    seed = seed_after(SEED_COUNTER)

    def step(live, rec=0):
        model.engine.recurrence = rec
        model._seed_counter = SEED_COUNTER
        before = Lb.persistent_status()
        try:
            loss, grads, got_seed = xe_step(model, with_live(batch, live), return_seed=True)
            st = Lb.persistent_status()
        finally:
            model.engine.recurrence = 0
        assert got_seed == seed
        # the persistent forward recurrence ran (one launch per 640 rows), and none of its waits timed out
        assert st[0] == 0 and (st[1] - before[1], st[2] - before[2]) == (0 if rec else (rows + 639) // 640, 0), (tag, live, before, st)
        return loss.item(), {k: g.detach().clone() for k, g in grads.items()}

    got, running = {}, None
    for live in forms:
        got[live] = step(live)
        if running is None:                                   # BatchNorm: what the FIRST training step left
            running = {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if "running" in k}
    again = step("device")
    chain = step(None, Lb.REC_FWD_CHAIN)
    ref_loss, ref_grads = oracle_step(W, b, kernel_dropout_masks(seed, rows, R, T, H, E), use_bn)
    e_chain = grad_errors(chain[1], ref_grads)
    e_got = {live: grad_errors(grads, ref_grads) for live, (_, grads) in got.items()}
    for live, (loss, _) in got.items():
        errs = e_got[live]
        worst = max(errs, key=errs.get)
        print("%s %s, list: %s: loss %.6f (oracle %.6f), worst L2 gradient error %.3e (%s); launch chain over every position: loss %.6f, %.3e on "
              "that tensor, worst %.3e (%s)" % (tag, dtype, live, loss, ref_loss, errs[worst], worst, chain[0], e_chain[worst], max(e_chain.values()),
                                                max(e_chain, key=e_chain.get)))
    over = {k: "%.3e" % e for k, e in e_chain.items() if e >= GRAD_TOL[dtype]}
    if over:
        print("%s %s: launch chain over every position at or above GRAD_TOL: %s" % (tag, dtype, over))
    for live, (loss, _) in got.items():
        assert abs(loss - ref_loss) < LOGP_TOL[dtype], (live, loss, ref_loss)
        for k, err in e_got[live].items():
            assert err < tol, (live, k, err, e_chain[k])
    # the three forms agree with each other (the bounds of tests/test_live_positions.py)
    if None in got and "rows" in got:
        assert abs(got["rows"][0] - got[None][0]) < (2e-6 if dtype == "f32" else 2e-5) * max(1.0, abs(got[None][0]))
        _same(got["rows"][1], got[None][1], 2e-5 if dtype == "f32" else 2e-3)
    if "rows" in got:
        assert abs(got["device"][0] - got["rows"][0]) <= 1e-6 * max(1.0, abs(got["rows"][0]))
        _same(got["device"][1], got["rows"][1], 2e-5 if dtype == "f32" else 2e-3)
    if None in got and "device" in got:
        _same(got["device"][1], got[None][1], 2e-5 if dtype == "f32" else 2e-3)
    # the same seed again: the same bits
    assert again[0] == got["device"][0]
    for k, g in again[1].items():
        assert torch.equal(g, got["device"][1][k]), k
    return running


# (caption rows, regions, masks).  bf16: every row count meets every mask pattern, the region counts go round; each case runs the
# step without a list, with the caller's list and with the list made on the device.  f32 (the parity path: the persistent kernel
# without the compact store): one case per row count, the other axes go round.
BF16_CASES = [(4, 1, "lengths"), (4, 7, "short"), (4, 36, "holes"),
              (85, 36, "lengths"), (85, 1, "short"), (85, 7, "holes"),
              (129, 7, "lengths"), (129, 36, "short"), (129, 1, "holes"),
              (700, 1, "lengths"), (700, 7, "short"), (700, 36, "holes"),
              (1050, 7, "lengths"), (1050, 1, "short"), (1050, 36, "holes")]
F32_CASES = [(4, 7, "lengths"), (85, 36, "holes"), (129, 1, "short"), (700, 36, "short"), (1050, 7, "holes")]
# Per-tensor L2 gradient bound of a case (floors as test_gpu_fullsize.GRAD_TOL): that file's bound unless listed here.
# Measured on an MI355X: f32 <= 1.8e-6 everywhere (bound 4e-6); bf16 between 3.8e-3 and 1.7e-2 (bound 2e-2) except three cases
# whose att_embed / fc_embed weight gradients -- few rows, or one region per image, or BatchNorm in front -- carry more bf16
# rounding.  Their bound is 3 x the worst per-tensor error of the per-step launch chain over EVERY position (neither the
# persistent kernel nor the list) against the oracle on the same batch, seed and masks, which check_case prints beside the
# case's own error -- never a figure of the step over the live positions (which measured the same to three digits):
#   4 rows, 1 region, lengths    launch chain 9.195e-2 (fc_embed.0.weight)   x 3 = 2.76e-1   (live step 9.194e-2)
#   85 rows, 1 region, short     launch chain 2.328e-2 (att_embed.0.weight)  x 3 = 6.98e-2   (live step 2.328e-2)
#   85 rows, use_bn, box         launch chain 3.551e-2 (att_embed.0.weight)  x 3 = 1.07e-1   (live step 3.548e-2)
# The f32 runs of the same kernels at 4 rows, at one region and with use_bn stay below 1.8e-6: the arithmetic is right, the
# figure is bf16's.  (profiles/LOG.md holds the same numbers.)
# (The bound holds for every tensor of such a case: which further tensors of it lie above GRAD_TOL on the launch chain has not been
# measured per tensor -- check_case prints them -- while every form still has to agree with the all-positions step within 2e-3.)
CASE_TOL = {(4, 1, "lengths", "bf16"): 3 * 9.195e-2, (85, 1, "short", "bf16"): 3 * 2.328e-2, ("use_bn", "bf16"): 3 * 3.551e-2}


@pytest.mark.parametrize("rows,R,pattern,dtype", [c + ("bf16",) for c in BF16_CASES] + [c + ("f32",) for c in F32_CASES])
def test_step_over_live_positions_at_512_hidden_units_vs_oracle(rows, R, pattern, dtype):
    if rows == 1050:
        assert rows * T > 16384                               # past the list kernel's single round trip
    W = O.init_weights(V + 1, E, H, A, D, D, seed=13)
    b = make_batch(rows, R, pattern)
    if pattern == "holes":
        m = b["masks"][:, 1:]
        assert (m[:, 4:6] == 0).all() and (m.sum(1) == 0).sum() >= 1 and (m[:, -1] != 0).sum() == 1
        assert ((m > 0) & (m < 1)).any() and (m[:, :-1] == 0).any()
    check_case("%d rows, %d regions, %s" % (rows, R, pattern), CFG, W, b, dtype, CASE_TOL.get((rows, R, pattern, dtype), GRAD_TOL[dtype]), pattern)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_per_image_features_over_live_positions_vs_oracle(dtype):
    """85 caption rows whose features are shipped once per image (dims.seq_per_img = 5: the replication happens on the device),
    with the list; the oracle runs on the replicated batch."""
    from test_gpu_topdown import _per_image
    W = O.init_weights(V + 1, E, H, A, D, D, seed=13)
    b = make_batch(85, 36, "lengths", seed=43)
    img = _per_image({k: v.cuda() for k, v in b.items()}, 5)
    assert img["att_feats"].shape[0] * 5 == img["labels"].shape[0] == 85
    check_case("85 rows, features per image", CFG, W, b, dtype, CASE_TOL.get(("per_image", dtype), GRAD_TOL[dtype]), device_batch=img)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_use_bn_box_features_over_live_positions_vs_oracle(dtype):
    """The reference's default feature configuration (use_bn = 1, 5 box features: D = 256 + 5, no multiple of 8) at 85 rows with
    dropout and the list made on the device: loss, every gradient tensor and the updated running statistics."""
    Dbox = D + 5
    cfg = dict(CFG, D=Dbox, Dfc=D, use_bn=1)
    W = O.init_weights(V + 1, E, H, A, Dbox, D, seed=17, use_bn=1)
    g = torch.Generator().manual_seed(3)
    W["att_embed.0.weight"] = 0.5 + torch.rand(Dbox, generator=g)            # non-trivial BatchNorm affine parameters
    W["att_embed.0.bias"] = 0.1 * torch.randn(Dbox, generator=g)
    b = make_batch(85, 36, "lengths", Datt=Dbox, seed=47)
    b["fc_feats"] = b["fc_feats"][:, :D].contiguous()
    Wo = {k: v.clone() for k, v in W.items()}                                # (the oracle updates the running statistics it is handed)
    running = check_case("85 rows, use_bn = 1, box features", cfg, Wo, b, dtype, CASE_TOL.get(("use_bn", dtype), GRAD_TOL[dtype]), use_bn=1,
                         forms=("device",))
    for k in ("att_embed.0.running_mean", "att_embed.0.running_var"):
        assert (W[k] - Wo[k]).abs().max().item() > 1e-4
        assert (running[k] - Wo[k]).abs().max().item() < (1e-5 if dtype == "f32" else 2e-3) * max(1.0, float(Wo[k].abs().max())), k


# ---------------------------------------------------------------------------------------------------------------- the benchmark's loop
LOOP_LR = 2e-3        # the oracle alone, three steps at this rate: loss 6.91 -> 6.77 -> 6.45 (CPU); at 5e-4 it moves by 0.09 only


def _bench_opt(dtype, seed):
    """bench.py's make_opt at this file's shape."""
    return argparse.Namespace(vocab_size=V, input_encoding_size=E, rnn_size=H, num_layers=1, drop_prob_lm=0.5, seq_length=L,
                              fc_feat_size=D, att_feat_size=D, att_hid_size=A, use_bn=0, logit_layers=1, caption_model="topdown",
                              compute_dtype=dtype, seed=seed, i2t_learning_rate=LOOP_LR, i2t_train_flag=1, seq_per_img=5)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_benchmark_loop_three_steps_vs_oracle_adam_trajectory(dtype):
    """bench.py's timed loop -- Trainer.build_optimizer, a resident batch with Trainer.attach_live, train_device_batch into the
    arena's gradient views, dropout 0.5, a new seed every step -- three times at 85 rows, against the oracle's own trajectory:
    xe_loss_and_grads under each step's exported masks, then adam_step.  The learning rate is large enough that the oracle's
    loss falls by more than ten times the bf16 loss tolerance over the three steps: a step that ignored the updated weights, or
    read a stale operand copy of them, misses the oracle's second and third loss."""
    from unpaired_image_captioning_amd.trainer import Trainer
    Lb = _lib()
    torch.manual_seed(1234)
    tr = Trainer(_bench_opt(dtype, 1234))
    model = tr.i2t_model
    P = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    tr.build_optimizer()
    poison_workspaces(model.engine)
    b = make_batch(85, 36, "lengths", seed=31)
    batch = {k: v.cuda() for k, v in b.items()}
    t_run = model._steps_to_run(batch["labels"])
    den = float(batch["masks"][:, 1:T + 1].sum().item())
    tr.attach_live(batch)
    assert "live_rows" not in batch and int(batch["live_count"].sum()) < 85 * T
    m1 = {k: torch.zeros_like(v) for k, v in P.items()}
    v1 = {k: torch.zeros_like(v) for k, v in P.items()}
    seeds, outs, got, want = [], [], [], []
    before = Lb.persistent_status()
    for step in range(1, 4):
        seed = seed_after(model._seed_counter)                # (the seed the step is about to draw)
        loss = tr.train_device_batch(batch, t_run, den, den)
        assert model._seed_counter == seed
        got.append(float(loss.item()))
        drop = kernel_dropout_masks(seed, 85, 36, T, H, E)
        seeds.append(seed)
        outs.append(drop["out"])
        ref_loss, ref_grads = oracle_step(P, b, drop)
        O.adam_step(P, ref_grads, m1, v1, step, LOOP_LR)
        want.append(ref_loss)
    st = Lb.persistent_status()
    assert st[0] == 0 and (st[1] - before[1], st[2] - before[2]) == (3, 0), (before, st)
    print("benchmark loop %s: losses %s, oracle %s" % (dtype, got, want))
    assert len(set(seeds)) == 3
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2]) and not torch.equal(outs[0], outs[2])
    assert want[0] - want[2] >= 10 * LOGP_TOL["bf16"], want   # the oracle alone moves: the checks below can fail
    for step in range(3):
        assert abs(got[step] - want[step]) < LOGP_TOL[dtype], (step, got, want)
    if dtype == "f32":
        for k, p in tr.arena.params.items():
            err = (p.detach().cpu() - P[k]).abs().max().item()
            assert err < 1e-4, (k, err)
