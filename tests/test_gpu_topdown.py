"""GPU parity of the TopDown captioner path (libuic_hip.so through the reference-shaped Python
surface) against the golden vectors produced from the reference's own modules and against the CPU
oracle.  Tolerances follow BASELINE.json's north_star: log-probs within 1e-3 (f32) / 1e-2 (bf16),
greedy token ids bit-exact on the f32 path."""
import argparse

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import topdown as O

pytestmark = pytest.mark.gpu

FIXTURES = ["topdown_tiny", "topdown_tiny_ragged", "topdown_tiny_nomask", "topdown_tiny_earlybreak", "topdown_odd", "topdown_tiny_logit2", "topdown_tiny_box"]
LOGP_TOL = {"f32": 1e-3, "bf16": 1e-2}
GRAD_TOL = {"f32": 2e-3, "bf16": 1e-1}      # f32: max-entry error; bf16: L2 error (see grads_close).  The bf16 bound is for the TINY
# fixtures (32 hidden units, a handful of rows), where one ReLU within bf16 rounding of zero moves a whole tensor by several
# per cent (worst measured over all fixtures: 0.10); at BASELINE's shapes the measured error is 6e-3 and
# tests/test_gpu_fullsize.py bounds it by 2e-2


def make_opt(cfg, dtype, drop=0.0, seed=0):
    return argparse.Namespace(vocab_size=cfg["V"], input_encoding_size=cfg["E"], rnn_size=cfg["H"], num_layers=1,
                              drop_prob_lm=drop, seq_length=cfg["L"], fc_feat_size=cfg.get("Dfc", cfg["D"]), att_feat_size=cfg["D"],
                              att_hid_size=cfg["A"], use_bn=cfg.get("use_bn", 0), logit_layers=cfg.get("logit_layers", 1), caption_model="topdown",
                              compute_dtype=dtype, seed=seed)


def build_model(cfg, W, dtype, drop=0.0):
    from unpaired_image_captioning_amd import models
    model = models.setup(make_opt(cfg, dtype, drop))
    missing = model.load_state_dict(W, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return model.cuda()


def final_logit(model):
    """The vocabulary Linear: model.logit, or the last module of the Sequential when logit_layers > 1."""
    return model.logit if isinstance(model.logit, torch.nn.Linear) else model.logit[-1]


def rel(got, ref):
    got = got.detach().float().cpu().double()
    ref = ref.detach().float().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-9)).item()


def grads_close(grads, ref, tol):
    """Every gradient tensor within `tol` of the reference, relative to max(|ref tensor|, 1e-3 * the largest
    gradient entry of the whole model): tensors whose true gradient is a cancellation (alpha_net.bias is
    mathematically 0, ctx2att.bias nearly so) are compared at the model's gradient scale, not their own."""
    floor = 1e-3 * max(float(v.abs().max()) for v in ref.values())
    for k, r in ref.items():
        g = grads[k].detach().float().cpu().double()
        r = r.double()
        assert g.shape == r.shape, (k, g.shape, r.shape)
        if tol < 1e-2:      # f32 path: worst single entry
            err = (g - r).abs().max().item() / max(r.abs().max().item(), floor)
        else:               # bf16 path: a ReLU whose pre-activation is within bf16 rounding of 0 may flip and move
                            # one entry by its full size, so the tensor is compared in the L2 norm
            err = (g - r).norm().item() / max(r.norm().item(), floor * r.numel() ** 0.5)
        assert err < tol, (k, err)


def absmax(got, ref):
    return (got.detach().float().cpu().double() - ref.detach().float().cpu().double()).abs().max().item()


def test_state_dict_matches_reference_contract():
    cfg, W, I, Out, G, X = load_golden("topdown_tiny")
    from unpaired_image_captioning_amd import models
    model = models.setup(make_opt(cfg, "f32"))
    sd = model.state_dict()
    assert list(sd.keys()) == list(W.keys())
    for k in W:
        assert tuple(sd[k].shape) == tuple(W[k].shape), k


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", FIXTURES)
def test_forward_loss_backward_vs_reference_golden(name, dtype):
    from unpaired_image_captioning_amd.misc.criterion import LanguageModelCriterion
    cfg, W, I, Out, G, X = load_golden(name)
    model = build_model(cfg, W, dtype)
    model.train(cfg["logit_layers"] == 1)          # drop_prob_lm = 0: train mode is deterministic -- except for the hard-coded
                                                    # Dropout(0.5) of hidden logit blocks, whose fixtures were made in eval mode
    fc, att, labels, masks = (I[k].cuda() for k in ("fc_feats", "att_feats", "labels", "masks"))
    am = I["att_masks"].cuda() if "att_masks" in I else None
    attri = torch.zeros(fc.shape[0], 1, device="cuda")
    logp = model(fc, attri, att, labels, am)
    assert logp.shape == Out["logprobs"].shape
    assert absmax(logp, Out["logprobs"]) < LOGP_TOL[dtype]
    loss = LanguageModelCriterion(make_opt(cfg, dtype))(logp, labels[:, 1:], masks[:, 1:])
    assert abs(loss.item() - float(Out["loss"])) < LOGP_TOL[dtype]
    loss.backward()
    assert set(G) == set(k for k, _ in model.named_parameters())
    grads_close({k: p.grad for k, p in model.named_parameters()}, G, GRAD_TOL[dtype])


def test_second_backward_over_one_forward_raises_clearly():
    """The reference's step is loss.backward(retain_graph=True) (P/trainer.py:173) -- one walk of the graph.  A SECOND walk over
    the same forward cannot be served (the first one returned the forward's workspace to the pool): it must say so, not die on
    a None workspace."""
    from unpaired_image_captioning_amd.misc.criterion import LanguageModelCriterion
    cfg, W, I, Out, G, X = load_golden("topdown_tiny")
    model = build_model(cfg, W, "f32").train()
    fc, att, labels, masks = (I[k].cuda() for k in ("fc_feats", "att_feats", "labels", "masks"))
    am = I["att_masks"].cuda() if "att_masks" in I else None
    logp = model(fc, torch.zeros(fc.shape[0], 1, device="cuda"), att, labels, am)
    loss = LanguageModelCriterion(make_opt(cfg, "f32"))(logp, labels[:, 1:], masks[:, 1:])
    loss.backward(retain_graph=True)                      # the reference's call: fine
    grads_close({k: p.grad for k, p in model.named_parameters()}, G, GRAD_TOL["f32"])
    with pytest.raises(RuntimeError, match="second time"):
        loss.backward()
    # and the model is still usable afterwards
    model.zero_grad()
    logp = model(fc, torch.zeros(fc.shape[0], 1, device="cuda"), att, labels, am)
    LanguageModelCriterion(make_opt(cfg, "f32"))(logp, labels[:, 1:], masks[:, 1:]).backward()
    grads_close({k: p.grad for k, p in model.named_parameters()}, G, GRAD_TOL["f32"])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", FIXTURES)
def test_intermediates_vs_reference_golden(name, dtype):
    """fc_embed / att_embed / p_att and the first decode steps' states, read back from the workspace."""
    cfg, W, I, Out, G, X = load_golden(name)
    model = build_model(cfg, W, dtype).eval()
    eng = model.engine
    fc, att, labels = (I[k].cuda() for k in ("fc_feats", "att_feats", "labels"))
    am = I["att_masks"].cuda() if "att_masks" in I else None
    pd = {k: v.detach() for k, v in model.param_dict().items()}
    N, R, H, A = fc.shape[0], att.shape[1], cfg["H"], cfg["A"]
    T = labels.shape[1] - 1
    t_run = model._steps_to_run(labels)
    logp, ws, _ = eng.forward(pd, fc, att, am, labels, t_run, False, 1)
    torch.cuda.synchronize()
    td = torch.float32 if dtype == "f32" else torch.bfloat16
    tol = 1e-4 if dtype == "f32" else 2e-2
    Rg = Out["att_embed"].shape[1]                    # the reference clips R to max(len) (clip_att)
    assert rel(eng.workspace_tensor(ws, "fc_embed", (N, H), td), Out["fc_embed"]) < tol
    assert rel(eng.workspace_tensor(ws, "att_embed", (N, R, H), td)[:, :Rg], Out["att_embed"]) < tol
    assert rel(eng.workspace_tensor(ws, "p_att", (N, R, A), td)[:, :Rg], Out["p_att"]) < tol
    h_att = eng.workspace_tensor(ws, "h_att", (T + 1, N, H), td)
    h_lang = eng.workspace_tensor(ws, "h_lang", (T + 1, N, H), td)
    c_att = eng.workspace_tensor(ws, "c_att", (T + 1, N, H), torch.float32)
    c_lang = eng.workspace_tensor(ws, "c_lang", (T + 1, N, H), torch.float32)
    ctx = eng.workspace_tensor(ws, "ctx", (T, N, H), td)
    for t in range(min(3, t_run)):
        assert rel(h_att[t + 1], Out["step%d_h_att" % t]) < tol
        assert rel(c_att[t + 1], Out["step%d_c_att" % t]) < tol
        assert rel(ctx[t], Out["step%d_att_res" % t]) < tol
        assert rel(h_lang[t + 1], Out["step%d_h_lang" % t]) < tol
        assert rel(c_lang[t + 1], Out["step%d_c_lang" % t]) < tol
        assert absmax(logp[:, t], Out["step%d_logp" % t]) < LOGP_TOL[dtype]
    eng.release(ws)


@pytest.mark.parametrize("name", FIXTURES)
def test_greedy_decode_bit_exact_f32(name):
    cfg, W, I, Out, G, X = load_golden(name)
    model = build_model(cfg, W, "f32").eval()
    idx = torch.arange(cfg["n_img"]) * cfg["S"]
    fc, att = I["fc_feats"][idx].cuda(), I["att_feats"][idx].cuda()
    am = I["att_masks"][idx].cuda() if "att_masks" in I else None
    attri = torch.zeros(fc.shape[0], 1, device="cuda")
    seq, lp = model(fc, attri, att, am, opt={"sample_max": 1, "beam_size": 1}, mode="sample")
    assert seq.dtype == torch.int64 and tuple(seq.shape) == tuple(Out["greedy_seq"].shape)
    assert torch.equal(seq.cpu(), Out["greedy_seq"])
    assert absmax(lp, Out["greedy_logp"]) < 1e-3


@pytest.mark.parametrize("name", ["topdown_tiny", "topdown_odd"])
def test_greedy_decode_bf16_close(name):
    cfg, W, I, Out, G, X = load_golden(name)
    model = build_model(cfg, W, "bf16").eval()
    idx = torch.arange(cfg["n_img"]) * cfg["S"]
    fc, att = I["fc_feats"][idx].cuda(), I["att_feats"][idx].cuda()
    am = I["att_masks"][idx].cuda() if "att_masks" in I else None
    seq, lp = model(fc, None, att, am, opt={"sample_max": 1}, mode="sample")
    # tokens may legitimately flip where two log-probs are closer than the bf16 tolerance: score the
    # device's own tokens with the oracle instead of demanding identical ids
    seq_o, lp_o = O.sample(W, I["fc_feats"][idx], I["att_feats"][idx], I.get("att_masks")[idx] if "att_masks" in I else None,
                           cfg["L"], sample_max=0, forced_tokens=seq.cpu())
    assert torch.equal(seq_o, seq.cpu())
    assert absmax(lp, lp_o) < 3e-2


def test_multinomial_sampling_scored_by_oracle():
    cfg, W, I, Out, G, X = load_golden("topdown_tiny_ragged")
    model = build_model(cfg, W, "f32").eval()
    fc, att, am = I["fc_feats"].cuda(), I["att_feats"].cuda(), I["att_masks"].cuda()
    seq, lp = model(fc, None, att, am, opt={"sample_max": 0, "temperature": 1.0}, mode="sample")
    assert int(seq.max()) <= cfg["V"] and int(seq.min()) >= 0
    seq_o, lp_o = O.sample(W, I["fc_feats"], I["att_feats"], I["att_masks"], cfg["L"], sample_max=0, forced_tokens=seq.cpu())
    assert torch.equal(seq_o, seq.cpu())               # same finished-row bookkeeping
    assert absmax(lp, lp_o) < 1e-3
    # forced tokens + decoding constraint path
    forced = torch.randint(0, cfg["V"] + 1, seq.shape)
    seq2, lp2 = model(fc, None, att, am, opt={"sample_max": 0, "forced_tokens": forced.cuda()}, mode="sample")
    seq_o2, lp_o2 = O.sample(W, I["fc_feats"], I["att_feats"], I["att_masks"], cfg["L"], sample_max=0, forced_tokens=forced)
    assert torch.equal(seq_o2, seq2.cpu()) and absmax(lp2, lp_o2) < 1e-3


def test_two_stream_train_step_equals_separate_calls():
    """uic_topdown_xe_train_step (recurrence + side-stream logit layer) == forward, xe_loss, backward in sequence.
    bf16: bit for bit (but for the chunk-accumulated weight gradients).  f32: to rounding -- v_mfma_f32_32x32x2_f32 rounds a
    row's dot product differently depending on the row's position inside the 32-row tile (measured with uic_linear: the same A
    row gives a last-bit different result at row offset 6 and at row offset 12), and the fused step hands the logit layer chunks
    of decode steps whose first row is a multiple of N = 6 here, not of 8 as for every real batch."""
    from unpaired_image_captioning_amd.trainer import xe_step
    cfg, W, I, Out, G, X = load_golden("topdown_odd")
    for dtype in ("f32", "bf16"):
        model = build_model(cfg, W, dtype, drop=0.5)
        model.train()
        batch = {k: I[k].cuda() for k in ("fc_feats", "att_feats", "labels", "masks", "att_masks")}
        model._seed_counter = 77
        l1, g1 = xe_step(model, batch, fused=True)
        model._seed_counter = 77
        l2, g2 = xe_step(model, batch, fused=False)
        torch.cuda.synchronize()
        assert l1.item() == l2.item()
        chunked = ("core.att_lstm.weight", "core.lang_lstm.weight", "core.attention.h2att.weight")
        for k in g1:
            if k.startswith(chunked):      # fused step: accumulated chunk by chunk (4 decode steps) behind the BPTT loop
                assert (g1[k] - g2[k]).abs().max().item() <= 2e-5 * max(1e-3, g2[k].abs().max().item()), k
            elif dtype == "f32":
                assert (g1[k] - g2[k]).abs().max().item() <= 2e-6 * max(1e-3, g2[k].abs().max().item()), k
            else:
                assert torch.equal(g1[k], g2[k]), k


def test_two_stream_train_step_equals_separate_calls_exactly_in_f32_at_whole_row_tiles():
    """The f32 half of the test above at N = 8 caption rows (every real batch has N % 8 == 0): the fused step's logit chunks then
    start at multiples of 8 rows, the MFMA row-position effect is gone and fused == separate must hold BIT FOR BIT for every
    tensor that is not accumulated chunk by chunk -- so that an ordering race between the fused step's streams (the first chunk on
    the main stream, the third / fourth stream, the masked sum on the side stream) cannot hide behind the rounding tolerance
    (ADVICE round 4)."""
    from unpaired_image_captioning_amd.trainer import xe_step
    V, E, H, A, D, L = 50, 32, 32, 32, 64, 6
    cfg = dict(V=V, E=E, H=H, A=A, D=D, L=L)
    W = O.init_weights(V + 1, E, H, A, D, D, seed=9)
    b = O.synthetic_batch(4, 2, 5, D, V, L, seed=13, ragged_regions=True)          # 4 images x 2 captions = 8 rows
    assert b["labels"].shape[0] % 8 == 0
    model = build_model(cfg, W, "f32", drop=0.5)
    model.train()
    batch = {k: v.cuda() for k, v in b.items()}
    for rep in range(3):
        model._seed_counter = 77 + rep
        l1, g1 = xe_step(model, batch, fused=True)
        model._seed_counter = 77 + rep
        l2, g2 = xe_step(model, batch, fused=False)
        torch.cuda.synchronize()
        assert l1.item() == l2.item()
        chunked = ("core.att_lstm.weight", "core.lang_lstm.weight", "core.attention.h2att.weight")
        for k in g1:
            if k.startswith(chunked):
                assert (g1[k] - g2[k]).abs().max().item() <= 2e-5 * max(1e-3, g2[k].abs().max().item()), k
            else:
                assert torch.equal(g1[k], g2[k]), (rep, k)


def test_weight_gradient_placement_does_not_outlive_a_training_step():
    """Where a weight gradient runs -- beside the fused step's BPTT loop or alone on the chip -- is an argument of every call,
    not state of the calling thread: uic_linear_wgrad gives the same bits before and after a fused training step on this
    thread.  The two placements take different kernels and K splits for this shape (alone: 128 x 128 tiles, 6 slices; beside:
    256 x 256, 2), so a placement left behind would change the f32 summation order."""
    from unpaired_image_captioning_amd import _lib as L
    from unpaired_image_captioning_amd.trainer import xe_step
    lib = L.load()
    M, N, K = 512, 2048, 4608
    g = torch.Generator().manual_seed(5)
    dY = torch.randn(K, M, generator=g).bfloat16().cuda()
    X = torch.randn(K, N, generator=g).bfloat16().cuda()
    ws = torch.empty(8 * M * N * 4, dtype=torch.uint8, device="cuda")

    def wgrad():
        dW = torch.zeros(M, N, device="cuda")
        L.check(lib.uic_linear_wgrad(L.BF16, M, N, K, L.ptr(dY), M, L.ptr(X), N, L.ptr(dW), N, L.ptr(ws), ws.numel(), 0, L.stream()),
                "linear_wgrad")
        torch.cuda.synchronize()
        return dW

    before = wgrad()
    cfg, W, I = load_golden("topdown_tiny")[:3]
    model = build_model(cfg, W, "bf16", drop=0.5)
    model.train()
    batch = {k: I[k].cuda() for k in ("fc_feats", "att_feats", "labels", "masks", "att_masks") if k in I}
    loss, _ = xe_step(model, batch, fused=True)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    assert torch.equal(wgrad(), before)


def test_unknown_recurrence_bits_are_refused():
    """uic_topdown_dims.recurrence takes the UIC_REC_* flags of include/uic_hip.h and nothing else: a training step with an
    unknown bit fails with an error that names the bit, and the same model steps normally again with a valid word."""
    from unpaired_image_captioning_amd.trainer import xe_step
    cfg, W, I = load_golden("topdown_tiny")[:3]
    model = build_model(cfg, W, "bf16")
    model.train()
    batch = {k: I[k].cuda() for k in ("fc_feats", "att_feats", "labels", "masks", "att_masks") if k in I}
    model.engine.recurrence = 0x4000
    try:
        with pytest.raises(RuntimeError, match="0x4000"):
            xe_step(model, batch)
    finally:
        model.engine.recurrence = 0
    loss, _ = xe_step(model, batch)
    assert torch.isfinite(loss).all()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["topdown_tiny_ragged", "topdown_tiny_logit2"])
def test_self_critical_step_vs_oracle(dtype, name):
    """SCST (P/trainer.py:167-171): multinomial sampling pass in train mode (dropout on), RewardCriterion,
    backward through the sampled log-probs.  The oracle replays the device's own tokens and dropout masks (with
    logit_layers = 2 also the hidden logit block's: the sampling pass and the teacher-forced replay must agree on them)."""
    from unpaired_image_captioning_amd import _lib as L
    from unpaired_image_captioning_amd.misc.criterion import RewardCriterion
    cfg, W, I, Out, G, X = load_golden(name)
    model = build_model(cfg, W, dtype, drop=0.5)
    model.train()
    fc, att, am = I["fc_feats"].cuda(), I["att_feats"].cuda(), I["att_masks"].cuda()
    seq, lp = model(fc, None, att, am, opt={"sample_max": 0}, mode="sample")
    seed = model._seed_counter
    assert lp.requires_grad and not seq.requires_grad
    g = torch.Generator().manual_seed(5)
    reward = torch.randn(seq.shape, generator=g)
    loss = RewardCriterion()(lp, seq, reward.cuda())
    loss.backward()
    lib = L.load()
    N, R, H, E, Ls = fc.shape[0], att.shape[1], cfg["H"], cfg["E"], cfg["L"]

    def mask(n, site, base=0):
        out = torch.empty(n, device="cuda")
        L.check(lib.uic_dropout_mask(L.ptr(out), n, 0.5, seed, site, base, L.stream()))
        return out.cpu()

    drop = dict(fc=mask(N * H, L.SITE_FC).view(N, H), att=mask(N * R * H, L.SITE_ATT).view(N, R, H),
                embed=mask(Ls * N * E, L.SITE_EMBED).view(Ls, N, E),
                out=torch.stack([mask(N * H, L.SITE_OUT0 + t).view(N, H) for t in range(Ls)]))
    if cfg["logit_layers"] > 1:
        drop["logit"] = [mask(Ls * N * H, L.SITE_LOGIT_H0 + l).view(Ls, N, H) for l in range(cfg["logit_layers"] - 1)]
    Wg = {k: v.clone().requires_grad_(True) for k, v in W.items()}
    seq_o, lp_o = O.sample(Wg, I["fc_feats"], I["att_feats"], I["att_masks"], Ls, sample_max=0, forced_tokens=seq.cpu(), drop=drop)
    assert torch.equal(seq_o, seq.cpu())
    assert absmax(lp, lp_o) < LOGP_TOL[dtype]
    loss_o = O.reward_criterion(lp_o, seq_o, reward)
    loss_o.backward()
    assert abs(loss.item() - loss_o.item()) < LOGP_TOL[dtype]
    grads_close({k: p.grad for k, p in model.named_parameters()}, {k: v.grad for k, v in Wg.items()}, GRAD_TOL[dtype])


def test_trainer_self_critical_step_runs_and_learns():
    """Trainer.train_self_critical: reward = +1 for sampled rows whose first token is even, -1 otherwise; a few
    steps must raise the probability of even first tokens (policy-gradient sign check, no scorer involved)."""
    from unpaired_image_captioning_amd.trainer import Trainer
    cfg, W, I, Out, G, X = load_golden("topdown_tiny")
    opt = make_opt(cfg, "f32")
    opt.i2t_learning_rate = 5e-3
    tr = Trainer(opt)
    tr.i2t_model.load_state_dict(W)
    tr.build_optimizer()
    data = {k: I[k].numpy() for k in ("fc_feats", "att_feats", "labels", "masks", "att_masks")}

    def reward_fn(data, sampled, greedy):
        r = np.where(sampled[:, :1] % 2 == 0, 1.0, -1.0)
        return np.repeat(r, sampled.shape[1], 1)

    def p_even():
        tr.i2t_model.eval()
        with torch.no_grad():
            lp = tr.i2t_model(I["fc_feats"].cuda(), None, I["att_feats"].cuda(), I["labels"].cuda(), I["att_masks"].cuda())
        tr.i2t_model.train()
        return lp[:, 0].exp()[:, 0::2].sum(1).mean().item()

    before = p_even()
    for _ in range(60):
        tr.train_self_critical(data, reward_fn)
    after = p_even()
    assert after > before + 0.02, (before, after)


def test_fused_xe_path_equals_api_path():
    """Trainer's fused log-softmax + criterion + backward == materialised log-probs + LanguageModelCriterion."""
    from unpaired_image_captioning_amd.trainer import xe_step
    cfg, W, I, Out, G, X = load_golden("topdown_tiny_ragged")
    model = build_model(cfg, W, "f32")
    model.train()
    batch = {k: I[k].cuda() for k in ("fc_feats", "att_feats", "labels", "masks", "att_masks")}
    loss, grads = xe_step(model, batch)
    assert abs(loss.item() - float(Out["loss"])) < 1e-4
    grads_close(grads, G, GRAD_TOL["f32"])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_training_mode_dropout_parity(dtype):
    """Dropout active (p = 0.5): export the kernels' own masks and feed them to the oracle."""
    from unpaired_image_captioning_amd import _lib as L
    from unpaired_image_captioning_amd.trainer import xe_step
    cfg, W, I, Out, G, X = load_golden("topdown_tiny_ragged")
    model = build_model(cfg, W, dtype, drop=0.5)
    model.train()
    batch = {k: I[k].cuda() for k in ("fc_feats", "att_feats", "labels", "masks", "att_masks")}
    loss, grads, seed = xe_step(model, batch, return_seed=True)
    lib = L.load()
    N, R, H, E = batch["fc_feats"].shape[0], batch["att_feats"].shape[1], cfg["H"], cfg["E"]
    T = batch["labels"].shape[1] - 1

    def mask(n, site):
        out = torch.empty(n, device="cuda")
        L.check(lib.uic_dropout_mask(L.ptr(out), n, 0.5, seed, site, 0, L.stream()))
        return out.cpu()

    drop = dict(fc=mask(N * H, L.SITE_FC).view(N, H), att=mask(N * R * H, L.SITE_ATT).view(N, R, H),
                embed=mask(T * N * E, L.SITE_EMBED).view(T, N, E),
                out=torch.stack([mask(N * H, L.SITE_OUT0 + t).view(N, H) for t in range(T)]))
    keep = torch.cat([v.flatten() for v in drop.values()])
    assert 0.35 < (keep > 0).float().mean().item() < 0.65 and set(keep.unique().tolist()) <= {0.0, 2.0}
    loss_o, grads_o, _ = O.xe_loss_and_grads(W, I["fc_feats"], I["att_feats"], I["labels"], I["masks"], I["att_masks"], drop)
    assert abs(loss.item() - loss_o.item()) < LOGP_TOL[dtype]
    grads_close(grads, grads_o, GRAD_TOL[dtype])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_real_size_rows_vs_reference_golden(dtype):
    """BASELINE config-2 shapes (R=36, D=2048, H=E=A=512, V1=9488) on 4 caption rows."""
    from unpaired_image_captioning_amd.trainer import xe_step
    cfg, W, I, Out, G, X = load_golden("topdown_real_n4")
    V, E, H, A, D, L = (cfg[k] for k in "VEHADL")
    wseed, dseed = [int(s) for s in torch.as_tensor(X["seeds"])]
    Wt = O.init_weights(V + 1, E, H, A, D, D, seed=wseed)
    b = O.synthetic_batch(cfg["n_img"], cfg["S"], cfg["R"], D, V, L, seed=dseed, ragged_regions=True)
    model = build_model(cfg, Wt, dtype).eval()
    batch = {k: v.cuda() for k, v in b.items()}
    logp = model(batch["fc_feats"], None, batch["att_feats"], batch["labels"], batch["att_masks"])
    assert absmax(logp[:, :, ::37], Out["logprobs_sub"]) < LOGP_TOL[dtype]
    t_run = model._steps_to_run(batch["labels"])
    assert (logp[:, :t_run].exp().sum(2) - 1).abs().max().item() < 1e-3
    assert logp[:, t_run:].abs().max().item() == 0 if t_run < logp.shape[1] else True
    loss, grads = xe_step(model, batch)
    assert abs(loss.item() - float(Out["loss"])) < LOGP_TOL[dtype]
    grads_close(grads, G, GRAD_TOL[dtype])
    for k, val in X.items():
        if k.startswith("gradnorm::"):
            n = grads[k.split("::", 1)[1]].double().norm().item()
            assert abs(n - float(torch.as_tensor(val))) <= GRAD_TOL[dtype] * float(torch.as_tensor(val)), k
    if dtype == "f32":
        idx = torch.arange(cfg["n_img"]) * cfg["S"]
        seq, lp = model(batch["fc_feats"][idx], None, batch["att_feats"][idx], batch["att_masks"][idx],
                        opt={"sample_max": 1}, mode="sample")
        assert torch.equal(seq.cpu(), Out["greedy_seq"])
        assert absmax(lp, Out["greedy_logp"]) < 1e-3


@pytest.mark.parametrize("per_image", [False, True])
def test_adam_trajectory_vs_reference_golden(per_image):
    """Three Trainer.train steps (forward, criterion, backward, Adam) reproduce the reference's losses -- also when the
    Trainer ships every image's features once (opt.seq_per_img) and the replication happens on the device."""
    from unpaired_image_captioning_amd.trainer import Trainer
    cfg, W, I, Out, G, X = load_golden("topdown_tiny")
    opt = make_opt(cfg, "f32")
    opt.i2t_learning_rate = 5e-4
    if per_image:
        opt.seq_per_img = cfg["S"]
        assert cfg["S"] > 1
    tr = Trainer(opt)
    tr.i2t_model.load_state_dict(W)
    tr.i2t_model.cuda()
    tr.build_optimizer()
    data = {k: I[k].numpy() for k in ("fc_feats", "att_feats", "labels", "masks", "att_masks")}
    losses = []
    for _ in range(3):
        tr.train(data)
        losses.append(tr.i2t_train_loss)
    np.testing.assert_allclose(losses, Out["adam_losses"].numpy(), rtol=0, atol=2e-4)
    sd = tr.i2t_model.state_dict()
    assert absmax(sd["logit.bias"], Out["adam_final_logit_bias"]) < 1e-4
    assert absmax(sd["core.attention.h2att.weight"], Out["adam_final_h2att_weight"]) < 1e-4
    if per_image:
        assert tr.to_device(data)["att_feats"].shape[0] * cfg["S"] == data["labels"].shape[0]
        bad = dict(data)
        bad["att_feats"] = data["att_feats"].copy()
        bad["att_feats"][1] += 1.0
        tr2 = Trainer(opt)
        with pytest.raises(ValueError, match="not 2-fold replicated|not %d-fold replicated" % cfg["S"]):
            tr2.to_device(bad)


def test_full_size_properties_bf16():
    """BASELINE config 2 at full size (N = 640): size-independent properties instead of an oracle run."""
    from unpaired_image_captioning_amd.trainer import xe_step
    V, E, H, A, D, L = 9487, 512, 512, 512, 2048, 16
    cfg = dict(V=V, E=E, H=H, A=A, D=D, L=L)
    Wt = O.init_weights(V + 1, E, H, A, D, D, seed=7)
    b = O.synthetic_batch(128, 5, 36, D, V, L, seed=1234)
    batch = {k: v.cuda() for k, v in b.items()}
    model = build_model(cfg, Wt, "bf16").eval()
    logp = model(batch["fc_feats"], None, batch["att_feats"], batch["labels"], batch["att_masks"])
    assert torch.isfinite(logp).all()
    t_run = model._steps_to_run(batch["labels"])
    assert (logp[:, :t_run].exp().sum(2) - 1).abs().max().item() < 2e-3   # each row is a distribution
    # the S = 5 replicas of an image share features: rows with equal label prefixes agree exactly
    l0 = logp[:, 0].view(128, 5, -1)
    assert (l0 - l0[:, :1]).abs().max().item() == 0.0                    # step 0 input is BOS for every row
    loss, grads = xe_step(model, batch)
    ref_first = -logp[:, 0].gather(1, batch["labels"][:, 1:2]).mean().item()
    assert torch.isfinite(loss) and abs(loss.item() - np.log(V + 1)) < 1.0 and ref_first > 0
    for k, g in grads.items():
        assert torch.isfinite(g).all(), k
    # linearity of backward in the upstream gradient: 2x grad_scale through the criterion scale
    f32 = build_model(cfg, Wt, "f32").eval()
    idx = torch.arange(0, 640, 160)
    sub = {k: v[idx].contiguous() for k, v in batch.items()}
    l_b = model(sub["fc_feats"], None, sub["att_feats"], sub["labels"], sub["att_masks"])
    l_f = f32(sub["fc_feats"], None, sub["att_feats"], sub["labels"], sub["att_masks"])
    assert absmax(l_b, l_f) < 1e-2


# ---------------------------------------------------------------- opt.use_bn (reference default 1, P/opts.py:52)
BN_FIXTURES = ["topdown_tiny_bn1_eval", "topdown_tiny_bn2_train", "topdown_tiny_logit3_bn1", "topdown_tiny_box_bn1"]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", BN_FIXTURES)
def test_use_bn_forward_backward_and_running_stats_vs_reference_golden(name, dtype):
    """BatchNorm1d in att_embed over the packed live regions: train mode (batch statistics + running-stat update,
    use_bn=2) and eval mode (running statistics, use_bn=1), forward + loss + every gradient incl. the BN affine
    parameters, then the greedy decode the reference ran afterwards with the updated statistics."""
    from unpaired_image_captioning_amd.misc.criterion import LanguageModelCriterion
    cfg, W, I, Out, G, X = load_golden(name)
    model = build_model(cfg, W, dtype)
    model.train(bool(cfg["bn_train"]))
    fc, att, labels, masks, am = (I[k].cuda() for k in ("fc_feats", "att_feats", "labels", "masks", "att_masks"))
    logp = model(fc, None, att, labels, am)
    assert absmax(logp, Out["logprobs"]) < LOGP_TOL[dtype]
    loss = LanguageModelCriterion(make_opt(cfg, dtype))(logp, labels[:, 1:], masks[:, 1:])
    assert abs(loss.item() - float(Out["loss"])) < LOGP_TOL[dtype]
    loss.backward()
    assert set(G) == set(k for k, _ in model.named_parameters())
    grads_close({k: p.grad for k, p in model.named_parameters()}, G, GRAD_TOL[dtype])
    sd = model.state_dict()
    n_stats = 0
    for k, v in X.items():
        if k.startswith("bnstat::"):
            key = k.split("::", 1)[1]
            ref = torch.as_tensor(v).double()
            got = sd[key].detach().cpu().double()
            tol = 1e-4 if dtype == "f32" else 3e-3           # BatchNorm1d(H) sees bf16 activations in bf16 mode
            assert (got - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item()), key
            assert not torch.equal(ref, W[key].double())          # the fixture really moved them
            n_stats += 1
    assert n_stats == (3 * cfg["use_bn"] if cfg["bn_train"] else 0)       # running_mean, running_var, num_batches_tracked per BatchNorm
    if dtype == "f32":
        model.eval()
        idx = torch.arange(cfg["n_img"]) * cfg["S"]
        seq, lp = model(fc[idx], None, att[idx], am[idx], opt={"sample_max": 1}, mode="sample")
        assert torch.equal(seq.cpu(), Out["greedy_seq"])
        assert absmax(lp, Out["greedy_logp"]) < 1e-3


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("use_bn", [1, 2])
def test_use_bn_training_step_with_dropout_vs_oracle(use_bn, dtype):
    """Fused two-stream training step with use_bn and dropout 0.5 at a mid size (ragged region counts), against the
    oracle fed with the kernels' own dropout masks; also: the self-critical replay (training flag bit 1) must leave
    the running statistics alone."""
    from unpaired_image_captioning_amd import _lib as L
    from unpaired_image_captioning_amd.trainer import xe_step
    cfg = dict(V=300, E=64, H=96, A=64, D=160, L=7, n_img=12, S=3, R=9, use_bn=use_bn, bn_train=1)
    from unpaired_image_captioning_amd import models
    torch.manual_seed(3)
    model = models.setup(make_opt(cfg, dtype, drop=0.5, seed=21))
    g = torch.Generator().manual_seed(4)
    for k, v in model.state_dict().items():                       # non-trivial affine parameters / running stats
        if "att_embed.0" in k and use_bn or "att_embed.4" in k:
            if k.endswith("weight"):
                v.copy_(1 + 0.2 * torch.randn(v.shape, generator=g))
            elif k.endswith("bias") or k.endswith("running_mean"):
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
            elif k.endswith("running_var"):
                v.copy_(0.5 + torch.rand(v.shape, generator=g))
    W = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.cuda().train()
    b = O.synthetic_batch(cfg["n_img"], cfg["S"], cfg["R"], cfg["D"], cfg["V"], cfg["L"], seed=8, ragged_regions=True)
    batch = {k: v.cuda() for k, v in b.items()}
    loss, grads, seed = xe_step(model, batch, return_seed=True)
    lib = L.load()
    N, R, H, E = batch["fc_feats"].shape[0], batch["att_feats"].shape[1], cfg["H"], cfg["E"]
    T = batch["labels"].shape[1] - 1

    def mask(n, site):
        out = torch.empty(n, device="cuda")
        L.check(lib.uic_dropout_mask(L.ptr(out), n, 0.5, seed, site, 0, L.stream()))
        return out.cpu()

    drop = dict(fc=mask(N * H, L.SITE_FC).view(N, H), att=mask(N * R * H, L.SITE_ATT).view(N, R, H),
                embed=mask(T * N * E, L.SITE_EMBED).view(T, N, E),
                out=torch.stack([mask(N * H, L.SITE_OUT0 + t).view(N, H) for t in range(T)]))
    Wo = {k: v.clone() for k, v in W.items()}
    loss_o, grads_o, _ = O.xe_loss_and_grads(Wo, b["fc_feats"], b["att_feats"], b["labels"], b["masks"], b["att_masks"], drop,
                                             use_bn, True)
    assert abs(loss.item() - loss_o.item()) < LOGP_TOL[dtype]
    # bf16: train-mode BatchNorm makes the column sums of the gradient behind it cancel (sum over the batch of d xhat is
    # 0), so the bias-type gradients in front of it (att_embed.0.bias, att_embed.1.bias) are small differences of
    # bf16-rounded terms: L2 tolerance 0.15 instead of 0.1 for this test; f32 stays at 2e-3 on the worst entry
    grads_close(grads, grads_o, GRAD_TOL[dtype] if dtype == "f32" else 0.15)
    sd = model.state_dict()
    for k in W:
        if "running" in k:
            assert absmax(sd[k], Wo[k]) <= (1e-4 if dtype == "f32" else 3e-3) * max(1.0, Wo[k].abs().max().item()), k
            assert absmax(sd[k], W[k]) > 1e-4
    # replay flag: same step again with bit 1 set -> identical loss / grads, running stats untouched
    before = {k: v.clone() for k, v in sd.items() if "running" in k}
    eng = model.engine
    pd = {k: v.detach() for k, v in model.param_dict().items()}
    g2 = {k: torch.empty_like(v) for k, v in pd.items()}
    t_run = model._steps_to_run(batch["labels"])
    out2 = eng.xe_train_step(pd, batch["fc_feats"], batch["att_feats"], batch["att_masks"], batch["labels"], batch["masks"],
                             t_run, 1 | 2, seed, g2)
    for k, v in before.items():
        assert torch.equal(model.state_dict()[k], v), k
    assert abs(out2[0].item() - loss.item()) < 1e-6


# ---------------------------------------------------------------- scheduled sampling (AttModel.py:130-143)
def _ss_run(model, batch, ss_prob, seed_counter):
    """One fused training step with scheduled sampling; returns loss, grads, the inputs actually used [N, t_run], the
    per-step selection mask [t_run, N] (from the kernels' own uniforms) and the dropout seed."""
    from unpaired_image_captioning_amd import _lib as L
    lib = L.load()
    eng = model.engine
    model._seed_counter = seed_counter
    seed = model.next_seed()
    pd = {k: v.detach() for k, v in model.param_dict().items()}
    grads = {k: torch.empty_like(v) for k, v in pd.items()}
    labels = batch["labels"]
    N, T = labels.shape[0], labels.shape[1] - 1
    t_run = model._steps_to_run(labels)
    out, ws = eng.xe_train_step(pd, batch["fc_feats"], batch["att_feats"], batch.get("att_masks"), labels, batch["masks"],
                                t_run, True, seed, grads, ss_prob=ss_prob, keep_workspace=True)
    torch.cuda.synchronize()
    used = eng.workspace_tensor(ws, "tok_used", (N, T), torch.int64)[:, :t_run].cpu().clone()
    eng.release(ws)
    sel = torch.zeros(t_run, N, dtype=torch.bool)
    for t in range(1, t_run):
        m = torch.empty(N, device="cuda")
        L.check(lib.uic_dropout_mask(L.ptr(m), N, ss_prob, seed, L.SITE_SS_MASK0 + t, 0, L.stream()))
        sel[t] = (m == 0).cpu()
    return out[0], grads, used, sel, seed


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_scheduled_sampling_step_vs_oracle(dtype):
    cfg, W, I, Out, G, X = load_golden("topdown_tiny_ss")
    ss_prob = float(X["ss"][0])
    model = build_model(cfg, W, dtype)
    model.train()
    batch = {k: I[k].cuda() for k in ("fc_feats", "att_feats", "labels", "masks", "att_masks")}
    loss, grads, used, sel, _ = _ss_run(model, batch, ss_prob, 1234)
    labels = I["labels"]
    t_run = used.shape[1]
    assert torch.equal(used[:, 0], labels[:, 0])
    keep = ~sel.t()
    assert torch.equal(used[keep], labels[:, :t_run][keep])             # unselected rows are teacher-forced
    assert sel[1:].any() and (used != labels[:, :t_run]).any()          # and some inputs really were re-sampled
    assert int(used.max()) <= cfg["V"] and int(used.min()) >= 0
    loss_o, grads_o, _ = O.xe_loss_and_grads(W, I["fc_feats"], I["att_feats"], labels, I["masks"], I["att_masks"], None, 0, True,
                                             ss={"prob": ss_prob, "mask": sel, "tokens": used})
    assert abs(loss.item() - loss_o.item()) < LOGP_TOL[dtype]
    grads_close(grads, grads_o, GRAD_TOL[dtype])
    assert abs(loss.item() - float(Out["loss"])) > 1e-5                 # different draws than the CPU golden's


def test_scheduled_sampling_api_path_equals_fused_path_and_eval_ignores_it():
    from unpaired_image_captioning_amd.misc.criterion import LanguageModelCriterion
    cfg, W, I, Out, G, X = load_golden("topdown_tiny_ss")
    model = build_model(cfg, W, "f32")
    model.train()
    model.ss_prob = 0.5
    batch = {k: I[k].cuda() for k in ("fc_feats", "att_feats", "labels", "masks", "att_masks")}
    loss_f, grads_f, used, sel, _ = _ss_run(model, batch, 0.5, 99)
    model._seed_counter = 99
    logp = model(batch["fc_feats"], None, batch["att_feats"], batch["labels"], batch["att_masks"])
    loss = LanguageModelCriterion(make_opt(cfg, "f32"))(logp, batch["labels"][:, 1:], batch["masks"][:, 1:])
    loss.backward()
    assert abs(loss.item() - loss_f.item()) < 1e-5
    for k, p in model.named_parameters():
        assert (p.grad - grads_f[k]).abs().max().item() <= 1e-5 * max(1.0, grads_f[k].abs().max().item()), k
    model.eval()                                                        # `self.training and ...` (:130)
    with torch.no_grad():
        lp_eval = model(batch["fc_feats"], None, batch["att_feats"], batch["labels"], batch["att_masks"])
    model.ss_prob = 0.0
    with torch.no_grad():
        lp_tf = model(batch["fc_feats"], None, batch["att_feats"], batch["labels"], batch["att_masks"])
    assert torch.equal(lp_eval, lp_tf)
    assert absmax(lp_tf, Out["logprobs"]) > 1e-4                        # golden logprobs are the ss ones


def test_scheduled_sampling_draw_statistics():
    """Selection rate ~ ss_prob and the drawn tokens follow exp(previous log-probs): E[p(drawn)] = sum p^2."""
    cfg = dict(V=40, E=32, H=32, A=32, D=64, L=8, n_img=100, S=3, R=4)
    from unpaired_image_captioning_amd import models
    torch.manual_seed(5)
    model = models.setup(make_opt(cfg, "f32", seed=3))
    with torch.no_grad():
        model.logit.weight.mul_(60.0)                                   # peaky, row-dependent distributions
    W = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.cuda().train()
    b = O.synthetic_batch(cfg["n_img"], cfg["S"], cfg["R"], cfg["D"], cfg["V"], cfg["L"], seed=2)
    batch = {k: v.cuda() for k, v in b.items()}
    ss_prob = 0.4
    loss, grads, used, sel, _ = _ss_run(model, batch, ss_prob, 7)
    t_run = used.shape[1]
    rate = sel[1:].float().mean().item()
    n_dec = sel[1:].numel()
    assert abs(rate - ss_prob) < 4 * (ss_prob * (1 - ss_prob) / n_dec) ** 0.5 + 1e-3, rate
    # replay on the oracle to get every step's previous distribution
    logp, aux = O.forward_logprobs(W, b["fc_feats"], b["att_feats"], b["labels"], b["att_masks"], None, 0, True, True,
                                   ss={"prob": ss_prob, "mask": sel, "tokens": used})
    got, want, var = 0.0, 0.0, 0.0
    for t in range(1, t_run):
        p = logp[:, t - 1].exp()[sel[t]]
        drawn = used[:, t][sel[t]]
        got += p.gather(1, drawn[:, None]).sum().item()
        want += (p * p).sum().item()
        var += ((p ** 3).sum(1) - (p * p).sum(1) ** 2).sum().item()
    n = int(sel[1:].sum())
    assert n > 500
    assert abs(got - want) < 5 * var ** 0.5 + 1e-6, (got / n, want / n)
    uniform_expect = 1.0 / (cfg["V"] + 1)
    assert got / n > 2 * uniform_expect                                 # clearly not uniform draws


# ---------------------------------------------------------------- beam search
BEAM_TAGS = ("b3", "b2c", "b3eos", "b4ppl")


@pytest.mark.parametrize("name", FIXTURES + BN_FIXTURES)
def test_beam_search_token_ids_bit_exact_vs_reference_golden(name):
    """AttModel._sample_beam + CaptionModel.beam_search (beam 2-4, decoding_constraint, max_ppl, early-finishing beams via a
    raised EOS bias): f32 token ids identical to the reference's, per-step log-probs within 1e-3."""
    cfg, W, I, Out, G, X = load_golden(name)
    W = dict(W)
    for k, v in X.items():          # the reference decoded after its train-mode forward updated BN stats
        if k.startswith("bnstat::"):
            W[k.split("::", 1)[1]] = torch.as_tensor(v)
    model = build_model(cfg, W, "f32").eval()
    idx = torch.arange(cfg["n_img"]) * cfg["S"]
    fc, att = I["fc_feats"][idx].cuda(), I["att_feats"][idx].cuda()
    am = I["att_masks"][idx].cuda() if "att_masks" in I else None
    for tag in BEAM_TAGS:
        bs, dc, mp, eos_bias = [float(x) for x in X["beam::%s_cfg" % tag]]
        with torch.no_grad():
            final_logit(model).bias[0] += eos_bias
        seq, lp = model(fc, None, att, am, opt={"sample_max": 1, "beam_size": int(bs), "decoding_constraint": int(dc), "max_ppl": int(mp)},
                        mode="sample")
        with torch.no_grad():
            final_logit(model).bias[0] -= eos_bias
        ref_seq = torch.as_tensor(X["beam::%s_seq" % tag])
        assert torch.equal(seq.cpu(), ref_seq), (tag, seq.cpu(), ref_seq)
        assert absmax(lp, torch.as_tensor(X["beam::%s_logp" % tag])) < 1e-3, tag
        assert len(model.done_beams) == cfg["n_img"] and torch.equal(model.done_beams[0][0]["seq"], seq[0])


@pytest.mark.parametrize("name", FIXTURES[:2] + BN_FIXTURES[:1])
def test_diverse_beam_groups_return_value_vs_reference_golden(name):
    """group_size > 1: _sample_beam returns the best beam of group 0 (AttModel.py:193-194), the group without a diversity
    penalty -- token ids identical to the reference's diverse search (tests/test_oracle_golden.py proves the equivalence
    with the full staggered algorithm)."""
    cfg, W, I, Out, G, X = load_golden(name)
    W = dict(W)
    for k, v in X.items():
        if k.startswith("bnstat::"):
            W[k.split("::", 1)[1]] = torch.as_tensor(v)
    model = build_model(cfg, W, "f32").eval()
    idx = torch.arange(cfg["n_img"]) * cfg["S"]
    fc, att = I["fc_feats"][idx].cuda(), I["att_feats"][idx].cuda()
    am = I["att_masks"][idx].cuda() if "att_masks" in I else None
    for tag in ("g2b4", "g3b6eos"):
        bs, gs, dc, mp, eos_bias, lam = [float(x) for x in X["beamg::%s_cfg" % tag]]
        with torch.no_grad():
            final_logit(model).bias[0] += eos_bias
        seq, lp = model(fc, None, att, am, opt={"sample_max": 1, "beam_size": int(bs), "group_size": int(gs),
                                                "diversity_lambda": lam, "decoding_constraint": int(dc),
                                                "max_ppl": int(mp)}, mode="sample")
        with torch.no_grad():
            final_logit(model).bias[0] -= eos_bias
        assert torch.equal(seq.cpu(), torch.as_tensor(X["beamg::%s_seq" % tag])), tag
        assert absmax(lp, torch.as_tensor(X["beamg::%s_logp" % tag])) < 1e-3, tag


def test_beam_search_bf16_and_real_vocab_vs_oracle():
    """bf16 + a 9488-word vocabulary on a few images: the device's beams scored by the oracle (same tokens re-run through
    the oracle's beam search must agree unless two candidates tie within bf16 noise, so compare log-probs of the
    device's own sequences teacher-forced through the oracle)."""
    cfg = dict(V=9487, E=64, H=64, A=64, D=128, L=8, n_img=5, S=1, R=6)
    from unpaired_image_captioning_amd import models
    torch.manual_seed(9)
    model = models.setup(make_opt(cfg, "bf16", seed=1))
    with torch.no_grad():
        model.logit.weight.mul_(20.0)
        final_logit(model).bias[0] += 2.0
    W = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.cuda().eval()
    b = O.synthetic_batch(cfg["n_img"], 1, cfg["R"], cfg["D"], cfg["V"], cfg["L"], seed=4, ragged_regions=True)
    seq, lp = model(b["fc_feats"].cuda(), None, b["att_feats"].cuda(), b["att_masks"].cuda(), opt={"beam_size": 3}, mode="sample")
    seq, lp = seq.cpu(), lp.cpu()
    assert seq.shape == (cfg["n_img"], cfg["L"]) and int(seq.max()) <= cfg["V"]
    # teacher-force the device's sequences through the oracle and compare the recorded per-step log-probs
    labels = torch.cat([torch.zeros(cfg["n_img"], 1, dtype=torch.long), seq, torch.zeros(cfg["n_img"], 1, dtype=torch.long)], 1)
    logp = O.forward_logprobs(W, b["fc_feats"], b["att_feats"], labels, b["att_masks"])
    for k in range(cfg["n_img"]):
        for t in range(cfg["L"]):
            tok = int(seq[k, t])
            ref = logp[k, t, tok].item() - (1000.0 if tok == cfg["V"] else 0.0)
            assert abs(lp[k, t].item() - ref) < 5e-2, (k, t, lp[k, t].item(), ref)
            if tok == 0:
                assert int(seq[k, t:].abs().sum()) == 0 and float(lp[k, t + 1:].abs().sum()) == 0
                break


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_shapes_off_the_fast_paths_vs_oracle(dtype):
    """R = 50 regions (beyond the 36-region fast attention kernels), A != H != E, 70 caption rows (not a tile multiple), a
    1001-word vocabulary: the generic kernels and the transposing fall-backs of the weight gradients against the oracle."""
    from unpaired_image_captioning_amd import models
    from unpaired_image_captioning_amd.trainer import xe_step
    cfg = dict(V=1000, E=96, H=160, A=128, D=200, L=9, n_img=14, S=5, R=50)
    torch.manual_seed(2)
    model = models.setup(make_opt(cfg, dtype, seed=4))
    W = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.cuda().train()
    b = O.synthetic_batch(cfg["n_img"], cfg["S"], cfg["R"], cfg["D"], cfg["V"], cfg["L"], seed=6, ragged_regions=True)
    batch = {k: v.cuda() for k, v in b.items()}
    loss, grads = xe_step(model, batch)
    loss_o, grads_o, logp_o = O.xe_loss_and_grads(W, b["fc_feats"], b["att_feats"], b["labels"], b["masks"], b["att_masks"])
    assert abs(loss.item() - loss_o.item()) < LOGP_TOL[dtype]
    grads_close(grads, grads_o, GRAD_TOL[dtype])
    model.eval()
    idx = torch.arange(cfg["n_img"]) * cfg["S"]
    seq, lp = model(batch["fc_feats"][idx], None, batch["att_feats"][idx], batch["att_masks"][idx], opt={"sample_max": 1}, mode="sample")
    seq_o, lp_o = O.sample(W, b["fc_feats"][idx], b["att_feats"][idx], b["att_masks"][idx], cfg["L"])
    if dtype == "f32":
        assert torch.equal(seq.cpu(), seq_o)
        assert absmax(lp, lp_o) < 1e-3
        bseq, blp = model(batch["fc_feats"][idx], None, batch["att_feats"][idx], batch["att_masks"][idx], opt={"beam_size": 4}, mode="sample")
        bseq_o, blp_o = O.sample_beam(W, b["fc_feats"][idx], b["att_feats"][idx], b["att_masks"][idx], cfg["L"], 4)
        # untrained weights give nearly flat distributions: two candidates can tie to within f32 rounding and swap between
        # the device and the CPU, so images may differ in the chosen beam -- but only between beams of (numerically) equal
        # score; wherever the tokens agree the recorded log-probs must agree too
        same = (bseq.cpu() == bseq_o).all(1)
        assert same.float().mean().item() >= 0.7
        assert absmax(blp[same.cuda()], blp_o[same]) < 1e-3
        assert (blp.cpu().sum(1) - blp_o.sum(1)).abs().max().item() < 2e-3


@pytest.mark.parametrize("cfg", [
    dict(V=20, E=8, H=8, A=8, D=8, L=1, n_img=1, S=1, R=1),          # one caption row, one region, one word
    dict(V=20, E=16, H=24, A=8, D=16, L=3, n_img=1, S=1, R=2),       # a single row
    dict(V=9, E=8, H=16, A=16, D=24, L=5, n_img=3, S=1, R=7),        # rows with empty captions, see below
    dict(V=300, E=32, H=32, A=32, D=64, L=20, n_img=2, S=2, R=64),   # 64 regions, captions longer than the usual 16
], ids=["1x1x1", "single-row", "empty-captions", "R64-L20"])
def test_degenerate_shapes_vs_oracle(cfg):
    """Smallest and oddest inputs through the fused training step, the API path and the greedy decoder (f32)."""
    from unpaired_image_captioning_amd import models
    from unpaired_image_captioning_amd.trainer import xe_step
    torch.manual_seed(7)
    model = models.setup(make_opt(cfg, "f32", seed=5))
    W = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.cuda().train()
    b = O.synthetic_batch(cfg["n_img"], cfg["S"], cfg["R"], cfg["D"], cfg["V"], cfg["L"], seed=3, ragged_regions=cfg["R"] > 2)
    if cfg["n_img"] == 3:
        b["labels"][1] = 0                                   # a caption with no words: only BOS -> EOS is scored
        b["masks"][1] = 0
        b["masks"][1, :2] = 1
        b["labels"][2, 2:] = 0                               # a one-word caption
        b["masks"][2] = 0
        b["masks"][2, :3] = 1
    batch = {k: v.cuda() for k, v in b.items()}
    loss_o, grads_o, logp_o = O.xe_loss_and_grads(W, b["fc_feats"], b["att_feats"], b["labels"], b["masks"], b["att_masks"])
    for fused in (True, False):
        loss, grads = xe_step(model, batch, fused=fused)
        assert abs(loss.item() - loss_o.item()) < 1e-4, (fused, loss.item(), loss_o.item())
        grads_close(grads, grads_o, GRAD_TOL["f32"])
    logp = model(batch["fc_feats"], None, batch["att_feats"], batch["labels"], batch["att_masks"])
    assert absmax(logp, logp_o) < LOGP_TOL["f32"]
    model.eval()
    seq, lp = model(batch["fc_feats"], None, batch["att_feats"], batch["att_masks"], opt={"sample_max": 1}, mode="sample")
    seq_o, lp_o = O.sample(W, b["fc_feats"], b["att_feats"], b["att_masks"], cfg["L"])
    assert torch.equal(seq.cpu(), seq_o) and absmax(lp, lp_o) < 1e-3


def _sweep_configs(n, seed):
    g = np.random.default_rng(seed)
    out = []
    for i in range(n):
        m8 = lambda lo, hi: int(g.integers(lo, hi + 1)) * 8          # noqa: E731
        out.append(dict(V=int(g.integers(5, 400)), E=m8(1, 20), H=m8(1, 20), A=m8(1, 20), D=m8(1, 30), L=int(g.integers(1, 21)),
                        n_img=int(g.integers(1, 15)), S=int(g.integers(1, 6)), R=int(g.integers(1, 70)),
                        use_bn=int(g.integers(0, 3)), per_image=bool(g.integers(0, 2)), drop=bool(g.integers(0, 2)), idx=i))
    for c in out:                                                    # (drawn afterwards so that the shapes above stay as they were)
        c["logit_layers"] = int(g.integers(1, 4))
    for c in out:                # att_feat_size off the multiples of 8 (box features): fc_feat_size keeps the old value
        c["Dfc"] = c["D"]
        if g.integers(0, 3) == 0:
            c["D"] += int(g.integers(1, 8))
    return out


@pytest.mark.parametrize("cfg", _sweep_configs(48, 2024), ids=lambda c: "cfg%d" % c["idx"])
def test_random_shape_sweep_vs_oracle(cfg):
    """48 seeded random configurations (sizes that are multiples of 8 but of nothing else, 1..14 images x 1..5 captions,
    1..69 regions with ragged masks, 1..20 words, use_bn 0/1/2, logit_layers 1..3, features per caption row or per image,
    dropout on/off):
    the fused f32 training step against the oracle (fed with the kernels' own dropout masks)."""
    from unpaired_image_captioning_amd import _lib as L
    from unpaired_image_captioning_amd import models
    from unpaired_image_captioning_amd.trainer import xe_step
    if cfg["use_bn"] and cfg["n_img"] * cfg["S"] < 2:
        cfg = dict(cfg, n_img=2)                              # batch statistics need more than one row
    torch.manual_seed(100 + cfg["idx"])
    p = 0.5 if cfg["drop"] else 0.0
    model = models.setup(make_opt(cfg, "f32", drop=p, seed=cfg["idx"]))
    gw = torch.Generator().manual_seed(cfg["idx"])
    for k, v in model.state_dict().items():
        if "att_embed" in k and ("running_var" in k):
            v.copy_(0.5 + torch.rand(v.shape, generator=gw))
    W = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.cuda().train()
    b = O.synthetic_batch(cfg["n_img"], cfg["S"], cfg["R"], cfg["D"], cfg["V"], cfg["L"], seed=cfg["idx"], ragged_regions=cfg["R"] > 1)
    b["fc_feats"] = b["fc_feats"][:, :cfg["Dfc"]].contiguous()
    full = {k: v.cuda() for k, v in b.items()}
    batch = _per_image(full, cfg["S"]) if cfg["per_image"] and cfg["S"] > 1 else full
    loss, grads, seed = xe_step(model, batch, return_seed=True)
    N, R, H, E = b["labels"].shape[0], cfg["R"], cfg["H"], cfg["E"]
    T = b["labels"].shape[1] - 1
    drop = None
    nlh = cfg["logit_layers"] - 1
    if p or nlh:
        lib = L.load()

        def mask(n, site, pp=p):
            if not pp:
                return torch.ones(n)
            out = torch.empty(n, device="cuda")
            L.check(lib.uic_dropout_mask(L.ptr(out), n, pp, seed, site, 0, L.stream()))
            return out.cpu()
        drop = dict(fc=mask(N * H, L.SITE_FC).view(N, H), att=mask(N * R * H, L.SITE_ATT).view(N, R, H),
                    embed=mask(T * N * E, L.SITE_EMBED).view(T, N, E),
                    out=torch.stack([mask(N * H, L.SITE_OUT0 + t).view(N, H) for t in range(T)]))
        if nlh:     # the hidden logit blocks' Dropout(0.5) is hard-coded: active in train mode whatever drop_prob_lm is
            drop["logit"] = [mask(T * N * H, L.SITE_LOGIT_H0 + l, 0.5).view(T, N, H) for l in range(nlh)]
    loss_o, grads_o, _ = O.xe_loss_and_grads(W, b["fc_feats"], b["att_feats"], b["labels"], b["masks"], b["att_masks"], drop,
                                             use_bn=cfg["use_bn"], training=True)
    assert abs(loss.item() - loss_o.item()) < 2e-4 * max(1.0, abs(loss_o.item())), (cfg, loss.item(), loss_o.item())
    grads_close(grads, {k: grads_o[k] for k in grads}, 5e-3)


def _sweep_configs_bf16(n, seed):
    g = np.random.default_rng(seed)
    pick = lambda xs: int(xs[int(g.integers(0, len(xs)))])       # noqa: E731
    return [dict(V=int(g.integers(100, 3000)), E=pick([64, 72, 128, 256]), H=pick([64, 128, 136, 256]), A=pick([40, 64, 128, 256, 520]),
                 D=pick([120, 128, 256, 512]), L=int(g.integers(4, 17)), n_img=int(g.integers(4, 41)), S=int(g.integers(1, 6)),
                 R=int(g.integers(4, 37)), use_bn=int(g.integers(0, 3)), per_image=bool(g.integers(0, 2)), idx=i) for i in range(n)]


@pytest.mark.parametrize("cfg", _sweep_configs_bf16(24, 31), ids=lambda c: "bf%d" % c["idx"])
def test_random_shape_sweep_bf16_vs_oracle(cfg):
    """24 seeded random mid-size configurations in bf16 -- sizes on and off the eligibility boundaries of the LDS-DMA and
    transposing-read GEMMs (multiples of 128 / 64 and not), att_hid_size above 4 * rnn_size, up to 200 caption rows --
    the fused training step (dropout off) against the f32 oracle at the bf16 tolerances."""
    from unpaired_image_captioning_amd import models
    from unpaired_image_captioning_amd.trainer import xe_step
    torch.manual_seed(300 + cfg["idx"])
    model = models.setup(make_opt(cfg, "bf16", seed=cfg["idx"]))
    W = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.cuda().train()
    b = O.synthetic_batch(cfg["n_img"], cfg["S"], cfg["R"], cfg["D"], cfg["V"], cfg["L"], seed=cfg["idx"], ragged_regions=True)
    full = {k: v.cuda() for k, v in b.items()}
    batch = _per_image(full, cfg["S"]) if cfg["per_image"] and cfg["S"] > 1 else full
    loss, grads = xe_step(model, batch)
    loss_o, grads_o, _ = O.xe_loss_and_grads(W, b["fc_feats"], b["att_feats"], b["labels"], b["masks"], b["att_masks"], None,
                                             use_bn=cfg["use_bn"], training=True)
    assert abs(loss.item() - loss_o.item()) < LOGP_TOL["bf16"], (cfg, loss.item(), loss_o.item())
    grads_close(grads, {k: grads_o[k] for k in grads}, 0.15 if cfg["use_bn"] else GRAD_TOL["bf16"])


@pytest.mark.parametrize("cfg", _sweep_configs(16, 555), ids=lambda c: "dec%d" % c["idx"])
def test_decode_paths_random_sweep_vs_oracle(cfg):
    """16 seeded random configurations through the decoders (f32, eval mode): multinomial sampling (the device's draws
    replayed by the oracle: same finished-row bookkeeping, same log-probs), greedy (every chosen token is the oracle's
    arg-max up to f32 noise) and beam search (final beam scored by the oracle)."""
    from unpaired_image_captioning_amd import models
    torch.manual_seed(500 + cfg["idx"])
    cfg = dict(cfg, V=max(cfg["V"], 8))
    model = models.setup(make_opt(cfg, "f32", seed=cfg["idx"]))
    gw = torch.Generator().manual_seed(cfg["idx"])
    for k, v in model.state_dict().items():
        if "running_var" in k:
            v.copy_(0.5 + torch.rand(v.shape, generator=gw))
        elif "running_mean" in k:
            v.copy_(0.1 * torch.randn(v.shape, generator=gw))
    with torch.no_grad():
        final_logit(model).bias[0] += 1.5                           # some captions end early
    W = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.cuda().eval()
    b = O.synthetic_batch(cfg["n_img"], 1, cfg["R"], cfg["D"], cfg["V"], cfg["L"], seed=cfg["idx"], ragged_regions=cfg["R"] > 1)
    b["fc_feats"] = b["fc_feats"][:, :cfg["Dfc"]].contiguous()
    fc, att, am = b["fc_feats"].cuda(), b["att_feats"].cuda(), b["att_masks"].cuda()
    ub = cfg["use_bn"]
    dc = cfg["idx"] % 2
    seq, lp = model(fc, None, att, am, opt={"sample_max": 0, "temperature": 1.0, "decoding_constraint": dc}, mode="sample")
    seq_o, lp_o = O.sample(W, b["fc_feats"], b["att_feats"], b["att_masks"], cfg["L"], sample_max=0, forced_tokens=seq.cpu(),
                           decoding_constraint=dc, use_bn=ub)
    # positions after a row's first 0 hold the log-prob of whatever was drawn there (AttModel.py:232-251 keeps sampling
    # for finished rows and stores token 0); the replay only knows the stored 0, so compare up to the first 0 -- the
    # positions RewardCriterion's mask keeps (criterion.py:113-116)
    live = torch.cat([torch.ones_like(seq[:, :1]), (seq[:, :-1] > 0).long().cumprod(1)], 1).bool().cpu()
    assert torch.equal(seq_o, seq.cpu()) and absmax(lp.cpu()[live], lp_o[live]) < 1e-3
    gseq, glp = model(fc, None, att, am, opt={"sample_max": 1, "decoding_constraint": dc}, mode="sample")
    gseq_o, glp_o = O.sample(W, b["fc_feats"], b["att_feats"], b["att_masks"], cfg["L"], sample_max=1, decoding_constraint=dc, use_bn=ub)
    same = (gseq.cpu() == gseq_o).all(1)
    assert same.float().mean().item() >= 0.6                  # untrained weights: near-ties may resolve differently
    assert absmax(glp[same.cuda()], glp_o[same]) < 1e-3
    # rows that differ: the device's tokens, replayed by the oracle, must score within f32 noise of the oracle's own choice
    if (~same).any():
        r_seq, r_lp = O.sample(W, b["fc_feats"], b["att_feats"], b["att_masks"], cfg["L"], sample_max=0, forced_tokens=gseq.cpu(),
                               decoding_constraint=dc, use_bn=ub)
        first = (gseq.cpu() != gseq_o).float().argmax(1)
        for n in (~same).nonzero().view(-1).tolist():
            t = int(first[n])
            assert abs(float(r_lp[n, t]) - float(glp_o[n, t])) < 1e-4, (n, t)
    K = 2 + cfg["idx"] % 3
    if K <= cfg["V"]:
        bseq, blp = model(fc, None, att, am, opt={"beam_size": K, "decoding_constraint": dc}, mode="sample")
        bseq_o, blp_o = O.sample_beam(W, b["fc_feats"], b["att_feats"], b["att_masks"], cfg["L"], K, dc, 0, use_bn=ub)
        sameb = (bseq.cpu() == bseq_o).all(1)
        assert sameb.float().mean().item() >= 0.6
        assert absmax(blp[sameb.cuda()], blp_o[sameb]) < 1e-3
        assert (blp.cpu().sum(1) - blp_o.sum(1)).abs().max().item() < 5e-3      # beams that differ tie in score


# ---------------------------------------------------------------- features once per image (dims.seq_per_img > 1)
def _per_image(batch, S):
    out = dict(batch)
    for k in ("fc_feats", "att_feats", "att_masks"):
        if out.get(k) is not None:
            full = out[k]
            assert torch.equal(full.view(-1, S, *full.shape[1:])[:, 0], full[::S])
            for j in range(1, S):
                assert torch.equal(full[j::S], full[::S]), "fixture rows are not replicated"
            out[k] = full[::S].contiguous()
    return out


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("use_bn", [0, 1, 2])
@pytest.mark.parametrize("fused", [True, False])
def test_features_per_image_equal_replicated_batch(dtype, use_bn, fused):
    """The loader's S-fold replication done on the device (dims.seq_per_img = S): a training step with dropout 0.5 on
    per-image features (ragged region counts) must give the loss and gradients of the replicated batch -- the same
    dropout masks per caption row; the att_embed Linear runs per image (use_bn = 0) and its weight gradient over the
    S-summed row gradients."""
    from unpaired_image_captioning_amd import models
    from unpaired_image_captioning_amd.trainer import xe_step
    cfg = dict(V=300, E=64, H=96, A=64, D=160, L=7, n_img=12, S=3, R=9, use_bn=use_bn)
    torch.manual_seed(5)
    b = O.synthetic_batch(cfg["n_img"], cfg["S"], cfg["R"], cfg["D"], cfg["V"], cfg["L"], seed=9, ragged_regions=True)
    full = {k: v.cuda() for k, v in b.items()}
    img = _per_image(full, cfg["S"])
    assert img["att_feats"].shape[0] * cfg["S"] == full["att_feats"].shape[0] == full["labels"].shape[0]
    res = []
    for batch in (full, img):
        torch.manual_seed(3)
        model = models.setup(make_opt(cfg, dtype, drop=0.5, seed=21)).cuda().train()
        loss, grads = xe_step(model, batch, fused=fused)
        res.append((loss.item(), {k: v.float().cpu() for k, v in grads.items()},
                    {k: v.float().cpu().clone() for k, v in model.state_dict().items() if "running" in k}))
    (l0, g0, s0), (l1, g1, s1) = res
    assert abs(l0 - l1) < (1e-5 if dtype == "f32" else 2e-3), (l0, l1)
    grads_close(g1, g0, 2e-4 if dtype == "f32" else 3e-2)
    for k in s0:
        assert absmax(s1[k], s0[k]) < 1e-6, k


def test_features_per_image_sampling_and_forward_logprobs():
    """mode='forward' log-probs and the multinomial sampling pass with per-image features (labels / rows per caption)."""
    from unpaired_image_captioning_amd import models
    cfg = dict(V=300, E=64, H=96, A=64, D=160, L=7, n_img=6, S=4, R=9, use_bn=0)
    b = O.synthetic_batch(cfg["n_img"], cfg["S"], cfg["R"], cfg["D"], cfg["V"], cfg["L"], seed=2, ragged_regions=True)
    full = {k: v.cuda() for k, v in b.items()}
    img = _per_image(full, cfg["S"])
    torch.manual_seed(1)
    model = models.setup(make_opt(cfg, "f32", drop=0.5, seed=7)).cuda().train()
    outs = []
    for batch in (full, img):
        model._seed_counter = 77
        lp = model(batch["fc_feats"], None, batch["att_feats"], batch["labels"], batch["att_masks"])
        outs.append(lp.detach().cpu())
    assert outs[0].shape == outs[1].shape and absmax(outs[1], outs[0]) < 1e-5
    eng = model.engine
    pd = {k: v.detach() for k, v in model.param_dict().items()}
    s0, lp0 = eng.sample(pd, full["fc_feats"], full["att_feats"], full["att_masks"], cfg["L"], sample_max=0, seed=5, training=True)
    s1, lp1 = eng.sample(pd, img["fc_feats"], img["att_feats"], img["att_masks"], cfg["L"], sample_max=0, seed=5, training=True,
                         seq_per_img=cfg["S"])
    assert torch.equal(s0, s1) and absmax(lp1, lp0) < 1e-5


def test_features_per_image_argument_errors():
    from unpaired_image_captioning_amd import models
    cfg = dict(V=50, E=32, H=32, A=32, D=64, L=6, n_img=3, S=2, R=5, use_bn=0)
    b = O.synthetic_batch(cfg["n_img"], cfg["S"], cfg["R"], cfg["D"], cfg["V"], cfg["L"], seed=2)
    full = {k: v.cuda() for k, v in b.items()}
    model = models.setup(make_opt(cfg, "f32")).cuda()
    with pytest.raises(ValueError, match="whole number"):
        model(full["fc_feats"][:4], None, full["att_feats"][:4], full["labels"], None)


def test_self_critical_step_per_image_features_equal_replicated():
    """Trainer.train_self_critical with every image shipped once (opt.seq_per_img: sampling pass with S captions per image,
    greedy baseline decoded once per image, replay with device-side replication) == the replicated batch."""
    from unpaired_image_captioning_amd.trainer import Trainer
    cfg, W, I, Out, G, X = load_golden("topdown_tiny_ragged")
    data = {k: I[k].numpy() for k in ("fc_feats", "att_feats", "labels", "masks", "att_masks")}

    def reward_fn(data, sampled, greedy):
        r = np.where(sampled[:, :1] % 2 == 0, 1.0, -1.0) - np.where(greedy[:, :1] % 2 == 0, 0.5, -0.5)
        return np.repeat(r, sampled.shape[1], 1)

    res = []
    for ship_replicated in (1, 0):
        opt = make_opt(cfg, "f32", drop=0.5, seed=3)
        opt.i2t_learning_rate = 1e-3
        opt.seq_per_img = cfg["S"]
        opt.ship_replicated_features = ship_replicated
        tr = Trainer(opt)
        tr.i2t_model.load_state_dict(W)
        tr.build_optimizer()
        assert tr.to_device(data)["att_feats"].shape[0] == (len(data["labels"]) if ship_replicated else len(data["labels"]) // cfg["S"])
        losses = [tr.train_self_critical(data, reward_fn) for _ in range(3)]
        res.append((losses, {k: v.detach().cpu().clone() for k, v in tr.i2t_model.state_dict().items()}))
    (l0, w0), (l1, w1) = res
    np.testing.assert_allclose(l1, l0, rtol=0, atol=1e-5)
    for k in w0:
        assert absmax(w1[k], w0[k]) < 2e-5, k


def test_trainer_prefetch_next_batch_equals_plain_training():
    """Trainer.train(data, next_data=...) ships batch k+1 on a copy stream while batch k computes: same losses and final
    weights as shipping every batch when it is needed; a batch that was not the prefetched one is shipped normally."""
    from unpaired_image_captioning_amd.trainer import Trainer
    cfg, W, I, Out, G, X = load_golden("topdown_tiny_ragged")
    base = {k: I[k].numpy() for k in ("fc_feats", "att_feats", "labels", "masks", "att_masks")}
    g = np.random.default_rng(0)
    batches = []
    for i in range(4):
        d = {k: v.copy() for k, v in base.items()}
        perm = g.permutation(len(d["labels"]) // cfg["S"])
        for k in d:
            d[k] = d[k].reshape(len(perm), cfg["S"], *d[k].shape[1:])[perm].reshape(d[k].shape)
        d["fc_feats"] = d["fc_feats"] * (1.0 + 0.1 * i)
        batches.append(d)
    res = []
    for mode in ("plain", "prefetch"):
        opt = make_opt(cfg, "f32", seed=3)
        opt.i2t_learning_rate = 1e-3
        opt.seq_per_img = cfg["S"]
        tr = Trainer(opt)
        tr.i2t_model.load_state_dict(W)
        tr.build_optimizer()
        losses = []
        for i, d in enumerate(batches):
            if mode == "plain":
                losses.append(tr.train(d))
            else:
                nxt = batches[i + 1] if i + 1 < len(batches) and i != 1 else None     # step 2's batch is NOT prefetched
                losses.append(tr.train(d, next_data=nxt))
        res.append((losses, {k: v.detach().cpu().clone() for k, v in tr.i2t_model.state_dict().items()}))
    (l0, w0), (l1, w1) = res
    assert l0 == l1, (l0, l1)
    for k in w0:
        assert torch.equal(w0[k], w1[k]), k


def test_hold_weights_refreshes_again_after_the_block():
    """engine.hold_weights() (one weight refresh for the passes of a self-critical step) must not outlive its block: a
    parameter changed afterwards is seen by the next call; inside the block the first call refreshes."""
    cfg, W, I, Out, G, X = load_golden("topdown_tiny")
    model = build_model(cfg, W, "f32").eval()
    fc, att, labels, am = (I[k].cuda() for k in ("fc_feats", "att_feats", "labels", "att_masks"))
    with torch.no_grad():
        base = model(fc, None, att, labels, am).clone()
        with model.engine.hold_weights():
            a = model(fc, None, att, labels, am)
            b = model(fc, None, att, labels, am)          # no refresh here
        assert torch.equal(a, base) and torch.equal(b, base)
        final_logit(model).bias[3] += 1.0
        c = model(fc, None, att, labels, am)
        assert (c - base).abs().max().item() > 1e-2       # the change is picked up: the hold is over
        with model.engine.hold_weights():
            d = model(fc, None, att, labels, am)          # first call inside a new block refreshes too
        assert torch.equal(c, d)


def test_multinomial_draws_follow_the_softmax():
    """The inverse-CDF draw of sample_step_kernel (segment scan across the workgroup + owner search): 8192 rows of ONE image
    draw their first token independently (the uniform number is a hash of the row index), so the histogram must match the
    model's own step-0 probabilities; every category within 5 sigma, and the total variation distance small."""
    cfg, W, I, Out, G, X = load_golden("topdown_tiny")
    model = build_model(cfg, W, "f32")
    model.eval()
    N = 8192
    fc = I["fc_feats"][:1].repeat(N, 1).cuda()
    att = I["att_feats"][:1].repeat(N, 1, 1).cuda()
    am = I["att_masks"][:1].repeat(N, 1).cuda()
    with torch.no_grad():
        seq, _ = model(fc, None, att, am, opt={"sample_max": 0, "temperature": 1.0}, mode="sample")
        labels = torch.zeros(1, cfg["L"] + 2, dtype=torch.long).cuda()
        logp = model(fc[:1], None, att[:1], labels, am[:1])
    p = logp[0, 0].exp().double().cpu()
    counts = torch.bincount(seq[:, 0].cpu(), minlength=p.numel()).double()
    sigma = (N * p * (1 - p)).sqrt().clamp_min(1.0)
    assert ((counts - N * p).abs() / sigma).max().item() < 5.0
    assert 0.5 * (counts / N - p).abs().sum().item() < 0.05


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("fused", [True, False])
def test_input_feature_gradients_vs_oracle(dtype, per_image, fused):
    """Optional outputs Batch.d_fc_feats / d_att_feats (an encoder in front of the captioner, BASELINE configs[4]): the loss
    gradient w.r.t. the input features against autograd through the oracle; with per-image features the S caption rows of
    an image are summed; padded regions get exact zeros; the weight gradients are untouched by asking for them."""
    from unpaired_image_captioning_amd import models
    from unpaired_image_captioning_amd.trainer import xe_step
    cfg = dict(V=300, E=64, H=96, A=64, D=157, Dfc=136, L=7, n_img=12, S=3, R=9)        # D is padded to 160 columns inside
    torch.manual_seed(5)
    model = models.setup(make_opt(cfg, dtype, seed=4))
    W = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.cuda().train()
    b = O.synthetic_batch(cfg["n_img"], cfg["S"], cfg["R"], cfg["D"], cfg["V"], cfg["L"], seed=9, ragged_regions=True)
    b["fc_feats"] = b["fc_feats"][:, :1].repeat(1, cfg["Dfc"]) * torch.linspace(0.5, 1.5, cfg["Dfc"])   # Dfc != D
    fc_o = b["fc_feats"].clone().requires_grad_(True)
    att_o = b["att_feats"].clone().requires_grad_(True)
    loss_o, grads_o, _ = O.xe_loss_and_grads(W, fc_o, att_o, b["labels"], b["masks"], b["att_masks"])
    dfc_o, datt_o = fc_o.grad, att_o.grad
    batch = {k: v.cuda() for k, v in b.items()}
    if per_image:
        batch = _per_image(batch, cfg["S"])
        dfc_o = dfc_o.view(cfg["n_img"], cfg["S"], -1).sum(1)
        datt_o = datt_o.view(cfg["n_img"], cfg["S"], cfg["R"], -1).sum(1)
    d_fc, d_att = model.engine.input_grad_buffers(batch["fc_feats"], batch["att_feats"])
    d_fc.fill_(float("nan"))
    d_att.fill_(float("nan"))
    loss, grads = xe_step(model, batch, fused=fused, d_fc=d_fc, d_att=d_att)
    assert abs(loss.item() - loss_o.item()) < LOGP_TOL[dtype]
    grads_close(grads, grads_o, GRAD_TOL[dtype])
    d_att = d_att[..., :cfg["D"]]
    # bf16: d att_feats sits behind the whole bf16 backward (attention, both ReLU masks, bf16 d_pre x bf16 W_att) -- 5e-2 measured
    tol = 2e-4 if dtype == "f32" else 8e-2
    for name, got, ref in (("d_fc", d_fc, dfc_o), ("d_att", d_att, datt_o)):
        got = got.cpu().double()
        assert torch.isfinite(got).all(), name
        err = ((got - ref.double()).norm() / ref.double().norm()).item()
        assert err < tol, (name, err)
    dead = batch["att_masks"].cpu() == 0
    assert dead.any() and (d_att.cpu()[dead] == 0).all()


def test_input_feature_gradient_refused_through_batchnorm():
    from unpaired_image_captioning_amd import models
    from unpaired_image_captioning_amd.trainer import xe_step
    cfg = dict(V=50, E=32, H=32, A=32, D=64, L=5, n_img=4, S=1, R=6, use_bn=1)
    model = models.setup(make_opt(cfg, "f32", seed=1)).cuda().train()
    b = O.synthetic_batch(cfg["n_img"], cfg["S"], cfg["R"], cfg["D"], cfg["V"], cfg["L"], seed=2)
    batch = {k: v.cuda() for k, v in b.items()}
    d_fc, d_att = model.engine.input_grad_buffers(batch["fc_feats"], batch["att_feats"])
    with pytest.raises(RuntimeError, match="d_att_feats"):
        xe_step(model, batch, d_fc=d_fc, d_att=d_att)
    torch.cuda.synchronize()
    loss, _ = xe_step(model, batch, d_fc=d_fc)          # the fc branch has no BatchNorm
    assert torch.isfinite(loss) and torch.isfinite(d_fc).all()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("use_bn,S", [(0, 1), (0, 3), (2, 1)])
def test_self_critical_backward_from_kept_forward_equals_replay(dtype, use_bn, S):
    """The train-mode sampling pass keeps its forward in the training layout (uic_topdown_sample_train) and the backward
    starts at the criterion (training bit 2); with model.scst_keep_forward = False the sampled captions are replayed
    teacher-forced (the round-1 path).  Same seed -> the same draws, log-probs and gradients (dropout 0.5, ragged regions,
    per-image features, BatchNorm running statistics updated exactly once)."""
    from unpaired_image_captioning_amd import models
    from unpaired_image_captioning_amd.misc.criterion import RewardCriterion
    cfg = dict(V=300, E=64, H=96, A=64, D=160, L=7, n_img=12, S=S, R=9, use_bn=use_bn)
    b = O.synthetic_batch(cfg["n_img"], 1, cfg["R"], cfg["D"], cfg["V"], cfg["L"], seed=9, ragged_regions=True)
    fc, att, am = b["fc_feats"].cuda(), b["att_feats"].cuda(), b["att_masks"].cuda()
    g = torch.Generator().manual_seed(5)
    reward = torch.randn(cfg["n_img"] * S, cfg["L"], generator=g).cuda()
    res = []
    for keep in (True, False):
        torch.manual_seed(3)
        model = models.setup(make_opt(cfg, dtype, drop=0.5, seed=21)).cuda().train()
        model.scst_keep_forward = keep
        seq, lp = model(fc, None, att, am, opt={"sample_max": 0, "captions_per_image": S}, mode="sample")
        loss = RewardCriterion()(lp, seq, reward)
        loss.backward()
        res.append((seq.cpu(), lp.detach().cpu(), loss.item(), {k: p.grad.float().cpu() for k, p in model.named_parameters()},
                    {k: v.float().cpu().clone() for k, v in model.state_dict().items() if "running" in k}))
        pool = model.engine._pool
        assert sum(len(v) for v in pool.values()) >= 1          # the kept workspace went back to the pool
    (seq0, lp0, l0, g0, s0), (seq1, lp1, l1, g1, s1) = res
    if dtype == "f32":
        assert torch.equal(seq0, seq1)
    same = (seq0 == seq1).all(1)
    assert same.float().mean().item() > 0.9                      # bf16: a near-tie in a draw may fall either way
    assert absmax(lp0[same], lp1[same]) < (2e-5 if dtype == "f32" else 2e-2)
    if bool(same.all()):
        assert abs(l0 - l1) < (1e-5 if dtype == "f32" else 2e-3)
        grads_close(g0, g1, 2e-4 if dtype == "f32" else 3e-2)
    for k in s0:
        assert absmax(s0[k], s1[k]) < 1e-6, k


# ---------------------------------------------------------------- UIC_REC_EARLY_GRADS (the order that finishes most gradient bytes early)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("fixture,ss_prob,drop", [("topdown_tiny", 0.0, 0.0), ("topdown_odd", 0.0, 0.5), ("topdown_tiny_earlybreak", 0.0, 0.0),
                                                  ("topdown_tiny_ss", 0.25, 0.5)])
def test_early_grads_order_gives_the_same_step(fixture, ss_prob, drop, dtype):
    """UIC_REC_EARLY_GRADS: a chunk's weight gradients on two side streams, the embedding gradient gathered in two halves
    (decode steps >= 4 while the BPTT loop still runs, the rest right after it), att_lstm.weight_ih finished before the bias
    sums -- against the default order.  Same loss, same gradients up to f32 summation order -- with dropout, scheduled
    sampling (the bucketed tokens are then the ones the forward pass fed), an early break and decode lengths that are not a
    multiple of the chunk."""
    from unpaired_image_captioning_amd import _lib as L
    cfg, W, I = load_golden(fixture)[:3]
    model = build_model(cfg, W, dtype, drop)
    model.train()
    batch = {k: I[k].cuda() for k in ("fc_feats", "att_feats", "labels", "masks", "att_masks") if k in I}
    runs = {}
    try:
        for name, rec in (("late", 0), ("early", L.REC_EARLY_GRADS), ("early_chain", L.REC_EARLY_GRADS | L.REC_FWD_CHAIN)):
            model.engine.recurrence = rec
            runs[name] = _ss_run(model, batch, ss_prob, 4321)
    finally:
        model.engine.recurrence = 0
    loss0, g0, used0 = runs["late"][:3]
    scale0 = 1e-3 * max(v.abs().max().item() for v in g0.values())
    for name in ("early", "early_chain"):
        loss1, g1, used1 = runs[name][:3]
        assert torch.equal(used0, used1)
        assert abs(loss0.item() - loss1.item()) < 1e-6
        for k in g0:
            a, b = g0[k].double(), g1[k].double()
            scale = max(a.abs().max().item(), scale0)
            assert (a - b).abs().max().item() <= {"f32": 2e-5, "bf16": 2e-2}[dtype] * scale, (name, k, (a - b).abs().max().item(), scale)
    assert any(v.abs().max().item() > 0 for v in g0.values())
