"""The FC captioner (caption_model='fc') through the Trainer on the GPU: the fused XE step, the train-mode sampling pass and its
backward from RewardCriterion, Trainer.train / train_self_critical / eval, checkpoints and two data-parallel ranks -- against the
reference's goldens, oracle/fc.py and the restatements of tests/fc_train_cases.py.  Tolerances: tests/test_gpu_topdown.py's."""
import ctypes as C
import datetime
import os
import sys
import time

import numpy as np
import pytest
import torch

import fc_train_cases as FT
from conftest import ROOT, load_golden
from oracle import fc as OF
from oracle import topdown as O
from test_gpu_fc import build
from test_gpu_topdown import GRAD_TOL, LOGP_TOL, absmax, grads_close

pytestmark = pytest.mark.gpu
TINY = ["fc_tiny", "fc_tiny_earlybreak", "fc_odd"]


@pytest.fixture(autouse=True)
def _poisoned_fc_workspaces(monkeypatch):
    """Every workspace an FC engine hands out is filled with 0xFF bytes first (NaN in f32 and bf16, -1 in the integer buffers):
    no result may depend on what a pooled buffer still held."""
    from unpaired_image_captioning_amd.models.FCModel_NMT import _FcEngine
    orig = _FcEngine.workspace

    def workspace(self, d, device):
        ws = orig(self, d, device)
        ws.fill_(255)
        return ws

    monkeypatch.setattr(_FcEngine, "workspace", workspace)
    yield


def lcg(c):
    """FCModel_NMT.next_seed."""
    return (c * 1103515245 + 12345) & 0x7FFFFFFF


def device_masks(seed, N, H, steps, p, total=None):
    """{'out': [total, N, H]} -- the dropout masks the kernels apply at core steps 0 .. steps-1 (ones behind them), or None."""
    from unpaired_image_captioning_amd import _lib as L
    if not p:
        return None
    lib = L.load()
    out = []
    for t in range(steps):
        m = torch.empty(N * H, device="cuda")
        L.check(lib.uic_dropout_mask(L.ptr(m), N * H, p, seed, L.SITE_OUT0 + t, 0, L.stream()))
        out.append(m.cpu().view(N, H))
    out += [torch.ones(N, H)] * ((total or steps) - steps)
    return {"out": torch.stack(out)}


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def cfg1_case():
    cfg, W, I, Out, G, X = load_golden("fc_cfg1")
    wseed, dseed = [int(s) for s in torch.as_tensor(X["seeds"])]
    Wt = OF.init_weights(cfg["V"] + 1, cfg["E"], cfg["H"], cfg["D"], seed=wseed)
    b = O.synthetic_batch(cfg["n_img"], cfg["S"], 3, cfg["D"], cfg["V"], cfg["L"], seed=dseed)
    return cfg, Wt, b, Out, G, X


def fused_step(model, fc, labels, masks, seed, training=True):
    """engine.xe_train_step as trainer.xe_step calls it -> (out [loss, mask sum], grads)."""
    eng = model.engine
    pd = {k: v.detach() for k, v in model.param_dict().items()}
    grads = {k: torch.full_like(v, float("nan")) for k, v in pd.items()}
    out = eng.xe_train_step(pd, fc, None, None, labels, masks, eng.token_steps(labels), training, seed, grads)
    return out, grads


def three_calls(model, fc, labels, masks, seed, training=True):
    """uic_fc_forward(logprobs_out = NULL) + uic_fc_xe_loss + uic_fc_backward(dlogprobs = NULL) on one poisoned workspace."""
    from unpaired_image_captioning_amd._lib import check, ptr, stream
    eng = model.engine
    pd = {k: v.detach() for k, v in model.param_dict().items()}
    grads = {k: torch.full_like(v, float("nan")) for k, v in pd.items()}
    d = eng.dims(fc.shape[0], labels.shape[1])
    ws = eng.workspace(d, fc.device)
    w, g, b = eng.weights(pd), eng.weights(grads), eng.batch(fc, labels, masks)
    s_run = model._steps_to_run(labels)
    loss = torch.empty(1, device=fc.device)
    check(eng.lib.uic_fc_forward(C.byref(d), C.byref(w), C.byref(b), s_run, int(training), seed, ptr(ws), None, stream()), "forward")
    check(eng.lib.uic_fc_xe_loss(C.byref(d), C.byref(b), s_run, ptr(ws), None, ptr(loss), stream()), "xe_loss")
    check(eng.lib.uic_fc_backward(C.byref(d), C.byref(w), C.byref(b), s_run, int(training), seed, ptr(ws), None, None, C.byref(g), stream()), "backward")
    eng.release(d, ws)
    return loss, grads


# ------------------------------------------------------------------------------------------------ 1. the fused XE step
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", TINY)
def test_fused_step_equals_the_three_calls_bit_for_bit_and_the_oracle(name, dtype):
    cfg, W, I, Out, G, X = load_golden(name)
    model = build(cfg, W, dtype, drop=0.5).train()
    fc, labels, masks = I["fc_feats"].cuda(), I["labels"].cuda(), I["masks"].cuda()
    seed = 12345
    out, grads = fused_step(model, fc, labels, masks, seed)
    loss3, grads3 = three_calls(model, fc, labels, masks, seed)
    assert torch.equal(bits(out[0:1]), bits(loss3))
    assert out[1].item() == float(I["masks"][:, 1:].sum())
    for k in grads:
        assert torch.equal(bits(grads[k]), bits(grads3[k])), k
    out2, grads2 = fused_step(model, fc, labels, masks, seed)          # no atomics: the same bits again
    assert torch.equal(bits(out), bits(out2)) and all(torch.equal(bits(grads[k]), bits(grads2[k])) for k in grads)
    drop = device_masks(seed, fc.shape[0], cfg["H"], labels.shape[1], 0.5)
    loss_o, grads_o, _ = OF.xe_loss_and_grads(W, I["fc_feats"], I["labels"], I["masks"], drop)
    print("loss", out[0].item(), "oracle", loss_o.item())
    assert abs(out[0].item() - loss_o.item()) < LOGP_TOL[dtype]
    grads_close(grads, grads_o, GRAD_TOL[dtype])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_fused_step_at_config1_vs_reference_golden(dtype):
    cfg, Wt, b, Out, G, X = cfg1_case()
    model = build(cfg, Wt, dtype).train()
    out, grads = fused_step(model, b["fc_feats"].cuda(), b["labels"].cuda(), b["masks"].cuda(), 7)
    print("loss", out[0].item(), "golden", float(Out["loss"]))
    assert abs(out[0].item() - float(Out["loss"])) < LOGP_TOL[dtype]
    grads_close(grads, G, GRAD_TOL[dtype])
    for k, v in X.items():
        if k.startswith("gradnorm::"):
            n = grads[k.split("::", 1)[1]].double().norm().item()
            assert abs(n - float(torch.as_tensor(v))) <= GRAD_TOL[dtype] * float(torch.as_tensor(v)), k


# ------------------------------------------------------------------------------------------------ 2. Trainer.train
def fc_trainer(cfg, W, dtype="f32", drop=0.0, seed=0, **kw):
    from unpaired_image_captioning_amd.trainer import Trainer
    tr = Trainer(FT.make_opt(cfg, dtype, drop, seed, **kw))
    tr.i2t_model.load_state_dict(W)
    tr.build_optimizer()
    return tr


def host_batch(I):
    return {k: I[k].numpy() for k in ("fc_feats", "labels", "masks")}


def test_trainer_train_golden_loss_and_adam_first_step():
    cfg, W, I, Out, G, X = load_golden("fc_tiny")
    lr = 5e-3
    tr = fc_trainer(cfg, W, i2t_learning_rate=lr)
    loss = tr.train(host_batch(I))
    print("loss", loss, "golden", float(Out["loss"]))
    assert abs(loss - float(Out["loss"])) < LOGP_TOL["f32"]
    # Adam's first step from zero state is -lr g / (|g| + eps) = -lr sign(g) wherever |g| >> eps = 1e-8
    big = 1e-2 * max(float(g.abs().max()) for g in G.values())
    sd = tr.i2t_model.state_dict()
    checked = 0
    for k, g in G.items():
        sel = g.abs() >= big
        step = (sd[k].cpu() - W[k])[sel]
        want = -lr * torch.sign(g[sel])
        # (the stored weight is rounded to f32: half an ulp of a weight below 1 is 3e-8, 6e-6 of the step)
        assert ((step - want).abs() <= 1e-3 * lr).all(), (k, (step - want).abs().max().item())
        checked += int(sel.sum())
        # Five of the nine tensors have no entry that large (img_embed.weight's largest is 1.4e-3 of logit.bias's).  So that EVERY
        # tensor is seen to move by its own gradient: its entries of at least 1e-2 of its own largest and 1e-6 in absolute value
        # (where eps / |g| <= 1e-2, and the device gradient's error -- GRAD_TOL of the tensor's largest -- cannot turn the sign)
        own = (g.abs() >= 1e-2 * g.abs().max()) & (g.abs() >= 1e-6)
        assert int(own.sum()) > 0, k
        step = (sd[k].cpu() - W[k])[own]
        assert ((step + lr * torch.sign(g[own])).abs() <= 2e-2 * lr).all(), k
    assert checked > 100


def initial_flat(tr, W):
    """The initial weights W laid out like the trainer's arena (up to its scalar slots)."""
    a = tr.arena
    flat = torch.zeros(a.scalars_off, device=a.flat.device)
    for k, off in a.offsets.items():
        flat[off:off + W[k].numel()] = W[k].reshape(-1).to(flat.device)
    return flat


def test_trainer_train_is_reproducible_and_learns():
    cfg, W, I, Out, G, X = load_golden("fc_odd")
    data = host_batch(I)
    runs = []
    for _ in range(2):
        tr = fc_trainer(cfg, W, drop=0.5, seed=3, i2t_learning_rate=5e-3)
        losses = [tr.train(data) for _ in range(3)]
        torch.cuda.synchronize()
        runs.append((losses, tr.arena.flat.clone(), tr))
    assert runs[0][0] == runs[1][0]
    assert torch.equal(bits(runs[0][1]), bits(runs[1][1]))
    assert not torch.equal(runs[0][1][:tr.arena.scalars_off], initial_flat(runs[0][2], W))        # (and the weights did move)
    tr = fc_trainer(cfg, W, i2t_learning_rate=5e-3)
    losses = [tr.train(data) for _ in range(30)]
    print("first", losses[0], "last", losses[-1])
    assert losses[-1] < losses[0]


# ------------------------------------------------------------------------------------------------ 3. the train-mode sampling pass
def forced_cases(N, L, V):
    return {"mixed": FT.forced_streams(N, L, V, 3), "all_ended": FT.all_ended_streams(N, L, V, 4, end=L // 2)}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["fc_tiny", "fc_odd"])
def test_sampling_pass_with_forced_tokens_vs_oracle_under_the_device_masks(name, dtype):
    cfg, W, I, Out, G, X = load_golden(name)
    model = build(cfg, W, dtype, drop=0.5).train()
    fc, L = I["fc_feats"].cuda(), cfg["L"]
    N = fc.shape[0]
    for tag, forced in forced_cases(N, L, cfg["V"]).items():
        seq, lp = model(fc, None, None, opt={"sample_max": 0, "forced_tokens": forced.cuda()}, mode="sample")
        seed = model._seed_counter
        assert lp.requires_grad and not seq.requires_grad and tuple(seq.shape) == (N, L + 1)
        assert torch.equal(seq.cpu(), FT.masked_stream(forced)), tag
        drop = device_masks(seed, N, cfg["H"], L + 1, 0.5, total=L + 2)
        lp_o = FT.sampled_logprobs(W, I["fc_feats"], seq.cpu(), drop, fed=forced)
        print(tag, "max |lp - oracle|", absmax(lp, lp_o))
        assert absmax(lp, lp_o) < LOGP_TOL[dtype], tag
        if tag == "all_ended":
            assert float(lp.detach()[:, L // 2:].abs().max()) == 0.0         # nothing written from the break on
    # without dropout the pass agrees with oracle/fc.py's own sampling loop
    model0 = build(cfg, W, dtype, drop=0.0).train()
    forced = forced_cases(N, L, cfg["V"])["mixed"]
    seq, lp = model0(fc, None, None, opt={"sample_max": 0, "forced_tokens": forced.cuda()}, mode="sample")
    seq_o, lp_o = OF.sample(W, I["fc_feats"], L, sample_max=0, forced_tokens=forced)
    assert torch.equal(seq.cpu(), seq_o) and absmax(lp, lp_o) < LOGP_TOL[dtype]


def test_sampling_pass_free_draws_rescored_by_the_oracle():
    cfg, W, I, Out, G, X = load_golden("fc_tiny")
    model = build(cfg, W, "f32", drop=0.5).train()
    fc, L = I["fc_feats"].cuda(), cfg["L"]
    N = fc.shape[0]
    seq, lp = model(fc, None, None, opt={"sample_max": 0}, mode="sample")
    seed = model._seed_counter
    seq_c = seq.cpu()
    assert int(seq_c.max()) <= cfg["V"] and int(seq_c.min()) >= 0 and int((seq_c > 0).sum()) > 0
    drop = device_masks(seed, N, cfg["H"], L + 1, 0.5, total=L + 2)
    lp_o = FT.sampled_logprobs(W, I["fc_feats"], seq_c, drop)
    # up to and including a row's first 0 the stored tokens are the tokens fed (behind it the raw draws are not kept)
    live = torch.cat([torch.ones(N, 1), (seq_c[:, :-1] > 0).float().cumprod(1)], 1)
    assert float(((lp.detach().cpu() - lp_o).abs() * live).max()) < LOGP_TOL["f32"]
    seq2, _ = model(fc, None, None, opt={"sample_max": 0}, mode="sample")
    assert not torch.equal(seq2, seq)                                 # a fresh seed per pass


@pytest.mark.parametrize("sample_max", [1, 0])
def test_eval_and_no_grad_sampling_keep_the_existing_path(sample_max):
    from unpaired_image_captioning_amd._lib import check, ptr, stream
    cfg, W, I, Out, G, X = load_golden("fc_odd")
    model = build(cfg, W, "f32", drop=0.5)
    fc, L = I["fc_feats"].cuda(), cfg["L"]
    N = fc.shape[0]
    eng = model.engine

    def direct(seed):
        d = eng.dims(N, L + 2)
        ws = eng.workspace(d, fc.device)
        seq = torch.zeros(N, L + 1, dtype=torch.int64, device="cuda")
        lp = torch.zeros(N, L + 1, device="cuda")
        w, b = eng.weights({k: v.detach() for k, v in model.param_dict().items()}), eng.batch(fc)
        check(eng.lib.uic_fc_sample(C.byref(d), C.byref(w), C.byref(b), L, sample_max, 1.0, seed, None, ptr(ws), ptr(seq), ptr(lp), stream()), "fc_sample")
        eng.release(d, ws)
        return seq, lp

    for mode, ctx in (("eval", torch.enable_grad()), ("train", torch.no_grad())):
        model.train(mode == "train")
        with ctx:
            seq, lp = model(fc, None, None, opt={"sample_max": sample_max}, mode="sample")
        assert not lp.requires_grad
        seq_d, lp_d = direct(model._seed_counter)
        assert torch.equal(seq, seq_d) and torch.equal(bits(lp), bits(lp_d)), mode


# ------------------------------------------------------------------------------------------------ 4. the SCST gradient
def scst_device(model, fc, forced, reward):
    from unpaired_image_captioning_amd.misc.criterion import RewardCriterion
    for p in model.parameters():
        p.grad = None
    seq, lp = model(fc, None, None, opt={"sample_max": 0, "forced_tokens": forced.cuda()}, mode="sample")
    seed = model._seed_counter
    loss = RewardCriterion()(lp, seq, reward.cuda())
    loss.backward()
    return loss, seq, seed, {k: p.grad.clone() for k, p in model.named_parameters()}


def mixed_reward(N, L1, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, L1, generator=g)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["fc_tiny", "fc_odd"])
def test_scst_gradient_vs_autograd_on_the_restatement(name, dtype):
    cfg, W, I, Out, G, X = load_golden(name)
    model = build(cfg, W, dtype, drop=0.5).train()
    fc, L = I["fc_feats"].cuda(), cfg["L"]
    N = fc.shape[0]
    reward = mixed_reward(N, L + 1, 5)
    for tag, forced in forced_cases(N, L, cfg["V"]).items():
        loss, seq, seed, grads = scst_device(model, fc, forced, reward)
        drop = device_masks(seed, N, cfg["H"], L + 1, 0.5, total=L + 2)
        loss_o, grads_o, _ = FT.scst_loss_and_grads(W, I["fc_feats"], seq.cpu(), reward, drop)
        print(tag, "loss", loss.item(), "restatement", loss_o.item())
        assert abs(loss.item() - loss_o.item()) < LOGP_TOL[dtype], tag
        grads_close(grads, grads_o, GRAD_TOL[dtype])


def test_scst_gradient_at_config1_f32():
    cfg, Wt, b, Out, G, X = cfg1_case()
    model = build(cfg, Wt, "f32", drop=0.5).train()
    fc, L = b["fc_feats"].cuda(), cfg["L"]
    N = fc.shape[0]
    forced = FT.forced_streams(N, L, cfg["V"], 8)
    reward = mixed_reward(N, L + 1, 6)
    loss, seq, seed, grads = scst_device(model, fc, forced, reward)
    drop = device_masks(seed, N, cfg["H"], L + 1, 0.5, total=L + 2)
    loss_o, grads_o, _ = FT.scst_loss_and_grads(Wt, b["fc_feats"], seq.cpu(), reward, drop)
    print("loss", loss.item(), "restatement", loss_o.item())
    assert abs(loss.item() - loss_o.item()) < LOGP_TOL["f32"]
    grads_close(grads, grads_o, GRAD_TOL["f32"])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_rows_behind_their_end_contribute_exact_zeros(dtype):
    cfg, W, I, Out, G, X = load_golden("fc_tiny")
    model = build(cfg, W, dtype, drop=0.5).train()
    fc, L, V = I["fc_feats"].cuda(), cfg["L"], cfg["V"]
    N = fc.shape[0]
    reward = mixed_reward(N, L + 1, 5)
    forced = FT.forced_streams(N, L, V, 3)
    other = forced.clone()
    behind = (forced > 0).long().cumprod(1) == 0                      # the first 0 of a row and everything behind it
    first0 = behind & (torch.cat([torch.ones(N, 1, dtype=torch.bool), ~behind[:, :-1]], 1))
    change = behind & ~first0
    assert int(change.sum()) > 3
    other[change] = (forced[change] + 7) % V + 1
    c0 = model._seed_counter
    loss_a, seq_a, _, grads_a = scst_device(model, fc, forced, reward)
    model._seed_counter = c0                                           # the same dropout masks
    loss_b, seq_b, _, grads_b = scst_device(model, fc, other, reward)
    assert torch.equal(seq_a, seq_b) and torch.equal(bits(loss_a), bits(loss_b))
    for k in grads_a:
        assert torch.equal(grads_a[k], grads_b[k]), k
        assert torch.isfinite(grads_a[k]).all(), k


def test_second_backward_over_one_sampling_pass_raises():
    from unpaired_image_captioning_amd.misc.criterion import RewardCriterion
    cfg, W, I, Out, G, X = load_golden("fc_tiny")
    model = build(cfg, W, "f32").train()
    fc = I["fc_feats"].cuda()
    seq, lp = model(fc, None, None, opt={"sample_max": 0}, mode="sample")
    loss = RewardCriterion()(lp, seq, torch.ones_like(lp))
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second backward"):
        loss.backward()
    # a pass whose graph is dropped without a backward hands its workspace back to the pool
    eng = model.engine
    seq, lp = model(fc, None, None, opt={"sample_max": 0}, mode="sample")
    key = (fc.shape[0], cfg["L"] + 2, eng.dtype)
    held = len(eng._pool.get(key, []))
    del seq, lp
    assert len(eng._pool[key]) == held + 1


# ------------------------------------------------------------------------------------------------ 5. Trainer.train_self_critical
def scst_data(cfg, I):
    data = host_batch(I)
    n_img = len(data["labels"]) // cfg["S"]
    data["gts"] = [data["labels"][i * cfg["S"]:(i + 1) * cfg["S"], 1:cfg["L"] + 1] for i in range(n_img)]
    return data


@pytest.mark.parametrize("scorer", ["host_reward_fn", "device_ciderd"])
def test_trainer_self_critical_runs_and_is_reproducible(scorer):
    from unpaired_image_captioning_amd.misc import rewards
    cfg, W, I, Out, G, X = load_golden("fc_tiny")
    data = scst_data(cfg, I)

    def reward_fn(data, sampled, greedy):
        r = np.where(sampled[:, :1] % 2 == 0, 1.0, -1.0)
        return np.repeat(r, sampled.shape[1], 1)

    runs = []
    for _ in range(2):
        rewards.CiderD_scorer = None
        tr = fc_trainer(cfg, W, drop=0.5, seed=9, i2t_learning_rate=1e-3, cached_tokens="corpus", cider_reward_weight=1.0, bleu_reward_weight=0.0)
        before = tr.arena.flat.clone()
        losses = [tr.train_self_critical(data, reward_fn if scorer == "host_reward_fn" else None) for _ in range(2)]
        assert all(np.isfinite(l) for l in losses) and np.isfinite(tr.i2t_avg_reward)
        torch.cuda.synchronize()
        assert not torch.equal(before, tr.arena.flat)
        runs.append((losses, tr.i2t_avg_reward, tr.arena.flat.clone()))
    rewards.CiderD_scorer = None
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    assert torch.equal(bits(runs[0][2]), bits(runs[1][2]))


def test_trainer_self_critical_loss_with_forced_samples_equals_the_restatement():
    cfg, W, I, Out, G, X = load_golden("fc_odd")
    data = scst_data(cfg, I)
    N, L = len(data["labels"]), cfg["L"]
    forced = FT.forced_streams(N, L, cfg["V"], 3)
    reward = mixed_reward(N, L + 1, 5)
    tr = fc_trainer(cfg, W, drop=0.5, seed=4, i2t_learning_rate=1e-3)
    tr.forced_samples = forced.cuda()
    seed = lcg(tr.i2t_model._seed_counter)                             # the sampling pass draws the step's first seed
    loss = tr.train_self_critical(data, lambda data, sampled, greedy: reward.numpy())
    drop = device_masks(seed, N, cfg["H"], L + 1, 0.5, total=L + 2)
    loss_o, grads_o, _ = FT.scst_loss_and_grads(W, I["fc_feats"], FT.masked_stream(forced), reward, drop)
    print("loss", loss, "restatement", loss_o.item())
    assert abs(loss - loss_o.item()) < LOGP_TOL["f32"]
    grads_close({k: v for k, v in tr.arena.grad_views.items()}, grads_o, GRAD_TOL["f32"])


# ------------------------------------------------------------------------------------------------ 6. Trainer.eval
def test_trainer_eval_on_the_synthetic_loader(tmp_path):
    import argparse
    import lang_eval_cases as LC
    from dataset_files import loader_opt, write_dataset
    from unpaired_image_captioning_amd.misc.dataloader.dataloader import DataLoader
    from unpaired_image_captioning_amd.trainer import Trainer
    V, L, D, n = 20, 6, 16, 11
    g = np.random.default_rng(3)
    ids = [100 + 3 * i for i in range(n)]
    splits = ["val" if i in (0, 1, 3, 4, 6, 7, 9) else "train" for i in range(n)]
    att = [g.standard_normal((int(g.integers(2, 6)), D)).astype(np.float32) for _ in range(n)]
    fc = [g.standard_normal(D).astype(np.float32) for _ in range(n)]
    counts = [int(g.integers(2, 5)) for _ in range(n)]
    end = np.cumsum(counts)
    start = end - np.array(counts) + 1
    labels = LC.caption_rows(g, int(end[-1]), L, V, min_words=1)
    label_path = write_dataset(str(tmp_path), att, None, fc, [(10, 10)] * n, ids, labels, start, end, V, splits=splits)
    lo = loader_opt(str(tmp_path), label_path, 3, 2, D, D, 0, 0, 0)
    opt = argparse.Namespace(vocab_size=V, input_encoding_size=32, rnn_type="LSTM", rnn_size=32, num_layers=1, drop_prob_lm=0.5, seq_length=L,
                             caption_model="fc", compute_dtype="f32", seed=2, i2t_train_flag=0, i2t_eval_flag=1,
                             language_eval=1, beam_size=1, verbose=False, **vars(lo))
    torch.manual_seed(4)
    tr = Trainer(opt)
    tr.i2t_model.cuda()
    loader = DataLoader(opt)
    tr.eval(loader)
    assert not tr.i2t_model.training
    assert tr.i2t_val_loss == tr.i2t_val_loss and 0 < tr.i2t_val_loss < 1e3
    got = [p["image_id"] for p in tr.predictions]
    assert sorted(got) == sorted(ids[i] for i in range(n) if splits[i] == "val") and len(set(got)) == 7
    assert set(LC.KEYS) <= set(tr.lang_stats) and all(v == v for v in tr.lang_stats.values())


# ------------------------------------------------------------------------------------------------ 7. checkpoints
def test_checkpoint_continues_bit_exactly(tmp_path):
    cfg, W, I, Out, G, X = load_golden("fc_tiny")
    data = scst_data(cfg, I)

    def reward_fn(data, sampled, greedy):
        r = np.where(sampled[:, :1] % 2 == 0, 1.0, -0.5)
        return np.repeat(r, sampled.shape[1], 1)

    def first_part(tr):
        for _ in range(3):
            tr.train(data)
        tr.train_self_critical(data, reward_fn)

    def second_part(tr):
        return tr.train(data), tr.train_self_critical(data, reward_fn)

    kw = dict(drop=0.5, seed=6, i2t_learning_rate=2e-3, checkpoint_path=str(tmp_path))
    whole = fc_trainer(cfg, W, **kw)
    first_part(whole)
    want = second_part(whole)
    stopped = fc_trainer(cfg, W, **kw)
    first_part(stopped)
    stopped.save_models("-t")
    resumed = fc_trainer(cfg, {k: torch.zeros_like(v) for k, v in W.items()}, **kw)
    resumed.load_models(str(tmp_path), "-t")
    assert resumed._step == 4 and resumed.i2t_model._seed_counter == stopped.i2t_model._seed_counter
    got = second_part(resumed)
    torch.cuda.synchronize()
    assert got == want
    assert torch.equal(bits(resumed.arena.flat[:resumed.arena.scalars_off]), bits(whole.arena.flat[:whole.arena.scalars_off]))
    assert len(whole.arena.states) == 2
    for a, b in zip(resumed.arena.states, whole.arena.states):
        assert torch.equal(bits(a[:resumed.arena.scalars_off]), bits(b[:whole.arena.scalars_off]))


# ------------------------------------------------------------------------------------------------ 8. two ranks on one GPU
STEP_LIMIT = 120          # seconds for the children's collectives and for the whole spawn


def _dp_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)                                           # gloo: both ranks share cuda:0
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=STEP_LIMIT))
    from unpaired_image_captioning_amd.parallel_exchange import GradientExchange
    from unpaired_image_captioning_amd.trainer import Trainer
    cfg, W, I, Out, G, X = load_golden("fc_tiny")
    lo, hi = GradientExchange().shard_images(cfg["n_img"])
    rows = slice(lo * cfg["S"], hi * cfg["S"])
    tr = Trainer(FT.make_opt(cfg, "f32", 0.0, 5, i2t_learning_rate=5e-3, allow_many_hw_queues=1))
    tr.i2t_model.load_state_dict(W)
    tr.build_optimizer()
    assert tr.exchange.world_size == world and not tr.sharded          # the all-reduce exchange (no sharded one for this model)
    loss = tr.train({k: I[k][rows].numpy() for k in ("fc_feats", "labels", "masks")})
    torch.cuda.synchronize()
    torch.save({"sd": {k: v.cpu() for k, v in tr.i2t_model.state_dict().items()}, "loss": loss}, os.path.join(out_dir, "fc_dp%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu_xe_step(tmp_path):
    import torch.multiprocessing as mp
    from test_gpu_dp2 import _free_port
    ctx = mp.spawn(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=False)
    deadline = time.monotonic() + STEP_LIMIT
    while not ctx.join(timeout=5):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the two ranks did not finish within %d s" % STEP_LIMIT)
    r0, r1 = (torch.load(os.path.join(str(tmp_path), "fc_dp%d.pt" % r)) for r in range(2))
    for k, v in r0["sd"].items():
        assert torch.equal(v, r1["sd"][k]), k
    cfg, W, I, Out, G, X = load_golden("fc_tiny")
    single = fc_trainer(cfg, W, seed=5, i2t_learning_rate=5e-3)
    loss = single.train(host_batch(I))
    print("ranks", r0["loss"], r1["loss"], "single", loss)
    assert r0["loss"] == r1["loss"]                                    # (already summed over the ranks)
    assert abs(r0["loss"] - loss) < LOGP_TOL["f32"]
    assert any(not torch.equal(v, W[k]) for k, v in r0["sd"].items())
