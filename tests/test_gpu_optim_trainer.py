"""--i2t_optim / --nmt_optim and --*_weight_decay through Trainer and Optim on the device: that the flags reach the kernel
(every step mirrored by the matching torch.optim instance on the CPU in float64), a trajectory against the oracle, the clipped
pivot-NMT step, bit-exact resume of methods with other state than Adam's, and the sharded exchange against the all-reduce one.
The kernels themselves: tests/test_gpu_optim_methods.py; the formats: tests/test_optim_methods_host.py."""
import argparse
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

KEYS = ("fc_feats", "att_feats", "labels", "masks", "att_masks")
K = 3                                                   # steps


def _f32(x):
    """The value the C ABI's float argument carries: the mirrors run in float64 on the hyper-parameters the kernel was given."""
    return float(torch.tensor(x, dtype=torch.float32))


LR, ALPHA, BETA, EPS, WD = _f32(5e-3), _f32(0.8), _f32(0.95), _f32(1e-6), _f32(1e-2)


def _torch_optim(method, params, lr, wd, alpha=ALPHA, eps=EPS):
    """The reference's create_optimizer, call for call (P/misc/optimizer.py:59-74)."""
    if method == "rmsprop":
        return torch.optim.RMSprop(params, lr, alpha, eps, weight_decay=wd)
    if method == "adagrad":
        return torch.optim.Adagrad(params, lr, weight_decay=wd)
    if method == "sgd":
        return torch.optim.SGD(params, lr, weight_decay=wd)
    if method == "sgdm":
        return torch.optim.SGD(params, lr, alpha, weight_decay=wd)
    if method == "sgdmom":
        return torch.optim.SGD(params, lr, alpha, weight_decay=wd, nesterov=True)
    return torch.optim.Adam(params, lr, (alpha, BETA), eps, weight_decay=wd)


def _opt(cfg, dtype="f32", path=None, drop=0.0, use_bn=0, **kw):
    return argparse.Namespace(vocab_size=cfg["V"], input_encoding_size=cfg["E"], rnn_size=cfg["H"], num_layers=1, drop_prob_lm=drop,
                              seq_length=cfg["L"], fc_feat_size=cfg["D"], att_feat_size=cfg["D"], att_hid_size=cfg["A"], use_bn=use_bn,
                              logit_layers=1, caption_model="topdown", compute_dtype=dtype, seed=5, i2t_train_flag=1,
                              checkpoint_path=str(path), start_from=str(path), allow_many_hw_queues=1, **kw)


class _Mirror(object):
    """One torch.optim instance in float64 on the CPU over the whole arena; each step starts from the device's own pre-step
    weights and gradient, so only one step's arithmetic (and the state's history) is compared.  check() applies the bound of
    tests/test_gpu_optim_methods.py: |p_dev - p_ref| <= K 2^-24 max |p| + K 2^-20 lr |d|."""

    def __init__(self, method, n, lr, wd):
        self.p = torch.nn.Parameter(torch.zeros(n, dtype=torch.float64))
        self.opt = _torch_optim(method, [self.p], lr, wd)
        self.lr = lr

    def check(self, pre, grad, post, what, defer=None):
        """defer (a list): a missed bound is appended to it instead of raised, so that every step's figures are printed."""
        pre, post = pre.double().cpu(), post.double().cpu()
        self.p.data.copy_(pre)
        self.p.grad = grad.double().cpu()
        self.opt.step()
        ref = self.p.detach()
        d = (pre - ref).abs() / self.lr
        bound = K * 2.0 ** -24 * torch.maximum(pre.abs(), ref.abs()) + K * 2.0 ** -20 * self.lr * d
        err = (post - ref).abs()
        ratio = err / bound.clamp_min(1e-300)
        print("%s: max err %.3e, worst err / bound %.3f, %d of %d elements over the bound, moved %.3e"
              % (what, err.max().item(), ratio.max().item(), int((err > bound).sum()), err.numel(), (post - pre).abs().max().item()))
        assert float((post - pre).abs().max()) > 0, what
        if defer is not None and not bool((err <= bound).all()):
            defer.append((what, err.max().item(), ratio.max().item()))
            return
        assert bool((err <= bound).all()), (what, err.max().item())


@pytest.mark.parametrize("method", ["sgd", "sgdm", "sgdmom", "rmsprop", "adagrad"])
def test_captioner_flags_reach_the_kernel(method):
    """Trainer.train on topdown_tiny (f32) with --i2t_optim, --i2t_weight_decay 1e-2 and non-default optim_alpha / optim_epsilon:
    after every step the device weights against the float64 mirror -- pins that lr, alpha, eps, wd and step arrive."""
    from unpaired_image_captioning_amd.trainer import Trainer
    cfg, W, I, Out, G, X = load_golden("topdown_tiny")
    data = {k: I[k].numpy() for k in KEYS}
    tr = Trainer(_opt(cfg, i2t_optim=method, i2t_weight_decay=WD, i2t_learning_rate=LR, i2t_optim_alpha=ALPHA, i2t_optim_beta=BETA,
                      i2t_optim_epsilon=EPS, i2t_momentum=0.33))
    tr.i2t_model.load_state_dict(W)
    tr.build_optimizer()
    a = tr.arena
    assert a.method == method and len(a.states) == (0 if method == "sgd" else 1)
    mirror = _Mirror(method, a.numel, LR, WD)
    for step in range(1, K + 1):
        pre = a.flat.clone()
        tr.train(data)
        torch.cuda.synchronize()
        mirror.check(pre, a.grad, a.flat, "%s step %d" % (method, step))


def test_unknown_method_is_rejected_when_the_optimizer_is_built():
    from unpaired_image_captioning_amd.trainer import Trainer
    cfg, W, I, Out, G, X = load_golden("topdown_tiny")
    tr = Trainer(_opt(cfg, i2t_optim="adadelta"))
    with pytest.raises(RuntimeError, match="Invalid optim method: adadelta"):
        tr.build_optimizer()


def test_captioner_sgdmom_trajectory_vs_oracle():
    """Three steps of Trainer.train with Nesterov momentum against oracle.topdown.xe_loss_and_grads + torch.optim.SGD on the CPU
    (the criterion of test_nmt_optim_trajectory_vs_reference_golden: per tensor err <= 2e-2 moved + 1e-6).  lr 0.1: the largest
    tensors move by 1e-2 and more in three steps.  Every tensor must have moved but core.attention.alpha_net.bias, whose gradient
    is identically zero (a shift of every attention score leaves the softmax unchanged): without decay SGD leaves it in place."""
    from oracle import topdown as O
    from unpaired_image_captioning_amd.trainer import Trainer
    cfg, W, I, Out, G, X = load_golden("topdown_tiny")
    lr, alpha = 0.1, 0.9
    tr = Trainer(_opt(cfg, i2t_optim="sgdmom", i2t_learning_rate=lr, i2t_optim_alpha=alpha))
    tr.i2t_model.load_state_dict(W)
    data = {k: I[k].numpy() for k in KEYS}
    params = {k: torch.nn.Parameter(v.clone()) for k, v in W.items()}
    opt = torch.optim.SGD(list(params.values()), lr, alpha, weight_decay=0, nesterov=True)
    got, want = [], []
    for _ in range(K):
        got.append(tr.train(data))
        loss, grads, _ = O.xe_loss_and_grads({k: p.detach() for k, p in params.items()}, I["fc_feats"], I["att_feats"], I["labels"], I["masks"],
                                             I.get("att_masks"))
        want.append(float(loss))
        for k, p in params.items():
            p.grad = grads[k].clone()
        opt.step()
    print("sgdmom trajectory: losses %s, oracle %s" % (got, want))
    for a, b in zip(got, want):
        assert abs(a - b) < 1e-4, (got, want)
    sd = tr.i2t_model.state_dict()
    for k, p in params.items():
        moved = (p.detach() - W[k]).norm().item()
        err = (sd[k].cpu() - p.detach()).norm().item()
        assert moved > 0 or k == "core.attention.alpha_net.bias", k
        assert err <= 2e-2 * moved + 1e-6, (k, err, moved)


def test_nmt_rmsprop_clipped_with_weight_decay_through_optim_step():
    """Optim.step on the nmt_tiny fixture: --nmt_optim rmsprop, --nmt_max_grad_norm 5, --nmt_weight_decay 1e-2.  The mirror gets
    the arena's gradient times the clip coefficient max_norm / (norm + 1e-6) (when < 1) computed in float64, then adds the decay
    itself: the decay is not clipped.

    Measured on an MI355X: 0.292 / 0.312 / 0.325 of the bound in the three steps (clip coefficients 0.859, 0.847, 0.689).  What
    it takes: in this model's first step ten elements have clip g and wd p cancel to 3e-5 of their size (g' of 6e-8 from terms of
    2e-3), next to eps / sqrt(1 - alpha) where RMSprop's first direction changes by 1 / eps per unit of g' -- so the kernel forms
    the coefficient in double from the norm as a float pair (uic_grad_sqnorm_f64) and rounds clip g + wd p once.  With the norm
    as one float (8e-9 off) the worst element stood at 1.095 of the bound, with a float coefficient at 3.712."""
    from test_gpu_nmt import build, load, run
    from unpaired_image_captioning_amd.misc.optimizer import Optim
    cfg, W, I, Out, G = load("nmt_tiny")
    model, crit = build(cfg, W, "f32")
    o = model.opt
    o.nmt_train_flag, o.i2t_train_flag = 1, 0
    o.nmt_optim, o.nmt_learning_rate, o.nmt_max_grad_norm, o.nmt_weight_decay = "rmsprop", LR, 5, WD
    o.nmt_optim_alpha, o.nmt_optim_beta, o.nmt_optim_epsilon, o.nmt_momentum = ALPHA, BETA, EPS, 0.33
    optim = Optim(o)
    optim.set_parameters(None, model)
    model.train()
    a = optim.nmt_arena
    assert a.method == "rmsprop" and [t.shape for t in a.states] == [a.flat.shape]
    mirror = _Mirror("rmsprop", a.numel, LR, WD)
    coefs, missed = [], []
    for step in range(1, K + 1):
        optim.zero_grad()
        outputs, attn, loss = run(model, crit, I)
        loss.backward()
        pre = a.flat.clone()
        optim.step()
        torch.cuda.synchronize()
        g = a.grad.double().cpu()
        coef = 5.0 / (float(g.pow(2).sum().sqrt()) + 1e-6)
        coefs.append(coef)
        mirror.check(pre, g * min(coef, 1.0), a.flat, "nmt rmsprop step %d (clip coefficient %.4f)" % (step, coef), defer=missed)
    assert not missed, missed
    assert min(coefs) < 1.0, coefs                      # (the clip was active: the summed loss of nmt_tiny has a gradient norm above 5)


def _snapshot(tr):
    torch.cuda.synchronize()
    snap = {"sd::" + k: v.detach().cpu().clone() for k, v in tr.i2t_model.state_dict().items()}
    for name, t in zip(tr.arena.state_names, tr.arena.states):
        snap[name] = t.cpu().clone()
    return snap


@pytest.mark.parametrize("method", ["sgdmom", "adagrad"])
def test_resume_is_bit_exact_for_other_state_than_adams(tmp_path, method):
    """2 steps + save + fresh Trainer + load + 2 steps against 4 steps straight (dropout 0.5, BatchNorm, two alternating batches,
    weight decay): losses, every state_dict tensor, the method's state arena, counters and learning rate."""
    from unpaired_image_captioning_amd.trainer import Trainer
    data = []
    for name in ("topdown_tiny", "topdown_tiny_ragged"):
        cfg, W, I, Out, G, X = load_golden(name)
        data.append({k: I[k].numpy() for k in KEYS})
    opt = _opt(cfg, path=tmp_path, drop=0.5, use_bn=1, i2t_optim=method, i2t_weight_decay=WD, i2t_learning_rate=5e-2)

    def new(seed):
        torch.manual_seed(seed)
        return Trainer(opt)
    straight = new(1)
    ref_losses = [straight.train(data[i % 2]) for i in range(4)]
    first = new(1)
    losses = [first.train(data[i % 2]) for i in range(2)]
    first.save_models("-best")
    sd = torch.load(os.path.join(str(tmp_path), "optimizer_i2t-best.pth"), weights_only=True)
    state_name = first.arena.state_names[0]
    assert all(state_name in st and ("step" in st) == (method == "adagrad") for st in sd["state"].values()) and len(sd["state"]) > 0
    assert sd["param_groups"][0]["weight_decay"] == WD and sd["param_groups"][0].get("nesterov", False) == (method == "sgdmom")
    assert torch.load(os.path.join(str(tmp_path), "trainer_state-best.pth"), weights_only=True)["i2t_optim"] == method
    resumed = new(99)
    resumed.load_models()
    assert resumed._step == 2 and resumed.arena.method == method
    losses += [resumed.train(data[i % 2]) for i in range(2, 4)]
    print("losses", ref_losses, losses)
    assert losses == ref_losses
    a, b = _snapshot(resumed), _snapshot(straight)
    assert set(a) == set(b) and state_name in a
    for k in a:
        assert torch.equal(a[k], b[k]), (k, (a[k].double() - b[k].double()).abs().max().item())
    assert float(b[state_name].abs().max()) > 0
    assert (resumed._step, resumed.i2t_model._seed_counter, resumed.i2t_current_lr) == (straight._step, straight.i2t_model._seed_counter,
                                                                                      straight.i2t_current_lr)


# ---------------------------------------------------------------- two ranks on one GPU (gloo): sharded exchange against all-reduce
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir, dtype):
    """Both exchanges one after the other in the same two processes: the sharded one (reduce-scatter, the step on the rank's
    ranges, all-gather) must leave the bits of the all-reduce one (the step on the whole arena on every rank)."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)                                   # gloo: both ranks share cuda:0
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from unpaired_image_captioning_amd.parallel_exchange import GradientExchange
    from unpaired_image_captioning_amd.trainer import Trainer
    cfg, W, I, Out, G, X = load_golden("topdown_tiny_ragged")
    lo, hi = GradientExchange().shard_images(cfg["n_img"])
    rows = slice(lo * cfg["S"], hi * cfg["S"])
    data = {k: I[k][rows].numpy() for k in KEYS}
    res = {}
    for tag, allreduce in (("sharded", 0), ("allreduce", 1)):
        tr = Trainer(_opt(cfg, dtype, i2t_optim="rmsprop", i2t_weight_decay=WD, i2t_learning_rate=LR, i2t_optim_alpha=ALPHA,
                          i2t_optim_epsilon=EPS, early_grads=False, allreduce_exchange=allreduce, bf16_gradient_exchange=0))
        tr.i2t_model.load_state_dict(W)
        tr.build_optimizer()
        assert tr.sharded == (not allreduce) and tr.arena.method == "rmsprop" and tr.exchange.world_size == world
        losses = [tr.train(data) for _ in range(K)]
        tr.gather_masters()
        if tr.sharded:
            tr.arena.gather_moments(tr.exchange)
        torch.cuda.synchronize()
        o = tr.arena.offsets
        res[tag] = (losses, {k: v.detach().cpu().clone() for k, v in tr.i2t_model.state_dict().items()},
                    {k: tr.arena.square_avg[o[k]:o[k] + tr.arena.params[k].numel()].cpu().clone() for k in o})
        dist.barrier()
    (ls, ws, ss), (la, wa, sa) = res["sharded"], res["allreduce"]
    assert ls == la, (ls, la)
    for k in wa:
        assert torch.equal(ws[k], wa[k]), (k, (ws[k].float() - wa[k].float()).abs().max().item())
        assert not torch.equal(wa[k].float(), W[k]), k
    for k in sa:                                                # (the arenas' layouts differ: compared per parameter)
        assert torch.equal(ss[k], sa[k]) and float(sa[k].abs().max()) > 0, k
    if rank == 0:
        torch.save({"losses": ls}, os.path.join(out_dir, "done.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_sharded_rmsprop_with_weight_decay_leaves_the_bits_of_the_all_reduce(tmp_path, dtype):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), dtype), nprocs=2, join=True)
    assert len(torch.load(os.path.join(str(tmp_path), "done.pt"))["losses"]) == K
