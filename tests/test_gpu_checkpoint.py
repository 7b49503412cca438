"""Checkpoint and resume on the device: a run that is saved (Trainer.save_models), thrown away and continued by a FRESH Trainer
(own random initialisation, then Trainer.load_models) must be BIT-identical to the run that never stopped -- losses, every
state_dict tensor (BatchNorm running statistics included), both Adam moments, the step counters, the learning rates and the seed
counter behind every dropout mask, multinomial draw and scheduled-sampling decision.  The step is bit-reproducible
(test_training_step_is_bit_reproducible), so nothing weaker than equality is asked for.  Host-side formats:
tests/test_checkpoint_host.py."""
import argparse
import os
import shutil
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

KEYS = ("fc_feats", "att_feats", "labels", "masks", "att_masks")


def _batches():
    """Two batches that alternate (same shapes, other captions and region masks)."""
    out = []
    for name in ("topdown_tiny", "topdown_tiny_ragged"):
        cfg, W, I, Out, G, X = load_golden(name)
        out.append({k: I[k].numpy() for k in KEYS})
    return cfg, out


def _opt(cfg, dtype, path, use_bn=1, drop=0.5):
    return argparse.Namespace(vocab_size=cfg["V"], input_encoding_size=cfg["E"], rnn_size=cfg["H"], num_layers=1, drop_prob_lm=drop,
                              seq_length=cfg["L"], fc_feat_size=cfg["D"], att_feat_size=cfg["D"], att_hid_size=cfg["A"], use_bn=use_bn,
                              logit_layers=1, caption_model="topdown", compute_dtype=dtype, seed=5, i2t_learning_rate=5e-3,
                              i2t_train_flag=1, checkpoint_path=str(path), start_from=str(path), allow_many_hw_queues=1)


def _new_trainer(opt, init_seed, ss_prob=None, exchange=None):
    from unpaired_image_captioning_amd.trainer import Trainer
    torch.manual_seed(init_seed)                      # (the modules' default initialisation draws from torch's global generator)
    tr = Trainer(opt, exchange=exchange)
    if ss_prob is not None:
        tr.i2t_model.ss_prob = ss_prob
    return tr


def _i2t_snapshot(tr):
    torch.cuda.synchronize()
    snap = {"sd::" + k: v.detach().cpu().clone() for k, v in tr.i2t_model.state_dict().items()}
    snap["exp_avg"], snap["exp_avg_sq"] = tr.arena.exp_avg.cpu().clone(), tr.arena.exp_avg_sq.cpu().clone()
    return snap


def _assert_same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (k, (a[k].double() - b[k].double()).abs().max().item())


def _host_state(tr):
    return (tr._step, tr.i2t_model._seed_counter, tr.i2t_current_lr, tr.i2t_model.ss_prob, tr.sc_flag)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_xe_continuation_is_bit_exact(tmp_path, dtype):
    """drop_prob_lm 0.5, scheduled sampling 0.25, BatchNorm in att_embed, two alternating batches: 5 steps straight against
    2 steps + save + fresh Trainer + load + 3 steps.  Control: the weights file alone -- all there was before optimizer_i2t and
    trainer_state were written -- does NOT reproduce step 3 (fresh moments, Adam's bias correction and the seed start over)."""
    cfg, data = _batches()
    opt = _opt(cfg, dtype, tmp_path)
    straight = _new_trainer(opt, 1, ss_prob=0.25)
    straight.i2t_current_lr = 4e-3                    # (a decayed learning rate: it has to come back from the checkpoint too)
    ref_losses, after3 = [], None
    for i in range(5):
        ref_losses.append(straight.train(data[i % 2]))
        if i == 2:
            after3 = _i2t_snapshot(straight)
    first = _new_trainer(opt, 1, ss_prob=0.25)
    first.i2t_current_lr = 4e-3
    losses = [first.train(data[i % 2]) for i in range(2)]
    first.save_models("-best")
    assert sorted(os.listdir(str(tmp_path))) == ["model_i2t-best.pth", "optimizer_i2t-best.pth", "trainer_state-best.pth"]
    bn = [k for k in torch.load(os.path.join(str(tmp_path), "model_i2t-best.pth"), weights_only=True) if "running_" in k or "num_batches" in k]
    assert len(bn) == 3, bn
    resumed = _new_trainer(opt, 99)                   # other weights, ss_prob 0, step 0
    resumed.load_models()                             # (opt.start_from, '-best')
    assert _host_state(resumed) == _host_state(first) and resumed._step == 2 and resumed.i2t_model.ss_prob == 0.25
    for i in range(2, 5):
        losses.append(resumed.train(data[i % 2]))
        if i == 2:
            _assert_same(_i2t_snapshot(resumed), after3)
    print("losses", ref_losses, losses)
    assert losses == ref_losses
    _assert_same(_i2t_snapshot(resumed), _i2t_snapshot(straight))
    assert _host_state(resumed) == _host_state(straight)
    assert float(straight.arena.exp_avg.abs().max()) > 0 and int(resumed.i2t_model.att_embed[0].num_batches_tracked) == 5
    # control
    alone = os.path.join(str(tmp_path), "weights_only")
    os.makedirs(alone)
    shutil.copy(os.path.join(str(tmp_path), "model_i2t-best.pth"), alone)
    ctl = _new_trainer(opt, 99, ss_prob=0.25)
    with pytest.warns(UserWarning, match="fresh Adam"):
        ctl.load_models(alone)
    assert ctl._step == 0 and float(ctl.arena.exp_avg.abs().max()) == 0
    ctl.i2t_current_lr = 4e-3
    ctl.train(data[0])
    got = _i2t_snapshot(ctl)
    differ = [k for k in after3 if k.startswith("sd::") and after3[k].is_floating_point() and not torch.equal(got[k], after3[k])]
    assert len(differ) > len(after3) // 2, differ


def _reward(data, sampled, greedy):
    """A deterministic stand-in for CIDEr-D(sampled) - CIDEr-D(greedy): a function of the two token matrices, per row."""
    r = (sampled.sum(1) % 7).astype(np.float32) / 7.0 - (greedy.sum(1) % 5).astype(np.float32) / 5.0 + 0.3
    return np.repeat(r[:, None], sampled.shape[1], 1)


def test_self_critical_continuation_is_bit_exact(tmp_path):
    """The self-critical step draws its captions from the seed counter (sampling pass, greedy baseline, replay): 2 + 2 steps
    against 4, dropout 0.5."""
    cfg, data = _batches()
    opt = _opt(cfg, "f32", tmp_path, use_bn=0)
    straight = _new_trainer(opt, 1)
    straight.sc_flag = True
    ref_losses = [straight.train_self_critical(data[i % 2], reward_fn=_reward) for i in range(4)]
    first = _new_trainer(opt, 1)
    first.sc_flag = True
    losses = [first.train_self_critical(data[i % 2], reward_fn=_reward) for i in range(2)]
    first.save_models()
    resumed = _new_trainer(opt, 99)
    resumed.load_models(tag="")
    assert resumed.sc_flag is True
    losses += [resumed.train_self_critical(data[i % 2], reward_fn=_reward) for i in range(2, 4)]
    print("losses", ref_losses, losses)
    assert losses == ref_losses
    _assert_same(_i2t_snapshot(resumed), _i2t_snapshot(straight))
    assert _host_state(resumed) == _host_state(straight)


# ---------------------------------------------------------------- pivot NMT half
NMT_CFG = dict(layers=2, H=64, W=64, B=8, S=10, T=9, Vs=120, Vt=130)


def _nmt_trainer(path, init_seed, noam):
    from test_gpu_nmt import make_opt
    from unpaired_image_captioning_amd.trainer import Trainer
    o = make_opt(NMT_CFG, "bf16", dropout=0.1, seed=3)
    o.nmt_train_flag, o.i2t_train_flag, o.checkpoint_path, o.start_from = 1, 0, str(path), str(path)
    o.nmt_learning_rate, o.nmt_max_grad_norm, o.param_init = 5e-3, 5, 0.1
    if noam:        # lr = nmt_lr * H^-0.5 * min(step^-0.5, step * warmup^-1.5) from the SHARED step counter: both branches in 4 steps
        o.nmt_decay_method, o.nmt_warmup_steps, o.nmt_learning_rate = "noam", 3, 0.05
    tr = Trainer(o)
    torch.manual_seed(init_seed)                      # (param_init draws from torch's global generator)
    tr.build_nmt(NMT_CFG["Vs"], NMT_CFG["Vt"])
    return tr


def _nmt_snapshot(tr):
    torch.cuda.synchronize()
    snap = {"sd::" + k: v.detach().cpu().clone() for k, v in tr.nmt_model.state_dict().items()}
    a = tr.optim.nmt_arena
    snap["exp_avg"], snap["exp_avg_sq"] = a.exp_avg.cpu().clone(), a.exp_avg_sq.cpu().clone()
    return snap


def _nmt_host_state(tr):
    o = tr.optim
    return (o._step, o._nmt_steps, o._i2t_steps, o.nmt_current_lr, o.i2t_current_lr, tr.nmt_model._seed_counter)


@pytest.mark.parametrize("noam", [False, True], ids=["clip5", "noam"])
def test_nmt_continuation_is_bit_exact(tmp_path, noam):
    """bf16, dropout 0.1; gradient clipping at 5, and the noam schedule, which reads Optim's shared step counter: 2 + 2 steps
    against 4 -- losses, weights, moments, learning rates."""
    from test_gpu_nmt import synthetic
    I = synthetic(NMT_CFG, 9)
    batch = argparse.Namespace(src=I["src"].cuda(), tgt=I["tgt"].cuda(), lengths=I["lengths"])
    straight = _nmt_trainer(tmp_path, 17, noam)
    ref_losses, ref_lrs = [], []
    for _ in range(4):
        ref_losses.append(straight.train_nmt(batch))
        ref_lrs.append(straight.optim.nmt_current_lr)
    first = _nmt_trainer(tmp_path, 17, noam)
    losses = [first.train_nmt(batch) for _ in range(2)]
    first.save_models("-best")
    assert sorted(os.listdir(str(tmp_path))) == ["model_nmt-best.pth", "optimizer_nmt-best.pth", "trainer_state-best.pth"]
    resumed = _nmt_trainer(tmp_path, 23, noam)
    resumed.load_models()
    assert _nmt_host_state(resumed) == _nmt_host_state(first) and resumed.optim._nmt_steps == 2
    lrs = ref_lrs[:2]
    for _ in range(2):
        losses.append(resumed.train_nmt(batch))
        lrs.append(resumed.optim.nmt_current_lr)
    print("losses", ref_losses, losses, "lrs", ref_lrs, lrs)
    assert losses == ref_losses and lrs == ref_lrs
    assert (len(set(ref_lrs)) == 4) == noam
    _assert_same(_nmt_snapshot(resumed), _nmt_snapshot(straight))
    assert _nmt_host_state(resumed) == _nmt_host_state(straight)
    # the optimizer file is a plain Adam state dict over nmt_model.parameters(), as the reference's load_state_dict needs it
    sd = torch.load(os.path.join(str(tmp_path), "optimizer_nmt-best.pth"), weights_only=True)
    params = list(resumed.nmt_model.parameters())
    assert sd["param_groups"][0]["params"] == list(range(len(params)))
    assert all(sd["state"][i]["exp_avg"].shape == p.shape and int(sd["state"][i]["step"]) == 2 for i, p in enumerate(params))


# ---------------------------------------------------------------- two ranks on one GPU, the sharded exchange
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_train(tr, data, lo, hi):
    return [tr.train(data[i % 2]) for i in range(lo, hi)]


def _dp_snapshot(tr):
    """Weights everywhere (after the collective that makes the masters whole), moments where this rank owns them."""
    tr.gather_masters()
    torch.cuda.synchronize()
    snap = {"sd::" + k: v.detach().cpu().clone() for k, v in tr.i2t_model.state_dict().items()}
    a = tr.arena
    for n, (l, h) in enumerate(a.owned_ranges()):
        snap["exp_avg::%d" % n], snap["exp_avg_sq::%d" % n] = a.exp_avg[l:h].cpu().clone(), a.exp_avg_sq[l:h].cpu().clone()
    if a.w16 is not None:
        snap["w16"] = a.w16[:a.repl_off].cpu().clone()
    return snap


def _dp_worker(rank, world, port, out_dir, dtype):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)                          # gloo: both ranks share cuda:0
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from unpaired_image_captioning_amd.parallel_exchange import GradientExchange
    cfg, whole = _batches()
    lo, hi = GradientExchange().shard_images(cfg["n_img"])
    rows = slice(lo * cfg["S"], hi * cfg["S"])
    data = [{k: b[k][rows] for k in KEYS} for b in whole]
    opt = _opt(cfg, dtype, out_dir, use_bn=0)
    straight = _new_trainer(opt, 1, ss_prob=0.25)
    ref_losses = _dp_train(straight, data, 0, 4)
    assert straight.sharded and straight.arena.world == world and (straight.arena.w16 is not None) == (dtype == "bf16")
    first = _new_trainer(opt, 1, ss_prob=0.25)
    losses = _dp_train(first, data, 0, 2)
    torch.cuda.synchronize()
    a = first.arena
    owned = [(l, h, a.exp_avg[l:h].cpu().clone(), a.exp_avg_sq[l:h].cpu().clone()) for l, h in a.owned_ranges()]
    saved = _host_state(first)
    # the save without the wait (a collective; rank 0 writes), and the SAME trainer goes on at once: steps 3 and 4 are enqueued
    # behind the snapshot, allocate on the stream the seed counters were summed on, and run beside the writer
    first.save_models_async("-best")
    went_on = [float(_enqueue(first, data[i % 2])) for i in range(2, 4)]
    first.wait_for_save()
    dist.barrier()
    assert went_on == ref_losses[2:]
    # the file's moments are this rank's arena on the ranges it owns
    sd = torch.load(os.path.join(out_dir, "optimizer_i2t-best.pth"), weights_only=True)
    m, v = torch.zeros(a.numel), torch.zeros(a.numel)
    for i, (k, shape) in enumerate(a.param_order):
        if k not in a.offsets:
            continue
        o = a.offsets[k]
        m[o:o + sd["state"][i]["exp_avg"].numel()] = sd["state"][i]["exp_avg"].reshape(-1)
        v[o:o + sd["state"][i]["exp_avg_sq"].numel()] = sd["state"][i]["exp_avg_sq"].reshape(-1)
    for l, h, em, ev in owned:
        assert float(em.abs().max()) > 0 and torch.equal(m[l:h], em) and torch.equal(v[l:h], ev), (rank, l, h)
    state = torch.load(os.path.join(out_dir, "trainer_state-best.pth"), weights_only=True)
    assert state["world_size"] == world and len(state["seed_counters"]["i2t"]) == world
    assert state["seed_counters"]["i2t"][rank] == saved[1] and len(set(state["seed_counters"]["i2t"])) == world
    assert state["step"] == 2
    resumed = _new_trainer(opt, 99 + rank)            # other weights on every rank
    resumed.load_models()
    assert _host_state(resumed) == saved
    losses += _dp_train(resumed, data, 2, 4)
    print("rank", rank, "losses", ref_losses, losses)
    assert losses == ref_losses
    ref = _dp_snapshot(straight)
    _assert_same(_dp_snapshot(resumed), ref)
    assert _host_state(resumed) == _host_state(straight)
    # the trainer that saved: the gathers left the other rank's moments in the slices it does not own, and nothing reads them
    _assert_same(_dp_snapshot(first), ref)
    assert _host_state(first) == _host_state(straight)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_two_rank_sharded_continuation_is_bit_exact(tmp_path, dtype):
    """Each rank holds moments for its owned ranges only, and with bf16 operands current f32 masters only there: save gathers
    both, load fills the whole arena on every rank and rebuilds the operand copy.  2 + save + fresh + load + 2 steps against 4,
    bit-equal on BOTH ranks (dropout 0.5 and scheduled sampling from per-rank seed counters); the save is save_models_async
    with the saving trainer's own steps 3 and 4 enqueued behind it, and that trainer ends bit-equal too; then the world-2 files
    in a single process."""
    world = 2
    mp.spawn(_dp_worker, args=(world, _free_port(), str(tmp_path), dtype), nprocs=world, join=True)
    cfg, data = _batches()
    one = _new_trainer(_opt(cfg, dtype, tmp_path, use_bn=0), 7)
    one.load_models()
    state = torch.load(os.path.join(str(tmp_path), "trainer_state-best.pth"), weights_only=True)
    assert one._step == 2 and one.i2t_model._seed_counter == state["seed_counters"]["i2t"][0] and not one.sharded
    got = one.arena.export_adam_state(one.i2t_current_lr, one.betas, one.eps, one._step)
    sd = torch.load(os.path.join(str(tmp_path), "optimizer_i2t-best.pth"), weights_only=True)
    assert set(got["state"]) == set(sd["state"]) and len(sd["state"]) == len(list(one.i2t_model.parameters()))
    for i, st in sd["state"].items():
        assert int(got["state"][i]["step"]) == int(st["step"]) == 2
        assert torch.equal(got["state"][i]["exp_avg"], st["exp_avg"]) and torch.equal(got["state"][i]["exp_avg_sq"], st["exp_avg_sq"]), i
    w = torch.load(os.path.join(str(tmp_path), "model_i2t-best.pth"), weights_only=True)
    for k, t in one.i2t_model.state_dict().items():
        assert torch.equal(t.cpu(), w[k]), k
    assert np.isfinite(one.train(data[0]))            # and it trains on


# ---------------------------------------------------------------- saves that do not stall the step
def _enqueue(tr, data):
    """One step as the benchmark's timed loop issues it: enqueued, no host synchronisation (Trainer.train adds the reference's
    loss.item())."""
    from unpaired_image_captioning_amd.trainer import _steps_from_host_labels
    return tr.train_device_batch(tr.to_device(data), _steps_from_host_labels(np.asarray(data["labels"])), tr._mask_sum(data))


def _files(path, tag):
    return {n: torch.load(os.path.join(str(path), n % tag), weights_only=True) for n in ("model_i2t%s.pth", "optimizer_i2t%s.pth", "trainer_state%s.pth")}


def _assert_same_files(a, b):
    assert a["trainer_state%s.pth"] == b["trainer_state%s.pth"]
    _assert_same(a["model_i2t%s.pth"], b["model_i2t%s.pth"])
    oa, ob = a["optimizer_i2t%s.pth"], b["optimizer_i2t%s.pth"]
    assert oa["param_groups"] == ob["param_groups"] and set(oa["state"]) == set(ob["state"]) and len(oa["state"]) > 0
    for i in oa["state"]:
        _assert_same(oa["state"][i], ob["state"][i])


SAVE_CASES = {
    # the tiny golden shapes, and the real hidden width, where the forward recurrence of every step is ONE persistent launch: the
    # snapshot and its copy to the host must not make a later step's launch time out
    # (cfg, dtype, use_bn, scheduled sampling -- which the persistent launch does not take)
    "tiny-bf16": (dict(V=50, E=32, H=32, A=32, D=64, L=6), "bf16", 1, 0.25),
    "h512-f32": (dict(V=50, E=512, H=512, A=512, D=64, L=6), "f32", 0, None),
}


@pytest.mark.parametrize("case", list(SAVE_CASES))
def test_async_save_snapshots_step_2_while_steps_3_to_5_run(tmp_path, case):
    """save_models_async after step 2 with steps 3-5 enqueued right behind it, and a second save issued while the first may
    still be in flight: the first save's files hold step 2 exactly -- every tensor equals the synchronous save of a twin run
    stopped there --, the second's hold step 5, and step 5's loss and weights are those of a run that never saved."""
    from unpaired_image_captioning_amd import _lib
    cfg, dtype, use_bn, ss_prob = SAVE_CASES[case]
    _, data = _batches()
    dirs = [os.path.join(str(tmp_path), d) for d in ("twin", "async", "never")]

    def new(path):
        tr = _new_trainer(_opt(cfg, dtype, path, use_bn=use_bn), 1, ss_prob=ss_prob)
        tr.build_optimizer()
        return tr

    before = _lib.persistent_status()
    twin = new(dirs[0])
    for i in range(2):
        _enqueue(twin, data[i % 2])
    twin.save_models()
    run = new(dirs[1])
    for i in range(2):
        _enqueue(run, data[i % 2])
    run.save_models_async()
    for i in range(2, 5):
        loss = _enqueue(run, data[i % 2])
    run.save_models_async("-5")                       # (waits for the writer of the first, then snapshots step 5)
    run.wait_for_save()
    never = new(dirs[2])
    for i in range(5):
        ref_loss = _enqueue(never, data[i % 2])
    assert float(loss) == float(ref_loss)
    after = _lib.persistent_status()                  # (raises if a persistent launch timed out)
    assert after[0] == 0
    if cfg["H"] == 512:
        assert after[1] + after[2] > before[1] + before[2]      # the steps really ran persistent launches
    _assert_same(_i2t_snapshot(run), _i2t_snapshot(never))
    assert _host_state(run) == _host_state(never) and run._step == 5
    _assert_same_files(_files(dirs[1], ""), _files(dirs[0], ""))
    never.save_models("-5")
    _assert_same_files(_files(dirs[1], "-5"), _files(dirs[2], "-5"))
    assert _files(dirs[1], "")["trainer_state%s.pth"]["step"] == 2 and _files(dirs[1], "-5")["trainer_state%s.pth"]["step"] == 5
    assert sorted(os.listdir(dirs[1])) == sorted(n % t for t in ("", "-5") for n in ("model_i2t%s.pth", "optimizer_i2t%s.pth", "trainer_state%s.pth"))


def test_unwritable_checkpoint_path_raises_from_wait_for_save(tmp_path):
    cfg, data = _batches()
    blocker = os.path.join(str(tmp_path), "a_file")
    open(blocker, "w").close()
    tr = _new_trainer(_opt(cfg, "f32", os.path.join(blocker, "ckpt")), 1)
    _enqueue(tr, data[0])
    tr.save_models_async()                            # returns: the failure belongs to the writer
    _enqueue(tr, data[1])
    with pytest.raises(OSError):
        tr.wait_for_save()
    tr.wait_for_save()                                # (reported once)
    with pytest.raises(OSError):
        tr.save_models()
    tr.opt.checkpoint_path = os.path.join(str(tmp_path), "ckpt")
    tr.save_models()                                  # and the trainer saves on
    assert _files(tr.opt.checkpoint_path, "")["trainer_state%s.pth"]["step"] == 2
