"""A/B of two source trees' Trainer on the smallest golden fixtures: same bits, same library calls.

    python tools/trainer_ab.py --package <dir that holds unpaired_image_captioning_amd/> --out a.json

Run it once per tree, each run in a fresh process, and diff the two JSON files (`--diff a.json b.json` prints the first
difference per case).  Per case and step the JSON holds SHA-256 hashes of the loss, the whole flat arena, every optimizer state
arena, the seed counters and the step counters, and the sequence of `uic_*` library calls the step made -- recorded by a Python
proxy around what `_lib.load()` returns, installed here only.  The save case hashes every tensor of every written file.
Fixtures: topdown_tiny, topdown_tiny_bn2_train, fc_tiny, nmt_tiny (tests/golden/ of the tree this tool lies in, for both
packages).  Both trees should load the same libuic_hip.so (UIC_LIB)."""
import argparse
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(HERE, "tests", "golden")
KEYS = ("fc_feats", "att_feats", "labels", "masks", "att_masks")
STEPS = 3


def sha(x):
    import torch
    h = hashlib.sha256()
    if torch.is_tensor(x):
        x = x.detach().cpu().contiguous()
        h.update(str((x.dtype, tuple(x.shape))).encode())
        h.update(x.reshape(-1).view(torch.uint8).numpy().tobytes() if x.numel() else b"")
    else:
        h.update(repr(x).encode())
    return h.hexdigest()


class CallLog(object):
    """Stands in for the loaded ctypes library: every uic_* function looked up on it is wrapped to append its name."""

    def __init__(self, lib):
        self._real = lib
        self.names = []
        self._wrapped = {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("uic_"):
            return fn
        w = self._wrapped.get(name)
        if w is None:
            def w(*a, _fn=fn, _name=name):
                self.names.append(_name)
                return _fn(*a)
            self._wrapped[name] = w
        return w

    def take(self):
        names, self.names = self.names, []
        return {"n": len(names), "sha": hashlib.sha256("\n".join(names).encode()).hexdigest(), "names": names}


def load_golden(name):
    import torch
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    keys = ["V", "E", "H", "A", "D", "L", "n_img", "S", "R", "use_bn", "bn_train"]
    cfg = dict(zip(keys, [int(x) for x in z["cfg"]]))
    W = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w::")}
    I = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in::")}
    cfg["logit_layers"] = int(z["logit_layers"]) if "logit_layers" in z.files else 1
    cfg["Dfc"] = int(z["fc_feat_size"]) if "fc_feat_size" in z.files else cfg["D"]
    return cfg, W, I


def load_nmt(name):
    import torch
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    W = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w::")}
    I = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("in::")}
    layers, H, B, S, T, Vs, Vt = [int(x) for x in z["cfg"]]
    return dict(layers=layers, H=H, W=W["encoder.embeddings.word_lut.weight"].shape[1], B=B, S=S, T=T, Vs=Vs, Vt=Vt), W, I


def topdown_opt(cfg, dtype, drop, path=None, use_bn=None):
    return argparse.Namespace(vocab_size=cfg["V"], input_encoding_size=cfg["E"], rnn_size=cfg["H"], num_layers=1, drop_prob_lm=drop,
                              seq_length=cfg["L"], fc_feat_size=cfg["Dfc"], att_feat_size=cfg["D"], att_hid_size=cfg["A"],
                              use_bn=cfg["use_bn"] if use_bn is None else use_bn, logit_layers=cfg["logit_layers"],
                              caption_model="topdown", compute_dtype=dtype, seed=5, i2t_learning_rate=5e-3, i2t_train_flag=1,
                              checkpoint_path=path, start_from=path)


def fc_opt(cfg, dtype, drop):
    return argparse.Namespace(vocab_size=cfg["V"], input_encoding_size=cfg["E"], rnn_type="LSTM", rnn_size=cfg["H"], num_layers=1,
                              drop_prob_lm=drop, seq_length=cfg["L"], fc_feat_size=cfg["D"], caption_model="fc", compute_dtype=dtype,
                              seed=5, i2t_learning_rate=5e-3)


def nmt_opt(cfg, dtype):
    return argparse.Namespace(layers=cfg["layers"], rnn_size=cfg["H"], word_vec_size=cfg["W"], brnn=True, rnn_type="LSTM",
                              dropout=0.1, input_feed=1, position_encoding=False, coverage_attn=False, copy_attn=False,
                              context_gate=None, attention_type="dot", attn_transform="softmax", fertility=None,
                              predict_fertility=False, guided_fertility=None, supervised_fertility=None,
                              lambda_coverage=0, lambda_fertility=0, lambda_exhaust=0, batch_size=cfg["B"], gpus=[0],
                              compute_dtype=dtype, seed=3, nmt_train_flag=1, i2t_train_flag=0, nmt_learning_rate=5e-3,
                              nmt_max_grad_norm=5, param_init=0.1)


def reward(data, sampled, greedy):
    """A deterministic stand-in for CIDEr-D(sampled) - CIDEr-D(greedy): a function of the two token matrices, per row."""
    r = (sampled.sum(1) % 7).astype(np.float32) / 7.0 - (greedy.sum(1) % 5).astype(np.float32) / 5.0 + 0.3
    return np.repeat(r[:, None], sampled.shape[1], 1)


def arena_state(prefix, arena):
    out = {prefix + "flat": sha(arena.flat)}
    for i, s in enumerate(arena.states):
        out[prefix + "state%d" % i] = sha(s)
    return out


def i2t_state(tr, loss):
    import torch
    torch.cuda.synchronize()
    out = {"loss": sha(float(loss)), "step": tr._step, "seed": int(getattr(tr.i2t_model, "_seed_counter", -1))}
    out.update(arena_state("arena.", tr.arena))
    out["buffers"] = sha([(k, sha(v)) for k, v in tr.i2t_model.state_dict().items()])
    return out


def captioner(Trainer, fixture, dtype, fc=False, drop=0.5, use_bn=None, path=None):
    import torch
    cfg, W, I = load_golden(fixture)
    torch.manual_seed(1)
    tr = Trainer(fc_opt(cfg, dtype, drop) if fc else topdown_opt(cfg, dtype, drop, path, use_bn))
    if use_bn is None:
        tr.i2t_model.load_state_dict(W)
    tr.build_optimizer()
    data = {k: I[k].numpy() for k in (("fc_feats", "labels", "masks") if fc else KEYS)}
    other = dict(data, labels=data["labels"].copy(), masks=data["masks"].copy())    # (another dict object: prefetches go by identity)
    return tr, [data, other]


def run_cases(pkg, log):
    import torch
    from unpaired_image_captioning_amd.trainer import Trainer
    res = {}

    def steps(name, tr, one, state):
        log.take()
        out = []
        for i in range(STEPS):
            loss = one(i)
            s = state(tr, loss)
            s["calls"] = log.take()
            out.append(s)
        res[name] = out
        print(name, "ok", flush=True)

    # Trainer.train, next_data as a dict and as a callable
    for fixture, fc in (("topdown_tiny", False), ("topdown_tiny_bn2_train", False), ("fc_tiny", True)):
        for dtype in ("f32", "bf16"):
            for kind in ("dict", "callable"):
                tr, d = captioner(Trainer, fixture, dtype, fc)
                if fixture == "topdown_tiny":
                    tr.i2t_model.ss_prob = 0.25
                nxt = (lambda i: d[(i + 1) % 2]) if kind == "dict" else (lambda i: (lambda: d[(i + 1) % 2]))
                steps("train/%s/%s/%s" % (fixture, dtype, kind), tr, lambda i: tr.train(d[i % 2], next_data=nxt(i)), i2t_state)
    # the self-critical step, serial and overlapped baseline
    for fixture, fc in (("topdown_tiny", False), ("fc_tiny", True)):
        for serial in (True, False):
            tr, d = captioner(Trainer, fixture, "f32", fc)
            tr.sc_flag = True
            tr.serial_baseline = serial
            steps("scst/%s/%s" % (fixture, "serial" if serial else "overlapped"), tr,
                  lambda i: tr.train_self_critical(d[i % 2], reward_fn=reward, next_data=d[(i + 1) % 2]), i2t_state)
    # the NMT step
    cfg, W, I = load_nmt("nmt_tiny")
    for dtype in ("f32", "bf16"):
        tr = Trainer(nmt_opt(cfg, dtype))
        torch.manual_seed(17)
        tr.build_nmt(cfg["Vs"], cfg["Vt"])
        tr.nmt_model.load_state_dict(W)
        batch = argparse.Namespace(src=I["src"].cuda(), tgt=I["tgt"].cuda(), lengths=I["lengths"])

        def nmt_state(tr, loss):
            torch.cuda.synchronize()
            o = tr.optim
            out = {"loss": sha(float(loss)), "step": [o._step, o._nmt_steps], "seed": int(tr.nmt_model._seed_counter),
                   "lr": sha(float(o.nmt_current_lr)), "ppl": sha(float(tr.nmt_train_ppl)), "acc": sha(float(tr.nmt_train_acc))}
            out.update(arena_state("arena.", o.nmt_arena))
            return out
        steps("nmt/nmt_tiny/%s" % dtype, tr, lambda i: tr.train_nmt(batch), nmt_state)
    # the discriminator step
    cfg, W, I = load_golden("topdown_tiny")
    opt = topdown_opt(cfg, "f32", 0.0)
    opt.disc_num_filters, opt.disc_filter_sizes, opt.disc_learning_rate = 16, (1, 2, 3), 1e-2
    torch.manual_seed(2)
    tr = Trainer(opt)
    tr.build_discriminator()
    g = torch.Generator().manual_seed(4)
    real = I["labels"][:, 1:1 + opt.seq_length]
    fake = torch.randint(0, cfg["V"] + 1, real.shape, generator=g)

    def disc_state(tr, loss):
        torch.cuda.synchronize()
        out = {"loss": sha(float(loss)), "step": tr._disc_step, "seed": int(tr.discriminator.seed)}
        out.update(arena_state("arena.", tr.disc_arena))
        return out
    steps("disc/topdown_tiny", tr, lambda i: tr.train_discriminator(real, fake), disc_state)
    # save_models_async / wait_for_save / load_models, then one more step
    for dtype in ("f32", "bf16"):
        with tempfile.TemporaryDirectory() as path:
            tr, d = captioner(Trainer, "topdown_tiny", dtype, use_bn=1, path=path)
            tr.i2t_model.ss_prob = 0.25
            log.take()
            out = {}
            for i in range(2):
                tr.train(d[i % 2], next_data=d[(i + 1) % 2])
            tr.save_models_async("-best")
            went_on = tr.train(d[0], next_data=d[1])
            tr.wait_for_save()
            out["saver"] = i2t_state(tr, went_on)
            files = {}
            for n in sorted(os.listdir(path)):
                flat = []

                def walk(prefix, o):
                    if isinstance(o, dict):
                        for k in o:
                            walk(prefix + "/" + str(k), o[k])
                    elif isinstance(o, (list, tuple)):
                        for j, v in enumerate(o):
                            walk(prefix + "/%d" % j, v)
                    else:
                        flat.append((prefix, sha(o)))
                walk("", torch.load(os.path.join(path, n), weights_only=True))
                files[n] = {"entries": len(flat), "sha": sha(flat)}
            out["files"] = files
            torch.manual_seed(99)
            fresh = Trainer(topdown_opt(load_golden("topdown_tiny")[0], dtype, 0.5, path, 1))
            fresh.load_models()
            out["resumed"] = i2t_state(fresh, fresh.train(d[0], next_data=d[1]))
            out["calls"] = log.take()
            res["save/topdown_tiny/%s" % dtype] = out
            print("save", dtype, "ok", flush=True)
    return res


def diff(a, b):
    A, B = json.load(open(a)), json.load(open(b))
    bad = 0
    for case in sorted(set(A) | set(B)):
        if A.get(case) == B.get(case):
            continue
        bad += 1
        x, y = json.dumps(A.get(case), sort_keys=True), json.dumps(B.get(case), sort_keys=True)
        at = next((i for i in range(min(len(x), len(y))) if x[i] != y[i]), min(len(x), len(y)))
        print("DIFFERENT %s at %d: ...%s | ...%s" % (case, at, x[max(0, at - 60):at + 60], y[max(0, at - 60):at + 60]))
    print("%d cases, %d differ" % (len(set(A) | set(B)), bad))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package", help="directory that holds the unpaired_image_captioning_amd package to drive")
    ap.add_argument("--out")
    ap.add_argument("--diff", nargs=2)
    args = ap.parse_args()
    if args.diff:
        sys.exit(diff(*args.diff))
    sys.path.insert(0, os.path.abspath(args.package))
    import unpaired_image_captioning_amd as pkg
    from unpaired_image_captioning_amd import _lib
    assert os.path.dirname(os.path.dirname(os.path.abspath(pkg.__file__))) == os.path.abspath(args.package), pkg.__file__
    log = CallLog(_lib.load())
    _lib._lib = log                             # (what _lib.load() returns from now on)
    res = run_cases(pkg, log)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)
    print("wrote", args.out, len(res), "cases")


if __name__ == "__main__":
    main()
