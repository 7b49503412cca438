#!/usr/bin/env python3
"""Generate tests/golden/transformer_*.npz from the REFERENCE's own models/TransformerModel.py.

Runs only where the reference tree is present; it is imported through the shims of make_golden.py and none of its text travels.
Each fixture holds the reference model's state_dict (float tensors as `w16::<key>`: the weights are rounded to bf16-representable
values BEFORE the reference runs and stored as their 16 high bits, half the bytes and exact; integer tensors as `w::<key>`; the
sinusoidal buffer `model.tgt_embed.1.pe` -- 5000 rows, over a megabyte -- only as its first 64 rows in `pe::head`: the loader
rebuilds the table and checks it against them), every key's shape (`shape::<key>`), the inputs (`in::`) and the reference outputs
(`out::`): _forward's log-probs, the encoder memory, the intermediates of encoder layer 0, _sample's greedy seq / seqLogprobs,
_sample_beam's seq and done lists (beam 3).  The reference module runs in float64 (`model.double()`; weights and inputs convert
exactly), so the outputs carry no f32 rounding of their own: at these log-probs of 30-40 that alone is 1.3e-5.  The gap search of
`--scan` prints which seeds meet the condition below; `att_masks=None` comes without BatchNorm because the reference's
BatchNorm1d then sees [n, R, D] and fails.

_forward itself cannot run under today's torch (`seq_mask[:, 0] += 1` on a bool tensor, TransformerModel.py:379), so the script
builds that one mask itself and calls model.model(...) + model.model.generator(...); _sample and _sample_beam run unmodified.

Condition on the inputs, checked here and again by the tests: at every live greedy step and every beam decision the gap between
the winner and the runner-up is >= 1e-2 (ten times the f32 log-prob tolerance), measured on the float64 restatement.

    python tests/golden/make_golden_transformer.py
"""
import argparse
import importlib.util
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)

MIN_GAP = 1e-2
BEAM = 3

# name -> (V, D, d_model, d_ff, N, n_img, R, L, use_bn, masks: 'ragged' | 'one' | None, seed)
CASES = {
    "transformer_tiny": (50, 64, 64, 100, 2, 4, 6, 7, 0, "ragged", 2),
    "transformer_bn1_wide": (50, 48, 128, 128, 1, 4, 5, 7, 1, "one", 22),
    "transformer_bn2": (50, 64, 64, 100, 2, 3, 6, 7, 2, "ragged", 16),
    "transformer_nomask": (50, 64, 64, 100, 1, 3, 6, 7, 0, None, 19),    # (att_masks=None with use_bn: the reference's BatchNorm1d sees [n, R, D] and fails)
}


def load_reference():
    import make_golden
    make_golden._load_reference()
    spec = importlib.util.spec_from_file_location("models.TransformerModel", os.path.join(make_golden.P, "models", "TransformerModel.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["models.TransformerModel"] = mod
    spec.loader.exec_module(mod)
    return mod


def inputs(V, D, n_img, R, L, masks, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    att = torch.randn(n_img, R, D, generator=g)
    am = None
    if masks is not None:
        lens = torch.randint(2, R + 1, (n_img,), generator=g)
        lens[0] = R                                   # clip_att keeps all R
        if masks == "one":
            lens[-1] = 1                              # an image with a single region
        am = (torch.arange(R)[None, :] < lens[:, None]).float()
    labels = torch.zeros(n_img, L + 2, dtype=torch.int64)
    for i in range(n_img):
        n = int(torch.randint(1, L + 1, (1,), generator=g))
        labels[i, 1:1 + n] = torch.randint(1, V + 1, (n,), generator=g)
    labels[1] = 0                                     # an empty caption
    return att, am, labels


def run_case(mod, name, spec, scan=False):
    import transformer_cases as TC
    V, D, dm, dff, N, n_img, R, L, use_bn, masks, seed = spec
    torch.manual_seed(seed)
    opt = argparse.Namespace(vocab_size=V, input_encoding_size=dm, rnn_size=dff, num_layers=N, drop_prob_lm=0.5, seq_length=L,
                             att_feat_size=D, use_bn=use_bn, caption_model="transformer")
    model = mod.TransformerModel(opt)
    model.eval()
    with torch.no_grad():
        model.model.generator.proj.weight.mul_(6.0)
        model.model.generator.proj.bias[0] += 1.5
        if use_bn:
            g = torch.Generator().manual_seed(seed + 7)
            for k, v in model.state_dict().items():
                if k.startswith("att_embed.0.") or k.startswith("att_embed.4."):
                    if k.endswith("weight"):
                        v.copy_(1 + 0.2 * torch.randn(v.shape, generator=g))
                    elif k.endswith("bias") or k.endswith("running_mean"):
                        v.copy_(0.1 * torch.randn(v.shape, generator=g))
                    elif k.endswith("running_var"):
                        v.copy_(0.5 + torch.rand(v.shape, generator=g))
        # the weights are stored as bf16 bit patterns (half the bytes): make them exactly representable BEFORE the reference runs
        for k, v in model.state_dict().items():
            if v.is_floating_point() and not k.endswith(".pe"):
                v.copy_(v.to(torch.bfloat16).float())
    # the reference runs in float64 (the stored weights and inputs convert exactly): its outputs then carry no f32 rounding of their
    # own -- at log-probs of magnitude 30-40 that rounding alone is 1.3e-5 -- and pin the restatement far below the tests' bounds
    model.double()
    att32, am32, labels = inputs(V, D, n_img, R, L, masks, seed)
    att, am = att32.double(), (am32.double() if am32 is not None else None)
    fc = torch.zeros(n_img, 8, dtype=torch.float64)
    out = {"cfg::" + k: np.int64(v) for k, v in dict(V=V, D=D, d_model=dm, d_ff=dff, N=N, n_img=n_img, R=R, L=L, use_bn=use_bn, beam=BEAM).items()}
    sd = model.state_dict()
    for k, v in sd.items():
        out["shape::" + k] = np.array(v.shape, dtype=np.int64)
        if k.endswith(".pe"):
            out["pe::head"] = v[0, :64].float().numpy().copy()
        elif v.is_floating_point():
            out["w16::" + k] = (v.detach().float().contiguous().view(torch.int32) >> 16).to(torch.int16).numpy().view(np.uint16)
        else:
            out["w::" + k] = v.detach().clone().numpy()
    out["in::att_feats"] = att32.numpy()
    if am32 is not None:
        out["in::att_masks"] = am32.numpy()
    out["in::labels"] = labels.numpy()
    taps = {}
    hooks = [model.att_embed.register_forward_hook(lambda m, i, o: taps.__setitem__("att_embed_packed", o.detach().clone())),
             model.model.encoder.layers[0].sublayer[0].register_forward_hook(lambda m, i, o: taps.__setitem__("enc0.after_attn", o.detach().clone())),
             model.model.encoder.layers[0].register_forward_hook(lambda m, i, o: taps.__setitem__("enc0.out", o.detach().clone()))]
    with torch.no_grad():
        a, _, m, _ = model._prepare_feature(att, am)
        memory = model.model.encode(a, m)
        for h in hooks:
            h.remove()
        tok = labels[:, :-1]
        seq_mask = (tok > 0)
        seq_mask[:, 0] = True
        seq_mask = seq_mask.unsqueeze(-2) & mod.subsequent_mask(tok.size(-1))
        logp = model.model.generator(model.model(a, tok, m, seq_mask))
        seq, slp = model._sample(fc, None, att, am, {"sample_max": 1})
        bseq, blp = model._sample_beam(fc, None, att, am, {"beam_size": BEAM})
        done = model.done_beams
    out["out::att_embed"] = a.numpy()
    out["out::enc0.after_attn"] = taps["enc0.after_attn"].numpy()
    out["out::enc0.out"] = taps["enc0.out"].numpy()
    out["out::memory"] = memory.numpy()
    out["out::logprobs"] = logp.numpy()
    out["out::greedy_seq"] = seq.numpy()
    out["out::greedy_logprobs"] = slp.numpy()
    out["out::beam_seq"] = bseq.numpy()
    out["out::beam_logprobs"] = blp.numpy()
    out["out::done_count"] = np.array([len(d) for d in done], dtype=np.int64)
    out["out::done_seq"] = np.stack([torch.stack([b["seq"] for b in d] + [torch.zeros(L, dtype=torch.int64)] * (BEAM - len(d))).numpy() for d in done])
    out["out::done_logps"] = np.stack([torch.stack([b["logps"].float() for b in d] + [torch.zeros(L)] * (BEAM - len(d))).numpy() for d in done])
    out["out::done_p"] = np.array([[float(b["p"]) for b in d] + [0.0] * (BEAM - len(d)) for d in done], dtype=np.float64)
    # the condition on the inputs, on the float64 restatement
    W64 = {k: v.clone() for k, v in sd.items()}
    s64, _, gap = TC.sample_greedy(W64, att, am, L, N, use_bn)
    b64, _, _, bgap = TC.beam_search(W64, att, am, L, N, use_bn, BEAM)
    ok = gap >= MIN_GAP and bgap >= MIN_GAP and torch.equal(s64, seq) and torch.equal(b64, bseq)
    print("%-26s greedy gap %.4f  beam gap %.4f  greedy %s  %s" % (name, gap, bgap, seq.tolist(), "ok" if ok else "REJECTED"))
    if scan:
        return ok
    if not ok:
        raise SystemExit("%s: seed %d does not meet the gap condition (or the restatement disagrees); choose another seed" % (name, seed))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print("  wrote %s (%d bytes)" % (path, os.path.getsize(path)))


def main():
    mod = load_reference()
    only = [a for a in sys.argv[1:] if not a.startswith("--")]
    for name, spec in CASES.items():
        if only and name not in only:
            continue
        if "--scan" in sys.argv:        # which seeds meet the condition (nothing is written)
            for seed in range(int(os.environ.get('SCAN_SEEDS', '12'))):
                run_case(mod, "%s seed %d" % (name, seed), spec[:-1] + (seed,), scan=True)
        else:
            run_case(mod, name, spec)


if __name__ == "__main__":
    main()
