#!/usr/bin/env python3
"""Generate tests/golden/adaatt*.npz from the REFERENCE's own AdaAttModel / AdaAttMOModel (models/AttModel.py).

Runs only where the reference tree is present; it is imported through the shims of make_golden.py and none of its text travels.
Each fixture holds the reference model's state_dict (float tensors as `w16::<key>`: the weights are rounded to bf16-representable
values BEFORE the reference runs and stored as their 16 high bits, half the bytes and exact; integer tensors as `w::<key>`), every
key's shape (`shape::<key>`), the inputs (`in::`) and the reference outputs (`out::`): _forward's log-probs, the prepared
features, the first three steps' (logprobs, h, c) of get_logprobs_state fed with the caption's own tokens, _sample's greedy
seq / seqLogprobs, _sample_beam's seq / logps and done lists (beam 3).  The reference module runs in float64 (`model.double()`;
weights and inputs convert exactly), so the outputs carry no f32 rounding of their own.

`att_masks=None` comes without BatchNorm: the reference's BatchNorm1d(att_feat_size) then sees [n, R, D] and raises (it takes R
for the channel axis); `--probe` shows it.  use_bn 2 therefore has a fixture of its own with masks.

Condition on the inputs, checked here and again by the tests: at every live greedy step and every beam decision the gap between
the winner and the runner-up is >= 1e-2 (ten times the f32 log-prob tolerance), measured on the float64 restatement.

    python tests/golden/make_golden_adaatt.py [--scan] [name ...]
"""
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)

# name -> (maxout, V, H, D, Dfc, layers, logit_layers, n_img, R, L, use_bn, masks: 'ragged' | 'one' | None, seed)
CASES = {
    "adaatt_tiny": (0, 50, 16, 32, 24, 1, 1, 4, 6, 7, 0, "ragged", 1),
    "adaattmo_tiny": (1, 50, 16, 32, 24, 1, 1, 4, 6, 7, 0, "ragged", 17),
    "adaatt_bn1_ragged": (0, 50, 16, 32, 24, 1, 1, 4, 6, 7, 1, "one", 12),
    "adaatt_nomask": (0, 50, 16, 32, 24, 1, 1, 3, 5, 7, 0, None, 5),
    "adaatt_bn2": (0, 50, 16, 32, 24, 1, 1, 4, 6, 7, 2, "ragged", 5),
    "adaattmo_2layer_logit2": (1, 50, 16, 32, 24, 2, 2, 4, 6, 7, 0, "ragged", 9),
}


def build(att_mod, spec):
    import adaatt_cases as AC
    maxout, V, H, D, Dfc, layers, logit_layers, n_img, R, L, use_bn, masks, seed = spec
    cfg = dict(V=V, H=H, D=D, Dfc=Dfc, layers=layers, logit_layers=logit_layers, n_img=n_img, R=R, L=L, use_bn=use_bn, maxout=maxout, beam=AC.BEAM)
    torch.manual_seed(seed)
    model = (att_mod.AdaAttMOModel if maxout else att_mod.AdaAttModel)(AC.opt_of(cfg))
    model.eval()
    g = torch.Generator().manual_seed(seed + 7)
    with torch.no_grad():
        sd = model.state_dict()
        for k, v in sd.items():
            if use_bn and v.dim() == 1 and (k.startswith("att_embed.0.") or k.startswith("att_embed.4.")):
                if k.endswith("weight"):
                    v.copy_(1 + 0.2 * torch.randn(v.shape, generator=g))
                elif k.endswith("bias") or k.endswith("running_mean"):
                    v.copy_(0.1 * torch.randn(v.shape, generator=g))
                elif k.endswith("running_var"):
                    v.copy_(0.5 + torch.rand(v.shape, generator=g))
            elif v.dim() == 2 and not k.startswith("embed."):
                v.mul_(3.0)
        last = [k for k in sd if k.startswith("logit.") and k.endswith("bias")][-1]
        sd[last][0] += 1.0
        for k, v in sd.items():
            if v.is_floating_point():
                v.copy_(v.to(torch.bfloat16).float())
    model.double()
    return cfg, model


def run_case(att_mod, name, spec, scan=False):
    import adaatt_cases as AC
    cfg, model = build(att_mod, spec)
    V, D, Dfc, n_img, R, L, masks, seed = cfg["V"], cfg["D"], cfg["Dfc"], cfg["n_img"], cfg["R"], cfg["L"], spec[11], spec[12]
    fc32, att32, am32, labels = AC.synthetic_inputs(V, D, Dfc, n_img, R, L, masks, seed)
    fc, att, am = fc32.double(), att32.double(), (am32.double() if am32 is not None else None)
    out = {"cfg::" + k: np.int64(v) for k, v in cfg.items()}
    sd = model.state_dict()
    for k, v in sd.items():
        out["shape::" + k] = np.array(v.shape, dtype=np.int64)
        if v.is_floating_point():
            out["w16::" + k] = (v.detach().float().contiguous().view(torch.int32) >> 16).to(torch.int16).numpy().view(np.uint16)
        else:
            out["w::" + k] = v.detach().clone().numpy()
    out["in::fc_feats"], out["in::att_feats"], out["in::labels"] = fc32.numpy(), att32.numpy(), labels.numpy()
    if am32 is not None:
        out["in::att_masks"] = am32.numpy()
    with torch.no_grad():
        logp = model._forward(fc, None, att, labels, am)
        p_fc, p_att, pp_att, p_m = model._prepare_feature(fc, att, am)
        state = model.init_hidden(n_img)
        steps = []
        for i in range(3):
            lp_i, state = model.get_logprobs_state(labels[:, i].clone(), p_fc, p_att, pp_att, p_m, state)
            steps.append((lp_i, state[0], state[1]))
        seq, slp = model._sample(fc, None, att, am, {"sample_max": 1})
        bseq, _ = model._sample_beam(fc, att, am, {"beam_size": AC.BEAM})
        done = model.done_beams
    out["out::logprobs"] = logp.numpy()
    out["out::fc_embed"], out["out::att_embed"], out["out::p_att"] = p_fc.numpy(), p_att.numpy(), pp_att.numpy()
    for i, (lp_i, h, c) in enumerate(steps):
        out["out::step%d_logprobs" % i], out["out::step%d_h" % i], out["out::step%d_c" % i] = lp_i.numpy(), h.numpy(), c.numpy()
    B = AC.BEAM
    out["out::greedy_seq"], out["out::greedy_logprobs"] = seq.numpy(), slp.numpy()
    out["out::beam_seq"] = bseq.numpy()
    out["out::beam_logprobs"] = np.stack([d[0]["logps"].double().numpy() for d in done])
    out["out::done_count"] = np.array([len(d) for d in done], dtype=np.int64)
    out["out::done_seq"] = np.stack([torch.stack([b["seq"] for b in d] + [torch.zeros(L, dtype=torch.int64)] * (B - len(d))).numpy() for d in done])
    out["out::done_logps"] = np.stack([torch.stack([b["logps"].double() for b in d] + [torch.zeros(L, dtype=torch.float64)] * (B - len(d))).numpy() for d in done])
    out["out::done_p"] = np.array([[float(b["p"]) for b in d] + [0.0] * (B - len(d)) for d in done], dtype=np.float64)
    # the condition on the inputs, on the float64 restatement
    W64 = {k: v.clone() for k, v in sd.items()}
    s64, _, gap = AC.sample_greedy(W64, cfg, fc, att, am)
    b64, _, _, bgap = AC.beam_search(W64, cfg, fc, att, am, B)
    ok = gap >= AC.MIN_GAP and bgap >= AC.MIN_GAP and torch.equal(s64, seq) and torch.equal(b64, bseq)
    print("%-30s greedy gap %.4f  beam gap %.4f  greedy %s  %s" % (name, gap, bgap, seq.tolist(), "ok" if ok else "REJECTED"))
    if scan:
        return ok
    if not ok:
        raise SystemExit("%s: seed %d does not meet the gap condition (or the restatement disagrees); choose another seed" % (name, seed))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print("  wrote %s (%d bytes)" % (path, os.path.getsize(path)))


def probe(att_mod):
    """att_masks=None with use_bn: what the reference does."""
    import adaatt_cases as AC
    spec = CASES["adaatt_bn2"]
    cfg, model = build(att_mod, spec)
    fc, att, _, labels = AC.synthetic_inputs(cfg["V"], cfg["D"], cfg["Dfc"], cfg["n_img"], cfg["R"], cfg["L"], None, 1)
    try:
        with torch.no_grad():
            model._forward(fc.double(), None, att.double(), labels, None)
        print("att_masks=None with use_bn=2: the reference ran")
    except Exception as e:      # noqa: BLE001
        print("att_masks=None with use_bn=2: the reference raises %s: %s" % (type(e).__name__, e))


def main():
    import make_golden
    att_mod, _ = make_golden._load_reference()
    if "--probe" in sys.argv:
        return probe(att_mod)
    only = [a for a in sys.argv[1:] if not a.startswith("--")]
    for name, spec in CASES.items():
        if only and name not in only:
            continue
        if "--scan" in sys.argv:        # which seeds meet the condition (nothing is written)
            for seed in range(int(os.environ.get('SCAN_SEEDS', '12'))):
                run_case(att_mod, "%s seed %d" % (name, seed), spec[:-1] + (seed,), scan=True)
        else:
            run_case(att_mod, name, spec)


if __name__ == "__main__":
    main()
