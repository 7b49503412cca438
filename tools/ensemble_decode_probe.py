#!/usr/bin/env python3
"""Ensemble decode (models/AttEnsemble.py, uic_topdown_ensemble_sample / _sample_beam) at BASELINE configs[1] size: ms per
decode for M = 1, 2, 4 members, beam 3 and greedy, and the share of the combining kernel (csrc/ensemble.hip), timed on its own
over the same rows.  Sanity line: M = 1 through the ensemble path against the single model's own launch chain
(UIC_REC_FWD_CHAIN) and its default path (the persistent decode launch where the shapes allow).
    python tools/ensemble_decode_probe.py [--iters 20] [--rows 128]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rows", type=int, default=0, help="images (default: the bench config's 128)")
args = ap.parse_args()

import torch
from bench import CFG, make_opt
from unpaired_image_captioning_amd import _lib as L
from unpaired_image_captioning_amd import models
from unpaired_image_captioning_amd.synthetic import synthetic_batch
from unpaired_image_captioning_amd.topdown_engine import ensemble_logprobs

c = CFG
n_img = args.rows or c["n_img"]
BEAM = 3


def make_member(seed):
    m = models.setup(make_opt("bf16", seed)).cuda().eval()
    with torch.no_grad():        # a logit layer with some contrast, or every row decodes the same flat distribution
        lw = m.logit.weight if isinstance(m.logit, torch.nn.Linear) else m.logit[-1].weight
        lw.mul_(25.0)
    m.defer_status_check = True
    return m


def timeit(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


members = [make_member(1234 + i) for i in range(4)]
batch = {k: v.cuda() for k, v in synthetic_batch(n_img, 1, c["R"], c["D"], c["V"], c["L"], seed=1).items()}
fc, att, am = batch["fc_feats"], batch["att_feats"], batch.get("att_masks")
V1, Lsteps = c["V"] + 1, c["L"]
ldv = (V1 + 63) // 64 * 64 if V1 >= 1024 else (V1 + 7) // 8 * 8

print("%d images, %d regions, vocabulary %d, %d decode steps, bf16" % (n_img, c["R"], V1, Lsteps))
for M in (1, 2, 4):
    ens = models.AttEnsemble(members[:M]).eval()
    for label, opt, rows in (("greedy", {"sample_max": 1}, n_img), ("beam %d" % BEAM, {"beam_size": BEAM}, n_img * BEAM)):
        t = timeit(lambda: ens(fc, None, att, am, opt=opt, mode="sample"), args.iters)
        # the combining kernel alone on the decode's rows and leading dimension, in place over member 0 as the sequencers run it
        bufs = [torch.randn(rows, ldv, device="cuda") for _ in range(M)]
        views = [b[:, :V1] for b in bufs]
        tk = timeit(lambda: ensemble_logprobs(views, out=views[0]), 50)
        print("M = %d  %-7s %8.3f ms per decode   combine kernel %6.1f us x %d steps = %.3f ms (%.1f %%)" %
              (M, label, t, tk * 1e3, Lsteps, tk * Lsteps, 100.0 * tk * Lsteps / t))

# sanity: one member through the ensemble path against the model itself
m = members[0]
ens1 = models.AttEnsemble([m]).eval()
for label, opt in (("greedy", {"sample_max": 1}), ("beam %d" % BEAM, {"beam_size": BEAM})):
    m.engine.recurrence = L.REC_FWD_CHAIN
    seq_c, _ = m(fc, None, att, am, opt=opt, mode="sample")
    t_chain = timeit(lambda: m(fc, None, att, am, opt=opt, mode="sample"), args.iters)
    m.engine.recurrence = 0
    t_def = timeit(lambda: m(fc, None, att, am, opt=opt, mode="sample"), args.iters)
    seq_e, _ = ens1(fc, None, att, am, opt=opt, mode="sample")
    t_ens = timeit(lambda: ens1(fc, None, att, am, opt=opt, mode="sample"), args.iters)
    print("M = 1  %-7s ensemble path %.3f ms   model, launch chain %.3f ms   model, default path %.3f ms   tokens equal to the chain's: %s" %
          (label, t_ens, t_chain, t_def, bool((seq_e == seq_c).all())))
print("persistent status:", L.persistent_status())
