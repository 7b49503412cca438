#!/usr/bin/env python3
"""uic_topdown_batch.unfinished_count (the BPTT loop's d x GEMMs over the unfinished captions only) against the same step without
it, in ONE process on one box -- the field is a run-time argument, so one build runs both:
  1. two trainers from the same weights train on the benchmark batch side by side: the losses must be EQUAL, step by step (the
     change is bit-exact);
  2. blocks of steps alternate between the batch without the counts ("full") and with them ("rows"): ms per step of every block,
     pair by pair; the step's own marks (uic_topdown_step_marks) of the last step of either kind.
    python tools/unfinished_ab.py [--steps 300] [--pairs 4] [--settle 3000]"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--pairs", type=int, default=4)
ap.add_argument("--trajectory", type=int, default=20)
ap.add_argument("--settle", type=int, default=3000, help="untimed steps in front of the pairs: the chip's clocks settle over the first seconds of load, "
                "which otherwise shows as a drift across the pairs of one setting")
args = ap.parse_args()

import torch
import bench
from unpaired_image_captioning_amd import _lib as L
from unpaired_image_captioning_amd.synthetic import synthetic_batch
from unpaired_image_captioning_amd.trainer import Trainer

c = bench.CFG
batch = {k: v.cuda() for k, v in synthetic_batch(c["n_img"], c["S"], c["R"], c["D"], c["V"], c["L"], seed=1234).items()}
rows = Trainer.attach_live(dict(batch))
full = {k: v for k, v in rows.items() if k != "unfinished_count"}
T = batch["labels"].shape[1] - 1
den = float(batch["masks"][:, 1:T + 1].sum().item())
print("rows %d, unfinished per step %s" % (batch["labels"].shape[0], rows["unfinished_count"].tolist()))

if args.trajectory:
    trs = []
    for _ in range(2):
        torch.manual_seed(1234)
        tr = Trainer(bench.make_opt("bf16", 1234))
        tr.build_optimizer()
        trs.append(tr)
    t_run = trs[0].i2t_model._steps_to_run(batch["labels"])
    same = True
    for i in range(args.trajectory):
        la = trs[0].train_device_batch(full, t_run, den).item()
        lb = trs[1].train_device_batch(rows, t_run, den).item()
        same = same and la == lb
    print("trajectory of %d steps: last loss full %.9f rows %.9f, equal at every step: %s" % (args.trajectory, la, lb, same))
    del trs

tr = Trainer(bench.make_opt("bf16", 1234))
tr.build_optimizer()
t_run = tr.i2t_model._steps_to_run(batch["labels"])
lib = L.load()
for i in range(args.settle):
    tr.train_device_batch(rows if i & 1 else full, t_run, den)
torch.cuda.synchronize()
res = {"full": [], "rows": []}
marks = {}
for r in range(args.pairs + 1):                      # (the first pair warms up and is dropped)
    for name, b in (("full", full), ("rows", rows)):
        for _ in range(5):
            tr.train_device_batch(b, t_run, den)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            tr.train_device_batch(b, t_run, den)
        torch.cuda.synchronize()
        if r:
            res[name].append((time.perf_counter() - t0) / args.steps * 1e3)
        L.check(lib.uic_topdown_step_marks(1, None))
        ms = (C.c_float * 16)()
        acc = [0.0] * 16
        for _ in range(20):
            tr.train_device_batch(b, t_run, den)
            L.check(lib.uic_topdown_step_marks(1, ms))
            acc = [a + m for a, m in zip(acc, ms)]
        L.check(lib.uic_topdown_step_marks(0, None))
        marks[name] = [a / 20 for a in acc]
n = C.c_int32(0)
L.check(lib.uic_topdown_compact_launches(C.byref(n)))
print("compact d x launches of the last step with the counts: %d" % n.value)
for i, (a, b) in enumerate(zip(res["full"], res["rows"])):
    print("pair %d: full %.4f ms  rows %.4f ms  diff %+.4f ms (%+.2f %%)" % (i, a, b, b - a, 100.0 * (b - a) / a))
fa, ra = res["full"], res["rows"]
print("mean full %.4f (spread %.4f)  mean rows %.4f (spread %.4f)  mean diff %+.4f ms" %
      (sum(fa) / len(fa), max(fa) - min(fa), sum(ra) / len(ra), max(ra) - min(ra), sum(ra) / len(ra) - sum(fa) / len(fa)))
for name in ("full", "rows"):
    m = marks[name]
    print("%-5s marks (ms from the step's start, mean of 20): recurrence %.3f-%.3f  BPTT window %.3f-%.3f = %.3f  main tail %.3f  side %.3f  join %.3f"
          % (name, m[1], m[2], m[4], m[5], m[5] - m[4], m[7], m[8], m[9]))
L.persistent_status()
