#!/usr/bin/env python3
"""The optimizer launch of every --i2t_optim / --nmt_optim method (csrc/adam.hip) at the two arena sizes a user runs: the
captioner's (19.7 M elements) and the pivot NMT model's (90 M).  Whole-arena launch (uic_optim_step) and ranges launch
(uic_optim_step_ranges: five ranges that cover the arena, as the sharded exchange's four pieces + tail), HIP events around every
launch, each method's launch alternating with the Adam launch in the same call, median over --reps after --warmup.  Bytes:
4 B x (p read + p written + g read + 2 x state arrays) per element -- sgd 12, one-state methods 20, Adam 28.
    python tools/optim_bench.py [--reps 30] [--warmup 5] [--weight-decay 0]
    python tools/optim_bench.py --yardstick <another build's libuic_hip.so>      # only: that build's uic_adam_step alternating with this
                                                                                 # build's, in one process (both libraries loaded)"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--weight-decay", type=float, default=0.0)
ap.add_argument("--yardstick", metavar="LIB", default="", help="another build's libuic_hip.so: time its uic_adam_step against this build's")
ap.add_argument("--sizes", type=int, nargs="+", default=[19_700_000, 90_000_000])
args = ap.parse_args()

import torch
from unpaired_image_captioning_amd import _lib as L

lib = L.load()
other = None
if args.yardstick:
    other = C.CDLL(args.yardstick)
    other.uic_adam_step.restype, other.uic_adam_step.argtypes = L._SIGS["uic_adam_step"]
LR, ALPHA, BETA, EPS = 5e-4, 0.9, 0.999, 1e-8
STATES = {"adam": 2, "sgd": 0, "sgdm": 1, "sgdmom": 1, "rmsprop": 1, "adagrad": 1}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def report(label, n, states, us):
    nbytes = 4 * n * (3 + 2 * states)
    med = statistics.median(us)
    print("%-34s n %9d: median %8.1f us  (min %8.1f, max %8.1f)  %6.2f TB/s over %d B/element"
          % (label, n, med, min(us), max(us), nbytes / med * 1e-6, 4 * (3 + 2 * states)), flush=True)


for n in args.sizes:
    g = torch.Generator(device="cuda").manual_seed(n % 1000)
    p = torch.randn(n, device="cuda", generator=g)
    gr = torch.randn(n, device="cuda", generator=g) * 1e-2
    s0, s1 = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")          # Adam's moments
    st = torch.zeros(n, device="cuda")                                               # the one-state methods' array
    step = [0]

    def adam_step(which):
        step[0] += 1
        rc = which.uic_adam_step(L.ptr(p), L.ptr(gr), L.ptr(s0), L.ptr(s1), n, LR, ALPHA, BETA, EPS, step[0], 1.0, L.stream())
        if rc != 0:
            raise RuntimeError("uic_adam_step failed (rc=%d)" % rc)

    if other is not None:
        for _ in range(args.warmup):
            adam_step(other)
            adam_step(lib)
        ev = [(timed(lambda: adam_step(other)), timed(lambda: adam_step(lib))) for _ in range(args.reps)]
        torch.cuda.synchronize()
        report("uic_adam_step, the yardstick build", n, 2, [a.elapsed_time(b) * 1e3 for (a, b), _ in ev])
        report("uic_adam_step, this build", n, 2, [a.elapsed_time(b) * 1e3 for _, (a, b) in ev])
        del p, gr, s0, s1, st
        continue
    # five ranges that cover the arena: four pieces of a quarter each (64-element units) + the tail
    q = n // 4 // 64 * 64
    bounds = [0, q, 2 * q, 3 * q, 4 * q, n]
    lo = (C.c_uint64 * 5)(*bounds[:-1])
    hi = (C.c_uint64 * 5)(*bounds[1:])

    def launch(method, ranges):
        step[0] += 1
        cfg = L.OptimConfig(L.OPTIM_METHODS[method], LR, ALPHA, BETA, 1e-10 if method == "adagrad" else EPS, args.weight_decay, step[0], 1.0,
                            0.0, None, None)
        a0, a1 = (L.ptr(s0), L.ptr(s1)) if method == "adam" else (L.ptr(st), None)
        if ranges:
            L.check(lib.uic_optim_step_ranges(C.byref(cfg), L.ptr(p), L.ptr(gr), a0, a1, 5, lo, hi, None, 0, L.stream()), "optim_step_ranges")
        else:
            L.check(lib.uic_optim_step(C.byref(cfg), L.ptr(p), L.ptr(gr), a0, a1, n, L.stream()), "optim_step")

    for ranges in (False, True):
        for method in ("adam", "sgd", "sgdm", "sgdmom", "rmsprop", "adagrad"):
            st.zero_()
            for _ in range(args.warmup):
                launch(method, ranges)
                launch("adam", ranges)
            ev = []
            for _ in range(args.reps):
                ev.append((timed(lambda: launch(method, ranges)), timed(lambda: launch("adam", ranges))))
            torch.cuda.synchronize()
            form = "ranges" if ranges else "whole"
            wd = " wd" if args.weight_decay else ""
            report("%s %s%s" % (method, form, wd), n, STATES[method], [a.elapsed_time(b) * 1e3 for (a, b), _ in ev])
            report("   adam beside it (%s)" % form, n, 2, [a.elapsed_time(b) * 1e3 for _, (a, b) in ev])
    del p, gr, s0, s1, st
