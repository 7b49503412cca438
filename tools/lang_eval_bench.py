#!/usr/bin/env python3
"""Device time of one language evaluation (misc/lang_eval.py: Bleu(4), Rouge(), Cider() on token rows) at the Karpathy `val`
size, beside the one-off document-frequency table build and the CPU restatement of the same scorers on the same rows.

    python tools/lang_eval_bench.py [--images 5000] [--refs 5] [--length 16] [--vocab 9487] [--reps 20] [--no-cpu]

Device time: HIP events around DeviceLanguageEval.score (the three scorer launches, the reduction and the read-back), after a
warm-up call of the same shapes; the median of --reps repetitions.  Prints one line per figure."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--refs", type=int, default=5)
    ap.add_argument("--length", type=int, default=16)
    ap.add_argument("--vocab", type=int, default=9487)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU restatement (about 10 s at the default size)")
    a = ap.parse_args()
    import lang_eval_cases as LC
    from unpaired_image_captioning_amd.misc import lang_eval
    hyp, ref_tok, ref_start = LC.random_case(1, a.vocab, a.length, a.length, a.images, a.refs)
    print("workload: %d images x %d references, L %d, V %d" % (a.images, a.refs, a.length, a.vocab))

    t0 = time.perf_counter()
    keys, counts = lang_eval.document_frequency(ref_tok, ref_start)
    t_df = time.perf_counter() - t0
    ev = lang_eval.DeviceLanguageEval.from_references(ref_tok, ref_start)
    ix = np.arange(a.images)
    hyp_d = torch.from_numpy(hyp).cuda()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    overall, _ = ev.score(ix, hyp_d)                    # builds and uploads the table, and warms every shape up
    torch.cuda.synchronize()
    t_first = time.perf_counter() - t0
    print("table: %d n-grams; host count %.1f ms; first score() with table build and upload %.1f ms" % (len(keys), t_df * 1e3, t_first * 1e3))

    dev, wall = [], []
    for _ in range(max(a.reps, 20)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        again, _ = ev.score(ix, hyp_d)
        e1.record()
        e1.synchronize()
        wall.append(time.perf_counter() - t0)
        dev.append(e0.elapsed_time(e1))
        assert again == overall and ev.tables_built == 1
    print("score(): device %.3f ms median (min %.3f, max %.3f) over %d repetitions; host wall %.3f ms median"
          % (np.median(dev), min(dev), max(dev), len(dev), np.median(wall) * 1e3))
    print("lang_stats: " + " ".join("%s %.4f" % (k, overall[k]) for k in LC.KEYS))

    if not a.no_cpu:
        t0 = time.perf_counter()
        want = LC.evaluate(hyp, ref_tok, ref_start)
        t_cpu = time.perf_counter() - t0
        err = max(abs(overall[k] - w) for k, w in zip(LC.KEYS, want["corpus"]))
        print("CPU restatement of the three scorers on the same rows: %.2f s (largest difference of the six values %.2e)" % (t_cpu, err))


if __name__ == "__main__":
    main()
