#!/usr/bin/env python3
"""Device time of the Transformer captioner's evaluation paths (models/TransformerModel.py over csrc/transformer.hip) at the real
widths -- d_model 512, d_ff 1300, 6 layers, 36 regions x 2048, V 9487, L 16 -- beside the CPU restatement of
tests/transformer_cases.py (f32, 16 threads) on the same inputs.

    python tools/transformer_eval_bench.py [--images 128] [--reps 10] [--dtypes bf16,f32] [--no-cpu]

Device time: HIP events around one call (encode / teacher-forced forward / greedy decode / beam 3), after a warm-up call of the
same shapes; the median of --reps repetitions.  Every call includes the encoder.  The figure to look at is greedy decode per
step against its launch count: embed + 11 launches per decoder layer (3 norms, 4 + 2 projections incl. the FFN, 2 attentions)
+ final norm + generator + sampling step."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    dev = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        dev.append(e0.elapsed_time(e1))
    return float(np.median(dev)), min(dev), max(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--dtypes", default="bf16,f32")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU restatement")
    a = ap.parse_args()
    import transformer_cases as TC
    from unpaired_image_captioning_amd import models
    c = dict(TC.REAL)
    n, R, D, L, V, N = a.images, c["R"], c["D"], c["L"], c["V"], c["N"]
    W = TC.make_weights(V + 1, D, c["d_model"], c["d_ff"], N, c["use_bn"], seed=c["seed"])
    g = torch.Generator().manual_seed(5)
    att = torch.randn(n, R, D, generator=g).abs()
    lens = torch.randint(10, R + 1, (n,), generator=g)
    lens[0] = R
    masks = (torch.arange(R)[None, :] < lens[:, None]).float()
    labels = torch.zeros(n, L + 2, dtype=torch.int64)
    labels[:, 1:L + 1] = torch.randint(1, V + 1, (n, L), generator=g)
    print("workload: %d images x %d regions x %d, d_model %d, d_ff %d, %d layers, V %d, L %d, use_bn %d"
          % (n, R, D, c["d_model"], c["d_ff"], N, V, L, c["use_bn"]))
    per_step = 1 + 11 * N + 3
    print("launches per greedy decode step: %d (embed + 11 x %d layers + norm + generator + sampling)" % (per_step, N))
    fc = torch.zeros(n, 8, device="cuda")
    att_d, masks_d, labels_d = att.cuda(), masks.cuda(), labels.cuda()
    for dtype in a.dtypes.split(","):
        opt = argparse.Namespace(vocab_size=V, input_encoding_size=c["d_model"], rnn_size=c["d_ff"], num_layers=N, drop_prob_lm=0.5,
                                 seq_length=L, att_feat_size=D, use_bn=c["use_bn"], caption_model="transformer", compute_dtype=dtype)
        m = models.setup(opt)
        m.load_state_dict(W, strict=True)
        m.cuda().eval()
        enc = timed(lambda: m.encode(att_d, masks_d), a.reps)
        fwd = timed(lambda: m(fc, None, att_d, labels_d, masks_d), a.reps)
        grd = timed(lambda: m(fc, None, att_d, masks_d, opt={"sample_max": 1}, mode="sample"), a.reps)
        bm3 = timed(lambda: m(fc, None, att_d, masks_d, opt={"beam_size": 3}, mode="sample"), a.reps)
        print("%-4s encode                %8.3f ms median (min %.3f, max %.3f)" % ((dtype,) + enc))
        print("%-4s teacher-forced forward %8.3f ms median (min %.3f, max %.3f)   [encoder included]" % ((dtype,) + fwd))
        print("%-4s greedy decode          %8.3f ms median (min %.3f, max %.3f)   [encoder included]; %.1f us per step beyond the encoder, "
              "%.2f us per launch" % ((dtype,) + grd + ((grd[0] - enc[0]) * 1e3 / L, (grd[0] - enc[0]) * 1e3 / L / per_step)))
        print("%-4s beam 3                 %8.3f ms median (min %.3f, max %.3f)   [encoder included, %d rows]" % ((dtype,) + bm3 + (3 * n,)))
        del m
    if not a.no_cpu:
        torch.set_num_threads(16)
        t0 = time.perf_counter()
        TC.encode(W, att, masks, N, c["use_bn"])
        t_enc = time.perf_counter() - t0
        t0 = time.perf_counter()
        TC.forward(W, att, masks, labels, N, c["use_bn"])
        t_fwd = time.perf_counter() - t0
        t0 = time.perf_counter()
        TC.sample_greedy(W, att, masks, L, N, c["use_bn"])
        t_grd = time.perf_counter() - t0
        print("CPU restatement (f32, %d threads): encode %.1f ms, teacher-forced forward %.1f ms, greedy decode %.1f ms "
              "(it re-decodes the whole prefix at every step, as the reference does)" % (torch.get_num_threads(), t_enc * 1e3, t_fwd * 1e3, t_grd * 1e3))


if __name__ == "__main__":
    main()
