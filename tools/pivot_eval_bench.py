#!/usr/bin/env python3
"""One COCO-half batch of the unpaired validation pass at BASELINE configs[2]'s shape: 64 images -> im2zh TopDown captioner
(beam 3) -> pivot caption -> zh->en NMT (beam 15) -> English rows -> Bleu / ROUGE_L / CIDEr against 5 references per image,
bf16, random weights of the real shapes (36 x 2048 features, hidden 512, caption vocabulary 9 487, NMT vocabularies 50 004).

Two ways through the same models, in one process, alternating, medians of --reps:

  device   PivotBridge.pivot (uic_pivot_source, uic_nmt_translate, uic_pivot_target) and DeviceLanguageEval.score: the host
           waits for max_len, the translator's stop checks and the six numbers
  host     what the glue was before the bridge: decode, .cpu(), decode_sequence + a Python dictionary lookup per word,
           translateBatch, its Python lists, buildTargetTokens on words (one .cpu() of a sentence's attention), a Python lookup
           into the scored vocabulary, upload, DeviceLanguageEval.score

The device path runs as two interleaved series (a, b) of the same code: their difference is the spread a difference between the
paths has to exceed.  Random weights rarely emit EOS, so the translator runs --nmt-steps steps (default 30, a typical sentence)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn as nn

import bench
from unpaired_image_captioning_amd import models
from unpaired_image_captioning_amd.misc import utils
from unpaired_image_captioning_amd.misc.lang_eval import DeviceLanguageEval
from unpaired_image_captioning_amd.misc.pivot import EOS, UNK, PivotBridge
from unpaired_image_captioning_amd.models import NMT_Models
from unpaired_image_captioning_amd.synthetic import synthetic_batch

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--beam", type=int, default=3)
ap.add_argument("--nmt-steps", type=int, default=30)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--unk-bias", type=float, default=2.0, help="added to the generator's UNK bias: 2.0 makes every word of these random "
                "weights' hypotheses an UNK (the copy branch, one attention read-back per sentence on the host path), 0 none (the table branch)")
ap.add_argument("--out", default=None, help="also append the report to this file")
a = ap.parse_args()
c = bench.CFG
torch.manual_seed(1)
cap = models.setup(bench.make_opt("bf16", 1)).cuda().eval()
V = 50004
SPECIALS = ['<blank>', '<unk>', '<s>', '</s>']
caption_vocab = {str(i + 1): "zh%d" % i for i in range(c["V"])}
scoring_vocab = {str(i + 1): "en%d" % i for i in range(c["V"])}
# the source dictionary knows 9 of 10 caption words, the scored vocabulary 1 of 5 target words: every branch of the glue runs
src_words = SPECIALS + ["zh%d" % i for i in range(c["V"]) if i % 10] + ["zz%d" % i for i in range(V)]
tgt_words = SPECIALS + ["en%d" % (i // 5) if i % 5 == 0 else "xx%d" % i for i in range(V)]
src_l2i = {w: i for i, w in enumerate(src_words[:V])}
tgt_i2l = dict(enumerate(tgt_words[:V]))
score_l2i = {w: int(k) for k, w in scoring_vocab.items()}
OOV = len(scoring_vocab) + 1
opt = argparse.Namespace(layers=2, rnn_size=512, word_vec_size=512, brnn=True, rnn_type="LSTM", dropout=0.3, input_feed=1,
                         position_encoding=False, coverage_attn=False, copy_attn=False, context_gate=None, attention_type="dot",
                         attn_transform="softmax", fertility=None, predict_fertility=False, guided_fertility=None,
                         supervised_fertility=None, lambda_coverage=0, lambda_fertility=0, lambda_exhaust=0, batch_size=a.batch,
                         gpus=[0], compute_dtype="bf16", seed=1)
nmt = NMT_Models.NMTModel(opt, NMT_Models.Encoder(opt, V), NMT_Models.Decoder(opt, V), src_l2i, tgt_i2l, False)
nmt.generator = nn.Sequential(nn.Linear(512, V), nn.LogSoftmax(dim=-1))
nmt.cuda().eval()
with torch.no_grad():
    nmt.generator[0].bias[UNK] += a.unk_bias
b = synthetic_batch(a.batch, 1, c["R"], c["D"], c["V"], c["L"], seed=5)
g = np.random.default_rng(7)
refs = g.integers(1, c["V"] + 1, size=(a.batch * 5, c["L"])).astype(np.int64)
scorer = DeviceLanguageEval.from_references(refs, np.arange(a.batch + 1) * 5)
image_ix = np.arange(a.batch)
bridge = PivotBridge(caption_vocab, src_l2i, tgt_i2l, scoring_vocab)
L_OUT = bridge.max_words


def caption():
    with torch.no_grad():
        return cap(b["fc_feats"], None, b["att_feats"], b["att_masks"], opt={"beam_size": a.beam}, mode="sample")[0]


def device_path():
    out, out_len, _ = bridge.pivot(caption(), nmt, max_steps=a.nmt_steps)
    return scorer.score(image_ix, out)[0], out


def host_path():
    seq = caption()
    sents = [s.split() for s in utils.decode_sequence(caption_vocab, seq)]                 # the .cpu() of the captions
    sents = [s if s else ['<unk>'] for s in sents]
    S = max(len(s) for s in sents)
    src = torch.zeros(S, a.batch, dtype=torch.int64)
    for k, s in enumerate(sents):
        src[:len(s), k] = torch.tensor([src_l2i.get(w, UNK) for w in s])
    allHyp, _, allAttn, _ = nmt.translateBatch(argparse.Namespace(src=src.cuda().unsqueeze(2), batchSize=a.batch), max_steps=a.nmt_steps)
    rows = np.zeros((a.batch, L_OUT), dtype=np.int64)
    for k in range(a.batch):
        pred, attn = allHyp[k][0], None
        tokens = [tgt_i2l[t] for t in (pred[:pred.index(EOS) + 1] if EOS in pred else pred)][:-1]   # convertToLabels(..)[:-1]
        for i in range(len(tokens)):
            if tokens[i] == '<unk>':
                if attn is None:
                    attn = allAttn[k][0].cpu()
                tokens[i] = sents[k][int(attn[i].argmax())]
        ids = [score_l2i.get(w, OOV) for w in tokens[:L_OUT]]
        rows[k, :len(ids)] = ids
    out = torch.from_numpy(rows).cuda()
    return scorer.score(image_ix, out)[0], out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


for _ in range(2):                                   # warm every shape of both paths
    stats_d, out_d = device_path()
    stats_h, out_h = host_path()
same = bool(torch.equal(out_d, out_h))
shape = "translator steps taken %d, source width %d, %d words in the %d rows, %d of them copied pivot words" % (
    bridge.last["n"], bridge.last["src"].shape[0], int((out_d != 0).sum()), a.batch, int((bridge.last["repl"] >= 0).sum()))
series = {"device a": [], "host": [], "device b": []}
for _ in range(a.reps):
    series["device a"].append(timed(device_path)[0])
    series["host"].append(timed(host_path)[0])
    series["device b"].append(timed(device_path)[0])
med = {k: float(np.median(v)) for k, v in series.items()}
lines = ["workload: %d images, captioner beam %d (L %d, V %d), translator beam 15 x %d steps (V %d), 5 references per image, bf16, UNK bias %+.1f"
         % (a.batch, a.beam, c["L"], c["V"], a.nmt_steps, V, a.unk_bias), shape,
         "one COCO-half batch, decode to lang_stats, wall ms, median of %d (min .. max), paths alternating in one process:" % a.reps]
for k in ("device a", "device b", "host"):
    lines.append("  %-9s %8.2f  (%.2f .. %.2f)" % (k, med[k], min(series[k]), max(series[k])))
lines.append("spread between the two device series (same code): %.2f ms = %.2f %%"
             % (abs(med["device a"] - med["device b"]), 100 * abs(med["device a"] - med["device b"]) / med["device a"]))
lines.append("host - device: %.2f ms of %.2f" % (med["host"] - 0.5 * (med["device a"] + med["device b"]), med["host"]))
lines.append("rows of the two paths identical: %s; CIDEr %.6f / %.6f, Bleu_1 %.6f / %.6f"
             % (same, stats_d["CIDEr"], stats_h["CIDEr"], stats_d["Bleu_1"], stats_h["Bleu_1"]))
report = "\n".join(lines)
print(report)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(report + "\n\n")
