#!/usr/bin/env python3
"""Golden vectors for the language evaluation of the validation pass (eval_utils.language_eval, 'zh' branch) from the
REFERENCE's own scorers: AI_Challenger/Evaluation/caption_eval/coco_caption/pycxevalcap/{bleu,rouge,cider}/ -- the three that
pycxevalcap/eval.py runs -- fed strings of token ids (python 2 sources: run through lib2to3 in memory, see
make_golden_cider.py).  A caption's words are its tokens BEFORE the first 0.  Build container only; run by hand.

    python tests/golden/make_golden_lang_eval.py        # writes tests/golden/lang_eval_*.npz
"""
import ast
import contextlib
import io
import os
import sys
import types

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_cider as mc
import lang_eval_cases as LC

E = os.path.join(mc.P, "AI_Challenger", "Evaluation", "caption_eval", "coco_caption", "pycxevalcap")


def load_scorers():
    for name in ("coco_caption", "coco_caption.pycxevalcap", "coco_caption.pycxevalcap.bleu", "coco_caption.pycxevalcap.rouge",
                 "coco_caption.pycxevalcap.cider"):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    pre = "coco_caption.pycxevalcap."
    mc.load_py2(pre + "bleu.bleu_scorer", os.path.join(E, "bleu", "bleu_scorer.py"))
    bleu = mc.load_py2(pre + "bleu.bleu", os.path.join(E, "bleu", "bleu.py"))
    rouge = mc.load_py2(pre + "rouge.rouge", os.path.join(E, "rouge", "rouge.py"))
    mc.load_py2(pre + "cider.cider_scorer", os.path.join(E, "cider", "cider_scorer.py"))
    cider = mc.load_py2(pre + "cider.cider", os.path.join(E, "cider", "cider.py"))
    return bleu.Bleu, rouge.Rouge, cider.Cider


def sentence(row):
    return " ".join(str(t) for t in LC.words(row))


def save(name, scorers, hyp, ref_tok, ref_start):
    Bleu, Rouge, Cider = scorers
    n = len(hyp)
    res = {i: [sentence(hyp[i])] for i in range(n)}
    gts = {i: [sentence(r) for r in ref_tok[ref_start[i]:ref_start[i + 1]]] for i in range(n)}
    assert all(len(s) > 0 for v in gts.values() for s in v), "references have at least one word"
    out = io.StringIO()
    with contextlib.redirect_stdout(out):                                   # Bleu prints its totals (verbose=1)
        corpus_bleu, bleu = Bleu(4).compute_score(gts, res)
    printed = ast.literal_eval(out.getvalue().splitlines()[0])
    corpus_rouge, rouge = Rouge().compute_score(gts, res)
    corpus_cider, cider = Cider().compute_score(gts, res)
    mine = LC.evaluate(hyp, ref_tok, ref_start)                              # the ten totals, recomputed from the inputs
    totals = mine["totals"]
    assert list(totals[0:4]) == printed["correct"] and list(totals[4:8]) == printed["guess"], (totals, printed)
    assert int(totals[8]) == printed["testlen"] and int(totals[9]) == printed["reflen"], (totals, printed)
    corpus = np.array(list(corpus_bleu) + [corpus_rouge, corpus_cider], dtype=np.float64)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, hyp=hyp, ref_tok=ref_tok, ref_start=np.asarray(ref_start, dtype=np.int32),
                        bleu=np.asarray(bleu, dtype=np.float64), rouge=np.asarray(rouge, dtype=np.float64),
                        cider=np.asarray(cider, dtype=np.float64), corpus=corpus, totals=np.asarray(totals, dtype=np.int64))
    print("wrote %s (%.1f KB): %s, length ratio %.3f" % (path, os.path.getsize(path) / 1024,
                                                         " ".join("%s %.4f" % kv for kv in zip(LC.KEYS, corpus)),
                                                         totals[8] / float(totals[9])))
    return corpus, totals


def tiny(scorers):
    """V 10, L = Lr = 8, 9 images with 1 to 7 references; see the asserts for what the hypotheses cover."""
    g = np.random.default_rng(31)
    V, L = 10, 8
    counts = [3, 7, 1, 2, 5, 4, 6, 2, 3]
    ref_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    ref_tok = np.zeros((ref_start[-1], L), dtype=np.int64)
    for r in range(len(ref_tok)):
        ln = int(g.integers(4, L + 1))
        ref_tok[r, :ln] = np.minimum(g.integers(1, V + 1, ln), g.integers(1, V + 1, ln))
    lo, hi = ref_start[4], ref_start[5]
    ref_tok[lo:hi] = np.where(ref_tok[lo:hi] > 0, (ref_tok[lo:hi] - 1) % 5 + 1, 0)      # image 4: tokens 1..5 only
    ref_tok[ref_start[:-1], 0] = 1                        # token 1 in a reference of every image: its unigram idf is 0
    hyp = np.zeros((9, L), dtype=np.int64)
    for i in range(9):
        ln = int(g.integers(2, 6))
        hyp[i, :ln] = np.minimum(g.integers(1, V + 1, ln), g.integers(1, V + 1, ln))
    hyp[0] = 0                                            # an empty caption
    hyp[1] = ref_tok[ref_start[1] + 3]                    # an exact copy of a reference (the image with 7)
    hyp[2] = g.integers(1, V + 1, L)                      # a row with no 0: 8 words
    hyp[3] = 0
    hyp[3, :5] = ref_tok[ref_start[3], 1]                 # one word repeated
    hyp[4] = 0
    hyp[4, :4] = g.integers(6, V + 1, 4)                  # shares no token with its references
    hyp[5, 0] = 1                                         # a caption whose only known unigram has idf 0
    corpus, totals = save("lang_eval_tiny", scorers, hyp, ref_tok, ref_start)
    assert totals[8] < totals[9], "the brevity penalty applies"
    assert max(counts) == 7 and min(counts) == 1
    assert all((ref_tok[ref_start[i]:ref_start[i + 1]] == 1).any() for i in range(9))
    assert not set(LC.words(hyp[4])) & set(t for r in ref_tok[lo:hi] for t in LC.words(r))


def long_rows(scorers):
    """V 6, L = Lr = 64: every hypothesis 64 words, long common subsequences over a small alphabet (bit 63, the carry out)."""
    g = np.random.default_rng(32)
    V, L = 6, 64
    counts = [2, 3, 1, 4]
    ref_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    ref_tok = np.zeros((ref_start[-1], L), dtype=np.int64)
    for r in range(len(ref_tok)):
        ln = L if r in (0, 2, 5, 6, 8) else int(g.integers(40, L + 1))
        ref_tok[r, :ln] = g.integers(1, V + 1, ln)
    hyp = g.integers(1, V + 1, (4, L)).astype(np.int64)
    hyp[1, 20:] = ref_tok[ref_start[1], 20:]              # a long shared tail that ends in the last position
    hyp[2, -1] = ref_tok[ref_start[2], -1]
    corpus, totals = save("lang_eval_long", scorers, hyp, ref_tok, ref_start)
    assert totals[8] >= totals[9] and (hyp > 0).all()


def real_shape(scorers):
    hyp, ref_tok, ref_start = LC.random_case(33, V=60, L=16, Lr=16, n_img=12, n_refs=5)
    save("lang_eval_real_shape", scorers, hyp, ref_tok, ref_start)


def main():
    scorers = load_scorers()
    tiny(scorers)
    long_rows(scorers)
    real_shape(scorers)


if __name__ == "__main__":
    main()
