#!/usr/bin/env python3
"""Golden data for the pivot bridge (misc/pivot.py, csrc/pivot.hip) from the REFERENCE's own code: ``onmt.Dict`` (convertToIdx,
convertToLabels; the vendored OpenNMT fork's Dict.py) and ``NMTModel.buildTargetTokens`` (models/NMT_Models.py:312-320), called
on a stub that holds ``tgt_dict`` only.

Build-container only.  Harness-side shims as in make_golden_nmt.py (reference files untouched).  Under this torch
``attn[i].max(0)`` followed by ``maxIndex[0]`` needs rows shaped [S, 1] (in the reference's torch 0.3, max(0) of a vector kept a
dimension), so the attention is handed over as [steps, S, 1]; `build_target_tokens_ran` in the fixture says whether the
reference's function itself produced the expected tokens.

Writes tests/golden/pivot_dict.json: data only -- words, dictionary contents, expected ids and tokens.

    python tests/golden/make_golden_pivot.py
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_nmt as G                                     # noqa: E402


def cases():
    """(name, src words in the dictionary, lower, sentence, tgt words, pred ids, attention [steps, S])."""
    g = np.random.default_rng(5)
    src_words = ['yi', 'ge', 'Ren', 'zai', 'chi', 'fan', 'gou']
    tgt_words = ['a', 'man', 'is', 'eating', 'dog', 'food', 'The']
    out = []

    def attn(steps, S, peaks=None):
        a = g.random((steps, S)).astype(np.float32)
        for i, j in (peaks or {}).items():
            a[i] = 0.01
            a[i, j] = 0.9
        return a
    # ids of tgt words: specials 0..3, then 4..
    out.append(('plain', src_words, False, ['yi', 'ge', 'Ren', 'zai', 'chi', 'fan'], tgt_words, [4, 5, 6, 7, 3], attn(5, 6)))
    out.append(('unknown_words', src_words, False, ['yi', 'zhi', 'mao', 'zai', 'chi'], tgt_words, [4, 1, 6, 7, 3, 9, 9], attn(7, 5, {1: 2})))
    out.append(('lower', src_words, True, ['YI', 'Ge', 'ren', 'REN', 'Mao'], tgt_words, [10, 5, 3], attn(3, 5)))
    out.append(('unk_in_hypothesis', src_words, False, ['gou', 'chi', 'fan', 'xx'], tgt_words, [1, 6, 1, 1, 3], attn(5, 4, {0: 3, 2: 0, 3: 1})))
    out.append(('unk_attention_tie', src_words, False, ['gou', 'chi', 'fan'], tgt_words, [1, 5, 3], np.full((3, 3), 0.25, dtype=np.float32)))
    out.append(('no_eos', src_words, False, ['yi', 'ge', 'gou'], tgt_words, [4, 8, 6, 7, 9], attn(5, 3)))
    out.append(('no_eos_unk_last', src_words, False, ['yi', 'ge', 'gou'], tgt_words, [4, 8, 1], attn(3, 3, {2: 1})))
    out.append(('eos_first', src_words, False, ['yi', 'ge'], tgt_words, [3, 4, 5], attn(3, 2)))
    out.append(('one_step_no_eos', src_words, False, ['yi'], tgt_words, [4], attn(1, 1)))
    return out


def main():
    nmt, _ = G.load_reference()
    import onmt
    O = G.O
    onmt.Dict = G.load("onmt.Dict", os.path.join(O, "Dict.py")).Dict
    C = onmt.Constants
    specials = [C.PAD_WORD, C.UNK_WORD, C.BOS_WORD, C.EOS_WORD]
    fixture = {"constants": {"PAD": C.PAD, "UNK": C.UNK, "BOS": C.BOS, "EOS": C.EOS, "words": specials}, "cases": []}
    ran = True
    for name, src_words, lower, sentence, tgt_words, pred, attn in cases():
        sd = onmt.Dict(specials, lower=lower)
        for w in src_words:
            sd.add(w)
        td = onmt.Dict(specials, lower=False)
        for w in tgt_words:
            td.add(w)
        ids = [int(x) for x in sd.convertToIdx(sentence, C.UNK_WORD)]
        labels = td.convertToLabels(pred, C.EOS)
        stub = types.SimpleNamespace(tgt_dict=td)
        try:
            tokens = nmt.NMTModel.buildTargetTokens(stub, pred, sentence, torch.from_numpy(attn).unsqueeze(2))
            tokens = [str(t) for t in tokens]
        except Exception as e:                                   # restate (and say so) if this torch cannot run it
            print("buildTargetTokens failed on %s: %r" % (name, e))
            ran = False
            tokens = labels[:-1]
            for i in range(len(tokens)):
                if tokens[i] == C.UNK_WORD:
                    tokens[i] = sentence[int(np.argmax(attn[i]))]
        fixture["cases"].append({
            "name": name, "lower": lower,
            "src_dict": {w: int(i) for w, i in sd.labelToIdx.items()},
            "tgt_dict": {w: int(i) for w, i in td.labelToIdx.items()},
            "sentence": sentence, "src_ids": ids,
            "pred": [int(p) for p in pred], "attn": [[float(x) for x in row] for row in attn],
            "labels": labels, "tokens": tokens})
    fixture["build_target_tokens_ran"] = ran
    with open(os.path.join(HERE, "pivot_dict.json"), "w") as f:
        json.dump(fixture, f, indent=1, ensure_ascii=True)
    print("wrote pivot_dict.json: %d cases, buildTargetTokens ran: %s" % (len(fixture["cases"]), ran))


if __name__ == "__main__":
    main()
