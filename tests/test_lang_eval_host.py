"""Language evaluation, host side (no GPU): the CPU restatement of Bleu(4) / Rouge() / Cider() on token rows
(tests/lang_eval_cases.py) equals the reference scorers' own numbers (tests/golden/lang_eval_*.npz), the vectorised
document-frequency table equals a brute-force count, and the C ABI declares and exports the new entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lang_eval_cases as LC
from conftest import GOLDEN, ROOT

FIXTURES = ("lang_eval_tiny", "lang_eval_long", "lang_eval_real_shape")
NEW_EXPORTS = ("uic_langeval_cider", "uic_langeval_bleu", "uic_langeval_rouge_l", "uic_langeval_reduce")


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_equals_the_reference_scorers(name):
    z = load(name)
    got = LC.evaluate(z["hyp"], z["ref_tok"], z["ref_start"])
    for k in ("bleu", "rouge", "cider"):
        assert got[k].shape == z[k].shape
        assert np.abs(got[k] - z[k]).max() <= 1e-12, k
    assert np.array_equal(got["totals"], z["totals"])
    assert np.array_equal(got["corpus"][:4], z["corpus"][:4])            # the same expression on the same integers
    assert np.abs(got["corpus"][4:] - z["corpus"][4:]).max() <= 1e-12


@pytest.mark.parametrize("name", FIXTURES)
def test_host_corpus_bleu_is_the_scorers_expression(name):
    from unpaired_image_captioning_amd.misc.lang_eval import corpus_bleu
    z = load(name)
    assert np.array_equal(np.array(corpus_bleu(z["totals"])), z["corpus"][:4])


def test_fixtures_cover_what_they_are_for():
    z = load("lang_eval_tiny")
    counts = np.diff(z["ref_start"])
    assert counts.max() == 7 and counts.min() == 1 and len(counts) == 9       # two rounds of the six-wave kernel, and one reference
    assert (z["hyp"][0] == 0).all() and z["rouge"][0] == 0 and z["cider"][0] == 0
    assert (z["hyp"] > 0).all(1).any()                                          # a row with no 0
    assert (z["rouge"] == 0).sum() >= 2                                         # the empty caption and the one without a shared token
    assert z["totals"][8] < z["totals"][9]                                      # the brevity penalty applies
    assert z["bleu"][:, 1].max() > 0.999 and z["rouge"][1] == 1.0               # the exact copy
    z = load("lang_eval_long")
    assert z["hyp"].shape[1] == 64 and (z["hyp"] > 0).all() and z["totals"][8] >= z["totals"][9]


def test_bitvector_lcs_equals_the_table():
    """The recurrence of csrc/cider.hip::rouge_l_kernel on one 64-bit word, lengths 0..64 (64: the sum carries out of the word)."""
    g = np.random.default_rng(5)
    for trial in range(600):
        V = int(g.choice([1, 2, 3, 6, 40]))
        la, lb = (64, 64) if trial % 10 == 0 else (int(g.integers(0, 65)), int(g.integers(0, 65)))
        a, b = list(g.integers(1, V + 1, la)), list(g.integers(1, V + 1, lb))
        assert LC.lcs_bitvector(a, b) == LC.lcs(a, b), (a, b)


@pytest.mark.parametrize("seed,V,Lr,n_img,n_refs", [(0, 4, 8, 7, 3), (1, 30, 5, 12, 1), (2, 70000, 6, 5, 4), (3, 9, 3, 4, 2), (4, 5, 1, 3, 2)])
def test_host_df_table_equals_a_brute_force_count(seed, V, Lr, n_img, n_refs):
    from unpaired_image_captioning_amd.misc.lang_eval import document_frequency
    _, ref_tok, ref_start = LC.random_case(seed, V, 4, Lr, n_img, n_refs)
    if V > 0xFFFF:
        ref_tok[0, 0] = V                                                      # a token past 16 bits: the general path
    keys, counts = document_frequency(ref_tok, ref_start)
    want = LC.document_frequency([[LC.words(r) for r in ref_tok[ref_start[i]:ref_start[i + 1]]] for i in range(n_img)])
    got = {tuple(int(t) for t in k if t >= 0): c for k, c in zip(keys, counts)}
    assert len(got) == len(keys)                                               # every n-gram once
    assert got == want


def test_one_image_raises_value_error():
    from unpaired_image_captioning_amd.misc.lang_eval import DeviceLanguageEval
    import torch
    ev = DeviceLanguageEval.from_references(np.array([[3, 4, 0], [4, 0, 0]]), [0, 2], device="cpu")
    with pytest.raises(ValueError, match="at least 2 images"):
        ev.score([0], torch.tensor([[3, 4, 0]]))


def test_new_entry_points_are_declared_and_exported():
    from unpaired_image_captioning_amd import _lib
    from unpaired_image_captioning_amd.build import build
    build(verbose=False)
    header = open(os.path.join(ROOT, "include", "uic_hip.h")).read()
    declared = set(re.findall(r"\b(uic_[a-z0-9_]+)\s*\(", header))
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW_EXPORTS:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
