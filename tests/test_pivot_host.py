"""The pivot bridge on the CPU: the restatement of tests/pivot_cases.py against the reference's own output
(tests/golden/pivot_dict.json), the three tables of misc.pivot, every refusal of uic_pivot_source / uic_pivot_target through the
C ABI (host pointers: a refused call launches nothing and touches no output), the exports, and the refusals of the Python surface."""
import argparse
import json
import os

import numpy as np
import pytest

import pivot_cases as PC
from unpaired_image_captioning_amd.misc import pivot

HERE = os.path.dirname(os.path.abspath(__file__))


def fixture():
    with open(os.path.join(HERE, "golden", "pivot_dict.json")) as f:
        return json.load(f)


FX = fixture()
REQUIRED = ("unknown_words", "lower", "unk_in_hypothesis", "no_eos", "eos_first")


def test_fixture_holds_the_required_cases_and_the_reference_function_ran():
    names = [c["name"] for c in FX["cases"]]
    assert set(REQUIRED) <= set(names)
    assert FX["build_target_tokens_ran"] is True
    k = FX["constants"]
    assert (k["PAD"], k["UNK"], k["BOS"], k["EOS"]) == (PC.PAD, PC.UNK, PC.BOS, PC.EOS) and k["words"] == PC.SPECIALS
    by = {c["name"]: c for c in FX["cases"]}
    assert PC.UNK in by["unknown_words"]["src_ids"] and PC.UNK in by["unk_in_hypothesis"]["pred"]
    assert PC.EOS not in by["no_eos"]["pred"] and by["eos_first"]["pred"][0] == PC.EOS and by["eos_first"]["tokens"] == []
    assert len(by["no_eos"]["tokens"]) == len(by["no_eos"]["pred"]) - 1


@pytest.mark.parametrize("c", FX["cases"], ids=[c["name"] for c in FX["cases"]])
def test_restated_words_equal_the_reference(c):
    assert PC.convert_to_idx(c["src_dict"], c["lower"], c["sentence"]) == c["src_ids"]
    idx_to_label = {i: w for w, i in c["tgt_dict"].items()}
    assert PC.convert_to_labels(idx_to_label, c["pred"], PC.EOS) == c["labels"]
    assert PC.build_target_tokens(idx_to_label, c["pred"], c["sentence"], c["attn"]) == c["tokens"]


@pytest.mark.parametrize("c", FX["cases"], ids=[c["name"] for c in FX["cases"]])
def test_restated_kernels_on_ids_give_the_references_words(c):
    """The id path -- tables, restated_source, restated_target, render by `repl` -- ends in the reference's tokens."""
    words = sorted(set(c["sentence"]))
    caption_vocab = {str(i + 1): w for i, w in enumerate(words)}
    tgt_i2l = {i: w for w, i in c["tgt_dict"].items()}
    src_l2i = dict(c["src_dict"])
    sd = argparse.Namespace(labelToIdx=src_l2i, idxToLabel={i: w for w, i in src_l2i.items()}, lower=c["lower"], size=lambda: len(src_l2i))
    scoring_vocab = {str(i + 1): w for i, w in enumerate(sorted(set(c["tgt_dict"]) - set(PC.SPECIALS)) + words[:1])}
    tables = pivot.build_tables(caption_vocab, sd, c["tgt_dict"], scoring_vocab)
    want = PC.restated_tables(caption_vocab, (src_l2i, None, c["lower"]), (c["tgt_dict"], tgt_i2l, False), scoring_vocab)
    for got, w in zip(tables[:3], want[:3]):
        assert got.dtype == np.int32 and np.array_equal(got, w)
    assert tables[3] == want[3] == len(scoring_vocab) + 1
    seq = np.array([[words.index(w) + 1 for w in c["sentence"]] + [0, 0]], dtype=np.int64)
    src, lengths, max_len = PC.restated_source(seq, seq.shape[1], tables[0])
    assert src[:max_len, 0].tolist() == c["src_ids"] and lengths[0] == len(c["sentence"]) == max_len
    n = len(c["pred"])
    attn = np.zeros((1, n, max_len), dtype=np.float32)
    attn[0] = np.array(c["attn"], dtype=np.float32)
    out, out_len, repl = PC.restated_target([c["pred"]], n, attn, lengths, seq, tables[1], tables[2], 16)
    score_w = {int(k): w for k, w in scoring_vocab.items()}
    got = []
    for i in range(int(out_len[0])):
        if repl[0, i] >= 0:
            got.append(c["sentence"][repl[0, i]])
            assert out[0, i] == tables[2][seq[0, repl[0, i]]]
        else:
            got.append(tgt_i2l[c["pred"][i]])
            assert score_w.get(int(out[0, i]), None) == got[-1] or out[0, i] == tables[3]
    assert got == c["tokens"]
    assert (out[0, out_len[0]:] == 0).all() and (repl[0, out_len[0]:] == -1).all()
    bridge = pivot.PivotBridge(caption_vocab, sd, c["tgt_dict"], scoring_vocab, device="cpu")
    assert bridge.render(np.array([c["pred"]]), out_len, repl, seq) == [" ".join(c["tokens"])]


def test_tables_oov_specials_and_lower():
    caption_vocab = {"1": "Gou", "2": "mao", "3": "chi", "5": "</s>"}        # (id 4 is a gap)
    src = PC.DictLike(["gou", "chi"], lower=True)
    tgt = PC.DictLike(["dog", "eats", "cat", "mao"])
    scoring_vocab = {"1": "eats", "2": "dog", "3": "mao", "4": "<unk>"}
    src_table, tgt_table, copy_table, oov = pivot.build_tables(caption_vocab, src, tgt, scoring_vocab)
    assert oov == 5 and str(oov) not in scoring_vocab
    assert src_table.tolist() == [PC.UNK, 4, PC.UNK, 5, PC.UNK, PC.EOS]      # 'Gou' is lower-cased before lookup; 'mao' is unknown
    assert tgt_table.tolist() == [oov, oov, oov, oov, 2, 1, oov, 3]          # every special is OOV, also '<unk>' that the scored vocabulary holds
    assert copy_table.tolist() == [oov, oov, 3, oov, oov, oov]               # the copied pivot word is looked up as it is spelled
    for t in (src_table, tgt_table, copy_table):
        assert t.dtype == np.int32
    # plain mappings, word -> id and id -> word, give the same tables
    a = pivot.build_tables(caption_vocab, dict(src.labelToIdx), dict(tgt.labelToIdx), scoring_vocab)
    b = pivot.build_tables(caption_vocab, dict(src.labelToIdx), dict(tgt.idxToLabel), scoring_vocab)
    assert np.array_equal(a[1], tgt_table) and np.array_equal(b[1], tgt_table) and np.array_equal(a[2], copy_table)
    assert a[0].tolist() == [PC.UNK, PC.UNK, PC.UNK, 5, PC.UNK, PC.EOS]      # (a plain mapping does not lower-case)
    want = PC.restated_tables(caption_vocab, (src.labelToIdx, src.idxToLabel, True), (tgt.labelToIdx, tgt.idxToLabel, False), scoring_vocab)
    assert np.array_equal(want[0], src_table) and np.array_equal(want[1], tgt_table) and np.array_equal(want[2], copy_table)
    with pytest.raises(TypeError, match="dictionary"):
        pivot.build_tables(caption_vocab, 50004, tgt, scoring_vocab)


def test_restatement_on_the_shared_cases_is_self_consistent():
    for B in PC.BATCHES:
        for L in (1, 16):
            seq, table = PC.source_case(B, L)
            src, lengths, max_len = PC.restated_source(seq, L, table)
            assert src.shape == (L, B) and lengths.min() >= 1 and max_len == lengths.max() <= L
            assert ((src != PC.PAD).sum(0) == lengths).all()
        for n in (1, 2, 100):
            c = PC.target_case(B, n)
            out, out_len, repl = PC.restated_target(**c)
            assert out_len.max() <= n and ((out != 0).sum(1) == out_len).all() and ((repl >= 0).sum(1) <= out_len).all()
    kinds = PC.target_case(130, 100)
    out, out_len, repl = PC.restated_target(**kinds)
    assert out_len[0] == 0 and out_len[1] == 99 and out_len[2] == 99 and repl[3, 0] == 0 and repl[4, 0] == kinds["src_len"][4] - 1
    assert out[5, 0] == kinds["tgt_table"][PC.UNK] and (repl[6, :99] >= 0).all()


# ---------------------------------------------------------------- the C ABI
def lib():
    from unpaired_image_captioning_amd import _lib
    return _lib.load()


def test_exports():
    from unpaired_image_captioning_amd import _lib
    L = lib()
    for name in ("uic_pivot_source", "uic_pivot_target"):
        assert name in _lib._SIGS and hasattr(L, name)
    with open(os.path.join(os.path.dirname(HERE), "include", "uic_hip.h")) as f:
        header = f.read()
    assert "int uic_pivot_source(" in header and "int uic_pivot_target(" in header
    from unpaired_image_captioning_amd import build
    assert "pivot.hip" in build.SOURCES


def host_source_args():
    B, L, ld, V1 = 3, 4, 6, 9
    bufs = dict(seq=np.ones((B, ld), dtype=np.int64), table=np.arange(V1, dtype=np.int32),
                src=np.full((L, B), PC.POISON, dtype=np.int64), lengths=np.full(B, PC.POISON, dtype=np.int32),
                max_len=np.full(1, PC.POISON, dtype=np.int32))
    args = dict(seq=bufs["seq"].ctypes.data, ld_seq=ld, B=B, L=L, table=bufs["table"].ctypes.data, V1=V1, src=bufs["src"].ctypes.data,
                lengths=bufs["lengths"].ctypes.data, max_len=bufs["max_len"].ctypes.data, stream=None)
    return args, bufs


SOURCE_REFUSALS = [("seq", None, b"seq"), ("table", None, b"table"), ("src", None, b"src"), ("lengths", None, b"lengths"),
                   ("max_len", None, b"max_len"), ("B", -1, b"B=-1"), ("L", 0, b"L=0"), ("ld_seq", 3, b"ld_seq=3"), ("V1", 0, b"V1=0")]


@pytest.mark.parametrize("field,bad,msg", SOURCE_REFUSALS, ids=[r[0] for r in SOURCE_REFUSALS])
def test_pivot_source_refusals(field, bad, msg):
    args, bufs = host_source_args()
    args[field] = bad
    L = lib()
    rc = L.uic_pivot_source(*args.values())
    assert rc != 0 and msg in L.uic_last_error_string() and b"pivot_source" in L.uic_last_error_string(), L.uic_last_error_string()
    for k in ("src", "lengths", "max_len"):
        assert (bufs[k] == PC.POISON).all(), k


def host_target_args():
    B, ld_hyp, n, S, ld_seq, Vt, V1, L_out = 2, 5, 4, 3, 6, 8, 7, 4
    bufs = dict(hyp=np.ones((B, ld_hyp), dtype=np.int64), attn=np.zeros((B, ld_hyp, S), dtype=np.float32),
                src_len=np.ones(B, dtype=np.int32), seq=np.ones((B, ld_seq), dtype=np.int64), tgt_table=np.arange(Vt, dtype=np.int32),
                copy_table=np.arange(V1, dtype=np.int32), out=np.full((B, L_out), PC.POISON, dtype=np.int64),
                out_len=np.full(B, PC.POISON, dtype=np.int32), repl=np.full((B, L_out), PC.POISON, dtype=np.int32))
    p = {k: v.ctypes.data for k, v in bufs.items()}
    args = dict(hyp=p["hyp"], ld_hyp=ld_hyp, n_steps=n, attn=p["attn"], attn_ld=ld_hyp, S=S, src_len=p["src_len"], seq=p["seq"],
                ld_seq=ld_seq, B=B, tgt_table=p["tgt_table"], Vt=Vt, copy_table=p["copy_table"], V1=V1, L_out=L_out, out=p["out"],
                out_len=p["out_len"], repl=p["repl"], stream=None)
    return args, bufs


TARGET_REFUSALS = [(k, None, k.encode()) for k in ("hyp", "attn", "src_len", "seq", "tgt_table", "copy_table", "out", "out_len", "repl")] + \
                  [("B", -1, b"B=-1"), ("n_steps", 0, b"n_steps=0"), ("ld_hyp", 3, b"ld_hyp=3"), ("attn_ld", 3, b"attn_ld=3"), ("S", 0, b"S=0"),
                   ("ld_seq", 0, b"ld_seq=0"), ("Vt", 1, b"Vt=1"), ("V1", 0, b"V1=0"), ("L_out", 0, b"L_out=0")]


@pytest.mark.parametrize("field,bad,msg", TARGET_REFUSALS, ids=[r[0] for r in TARGET_REFUSALS])
def test_pivot_target_refusals(field, bad, msg):
    args, bufs = host_target_args()
    args[field] = bad
    L = lib()
    rc = L.uic_pivot_target(*args.values())
    assert rc != 0 and msg in L.uic_last_error_string() and b"pivot_target" in L.uic_last_error_string(), L.uic_last_error_string()
    for k in ("out", "out_len", "repl"):
        assert (bufs[k] == PC.POISON).all(), k


def test_an_empty_batch_is_a_successful_no_op():
    L = lib()
    args, bufs = host_source_args()
    args["B"] = 0
    assert L.uic_pivot_source(*args.values()) == 0
    for k in ("src", "lengths", "max_len"):
        assert (bufs[k] == PC.POISON).all()
    args, bufs = host_target_args()
    args["B"] = 0
    assert L.uic_pivot_target(*args.values()) == 0
    for k in ("out", "out_len", "repl"):
        assert (bufs[k] == PC.POISON).all()


# ---------------------------------------------------------------- the Python surface
def nmt_model(src_dict, tgt_dict):
    from unpaired_image_captioning_amd.models import NMT_Models
    opt = argparse.Namespace(layers=1, rnn_size=8, word_vec_size=8, dropout=0.0, brnn=True, rnn_type="LSTM", input_feed=1,
                             compute_dtype="f32", seed=1)
    return NMT_Models.NMTModel(opt, NMT_Models.Encoder(opt, src_dict), NMT_Models.Decoder(opt, tgt_dict), src_dict, tgt_dict)


def test_translate_without_dictionaries_raises():
    m = nmt_model(12, 13).eval()
    with pytest.raises(RuntimeError, match="dictionaries"):
        m.translate([["a", "b"]])
    m = nmt_model(PC.DictLike(PC.word_list("z", 8)), PC.DictLike(PC.word_list("e", 9))).eval()
    assert m.translate([]) == []
    with pytest.raises(ValueError, match="empty source sentence"):
        m.translate([["z1"], []])
    assert hasattr(m, "translate_device")


def test_eval_unpaired_refuses_two_ranks_and_a_missing_bridge():
    from unpaired_image_captioning_amd import eval_utils
    from unpaired_image_captioning_amd.trainer import Trainer
    two = argparse.Namespace(exchange=argparse.Namespace(world_size=2, rank=0))
    with pytest.raises(NotImplementedError, match="ranks"):
        Trainer.eval_unpaired(two, None, None)
    one = argparse.Namespace(exchange=argparse.Namespace(world_size=1, rank=0), pivot_bridge=None)
    with pytest.raises(RuntimeError, match="build_pivot"):
        Trainer.eval_unpaired(one, None, None)
    with pytest.raises(ValueError, match="pivot_bridge"):
        eval_utils.eval_split_coco_unpaired(argparse.Namespace(), None, None, None, None, {})
    with pytest.raises(NotImplementedError, match="Trainer.eval_nmt"):
        eval_utils.eval_split_coco_unpaired(argparse.Namespace(nmt_eval_flag=1, coco_eval_flag=1), None, None, None, None, {"pivot_bridge": object()})
    with pytest.raises(NotImplementedError, match="coco_eval_flag"):
        eval_utils.eval_split(argparse.Namespace(coco_eval_flag=1), None, None, None, {})
