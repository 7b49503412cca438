"""The unpaired validation chain on the device, with tiny models (the widths of the nmt_translate_tiny / topdown_tiny fixtures,
dictionaries of a few dozen words): NMTModel.translate_device against translateBatch, PivotBridge.pivot against the two oracles
chained (f32) and against the restated glue on the device's own tensors (bf16, exact), NMTModel.translate on words, and
eval_split_coco_unpaired / Trainer.eval_unpaired on two synthetic on-disk data sets."""
import argparse
import random

import numpy as np
import pytest
import torch

import lang_eval_cases as LC
import pivot_cases as PC
from oracle import nmt as ON
from oracle import topdown as O

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------- vocabularies (dataset_files: caption id i + 1 is the word 'w<i>')
V_ZH, V_EN, L, D, R = 24, 18, 8, 64, 5
ZH_VOCAB = {str(i + 1): "w%d" % i for i in range(V_ZH)}
EN_VOCAB = {str(i + 1): "w%d" % i for i in range(V_EN)}
SRC_DICT = PC.DictLike(PC.word_list("w", 20))                              # w20 .. w23 are unknown to the translator
TGT_DICT = PC.DictLike(PC.word_list("w", 14) + PC.word_list("x", 6))       # x0 .. x5 are not in the scored vocabulary
CAP = dict(V=V_ZH, E=32, H=32, A=32, D=D, L=L)
B_PIVOT = 9


def nmt_cfg(B, S=L):
    return dict(layers=2, H=32, W=32, B=B, S=S, T=2, Vs=SRC_DICT.size(), Vt=TGT_DICT.size())


def nmt_weights(seed=5):
    from test_gpu_nmt import random_weights
    W = random_weights(nmt_cfg(B_PIVOT), seed, scale=0.6)
    W["generator.0.bias"][PC.EOS] += 3.0                                  # sentences that end at different steps
    W["generator.0.bias"][PC.UNK] += 1.5                                  # ... and hold UNK, so that words are copied
    return W


def cap_weights(seed=3):
    W = O.init_weights(V_ZH + 1, CAP["E"], CAP["H"], CAP["A"], D, D, seed=seed)
    W["logit.weight"] *= 8.0                                              # a peaked word distribution ...
    W["logit.bias"][0] += 0.15                                            # ... whose captions end at different steps
    return W


def build_nmt(W, dtype):
    from test_gpu_nmt import build
    model, _ = build(nmt_cfg(B_PIVOT), W, dtype)
    model.src_dict, model.tgt_dict = SRC_DICT, TGT_DICT
    return model.eval()


def bridge():
    from unpaired_image_captioning_amd.misc.pivot import PivotBridge
    return PivotBridge(ZH_VOCAB, SRC_DICT, TGT_DICT, EN_VOCAB)


def restated():
    return PC.restated_tables(ZH_VOCAB, (SRC_DICT.labelToIdx, SRC_DICT.idxToLabel, False), (TGT_DICT.labelToIdx, TGT_DICT.idxToLabel, False), EN_VOCAB)


@pytest.fixture(scope="module")
def chain():
    """Weights, features and the oracle's own chain, computed once: greedy captions, their source batch, its translation."""
    Wc, Wn = cap_weights(), nmt_weights()
    b = O.synthetic_batch(B_PIVOT, 1, R, D, V_ZH, L, seed=21, ragged_regions=True)
    sc = 1 + 2.0 * (torch.arange(B_PIVOT) % 8).float()                    # images of very different feature magnitude
    b["att_feats"], b["fc_feats"] = b["att_feats"] * sc[:, None, None], b["fc_feats"] * sc[:, None]
    seq_o, _ = O.sample(Wc, b["fc_feats"], b["att_feats"], b["att_masks"], L)
    src_table, tgt_table, copy_table, oov = restated()
    src_o, len_o, max_o = PC.restated_source(seq_o.numpy(), L, src_table)
    src_o = torch.from_numpy(src_o[:max_o])
    hyp_o, scores_o, attn_o = ON.translate_batch(Wn, src_o.unsqueeze(2), max_steps=12)
    return dict(Wc=Wc, Wn=Wn, b=b, seq_o=seq_o, src_o=src_o, len_o=len_o, hyp_o=hyp_o, scores_o=scores_o, attn_o=attn_o)


def device_chain(chain, dtype):
    from test_gpu_topdown import build_model
    cap = build_model(CAP, chain["Wc"], dtype).eval()
    nmt = build_nmt(chain["Wn"], dtype)
    br = bridge()
    b = chain["b"]
    with torch.no_grad():
        seq = cap(b["fc_feats"].cuda(), None, b["att_feats"].cuda(), b["att_masks"].cuda(), opt={"beam_size": 1}, mode="sample")[0]
        out, out_len, scores = br.pivot(seq, nmt, max_steps=12)
    torch.cuda.synchronize()
    return br, seq, out, out_len, scores


def test_translate_device_equals_translate_batch(chain):
    nmt = build_nmt(chain["Wn"], "f32")
    src = chain["src_o"].cuda()
    hyp, scores, attn, n = nmt.translate_device(src, max_steps=12)
    assert hyp.is_cuda and scores.is_cuda and attn.is_cuda and isinstance(n, int)
    assert hyp.shape == (B_PIVOT, 12) and attn.shape == (B_PIVOT, 12, src.shape[0])
    allHyp, allScores, allAttn, gold = nmt.translateBatch(argparse.Namespace(src=src.unsqueeze(2), batchSize=B_PIVOT), max_steps=12)
    assert [h[0] for h in allHyp] == hyp[:, :n].cpu().tolist()
    assert torch.equal(torch.cat(allScores), scores)
    valid = (src != 0).sum(0).cpu().tolist()
    for k in range(B_PIVOT):
        assert torch.equal(allAttn[k][0], attn[k, :n, :valid[k]])
    assert float(gold.abs().sum()) == 0


def test_pivot_f32_equals_the_two_oracles_chained(chain):
    br, seq, out, out_len, scores = device_chain(chain, "f32")
    lens = (chain["seq_o"] > 0).sum(1)
    assert len(set(lens.tolist())) > 1                                     # captions of different lengths in one batch
    assert torch.equal(seq.cpu(), chain["seq_o"])
    last = br.last
    assert torch.equal(last["src"].cpu(), chain["src_o"])                  # the restated mapping of the oracle's captions ...
    assert torch.equal(last["lengths"].cpu(), torch.from_numpy(chain["len_o"]))
    hyp_o = chain["hyp_o"]
    assert last["n"] == hyp_o.shape[1]
    assert torch.equal(last["hyp"][:, :last["n"]].cpu(), hyp_o)            # ... and the oracle's translation of that padded batch
    assert (scores.cpu() - chain["scores_o"]).abs().max().item() < 2e-3 * max(1.0, chain["scores_o"].abs().max().item())
    assert (hyp_o == PC.UNK).any()                                         # a word is copied somewhere
    src_table, tgt_table, copy_table, oov = restated()
    want = PC.restated_target(hyp_o.numpy(), hyp_o.shape[1], last["attn"].cpu().numpy(), chain["len_o"], chain["seq_o"].numpy(), tgt_table,
                              copy_table, br.max_words)
    assert torch.equal(out.cpu(), torch.from_numpy(want[0])) and torch.equal(out_len.cpu(), torch.from_numpy(want[1]))


def test_pivot_bf16_equals_the_restated_glue_on_the_devices_own_tensors(chain):
    br, seq, out, out_len, scores = device_chain(chain, "bf16")
    last = br.last
    src_table, tgt_table, copy_table, oov = restated()
    seq_h = seq.cpu().numpy()
    src_w, len_w, max_w = PC.restated_source(seq_h, L, src_table)
    assert torch.equal(last["src"].cpu(), torch.from_numpy(src_w[:max_w])) and last["src"].shape[0] == max_w
    assert torch.equal(last["lengths"].cpu(), torch.from_numpy(len_w))
    want = PC.restated_target(last["hyp"].cpu().numpy(), last["n"], last["attn"].cpu().numpy(), len_w, seq_h, tgt_table, copy_table, br.max_words)
    assert torch.equal(out.cpu(), torch.from_numpy(want[0]))
    assert torch.equal(out_len.cpu(), torch.from_numpy(want[1]))
    assert torch.equal(last["repl"].cpu(), torch.from_numpy(want[2]))
    assert out.shape == (B_PIVOT, br.max_words) and scores.shape == (B_PIVOT,)


def test_translate_on_words_returns_the_callers_word_at_a_replaced_position(chain):
    nmt = build_nmt(chain["Wn"], "f32")
    sents = [["w3", "Zebra", "w7"], ["Qq", "Zz"], ["w1", "w2", "w3", "w4", "w19"], ["w23"]]
    pred = nmt.translate(sents, max_steps=12)
    assert len(pred) == len(sents) and all(len(p) == 1 for p in pred)
    # the same through translate_device and the restated buildTargetTokens (checked against the reference in test_pivot_host.py)
    ids = [PC.convert_to_idx(SRC_DICT.labelToIdx, False, s) for s in sents]
    assert ids[1] == [PC.UNK, PC.UNK] and ids[0][1] == PC.UNK
    S = max(len(s) for s in sents)
    src = torch.zeros(S, len(sents), dtype=torch.int64)
    for b, row in enumerate(ids):
        src[:len(row), b] = torch.tensor(row)
    hyp, scores, attn, n = nmt.translate_device(src.cuda(), max_steps=12)
    hyp, attn = hyp.cpu().numpy(), attn.cpu().numpy()
    copied = 0
    for b, s in enumerate(sents):
        want = PC.build_target_tokens(TGT_DICT.idxToLabel, hyp[b, :n].tolist(), s, attn[b, :n, :len(s)])
        assert pred[b][0] == want, (b, pred[b][0], want)
        kept = hyp[b, :len(want)]
        assert all(w in s for w, t in zip(want, kept) if t == PC.UNK)
        copied += int((kept == PC.UNK).sum())
    assert copied > 0
    assert any(w in ("Qq", "Zz") for w in pred[1][0]) or not (hyp[1, :len(pred[1][0])] == PC.UNK).any()


# ---------------------------------------------------------------- eval_split_coco_unpaired / Trainer.eval_unpaired
BATCH, S_PER, N_VAL_ZH, N_VAL_EN, D_EVAL = 3, 2, 7, 5, 16


def write_set(root, g, n, val, V, seq_len):
    from dataset_files import loader_opt, write_dataset
    ids = [100 + 3 * i for i in range(n)]
    splits = ["val" if i in val else "train" for i in range(n)]
    att = [g.standard_normal((int(g.integers(2, 6)), D_EVAL)).astype(np.float32) for _ in range(n)]
    fc = [g.standard_normal(D_EVAL).astype(np.float32) for _ in range(n)]
    counts = [int(g.integers(2, 5)) for _ in range(n)]
    end = np.cumsum(counts)
    start = end - np.array(counts) + 1
    labels = LC.caption_rows(g, int(end[-1]), seq_len, V, min_words=1)
    label_path = write_dataset(root, att, None, fc, [(10, 10)] * n, ids, labels, start, end, V, splits=splits)
    lo = loader_opt(root, label_path, BATCH, S_PER, D_EVAL, D_EVAL, 0, 0, 0)
    refs = {ids[i]: labels[start[i] - 1:end[i]] for i in range(n)}
    return lo, refs, [ids[i] for i in range(n) if splits[i] == "val"]


@pytest.fixture(scope="module")
def unpaired(tmp_path_factory, chain):
    """A zh-side data set (11 images, 7 'val') and a COCO-side one (9 images, 5 'val') with different vocabularies; neither
    split is a multiple of the batch size 3.  A tiny TopDown captioner in a Trainer, the tiny translator beside it."""
    from unpaired_image_captioning_amd.misc.dataloader.dataloader import DataLoader
    from unpaired_image_captioning_amd.trainer import Trainer
    g = np.random.default_rng(3)
    lo, refs, val_ids = write_set(str(tmp_path_factory.mktemp("zh")), g, 11, (0, 1, 3, 4, 6, 7, 9), V_ZH, L)
    lo_en, refs_en, val_ids_en = write_set(str(tmp_path_factory.mktemp("en")), g, 9, (1, 2, 4, 6, 8), V_EN, 10)
    assert len(val_ids) == N_VAL_ZH and len(val_ids_en) == N_VAL_EN and N_VAL_ZH % BATCH and N_VAL_EN % BATCH
    opt = argparse.Namespace(vocab_size=V_ZH, input_encoding_size=32, rnn_size=32, num_layers=1, drop_prob_lm=0.0, seq_length=L,
                             att_hid_size=32, use_bn=0, logit_layers=1, caption_model="topdown", compute_dtype="f32", seed=2,
                             i2t_train_flag=1, i2t_eval_flag=1, language_eval=1, beam_size=1, verbose=False, nmt_max_steps=12, **vars(lo))
    torch.manual_seed(4)
    tr = Trainer(opt)
    tr.i2t_model.cuda()
    tr.nmt_model = tr.dp_nmt_model = build_nmt(chain["Wn"], "f32")
    loader, coco_loader = DataLoader(opt), DataLoader(argparse.Namespace(**vars(lo_en)))
    assert loader.get_vocab() == ZH_VOCAB and coco_loader.get_vocab() == EN_VOCAB
    tr.build_pivot(loader.get_vocab(), coco_loader.get_vocab())
    return tr, loader, coco_loader, refs_en, val_ids, val_ids_en


def restate_coco(predictions, refs, width):
    """coco_lang_stats from the returned captions: a word of the scored vocabulary is its id, any other word the OOV id."""
    word_id = {w: int(k) for k, w in EN_VOCAB.items()}
    hyp = np.zeros((len(predictions), width), dtype=np.int64)
    for i, p in enumerate(predictions):
        toks = [word_id.get(w, len(EN_VOCAB) + 1) for w in p["caption"].split()]
        hyp[i, :len(toks)] = toks
    ref_tok = np.concatenate([refs[p["image_id"]] for p in predictions])
    ref_start = np.concatenate([[0], np.cumsum([len(refs[p["image_id"]]) for p in predictions])])
    return LC.evaluate(hyp, ref_tok, ref_start)


def test_eval_unpaired_both_halves_and_the_best_flag(unpaired):
    from test_gpu_lang_eval import check_lang_stats
    from unpaired_image_captioning_amd import eval_utils
    tr, loader, coco_loader, refs_en, val_ids, val_ids_en = unpaired
    tr.best_i2t_val_score, tr.best_flag_i2t = None, False
    tr.opt.language_eval = 1
    tr.i2t_model.train()
    tr.nmt_model.eval()
    random.seed(11)
    tr.eval_unpaired(loader, coco_loader)
    assert tr.i2t_model.training and not tr.nmt_model.training            # the modes are restored
    # the paired half is eval_split's
    kwargs = {'split': 'val', 'dataset': ''}
    kwargs.update(vars(tr.opt))
    random.seed(11)
    val_loss, predictions, lang_stats, _, _ = eval_utils.eval_split(tr.opt, loader, tr.dp_i2t_model, None, kwargs)
    assert tr.predictions == predictions and tr.lang_stats == lang_stats and len(predictions) == N_VAL_ZH
    assert abs(tr.i2t_val_loss - val_loss) <= 1e-6 * max(1.0, abs(val_loss)) and val_loss > 0
    # the COCO half: every image once, scored against the COCO references
    got = [p["image_id"] for p in tr.coco_predictions]
    assert sorted(got) == sorted(val_ids_en) and len(set(got)) == N_VAL_EN
    assert all(set(p) == {"image_id", "caption"} for p in tr.coco_predictions)
    words = set(w for p in tr.coco_predictions for w in p["caption"].split())
    assert words and words <= set(TGT_DICT.labelToIdx) | set(ZH_VOCAB.values())       # the target dictionary's words, or copied pivot words
    check_lang_stats(tr.coco_lang_stats, restate_coco(tr.coco_predictions, refs_en, tr.pivot_bridge.max_words), N_VAL_EN)
    assert tr.coco_lang_stats is not tr.lang_stats
    assert tr.best_flag_i2t and tr.best_i2t_val_score == tr.coco_lang_stats["CIDEr"]
    # a second evaluation of the same weights does not beat the first (strict >); the translator's mode is restored to train too
    first, first_pred = tr.best_i2t_val_score, tr.coco_predictions
    tr.best_flag_i2t = False
    tr.nmt_model.train()
    random.seed(11)
    tr.eval_unpaired(loader, coco_loader)
    assert tr.nmt_model.training
    tr.nmt_model.eval()
    assert not tr.best_flag_i2t and tr.best_i2t_val_score == first and tr.coco_predictions == first_pred


def test_eval_unpaired_val_images_use_and_ranking_by_loss(unpaired):
    from test_gpu_lang_eval import check_lang_stats
    tr, loader, coco_loader, refs_en, val_ids, val_ids_en = unpaired
    tr.best_i2t_val_score, tr.best_flag_i2t = None, False
    tr.opt.language_eval, tr.opt.val_images_use = 1, 4
    try:
        tr.eval_unpaired(loader, coco_loader)
        assert sorted(p["image_id"] for p in tr.predictions) == sorted(val_ids[:4])
        assert sorted(p["image_id"] for p in tr.coco_predictions) == sorted(val_ids_en[:4])
        check_lang_stats(tr.coco_lang_stats, restate_coco(tr.coco_predictions, refs_en, tr.pivot_bridge.max_words), 4)
    finally:
        del tr.opt.val_images_use
    tr.best_i2t_val_score, tr.best_flag_i2t = None, False
    tr.opt.language_eval = 0
    try:
        tr.eval_unpaired(loader, coco_loader)
        assert tr.lang_stats is None and tr.coco_lang_stats is None and len(tr.coco_predictions) == N_VAL_EN
        assert tr.best_flag_i2t and tr.best_i2t_val_score == -tr.i2t_val_loss
        tr.best_i2t_val_score, tr.best_flag_i2t = -tr.i2t_val_loss + 1.0, False
        tr.eval_unpaired(loader, coco_loader)
        assert not tr.best_flag_i2t
    finally:
        tr.opt.language_eval = 1


def test_eval_unpaired_refusals_and_trainer_eval_unchanged(unpaired):
    from unpaired_image_captioning_amd import eval_utils
    tr, loader, coco_loader, refs_en, val_ids, val_ids_en = unpaired
    tr.opt.coco_eval_flag = 1
    try:
        with pytest.raises(NotImplementedError, match="coco_eval_flag"):
            tr.eval(loader)
        with pytest.raises(NotImplementedError, match="coco_eval_flag"):
            tr.eval(loader, coco_loader)
    finally:
        del tr.opt.coco_eval_flag
    tr.opt.nmt_eval_flag = 1
    try:
        with pytest.raises(NotImplementedError, match="eval_nmt"):
            tr.eval_unpaired(loader, coco_loader)
    finally:
        tr.opt.nmt_eval_flag = 0
    exchange = tr.exchange
    tr.exchange = argparse.Namespace(world_size=2, rank=0)
    try:
        with pytest.raises(NotImplementedError, match="ranks"):
            tr.eval_unpaired(loader, coco_loader)
    finally:
        tr.exchange = exchange
    with pytest.raises(ValueError, match="pivot_bridge"):
        eval_utils.eval_split_coco_unpaired(tr.opt, loader, coco_loader, tr.dp_i2t_model, tr.nmt_model, {})
    assert tr.i2t_model.training
