"""Validation on the device: the language-evaluation kernels (csrc/cider.hip: uic_langeval_*) behind misc/lang_eval.py against
the reference scorers' own numbers (tests/golden/lang_eval_*.npz) and against the CPU restatement (tests/lang_eval_cases.py),
and Trainer.eval / Trainer.eval_nmt end to end.

Tolerances: the integer counts and everything formed from them on the host are EXACT; per-image f64 scores end in the device
math library's pow / exp / log tail, TOL = 1e-13 * max(1, max|want|) as in tests/test_gpu_bleu.py; a corpus mean adds the bound
of an n-term f64 sum taken in another order, n * 2^-53 * max|score|."""
import argparse
import ctypes as C
import random

import numpy as np
import pytest
import torch

import lang_eval_cases as LC
from test_lang_eval_host import FIXTURES, load

pytestmark = pytest.mark.gpu


def tol(want):
    return 1e-13 * max(1.0, float(np.abs(want).max()))


def device_eval(hyp, ref_tok, ref_start, image_ix=None):
    from unpaired_image_captioning_amd.misc.lang_eval import DeviceLanguageEval
    ev = DeviceLanguageEval.from_references(ref_tok, ref_start)
    ix = np.arange(len(hyp)) if image_ix is None else image_ix
    overall, per_image = ev.score(ix, torch.from_numpy(np.ascontiguousarray(hyp)).cuda())
    return ev, overall, per_image


def check_against(want, ev, overall, per_image):
    """want: dict(bleu [4, n], rouge, cider, totals, corpus [6])."""
    n = len(want["rouge"])
    assert np.array_equal(ev.last_totals, want["totals"])
    assert [overall[k] for k in LC.KEYS[:4]] == [float(x) for x in want["corpus"][:4]]
    for k in range(4):
        got, w = per_image["Bleu_%d" % (k + 1)], want["bleu"][k]
        print("Bleu_%d max error %.3e (bound %.3e)" % (k + 1, np.abs(got - w).max(), tol(w)))
        assert np.abs(got - w).max() <= tol(w)
    for key, w, c in (("ROUGE_L", want["rouge"], want["corpus"][4]), ("CIDEr", want["cider"], want["corpus"][5])):
        got = per_image[key]
        bound = tol(w) + n * 2.0 ** -53 * float(np.abs(w).max())
        print("%s max error %.3e (bound %.3e), corpus error %.3e (bound %.3e)" % (key, np.abs(got - w).max(), tol(w), abs(overall[key] - c), bound))
        assert np.abs(got - w).max() <= tol(w)
        assert (got[w == 0.0] == 0.0).all() and (got[w == 1.0] == 1.0).all()
        assert abs(overall[key] - c) <= bound
    assert all(isinstance(overall[k], float) for k in LC.KEYS) and set(overall) == set(LC.KEYS) == set(per_image)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_of_the_reference_scorers(name):
    z = load(name)
    ev, overall, per_image = device_eval(z["hyp"], z["ref_tok"], z["ref_start"])
    check_against({k: z[k] for k in ("bleu", "rouge", "cider", "totals", "corpus")}, ev, overall, per_image)


SWEEP = [(0, 4, 8, 5, 6, 3), (1, 50, 1, 7, 5, 6), (2, 9, 13, 20, 4, 11), (3, 3, 24, 24, 7, [1, 6, 2, 5, 11, 3, 4]),
         (4, 9487, 16, 16, 8, 5), (5, 2, 64, 40, 3, 2), (6, 6, 5, 1, 4, 2)]


@pytest.mark.parametrize("seed,V,L,Lr,n_img,n_refs", SWEEP)
def test_random_captions_against_the_restatement(seed, V, L, Lr, n_img, n_refs):
    hyp, ref_tok, ref_start = LC.random_case(100 + seed, V, L, Lr, n_img, n_refs)
    ev, overall, per_image = device_eval(hyp, ref_tok, ref_start)
    check_against(LC.evaluate(hyp, ref_tok, ref_start), ev, overall, per_image)


def test_at_size_600_images():
    hyp, ref_tok, ref_start = LC.random_case(7, V=2000, L=16, Lr=16, n_img=600, n_refs=5)
    ev, overall, per_image = device_eval(hyp, ref_tok, ref_start)
    check_against(LC.evaluate(hyp, ref_tok, ref_start), ev, overall, per_image)


def test_image_subset_in_another_order_and_the_cached_table():
    """df is computed over the evaluated images only; a second score() of the same image set builds no table."""
    z = load("lang_eval_real_shape")
    hyp, ref_tok, ref_start = z["hyp"], z["ref_tok"], z["ref_start"]
    ev, overall, _ = device_eval(hyp, ref_tok, ref_start)
    assert ev.tables_built == 1
    again, _ = ev.score(np.arange(len(hyp)), torch.from_numpy(hyp).cuda())
    assert ev.tables_built == 1 and again == overall                      # (fixed-order sums: the same bits)
    pick = np.array([7, 2, 9, 0, 5])
    sub_overall, sub_img = ev.score(pick, torch.from_numpy(hyp[pick]).cuda())
    assert ev.tables_built == 2
    sub_tok = np.concatenate([ref_tok[ref_start[i]:ref_start[i + 1]] for i in pick])
    sub_start = np.concatenate([[0], np.cumsum([ref_start[i + 1] - ref_start[i] for i in pick])])
    check_against(LC.evaluate(hyp[pick], sub_tok, sub_start), ev, sub_overall, sub_img)
    with pytest.raises(ValueError, match="twice"):
        ev.score(np.array([1, 1]), torch.from_numpy(hyp[:2]).cuda())


def test_end_token_1_is_the_reward_kernels_bit_for_bit():
    from test_oracle_bleu import load as load_bleu
    from unpaired_image_captioning_amd import _lib
    from unpaired_image_captioning_amd._lib import check, ptr, stream
    from unpaired_image_captioning_amd.misc import rewards
    z, gts, S = load_bleu("bleu_real_shape")
    lib = _lib.load()
    hyp = torch.from_numpy(np.concatenate([z["gen"], z["greedy"]], 0)).cuda()
    n_hyp, L = hyp.shape
    N = len(z["gen"])
    ref_d, start_d, Lr = rewards.upload_references(gts, hyp.device)
    args = (ptr(hyp), n_hyp, L, N, S, ptr(ref_d), Lr, ptr(start_d), len(gts))
    old = torch.empty(n_hyp, dtype=torch.float64, device="cuda")
    new = torch.empty(4, n_hyp, dtype=torch.float64, device="cuda")
    comps = torch.empty(n_hyp, 10, dtype=torch.int32, device="cuda")
    check(lib.uic_bleu_scores(*args, ptr(old), stream()), "bleu_scores")
    check(lib.uic_langeval_bleu(*args, 1, ptr(comps), ptr(new), stream()), "langeval_bleu")
    assert torch.equal(old, new[3])
    assert np.abs(new.cpu().numpy() - z["bleu"]).max() <= tol(z["bleu"])   # and BLEU-1..3 are the reference scorer's
    scorer = rewards.DeviceCiderD(None, None)
    sk, sv, slots, ref_len = scorer._corpus_table(gts, n_hyp, N, S)
    half = max(L, Lr, 32)
    pen = scorer._penalty(half)
    a, b = torch.empty_like(old), torch.empty_like(old)
    targs = (ptr(sk), ptr(sv), slots, C.c_double(ref_len), ptr(pen), half)
    check(lib.uic_ciderd_scores(*args, *targs, ptr(a), stream()), "ciderd_scores")
    check(lib.uic_langeval_cider(*args, *targs, 1, ptr(b), stream()), "langeval_cider")
    assert torch.equal(a, b) and float(a.abs().max()) > 0
    check(lib.uic_langeval_cider(*args, *targs, 0, ptr(b), stream()), "langeval_cider")
    assert not torch.equal(a, b)                                            # (the end token is a word in one, not in the other)


# ---------------------------------------------------------------- Trainer.eval
V, L, D, S_PER, BATCH, N_VAL = 20, 6, 16, 2, 3, 7


@pytest.fixture(scope="module")
def val_setup(tmp_path_factory):
    """11 images (7 'val': not a multiple of the batch size 3), 2 to 4 captions each, a tiny TopDown captioner."""
    from dataset_files import loader_opt, write_dataset
    from unpaired_image_captioning_amd.misc.dataloader.dataloader import DataLoader
    from unpaired_image_captioning_amd.trainer import Trainer
    root = str(tmp_path_factory.mktemp("langeval"))
    g = np.random.default_rng(3)
    n = 11
    ids = [100 + 3 * i for i in range(n)]
    splits = ["val" if i in (0, 1, 3, 4, 6, 7, 9) else "train" for i in range(n)]
    assert splits.count("val") == N_VAL and N_VAL % BATCH != 0
    att = [g.standard_normal((int(g.integers(2, 6)), D)).astype(np.float32) for _ in range(n)]
    fc = [g.standard_normal(D).astype(np.float32) for _ in range(n)]
    counts = [int(g.integers(2, 5)) for _ in range(n)]
    end = np.cumsum(counts)
    start = end - np.array(counts) + 1
    labels = LC.caption_rows(g, int(end[-1]), L, V, min_words=1)
    label_path = write_dataset(root, att, None, fc, [(10, 10)] * n, ids, labels, start, end, V, splits=splits)
    lo = loader_opt(root, label_path, BATCH, S_PER, D, D, 0, 0, 0)
    opt = argparse.Namespace(vocab_size=V, input_encoding_size=32, rnn_size=32, num_layers=1, drop_prob_lm=0.0, seq_length=L,
                             att_hid_size=32, use_bn=0, logit_layers=1, caption_model="topdown", compute_dtype="f32", seed=2,
                             i2t_train_flag=1, i2t_eval_flag=1, language_eval=1, beam_size=1, verbose=False, **vars(lo))
    torch.manual_seed(4)
    tr = Trainer(opt)
    tr.i2t_model.cuda()
    loader = DataLoader(opt)
    refs = {ids[i]: labels[start[i] - 1:end[i]] for i in range(n)}
    return tr, loader, refs, [ids[i] for i in range(n) if splits[i] == "val"]


def restate(predictions, refs):
    """lang_stats from the returned captions: word 'w<k>' is token k + 1 (dataset_files.write_dataset)."""
    hyp = np.zeros((len(predictions), L), dtype=np.int64)
    for i, p in enumerate(predictions):
        toks = [int(w[1:]) + 1 for w in p["caption"].split()]
        hyp[i, :len(toks)] = toks
    ref_tok = np.concatenate([refs[p["image_id"]] for p in predictions])
    ref_start = np.concatenate([[0], np.cumsum([len(refs[p["image_id"]]) for p in predictions])])
    return LC.evaluate(hyp, ref_tok, ref_start)


def check_lang_stats(stats, want, n):
    assert [stats[k] for k in LC.KEYS[:4]] == [float(x) for x in want["corpus"][:4]]
    for key, w, c in (("ROUGE_L", want["rouge"], want["corpus"][4]), ("CIDEr", want["cider"], want["corpus"][5])):
        assert abs(stats[key] - c) <= tol(w) + n * 2.0 ** -53 * float(np.abs(w).max()), key


def test_trainer_eval_on_a_split_that_is_no_multiple_of_the_batch(val_setup):
    from unpaired_image_captioning_amd.misc.criterion import LanguageModelCriterion
    tr, loader, refs, val_ids = val_setup
    tr.best_i2t_val_score, tr.best_flag_i2t = None, False
    tr.opt.language_eval, tr.opt.beam_size = 1, 1
    tr.i2t_model.train()
    random.seed(11)
    tr.eval(loader)
    assert tr.i2t_model.training                                            # back in train mode
    got_ids = [p["image_id"] for p in tr.predictions]
    assert sorted(got_ids) == sorted(val_ids) and len(set(got_ids)) == N_VAL      # one prediction per val image, none twice
    assert all(set(p) == {"image_id", "caption"} for p in tr.predictions)
    check_lang_stats(tr.lang_stats, restate(tr.predictions, refs), N_VAL)
    assert tr.coco_lang_stats is tr.lang_stats
    assert tr.best_flag_i2t and tr.best_i2t_val_score == tr.lang_stats["CIDEr"]
    # the loss: the mean of the per-batch criterion over the same batches, by direct calls
    random.seed(11)
    loader.reset_iterator("val")
    crit, losses = LanguageModelCriterion(tr.opt), []
    tr.i2t_model.eval()
    while True:
        data = loader.get_batch("val")
        labels, masks = torch.from_numpy(data["labels"]).cuda(), torch.from_numpy(data["masks"]).cuda()
        with torch.no_grad():
            out = tr.i2t_model(data["fc_feats"], None, data["att_feats"], labels, data["att_masks"])
            losses.append(float(crit(out, labels[:, 1:], masks[:, 1:]).item()))
        if data["bounds"]["wrapped"]:
            break
    tr.i2t_model.train()
    assert len(losses) == 3
    want = sum(losses) / (1e-8 + len(losses))
    print("val loss", tr.i2t_val_loss, want)
    assert abs(tr.i2t_val_loss - want) <= 1e-6 * max(1.0, abs(want))       # f32 losses; equal up to the kernels' summation order
    # a second evaluation of the same weights does not beat the first (strict >)
    first = tr.best_i2t_val_score
    tr.best_flag_i2t = False
    random.seed(11)
    tr.eval(loader)
    assert not tr.best_flag_i2t and tr.best_i2t_val_score == first


def test_trainer_eval_ranks_by_val_loss_without_language_eval(val_setup):
    tr, loader, refs, val_ids = val_setup
    tr.best_i2t_val_score, tr.best_flag_i2t = None, False
    tr.opt.language_eval, tr.opt.beam_size = 0, 1
    tr.eval(loader)
    assert tr.lang_stats is None and tr.best_flag_i2t and tr.best_i2t_val_score == -tr.i2t_val_loss and tr.i2t_val_loss > 0
    tr.best_i2t_val_score, tr.best_flag_i2t = -tr.i2t_val_loss + 1.0, False      # a better score restored from `infos`
    tr.eval(loader)
    assert not tr.best_flag_i2t


def test_trainer_eval_with_beam_size_2_and_val_images_use(val_setup):
    tr, loader, refs, val_ids = val_setup
    tr.best_i2t_val_score, tr.best_flag_i2t = None, False
    tr.opt.language_eval, tr.opt.beam_size = 1, 2
    tr.opt.verbose_beam, tr.opt.dump_path = 0, 1
    try:
        tr.eval(loader)
        assert len(tr.predictions) == N_VAL and all(p["file_name"] == "img/%d.jpg" % p["image_id"] for p in tr.predictions)
        check_lang_stats(tr.lang_stats, restate(tr.predictions, refs), N_VAL)
        tr.opt.val_images_use = 4                                           # the first 4 images of the split's order, each once
        tr.eval(loader)
        assert sorted(p["image_id"] for p in tr.predictions) == sorted(val_ids[:4])
        check_lang_stats(tr.lang_stats, restate(tr.predictions, refs), 4)
    finally:
        tr.opt.beam_size = 1
        del tr.opt.verbose_beam, tr.opt.dump_path
        if hasattr(tr.opt, "val_images_use"):
            del tr.opt.val_images_use


def test_trainer_eval_refuses_what_it_does_not_do(val_setup):
    tr, loader, refs, val_ids = val_setup
    exchange = tr.exchange
    tr.exchange = argparse.Namespace(world_size=2, rank=0)
    try:
        with pytest.raises(NotImplementedError, match="ranks"):
            tr.eval(loader)
    finally:
        tr.exchange = exchange
    tr.opt.coco_eval_flag = 1
    try:
        with pytest.raises(NotImplementedError, match="coco_eval_flag"):
            tr.eval(loader)
    finally:
        del tr.opt.coco_eval_flag
    tr.opt.dump_images = 1
    try:
        with pytest.raises(NotImplementedError, match="dump_images"):
            tr.eval(loader)
    finally:
        del tr.opt.dump_images
    assert tr.i2t_model.training


# ---------------------------------------------------------------- Trainer.eval_nmt
NMT_CFG = dict(layers=2, H=64, W=64, B=8, S=10, T=9, Vs=120, Vt=130)


def test_trainer_eval_nmt_statistics_and_no_side_effects(tmp_path):
    from test_gpu_nmt import make_opt, synthetic
    from unpaired_image_captioning_amd.misc.criterion import Statistics
    from unpaired_image_captioning_amd.trainer import Trainer
    o = make_opt(NMT_CFG, "f32", dropout=0.3, seed=3)
    o.nmt_train_flag, o.i2t_train_flag, o.checkpoint_path = 1, 0, str(tmp_path)
    o.nmt_learning_rate, o.nmt_max_grad_norm, o.param_init, o.caption_model = 5e-3, 5, 0.1, None
    tr = Trainer(o)
    torch.manual_seed(17)
    tr.build_nmt(NMT_CFG["Vs"], NMT_CFG["Vt"])
    batches = []
    for seed in (9, 10, 11):
        I = synthetic(NMT_CFG, seed)
        batches.append(argparse.Namespace(src=I["src"].cuda(), tgt=I["tgt"].cuda(), lengths=I["lengths"]))
    tr.train_nmt(batches[0])                                                # (non-trivial optimizer state)

    def snapshot():
        torch.cuda.synchronize()
        snap = {k: v.detach().cpu().clone() for k, v in tr.nmt_model.state_dict().items()}
        a = tr.optim.nmt_arena
        snap["exp_avg"], snap["exp_avg_sq"] = a.exp_avg.cpu().clone(), a.exp_avg_sq.cpu().clone()
        return snap, (tr.optim._step, tr.optim._nmt_steps)
    before = snapshot()
    assert tr.nmt_model.training and tr.best_nmt_val_acc is None
    tr.eval_nmt(batches)
    assert tr.nmt_model.training
    after = snapshot()
    assert before[1] == after[1] and all(torch.equal(before[0][k], after[0][k]) for k in before[0])
    # the same batches by hand: eval mode (no dropout), Statistics over uic_loss / uic_stats
    want = Statistics()
    tr.nmt_model.eval()
    with torch.no_grad():
        for b in batches:
            out, _, _, _ = tr.nmt_model(b.src, b.tgt, b.lengths, None)
            n_correct, n_words = [int(x) for x in out.uic_stats.tolist()]
            want.update(Statistics(float(out.uic_loss), n_words, n_correct))
    tr.nmt_model.train()
    # accuracy is a ratio of integers: exact.  The NLL is an f32 sum over n_words terms whose order the kernel does not fix:
    # |d loss| <= n_words 2^-24 |loss|, and ppl = exp(loss / n_words) moves by ppl * |d loss| / n_words
    assert tr.nmt_valid_acc == want.accuracy() and want.n_words > 0
    print("ppl", tr.nmt_valid_ppl, want.ppl())
    assert abs(tr.nmt_valid_ppl - want.ppl()) <= want.ppl() * 2.0 ** -24 * abs(want.loss)
    assert tr.best_flag_nmt and tr.best_nmt_val_acc == tr.nmt_valid_acc
    tr.best_flag_nmt = False
    tr.eval_nmt(batches)
    assert not tr.best_flag_nmt                                             # strict >
