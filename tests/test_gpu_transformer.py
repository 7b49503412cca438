"""The Transformer captioner on the device (models/TransformerModel.py over csrc/transformer.hip) against the fixtures generated
from the reference's own module and against the float64 restatement of tests/transformer_cases.py.

Between them the fixtures cover N in {1, 2}, d_model in {64, 128}, d_ff in {100, 128}, V + 1 = 51, L = 7, use_bn 0 / 1 / 2 with
non-trivial running statistics, att_masks=None, ragged regions including an image with one region, an empty caption (labels and
decoded).  Tolerances: the project's 1e-3 on f32 log-probs; token ids exactly on f32 (the fixtures' decisions have gaps >= 1e-2, asserted in
test_transformer_host.py).  bf16: 4 x the deviation of the bf16-emulating restatement on the same case (transformer_cases.py,
BF16_EMULATED: the project's 1e-2 is out of reach of any bf16 evaluation of log-probs of magnitude 20-40); there the device's own
tokens are re-scored by the restatement."""
import argparse
import functools

import pytest
import torch

import transformer_cases as TC

pytestmark = pytest.mark.gpu

DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _bounds(name, dtype):
    """(log-prob bound, memory bound) of a fixture on `dtype`."""
    if dtype == "f32":
        return TC.TOL_F32, TC.TOL_F32
    cfg, W, I, O, W64, I64 = _fixture(name)
    return TC.bf16_bounds(name, W64, I64["att_feats"], I64.get("att_masks"), I["labels"], cfg["N"], cfg["use_bn"])


def _opt(cfg, dtype, **kw):
    base = dict(vocab_size=cfg["V"], input_encoding_size=cfg["d_model"], rnn_size=cfg["d_ff"], num_layers=cfg["N"], drop_prob_lm=0.5,
                seq_length=cfg["L"], att_feat_size=cfg["D"], fc_feat_size=cfg["D"], use_bn=cfg["use_bn"], caption_model="transformer",
                compute_dtype=dtype)
    base.update(kw)
    return argparse.Namespace(**base)


@functools.lru_cache(maxsize=None)
def _fixture(name):
    cfg, W, I, O = TC.load_fixture(name)
    W64 = TC.cast_weights(W, torch.float64)
    I64 = {k: (v.double() if v.is_floating_point() else v) for k, v in I.items()}
    return cfg, W, I, O, W64, I64


def _model(cfg, W, dtype):
    from unpaired_image_captioning_amd import models
    m = models.setup(_opt(cfg, dtype))
    m.load_state_dict(W, strict=True)
    return m.to(DEV).eval()


def _inputs(I):
    att = I["att_feats"].to(DEV)
    am = I["att_masks"].to(DEV) if "att_masks" in I else None
    fc = torch.zeros(att.shape[0], 8, device=DEV)
    return fc, att, am


CASES = [(n, d) for n in TC.FIXTURES for d in ("f32", "bf16")]


@pytest.mark.parametrize("name,dtype", CASES)
def test_forward_and_memory_match_the_reference(name, dtype):
    cfg, W, I, O, W64, I64 = _fixture(name)
    m = _model(cfg, W, dtype)
    fc, att, am = _inputs(I)
    logp = m(fc, None, att, I["labels"].to(DEV), am)
    assert logp.shape == O["logprobs"].shape and logp.dtype == torch.float32
    err = (logp.cpu().double() - O["logprobs"]).abs().max().item()
    print("%s %s: max |d log-prob| = %.3g" % (name, dtype, err))
    tol, mtol = _bounds(name, dtype)
    assert err < tol
    mem = m.encode(att, am).cpu().double()
    merr = (mem - O["memory"]).abs().max().item()
    print("%s %s: max |d memory| = %.3g" % (name, dtype, merr))
    assert merr < mtol


@pytest.mark.parametrize("name", TC.FIXTURES)
def test_greedy_ids_exact_f32_and_cache_equals_teacher_forcing(name):
    cfg, W, I, O, W64, I64 = _fixture(name)
    m = _model(cfg, W, "f32")
    fc, att, am = _inputs(I)
    seq, lp = m(fc, None, att, am, opt={"sample_max": 1}, mode="sample")
    assert seq.shape == (cfg["n_img"], cfg["L"]) and seq.dtype == torch.int64
    assert torch.equal(seq.cpu(), O["greedy_seq"])
    assert (lp.cpu().double() - O["greedy_logprobs"]).abs().max().item() < TC.TOL_F32
    # incremental decoding (K/V cache, one position per step) equals the teacher-forced pass over the decoded tokens
    full = torch.cat([torch.zeros(seq.shape[0], 1, dtype=torch.int64, device=DEV), seq, torch.zeros(seq.shape[0], 1, dtype=torch.int64, device=DEV)], 1)
    logp = m(fc, None, att, full, am)[:, :cfg["L"]]
    again = logp.gather(2, seq[:, :, None]).squeeze(2)
    live = TC.live_positions(seq.cpu())
    assert live.any() and ((again - lp).abs().cpu() * live).max().item() < TC.TOL_F32


@pytest.mark.parametrize("name", TC.FIXTURES)
def test_greedy_bf16_tokens_rescored_by_the_restatement(name):
    cfg, W, I, O, W64, I64 = _fixture(name)
    m = _model(cfg, W, "bf16")
    fc, att, am = _inputs(I)
    seq, lp = m(fc, None, att, am, opt={"sample_max": 1}, mode="sample")
    seq, lp = seq.cpu(), lp.cpu().double()
    assert int(seq.min()) >= 0 and int(seq.max()) <= cfg["V"]
    full = torch.cat([torch.zeros(seq.shape[0], 1, dtype=torch.int64), seq, torch.zeros(seq.shape[0], 1, dtype=torch.int64)], 1)
    ref = TC.forward(W64, I64["att_feats"], I64.get("att_masks"), full, cfg["N"], cfg["use_bn"])[:, :cfg["L"]]
    live = TC.live_positions(seq)
    chosen = ref.gather(2, seq[:, :, None]).squeeze(2)
    tol, _ = _bounds(name, "bf16")
    assert ((chosen - lp).abs() * live).max().item() < tol
    # every live choice is the restatement's arg-max up to twice the bound (the winner and the runner-up each move by one)
    assert (((ref.max(2).values - chosen) * live).max().item()) < 2 * tol
    # finished rows emit 0 from their first 0 on
    assert (seq[~live] == 0).all()


@pytest.mark.parametrize("name", TC.FIXTURES)
def test_beam_ids_and_done_lists_exact_f32(name):
    cfg, W, I, O, W64, I64 = _fixture(name)
    m = _model(cfg, W, "f32")
    fc, att, am = _inputs(I)
    B = cfg["beam"]
    seq, lp = m(fc, None, att, am, opt={"beam_size": B}, mode="sample")
    assert torch.equal(seq.cpu(), O["beam_seq"])
    assert (lp.cpu().double() - O["beam_logprobs"].double()).abs().max().item() < TC.TOL_F32
    done = m.done_beams
    assert len(done) == cfg["n_img"]
    for k, d in enumerate(done):
        assert len(d) == int(O["done_count"][k])
        for i, b in enumerate(d):
            assert torch.equal(b["seq"].cpu(), O["done_seq"][k, i])
            assert (b["logps"].cpu() - O["done_logps"][k, i]).abs().max().item() < TC.TOL_F32
            assert abs(b["p"] - float(O["done_p"][k, i])) < TC.TOL_F32 * cfg["L"]
    # group_size is handled as models/AttModel.py handles it: the best beam of group 0 = a plain search over beam_size / group_size beams
    seq2, _ = m(fc, None, att, am, opt={"beam_size": 2 * B, "group_size": 2}, mode="sample")
    assert torch.equal(seq2, seq)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("temperature", [1.0, 0.7])
def test_sampled_tokens_rescore_to_their_reported_logprobs(dtype, temperature):
    cfg, W, I, O, W64, I64 = _fixture("transformer_tiny")
    m = _model(cfg, W, dtype)
    fc, att, am = _inputs(I)
    seq, lp = m(fc, None, att, am, opt={"sample_max": 0, "temperature": temperature}, mode="sample")
    seq2, _ = m(fc, None, att, am, opt={"sample_max": 0, "temperature": temperature}, mode="sample")
    seq, lp = seq.cpu(), lp.cpu().double()
    assert not torch.equal(seq, O["greedy_seq"]) or not torch.equal(seq2.cpu(), O["greedy_seq"])      # draws, not arg-maxes
    full = torch.cat([torch.zeros(seq.shape[0], 1, dtype=torch.int64), seq, torch.zeros(seq.shape[0], 1, dtype=torch.int64)], 1)
    ref = TC.forward(W64, I64["att_feats"], I64.get("att_masks"), full, cfg["N"], cfg["use_bn"])[:, :cfg["L"]]
    live = TC.live_positions(seq)
    chosen = ref.gather(2, seq[:, :, None]).squeeze(2)
    assert ((chosen - lp).abs() * live).max().item() < _bounds("transformer_tiny", dtype)[0]
    assert (seq[~live] == 0).all()


def test_state_dict_round_trip_and_refresh_after_load():
    """A second checkpoint loaded into the same model is what the next call computes (the derived copies follow the masters)."""
    cfg, W, I, O, W64, I64 = _fixture("transformer_tiny")
    m = _model(cfg, W, "f32")
    fc, att, am = _inputs(I)
    a = m(fc, None, att, I["labels"].to(DEV), am)
    W2 = {k: (v * 0.5 if k == "model.generator.proj.weight" else v) for k, v in W.items()}
    m.load_state_dict(W2, strict=True)
    b = m(fc, None, att, I["labels"].to(DEV), am)
    ref = TC.forward(TC.cast_weights(W2, torch.float64), I64["att_feats"], I64.get("att_masks"), I["labels"], cfg["N"], cfg["use_bn"])
    assert (a - b).abs().max().item() > 0.1 and (b.cpu().double() - ref).abs().max().item() < TC.TOL_F32
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    assert list(sd) == list(cfg["shapes"]) and all(torch.equal(sd[k], W2[k]) for k in W2)


@pytest.mark.parametrize("use_bn", [0, 1])
def test_att_feat_size_that_is_no_multiple_of_8(use_bn):
    """2053 columns with the reference's default use_box = 1; here 53: the features and att_embed's input side are zero-padded to 56."""
    cfg = dict(V=50, D=53, d_model=64, d_ff=100, N=1, L=7, use_bn=use_bn, n_img=3)
    W = TC.make_weights(cfg["V"] + 1, cfg["D"], cfg["d_model"], cfg["d_ff"], cfg["N"], use_bn, seed=21)
    g = torch.Generator().manual_seed(22)
    att = torch.randn(3, 5, 53, generator=g)
    masks = (torch.arange(5)[None, :] < torch.tensor([5, 2, 4])[:, None]).float()
    labels = torch.zeros(3, 9, dtype=torch.int64)
    labels[:, 1:5] = torch.randint(1, 51, (3, 4), generator=g)
    m = _model(cfg, W, "f32")
    logp = m(torch.zeros(3, 8, device=DEV), None, att.to(DEV), labels.to(DEV), masks.to(DEV))
    ref = TC.forward(TC.cast_weights(W, torch.float64), att.double(), masks.double(), labels, 1, use_bn)
    assert (logp.cpu().double() - ref).abs().max().item() < TC.TOL_F32
    again = m(torch.zeros(3, 8, device=DEV), None, att.to(DEV), labels.to(DEV), masks.to(DEV))     # (the padded copies are kept)
    assert torch.equal(again, logp)


@functools.lru_cache(maxsize=None)
def _real_reference():
    c, W, att, masks, labels = TC.real_case()
    W64 = TC.cast_weights(W, torch.float64)
    ref = TC.forward(W64, att.double(), masks.double(), labels, c["N"], c["use_bn"])
    return W64, ref, TC.bf16_bounds("real", W64, att.double(), masks.double(), labels, c["N"], c["use_bn"])[0]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_real_widths_against_the_restatement(dtype):
    """d_model 512, d_ff 1300 (padded to 1304 in the derived copies), 6 layers, 36 regions x 2048, V 9487, L 16, 8 images."""
    c, W, att, masks, labels = TC.real_case()
    W64, ref, bf16_tol = _real_reference()
    m = _model(dict(c), W, dtype)
    fc = torch.zeros(c["n_img"], 8, device=DEV)
    logp = m(fc, None, att.to(DEV), labels.to(DEV), masks.to(DEV))
    err = (logp.cpu().double() - ref).abs().max().item()
    tol = TC.TOL_F32 if dtype == "f32" else bf16_tol
    print("real widths %s: max |d log-prob| = %.3g (bound %.3g)" % (dtype, err, tol))
    assert err < tol
    # decode: the device's own greedy tokens re-scored by the restatement
    seq, lp = m(fc, None, att.to(DEV), masks.to(DEV), opt={"sample_max": 1}, mode="sample")
    seq, lp = seq.cpu(), lp.cpu().double()
    assert seq.shape == (c["n_img"], c["L"])
    full = torch.cat([torch.zeros(seq.shape[0], 1, dtype=torch.int64), seq, torch.zeros(seq.shape[0], 1, dtype=torch.int64)], 1)
    again = TC.forward(W64, att.double(), masks.double(), full, c["N"], c["use_bn"])[:, :c["L"]]
    live = TC.live_positions(seq)
    chosen = again.gather(2, seq[:, :, None]).squeeze(2)
    assert ((chosen - lp).abs() * live).max().item() < tol
    assert (((again.max(2).values - chosen) * live).max().item()) < 2 * tol


def test_eval_split_end_to_end_on_the_synthetic_loader(tmp_path):
    """Trainer.eval with caption_model='transformer', i2t_train_flag=0: 11 images (7 'val', batches of 3), 2 captions per image in the
    loss, one decoded caption per image, lang_stats scored on the device."""
    import numpy as np
    import lang_eval_cases as LC
    from dataset_files import loader_opt, write_dataset
    from unpaired_image_captioning_amd.misc.dataloader.dataloader import DataLoader
    from unpaired_image_captioning_amd.trainer import Trainer
    V, L, D, n = 20, 6, 16, 11
    g = np.random.default_rng(3)
    ids = [100 + 3 * i for i in range(n)]
    splits = ["val" if i in (0, 1, 3, 4, 6, 7, 9) else "train" for i in range(n)]
    att = [g.standard_normal((int(g.integers(2, 6)), D)).astype(np.float32) for _ in range(n)]
    fc = [g.standard_normal(D).astype(np.float32) for _ in range(n)]
    counts = [int(g.integers(2, 5)) for _ in range(n)]
    end = np.cumsum(counts)
    start = end - np.array(counts) + 1
    labels = LC.caption_rows(g, int(end[-1]), L, V, min_words=1)
    label_path = write_dataset(str(tmp_path), att, None, fc, [(10, 10)] * n, ids, labels, start, end, V, splits=splits)
    lo = loader_opt(str(tmp_path), label_path, 3, 2, D, D, 0, 0, 0)
    opt = argparse.Namespace(vocab_size=V, input_encoding_size=64, rnn_size=100, num_layers=2, drop_prob_lm=0.5, seq_length=L, use_bn=1,
                             caption_model="transformer", compute_dtype="f32", seed=2, i2t_train_flag=0, i2t_eval_flag=1, language_eval=1,
                             beam_size=1, verbose=False, **vars(lo))
    torch.manual_seed(4)
    tr = Trainer(opt)
    tr.i2t_model.to(DEV)
    loader = DataLoader(opt)
    tr.eval(loader)
    assert not tr.i2t_model.training
    assert tr.i2t_val_loss == tr.i2t_val_loss and 0 < tr.i2t_val_loss < 1e3          # finite
    got = [p["image_id"] for p in tr.predictions]
    assert sorted(got) == sorted(ids[i] for i in range(n) if splits[i] == "val") and len(set(got)) == 7     # one caption per image
    assert set(LC.KEYS) <= set(tr.lang_stats) and all(v == v for v in tr.lang_stats.values())
    assert tr.best_flag_i2t and tr.best_i2t_val_score == tr.lang_stats["CIDEr"]
    tr.opt.beam_size = 2
    tr.opt.verbose_beam = 0
    tr.eval(loader)
    assert len(tr.predictions) == 7
