"""The AdaAtt captioners on the device (AdaAttModel / AdaAttMOModel over csrc/adaatt.hip) against the fixtures generated from the
reference's own classes and against the float64 restatement of tests/adaatt_cases.py.

Between them the fixtures cover adaatt and adaattmo, one and two LSTM layers, logit_layers 1 / 2, use_bn 0 / 1 / 2 with non-trivial
running statistics, att_masks=None, ragged regions including an image with one region, an empty caption.  Tolerances: the project's
1e-3 on f32 log-probs; token ids exactly on f32 (the fixtures' decisions have gaps >= 1e-2, asserted in test_adaatt_host.py).
bf16: max(1e-2, 4 x the deviation of the bf16-emulating restatement on the same case) (adaatt_cases.BF16_EMULATED); there the
device's own tokens are re-scored by the restatement."""
import argparse
import functools

import pytest
import torch

import adaatt_cases as AC

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(autouse=True)
def _poisoned_adaatt_workspace(monkeypatch):
    """Every call finds its workspace filled with 0xFF bytes (NaN in f32 and bf16, -1 in the integer buffers): no result may depend on
    what an earlier call left there."""
    from unpaired_image_captioning_amd.models.AttModel import AdaAttModel
    orig = AdaAttModel._workspace

    def workspace(self, lib, d, device):
        ws = orig(self, lib, d, device)
        ws.fill_(255)
        return ws

    monkeypatch.setattr(AdaAttModel, "_workspace", workspace)
    yield


@functools.lru_cache(maxsize=None)
def _fixture(name):
    cfg, W, I, O = AC.load_fixture(name)
    I64 = (I["fc_feats"].double(), I["att_feats"].double(), I["att_masks"].double() if "att_masks" in I else None)
    return cfg, W, I, O, AC.to64(W), I64


@functools.lru_cache(maxsize=None)
def _bound(name, dtype):
    if dtype == "f32":
        return AC.TOL_F32
    cfg, W, I, O, W64, (fc, att, am) = _fixture(name)
    return AC.bf16_bounds(name, W64, cfg, fc, att, am, I["labels"])


def _model(cfg, W, dtype):
    from unpaired_image_captioning_amd import models
    m = models.setup(AC.opt_of(cfg, dtype))
    m.load_state_dict(W, strict=True)
    return m.to(DEV).eval()


def _inputs(I):
    return I["fc_feats"].to(DEV), I["att_feats"].to(DEV), (I["att_masks"].to(DEV) if "att_masks" in I else None)


CASES = [(n, d) for n in AC.FIXTURES for d in ("f32", "bf16")]


@pytest.mark.parametrize("name,dtype", CASES)
def test_forward_and_recorded_steps_match_the_reference(name, dtype):
    cfg, W, I, O, W64, I64 = _fixture(name)
    m = _model(cfg, W, dtype)
    fc, att, am = _inputs(I)
    tol = _bound(name, dtype)
    logp = m(fc, None, att, I["labels"].to(DEV), am)
    assert logp.shape == O["logprobs"].shape and logp.dtype == torch.float32
    err = (logp.cpu().double() - O["logprobs"]).abs().max().item()
    print("%s %s: max |d log-prob| = %.3g (bound %.3g)" % (name, dtype, err, tol))
    assert err < tol
    # _prepare_feature, then the three recorded steps of get_logprobs_state fed with the caption's own tokens
    p_fc, p_att, pp_att, p_m = m._prepare_feature(fc, att, am)
    ftol = 1e-5 if dtype == "f32" else tol
    assert (p_fc.cpu().double() - O["fc_embed"]).abs().max().item() < ftol * 10
    assert (p_att.cpu().double() - O["att_embed"]).abs().max().item() < ftol * 10 and (pp_att.cpu().double() - O["p_att"]).abs().max().item() < ftol * 10
    state = m.init_hidden(fc.shape[0])
    assert tuple(state[0].shape) == (cfg["layers"], fc.shape[0], cfg["H"])
    for i in range(3):
        lp, state = m.get_logprobs_state(I["labels"][:, i].to(DEV), p_fc, p_att, pp_att, p_m, state)
        assert (lp.cpu().double() - O["step%d_logprobs" % i]).abs().max().item() < tol, i
        assert (state[0].cpu().double() - O["step%d_h" % i]).abs().max().item() < tol and \
            (state[1].cpu().double() - O["step%d_c" % i]).abs().max().item() < tol, i


@pytest.mark.parametrize("name", AC.FIXTURES)
def test_greedy_ids_exact_f32_and_equal_to_teacher_forcing(name):
    cfg, W, I, O, W64, I64 = _fixture(name)
    m = _model(cfg, W, "f32")
    fc, att, am = _inputs(I)
    seq, lp = m(fc, None, att, am, opt={"sample_max": 1}, mode="sample")
    assert seq.shape == (cfg["n_img"], cfg["L"]) and seq.dtype == torch.int64
    assert torch.equal(seq.cpu(), O["greedy_seq"])
    assert (lp.cpu().double() - O["greedy_logprobs"]).abs().max().item() < AC.TOL_F32
    # decoding equals the teacher-forced pass over the decoded tokens
    z = torch.zeros(seq.shape[0], 1, dtype=torch.int64, device=DEV)
    logp = m(fc, None, att, torch.cat([z, seq, z], 1), am)[:, :cfg["L"]]
    again = logp.gather(2, seq[:, :, None]).squeeze(2)
    live = AC.live_positions(seq.cpu())
    assert live.any() and ((again - lp).abs().cpu() * live).max().item() < AC.TOL_F32


@pytest.mark.parametrize("name", AC.FIXTURES)
def test_greedy_bf16_tokens_rescored_by_the_restatement(name):
    cfg, W, I, O, W64, (fc64, att64, am64) = _fixture(name)
    m = _model(cfg, W, "bf16")
    fc, att, am = _inputs(I)
    seq, lp = m(fc, None, att, am, opt={"sample_max": 1}, mode="sample")
    seq, lp = seq.cpu(), lp.cpu().double()
    assert int(seq.min()) >= 0 and int(seq.max()) <= cfg["V"]
    chosen, top = AC.rescore(W64, cfg, fc64, att64, am64, seq)
    live = AC.live_positions(seq)
    tol = _bound(name, "bf16")
    assert ((chosen - lp).abs() * live).max().item() < tol
    # every live choice is the restatement's arg-max up to twice the bound (the winner and the runner-up each move by one)
    assert ((top - chosen) * live).max().item() < 2 * tol
    assert (seq[~live] == 0).all()


@pytest.mark.parametrize("name", AC.FIXTURES)
def test_beam_ids_and_done_lists_exact_f32(name):
    cfg, W, I, O, W64, I64 = _fixture(name)
    m = _model(cfg, W, "f32")
    fc, att, am = _inputs(I)
    B = cfg["beam"]
    seq, lp = m(fc, None, att, am, opt={"beam_size": B}, mode="sample")
    assert torch.equal(seq.cpu(), O["beam_seq"])
    assert (lp.cpu().double() - O["beam_logprobs"]).abs().max().item() < AC.TOL_F32
    done = m.done_beams
    assert len(done) == cfg["n_img"]
    for k, d in enumerate(done):
        assert len(d) == int(O["done_count"][k])
        for i, b in enumerate(d):
            assert torch.equal(b["seq"].cpu(), O["done_seq"][k, i])
            assert (b["logps"].cpu().double() - O["done_logps"][k, i]).abs().max().item() < AC.TOL_F32
            assert abs(b["p"] - float(O["done_p"][k, i])) < AC.TOL_F32 * cfg["L"]
    seq2, _ = m(fc, None, att, am, opt={"beam_size": 2 * B, "group_size": 2}, mode="sample")
    assert torch.equal(seq2, seq)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("temperature", [1.0, 0.7])
def test_sampled_tokens_rescore_to_their_reported_logprobs(dtype, temperature):
    name = "adaattmo_tiny"
    cfg, W, I, O, W64, (fc64, att64, am64) = _fixture(name)
    m = _model(cfg, W, dtype)
    fc, att, am = _inputs(I)
    seq, lp = m(fc, None, att, am, opt={"sample_max": 0, "temperature": temperature}, mode="sample")
    seq2, _ = m(fc, None, att, am, opt={"sample_max": 0, "temperature": temperature}, mode="sample")
    seq, lp = seq.cpu(), lp.cpu().double()
    assert not torch.equal(seq, O["greedy_seq"]) or not torch.equal(seq2.cpu(), O["greedy_seq"])      # draws, not arg-maxes
    chosen, _ = AC.rescore(W64, cfg, fc64, att64, am64, seq)
    live = AC.live_positions(seq)
    assert ((chosen - lp).abs() * live).max().item() < _bound(name, dtype)
    assert (seq[~live] == 0).all()


def test_decoding_constraint():
    """No token follows itself (:220-223); the tokens are the restatement's under the same rule."""
    name = "adaatt_tiny"
    cfg, W, I, O, W64, (fc64, att64, am64) = _fixture(name)
    assert any(int(r[t]) == int(r[t + 1]) != 0 for r in O["greedy_seq"] for t in range(cfg["L"] - 1))      # the rule changes this case
    m = _model(cfg, W, "f32")
    fc, att, am = _inputs(I)
    seq, lp = m(fc, None, att, am, opt={"sample_max": 1, "decoding_constraint": 1}, mode="sample")
    seq = seq.cpu()
    live = AC.live_positions(seq)
    assert not ((seq[:, 1:] == seq[:, :-1]) & live[:, 1:] & (seq[:, 1:] > 0)).any()
    ref, rlp, gap = AC.sample_greedy(W64, cfg, fc64, att64, am64, decoding_constraint=1)
    if gap >= AC.MIN_GAP:
        assert torch.equal(seq, ref) and ((lp.cpu().double() - rlp).abs() * live).max().item() < AC.TOL_F32
    else:       # a close decision under the rule: the device's tokens re-scored instead
        chosen, _ = AC.rescore(W64, cfg, fc64, att64, am64, seq)
        assert ((chosen - lp.cpu().double()).abs() * live).max().item() < AC.TOL_F32


def test_load_state_dict_then_the_next_call_uses_the_new_weights():
    name = "adaatt_tiny"
    cfg, W, I, O, W64, (fc64, att64, am64) = _fixture(name)
    m = _model(cfg, W, "f32")
    fc, att, am = _inputs(I)
    a = m(fc, None, att, I["labels"].to(DEV), am)
    W2 = {k: (v * 0.5 if k in ("logit.weight", "core.lstm.r_h2h.weight") else v) for k, v in W.items()}
    m.load_state_dict(W2, strict=True)
    b = m(fc, None, att, I["labels"].to(DEV), am)
    ref = AC.forward(AC.to64(W2), cfg, fc64, att64, am64, I["labels"])
    assert (a - b).abs().max().item() > 0.1 and (b.cpu().double() - ref).abs().max().item() < AC.TOL_F32
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    assert list(sd) == list(cfg["shapes"]) and all(torch.equal(sd[k], W2[k]) for k in W2)


@pytest.mark.parametrize("use_bn", [0, 1])
def test_feature_sizes_that_are_no_multiple_of_8(use_bn):
    """att_feat_size 2053 with the reference's default use_box = 1; here 53 (and fc_feat_size 27): zero-padded to 56 / 32."""
    cfg = dict(V=50, H=16, D=53, Dfc=27, layers=1, logit_layers=1, L=7, use_bn=use_bn, maxout=1, n_img=3)
    W = AC.make_weights(cfg, seed=21)
    fc, att, am, labels = AC.synthetic_inputs(50, 53, 27, 3, 5, 7, "ragged", 22)
    m = _model(cfg, W, "f32")
    logp = m(fc.to(DEV), None, att.to(DEV), labels.to(DEV), am.to(DEV))
    ref = AC.forward(AC.to64(W), cfg, fc.double(), att.double(), am.double(), labels)
    assert (logp.cpu().double() - ref).abs().max().item() < AC.TOL_F32
    again = m(fc.to(DEV), None, att.to(DEV), labels.to(DEV), am.to(DEV))     # (the padded copies are kept)
    assert torch.equal(again, logp)


@functools.lru_cache(maxsize=None)
def _real_reference():
    c, W, fc, att, am, labels = AC.real_case()
    W64 = AC.to64(W)
    ref = AC.forward(W64, c, fc.double(), att.double(), am.double(), labels)
    return W64, ref, AC.bf16_bounds("real", W64, c, fc.double(), att.double(), am.double(), labels)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_real_widths_against_the_restatement(dtype):
    """E = H = A = 512, D = 2048, R = 36, V = 9487, L = 16, 4 images."""
    c, W, fc, att, am, labels = AC.real_case()
    W64, ref, bf16_tol = _real_reference()
    m = _model(c, W, dtype)
    logp = m(fc.to(DEV), None, att.to(DEV), labels.to(DEV), am.to(DEV))
    err = (logp.cpu().double() - ref).abs().max().item()
    tol = AC.TOL_F32 if dtype == "f32" else bf16_tol
    print("real widths %s: max |d log-prob| = %.3g (bound %.3g)" % (dtype, err, tol))
    assert err < tol
    # decode: the device's own greedy tokens re-scored by the restatement; beam search runs and returns finished captions
    seq, lp = m(fc.to(DEV), None, att.to(DEV), am.to(DEV), opt={"sample_max": 1}, mode="sample")
    seq, lp = seq.cpu(), lp.cpu().double()
    assert seq.shape == (c["n_img"], c["L"])
    chosen, top = AC.rescore(W64, c, fc.double(), att.double(), am.double(), seq)
    live = AC.live_positions(seq)
    assert ((chosen - lp).abs() * live).max().item() < tol
    assert ((top - chosen) * live).max().item() < 2 * tol
    bseq, blp = m(fc.to(DEV), None, att.to(DEV), am.to(DEV), opt={"beam_size": 3}, mode="sample")
    bchosen, _ = AC.rescore(W64, c, fc.double(), att.double(), am.double(), bseq.cpu())
    blive = AC.live_positions(bseq.cpu())
    assert ((bchosen - blp.cpu().double()).abs() * blive).max().item() < tol


def test_eval_split_end_to_end_on_the_synthetic_loader(tmp_path):
    """Trainer.eval with caption_model='adaattmo', i2t_train_flag=0: 11 images (7 'val', batches of 3), 2 captions per image in the
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
    opt = argparse.Namespace(vocab_size=V, input_encoding_size=32, rnn_size=32, att_hid_size=32, num_layers=2, drop_prob_lm=0.5, seq_length=L,
                             use_bn=1, logit_layers=1, caption_model="adaattmo", compute_dtype="f32", seed=2, i2t_train_flag=0, i2t_eval_flag=1,
                             language_eval=1, beam_size=1, verbose=False, **vars(lo))
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
    tr.opt.beam_size = 2
    tr.opt.verbose_beam = 0
    tr.eval(loader)
    assert len(tr.predictions) == 7
