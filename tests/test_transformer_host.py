"""CPU-side checks of the Transformer captioner (no GPU): the restatement of tests/transformer_cases.py reproduces every fixture
generated from the reference's own module, `models.setup` builds a model with exactly the reference's state_dict, the modes that
are not built raise, and the device limits agree with their restatement."""
import argparse

import pytest
import torch

import transformer_cases as TC


def _opt(cfg, **kw):
    base = dict(vocab_size=cfg["V"], input_encoding_size=cfg["d_model"], rnn_size=cfg["d_ff"], num_layers=cfg["N"], drop_prob_lm=0.5,
                seq_length=cfg["L"], att_feat_size=cfg["D"], fc_feat_size=cfg["D"], use_bn=cfg["use_bn"], caption_model="transformer",
                compute_dtype="f32")
    base.update(kw)
    return argparse.Namespace(**base)


@pytest.fixture(scope="module", params=TC.FIXTURES)
def fx(request):
    """A fixture with weights and inputs in float64, as the reference ran when the fixture was made (its stored f32 values convert
    exactly): the comparison then measures the restatement, not f32 rounding -- which alone is 1.3e-5 at these log-probs of 30-40."""
    cfg, W, I, O = TC.load_fixture(request.param)
    I = {k: (v.double() if v.is_floating_point() else v) for k, v in I.items()}
    return cfg, TC.cast_weights(W, torch.float64), I, O


def test_restatement_reproduces_the_reference_forward(fx):
    cfg, W, I, O = fx
    taps = {}
    memory, _ = TC.encode(W, I["att_feats"], I.get("att_masks"), cfg["N"], cfg["use_bn"], taps=taps)
    for name, got in (("att_embed", taps["att_embed"]), ("enc0.after_attn", taps["enc0.after_attn"]), ("enc0.out", taps["enc0.out"]),
                      ("memory", memory)):
        assert got.shape == O[name].shape, name
        assert (got - O[name]).abs().max().item() < 1e-5, (name, (got - O[name]).abs().max().item())
    logp = TC.forward(W, I["att_feats"], I.get("att_masks"), I["labels"], cfg["N"], cfg["use_bn"])
    assert logp.shape == (cfg["n_img"], cfg["L"] + 1, cfg["V"] + 1)
    assert (logp - O["logprobs"]).abs().max().item() < 1e-5


@pytest.mark.parametrize("name", [n for n in TC.FIXTURES if n != "transformer_nomask"])
def test_padded_regions_are_exact_zeros_and_still_encoded(name):
    cfg, W, I, O = TC.load_fixture(name)
    dead = I["att_masks"] == 0
    assert dead.any()
    assert (O["att_embed"][dead] == 0).all()
    assert (O["memory"][dead].abs().sum(-1) > 0).all()      # the encoder runs over them: they are masked as keys only


def test_restatement_reproduces_greedy_and_beam(fx):
    cfg, W, I, O = fx
    N, bn, L = cfg["N"], cfg["use_bn"], cfg["L"]
    seq, lp, _ = TC.sample_greedy(W, I["att_feats"], I.get("att_masks"), L, N, bn)
    assert torch.equal(seq, O["greedy_seq"])
    assert (lp - O["greedy_logprobs"]).abs().max().item() < 1e-5
    bseq, blp, done, _ = TC.beam_search(W, I["att_feats"], I.get("att_masks"), L, N, bn, cfg["beam"])
    assert torch.equal(bseq, O["beam_seq"])
    assert (blp - O["beam_logprobs"]).abs().max().item() < 1e-5
    for k, d in enumerate(done):
        assert len(d) == int(O["done_count"][k])
        for i, (s, l, p) in enumerate(d):
            assert torch.equal(s, O["done_seq"][k, i])
            assert (l - O["done_logps"][k, i]).abs().max().item() < 1e-5
            assert abs(p - float(O["done_p"][k, i])) < 1e-4


def test_decisions_of_the_fixtures_are_clear(fx):
    """The condition on the seeds: every live greedy step and every beam decision has a gap >= 1e-2 (ten times the f32 log-prob
    tolerance), measured in float64."""
    cfg, W, I, O = fx
    seq, _, gap = TC.sample_greedy(W, I["att_feats"], I.get("att_masks"), cfg["L"], cfg["N"], cfg["use_bn"])
    bseq, _, _, bgap = TC.beam_search(W, I["att_feats"], I.get("att_masks"), cfg["L"], cfg["N"], cfg["use_bn"], cfg["beam"])
    assert torch.equal(seq, O["greedy_seq"]) and torch.equal(bseq, O["beam_seq"])
    assert gap >= 1e-2 and bgap >= 1e-2, (gap, bgap)


def test_incremental_decoding_equals_teacher_forcing_in_the_restatement(fx):
    cfg, W, I, O = fx
    seq = O["greedy_seq"]
    lp = TC.rescore(W, I["att_feats"], I.get("att_masks"), seq, cfg["N"], cfg["use_bn"])
    live = TC.live_positions(seq)
    assert ((lp - O["greedy_logprobs"]).abs() * live).max().item() < 1e-5


def test_setup_builds_the_reference_state_dict(fx):
    """Fails before `models.setup` knows 'transformer'."""
    from unpaired_image_captioning_amd import models
    cfg, W, I, O = fx
    model = models.setup(_opt(cfg))
    sd = model.state_dict()
    assert list(sd.keys()) == list(cfg["shapes"].keys()) == TC.state_dict_keys(cfg, cfg["use_bn"])
    for k, v in sd.items():
        assert tuple(v.shape) == cfg["shapes"][k], k
    assert tuple(sd["model.tgt_embed.1.pe"].shape) == (1, 5000, cfg["d_model"])
    model.load_state_dict(W, strict=True)             # (copy_ converts the float64 tensors back, exactly)
    assert model.att_embed[1 if cfg["use_bn"] else 0].weight.dtype == torch.float32
    assert "model.tgt_embed.1.pe" in dict(model.named_buffers())


def test_xavier_initialisation_of_every_matrix():
    from unpaired_image_captioning_amd import models
    cfg = dict(V=50, d_model=64, d_ff=100, N=1, L=7, D=64, use_bn=0)
    torch.manual_seed(0)
    model = models.setup(_opt(cfg))
    for k, p in model.model.named_parameters():
        if p.dim() > 1:
            bound = (6.0 / (p.shape[0] + p.shape[1])) ** 0.5
            assert p.abs().max().item() <= bound and p.abs().max().item() > 0.8 * bound, k


def test_training_mode_and_decoding_constraint_raise():
    from unpaired_image_captioning_amd import models
    from unpaired_image_captioning_amd.trainer import Trainer
    cfg = dict(V=50, d_model=64, d_ff=100, N=1, L=7, D=64, use_bn=0)
    model = models.setup(_opt(cfg))
    fc, att, seq = torch.zeros(2, 8), torch.zeros(2, 3, 64), torch.zeros(2, 9, dtype=torch.int64)
    model.train()
    for call in (lambda: model(fc, None, att, seq, None), lambda: model(fc, None, att, None, opt={}, mode='sample'),
                 lambda: model(fc, None, att, None, opt={'beam_size': 3}, mode='sample'),
                 lambda: model._sample_beam(fc, None, att, None, {'beam_size': 3})):
        with pytest.raises(NotImplementedError, match="evaluation and decoding only; training is not built"):
            call()
    model.eval()
    with pytest.raises(NotImplementedError, match="undefined name"):
        model(fc, None, att, None, opt={'decoding_constraint': 1}, mode='sample')
    with pytest.raises(RuntimeError, match="device tensors"):          # no eager fallback
        model(fc, None, att, seq, None)
    with pytest.raises(NotImplementedError, match="evaluation and decoding only; training is not built"):
        Trainer(_opt(cfg, i2t_train_flag=1))
    tr = Trainer(_opt(cfg, i2t_train_flag=0))
    assert type(tr.i2t_model).__name__ == "TransformerModel" and not tr.i2t_model.training


def test_unsupported_sizes_are_refused_at_construction():
    from unpaired_image_captioning_amd import models
    cfg = dict(V=50, d_model=64, d_ff=100, N=1, L=7, D=64, use_bn=0)
    for kw in (dict(input_encoding_size=100), dict(input_encoding_size=2048), dict(num_layers=9), dict(seq_length=128), dict(use_bn=3)):
        with pytest.raises((NotImplementedError, ValueError)):
            models.setup(_opt(cfg, **kw))
    for caption_model in ("att2in", "denseatt"):
        with pytest.raises(Exception, match="not supported"):
            models.setup(_opt(cfg, caption_model=caption_model))


def test_device_limits_and_padding_restated():
    from unpaired_image_captioning_amd import _lib
    assert TC.d_ff_padded(1300) == 1304 == _lib.transformer_d_ff_padded(1300)
    for d_ff in (1, 8, 100, 128, 1300, 2048):
        p = _lib.transformer_d_ff_padded(d_ff)
        assert p == TC.d_ff_padded(d_ff) and p % 8 == 0 and 0 <= p - d_ff < 8
    # every supported (Sk, d_k) fits the 160 KB of LDS of a gfx950 workgroup, the largest with room to spare
    assert (_lib.MHA_MAX_SK, _lib.MHA_MAX_DK) == (128, 128)
    for Sk in (1, 5, 36, 63, 64, 65, 100, 128):
        for d_k in (8, 16, 64, 128):
            assert TC.mha_supported(Sk, d_k)
            assert _lib.mha_lds_bytes(Sk, d_k) == TC.mha_lds_bytes(Sk, d_k) <= TC.LDS_BYTES
    assert not TC.mha_supported(129, 64) and not TC.mha_supported(64, 12) and not TC.mha_supported(64, 136)
    assert TC.mha_lds_bytes(128, 128) == 135680
    # the argument checks of the C entry points run before any device work: usable without a GPU
    import ctypes as C
    lib = _lib.load()
    d = _lib.TransformerDims(N=8, R=36, D=2048, d_model=512, d_ff=1300, layers=6, V1=9488, T=17, beam=1, dtype=1, use_bn=1)
    ws, dv = lib.uic_transformer_workspace_bytes(C.byref(d)), lib.uic_transformer_derived_bytes(C.byref(d))
    assert ws > 0 and ws % 256 == 0 and dv > 2 * (6 * (12 * 512 * 512 + 4 * 512 * 1304))
    d.R = 129
    assert lib.uic_transformer_workspace_bytes(C.byref(d)) == 0 and b"R=129" in lib.uic_last_error_string()
    d.R, d.d_model = 36, 520
    assert lib.uic_transformer_workspace_bytes(C.byref(d)) == 0
    assert lib.uic_mha_fwd(0, 1, 1, 129, 64, 1, 512, 0, 1, 512, 0, 1, 512, 0, 1, 512, 0, None, 0, 0, 0, 1, None) == -1
    assert b"Sk=129" in lib.uic_last_error_string()
    assert lib.uic_mha_fwd(0, 1, 1, 64, 12, 1, 512, 0, 1, 512, 0, 1, 512, 0, 1, 512, 0, None, 0, 0, 0, 1, None) == -1
    assert lib.uic_layernorm_std(0, 0, 1, 2048, 1, 2048, 1, 1, 1e-6, 1, 2048, None) == -1
    assert lib.uic_layernorm_std(0, 0, 1, 1, 1, 1, 1, 1, 1e-6, 1, 1, None) == -1


def _reference_default_opt():
    import json
    import os
    with open(os.path.join(TC.GOLDEN, "opts_default.json")) as f:
        return argparse.Namespace(**json.load(f))


def test_reference_default_options_with_the_training_flag_cleared_build_the_model():
    """parse_opt() with no flags names caption_model = 'transformer' for a TRAINING run (i2t_train_flag = 1): setup refuses that, as
    it did before the model existed.  The same options with the flag cleared -- what an evaluation of a checkpoint trained with them
    sets -- build the model at the reference's widths: d_model 512, d_ff 1300, att_feat_size 2053 with the box features."""
    from unpaired_image_captioning_amd import models
    from unpaired_image_captioning_amd.trainer import Trainer
    opt = _reference_default_opt()
    assert (opt.caption_model, opt.rnn_size, opt.use_bn, opt.use_box, opt.i2t_train_flag) == ("transformer", 1300, 1, 1, 1)
    if opt.use_box:
        opt.att_feat_size = opt.att_feat_size + 5            # P/train.py:22
    opt.vocab_size, opt.seq_length = 50, 8                   # P/train.py:25-26 (from the loader)
    with pytest.raises(NotImplementedError, match="not supported by the MI355X hot path.*training is not built"):
        models.setup(opt)
    with pytest.raises(NotImplementedError, match="evaluation and decoding only; training is not built"):
        Trainer(opt)
    opt.i2t_train_flag = 0
    model = models.setup(opt)
    assert type(model).__name__ == "TransformerModel" and model.use_bn == 1 and model._D8 == 2056
    sd = model.state_dict()
    assert tuple(sd["att_embed.1.weight"].shape) == (512, 2053)
    assert tuple(sd["model.encoder.layers.0.feed_forward.w_1.weight"].shape) == (1300, 512)
    assert tuple(sd["model.tgt_embed.1.pe"].shape) == (1, 5000, 512)
    assert list(sd) == TC.state_dict_keys(opt.num_layers, 1)
    tr = Trainer(opt)
    assert tr.i2t_model is not None and not tr.i2t_model.training
