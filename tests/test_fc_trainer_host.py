"""CPU-side checks of the FC captioner's training entry points: exported and declared, refusals with a message before anything
is launched, Trainer(caption_model='fc') constructs, and the SCST restatement of tests/fc_train_cases.py agrees with
oracle/fc.py (it is pinned here before the GPU tests use it)."""
import ctypes as C
import os
import re

import pytest
import torch

import fc_train_cases as FT
from conftest import ROOT, load_golden
from oracle import fc as OF
from oracle import topdown as O

NEW_SYMBOLS = ("uic_fc_xe_train_step", "uic_fc_sample_train", "uic_fc_reward_backward")


def test_new_symbols_are_exported_declared_and_bound():
    from unpaired_image_captioning_amd import _lib
    header = open(os.path.join(ROOT, "include", "uic_hip.h")).read()
    declared = set(re.findall(r"\b(uic_[a-z0-9_]+)\s*\(", header)) - {"uic_topdown_dims", "uic_topdown_weights", "uic_topdown_batch"}
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(raw, name), name
    # header and .so still equal
    assert set(_lib.EXPORTS) == declared, set(_lib.EXPORTS) ^ declared
    for name in sorted(declared):
        assert hasattr(raw, name), name


def _args():
    """Dims, and non-null pointers that a refused call never follows (host memory: nothing may be launched on them)."""
    from unpaired_image_captioning_amd import _lib
    d = _lib.FcDims(N=6, Dfc=64, H=32, E=32, V1=51, S=8, dtype=0, drop_p=0.5)
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    w = _lib.FcWeights()
    for f, _ in _lib.FC_WEIGHT_FIELDS:
        setattr(w, f, p)
    b = _lib.Batch()
    b.fc_feats = b.labels = b.masks = p
    b.ld_labels = b.ld_masks = 8
    return _lib, _lib.load(), d, w, b, p, buf


def _refused(lib, rc, *words):
    msg = lib.uic_last_error_string()
    assert rc != 0 and msg, (rc, msg)
    for word in words:
        assert word in msg, (word, msg)


def test_xe_train_step_refusals():
    _lib, lib, d, w, b, p, keep = _args()
    call = lambda d, w, b, s_run, ws=p, out=p, g=None: lib.uic_fc_xe_train_step(  # noqa: E731
        C.byref(d), C.byref(w) if w else None, C.byref(b) if b else None, s_run, 1, 7, ws, None, out, C.byref(g if g is not None else w) if w else None, None)
    _refused(lib, call(d, None, b, 4), b"fc_xe_train_step", b"null")
    _refused(lib, call(d, w, None, 4), b"null")
    _refused(lib, call(d, w, b, 4, ws=None), b"null")
    _refused(lib, call(d, w, b, 4, out=None), b"null")
    nb = _lib.Batch()
    nb.fc_feats = nb.labels = p
    nb.ld_labels = 8
    _refused(lib, call(d, w, nb, 4), b"null")                       # no masks
    for s_run in (1, 0, -3, 9):
        _refused(lib, call(d, w, b, s_run), b"s_run", b"[2,8]")
    b.ld_masks = 7
    _refused(lib, call(d, w, b, 4), b"columns")
    b.ld_masks = 8
    d.H = 36
    _refused(lib, call(d, w, b, 4), b"multiples of 8")


def test_sample_train_refusals():
    _lib, lib, d, w, b, p, keep = _args()
    call = lambda d, w, b, L, temp=1.0, ws=p, seq=p, lp=p: lib.uic_fc_sample_train(  # noqa: E731
        C.byref(d), C.byref(w) if w else None, C.byref(b) if b else None, L, temp, 7, None, ws, seq, lp, None)
    _refused(lib, call(d, None, b, 6), b"fc_sample_train", b"null")
    _refused(lib, call(d, w, None, 6), b"null")
    _refused(lib, call(d, w, b, 6, ws=None), b"null")
    _refused(lib, call(d, w, b, 6, seq=None), b"null")
    _refused(lib, call(d, w, b, 6, lp=None), b"null")
    for L in (0, -1, 8, 100):
        _refused(lib, call(d, w, b, L), b"L=")
    _refused(lib, call(d, w, b, 6, temp=0.0), b"temperature")
    d.E = 12
    _refused(lib, call(d, w, b, 6), b"multiples of 8")


def test_reward_backward_refusals():
    _lib, lib, d, w, b, p, keep = _args()
    call = lambda d, w, b, L, ws=p, g=p, G=True: lib.uic_fc_reward_backward(  # noqa: E731
        C.byref(d), C.byref(w) if w else None, C.byref(b) if b else None, L, 7, ws, g, C.byref(w) if (G and w) else None, None)
    _refused(lib, call(d, None, b, 6), b"fc_reward_backward", b"null")
    _refused(lib, call(d, w, None, 6), b"null")
    _refused(lib, call(d, w, b, 6, ws=None), b"null")
    _refused(lib, call(d, w, b, 6, g=None), b"null")
    _refused(lib, call(d, w, b, 6, G=False), b"null")
    for L in (0, -1, 8):
        _refused(lib, call(d, w, b, L), b"L=")


def test_trainer_constructs_an_fc_model_in_train_mode():
    from unpaired_image_captioning_amd.models.FCModel_NMT import FCModel_NMT
    from unpaired_image_captioning_amd.trainer import Trainer
    cfg = load_golden("fc_tiny")[0]
    tr = Trainer(FT.make_opt(cfg, "f32", drop=0.5))
    assert isinstance(tr.i2t_model, FCModel_NMT) and tr.i2t_model.training
    eng = tr.i2t_model.engine
    for name in ("xe_train_step", "sample_train", "reward_backward"):
        assert callable(getattr(eng, name))
    assert tr.i2t_model.supports_grad_sink and not tr.i2t_model.uses_att_feats
    # scheduled sampling stays refused (broken in the reference), through the Trainer's step as through the model call
    with pytest.raises(NotImplementedError, match="scheduled sampling"):
        eng.xe_train_step({}, None, None, None, None, None, 3, True, 1, {}, ss_prob=0.25)


@pytest.mark.parametrize("name", ["fc_tiny", "fc_odd"])
def test_scst_restatement_agrees_with_the_oracle_on_a_forced_stream(name):
    cfg, W, I, Out, G, X = load_golden(name)
    fc, L, V = I["fc_feats"], cfg["L"], cfg["V"]
    N = fc.shape[0]
    g = torch.Generator().manual_seed(11)
    reward = torch.randn(N, L + 1, generator=g)
    for forced in (FT.forced_streams(N, L, V, 3), FT.all_ended_streams(N, L, V, 4, end=L // 2), FT.all_ended_streams(N, L, V, 5, end=0)):
        seq_o, lp_o = OF.sample(W, fc, L, sample_max=0, forced_tokens=forced)
        assert torch.equal(FT.masked_stream(forced), seq_o)
        # fed = the raw stream: every entry of seqLogprobs, also those behind a row's end
        lp = FT.sampled_logprobs(W, fc, seq_o, fed=forced)
        assert torch.allclose(lp, lp_o, atol=1e-6), (lp - lp_o).abs().max()
        # fed = the stored tokens: the same loss (the entries behind a row's end are masked) and, through it, the same gradients
        loss, grads, _ = FT.scst_loss_and_grads(W, fc, seq_o, reward)
        loss_raw, grads_raw, _ = FT.scst_loss_and_grads(W, fc, seq_o, reward, fed=forced)
        assert abs(float(loss) - float(O.reward_criterion(lp_o, seq_o, reward))) < 1e-6
        assert abs(float(loss) - float(loss_raw)) < 1e-6
        for k in grads:
            assert torch.allclose(grads[k], grads_raw[k], atol=1e-6), k
