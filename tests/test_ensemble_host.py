"""CPU-side checks of the ensemble surface (no GPU): AttEnsemble keeps the reference's constructor contract
(P/models/AttEnsemble.py:29-37), refuses what it cannot serve with a message, and the three ensemble entry points are both
declared in include/uic_hip.h and exported by libuic_hip.so."""
import argparse
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn as nn

from conftest import ROOT


def _opt(**kw):
    base = dict(vocab_size=50, input_encoding_size=32, rnn_size=32, num_layers=1, drop_prob_lm=0.5, seq_length=6,
                fc_feat_size=64, att_feat_size=64, att_hid_size=32, use_bn=0, caption_model="topdown", compute_dtype="f32")
    base.update(kw)
    return argparse.Namespace(**base)


NEW_SYMBOLS = ("uic_ensemble_logprobs", "uic_topdown_ensemble_sample", "uic_topdown_ensemble_sample_beam")


def test_constructor_attributes():
    from unpaired_image_captioning_amd import models
    from unpaired_image_captioning_amd.models.AttEnsemble import AttEnsemble
    from unpaired_image_captioning_amd.models.AttModel import AttModel
    ms = [models.setup(_opt()), models.setup(_opt(rnn_size=64, att_feat_size=48, use_bn=1))]
    ens = AttEnsemble(ms)
    assert isinstance(ens, AttModel) and isinstance(ens.models, nn.ModuleList) and len(ens.models) == 2
    assert ens.models[0] is ms[0] and ens.models[1] is ms[1]
    assert ens.vocab_size == 50 and ens.seq_length == 6 and ens.ss_prob == 0
    # the members' parameters are the ensemble's (eval_ensemble.py moves it to the device as one module)
    assert len(list(ens.parameters())) == sum(len(list(m.parameters())) for m in ms)
    hid = ens.init_hidden(3)
    assert isinstance(hid, list) and len(hid) == 2
    assert hid[0][0].shape == (2, 3, 32) and hid[1][1].shape == (2, 3, 64)
    assert models.AttEnsemble is AttEnsemble


def test_training_mode_raises():
    from unpaired_image_captioning_amd import models
    ens = models.AttEnsemble([models.setup(_opt()), models.setup(_opt())])
    fc, att = torch.zeros(2, 64), torch.zeros(2, 5, 64)
    assert ens.training                                  # a fresh nn.Module: the caller has not called eval() yet
    for opt in ({"sample_max": 1}, {"beam_size": 3}):
        with pytest.raises(NotImplementedError, match="eval mode"):
            ens(fc, None, att, None, opt=opt, mode="sample")
    with pytest.raises(NotImplementedError, match="eval mode"):
        ens._prepare_feature(fc, att, None)
    with pytest.raises(NotImplementedError, match="eval mode"):
        ens.get_logprobs_state(torch.zeros(2, dtype=torch.long), [fc] * 2, [att] * 2, [att] * 2, [None] * 2, ens.init_hidden(2))
    ens.eval()
    ens.models[1].train()                                # one member left in train mode is refused too
    with pytest.raises(NotImplementedError, match="eval mode"):
        ens(fc, None, att, None, opt={"sample_max": 1}, mode="sample")
    with pytest.raises(NotImplementedError, match="only decodes"):
        ens(fc, None, att, torch.zeros(2, 8, dtype=torch.long), None)


def test_mismatched_members_raise():
    from unpaired_image_captioning_amd import _lib, models
    a = models.setup(_opt())
    with pytest.raises(ValueError, match="vocab"):
        models.AttEnsemble([a, models.setup(_opt(vocab_size=51))])
    with pytest.raises(ValueError, match="caption length"):
        models.AttEnsemble([a, models.setup(_opt(seq_length=7))])
    with pytest.raises(ValueError, match="members"):
        models.AttEnsemble([])
    with pytest.raises(ValueError, match="members"):
        models.AttEnsemble([a] * (_lib.ENSEMBLE_MAX + 1))
    with pytest.raises(TypeError):
        models.AttEnsemble([a, nn.Linear(2, 2)])


def test_eval_mode_without_a_device_raises():
    """No eager fallback: an eval-mode decode of CPU tensors fails loudly instead of computing on the host."""
    from unpaired_image_captioning_amd import models
    ens = models.AttEnsemble([models.setup(_opt()), models.setup(_opt())]).eval()
    with pytest.raises(RuntimeError):
        ens(torch.zeros(2, 64), None, torch.zeros(2, 5, 64), None, opt={"sample_max": 1}, mode="sample")


def test_entry_points_in_header_and_export_list():
    from unpaired_image_captioning_amd import _lib
    from unpaired_image_captioning_amd.build import build
    build(verbose=False)
    header = open(os.path.join(ROOT, "include", "uic_hip.h")).read()
    declared = set(re.findall(r"\b(uic_[a-z0-9_]+)\s*\(", header))
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
    assert int(re.search(r"#define\s+UIC_ENSEMBLE_MAX\s+(\d+)", header).group(1)) == _lib.ENSEMBLE_MAX == 8


def test_argument_errors_have_messages():
    """The sequencers check their arrays before any device work: bad member counts and null arrays are argument errors."""
    from unpaired_image_captioning_amd import _lib
    lib = _lib.load()
    null = C.POINTER(C.c_void_p)()
    assert lib.uic_topdown_ensemble_sample(0, null, null, null, null, 4, 1, 1.0, 0, 0, None, null, None, None, None) < 0
    assert b"members" in lib.uic_last_error_string()
    assert lib.uic_topdown_ensemble_sample_beam(9, null, null, null, null, 4, 3, 0, 0, null, None, None, None) < 0
    assert b"members" in lib.uic_last_error_string()
    assert lib.uic_topdown_ensemble_sample(2, null, null, null, null, 4, 1, 1.0, 0, 0, None, null, None, None, None) < 0
    assert b"null pointer" in lib.uic_last_error_string()
    assert lib.uic_ensemble_logprobs(9, 1, 8, null, None, None, 8, None) < 0
    # members that disagree on the vocabulary: refused with both sizes in the message (pointers are never dereferenced as
    # device memory before the checks are through)
    M = 2
    dims = [_lib.Dims(N=6, R=5, D=64, Dfc=64, H=32, E=32, A=32, V1=51 + m, T=7, dtype=0, drop_p=0.5, logit_layers=1) for m in range(M)]
    ws, bs = [_lib.Weights() for _ in range(M)], [_lib.Batch() for _ in range(M)]
    for b in bs:
        b.fc_feats = b.att_feats = 1 << 40
    arr = lambda xs: (C.c_void_p * M)(*[C.addressof(x) for x in xs])
    fake = (C.c_void_p * M)(1 << 40, (1 << 40) + (1 << 30))
    assert lib.uic_topdown_ensemble_sample(M, arr(dims), arr(ws), fake, arr(bs), 6, 1, 1.0, 0, 0, None, fake,
                                           C.c_void_p(1 << 41), C.c_void_p(1 << 41), None) < 0
    assert b"V1=52" in lib.uic_last_error_string() and b"V1=51" in lib.uic_last_error_string()
