"""CPU-side checks of the AdaAtt captioners (no GPU): the float64 restatement (tests/adaatt_cases.py) against fixtures generated
from the reference's own classes, the condition that makes exact ids a fair demand, the module's state_dict contract, every
refusal, and the operator bounds -- a float32 evaluation stays inside them, each deliberate error lands outside."""
import argparse
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn as nn

import adaatt_cases as AC
from conftest import ROOT

NEW_SYMBOLS = ("uic_adaatt_cell_fwd", "uic_adaatt_attention_fwd", "uic_adaatt_workspace_bytes", "uic_adaatt_prepare_feature",
               "uic_adaatt_forward", "uic_adaatt_logprobs_state", "uic_adaatt_sample", "uic_adaatt_sample_beam", "uic_adaatt_beam_done_lists")
_cache = {}


def fixture64(name):
    if name not in _cache:
        cfg, W, I, O = AC.load_fixture(name)
        ins = (I["fc_feats"].double(), I["att_feats"].double(), I["att_masks"].double() if "att_masks" in I else None)
        _cache[name] = (cfg, AC.to64(W), ins, I["labels"], O)
    return _cache[name]


def _opt(**kw):
    base = dict(vocab_size=50, input_encoding_size=16, rnn_size=16, att_hid_size=16, num_layers=1, drop_prob_lm=0.5, seq_length=7,
                fc_feat_size=24, att_feat_size=32, use_bn=0, logit_layers=1, caption_model="adaatt", compute_dtype="f32")
    base.update(kw)
    return argparse.Namespace(**base)


@pytest.mark.parametrize("name", AC.FIXTURES)
def test_restatement_matches_the_reference_fixture(name):
    cfg, W, (fc, att, am), labels, O = fixture64(name)
    tol = 1e-6
    fcp, attp, patt, m = AC.prepare(W, cfg, fc, att, am)
    assert (fcp - O["fc_embed"]).abs().max() < tol and (attp - O["att_embed"]).abs().max() < tol and (patt - O["p_att"]).abs().max() < tol
    assert (AC.forward(W, cfg, fc, att, am, labels) - O["logprobs"]).abs().max() < tol
    state = AC.init_state(cfg, fc.shape[0], torch.float64)
    for i in range(3):
        lp, state = AC.logprobs_state(W, cfg, labels[:, i], fcp, attp, patt, m, state)
        assert (lp - O["step%d_logprobs" % i]).abs().max() < tol, i
        assert (state[0] - O["step%d_h" % i]).abs().max() < tol and (state[1] - O["step%d_c" % i]).abs().max() < tol, i
        assert tuple(state[0].shape) == (cfg["layers"], fc.shape[0], cfg["H"])
    seq, lp, gap = AC.sample_greedy(W, cfg, fc, att, am)
    assert torch.equal(seq, O["greedy_seq"]) and (lp - O["greedy_logprobs"]).abs().max() < tol
    bseq, blp, done, bgap = AC.beam_search(W, cfg, fc, att, am, cfg["beam"])
    assert torch.equal(bseq, O["beam_seq"]) and (blp - O["beam_logprobs"]).abs().max() < tol
    for k, d in enumerate(done):
        assert len(d) == int(O["done_count"][k])
        for j, (s, l, p) in enumerate(d):
            assert torch.equal(s, O["done_seq"][k, j]) and (l - O["done_logps"][k, j]).abs().max() < tol
            # (the reference keeps beam_logprobs_sum in a FloatTensor whatever the model's dtype: `p` is an f32 running sum of up to
            # L terms, each addition within 2^-24 |p|)
            assert abs(p - float(O["done_p"][k, j])) < tol + cfg["L"] * 2.0 ** -24 * abs(p)
    # the condition that makes exact ids a fair demand of an f32 run: every live decision is clear by ten tolerances
    assert gap >= AC.MIN_GAP and bgap >= AC.MIN_GAP, (gap, bgap)
    # the rescoring helper is the same recurrence
    got, top = AC.rescore(W, cfg, fc, att, am, seq)
    live = AC.live_positions(seq)
    assert (got - lp)[live].abs().max() < 1e-12 and (top - lp)[live].abs().max() < 1e-12


def test_fixtures_cover_the_listed_ground():
    cfgs = {n: fixture64(n) for n in AC.FIXTURES}
    assert cfgs["adaattmo_tiny"][0]["maxout"] == 1 and cfgs["adaatt_tiny"][0]["maxout"] == 0
    c, _, (fc, att, am), labels, _ = cfgs["adaatt_bn1_ragged"]
    lens = am.sum(1)
    assert c["use_bn"] == 1 and lens.min() == 1 and lens.max() == att.shape[1] and len(set(lens.tolist())) > 2 and (labels[1] == 0).all()
    assert cfgs["adaatt_nomask"][2][2] is None and cfgs["adaatt_bn2"][0]["use_bn"] == 2
    c = cfgs["adaattmo_2layer_logit2"][0]
    assert (c["layers"], c["logit_layers"], c["maxout"]) == (2, 2, 1)
    for n in AC.FIXTURES:
        assert os.path.getsize(os.path.join(AC.GOLDEN, n + ".npz")) < 200 * 1024


@pytest.mark.parametrize("name", AC.FIXTURES)
def test_state_dict_keys_shapes_and_weight_struct(name):
    from unpaired_image_captioning_amd import _lib, models
    cfg, W, _, _, _ = fixture64(name)
    model = models.setup(AC.opt_of(cfg))
    assert type(model).__name__ == ("AdaAttMOModel" if cfg["maxout"] else "AdaAttModel") and model.eval_only
    sd = model.state_dict()
    assert list(sd) == list(cfg["shapes"])
    assert {k: tuple(v.shape) for k, v in sd.items()} == cfg["shapes"]
    model.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in W.items()}, strict=True)
    keys = [k for _, _, k in _lib.adaatt_weight_keys(cfg["layers"], cfg["use_bn"], cfg["logit_layers"])]
    assert keys == [k for k in sd if not k.endswith("num_batches_tracked")]
    h, c = model.init_hidden(5)
    assert tuple(h.shape) == tuple(c.shape) == (cfg["layers"], 5, cfg["H"])


def test_same_seed_gives_reference_initialisation_order():
    """The parameter-owning tree is built in the reference's order: two builds from one seed agree, and AdaAttMO differs from
    AdaAtt only by the fifth chunk of the gate matrices."""
    from unpaired_image_captioning_amd import models
    from unpaired_image_captioning_amd.models import AttModel as AM
    assert AM.AdaAttModel is models.AdaAttModel and AM.AdaAttMOModel is models.AdaAttMOModel
    torch.manual_seed(3)
    a = models.setup(_opt()).state_dict()
    torch.manual_seed(3)
    b = models.setup(_opt()).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert tuple(a["core.lstm.w2h.weight"].shape) == (64, 16)
    assert tuple(models.setup(_opt(caption_model="adaattmo")).state_dict()["core.lstm.w2h.weight"].shape) == (80, 16)


def test_refusals_at_construction():
    from unpaired_image_captioning_amd import _lib, models
    for kw in (dict(input_encoding_size=24), dict(rnn_size=24), dict(att_hid_size=8)):
        with pytest.raises(NotImplementedError, match="must all be equal"):
            models.setup(_opt(**kw))
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        models.setup(_opt(input_encoding_size=12, rnn_size=12, att_hid_size=12))
    for n in (0, 3):
        with pytest.raises(NotImplementedError, match="num_layers"):
            models.setup(_opt(num_layers=n))
    for n in (0, _lib.MAX_LOGIT_LAYERS + 1):
        with pytest.raises(NotImplementedError, match="logit_layers"):
            models.setup(_opt(logit_layers=n))
    for n in (-1, 3):
        with pytest.raises(ValueError, match="use_bn"):
            models.setup(_opt(use_bn=n))
    for name in ("adaatt", "adaattmo"):
        assert models.setup(_opt(caption_model=name, num_layers=2, logit_layers=_lib.MAX_LOGIT_LAYERS, use_bn=2)) is not None


def test_training_is_refused_and_eval_builds():
    from unpaired_image_captioning_amd import models
    from unpaired_image_captioning_amd.trainer import Trainer
    for name in ("adaatt", "adaattmo"):
        with pytest.raises(NotImplementedError, match="not supported by the MI355X hot path.*training is not built"):
            models.setup(_opt(caption_model=name, i2t_train_flag=1))
        with pytest.raises(NotImplementedError, match="training is not built"):
            Trainer(_opt(caption_model=name, i2t_train_flag=1))
        with pytest.raises(NotImplementedError, match="evaluation and decoding only; training is not built"):
            Trainer(_opt(caption_model=name))                          # the flag's default is 1, as in opts.py
        tr = Trainer(_opt(caption_model=name, i2t_train_flag=0))
        assert type(tr.i2t_model).__name__ == ("AdaAttModel" if name == "adaatt" else "AdaAttMOModel") and not tr.i2t_model.training
    model = models.setup(_opt()).train()
    fc, att, seq = torch.zeros(2, 24), torch.zeros(2, 5, 32), torch.zeros(2, 9, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="training is not built"):
        model(fc, None, att, seq, None)
    with pytest.raises(NotImplementedError, match="training is not built"):
        model(fc, None, att, None, opt={"sample_max": 1}, mode="sample")
    with pytest.raises(NotImplementedError, match="training is not built"):
        model(fc, None, att, None, opt={"beam_size": 3}, mode="sample")
    with pytest.raises(NotImplementedError, match="training is not built"):
        model._sample_beam(fc, att, None, {"beam_size": 3})


def test_no_cpu_fallback_and_topdown_extensions_refused():
    from unpaired_image_captioning_amd import models
    model = models.setup(_opt()).eval()
    fc, att, seq = torch.zeros(2, 24), torch.zeros(2, 5, 32), torch.zeros(2, 9, dtype=torch.long)
    with pytest.raises(RuntimeError, match="device tensors"):
        model(fc, None, att, seq, None)
    with pytest.raises(RuntimeError, match="device tensors"):
        model(fc, None, att, None, opt={"sample_max": 1}, mode="sample")
    with pytest.raises(RuntimeError, match="device tensors"):
        model._sample_beam(fc, att, None, {"beam_size": 3})
    with pytest.raises(RuntimeError, match="device tensors"):
        model._prepare_feature(fc, att, None)
    with pytest.raises(NotImplementedError, match="captions_per_image"):
        model(fc, None, att, None, opt={"captions_per_image": 5}, mode="sample")
    with pytest.raises(NotImplementedError, match="forced_tokens"):
        model(fc, None, att, None, opt={"forced_tokens": torch.zeros(2, 7, dtype=torch.long)}, mode="sample")
    with pytest.raises(NotImplementedError, match="beam_size"):
        model._sample_beam(fc, att, None, {"beam_size": 17})


def test_ensemble_refuses_members_that_are_not_topdown():
    from unpaired_image_captioning_amd import models
    td = models.setup(_opt(caption_model="topdown", input_encoding_size=32, rnn_size=32, att_hid_size=32, fc_feat_size=64, att_feat_size=64))
    ada = models.setup(_opt())
    with pytest.raises(TypeError, match="member 1 is a AdaAttModel"):
        models.AttEnsemble([td, ada])
    with pytest.raises(TypeError, match="member 0 is a AdaAttMOModel"):
        models.AttEnsemble([models.setup(_opt(caption_model="adaattmo"))])
    with pytest.raises(TypeError, match="member 1 is a Linear"):
        models.AttEnsemble([td, nn.Linear(2, 2)])
    with pytest.raises(TypeError, match="member 1 is a AttEnsemble"):
        models.AttEnsemble([td, models.AttEnsemble([td])])
    assert len(models.AttEnsemble([td, td]).models) == 2


def test_exports_and_argument_checks_without_a_device():
    from unpaired_image_captioning_amd import _lib
    from unpaired_image_captioning_amd.build import SOURCES, build
    build(verbose=False)
    assert "adaatt.hip" in SOURCES
    header = open(os.path.join(ROOT, "include", "uic_hip.h")).read()
    declared = set(re.findall(r"\b(uic_[a-z0-9_]+)\s*\(", header))
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(raw, name), name
    assert int(re.search(r"#define\s+UIC_ADAATT_MAX_LAYERS\s+(\d+)", header).group(1)) == _lib.ADAATT_MAX_LAYERS
    common = open(os.path.join(ROOT, "unpaired_image_captioning_amd", "csrc", "uic_common.h")).read()
    assert int(re.search(r"#define\s+UIC_BEAM_MAX\s+(\d+)", common).group(1)) == _lib.BEAM_MAX
    lib = _lib.load()
    d = _lib.AdaAttDims(N=128, R=36, D=2056, Dfc=2048, H=512, V1=9488, S=18, layers=1, maxout=1, logit_layers=1, use_bn=1, dtype=1, beam=3)
    ws = lib.uic_adaatt_workspace_bytes(C.byref(d))
    assert ws > 0 and ws % 256 == 0
    for field, bad, msg in (("H", 510, b"multiples of 8"), ("layers", 3, b"layers"), ("maxout", 2, b"maxout"), ("logit_layers", 5, b"logit_layers"),
                            ("use_bn", 3, b"use_bn"), ("beam", 17, b"beam"), ("dtype", 7, b"dtype"), ("R", 40000, b"LDS")):
        good = getattr(d, field)
        setattr(d, field, bad)
        assert lib.uic_adaatt_workspace_bytes(C.byref(d)) == 0 and msg in lib.uic_last_error_string(), field
        setattr(d, field, good)
    # the operators' refusals come before any device work (the pointers are never dereferenced)
    P = 1 << 20
    ok_cell = [0, 3, 8, 1, P, 48, P + 160, 48, P, P, P, 8, P, 8, None]
    for pos, bad, msg in ((0, 5, b"dtype"), (2, 6, b"multiple of 4"), (3, 2, b"maxout"), (4, None, b"null"), (5, 36, b"ld_sums"), (11, 4, b"ld_h"),
                          (6, None, b"come together"), (12, None, b"come together"), (7, 6, b"ld_n5"), (4, P + 4, b"aligned")):
        a = list(ok_cell)
        a[pos] = bad
        assert lib.uic_adaatt_cell_fwd(*a) == -1 and msg in lib.uic_last_error_string(), (pos, lib.uic_last_error_string())
    ok_att = [0, 6, 5, 16, 8, 3, P, P, 16, P, P, 8, P, P, P, P, P, 5, P, P, 8, None]
    for pos, bad, msg in ((0, 2, b"dtype"), (2, 0, b"bad sizes"), (3, 18, b"multiples of 4"), (4, 6, b"multiples of 4"), (5, 4, b"row_div"),
                          (5, 0, b"row_div"), (6, None, b"null"), (18, None, b"null"), (8, 12, b"leading dimension"), (17, 4, b"leading dimension"),
                          (20, 4, b"leading dimension"), (12, P + 8, b"16 bytes")):
        a = list(ok_att)
        a[pos] = bad
        assert lib.uic_adaatt_attention_fwd(*a) == -1 and msg in lib.uic_last_error_string(), (pos, lib.uic_last_error_string())
    a = list(ok_att)
    a[2] = a[17] = 50000        # 4 (3 A + R + 1 + 4 H) bytes of LDS
    assert lib.uic_adaatt_attention_fwd(*a) == -1 and b"160 KB" in lib.uic_last_error_string()
    a = list(ok_att)
    a[0], a[3] = 1, 20          # bf16 reads 8 elements at a time
    assert lib.uic_adaatt_attention_fwd(*a) == -1 and b"multiples of 8" in lib.uic_last_error_string()
    for R, A, H in ((36, 512, 512), (1, 8, 8), (64, 520, 40)):
        assert _lib.adaatt_attention_lds_bytes(R, A, H) == AC.att_lds_bytes(R, A, H) <= _lib.LDS_BYTES
    assert AC.att_lds_bytes(36, 512, 512) == 4 * (1536 + 40 + 2048)


# ---------------------------------------------------------------------------------------------------------------- operator bounds
def _inside(got, ref, bound):
    return bool(((got.double() - ref).abs() <= bound).all())       # (a NaN is outside)


def _cell_eval(inp, dtype=torch.float64, variant=None):
    f = lambda t: None if t is None else t.to(dtype)          # noqa: E731
    return AC.cell(f(inp["sums"]), f(inp["n5"]), f(inp["c_prev"]), inp["H"], inp["maxout"], variant)


def _att_eval(inp, dtype=torch.float64, variant=None):
    f = lambda t: None if t is None else t.to(dtype)          # noqa: E731
    return AC.attention(f(inp["fr_e"]), f(inp["hl_e"]), f(inp["fr"]), f(inp["hl"]), f(inp["p_att"]), f(inp["att"]), f(inp["w"]), f(inp["b"]),
                        f(inp["mask"]), inp["row_div"], variant)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_float32_evaluation_stays_inside_the_operator_bounds(dtype):
    for case in AC.CELL_CASES:
        inp = AC.cell_inputs(case, dtype)
        ref, got = _cell_eval(inp), _cell_eval(inp, torch.float32)
        for r, g, b in zip(ref, got, AC.cell_bounds(inp, ref, "f32")):
            assert r is None or _inside(g, r, b), case
        assert float(AC.cell_bounds(inp, ref, dtype)[1].max()) < (1e-5 if dtype == "f32" else 5e-3), case     # the bounds stay tight
    for case in AC.ATT_CASES:
        inp = AC.att_inputs(case, dtype)
        ref, got = _att_eval(inp), _att_eval(inp, torch.float32)
        for r, g, b in zip(ref, got, AC.att_bounds(inp, ref, "f32")):
            assert _inside(g, r, b), case
        assert float(AC.att_bounds(inp, ref, dtype)[1].max()) < 5e-3, case


def test_cases_cover_what_they_claim():
    sat = [c for c in AC.ATT_CASES if c[6]]
    for case in sat:
        inp = AC.att_inputs(case, "f32")
        e0 = (torch.tanh(inp["fr_e"] + inp["hl_e"]) @ inp["w"] + inp["b"])
        assert 89 < float(e0.min()) and 60 < float(inp["w"].abs().sum()) < 140          # exp(e) overflows f32 (e^88.7)
    assert {c[1] for c in AC.ATT_CASES} >= {1, 2, 36, 63, 64} and {c[4] for c in AC.ATT_CASES} == {1, 3}
    assert any(c[2] != c[3] and 520 in (c[2], c[3]) for c in AC.ATT_CASES) and any(8 in (c[2], c[3]) for c in AC.ATT_CASES)
    m0 = [AC.att_inputs(c, "f32")["mask"] for c in AC.ATT_CASES if c[5] == "m0"]
    assert m0 and all(float(m[-1, 0]) == 0 and float(m[-1, 1:].min()) == 1 for m in m0)
    assert {c[0] for c in AC.CELL_CASES} == {1, 3, 33} and {c[1] for c in AC.CELL_CASES} == {8, 40, 512}
    assert {c[4] for c in AC.CELL_CASES} == {"inside", "apart", None} and any(not c[5] for c in AC.CELL_CASES) and any(c[6] == 30.0 for c in AC.CELL_CASES)


@pytest.mark.parametrize("variant,pick", [
    ("no_max", lambda c: c[6]),                         # softmax without subtracting the maximum, on the saturated cases
    ("sentinel_unmasked", lambda c: c[5] == "m0"),      # sentinel masked by 1 instead of m_0
    ("no_renorm", lambda c: c[5] == "ragged"),          # PI not renormalised after the mask
    ("no_hl", lambda c: True),                          # hl not added
])
def test_deliberate_attention_errors_land_outside(variant, pick):
    cases = [c for c in AC.ATT_CASES if pick(c)]
    assert cases
    for dtype in ("f32", "bf16"):
        for case in cases:
            inp = AC.att_inputs(case, dtype)
            ref = _att_eval(inp)
            # (no_max: evaluated in float32, where exp overflows; float64 would hide it)
            got = _att_eval(inp, torch.float32 if variant == "no_max" else torch.float64, variant)
            bo, bp = AC.att_bounds(inp, ref, dtype)
            assert not _inside(got[0], ref[0], bo) or not _inside(got[1], ref[1], bp), (variant, case, dtype)


@pytest.mark.parametrize("variant,pick", [
    ("fake_prev", lambda c: c[4] is not None),          # fake taken from tanh(c_prev)
    ("swap_out", lambda c: c[2] == 1),                  # maxout chunks swapped with the out gate
])
def test_deliberate_cell_errors_land_outside(variant, pick):
    cases = [c for c in AC.CELL_CASES if pick(c)]
    assert cases
    for dtype in ("f32", "bf16"):
        for case in cases:
            inp = AC.cell_inputs(case, dtype)
            ref, got = _cell_eval(inp), _cell_eval(inp, variant=variant)
            bounds = AC.cell_bounds(inp, ref, dtype)
            assert any(r is not None and not _inside(g, r, b) for r, g, b in zip(ref, got, bounds)), (variant, case, dtype)


def test_bf16_bounds_follow_the_recorded_deviations():
    for name in AC.FIXTURES:
        cfg, W, (fc, att, am), labels, _ = fixture64(name)
        b = AC.bf16_bounds(name, W, cfg, fc, att, am, labels)
        assert AC.TOL_BF16 <= b == max(AC.TOL_BF16, b) < 0.2
    assert set(AC.BF16_EMULATED) == set(AC.FIXTURES) | {"real"}
