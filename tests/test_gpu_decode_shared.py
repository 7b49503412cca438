"""The decode scaffolding the captioners share (csrc/decode_internal.h, models/CaptionModel.py) at the edges where "rows", "images" and
"step capacity" differ:

  * a beam search SHORTER than the workspace's step capacity (seq_length 5, 3 steps) and one of a single step (the loop never
    advances the model), beam 3 on 2 images, for TopDown, FC, AdaAtt and the Transformer, each through its own library call with its
    own workspace: the best beam against a host beam search (oracle.topdown.beam_search_core) over the same model's
    get_logprobs_state -- for FC, which has no such method, over the oracle's restatement of it; for the Transformer, which has no
    state surface, the returned beam is re-scored by its teacher-forced forward pass -- and the exported done lists: at most
    Lsteps * beam_size entries per image;
  * the same exports hold zeros behind an image's last entry, whatever the workspace held before;
  * `done_beams` of every model class through CaptionModel's one property: the reference's list (stable sort by -p, the first
    beam_size) built here straight from the raw arrays, and assignment clearing the raw arrays.

Every search that exports done lists finds its workspace filled with 0xFF bytes first, as conftest.py and test_gpu_adaatt.py
arrange it for the engines' workspaces: no result may depend on what an earlier call left there.

Log-probabilities are held to the 1e-3 of the neighbouring beam tests (test_gpu_boundary.py, test_gpu_fc.py, TOL_F32 of the AdaAtt and
Transformer cases); token ids and counts are exact."""
import ctypes as C

import pytest
import torch

import adaatt_cases as AC
import transformer_cases as TC
from conftest import load_golden
from oracle import fc as OF
from oracle import topdown as O
from test_gpu_topdown import absmax, build_model

pytestmark = pytest.mark.gpu

TOL = 1e-3
CAP_L, B, N_IMG = 5, 3, 2          # the models' seq_length (their workspaces hold CAP_L + 1 or + 2 steps), beams, images


def _lib():
    from unpaired_image_captioning_amd import _lib
    return _lib


def _topdown():
    cfg, W, I, Out, G, X = load_golden("topdown_tiny_ragged")
    model = build_model(dict(cfg, L=CAP_L), W, "f32").eval()
    idx = torch.arange(N_IMG) * cfg["S"]
    return model, (I["fc_feats"][idx].cuda(), I["att_feats"][idx].cuda(), I["att_masks"][idx].cuda())


def _adaatt():
    from unpaired_image_captioning_amd import models
    cfg, W, I, Out = AC.load_fixture("adaatt_bn1_ragged")
    model = models.setup(AC.opt_of(dict(cfg, L=CAP_L), "f32"))
    model.load_state_dict(W, strict=True)
    return model.cuda().eval(), (I["fc_feats"][:N_IMG].cuda(), I["att_feats"][:N_IMG].cuda(), I["att_masks"][:N_IMG].cuda())


def _transformer():
    from test_gpu_transformer import _opt
    from unpaired_image_captioning_amd import models
    cfg, W, I, Out = TC.load_fixture("transformer_tiny")
    model = models.setup(_opt(cfg, "f32", seq_length=CAP_L))
    model.load_state_dict(W, strict=True)
    att = I["att_feats"][:N_IMG].cuda()
    return model.cuda().eval(), (torch.zeros(N_IMG, 8, device="cuda"), att, I["att_masks"][:N_IMG].cuda() if "att_masks" in I else None)


def _fc():
    from test_gpu_fc import build
    cfg, W, I, Out, G, X = load_golden("fc_tiny")
    idx = torch.arange(N_IMG) * cfg["S"]
    return build(dict(cfg, L=CAP_L), W, "f32").eval(), (I["fc_feats"][idx].cuda(),)


# ---------------------------------------------------------------- each captioner's own library call, Lsteps below its capacity
def _search_topdown(model, feats, L):
    U = _lib()
    fc, att, am = (x.contiguous().float() for x in feats)
    eng = model.engine
    pd = {k: v.detach() for k, v in model.param_dict().items()}
    d = eng.dims(N_IMG * B, att.shape[1], CAP_L + 1, B)
    w, ws, b = eng.refresh(pd, d), eng.checkout(d, fc.device), eng.batch_struct(fc, att, am)
    seq = torch.zeros(N_IMG, L, dtype=torch.int64, device="cuda")
    lp = torch.zeros(N_IMG, L, device="cuda")
    lists = U.done_list_buffers(N_IMG, L, B, "cuda")
    try:
        U.check(eng.lib.uic_topdown_sample_beam(C.byref(d), C.byref(w), U.ptr(eng._derived), C.byref(b), L, B, 0, 0, U.ptr(ws.buf), U.ptr(seq),
                                                U.ptr(lp), U.stream()), "sample_beam")
        U.check(eng.lib.uic_topdown_beam_done_lists(C.byref(d), U.ptr(ws.buf), L, B, *[U.ptr(x) for x in lists], U.stream()), "beam_done_lists")
    finally:
        eng.release(ws)
    return seq, lp, lists


def _search_adaatt(model, feats, L):
    U = _lib()
    with torch.no_grad():
        lib, d, w, ws, fc, att, am = model._prepare(*feats, beam=B)
    assert d.S == CAP_L + 2
    ws.fill_(255)
    seq = torch.zeros(N_IMG, L, dtype=torch.int64, device="cuda")
    lp = torch.zeros(N_IMG, L, device="cuda")
    lists = U.done_list_buffers(N_IMG, L, B, "cuda")
    U.check(lib.uic_adaatt_sample_beam(C.byref(d), C.byref(w), U.ptr(fc), U.ptr(att), U.ptr(am), L, B, 0, 0, U.ptr(ws), U.ptr(seq), U.ptr(lp),
                                       U.stream()), "adaatt_sample_beam")
    U.check(lib.uic_adaatt_beam_done_lists(C.byref(d), U.ptr(ws), L, B, *[U.ptr(x) for x in lists], U.stream()), "adaatt_beam_done_lists")
    return seq, lp, lists


def _search_transformer(model, feats, L):
    U = _lib()
    with torch.no_grad():
        lib, d, w, dv, ws, att, am = model._prepare(feats[1], feats[2], beam=B)
    assert d.T == CAP_L + 1
    ws.fill_(255)
    seq = torch.zeros(N_IMG, L, dtype=torch.int64, device="cuda")
    lp = torch.zeros(N_IMG, L, device="cuda")
    lists = U.done_list_buffers(N_IMG, L, B, "cuda")
    U.check(lib.uic_transformer_sample_beam(C.byref(d), C.byref(w), U.ptr(dv), U.ptr(att), U.ptr(am), L, B, 0, 0, U.ptr(ws), U.ptr(seq), U.ptr(lp),
                                            U.stream()), "transformer_sample_beam")
    U.check(lib.uic_transformer_beam_done_lists(C.byref(d), U.ptr(ws), L, B, *[U.ptr(x) for x in lists], U.stream()), "transformer_beam_done_lists")
    return seq, lp, lists


def _search_fc(model, feats, L):
    U = _lib()
    eng = model.engine
    fcb = feats[0].contiguous().float().repeat_interleave(B, 0).contiguous()
    d = eng.dims(N_IMG * B, CAP_L + 2)
    ws = eng.workspace(d, fcb.device)
    seq = torch.zeros(N_IMG, L, dtype=torch.int64, device="cuda")
    lp = torch.zeros(N_IMG, L, device="cuda")
    w = eng.weights({k: v.detach() for k, v in model.param_dict().items()})
    b = eng.batch(fcb)
    U.check(eng.lib.uic_fc_sample_beam(C.byref(d), C.byref(w), C.byref(b), L, B, 0, 0, U.ptr(ws), U.ptr(seq), U.ptr(lp), U.stream()), "fc_sample_beam")
    eng.release(d, ws)
    return seq, lp, None          # (the FC captioner exports no done lists)


# ---------------------------------------------------------------- the host side of the comparison
def _host_search_by_state(model, feats, L):
    """AttModel._sample_beam's per-image loop (:181-194) over the model's own _prepare_feature / get_logprobs_state."""
    p_fc, p_att, pp_att, p_am = model._prepare_feature(*feats)
    seqs, lps = [], []
    for k in range(N_IMG):
        t = [x[k:k + 1].expand(B, *x.shape[1:]).contiguous() if x is not None else None for x in (p_fc, p_att, pp_att, p_am)]

        def step_fn(it, st):
            logp, st2 = model.get_logprobs_state(it.cuda(), t[0], t[1], t[2], t[3], tuple(s_.cuda() for s_ in st))
            return logp.cpu(), tuple(s_.cpu() for s_ in st2)
        logprobs, state = step_fn(torch.zeros(B, dtype=torch.long), tuple(s_.cpu() for s_ in model.init_hidden(B)))
        done = O.beam_search_core(step_fn, logprobs, state, L, B, 0, 0)
        seqs.append(done[0]["seq"])
        lps.append(done[0]["logps"])
    return torch.stack(seqs), torch.stack(lps)


def _check_topdown_like(model, feats, L, seq, lp):
    ref_seq, ref_lp = _host_search_by_state(model, feats, L)
    assert torch.equal(seq.cpu(), ref_seq)
    assert absmax(lp, ref_lp) < TOL


def _check_fc(model, feats, L, seq, lp):
    W = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ref_seq, ref_lp = OF.sample_beam(W, feats[0].cpu(), L, B, 0, 0)
    assert torch.equal(seq.cpu(), ref_seq)
    assert absmax(lp, ref_lp) < TOL


def _check_transformer(model, feats, L, seq, lp):
    """The beam's tokens fed back teacher-forced: every recorded log-prob up to the beam's end is the forward pass's for that token
    (the beam records -1000 less for the last vocabulary index, CaptionModel.py:133)."""
    fc, att, am = feats
    V1 = model.vocab_size + 1
    with torch.no_grad():
        logp = model(fc, None, att, torch.cat([torch.zeros(N_IMG, 1, dtype=torch.int64, device="cuda"), seq], 1), am)
    for k in range(N_IMG):
        toks = seq[k].tolist()
        end = toks.index(0) + 1 if 0 in toks else L        # (the forward pass stops where every row has ended: compare what was searched)
        for t in range(end):
            want = float(logp[k, t, toks[t]]) - (1000.0 if toks[t] == V1 - 1 else 0.0)
            assert abs(float(lp[k, t]) - want) < TOL, (k, t)
        assert not lp[k, end:].any() and not seq[k, end:].any()


def _check_lists(L, seq, lp, lists):
    cnt, dp, dseq, dlp = (x.cpu() for x in lists)
    assert dp.shape == (N_IMG, L * B) and dseq.shape == dlp.shape == (N_IMG, L * B, L)
    for k in range(N_IMG):
        c = int(cnt[k])
        assert 1 <= c <= L * B
        best = sorted(range(c), key=lambda i: -float(dp[k, i]))[0]
        assert torch.equal(dseq[k, best], seq[k].cpu()) and torch.equal(dlp[k, best], lp[k].cpu())
        assert (dp[k, :c] - dlp[k, :c].sum(-1)).abs().max().item() < TOL                   # max_ppl = 0: p is the sum of the log-probs
        if L == 1:
            assert c == B                                   # every beam ends at the last step, which is the first
    return cnt, dp, dseq, dlp


CAPTIONERS = {
    "topdown": (_topdown, _search_topdown, _check_topdown_like),
    "fc": (_fc, _search_fc, _check_fc),
    "transformer": (_transformer, _search_transformer, _check_transformer),
    "adaatt": (_adaatt, _search_adaatt, _check_topdown_like),
}


@pytest.mark.parametrize("L", [3, 1])
@pytest.mark.parametrize("name", sorted(CAPTIONERS))
def test_beam_search_shorter_than_the_step_capacity(name, L):
    make, search, check = CAPTIONERS[name]
    model, feats = make()
    assert model.seq_length == CAP_L
    seq, lp, lists = search(model, feats, L)
    assert seq.shape == lp.shape == (N_IMG, L)
    check(model, feats, L, seq, lp)
    if lists is not None:
        cnt, dp, dseq, dlp = _check_lists(L, seq, lp, lists)
        seq2, lp2, lists2 = search(model, feats, L)             # the same workspace again: nothing of the first search is left in it
        assert torch.equal(seq2, seq) and torch.equal(lp2, lp) and torch.equal(lists2[0].cpu(), cnt)
        for k in range(N_IMG):
            c = int(cnt[k])
            assert all(torch.equal(b[k, :c].cpu(), a[k, :c]) for a, b in zip((dp, dseq, dlp), lists2[1:]))


@pytest.mark.parametrize("L", [3, 1])
@pytest.mark.parametrize("name", ["adaatt", "topdown", "transformer"])
def test_done_list_entries_behind_the_count_are_untouched_zeros(name, L):
    """Behind done_count[k] the exported arrays hold zeros, whatever the workspace held before the search (here the 0xFF poison):
    the export copies the whole [n_img, L*B(, L)] range and the beam kernels write an image's first done_count[k] entries only, so
    the start of a search clears the lists."""
    make, search, check = CAPTIONERS[name]
    model, feats = make()
    seq, lp, lists = search(model, feats, L)
    cnt, dp, dseq, dlp = (x.cpu() for x in lists)
    for k in range(N_IMG):
        c = int(cnt[k])
        print("%s L=%d image %d: %d of %d entries; behind them %d of done_p, %d of done_seq, %d of done_lp are not zero"
              % (name, L, k, c, L * B, int((dp[k, c:] != 0).sum()), int((dseq[k, c:] != 0).sum()), int((dlp[k, c:] != 0).sum())))
    for k in range(N_IMG):
        c = int(cnt[k])
        assert not (dp[k, c:] != 0).any() and not (dseq[k, c:] != 0).any() and not (dlp[k, c:] != 0).any()      # (NaN != 0)


# ---------------------------------------------------------------- done_beams through CaptionModel's property
def _ensemble():
    from unpaired_image_captioning_amd import models
    from test_gpu_topdown import make_opt
    cfg, W, I, Out, G, X = load_golden("topdown_tiny_ragged")
    a = build_model(dict(cfg, L=CAP_L), W, "f32")
    torch.manual_seed(5)
    b = models.setup(make_opt(dict(cfg, L=CAP_L), "f32"))       # a second member with weights of its own
    idx = torch.arange(N_IMG) * cfg["S"]
    return models.AttEnsemble([a, b]).cuda().eval(), (I["fc_feats"][idx].cuda(), I["att_feats"][idx].cuda(), I["att_masks"][idx].cuda())


@pytest.mark.parametrize("name", ["topdown", "adaatt", "transformer", "ensemble"])
def test_done_beams_is_the_reference_list_of_the_raw_arrays(name):
    model, feats = (_ensemble if name == "ensemble" else CAPTIONERS[name][0])()
    fc, att, am = feats
    seq, lp = model(fc, None, att, am, opt={"sample_max": 1, "beam_size": B}, mode="sample")
    assert model._done_raw is not None and model._done_raw[4] == B
    cnt, dp, dseq, dlp = (x.cpu() for x in model._done_raw[:4])
    assert cnt.shape == (N_IMG,) and dp.shape == (N_IMG, CAP_L * B) and dseq.shape == dlp.shape == (N_IMG, CAP_L * B, CAP_L)
    done = model.done_beams
    assert model.done_beams is done                             # built once
    assert len(done) == N_IMG
    for k in range(N_IMG):
        c = int(cnt[k])
        assert 1 <= c <= CAP_L * B
        ps = [float(dp[k, i]) for i in range(c)]
        order = [i for _, i in sorted(zip([-p for p in ps], range(c)))][:B]      # by -p, ties by position: a stable sort, its first B
        assert len(done[k]) == len(order)
        for got, i in zip(done[k], order):
            assert torch.equal(got["seq"].cpu(), dseq[k, i]) and torch.equal(got["logps"].cpu(), dlp[k, i])
            assert got["p"] == ps[i] and abs(got["unaug_p"] - float(dlp[k, i].sum())) < TOL      # (summed on the device there, on the host here)
        assert torch.equal(done[k][0]["seq"], seq[k]) and torch.equal(done[k][0]["logps"], lp[k])
    model.done_beams = []
    assert model._done_raw is None and model.done_beams == []


def test_fc_done_beams_goes_through_the_same_setter():
    model, (fc,) = _fc()
    assert model.done_beams is None and model._done_raw is None
    seq, lp = model._sample_beam(fc, None, None, {"beam_size": B})
    assert model._done_raw is None and len(model.done_beams) == N_IMG
    for k in range(N_IMG):
        assert torch.equal(model.done_beams[k][0]["seq"], seq[k]) and torch.equal(model.done_beams[k][0]["logps"], lp[k])
