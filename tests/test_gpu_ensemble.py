"""AttEnsemble on the device (models/AttEnsemble.py, csrc/ensemble.hip, the uic_topdown_ensemble_* sequencers) against the
oracle: the oracle's own single-model step (oracle.topdown.logprobs_step) per member, combined as the reference combines them
(P/models/AttEnsemble.py:53: softmax, mean over the members, log), driving the oracle's unchanged greedy loop / beam_search_core.

Exact token ids are demanded only where the ORACLE's decisions are not near-ties: every exact-id test first asserts, on the
oracle side, that the smallest gap it met between the winner and the runner-up is >= MARGIN = 1e-2 -- ten times the f32
log-prob tolerance.  The member seeds / the fixed logit scale below were chosen on the CPU so that this holds; it is a
condition on the inputs, never a reason to leave a row out."""
import argparse
import functools

import pytest
import torch

from oracle import topdown as O

pytestmark = pytest.mark.gpu

V1, E, H, A, D, R, L, N_IMG = 51, 32, 32, 32, 64, 5, 6, 3
MARGIN = 1e-2
LOGIT_SCALE = 6.0            # contrast of the word distributions (torch's default initialiser gives nearly flat ones)
EOS_BIAS = 1.5               # some captions / beams finish before step L
JUNK = -100.0                # below any real caption's score (or score / length): a continuation of a finished beam


def member(seed, rnn=H, att_size=D, use_bn=0, eos=None):
    W = O.init_weights(V1, E, rnn, A, att_size, D, seed=seed, use_bn=use_bn)
    W["logit.weight"] = W["logit.weight"] * LOGIT_SCALE
    W["logit.bias"][0] += EOS_BIAS if eos is None else eos
    if use_bn:               # running statistics that do something (eval mode reads them)
        g = torch.Generator().manual_seed(seed + 1000)
        W["att_embed.0.running_mean"] = torch.rand(att_size, generator=g) * 0.05
        W["att_embed.0.running_var"] = 0.5 + torch.rand(att_size, generator=g)
    return dict(W=W, H=rnn, D=att_size, use_bn=use_bn)


MEMBERS = {
    "m2": lambda: [member(11), member(26)],
    "m3": lambda: [member(11), member(26), member(17)],
    "mixed": lambda: [member(11), member(71, rnn=64, att_size=48, use_bn=1)],
    "m1": lambda: [member(11)],
    # the same members without the raised EOS bias: greedy captions that run to the full length
    "g2": lambda: [member(11, eos=0.0), member(26, eos=0.0)],
    "g3": lambda: [member(11, eos=0.0), member(26, eos=0.0), member(17, eos=0.0)],
    "gmixed": lambda: [member(11, eos=0.0), member(71, rnn=64, att_size=48, use_bn=1, eos=0.0)],
}


@functools.lru_cache(maxsize=None)
def members(name):
    return MEMBERS[name]()


@functools.lru_cache(maxsize=None)
def batch():
    return O.synthetic_batch(N_IMG, 1, R, D, V1 - 1, L, seed=5, ragged_regions=True)


# ------------------------------------------------------------------ the oracle's ensemble
def o_prepare(ms, fc, att, am):
    return [O.prepare_feature(m["W"], fc, att[..., :m["D"]].contiguous(), am, None, m["use_bn"], False) for m in ms]


def o_step(ms, feats, it, state):
    """AttEnsemble.get_logprobs_state: `state` is ONE tuple of the 2M tensors (h_0, c_0, h_1, c_1, ...)."""
    lps, new = [], []
    for i, m in enumerate(ms):
        fc, att, p_att, am = feats[i]
        lp, st, _ = O.logprobs_step(m["W"], it, fc, att, p_att, am, (state[2 * i], state[2 * i + 1]))
        lps.append(lp)
        new += [st[0], st[1]]
    return torch.stack([lp.exp() for lp in lps], 2).mean(2).log(), tuple(new)


def o_zero_state(ms, n):
    return tuple(torch.zeros(2, n, m["H"]) for m in ms for _ in range(2))


def o_sample(ms, fc, att, am, sample_max=1, decoding_constraint=0, forced=None):
    """The loop of oracle.topdown.sample with the ensemble step -> (seq, logp, smallest top-1 / top-2 gap over the steps of
    rows that were still unfinished, i.e. over every choice that reaches the output)."""
    n = fc.shape[0]
    feats = o_prepare(ms, fc, att, am)
    state = o_zero_state(ms, n)
    seq = torch.zeros(n, L, dtype=torch.long)
    lps = torch.zeros(n, L)
    it = torch.zeros(n, dtype=torch.long)
    unfinished = torch.ones(n, dtype=torch.bool)
    gap = float("inf")
    for t in range(L):
        logp, state = o_step(ms, feats, it, state)
        if decoding_constraint and t > 0:
            tmp = torch.zeros_like(logp)
            tmp.scatter_(1, seq[:, t - 1].unsqueeze(1), float("-inf"))
            logp = logp + tmp
        if sample_max:
            top = logp.topk(2, 1).values
            gap = min(gap, float((top[:, 0] - top[:, 1])[unfinished].min()))
            lp, it = torch.max(logp, 1)
        else:
            it = forced[:, t].clone()
            lp = logp.gather(1, it.unsqueeze(1)).view(-1)
        unfinished = (it > 0) if t == 0 else unfinished & (it > 0)
        it = it * unfinished.long()
        seq[:, t] = it
        lps[:, t] = lp
        if int(unfinished.sum()) == 0:
            break
    return seq, lps, gap


def o_beam(ms, fc, att, am, B, decoding_constraint, max_ppl):
    """oracle.topdown.beam_search_core, unchanged, image by image over the ensemble step -> (seq, logp, done lists, smallest gap).
    The gap is taken where the search decides: between neighbours among the B + 1 best joint scores of every step; for each of
    those candidates, between its word and the nearest other word of its beam row (after the search's own modifications: a
    closer word could have taken its place in the row's ranking); and between neighbours among the B + 1 best finished beams.
    The joint scores are read off the lists beam_search_core hands to sorted(): while it runs, the oracle module sees a `sorted`
    that notes the scores and then sorts as the built-in does.
    Continuations of a beam that has finished are left out (joint score below JUNK: the search set its sum to -1000, where f32
    numbers are 6e-5 apart and ties are the rule).  They are ranked below every live candidate, and what they leave in the done
    list ranks below every properly finished beam: the callers assert that the first B finished beams of every image are proper
    ones, so nothing that is returned depends on them."""
    feats = o_prepare(ms, fc, att, am)
    gaps = []
    cur = [None]                         # the rows the search ranks next, with its modifications applied

    def modified(prev_it, logp):
        lpf = logp.clone()
        if decoding_constraint and prev_it is not None:
            lpf.scatter_(1, prev_it.unsqueeze(1), float("-inf"))
        lpf[:, -1] -= 1000
        return lpf

    def recording_sorted(items, key=None):
        out = sorted(items, key=key)
        top = [x for x in out[:B + 1] if x["p"] > JUNK]
        p = torch.tensor([x["p"] for x in top], dtype=torch.float64)
        p = p[torch.isfinite(p)]
        if p.numel() > 1:
            gaps.append(float((p[:-1] - p[1:]).min()))
        for x in top:
            if "q" in x:                 # a candidate (beam row q, word c), not a finished beam
                row = cur[0][x["q"]].double()
                d = (row - row[x["c"]]).abs()
                d[x["c"]] = float("inf")
                gaps.append(float(d[torch.isfinite(row)].min()))
        return out

    seqs, lps, dones = [], [], []
    for k in range(fc.shape[0]):
        fk = [(f[k:k + 1].expand(B, -1), a[k:k + 1].expand(B, -1, -1).contiguous(), p[k:k + 1].expand(B, -1, -1).contiguous(),
               m[k:k + 1].expand(B, -1).contiguous() if m is not None else None) for f, a, p, m in feats]

        def step_fn(it, state):
            logp, st = o_step(ms, fk, it, state)
            cur[0] = modified(it, logp)
            return logp, st

        logprobs, state = o_step(ms, fk, torch.zeros(B, dtype=torch.long), o_zero_state(ms, B))
        cur[0] = modified(None, logprobs)
        with pytest.MonkeyPatch.context() as mp:      # (scoped: the oracle module is as it was once the search returns)
            mp.setattr(O, "sorted", recording_sorted, raising=False)
            done = O.beam_search_core(step_fn, logprobs, state, L, B, decoding_constraint, max_ppl)
        assert not hasattr(O, "sorted")
        seqs.append(done[0]["seq"])
        lps.append(done[0]["logps"])
        dones.append(done)
    return torch.stack(seqs), torch.stack(lps), dones, min(gaps)


# ------------------------------------------------------------------ the device's ensemble
def build_member(m, dtype):
    from unpaired_image_captioning_amd import models
    opt = argparse.Namespace(vocab_size=V1 - 1, input_encoding_size=E, rnn_size=m["H"], num_layers=1, drop_prob_lm=0.5, seq_length=L,
                             fc_feat_size=D, att_feat_size=m["D"], att_hid_size=A, use_bn=m["use_bn"], logit_layers=1,
                             caption_model="topdown", compute_dtype=dtype, seed=0)
    model = models.setup(opt)
    res = model.load_state_dict(m["W"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return model


def build_ensemble(name, dtype):
    from unpaired_image_captioning_amd import models
    return models.AttEnsemble([build_member(m, dtype) for m in members(name)]).cuda().eval()


def absmax(got, ref):
    return (got.detach().float().cpu().double() - ref.detach().float().cpu().double()).abs().max().item()


def dev_batch():
    b = batch()
    return b["fc_feats"].cuda(), b["att_feats"].cuda(), b["att_masks"].cuda()


# ------------------------------------------------------------------ 1. the op
def torch_formula(xs):
    return torch.stack([torch.softmax(x, 1) for x in xs], 2).mean(2).log()


@pytest.mark.parametrize("v1", [51, 257, 9488])
@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_op_vs_torch_formula(M, v1):
    """uic_ensemble_logprobs against softmax -> mean -> log in f32, 1e-5 absolute: contiguous rows (odd lengths take the 4-byte
    loads, 9488 the 16-byte ones with a partial last trip), rows with a leading dimension > V1 whose padding holds NaN and must
    be neither used nor written, and the output written over member 0's rows as the sequencers do."""
    from unpaired_image_captioning_amd.topdown_engine import ensemble_logprobs
    n = 5
    g = torch.Generator().manual_seed(100 * M + v1)
    xs = [torch.randn(n, v1, generator=g) * (1.0 + m) for m in range(M)]
    ref = torch_formula(xs)
    assert torch.isfinite(ref).all()
    out = ensemble_logprobs(tuple(x.cuda() for x in xs))     # (any sequence of tensors)
    print("M=%d V1=%d contiguous: max |d| %.3e" % (M, v1, absmax(out, ref)))
    assert out.shape == (n, v1) and absmax(out, ref) < 1e-5
    if M == 1:
        assert absmax(out, torch.log_softmax(xs[0], 1)) < 1e-5
    for ld in (v1 + 3, (v1 + 63) // 64 * 64 + 8):           # an odd leading dimension; a 16-byte one with the last group half padding
        bufs = [torch.full((n, ld), float("nan")) for _ in range(M)]
        for b, x in zip(bufs, xs):
            b[:, :v1] = x
        bufs = [b.cuda() for b in bufs]
        obuf = torch.full((n, ld), 7.0, device="cuda")
        got = ensemble_logprobs([b[:, :v1] for b in bufs], out=obuf[:, :v1])
        print("M=%d V1=%d ld=%d: max |d| %.3e" % (M, v1, ld, absmax(got, ref)))
        assert absmax(got, ref) < 1e-5
        assert bool((obuf[:, v1:] == 7.0).all())            # the padding columns of the output stay as they were
        # in place over member 0 (the sequencers combine into member 0's step logits)
        ensemble_logprobs([b[:, :v1] for b in bufs], out=bufs[0][:, :v1])
        assert absmax(bufs[0][:, :v1], ref) < 1e-5 and bool(torch.isnan(bufs[0][:, v1:]).all())
        for b, x in zip(bufs[1:], xs[1:]):                  # the other members' rows are inputs only
            assert torch.equal(b[:, :v1].cpu(), x)


@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_op_one_dominant_logit(M):
    """One member's row has a logit 200 above the rest: its other probabilities underflow in f32 (e^-200).  The result must be
    finite wherever the reference formula's is and agree with it there; with M = 1 it is log_softmax (-200, not -inf)."""
    from unpaired_image_captioning_amd.topdown_engine import ensemble_logprobs
    n, v1 = 4, 257
    g = torch.Generator().manual_seed(M)
    xs = [torch.randn(n, v1, generator=g) for _ in range(M)]
    xs[M // 2][torch.arange(n), torch.tensor([0, 100, 255, 256])] += 200.0
    ref = torch_formula(xs)
    out = ensemble_logprobs([x.cuda() for x in xs]).cpu()
    fin = torch.isfinite(ref)
    assert bool(fin.any()) and bool(torch.isfinite(out[fin]).all())
    print("M=%d dominant logit: max |d| %.3e over %d finite reference entries of %d" % (M, absmax(out[fin], ref[fin]), int(fin.sum()), fin.numel()))
    assert absmax(out[fin], ref[fin]) < 1e-5
    if M == 1:
        assert int(fin.sum()) == n                           # the formula keeps only the dominant word ...
        ls = torch.log_softmax(xs[0], 1)
        # ... log_softmax keeps all: values near -200, where f32 numbers are 1.5e-5 apart -- lse rounded once on either side and
        # one subtraction each, so up to four spacings between two correct evaluations
        assert bool(torch.isfinite(out).all()) and absmax(out, ls) < 6.2e-5
    else:
        assert bool(fin.all())


def test_op_argument_errors():
    from unpaired_image_captioning_amd.topdown_engine import ensemble_logprobs
    x = torch.zeros(2, 8, device="cuda")
    with pytest.raises(ValueError, match="members"):
        ensemble_logprobs([x] * 9)
    with pytest.raises(ValueError, match="float32"):
        ensemble_logprobs([x, torch.zeros(2, 9, device="cuda")])
    with pytest.raises(ValueError, match="float32"):
        ensemble_logprobs([x.double()])


# ------------------------------------------------------------------ 2. get_logprobs_state
@pytest.mark.parametrize("dtype,tol", [("f32", 1e-3), ("bf16", 1e-2)])
def test_get_logprobs_state_two_steps_vs_oracle(dtype, tol):
    ms = members("mixed")
    ens = build_ensemble("mixed", dtype)
    b = batch()
    fc, att, am = dev_batch()
    p_fc, p_att, pp_att, p_am = ens._prepare_feature(fc, att, am)
    assert all(isinstance(x, list) and len(x) == 2 for x in (p_fc, p_att, pp_att, p_am)) and p_am[0] is p_am[1]
    assert p_att[0].shape == (N_IMG, R, 32) and p_att[1].shape == (N_IMG, R, 64)
    feats = o_prepare(ms, b["fc_feats"], b["att_feats"], b["att_masks"])
    for i in range(2):
        assert absmax(p_fc[i], feats[i][0]) < tol and absmax(p_att[i], feats[i][1]) < tol and absmax(pp_att[i], feats[i][2]) < tol
    state = ens.init_hidden(N_IMG)
    o_state = o_zero_state(ms, N_IMG)
    it = torch.zeros(N_IMG, dtype=torch.long)
    for t in range(2):
        lp, state = ens.get_logprobs_state(it.cuda(), p_fc, p_att, pp_att, p_am, state)
        lp_o, o_state = o_step(ms, feats, it, o_state)
        print("%s step %d: max |d logprobs| %.3e" % (dtype, t, absmax(lp, lp_o)))
        assert lp.shape == (N_IMG, V1) and absmax(lp, lp_o) < tol, t
        assert isinstance(state, list) and len(state) == 2
        for i in range(2):
            # (the states are not the issue's log-prob bound: h comes back through the operand dtype -- bf16 keeps 8 bits, up to
            # 2e-3 of |h| < 1 on top of the step's own error -- so they get twice the log-prob tolerance)
            assert absmax(state[i][0], o_state[2 * i]) < 2 * tol and absmax(state[i][1], o_state[2 * i + 1]) < 2 * tol
        it = lp_o.argmax(1)


# ------------------------------------------------------------------ 3. greedy, f32
@pytest.mark.parametrize("name", ["g2", "g3", "m2", "m3"])
@pytest.mark.parametrize("dc", [0, 1])
def test_greedy_f32_exact_ids(name, dc):
    b = batch()
    seq_o, lp_o, gap = o_sample(members(name), b["fc_feats"], b["att_feats"], b["att_masks"], decoding_constraint=dc)
    assert gap >= MARGIN, "the oracle's own greedy decisions come within %.3e: choose other member seeds" % gap
    ens = build_ensemble(name, "f32")
    fc, att, am = dev_batch()
    seq, lp = ens(fc, None, att, am, opt={"sample_max": 1, "decoding_constraint": dc}, mode="sample")
    print("%s dc=%d: oracle gap %.3e, max |d logp| %.3e" % (name, dc, gap, absmax(lp, lp_o)))
    assert seq.dtype == torch.int64 and torch.equal(seq.cpu(), seq_o), (seq.cpu(), seq_o)
    assert absmax(lp, lp_o) < 1e-3


# ------------------------------------------------------------------ 4. bf16: the device's tokens scored by the oracle
@pytest.mark.parametrize("name", ["g2", "gmixed"])
def test_greedy_and_forced_multinomial_bf16_scored_by_oracle(name):
    ms = members(name)
    b = batch()
    ens = build_ensemble(name, "bf16")
    fc, att, am = dev_batch()
    seq, lp = ens(fc, None, att, am, opt={"sample_max": 1}, mode="sample")
    seq_o, lp_o, _ = o_sample(ms, b["fc_feats"], b["att_feats"], b["att_masks"], sample_max=0, forced=seq.cpu())
    print("%s bf16 greedy: max |d logp| %.3e" % (name, absmax(lp, lp_o)))
    assert torch.equal(seq_o, seq.cpu()) and absmax(lp, lp_o) < 1e-2
    forced = torch.randint(0, V1, (N_IMG, L), generator=torch.Generator().manual_seed(3))
    seq2, lp2 = ens(fc, None, att, am, opt={"sample_max": 0, "forced_tokens": forced.cuda()}, mode="sample")
    seq_o2, lp_o2, _ = o_sample(ms, b["fc_feats"], b["att_feats"], b["att_masks"], sample_max=0, forced=forced)
    print("%s bf16 forced: max |d logp| %.3e" % (name, absmax(lp2, lp_o2)))
    assert torch.equal(seq_o2, seq2.cpu()) and absmax(lp2, lp_o2) < 1e-2
    # a multinomial draw of the device itself: its tokens replayed through the oracle, same finished-row bookkeeping
    seq3, lp3 = ens(fc, None, att, am, opt={"sample_max": 0, "temperature": 0.8}, mode="sample")
    seq_o3, lp_o3, _ = o_sample(ms, b["fc_feats"], b["att_feats"], b["att_masks"], sample_max=0, forced=seq3.cpu())
    assert torch.equal(seq_o3, seq3.cpu()) and absmax(lp3, lp_o3) < 1e-2


# ------------------------------------------------------------------ 5. / 6. beam search, f32
def _beam_case(name, dc, mp):
    b = batch()
    seq_o, lp_o, done_o, gap = o_beam(members(name), b["fc_feats"], b["att_feats"], b["att_masks"], 3, dc, mp)
    assert gap >= MARGIN, "the oracle's own beam decisions come within %.3e: choose other member seeds" % gap
    ens = build_ensemble(name, "f32")
    fc, att, am = dev_batch()
    seq, lp = ens(fc, None, att, am, opt={"beam_size": 3, "decoding_constraint": dc, "max_ppl": mp}, mode="sample")
    print("%s beam dc=%d max_ppl=%d: oracle gap %.3e, max |d logp| %.3e" % (name, dc, mp, gap, absmax(lp, lp_o)))
    assert torch.equal(seq.cpu(), seq_o), (seq.cpu(), seq_o)
    assert absmax(lp, lp_o) < 1e-3
    assert all(d["p"] > JUNK for done in done_o for d in done)                # (see o_beam)
    beams = ens.done_beams
    assert len(beams) == N_IMG
    for k in range(N_IMG):
        assert len(beams[k]) == len(done_o[k]), k
        for got, ref in zip(beams[k], done_o[k]):
            assert torch.equal(got["seq"].cpu(), ref["seq"]), k
            assert absmax(got["logps"], ref["logps"]) < 1e-3 and abs(got["p"] - ref["p"]) < 1e-3 * L, k
    assert any((d["seq"] == 0).any() for done in done_o for d in done)      # (the fixture has beams that finish early)


@pytest.mark.parametrize("dc,mp", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_beam3_f32_exact_ids_and_done_beams(dc, mp):
    _beam_case("m2", dc, mp)


def test_members_of_different_shape():
    """One member with rnn_size 64, att_feat_size 48 (it reads the first 48 feature columns) and a BatchNorm in front of
    att_embed: greedy and beam search against the oracle."""
    b = batch()
    for name in ("gmixed", "mixed"):
        seq_o, lp_o, gap = o_sample(members(name), b["fc_feats"], b["att_feats"], b["att_masks"])
        assert gap >= MARGIN, gap
        ens = build_ensemble(name, "f32")
        fc, att, am = dev_batch()
        seq, lp = ens(fc, None, att, am, opt={"sample_max": 1}, mode="sample")
        print("%s greedy: oracle gap %.3e, max |d logp| %.3e" % (name, gap, absmax(lp, lp_o)))
        assert torch.equal(seq.cpu(), seq_o) and absmax(lp, lp_o) < 1e-3
    _beam_case("mixed", 0, 0)


# ------------------------------------------------------------------ 7. M = 1
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_single_member_equals_the_model_itself(dtype):
    from unpaired_image_captioning_amd import _lib
    m = build_member(members("m1")[0], dtype).cuda().eval()
    m.engine.recurrence = _lib.REC_FWD_CHAIN
    from unpaired_image_captioning_amd import models
    ens = models.AttEnsemble([m]).eval()
    fc, att, am = dev_batch()
    for opt in ({"sample_max": 1}, {"sample_max": 1, "decoding_constraint": 1}, {"sample_max": 1, "captions_per_image": 2},
                {"beam_size": 3}, {"beam_size": 2, "max_ppl": 1}):
        seq_m, lp_m = m(fc, None, att, am, opt=opt, mode="sample")
        seq_e, lp_e = ens(fc, None, att, am, opt=opt, mode="sample")
        assert torch.equal(seq_e, seq_m), opt
        assert absmax(lp_e, lp_m) < 1e-5, opt


def test_group_size_is_handled_as_in_attmodel():
    """group_size > 1: a plain search over beam_size // group_size beams, as AttModel._sample_beam does."""
    ens = build_ensemble("m2", "f32")
    fc, att, am = dev_batch()
    seq_g, lp_g = ens(fc, None, att, am, opt={"beam_size": 6, "group_size": 2}, mode="sample")
    seq_p, lp_p = ens(fc, None, att, am, opt={"beam_size": 3}, mode="sample")
    assert torch.equal(seq_g, seq_p) and torch.equal(lp_g, lp_p)


def test_sequencer_argument_errors():
    """Members that disagree on what must be shared are refused with a message; so is a member in train mode."""
    from unpaired_image_captioning_amd import models
    from unpaired_image_captioning_amd import topdown_engine as TE
    ens = build_ensemble("m2", "f32")
    fc, att, am = dev_batch()
    engines, params = ens._members()
    with pytest.raises(RuntimeError, match="share rows, vocabulary, regions"):
        TE.ensemble_sample(engines, params, fc, [att, att[:, :4].contiguous()], None, L)
    ens.train()
    with pytest.raises(NotImplementedError, match="eval mode"):
        ens(fc, None, att, am, opt={"beam_size": 3}, mode="sample")
    assert isinstance(ens, models.AttEnsemble)
