"""Small captioners on either side of the vocabulary-size thresholds that no other module reaches (V1 = V + 1 words):
  * vpad() pads the logit row to 8 below 1024 words and to 64 from 1024 on; embed_scan_kernel walks its keys in trips of 4096
    (2 * V1 keys in the early-gradient order); the register criterion ends at 10240 columns, the wide one at 53248
    -> one training step against the oracle at V1 = 1023 ... 53249, f32 and bf16, fused and through the three API calls;
  * sample_step_kernel stages the row in LDS up to 15360 columns; beam search changes its top-k kernel at 16384
    -> greedy, multinomial (with and without decoding_constraint) and beam-3 decoding at V1 = 15360 ... 16384;
  * the persistent decode launch holds at most 10240 vocabulary columns -> at 17, 10225 and 10240 it must run and agree with the
    launch chain and the oracle, at 10241 the chain must run.
A model with random weights spreads its probability flat over the vocabulary, where a misplaced column moves nothing measurable.
So `logit.bias` gets +8 at V1-1, V1-2 and at the multiples of 1024 and 4096 next to V1 on either side, and half of the label
words are drawn from those columns: the boundary columns carry the loss, the gradient and the decoded captions.
Tolerances are those of tests/test_gpu_topdown.py and tests/test_gpu_fullsize_decode.py."""
import functools
import math

import pytest
import torch

from conftest import poison_workspaces
from oracle import topdown as O
from test_gpu_fullsize_decode import alive_mask
from test_gpu_topdown import GRAD_TOL, LOGP_TOL, absmax, build_model, grads_close

pytestmark = pytest.mark.gpu

SMALL = dict(E=32, H=32, A=32, D=64, R=5, n_img=4, S=2, L=5)


def boundary_words(V1):
    """V1-1, V1-2 and the multiples of 1024 and 4096 next to V1 on either side, as far as they are words (0 is the end token)."""
    c = {V1 - 1, V1 - 2}
    for q in (1024, 4096):
        c |= {(V1 - 1) // q * q, -(-V1 // q) * q}
    return sorted(w for w in c if 0 < w < V1)


def weights_and_batch(V1, cfg, seed, end_bias=0.0, logit_scale=1.0):
    """logit_scale > 1 (the decoders): the hidden state moves the logits by about as much as the +8, so the captions differ from
    image to image and step to step while the boundary words stay among the candidates."""
    W = O.init_weights(V1, cfg["E"], cfg["H"], cfg["A"], cfg["D"], cfg["D"], seed=seed)
    W["logit.weight"] *= logit_scale
    words = boundary_words(V1)
    W["logit.bias"][words] += 8.0
    W["logit.bias"][0] += end_bias
    b = O.synthetic_batch(cfg["n_img"], cfg["S"], cfg["R"], cfg["D"], V1 - 1, cfg["L"], seed=seed + 1, ragged_regions=True)
    g = torch.Generator().manual_seed(seed + 2)
    lab = b["labels"]
    pick = torch.tensor(words)[torch.randint(0, len(words), lab.shape, generator=g)]
    swap = (torch.rand(lab.shape, generator=g) < 0.5) & (lab > 0)
    b["labels"] = torch.where(swap, pick, lab)
    return W, b, words


@functools.lru_cache(maxsize=2)
def training_case(V1):
    """Weights, batch and the oracle's step for one vocabulary size: computed once, shared by the dtypes and call paths."""
    cfg = dict(SMALL, V=V1 - 1)
    W, b, words = weights_and_batch(V1, cfg, seed=V1 % 1000)
    loss_o, grads_o, logp_o = O.xe_loss_and_grads(W, b["fc_feats"], b["att_feats"], b["labels"], b["masks"], b["att_masks"])
    return cfg, W, b, words, loss_o, grads_o, logp_o


def check_training_step(V1, dtype, loss, grads):
    cfg, W, b, words, loss_o, grads_o, logp_o = training_case(V1)
    tol = LOGP_TOL[dtype]
    assert abs(loss.item() - loss_o.item()) < tol, (loss.item(), loss_o.item())
    grads_close(grads, grads_o, GRAD_TOL[dtype])
    # logit.bias's gradient is the column sum of d logits, so it localises an error in d logits to a column.  Per column, from the
    # oracle alone: every log-prob within `tol` moves its probability by at most expm1(tol) * p, weighted by the position's
    # mask / sum(mask) and summed over the positions; bf16 d logits carry one rounding (2^-8 |g|) each; 1e-6 for f32 summation.
    Tn = logp_o.shape[1]
    w = (b["masks"][:, 1:1 + Tn] / b["masks"][:, 1:1 + Tn].sum()).double()
    p = logp_o.double().exp()
    onehot = torch.zeros_like(p).scatter_(2, b["labels"][:, 1:1 + Tn].unsqueeze(2), 1.0)
    bound = math.expm1(tol) * (p * w[:, :, None]).sum((0, 1)) + 1e-6
    if dtype == "bf16":
        bound = bound + 2.0 ** -8 * ((p - onehot) * w[:, :, None]).abs().sum((0, 1))
    ref = grads_o["logit.bias"].double()
    err = (grads["logit.bias"].detach().float().cpu().double() - ref).abs()
    worst = int((err / bound).argmax())
    assert (err <= bound).all(), (worst, float(err[worst]), float(bound[worst]), float(ref[worst]))
    assert ref[words].abs().min().item() > 1e-3                  # (the boundary columns do carry gradient)
    # embed.weight's gradient row by row: a row no token selects is exactly zero (one owner per table row, no atomics); a live
    # row is held to the tensor tolerance at the scale of the live rows (f32: worst entry; bf16: the row's L2 norm)
    g = grads["embed.0.weight"].detach().float().cpu().double()
    r = grads_o["embed.0.weight"].double()
    live = r.abs().amax(1) > 0
    assert (g[~live] == 0).all(), (~live & (g.abs().amax(1) > 0)).nonzero().flatten().tolist()[:8]
    assert any(bool(live[x]) for x in words)
    if dtype == "f32":
        row_err = (g - r).abs().amax(1)
        assert (row_err <= GRAD_TOL["f32"] * r.abs().max()).all(), int(row_err.argmax())
    else:
        rms = float(r[live].norm(dim=1).pow(2).mean().sqrt())
        row_err = (g - r).norm(dim=1)
        lim = GRAD_TOL["bf16"] * r.norm(dim=1).clamp_min(rms)
        assert (row_err <= lim).all(), (int((row_err / lim).argmax()), float((row_err / lim).max()))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("V1", [1023, 1024, 1025, 4096, 4097, 8192, 10240, 10241, 53249])
def test_training_step_at_the_vocabulary_thresholds_vs_oracle(V1, dtype):
    from unpaired_image_captioning_amd import _lib as L
    from unpaired_image_captioning_amd.trainer import xe_step
    cfg, W, b = training_case(V1)[:3]
    model = build_model(cfg, W, dtype)
    model.train()
    batch = {k: v.cuda() for k, v in b.items()}
    for fused in (True, False):
        loss, grads = xe_step(model, batch, fused=fused)
        check_training_step(V1, dtype, loss, grads)
    if V1 in (4096, 4097):
        # the early-gradient order gathers the embedding gradient in two halves: 2 * V1 keys through the 4096-key trips of the scan
        model.engine.recurrence = L.REC_EARLY_GRADS
        try:
            loss, grads = xe_step(model, batch, fused=True)
        finally:
            model.engine.recurrence = 0
        check_training_step(V1, dtype, loss, grads)


DEC_END, DEC_SCALE, WIDE_END, WIDE_SCALE = 6.0, 8.0, 6.0, 20.0
DECODE_TOL = {"f32": 1e-3, "bf16": 3e-2}          # (bf16 at 32 hidden units: test_greedy_decode_bf16_close's bound)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("V1", [15360, 15361, 16383, 16384])
def test_decoders_at_the_sampling_and_beam_thresholds_vs_oracle(V1, dtype):
    cfg = dict(SMALL, V=V1 - 1)
    W, b, words = weights_and_batch(V1, cfg, seed=V1 % 1000, end_bias=DEC_END, logit_scale=DEC_SCALE)
    idx = torch.arange(cfg["n_img"]) * cfg["S"]
    fc_h, att_h, am_h = b["fc_feats"][idx], b["att_feats"][idx], b["att_masks"][idx]
    fc, att, am = fc_h.cuda(), att_h.cuda(), am_h.cuda()
    L = cfg["L"]
    model = build_model(cfg, W, dtype).eval()
    tol = DECODE_TOL[dtype]
    # greedy: f32 the oracle's own ids; bf16 the device's tokens replayed by the oracle
    seq, lp = model(fc, None, att, am, opt={"sample_max": 1}, mode="sample")
    seq, lp = seq.cpu(), lp.cpu()
    if dtype == "f32":
        seq_o, lp_o = O.sample(W, fc_h, att_h, am_h, L)
        assert torch.equal(seq, seq_o) and absmax(lp, lp_o) < tol
    else:
        seq_o, lp_o = O.sample(W, fc_h, att_h, am_h, L, sample_max=0, forced_tokens=seq)
        assert torch.equal(seq, seq_o) and absmax(lp[alive_mask(seq)], lp_o[alive_mask(seq)]) < tol
    assert any(int(x) in words for x in seq.flatten())              # the boundary words are what gets decoded
    # multinomial, without and with the constraint that forbids repeating the previous word
    drawn = set()
    for dc in (0, 1):
        seq, lp = model(fc, None, att, am, opt={"sample_max": 0, "temperature": 1.0, "decoding_constraint": dc}, mode="sample")
        seq, lp = seq.cpu(), lp.cpu()
        assert int(seq.min()) >= 0 and int(seq.max()) < V1
        seq_o, lp_o = O.sample(W, fc_h, att_h, am_h, L, sample_max=0, forced_tokens=seq, decoding_constraint=dc)
        live = alive_mask(seq)
        assert torch.equal(seq_o, seq) and absmax(lp[live], lp_o[live]) < tol, dc
        if dc:
            assert not ((seq[:, 1:] == seq[:, :-1]) & (seq[:, 1:] > 0)).any()
        drawn |= set(seq.flatten().tolist())
    assert drawn & set(words)
    # beam search, 3 beams (the last word is barred by its -1000, so V1-2 is the top boundary word here)
    bseq, blp = model(fc, None, att, am, opt={"beam_size": 3}, mode="sample")
    bseq, blp = bseq.cpu(), blp.cpu()
    bseq_o, blp_o = O.sample_beam(W, fc_h, att_h, am_h, L, 3)
    if dtype == "f32":
        same = (bseq == bseq_o).all(1)
        assert same.float().mean().item() >= 0.7
        assert absmax(blp[same], blp_o[same]) < 1e-3
        assert (blp.sum(1) - blp_o.sum(1)).abs().max().item() < 2e-3
    else:
        # teacher-force the device's beams through the oracle (test_beam_search_bf16_and_real_vocab_vs_oracle's 5e-2 per step)
        labels = torch.cat([torch.zeros(len(idx), 1, dtype=torch.long), bseq, torch.zeros(len(idx), 1, dtype=torch.long)], 1)
        logp = O.forward_logprobs(W, fc_h, att_h, labels, am_h)
        for k in range(len(idx)):
            for t in range(L):
                tok = int(bseq[k, t])
                ref = logp[k, t, tok].item() - (1000.0 if tok == V1 - 1 else 0.0)
                assert abs(blp[k, t].item() - ref) < 5e-2, (k, t, blp[k, t].item(), ref)
                if tok == 0:
                    break
        assert (blp.sum(1) - blp_o.sum(1)).abs().max().item() < 5e-2 * L      # and they score what the oracle's best beams score


WIDE = dict(E=512, H=512, A=512, D=128, R=36, n_img=24, S=1, L=6)


@pytest.mark.parametrize("V1", [17, 10225, 10240, 10241])
def test_persistent_decode_at_its_vocabulary_bound(V1):
    """bf16, 512 hidden units, 24 rows: up to 10240 words the decode pass is ONE persistent launch -- the chain's multinomial
    tokens forced through it give the same ids and log-probs within 1e-2, and the oracle's replay of those tokens agrees too; at
    10241 words the launch chain runs instead, with the same result against the oracle."""
    from unpaired_image_captioning_amd import _lib as Lb
    cfg = dict(WIDE, V=V1 - 1)
    W, b, words = weights_and_batch(V1, cfg, seed=V1 % 1000, end_bias=WIDE_END if V1 > 100 else 0.0, logit_scale=WIDE_SCALE)
    fc, att, am = b["fc_feats"].cuda(), b["att_feats"].cuda(), b["att_masks"].cuda()
    L = cfg["L"]
    model = build_model(cfg, W, "bf16").eval()
    eng = poison_workspaces(model.engine)
    pd = {k: v.detach() for k, v in model.param_dict().items()}
    tol = LOGP_TOL["bf16"]

    def run(flags, sample_max, forced=None):
        eng.recurrence = flags
        try:
            out = eng.sample(pd, fc, att, am, L, sample_max=sample_max, seed=777, forced=forced)
        finally:
            eng.recurrence = 0
        return out[0].cpu(), out[1].cpu()

    before = Lb.persistent_status()
    seq_c, lp_c = run(Lb.REC_FWD_CHAIN, 0)
    mid = Lb.persistent_status()
    assert (mid[1], mid[2]) == (before[1], before[2])                  # the chain launched no persistent kernel
    seq_f, lp_f = run(0, 0, forced=seq_c.cuda())
    after = Lb.persistent_status()
    assert after[0] == 0 and after[2] == mid[2]
    assert after[1] - mid[1] == (1 if V1 <= 10240 else 0), (V1, mid, after)
    live = alive_mask(seq_c)
    assert torch.equal(seq_f, seq_c)
    assert (lp_f - lp_c)[live].abs().max().item() < tol
    seq_o, lp_o = O.sample(W, b["fc_feats"], b["att_feats"], b["att_masks"], L, sample_max=0, forced_tokens=seq_c)
    assert torch.equal(seq_o, seq_c)
    assert (lp_f - lp_o)[live].abs().max().item() < tol
    assert set(seq_c.flatten().tolist()) & set(words)                  # boundary words were drawn
    # greedy through the default path (persistent up to the bound), the device's tokens replayed by the oracle
    seq_g, lp_g = run(0, 1)
    last = Lb.persistent_status()
    assert last[0] == 0 and last[1] - after[1] == (1 if V1 <= 10240 else 0)
    seq_o, lp_o = O.sample(W, b["fc_feats"], b["att_feats"], b["att_masks"], L, sample_max=0, forced_tokens=seq_g)
    assert torch.equal(seq_o, seq_g)
    assert (lp_g - lp_o)[alive_mask(seq_g)].abs().max().item() < tol
