"""CPU restatement of the AdaAtt captioners in eval mode (AdaAtt_lstm, AdaAtt_attention, AdaAttCore, AdaAttModel, AdaAttMOModel of
the reference's models/AttModel.py), written from the maths: plain torch, any float dtype (the tests run it in float64).  It is the
reference of tests/test_gpu_adaatt*.py and is itself pinned to fixtures generated from the reference's own classes
(tests/golden/make_golden_adaatt.py -> tests/golden/adaatt*.npz; tests/test_adaatt_host.py).

Weights are a dict {reference state_dict key: tensor}.  `rnd` (default: identity) is applied where the device rounds to its operand
dtype -- GEMM operands, and every activation it stores in that dtype -- `bf16_round` gives the bf16 emulation that the bf16
tolerances are derived from.  `variant` switches ONE deliberate error on (the host tests show that the operator bounds catch it).
"""
import argparse
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BN_EPS = 1e-5
FIXTURES = ("adaatt_tiny", "adaattmo_tiny", "adaatt_bn1_ragged", "adaatt_nomask", "adaatt_bn2", "adaattmo_2layer_logit2")
BEAM = 3
MIN_GAP = 1e-2

# Tolerances of the model tests.  f32: the project's 1e-3 on log-probs.  bf16: max(1e-2, 4 x the deviation of the bf16-emulating
# restatement on the same case) -- the rule of transformer_cases.bf16_bounds; the deviations measured on the CPU are recorded here
# and bf16_bounds() asserts that what it recomputes agrees with them (within a quarter).
TOL_F32, TOL_BF16 = 1e-3, 1e-2
BF16_EMULATED = {
    "adaatt_tiny": 0.0290,
    "adaattmo_tiny": 0.0331,
    "adaatt_bn1_ragged": 0.0268,
    "adaatt_nomask": 0.0127,
    "adaatt_bn2": 0.0217,
    "adaattmo_2layer_logit2": 0.0351,
    "real": 0.0309,            # real_case(): E = H = A = 512, D = 2048, R = 36, V = 9487, L = 16
}
REAL = dict(V=9487, D=2048, Dfc=2048, H=512, n_img=4, R=36, L=16, use_bn=1, layers=1, logit_layers=1, maxout=1, seed=5)


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def ident(t):
    return t


# ---------------------------------------------------------------------------------------------------------------- fixtures
def load_fixture(name):
    """(cfg, W, I, O): cfg a dict of ints plus cfg['shapes'] = {state_dict key: shape} in the reference's order, W / I / O the weights,
    inputs and reference outputs as torch tensors (float weights are stored as bf16 bit patterns, `w16::`: exact)."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg, W, I, O, shapes = {}, {}, {}, {}, {}
    for k in z.files:
        kind, key = k.split("::", 1)
        if kind == "cfg":
            cfg[key] = int(z[k])
        elif kind == "shape":
            shapes[key] = tuple(int(x) for x in z[k])
        elif kind == "w16":
            W[key] = (torch.from_numpy(z[k].astype(np.int32)) << 16).view(torch.float32)
        elif kind == "w":
            W[key] = torch.from_numpy(z[k])
        elif kind == "in":
            I[key] = torch.from_numpy(z[k])
        elif kind == "out":
            O[key] = torch.from_numpy(z[k])
    W = {k: W[k].reshape(shapes[k]) for k in shapes}       # the reference's order
    cfg["shapes"] = shapes
    return cfg, W, I, O


def opt_of(cfg, compute_dtype="f32"):
    return argparse.Namespace(vocab_size=cfg["V"], input_encoding_size=cfg["H"], rnn_size=cfg["H"], att_hid_size=cfg["H"],
                              num_layers=cfg["layers"], drop_prob_lm=0.5, seq_length=cfg["L"], fc_feat_size=cfg["Dfc"], att_feat_size=cfg["D"],
                              use_bn=cfg["use_bn"], logit_layers=cfg["logit_layers"], caption_model="adaattmo" if cfg["maxout"] else "adaatt",
                              compute_dtype=compute_dtype)


def to64(W):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in W.items()}


def make_weights(cfg, seed, scale=3.0, end_bias=1.0):
    """A state_dict drawn like the reference's (the parameter tree is built in its order), every 2-D weight but the embedding scaled and
    the end token biased so that captions vary and end; BatchNorm given non-trivial statistics; all values bf16-representable."""
    from unpaired_image_captioning_amd import models
    torch.manual_seed(seed)
    model = models.setup(opt_of(cfg))
    g = torch.Generator().manual_seed(seed + 7)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if k.startswith("att_embed.") and v.dim() == 1 and cfg["use_bn"] and (k.startswith("att_embed.0.") or k.startswith("att_embed.4.")):
                if k.endswith("weight"):
                    v.copy_(1 + 0.2 * torch.randn(v.shape, generator=g))
                elif k.endswith("bias") or k.endswith("running_mean"):
                    v.copy_(0.1 * torch.randn(v.shape, generator=g))
                elif k.endswith("running_var"):
                    v.copy_(0.5 + torch.rand(v.shape, generator=g))
            elif v.dim() == 2 and not k.startswith("embed."):
                v.mul_(scale)
        last = [k for k in model.state_dict() if k.startswith("logit.") and k.endswith("bias")][-1]
        model.state_dict()[last][0] += end_bias
        for k, v in model.state_dict().items():
            if v.is_floating_point():
                v.copy_(v.to(torch.bfloat16).float())
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


# ---------------------------------------------------------------------------------------------------------------- the two operators
def cell(sums, n5, c_prev, H, maxout, variant=None):
    """AdaAtt_lstm.forward's pointwise part (:304-329) -> (next_c, next_h, fake or None)."""
    i, f, o = (torch.sigmoid(sums[:, k * H:(k + 1) * H]) for k in range(3))
    if variant == "swap_out":        # the maxout chunks taken where the out gate lies, and the reverse
        o = torch.sigmoid(sums[:, 3 * H:4 * H])
        tr = torch.maximum(sums[:, 2 * H:3 * H], sums[:, 4 * H:5 * H])
    elif maxout:
        tr = torch.maximum(sums[:, 3 * H:4 * H], sums[:, 4 * H:5 * H])
    else:
        tr = torch.tanh(sums[:, 3 * H:4 * H])
    c = i * tr + (f * c_prev if c_prev is not None else 0)
    tc = torch.tanh(c)
    fake = None
    if n5 is not None:
        fake = torch.sigmoid(n5) * (torch.tanh(c_prev if c_prev is not None else torch.zeros_like(c)) if variant == "fake_prev" else tc)
    return c, o * tc, fake


def attention(fr_e, hl_e, fr, hl, p_att, att, w, b, mask, row_div=1, variant=None):
    """AdaAtt_attention.forward between its linears (:383-402) -> (out [N, H], PI [N, R + 1]); rows n read image n // row_div."""
    idx = torch.arange(fr.shape[0]) // row_div
    emb = torch.cat([fr_e[:, None], p_att[idx]], 1)                      # [N, R + 1, A]
    e = torch.tanh(emb + hl_e[:, None]) @ w + b
    if variant == "no_max":
        ex = torch.exp(e)
    else:
        ex = torch.exp(e - e.max(1, keepdim=True).values)
    PI = ex / ex.sum(1, keepdim=True)
    if mask is not None:
        m = mask[idx]
        m = torch.cat([torch.ones_like(m[:, :1]) if variant == "sentinel_unmasked" else m[:, :1], m], 1)
        PI = PI * m
        if variant != "no_renorm":
            PI = PI / PI.sum(1, keepdim=True)
    out = (PI[:, :, None] * torch.cat([fr[:, None], att[idx]], 1)).sum(1)
    if variant != "no_hl":
        out = out + hl
    return out, PI


# ---------------------------------------------------------------------------------------------------------------- the model
def linear(x, w, b, rnd=ident):
    return rnd(x) @ rnd(w).t() + b


def clip_att(att, masks):
    if masks is not None:
        n = int(masks.long().sum(1).max())
        att, masks = att[:, :n], masks[:, :n]
    return att, masks


def prepare(W, cfg, fc, att, masks, rnd=ident):
    """_prepare_feature (:107-117) in eval mode -> (fc', att', p_att, masks); pack_wrapper leaves exact zeros in the padded regions."""
    att, masks = clip_att(att, masks)
    use_bn = cfg["use_bn"]
    lin = 1 if use_bn else 0
    fcp = rnd(torch.relu(linear(fc, W["fc_embed.0.weight"], W["fc_embed.0.bias"], rnd)))
    aw, ab = W["att_embed.%d.weight" % lin], W["att_embed.%d.bias" % lin]
    x = att
    if use_bn:          # BatchNorm1d(D) on running statistics; its affine part folded into the Linear, as the device does
        x = (x - W["att_embed.0.running_mean"]) / torch.sqrt(W["att_embed.0.running_var"] + BN_EPS)
        ab = ab + aw @ W["att_embed.0.bias"]
        aw = aw * W["att_embed.0.weight"][None, :]
    y = torch.relu(linear(x, aw, ab, rnd))
    if use_bn == 2:
        alpha = W["att_embed.4.weight"] / torch.sqrt(W["att_embed.4.running_var"] + BN_EPS)
        y = (y - W["att_embed.4.running_mean"]) * alpha + W["att_embed.4.bias"]
    if masks is not None:
        valid = torch.arange(att.shape[1])[None, :] < masks.long().sum(1)[:, None]
        y = y * valid[..., None].to(y.dtype)
    attp = rnd(y)
    patt = rnd(linear(attp, W["ctx2att.weight"], W["ctx2att.bias"], rnd))
    return fcp, attp, patt, masks


def _logit_keys(cfg):
    n = cfg["logit_layers"]
    if n == 1:
        return [], "logit"
    return ["logit.%d" % (3 * l) for l in range(n - 1)], "logit.%d" % (3 * (n - 1))


def core(W, cfg, xt, fcp, attp, patt, masks, state, rnd=ident, row_div=1):
    """AdaAttCore.forward (:415-418) -> (h [N, H], new state)."""
    H, layers, maxout = cfg["H"], cfg["layers"], cfg["maxout"]
    p = "core.lstm."
    idx = torch.arange(xt.shape[0]) // row_div
    hs, cs, fake = [], [], None
    for l in range(layers):
        ph, pc = state[0][l], state[1][l]
        last = l == layers - 1
        if l == 0:
            x = xt
            i2h = linear(x, W[p + "w2h.weight"], W[p + "w2h.bias"], rnd) + linear(fcp, W[p + "v2h.weight"], W[p + "v2h.bias"], rnd)[idx]
        else:
            x = hs[-1]
            i2h = linear(x, W[p + "i2h.%d.weight" % (l - 1)], W[p + "i2h.%d.bias" % (l - 1)], rnd)
        sums = i2h + linear(ph, W[p + "h2h.%d.weight" % l], W[p + "h2h.%d.bias" % l], rnd)
        n5 = None
        if last:
            if l == 0:
                r = linear(x, W[p + "r_w2h.weight"], W[p + "r_w2h.bias"], rnd) + linear(fcp, W[p + "r_v2h.weight"], W[p + "r_v2h.bias"], rnd)[idx]
            else:
                r = linear(x, W[p + "r_i2h.weight"], W[p + "r_i2h.bias"], rnd)
            n5 = r + linear(ph, W[p + "r_h2h.weight"], W[p + "r_h2h.bias"], rnd)
        c, h, f = cell(sums, n5, pc, H, maxout)
        hs.append(rnd(h))
        cs.append(c)
        if last:
            fake = rnd(f)
    a = "core.attention."
    fr = rnd(torch.relu(linear(fake, W[a + "fr_linear.0.weight"], W[a + "fr_linear.0.bias"], rnd)))
    fr_e = linear(fr, W[a + "fr_embed.weight"], W[a + "fr_embed.bias"], rnd)
    hl = rnd(torch.tanh(linear(hs[-1], W[a + "ho_linear.0.weight"], W[a + "ho_linear.0.bias"], rnd)))
    hl_e = linear(hl, W[a + "ho_embed.weight"], W[a + "ho_embed.bias"], rnd)
    out, _ = attention(fr_e, hl_e, fr, hl, patt, attp, W[a + "alpha_net.weight"][0], W[a + "alpha_net.bias"][0], masks, row_div)
    h = rnd(torch.tanh(linear(rnd(out), W[a + "att2h.weight"], W[a + "att2h.bias"], rnd)))
    return h, (torch.stack(hs), torch.stack(cs))


def logprobs_state(W, cfg, it, fcp, attp, patt, masks, state, rnd=ident, row_div=1):
    """get_logprobs_state (:158-165)."""
    xt = rnd(torch.relu(W["embed.0.weight"][it]))
    x, state = core(W, cfg, xt, fcp, attp, patt, masks, state, rnd, row_div)
    hidden, last = _logit_keys(cfg)
    for k in hidden:
        x = rnd(torch.relu(linear(x, W[k + ".weight"], W[k + ".bias"], rnd)))
    return torch.log_softmax(linear(x, W[last + ".weight"], W[last + ".bias"], rnd), 1), state


def init_state(cfg, n, dtype):
    return (torch.zeros(cfg["layers"], n, cfg["H"], dtype=dtype), torch.zeros(cfg["layers"], n, cfg["H"], dtype=dtype))


def forward(W, cfg, fc, att, masks, seq, rnd=ident):
    """_forward (:119-156): log-probs [n, seq.size(1) - 1, V + 1], zeros behind the early break."""
    fcp, attp, patt, m = prepare(W, cfg, fc, att, masks, rnd)
    n, T = seq.shape[0], seq.shape[1] - 1
    out = torch.zeros(n, T, cfg["V"] + 1, dtype=fcp.dtype)
    state = init_state(cfg, n, fcp.dtype)
    for i in range(T):
        if i >= 1 and seq[:, i].sum() == 0:
            break
        out[:, i], state = logprobs_state(W, cfg, seq[:, i], fcp, attp, patt, m, state, rnd)
    return out


def sample_greedy(W, cfg, fc, att, masks, decoding_constraint=0):
    """_sample with sample_max (:198-253): (seq [n, L], seqLogprobs [n, L], the smallest winner / runner-up gap over the live steps)."""
    fcp, attp, patt, m = prepare(W, cfg, fc, att, masks)
    n, L = fc.shape[0], cfg["L"]
    seq = torch.zeros(n, L, dtype=torch.int64)
    lp = torch.zeros(n, L, dtype=fcp.dtype)
    state = init_state(cfg, n, fcp.dtype)
    it = torch.zeros(n, dtype=torch.int64)
    unfinished = torch.ones(n, dtype=torch.bool)
    gap = float("inf")
    for t in range(L):
        logp, state = logprobs_state(W, cfg, it, fcp, attp, patt, m, state)
        if decoding_constraint and t > 0:
            logp = logp.scatter(1, seq[:, t - 1:t], float("-inf"))
        top = logp.topk(2, 1).values
        if unfinished.any():
            gap = min(gap, float((top[:, 0] - top[:, 1])[unfinished].min()))
        best, it = logp.max(1)
        unfinished = unfinished & (it > 0)
        it = it * unfinished.long()
        seq[:, t], lp[:, t] = it, best
        if not unfinished.any():
            break
    return seq, lp, gap


def rescore(W, cfg, fc, att, masks, seq, temperature=None):
    """Teacher-forced log-probs of decoded tokens [n, L]: position t scores seq[:, t] given <bos> seq[:, :t] (the recurrence is the
    same one, so this is exact wherever the row is live)."""
    n, L = seq.shape
    fcp, attp, patt, m = prepare(W, cfg, fc, att, masks)
    state = init_state(cfg, n, fcp.dtype)
    it = torch.zeros(n, dtype=torch.int64)
    out = torch.zeros(n, L, dtype=fcp.dtype)
    top = torch.zeros(n, L, dtype=fcp.dtype)
    for t in range(L):
        logp, state = logprobs_state(W, cfg, it, fcp, attp, patt, m, state)
        out[:, t] = logp.gather(1, seq[:, t:t + 1]).squeeze(1)
        top[:, t] = logp.max(1).values
        it = seq[:, t]
    return out, top


def live_positions(seq):
    """[n, L] bool: positions up to and including each row's first 0."""
    ended = torch.cat([torch.zeros(seq.shape[0], 1, dtype=torch.bool), (seq == 0)[:, :-1]], 1)
    return ended.long().cumsum(1) == 0


def beam_search(W, cfg, fc, att, masks, beam_size, max_ppl=0):
    """_sample_beam over CaptionModel.beam_search, group_size 1, image by image.  -> (seq [n, L], logps [n, L], done lists, the
    smallest gap between the last accepted and the first rejected candidate over all decisions).  done[k] = [(seq, logps, p)] sorted
    by -p (stable), the first beam_size."""
    fcp, attp, patt, m = prepare(W, cfg, fc, att, masks)
    n, B, L = fc.shape[0], beam_size, cfg["L"]
    out_seq = torch.zeros(n, L, dtype=torch.int64)
    out_lp = torch.zeros(n, L, dtype=fcp.dtype)
    done_all, gap = [], float("inf")
    for k in range(n):
        feats = (fcp[k:k + 1], attp[k:k + 1], patt[k:k + 1], m[k:k + 1] if m is not None else None)
        state = init_state(cfg, B, fcp.dtype)
        logp, state = logprobs_state(W, cfg, torch.zeros(B, dtype=torch.int64), *feats, state, row_div=B)
        beam_seq = torch.zeros(L, B, dtype=torch.int64)
        beam_lp = torch.zeros(L, B, dtype=fcp.dtype)
        beam_sum = torch.zeros(B, dtype=fcp.dtype)
        done = []
        for t in range(L):
            f = logp.clone()
            f[:, -1] -= 1000
            vals, ix = torch.sort(f, 1, True)
            rows = 1 if t == 0 else B
            cand = [(int(ix[q, c]), q, float(beam_sum[q] + vals[q, c]), vals[q, c]) for c in range(min(B, f.shape[1])) for q in range(rows)]
            cand.sort(key=lambda x: -x[2])
            if len(cand) > B and cand[B - 1][2] > -500:      # (finished beams sit at -1000: nothing kept depends on their order)
                gap = min(gap, cand[B - 1][2] - cand[B][2])
            prev_seq, prev_lp = beam_seq[:t].clone(), beam_lp[:t].clone()
            parents = []
            for vix in range(B):
                c, q, p, r = cand[vix]
                beam_seq[:t, vix], beam_lp[:t, vix] = prev_seq[:, q], prev_lp[:, q]
                parents.append(q)
                beam_seq[t, vix], beam_lp[t, vix], beam_sum[vix] = c, r, p
            state = (state[0][:, parents], state[1][:, parents])
            for vix in range(B):
                if beam_seq[t, vix] == 0 or t == L - 1:
                    p = float(beam_sum[vix])
                    done.append((beam_seq[:, vix].clone(), beam_lp[:, vix].clone(), p / (t + 1) if max_ppl else p))
                    beam_sum[vix] = -1000
            if t + 1 < L:
                logp, state = logprobs_state(W, cfg, beam_seq[t].clone(), *feats, state, row_div=B)
        done = sorted(done, key=lambda x: -x[2])
        for a, b in zip(done[:B], done[1:B + 1]):            # the order of the kept list, and its cut
            gap = min(gap, a[2] - b[2])
        done = done[:B]
        done_all.append(done)
        out_seq[k], out_lp[k] = done[0][0], done[0][1]
    return out_seq, out_lp, done_all, gap


def bf16_bounds(name, W64, cfg, fc, att, masks, labels):
    """The log-prob bound of a bf16 run of this case: 4 x the deviation of the bf16-emulating restatement from the plain one (float64
    inputs), at least TOL_BF16; the deviation must be the one recorded in BF16_EMULATED (within a quarter)."""
    ref = forward(W64, cfg, fc, att, masks, labels)
    emu = forward(W64, cfg, fc, att, masks, labels, rnd=bf16_round)
    dev = (emu - ref).abs().max().item()
    want = BF16_EMULATED[name]
    assert abs(dev - want) < 0.25 * want, (name, dev, want)
    return max(TOL_BF16, 4 * dev)


def synthetic_inputs(V, D, Dfc, n_img, R, L, masks, seed):
    """fc / att features, att_masks ('ragged': lengths 2..R, the first full; 'one': also an image with one region; None) and labels
    [n, L + 2] with one empty caption."""
    g = torch.Generator().manual_seed(1000 + seed)
    fc = torch.randn(n_img, Dfc, generator=g).abs()
    att = torch.randn(n_img, R, D, generator=g)
    am = None
    if masks is not None:
        lens = torch.randint(2, R + 1, (n_img,), generator=g)
        lens[0] = R
        if masks == "one":
            lens[-1] = 1
        am = (torch.arange(R)[None, :] < lens[:, None]).float()
    labels = torch.zeros(n_img, L + 2, dtype=torch.int64)
    for i in range(n_img):
        n = int(torch.randint(1, L + 1, (1,), generator=g))
        labels[i, 1:1 + n] = torch.randint(1, V + 1, (n,), generator=g)
    labels[1] = 0                                     # an empty caption
    return fc, att, am, labels


_real = {}


def real_case():
    """The one case at the real widths: weights from a seed (a fixture would be ~40 MB), 4 images x 36 regions x 2048 with ragged masks,
    captions of up to 16 words.  -> (cfg, W f32, fc, att, masks, labels)."""
    if not _real:
        c = dict(REAL)
        W = make_weights(c, c["seed"])
        fc, att, am, labels = synthetic_inputs(c["V"], c["D"], c["Dfc"], c["n_img"], c["R"], c["L"], "ragged", c["seed"])
        _real["case"] = (c, W, fc, att.abs(), am, labels)
    return _real["case"]


# ---------------------------------------------------------------------------------------------------------------- operator cases
EPS32 = 2.0 ** -24          # unit roundoff of f32
EPS_BF16 = 2.0 ** -8        # ... of bf16 (8 significand bits, round to nearest: half a unit in the last place, relative to the value)


def round_to(t, dtype):
    """float64 values exactly representable in the operand dtype ('f32' / 'bf16')."""
    return (t.float() if dtype == "f32" else t.to(torch.bfloat16)).double()


# (N, H, maxout, ld_sums extra, n5: 'inside' the sums buffer | 'apart' | None, c_prev given, pre-activation scale)
CELL_CASES = [
    (1, 8, 0, 0, "inside", True, 1.0),
    (3, 40, 1, 8, "apart", True, 1.0),
    (33, 512, 1, 0, "inside", True, 1.0),
    (33, 40, 0, 4, None, True, 1.0),              # a layer below the last: no sentinel
    (3, 8, 1, 0, "inside", False, 1.0),           # c_prev NULL
    (3, 40, 0, 0, "apart", True, 30.0),           # pre-activations at +-30
    (1, 512, 0, 16, "inside", False, 30.0),
]


def cell_inputs(case, dtype, seed=0):
    N, H, maxout, extra, n5, has_c, scale = case
    g = torch.Generator().manual_seed(77 + seed + 13 * N + H)
    G = 4 + maxout
    sums = torch.randn(N, G * H, generator=g, dtype=torch.float64) * 1.5
    q = torch.randn(N, H, generator=g, dtype=torch.float64) * 1.5
    if scale != 1.0:      # every pre-activation at +-scale
        sums, q = torch.sign(sums) * scale, torch.sign(q) * scale
    c_prev = torch.randn(N, H, generator=g, dtype=torch.float64) * 2 if has_c else None
    f = lambda t: None if t is None else t.float().double()          # noqa: E731 (sums, n5 and c are f32 on the device)
    return dict(N=N, H=H, maxout=maxout, ld_extra=extra, n5_mode=n5, sums=f(sums), n5=f(q) if n5 else None, c_prev=f(c_prev))


def cell_bounds(inp, ref, dtype):
    """(bound c, bound h, bound fake), absolute, per element.  Counted: a sigmoid is exp, add, divide, an f32 libm call within 2 ulp --
    4 roundings; the hardware forms of the bf16 path (v_exp_f32, v_rcp_f32: 1 ulp each) add the argument's scaling, whose rounding
    error the exponential multiplies by |x| <= 30: 40 roundings cover it.  c = f c_prev + i tr: both products carry their factor's
    error, then one add -- (n + 3) eps (|c_prev| + |tr|).  tanh(c) has slope <= 1: the error of c passes through, plus its own; h and
    fake are products of two such factors in [-1, 1].  A bf16 output adds its rounding, 2^-8 |value|."""
    n = 4 if dtype == "f32" else 40
    c, h, fake = ref
    H, mo = inp["H"], inp["maxout"]
    tr = torch.maximum(inp["sums"][:, 3 * H:4 * H], inp["sums"][:, 4 * H:5 * H]).abs() if mo else torch.ones_like(c)
    bc = (n + 3) * EPS32 * ((inp["c_prev"].abs() if inp["c_prev"] is not None else 0) + tr) + EPS32
    bo = bc + (2 * n + 2) * EPS32
    out_r = EPS_BF16 if dtype == "bf16" else 0.0
    return bc, bo + out_r * h.abs(), (bo + out_r * fake.abs()) if fake is not None else None


# (N, R, A, H, row_div, mask: None | 'ragged' | 'm0', saturated)
ATT_CASES = [
    (3, 1, 8, 8, 1, None, False),
    (3, 2, 16, 8, 1, "ragged", False),
    (6, 36, 64, 520, 3, "ragged", False),
    (2, 63, 520, 64, 1, None, False),             # 64 slots: one wave exactly
    (3, 64, 40, 48, 3, "m0", False),              # 65 slots cross a wave; m_0 = 0 with later ones set
    (2, 36, 64, 64, 1, None, True),               # sum |w| ~ 100: exp overflows f32 without the maximum
    (2, 5, 64, 64, 1, "m0", True),
]


def att_inputs(case, dtype, seed=0):
    N, R, A, H, div, mask, sat = case
    g = torch.Generator().manual_seed(91 + seed + 7 * R + A)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)          # noqa: E731
    n_img = N // div
    w = rn(A) * (100.0 / (0.8 * A) if sat else 8.0 / A)
    p_att, hl_e, fr_e = rn(n_img, R, A), rn(N, A), rn(N, A)
    if sat:       # the scores of the first region and of the sentinel reach +sum |w|, the others -sum |w| .. sum |w|
        p_att[:, 0] = torch.sign(w) * 20
        p_att[:, 1:] = p_att[:, 1:] * 3
        fr_e = torch.sign(w)[None, :] * 19.5 + 0 * fr_e
        hl_e = hl_e * 0.1
    m = None
    if mask is not None:
        lens = torch.randint(1, R + 1, (n_img,), generator=g)
        lens[0] = R
        lens[-1] = max(1, R - 1)                  # (at least one image with padded regions)
        m = (torch.arange(R)[None, :] < lens[:, None]).double()
        if mask == "m0":
            m[-1] = 1
            m[-1, 0] = 0
    f32 = lambda t: t.float().double()          # noqa: E731
    return dict(N=N, R=R, A=A, H=H, row_div=div, fr_e=f32(fr_e), hl_e=f32(hl_e), fr=round_to(rn(N, H), dtype), hl=round_to(rn(N, H), dtype),
                p_att=round_to(p_att, dtype), att=round_to(rn(n_img, R, H), dtype), w=f32(w), b=f32(rn(1))[0], mask=m)


def att_bounds(inp, ref, dtype):
    """(bound out per element, bound PI), absolute.  Counted: a score is a sum of A terms w_a tanh(x_a); tanh within 4 roundings on the
    f32 path (add, libm), 12 on the bf16 path (add, scaling, v_exp_f32, add, v_rcp_f32, multiply, subtract -- absolute, |tanh| <= 1),
    the sum within A roundings of sum |w| in any order: d e = (A + n) eps sum |w| + eps |b|.  Softmax: d PI_s <= PI_s (2 d e + 6 eps)
    (shift, exp within 2 ulp of an argument off by d e, divide), twice over with the mask's renormalisation; sum_s d PI_s is the same
    figure.  out = sum_s PI_s v_s + hl: sum_s |d PI_s| |v_s| + (R + 3) eps sum PI |v| + eps |hl|.  A bf16 output adds 2^-8 |value|."""
    n = 4 if dtype == "f32" else 12
    out, PI = ref
    de = (inp["A"] + n) * EPS32 * float(inp["w"].abs().sum()) + EPS32 * abs(float(inp["b"]))
    dpi = 2 * (2 * de + 6 * EPS32)
    vmax = max(float(inp["fr"].abs().max()), float(inp["att"].abs().max()))
    bo = dpi * vmax + (inp["R"] + 3) * EPS32 * vmax + EPS32 * inp["hl"].abs()
    if dtype == "bf16":
        bo = bo + EPS_BF16 * out.abs()
    return bo, dpi * torch.ones_like(PI) + EPS32


def att_lds_bytes(R, A, H):
    return 4 * (3 * A + (R + 1 + 3) // 4 * 4 + 4 * H)
