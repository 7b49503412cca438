"""CPU restatement of the Transformer captioner in eval mode (the reference's models/TransformerModel.py), written from the
maths: plain torch, any float dtype (the tests run it in float64).  It is the reference of tests/test_gpu_transformer*.py and is
itself pinned to fixtures generated from the reference's own module (tests/golden/make_golden_transformer.py ->
tests/golden/transformer_*.npz; tests/test_transformer_host.py).

Weights are a dict {reference state_dict key: tensor}.  `rnd` (default: identity) is applied to every GEMM operand at the points
where the device rounds to its operand dtype -- `bf16_round` gives the bf16 emulation that the bf16 tolerances are derived from.
"""
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H = 8                      # make_model(..., h=8)
LN_EPS = 1e-6
BN_EPS = 1e-5
MASK_FILL = -1e9
FIXTURES = ("transformer_tiny", "transformer_bn1_wide", "transformer_bn2", "transformer_nomask")

# Tolerances.  f32: the project's 1e-3 on log-probs (1e-5 on single operators with O(1) outputs).
# bf16: the project's 1e-2 is out of reach of ANY bf16 evaluation of these cases: generator.proj is scaled by 6 (so that the decisions
# are clear), the log-probs reach magnitudes of 20-40, and the restatement itself, run in float64 with only its GEMM operands rounded
# to bf16 where the device rounds them (rnd=bf16_round), moves by BF16_EMULATED below.  The bound is therefore derived, not chosen:
# 4 x the emulated deviation of the same case (never below 1e-2), recomputed by the tests from the restatement alone; the values
# measured on the CPU are written here and the tests assert that what they recompute agrees with them.
#   name: (largest |d log-prob| of forward(), largest |d memory| of encode())
TOL_F32, TOL_BF16 = 1e-3, 1e-2
BF16_EMULATED = {
    "transformer_tiny": (0.127, 0.0209),
    "transformer_bn1_wide": (0.0967, 0.0192),
    "transformer_bn2": (0.0936, 0.0131),
    "transformer_nomask": (0.0844, 0.0193),
    "real": (0.0632, None),          # real_case(): depth 6, d_model 512, d_ff 1300, V 9487
}
REAL = dict(V=9487, D=2048, d_model=512, d_ff=1300, N=6, n_img=8, R=36, L=16, use_bn=1, seed=11)


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def ident(t):
    return t


# ---------------------------------------------------------------------------------------------------------------- fixtures
def load_fixture(name):
    """(cfg, W, I, O): cfg a dict of ints plus cfg['shapes'] = {state_dict key: shape} in the reference's order, W / I / O the `w::` /
    `in::` / `out::` entries as torch tensors.  The sinusoidal buffer is stored by its first 64 rows only (5000 rows are over a
    megabyte): it is rebuilt here and checked against them."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg, W, I, O, shapes = {}, {}, {}, {}, {}
    for k in z.files:
        kind, key = k.split("::", 1)
        if kind == "cfg":
            cfg[key] = int(z[k])
        elif kind == "shape":
            shapes[key] = tuple(int(x) for x in z[k])
        elif kind == "w16":        # a float32 whose low 16 bits are zero, stored as its high half
            W[key] = torch.from_numpy((z[k].astype(np.uint32) << 16).view(np.float32))
        elif kind in ("w", "in", "out"):
            {"w": W, "in": I, "out": O}[kind][key] = torch.from_numpy(z[k])
    pe = positional_table(cfg["d_model"])
    head = torch.from_numpy(z["pe::head"])
    # the table is sin / cos of position * exp(...) in f32: one ulp of the exponential (6e-8 relative, a matter of the host's
    # vector maths library) moves row p by p * 6e-8 -- up to 4e-6 over the 64 stored rows, 2e-5 with room for a few ulps
    assert torch.allclose(pe[0, :head.shape[0]], head, rtol=0, atol=2e-5), "positional table differs from the reference's"
    pe[0, :head.shape[0]] = head          # the rows the cases use (L + 1 <= 64) are the reference's own, bit for bit
    W["model.tgt_embed.1.pe"] = pe
    cfg["shapes"] = shapes
    return cfg, W, I, O


def state_dict_keys(cfg_or_layers, use_bn=0):
    """The reference's state_dict keys, in its order."""
    N = cfg_or_layers if isinstance(cfg_or_layers, int) else cfg_or_layers["N"]
    keys = []
    bn = lambda i: ["att_embed.%d.%s" % (i, s) for s in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    if use_bn:
        keys += bn(0)
    keys += ["att_embed.%d.weight" % (1 if use_bn else 0), "att_embed.%d.bias" % (1 if use_bn else 0)]
    if use_bn == 2:
        keys += bn(4)
    attn = lambda p: ["%s.linears.%d.%s" % (p, i, s) for i in range(4) for s in ("weight", "bias")]
    ffn = lambda p: ["%s.%s.%s" % (p, m, s) for m in ("w_1", "w_2") for s in ("weight", "bias")]
    norms = lambda p, n: ["%s.sublayer.%d.norm.%s" % (p, i, s) for i in range(n) for s in ("a_2", "b_2")]
    for l in range(N):
        p = "model.encoder.layers.%d" % l
        keys += attn(p + ".self_attn") + ffn(p + ".feed_forward") + norms(p, 2)
    keys += ["model.encoder.norm.a_2", "model.encoder.norm.b_2"]
    for l in range(N):
        p = "model.decoder.layers.%d" % l
        keys += attn(p + ".self_attn") + attn(p + ".src_attn") + ffn(p + ".feed_forward") + norms(p, 3)
    keys += ["model.decoder.norm.a_2", "model.decoder.norm.b_2", "model.tgt_embed.0.lut.weight", "model.tgt_embed.1.pe",
             "model.generator.proj.weight", "model.generator.proj.bias"]
    return keys


def positional_table(d_model, max_len=5000):
    pe = torch.zeros(max_len, d_model)
    position = torch.arange(0, max_len).unsqueeze(1).float()
    div_term = torch.exp(torch.arange(0, d_model, 2).float() * -(math.log(10000.0) / d_model))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe.unsqueeze(0)


def make_weights(V1, D, d_model, d_ff, N, use_bn=0, seed=0, gen_scale=6.0, eos_bias=1.5):
    """A seeded model without the reference: Xavier-uniform on every matrix of `model`, nn.Linear's default range on att_embed, ones /
    zeros on the norms, non-trivial BatchNorm tensors; generator.proj scaled so that decisions are clear and some captions end early
    (as tests/test_gpu_ensemble.py does)."""
    g = torch.Generator().manual_seed(seed)
    W = {}

    def xavier(out_f, in_f):
        a = math.sqrt(6.0 / (in_f + out_f))
        return (torch.rand(out_f, in_f, generator=g) * 2 - 1) * a

    def bias(n, fan_in):
        a = 1.0 / math.sqrt(fan_in)
        return (torch.rand(n, generator=g) * 2 - 1) * a

    for k in state_dict_keys(N, use_bn):
        if k.endswith("num_batches_tracked"):
            W[k] = torch.tensor(0, dtype=torch.int64)
        elif k.startswith("att_embed"):
            i = int(k.split(".")[1])
            width = D if i == 0 else d_model
            if use_bn and i in (0, 4):
                W[k] = {"weight": 1 + 0.2 * torch.randn(width, generator=g), "bias": 0.1 * torch.randn(width, generator=g),
                        "running_mean": 0.1 * torch.randn(width, generator=g), "running_var": 0.5 + torch.rand(width, generator=g)}[k.split(".")[2]]
            else:
                W[k] = (torch.rand(d_model, D, generator=g) * 2 - 1) / math.sqrt(D) if k.endswith("weight") else bias(d_model, D)
        elif k.endswith("a_2"):
            W[k] = torch.ones(d_model)
        elif k.endswith("b_2"):
            W[k] = torch.zeros(d_model)
        elif k.endswith("pe"):
            W[k] = positional_table(d_model)
        elif k.endswith("lut.weight"):
            W[k] = xavier(V1, d_model)
        elif "w_1" in k:
            W[k] = xavier(d_ff, d_model) if k.endswith("weight") else bias(d_ff, d_model)
        elif "w_2" in k:
            W[k] = xavier(d_model, d_ff) if k.endswith("weight") else bias(d_model, d_ff)
        elif "generator" in k:
            W[k] = xavier(V1, d_model) * gen_scale if k.endswith("weight") else bias(V1, d_model)
        else:
            W[k] = xavier(d_model, d_model) if k.endswith("weight") else bias(d_model, d_model)
    W["model.generator.proj.bias"][0] += eos_bias
    return W


def cast_weights(W, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in W.items()}


# ---------------------------------------------------------------------------------------------------------------- operators
def layer_norm(x, a, b, eps=LN_EPS):
    """a (x - mean) / (std + eps) + b with the unbiased std: not nn.LayerNorm."""
    mean = x.mean(-1, keepdim=True)
    std = x.std(-1, keepdim=True)          # torch's default: divisor d - 1
    return a * (x - mean) / (std + eps) + b


def attention(Q, K, V, d_k, key_mask=None, causal=False, q_offset=0, row_div=1):
    """Q [B, Sq, h d_k], K / V [B / row_div, Sk, h d_k] -> [B, Sq, h d_k]; key_mask [B, Sk] (0 = masked) or None."""
    B, Sq, Sk = Q.shape[0], Q.shape[1], K.shape[1]
    h = Q.shape[2] // d_k
    if row_div > 1:
        K, V = K.repeat_interleave(row_div, 0), V.repeat_interleave(row_div, 0)
    q = Q.reshape(B, Sq, h, d_k).transpose(1, 2)
    k = K.reshape(B, Sk, h, d_k).transpose(1, 2)
    v = V.reshape(B, Sk, h, d_k).transpose(1, 2)
    scores = q @ k.transpose(-2, -1) / math.sqrt(d_k)
    keep = torch.ones(B, 1, Sq, Sk, dtype=torch.bool)
    if key_mask is not None:
        keep = keep & (key_mask != 0)[:, None, None, :]
    if causal:
        keep = keep & (torch.arange(Sk)[None, :] <= (q_offset + torch.arange(Sq))[:, None])[None, None]
    scores = scores.masked_fill(~keep, MASK_FILL)
    p = torch.softmax(scores, -1)
    return (p @ v).transpose(1, 2).reshape(B, Sq, h * d_k)


def linear(x, W, b, rnd=ident):
    return rnd(x) @ rnd(W).t() + b


def mha(W, prefix, xq, xkv, key_mask, causal, rnd=ident, taps=None):
    d_k = xq.shape[-1] // H
    lin = lambda i, x: linear(x, W["%s.linears.%d.weight" % (prefix, i)], W["%s.linears.%d.bias" % (prefix, i)], rnd)
    q, k, v = rnd(lin(0, xq)), rnd(lin(1, xkv)), rnd(lin(2, xkv))
    ctx = rnd(attention(q, k, v, d_k, key_mask, causal))
    if taps is not None:
        taps[prefix + ".ctx"] = ctx
    return lin(3, ctx)


def ffn(W, prefix, x, rnd=ident):
    hid = rnd(torch.relu(linear(x, W[prefix + ".w_1.weight"], W[prefix + ".w_1.bias"], rnd)))
    return linear(hid, W[prefix + ".w_2.weight"], W[prefix + ".w_2.bias"], rnd)


def _norm(W, prefix, x, rnd=ident):
    return rnd(layer_norm(x, W[prefix + ".a_2"], W[prefix + ".b_2"]))


# ---------------------------------------------------------------------------------------------------------------- the model
def clip_att(att, masks):
    if masks is not None:
        n = int(masks.long().sum(1).max())
        att, masks = att[:, :n], masks[:, :n]
    return att, masks


def batch_norm_eval(W, prefix, x):
    """BatchNorm1d on running statistics: y = x alpha + beta, alpha = gamma / sqrt(var + eps), beta = bias - mean alpha."""
    alpha = W[prefix + ".weight"] / torch.sqrt(W[prefix + ".running_var"] + BN_EPS)
    return x * alpha + (W[prefix + ".bias"] - W[prefix + ".running_mean"] * alpha)


def att_embed(W, att, masks, use_bn, rnd=ident):
    """pack_wrapper(att_embed): the valid regions through (BN) Linear ReLU (BN), exact zeros elsewhere."""
    lin = 1 if use_bn else 0
    x = att
    if use_bn:
        x = batch_norm_eval(W, "att_embed.0", x)
    x = torch.relu(linear(x, W["att_embed.%d.weight" % lin], W["att_embed.%d.bias" % lin], rnd))
    if use_bn == 2:
        x = batch_norm_eval(W, "att_embed.4", x)
    if masks is not None:
        lens = masks.long().sum(1)
        valid = torch.arange(att.shape[1])[None, :] < lens[:, None]
        x = x * valid[..., None].to(x.dtype)
    return x


def encode(W, att, masks, N, use_bn, rnd=ident, taps=None):
    """-> (memory [n, R', d_model], key mask [n, R'])."""
    att, masks = clip_att(att, masks)
    x = att_embed(W, att, masks, use_bn, rnd)
    if taps is not None:
        taps["att_embed"] = x
    kmask = masks if masks is not None else torch.ones(att.shape[:2], dtype=att.dtype)
    for l in range(N):
        p = "model.encoder.layers.%d" % l
        xn = _norm(W, p + ".sublayer.0.norm", x, rnd)
        x = x + mha(W, p + ".self_attn", xn, xn, kmask, False, rnd, taps if l == 0 else None)
        if taps is not None and l == 0:
            taps["enc0.after_attn"] = x
        x = x + ffn(W, p + ".feed_forward", _norm(W, p + ".sublayer.1.norm", x, rnd), rnd)
        if taps is not None and l == 0:
            taps["enc0.out"] = x
    return _norm(W, "model.encoder.norm", x, rnd), kmask


def target_embed(W, tokens, pos0=0):
    lut, pe = W["model.tgt_embed.0.lut.weight"], W["model.tgt_embed.1.pe"]
    return lut[tokens] * math.sqrt(lut.shape[1]) + pe[0, pos0:pos0 + tokens.shape[1]].to(lut.dtype)


def decode(W, memory, kmask, tokens, tmask, N, rnd=ident):
    """The decoder stack over `tokens` [n, T] (causal, key mask tmask [n, T] or None) -> norm(x) [n, T, d_model]."""
    x = target_embed(W, tokens)
    for l in range(N):
        p = "model.decoder.layers.%d" % l
        xn = _norm(W, p + ".sublayer.0.norm", x, rnd)
        x = x + mha(W, p + ".self_attn", xn, xn, tmask, True, rnd)
        x = x + mha(W, p + ".src_attn", _norm(W, p + ".sublayer.1.norm", x, rnd), memory, kmask, False, rnd)
        x = x + ffn(W, p + ".feed_forward", _norm(W, p + ".sublayer.2.norm", x, rnd), rnd)
    return _norm(W, "model.decoder.norm", x, rnd)


def generator(W, x, rnd=ident):
    return torch.log_softmax(linear(x, W["model.generator.proj.weight"], W["model.generator.proj.bias"], rnd), -1)


def forward(W, att, masks, seq, N, use_bn, rnd=ident):
    """_forward: log-probs [n, seq.size(1) - 1, V + 1]."""
    memory, kmask = encode(W, att, masks, N, use_bn, rnd)
    tok = seq[:, :-1]
    tmask = (tok > 0)
    tmask[:, 0] = True
    return generator(W, decode(W, rnd(memory), kmask, tok, tmask.to(memory.dtype), N, rnd), rnd)


def step_logprobs(W, memory, kmask, ys, N, rnd=ident):
    """get_logprobs_state: the log-probs after the last token of ys [n, t] (no key mask on the targets, causal only)."""
    return generator(W, decode(W, rnd(memory), kmask, ys, None, N, rnd)[:, -1], rnd)


def sample_greedy(W, att, masks, L, N, use_bn):
    """_sample with sample_max: (seq [n, L], seqLogprobs [n, L], the smallest winner / runner-up gap over the live steps)."""
    memory, kmask = encode(W, att, masks, N, use_bn)
    n = att.shape[0]
    ys = torch.zeros(n, 1, dtype=torch.int64)
    seq = torch.zeros(n, L, dtype=torch.int64)
    lp = torch.zeros(n, L, dtype=memory.dtype)
    unfinished = torch.ones(n, dtype=torch.bool)
    gap = float("inf")
    for t in range(L):
        logp = step_logprobs(W, memory, kmask, ys, N)
        top = logp.topk(2, 1).values
        if unfinished.any():
            gap = min(gap, float((top[:, 0] - top[:, 1])[unfinished].min()))
        best, it = logp.max(1)
        unfinished = unfinished & (it > 0)
        it = it * unfinished.long()
        seq[:, t], lp[:, t] = it, best
        ys = torch.cat([ys, it[:, None]], 1)
        if not unfinished.any():
            break
    return seq, lp, gap


def rescore(W, att, masks, seq, N, use_bn):
    """Teacher-forced log-probs of the decoded tokens, [n, L]: position t scores seq[:, t] given <bos> seq[:, :t].  Valid up to and
    including a row's first 0 (behind it the teacher-forced pass masks keys that incremental decoding does not)."""
    n, L = seq.shape
    full = torch.cat([torch.zeros(n, 1, dtype=torch.int64), seq], 1)           # [n, L + 1]; _forward drops the last column
    logp = forward(W, att, masks, full, N, use_bn)
    return logp.gather(2, seq[:, :, None]).squeeze(2)


def live_positions(seq):
    """[n, L] bool: positions up to and including each row's first 0."""
    ended = torch.cat([torch.zeros(seq.shape[0], 1, dtype=torch.bool), (seq == 0)[:, :-1]], 1)
    return ended.long().cumsum(1) == 0


def beam_search(W, att, masks, L, N, use_bn, beam_size, max_ppl=0):
    """_sample_beam over CaptionModel.beam_search, group_size 1, image by image.  -> (seq [n, L], logps [n, L], done lists, the
    smallest gap between the last accepted and the first rejected candidate over all decisions).  done[k] = [(seq, logps, p)] sorted
    by -p (stable), the first beam_size."""
    memory, kmask = encode(W, att, masks, N, use_bn)
    n, B = att.shape[0], beam_size
    out_seq = torch.zeros(n, L, dtype=torch.int64)
    out_lp = torch.zeros(n, L, dtype=memory.dtype)
    done_all, gap = [], float("inf")
    for k in range(n):
        mem_k, km_k = memory[k:k + 1].expand(B, -1, -1), kmask[k:k + 1].expand(B, -1)
        ys = torch.zeros(B, 1, dtype=torch.int64)
        logp = step_logprobs(W, mem_k, km_k, ys, N)
        beam_seq = torch.zeros(L, B, dtype=torch.int64)
        beam_lp = torch.zeros(L, B, dtype=memory.dtype)
        beam_sum = torch.zeros(B, dtype=memory.dtype)
        done = []
        for t in range(L):
            f = logp.clone()
            f[:, -1] -= 1000
            vals, ix = torch.sort(f, 1, True)
            rows = 1 if t == 0 else B
            cand = [(int(ix[q, c]), q, float(beam_sum[q] + vals[q, c]), vals[q, c]) for c in range(min(B, f.shape[1])) for q in range(rows)]
            cand.sort(key=lambda x: -x[2])
            # the decision of a step: which candidates survive.  (The order AMONG the survivors only breaks exact ties later on.)
            if len(cand) > B and cand[B - 1][2] > -500:      # (finished beams sit at -1000: nothing kept depends on their order)
                gap = min(gap, cand[B - 1][2] - cand[B][2])
            prev_seq, prev_lp, prev_ys = beam_seq[:t].clone(), beam_lp[:t].clone(), ys.clone()
            for vix in range(B):
                c, q, p, r = cand[vix]
                beam_seq[:t, vix], beam_lp[:t, vix] = prev_seq[:, q], prev_lp[:, q]
                ys[vix] = prev_ys[q]
                beam_seq[t, vix], beam_lp[t, vix], beam_sum[vix] = c, r, p
            for vix in range(B):
                if beam_seq[t, vix] == 0 or t == L - 1:
                    p = float(beam_sum[vix])
                    done.append((beam_seq[:, vix].clone(), beam_lp[:, vix].clone(), p / (t + 1) if max_ppl else p))
                    beam_sum[vix] = -1000
            if t + 1 < L:
                ys = torch.cat([ys, beam_seq[t][:, None]], 1)
                logp = step_logprobs(W, mem_k, km_k, ys, N)
        done = sorted(done, key=lambda x: -x[2])
        for a, b in zip(done[:B], done[1:B + 1]):            # the order of the kept list, and its cut
            gap = min(gap, a[2] - b[2])
        done = done[:B]
        done_all.append(done)
        out_seq[k], out_lp[k] = done[0][0], done[0][1]
    return out_seq, out_lp, done_all, gap


# ---------------------------------------------------------------------------------------------------------------- device limits
def d_ff_padded(d_ff):
    """w_2's reduction length in the derived copies: the bf16 GEMM needs K % 8 == 0 and opts.py's default 1300 is no multiple."""
    return (d_ff + 7) // 8 * 8


def mha_supported(Sk, d_k):
    return 1 <= Sk <= 128 and 8 <= d_k <= 128 and d_k % 8 == 0


def mha_lds_bytes(Sk, d_k):
    """K [Sk][d_k + 1] + V [Sk][d_k] + 4 waves x (probabilities [Sk] + query [d_k]), f32."""
    return 4 * (Sk * (d_k + 1) + Sk * d_k + 4 * (Sk + d_k))


LDS_BYTES = 160 * 1024     # per workgroup on gfx950


_real = {}


def real_case():
    """The one case at the real widths (opts.py's defaults, bottom-up features): weights from a seed (they would be ~190 MB as a
    fixture), 8 images x 36 regions x 2048 with ragged masks, captions of up to 16 words.  -> (cfg, W f32, att, masks, labels)."""
    if not _real:
        c = REAL
        W = make_weights(c["V"] + 1, c["D"], c["d_model"], c["d_ff"], c["N"], c["use_bn"], seed=c["seed"])
        g = torch.Generator().manual_seed(c["seed"] + 1)
        att = torch.randn(c["n_img"], c["R"], c["D"], generator=g).abs()          # (ReLU features are non-negative)
        lens = torch.randint(10, c["R"] + 1, (c["n_img"],), generator=g)
        lens[0] = c["R"]
        masks = (torch.arange(c["R"])[None, :] < lens[:, None]).float()
        labels = torch.zeros(c["n_img"], c["L"] + 2, dtype=torch.int64)
        for i in range(c["n_img"]):
            n = int(torch.randint(3, c["L"] + 1, (1,), generator=g))
            labels[i, 1:1 + n] = torch.randint(1, c["V"] + 1, (n,), generator=g)
        _real["case"] = (c, W, att, masks, labels)
    return _real["case"]


def bf16_bounds(name, W64, att, masks, labels, N, use_bn):
    """(log-prob bound, memory bound) of a bf16 run of this case: 4 x the deviation of the bf16-emulating restatement from the plain
    one (float64 inputs), at least TOL_BF16; the deviation must be the one recorded in BF16_EMULATED (within a quarter)."""
    ref = forward(W64, att, masks, labels, N, use_bn)
    emu = forward(W64, att, masks, labels, N, use_bn, rnd=bf16_round)
    dev = (emu - ref).abs().max().item()
    m0, _ = encode(W64, att, masks, N, use_bn)
    m1, _ = encode(W64, att, masks, N, use_bn, rnd=bf16_round)
    mdev = (m1 - m0).abs().max().item()
    want = BF16_EMULATED[name]
    assert abs(dev - want[0]) < 0.25 * want[0], (name, dev, want)
    assert want[1] is None or abs(mdev - want[1]) < 0.25 * want[1], (name, mdev, want)
    return max(TOL_BF16, 4 * dev), max(TOL_BF16, 4 * mdev)
