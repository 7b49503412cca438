"""TransformerModel behind the reference's constructor / call / state_dict contract (P/models/TransformerModel.py), computed
by libuic_hip.so (csrc/transformer.hip) -- evaluation and decoding only; training is not built.

The nn.Module tree below exists only to own parameters (and the `pe` buffer) under the reference's names
(`model.encoder.layers.0.self_attn.linears.0.weight`, `model.tgt_embed.1.pe`, ...), so a checkpoint saved by the reference
loads with a strict `load_state_dict`; none of these sub-modules' `forward` is ever called.  There is no eager fallback:
without the HIP library, or on a CPU tensor, every call raises.
"""
import ctypes as C
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .CaptionModel import CaptionModel
from .. import _lib
from .._lib import check, ptr, stream

_TRAINING = "TransformerModel: evaluation and decoding only; training is not built (call model.eval())"


class LayerNorm(nn.Module):
    def __init__(self, features, eps=1e-6):
        super(LayerNorm, self).__init__()
        self.a_2 = nn.Parameter(torch.ones(features))
        self.b_2 = nn.Parameter(torch.zeros(features))
        self.eps = eps


class SublayerConnection(nn.Module):
    def __init__(self, size):
        super(SublayerConnection, self).__init__()
        self.norm = LayerNorm(size)


class MultiHeadedAttention(nn.Module):
    def __init__(self, h, d_model):
        super(MultiHeadedAttention, self).__init__()
        assert d_model % h == 0
        self.d_k, self.h = d_model // h, h
        self.linears = nn.ModuleList([nn.Linear(d_model, d_model) for _ in range(4)])


class PositionwiseFeedForward(nn.Module):
    def __init__(self, d_model, d_ff):
        super(PositionwiseFeedForward, self).__init__()
        self.w_1 = nn.Linear(d_model, d_ff)
        self.w_2 = nn.Linear(d_ff, d_model)


class EncoderLayer(nn.Module):
    def __init__(self, size, h, d_ff):
        super(EncoderLayer, self).__init__()
        self.self_attn = MultiHeadedAttention(h, size)
        self.feed_forward = PositionwiseFeedForward(size, d_ff)
        self.sublayer = nn.ModuleList([SublayerConnection(size) for _ in range(2)])
        self.size = size


class DecoderLayer(nn.Module):
    def __init__(self, size, h, d_ff):
        super(DecoderLayer, self).__init__()
        self.size = size
        self.self_attn = MultiHeadedAttention(h, size)
        self.src_attn = MultiHeadedAttention(h, size)
        self.feed_forward = PositionwiseFeedForward(size, d_ff)
        self.sublayer = nn.ModuleList([SublayerConnection(size) for _ in range(3)])


class _Stack(nn.Module):
    def __init__(self, layers, size):
        super(_Stack, self).__init__()
        self.layers = nn.ModuleList(layers)
        self.norm = LayerNorm(size)


class Embeddings(nn.Module):
    def __init__(self, d_model, vocab):
        super(Embeddings, self).__init__()
        self.lut = nn.Embedding(vocab, d_model)
        self.d_model = d_model


class PositionalEncoding(nn.Module):
    def __init__(self, d_model, max_len=5000):
        super(PositionalEncoding, self).__init__()
        pe = torch.zeros(max_len, d_model)
        position = torch.arange(0, max_len).unsqueeze(1).float()
        div_term = torch.exp(torch.arange(0, d_model, 2).float() * -(math.log(10000.0) / d_model))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.register_buffer('pe', pe.unsqueeze(0))


class Generator(nn.Module):
    def __init__(self, d_model, vocab):
        super(Generator, self).__init__()
        self.proj = nn.Linear(d_model, vocab)


class EncoderDecoder(nn.Module):
    def __init__(self, encoder, decoder, tgt_embed, generator):
        super(EncoderDecoder, self).__init__()
        self.encoder = encoder
        self.decoder = decoder
        self.tgt_embed = tgt_embed
        self.generator = generator


class TransformerModel(CaptionModel):
    H = _lib.TRANSFORMER_HEADS
    eval_only = True        # Trainer refuses to build a training run around it

    def make_model(self, tgt_vocab, N=6, d_model=512, d_ff=2048):
        """P/models/TransformerModel.py:272-292 (the source embedding is the identity there)."""
        h = self.H
        model = EncoderDecoder(
            _Stack([EncoderLayer(d_model, h, d_ff) for _ in range(N)], d_model),
            _Stack([DecoderLayer(d_model, h, d_ff) for _ in range(N)], d_model),
            nn.Sequential(Embeddings(d_model, tgt_vocab), PositionalEncoding(d_model)),
            Generator(d_model, tgt_vocab))
        for p in model.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        return model

    def __init__(self, opt):
        super(TransformerModel, self).__init__()
        self.opt = opt
        self.vocab_size = opt.vocab_size
        self.input_encoding_size = opt.input_encoding_size
        self.rnn_size = opt.rnn_size
        self.num_layers = opt.num_layers
        self.drop_prob_lm = opt.drop_prob_lm
        self.seq_length = opt.seq_length
        self.att_feat_size = opt.att_feat_size
        self.use_bn = getattr(opt, 'use_bn', 0)
        self.ss_prob = 0.0
        if self.use_bn not in (0, 1, 2):
            raise ValueError("use_bn=%r must be 0, 1 or 2" % (self.use_bn,))
        if not 1 <= self.num_layers <= _lib.TRANSFORMER_MAX_LAYERS:
            raise NotImplementedError("num_layers=%r: the MI355X path supports 1..%d" % (self.num_layers, _lib.TRANSFORMER_MAX_LAYERS))
        d_model = self.input_encoding_size
        if d_model % (8 * self.H) or not 8 * self.H <= d_model <= min(_lib.LAYERNORM_MAX_D, self.H * _lib.MHA_MAX_DK):
            raise NotImplementedError("input_encoding_size=%r is not supported by the MI355X transformer path: d_model must be a multiple of "
                                      "%d in [%d, %d] (h = %d heads, d_k a multiple of 8 up to %d)"
                                      % (d_model, 8 * self.H, 8 * self.H, min(_lib.LAYERNORM_MAX_D, self.H * _lib.MHA_MAX_DK),
                                                     self.H, _lib.MHA_MAX_DK))
        if self.seq_length + 1 > _lib.MHA_MAX_SK:
            raise NotImplementedError("seq_length=%r: at most %d target positions" % (self.seq_length, _lib.MHA_MAX_SK - 1))
        self.att_embed = nn.Sequential(*(
            ((nn.BatchNorm1d(self.att_feat_size),) if self.use_bn else ()) +
            (nn.Linear(self.att_feat_size, self.input_encoding_size),
             nn.ReLU(),
             nn.Dropout(self.drop_prob_lm)) +
            ((nn.BatchNorm1d(self.input_encoding_size),) if self.use_bn == 2 else ())))
        self.model = self.make_model(self.vocab_size + 1, N=self.num_layers, d_model=d_model, d_ff=self.rnn_size)

        # MI355X engine state (not part of the checkpoint)
        self.compute_dtype = getattr(opt, 'compute_dtype', 'bf16')
        self._derived = None
        self._derived_key = None
        self._ws = None
        self._padded = self._padded_key = None
        self._seed_counter = int(getattr(opt, 'seed', 0) or 0) & 0x7FFFFFFF

    # ------------------------------------------------------------------ engine plumbing
    def next_seed(self):
        self._seed_counter = (self._seed_counter * 1103515245 + 12345) & 0x7FFFFFFF
        return self._seed_counter

    def _dims(self, N, R, beam=1):
        return _lib.TransformerDims(N=N, R=R, D=self._D8, d_model=self.input_encoding_size, d_ff=self.rnn_size, layers=self.num_layers,
                                    V1=self.vocab_size + 1, T=self.seq_length + 1, beam=beam, dtype=_lib.dtype_id(self.compute_dtype),
                                    use_bn=self.use_bn)

    @property
    def _D8(self):
        """att_feat_size rounded up to a multiple of 8 (2053 with the reference's default use_box = 1): the library's GEMM operands are
        read in 16-byte pieces, so the features and att_embed's input side are zero-padded up to it."""
        return (self.att_feat_size + 7) // 8 * 8

    def _tensors(self):
        sd = dict(self.named_parameters())
        sd.update(dict(self.named_buffers()))
        t = {k: sd[k].detach() for _, _, _, k in _lib.transformer_weight_keys(self.num_layers, self.use_bn)}
        extra = self._D8 - self.att_feat_size
        if extra:
            # zero columns on the Linear; on BatchNorm1d(D) the identity (gamma 1, beta 0, mean 0, var 1) over zero features: nothing added
            lin = "att_embed.%d.weight" % (1 if self.use_bn else 0)
            fills = {lin: 0.0}
            if self.use_bn:
                fills.update({"att_embed.0.weight": 1.0, "att_embed.0.bias": 0.0, "att_embed.0.running_mean": 0.0, "att_embed.0.running_var": 1.0})
            key = tuple((t[k].data_ptr(), t[k]._version) for k in fills)
            if self._padded_key != key:       # (kept: the derived copies are refreshed when a tensor's address or version changes)
                self._padded = {k: F.pad(t[k], (0, extra), value=v).contiguous() for k, v in fills.items()}
                self._padded_key = key
            t.update(self._padded)
        return t

    def _prepare(self, att_feats, att_masks, beam=1):
        """(lib, dims, weights, derived, workspace, att, masks) for one call: the region axis clipped (clip_att, :347-353), the
        derived weight copies refreshed if a master changed, a workspace of the call's size."""
        if self.training:
            raise NotImplementedError(_TRAINING)
        lib = _lib.load()
        if att_masks is not None:
            max_len = int(att_masks.long().sum(1).max())
            att_feats, att_masks = att_feats[:, :max_len], att_masks[:, :max_len]
        if att_feats.shape[-1] != self.att_feat_size:
            raise ValueError("att_feats have %d columns, opt.att_feat_size is %d" % (att_feats.shape[-1], self.att_feat_size))
        att = F.pad(att_feats.float(), (0, self._D8 - self.att_feat_size)).contiguous()
        am = att_masks.contiguous().float() if att_masks is not None else None
        if not att.is_cuda:
            raise RuntimeError("TransformerModel needs device tensors; got a %s tensor (there is no CPU fallback)" % att.device)
        N, R = att.shape[0], att.shape[1]
        if not 1 <= R <= _lib.MHA_MAX_SK:
            raise NotImplementedError("%d regions per image: uic_mha_fwd keeps a head's keys in LDS, 1..%d" % (R, _lib.MHA_MAX_SK))
        d = self._dims(N, R, beam)
        tensors = self._tensors()
        w = _lib.transformer_weights(tensors, self.num_layers, self.use_bn)
        key = (d.dtype, str(att.device)) + tuple((t.data_ptr(), t._version) for t in tensors.values())
        if self._derived_key != key:
            nbytes = lib.uic_transformer_derived_bytes(C.byref(d))
            if nbytes == 0:
                check(-1, "transformer_derived_bytes")
            self._derived = torch.empty(nbytes, dtype=torch.uint8, device=att.device)
            check(lib.uic_transformer_refresh_weights(C.byref(d), C.byref(w), ptr(self._derived), stream()), "transformer_refresh_weights")
            self._derived_key = key
        nbytes = lib.uic_transformer_workspace_bytes(C.byref(d))
        if nbytes == 0:
            check(-1, "transformer_workspace_bytes")
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != att.device:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=att.device)
        return lib, d, w, self._derived, self._ws, att, am

    # ------------------------------------------------------------------ reference call surface
    def encode(self, att_feats, att_masks=None):
        """model.encode over _prepare_feature's source side: the memory [N, R', d_model] f32 (R' = the longest row of att_masks)."""
        with torch.no_grad():
            lib, d, w, dv, ws, att, am = self._prepare(att_feats, att_masks)
            mem = torch.empty(d.N, d.R, d.d_model, dtype=torch.float32, device=att.device)
            check(lib.uic_transformer_encode(C.byref(d), C.byref(w), ptr(dv), ptr(att), ptr(am), ptr(ws), ptr(mem), stream()), "transformer_encode")
        return mem

    def _forward(self, fc_feats, attri_feats, att_feats, seq, att_masks=None):
        """P/models/TransformerModel.py:390-428: log-probs [N, seq.size(1) - 1, V + 1]."""
        with torch.no_grad():
            if att_feats is not None and seq is not None and seq.shape[0] != att_feats.shape[0]:
                # features once per image, seq_per_img caption rows per image (the loader's validation batches): one row per caption
                S = seq.shape[0] // att_feats.shape[0]
                att_feats = att_feats.repeat_interleave(S, 0)
                att_masks = att_masks.repeat_interleave(S, 0) if att_masks is not None else None
            lib, d, w, dv, ws, att, am = self._prepare(att_feats, att_masks)
            seq = seq.contiguous().long()
            Tq = seq.shape[1] - 1
            if not 1 <= Tq <= d.T:
                raise ValueError("seq has %d columns; the model decodes 1..%d positions (seq_length + 1)" % (seq.shape[1], d.T))
            logp = torch.empty(d.N, Tq, d.V1, dtype=torch.float32, device=att.device)
            check(lib.uic_transformer_forward(C.byref(d), C.byref(w), ptr(dv), ptr(att), ptr(am), ptr(seq), seq.shape[1], Tq, ptr(ws), ptr(logp),
                                              stream()), "transformer_forward")
        return logp

    def _sample_beam(self, fc_feats, attri_feats, att_feats, att_masks=None, opt={}):
        """P/models/TransformerModel.py:444-475 over CaptionModel.beam_search, all images in one device pass.  `self.done_beams[k]`
        is the reference's list for image k (CaptionModel.done_beams)."""
        beam_size = self._effective_beam_size(opt)
        assert beam_size <= self.vocab_size + 1
        with torch.no_grad():
            lib, d, w, dv, ws, att, am = self._prepare(att_feats, att_masks, beam=int(beam_size))
            L, n_img = self.seq_length, d.N
            seq = torch.zeros(n_img, L, dtype=torch.int64, device=att.device)
            lp = torch.zeros(n_img, L, dtype=torch.float32, device=att.device)
            check(lib.uic_transformer_sample_beam(C.byref(d), C.byref(w), ptr(dv), ptr(att), ptr(am), L, int(beam_size),
                                                  int(opt.get('decoding_constraint', 0)), int(opt.get('max_ppl', 0)), ptr(ws), ptr(seq), ptr(lp),
                                                  stream()), "transformer_sample_beam")
            lists = _lib.done_list_buffers(n_img, L, int(beam_size), att.device)
            check(lib.uic_transformer_beam_done_lists(C.byref(d), ptr(ws), L, int(beam_size), *[ptr(x) for x in lists], stream()),
                  "transformer_beam_done_lists")
        self._set_done_raw(*lists, int(beam_size))
        return seq, lp

    def _sample(self, fc_feats, attri_feats, att_feats, att_masks=None, opt={}):
        """P/models/TransformerModel.py:520-576: (seq, seqLogprobs), both [N, seq_length]."""
        if self.training:
            raise NotImplementedError(_TRAINING)
        sample_max = opt.get('sample_max', 1)
        beam_size = opt.get('beam_size', 1)
        temperature = opt.get('temperature', 1.0)
        if opt.get('decoding_constraint', 0):
            # P/models/TransformerModel.py:543-546 builds the penalty from `output`, a name the method never defines: the reference
            # raises NameError at the second step.  There is no behaviour to reproduce.
            raise NotImplementedError("TransformerModel._sample: decoding_constraint refers to an undefined name in the reference "
                                      "(`output`, P/models/TransformerModel.py:544) and cannot run there; not provided")
        if beam_size > 1:
            return self._sample_beam(fc_feats, attri_feats, att_feats, att_masks, opt)
        with torch.no_grad():
            lib, d, w, dv, ws, att, am = self._prepare(att_feats, att_masks)
            L = self.seq_length
            seq = torch.zeros(d.N, L, dtype=torch.int64, device=att.device)
            lp = torch.zeros(d.N, L, dtype=torch.float32, device=att.device)
            check(lib.uic_transformer_sample(C.byref(d), C.byref(w), ptr(dv), ptr(att), ptr(am), L, int(bool(sample_max)), float(temperature),
                                             self.next_seed(), ptr(ws), ptr(seq), ptr(lp), stream()), "transformer_sample")
        return seq, lp
