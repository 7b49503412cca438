"""The pivot bridge of the unpaired validation chain (P/eval_utils.py:329-473): image -> pivot-language captioner ->
zh->en translator -> English caption scored against the COCO references, with every stage on the MI355X.

The reference joins the stages with strings: utils.decode_sequence, str.split, onmt.Dict.convertToIdx, NMTModel.translate,
buildTargetTokens, ' '.join, and a json file for the scorers.  Here the joins are two gather kernels on token ids
(csrc/pivot.hip: uic_pivot_source, uic_pivot_target) and the word <-> id work is done ONCE, on the host, as three int32 tables:

    src_table  [V1]  caption id -> source-dictionary id       (a word the dictionary lacks: UNK)
    tgt_table  [Vt]  target-dictionary id -> scoring id       (a word the scored vocabulary lacks, and every special: OOV)
    copy_table [V1]  caption id -> scoring id                 (the pivot word copied in place of an UNK, P/models/NMT_Models.py:316-318)

OOV = len(scoring_vocab) + 1: no reference row can hold that id, so such a word never matches -- as a string outside the
references' vocabulary never does.  `caption_vocab` / `scoring_vocab` are the loaders' ix_to_word ({'1': word, ..}, 0 = end).

Deviations from the reference: an empty pivot caption is translated as the one-token sentence [UNK] (the reference crashes on an
empty source line), and the batch is not sorted by length (onmt.Dataset sorts for packing only; translateBatch does not pack).
"""
import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr, stream

PAD, UNK, BOS, EOS = 0, 1, 2, 3           # onmt.Constants
N_SPECIAL = 4
MAX_WORDS = 64                            # the scorers' row width (csrc/cider.hip)


class _Dict(object):
    """An onmt.Dict-like object (labelToIdx, idxToLabel, lower, size()) or a plain mapping, word -> id or id -> word."""

    def __init__(self, d):
        if hasattr(d, 'labelToIdx') and hasattr(d, 'idxToLabel'):
            self.label_to_idx, self.idx_to_label = dict(d.labelToIdx), dict(d.idxToLabel)
            self.lower = bool(getattr(d, 'lower', False))
            self.n = int(d.size()) if hasattr(d, 'size') else len(self.idx_to_label)
        elif hasattr(d, 'items'):
            items = list(d.items())
            if items and isinstance(items[0][1], str):               # id -> word
                self.idx_to_label = {int(k): v for k, v in items}
                self.label_to_idx = {v: k for k, v in self.idx_to_label.items()}
            else:
                self.label_to_idx = {k: int(v) for k, v in items}
                self.idx_to_label = {v: k for k, v in self.label_to_idx.items()}
            self.lower = False
            self.n = (max(self.idx_to_label) + 1) if self.idx_to_label else 0
        else:
            raise TypeError("a dictionary is an onmt.Dict-like object (labelToIdx, idxToLabel, lower, size()) or a mapping; got %r" % type(d))

    def lookup(self, word, default=None):
        """onmt.Dict.lookup (O/Dict.py:42-47)."""
        return self.label_to_idx.get(word.lower() if self.lower else word, default)

    def label(self, idx, default=None):
        return self.idx_to_label.get(int(idx), default)


def as_dict(d):
    return d if isinstance(d, _Dict) else _Dict(d)


def _vocab_words(ix_to_word):
    """ix_to_word ({'1': word, ..}) -> list indexed by id; entry 0 (the end token) and gaps are None."""
    ids = {int(k): v for k, v in ix_to_word.items()}
    words = [None] * (max(ids) + 1 if ids else 1)
    for k, v in ids.items():
        if k >= 1:
            words[k] = v
    return words


def build_tables(caption_vocab, src_dict, tgt_dict, scoring_vocab):
    """(src_table [V1], tgt_table [Vt], copy_table [V1]) as int32 numpy arrays, and the OOV scoring id."""
    src, tgt = as_dict(src_dict), as_dict(tgt_dict)
    cap = _vocab_words(caption_vocab)
    score_id = {}
    for k, w in scoring_vocab.items():
        score_id.setdefault(w, int(k))
    oov = len(scoring_vocab) + 1
    unk = UNK
    src_table = np.full(len(cap), unk, dtype=np.int32)
    copy_table = np.full(len(cap), oov, dtype=np.int32)
    for i, w in enumerate(cap):
        if w is None:
            continue
        src_table[i] = src.lookup(w, unk)                            # convertToIdx(words, UNK_WORD)
        copy_table[i] = score_id.get(w, oov)
    tgt_table = np.full(max(tgt.n, 2), oov, dtype=np.int32)
    for i in range(N_SPECIAL, tgt.n):
        w = tgt.label(i)
        if w is not None:
            tgt_table[i] = score_id.get(w, oov)
    return src_table, tgt_table, copy_table, oov


class PivotBridge(object):
    """The three tables on the device and the calls around them.  Built once per (captioner, translator, scored data set)."""

    def __init__(self, caption_vocab, src_dict, tgt_dict, scoring_vocab, device="cuda", max_words=MAX_WORDS):
        self.caption_vocab, self.scoring_vocab = caption_vocab, scoring_vocab
        self.src_dict, self.tgt_dict = as_dict(src_dict), as_dict(tgt_dict)
        self.host_tables = build_tables(caption_vocab, self.src_dict, self.tgt_dict, scoring_vocab)
        self.oov = self.host_tables[3]
        self.device = torch.device(device)
        self.max_words = int(max_words)
        self._tables = None
        self.last = None

    @property
    def tables(self):
        if self._tables is None:                                     # the one upload
            self._tables = tuple(torch.from_numpy(t).to(self.device) for t in self.host_tables[:3])
        return self._tables

    def to_source(self, seq):
        """seq [B, L] int64 device rows of the captioner -> (src [max_len, B] int64, lengths [B] int32): uic_pivot_source and
        the one read-back of max_len."""
        lib = _lib.load()
        seq = seq.contiguous()
        B, L = seq.shape
        src_table = self.tables[0]
        src = torch.empty(L, B, dtype=torch.int64, device=seq.device)
        lengths = torch.empty(B, dtype=torch.int32, device=seq.device)
        max_len = torch.empty(1, dtype=torch.int32, device=seq.device)
        check(lib.uic_pivot_source(ptr(seq), L, B, L, ptr(src_table), src_table.numel(), ptr(src), ptr(lengths), ptr(max_len),
                                   stream()), "pivot_source")
        n = int(max_len.item()) if B else 0
        return src[:n], lengths

    def to_target(self, hyp, n, attn, src_len, seq, max_words=None):
        """uic_pivot_target: (out [B, L_out] int64 scoring ids, out_len [B] int32, repl [B, L_out] int32).  hyp [B, ld], attn
        [B, ld, S] and n as NMTModel.translate_device returns them."""
        lib = _lib.load()
        _, tgt_table, copy_table = self.tables
        hyp, attn, seq, src_len = hyp.contiguous(), attn.contiguous(), seq.contiguous(), src_len.contiguous()
        B = hyp.shape[0]
        L_out = int(self.max_words if max_words is None else max_words)
        out = torch.empty(B, L_out, dtype=torch.int64, device=hyp.device)
        out_len = torch.empty(B, dtype=torch.int32, device=hyp.device)
        repl = torch.empty(B, L_out, dtype=torch.int32, device=hyp.device)
        check(lib.uic_pivot_target(ptr(hyp), hyp.shape[1], int(n), ptr(attn), attn.shape[1], attn.shape[2], ptr(src_len), ptr(seq),
                                   seq.shape[1], B, ptr(tgt_table), tgt_table.numel(), ptr(copy_table), copy_table.numel(), L_out,
                                   ptr(out), ptr(out_len), ptr(repl), stream()), "pivot_target")
        return out, out_len, repl

    def pivot(self, seq, nmt_model, beam_size=15, max_steps=100):
        """The whole chain on the device: caption rows -> (out [B, max_words] scoring ids, out_len [B], scores [B]).  The host
        waits for max_len and for the translator's own stop checks, nothing else.  `self.last` keeps the device tensors a
        caller needs to render words (render())."""
        seq = seq.contiguous()
        src, lengths = self.to_source(seq)
        hyp, scores, attn, n = nmt_model.translate_device(src, beam_size=beam_size, max_steps=max_steps)
        out, out_len, repl = self.to_target(hyp, n, attn, lengths, seq)
        self.last = dict(seq=seq, src=src, lengths=lengths, hyp=hyp, attn=attn, n=n, out_len=out_len, repl=repl)
        return out, out_len, scores

    def render(self, hyp, out_len, repl, seq):
        """Word strings of translated rows (host tensors / arrays): the target dictionary's word of every kept token, the pivot
        caption's own word at a replaced position."""
        hyp, out_len, repl, seq = (np.asarray(x.cpu() if torch.is_tensor(x) else x) for x in (hyp, out_len, repl, seq))
        sents = []
        for b in range(len(hyp)):
            words = []
            for i in range(int(out_len[b])):
                if repl[b, i] >= 0:
                    c = int(seq[b, repl[b, i]])
                    words.append(self.caption_vocab.get(str(c), self.tgt_dict.label(UNK, '<unk>')))
                else:
                    words.append(str(self.tgt_dict.label(int(hyp[b, i]), self.tgt_dict.label(UNK, '<unk>'))))
            sents.append(' '.join(words))
        return sents
