"""The rules of the pivot bridge restated in plain Python, and the cases the CPU and GPU tests share.

    restated_source / restated_target   the two kernels of csrc/pivot.hip (include/uic_hip.h: uic_pivot_source, uic_pivot_target)
    restated_tables                     misc.pivot.build_tables
    convert_to_idx / build_target_tokens   onmt.Dict.convertToIdx and NMTModel.buildTargetTokens on words, as the reference writes
                                        them (checked against the reference's own output in tests/golden/pivot_dict.json)

Nothing here imports the package: the restatement is written from the contract, not from the implementation."""
import numpy as np

PAD, UNK, BOS, EOS = 0, 1, 2, 3
PAD_WORD, UNK_WORD, BOS_WORD, EOS_WORD = '<blank>', '<unk>', '<s>', '</s>'
SPECIALS = [PAD_WORD, UNK_WORD, BOS_WORD, EOS_WORD]

# launch geometry: uic_pivot_source runs 64 captions per workgroup (one per lane), uic_pivot_target one 64-lane workgroup per
# sentence whose lanes stride over the columns -- so the batch sizes cross 64 and the widths cross 64 columns
WAVE = 64
BATCHES = (1, 2, 63, 64, 65, 130)
POISON = -77


# ------------------------------------------------------------------ the kernels
def restated_source(seq, L, table):
    """seq [B, ld >= L] ints, table [V1] -> (src [L, B] int64, lengths [B] int32, max_len)."""
    B, V1 = len(seq), len(table)
    src = np.zeros((L, B), dtype=np.int64)
    lengths = np.zeros(B, dtype=np.int32)
    for b in range(B):
        n = 0
        for t in range(L):
            tok = int(seq[b][t])
            if tok <= 0:
                break
            src[t, b] = int(table[tok]) if tok < V1 else UNK
            n = t + 1
        if n == 0:
            src[0, b] = UNK
            n = 1
        lengths[b] = n
    return src, lengths, int(lengths.max()) if B else 0


def restated_target(hyp, n_steps, attn, src_len, seq, tgt_table, copy_table, L_out):
    """-> (out [B, L_out] int64, out_len [B] int32, repl [B, L_out] int32)."""
    B, Vt, V1 = len(hyp), len(tgt_table), len(copy_table)
    out = np.zeros((B, L_out), dtype=np.int64)
    repl = np.full((B, L_out), -1, dtype=np.int32)
    out_len = np.zeros(B, dtype=np.int32)
    for b in range(B):
        row = [int(t) for t in hyp[b][:n_steps]]
        toks = row[:row.index(EOS)] if EOS in row else row[:n_steps - 1]
        toks = toks[:L_out]
        out_len[b] = len(toks)
        for i, tok in enumerate(toks):
            if tok == UNK:
                a = [float(x) for x in attn[b][i][:int(src_len[b])]]
                j = a.index(max(a))                          # the lowest index among equals
                c = int(seq[b][j])
                out[b, i] = int(copy_table[c if 0 <= c < V1 else 0])
                repl[b, i] = j
            elif 0 <= tok < Vt:
                out[b, i] = int(tgt_table[tok])
            else:
                out[b, i] = int(tgt_table[UNK])
    return out, out_len, repl


# ------------------------------------------------------------------ the host side
def make_dict(words, lower=False):
    """An onmt.Dict restated: the four specials first, then `words`; returns (labelToIdx, idxToLabel, lower)."""
    label_to_idx, idx_to_label = {}, {}
    for w in SPECIALS + list(words):
        w = w.lower() if lower else w
        if w not in label_to_idx:
            label_to_idx[w] = len(idx_to_label)
            idx_to_label[label_to_idx[w]] = w
    return label_to_idx, idx_to_label, lower


class DictLike(object):
    """The four attributes misc.pivot reads from an onmt.Dict."""

    def __init__(self, words, lower=False):
        self.labelToIdx, self.idxToLabel, self.lower = make_dict(words, lower)

    def size(self):
        return len(self.idxToLabel)


def convert_to_idx(label_to_idx, lower, words):
    """Dict.convertToIdx(words, UNK_WORD): no BOS, no EOS."""
    return [label_to_idx.get(w.lower() if lower else w, label_to_idx[UNK_WORD]) for w in words]


def convert_to_labels(idx_to_label, ids, stop):
    out = []
    for i in ids:
        out.append(idx_to_label.get(int(i)))
        if i == stop:
            break
    return out


def build_target_tokens(idx_to_label, pred, src_words, attn):
    """NMTModel.buildTargetTokens: attn [len(pred), len(src_words)]."""
    tokens = convert_to_labels(idx_to_label, pred, EOS)[:-1]
    for i in range(len(tokens)):
        if tokens[i] == UNK_WORD:
            a = [float(x) for x in attn[i]]
            tokens[i] = src_words[a.index(max(a))]
    return tokens


def restated_tables(caption_vocab, src, tgt, scoring_vocab):
    """caption_vocab / scoring_vocab: ix_to_word {'1': word, ..}; src / tgt: (labelToIdx, idxToLabel, lower).
    -> (src_table, tgt_table, copy_table, oov)."""
    V1 = max(int(k) for k in caption_vocab) + 1
    oov = len(scoring_vocab) + 1
    score = {}
    for k in sorted(scoring_vocab, key=int):
        score.setdefault(scoring_vocab[k], int(k))
    src_table, copy_table = [UNK] * V1, [oov] * V1
    for k, w in caption_vocab.items():
        src_table[int(k)] = convert_to_idx(src[0], src[2], [w])[0]
        copy_table[int(k)] = score.get(w, oov)
    tgt_table = [oov] * len(tgt[1])
    for i, w in tgt[1].items():
        if i >= len(SPECIALS):
            tgt_table[i] = score.get(w, oov)
    return (np.array(src_table, dtype=np.int32), np.array(tgt_table, dtype=np.int32), np.array(copy_table, dtype=np.int32), oov)


# ------------------------------------------------------------------ cases of uic_pivot_source
def source_case(B, L, V1=23, pad_cols=3, seed=0):
    """seq [B, L + pad_cols] whose first rows are the named edge rows (cycled through the batch), the rest random; the
    columns behind L hold live tokens that must not be read as part of the caption."""
    g = np.random.default_rng(1000 * B + 10 * L + seed)
    seq = g.integers(1, V1, size=(B, L + pad_cols)).astype(np.int64)         # full length, no terminator
    for b in range(B):
        kind = b % 7
        if kind == 0:
            seq[b, :L] = 0                                                   # empty
        elif kind == 1:
            pass                                                             # full length with no terminator
        elif kind == 2:
            seq[b, L // 2:L] = -1                                            # ended by -1 (a timed-out decode)
        elif kind == 3:
            seq[b, 0] = V1 - 1                                               # the last table entry
        elif kind == 4:
            seq[b, min(1, L - 1)] = V1 + int(g.integers(0, 5))               # an id >= V1
            seq[b, 0] = 2 ** 40
        elif kind == 5:
            seq[b, int(g.integers(0, L)):L] = 0                              # a random end, live tokens behind a 0 ...
            if L > 2:
                seq[b, L - 1] = 5                                            # ... that are not part of the caption
    table = g.permutation(np.arange(4, 4 + V1)).astype(np.int32)
    table[::5] = UNK                                                         # words the source dictionary lacks
    return seq, table


# ------------------------------------------------------------------ cases of uic_pivot_target
def target_case(B, n_steps, ld_hyp=None, S=9, L=12, Vt=31, V1=23, L_out=None, seed=0):
    """Hypotheses / attention with the named edge rows cycled through the batch."""
    g = np.random.default_rng(7000 * B + 13 * n_steps + seed)
    ld_hyp = max(n_steps, 1) + 2 if ld_hyp is None else ld_hyp
    L_out = max(n_steps, 1) if L_out is None else L_out
    hyp = g.integers(4, Vt, size=(B, ld_hyp)).astype(np.int64)
    hyp[:, n_steps:] = EOS                                                   # an EOS behind the valid columns is not one
    attn = g.random((B, ld_hyp, S)).astype(np.float32)
    src_len = g.integers(1, min(S, L) + 1, size=B).astype(np.int32)
    seq = g.integers(1, V1, size=(B, L)).astype(np.int64)
    for b in range(B):
        kind = b % 9
        sl = int(src_len[b])
        attn[b, :, sl:] = 2.0                                                # larger values behind src_len: ignored
        if kind == 0:
            hyp[b, 0] = EOS                                                  # EOS first: no tokens
        elif kind == 1:
            hyp[b, n_steps - 1] = EOS                                        # EOS at the last column
        elif kind == 2:
            pass                                                             # no EOS: the last token is dropped
        elif kind == 3:
            hyp[b, 0] = UNK                                                  # UNK, attention tie: the lowest index
            attn[b, 0, :sl] = 0.5
        elif kind == 4:
            hyp[b, 0] = UNK                                                  # UNK, the maximum on the last valid column
            attn[b, 0, :sl] = 0.1
            attn[b, 0, sl - 1] = 0.9
        elif kind == 5:
            hyp[b, 0] = Vt + int(g.integers(0, 3))                           # a token >= Vt
            if n_steps > 1:
                hyp[b, 1] = -5
        elif kind == 6:
            hyp[b, :n_steps] = UNK                                           # every token replaced
            seq[b, 0] = V1 + 3                                               # ... one of them by a pivot token outside the table
        elif kind == 7:
            hyp[b, n_steps // 2] = EOS
            hyp[b, 0] = BOS                                                  # a special inside the hypothesis
    tgt_table = g.integers(1, 40, size=Vt).astype(np.int32)
    copy_table = g.integers(40, 80, size=V1).astype(np.int32)
    return dict(hyp=hyp, n_steps=n_steps, attn=attn, src_len=src_len, seq=seq, tgt_table=tgt_table, copy_table=copy_table, L_out=L_out)


# ------------------------------------------------------------------ the dictionaries of the end-to-end tests
def word_list(prefix, n):
    return ['%s%d' % (prefix, i) for i in range(n)]
