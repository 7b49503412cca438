"""Language evaluation of a validation pass on the MI355X: the `lang_stats` of eval_utils.language_eval (P/eval_utils.py:26-86,
'zh' branch) -- Bleu_1..4, ROUGE_L, CIDEr of AI_Challenger/Evaluation/caption_eval/coco_caption/pycxevalcap/eval.py -- scored on
the device (csrc/cider.hip: uic_langeval_bleu / uic_langeval_rouge_l / uic_langeval_cider / uic_langeval_reduce), so that the
decoded captions of the split never visit the host before the six numbers do.

The scorers run on TOKEN IDS.  A caption's words are its tokens before the first 0 (utils.decode_sequence); a row that begins
with 0 is the empty caption.  References are the label rows of the image, read the same way.  The result equals the reference's
Bleu(4), Rouge() and Cider() applied to strings of ids (tests/golden/lang_eval_*.npz); it is NOT the Java pipeline's result where
the annotation file holds words outside the vocabulary or where the PTB tokenizer would change the text.
"""
import ctypes as C
import math

import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr, stream
from .rewards import SIGMA

KEYS = ('Bleu_1', 'Bleu_2', 'Bleu_3', 'Bleu_4', 'ROUGE_L', 'CIDEr')
BETA2 = 1.2 ** 2          # Rouge.beta ** 2, rouge.py:43,69


def word_counts(rows):
    """Words per row: tokens before the first 0."""
    rows = np.asarray(rows)
    zero = rows == 0
    return np.where(zero.any(1), zero.argmax(1), rows.shape[1])


def document_frequency(rows, start):
    """CiderScorer.compute_doc_freq (cider_scorer.py:93-104) over label rows, vectorised: one document per image = its
    reference set.  rows [R, Lr] integers, start [n_img + 1].  Returns (keys [n, 4] int32, unused positions -1; counts [n] f64 =
    the number of images whose references hold the n-gram), keys in ascending order."""
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    start = np.asarray(start, dtype=np.int64)
    R, Lr = rows.shape
    W = word_counts(rows)
    img = np.repeat(np.arange(len(start) - 1, dtype=np.int64), np.diff(start))
    keys, imgs = [], []
    for k in range(1, min(4, Lr) + 1):
        win = np.lib.stride_tricks.sliding_window_view(rows, k, axis=1)            # [R, Lr - k + 1, k]
        valid = np.arange(Lr - k + 1)[None, :] + k <= W[:, None]
        g = win[valid]
        key = np.full((len(g), 4), -1, dtype=np.int64)
        key[:, :k] = g
        keys.append(key)
        imgs.append(np.broadcast_to(img[:, None], valid.shape)[valid])
    keys, imgs = np.concatenate(keys, 0), np.concatenate(imgs, 0)
    if len(keys) == 0:
        return np.zeros((0, 4), dtype=np.int32), np.zeros(0, dtype=np.float64)
    if keys.max() < 0xFFFF:
        # four tokens in one 64-bit word (token + 1 per 16-bit field, 0 = unused): one sort of (n-gram, image) pairs
        packed = ((keys[:, 0] + 1).astype(np.uint64) << np.uint64(48)) | ((keys[:, 1] + 1).astype(np.uint64) << np.uint64(32)) | \
                 ((keys[:, 2] + 1).astype(np.uint64) << np.uint64(16)) | (keys[:, 3] + 1).astype(np.uint64)
        order = np.lexsort((imgs, packed))
        packed, imgs = packed[order], imgs[order]
        new_key = np.ones(len(packed), dtype=bool)
        new_key[1:] = packed[1:] != packed[:-1]
        new_pair = new_key.copy()
        new_pair[1:] |= imgs[1:] != imgs[:-1]
        group = np.cumsum(new_key) - 1
        counts = np.bincount(group[new_pair], minlength=int(group[-1]) + 1).astype(np.float64)
        uniq = keys[order][new_key]
    else:
        pairs = np.unique(np.concatenate([keys, imgs[:, None]], 1), axis=0)
        uniq, counts = np.unique(pairs[:, :4], axis=0, return_counts=True)
        counts = counts.astype(np.float64)
    return np.ascontiguousarray(uniq, dtype=np.int32), counts


def corpus_bleu(totals):
    """Corpus Bleu_1..4 from the ten integer totals (correct[0..3], guess[0..3], testlen, reflen): the expression of
    BleuScorer.compute_score, bleu_scorer.py:247-256, on python ints."""
    t = [int(x) for x in totals]
    correct, guess, testlen, reflen = t[0:4], t[4:8], t[8], t[9]
    small, tiny = 1e-9, 1e-15
    bleus = []
    bleu = 1.
    for k in range(4):
        bleu *= float(correct[k] + tiny) / (guess[k] + small)
        bleus.append(bleu ** (1. / (k + 1)))
    ratio = (testlen + tiny) / (reflen + small)
    if ratio < 1:
        for k in range(4):
            bleus[k] *= math.exp(1 - 1 / ratio)
    return bleus


class DeviceLanguageEval(object):
    """The scorers of one split.  Built once from the loader's label arrays (`labels`, `label_start_ix`, `label_end_ix`,
    `split_ix[split]`): the reference rows of every image of the split are uploaded once, at the first score()."""

    def __init__(self, loader, split='val', device="cuda"):
        images = np.asarray(loader.split_ix[split], dtype=np.int64)
        first = np.asarray(loader.label_start_ix, dtype=np.int64)[images] - 1          # (1-indexed on disk)
        count = np.asarray(loader.label_end_ix, dtype=np.int64)[images] - first
        self._init(np.asarray(loader.labels), images, first, count, device)

    @classmethod
    def from_references(cls, ref_rows, ref_start, device="cuda"):
        """ref_rows [R, Lr] integers; the references of image i (i = 0 .. n_img - 1) are rows ref_start[i] .. ref_start[i + 1] - 1."""
        self = cls.__new__(cls)
        start = np.asarray(ref_start, dtype=np.int64)
        self._init(np.asarray(ref_rows), np.arange(len(start) - 1, dtype=np.int64), start[:-1], np.diff(start), device)
        return self

    def _init(self, labels, images, first, count, device):
        assert (count > 0).all(), "an image of the split has no caption"       # (DataLoader.get_captions asserts the same)
        assert labels.shape[1] <= 64, "caption rows of %d tokens (the kernels hold 64 words)" % labels.shape[1]
        self.device = torch.device(device)
        self.position = {int(ix): i for i, ix in enumerate(images)}
        self.start = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
        idx = np.concatenate([np.arange(f, f + c) for f, c in zip(first, count)])
        self.rows = np.ascontiguousarray(labels[idx], dtype=np.int64)            # the split's reference rows, image after image
        self.Lr = self.rows.shape[1]
        self._rows_d = None
        self._sets = {}
        self._pen = {}
        self.tables_built = 0

    def _penalty(self, half):
        if half not in self._pen:
            t = np.array([np.e ** (-(float(d) ** 2) / (2 * SIGMA ** 2)) for d in range(-half, half + 1)], dtype=np.float64)
            self._pen[half] = torch.from_numpy(t).to(self.device)            # cider_scorer.py:150, as the scorer evaluates it
        return self._pen[half]

    def _image_set(self, image_ix):
        """References, their starts and the document-frequency table of one evaluated image set, on the device.  Cached: the
        references of a split do not change between evaluations, and the reference computes df over the evaluated images only."""
        key = image_ix.tobytes()
        if key not in self._sets:
            lib = _lib.load()
            if self._rows_d is None:
                self._rows_d = torch.from_numpy(self.rows).to(self.device)
            try:
                pos = np.array([self.position[int(ix)] for ix in image_ix], dtype=np.int64)
            except KeyError as e:
                raise KeyError("image %s is not in the split this DeviceLanguageEval was built for" % e)
            count = self.start[pos + 1] - self.start[pos]
            start = np.concatenate([[0], np.cumsum(count)])
            idx = np.concatenate([np.arange(self.start[p], self.start[p + 1]) for p in pos])
            if len(idx) == len(self.rows) and (idx == np.arange(len(idx))).all():
                ref_d = self._rows_d                                             # the whole split in its own order
            else:
                ref_d = self._rows_d.index_select(0, torch.from_numpy(idx).to(self.device))
            keys, counts = document_frequency(self.rows[idx], start)
            n = len(keys)
            vals = np.log(np.maximum(1.0, counts))                               # counts2vec, cider_scorer.py:121
            slots = int(lib.uic_ciderd_table_slots(n))
            sk = np.empty((slots, 4), dtype=np.int32)
            sv = np.empty(slots, dtype=np.float64)
            keys = np.ascontiguousarray(keys) if n else np.full((1, 4), -1, dtype=np.int32)
            vals = np.ascontiguousarray(vals) if n else np.zeros(1)
            check(lib.uic_ciderd_table_build(keys.ctypes.data, vals.ctypes.data, n, sk.ctypes.data, sv.ctypes.data, slots),
                  "ciderd_table_build")
            self.tables_built += 1
            self._sets[key] = (ref_d, torch.from_numpy(start.astype(np.int32)).to(self.device), torch.from_numpy(sk).to(self.device),
                               torch.from_numpy(sv).to(self.device), slots, float(np.log(float(len(image_ix)))))
        return self._sets[key]

    def score(self, image_ix, hyp):
        """image_ix: the loader's image index (data['infos'][k]['ix']) of every row of hyp [n_img, L] (device int64, one caption
        per image).  Returns (overall, per_image): the six KEYS as python floats, and as arrays with one value per image (the
        imgToEval of language_eval).  Enqueue only, until ONE copy to the host ends the evaluation."""
        image_ix = np.ascontiguousarray(image_ix, dtype=np.int64)
        n = len(image_ix)
        if n < 2:
            raise ValueError("language evaluation needs at least 2 images (got %d): BleuScorer's default for a one-image corpus is "
                             "option='average' (bleu_scorer.py:207-208), which is not supported" % n)
        if len(set(image_ix.tolist())) != n:
            raise ValueError("language evaluation scores every image once; image_ix holds an image twice")
        lib = _lib.load()
        hyp = hyp.to(self.device, torch.int64).contiguous()
        assert hyp.dim() == 2 and hyp.shape[0] == n and hyp.shape[1] <= 64, tuple(hyp.shape)
        L = hyp.shape[1]
        ref_d, start_d, sk, sv, slots, ref_len = self._image_set(image_ix)
        half = max(L, self.Lr, 32)
        pen = self._penalty(half)
        # one buffer, one copy: bleu [4, n] | rouge [n] | cider [n] | means [2] | totals [10] (int64 bits)
        buf = torch.empty(6 * n + 12, dtype=torch.float64, device=self.device)
        bleu, rouge, cider, means = buf[:4 * n], buf[4 * n:5 * n], buf[5 * n:6 * n], buf[6 * n:6 * n + 2]
        totals = buf[6 * n + 2:].view(torch.int64)
        comps = torch.empty(n, 10, dtype=torch.int32, device=self.device)
        args = (ptr(hyp), n, L, n, 1, ptr(ref_d), self.Lr, ptr(start_d), n)
        check(lib.uic_langeval_bleu(*args, 0, ptr(comps), ptr(bleu), stream()), "langeval_bleu")
        check(lib.uic_langeval_rouge_l(*args, 0, C.c_double(BETA2), ptr(rouge), stream()), "langeval_rouge_l")
        check(lib.uic_langeval_cider(*args, ptr(sk), ptr(sv), slots, C.c_double(ref_len), ptr(pen), half, 0, ptr(cider), stream()),
              "langeval_cider")
        check(lib.uic_langeval_reduce(ptr(comps), ptr(rouge), ptr(cider), n, ptr(totals), ptr(means), stream()), "langeval_reduce")
        host = buf.cpu().numpy()
        self.last_totals = host[6 * n + 2:].view(np.int64).copy()
        b = corpus_bleu(self.last_totals)
        overall = {'Bleu_1': b[0], 'Bleu_2': b[1], 'Bleu_3': b[2], 'Bleu_4': b[3],
                   'ROUGE_L': float(host[6 * n]), 'CIDEr': float(host[6 * n + 1])}
        per_image = {'Bleu_%d' % (k + 1): host[k * n:(k + 1) * n].copy() for k in range(4)}
        per_image['ROUGE_L'] = host[4 * n:5 * n].copy()
        per_image['CIDEr'] = host[5 * n:6 * n].copy()
        return overall, per_image
