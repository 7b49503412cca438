"""CPU restatement of the three scorers behind `lang_stats` on integer token rows, and the random case generator of the
language-evaluation tests.  The scorers restated (nothing of their text is copied):

    Bleu(4)   P/AI_Challenger/Evaluation/caption_eval/coco_caption/pycxevalcap/bleu/bleu_scorer.py:23-88 (counts), :199-256
    Rouge()   .../pycxevalcap/rouge/rouge.py:13-75
    Cider()   .../pycxevalcap/cider/cider_scorer.py:11-27 (n-grams), :93-181

A caption's words are its tokens BEFORE the first 0 (utils.decode_sequence); the scorers see them as strings of ids joined by
one blank, so an empty caption is [] for Bleu / Cider (str.split()) and [''] for Rouge (str.split(" ")).
"""
import math

import numpy as np

KEYS = ('Bleu_1', 'Bleu_2', 'Bleu_3', 'Bleu_4', 'ROUGE_L', 'CIDEr')
SMALL, TINY = 1e-9, 1e-15


def words(row):
    out = []
    for t in row:
        if int(t) == 0:
            break
        out.append(int(t))
    return out


def ngram_counts(w, n=4):
    """precook: n-gram -> count, in order of first occurrence per order (a dict keeps insertion order)."""
    counts = {}
    for k in range(1, n + 1):
        for i in range(len(w) - k + 1):
            g = tuple(w[i:i + k])
            counts[g] = counts.get(g, 0) + 1
    return counts


# ---------------------------------------------------------------- BLEU
def bleu_comps(hyp, refs):
    """[correct[0..3], guess[0..3], testlen, closest reflen] of one hypothesis (cook_refs / cook_test, option='closest')."""
    test = ngram_counts(hyp)
    maxcounts = {}
    for r in refs:
        for g, c in ngram_counts(r).items():
            maxcounts[g] = max(maxcounts.get(g, 0), c)
    testlen = len(hyp)
    reflen = min((abs(len(r) - testlen), len(r)) for r in refs)[1]
    guess = [max(0, testlen - k) for k in range(4)]
    correct = [0] * 4
    for g, c in test.items():
        correct[len(g) - 1] += min(maxcounts.get(g, 0), c)
    return correct + guess + [testlen, reflen]


def bleu_from_comps(c):
    """BLEU-1..4 from the ten integers, per sentence (:230-239) and per corpus (:247-256): the same expression."""
    correct, guess, testlen, reflen = c[0:4], c[4:8], c[8], c[9]
    out = []
    bleu = 1.
    for k in range(4):
        bleu *= (float(correct[k]) + TINY) / (float(guess[k]) + SMALL)
        out.append(bleu ** (1. / (k + 1)))
    ratio = (testlen + TINY) / (reflen + SMALL)
    if ratio < 1:
        for k in range(4):
            out[k] *= math.exp(1 - 1 / ratio)
    return out


# ---------------------------------------------------------------- ROUGE-L
def lcs(a, b):
    """Length of the longest common subsequence, by the textbook table."""
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b):
            cur.append(prev[j] + 1 if x == y else max(prev[j + 1], cur[j]))
        prev = cur
    return prev[-1]


def lcs_bitvector(a, b):
    """The recurrence the kernel runs, on one 64-bit word: the number of zero bits among the low len(a) bits."""
    assert len(a) <= 64 and len(b) <= 64
    full = (1 << 64) - 1
    V = full
    for y in b:
        M = sum(1 << i for i, x in enumerate(a) if x == y)
        U = V & M
        V = (((V + U) & full) | ((V - U) & full)) & full
    return bin(~V & ((1 << len(a)) - 1)).count("1")


def rouge_l(hyp, refs, beta=1.2):
    c = hyp if hyp else ['']
    prec, rec = [], []
    for r in refs:
        r = r if r else ['']
        n = lcs(r, c)
        prec.append(n / float(len(c)))
        rec.append(n / float(len(r)))
    p, r = max(prec), max(rec)
    if p != 0 and r != 0:
        return ((1 + beta ** 2) * p * r) / float(r + beta ** 2 * p)
    return 0.0


# ---------------------------------------------------------------- CIDEr
def document_frequency(ref_sets):
    """n-gram -> number of images whose reference set holds it (compute_doc_freq)."""
    df = {}
    for refs in ref_sets:
        for g in set(g for r in refs for g in ngram_counts(r)):
            df[g] = df.get(g, 0.0) + 1
    return df


def cider(hyps, ref_sets, sigma=6.0):
    df = document_frequency(ref_sets)
    ref_len = np.log(float(len(ref_sets)))

    def vec(cnts):
        v = [dict() for _ in range(4)]
        norm = [0.0] * 4
        length = 0
        for g, tf in cnts.items():
            n = len(g) - 1
            v[n][g] = float(tf) * (ref_len - np.log(max(1.0, df.get(g, 0.0))))
            norm[n] += pow(v[n][g], 2)
            if n == 1:
                length += tf
        return v, [np.sqrt(x) for x in norm], length

    scores = []
    for hyp, refs in zip(hyps, ref_sets):
        vh, nh, lh = vec(ngram_counts(hyp))
        score = np.zeros(4)
        for r in refs:
            vr, nr, lr = vec(ngram_counts(r))
            delta = float(lh - lr)
            val = np.zeros(4)
            for n in range(4):
                for g in vh[n]:
                    val[n] += min(vh[n][g], vr[n].get(g, 0.0)) * vr[n].get(g, 0.0)
                if nh[n] != 0 and nr[n] != 0:
                    val[n] /= (nh[n] * nr[n])
                val[n] *= np.e ** (-(delta ** 2) / (2 * sigma ** 2))
            score += val
        s = np.mean(score)
        s /= len(refs)
        s *= 10.0
        scores.append(s)
    return np.array(scores)


# ---------------------------------------------------------------- the whole evaluation
def evaluate(hyp, ref_tok, ref_start):
    """hyp [n, L], ref_tok [R, Lr], ref_start [n + 1] -> dict(bleu [4, n], rouge [n], cider [n], totals [10] int64,
    corpus [6] in KEYS order)."""
    n = len(hyp)
    hyps = [words(r) for r in hyp]
    ref_sets = [[words(r) for r in ref_tok[ref_start[i]:ref_start[i + 1]]] for i in range(n)]
    comps = np.array([bleu_comps(h, rs) for h, rs in zip(hyps, ref_sets)], dtype=np.int64)
    bleu = np.array([bleu_from_comps([int(x) for x in c]) for c in comps]).T
    rouge = np.array([rouge_l(h, rs) for h, rs in zip(hyps, ref_sets)])
    cid = cider(hyps, ref_sets)
    totals = comps.sum(0)
    corpus = np.array(bleu_from_comps([int(x) for x in totals]) + [np.mean(rouge), np.mean(cid)])
    return dict(bleu=bleu, rouge=rouge, cider=cid, totals=totals, corpus=corpus)


def caption_rows(g, n, width, V, p_full=0.3, min_words=0):
    """Label-style rows: tokens 1..V skewed towards small ids (so that n-grams repeat), zero padded; some fill the row."""
    rows = np.zeros((n, width), dtype=np.int64)
    for i in range(n):
        ln = width if g.random() < p_full else int(g.integers(min(min_words, width), width + 1))
        rows[i, :ln] = np.minimum(g.integers(1, V + 1, ln), g.integers(1, V + 1, ln))
    return rows


def random_case(seed, V, L, Lr, n_img, n_refs):
    """(hyp [n_img, L], ref_tok, ref_start).  n_refs: references per image, an int or one int per image.  References have at
    least one word; every third hypothesis copies the head of a reference, one is empty, one repeats a word."""
    g = np.random.default_rng(seed)
    counts = [n_refs] * n_img if np.isscalar(n_refs) else list(n_refs)
    ref_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    ref_tok = caption_rows(g, int(ref_start[-1]), Lr, V, min_words=1)
    hyp = caption_rows(g, n_img, L, V)
    m = min(L, Lr)
    for i in range(0, n_img, 3):
        hyp[i, :m] = ref_tok[ref_start[i]][:m]
    if n_img > 1:
        hyp[1] = 0
    if n_img > 2:
        hyp[2, :] = ref_tok[ref_start[2]][0]
    return hyp, ref_tok, ref_start
