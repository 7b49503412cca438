"""Restatements and small helpers for the FC captioner's training tests (tests/test_fc_trainer_host.py,
tests/test_gpu_fc_trainer.py), on top of oracle/fc.py, which stays the one statement of the model itself.

The self-critical step's sampling pass (P/trainer.py:167 -> FCModel_NMT._sample, sample_max = 0) is restated teacher-forced:
the tokens the pass fed are known afterwards, so its log-probs are `forward_logprobs` on [<bos> | tokens] gathered at those
tokens -- with two things the sampling loop does that a teacher-forced pass does not:
  * the loop breaks BEFORE it writes the column at which every row has finished (P/models/FCModel_NMT.py:203-206), and the last
    of the L + 1 columns is never reached: seqLogprobs stays a CONSTANT 0 there (no gradient), although RewardCriterion's mask
    may still count such a position in its denominator;
  * the RAW sampled token feeds the next step, also behind a row's end (:199), and seqLogprobs records the raw token's log-prob.
"""
import argparse

import torch

from oracle import fc as OF
from oracle import topdown as O


def make_opt(cfg, dtype, drop=0.0, seed=0, **kw):
    """Trainer options for caption_model='fc' at a golden fixture's shapes."""
    return argparse.Namespace(vocab_size=cfg["V"], input_encoding_size=cfg["E"], rnn_type="LSTM", rnn_size=cfg["H"], num_layers=1,
                              drop_prob_lm=drop, seq_length=cfg["L"], fc_feat_size=cfg["D"], caption_model="fc", compute_dtype=dtype,
                              seed=seed, **kw)


def masked_stream(tokens):
    """What the sampling loop stores for a stream of raw tokens [N, L] (:200-208): [N, L+1], a row's tokens up to its first 0,
    zeros behind it, and nothing from the column on at which every row has finished."""
    unfinished = (tokens > 0).long().cumprod(1)
    seq = tokens * unfinished
    return torch.cat([seq, torch.zeros(seq.shape[0], 1, dtype=seq.dtype)], 1)


def written_columns(seq):
    """Number of leading columns of seq [N, L+1] the sampling loop wrote: up to the first all-zero column (the break)."""
    zero = (seq.sum(0) == 0).nonzero()
    return int(zero[0]) if zero.numel() else seq.shape[1]


def sampled_logprobs(W, fc_feats, seq, drop=None, fed=None):
    """seqLogprobs [N, L+1] of the sampling pass that returned `seq`, differentiable w.r.t. W.  fed [N, L]: the raw tokens the
    pass fed (forced tokens); default: seq itself, which is the same in front of every row's end -- the only positions
    RewardCriterion's mask lets through.  drop: {'out': [>= L+2, N, H]} dropout masks of the core steps."""
    N, L1 = seq.shape
    raw = seq[:, :L1 - 1] if fed is None else fed
    labels = torch.cat([torch.zeros(N, 1, dtype=torch.long), raw, torch.zeros(N, 1, dtype=torch.long)], 1)       # [N, L+2]
    logp = OF.forward_logprobs(W, fc_feats, labels, drop)                                                        # [N, L+1, V1]
    lp = logp.gather(2, labels[:, 1:].unsqueeze(2)).squeeze(2)
    keep = (torch.arange(L1) < min(written_columns(seq), L1 - 1)).to(lp.dtype)
    return lp * keep


def scst_loss_and_grads(W, fc_feats, seq, reward, drop=None, fed=None):
    """RewardCriterion (P/misc/criterion.py:117-124) on the restated pass: (loss, {key: gradient}, seqLogprobs)."""
    Wg = {k: v.detach().clone().requires_grad_(True) for k, v in W.items()}
    lp = sampled_logprobs(Wg, fc_feats, seq, drop, fed)
    loss = O.reward_criterion(lp, seq, reward)
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in Wg.items()}
    return loss.detach(), grads, lp.detach()


def forced_streams(N, L, V, seed):
    """Raw token streams [N, L] that reach every branch of the sampling loop: row 0 ends at its first token and is fed non-zero
    tokens behind its end, row 1 never ends, the others end somewhere in the middle (and carry non-zero tokens behind)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(1, V + 1, (N, L), generator=g)
    t[0, 0] = 0
    for n in range(2, N):
        t[n, 1 + (n * 2) % max(L - 1, 1)] = 0
    return t


def all_ended_streams(N, L, V, seed, end):
    """Streams in which every row has ended at column `end` < L at the latest: the loop breaks there."""
    t = forced_streams(N, L, V, seed)
    t[:, end] = 0
    for n in range(N):
        if n % 2:
            t[n, max(end - 1, 0)] = 0
    return t
