"""AttEnsemble behind the reference's constructor / call contract (P/models/AttEnsemble.py:29-98, eval_ensemble.py:118-129):
several captioners decode together with the MEAN of their word distributions.

Every member keeps its own TopDownEngine (weights, derived copies, workspaces); the decode loops are the library's ensemble
sequencers (uic_topdown_ensemble_sample / _sample_beam): per step every member's decode step, one kernel that folds the
members' logits into log(mean(softmax)), then the single model's sampling / beam kernels.  Eval mode only, as in the
reference (eval_ensemble.py calls model.eval() before anything else).  There is no eager fallback.
"""
import torch
import torch.nn as nn

from .AttModel import AttModel, TopDownModel
from .CaptionModel import CaptionModel
from .. import topdown_engine as TE


class AttEnsemble(AttModel):
    def __init__(self, models):
        CaptionModel.__init__(self)      # (not AttModel's: the ensemble owns no parameters of its own, AttEnsemble.py:31)
        models = list(models)
        if not 1 <= len(models) <= TE._lib.ENSEMBLE_MAX:
            raise ValueError("an ensemble has 1..%d members, got %d" % (TE._lib.ENSEMBLE_MAX, len(models)))
        for i, m in enumerate(models):
            # (AdaAttModel is an AttModel too, but has no TopDownEngine for the ensemble sequencers to step)
            if not isinstance(m, TopDownModel):
                raise TypeError("ensemble member %d is a %s, not a TopDownModel" % (i, type(m).__name__))
            if m.vocab_size != models[0].vocab_size or m.seq_length != models[0].seq_length:
                raise ValueError("ensemble member %d has vocab_size=%d seq_length=%d, member 0 vocab_size=%d seq_length=%d: the members "
                                 "must share the vocabulary and the caption length" %
                                 (i, m.vocab_size, m.seq_length, models[0].vocab_size, models[0].seq_length))
        self.models = nn.ModuleList(models)
        self.vocab_size = models[0].vocab_size
        self.seq_length = models[0].seq_length
        self.ss_prob = 0

    # ------------------------------------------------------------------ plumbing
    def _require_eval(self, what):
        if self.training or any(m.training for m in self.models):
            raise NotImplementedError("AttEnsemble.%s runs in eval mode only (eval_ensemble.py calls model.eval() first)" % what)

    def _members(self):
        """(engines, parameter dicts) of the members."""
        return [m.engine for m in self.models], [{k: v.detach() for k, v in m.param_dict().items()} for m in self.models]

    def _features(self, fc_feats, att_feats, att_masks):
        """Shared fc_feats / att_masks and every member's slice of the region features (AttEnsemble.py:62)."""
        fc = fc_feats.contiguous().float()
        am = att_masks.contiguous().float() if att_masks is not None else None
        atts = [att_feats[..., :m.att_feat_size].contiguous().float() for m in self.models]
        return fc, atts, am

    # ------------------------------------------------------------------ reference call surface
    def _forward(self, *args, **kwargs):
        raise NotImplementedError("AttEnsemble only decodes (the reference never trains an ensemble)")

    def init_hidden(self, batch_size):
        return [m.init_hidden(batch_size) for m in self.models]

    def _prepare_feature(self, fc_feats, att_feats, att_masks):
        """AttEnsemble.py:57-67 -> ([fc'], [att'], [p_att], [att_masks] * M), per-member lists of f32 device tensors."""
        self._require_eval("_prepare_feature")
        att_feats, att_masks = self.clip_att(att_feats, att_masks)
        out = [m._prepare_feature(fc_feats, att_feats[..., :m.att_feat_size], att_masks) for m in self.models]
        return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out], [out[0][3]] * len(self.models)

    def get_logprobs_state(self, it, fc_feats, att_feats, p_att_feats, att_masks, state, t=0):
        """AttEnsemble.py:48-55: one decode step of every member from its prepared features and state, then
        log(mean_m softmax_m) -> (log-probs [N, V+1], [member states])."""
        self._require_eval("get_logprobs_state")
        steps = [m.get_logprobs_state(it, fc_feats[i], att_feats[i], p_att_feats[i], att_masks[i], state[i], t=t)
                 for i, m in enumerate(self.models)]
        # (softmax of a member's log-probs is its word distribution)
        return TE.ensemble_logprobs([lp for lp, _ in steps]), [st for _, st in steps]

    def _sample_beam(self, fc_feats, att_feats, att_masks=None, opt={}):
        """AttEnsemble.py:69-98 + beam_search :100-244 with group_size = 1: all images in one device pass; `done_beams` as in
        AttModel (built on first access from the raw lists in member 0's workspace)."""
        beam_size = self._effective_beam_size(opt)
        self._require_eval("_sample_beam")
        assert beam_size <= self.vocab_size + 1
        fc, atts, am = self._features(fc_feats, att_feats, att_masks)
        with torch.no_grad():
            engines, params = self._members()
            seq, lp, lists = TE.ensemble_sample_beam(engines, params, fc, atts, am, self.seq_length, beam_size,
                                                     opt.get('decoding_constraint', 0), opt.get('max_ppl', 0), done_lists=True)
        self._set_done_raw(*lists, beam_size)
        return seq, lp

    def _sample(self, fc_feats, attri_feats, att_feats, att_masks=None, opt={}):
        if opt.get('beam_size', 1) > 1:
            return self._sample_beam(fc_feats, att_feats, att_masks, opt)
        self._require_eval("_sample")
        fc, atts, am = self._features(fc_feats, att_feats, att_masks)
        with torch.no_grad():
            engines, params = self._members()
            return TE.ensemble_sample(engines, params, fc, atts, am, self.seq_length, sample_max=opt.get('sample_max', 1),
                                      temperature=opt.get('temperature', 1.0), decoding_constraint=opt.get('decoding_constraint', 0),
                                      seed=self.models[0].next_seed(), forced=opt.get('forced_tokens'),
                                      seq_per_img=int(opt.get('captions_per_image', 1) or 1))      # (as AttModel._sample)
