"""Mode dispatch of the reference's CaptionModel (P/models/CaptionModel.py:27-31) and what every captioner's `_sample_beam` shares:
the beam count a search really runs with, and `done_beams`, built on first access from the raw lists the beam kernels leave."""
import torch.nn as nn


class CaptionModel(nn.Module):
    def __init__(self):
        super(CaptionModel, self).__init__()
        self._done_beams = self._done_raw = None

    def forward(self, *args, **kwargs):
        mode = kwargs.get('mode', 'forward')
        if 'mode' in kwargs:
            del kwargs['mode']
        return getattr(self, '_' + mode)(*args, **kwargs)

    @staticmethod
    def _effective_beam_size(opt):
        beam_size = opt.get('beam_size', 10)
        group_size = opt.get('group_size', 1)
        if group_size > 1:
            # diverse groups (CaptionModel.py:100-177): the caller only ever receives done_beams[k][0] (AttModel.py:193-194,
            # FCModel_NMT.py:159-160), the best beam of group 0, which never sees a diversity penalty -- a plain search over its
            # bdash beams
            beam_size = beam_size // group_size
        return beam_size

    def _set_done_raw(self, cnt, dp, dseq, dlp, beam_size):
        """The finished beams of a search as the library exports them (`_lib.done_list_buffers`).  The per-image lists are built on
        first access to `self.done_beams` (one D2H copy per array then): a caller that only wants the best captions -- eval_split
        without `verbose_beam`, the pivot decode -- pays nothing for them."""
        self._done_raw = (cnt, dp, dseq, dlp, beam_size)
        self._done_beams = None

    @property
    def done_beams(self):
        """done_beams[k] is the reference's list for image k: its finished beams sorted by -p (stable), the first beam_size of them,
        each {'seq', 'logps', 'unaug_p', 'p'} (CaptionModel.py:147-161, 174-176)."""
        if self._done_beams is None and self._done_raw is not None:
            cnt, dp, dseq, dlp, beam_size = self._done_raw
            cnt_h, dp_h, unaug = cnt.cpu().tolist(), dp.cpu(), dlp.sum(-1).cpu()
            out = []
            for k in range(len(cnt_h)):
                order = sorted(range(cnt_h[k]), key=lambda i: -float(dp_h[k, i]))[:beam_size]     # sorted() is stable, like the reference's
                out.append([{'seq': dseq[k, i], 'logps': dlp[k, i], 'unaug_p': float(unaug[k, i]), 'p': float(dp_h[k, i])} for i in order])
            self._done_beams = out
        return self._done_beams

    @done_beams.setter
    def done_beams(self, value):
        self._done_beams, self._done_raw = value, None
