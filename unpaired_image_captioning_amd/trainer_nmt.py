"""The pivot NMT half of the Trainer (trainer.py; P/trainer.py:80-94,175-193): a plain base class of Trainer -- its state is
public surface that tests and INTEGRATION.md read on the trainer.  Uses the Trainer's opt, exchange, _mix_rank_into_seed and
_roll_back."""
import torch

from . import _lib
from .misc.optimizer import Optim


class NMTHalf(object):

    def _init_nmt(self):
        """The attributes this half owns; build_nmt fills the models, the criterion and `optim`, build_pivot the bridge."""
        self.nmt_model = None
        self.dp_nmt_model = None
        self.nmt_encoder = self.nmt_decoder = self.nmt_generator = None
        self.nmt_loss = self.nmt_crit = None
        self.optim = None
        self.nmt_train_ppl = self.nmt_train_acc = 0.0
        self.nmt_valid_ppl = self.nmt_valid_acc = None
        self.best_nmt_val_acc = None
        self.best_flag_nmt = False
        self.pivot_bridge = None

    def build_nmt(self, src_dict, tgt_dict):
        """Trainer.build_nmt: encoder/decoder/NMTModel, the generator attached as `model.generator`, NMT_loss, and the
        optimizer over the model's flat arena.  `src_dict` / `tgt_dict`: onmt.Dict-like (`.size()`) or plain sizes."""
        import torch.nn as nn
        from .models import NMT_Models
        from .misc import criterion
        opt = self.opt
        tgt_size = int(tgt_dict.size()) if hasattr(tgt_dict, 'size') else int(tgt_dict)
        self.nmt_encoder = NMT_Models.Encoder(opt, src_dict)
        self.nmt_decoder = NMT_Models.Decoder(opt, tgt_dict)
        self.nmt_model = NMT_Models.NMTModel(opt, self.nmt_encoder, self.nmt_decoder, src_dict, tgt_dict, False)
        self._mix_rank_into_seed(self.nmt_model, self.exchange)
        self.nmt_generator = nn.Sequential(nn.Linear(opt.rnn_size, tgt_size), nn.LogSoftmax(dim=-1))
        param_init = getattr(opt, 'param_init', 0.1)
        if param_init:
            for p in list(self.nmt_model.parameters()) + list(self.nmt_generator.parameters()):
                p.data.uniform_(-param_init, param_init)
        self.nmt_model.generator = self.nmt_generator
        self.dp_nmt_model = self.nmt_model
        self.nmt_model.cuda()
        self.nmt_model.train(bool(getattr(opt, 'nmt_train_flag', 1)))
        self.nmt_loss = criterion.NMTCriterion(tgt_size, opt)
        self.nmt_crit = criterion.NMT_loss(opt, self.nmt_generator, self.nmt_loss)
        self.optim = Optim(opt, self.exchange)
        self.optim.set_parameters(None, self.nmt_model)
        self.nmt_train_ppl = self.nmt_train_acc = 0.0
        return self.nmt_model

    def train_nmt(self, nmt_batch, loader=None, nmt_epoch=None, update_lr=False):
        """The NMT branch of Trainer.train (P/trainer.py:175-193): zero_grad, forward, NMT_loss, backward,
        Optim.step (noam LR, clip_grad_norm, Adam).  Returns the summed NLL of the batch (host float)."""
        if update_lr:
            self.optim.update_LearningRate('nmt', nmt_epoch)
        self.optim.zero_grad(nmt_direct=True)         # (no 360 MB fill: the in-place backward below overwrites every gradient)
        self.nmt_model.unit_loss_gradient = True      # loss.backward() below: the kernels may write the gradient arena in place
        outputs, attn, dec_state, upper_bounds = self.dp_nmt_model(nmt_batch.src, nmt_batch.tgt, nmt_batch.lengths, None)
        nmt_loss = self.nmt_crit(loader, nmt_batch, outputs, attn)
        nmt_loss.backward()
        sharded = getattr(self.optim, 'nmt_sharded', False)
        if sharded:
            # the step's loss rides in the sharded exchange's small all-reduce (slot 0 of the arena's scalar slots)
            self.optim.nmt_arena.scalars[0:1].copy_(nmt_loss.detach().reshape(1))
        self.optim.step()
        # the statistics are read AFTER the whole step is enqueued (one host sync per step, at its end)
        self.nmt_crit.report_stats.n_src_words += int(nmt_batch.lengths.sum())
        self.nmt_train_ppl = self.nmt_crit.report_stats.ppl()
        self.nmt_train_acc = self.nmt_crit.report_stats.accuracy()
        loss_d = nmt_loss.detach()
        if sharded:
            loss_d = self.optim.last_pair[0]
        elif self.exchange is not None and self.exchange.world_size > 1:
            # the criterion is a SUM over target words (size_average=False, P/misc/criterion.py:126-136): the whole batch's loss
            # is the sum over the ranks' column shards, as DataParallel(dim=1) + gather gives the reference (P/trainer.py:88,178)
            loss_d = loss_d.float().reshape(1).clone()
            self.exchange._sum(loss_d)
        val = float(loss_d)                           # (the step's host sync)
        guard = getattr(self.optim, 'last_guard', None)
        if guard is not None and float(guard[0].item()) != 0:
            # a persistent launch of this step timed out (on some rank): Optim.step skipped the update on the device
            self._roll_back(self.optim.nmt_arena.flat.device, self.optim, ('_step', '_nmt_steps'), _lib.PersistentTimeout(
                "persistent NMT kernel timed out: this step's update was skipped (weights and moments unchanged); "
                "engine.recurrence |= _lib.REC_FWD_CHAIN selects per-step launches"))
        return val

    def eval_nmt(self, batches):
        """The NMT half of the validation pass (P/trainer.py:212-215, P/eval_utils.py:313-317): the given validation batches
        through dp_nmt_model in eval mode and a fresh NMT_loss, no backward pass.  Sets nmt_valid_ppl, nmt_valid_acc,
        best_nmt_val_acc and best_flag_nmt (strict `>`)."""
        from .misc import criterion
        crit = criterion.NMT_loss(self.opt, self.nmt_generator, self.nmt_loss, eval=True)
        was_training = self.nmt_model.training
        self.nmt_model.eval()
        try:
            with torch.no_grad():
                for batch in batches:
                    outputs, attn, _, _ = self.dp_nmt_model(batch.src, batch.tgt, batch.lengths, None)
                    crit(None, batch, outputs, attn)
        finally:
            self.nmt_model.train(was_training)
        self.nmt_valid_ppl = crit.total_stats.ppl()
        self.nmt_valid_acc = crit.total_stats.accuracy()
        if self.best_nmt_val_acc is None or self.nmt_valid_acc > self.best_nmt_val_acc:
            self.best_nmt_val_acc = self.nmt_valid_acc
            self.best_flag_nmt = True

    def build_pivot(self, caption_vocab, scoring_vocab, src_dict=None, tgt_dict=None, max_words=None):
        """The bridge of the unpaired validation pass (misc/pivot.py): `caption_vocab` / `scoring_vocab` are the ix_to_word of the
        pivot-language loader and of the COCO loader; the dictionaries default to the NMT model's.  Stored as self.pivot_bridge."""
        from .misc import pivot
        src_dict = self.nmt_model.src_dict if src_dict is None else src_dict
        tgt_dict = self.nmt_model.tgt_dict if tgt_dict is None else tgt_dict
        device = next(self.nmt_model.parameters()).device
        self.pivot_bridge = pivot.PivotBridge(caption_vocab, src_dict, tgt_dict, scoring_vocab, device=device,
                                              max_words=pivot.MAX_WORDS if max_words is None else max_words)
        return self.pivot_bridge
