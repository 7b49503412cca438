"""The sentence discriminator of the Trainer (trainer.py; BASELINE configs[3], parity unpinned): a plain base class of Trainer --
its state is public surface that tests and INTEGRATION.md read on the trainer.  Uses the Trainer's opt, exchange, betas and
eps."""
import torch

from .misc.optimizer import FlatArena


class DiscriminatorHalf(object):

    def _init_disc(self):
        """The attributes this half owns; build_discriminator fills them."""
        self.discriminator = None
        self.disc_sharded = False
        self.disc_arena = None
        self.disc_lr = None
        self._disc_step = 0
        self.disc_train_loss = None

    def build_discriminator(self):
        """The CNN sentence discriminator of the unpaired / adversarial configuration (models/Discriminator.py) with its own flat
        Adam arena; data parallel like the captioner (gradient arena summed over the ranks)."""
        from .models import SentenceDiscriminator
        from .trainer import rank_seed
        self.discriminator = SentenceDiscriminator(self.opt).cuda()
        rank = self.exchange.rank if self.exchange is not None else 0
        self.discriminator.seed = rank_seed(self.discriminator.seed, rank)    # per-rank dropout noise
        ex = self.exchange
        self.disc_sharded = bool(ex is not None and ex.world_size > 1 and not getattr(self.opt, 'allreduce_exchange', 0))
        if self.disc_sharded:        # one piece, f32 masters gathered in place (the discriminator's kernels read the masters)
            names = [k for k, _ in self.discriminator.named_parameters()]
            self.disc_arena = FlatArena(self.discriminator, names, world=ex.world_size, rank=ex.rank, pieces=[names])
        else:
            self.disc_arena = FlatArena(self.discriminator)
        self.disc_lr = float(getattr(self.opt, 'disc_learning_rate', 1e-4) or 1e-4)
        self._disc_step = 0
        return self.discriminator

    def _pad_rows(self, seq):
        """Caption rows [N, L'] (int64, 0 = end) as the discriminator's [N, seq_length] rows."""
        L = self.discriminator.L
        seq = seq.cuda() if not seq.is_cuda else seq
        if seq.shape[1] < L:
            seq = torch.cat([seq, seq.new_zeros(seq.shape[0], L - seq.shape[1])], 1)
        return seq[:, :L].contiguous().long()

    def discriminator_scores(self, seq):
        self.discriminator.eval()
        return self.discriminator.scores(self._pad_rows(seq))

    def train_discriminator(self, real_seq, fake_seq):
        """One BCE step: real caption rows (label 1) against generated rows (label 0).  Returns the loss (one host sync)."""
        if self.discriminator is None:
            self.build_discriminator()
        D, a = self.discriminator, self.disc_arena
        D.train()
        tok = torch.cat([self._pad_rows(real_seq), self._pad_rows(fake_seq)])
        lab = torch.cat([torch.ones(real_seq.shape[0]), torch.zeros(fake_seq.shape[0])]).cuda()
        a.zero_grad()
        loss = D.bce(D(tok), lab)
        loss.backward()
        self._disc_step += 1
        if self.disc_sharded:
            a.scalars[0:2].zero_()
            a.scalars[0:1].copy_(loss.detach().reshape(1))
            pair, _ = a.sharded_step(self.exchange, self.disc_lr, self.betas, self.eps, self._disc_step, 1.0 / self.exchange.world_size)
            self.disc_train_loss = float(pair[0].item()) / self.exchange.world_size      # (mean of the ranks' batch means)
            return self.disc_train_loss
        self.exchange.allreduce_sum(a.grad)
        a.adam(self.disc_lr, self.betas, self.eps, self._disc_step, grad_scale=1.0 / self.exchange.world_size)
        self.disc_train_loss = loss.item()
        return self.disc_train_loss
