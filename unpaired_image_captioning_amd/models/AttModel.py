"""TopDownModel behind the reference's constructor / call / state_dict contract
(P/models/AttModel.py:55-253, 421-446, 529-558, 686-690), computed by libuic_hip.so.

The nn.Module tree below exists only to own parameters under the reference's names
(`embed.0.weight`, `core.att_lstm.weight_ih`, ...), so `state_dict()` / `load_state_dict()`
round-trip the reference's `model_i2t-best.pth` unchanged; none of these sub-modules'
`forward` is ever called.  There is no eager fallback: without the HIP library, or on a
CPU tensor, every call raises.

AdaAttModel / AdaAttMOModel (P/models/AttModel.py:256-418, 657-667) follow at the end of the file under the same
contract, for evaluation and decoding only: they are computed by the uic_adaatt_* sequencers (csrc/adaatt.hip),
not by a TopDownEngine.
"""
import ctypes as C

import torch
import torch.nn as nn
import torch.nn.functional as F

from .CaptionModel import CaptionModel
from .. import _lib
from .._lib import check, ptr, stream
from ..topdown_engine import TopDownEngine


class Attention(nn.Module):
    def __init__(self, opt):
        super(Attention, self).__init__()
        self.rnn_size = opt.rnn_size
        self.att_hid_size = opt.att_hid_size
        self.h2att = nn.Linear(self.rnn_size, self.att_hid_size)
        self.alpha_net = nn.Linear(self.att_hid_size, 1)


class TopDownCore(nn.Module):
    def __init__(self, opt, use_maxout=False):
        super(TopDownCore, self).__init__()
        self.drop_prob_lm = opt.drop_prob_lm
        self.att_lstm = nn.LSTMCell(opt.input_encoding_size + opt.rnn_size * 2, opt.rnn_size)
        self.lang_lstm = nn.LSTMCell(opt.rnn_size * 2, opt.rnn_size)
        self.attention = Attention(opt)


class _TopDownForward(torch.autograd.Function):
    """log-probs = AttModel._forward(...); backward = the library's BPTT."""

    @staticmethod
    def forward(ctx, model, fc, att, seq, att_masks, t_run, *params):
        eng = model.engine
        names = model.param_names
        pd = dict(zip(names, params))
        seed = model.next_seed()
        training = model.training
        ss_prob = float(model.ss_prob) if training else 0.0          # AttModel.py:130
        logp, ws, (d, w, b) = eng.forward(pd, fc, att, att_masks, seq, t_run, training, seed, want_logprobs=True, ss_prob=ss_prob)
        ctx.model = model
        ctx.ws = ws
        ctx.call = (d, t_run, training, seed, ss_prob)
        ctx.inputs = (fc, att, att_masks, seq)
        ctx.params = params
        ctx.save_for_backward(logp)
        return logp

    @staticmethod
    def backward(ctx, g):
        model = ctx.model
        eng = model.engine
        if ctx.ws is None:
            # the reference calls loss.backward(retain_graph=True) (P/trainer.py:173) but never walks the graph twice; here the
            # first backward hands the forward's workspace (activations of every decode step) back to the engine's pool
            raise RuntimeError("TopDownModel: backward ran a second time over the same forward pass; its workspace was released "
                               "after the first one (retain_graph=True keeps the autograd graph, not the HIP workspace) -- run the "
                               "forward again")
        (logp,) = ctx.saved_tensors
        d, t_run, training, seed, ss_prob = ctx.call
        fc, att, att_masks, seq = ctx.inputs
        pd = dict(zip(model.param_names, ctx.params))
        w = eng.refresh(pd, d)
        # features that came out of an encoder (the scene-graph GCN of configs[4]) ask for their gradient; the reference's
        # own features are data and pay nothing
        d_fc, d_att = eng.input_grad_buffers(fc, att, ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        b = eng.batch_struct(fc, att, att_masks, seq, ss_prob=ss_prob, d_fc=d_fc, d_att=d_att)
        grads = {k: torch.empty_like(v) for k, v in pd.items()}
        eng.backward(ctx.ws, d, w, b, t_run, training, seed, grads, dlogprobs=g.contiguous(), logprobs=logp)
        eng.release(ctx.ws)
        ctx.ws = None
        if d_att is not None:
            d_att = d_att[..., :att.shape[-1]]
        return (None, d_fc, d_att, None, None, None) + tuple(grads[k] for k in model.param_names)


class _HeldWorkspace(object):
    """A checked-out engine workspace that goes back to the pool when backward has used it -- or when the graph that
    holds it is dropped without a backward pass."""

    def __init__(self, eng, ws):
        self.eng, self.ws = eng, ws

    def take(self):
        ws, self.ws = self.ws, None
        return ws

    def __del__(self):
        if self.ws is not None:
            try:
                self.eng.release(self.ws)
            except Exception:
                pass
            self.ws = None


class _TopDownSample(torch.autograd.Function):
    """Multinomial sampling pass of the self-critical step (P/trainer.py:167): returns (seq, seqLogprobs) with
    seqLogprobs differentiable.  Backward replays the sampled sequence teacher-forced with the SAME dropout seed
    (the masks are a pure function of seed/site/index) and feeds d loss / d logprob of the sampled tokens
    straight into the fused training step."""

    @staticmethod
    def forward(ctx, model, fc, att, att_masks, sample_kw, *params):
        eng = model.engine
        pd = dict(zip(model.param_names, params))
        seed = model.next_seed()
        # in train mode the pass keeps its forward (training layout): backward starts at the criterion instead of replaying
        keep = bool(model.training) and getattr(model, 'scst_keep_forward', True)
        if keep:
            seq, lp, ws = eng.sample(pd, fc, att, att_masks, model.seq_length, seed=seed, training=True, keep_forward=True, **sample_kw)
            ctx.ws = _HeldWorkspace(eng, ws)
        else:
            seq, lp = eng.sample(pd, fc, att, att_masks, model.seq_length, seed=seed, training=model.training, **sample_kw)
            ctx.ws = None
        ctx.model = model
        ctx.call = (seed, model.training)
        ctx.inputs = (fc, att, att_masks, seq)
        ctx.params = params
        ctx.mark_non_differentiable(seq)
        return seq, lp

    @staticmethod
    def backward(ctx, g_seq, g_lp):
        model = ctx.model
        eng = model.engine
        seed, training = ctx.call
        fc, att, att_masks, seq = ctx.inputs
        pd = dict(zip(model.param_names, ctx.params))
        N, L = seq.shape
        labels = torch.zeros(N, L + 2, dtype=torch.int64, device=seq.device)
        labels[:, 1:L + 1] = seq
        # direct: every p.grad IS its view of the optimizer's flat gradient arena (Trainer.train_self_critical set both up):
        # the kernels write there and autograd gets nothing to copy or accumulate; otherwise fresh tensors go back to autograd
        sink = getattr(model, '_grad_sink', None)
        direct = sink is not None and all(p.grad is sink[k] for k, p in zip(model.param_names, ctx.params))
        grads = sink if direct else {k: torch.empty_like(v) for k, v in pd.items()}
        # d loss / d logits = -g * (softmax - onehot)  ->  gradient weight of position (n, t) is -g[n, t]
        # bit 1: the sampling pass of this iteration already updated the BatchNorm running statistics
        held = ctx.ws.take() if ctx.ws is not None else None
        if held is not None:
            # the sampling pass left its whole forward in `held` (dims T = L + 1: the labels keep their L + 2 columns)
            eng.xe_train_step(pd, fc, att, att_masks, labels, None, L, int(training) | 2, seed, grads,
                              grad_scale=(-g_lp).contiguous(), resume_ws=held)
        else:
            eng.xe_train_step(pd, fc, att, att_masks, labels[:, :L + 1].contiguous(), None, L, int(training) | 2, seed, grads,
                              grad_scale=(-g_lp).contiguous())
        if direct:
            return (None, None, None, None, None) + (None,) * len(model.param_names)
        return (None, None, None, None, None) + tuple(grads[k] for k in model.param_names)


class AttModel(CaptionModel):
    supports_grad_sink = True      # _TopDownSample.backward can write straight into Trainer's flat gradient arena

    def __init__(self, opt):
        super(AttModel, self).__init__()
        self.vocab_size = opt.vocab_size
        self.input_encoding_size = opt.input_encoding_size
        self.rnn_size = opt.rnn_size
        self.num_layers = opt.num_layers
        self.drop_prob_lm = opt.drop_prob_lm
        self.seq_length = opt.seq_length
        self.fc_feat_size = opt.fc_feat_size
        self.att_feat_size = opt.att_feat_size
        self.att_hid_size = opt.att_hid_size
        self.use_bn = getattr(opt, 'use_bn', 0)
        self.ss_prob = 0.0  # Schedule sampling probability
        if self.use_bn not in (0, 1, 2):
            raise ValueError("use_bn=%r must be 0, 1 or 2" % (self.use_bn,))
        self.logit_layers = getattr(opt, 'logit_layers', 1)
        if not 1 <= self.logit_layers <= _lib.MAX_LOGIT_LAYERS:
            raise NotImplementedError("logit_layers=%r: the MI355X path supports 1..%d" % (self.logit_layers, _lib.MAX_LOGIT_LAYERS))

        self.embed = nn.Sequential(nn.Embedding(self.vocab_size + 1, self.input_encoding_size),
                                   nn.ReLU(),
                                   nn.Dropout(self.drop_prob_lm))
        self.fc_embed = nn.Sequential(nn.Linear(self.fc_feat_size, self.rnn_size),
                                      nn.ReLU(),
                                      nn.Dropout(self.drop_prob_lm))
        self.att_embed = nn.Sequential(*(
            ((nn.BatchNorm1d(self.att_feat_size),) if self.use_bn else ()) +
            (nn.Linear(self.att_feat_size, self.rnn_size),
             nn.ReLU(),
             nn.Dropout(self.drop_prob_lm)) +
            ((nn.BatchNorm1d(self.rnn_size),) if self.use_bn == 2 else ())))
        if self.logit_layers == 1:
            self.logit = nn.Linear(self.rnn_size, self.vocab_size + 1)
        else:       # P/models/AttModel.py:90-91: blocks [Linear(H, H), ReLU, Dropout(0.5)] in front of the vocabulary layer
            blocks = []
            for _ in range(self.logit_layers - 1):
                blocks += [nn.Linear(self.rnn_size, self.rnn_size), nn.ReLU(), nn.Dropout(0.5)]
            self.logit = nn.Sequential(*(blocks + [nn.Linear(self.rnn_size, self.vocab_size + 1)]))
        self.ctx2att = nn.Linear(self.rnn_size, self.att_hid_size)

        # MI355X engine state (not part of the checkpoint)
        self.compute_dtype = getattr(opt, 'compute_dtype', 'bf16')
        self._engine = None
        self._seed_counter = int(getattr(opt, 'seed', 0) or 0) & 0x7FFFFFFF

    # ------------------------------------------------------------------ engine plumbing
    @property
    def engine(self):
        if self._engine is None:
            self._engine = TopDownEngine(dict(V1=self.vocab_size + 1, E=self.input_encoding_size, H=self.rnn_size,
                                              A=self.att_hid_size, D=self.att_feat_size, Dfc=self.fc_feat_size),
                                         dtype=self.compute_dtype, drop_p=self.drop_prob_lm, use_bn=self.use_bn,
                                         logit_layers=self.logit_layers)
        if self.use_bn:      # buffers may have been re-homed by .cuda()/.to(): always hand the live tensors over
            self._engine.buffers = {k: v for k, v in self.named_buffers() if k.endswith(("running_mean", "running_var"))}
        return self._engine

    @property
    def param_names(self):
        return [k for _, k, is_param in _lib.weight_fields(self.use_bn, self.logit_layers) if is_param]

    def _bn_count_batch(self):
        """num_batches_tracked += 1, as a train-mode nn.BatchNorm1d forward does."""
        if self.use_bn and self.training:
            for m in self.att_embed:
                if isinstance(m, nn.BatchNorm1d):
                    m.num_batches_tracked += 1

    def state_dict(self, *args, **kwargs):
        """The reference's checkpoint contract.  Under the sharded data-parallel exchange with bf16 operands a rank's f32 masters
        are current only inside its own shard between steps: Trainer.gather_masters() (a collective) makes them whole again, and
        this call refuses to hand out a stale mixture."""
        stale = getattr(self, '_stale_masters', None)
        if stale is not None and stale():
            raise RuntimeError("state_dict(): this rank's f32 master weights are current only inside its own shard (sharded bf16 exchange); "
                               "call Trainer.gather_masters() -- or save_models() -- on EVERY rank first")
        return super(AttModel, self).state_dict(*args, **kwargs)

    def param_dict(self):
        sd = dict(self.named_parameters())
        return {k: sd[k] for k in self.param_names}

    def next_seed(self):
        self._seed_counter = (self._seed_counter * 1103515245 + 12345) & 0x7FFFFFFF
        return self._seed_counter

    def init_hidden(self, bsz):
        weight = next(self.parameters())
        return (weight.new_zeros(self.num_layers, bsz, self.rnn_size),
                weight.new_zeros(self.num_layers, bsz, self.rnn_size))

    @staticmethod
    def _steps_to_run(seq):
        """Early break of AttModel._forward (:148-151): stop at the first all-zero column i >= 1."""
        T = seq.size(1) - 1
        zero_cols = (seq[:, 1:T].sum(0) == 0).nonzero()
        return int(zero_cols[0].item()) + 1 if zero_cols.numel() else T

    # ------------------------------------------------------------------ reference call surface
    def _forward(self, fc_feats, attri_feats, att_feats, seq, att_masks=None):
        t_run = self._steps_to_run(seq)
        self._bn_count_batch()
        fc = fc_feats.contiguous().float()
        att = att_feats.contiguous().float()
        am = att_masks.contiguous().float() if att_masks is not None else None
        params = [self.param_dict()[k] for k in self.param_names]
        return _TopDownForward.apply(self, fc, att, seq.contiguous(), am, t_run, *params)

    def clip_att(self, att_feats, att_masks):
        """P/models/AttModel.py:99-105: clip the region axis to the longest row of att_masks."""
        if att_masks is not None:
            max_len = int(att_masks.long().sum(1).max())
            att_feats = att_feats[:, :max_len].contiguous()
            att_masks = att_masks[:, :max_len].contiguous()
        return att_feats, att_masks

    def _prepare_feature(self, fc_feats, att_feats, att_masks):
        """P/models/AttModel.py:107-117 -> (fc', att', p_att, att_masks), f32 device tensors (no autograd: this is the
        decode-time call of beam search / ensembles; training goes through _forward)."""
        att_feats, att_masks = self.clip_att(att_feats, att_masks)
        fc = fc_feats.contiguous().float()
        att = att_feats.contiguous().float()
        am = att_masks.contiguous().float() if att_masks is not None else None
        with torch.no_grad():
            pd = {k: v.detach() for k, v in self.param_dict().items()}
            self._bn_count_batch()
            fc_p, att_p, p_att = self.engine.prepare_feature(pd, fc, att, am, training=self.training,
                                                             seed=self.next_seed() if self.training else 0)
        return fc_p, att_p, p_att, am

    def get_logprobs_state(self, it, fc_feats, att_feats, p_att_feats, att_masks, state, t=0):
        """P/models/AttModel.py:158-165: one decode step from prepared features -> (log-probs [N, V+1], new state);
        state = (h [2, N, H], c [2, N, H]) stacked (att_lstm, lang_lstm) as TopDownCore returns it (:445)."""
        with torch.no_grad():
            pd = {k: v.detach() for k, v in self.param_dict().items()}
            am = att_masks.contiguous().float() if att_masks is not None else None
            logp, h, c = self.engine.logprobs_state(pd, it.contiguous().long(), fc_feats.contiguous().float(), att_feats.contiguous().float(),
                                                    p_att_feats.contiguous().float(), am, state[0].contiguous().float(),
                                                    state[1].contiguous().float(), t=t, training=self.training,
                                                    seed=self._seed_counter if self.training else 0)
        return logp, (h, c)

    def _sample_beam(self, fc_feats, att_feats, att_masks=None, opt={}):
        """AttModel._sample_beam (P/models/AttModel.py:167-196) over CaptionModel.beam_search (P/models/CaptionModel.py:
        33-177): all images in one device pass.  `self.done_beams[k]` is the reference's list for image k: its finished
        beams sorted by -p (stable), the first beam_size of them (CaptionModel.done_beams)."""
        beam_size = self._effective_beam_size(opt)
        if self.training:
            raise NotImplementedError("beam search runs in eval mode (eval_utils.eval_split calls model.eval() first)")
        assert beam_size <= self.vocab_size + 1
        fc = fc_feats.contiguous().float()
        att = att_feats.contiguous().float()
        am = att_masks.contiguous().float() if att_masks is not None else None
        with torch.no_grad():
            pd = {k: v.detach() for k, v in self.param_dict().items()}
            seq, lp, lists = self.engine.sample_beam(pd, fc, att, am, self.seq_length, beam_size, opt.get('decoding_constraint', 0),
                                                     opt.get('max_ppl', 0), done_lists=True)
        self._set_done_raw(*lists, beam_size)
        return seq, lp

    def _sample(self, fc_feats, attri_feats, att_feats, att_masks=None, opt={}):
        sample_max = opt.get('sample_max', 1)
        beam_size = opt.get('beam_size', 1)
        temperature = opt.get('temperature', 1.0)
        decoding_constraint = opt.get('decoding_constraint', 0)
        if beam_size > 1:
            return self._sample_beam(fc_feats, att_feats, att_masks, opt)
        self._bn_count_batch()
        fc = fc_feats.contiguous().float()
        att = att_feats.contiguous().float()
        am = att_masks.contiguous().float() if att_masks is not None else None
        # opt['captions_per_image'] = S > 1 (extension; not 'seq_per_img': callers pass all of vars(opt) as eval_kwargs, P/train.py): features come once per image, S captions are decoded per image
        kw = dict(sample_max=sample_max, temperature=temperature, decoding_constraint=decoding_constraint,
                  forced=opt.get('forced_tokens'), seq_per_img=int(opt.get('captions_per_image', 1) or 1))
        if torch.is_grad_enabled() and not sample_max:
            params = [self.param_dict()[k] for k in self.param_names]
            return _TopDownSample.apply(self, fc, att, am, kw, *params)
        with torch.no_grad():
            pd = {k: v.detach() for k, v in self.param_dict().items()}
            out = self.engine.sample(pd, fc, att, am, self.seq_length, seed=self.next_seed(), training=self.training, **kw)
        # A lone decode pass is ONE persistent launch (csrc/rnn_persist.hip) whose bounded spin gives up if its workgroups
        # cannot all become resident (another process on the GPU): the library then poisons the captions (token -1, log-prob
        # NaN) and sets the status word.  Callers of this path read the captions back at once (eval_utils.eval_split), so the
        # word is checked HERE -- one 16-byte read-back -- and a time-out raises at the call that suffered it.
        # `defer_status_check = True`: the caller checks at its own host sync (Trainer's self-critical step, timing loops).
        if not getattr(self, 'defer_status_check', False):
            _lib.persistent_status(out[0].device)
        return out


class TopDownModel(AttModel):
    def __init__(self, opt):
        super(TopDownModel, self).__init__(opt)
        self.num_layers = 2
        self.core = TopDownCore(opt)


# ---------------------------------------------------------------------------------------------------------------- AdaAtt
class AdaAtt_lstm(nn.Module):
    """P/models/AttModel.py:256-283: parameters only."""

    def __init__(self, opt, use_maxout=True):
        super(AdaAtt_lstm, self).__init__()
        self.use_maxout = use_maxout
        self.num_layers = opt.num_layers
        G = (4 + (use_maxout == True)) * opt.rnn_size       # noqa: E712 (the reference's expression)
        self.w2h = nn.Linear(opt.input_encoding_size, G)
        self.v2h = nn.Linear(opt.rnn_size, G)
        self.i2h = nn.ModuleList([nn.Linear(opt.rnn_size, G) for _ in range(self.num_layers - 1)])
        self.h2h = nn.ModuleList([nn.Linear(opt.rnn_size, G) for _ in range(self.num_layers)])
        if self.num_layers == 1:
            self.r_w2h = nn.Linear(opt.input_encoding_size, opt.rnn_size)
            self.r_v2h = nn.Linear(opt.rnn_size, opt.rnn_size)
        else:
            self.r_i2h = nn.Linear(opt.rnn_size, opt.rnn_size)
        self.r_h2h = nn.Linear(opt.rnn_size, opt.rnn_size)


class AdaAtt_attention(nn.Module):
    """P/models/AttModel.py:344-368: parameters only."""

    def __init__(self, opt):
        super(AdaAtt_attention, self).__init__()
        self.fr_linear = nn.Sequential(nn.Linear(opt.rnn_size, opt.input_encoding_size), nn.ReLU(), nn.Dropout(opt.drop_prob_lm))
        self.fr_embed = nn.Linear(opt.input_encoding_size, opt.att_hid_size)
        self.ho_linear = nn.Sequential(nn.Linear(opt.rnn_size, opt.input_encoding_size), nn.Tanh(), nn.Dropout(opt.drop_prob_lm))
        self.ho_embed = nn.Linear(opt.input_encoding_size, opt.att_hid_size)
        self.alpha_net = nn.Linear(opt.att_hid_size, 1)
        self.att2h = nn.Linear(opt.rnn_size, opt.rnn_size)


class AdaAttCore(nn.Module):
    def __init__(self, opt, use_maxout=False):
        super(AdaAttCore, self).__init__()
        self.lstm = AdaAtt_lstm(opt, use_maxout)
        self.attention = AdaAtt_attention(opt)


class AdaAttModel(AttModel):
    """The adaptive-attention captioner (P/models/AttModel.py:657-660) computed by csrc/adaatt.hip -- evaluation and decoding only;
    training is not built.  There is no eager fallback: without the HIP library, or on a CPU tensor, every call raises."""
    eval_only = True            # Trainer refuses to build a training run around it
    supports_grad_sink = False
    use_maxout = False
    _TRAINING = "%s: evaluation and decoding only; training is not built (call model.eval())"

    def __init__(self, opt):
        name = type(self).__name__
        E, H, A = opt.input_encoding_size, opt.rnn_size, opt.att_hid_size
        if not E == H == A:
            # AdaAtt_attention.forward views fr_embed's output with input_encoding_size and cats it with p_att_feats (:385-386), and
            # adds h_out_linear [input_encoding_size] to the attended features [rnn_size] (:402): the reference fails at its first forward
            raise NotImplementedError("%s: input_encoding_size=%r, rnn_size=%r and att_hid_size=%r must all be equal (the reference's "
                                      "AdaAtt_attention fails at its first forward otherwise)" % (name, E, H, A))
        if H % 8:
            raise NotImplementedError("%s: rnn_size=%r must be a multiple of 8 (the GEMM operands are read in 16-byte pieces)" % (name, H))
        if not 1 <= opt.num_layers <= _lib.ADAATT_MAX_LAYERS:
            raise NotImplementedError("%s: num_layers=%r: the MI355X path supports 1..%d" % (name, opt.num_layers, _lib.ADAATT_MAX_LAYERS))
        super(AdaAttModel, self).__init__(opt)
        self.core = AdaAttCore(opt, self.use_maxout)
        self._ws = None
        self._padded = self._padded_key = None

    # ------------------------------------------------------------------ engine plumbing
    @property
    def engine(self):
        # (AttributeError: `getattr(model, 'engine', None)` is how Trainer and eval_utils ask whether a model has one)
        raise AttributeError("%s has no TopDownEngine: it is computed by the uic_adaatt_* sequencers (csrc/adaatt.hip)" % type(self).__name__)

    @property
    def param_names(self):
        return [k for k, _ in self.named_parameters()]

    @property
    def _D8(self):
        """att_feat_size rounded up to a multiple of 8 (2053 with the reference's default use_box = 1): the features and att_embed's
        input side are zero-padded up to it, as in TransformerModel."""
        return (self.att_feat_size + 7) // 8 * 8

    @property
    def _Dfc8(self):
        return (self.fc_feat_size + 7) // 8 * 8

    def _dims(self, N, R, beam=1):
        return _lib.AdaAttDims(N=N, R=R, D=self._D8, Dfc=self._Dfc8, H=self.rnn_size, V1=self.vocab_size + 1, S=self.seq_length + 2,
                               layers=self.num_layers, maxout=int(self.use_maxout), logit_layers=self.logit_layers, use_bn=self.use_bn,
                               dtype=_lib.dtype_id(self.compute_dtype), beam=beam)

    def _tensors(self):
        sd = dict(self.named_parameters())
        sd.update(dict(self.named_buffers()))
        t = {k: sd[k].detach() for _, _, k in _lib.adaatt_weight_keys(self.num_layers, self.use_bn, self.logit_layers)}
        fills = {}
        if self._D8 != self.att_feat_size:
            # zero columns on the Linear; on BatchNorm1d(D) the identity (gamma 1, beta 0, mean 0, var 1) over zero features: nothing added
            fills["att_embed.%d.weight" % (1 if self.use_bn else 0)] = (self._D8 - self.att_feat_size, 0.0)
            if self.use_bn:
                for k, v in (("weight", 1.0), ("bias", 0.0), ("running_mean", 0.0), ("running_var", 1.0)):
                    fills["att_embed.0." + k] = (self._D8 - self.att_feat_size, v)
        if self._Dfc8 != self.fc_feat_size:
            fills["fc_embed.0.weight"] = (self._Dfc8 - self.fc_feat_size, 0.0)
        if fills:
            key = tuple((t[k].data_ptr(), t[k]._version) for k in fills)
            if self._padded_key != key:
                self._padded = {k: F.pad(t[k], (0, extra), value=v).contiguous() for k, (extra, v) in fills.items()}
                self._padded_key = key
            t.update(self._padded)
        return t

    def _prepare(self, fc_feats, att_feats, att_masks, beam=1):
        """(lib, dims, weights, workspace, fc, att, masks) for one call: the region axis clipped (clip_att), the features zero-padded
        to multiples of 8 columns, a workspace of the call's size."""
        if self.training:
            raise NotImplementedError(self._TRAINING % type(self).__name__)
        lib = _lib.load()
        att_feats, att_masks = self.clip_att(att_feats, att_masks)
        if att_feats.shape[-1] != self.att_feat_size or fc_feats.shape[-1] != self.fc_feat_size:
            raise ValueError("features have %d / %d columns, opt.fc_feat_size / att_feat_size are %d / %d"
                             % (fc_feats.shape[-1], att_feats.shape[-1], self.fc_feat_size, self.att_feat_size))
        fc = F.pad(fc_feats.float(), (0, self._Dfc8 - self.fc_feat_size)).contiguous()
        att = F.pad(att_feats.float(), (0, self._D8 - self.att_feat_size)).contiguous()
        am = att_masks.contiguous().float() if att_masks is not None else None
        if not att.is_cuda or not fc.is_cuda:
            raise RuntimeError("%s needs device tensors; got a %s tensor (there is no CPU fallback)" % (type(self).__name__, att.device))
        d = self._dims(att.shape[0], att.shape[1], beam)
        if _lib.adaatt_attention_lds_bytes(d.R, d.H, d.H) > _lib.LDS_BYTES:
            raise NotImplementedError("%d regions at rnn_size %d: uic_adaatt_attention_fwd keeps a row's scores and partial sums in LDS (160 KB)"
                                      % (d.R, d.H))
        w = _lib.adaatt_weights(self._tensors(), self.num_layers, self.use_bn, self.logit_layers)
        return lib, d, w, self._workspace(lib, d, att.device), fc, att, am

    def _workspace(self, lib, d, device):
        nbytes = lib.uic_adaatt_workspace_bytes(C.byref(d))
        if nbytes == 0:
            check(-1, "adaatt_workspace_bytes")
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return self._ws

    # ------------------------------------------------------------------ reference call surface
    def _forward(self, fc_feats, attri_feats, att_feats, seq, att_masks=None):
        """P/models/AttModel.py:119-156 in eval mode: log-probs [N, seq.size(1) - 1, V + 1]; the steps behind the early break are zeros."""
        with torch.no_grad():
            if seq.shape[0] != fc_feats.shape[0]:
                # features once per image, seq_per_img caption rows per image (the loader's validation batches): one row per caption
                S = seq.shape[0] // fc_feats.shape[0]
                fc_feats, att_feats = fc_feats.repeat_interleave(S, 0), att_feats.repeat_interleave(S, 0)
                att_masks = att_masks.repeat_interleave(S, 0) if att_masks is not None else None
            lib, d, w, ws, fc, att, am = self._prepare(fc_feats, att_feats, att_masks)
            seq = seq.contiguous().long()
            Tq = seq.shape[1] - 1
            if not 1 <= Tq <= d.S - 1:
                raise ValueError("seq has %d columns; the model scores 2..%d (seq_length + 2)" % (seq.shape[1], d.S))
            logp = torch.zeros(d.N, Tq, d.V1, dtype=torch.float32, device=att.device)
            check(lib.uic_adaatt_forward(C.byref(d), C.byref(w), ptr(fc), ptr(att), ptr(am), ptr(seq), seq.shape[1], Tq, self._steps_to_run(seq),
                                         ptr(ws), ptr(logp), stream()), "adaatt_forward")
        return logp

    def _prepare_feature(self, fc_feats, att_feats, att_masks):
        """P/models/AttModel.py:107-117 -> (fc', att', p_att, att_masks), f32 device tensors."""
        with torch.no_grad():
            lib, d, w, ws, fc, att, am = self._prepare(fc_feats, att_feats, att_masks)
            H = self.rnn_size
            fc_p = torch.empty(d.N, H, dtype=torch.float32, device=att.device)
            att_p = torch.empty(d.N, d.R, H, dtype=torch.float32, device=att.device)
            p_att = torch.empty(d.N, d.R, H, dtype=torch.float32, device=att.device)
            check(lib.uic_adaatt_prepare_feature(C.byref(d), C.byref(w), ptr(fc), ptr(att), ptr(am), ptr(ws), ptr(fc_p), ptr(att_p), ptr(p_att),
                                                 stream()), "adaatt_prepare_feature")
        return fc_p, att_p, p_att, am

    def get_logprobs_state(self, it, fc_feats, att_feats, p_att_feats, att_masks, state, t=0):
        """P/models/AttModel.py:158-165: one decode step from prepared features -> (log-probs [N, V+1], new state);
        state = (h, c), each [num_layers, N, H].  (`t` only numbers the dropout draws of a TopDown training step; unused here.)"""
        if self.training:
            raise NotImplementedError(self._TRAINING % type(self).__name__)
        with torch.no_grad():
            lib = _lib.load()
            fc, att, p_att = fc_feats.contiguous().float(), att_feats.contiguous().float(), p_att_feats.contiguous().float()
            am = att_masks.contiguous().float() if att_masks is not None else None
            if not att.is_cuda:
                raise RuntimeError("%s needs device tensors; got a %s tensor (there is no CPU fallback)" % (type(self).__name__, att.device))
            N, R, H = att.shape[0], att.shape[1], self.rnn_size
            d = self._dims(N, R)
            w = _lib.adaatt_weights(self._tensors(), self.num_layers, self.use_bn, self.logit_layers)
            ws = self._workspace(lib, d, att.device)
            h_in, c_in = state[0].contiguous().float(), state[1].contiguous().float()
            logp = torch.empty(N, d.V1, dtype=torch.float32, device=att.device)
            h, c = torch.empty_like(h_in), torch.empty_like(c_in)
            check(lib.uic_adaatt_logprobs_state(C.byref(d), C.byref(w), ptr(it.contiguous().long()), ptr(fc), ptr(att), ptr(p_att), ptr(am),
                                                ptr(h_in), ptr(c_in), ptr(ws), ptr(logp), ptr(h), ptr(c), stream()), "adaatt_logprobs_state")
        return logp, (h, c)

    def _sample_beam(self, fc_feats, att_feats, att_masks=None, opt={}):
        """AttModel._sample_beam (:167-196) over CaptionModel.beam_search, all images in one device pass; `self.done_beams[k]` is the
        reference's list for image k (built on first access)."""
        beam_size = self._effective_beam_size(opt)
        if not 1 <= beam_size <= _lib.BEAM_MAX:
            raise NotImplementedError("beam_size=%r: the MI355X beam kernels hold 1..%d beams" % (beam_size, _lib.BEAM_MAX))
        assert beam_size <= self.vocab_size + 1
        with torch.no_grad():
            lib, d, w, ws, fc, att, am = self._prepare(fc_feats, att_feats, att_masks, beam=int(beam_size))
            L, n_img, B = self.seq_length, d.N, int(beam_size)
            seq = torch.zeros(n_img, L, dtype=torch.int64, device=att.device)
            lp = torch.zeros(n_img, L, dtype=torch.float32, device=att.device)
            check(lib.uic_adaatt_sample_beam(C.byref(d), C.byref(w), ptr(fc), ptr(att), ptr(am), L, B, int(opt.get('decoding_constraint', 0)),
                                             int(opt.get('max_ppl', 0)), ptr(ws), ptr(seq), ptr(lp), stream()), "adaatt_sample_beam")
            lists = _lib.done_list_buffers(n_img, L, B, att.device)
            check(lib.uic_adaatt_beam_done_lists(C.byref(d), ptr(ws), L, B, *[ptr(x) for x in lists], stream()), "adaatt_beam_done_lists")
        self._set_done_raw(*lists, B)
        return seq, lp

    def _sample(self, fc_feats, attri_feats, att_feats, att_masks=None, opt={}):
        """P/models/AttModel.py:198-253: (seq, seqLogprobs), both [N, seq_length]."""
        if self.training:
            raise NotImplementedError(self._TRAINING % type(self).__name__)
        if int(opt.get('captions_per_image', 1) or 1) > 1 or opt.get('forced_tokens') is not None:
            raise NotImplementedError("%s._sample: opt['captions_per_image'] > 1 and opt['forced_tokens'] are extensions of the TopDown "
                                      "training path" % type(self).__name__)
        if opt.get('beam_size', 1) > 1:
            return self._sample_beam(fc_feats, att_feats, att_masks, opt)
        with torch.no_grad():
            lib, d, w, ws, fc, att, am = self._prepare(fc_feats, att_feats, att_masks)
            L = self.seq_length
            seq = torch.zeros(d.N, L, dtype=torch.int64, device=att.device)
            lp = torch.zeros(d.N, L, dtype=torch.float32, device=att.device)
            check(lib.uic_adaatt_sample(C.byref(d), C.byref(w), ptr(fc), ptr(att), ptr(am), L, int(bool(opt.get('sample_max', 1))),
                                        float(opt.get('temperature', 1.0)), int(opt.get('decoding_constraint', 0)), self.next_seed(), ptr(ws),
                                        ptr(seq), ptr(lp), stream()), "adaatt_sample")
        return seq, lp


class AdaAttMOModel(AdaAttModel):
    """AdaAtt with the maxout LSTM (P/models/AttModel.py:663-667)."""
    use_maxout = True
