"""`models.setup(opt)` with the reference's dispatch (P/models/__init__.py:22-58), restricted to
the architectures on the hot path."""
from .AttModel import TopDownModel, AdaAttModel, AdaAttMOModel  # noqa: F401
from .AttEnsemble import AttEnsemble  # noqa: F401
from .CaptionModel import CaptionModel  # noqa: F401
from .FCModel_NMT import FCModel_NMT  # noqa: F401
from . import NMT_Models  # noqa: F401
from .Discriminator import SentenceDiscriminator  # noqa: F401
from .GCN import SceneGraphEncoder  # noqa: F401
from .TransformerModel import TransformerModel  # noqa: F401


def setup(opt):
    if opt.caption_model == 'fc':
        return FCModel_NMT(opt)          # P/models/__init__.py:24-26
    if opt.caption_model == 'topdown':
        return TopDownModel(opt)
    if opt.caption_model == 'transformer':            # P/models/__init__.py:52-53
        # evaluation and decoding only.  Options that ask for a training run of it (opts.py's defaults: i2t_train_flag = 1) are
        # refused HERE, before anything is allocated; an opt without the flag (eval scripts, tests) or with 0 builds the model.
        if getattr(opt, 'i2t_train_flag', 0):
            raise NotImplementedError("Caption model not supported by the MI355X hot path: transformer with i2t_train_flag=%r -- evaluation "
                                      "and decoding only; training is not built (set i2t_train_flag=0 to load, score and decode a checkpoint)"
                                      % (opt.i2t_train_flag,))
        return TransformerModel(opt)
    if opt.caption_model in ('adaatt', 'adaattmo'):   # P/models/__init__.py:36-41
        # evaluation and decoding only, as the transformer
        if getattr(opt, 'i2t_train_flag', 0):
            raise NotImplementedError("Caption model not supported by the MI355X hot path: %s with i2t_train_flag=%r -- evaluation "
                                      "and decoding only; training is not built (set i2t_train_flag=0 to load, score and decode a checkpoint)"
                                      % (opt.caption_model, opt.i2t_train_flag))
        return AdaAttModel(opt) if opt.caption_model == 'adaatt' else AdaAttMOModel(opt)
    raise Exception("Caption model not supported by the MI355X hot path: {}".format(opt.caption_model))
