"""The validation pass of the captioner (P/eval_utils.py): `eval_split` -- the teacher-forced loss of every batch of the split
and one decoded caption per image -- and `language_eval`, the `lang_stats` the trainer picks its '-best' checkpoint by.

MI355X-first differences: the per-batch losses and the decoded token rows stay on the device until the pass is over (one
read-back each), and the captions are scored there (misc/lang_eval.py) on token ids instead of being written to a json file
for the python / Java scorers.  `eval_split_coco_unpaired` is the unpaired pass: the same paired half, then pivot caption ->
translator -> English rows scored against the COCO loader's references, joined on the device by misc/pivot.py.  Not carried
over: `coco_eval_flag` inside eval_split / Trainer.eval (call eval_split_coco_unpaired / Trainer.eval_unpaired), `dump_images`,
and the 'coco' / '30k' branches of language_eval, whose PTB tokenizer, METEOR and SPICE are Java.
"""
import numpy as np
import torch

from .misc import criterion
from .misc import utils
from .misc.lang_eval import DeviceLanguageEval


def language_eval(loader, split, image_ix, seq):
    """lang_stats of language_eval (P/eval_utils.py:26-86): {'Bleu_1'..'Bleu_4', 'ROUGE_L', 'CIDEr'} of the caption rows `seq`
    [n, L] (device int64, 0 = end) of the images `image_ix` (loader indices) against the split's label rows.  The scorer object --
    references on the device, document-frequency table -- is built at the first call and kept on the loader."""
    cache = loader.__dict__.setdefault('_lang_eval', {})
    if split not in cache:
        cache[split] = DeviceLanguageEval(loader, split, seq.device)
    return cache[split].score(image_ix, seq)[0]


def _refuse(opt, eval_kwargs, coco_ok=False):
    """What neither validation pass does."""
    if getattr(opt, 'coco_eval_flag', 0) and not coco_ok:
        raise NotImplementedError("coco_eval_flag (eval_split_coco_unpaired) is outside this port")
    if eval_kwargs.get('dump_images', 0) == 1:
        raise NotImplementedError("dump_images is outside this port")
    if getattr(opt, 'nmt_eval_flag', 0):
        raise NotImplementedError("the NMT half of the validation pass is Trainer.eval_nmt(batches)")
    input_json = str(getattr(opt, 'input_json', ''))
    if eval_kwargs.get('language_eval', 0) == 1 and ('coco' in input_json or '30k' in input_json):
        raise NotImplementedError("the 'coco' / '30k' annotation paths of language_eval (PTB tokenizer, METEOR, SPICE: Java) are "
                                  "outside this port; misc.lang_eval.DeviceLanguageEval scores token ids with Bleu(4), Rouge(), Cider()")


def _decode_split(opt, loader, i2t_model, eval_kwargs, with_loss=True, vocab=None):
    """One pass over the split of `loader` (i2t_model in eval mode): the teacher-forced loss of every batch (with_loss) and one
    decoded caption per image (`vocab`: the captioner's ix_to_word where it is not the loader's, for the beam print-out).
    Returns (val_loss, seq [n, L] device rows, infos): the first min(it_max, num_images) images of the split's iteration order,
    each once."""
    verbose = eval_kwargs.get('verbose', True)
    verbose_beam = eval_kwargs.get('verbose_beam', 1)
    verbose_loss = eval_kwargs.get('verbose_loss', 1)
    num_images = eval_kwargs.get('num_images', eval_kwargs.get('val_images_use', -1))
    split = eval_kwargs.get('split', 'val')
    beam_size = eval_kwargs.get('beam_size', 1)
    vocab = loader.get_vocab() if vocab is None else vocab
    i2t_crit = criterion.LanguageModelCriterion(opt)
    loader.reset_iterator(split)
    it_max = len(loader.split_ix[split])
    limit = it_max if num_images == -1 else min(it_max, num_images)
    wanted = set(int(ix) for ix in loader.split_ix[split][:limit])
    n = 0
    losses, seqs, rows, infos = [], [], [], []
    seen = set()
    while True:
        data = loader.get_batch(split)
        fc_feats, att_feats, att_masks = data['fc_feats'], data['att_feats'], data['att_masks']
        device = fc_feats.device
        with torch.no_grad():
            if with_loss and data.get('labels', None) is not None and verbose_loss:
                labels = torch.from_numpy(np.ascontiguousarray(data['labels'])).to(device)
                masks = torch.from_numpy(np.ascontiguousarray(data['masks'])).to(device)
                outputs = i2t_model(fc_feats, data['attri_feats'], att_feats, labels, att_masks)
                losses.append(i2t_crit(outputs, labels[:, 1:], masks[:, 1:]).detach().reshape(1))
            # one caption per image (the loader ships every image's features once)
            seq = i2t_model(fc_feats, data['attri_feats'], att_feats, att_masks, opt=eval_kwargs, mode='sample')[0]
        if beam_size > 1 and verbose_beam:
            for i in range(seq.shape[0]):
                print('\n'.join([utils.decode_sequence(vocab, _['seq'].unsqueeze(0))[0] for _ in i2t_model.done_beams[i]]))
                print('--' * 10)
        for k, info in enumerate(data['infos']):
            if info['ix'] in wanted and info['ix'] not in seen:
                seen.add(info['ix'])
                rows.append(n + k)
                infos.append(info)
        seqs.append(seq)
        n = n + seq.shape[0]
        if verbose:
            print('evaluating validation preformance... %d/%d' % (data['bounds']['it_pos_now'] - 1, limit))
        if data['bounds']['wrapped']:
            break
        if num_images >= 0 and n >= num_images:
            break

    seq = torch.cat(seqs, 0).index_select(0, torch.tensor(rows, dtype=torch.int64, device=seqs[0].device))
    loss_sum = 0
    for loss in (torch.cat(losses).cpu().tolist() if losses else []):      # the ONE read-back of the losses
        loss_sum = loss_sum + loss
    return loss_sum / (1e-8 + len(losses)), seq, infos


def _paired_half(opt, loader, i2t_model, eval_kwargs):
    """(val_loss, predictions, lang_stats) of `loader`'s split: the captioner scored in its own language."""
    verbose = eval_kwargs.get('verbose', True)
    split = eval_kwargs.get('split', 'val')
    val_loss, seq, infos = _decode_split(opt, loader, i2t_model, eval_kwargs)
    sents = utils.decode_sequence(loader.get_vocab(), seq)
    predictions = []
    for info, sent in zip(infos, sents):
        if verbose:
            print('image %s: ' % (info['id']), sent)
        entry = {'image_id': info['id'], 'caption': sent}
        if eval_kwargs.get('dump_path', 0) == 1:
            entry['file_name'] = info['file_path']
        predictions.append(entry)
    lang_stats = None
    if eval_kwargs.get('language_eval', 0) == 1:
        lang_stats = language_eval(loader, split, [info['ix'] for info in infos], seq)
    return val_loss, predictions, lang_stats


def eval_split(opt, loader, i2t_model, nmt_model, eval_kwargs={}):
    """eval_split, i2t branch (P/eval_utils.py:208-327) -> (val_loss, predictions, lang_stats, 0.0, 0.0).

    The reference drops the overshoot of the last batch by popping the tail of `predictions` (:287-292).  get_batch here returns
    a batch's images in the assembly kernel's order, not in iteration order, so the overshoot is dropped by IMAGE: the first
    min(it_max, num_images) images of the split's iteration order are kept, each once."""
    _refuse(opt, eval_kwargs)
    was_training = i2t_model.training
    i2t_model.eval()
    try:
        val_loss, predictions, lang_stats = _paired_half(opt, loader, i2t_model, eval_kwargs)
    finally:
        i2t_model.train(was_training)
    return val_loss, predictions, lang_stats, 0.0, 0.0


def eval_split_coco_unpaired(opt, loader, coco_loader, i2t_model, nmt_model, eval_kwargs={}):
    """eval_split_coco_unpaired (P/eval_utils.py:329-473) -> (val_loss, predictions, coco_predictions, lang_stats, coco_lang_stats,
    0.0, 0.0): the paired half is eval_split's on `loader`; the COCO half decodes one pivot caption per image of `coco_loader`'s
    split, translates it (eval_kwargs['pivot_bridge'].pivot: uic_pivot_source, uic_nmt_translate, uic_pivot_target) and scores the
    English rows against coco_loader's references on the device.  Between the decode and the scores the host waits only for each
    batch's max_len and for the translator's own stop checks; the words of coco_predictions are read back afterwards.

    Differences from the reference: the two loaders run as two passes, not in lock-step; the reference's
    string edits ("'s" -> "is", dropping "there is") never reach its own predictions (:410-430 appends the edited lists behind the
    unedited ones and reads the unedited ones), so they are not reproduced; the COCO images get the features the captioner uses
    (the reference feeds fc_feats only).  The NMT half of the validation pass is Trainer.eval_nmt."""
    bridge = eval_kwargs.get('pivot_bridge', None)
    if bridge is None:
        raise ValueError("eval_split_coco_unpaired needs eval_kwargs['pivot_bridge'] (misc.pivot.PivotBridge; Trainer.build_pivot)")
    _refuse(opt, eval_kwargs, coco_ok=True)
    verbose = eval_kwargs.get('verbose', True)
    split = eval_kwargs.get('split', 'val')
    i2t_training, nmt_training = i2t_model.training, nmt_model.training
    i2t_model.eval()
    nmt_model.eval()
    try:
        val_loss, predictions, lang_stats = _paired_half(opt, loader, i2t_model, eval_kwargs)
        _, seq, infos = _decode_split(opt, coco_loader, i2t_model, eval_kwargs, with_loss=False, vocab=loader.get_vocab())
        outs, kept = [], []
        step = max(1, int(getattr(coco_loader, 'batch_size', seq.shape[0])))
        for lo in range(0, seq.shape[0], step):                       # the reference translates batch by batch (:410)
            out, out_len, _ = bridge.pivot(seq[lo:lo + step], nmt_model, beam_size=eval_kwargs.get('nmt_beam_size', 15),
                                           max_steps=eval_kwargs.get('nmt_max_steps', 100))
            outs.append(out)
            kept.append((bridge.last['hyp'][:, :out.shape[1]], out_len, bridge.last['repl']))
        out = torch.cat(outs, 0)
        coco_lang_stats = None
        if eval_kwargs.get('language_eval', 0) == 1:
            coco_lang_stats = language_eval(coco_loader, split, [info['ix'] for info in infos], out)
        # the words, after the scores: one read-back
        width = out.shape[1]
        hyp = torch.cat([torch.nn.functional.pad(h, (0, width - h.shape[1])) for h, _, _ in kept], 0)
        sents = bridge.render(hyp, torch.cat([l for _, l, _ in kept]), torch.cat([r for _, _, r in kept], 0), seq)
        coco_predictions = []
        for info, sent in zip(infos, sents):
            if verbose:
                print('image %s | EN: %s' % (info['id'], sent))
            coco_predictions.append({'image_id': info['id'], 'caption': sent})
    finally:
        i2t_model.train(i2t_training)
        nmt_model.train(nmt_training)
    return val_loss, predictions, coco_predictions, lang_stats, coco_lang_stats, 0.0, 0.0
