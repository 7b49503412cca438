#!/usr/bin/env python3
"""BASELINE config 1 (the reference's own CPU-runnable case): FC caption model (FCModel_NMT + maxout LSTMCore) on 2048-d fc
features, 16 images x 5 captions = 80 rows, seq_len 16, hidden 512, V + 1 = 9 488.

Three things are timed, GPU in bf16 and f32:
  * the model-call step: forward (dense log-probs like the reference) + LanguageModelCriterion + backward + torch Adam, and
    beside it the CPU oracle (oracle/fc.py, results-identical restatement of the reference) on this host (--skip-cpu: not);
  * the Trainer's XE step (Trainer.train_device_batch: uic_fc_xe_train_step into the flat arena + the arena's optimizer launch)
    against the only way to take that step without it -- model(...), LanguageModelCriterion, loss.backward(), p.grad copied into
    the arena, the arena's optimizer launch -- in the same process, ALTERNATING: new, old, new again.  The two series of the new
    step are the same code: the distance between their medians is the spread a difference has to exceed;
  * the Trainer's self-critical step (Trainer.train_self_critical with the device CIDEr-D scorer on cached document
    frequencies, one host sync per step).
HIP events around blocks of --inner steps after a warm-up, medians of --reps blocks, at config 1's batch (16 x 5 rows) and at
train.sh's (50 x 5 rows).  --out FILE: the report is also written there (profiles/fc_trainer_bench.txt)."""
import argparse, os, pickle, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from unpaired_image_captioning_amd import models
from unpaired_image_captioning_amd.misc.criterion import LanguageModelCriterion

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=16); ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--cpu-threads", type=int, default=16)
ap.add_argument("--skip-cpu", action="store_true"); ap.add_argument("--skip-model-call", action="store_true")
ap.add_argument("--reps", type=int, default=10); ap.add_argument("--inner", type=int, default=10); ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()
V, E, H, D, L, S = 9487, 512, 512, 2048, 16, 5
from oracle import fc as OF, topdown as O
assert torch.cuda.is_available(), "fc_bench measures on the GPU"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def fc_opt(dtype, **kw):
    return argparse.Namespace(vocab_size=V, input_encoding_size=E, rnn_type="LSTM", rnn_size=H, num_layers=1, drop_prob_lm=0.5,
                              seq_length=L, fc_feat_size=D, caption_model="fc", compute_dtype=dtype, **kw)


b = O.synthetic_batch(a.images, S, 3, D, V, L, seed=3)
N = a.images * S
for dtype in ("bf16", "f32"):
    if a.skip_model_call:
        break
    torch.manual_seed(1)
    m = models.setup(fc_opt(dtype)).cuda().train()
    optim = torch.optim.Adam(m.parameters(), lr=5e-4)
    fc, labels, masks = b["fc_feats"].cuda(), b["labels"].cuda(), b["masks"].cuda()
    crit = LanguageModelCriterion()

    def step():
        optim.zero_grad(set_to_none=True)
        loss = crit(m(fc, None, None, labels, None), labels[:, 1:], masks[:, 1:])
        loss.backward()
        optim.step()
        return loss
    for _ in range(5):
        step()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(a.steps):
        loss = step()
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / a.steps
    say("fc %s: %.3f ms/step, %.0f captions/s (N=%d rows), loss %.3f" % (dtype, dt * 1e3, N / dt, N, loss.item()))


# ---------------------------------------------------------------------------------------------------- the Trainer's steps
def timed_block(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def trainer_bench(dtype, n_img):
    from unpaired_image_captioning_amd.misc import rewards
    from unpaired_image_captioning_amd.trainer import Trainer, _steps_from_host_labels
    rows = n_img * S
    bt = O.synthetic_batch(n_img, S, 3, D, V, L, seed=3)
    torch.manual_seed(1)
    tr = Trainer(fc_opt(dtype, seed=1, i2t_learning_rate=5e-4, cached_tokens="corpus", cider_reward_weight=1.0, bleu_reward_weight=0.0))
    tr.build_optimizer()
    model, arena = tr.i2t_model, tr.arena
    data = {k: bt[k].numpy() for k in ("fc_feats", "labels", "masks")}
    data["gts"] = [data["labels"][i * S:(i + 1) * S, 1:L + 1] for i in range(n_img)]
    # cached document frequencies, as the reference's workflow has them (--cached_tokens, scripts/prepro_ngrams.py): the table is
    # uploaded once, the scorer then works on the device ('corpus' would rebuild it on the host from every batch)
    df = {}
    for img in data["gts"]:
        grams = set()
        for r in img:
            w = rewards.DeviceCiderD._words(r)
            for k in range(1, 5):
                for i in range(len(w) - k + 1):
                    grams.add(tuple(str(t) for t in w[i:i + k]))
        for ng in grams:
            df[ng] = df.get(ng, 0.0) + 1.0
    pk = os.path.join(tempfile.gettempdir(), "uic_fc_bench-idxs-%d.p" % n_img)
    with open(pk, "wb") as f:
        pickle.dump({"document_frequency": df, "ref_len": float(n_img)}, f)
    tr.opt.cached_tokens = pk
    batch = {k: bt[k].cuda() for k in ("fc_feats", "labels", "masks")}
    t_run = _steps_from_host_labels(data["labels"])
    den = float(data["masks"][:, 1:].sum())
    crit = LanguageModelCriterion()
    params = dict(model.named_parameters())
    fc, labels, masks = batch["fc_feats"], batch["labels"], batch["masks"]

    def new_step():
        tr.train_device_batch(batch, t_run, den)

    def old_step():
        for p in params.values():
            p.grad = None
        loss = crit(model(fc, None, None, labels, None), labels[:, 1:], masks[:, 1:])
        loss.backward()
        for k, view in arena.grad_views.items():
            view.copy_(params[k].grad)
        tr._guarded_adam(loss.detach(), 1.0)

    for _ in range(a.warmup):
        new_step(); old_step()
    torch.cuda.synchronize()
    new1, old, new2 = [], [], []
    for _ in range(a.reps):
        new1.append(timed_block(new_step, a.inner))
        old.append(timed_block(old_step, a.inner))
        new2.append(timed_block(new_step, a.inner))
    m1, mo, m2 = statistics.median(new1), statistics.median(old), statistics.median(new2)
    spread = abs(m1 - m2)
    say("fc %s %d x %d rows  Trainer XE step %.3f ms (second series of the same code %.3f ms: spread %.3f ms; blocks %.3f .. %.3f) | "
        "model call + criterion + backward + grad copy + arena optimizer %.3f ms (blocks %.3f .. %.3f) | %.0f captions/s | %s"
        % (dtype, n_img, S, m1, m2, spread, min(new1 + new2), max(new1 + new2), mo, min(old), max(old), rows / (min(m1, m2) * 1e-3),
           "not slower" if min(m1, m2) <= mo + spread else "SLOWER"))
    rewards.CiderD_scorer = None
    for _ in range(3):
        tr.train_self_critical(data)
    sc = [timed_block(lambda: tr.train_self_critical(data), 3) for _ in range(a.reps)]
    rewards.CiderD_scorer = None
    say("fc %s %d x %d rows  Trainer self-critical step (sampling pass + greedy baseline + CIDEr-D on cached document frequencies + backward + optimizer, one host sync) "
        "%.3f ms (blocks %.3f .. %.3f), loss %.4f, avg reward %.4f"
        % (dtype, n_img, S, statistics.median(sc), min(sc), max(sc), tr.i2t_train_loss, tr.i2t_avg_reward))


say("# Trainer steps of caption_model='fc': HIP events, warm-up %d, medians of %d blocks of %d steps (self-critical: 3), L %d, %d-d, H %d, V %d"
    % (a.warmup, a.reps, a.inner, L, D, H, V))
for n_img in (16, 50):
    for dtype in ("bf16", "f32"):
        trainer_bench(dtype, n_img)

if not a.skip_cpu:
    torch.set_num_threads(a.cpu_threads)
    W = OF.init_weights(V + 1, E, H, D, seed=1)
    Wp = {k: v.clone().requires_grad_(True) for k, v in W.items()}
    opt_c = torch.optim.Adam(list(Wp.values()), lr=5e-4)
    g = torch.Generator().manual_seed(0)

    def cpu_step():
        opt_c.zero_grad(set_to_none=True)
        drop = dict(out=(torch.rand(L + 2, N, H, generator=g) >= 0.5).float() * 2.0)      # dropout 0.5 on next_h (FCModel_NMT.py:47-50)
        loss, grads, _ = OF.xe_loss_and_grads({k: v.detach() for k, v in Wp.items()}, b["fc_feats"], b["labels"], b["masks"], drop)
        for k, v in Wp.items():
            v.grad = grads[k]
        opt_c.step()
        return loss

    cpu_step(); t0 = time.perf_counter()
    for _ in range(5):
        cpu_step()
    dt = (time.perf_counter() - t0) / 5
    say("fc CPU oracle (%d threads): %.1f ms/step, %.0f captions/s" % (a.cpu_threads, dt * 1e3, N / dt))

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
