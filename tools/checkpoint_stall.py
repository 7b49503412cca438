"""What a checkpoint costs the training loop: the benchmark's synthetic configuration (640 caption rows, bf16), a warmed
200-step loop timed with a host clock that ends in a device synchronise, in three variants that alternate and repeat in one
process: no save, Trainer.save_models every 50 steps, Trainer.save_models_async every 50 steps (skipped where the Trainer has
none).  Prints one JSON line: per variant the loop times, and per save the time added over the no-save loop of the same repeat.

    python tools/checkpoint_stall.py [--steps 200] [--every 50] [--repeats 3] [--out FILE]
"""
import argparse, gc, json, os, shutil, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from unpaired_image_captioning_amd import _lib as L
from unpaired_image_captioning_amd.synthetic import synthetic_batch
from unpaired_image_captioning_amd.trainer import Trainer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--every", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    c = bench.CFG
    torch.manual_seed(1234)
    opt = bench.make_opt("bf16", 1234, 0, c["D"])
    opt.checkpoint_path = tempfile.mkdtemp(prefix="uic_ckpt_")
    tr = Trainer(opt)
    tr.build_optimizer()
    batch = synthetic_batch(c["n_img"], c["S"], c["R"], c["D"], c["V"], c["L"], seed=1234)
    batch["fc_feats"] = batch["fc_feats"][:, :c["D"]].contiguous()
    t_run = tr.i2t_model._steps_to_run(batch["labels"])
    den = float(batch["masks"][:, 1:c["L"] + 2].sum().item())
    tr.attach_live(batch)
    variants = ["none", "sync"] + (["async"] if hasattr(tr, "save_models_async") else [])
    save = {"none": None, "sync": tr.save_models, "async": getattr(tr, "save_models_async", None)}

    def loop(variant):
        for _ in range(args.warmup):
            tr.train_device_batch(batch, t_run, den, den)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            tr.train_device_batch(batch, t_run, den, den)
            if save[variant] is not None and (i + 1) % args.every == 0:
                save[variant]()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        t1 = time.perf_counter()
        if hasattr(tr, "wait_for_save"):
            tr.wait_for_save()                 # (the last save's writer, outside the timed loop: reported as `drain_s`)
        L.persistent_status()                  # raises if a persistent launch of the loop timed out
        return el, time.perf_counter() - t1

    gc.collect()
    gc.freeze()
    for v in variants:                         # first saves allocate the snapshot and the pinned buffers: not timed
        if save[v] is not None:
            save[v]()
    loop("none")
    times = {v: [] for v in variants}
    drain = {v: [] for v in variants}
    for _ in range(args.repeats):
        for v in variants:
            el, dr = loop(v)
            times[v].append(el)
            drain[v].append(dr)
    n_saves = args.steps // args.every
    sizes = {f: os.path.getsize(os.path.join(opt.checkpoint_path, f)) for f in sorted(os.listdir(opt.checkpoint_path))}
    shutil.rmtree(opt.checkpoint_path, ignore_errors=True)
    out = {"steps": args.steps, "save_every": args.every, "saves_per_loop": n_saves, "repeats": args.repeats,
           "loop_s": {v: [round(x, 5) for x in t] for v, t in times.items()},
           "ms_per_step_no_save": [round(x / args.steps * 1e3, 4) for x in times["none"]],
           "no_save_spread_ms_per_loop": round((max(times["none"]) - min(times["none"])) * 1e3, 3),
           "added_ms_per_save": {v: [round((t - n) / n_saves * 1e3, 3) for t, n in zip(times[v], times["none"])] for v in variants if v != "none"},
           "drain_s": {v: [round(x, 4) for x in d] for v, d in drain.items() if v != "none"},
           "file_bytes": sizes, "final_loss": float(tr.last_loss.item())}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
