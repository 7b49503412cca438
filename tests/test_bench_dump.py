"""bench.py --dump-outputs DIR: what the timed path computed in its last timed step (loss, updated weights, gradients) as
DIR/<name>.npy in float32 / float64, at most 64 MB, large tensors as a fixed seeded sample -- so that two builds run with the
same arguments can be compared output for output."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT


def _fake_trainer(params):
    arena = types.SimpleNamespace(params=params, grad_views={k: -2.0 * v for k, v in params.items()})
    return types.SimpleNamespace(arena=arena)


def test_dump_outputs_writes_float_arrays_and_samples_large_tensors_at_fixed_positions(tmp_path):
    import bench
    n_big = 9488 * 512
    params = {"logit.weight": torch.arange(n_big, dtype=torch.float32).reshape(9488, 512),
              "logit.bias": torch.arange(9488, dtype=torch.float32) + 0.5}
    tr = _fake_trainer(params)
    info = bench.dump_outputs(str(tmp_path / "a"), tr, torch.tensor(3.25))
    assert info["files"] == 5 and info["bytes"] <= 64 << 20
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["grad.logit.bias.npy", "grad.logit.weight.npy", "loss.npy", "param.logit.bias.npy", "param.logit.weight.npy"]
    arrays = {f: np.load(str(tmp_path / "a" / f)) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert arrays["loss.npy"].tolist() == [3.25]
    # small tensors whole, large ones a sample of DUMP_SAMPLE distinct positions in increasing order
    assert np.array_equal(arrays["param.logit.bias.npy"], params["logit.bias"].numpy())
    assert np.array_equal(arrays["grad.logit.bias.npy"], -2.0 * params["logit.bias"].numpy())
    pos = arrays["param.logit.weight.npy"].astype(np.int64)
    assert pos.size == bench.DUMP_SAMPLE < n_big and np.all(np.diff(pos) > 0) and pos[-1] < n_big
    assert np.array_equal(arrays["grad.logit.weight.npy"], -2.0 * params["logit.weight"].reshape(-1).numpy()[pos])
    # the same positions in another run
    bench.dump_outputs(str(tmp_path / "b"), _fake_trainer(params), torch.tensor(3.25), grads=False)
    assert sorted(os.listdir(tmp_path / "b")) == ["loss.npy", "param.logit.bias.npy", "param.logit.weight.npy"]
    assert np.array_equal(np.load(str(tmp_path / "b" / "param.logit.weight.npy")), arrays["param.logit.weight.npy"])


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(tmp_path):
    """The benchmark's own command with --dump-outputs: one JSON line whose `steps` / `ms_per_step` describe the timed region,
    and a dump of that region's last step -- its loss is the line's final_loss, every parameter of the captioner has its updated
    weights and its gradient, everything finite, float32, within 64 MB."""
    out_dir = str(tmp_path / "dump")
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "UIC_BENCH_SHARE_GPU"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-f32",
                          "--no-cpu-baseline", "--long-run", "0", "--dump-outputs", out_dir], env=env, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    files = sorted(os.listdir(out_dir))
    assert d["dumped_outputs"]["files"] == len(files)
    assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in files) <= 64 << 20
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert round(float(arrays["loss"][0]), 4) == d["final_loss"]
    params = {k[6:] for k in arrays if k.startswith("param.")}
    assert params == {k[5:] for k in arrays if k.startswith("grad.")}
    assert {"logit.weight", "embed.0.weight", "core.att_lstm.weight_ih", "core.lang_lstm.weight_hh"} <= params
    assert np.abs(arrays["grad.logit.weight"]).max() > 0
