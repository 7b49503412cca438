"""The fused training step with uic_topdown_batch.unfinished_count: the BPTT loop's two d x GEMMs of a decode step run over the rows
whose caption has not ended, wherever those fill fewer 128-row tiles than the batch (Step::compact_step, csrc/topdown_step.hip).
An ended row's gradients are exact zeros and a GEMM row depends on its own A row only, so the loss and EVERY gradient tensor must
be bit for bit those of the same build without the counts -- at the shapes of tests/test_gpu_live_persist.py (bf16, H = A = 512,
D = 256, V = 1001, dropout 0.5): 4 / 85 / 129 rows (one or two tiles, off the split-K chain: the counts change nothing), 300 rows
(three tiles: compact at some steps, not at others), captions of full length (never compact: asserted on the step's launch
count), one row that outlives the others by eight steps, masks with holes, an early break; one case against the CPU oracle; and
counts that are not the masks', which must fail by name and leave the weights alone."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import poison_workspaces

from oracle import topdown as O
from test_gpu_fullsize import GRAD_TOL
from test_gpu_live_persist import CFG, D, E, H, A, L, T, V, SEED_COUNTER, _bench_opt, check_case
from test_gpu_topdown import build_model

pytestmark = pytest.mark.gpu

IMAGES = {4: (1, 4), 85: (17, 5), 129: (129, 1), 300: (60, 5)}


def _lib():
    from unpaired_image_captioning_amd import _lib as L_
    return L_


def make_batch(rows, R, pattern, seed=41):
    n_img, S = IMAGES[rows]
    b = O.synthetic_batch(n_img, S, R, D, V, L, seed=seed, ragged_regions=True)
    g = torch.Generator().manual_seed(4)
    if pattern == "short":                                    # an early break: no caption beyond 11 tokens
        b["labels"][:, 1 + L - 5:] = 0
        b["masks"][:, 2 + L - 5:] = 0.0
    elif pattern == "holes":
        m = (torch.rand(b["masks"].shape, generator=g) < 0.6).float() * (0.25 + torch.rand(b["masks"].shape, generator=g))
        m[:, 1 + 4] = 0.0
        m[min(7, rows - 1), :] = 0.0
        m[:, 1 + 9:] *= (torch.rand(rows, 1, generator=g) < 0.4).float()      # (most rows end by step 9, so that tiles empty)
        b["labels"][1, 1:] = torch.randint(1, V, (T,), generator=g)
        m[1, 1 + T - 1] = 1.0
        b["masks"] = m
    elif pattern == "full":                                   # every caption runs to the last step
        b["labels"][:, 1:] = torch.randint(1, V, (rows, T), generator=g)
        b["masks"][:] = 1.0
    elif pattern == "outlier":                                # one row outlives all the others by eight steps
        b["labels"][:, 1:] = torch.randint(1, V, (rows, T), generator=g)
        b["masks"][:] = 0.0
        b["masks"][:, :1 + 8] = 1.0
        b["labels"][:, 1 + 8:] = 0
        b["labels"][rows // 2, 1:] = torch.randint(1, V, (T,), generator=g)
        b["masks"][rows // 2, :1 + 16] = 1.0
    else:
        assert pattern == "lengths", pattern
    return b


def fused_step(model, batch, with_counts):
    """(loss, gradients, compact d x launches) of one fused step from the same seed, the list made on the device."""
    from unpaired_image_captioning_amd.trainer import Trainer, xe_step
    Lb = _lib()
    b = Trainer.attach_live({k: v for k, v in batch.items() if k not in ("live_count", "live_rows", "unfinished_count")})
    assert b["unfinished_count"].dtype == np.int32
    if not with_counts:
        del b["unfinished_count"]
    model._seed_counter = SEED_COUNTER
    loss, grads = xe_step(model, b)
    st = Lb.persistent_status()
    assert st[0] == 0
    n = C.c_int32(-1)
    Lb.check(Lb.load().uic_topdown_compact_launches(C.byref(n)))
    return loss.item(), {k: g.detach().clone() for k, g in grads.items()}, n.value, b


def expected_compact_launches(unf, rows, t_run):
    """Two GEMMs per decode step whose unfinished rows leave a 128-row tile empty -- one at step 0, which has no d x1 -- on the
    split-K chain (256 rows and more)."""
    if rows < 256:
        return 0
    tiles = (rows + 127) // 128
    return sum((2 if t > 0 else 1) for t in range(t_run) if unf[t] > 0 and (unf[t] + 127) // 128 < tiles)


# every row count meets every mask pattern, the region counts go round; then the two batches built for this change
CASES = [(rows, (1, 7, 36)[(i + j) % 3], pattern) for i, rows in enumerate((4, 85, 129, 300))
         for j, pattern in enumerate(("lengths", "short", "holes"))] + [(300, 7, "full"), (300, 7, "outlier")]


@pytest.mark.parametrize("rows,R,pattern", CASES)
def test_step_with_unfinished_counts_is_bit_equal_to_the_step_without(rows, R, pattern):
    W = O.init_weights(V + 1, E, H, A, D, D, seed=13)
    batch = {k: v.cuda() for k, v in make_batch(rows, R, pattern).items()}
    model = build_model(CFG, W, "bf16", drop=0.5)
    model.train()
    poison_workspaces(model.engine)
    t_run = model._steps_to_run(batch["labels"])
    loss0, g0, n0, _ = fused_step(model, batch, False)
    loss1, g1, n1, b = fused_step(model, batch, True)
    unf = b["unfinished_count"]
    want = expected_compact_launches(unf, rows, t_run)
    print("%d rows, %s: t_run %d, unfinished %s, compact d x launches %d" % (rows, pattern, t_run, unf.tolist(), n1))
    assert n0 == 0 and n1 == want
    if pattern == "full":
        assert t_run == T and (unf == rows).all() and n1 == 0              # every tile live at every step: never compact
    elif pattern == "outlier":
        assert unf.tolist() == [rows] * 8 + [1] * 8 + [0] and n1 == 16
    elif rows == 300:
        assert 0 < n1 < 2 * t_run - 1                                       # compact at some steps, not at others
    if pattern == "holes":
        assert (unf != b["live_count"]).any()
    assert loss1 == loss0
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k
    assert all(torch.isfinite(g).all() for g in g1.values())


def test_step_with_unfinished_counts_vs_oracle():
    """300 rows through the oracle comparison of tests/test_gpu_live_persist.py (its "device" form is Trainer.attach_live, which
    hands the step the counts), every gradient tensor at GRAD_TOL."""
    W = O.init_weights(V + 1, E, H, A, D, D, seed=13)
    b = make_batch(300, 7, "lengths")
    check_case("300 rows, unfinished counts", CFG, W, b, "bf16", GRAD_TOL["bf16"], "lengths", forms=("device",))


def test_counts_that_are_not_the_masks_fail_by_name_and_leave_the_weights_alone():
    """One count one too small at one step.  The launches are sized by it and stay inside their buffers either way -- a GEMM over
    count rows of an [N, 4H] operand, count <= N, placed by the device's own order --, so nothing faults; the list kernel sees the
    difference and sets the status word: the optimizer step is skipped on the device and the next look at the status raises."""
    from unpaired_image_captioning_amd.trainer import Trainer
    Lb = _lib()
    torch.manual_seed(1234)
    tr = Trainer(_bench_opt("bf16", 1234))
    model = tr.i2t_model
    tr.build_optimizer()
    batch = {k: v.cuda() for k, v in make_batch(300, 7, "lengths", seed=31).items()}
    t_run = model._steps_to_run(batch["labels"])
    den = float(batch["masks"][:, 1:T + 1].sum().item())
    tr.attach_live(batch)
    good = batch["unfinished_count"].copy()
    t_bad = int(np.flatnonzero((good > 1) & (good <= 256))[0])              # a step that takes the compact form
    Lb.persistent_status()
    before = {k: p.detach().clone() for k, p in tr.arena.params.items()}
    batch["unfinished_count"] = good.copy()
    batch["unfinished_count"][t_bad] -= 1
    tr.train_device_batch(batch, t_run, den, den)
    with pytest.raises(Lb.UnfinishedCountMismatch, match=r"unfinished_count\[%d\]" % t_bad):
        Lb.persistent_status()
    for k, p in tr.arena.params.items():
        assert torch.equal(p.detach(), before[k]), k
    # the right counts afterwards: an ordinary step
    batch["unfinished_count"] = good
    loss = tr.train_device_batch(batch, t_run, den, den)
    assert Lb.persistent_status()[0] == 0 and np.isfinite(float(loss.item()))
    assert any(not torch.equal(p.detach(), before[k]) for k, p in tr.arena.params.items())
