"""Host-to-device batch shipping of the Trainer (trainer.py): the pinned staging rings, the copy stream of the prefetch, the
prefetched batch and the seq_per_img replication check.  One BatchShipper per Trainer; nothing here touches a model's weights
or the optimizer."""
import numpy as np
import torch

from .topdown_engine import live_counts, unfinished_counts


def attach_live(batch):
    """Adds the per-step counts of unmasked positions to a DEVICE batch (a resident benchmark batch; BatchShipper.to_device does
    it for host batches).  One device-to-host read of the masks: call it once per batch, outside a timed region."""
    batch["live_count"] = live_counts(batch["masks"])
    batch["unfinished_count"] = unfinished_counts(batch["masks"])     # (rows per step the BPTT loop's d x GEMMs run over)
    return batch


class BatchShipper(object):
    """State, all of it owned here: `_pin` / `_pin_slot` (two pinned staging buffers per batch key, each with the event of the
    copy that last read it), `_pinf` (a ring of pinned floats), `_copy_stream` (created by the first prefetch: a Trainer that
    never prefetches must not initialise HIP in its constructor; checkpoints copy on a stream of their own,
    trainer_checkpoint.py), `_prefetched` and `_replication_checked`."""

    def __init__(self, opt, model):
        self.opt = opt
        self.model = model
        self._pin = {}
        self._pin_slot = {}
        self._pinf = None
        self._pinf_i = 0
        self._copy_stream = None
        self._prefetched = None
        self._replication_checked = False

    def to_device(self, data, per_image=True):
        """numpy batch dict of DataLoader.get_batch -> device tensors (P/trainer.py:147-149).

        The loader replicates every image's features seq_per_img times on the host (P/misc/dataloader/dataloader.py:
        270-277).  With opt.seq_per_img > 1 only every seq_per_img-th feature row crosses PCIe (37.7 MB instead of
        188.7 MB at config 2) and the replication happens on the device (uic_topdown_dims.seq_per_img); the first batch
        is checked to really be replicated.  opt.ship_replicated_features = 1 keeps the reference's behaviour."""
        S = int(getattr(self.opt, 'seq_per_img', 1) or 1)
        if not per_image or getattr(self.opt, 'ship_replicated_features', 0) or not hasattr(self.model, 'use_bn'):
            S = 1
        out = {}
        for k in ("fc_feats", "att_feats", "labels", "masks", "att_masks"):
            v = data.get(k)
            if v is None:
                continue
            if S > 1 and k in ("fc_feats", "att_feats", "att_masks") and isinstance(v, np.ndarray) and len(v) == len(data["labels"]):
                if not self._replication_checked:
                    for j in range(1, S):
                        if not (np.asarray(v[j::S]) == np.asarray(v[::S])).all():
                            raise ValueError("opt.seq_per_img=%d but the rows of %s are not %d-fold replicated; set "
                                             "opt.ship_replicated_features=1 for per-caption features" % (S, k, S))
                v = v[::S]
            if isinstance(v, np.ndarray):
                v = torch.from_numpy(v if v.flags.writeable else v.copy())
            out[k] = self._ship(k, v, torch.int64 if k == "labels" else torch.float32)
        self._replication_checked = True
        if getattr(self.opt, 'live_positions', 1) and data.get("masks") is not None and not torch.is_tensor(data["masks"]):
            # how many positions of each decode step lie in front of their caption's end is known here, on the host, where the
            # loader made the masks: the step's logit layer and criterion skip the others (uic_topdown_batch.live_count: the step
            # compacts the device masks itself, nothing more is shipped; opt.live_positions = 0 computes every position)
            out["live_count"] = live_counts(data["masks"])
            out["unfinished_count"] = unfinished_counts(data["masks"])
        return out

    def _ship(self, key, t, dtype):
        """Host tensor (any strides / dtype) -> device: ONE threaded gather-and-convert pass into a pinned staging buffer
        (two per key, guarded by events) and an asynchronous copy, instead of ascontiguousarray + a pageable hipMemcpy
        that stages a second time."""
        if t.is_cuda:
            return t.to(dtype)
        ring = self._pin.setdefault(key, [])
        i = self._pin_slot.get(key, 0)
        self._pin_slot[key] = (i + 1) % 2
        while len(ring) <= i:
            ring.append(None)
        if ring[i] is None or ring[i][0].shape != t.shape or ring[i][0].dtype != dtype:
            ring[i] = [torch.empty(t.shape, dtype=dtype, pin_memory=True), None]
        pin, ev = ring[i]
        if ev is not None:
            ev.synchronize()                       # the copy that last read this buffer has finished
        # at most 8 copy threads: a machine-wide OpenMP team (256 threads on the MI355X hosts) keeps spinning after the
        # copy and slows the following kernel enqueues 4x (measured: the replay + BPTT enqueue 4.2 -> 16.7 ms)
        nthr = torch.get_num_threads()
        if nthr > 8:
            torch.set_num_threads(8)
        try:
            pin.copy_(t)
        finally:
            if nthr > 8:
                torch.set_num_threads(nthr)
        dev = pin.cuda(non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        ring[i][1] = ev
        return dev

    def host_float(self, x, dev):
        """A host float as a 1-element device tensor without a synchronous pageable copy (ring of pinned floats)."""
        if self._pinf is None:
            self._pinf = torch.zeros(64, dtype=torch.float32).pin_memory()
            self._pinf_i = 0
        i = self._pinf_i
        self._pinf_i = (i + 1) % 64
        self._pinf[i] = x
        return self._pinf[i:i + 1].to(dev, non_blocking=True)

    def prefetch(self, data, per_image, holder):
        """Ship a batch to the device on the copy stream NOW (pinned staging + asynchronous H2D), to be consumed by the next
        device_batch() call with this very dict.  `holder` (the Trainer): its `next_data` receives the batch -- for a callable
        the one it returned -- before the copies start."""
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream()
        with torch.cuda.stream(self._copy_stream):
            if callable(data):
                # e.g. `lambda: loader.get_batch('train')`: the loader's host work, its H2D copies and its assembly kernel
                # all happen here -- after this step was enqueued, on the copy stream; the batch is left in holder.next_data
                data = data()
            holder.next_data = data
            if data is None:                          # the caller's source is exhausted
                self._prefetched = None
                return
            batch = self.to_device(data, per_image)
            ev = torch.cuda.Event()
            ev.record()
        self._prefetched = (id(data), per_image, batch, ev)

    def device_batch(self, data, per_image=True):
        """The device tensors of `data`: the prefetched ones if this very dict was prefetched, else shipped now."""
        pf = self._prefetched
        self._prefetched = None
        if pf is not None and pf[0] == id(data) and pf[1] == per_image:
            cur = torch.cuda.current_stream()
            cur.wait_event(pf[3])
            for t in pf[2].values():
                if torch.is_tensor(t):
                    t.record_stream(cur)               # allocated on the copy stream, consumed on this one
            return pf[2]
        return self.to_device(data, per_image)

    def drop_prefetched(self):
        """A prefetched batch is not part of a checkpoint (Checkpointer.load)."""
        self._prefetched = None
