"""uic_topdown_batch.unfinished_count on the host: topdown_engine.unfinished_counts (what Trainer.attach_live / Trainer.to_device hand
the step) against a plain restatement -- per decode step, the rows whose LAST non-zero mask lies at that step or behind it --
on masks without holes (where it equals live_counts), with holes (where it does not), empty rows and empty steps; and
batch_struct's handling of the third entry of `live`.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from unpaired_image_captioning_amd.topdown_engine import live_counts, unfinished_counts


def restated(masks):
    m = np.asarray(masks)
    N, T = m.shape[0], m.shape[1] - 1
    out = np.zeros(T, dtype=np.int32)
    for n in range(N):
        length = 0
        for t in range(T):
            if m[n, 1 + t] != 0:
                length = t + 1
        for t in range(length):
            out[t] += 1
    return out


def prefix_masks(lengths, T):
    m = np.zeros((len(lengths), T + 1), dtype=np.float32)
    for n, k in enumerate(lengths):
        m[n, :1 + k] = 1.0
    return m


def test_prefix_masks_give_the_live_counts():
    rng = np.random.default_rng(0)
    for N, T in ((1, 1), (4, 6), (85, 17), (640, 17)):
        m = prefix_masks(rng.integers(0, T + 1, N), T)
        u = unfinished_counts(m)
        assert u.dtype == np.int32 and u.shape == (T,)
        assert u.tolist() == restated(m).tolist() == live_counts(m).tolist()
        assert all(u[t] >= u[t + 1] for t in range(T - 1))


def test_masks_with_holes_count_rows_up_to_their_last_position():
    rng = np.random.default_rng(1)
    T = 17
    m = (rng.random((129, T + 1)) < 0.5).astype(np.float32) * (0.25 + rng.random((129, T + 1)).astype(np.float32))
    m[:, 1 + 4] = 0.0                      # an empty decode step in front of live ones
    m[7, :] = 0.0                          # a row without a live position
    m[3, 1:] = 0.0
    m[3, T] = 1.0                          # a row whose only live position is the last step
    u, want = unfinished_counts(m), restated(m)
    assert u.tolist() == want.tolist()
    lc = live_counts(m)
    assert lc[4] == 0 and u[4] > 0         # the hole does not end the captions
    assert (u >= lc).all() and (u != lc).any()
    assert u[T - 1] >= 1 and u[0] <= 128
    assert unfinished_counts(torch.from_numpy(m)).tolist() == want.tolist()
    assert unfinished_counts(np.zeros((4, 6), dtype=np.float32)).tolist() == [0] * 5


def test_column_zero_is_not_a_decode_step():
    m = np.zeros((2, 4), dtype=np.float32)
    m[:, 0] = 1.0
    assert unfinished_counts(m).tolist() == [0, 0, 0]


def test_batch_struct_takes_the_counts_as_a_third_entry():
    from unpaired_image_captioning_amd import _lib
    from unpaired_image_captioning_amd.topdown_engine import TopDownEngine
    assert [f for f, _ in _lib.Batch._fields_].count("unfinished_count") == 1

    class _T:                              # (batch_struct reads shapes only, until it asks for device pointers)
        def __init__(self, *shape):
            self.shape = shape
    eng = TopDownEngine.__new__(TopDownEngine)
    m = prefix_masks([3, 5, 0, 6], 6)
    count, unf = live_counts(m), unfinished_counts(m)
    with pytest.raises(ValueError):
        eng.batch_struct(None, None, None, _T(4, 7), None, live=(None, count, unf[:-1]))
    # without the third entry, or with None, the field stays NULL (the step's earlier path)
    b = _lib.Batch()
    assert not b.unfinished_count
    assert C.sizeof(_lib.Batch) % 8 == 0
