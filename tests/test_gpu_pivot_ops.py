"""uic_pivot_source / uic_pivot_target (csrc/pivot.hip) on the device against the plain-Python restatement of
tests/pivot_cases.py: integer and gather work, so every output is compared with torch.equal.  Every output buffer is pre-filled
with a poison value, so each element the contract names is seen to be written -- and nothing beside them."""
import numpy as np
import pytest
import torch

import pivot_cases as PC

pytestmark = pytest.mark.gpu


def lib():
    from unpaired_image_captioning_amd import _lib
    return _lib.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_source(seq, L, table, guard=5):
    from unpaired_image_captioning_amd._lib import check, ptr, stream
    B, ld = seq.shape
    seq_d, table_d = dev(seq), dev(table)
    src = torch.full((L * B + guard,), PC.POISON, dtype=torch.int64, device="cuda")
    lengths = torch.full((B + guard,), PC.POISON, dtype=torch.int32, device="cuda")
    max_len = torch.full((1 + guard,), PC.POISON, dtype=torch.int32, device="cuda")
    check(lib().uic_pivot_source(ptr(seq_d), ld, B, L, ptr(table_d), len(table), ptr(src), ptr(lengths), ptr(max_len), stream()), "pivot_source")
    torch.cuda.synchronize()
    for t, n in ((src, L * B), (lengths, B), (max_len, 1)):
        assert (t[n:] == PC.POISON).all()                                   # nothing written behind the outputs
    return src[:L * B].view(L, B).cpu(), lengths[:B].cpu(), int(max_len[0])


@pytest.mark.parametrize("L", [1, 16])
@pytest.mark.parametrize("B", PC.BATCHES)
def test_pivot_source_equals_the_restatement(B, L):
    seq, table = PC.source_case(B, L)
    assert seq.shape[1] > L
    src, lengths, max_len = run_source(seq, L, table)
    want_src, want_len, want_max = PC.restated_source(seq, L, table)
    assert torch.equal(src, torch.from_numpy(want_src))
    assert torch.equal(lengths, torch.from_numpy(want_len))
    assert max_len == want_max
    assert not (src == PC.POISON).any()
    if B >= 7:                                                              # every named row kind is in the batch
        assert lengths[0] == 1 and src[0, 0] == PC.UNK and (src[1:, 0] == PC.PAD).all()       # empty -> [UNK]
        assert lengths[1] == L                                                                 # no terminator
        assert lengths[2] == max(L // 2, 1)                                                   # ended by -1 (L = 1: the empty caption)
        assert src[0, 3] == table[len(table) - 1]                                              # V1 - 1 is looked up
        assert src[0, 4] == PC.UNK and src[min(1, L - 1), 4] == PC.UNK                         # ids >= V1


def test_pivot_source_is_bit_reproducible_and_max_len_can_be_below_L():
    seq, table = PC.source_case(130, 16, seed=3)
    seq[:, 9:] = 0
    a = run_source(seq, 16, table)
    b = run_source(seq, 16, table)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2] == 9
    assert (a[0][9:] == PC.PAD).all()


def run_target(c, guard=5):
    from unpaired_image_captioning_amd._lib import check, ptr, stream
    hyp, attn, src_len, seq = dev(c["hyp"]), dev(c["attn"]), dev(c["src_len"]), dev(c["seq"])
    tgt_table, copy_table = dev(c["tgt_table"]), dev(c["copy_table"])
    B, L_out = hyp.shape[0], c["L_out"]
    out = torch.full((B * L_out + guard,), PC.POISON, dtype=torch.int64, device="cuda")
    out_len = torch.full((B + guard,), PC.POISON, dtype=torch.int32, device="cuda")
    repl = torch.full((B * L_out + guard,), PC.POISON, dtype=torch.int32, device="cuda")
    check(lib().uic_pivot_target(ptr(hyp), hyp.shape[1], c["n_steps"], ptr(attn), attn.shape[1], attn.shape[2], ptr(src_len), ptr(seq),
                                 seq.shape[1], B, ptr(tgt_table), len(c["tgt_table"]), ptr(copy_table), len(c["copy_table"]), L_out,
                                 ptr(out), ptr(out_len), ptr(repl), stream()), "pivot_target")
    torch.cuda.synchronize()
    for t, n in ((out, B * L_out), (out_len, B), (repl, B * L_out)):
        assert (t[n:] == PC.POISON).all()
    return out[:B * L_out].view(B, L_out).cpu(), out_len[:B].cpu(), repl[:B * L_out].view(B, L_out).cpu()


def check_target(c):
    out, out_len, repl = run_target(c)
    want = PC.restated_target(**c)
    assert torch.equal(out, torch.from_numpy(want[0]))
    assert torch.equal(out_len, torch.from_numpy(want[1]))
    assert torch.equal(repl, torch.from_numpy(want[2]))
    return out, out_len, repl


MAX_STEPS = 100


@pytest.mark.parametrize("n_steps", [1, 2, MAX_STEPS])
@pytest.mark.parametrize("B", PC.BATCHES)
def test_pivot_target_equals_the_restatement(B, n_steps):
    c = PC.target_case(B, n_steps, ld_hyp=MAX_STEPS)
    out, out_len, repl = check_target(c)
    if B >= 9 and n_steps == MAX_STEPS:
        sl = c["src_len"]
        assert out_len[0] == 0 and (out[0] == 0).all() and (repl[0] == -1).all()                 # EOS at column 0
        assert out_len[1] == n_steps - 1 and out_len[2] == n_steps - 1                             # EOS last / absent
        assert repl[3, 0] == 0                                                                     # attention tie: the lowest index
        assert repl[4, 0] == sl[4] - 1                                                             # the maximum on the last valid column
        assert (repl < torch.from_numpy(sl)[:, None]).all() and (repl >= 0).any()               # never a column behind src_len
        assert out[5, 0] == c["tgt_table"][PC.UNK] and repl[5, 0] == -1                            # a token >= Vt
        assert (repl[6, :n_steps - 1] >= 0).all()


@pytest.mark.parametrize("L_out", [1, 7, 64, 65])
def test_pivot_target_cuts_at_L_out(L_out):
    c = PC.target_case(65, MAX_STEPS, ld_hyp=MAX_STEPS + 3, L_out=L_out, seed=2)
    out, out_len, repl = check_target(c)
    assert out_len.max() == L_out                                           # hypotheses longer than the rows


def test_pivot_target_with_the_widest_source_and_attention_rows_behind_n_steps_unread():
    c = PC.target_case(64, 5, ld_hyp=9, S=70, L=70, seed=4)
    c["attn"][:, 5:] = np.nan                                               # rows behind n_steps are not read
    c["hyp"][:, 5:] = PC.UNK
    check_target(c)
    a, b = run_target(c), run_target(c)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
