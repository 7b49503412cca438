"""The token sets of tests/embedding_cases.py on the CPU: together they reach every class of launch geometry the classifier knows
(a condition: a class nobody reaches is a hole in tests/test_gpu_embedding.py), and a numpy restatement of the kernels' pipeline
-- stable counting sort, one owner per table row, two planes of partial rows, the finish kernel's eight interleaved groups --
equals index_add_ in float64 on every case."""
import numpy as np
import pytest
import torch

import embedding_cases as EC

CASES = EC.backward_cases()


def test_the_cases_reach_every_class_of_the_launch_geometry():
    reached = {}
    for c in CASES:
        for k in EC.classify(c):
            reached.setdefault(k, []).append(c.name)
    missing = [k for k in EC.CLASSES if k not in reached]
    assert not missing, missing
    # the classes of the two-half mode come from cases that split; the padding-index class from cases that have one
    split_names = {c.name for c in CASES if c.split}
    for k in ("l_aligned", "l_unaligned", "l_b", "l_c", "l_d"):
        assert set(reached[k]) <= split_names, k


def test_the_constructed_layouts_are_what_they_say():
    a = EC.case_by_name("layoutA-0")
    hit = EC.classify(a)
    assert {"a", "b", "c", "d", "e_inside", "e_arriving", "f", "g", "i_short"} <= hit, hit
    _, off = EC.sorted_list(a)
    assert off.tolist() == [0, 1, 3, 16, 32, 40, 56, 73, 80, 209, 354, 514, 544, 549, 549]
    assert np.diff(off).tolist()[:12] == [1, 2, 13, 16, 8, 16, 17, 7, 129, 145, 160, 30]
    b = EC.case_by_name("layoutB-E8")
    assert {"h_key0", "h_keylast", "i_one"} <= EC.classify(b)
    assert "m" in EC.classify(EC.case_by_name("layoutA-skip-hot")) and "m" not in EC.classify(EC.case_by_name("layoutA-skip-cold"))
    for name in ("split1-0", "splitmid-0"):
        assert {"l_b", "l_c", "l_d"} <= EC.classify(EC.case_by_name(name)), name
    assert "l_unaligned" in EC.classify(EC.case_by_name("split1-0")) and "l_aligned" in EC.classify(EC.case_by_name("splitmid-0"))


def test_the_sizes_the_issue_names_are_there():
    sizes = {c.positions for c in CASES}
    assert {1, 15, 16, 17, 1023, 1024, 1025, 2049} <= sizes
    assert {EC.hist_blocks(n) for n in (1023, 1024, 1025, 2049)} == {1, 2, 3}
    assert any(c.T == 1 and c.ld == 1 for c in CASES)
    assert {c.positions for c in CASES if c.name.startswith("onetoken")} == {16, 160, 161, 2049}
    assert {c.V1 for c in CASES if c.name.startswith("keys") and not c.split} == {1, 3, 4, 5, 4095, 4096, 4097, 8193}
    assert {c.nkeys() for c in CASES if c.name.startswith("keys") and c.split} == {4098, 8194}
    assert {EC.SCAN_TRIP - 1, EC.SCAN_TRIP, EC.SCAN_TRIP + 1, 2 * EC.SCAN_TRIP + 1, 2 * EC.SCAN_TRIP + 2} <= {c.nkeys() for c in CASES}
    assert {4, 8, 12, 512, 516} <= {c.E for c in CASES}
    assert 512 // 4 == EC.FINISH_COLS and 516 // 4 == EC.FINISH_COLS + 1
    assert {(c.drop_p, c.xt) for c in CASES} == {(p, x) for p in EC.DROPS for x in EC.XT_MODES}
    layout_a = {(c.drop_p, c.xt) for c in CASES if c.name.startswith("layoutA-") and c.name[8:].isdigit()}
    assert len(layout_a) == 15
    splits = {(c.split, c.T) for c in CASES if c.split}
    assert any(s == 1 for s, _ in splits) and any(s == t - 1 for s, t in splits) and any(1 < s < t - 1 for s, t in splits)
    z = EC.case_by_name("zipf")
    assert z.ld > z.T and 250 <= np.unique(z.row_token()).size <= 300 and 2200 <= z.positions <= 2400
    sz = np.bincount(z.row_token())
    assert ((sz >= 17) & (sz <= 200)).sum() >= 10                        # the buckets uniform draws never make
    o = EC.case_by_name("outside")
    assert {-1, o.V1, 2 ** 40, EC.INT64_MIN} <= set(o.rows.tolist())
    d = EC.dirty_case()
    assert d.positions > max(c.positions for c in CASES)


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_restated_pipeline_equals_index_add(c):
    perm, off = EC.restated_sort(c)
    perm_ref, off_ref = EC.sorted_list(c)
    assert (perm == perm_ref).all() and (off == off_ref).all()           # the list order: a stable sort by key
    g = c.grad().astype(np.float64)
    table = np.zeros((c.V1, c.E))
    if c.split:
        stores = EC.restated_gather(c, perm, off, g, table, halves=(1,))
        assert torch.equal(torch.from_numpy(table), EC.reference(c, g, halves=(1,)))
        stores += EC.restated_gather(c, perm, off, g, table, halves=(0,))
    else:
        stores = EC.restated_gather(c, perm, off, g, table)
    assert not np.isnan(table).any()                                     # no partial row was read before it was written
    assert torch.equal(torch.from_numpy(table), EC.reference(c, g))
    for count in stores:                                                 # one owner per table row and launch
        assert count.max() <= 1
    present = np.zeros(c.V1, dtype=bool)
    present[c.row_token()] = True
    if c.skip >= 0:
        present[c.skip] = False
    total = np.sum(stores, axis=0)
    assert ((total > 0) == present).all()
    assert (table[~present] == 0).all()


def test_scratch_formula_has_room_for_every_region():
    for c in CASES + (EC.dirty_case(),):
        n = EC.scratch_ints(c.N, c.T, c.V1, c.E)
        perm_end = 3 * (c.nkeys() + 1) + c.positions
        fixed = n - 2 * EC.chunk_slots(c.N, c.T) * c.E - (EC.hist_blocks(c.positions) * 2 * c.V1 + 63) // 64 * 64
        assert perm_end <= fixed and fixed % 4 == 0
        used = max(chunk0 + -(-(total - base) // EC.CH) for _, base, total, _, chunk0 in c.halves())
        assert used <= EC.chunk_slots(c.N, c.T)


def test_dropout_hash_restatement_is_a_fair_coin():
    keep = EC.drop_keep(100003, 0.5, 7, 3, 2 ** 32 - 50000)
    assert abs(keep.mean() - 0.5) < 0.01
    assert EC.drop_keep(1000, 0.0, 7, 3, 0).all()
    assert (EC.drop_keep(64, 0.5, 7, 3, 2 ** 32 - 10)[10:] == EC.drop_keep(54, 0.5, 7, 3, 0)).all()     # the index wraps
