"""The cases of tests/attention_cases.py on the CPU (an edge nobody reaches is a hole in tests/test_gpu_attention.py).

* The case list reaches every kernel id of the three launchers in every dtype the kernel is built for, and for every condition of
  the fast / round-6 choice a case where that condition ALONE fails beside cases where all hold.  A list that loses one fails here.
* Every refusal the launchers are asked to make is in the list, and the restated refusal() agrees with why each was put there.
* A float32 restatement of the kernels' formulas -- correctly rounded tanh, the exp2 / reciprocal form, the factored e^{2p} e^{2h}
  form with both limits and with the reciprocal shared by two steps -- stays within a QUARTER of the bound on every case.  Measured
  maxima of error / bound over the 235 cases (a run with -s prints them per output and form): forward 0.051 (alpha, exp form;
  0.038 with tanhf), step 0.077 (de) and 0.158 (the slabs' sum), accumulation 0.208 (d_p_att of a one-step row in the exp form),
  0.168 (d_p_att, shared reciprocal), 0.121 (d_p_att, factored up to 40), 0.158 (d_att), 0.093 (part).  The counts of
  tests/attention_cases.py are worst cases of serial chains; the restatement rounds at random and sums pairwise.
* Planted mistakes leave the bound by orders of magnitude; no case's largest buffer exceeds 4 MB.
"""
import numpy as np
import pytest

import attention_cases as AC

FWD, STEP, ACCUM = AC.fwd_cases(), AC.step_cases(), AC.accum_cases()
EVERY = [(c, dt) for c in AC.all_cases() for dt in c.dtypes]
BOTH = (AC.F32, AC.BF16)
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print("\n[attention, host] %-6s %-9s %-21s worst error / bound: %.4f (%s)" % (k + WORST[k]))


def _alone(cases, names, part=None):
    """For both dtypes: every condition in `names` fails alone in some case, and some case breaks none."""
    for dt in BOTH:
        alone, none = set(), 0
        for c in cases:
            if dt not in c.dtypes:
                continue
            bad = AC.broken_conditions(c, dt, part)
            none += not bad
            if len(bad) == 1:
                alone |= bad
        yield dt, [n for n in names if n not in alone], none


def test_the_cases_reach_every_kernel_and_both_sides_of_every_condition():
    for cases in (FWD, STEP):
        kinds = {(AC.classify(c, dt), dt) for c in cases for dt in c.dtypes}
        assert kinds == {(k, dt) for k in (AC.GENERIC, AC.FAST, AC.FAST_FULL) for dt in BOTH}
    for dt, missing, none in _alone(FWD, AC.CONDITIONS["fwd"]):
        assert not missing and none, (dt, missing)
    for dt, missing, none in _alone(STEP, AC.CONDITIONS["step"]):
        assert not missing and none, (dt, missing)
    bits = {(AC.classify(c, dt), dt) for c in ACCUM for dt in c.dtypes}
    assert bits == {(0, AC.F32), (AC.P1_R6, AC.F32)} | {(b, AC.BF16) for b in (0, 1, 2, 3)}
    for dt, missing, none in _alone(ACCUM, AC.CONDITIONS["p1"], "p1"):
        assert not missing and none, (dt, missing)
    for dt, missing, none in _alone(ACCUM, AC.CONDITIONS["p2"], "p2"):
        # the dtype: f32 never takes the round-6 PART 2 kernel (and fails nothing else alone), bf16 always holds it;
        # 8-byte alignment of p_att / d_p_att fails only in refused calls (test_every_requested_refusal_is_present)
        if dt == AC.F32:
            assert set(missing) == set(AC.CONDITIONS["p2"]) - {"dtype"} and not none
        else:
            assert none and set(missing) == {"dtype", "p_att_al8", "d_p_att_al8"}, missing
    # 8 bytes off: the bf16 round-6 kernel takes it, and those cases run
    by = {c.name: c for c in ACCUM}
    for n in ("accum-mis-patt-8", "accum-mis-dpatt-8"):
        assert AC.classify(by[n], AC.BF16) == AC.P1_R6 | AC.P2_R6 and AC.refusal(by[n], AC.BF16) is None and by[n].dtypes == (AC.BF16,)
    for c, dt in EVERY:
        assert AC.refusal(c, dt) is None, (c, dt)


def test_the_choice_boundaries_of_the_issue_are_in_the_list():
    for cases, op in ((FWD, "fwd"), (STEP, "step")):
        shapes = {(c.R, c.Av, c.Hv) for c in cases if c.name.startswith(op + "-R")}
        assert {r for r, _, _ in shapes} == set(AC.CHOICE_R) == {1, 3, 35, 36, 37, 40}
        for R in (36, 37):
            assert {(a, h) for r, a, h in shapes if r == R} >= {(64, 64), (64, 63), (63, 64), (65, 64), (64, 65), (1, 1), (65, 65)}
        by = {c.name: c for c in cases}
        for dt in BOTH:
            v = AC.vec(dt)
            assert by[op + "-R36-64x64"].A(dt) == 64 * v == by[op + "-R36-64x64"].H(dt) and (v, 64 * v) in ((4, 256), (8, 512))
            assert AC.classify(by[op + "-R36-64x64"], dt) == AC.FAST_FULL and AC.classify(by[op + "-R37-64x64"], dt) == AC.GENERIC
            assert AC.classify(by[op + "-R36-64x63"], dt) == AC.FAST == AC.classify(by[op + "-R36-63x64"], dt)
            assert AC.broken_conditions(by[op + "-R36-65x64"], dt) == {"A"} and AC.broken_conditions(by[op + "-R36-64x65"], dt) == {"H"}
    assert {c._lddctx for c in STEP if c.name.startswith("step-lddctx")} == {(1, 0), (3, 0), (1, 2)}
    assert {c.nslab for c in STEP} >= set(AC.STEP_NSLAB) == {0, 1, 2, 3, 4, 5, 7}
    for k in (AC.GENERIC, AC.FAST, AC.FAST_FULL):                                     # every slab count, dctx_sum, row_len in every kernel
        mine = [c for c in STEP if AC.classify(c, AC.BF16) == k]
        assert {c.nslab for c in mine} >= set(AC.STEP_NSLAB), k
        assert {c.dsum for c in mine} == {True, False}
        rl = [c for c in mine if c.row_len is not None]
        assert any(set(np.sign(np.asarray(c.row_len) - c.step)) == {-1, 0, 1} and 0 in c.row_len for c in rl), k
        assert all(c.ld_sum(AC.BF16) == 3 * c.H(AC.BF16) for c in mine if c.dsum and c.name != "step-mis-ld-sum")
    assert {c.T for c in ACCUM} >= set(AC.ACCUM_T) == {1, 2, 5, 6, 7, 12, 13}
    assert {c.R for c in ACCUM} >= set(AC.ACCUM_R) == {1, 3, 4, 36, 37, 72, 73}
    assert {c.A(0) for c in ACCUM} >= {8, 72, 512} and {c.H(0) for c in ACCUM} >= {8, 40, 512}
    assert any(c._lddctx == (3, 0) and c.stride(0) == 3 * c.N * c.H(0) for c in ACCUM)
    seen = set()
    for c in ACCUM:
        if c.row_len is not None and c.T == 7 and len(set(c.row_len)) > 2:
            seen |= set(c.row_len)
    assert seen >= {0, 1, 6, 7, 10}                                                    # {0, 1, T - 1, T, T + 3}, mixed within a call
    assert {c.mask for c in FWD} == set(AC.MASKS) and any(c.ld_mask_extra for c in FWD) and any(not c.bias for c in FWD)
    vals = {c.values for c in ACCUM}
    assert vals >= {"wide", "wide10", "wide20"} | {"limit" + l for l in AC.LIMITS}
    assert {c.values for c in FWD} >= {"wide", "spread110", "spread90"}
    assert all(c.N <= 4 for c in AC.all_cases())


def test_the_values_sit_where_the_issue_puts_them():
    x = AC.inputs(next(c for c in ACCUM if c.name == "accum-wide-T5"), AC.BF16)
    s = x.p_att[None].astype(np.float64) + x.att_h[:, :, None, :]
    assert 45 < np.abs(s).max() <= 50 and np.abs(s[0, :, 0]).max() < 3 and (np.sign(x.p_att[:, 0]) != np.sign(x.att_h[0])).mean() > 0.9
    for l in AC.LIMITS:
        x = AC.inputs(next(c for c in ACCUM if c.name == "accum-limit%s-T2" % l), AC.BF16)
        assert (x.p_att[:, :, 1] == float(l)).all() and (x.att_h[:, :, 1] == float(l)).all() and (x.att_h[:, :, 2] == -float(l)).all()
        assert float(AC.round_bf16(np.float32(float(l)))) == float(l)                  # one bf16 step: 10.75 | 10.8125, 20 | 20.125
    assert 2 * 10.75 == AC.P2_LIM and 2 * 20 == AC.EXP_LIM
    one = np.float32(1) + np.exp2(np.float32(4 * 10.75) * np.float32(1.4426950408889634))
    assert np.isfinite(one * one) and 85 < np.log(np.float64(one) ** 2) < 87           # the shared reciprocal sees e^86
    for name, lo, hi in (("fwd-spread110-R37", 104, 1e9), ("fwd-spread90-R37", 80, 100)):
        x = AC.inputs(next(c for c in FWD if c.name == name), AC.F32)
        e = np.tanh(x.p_att.astype(np.float64) + x.att_h[:, None, :]) @ x.w_alpha.astype(np.float64)
        sp = e.max(1) - e.min(1)
        assert lo < sp.min() and sp.min() <= hi, (name, sp)
    ref, _ = AC.reference(AC.inputs(next(c for c in FWD if c.name == "fwd-spread110-R37"), AC.F32))
    assert (ref["alpha"].astype(np.float32) == 0).any()                                # weights that underflow to exact 0
    for c, dt in EVERY:                                                                # finite operands everywhere
        x = AC.inputs(c, dt)
        for k, v in x.__dict__.items():
            if isinstance(v, np.ndarray) and v.dtype.kind == "f":
                assert np.isfinite(v).all(), (c, k)
        if c.poison:
            assert (np.abs(x.att[x.mask == 0]) > 9e29).all() and (x.mask == 0).any()


def test_every_requested_refusal_is_present():
    got = {}
    for c, dt, null, why in AC.refused_cases():
        got.setdefault(why, set()).add(c.op)
        if why == "null":
            assert null in AC.REQUIRED[c.op] and AC.refusal(c, dt) is None
        else:
            assert AC.refusal(c, dt) == why, (c, dt, AC.refusal(c, dt))
    assert set(got) == set(AC.REFUSALS_ASKED)
    for why in ("dtype", "vec", "null", "lds"):
        assert got[why] == set(AC.OPS), why
    assert got["p_att_al"] == set(AC.OPS) and got["att_al"] == {"fwd", "step"} and got["d_att_al"] == got["d_p_att_al"] == {"accum"}
    nulls = {(c.op, null) for c, _, null, why in AC.refused_cases() if why == "null"}
    assert nulls == {(op, n) for op in AC.OPS for n in AC.REQUIRED[op]}
    # the LDS bound, both sides: the sizes of the issue, the last below 64 KB, the last the launcher admits and the first it does not
    size = {c.name: AC.lds_bytes(c, AC.F32) for c in FWD + STEP if "-lds-" in c.name}
    assert size["fwd-lds-H4096"] == 65632 and size["step-lds-A2728"] == 65584
    assert size["fwd-lds-H4088"] < AC.LDS_DEFAULT < size["fwd-lds-H4096"] and size["step-lds-A2724"] < AC.LDS_DEFAULT < size["step-lds-A2728"]
    assert AC.LDS_MAX - 64 < size["fwd-lds-H10232"] <= AC.LDS_MAX and AC.LDS_MAX - 64 < size["step-lds-A6820"] <= AC.LDS_MAX
    ref = {c.name: AC.lds_bytes(c, AC.F32) for c, dt, _, why in AC.refused_cases() if why == "lds"}
    assert AC.LDS_MAX < ref["refuse-fwd-lds-H10240"] < AC.LDS_MAX + 128 and AC.LDS_MAX < ref["refuse-step-lds-A6824"] < AC.LDS_MAX + 128


def test_no_buffer_is_large():
    for c, dt in EVERY + [(c, dt if dt in BOTH else AC.F32) for c, dt, _, _ in AC.refused_cases()]:
        for name, l in AC.layout(c, dt).items():
            assert l["elems"] * 4 <= 4 * 2 ** 20, (c, name, l["elems"])


@pytest.mark.parametrize("op", AC.OPS)
def test_float32_restatement_stays_within_a_quarter_of_the_bound(op):
    worst = 0.0
    for c, dt in EVERY:
        if c.op != op:
            continue
        x = AC.inputs(c, dt)
        ref, tol = AC.reference(x, out_bf16=False)                                       # (the restatement stops before that rounding)
        for form in AC.FORMS[op]:
            if form.startswith("factored") and dt != AC.BF16:
                continue
            got = AC.restated_f32(x, form)
            assert set(got) == set(ref)
            for n in ref:
                r = AC.worst_ratio(got[n], ref[n], tol[n])
                key = (op, n, form)
                if r >= WORST.get(key, (-1.0,))[0]:
                    WORST[key] = (r, "%s %s" % (c.name, AC.DT_NAMES[dt]))
                assert r <= 0.25, (c, dt, form, n, r)
                worst = max(worst, r)
    assert worst > 0.01                                                                 # (a bound hundreds of times too wide says nothing)


def test_planted_mistakes_leave_the_bound():
    def ratio(c, dt, change, out):
        x = AC.inputs(c, dt)
        ref, tol = AC.reference(x, out_bf16=False)
        change(x)
        return AC.worst_ratio(AC.restated_f32(x, "tanhf")[out], ref[out], tol[out])
    fw = next(c for c in FWD if c.name == "fwd-mask-holes-R37")
    st = next(c for c in STEP if c.name == "step-nslab5-generic")
    ac = next(c for c in ACCUM if c.name == "accum-base")

    def last_chunk(x):                                                                  # the last 16-byte chunk of p_att's rows of region 36
        x.p_att[:, 36, -4:] = 0

    def drop_slab(x):
        x.dctx = x.dctx[:-1]

    def one_step_more(x):
        x.case = AC.Case("x", "accum", T=7, R=37, A=72, H=40, N=3, row_len=(7, 4, 9))
    assert ratio(fw, AC.F32, last_chunk, "alpha") > 100
    assert ratio(fw, AC.F32, lambda x: x.mask.__setitem__((0, 1), 1.0 - x.mask[0, 1]), "alpha") > 1e6
    assert ratio(st, AC.F32, drop_slab, "dctx") > 1 and ratio(st, AC.F32, drop_slab, "de") > 10
    assert ratio(st, AC.F32, lambda x: x.alpha.__setitem__((0, 36), 0.0), "de") > 100
    assert ratio(ac, AC.F32, one_step_more, "d_p_att") > 100 and ratio(ac, AC.F32, one_step_more, "d_att") > 100
    assert ratio(ac, AC.F32, lambda x: x.w_alpha.__setitem__(-1, 0.0), "d_p_att") > 100
