"""The nine kernels of csrc/attention.hip on their own, through raw pointers and with every argument the model steps pass:
uic_attention_fwd_strided (attn_fwd_kernel, attn_fwd_fast_kernel<FULL>), uic_attention_bwd_step_sources (attn_bwd_step_kernel,
attn_bwd_step_fast_kernel<FULL>) and uic_attention_bwd_accum_strided (attn_bwd_accum_kernel<PART>, attn_bwd_accum_p1_kernel,
attn_bwd_accum_p2_bf16_kernel).

Every case (tests/attention_cases.py; tests/test_attention_cases_host.py shows on the CPU what the list reaches) checks
  * every output -- alpha, ctx; de, d_att_h, dctx_sum; d_att, d_p_att, part -- ELEMENT BY ELEMENT against the float64 reference on
    the stored operands with the bound of that module (counted roundings x the element's own magnitude, + 2^-8 |ref| for a bf16
    result) -- no whole-tensor norm; masked regions have alpha == 0 exactly, sum alpha = 1 and sum de = 0 within their bounds;
  * the kernel the launcher reports against the restated choice (AC.classify);
  * that a second launch from the same inputs gives the same bits;
  * that nothing but the views of the outputs is written: every operand is a view into a buffer of NaN canaries (d ctx a column
    block of a 3H-wide row, ctx and dctx_sum rows of a wider buffer), inputs and canaries keep their bits;
  * rows behind their caption's end (step >= row_len[n]): exact zeros in de, d_att_h and dctx_sum while ALL their operands hold NaN;
    steps behind the end of an accumulation hold NaN as well;
  * dctx_sum equals the sequential float32 sum of the slabs bit for bit, in the fast and in the generic kernel.
Refused calls return non-zero, name the operator, leave every buffer untouched, and the next valid call works.

Measured on an MI355X: 579 tests (235 cases = 465 calls over the dtypes, 102 refusals, 12 others) in 4.2 s, the slowest 0.5 s (the first
launch).  Worst error / bound over all cases, per kernel, dtype and output.  Results stored in bf16 (ctx, d_att_h, d_p_att) are
bounded by their own rounding (2^-8 |ref|; round-to-nearest takes up to 0.996 of it), so there the f32 outputs of the same kernel
(alpha, de, dctx_sum, part) measure the arithmetic.
    kernel                              f32: outputs                                   bf16: outputs
    attn_fwd_kernel                     alpha 0.035  ctx 0.011                         alpha 0.032  ctx 0.924
    attn_fwd_fast_kernel<FULL=0>        alpha 0.038  ctx 0.012                         alpha 0.303  ctx 0.975
    attn_fwd_fast_kernel<FULL=1>        alpha 0.012  ctx 0.005                         alpha 0.725  ctx 0.934
    attn_bwd_step_kernel                de 0.074  d_att_h 0.020  dctx_sum 0.126        de 0.054  d_att_h 0.973  dctx_sum 0.158
    attn_bwd_step_fast_kernel<FULL=0>   de 0.074  d_att_h 0.019  dctx_sum 0.113        de 0.052  d_att_h 0.938  dctx_sum 0.121
    attn_bwd_step_fast_kernel<FULL=1>   de 0.024  d_att_h 0.007  dctx_sum 0.149        de 0.018  d_att_h 0.944  dctx_sum 0.158
    attn_bwd_accum_kernel<PART=1>       d_att 0.152                                    d_att 0.152
    attn_bwd_accum_p1_kernel            d_att 0.159                                    d_att 0.159
    attn_bwd_accum_kernel<PART=2>       d_p_att 0.090  part 0.093                      d_p_att 0.988  part 0.070
    attn_bwd_accum_p2_bf16_kernel       -                                              d_p_att 0.991  part 0.102
The largest arithmetic figure, 0.725, is alpha of the bf16 fast-full forward kernel where the scores of a row spread over 110
(fwd-spread110-R36): v_exp_f32 at arguments near -100, inside the 3 u |e - max| the bound gives the exponent's argument.  Nothing
else passes a third of its bound; the CPU restatement of the same formulas stays below a quarter.  Every run of this module with
-s prints the table again.
"""
import ctypes

import numpy as np
import pytest
import torch

import attention_cases as AC

pytestmark = pytest.mark.gpu

NAN = float("nan")
INT_CANARY = -7777
WORST = {}
OUT_BF16 = ("ctx", "d_att_h", "d_p_att")


def _L():
    from unpaired_image_captioning_amd import _lib
    return _lib


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n[attention] worst error / bound per kernel, dtype and output (the case)")
    for k in sorted(WORST):
        print("[attention] %-36s %-4s %-8s %.4f  (%s)" % (k + WORST[k]))


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def sync():
    torch.cuda.synchronize()


class Call:
    """The operands of one case laid out as AC.layout says, on the device; `dt` is what the call passes, which may be no dtype."""

    def __init__(self, case, dt, null=None, dev="cuda"):
        self.case, self.dt, self.null, self.dev = case, dt, null, dev
        self.ldt = ldt = dt if dt in (AC.F32, AC.BF16) else AC.F32
        self.lay = AC.layout(case, ldt)
        self.x = x = AC.inputs(case, ldt)
        src = {"p_att": x.p_att, "w_alpha": x.w_alpha, "row_len": x.row_len}
        if case.op == "accum":
            src.update(att_h_all=x.att_h, alpha_all=x.alpha_all, de_all=x.de_all, dctx_all=x.dctx_all)
        else:
            src.update(att_h=x.att_h, att=x.att)
            if case.op == "fwd":
                src.update(b_alpha=None if x.b_alpha is None else np.asarray([x.b_alpha], dtype=np.float32), mask=x.mask)
            else:
                src.update(alpha=x.alpha, dctx=x.dctx)
        self.outputs = AC.OUTPUTS[case.op]
        self.buf, self.view, self.inside = {}, {}, {}
        for name, l in self.lay.items():
            if name == "row_len":
                b = torch.full((l["elems"],), INT_CANARY, dtype=torch.int32, device=dev)
            else:
                b = torch.full((l["elems"],), NAN, dtype=torch.bfloat16 if AC.esize(name, ldt) == 2 else torch.float32, device=dev)
            m = torch.zeros(l["elems"], dtype=torch.bool, device=dev)
            torch.as_strided(m, l["shape"], l["strides"], l["start"]).fill_(True)
            self.inside[name] = m
            self.buf[name] = b
            self.view[name] = torch.as_strided(b, l["shape"], l["strides"], l["start"])
            if name in src and src[name] is not None:
                self.view[name].copy_(torch.from_numpy(np.ascontiguousarray(src[name])).to(dev))
        # what a kernel has no business reading holds NaN: the rows behind their caption's end, the steps behind a row's last
        if case.op == "step" and case.row_len is not None:
            dead = torch.from_numpy(~case.live_rows()).to(dev)
            for name in ("p_att", "att", "att_h", "alpha"):
                self.view[name][dead] = NAN
            self.view["dctx"][:, dead] = NAN
        if case.op == "accum" and case.row_len is not None:
            gone = torch.from_numpy(np.arange(case.T)[:, None] >= case.ts()[None, :]).to(dev)
            for name in ("att_h_all", "alpha_all", "de_all", "dctx_all"):
                self.view[name][gone] = NAN
        self.before = {n: b.clone() for n, b in self.buf.items()}

    def p(self, name):
        if name not in self.buf or name == self.null:
            return None
        return self.buf[name].data_ptr() + self.lay[name]["start"] * AC.esize(name, self.ldt)

    def launch(self, N=None, **kw):
        """One launch.  Returns (return code, kernel id).  kw overrides integer arguments by name."""
        L = _L()
        lib, c, p, dt = L.load(), self.case, self.p, self.ldt
        kid = ctypes.c_int32(-1)
        N = c.N if N is None else N
        a = dict(R=c.R, A=c.A(dt), H=c.H(dt), T=c.T, ld_mask=c.ld_mask() if c.mask else 0, ld_ctx=c.ld_ctx(dt), lddctx=c.lddctx(dt),
                 nslab=c.nslab, stride=c.stride(dt), ld_sum=c.ld_sum(dt) if c.dsum else 0, step=c.step if c.row_len is not None else 0)
        a.update(kw)
        dims = (self.dt, N, a["R"], a["A"], a["H"])
        if c.op == "fwd":
            rc = lib.uic_attention_fwd_strided(*dims, p("att_h"), p("p_att"), p("att"), p("w_alpha"), p("b_alpha"), p("mask"), a["ld_mask"],
                                               p("alpha"), p("ctx"), a["ld_ctx"], ctypes.byref(kid), L.stream())
        elif c.op == "step":
            rc = lib.uic_attention_bwd_step_sources(*dims, p("att_h"), p("p_att"), p("att"), p("w_alpha"), p("alpha"), p("dctx"), a["lddctx"],
                                                    a["nslab"], a["stride"], p("dctx_sum"), a["ld_sum"], p("row_len"), a["step"], p("de"),
                                                    p("d_att_h"), ctypes.byref(kid), L.stream())
        else:
            rc = lib.uic_attention_bwd_accum_strided(*dims, a["T"], p("att_h_all"), p("alpha_all"), p("de_all"), p("dctx_all"), a["lddctx"],
                                                     a["stride"], p("row_len"), p("p_att"), p("w_alpha"), p("d_att"), p("d_p_att"), p("part"),
                                                     ctypes.byref(kid), L.stream())
        return rc, kid.value

    def results(self):
        return {n: self.view[n].float().cpu().double().numpy() for n in self.outputs if n in self.view}

    def changed(self, outputs_too=False):
        """Names of the buffers in which a bit changed that the call has no business changing."""
        bad = []
        for n, b in self.buf.items():
            if n in self.outputs and not outputs_too:
                out = ~self.inside[n]
                same = torch.equal(bits(b)[out], bits(self.before[n])[out])
            else:
                same = torch.equal(bits(b), bits(self.before[n]))
            if not same:
                bad.append(n)
        return bad

    def output_bits(self):
        return [bits(self.buf[n]).clone() for n in self.outputs if n in self.buf]

    def reset(self):
        for n in self.outputs:
            if n in self.buf:
                self.buf[n].copy_(self.before[n])


def run_case(case, dt):
    L = _L()
    call = Call(case, dt)
    rc, kid = call.launch()
    L.check(rc, case.name)
    sync()
    first = call.output_bits()
    got = call.results()
    ref, tol = AC.reference(call.x)
    problems = []
    want = AC.classify(case, dt)
    if kid != want:
        parts = ("p1", "p2") if case.op == "accum" else (None,)
        problems.append("kernel id %d, the restated choice says %d (%s)" % (kid, want, [sorted(AC.broken_conditions(case, dt, q)) for q in parts]))
    for n in got:
        r = AC.worst_ratio(got[n], ref[n], tol[n])
        key = (AC.kernel_of(case, dt, n), AC.DT_NAMES[dt], n)
        if r >= WORST.get(key, (-1.0,))[0]:
            WORST[key] = (r, case.name)
        if not r <= 1.0:
            err = np.abs(got[n] - ref[n])
            err = np.where(np.isfinite(err), err, np.inf)
            at = np.unravel_index(np.argmax(err / np.maximum(tol[n], AC.TINY ** 2)), err.shape)
            problems.append("%s leaves the bound: %.3f x at %s (got %r, reference %r, bound %.3g; %d elements outside)"
                            % (n, r, at, got[n][at], ref[n][at], tol[n][at], int((err > tol[n]).sum())))
    if case.op == "fwd":
        off = np.abs(got["alpha"].sum(1) - 1.0)
        if not (off <= tol["alpha"].sum(1)).all():
            problems.append("sum alpha != 1: off by %r, bound %r" % (off, tol["alpha"].sum(1)))
        if case.mask and np.any(got["alpha"][call.x.mask == 0] != 0.0):
            problems.append("a masked region has alpha != 0")
    if case.op == "step":
        off = np.abs(got["de"].sum(1))
        if not (off <= tol["de"].sum(1) + AC.TINY).all():
            problems.append("sum de != 0: %r, bound %r" % (off, tol["de"].sum(1)))
        if case.dsum:
            mine = bits(call.view["dctx_sum"].contiguous()).cpu()
            seq = bits(torch.from_numpy(AC.dctx_sum_f32(call.x)))
            if not torch.equal(mine, seq):
                problems.append("dctx_sum is not the sequential float32 sum of the slabs")
        dead = ~case.live_rows()
        for n in got:
            if np.any(got[n][dead] != 0.0):
                problems.append("%s of a row behind its caption's end is not zero" % n)
    bad = call.changed()
    if bad:
        problems.append("written outside the outputs, or an input changed: %s" % bad)
    call.reset()
    rc2, kid2 = call.launch()
    L.check(rc2, case.name)
    sync()
    second = call.output_bits()
    if kid2 != kid or not all(torch.equal(a, b) for a, b in zip(first, second)):
        problems.append("a second launch from the same inputs differs")
    assert not problems, (case.name, AC.DT_NAMES[dt], problems)
    return call


def _params(cases):
    ps = [(c, dt) for c in cases for dt in c.dtypes]
    return dict(argnames="case,dt", argvalues=ps, ids=["%s-%s" % (c.name, AC.DT_NAMES[dt]) for c, dt in ps])


@pytest.mark.parametrize(**_params(AC.fwd_cases()))
def test_attention_forward(case, dt):
    run_case(case, dt)


@pytest.mark.parametrize(**_params(AC.step_cases()))
def test_attention_backward_step(case, dt):
    run_case(case, dt)


@pytest.mark.parametrize(**_params(AC.accum_cases()))
def test_attention_backward_accumulation(case, dt):
    run_case(case, dt)


@pytest.mark.parametrize("shape", ["R36-64x64", "R36-2x3"])
@pytest.mark.parametrize("dt", [AC.F32, AC.BF16])
def test_fast_and_generic_step_kernel_agree_on_dctx_sum(shape, dt):
    """lddctx = H against H + 2 flips the kernel without touching the data: the slabs' sum must not depend on it."""
    by = {c.name: c for c in AC.step_cases()}
    a, b = by["step-lddctx-1-0-" + shape], by["step-lddctx-1-2-" + shape]
    assert AC.classify(a, dt) != AC.GENERIC and AC.classify(b, dt) == AC.GENERIC and a.nslab == b.nslab == 3
    out = []
    for c in (a, b):
        call = Call(c, dt)
        rc, kid = call.launch()
        _L().check(rc, c.name)
        sync()
        assert kid == AC.classify(c, dt)
        out.append((bits(call.view["dctx_sum"].contiguous()).cpu(), bits(call.view["de"].contiguous()).cpu(), call.x))
    assert np.array_equal(out[0][2].dctx, out[1][2].dctx)
    assert torch.equal(out[0][0], out[1][0])


_REFUSED = AC.refused_cases()


@pytest.mark.parametrize("case,dt,null,why", _REFUSED, ids=["%s-dt%d" % (c.name, dt) for c, dt, _, _ in _REFUSED])
def test_what_no_kernel_can_run_is_refused_and_nothing_is_launched(case, dt, null, why):
    lib = _L().load()
    call = Call(case, dt, null=null)
    rc, _ = call.launch()
    sync()
    assert rc != 0, why
    msg = lib.uic_last_error_string().decode()
    assert AC.OP_NAMES[case.op] + ":" in msg, msg
    if why == "lds":
        assert "of LDS" in msg, msg
    if why.endswith("_al"):
        assert "aligned" in msg, msg
    assert not call.changed(outputs_too=True)
    # ... and the library goes on working
    ok = next(c for c in AC.all_cases() if c.op == case.op)
    run_case(ok, AC.F32)


@pytest.mark.parametrize("op", AC.OPS)
@pytest.mark.parametrize("dt", [AC.F32, AC.BF16])
def test_bad_arguments_and_the_empty_call(op, dt):
    lib = _L().load()
    case = {"fwd": AC.Case("args-fwd", "fwd", mask="prefix", ld_mask=2, ld_ctx=(2, 0)),
            "step": AC.Case("args-step", "step", nslab=2, dsum=True, lddctx=(3, 0), row_len=(3, 3, 3), step=1),
            "accum": AC.Case("args-accum", "accum", T=3, lddctx=(3, 0), row_len=(3, 2, 1))}[op]
    call = Call(case, dt)
    H, R = case.H(dt), case.R
    bad = [dict(N=-1), dict(R=0), dict(A=0), dict(H=0), dict(A=-8)]
    bad += {"fwd": [dict(ld_ctx=H - 1), dict(ld_mask=R - 1)],
            "step": [dict(lddctx=H - 1), dict(nslab=-1), dict(ld_sum=H - 1), dict(step=-1)],
            "accum": [dict(T=0), dict(T=-1), dict(lddctx=H - 1)]}[op]
    for kw in bad:
        rc, _ = call.launch(**kw)
        assert rc != 0, kw
        assert AC.OP_NAMES[op] + ":" in lib.uic_last_error_string().decode(), kw
    rc, kid = call.launch(N=0)                                                   # a no-op that still says which kernel it would be
    assert rc == 0 and kid == AC.classify(case, dt)
    sync()
    assert not call.changed(outputs_too=True)
    rc, _ = call.launch()
    assert rc == 0
    sync()
    ref, tol = AC.reference(call.x)
    for n, g in call.results().items():
        assert AC.worst_ratio(g, ref[n], tol[n]) <= 1.0, n
    assert not call.changed()


@pytest.mark.parametrize("dt", [AC.F32, AC.BF16])
def test_the_first_entries_are_the_new_ones_with_plain_strides(dt):
    """uic_attention_fwd / _bwd_step / _bwd_accum: ld_mask = R, ld_ctx = lddctx = H, step stride N H, no slabs, no row_len -- the same bits."""
    L = _L()
    lib = L.load()
    for case in (AC.Case("plain-fwd", "fwd", R=36, Av=64, Hv=64, mask="holes"), AC.Case("plain-step", "step", R=37),
                 AC.Case("plain-accum", "accum", T=5, R=7)):
        call = Call(case, dt)
        p, N, R, A, H = call.p, case.N, case.R, case.A(dt), case.H(dt)
        L.check(call.launch()[0], case.name)
        sync()
        new = call.output_bits()
        call.reset()
        if case.op == "fwd":
            rc = lib.uic_attention_fwd(dt, N, R, A, H, p("att_h"), p("p_att"), p("att"), p("w_alpha"), p("b_alpha"), p("mask"), p("alpha"), p("ctx"), L.stream())
        elif case.op == "step":
            rc = lib.uic_attention_bwd_step(dt, N, R, A, H, p("att_h"), p("p_att"), p("att"), p("w_alpha"), p("alpha"), p("dctx"), p("de"), p("d_att_h"),
                                            L.stream())
        else:
            rc = lib.uic_attention_bwd_accum(dt, N, R, A, H, case.T, p("att_h_all"), p("alpha_all"), p("de_all"), p("dctx_all"), p("p_att"), p("w_alpha"),
                                             p("d_att"), p("d_p_att"), p("part"), L.stream())
        L.check(rc, case.name)
        sync()
        assert all(torch.equal(a, b) for a, b in zip(new, call.output_bits())), case.name
        assert not call.changed()
