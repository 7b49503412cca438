"""The LSTM cell backward kernels on their own, through raw pointers: lstm_bwd_kernel, lstm_bwd_vec4_kernel<T, SIMPLE> (both
variants) and maxout_lstm_bwd_kernel (csrc/lstm_cell.hip) behind uic_lstm_cell_bwd_sources / uic_maxout_lstm_cell_bwd, and
h2att_cell_bwd_kernel<KS> (csrc/bptt_fused.hip; the kernel of the benchmarked step) behind uic_h2att_cell_bwd.

Every case (tests/lstm_cell_cases.py; tests/test_lstm_cell_cases_host.py shows on the CPU what the list reaches) checks
  * all five outputs, ELEMENT BY ELEMENT, against the float64 reference on the stored gates with the bound of that module
    (C = 32 units of eps x the element's own magnitude, plus 2^-8 |ref| for a bf16 result) -- no whole-tensor norm;
  * the kernel the launcher reports against the restated choice (LC.classify);
  * that a second launch from the same inputs gives the same bits;
  * that nothing but the views of dgates and dc is written: every operand is a view into a buffer of NaN canaries (strided sources
    as Step::bwd_step passes them: a column block of a wider row), the inputs and all canaries keep their bits -- for the fused
    operator that includes rows N ... of the last 32-row tile of dgates and dc.
The dropout factors are the library's own (uic_dropout_mask).

Measured on an MI355X, 226 cases in 4.9 s (the slowest 0.6 s, the first launch): worst error / bound over all cases.  The bf16
gate gradients are bounded by their own rounding (2^-8 |ref|; a round-to-nearest bf16 takes up to 0.996 of it), so what measures
the arithmetic there is dc, which is f32 in both dtypes; x 32 gives the error in units of eps x the element's magnitude.
    kernel                          f32: d_i    d_f    d_g    d_o    dc      bf16: dgates (worst)   dc
    lstm_bwd_kernel                      0.170  0.180  0.168  0.179  0.150         0.9955           0.206
    lstm_bwd_vec4_kernel<T, false>       0.139  0.133  0.116  0.146  0.104         0.9956           0.184
    lstm_bwd_vec4_kernel<T, true>        0.151  0.128  0.100  0.158  0.093         0.9956           0.194
    maxout_lstm_bwd_kernel               0.126  0.119  0.084  0.104  0.089         0.9953           0.094
    h2att_cell_bwd_kernel<1>             -                                         0.9882           0.074
    h2att_cell_bwd_kernel<2>             -                                         0.9901           0.041
    h2att_cell_bwd_kernel<4>             -                                         0.9933           0.048
The largest, 0.206 (6.6 units), is dc on the bf16 path's exp / rcp tanh; the CPU restatement of the same form gives 6.5.  Nothing
comes near C = 32.  Every run of this module with -s prints the table again.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

import lstm_cell_cases as LC

pytestmark = pytest.mark.gpu

NAN = float("nan")
WORST = {}
KERNEL_NAMES = ("lstm_bwd_kernel", "lstm_bwd_vec4_kernel<false>", "lstm_bwd_vec4_kernel<true>")
DT_NAMES = ("f32", "bf16")


def _L():
    from unpaired_image_captioning_amd import _lib
    return _lib


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print("\n[lstm cell] %-30s %-4s %-5s worst error / bound: %.4f  (%s)" % (k + WORST[k]))


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class Call:
    """The operands of one case laid out as LC.layout says, on `dev`."""

    def __init__(self, case, dt, dev="cuda"):
        self.case, self.dt, self.dev = case, dt, dev
        self.lay = LC.layout(case, dt)
        self.x = x = LC.inputs(case, dt)
        src = {"dc": x.dc, "c": x.c, "c_prev": x.c_prev, "gates": x.gates.reshape(case.M, -1), "slabA": x.slabA, "slabB": x.slabB,
               "datth": x.datth, "h2attT": x.h2attT, "dh0": x.dh[0], "dh1": x.dh[1], "dh2": x.dh[2]}
        self.buf, self.view, self.inside = {}, {}, {}
        for name, l in self.lay.items():
            tdt = torch.bfloat16 if LC.esize(name, dt) == 2 else torch.float32
            if l["sparse"]:                                                   # (over 2 GiB: only the view is written and checked)
                b = torch.empty(l["elems"], dtype=tdt, device=dev)
            else:
                b = torch.full((l["elems"],), NAN, dtype=tdt, device=dev)
                m = torch.zeros(l["elems"], dtype=torch.bool, device=dev)
                torch.as_strided(m, l["shape"], l["strides"], l["start"]).fill_(True)
                self.inside[name] = m
            self.buf[name] = b
            self.view[name] = torch.as_strided(b, l["shape"], l["strides"], l["start"])
            if name != "dgates":
                self.view[name].copy_(torch.from_numpy(np.ascontiguousarray(src[name])).to(dev))
        self.mask = None
        if case.drop_p > 0:
            L = _L()
            out = torch.empty(case.M * case.H, device=dev)
            L.check(L.load().uic_dropout_mask(L.ptr(out), case.M * case.H, case.drop_p, case.seed, case.site, 0, L.stream()), "dropout_mask")
            self.mask = out.cpu().double().numpy().reshape(case.M, case.H)
        self.before = {n: (self.view[n] if self.lay[n]["sparse"] else b).clone() for n, b in self.buf.items()}

    def p(self, name):
        if name not in self.buf:
            return None
        return self.buf[name].data_ptr() + self.lay[name]["start"] * LC.esize(name, self.dt)

    def launch(self):
        """One launch.  Returns (return code, kernel id or None)."""
        L = _L()
        lib, c, p = L.load(), self.case, self.p
        ld = [l[0] if l is not None else 0 for l in c.dh]
        slabs = (p("slabA"), c.layA[0] if c.nA else 0, c.nA, c.strideA if c.nA else 0, p("slabB"), c.layB[0] if c.nB else 0, c.nB,
                 c.strideB if c.nB else 0)
        tail = (p("dc"), p("gates"), p("c_prev"), p("c"), p("dgates"))
        if c.op == "cell":
            kid = ctypes.c_int32(-1)
            rc = lib.uic_lstm_cell_bwd_sources(self.dt, c.M, c.H, p("dh0"), ld[0], c.drop_p, c.seed, c.site, p("dh1"), ld[1], p("dh2"), ld[2],
                                               *slabs, *tail, ctypes.byref(kid), L.stream())
            return rc, kid.value
        if c.op == "maxout":
            return lib.uic_maxout_lstm_cell_bwd(self.dt, c.M, c.H, p("dh0"), ld[0], p("dh1"), ld[1], c.drop_p, c.seed, c.site, *tail, L.stream()), None
        return lib.uic_h2att_cell_bwd(self.dt, c.M, c.H, c.A, p("datth"), p("h2attT"), *slabs, *tail, L.stream()), None

    def results(self):
        """{output name: float64 [M, H]} in the order of LC.reference."""
        c = self.case
        dg = self.view["dgates"].float().cpu().double().numpy().reshape(c.M, c.G, c.H)
        names = ("d_i", "d_f", "d_o", "d_g1", "d_g2") if c.op == "maxout" else ("d_i", "d_f", "d_g", "d_o")
        out = {n: dg[:, q] for q, n in enumerate(names)}
        out["dc"] = self.view["dc"].cpu().double().numpy()
        return out

    def untouched(self):
        """Names of the buffers in which a bit changed that the call has no business changing."""
        bad = []
        for n, b in self.buf.items():
            if self.lay[n]["sparse"]:
                same = torch.equal(bits(self.view[n].contiguous()), bits(self.before[n].contiguous()))
            elif n in ("dgates", "dc"):
                out = ~self.inside[n]
                same = torch.equal(bits(b)[out], bits(self.before[n])[out])
            else:
                same = torch.equal(bits(b), bits(self.before[n]))
            if not same:
                bad.append(n)
        return bad

    def output_bits(self):
        return bits(self.buf["dgates"]).clone(), bits(self.buf["dc"]).clone()

    def reset(self):
        for n in ("dgates", "dc"):
            self.buf[n].copy_(self.before[n])


def sync():
    torch.cuda.synchronize()


def run_case(case, dt, kernel_name=None):
    L = _L()
    call = Call(case, dt)
    rc, kid = call.launch()
    L.check(rc, case.name)
    sync()
    first = call.output_bits()
    got = call.results()
    ref, tol = LC.reference(call.x, call.mask)
    assert list(got) == list(ref)
    problems = []
    if case.op == "cell":
        want = LC.classify(case, dt)
        kernel_name = KERNEL_NAMES[kid] if 0 <= kid < 3 else "?"
        if kid != want:
            problems.append("kernel %d, the restated choice says %d (%s)" % (kid, want, sorted(LC.broken_conditions(case, dt))))
    for n in ref:
        r = LC.worst_ratio(got[n], ref[n], tol[n])
        print("[lstm cell] %s %s %s %s: worst error / bound %.4f" % (case.name, DT_NAMES[dt], kernel_name, n, r))
        key = (kernel_name, DT_NAMES[dt], n)
        if r >= WORST.get(key, (-1.0,))[0]:
            WORST[key] = (r, case.name)
        if not r <= 1.0:
            err = np.abs(got[n] - ref[n])
            err = np.where(np.isfinite(err), err, np.inf)
            at = np.unravel_index(np.argmax(err / np.maximum(tol[n], LC.TINY ** 2)), err.shape)
            problems.append("%s leaves the bound: %.3f x at %s (got %r, reference %r, bound %.3g; %d elements outside)"
                            % (n, r, at, got[n][at], ref[n][at], tol[n][at], int((err > tol[n]).sum())))
    bad = call.untouched()
    if bad:
        problems.append("written outside dgates / dc, or an input changed: %s" % bad)
    call.reset()
    rc2, kid2 = call.launch()
    L.check(rc2, case.name)
    sync()
    second = call.output_bits()
    if not (torch.equal(first[0], second[0]) and torch.equal(first[1], second[1]) and kid2 == kid):
        problems.append("a second launch from the same inputs differs")
    assert not problems, (case.name, DT_NAMES[dt], problems)


def _params(cases):
    ps = [(c, dt) for c in cases for dt in c.dtypes]
    return dict(argnames="case,dt", argvalues=ps, ids=["%s-%s" % (c.name, DT_NAMES[dt]) for c, dt in ps])


@pytest.mark.parametrize(**_params([c for c in LC.cell_cases() if not c.far]))
def test_cell_backward_sources(case, dt):
    run_case(case, dt)


@pytest.mark.parametrize(**_params([c for c in LC.cell_cases() if c.far]))
def test_cell_backward_source_beyond_2_gib(case, dt):
    """Slice 1 of slabA begins at byte offset 2^31 from the slab pointer: out of reach of the vec4 kernel's 32-bit buffer offsets
    (it would be read as zeros), so the launcher must take the scalar kernel, and the result holds the same bound."""
    free, _ = torch.cuda.mem_get_info()
    if free < 4 * 2 ** 30:
        pytest.skip("needs 4 GiB of free device memory, %.1f GiB are free" % (free / 2 ** 30))
    run_case(case, dt)
    torch.cuda.empty_cache()


@pytest.mark.parametrize(**_params(LC.maxout_cases()))
def test_maxout_cell_backward(case, dt):
    run_case(case, dt, "maxout_lstm_bwd_kernel")


@pytest.mark.parametrize(**_params(LC.fused_cases()))
def test_h2att_cell_backward_fused(case, dt):
    run_case(case, dt, "h2att_cell_bwd_kernel<%d>" % (case.A // 128))


@pytest.mark.parametrize("case,dt,why", LC.fused_refused(), ids=[c.name for c, _, _ in LC.fused_refused()])
def test_h2att_cell_backward_refuses_what_it_cannot_run(case, dt, why):
    call = Call(case, dt)
    rc, _ = call.launch()
    sync()
    assert rc != 0
    msg = _L().load().uic_last_error_string().decode()
    assert "h2att_cell_bwd: shape not eligible" in msg, msg
    assert not call.untouched()
    assert torch.equal(bits(call.buf["dgates"]), bits(call.before["dgates"])) and torch.equal(bits(call.buf["dc"]), bits(call.before["dc"]))


def test_bad_arguments_are_refused_and_nothing_is_launched():
    L = _L()
    lib = L.load()
    case = LC.Case("args", M=6, H=32, nA=1, nB=1, **LC.GEN)
    for dt in (LC.F32, LC.BF16):
        call = Call(case, dt)
        p = call.p
        good = dict(dt=dt, M=6, H=32, dh0=p("dh0"), ld0=32, drop_p=0.0, dh1=p("dh1"), ld1=96, dh2=p("dh2"), ld2=64, A=p("slabA"), ldA=96, nA=1, B=p("slabB"),
                    ldB=64, nB=1, dc=p("dc"), gates=p("gates"), c_prev=p("c_prev"), c=p("c"), dgates=p("dgates"))

        def go(**kw):
            a = dict(good, **kw)
            return lib.uic_lstm_cell_bwd_sources(a["dt"], a["M"], a["H"], a["dh0"], a["ld0"], a["drop_p"], 1, 2, a["dh1"], a["ld1"], a["dh2"], a["ld2"],
                                                 a["A"], a["ldA"], a["nA"], 6 * 96, a["B"], a["ldB"], a["nB"], 6 * 64, a["dc"], a["gates"], a["c_prev"],
                                                 a["c"], a["dgates"], None, L.stream())
        for bad in (dict(dc=None), dict(gates=None), dict(c=None), dict(dgates=None), dict(M=-1), dict(H=0), dict(H=-4), dict(nA=-1), dict(nB=-1),
                    dict(A=None), dict(B=None), dict(ld0=31), dict(ld1=31), dict(ld2=0), dict(ldA=31), dict(ldB=31), dict(drop_p=1.0),
                    dict(drop_p=-0.5), dict(drop_p=NAN), dict(dt=7)):
            assert go(**bad) != 0, bad
            assert lib.uic_last_error_string(), bad
        assert go(M=0) == 0                                                   # a no-op
        sync()
        assert not call.untouched() and torch.equal(bits(call.buf["dgates"]), bits(call.before["dgates"]))
        assert torch.equal(bits(call.buf["dc"]), bits(call.before["dc"]))
        # absent sources are not looked at: their leading dimensions and pointers may be anything
        assert go(dh1=None, ld1=0, dh2=None, ld2=0, nA=0, A=None, ldA=0, nB=0, B=None, ldB=0) == 0
        sync()
        x = copy.copy(call.x)
        x.dh, x.slabA, x.slabB = [call.x.dh[0], None, None], None, None
        ref, tol = LC.reference(x, None)
        got = call.results()
        for n in ref:
            assert LC.worst_ratio(got[n], ref[n], tol[n]) <= 1.0, (dt, n)
        assert not call.untouched()
        tail = (p("dc"), p("gates"), p("c_prev"), p("c"), p("dgates"))
        assert lib.uic_maxout_lstm_cell_bwd(dt, 6, 32, p("dh0"), 31, None, 0, 0.0, 1, 2, *tail, L.stream()) != 0
        assert lib.uic_maxout_lstm_cell_bwd(dt, 6, 32, p("dh0"), 32, None, 0, 1.0, 1, 2, *tail, L.stream()) != 0
        assert lib.uic_maxout_lstm_cell_bwd(dt, 6, 0, p("dh0"), 32, None, 0, 0.0, 1, 2, *tail, L.stream()) != 0
        assert lib.uic_maxout_lstm_cell_bwd(dt, 0, 32, p("dh0"), 32, None, 0, 0.0, 1, 2, *tail, L.stream()) == 0
    f = Call(LC.Case("fargs", op="fused", M=33, H=96, A=256, nA=2, nB=2, layA=((3, 0), (1, 0)), layB=((2, 0), (1, 0))), LC.BF16)
    p = f.p
    tail = (p("dc"), p("gates"), p("c_prev"), p("c"), p("dgates"))

    def fused(N=33, H=96, A=256, a=p("datth"), b=p("h2attT"), sA=p("slabA"), ldA=288, nA=2, sB=p("slabB"), ldB=192, nB=2):
        return lib.uic_h2att_cell_bwd(LC.BF16, N, H, A, a, b, sA, ldA, nA, 33 * 288, sB, ldB, nB, 33 * 192, *tail, L.stream())
    for bad in (dict(N=-1), dict(H=0), dict(A=0), dict(a=None), dict(b=None), dict(sA=None), dict(nA=-1), dict(nB=-2), dict(ldA=95), dict(ldB=64)):
        assert fused(**bad) != 0, bad
    assert fused(N=0) == 0
    sync()
    assert not f.untouched() and torch.equal(bits(f.buf["dgates"]), bits(f.before["dgates"]))
