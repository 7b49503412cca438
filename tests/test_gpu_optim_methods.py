"""uic_optim_step / uic_optim_step_ranges (csrc/adam.hip) through the C ABI: every --i2t_optim / --nmt_optim method, with and
without weight decay, against the installed torch.optim class built as the reference's create_optimizer builds it
(P/misc/optimizer.py:59-74) and run on the CPU in float64; the ranges form against the whole-arena form bit for bit; the Adam
case against uic_adam_step bit for bit."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

METHODS = ("adam", "sgd", "sgdm", "sgdmom", "rmsprop", "adagrad")
STATES = {"adam": ("exp_avg", "exp_avg_sq"), "sgd": (), "sgdm": ("momentum_buffer",), "sgdmom": ("momentum_buffer",),
          "rmsprop": ("square_avg",), "adagrad": ("sum",)}
STEPS = 3


def _f32(x):
    """The value the C ABI's float argument carries.  The float64 reference gets the hyper-parameters the kernel gets: 1 - beta2
    of 0.999f is 4.7e-5 off 1 - 0.999, which is the caller's rounding, not the kernel's."""
    return float(torch.tensor(x, dtype=torch.float32))


LR, ALPHA, BETA, EPS, EPS_ADAGRAD = _f32(5e-4), _f32(0.9), _f32(0.999), _f32(1e-8), _f32(1e-10)
WDS = (0.0, _f32(1e-2))
BIG = 65536 * 256 + 5          # the first size at which uic_grid_for's grid-stride loop makes a second pass


def _L():
    from unpaired_image_captioning_amd import _lib
    return _lib


def _cfg(method, wd, step, lr=LR, grad_scale=1.0, max_norm=0.0, sqnorm=None, guard=None):
    L = _L()
    return L.OptimConfig(L.OPTIM_METHODS[method], lr, ALPHA, BETA, EPS_ADAGRAD if method == "adagrad" else EPS, wd, step, grad_scale, max_norm,
                         sqnorm.data_ptr() if sqnorm is not None else None, guard.data_ptr() if guard is not None else None)


def _torch_optim(method, params, lr, wd):
    """The reference's create_optimizer, call for call."""
    if method == "rmsprop":
        return torch.optim.RMSprop(params, lr, ALPHA, EPS, weight_decay=wd)
    if method == "adagrad":
        return torch.optim.Adagrad(params, lr, eps=EPS_ADAGRAD, weight_decay=wd)      # (torch's own 1e-10, as a float)
    if method == "sgd":
        return torch.optim.SGD(params, lr, weight_decay=wd)
    if method == "sgdm":
        return torch.optim.SGD(params, lr, ALPHA, weight_decay=wd)
    if method == "sgdmom":
        return torch.optim.SGD(params, lr, ALPHA, weight_decay=wd, nesterov=True)
    return torch.optim.Adam(params, lr, (ALPHA, BETA), EPS, weight_decay=wd)


@functools.lru_cache(maxsize=1)          # (the aligned and the offset case of one size follow each other and share it)
def _float64_run(method, wd, n):
    """STEPS steps of torch.optim in float64 on the CPU from f32 inputs.  Returns the inputs (p0, [g_k]), the final parameter and
    state, max_k |p_k|, max_k |d_k| (d_k = (p_{k-1} - p_k) / lr, the update direction) and, for the momentum buffer, the sum of
    the magnitudes of the terms that formed it: sum_k alpha^(K-k) (|g_k| + wd |p_{k-1}|) -- with weight decay the term added in
    step k is g_k + wd p_{k-1}, two terms (Adam's exp_avg: each weighted by 1 - alpha)."""
    gen = torch.Generator().manual_seed(1000 + n % 9973)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) for _ in range(STEPS)]
    idx = torch.arange(n)
    for k, g in enumerate(grads):
        g[idx % 7 == 3] = 0.0                      # exact zeros in every step: the state of these elements stays what decay makes it
        if k == 1:
            g[idx % 11 == 5] = 0.0                 # and a zero gradient over a non-zero state
    p = torch.nn.Parameter(p0.double())
    opt = _torch_optim(method, [p], LR, wd)
    pmax, dmax, terms = p0.double().abs(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for g in grads:
        before = p.detach().clone()
        p.grad = g.double()
        opt.step()
        after = p.detach()
        pmax = torch.maximum(pmax, after.abs())
        dmax = torch.maximum(dmax, ((before - after) / LR).abs())
        terms = ALPHA * terms + (1 - ALPHA if method == "adam" else 1.0) * (g.double().abs() + wd * before.abs())
    state = [opt.state[p][s].detach().clone() for s in STATES[method]]
    return p0, grads, p.detach().clone(), state, pmax, dmax, terms


def _device_run(method, wd, n, p0, grads, offset=0):
    """STEPS calls of uic_optim_step on arrays that start `offset` floats past a 256-byte boundary."""
    L = _L()
    lib = L.load()

    def arr(src=None):
        t = torch.zeros(n + 64, device="cuda")
        assert t.data_ptr() % 256 == 0
        v = t[offset:offset + n]
        if src is not None:
            v.copy_(src)
        return v
    p, g = arr(p0), arr()
    states = [arr() for _ in STATES[method]]
    s = [t.data_ptr() for t in states] + [None, None]
    assert lib.uic_optim_states(L.OPTIM_METHODS[method]) == len(states)
    for step, gr in enumerate(grads, 1):
        g.copy_(gr)
        L.check(lib.uic_optim_step(C.byref(_cfg(method, wd, step)), p.data_ptr(), g.data_ptr(), s[0], s[1], n, L.stream()), "optim_step")
    torch.cuda.synchronize()
    return p.cpu(), [t.cpu() for t in states]


SIZES = [(1, 0), (63, 0), (64, 0), (257, 0), (1027, 0), (1027, 1)]          # (n, floats past the 256-byte boundary)
CASES = [(m, wd, n, off) for m in METHODS for wd in WDS for n, off in SIZES + ([(BIG, 0)] if m == "sgdmom" else [])]


@pytest.mark.parametrize("method,wd,n,offset", CASES, ids=["%s-wd%g-n%d+%d" % c for c in CASES])
def test_optim_step_matches_torch_optim_in_float64(method, wd, n, offset):
    """Three steps, lr 5e-4, standard-normal p and g.  Per element
        |p_dev - p_ref| <= K 2^-24 max_k |p_k| + K 2^-20 lr max_k |d_k|,  K = 3 steps:
    one rounding of the stored parameter per step, and 16 ulp on the direction (its roundings, sqrtf, the division, the state's
    accumulated error).  State arrays within 4 K 2^-24 of the sum of the magnitudes of the terms that formed them: the value itself
    for square_avg, sum and exp_avg_sq, sum_k alpha^(K-k) |term_k| for momentum_buffer and exp_avg (_float64_run).  The size past
    65536 workgroups runs for sgdmom only: the second pass of the grid-stride loop is the launch geometry's, shared by all."""
    p0, grads, p_ref, s_ref, pmax, dmax, terms = _float64_run(method, wd, n)
    p_dev, s_dev = _device_run(method, wd, n, p0, grads, offset)
    K = STEPS
    err = (p_dev.double() - p_ref).abs()
    bound = K * 2.0 ** -24 * pmax + K * 2.0 ** -20 * LR * dmax
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print("%s wd=%g n=%d: max |p err| %.3e, worst err / bound %.3f, bound <= %.3e" % (method, wd, n, err.max().item(), worst, bound.max().item()))
    assert bool((err <= bound).all()), (err.max().item(), worst)
    assert bool((p_dev.double() - p0.double()).abs().max() > 0)
    for name, dev, ref in zip(STATES[method], s_dev, s_ref):
        mag = terms if name in ("momentum_buffer", "exp_avg") else ref.abs()
        serr = (dev.double() - ref).abs()
        sbound = 4 * K * 2.0 ** -24 * mag
        print("   %s: max err %.3e, worst err / bound %.3f" % (name, serr.max().item(), (serr / sbound.clamp_min(1e-300)).max().item()))
        assert bool((serr <= sbound).all()), (name, serr.max().item())


@pytest.mark.parametrize("wd", WDS, ids=["wd0", "wd1e-2"])
@pytest.mark.parametrize("w16", [False, True], ids=["f32", "bf16-copy"])
@pytest.mark.parametrize("clip,guard", [(False, None), (True, None), (False, 0), (False, 7)])
@pytest.mark.parametrize("method", METHODS)
def test_optim_step_ranges_is_optim_step_on_the_ranges_and_nowhere_else(method, clip, guard, w16, wd):
    """The layout of test_adam_step_ranges_is_adam_step_on_the_ranges_and_nowhere_else: five ranges (one empty, one single
    element, the tail), canaries around all four arrays and the operand copy.  Inside the ranges bit for bit what
    uic_optim_step leaves, nothing written outside them, the bf16 copy of exactly the updated elements, and behind a non-zero
    guard word nothing at all -- from either entry point."""
    L = _L()
    lib = L.load()
    g = torch.Generator().manual_seed(21)
    n, pad = 70016, 256
    ranges = [(0, 64), (128, 128), (4096, 4096 + 9984), (20032, 20032 + 1), (50048, 70016)]
    big = torch.full((5, n + 2 * pad), 7.25)
    p0, gr = torch.randn(n, generator=g), torch.randn(n, generator=g)
    s0, s1 = torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01
    if method not in ("adam", "sgdm", "sgdmom"):
        s0 = s0.abs()                                            # (square_avg and sum are sums of squares)
    for row, t in enumerate((p0, gr, s0, s1)):
        big[row, pad:pad + n] = t
    dev_big = big.cuda()
    P, G, S0, S1 = (dev_big[r, pad:pad + n] for r in range(4))
    w_out = torch.full((n + 2 * pad,), 3.0, device="cuda").bfloat16()
    W = w_out[pad:pad + n]
    sq = torch.tensor([float((gr * gr).sum()), 0.0], device="cuda") if clip else None      # (with decay: read as a float pair)
    gw = torch.tensor([0, guard if guard is not None else 0], dtype=torch.int32, device="cuda") if guard is not None else None
    cfg = _cfg(method, wd, 3, lr=5e-3, grad_scale=0.5, max_norm=0.25 if clip else 0.0, sqnorm=sq, guard=gw[1:2] if gw is not None else None)
    lo = (C.c_uint64 * len(ranges))(*[a for a, _ in ranges])
    hi = (C.c_uint64 * len(ranges))(*[b for _, b in ranges])
    # (all four pointers are handed in for every method: a method must ignore the state arrays it does not use)
    L.check(lib.uic_optim_step_ranges(C.byref(cfg), P.data_ptr(), G.data_ptr(), S0.data_ptr(), S1.data_ptr(), len(ranges), lo, hi,
                                      W.data_ptr() if w16 else None, 1 if w16 else 0, L.stream()), "optim_step_ranges")
    # the reference: the whole-arena kernel on copies, without the guard
    rp, rg, r0, r1 = p0.cuda(), gr.cuda(), s0.cuda(), s1.cuda()
    ref_cfg = _cfg(method, wd, 3, lr=5e-3, grad_scale=0.5, max_norm=0.25 if clip else 0.0, sqnorm=sq)
    L.check(lib.uic_optim_step(C.byref(ref_cfg), rp.data_ptr(), rg.data_ptr(), r0.data_ptr(), r1.data_ptr(), n, L.stream()), "optim_step")
    torch.cuda.synchronize()
    used = len(STATES[method])
    assert not torch.equal(rp.cpu(), p0) and torch.equal(rg.cpu(), gr)
    assert torch.equal(r0.cpu(), s0) == (used < 1) and torch.equal(r1.cpu(), s1) == (used < 2)
    inside = torch.zeros(n, dtype=torch.bool)
    for a, b in ranges:
        inside[a:b] = True
    skipped = guard is not None and guard != 0
    out = dev_big.cpu()
    for row, (new, old) in enumerate(((rp.cpu(), p0), (None, gr), (r0.cpu(), s0), (r1.cpu(), s1))):
        got = out[row, pad:pad + n]
        want = old.clone()
        if new is not None and not skipped:
            want[inside] = new[inside]
        assert torch.equal(got, want), (row, (got - want).abs().max().item(), (got != want).nonzero()[:4].tolist())
        assert (out[row, :pad] == 7.25).all() and (out[row, pad + n:] == 7.25).all(), row        # canaries
    assert (out[4] == 7.25).all()
    wo = w_out.float().cpu()
    assert (wo[:pad] == 3.0).all() and (wo[pad + n:] == 3.0).all()
    wmid = wo[pad:pad + n]
    if w16 and not skipped:
        assert torch.equal(wmid[inside], rp.cpu()[inside].bfloat16().float()) and (wmid[~inside] == 3.0).all()
    else:
        assert (wmid == 3.0).all()
    if skipped:                                                  # the whole-arena entry behind the same guard word
        qp, q0, q1 = p0.cuda(), s0.cuda(), s1.cuda()
        L.check(lib.uic_optim_step(C.byref(cfg), qp.data_ptr(), rg.data_ptr(), q0.data_ptr(), q1.data_ptr(), n, L.stream()), "optim_step")
        torch.cuda.synchronize()
        assert torch.equal(qp.cpu(), p0) and torch.equal(q0.cpu(), s0) and torch.equal(q1.cpu(), s1)


@pytest.mark.parametrize("clip", [False, True])
def test_adam_without_weight_decay_is_uic_adam_step_bit_for_bit(clip):
    L = _L()
    lib = L.load()
    g = torch.Generator().manual_seed(9)
    n = 100003
    p0, grads = torch.randn(n, generator=g), [torch.randn(n, generator=g) for _ in range(3)]
    new = [p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]
    old = [p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]
    for step, gr in enumerate(grads, 1):
        gd = gr.cuda()
        sq = torch.tensor([float((gr * gr).sum())], device="cuda") if clip else None
        cfg = _cfg("adam", 0.0, step, grad_scale=0.5, max_norm=5.0 if clip else 0.0, sqnorm=sq)
        L.check(lib.uic_optim_step(C.byref(cfg), new[0].data_ptr(), gd.data_ptr(), new[1].data_ptr(), new[2].data_ptr(), n, L.stream()))
        if clip:
            L.check(lib.uic_adam_step_clip(L.ptr(old[0]), L.ptr(gd), L.ptr(old[1]), L.ptr(old[2]), n, LR, ALPHA, BETA, EPS, step, 0.5, 5.0,
                                           L.ptr(sq), L.stream()))
        else:
            L.check(lib.uic_adam_step(L.ptr(old[0]), L.ptr(gd), L.ptr(old[1]), L.ptr(old[2]), n, LR, ALPHA, BETA, EPS, step, 0.5, L.stream()))
    torch.cuda.synchronize()
    for a, b in zip(new, old):
        assert torch.equal(a, b)
    assert not torch.equal(new[0].cpu(), p0)


def test_optim_step_argument_errors():
    L = _L()
    lib = L.load()
    x = torch.zeros(64, device="cuda")
    bad = L.OptimConfig(17, LR, ALPHA, BETA, EPS, 0.0, 1, 1.0, 0.0, None, None)
    assert lib.uic_optim_step(C.byref(bad), x.data_ptr(), x.data_ptr(), None, None, 64, L.stream()) < 0
    assert b"unknown method 17" in lib.uic_last_error_string() and lib.uic_optim_states(17) == -1
    assert lib.uic_optim_step(C.byref(_cfg("sgdm", 0.0, 1)), x.data_ptr(), x.data_ptr(), None, None, 64, L.stream()) < 0     # momentum_buffer missing
    assert lib.uic_optim_step(C.byref(_cfg("sgd", 0.0, 0)), x.data_ptr(), x.data_ptr(), None, None, 64, L.stream()) < 0      # step is 1-based
    assert lib.uic_optim_step(C.byref(_cfg("sgd", -1e-2, 1)), x.data_ptr(), x.data_ptr(), None, None, 64, L.stream()) < 0
    assert lib.uic_optim_step(C.byref(_cfg("sgd", 0.0, 1, max_norm=1.0)), x.data_ptr(), x.data_ptr(), None, None, 64, L.stream()) < 0
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0


@pytest.mark.parametrize("n", [1, 63, 2049, 100003, 512 * 2048 + 4099])
def test_grad_sqnorm_f64_is_the_float64_sum_as_a_float_pair(n):
    """uic_grad_sqnorm_f64 (the norm of a clipped step with weight decay): sum g^2 accumulated in double, left as out[0] + out[1]
    -- out[0] within one float rounding (2^-24 relative) of the float64 sum, the pair within 2^-44; uic_grad_sqnorm's own error is
    printed beside it.  The last
    size is past the 512 partials the scratch holds (a second pass of each workgroup); nothing is written past 1024 floats of
    scratch, and the gradient on a base pointer one float past a 16-byte boundary gives the same value."""
    L = _L()
    lib = L.load()
    gen = torch.Generator().manual_seed(n)
    g = torch.randn(n + 1, generator=gen) * torch.logspace(-3, 1, n + 1)
    gd = g.cuda()
    ref = float(g[1:].double().pow(2).sum())
    scratch = torch.full((1024 + 64,), 7.25, device="cuda")
    out = torch.full((4,), 7.25, device="cuda")
    L.check(lib.uic_grad_sqnorm_f64(gd[1:].data_ptr(), n, scratch.data_ptr(), out.data_ptr(), L.stream()), "grad_sqnorm_f64")
    old = torch.zeros(1, device="cuda")
    L.check(lib.uic_grad_sqnorm(gd[1:].data_ptr(), n, torch.zeros(1024, device="cuda").data_ptr(), old.data_ptr(), L.stream()), "grad_sqnorm")
    torch.cuda.synchronize()
    got = float(out[0])
    print("n %d: f64-accumulated relative error %.3e, float sum's %.3e" % (n, abs(got - ref) / ref, abs(float(old[0]) - ref) / ref))
    pair = float(out[0].double() + out[1].double())
    assert abs(got - ref) <= 2.0 ** -24 * ref and abs(pair - ref) <= 2.0 ** -44 * ref, (got, pair, ref)
    assert bool((out[2:] == 7.25).all()) and bool((scratch[1024:] == 7.25).all())
    assert lib.uic_grad_sqnorm_f64(gd[1:].data_ptr(), n, scratch[1:].data_ptr(), out.data_ptr(), L.stream()) < 0      # scratch not 8-byte aligned
