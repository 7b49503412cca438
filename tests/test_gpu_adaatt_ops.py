"""uic_adaatt_cell_fwd and uic_adaatt_attention_fwd (csrc/adaatt.hip) against float64, element by element, f32 and bf16.

The cases and the bounds are those of tests/adaatt_cases.py (counted roundings; tests/test_adaatt_host.py shows that a float32
evaluation stays inside them and that each deliberate error lands outside).  Inputs are exactly representable in the dtype they
have on the device, so the bounds cover the operators' own arithmetic and the rounding of their outputs, nothing else.  Every
output buffer is filled with 0xFF bytes first; the padding behind a leading dimension and every refused call must leave them."""
import pytest
import torch

import adaatt_cases as AC

pytestmark = pytest.mark.gpu

DEV = "cuda"
TD = {"f32": torch.float32, "bf16": torch.bfloat16}
ID = {"f32": 0, "bf16": 1}


def _lib():
    from unpaired_image_captioning_amd import _lib as L
    return L, L.load()


def _poisoned(rows, ld, dtype):
    t = torch.empty(rows, ld, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(255)
    return t


def _untouched(t):
    return bool((t.view(torch.uint8) == 255).all())


def _run_cell(inp, dtype):
    L, lib = _lib()
    N, H, G = inp["N"], inp["H"], 4 + inp["maxout"]
    inside = inp["n5_mode"] == "inside"
    ld = G * H + (H if inside else 0) + inp["ld_extra"]
    buf = torch.zeros(N, ld, dtype=torch.float32, device=DEV)
    buf[:, :G * H] = inp["sums"].float().to(DEV)
    n5, ld_n5 = None, 0
    if inside:
        buf[:, G * H:(G + 1) * H] = inp["n5"].float().to(DEV)
        n5, ld_n5 = buf[:, G * H:], ld
    elif inp["n5_mode"] == "apart":
        n5t = torch.zeros(N, H + 4, dtype=torch.float32, device=DEV)
        n5t[:, :H] = inp["n5"].float().to(DEV)
        n5, ld_n5 = n5t, H + 4
    c_prev = inp["c_prev"].float().to(DEV).contiguous() if inp["c_prev"] is not None else None
    c_out = _poisoned(N, H, torch.float32)
    h_out = _poisoned(N, H + 8, TD[dtype])
    fake = _poisoned(N, H + 16, TD[dtype]) if n5 is not None else None
    rc = lib.uic_adaatt_cell_fwd(ID[dtype], N, H, inp["maxout"], buf.data_ptr(), ld, n5.data_ptr() if n5 is not None else None, ld_n5,
                                 L.ptr(c_prev), c_out.data_ptr(), h_out.data_ptr(), H + 8, fake.data_ptr() if fake is not None else None, H + 16,
                                 L.stream())
    L.check(rc, "adaatt_cell_fwd")
    torch.cuda.synchronize()
    assert _untouched(h_out[:, H:]) and (fake is None or _untouched(fake[:, H:]))        # nothing behind the widths
    return c_out.cpu().double(), h_out[:, :H].float().cpu().double(), fake[:, :H].float().cpu().double() if fake is not None else None


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_cell_against_float64(dtype):
    for case in AC.CELL_CASES:
        inp = AC.cell_inputs(case, dtype)
        ref = AC.cell(inp["sums"], inp["n5"], inp["c_prev"], inp["H"], inp["maxout"])
        got = _run_cell(inp, dtype)
        for name, r, g, b in zip(("c", "h", "fake"), ref, got, AC.cell_bounds(inp, ref, dtype)):
            if r is None:
                assert g is None
                continue
            err = (g - r).abs()
            print("cell %s %s %s: max err %.3g (bound up to %.3g)" % (case, dtype, name, err.max().item(), float(torch.as_tensor(b).max())))
            assert bool((err <= b).all()), (case, name)


def _run_att(inp, dtype, call=None):
    L, lib = _lib()
    N, R, A, H, div = inp["N"], inp["R"], inp["A"], inp["H"], inp["row_div"]
    t = TD[dtype]
    dev = lambda x, d=torch.float32: x.to(d).to(DEV).contiguous()          # noqa: E731
    fr_e, hl_e = dev(inp["fr_e"]), dev(inp["hl_e"])
    fr, hl, p_att, att = dev(inp["fr"], t), dev(inp["hl"], t), dev(inp["p_att"], t), dev(inp["att"], t)
    w, b = dev(inp["w"]), dev(inp["b"].reshape(1))
    mask, ld_mask = None, 0
    if inp["mask"] is not None:
        ld_mask = R + 3
        mask = torch.full((N // div, ld_mask), 7.0, dtype=torch.float32, device=DEV)
        mask[:, :R] = inp["mask"].float().to(DEV)
    PI = _poisoned(N, R + 1, torch.float32)
    out = _poisoned(N, H + 8, t)
    args = [ID[dtype], N, R, A, H, div, fr_e.data_ptr(), hl_e.data_ptr(), A, fr.data_ptr(), hl.data_ptr(), H, p_att.data_ptr(), att.data_ptr(),
            w.data_ptr(), b.data_ptr(), L.ptr(mask), ld_mask, PI.data_ptr(), out.data_ptr(), H + 8, L.stream()]
    if call is not None:
        call(args)
    rc = lib.uic_adaatt_attention_fwd(*args)
    torch.cuda.synchronize()
    return rc, PI, out


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_attention_against_float64(dtype):
    L, lib = _lib()
    for case in AC.ATT_CASES:
        inp = AC.att_inputs(case, dtype)
        ref_out, ref_PI = AC.attention(inp["fr_e"], inp["hl_e"], inp["fr"], inp["hl"], inp["p_att"], inp["att"], inp["w"], inp["b"], inp["mask"],
                                       inp["row_div"])
        rc, PI, out = _run_att(inp, dtype)
        L.check(rc, "adaatt_attention_fwd")
        H = inp["H"]
        assert _untouched(out[:, H:])
        bo, bp = AC.att_bounds(inp, (ref_out, ref_PI), dtype)
        e_out = (out[:, :H].float().cpu().double() - ref_out).abs()
        e_pi = (PI.cpu().double() - ref_PI).abs()
        print("attention %s %s: out err %.3g (bound up to %.3g), PI err %.3g (bound %.3g)" % (case, dtype, e_out.max().item(), float(bo.max()),
                                                                                            e_pi.max().item(), float(bp.max())))
        assert bool((e_out <= bo).all()) and bool((e_pi <= bp).all()), case
        # a second run gives the same bits (one workgroup owns a row, one order of operations)
        rc2, PI2, out2 = _run_att(inp, dtype)
        assert rc2 == 0 and torch.equal(PI2, PI) and torch.equal(out2[:, :H], out[:, :H])


def test_refused_calls_leave_their_outputs_untouched():
    L, lib = _lib()
    inp = AC.att_inputs(AC.ATT_CASES[1], "f32")

    for pos, val in ((0, 4), (2, 0), (3, 18), (4, 6), (5, 2), (6, None), (8, 8), (11, 4), (17, 1), (20, 4), (12, "off")):
        def change(args, pos=pos, val=val):
            args[pos] = args[pos] + 4 if val == "off" else val
        rc, PI, out = _run_att(inp, "f32", change)
        assert rc == -1 and lib.uic_last_error_string(), pos
        assert _untouched(PI) and _untouched(out), pos
    # the cell
    ci = AC.cell_inputs(AC.CELL_CASES[1], "f32")
    N, H = ci["N"], ci["H"]
    sums = ci["sums"].float().to(DEV).contiguous()
    n5 = ci["n5"].float().to(DEV).contiguous()
    for bad in (dict(dtype=3), dict(H=H + 2), dict(maxout=2), dict(ld=4 * H), dict(n5=None), dict(ld_h=H - 4)):
        c_out, h_out, fake = _poisoned(N, H, torch.float32), _poisoned(N, H, torch.float32), _poisoned(N, H, torch.float32)
        rc = lib.uic_adaatt_cell_fwd(bad.get("dtype", 0), N, bad.get("H", H), bad.get("maxout", 1), sums.data_ptr(), bad.get("ld", 5 * H),
                                     None if "n5" in bad else n5.data_ptr(), H, None, c_out.data_ptr(), h_out.data_ptr(), bad.get("ld_h", H),
                                     fake.data_ptr(), H, L.stream())
        torch.cuda.synchronize()
        assert rc == -1 and _untouched(c_out) and _untouched(h_out) and _untouched(fake), bad
    # N == 0 is a successful no-op
    assert lib.uic_adaatt_cell_fwd(0, 0, H, 1, sums.data_ptr(), 5 * H, None, 0, None, c_out.data_ptr(), h_out.data_ptr(), H, None, 0, L.stream()) == 0
    torch.cuda.synchronize()
    assert _untouched(c_out)
