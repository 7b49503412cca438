"""uic_layernorm_std and uic_mha_fwd (csrc/transformer.hip) against float64, element by element.

Tolerances.  f32: 1e-5 on outputs of O(1).  bf16: the float64 result of the SAME operands after rounding to bf16, plus one bf16
ulp of the output (2^-8 relative: the store rounds to nearest, half an ulp, and the f32 arithmetic in between is far below that)."""
import ctypes as C

import pytest
import torch

import transformer_cases as TC

pytestmark = pytest.mark.gpu

DEV = "cuda"
TD = {0: torch.float32, 1: torch.bfloat16}


def _lib():
    from unpaired_image_captioning_amd import _lib as L
    return L, L.load()


def _ulp_bf16(ref):
    return ref.abs().clamp_min(2.0 ** -126) * 2.0 ** -8


def _layernorm(x, a, b, in_dt=0, out_dt=0, ldx=None, ldy=None):
    L, lib = _lib()
    rows, d = x.shape
    ldx, ldy = ldx or d, ldy or d
    xb = torch.full((rows, ldx), float("nan"), dtype=TD[in_dt], device=DEV)
    xb[:, :d] = x.to(TD[in_dt])
    y = torch.full((rows, ldy), 7.0, dtype=TD[out_dt], device=DEV)
    L.check(lib.uic_layernorm_std(in_dt, out_dt, xb.data_ptr(), ldx, rows, d, a.data_ptr(), b.data_ptr(), 1e-6, y.data_ptr(), ldy, L.stream()),
            "layernorm_std")
    assert (y[:, d:] == 7.0).all()                 # nothing written beyond the row
    return y[:, :d].float().cpu()


@pytest.mark.parametrize("d", [8, 64, 100, 512, 520])
@pytest.mark.parametrize("rows", [1, 3])
def test_layernorm_std_against_float64(d, rows):
    g = torch.Generator().manual_seed(d * 10 + rows)
    x = torch.randn(rows, d, generator=g)
    a, b = 1 + 0.3 * torch.randn(d, generator=g), 0.2 * torch.randn(d, generator=g)
    ref = TC.layer_norm(x.double(), a.double(), b.double())
    got = _layernorm(x.to(DEV), a.to(DEV), b.to(DEV), ldx=d + 3, ldy=d + 5)
    assert (got.double() - ref).abs().max().item() < 1e-5
    # and it is not nn.LayerNorm: the biased variance with eps inside the root differs visibly at small d
    other = torch.nn.functional.layer_norm(x.double(), (d,), a.double(), b.double(), 1e-6)
    assert (ref - other).abs().max().item() > 1e-4


@pytest.mark.parametrize("d", [8, 100, 520])
def test_layernorm_std_constant_rows_give_b2(d):
    g = torch.Generator().manual_seed(d)
    a, b = 1 + 0.3 * torch.randn(d, generator=g), 0.2 * torch.randn(d, generator=g)
    x = torch.tensor([[3.25], [0.0], [-1e4]]).expand(3, d).contiguous()       # std = 0: (x - mean) / (0 + eps) = 0
    got = _layernorm(x.to(DEV), a.to(DEV), b.to(DEV))
    assert torch.equal(got, b.expand(3, d))


@pytest.mark.parametrize("d", [64, 100, 512])
def test_layernorm_std_survives_a_large_offset(d):
    """Rows of 1e4 + O(1): E[x^2] - E[x]^2 in f32 would lose every digit (1e8 against 1).  The reference is float64 on the SAME f32
    inputs.  Bound: the inputs are exact, the centred values are exact differences, so the error is that of a row of O(1) values:
    1e-5, as everywhere."""
    g = torch.Generator().manual_seed(d)
    x = (1e4 + torch.randn(3, d, generator=g)).float()
    a, b = 1 + 0.3 * torch.randn(d, generator=g), 0.2 * torch.randn(d, generator=g)
    ref = TC.layer_norm(x.double(), a.double(), b.double())
    got = _layernorm(x.to(DEV), a.to(DEV), b.to(DEV))
    assert (got.double() - ref).abs().max().item() < 1e-5


@pytest.mark.parametrize("in_dt,out_dt", [(1, 1), (0, 1), (1, 0)])
def test_layernorm_std_bf16(in_dt, out_dt):
    d = 100
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, d, generator=g)
    a, b = 1 + 0.3 * torch.randn(d, generator=g), 0.2 * torch.randn(d, generator=g)
    xr = x.to(TD[in_dt]).double()
    ref = TC.layer_norm(xr, a.double(), b.double())
    got = _layernorm(x.to(DEV), a.to(DEV), b.to(DEV), in_dt, out_dt)
    bound = 1e-5 + (_ulp_bf16(ref) if out_dt else 0)
    assert ((got.double() - ref).abs() <= bound).all()


def _mha(dt, Q, K, V, d_k, mask=None, causal=0, q_off=0, div=1, pad=0):
    """Q [B, Sq, h d_k], K / V [B / div, Sk, h d_k] (f32 host tensors); pad > 0: operands live in wider, strided buffers."""
    L, lib = _lib()
    B, Sq, dm = Q.shape
    Sk = K.shape[1]

    def place(t):
        buf = torch.full((t.shape[0], t.shape[1] + (1 if pad else 0), dm + pad), float("nan"), dtype=TD[dt], device=DEV)
        buf[:, :t.shape[1], :dm] = t.to(TD[dt])
        return buf
    q, k, v = place(Q), place(K), place(V)
    o = torch.full((B, Sq + (1 if pad else 0), dm + pad), 7.0, dtype=TD[dt], device=DEV)
    m = mask.to(torch.uint8).to(DEV).contiguous() if mask is not None else None
    rc = lib.uic_mha_fwd(dt, B, Sq, Sk, d_k, q.data_ptr(), q.stride(1), q.stride(0), k.data_ptr(), k.stride(1), k.stride(0),
                         v.data_ptr(), v.stride(1), v.stride(0), o.data_ptr(), o.stride(1), o.stride(0),
                         m.data_ptr() if m is not None else None, Sk, causal, q_off, div, L.stream())
    if rc:
        return rc
    torch.cuda.synchronize()
    if pad:
        assert (o[:, Sq:] == 7.0).all() and (o[:, :, dm:] == 7.0).all()
    return o[:, :Sq, :dm].float().cpu()


def _check(dt, got, Q, K, V, d_k, **kw):
    r = (lambda t: t.to(TD[dt]).double())
    ref = TC.attention(r(Q), r(K), r(V), d_k, **kw)
    bound = 1e-5 + (_ulp_bf16(ref) if dt else 0)
    err = (got.double() - ref).abs()
    assert (err <= bound).all(), (err.max().item(), ref.abs().max().item())


def _rand(B, S, d_k, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, S, 8 * d_k, generator=g)


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("d_k", [8, 16, 64])
@pytest.mark.parametrize("Sk", [1, 5, 36, 63, 64, 65, 128])
def test_mha_fwd_key_lengths(dt, d_k, Sk):
    B, Sq = 2, 5
    Q, K, V = _rand(B, Sq, d_k, 1), _rand(B, Sk, d_k, 2), _rand(B, Sk, d_k, 3)
    g = torch.Generator().manual_seed(Sk)
    mask = (torch.rand(B, Sk, generator=g) < 0.7).float()
    mask[:, 0] = 1
    _check(dt, _mha(dt, Q, K, V, d_k, mask), Q, K, V, d_k, key_mask=mask)


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("Sq", [1, 17, 36])
def test_mha_fwd_query_lengths_causal_with_offset(dt, Sq):
    d_k, off = 16, 3
    Sk = Sq + off
    Q, K, V = _rand(3, Sq, d_k, 4), _rand(3, Sk, d_k, 5), _rand(3, Sk, d_k, 6)
    got = _mha(dt, Q, K, V, d_k, None, causal=1, q_off=off)
    _check(dt, got, Q, K, V, d_k, causal=True, q_offset=off)
    # query i sees keys 0 .. off + i only: changing a later key changes no earlier row
    K2, V2 = K.clone(), V.clone()
    K2[:, -1], V2[:, -1] = 9.0, -9.0
    got2 = _mha(dt, Q, K2, V2, d_k, None, causal=1, q_off=off)
    assert torch.equal(got[:, :-1], got2[:, :-1])


@pytest.mark.parametrize("dt", [0, 1])
def test_mha_fwd_masks_one_live_key_and_fully_masked_row(dt):
    d_k, Sk = 16, 37
    Q, K, V = _rand(3, 4, d_k, 7), _rand(3, Sk, d_k, 8), _rand(3, Sk, d_k, 9)
    mask = torch.ones(3, Sk)
    mask[0] = 0
    mask[0, 11] = 1                      # one live key: the output is that key's value row
    mask[1] = 0                          # fully masked: the finite -1e9 makes the row uniform over ALL Sk keys, not NaN
    got = _mha(dt, Q, K, V, d_k, mask)
    _check(dt, got, Q, K, V, d_k, key_mask=mask)
    r = (lambda t: t.to(TD[dt]).float())
    assert torch.equal(got[0], r(V)[0, 11].expand(4, -1))
    assert torch.isfinite(got).all()
    assert ((got[1].double() - r(V)[1].double().mean(0)).abs() <= 1e-5 + (_ulp_bf16(r(V)[1].double().mean(0)) if dt else 0)).all()


@pytest.mark.parametrize("dt", [0, 1])
def test_mha_fwd_row_divisor_and_strided_operands(dt):
    d_k, Sk, div = 8, 21, 3
    Q, K, V = _rand(6, 2, d_k, 10), _rand(2, Sk, d_k, 11), _rand(2, Sk, d_k, 12)
    g = torch.Generator().manual_seed(3)
    mask = (torch.rand(6, Sk, generator=g) < 0.6).float()
    mask[:, 2] = 1
    got = _mha(dt, Q, K, V, d_k, mask, div=div, pad=8)
    _check(dt, got, Q, K, V, d_k, key_mask=mask, row_div=div)


def test_mha_fwd_rejects_what_it_does_not_support():
    L, lib = _lib()
    Q = _rand(2, 3, 16, 1)
    for bad in (dict(Sk=129, d_k=16), dict(Sk=8, d_k=12), dict(Sk=8, d_k=136)):
        K = torch.zeros(2, bad["Sk"], 8 * bad["d_k"])
        Qb = torch.zeros(2, 3, 8 * bad["d_k"])
        assert _mha(0, Qb, K, K, bad["d_k"]) == -1, bad
        assert b"mha_fwd" in lib.uic_last_error_string()
    K = _rand(2, 8, 16, 2)
    assert _mha(0, Q, K, K, 16, div=3) == -1          # 3 does not divide B = 2
    assert torch.isfinite(_mha(0, Q, K, K, 16)).all()  # and the library still works afterwards
