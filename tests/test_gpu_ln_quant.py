"""The quantising LayerNorm (csrc/norm.hip ln_fwd_kernel with its quantising outputs, sv_layernorm_quant_fwd) through the C ABI, every
comparison bit for bit: y / mean / rstd against sv_layernorm_fwd on the same input, the e4m3 rows and scales against sv_quant_rows_e4m3
applied to that y.  The second comparison holds if and only if the scale recipe, the rounding of the stored value, the zero padding and the
lane map of the byte stores are all right."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_linear_fp8_recipe import integer_case  # noqa: E402

from swinvox_amd import hip, ops  # noqa: E402
from swinvox_amd.ops import call, ptr  # noqa: E402

GUARD = 3                       # rows past `rows` in every output buffer; they must keep their fill
ROWS = (1, 37, 130)             # one lane group; several waves with an idle tail; more than one workgroup at every LPR (16 rows each at most)
# C: 64 / 96 -> LPR 16 (bf16, VEC 8) or 16 / 32 (VEC 4); 100 -> VEC 4 in both storages; 192, 384 -> LPR 32 / 64; 3072 -> NV = 6 (bf16, VEC 8) and NV = 12,
# the widest VEC 4 kernel (fp32 storage); tests/test_cpu_norm_plan.py pins these through sv_layernorm_plan.  C = 64 in fp32: 16 chunks x 4 = 64 elements in the lane group against Kp = 128 (the padding loop runs past the registers)
CS = (64, 96, 100, 192, 384, 3072)
MERGED = ((2, 4, 4, 24), (1, 6, 6, 96), (3, 2, 2, 384))      # (I, H, W, C0): C = 4 C0 = 96, 384, 1536


def _dt(store):
    return torch.bfloat16 if store == "bf16" else torch.float32


def _code(store):
    return hip.BF16 if store == "bf16" else hip.F32


def _inputs(rows, Cd, store, merge, seed, beta_zero=False, gamma_zero=False, const_row=None):
    """x: N(0, 1) times a per-row factor spanning 1e-3 ... 1e3, random gamma / beta.  merge = (I, H, W, C0): x is the un-merged map."""
    g = torch.Generator().manual_seed(seed)
    n_in, c_in = (merge[0] * merge[1] * merge[2], merge[3]) if merge else (rows, Cd)
    x = torch.randn(n_in, c_in, generator=g) * (10.0 ** (6.0 * torch.rand(n_in, 1, generator=g) - 3.0))
    if const_row is not None:
        # 2.0: the row sum C * 2 and, for every C of this file, mean = fl(C * 2 * fl(1 / C)) = 2 are exact, so x - mean is exactly 0
        x[const_row] = 2.0
    gamma = torch.zeros(Cd) if gamma_zero else 1.0 + 0.5 * torch.randn(Cd, generator=g)
    beta = torch.zeros(Cd) if beta_zero else 0.5 * torch.randn(Cd, generator=g)
    return x.to(_dt(store)), gamma, beta


def _filled(shape, dtype, dev):
    """guard fill: 0xAB bytes for the byte rows, NaN for the float buffers"""
    if dtype == torch.uint8:
        return torch.full(shape, 0xAB, dtype=torch.uint8, device=dev)
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _plain(x, gamma, beta, rows, Cd, store, mhw):
    y = _filled((rows + GUARD, Cd), _dt(store), x.device)
    mean, rstd = _filled((rows + GUARD,), torch.float32, x.device), _filled((rows + GUARD,), torch.float32, x.device)
    call("sv_layernorm_fwd", ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), rows, Cd, 1e-5, mhw[0], mhw[1], act=_code(store))
    return y, mean, rstd


def _two_kernel_rows(y, rows, Cd):
    Kp = (Cd + 127) // 128 * 128
    q = _filled((rows + GUARD, Kp), torch.uint8, y.device)
    s = _filled((rows + GUARD,), torch.float32, y.device)
    call("sv_quant_rows_e4m3", ptr(y), hip.BF16 if y.dtype == torch.bfloat16 else hip.F32, rows, Cd, Cd, ptr(q), Kp, ptr(s))
    return q, s


def _fused(x, gamma, beta, rows, Cd, store, mhw, stored=True):
    dev = x.device
    Kp = (Cd + 127) // 128 * 128
    y = mean = rstd = None
    if stored:
        y = _filled((rows + GUARD, Cd), _dt(store), dev)
        mean, rstd = _filled((rows + GUARD,), torch.float32, dev), _filled((rows + GUARD,), torch.float32, dev)
    q, s = _filled((rows + GUARD, Kp), torch.uint8, dev), _filled((rows + GUARD,), torch.float32, dev)
    n0 = ops.layernorm_quant_launches()
    call("sv_layernorm_quant_fwd", ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), ptr(q), Kp, ptr(s), rows, Cd, 1e-5, mhw[0], mhw[1],
         act=_code(store))               # a non-zero return raises: "the launch returns 0"
    assert ops.layernorm_quant_launches() == n0 + 1
    return y, mean, rstd, q, s


def _check_case(dev, rows, Cd, store, merge=None, **inp):
    mhw = (merge[1], merge[2]) if merge else (0, 0)
    x, gamma, beta = (t.to(dev) for t in _inputs(rows, Cd, store, merge, seed=rows * 7919 + Cd, **inp))
    y0, m0, r0 = _plain(x, gamma, beta, rows, Cd, store, mhw)
    q0, s0 = _two_kernel_rows(y0, rows, Cd)
    y1, m1, r1, q1, s1 = _fused(x, gamma, beta, rows, Cd, store, mhw)
    _, _, _, q2, s2 = _fused(x, gamma, beta, rows, Cd, store, mhw, stored=False)          # y = mean = rstd = NULL
    torch.cuda.synchronize()
    # bytes: compare storage bit patterns, so that NaN guard rows compare equal to themselves
    bits = lambda t: t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)     # noqa: E731
    assert bool(torch.isfinite(y0[:rows].float()).all())
    assert torch.equal(bits(y1[:rows]), bits(y0[:rows])), "y"
    assert torch.equal(bits(m1[:rows]), bits(m0[:rows])) and torch.equal(bits(r1[:rows]), bits(r0[:rows])), "mean / rstd"
    assert torch.equal(q1[:rows], q0[:rows]), f"q differs in {int((q1[:rows] != q0[:rows]).sum())} bytes"
    assert torch.equal(bits(s1[:rows]), bits(s0[:rows])), "scales"
    assert torch.equal(q2, q1) and torch.equal(bits(s2), bits(s1)), "the non-storing call writes other rows"
    # bounds: guard rows untouched, padding bytes of every real row zero
    assert bool((q1[rows:] == 0xAB).all()) and bool(torch.isnan(s1[rows:]).all())
    assert bool(torch.isnan(y1[rows:].float()).all()) and bool(torch.isnan(m1[rows:]).all()) and bool(torch.isnan(r1[rows:]).all())
    assert q1.shape[1] == Cd or int(q1[:rows, Cd:].max()) == 0
    return y1, q1, s1


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["bf16", "f32"])
@pytest.mark.parametrize("Cd", CS)
@pytest.mark.parametrize("rows", ROWS)
def test_rows_and_scales_equal_the_two_kernel_operand(dev, rows, Cd, store):
    _check_case(dev, rows, Cd, store)


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["bf16", "f32"])
@pytest.mark.parametrize("merge", MERGED)
def test_merged_form(dev, merge, store):
    """PatchMerging gather in front of the LayerNorm: the quantised row is the row of y (4 C0 wide), not a row of the source map."""
    I, H, W, C0 = merge
    _check_case(dev, I * (H // 2) * (W // 2), 4 * C0, store, merge=merge)


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["bf16", "f32"])
@pytest.mark.parametrize("which", ["constant row", "gamma zero"])
@pytest.mark.parametrize("Cd", CS)
def test_zero_rule(dev, Cd, which, store):
    """beta = 0 and a constant row of x (or gamma = 0 everywhere): the row of y is all zeros, its scale is exactly 1.0 and all its Kp bytes
    are zero - next to rows that quantise normally."""
    rows, r = 37, 5
    kw = dict(beta_zero=True, const_row=r) if which == "constant row" else dict(beta_zero=True, gamma_zero=True)
    y, q, s = _check_case(dev, rows, Cd, store, **kw)
    zero_rows = [r] if which == "constant row" else list(range(rows))
    for i in zero_rows:
        assert float(y[i].float().abs().max()) == 0.0, i
        assert float(s[i]) == 1.0 and int(q[i].max()) == 0, i
    if which == "constant row":
        assert float(y[r + 1].float().abs().max()) > 0.0 and float(s[r + 1]) != 1.0 and int(q[r + 1].max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["bf16", "f32"])
def test_zero_rule_merged(dev, store):
    """the same on the merged form: image 0 of the source map is constant, so every merged row of it is"""
    I, H, W, C0 = 2, 4, 4, 24
    rows, Cd = I * (H // 2) * (W // 2), 4 * C0
    y, q, s = _check_case(dev, rows, Cd, store, merge=(I, H, W, C0), beta_zero=True, const_row=slice(0, H * W))
    per = rows // I
    assert float(y[:per].float().abs().max()) == 0.0 and bool((s[:per] == 1.0).all()) and int(q[:per].max()) == 0
    assert float(y[per:rows].float().abs().max()) > 0.0 and bool((s[per:rows] != 1.0).all())


@pytest.mark.gpu
def test_refused_call_does_not_count(dev):
    rows, Cd = 8, 96
    x, gamma, beta = (t.to(dev) for t in _inputs(rows, Cd, "bf16", None, seed=1))
    q = torch.zeros(rows, 256, dtype=torch.uint8, device=dev)
    s = torch.zeros(rows, dtype=torch.float32, device=dev)
    mean = torch.zeros(rows, dtype=torch.float32, device=dev)
    n0 = ops.layernorm_quant_launches()
    for args in ((ptr(q), 256, ptr(s), None, None),        # Kp != roundup(C, 128)
                 (None, 128, ptr(s), None, None),          # q null
                 (ptr(q), 128, ptr(s), ptr(mean), None)):  # mean without rstd
        qp, Kp, sp, mp, rp = args
        with pytest.raises(RuntimeError, match="sv_layernorm_quant_fwd"):
            call("sv_layernorm_quant_fwd", ptr(x), ptr(gamma), ptr(beta), None, mp, rp, qp, Kp, sp, rows, Cd, 1e-5, 0, 0, act=hip.BF16)
    assert ops.layernorm_quant_launches() == n0
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["bf16", "f32"])
@pytest.mark.parametrize("shape", [(49, 96, 288), (98, 192, 192)])
def test_end_to_end_into_the_fp8_linear(dev, shape, store):
    """sv_linear_fp8 on the fused kernel's rows and scales and the quantised weight (the integer weights of the exact-integer test: every
    weight scale a power of two) gives, bit for bit, the output it gives on the two-kernel operand."""
    M, K, N = shape
    xi, W = integer_case(M, K, N)
    g = torch.Generator().manual_seed(9)
    gamma, beta = (1.0 + 0.5 * torch.randn(K, generator=g)).to(dev), (0.5 * torch.randn(K, generator=g)).to(dev)
    x = xi.to(_dt(store)).to(dev)
    W = W.to(dev)
    y0, _, _ = _plain(x, gamma, beta, M, K, store, (0, 0))
    q0, s0 = _two_kernel_rows(y0, M, K)
    _, _, _, q1, s1 = _fused(x, gamma, beta, M, K, store, (0, 0), stored=False)
    wq, sw = ops.quantize_rows_fp8(W, N, K)
    outs = []
    for q, s in ((q0, s0), (q1, s1)):
        out = torch.full((M, N), float("nan"), dtype=_dt(store), device=dev)
        e = ops._epilogue(N)
        call("sv_linear_fp8", ptr(q), ptr(s), ptr(wq), ptr(sw), ptr(out), M, K, N, C.byref(e), act=_code(store))
        outs.append(out)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0].float()).all()) and float(outs[0].float().abs().max()) > 0.0
    assert torch.equal(outs[0], outs[1])
