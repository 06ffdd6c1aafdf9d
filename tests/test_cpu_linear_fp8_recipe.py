"""The fp8 linear recipe (swinvox_amd/csrc/linear_fp8.hip) as a torch emulation, and the checks that pin it.

The emulation is the yardstick tests/test_gpu_linear_fp8.py measures the kernels with, so it is tested here on its own, on the CPU:
integer data come out exact, an all-zero row takes scale 1, the K padding changes nothing, and on N(0, 1) data the recipe sits at the known
3.5e-2 ... 3.8e-2 L1-relative distance from an exact linear (what separates it from a bf16-operand linear, which is ~1e-3 away)."""
import math

import pytest
import torch

ROW_TARGET = 224.0          # half of e4m3's 448: the constant of the fp8 window attention
SCALE_MAX = 2.0 ** 60       # clamp of a row scale: the epilogue's product sx * sw stays finite in fp32

INT_SHAPES = [(49, 96, 288), (98, 192, 192), (196, 384, 1536), (130, 1536, 384)]      # (M, K, N)
RECIPE_SHAPES = INT_SHAPES + [(64, 3072, 768)]


def row_scales(t32):
    """fp32 [R, K] -> fp32 [R]: 224 / max|row| formed in fp32, 1 for an all-zero row, at most 2^60"""
    assert t32.dtype == torch.float32
    amax = t32.abs().amax(dim=1)
    s = torch.full_like(amax, ROW_TARGET) / torch.where(amax > 0, amax, torch.full_like(amax, ROW_TARGET))
    return torch.clamp(s, max=SCALE_MAX)


def quantize_rows(t, pad=True):
    """stored tensor [R, K] (fp32 or bf16) -> (e4m3 values as fp32 [R, Kp], scales [R]); Kp = roundup(K, 128) with zero padding"""
    t32 = t.float()
    s = row_scales(t32)
    q = (t32 * s[:, None]).to(torch.float8_e4m3fn).float()      # product in fp32, round to nearest even
    if pad:
        Kp = (t.shape[1] + 127) // 128 * 128
        q = torch.nn.functional.pad(q, (0, Kp - t.shape[1]))
    return q, s


def emulate_linear(x, W, bias=None, gelu=False, residual=None, row_scale=None, rows_per_scale=1, acc_dtype=torch.float64, pad=True):
    """The recipe on the stored inputs; contraction and epilogue in acc_dtype.  Returns (out, pre_act) in acc_dtype, before the store rounding."""
    xq, sx = quantize_rows(x, pad)
    wq, sw = quantize_rows(W, pad)
    acc = xq.to(acc_dtype) @ wq.to(acc_dtype).T
    val = acc / (sx[:, None] * sw[None, :]).to(acc_dtype)          # the scale product is formed in fp32
    if bias is not None:
        val = val + bias.to(acc_dtype)
    pre = val
    if gelu:
        val = 0.5 * val * (1.0 + torch.erf(val / math.sqrt(2.0)))
    if residual is not None:
        sc = torch.ones(x.shape[0], dtype=acc_dtype)
        if row_scale is not None:
            sc = row_scale.to(acc_dtype)[torch.arange(x.shape[0]) // rows_per_scale]
        val = residual.to(acc_dtype) + sc[:, None] * val
    return val, pre


def integer_case(M, K, N, seed=0):
    """x: integers in [-7, 7] with one |7| per row, row m times 2^((m mod 4) - 1); W likewise with factors {1, 1/4, 8, 2} and a -7 in every
    row.  Every scale is a power of two, every scaled value a multiple of 32 not above 224 (exact in e4m3), every partial sum exact in fp32."""
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randint(-7, 8, (M, K), generator=g).float()
    W = torch.randint(-7, 8, (N, K), generator=g).float()
    x[torch.arange(M), torch.randint(0, K, (M,), generator=g)] = 7.0 * (1 - 2 * (torch.arange(M) % 2)).float()
    W[torch.arange(N), torch.randint(0, K, (N,), generator=g)] = -7.0
    x *= (2.0 ** ((torch.arange(M) % 4) - 1).float())[:, None]
    W *= torch.tensor([1.0, 0.25, 8.0, 2.0])[torch.arange(N) % 4][:, None]
    return x, W


def l1_rel(a, ref):
    return float((a.double() - ref.double()).abs().sum() / ref.double().abs().sum())


def nan_padded(t, rows, ld, dev):
    """t in the corner of a NaN-filled [rows, ld] buffer of its type on `dev` (the GPU tests' guard regions)"""
    buf = torch.full((rows, ld), float("nan"), dtype=t.dtype, device=dev)
    buf[: t.shape[0], : t.shape[1]] = t.to(dev)
    return buf


def raw_bytes(t):
    """the bytes of a tensor, for bit comparisons across storage types"""
    return t.contiguous().view(torch.uint8).cpu()


def gauss_case(M, K, N, seed=0):
    g = torch.Generator().manual_seed(2000 + seed)
    return torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)


@pytest.mark.parametrize("shape", INT_SHAPES)
def test_integer_data_are_exact(shape):
    x, W = integer_case(*shape)
    ref = x.double() @ W.double().T
    assert torch.equal(ref.float().double(), ref)                 # the fp32 product itself is exact
    sx, sw = row_scales(x), row_scales(W)
    for s in (sx, sw):
        assert torch.equal(torch.exp2(torch.log2(s).round()), s)     # powers of two
    xq, _ = quantize_rows(x)
    assert torch.equal(xq[:, :shape[1]], x * sx[:, None]) and float(xq.abs().max()) == ROW_TARGET and torch.equal(xq % 32, torch.zeros_like(xq))
    out, _ = emulate_linear(x, W, acc_dtype=torch.float32)
    assert torch.equal(out, ref.float())


def test_zero_and_tiny_rows():
    x, W = gauss_case(8, 96, 12)
    x[3] = 0.0
    W[5] = 0.0
    x[6] = 1e-30 * torch.sign(x[6])
    sx, sw = row_scales(x), row_scales(W)
    assert float(sx[3]) == 1.0 and float(sw[5]) == 1.0 and float(sx[6]) == SCALE_MAX
    bias = torch.linspace(-1, 1, 12)
    out, _ = emulate_linear(x, W, bias=bias)
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out[3], bias.double()) and torch.equal(out[:, 5], bias.double()[5].expand(8))
    assert torch.equal(out[6], bias.double())                        # 1e-30 * 2^60 is below e4m3's smallest subnormal: the row quantises to zero
    assert bool(torch.isfinite(torch.full((1,), SCALE_MAX) * torch.full((1,), SCALE_MAX)).all())


@pytest.mark.parametrize("K", [96, 192, 100])
def test_k_padding_changes_nothing(K):
    x, W = gauss_case(20, K, 24, seed=K)
    a, _ = emulate_linear(x, W, pad=True)
    b, _ = emulate_linear(x, W, pad=False)
    assert torch.equal(a, b)
    q, _ = quantize_rows(x)
    assert q.shape[1] == 128 * ((K + 127) // 128) and float(q[:, K:].abs().max()) == 0.0


@pytest.mark.parametrize("shape", RECIPE_SHAPES)
def test_distance_from_an_exact_linear(shape):
    """e4m3 carries 3 mantissa bits: on N(0, 1) activations and N(0, 1/K) weights the recipe is 3.5e-2 ... 3.8e-2 (L1-relative) away from
    the exact product, at every shape; fp32 accumulation of the same operands is ~5e-8 away from fp64 accumulation."""
    x, W = gauss_case(*shape)
    exact = x.double() @ W.double().T
    out, _ = emulate_linear(x, W)
    d = l1_rel(out, exact)
    print(f"{shape}: recipe vs exact {d:.3e}")
    assert 3.5e-2 <= d <= 3.8e-2, d
    out32, _ = emulate_linear(x, W, acc_dtype=torch.float32)
    assert l1_rel(out32, out) < 1e-6
