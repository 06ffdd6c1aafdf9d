"""The fp8 BACKWARD recipe of the Swin linears (swinvox_amd/csrc/linear_fp8.hip, header comment) as a torch emulation on the helpers of
test_cpu_linear_fp8_recipe.py, and the checks that pin it.

The emulation is the yardstick tests/test_gpu_linear_fp8_bwd.py measures the kernels with, so it is tested here on its own, on the CPU:
integer data give the exact fp32 product, an all-zero column takes scale 1, the padding along either contraction changes nothing, and on
N(0, 1) data both gradients sit in the measured band around 3.6e-2 (L1-relative) from the exact product."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_linear_fp8_recipe import ROW_TARGET, gauss_case, l1_rel, quantize_rows, row_scales  # noqa: E402

BWD_SHAPES = [(49, 96, 288), (98, 192, 192), (196, 384, 1536), (130, 1536, 384), (392, 768, 96), (1000, 128, 128)]      # (M, K, N)
# measured on these shapes with gauss_bwd_case (seed 0): dgrad 3.585e-2 ... 3.725e-2, wgrad 3.510e-2 ... 3.734e-2; the band leaves ~3 % either side
DGRAD_BAND = (3.45e-2, 3.85e-2)
WGRAD_BAND = (3.40e-2, 3.85e-2)


def gelu_grad(h):
    """d/dh of the erf GELU, in the dtype of h"""
    return 0.5 * (1.0 + torch.erf(h / math.sqrt(2.0))) + h * torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)


def emulate_dgrad(dy, W, hpre=None, acc_dtype=torch.float64, pad=True):
    """dx [M, K] = dy [M, N] W [N, K]: dy quantised per row (scale over N), W^T per row = per column k of W (scale over N); contraction and
    epilogue in acc_dtype, the scale product in fp32; optional val *= gelu'(hpre).  Before the store rounding."""
    dq, sd = quantize_rows(dy, pad)
    wtq, swt = quantize_rows(W.float().T.contiguous(), pad)
    acc = dq.to(acc_dtype) @ wtq.to(acc_dtype).T
    val = acc / (sd[:, None] * swt[None, :]).to(acc_dtype)
    if hpre is not None:
        val = val * gelu_grad(hpre.to(acc_dtype))
    return val


def emulate_wgrad(dy, x, acc_dtype=torch.float64, pad=True):
    """dw [N, K] = dy^T [N, M] x [M, K]: dy and x quantised per column (one scale per column over all M rows), written transposed with zero
    padding to a multiple of 128 along M; contraction in acc_dtype, the scale product in fp32."""
    dyt, sdc = quantize_rows(dy.float().T.contiguous(), pad)
    xt, sxc = quantize_rows(x.float().T.contiguous(), pad)
    acc = dyt.to(acc_dtype) @ xt.to(acc_dtype).T
    return acc / (sdc[:, None] * sxc[None, :]).to(acc_dtype)


def integer_bwd_case(M, K, N, seed=0):
    """dy [M, N], x [M, K], W [N, K]: integers in [-7, 7] times a power-of-two ROW factor and a power-of-two COLUMN factor (each set spans a
    factor 4), with a |7| in every row at a column of the largest column factor and in every column at a row of the largest row factor.
    Every row maximum and every column maximum is then 7 * a power of two: every scale is a power of two, every scaled value is an integer
    <= 7 times a power of two between 8 and 32 (exact in e4m3), every product a multiple of 64 not above 49 * 1024, and a sum of at most
    1536 of them stays below 2^24 * 64: every partial sum is exact in fp32 in any order."""
    assert M <= 1000 and max(K, N) <= 1536
    g = torch.Generator().manual_seed(3000 + seed)

    def make(R, Cc, rf, cf):
        t = torch.randint(-7, 8, (R, Cc), generator=g).float()
        top_c = [c for c in range(Cc) if cf[c % len(cf)] == max(cf)]
        top_r = [r for r in range(R) if rf[r % len(rf)] == max(rf)]
        for r in range(R):
            t[r, top_c[r % len(top_c)]] = 7.0 if r % 2 else -7.0
        for c in range(Cc):
            t[top_r[c % len(top_r)], c] = -7.0 if c % 2 else 7.0
        rft, cft = torch.tensor(rf), torch.tensor(cf)
        return t * rft[torch.arange(R) % len(rf)][:, None] * cft[torch.arange(Cc) % len(cf)][None, :]

    dy = make(M, N, [0.5, 1.0, 2.0, 1.0], [1.0, 0.5, 2.0])
    x = make(M, K, [1.0, 2.0, 0.5], [2.0, 1.0, 0.5, 1.0])
    W = make(N, K, [1.0, 0.5, 2.0, 2.0], [0.5, 2.0, 1.0])
    return dy, x, W


@pytest.mark.parametrize("shape", BWD_SHAPES + [(37, 99, 30)])
def test_integer_data_are_exact(shape):
    M, K, N = shape
    dy, x, W = integer_bwd_case(M, K, N)
    for t in (dy, x, W):
        for s in (row_scales(t), row_scales(t.T.contiguous())):
            assert torch.equal(torch.exp2(torch.log2(s).round()), s)          # powers of two, per row and per column
        for u in (t, t.T.contiguous()):
            q, sc = quantize_rows(u, pad=False)
            assert torch.equal(q, u * sc[:, None]) and torch.equal(q.abs().amax(dim=1), torch.full((u.shape[0],), ROW_TARGET))
    ref_dx = dy.double() @ W.double()
    ref_dw = dy.double().T @ x.double()
    assert torch.equal(ref_dx.float().double(), ref_dx) and torch.equal(ref_dw.float().double(), ref_dw)
    assert torch.equal(emulate_dgrad(dy, W, acc_dtype=torch.float32), ref_dx.float())
    assert torch.equal(emulate_wgrad(dy, x, acc_dtype=torch.float32), ref_dw.float())


def test_zero_column_takes_scale_one():
    M, K, N = 40, 96, 24
    g = torch.Generator().manual_seed(5)
    dy, x, W = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    dy[:, 3] = 0.0
    x[:, 7] = 0.0
    W[:, 11] = 0.0
    assert float(row_scales(dy.T.contiguous())[3]) == 1.0 and float(row_scales(x.T.contiguous())[7]) == 1.0
    assert float(row_scales(W.T.contiguous())[11]) == 1.0
    dw, dx = emulate_wgrad(dy, x), emulate_dgrad(dy, W)
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(dx).all())
    assert float(dw[3].abs().max()) == 0.0 and float(dw[:, 7].abs().max()) == 0.0 and float(dx[:, 11].abs().max()) == 0.0


@pytest.mark.parametrize("shape", [(37, 99, 30), (130, 96, 200), (128, 128, 128)])
def test_m_and_n_padding_change_nothing(shape):
    M, K, N = shape
    g = torch.Generator().manual_seed(M)
    dy, x, W = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    assert torch.equal(emulate_wgrad(dy, x, pad=True), emulate_wgrad(dy, x, pad=False))          # M padding
    assert torch.equal(emulate_dgrad(dy, W, pad=True), emulate_dgrad(dy, W, pad=False))          # N padding
    q, _ = quantize_rows(dy.T.contiguous())
    assert q.shape == (N, (M + 127) // 128 * 128) and (q.shape[1] == M or float(q[:, M:].abs().max()) == 0.0)


def gauss_bwd_case(M, K, N, seed=0):
    """x, W of the forward's gauss_case; dy ~ N(0, 1)"""
    x, W = gauss_case(M, K, N, seed)
    dy = torch.randn(M, N, generator=torch.Generator().manual_seed(4000 + seed))
    return dy, x, W


@pytest.mark.parametrize("shape", BWD_SHAPES)
def test_distance_from_the_exact_products(shape):
    """e4m3 carries 3 mantissa bits: both gradients are ~3.6e-2 (L1-relative) away from the exact product at every shape, whichever way the
    scales run; fp32 accumulation of the same operands is < 1e-6 away from fp64 accumulation."""
    M, K, N = shape
    dy, x, W = gauss_bwd_case(M, K, N)
    dx, dw = emulate_dgrad(dy, W), emulate_wgrad(dy, x)
    d_dx, d_dw = l1_rel(dx, dy.double() @ W.double()), l1_rel(dw, dy.double().T @ x.double())
    print(f"{shape}: dgrad vs exact {d_dx:.3e}, wgrad vs exact {d_dw:.3e}")
    assert DGRAD_BAND[0] <= d_dx <= DGRAD_BAND[1], d_dx
    assert WGRAD_BAND[0] <= d_dw <= WGRAD_BAND[1], d_dw
    assert l1_rel(emulate_dgrad(dy, W, acc_dtype=torch.float32), dx) < 1e-6
    assert l1_rel(emulate_wgrad(dy, x, acc_dtype=torch.float32), dw) < 1e-6
