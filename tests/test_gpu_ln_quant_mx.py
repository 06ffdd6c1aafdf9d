"""The MX quantising LayerNorm (csrc/norm.hip ln_fwd_kernel with its LnQuantMxOut outputs, sv_layernorm_quant_mx_fwd) through the C ABI, every
comparison bit for bit: y / mean / rstd against sv_layernorm_fwd on the same input; the e4m3 rows and E8M0 block scales against
sv_quant_rows_mx_e4m3 applied to that y, and against the CPU emulation mx_quant_rows of tests/test_cpu_linear_mxfp8_recipe.py applied to the
downloaded y (exact arithmetic, independent of the GPU quantiser).  The inputs make the blocks of one row differ by powers of two (LayerNorm
normalises a per-row factor away, so the spread sits in the affine): a per-row scale written into every block does not pass."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_linear_mxfp8_recipe import mx_integer_case, mx_quant_rows  # noqa: E402

from swinvox_amd import hip, ops  # noqa: E402
from swinvox_amd.ops import call, ptr  # noqa: E402

GUARD = 3                       # rows past `rows` in every output buffer; they must keep their fill
ROWS = (1, 37, 130)             # one lane group; several waves with an idle tail; more than one workgroup at every LPR (16 rows each at most)
# C: 64 / 96 -> LPR 16 (bf16, VEC 8) or 16 / 32 (VEC 4); 100 -> VEC 4 in both storages and a block with 4 valid columns (one lane of eight);
# 192, 384 -> LPR 32 / 64; 3072 -> NV = 12 (VEC 4) and NV = 6 (VEC 8).  64, 96, 192: Kp > C with 2, 1, 2 blocks wholly in the padding
CS = (64, 96, 100, 192, 384, 3072)
MERGED = ((2, 4, 4, 24), (1, 6, 6, 96), (3, 2, 2, 384))      # (I, H, W, C0): C = 4 C0 = 96, 384, 1536


def _dt(store):
    return torch.bfloat16 if store == "bf16" else torch.float32


def _code(store):
    return hip.BF16 if store == "bf16" else hip.F32


def _block_factors(Cd, wide=False):
    """2^(3 ((k // 32) mod 5) - 6) per column; wide: block exponents spread evenly over -40 ... 40"""
    blk = torch.arange(Cd) // 32
    if wide:
        nb = int(blk.max()) + 1
        e = torch.round(-40.0 + 80.0 * blk.float() / max(nb - 1, 1))
    else:
        e = 3.0 * (blk % 5).float() - 6.0
    return torch.exp2(e)


def _inputs(rows, Cd, store, merge, seed, beta_zero=False, gamma_zero=False, const_row=None, wide=False):
    """x: N(0, 1) times a per-row factor spanning 1e-3 ... 1e3; gamma = (1 + 0.5 randn) * block factor, beta = 0.5 randn * block factor.
    merge = (I, H, W, C0): x is the un-merged map."""
    g = torch.Generator().manual_seed(seed)
    n_in, c_in = (merge[0] * merge[1] * merge[2], merge[3]) if merge else (rows, Cd)
    x = torch.randn(n_in, c_in, generator=g) * (10.0 ** (6.0 * torch.rand(n_in, 1, generator=g) - 3.0))
    if const_row is not None:
        # 2.0: the row sum C * 2 and, for every C of this file, mean = fl(C * 2 * fl(1 / C)) = 2 are exact, so x - mean is exactly 0
        x[const_row] = 2.0
    f = _block_factors(Cd, wide)
    gamma = torch.zeros(Cd) if gamma_zero else (1.0 + 0.5 * torch.randn(Cd, generator=g)) * f
    beta = torch.zeros(Cd) if beta_zero else 0.5 * torch.randn(Cd, generator=g) * f
    return x.to(_dt(store)), gamma, beta


def _filled(shape, dtype, dev):
    """guard fill: 0xAB bytes for the byte buffers, NaN for the float buffers"""
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
    s = _filled((rows + GUARD, Kp // 32), torch.uint8, y.device)
    call("sv_quant_rows_mx_e4m3", ptr(y), hip.BF16 if y.dtype == torch.bfloat16 else hip.F32, rows, Cd, Cd, ptr(q), Kp, ptr(s))
    return q, s


def _counters():
    lib = hip.load()
    return (ops.layernorm_quant_mx_launches(), ops.layernorm_quant_launches(), int(lib.sv_quant_rows_mx_launches()), ops.mx_act_quant_launches())


def _fused(x, gamma, beta, rows, Cd, store, mhw, stored=True):
    dev = x.device
    Kp = (Cd + 127) // 128 * 128
    y = mean = rstd = None
    if stored:
        y = _filled((rows + GUARD, Cd), _dt(store), dev)
        mean, rstd = _filled((rows + GUARD,), torch.float32, dev), _filled((rows + GUARD,), torch.float32, dev)
    q, s = _filled((rows + GUARD, Kp), torch.uint8, dev), _filled((rows + GUARD, Kp // 32), torch.uint8, dev)
    n0 = _counters()
    call("sv_layernorm_quant_mx_fwd", ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), ptr(q), Kp, ptr(s), rows, Cd, 1e-5, mhw[0], mhw[1],
         act=_code(store))               # a non-zero return raises: "the launch returns 0"
    n1 = _counters()
    assert n1[0] == n0[0] + 1 and n1[1:] == n0[1:], (n0, n1)     # a successful call moves the MX counter and no other
    return y, mean, rstd, q, s


def _check_case(dev, rows, Cd, store, merge=None, distinct=True, **inp):
    mhw = (merge[1], merge[2]) if merge else (0, 0)
    x, gamma, beta = (t.to(dev) for t in _inputs(rows, Cd, store, merge, seed=rows * 7919 + Cd, **inp))
    y0, m0, r0 = _plain(x, gamma, beta, rows, Cd, store, mhw)
    q0, s0 = _two_kernel_rows(y0, rows, Cd)
    y1, m1, r1, q1, s1 = _fused(x, gamma, beta, rows, Cd, store, mhw)
    _, _, _, q2, s2 = _fused(x, gamma, beta, rows, Cd, store, mhw, stored=False)          # y = mean = rstd = NULL
    torch.cuda.synchronize()
    # compare storage bit patterns, so that NaN guard rows compare equal to themselves
    bits = lambda t: t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)     # noqa: E731
    assert bool(torch.isfinite(y0[:rows].float()).all())
    assert torch.equal(bits(y1[:rows]), bits(y0[:rows])), "y"
    assert torch.equal(bits(m1[:rows]), bits(m0[:rows])) and torch.equal(bits(r1[:rows]), bits(r0[:rows])), "mean / rstd"
    assert torch.equal(q1[:rows], q0[:rows]), f"q differs from the GPU quantiser's in {int((q1[:rows] != q0[:rows]).sum())} bytes"
    assert torch.equal(s1[:rows], s0[:rows]), f"scales differ from the GPU quantiser's in {int((s1[:rows] != s0[:rows]).sum())} bytes"
    qe, se = mx_quant_rows(y0[:rows].cpu())                      # the CPU emulation on the downloaded y
    assert torch.equal(q1[:rows].cpu(), qe), f"q differs from the emulation in {int((q1[:rows].cpu() != qe).sum())} bytes"
    assert torch.equal(s1[:rows].cpu(), se), f"scales differ from the emulation in {int((s1[:rows].cpu() != se).sum())} bytes"
    assert torch.equal(q2, q1) and torch.equal(s2, s1), "the non-storing call writes other rows"
    # bounds: guard rows untouched, padding bytes of every real row zero, padding blocks' scale bytes 127
    assert bool((q1[rows:] == 0xAB).all()) and bool((s1[rows:] == 0xAB).all())
    assert bool(torch.isnan(y1[rows:].float()).all()) and bool(torch.isnan(m1[rows:]).all()) and bool(torch.isnan(r1[rows:]).all())
    nb = (Cd + 31) // 32                                         # real blocks
    assert q1.shape[1] == Cd or int(q1[:rows, Cd:].max()) == 0
    assert s1.shape[1] == nb or bool((s1[:rows, nb:] == 127).all())
    if distinct:
        n_distinct = min(len(set(row.tolist())) for row in s1[:rows, :nb].cpu())
        assert n_distinct >= 2, f"a row has {n_distinct} distinct scale byte(s): the inputs do not tell a block scale from a row scale"
    return y1, q1, s1


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["bf16", "f32"])
@pytest.mark.parametrize("Cd", CS)
@pytest.mark.parametrize("rows", ROWS)
def test_rows_and_block_scales_equal_the_two_kernel_operand(dev, rows, Cd, store):
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
    """beta = 0 and a constant row of x (or gamma = 0 everywhere): the row of y is all zeros, all its Kp bytes are zero and all its scale
    bytes 127 - next to rows that quantise normally."""
    rows, r = 37, 5
    kw = dict(beta_zero=True, const_row=r) if which == "constant row" else dict(beta_zero=True, gamma_zero=True)
    y, q, s = _check_case(dev, rows, Cd, store, distinct=False, **kw)
    zero_rows = [r] if which == "constant row" else list(range(rows))
    for i in zero_rows:
        assert float(y[i].float().abs().max()) == 0.0, i
        assert int(q[i].max()) == 0 and bool((s[i] == 127).all()), i
    if which == "constant row":
        nb = (Cd + 31) // 32
        assert float(y[r + 1].float().abs().max()) > 0.0 and int(q[r + 1].max()) > 0 and len(set(s[r + 1, :nb].tolist())) >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["bf16", "f32"])
def test_zero_rule_merged(dev, store):
    """the same on the merged form: image 0 of the source map is constant, so every merged row of it is"""
    I, H, W, C0 = 2, 4, 4, 24
    rows, Cd = I * (H // 2) * (W // 2), 4 * C0
    y, q, s = _check_case(dev, rows, Cd, store, merge=(I, H, W, C0), distinct=False, beta_zero=True, const_row=slice(0, H * W))
    per, nb = rows // I, (Cd + 31) // 32
    assert float(y[:per].float().abs().max()) == 0.0 and bool((s[:per] == 127).all()) and int(q[:per].max()) == 0
    assert float(y[per:rows].float().abs().max()) > 0.0 and all(len(set(row.tolist())) >= 2 for row in s[per:rows, :nb].cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("rows,Cd", [(37, 384), (5, 3072)])
def test_wide_range_f32(dev, rows, Cd):
    """fp32 storage, gamma / beta block factors 2^-40 ... 2^40 (every value normal): equality still holds, the scale bytes span the range, and
    no byte is 0x7F or 0xFF - nothing saturates and e4m3fn's NaN encoding never appears."""
    y, q, s = _check_case(dev, rows, Cd, "f32", wide=True)
    nb = (Cd + 31) // 32
    assert float(y[:rows].abs().max()) < 2.0 ** 60 and float(y[:rows][y[:rows] != 0].abs().min()) > 2.0 ** -100
    assert not bool(((q[:rows] & 0x7F) == 0x7F).any())
    assert int(s[:rows, :nb].max()) - int(s[:rows, :nb].min()) >= 70


@pytest.mark.gpu
def test_refused_call_does_not_count(dev):
    rows, Cd = 8, 96
    x, gamma, beta = (t.to(dev) for t in _inputs(rows, Cd, "bf16", None, seed=1))
    q = torch.zeros(rows + 1, 256, dtype=torch.uint8, device=dev)
    s = torch.zeros(rows + 1, 8, dtype=torch.uint8, device=dev)
    mean = torch.zeros(rows, dtype=torch.float32, device=dev)
    n0 = _counters()
    for args in ((ptr(q), 256, ptr(s), None, None),            # Kp != roundup(C, 128)
                 (None, 128, ptr(s), None, None),              # q null
                 (ptr(q), 128, None, None, None),              # scales_u8 null
                 (ptr(q), 128, ptr(s), ptr(mean), None),       # mean without rstd
                 (ptr(q) + 4, 128, ptr(s), None, None),        # q not 16-byte aligned
                 (ptr(q), 128, ptr(s) + 1, None, None)):       # scales_u8 not 4-byte aligned
        qp, Kp, sp, mp, rp = args
        with pytest.raises(RuntimeError, match="sv_layernorm_quant_mx_fwd"):
            call("sv_layernorm_quant_mx_fwd", ptr(x), ptr(gamma), ptr(beta), None, mp, rp, qp, Kp, sp, rows, Cd, 1e-5, 0, 0, act=hip.BF16)
    assert _counters() == n0
    _fused(x, gamma, beta, rows, Cd, "bf16", (0, 0), stored=False)          # asserts: only the MX counter moves
    torch.cuda.synchronize()
    assert bool((q == 0).all()) and bool((s == 0).all())         # and a refused call wrote nothing


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["bf16", "f32"])
@pytest.mark.parametrize("shape", [(49, 96, 288), (98, 192, 192)])
def test_end_to_end_into_the_mxfp8_linear(dev, shape, store):
    """sv_linear_mxfp8 on the fused kernel's rows and block scales and MX weight rows (the operand of the exact-integer test: block exponents
    -1 ... 2) gives, bit for bit, the output it gives on the two-kernel operand."""
    M, K, N = shape
    _, (wq, ws) = mx_integer_case(M, K, N)
    wq, ws = wq.contiguous().to(dev), ws.contiguous().to(dev)
    x, gamma, beta = (t.to(dev) for t in _inputs(M, K, store, None, seed=9 + M))
    y0, _, _ = _plain(x, gamma, beta, M, K, store, (0, 0))
    q0, s0 = _two_kernel_rows(y0, M, K)
    _, _, _, q1, s1 = _fused(x, gamma, beta, M, K, store, (0, 0), stored=False)
    outs = []
    for q, s in ((q0, s0), (q1, s1)):
        out = torch.full((M, N), float("nan"), dtype=_dt(store), device=dev)
        e = ops._epilogue(N)
        call("sv_linear_mxfp8", ptr(q), ptr(s), ptr(wq), ptr(ws), ptr(out), M, K, N, C.byref(e), None, None, act=_code(store))
        outs.append(out)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0].float()).all()) and float(outs[0].float().abs().max()) > 0.0
    assert torch.equal(outs[0], outs[1])
