"""The MX recipe of the fp8 Swin linears (swinvox_amd/csrc/linear_fp8.hip, "MX recipe") as a torch emulation, the checks that pin it, and the C
ABI of its entry points without a GPU.

The emulation is the yardstick tests/test_gpu_linear_mxfp8.py and tests/test_gpu_window_attention_mxq.py measure the kernels with, so it is
tested here on its own: the scale byte and the quantised maximum at the pinned block maxima, nothing saturates over 80 binades of bf16
data, the padding bytes and padding scales, exact integers, and the distance from the per-row recipe on N(0, 1) data.  The ABI part follows
tests/test_cpu_ln_quant_abi.py: the header declares and cites the entries, the ctypes tables bind them, and the refusals - host-side checks
that run before any GPU call - answer SV_ERR_INVALID and move no counter."""
import ctypes as C
import itertools
import math
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_linear_fp8_recipe import RECIPE_SHAPES, emulate_linear, gauss_case, l1_rel  # noqa: E402

from swinvox_amd import hip  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEPARATION = 1.5e-2        # the project's value (tests/test_gpu_linear_fp8.py): two recipes closer than this cannot be told apart by the bounds
BLOCK = 32


# ---- the emulation --------------------------------------------------------------------------------------------------------------------
def mx_block_exp(amax):
    """fp32 block maxima -> int32 E: amax = m 2^e, m in [1, 2): E = e - 8 + (m > 1.75) = ceil(log2(amax / 448)), read from the float's bits;
    clamped to >= -127 (e <= 128 keeps it <= 121); 0 for an all-zero block"""
    assert amax.dtype == torch.float32
    bits = amax.contiguous().view(torch.int32) & 0x7FFFFFFF
    E = (bits >> 23) - 127 - 8 + ((bits & 0x7FFFFF) > 0x600000).to(torch.int32)
    return torch.where(bits == 0, torch.zeros_like(E), torch.clamp(E, min=-127))


def mx_quant_rows(t):
    """stored tensor [R, K] (fp32 or bf16) -> (e4m3 bytes [R, Kp] uint8, E8M0 bytes [R, Kp / 32] uint8), Kp = roundup(K, 128): zero padding
    bytes, byte 127 for the blocks that lie wholly in the padding (they are all-zero blocks)"""
    t32 = t.float()
    R, K = t32.shape
    Kp = (K + 127) // 128 * 128
    blocks = torch.nn.functional.pad(t32, (0, Kp - K)).view(R, Kp // BLOCK, BLOCK)
    E = mx_block_exp(blocks.abs().amax(dim=2))
    q = torch.ldexp(blocks, -E[:, :, None]).to(torch.float8_e4m3fn)      # an exponent add: exact; then round to nearest even
    return q.view(torch.uint8).reshape(R, Kp), (E + 127).to(torch.uint8)


def mx_dequant(q, s, dtype=torch.float64):
    """(bytes, scale bytes) -> the values they stand for, [R, Kp]"""
    R, Kp = q.shape
    v = q.view(torch.float8_e4m3fn).float().to(dtype).view(R, Kp // BLOCK, BLOCK)
    return torch.ldexp(v, s.to(torch.int32)[:, :, None] - 127).reshape(R, Kp)


def emulate_linear_mx(x, W, bias=None, gelu=False, residual=None, row_scale=None, rows_per_scale=1, acc_dtype=torch.float64):
    """The MX recipe on the stored inputs: val = sum_k of the block-scaled products, no division; contraction and epilogue in acc_dtype.
    Returns (out, pre_act) in acc_dtype, before the store rounding."""
    val = mx_dequant(*mx_quant_rows(x), dtype=acc_dtype) @ mx_dequant(*mx_quant_rows(W), dtype=acc_dtype).T
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


PERMS = torch.tensor(list(itertools.permutations([-1, 0, 1, 2])), dtype=torch.int32)      # [24, 4]


def mx_integer_case(M, K, N, seed=0):
    """Operand BYTES and SCALE BYTES built directly (not through a quantiser): integer values |v| <= 2 and block exponents in {-1, 0, 1, 2}.
    The four blocks of a row in a k-step carry one of the 24 orderings of the four exponents, ordering (r mod 16 + k-step + 5 (r div 16)) mod 24:
    no two blocks of a k-step, no two rows of a 16-row fragment and no two k-steps of a row (up to 24) agree.  Every product term is a
    multiple of 2^-2 and |sum| <= 64 K <= 2^17 at the largest K here (1536), so every partial sum is exact in fp32 whatever the order.  A scale
    applied to the wrong row, block or k-step changes the result."""
    g = torch.Generator().manual_seed(3000 + seed)
    Kp = (K + 127) // 128 * 128

    def operand(R, salt):
        v = torch.randint(-2, 3, (R, Kp), generator=g).float()
        v[:, K:] = 0.0
        r, ks = torch.arange(R)[:, None], torch.arange(Kp // 128)[None, :]
        E = PERMS[(r % 16 + ks + 5 * (r // 16) + salt) % 24].reshape(R, Kp // BLOCK)
        return v.to(torch.float8_e4m3fn).view(torch.uint8), (E + 127).to(torch.uint8)

    return operand(M, 0), operand(N, 1)


# ---- pins -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amax,byte,qmax", [(1.0, 119, 256.0), (1.75, 119, 448.0), (1.7578125, 120, 224.0), (224.0, 126, 448.0),
                                            (448.0, 127, 448.0), (450.0, 128, None), (0.0, 127, 0.0), (1e-30, 19, None)])
def test_pins(amax, byte, qmax):
    x = torch.zeros(1, 32)
    x[0, 5] = -amax
    x[0, 17] = amax / 3
    q, s = mx_quant_rows(x)
    assert q.shape == (1, 128) and s.shape == (1, 4)
    assert int(s[0, 0]) == byte, (amax, int(s[0, 0]))
    if qmax is not None:
        assert float(q.view(torch.float8_e4m3fn).float()[0, 5]) == -qmax
    assert s[0, 1:].tolist() == [127, 127, 127] and int(q[0, 32:].max()) == 0       # padding blocks


def test_scale_is_the_ceiling_of_log2():
    g = torch.Generator().manual_seed(1)
    a = torch.exp2(torch.empty(20000).uniform_(-100, 100, generator=g)).float()
    a = torch.cat([a, torch.tensor([448.0, 448.0 * 2, 224.0, 1.75, 3.5, 7.0, 1.875, 2.0 ** -126, 2.0 ** -140, 3e38])])
    E = mx_block_exp(a)
    ref = torch.clamp(torch.ceil(torch.log2(a.double() / 448.0)), min=-127).to(torch.int32)
    assert torch.equal(E, ref)
    assert int(E.max()) <= 127 and int((E + 127).max()) < 255                       # byte 255 (NaN in E8M0) is never produced


def test_nothing_saturates():
    """max|q| <= 448 over bf16 data scaled by 2^-40 ... 2^40, and the block maximum lands in (224, 448]"""
    g = torch.Generator().manual_seed(2)
    for e in range(-40, 41, 4):
        x = (torch.randn(64, 200, generator=g) * 2.0 ** e).to(torch.bfloat16)
        q, s = mx_quant_rows(x)
        v = q.view(torch.float8_e4m3fn).float()
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) <= 448.0
        bm = v.view(64, -1, 32).abs().amax(dim=2)[:, :200 // 32]                    # the blocks that lie wholly inside K
        assert float(bm.min()) > 200.0                                              # 224 less e4m3's rounding
        assert l1_rel(mx_dequant(q, s)[:, :200], x.double()) < 4e-2


@pytest.mark.parametrize("K", [64, 96, 100, 192])
def test_padding(K):
    x, _ = gauss_case(20, K, 8, seed=K)
    q, s = mx_quant_rows(x)
    Kp = (K + 127) // 128 * 128
    assert q.shape == (20, Kp) and s.shape == (20, Kp // 32)
    assert int(q[:, K:].max()) == 0
    assert bool((s[:, (K + 31) // 32:] == 127).all())
    # a block that straddles K is scaled by its real elements only
    if K % 32:
        b = K // 32
        assert torch.equal(s[:, b].to(torch.int32) - 127, mx_block_exp(x[:, 32 * b:].abs().amax(dim=1)))


@pytest.mark.parametrize("shape", [(49, 96, 288), (130, 1536, 384)])
def test_integer_case_is_exact(shape):
    M, K, N = shape
    (xq, xs), (wq, ws) = mx_integer_case(M, K, N)
    for s in (xs, ws):
        e = s.to(torch.int32) - 127
        assert int(e.min()) == -1 and int(e.max()) == 2
        st = e.view(e.shape[0], -1, 4)                                                # [row][k-step][block]
        assert bool((st.sort(dim=2).values == torch.tensor([-1, 0, 1, 2])).all())     # the four blocks of a k-step all differ
        code = (st + 1).mul(torch.tensor([64, 16, 4, 1])).sum(dim=2)                  # one number per (row, k-step) ordering
        for f in range(0, e.shape[0] - 15, 16):                                       # the 16 rows of a fragment all differ, in every k-step
            assert all(len(set(code[f:f + 16, k].tolist())) == 16 for k in range(code.shape[1]))
        assert all(len(set(row.tolist())) == code.shape[1] for row in code)           # the k-steps of a row all differ
    ref64 = mx_dequant(xq, xs) @ mx_dequant(wq, ws).T
    ref32 = mx_dequant(xq, xs, torch.float32) @ mx_dequant(wq, ws, torch.float32).T
    assert torch.equal(ref32.double(), ref64) and float(ref64.abs().max()) < 2.0 ** 17
    unit = mx_dequant(xq, torch.full_like(xs, 127)) @ mx_dequant(wq, torch.full_like(ws, 127)).T
    assert not torch.equal(unit, ref64)                                               # the scales matter


@pytest.mark.parametrize("shape", RECIPE_SHAPES)
def test_distance_from_the_row_recipe(shape):
    """MX and the per-row recipe are two different roundings of the same product: each ~3.7e-2 from the exact product (e4m3's three mantissa
    bits set the error, not the granularity of the scales) and 5.25e-2 ... 5.35e-2 from one another - far enough apart for the bounds of the
    GPU tests to tell the two kernels apart."""
    x, W = gauss_case(*shape)
    exact = x.double() @ W.double().T
    mx, _ = emulate_linear_mx(x, W)
    row, _ = emulate_linear(x, W)
    d_exact, d_row = l1_rel(mx, exact), l1_rel(mx, row)
    print(f"{shape}: MX vs exact {d_exact:.3e}, row recipe vs exact {l1_rel(row, exact):.3e}, MX vs row recipe {d_row:.3e}")
    assert 3.5e-2 <= d_exact <= 3.9e-2, d_exact
    assert d_row >= SEPARATION, d_row
    mx32, _ = emulate_linear_mx(x, W, acc_dtype=torch.float32)
    assert l1_rel(mx32, mx) < 1e-6


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("sv_quant_rows_mx_e4m3", "sv_linear_mxfp8", "sv_window_attention_fwd_mxq", "sv_linear_mxfp8_launches", "sv_quant_rows_mx_launches")
SV_ERR_INVALID = -1


def test_header_declares_and_cites():
    hdr = open(os.path.join(ROOT, "include", "swinvox_hip.h")).read()
    for name in ENTRIES:
        m = re.search(r"(/\*(?:(?!\*/).)*\*/\s*)?\b(?:int|long long)\s+" + name + r"\s*\([^;]*\)\s*;[ \t]*(/\*(?:(?!\*/).)*\*/)?", hdr, flags=re.S)
        assert m, f"{name} is not declared"
        comment = (m.group(1) or "") + (m.group(2) or "")
        assert "models/swin_transformer.py:78" in comment, (name, comment)


def test_exported_and_bound():
    for name in ENTRIES:
        assert name in hip.EXPORTED_SYMBOLS
    assert "sv_linear_mxfp8" in hip._ACT_TYPED and "sv_window_attention_fwd_mxq" in hip._ACT_TYPED
    assert "sv_quant_rows_mx_e4m3" not in hip._ACT_TYPED
    lib = hip.load()                          # dlopen only: no GPU call is made
    assert lib.sv_linear_mxfp8_launches() >= 0 and lib.sv_quant_rows_mx_launches() >= 0
    assert len(hip._argtypes("sv_quant_rows_mx_e4m3")) == 9 and len(hip._argtypes("sv_linear_mxfp8")) == 13
    assert len(hip._argtypes("sv_window_attention_fwd_mxq")) == 15


# fake, suitably aligned device addresses: every call below is refused before anything could read them
XQ, XS, WQ, WS, OUT, QO, QSO, PTR = (0x10000 * (i + 1) for i in range(8))


def _epi(N=128, **kw):
    f = dict(bias=None, residual=None, ldr=0, row_scale=None, rows_per_scale=1, pre_act=None, stats=None, act=hip.ACT_NONE, slope=0.0,
             act_grad_src=None, act_grad_kind=hip.ACT_NONE, ldc=N, col_off=0)
    f.update(kw)
    return hip.Epilogue(f["bias"], f["residual"], f["ldr"], f["row_scale"], f["rows_per_scale"], f["pre_act"], f["stats"], f["act"], f["slope"],
                        f["act_grad_src"], f["act_grad_kind"], f["ldc"], f["col_off"])


def _counters(lib):
    return lib.sv_linear_mxfp8_launches(), lib.sv_quant_rows_mx_launches(), lib.sv_linear_fp8_launches()


@pytest.mark.parametrize("what,over", [
    ("src null", dict(src=None)),
    ("dst_q null", dict(q=None)),
    ("scales null", dict(s=None)),
    ("Kp not roundup(K, 128)", dict(Kp=256)),
    ("Kp below K", dict(K=192, ld=192, Kp=128)),
    ("Kp not a multiple of 128", dict(Kp=96)),
    ("bad dtype", dict(dt=7)),
    ("rows = 0", dict(rows=0)),
    ("ld < K", dict(ld=64)),
])
def test_quantiser_refusals_before_any_gpu_call(what, over):
    lib = hip.load()
    a = dict(src=PTR, dt=hip.F32, rows=4, K=96, ld=96, q=XQ, Kp=128, s=XS)
    a.update(over)
    n0 = _counters(lib)
    rc = lib.sv_quant_rows_mx_e4m3(a["src"], a["dt"], a["rows"], a["K"], a["ld"], a["q"], a["Kp"], a["s"], None)
    assert rc == SV_ERR_INVALID, (what, rc)
    assert "sv_quant_rows_mx_e4m3" in lib.sv_last_error().decode(), (what, lib.sv_last_error())
    assert _counters(lib) == n0, what


@pytest.mark.parametrize("what,over,epi", [
    ("xq null", dict(xq=None), {}),
    ("xs null", dict(xs=None), {}),
    ("wq null", dict(wq=None), {}),
    ("ws null", dict(ws=None), {}),
    ("out null without q_out", dict(out=None), {}),
    ("q_out without qs_out", dict(q_out=QO), {}),
    ("qs_out without q_out", dict(qs_out=QSO), {}),
    ("emission with a residual", dict(q_out=QO, qs_out=QSO), dict(residual=PTR, ldr=128)),
    ("emission with N % 128 != 0", dict(q_out=QO, qs_out=QSO, N=96), dict(ldc=96)),
    ("out null with pre_act", dict(out=None, q_out=QO, qs_out=QSO), dict(pre_act=PTR)),
    ("stats", {}, dict(stats=PTR)),
    ("act_grad_src", {}, dict(act_grad_src=PTR, act_grad_kind=hip.ACT_GELU)),
    ("col_off", {}, dict(ldc=256, col_off=128)),
    ("lrelu", {}, dict(act=hip.ACT_LRELU, slope=0.2)),
    ("ldc < N", {}, dict(ldc=64)),
    ("bad activation dtype", dict(act=7), {}),
    ("M = 0", dict(M=0), {}),
])
def test_gemm_refusals_before_any_gpu_call(what, over, epi):
    lib = hip.load()
    a = dict(xq=XQ, xs=XS, wq=WQ, ws=WS, out=OUT, M=16, K=128, N=128, q_out=None, qs_out=None, act=hip.BF16)
    a.update(over)
    e = _epi(a["N"], **epi)
    n0 = _counters(lib)
    rc = lib.sv_linear_mxfp8(a["xq"], a["xs"], a["wq"], a["ws"], a["out"], a["M"], a["K"], a["N"], C.byref(e), a["q_out"], a["qs_out"], a["act"], None)
    assert rc == SV_ERR_INVALID, (what, rc)
    assert "sv_linear_mxfp8" in lib.sv_last_error().decode() or what == "bad activation dtype", (what, lib.sv_last_error())
    assert _counters(lib) == n0, what


@pytest.mark.parametrize("what,over", [
    ("exact-f32 math", dict(math=hip.MATH_F32, act=hip.F32)),
    ("q_out null", dict(q_out=None)),
    ("qs_out null", dict(qs_out=None)),
    ("Kp not roundup(C, 128)", dict(Kp=256)),
    ("Kp below C", dict(C=192, heads=6, Kp=128)),
    ("qkv null", dict(qkv=None)),
    ("C != 32 heads", dict(heads=4)),
])
def test_attention_emission_refusals_before_any_gpu_call(what, over):
    lib = hip.load()
    a = dict(qkv=PTR, table=WQ, out=OUT, I=1, H=7, W=7, C=96, heads=3, shift=0, math=hip.MATH_BF16, q_out=QO, Kp=128, qs_out=QSO, act=hip.BF16)
    a.update(over)
    rc = lib.sv_window_attention_fwd_mxq(a["qkv"], a["table"], a["out"], a["I"], a["H"], a["W"], a["C"], a["heads"], a["shift"], a["math"],
                                         a["q_out"], a["Kp"], a["qs_out"], a["act"], None)
    assert rc == SV_ERR_INVALID, (what, rc)
    assert "window_attention" in lib.sv_last_error().decode(), (what, lib.sv_last_error())
