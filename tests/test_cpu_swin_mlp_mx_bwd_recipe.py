"""The MXFP8 data gradient of the fused Swin MLP (swinvox_amd/csrc/swin_mlp.hip, swin_mlp_bwd_mx_kernel) as a torch emulation, and the C ABI of its
entry points without a GPU.

The recipe is the unfused MX backward chain's, composed: recompute LN(x1) -> MX rows -> fc1 on MX operands -> hpre = bf16(acc + b1) as the MX forward
does; dbr = bf16(s dx2) -> MX rows (blocks of 32 channels) -> . W2^T in MX rows (blocks of 32 output channels of one hidden unit) -> * gelu_grad_fast(hpre),
bf16 -> MX rows (blocks of 32 hidden units) -> . W1^T in MX rows (blocks of 32 hidden units of one channel) -> bf16 -> LayerNorm backward + residual.
tests/test_gpu_swin_mlp_mx_bwd.py measures the kernel with emulate_swin_mlp_bwd_mx, so it is tested on its own here."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_linear_mxfp8_recipe import emulate_linear_mx, mx_dequant, mx_quant_rows  # noqa: E402
from test_cpu_linear_mxfp8_bwd_recipe import emulate_dgrad_mx, mx_quant_cols  # noqa: E402
from test_cpu_swin_mlp_mx_recipe import gauss_mlp_case, gelu_fast32, layernorm_bf16  # noqa: E402

from swinvox_amd import hip  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GELU_GRAD_BOUND = 1.1e-4          # common.h / DESIGN 4a: |gelu_grad_fast - d/dx GELU_erf| everywhere


# ---- the emulation --------------------------------------------------------------------------------------------------------------------
def gelu_grad_fast32(x):
    """common.h gelu_grad_fast restated: s (1 + x (1 - s) q'), s = 1 / (1 + exp2(x p)) as in gelu_fast32, q' = d/dx [x (c0 + c1 x^2 + c2 x^4)]"""
    x2 = torch.clamp(x * x, max=64.0)
    p = x2 * (x2 * 9.975397e-04 + -1.0665937e-01) + -2.3012706e+00
    s = 1.0 / (1.0 + torch.exp2(x * p))
    qd = x2 * (x2 * -3.45720919e-03 + 2.21791923e-01) + 1.59511919
    return s * (x * (1.0 - s) * qd + 1.0)


def dgrad_seed(x1, seed=0):
    """the seeded N(0, 1) dx2 (bf16) that goes with gauss_mlp_case"""
    g = torch.Generator().manual_seed(8100 + 17 * x1.shape[1] + seed)
    return torch.randn(x1.shape, generator=g).to(torch.bfloat16)


def _token_scale(M, row_scale, rows_per_scale):
    if row_scale is None:
        return torch.ones(M, dtype=torch.float32)
    return row_scale.float()[torch.arange(M) // rows_per_scale]


def layernorm_bwd64(dln, x1, dx2, ln_g, eps):
    """step 6 in fp64: dx1 = dx2 + rstd (dln g - mean(dln g) - xh mean(dln g xh)), dgamma = sum dln xh, dbeta = sum dln"""
    x, d = x1.double(), dln.double()
    mean = x.mean(dim=1, keepdim=True)
    rstd = torch.rsqrt(((x - mean) ** 2).mean(dim=1, keepdim=True) + eps)
    xh = (x - mean) * rstd
    gg = d * ln_g.double()
    dx1 = dx2.double() + rstd * (gg - gg.mean(dim=1, keepdim=True) - xh * (gg * xh).mean(dim=1, keepdim=True))
    return dx1, (d * xh).sum(dim=0), d.sum(dim=0)


def emulate_swin_mlp_bwd_mx(x1, dx2, ln_g, ln_b, W1, b1, W2, row_scale=None, rows_per_scale=1, eps=1e-5, exact=False, **_unused):
    """(dx1 [M, C], dgamma [C], dbeta [C]) in fp64 before the store rounding of dx1.  exact=True replaces every quantiser and every bf16 rounding by
    the identity (fp64 throughout): the formula without the rounding."""
    M = x1.shape[0]
    sc = _token_scale(M, row_scale, rows_per_scale)
    if exact:
        x = x1.double()
        ln = torch.nn.functional.layer_norm(x, x.shape[1:], ln_g.double(), ln_b.double(), eps)
        hpre = ln @ W1.double().T + b1.double()
        dbr = sc.double()[:, None] * dx2.double()
        dh = (dbr @ W2.double()) * gelu_grad_fast32(hpre)
        dln = dh @ W1.double()
        return layernorm_bwd64(dln, x1, dx2, ln_g, eps)
    ln = layernorm_bf16(x1, ln_g, ln_b, eps)                                     # 1. the recompute of swin_mlp_fwd_mx_kernel
    pre, _ = emulate_linear_mx(ln, W1, bias=b1)
    hpre = pre.float().to(torch.bfloat16)
    dbr = (sc[:, None] * dx2.float()).to(torch.bfloat16)                         # 2. sv_rowscale's value
    acc = emulate_dgrad_mx(dbr, W2)                                              # 3. fc2 data gradient
    dh = (acc.float() * gelu_grad_fast32(hpre.float())).to(torch.bfloat16)
    dln = emulate_dgrad_mx(dh, W1).to(torch.bfloat16)                            # 4 + 5. quantise dh, fc1 data gradient
    return layernorm_bwd64(dln, x1, dx2, ln_g, eps)                              # 6.


@pytest.mark.parametrize("C", [96, 128])
def test_emulation_is_the_composition_of_the_mx_helpers(C):
    M = 37
    c = gauss_mlp_case(M, C, windows=5)
    dx2 = dgrad_seed(c["x1"])
    dx1, dg, db = emulate_swin_mlp_bwd_mx(dx2=dx2, **c)
    ln = layernorm_bf16(c["x1"], c["ln_g"], c["ln_b"], c["eps"])
    lq, ls = mx_quant_rows(ln)
    w1q, w1s = mx_quant_rows(c["W1"])
    hpre = (mx_dequant(lq, ls) @ mx_dequant(w1q, w1s).T + c["b1"].double()).float().to(torch.bfloat16)
    sc = c["row_scale"][torch.arange(M) // c["rows_per_scale"]]
    assert bool((sc == 0).any()) and bool((sc != 0).any())                                         # dropped and live scale groups
    dbr = (sc[:, None] * dx2.float()).to(torch.bfloat16)
    dq, ds = mx_quant_rows(dbr)
    assert dq.shape == (M, 128) and ds.shape == (M, 4)
    if C == 96:
        assert int(dq[:, 96:].max()) == 0 and bool((ds[:, 3] == 127).all())                        # K padding: zero bytes, byte 127
    assert bool((ds[sc == 0] == 127).all())                                                        # all-zero rows: byte 127
    w2tq, w2ts = mx_quant_cols(c["W2"])
    assert w2tq.shape == (4 * C, 128) and w2ts.shape == (4 * C, 4)                                 # [4C][Np]: a block = 32 output channels of a hidden unit
    if C == 96:
        assert int(w2tq[:, 96:].max()) == 0 and bool((w2ts[:, 3] == 127).all())
    acc = mx_dequant(dq, ds) @ mx_dequant(w2tq, w2ts).T
    dh = (acc.float() * gelu_grad_fast32(hpre.float())).to(torch.bfloat16)
    hq, hs = mx_quant_rows(dh)
    assert hq.shape == (M, 4 * C) and hs.shape == (M, 4 * C // 32)                                 # blocks of 32 consecutive hidden units
    w1tq, w1ts = mx_quant_cols(c["W1"])
    assert w1tq.shape == (C, 4 * C) and w1ts.shape == (C, 4 * C // 32)                             # [C][4C]: a block = 32 hidden units of a channel
    dln = (mx_dequant(hq, hs) @ mx_dequant(w1tq, w1ts).T).to(torch.bfloat16)
    rx1, rdg, rdb = layernorm_bwd64(dln, c["x1"], dx2, c["ln_g"], c["eps"])
    assert torch.equal(dx1, rx1) and torch.equal(dg, rdg) and torch.equal(db, rdb)
    # gelu_grad_fast32 is the derivative of the forward's gelu_fast32 (central difference in fp64 arithmetic on the fp32 form)
    hp, eps_fd = hpre.double(), 1e-3
    fd = (gelu_fast32((hp + eps_fd).float()).double() - gelu_fast32((hp - eps_fd).float()).double()) / (2 * eps_fd)
    assert float((gelu_grad_fast32(hp) - fd).abs().max()) < 5e-3


@pytest.mark.parametrize("C", [96, 128])
def test_formula_matches_autograd_without_the_rounding(C):
    """Identity quantisers: the emulation against torch.autograd through fp64 LayerNorm -> Linear -> GELU(erf) -> Linear -> scale -> residual.  The only
    difference is gelu_grad_fast against the erf derivative, |.| <= 1.1e-4 on dh / (dy W2); it passes through the two linear maps that follow, which
    gives the element-wise bound asserted here."""
    M = 37
    c = gauss_mlp_case(M, C, windows=5)
    dx2 = dgrad_seed(c["x1"])
    dx1, dg, db = emulate_swin_mlp_bwd_mx(dx2=dx2, exact=True, **c)
    x = c["x1"].double().requires_grad_(True)
    gam, bet = c["ln_g"].double().requires_grad_(True), c["ln_b"].double().requires_grad_(True)
    sc = _token_scale(M, c["row_scale"], c["rows_per_scale"]).double()
    ln = torch.nn.functional.layer_norm(x, (C,), gam, bet, c["eps"])
    h = torch.nn.functional.gelu(ln @ c["W1"].double().T + c["b1"].double())
    x2 = x + sc[:, None] * (h @ c["W2"].double().T + c["b2"].double())
    x2.backward(dx2.double())
    # |d dh| <= bound |acc|; |d dln| <= that @ |W1|; the LayerNorm backward is linear in dln
    acc = (sc[:, None] * dx2.double()) @ c["W2"].double()
    e_dln = (GELU_GRAD_BOUND * acc.abs()) @ c["W1"].double().abs()
    xd = c["x1"].double()
    mean = xd.mean(dim=1, keepdim=True)
    rstd = torch.rsqrt(((xd - mean) ** 2).mean(dim=1, keepdim=True) + c["eps"])
    xh = ((xd - mean) * rstd).abs()
    B = e_dln * c["ln_g"].double().abs()
    e_dx = rstd * (B + B.mean(dim=1, keepdim=True) + xh * (B * xh).mean(dim=1, keepdim=True))
    slack = 1e-9
    assert bool(((dx1 - x.grad).abs() <= e_dx + slack).all()), float(((dx1 - x.grad).abs() - e_dx).max())
    assert bool(((dg - gam.grad).abs() <= (e_dln * xh).sum(dim=0) + slack).all())
    assert bool(((db - bet.grad).abs() <= e_dln.sum(dim=0) + slack).all())
    assert float((dx1 - x.grad).abs().max()) > 0                                                    # and it IS the fast derivative
    rel = float((dx1 - x.grad).abs().max() / (x.grad - dx2.double()).abs().max())
    assert rel < 1e-3, rel


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("sv_swin_mlp_bwd_mx_supported", "sv_swin_mlp_bwd_mx_pack_bytes", "sv_swin_mlp_bwd_mx_pack", "sv_swin_mlp_bwd_mx", "sv_swin_mlp_bwd_mx_launches")
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
    lib = hip.load()                          # dlopen only: no GPU call is made
    assert lib.sv_swin_mlp_bwd_mx_launches() >= 0
    assert lib.sv_swin_mlp_bwd_mx_supported(96) == 1                            # C = 96 is not optional
    assert lib.sv_swin_mlp_bwd_mx_supported(128) in (0, 1)                      # C = 128: while its instantiation is spill-free
    assert [lib.sv_swin_mlp_bwd_mx_supported(c) for c in (192, 64, 0)] == [0, 0, 0]
    # W1 rows and W2^T rows padded to 128 + W1^T rows + one E8M0 byte per 32 elements of each
    assert lib.sv_swin_mlp_bwd_mx_pack_bytes(96) == 2 * (384 * 128 + 384 * 4) + 96 * 384 + 96 * 12
    if lib.sv_swin_mlp_bwd_mx_supported(128):
        assert lib.sv_swin_mlp_bwd_mx_pack_bytes(128) == 2 * (512 * 128 + 512 * 4) + 128 * 512 + 128 * 16
    else:
        assert lib.sv_swin_mlp_bwd_mx_pack_bytes(128) == 0
    assert lib.sv_swin_mlp_bwd_mx_pack_bytes(192) == 0
    assert len(hip._argtypes("sv_swin_mlp_bwd_mx")) == 15 and len(hip._argtypes("sv_swin_mlp_bwd_mx_pack")) == 9
    assert hip._argtypes("sv_swin_mlp_bwd_mx") == hip._argtypes("sv_swin_mlp_bwd")


# fake, suitably aligned device addresses: every call below is refused before anything could read them
X1, DX2, DX1, LG, LB, PK, B1, RS, DG, DB, W1Q, W1S, W2TQ, W2TS, W1TQ, W1TS = (0x10000 * (i + 1) for i in range(16))


@pytest.mark.parametrize("what,over", [
    ("x1 null", dict(x1=None)),
    ("dx2 null", dict(dx2=None)),
    ("dx1 null", dict(dx1=None)),
    ("ln_g null", dict(g=None)),
    ("ln_b null", dict(b=None)),
    ("packs null", dict(packs=None)),
    ("b1 null", dict(b1=None)),
    ("dgamma null", dict(dg=None)),
    ("dbeta null", dict(db=None)),
    ("C = 192", dict(C=192)),
    ("C = 64", dict(C=64)),
    ("M = 0", dict(M=0)),
    ("M < 0", dict(M=-5)),
    ("M = 2^31", dict(M=1 << 31)),
    ("x1 misaligned", dict(x1=X1 + 8)),
    ("dx2 misaligned", dict(dx2=DX2 + 4)),
    ("dx1 misaligned", dict(dx1=DX1 + 2)),
    ("packs misaligned", dict(packs=PK + 4)),
    ("ln_g misaligned", dict(g=LG + 4)),
    ("ln_b misaligned", dict(b=LB + 8)),
    ("rows_per_scale = 0", dict(rps=0)),
    ("rows_per_scale < 0", dict(rps=-49)),
])
def test_backward_refusals_before_any_gpu_call(what, over):
    lib = hip.load()
    a = dict(x1=X1, dx2=DX2, dx1=DX1, g=LG, b=LB, packs=PK, b1=B1, rs=RS, rps=49, dg=DG, db=DB, M=147, C=96)
    a.update(over)
    n0 = lib.sv_swin_mlp_bwd_mx_launches()
    rc = lib.sv_swin_mlp_bwd_mx(a["x1"], a["dx2"], a["dx1"], a["g"], a["b"], a["packs"], a["b1"], a["rs"], a["rps"], a["dg"], a["db"], a["M"], a["C"],
                                1e-5, None)
    assert rc == SV_ERR_INVALID, (what, rc)
    assert "sv_swin_mlp_bwd_mx" in lib.sv_last_error().decode(), (what, lib.sv_last_error())
    assert lib.sv_swin_mlp_bwd_mx_launches() == n0, what


@pytest.mark.parametrize("what,over", [
    ("w1q null", dict(w1q=None)),
    ("w1s null", dict(w1s=None)),
    ("w2tq null", dict(w2tq=None)),
    ("w2ts null", dict(w2ts=None)),
    ("w1tq null", dict(w1tq=None)),
    ("w1ts null", dict(w1ts=None)),
    ("packs null", dict(packs=None)),
    ("C = 192", dict(C=192)),
    ("C = 0", dict(C=0)),
    ("w1q misaligned", dict(w1q=W1Q + 4)),
    ("w2tq misaligned", dict(w2tq=W2TQ + 8)),
    ("w1tq misaligned", dict(w1tq=W1TQ + 2)),
    ("packs misaligned", dict(packs=PK + 1)),
])
def test_pack_refusals_before_any_gpu_call(what, over):
    lib = hip.load()
    a = dict(w1q=W1Q, w1s=W1S, w2tq=W2TQ, w2ts=W2TS, w1tq=W1TQ, w1ts=W1TS, packs=PK, C=96)
    a.update(over)
    rc = lib.sv_swin_mlp_bwd_mx_pack(a["w1q"], a["w1s"], a["w2tq"], a["w2ts"], a["w1tq"], a["w1ts"], a["packs"], a["C"], None)
    assert rc == SV_ERR_INVALID, (what, rc)
    assert "sv_swin_mlp_bwd_mx_pack" in lib.sv_last_error().decode(), (what, lib.sv_last_error())


def test_existing_entry_keeps_its_refusals():
    lib = hip.load()
    assert lib.sv_swin_mlp_bwd(X1, DX2, DX1, LG, LB, PK, B1, RS, 0, DG, DB, 147, 96, 1e-5, None) == SV_ERR_INVALID
    assert "swin_mlp" in lib.sv_last_error().decode()
    assert lib.sv_swin_mlp_bwd(X1, None, DX1, LG, LB, PK, B1, RS, 49, DG, DB, 147, 96, 1e-5, None) == SV_ERR_INVALID
    assert lib.sv_swin_mlp_bwd(X1, DX2, DX1, LG, LB, PK, B1, RS, 49, DG, DB, 147, 64, 1e-5, None) == SV_ERR_INVALID


def test_switch_is_off_by_default_and_needs_both_mx_recipes():
    import swinvox_amd as S
    from swinvox_amd import ops
    assert not ops._STATE.get("fused_mlp_mx_bwd", False)
    assert not ops.fused_mlp_mx_bwd_enabled(96)
    try:
        ops.set_math("bf16")
        ops.set_storage("bf16")
        ops.set_fused_mlp_mx(True)                                               # the forward switch alone
        S.set_linear_fp8(True, backward=True, recipe="mx", backward_recipe="mx")
        assert ops.fused_mlp_mx_enabled(96) and not ops.fused_mlp_mx_bwd_enabled(96)
        ops.set_fused_mlp_mx(True, backward=True)
        assert ops.fused_mlp_mx_bwd_enabled(96)
        assert ops.fused_mlp_mx_bwd_enabled(128) == (hip.load().sv_swin_mlp_bwd_mx_supported(128) == 1)
        assert not ops.fused_mlp_mx_bwd_enabled(192)
        S.set_linear_fp8(True, backward=True, recipe="mx", backward_recipe="row")
        assert not ops.fused_mlp_mx_bwd_enabled(96)
        S.set_linear_fp8(True, backward=True, recipe="row", backward_recipe="mx")
        assert not ops.fused_mlp_mx_bwd_enabled(96)
        S.set_linear_fp8(True, backward=False, recipe="mx", backward_recipe="mx")
        assert not ops.fused_mlp_mx_bwd_enabled(96)
        S.set_linear_fp8(True, backward=True, recipe="mx", backward_recipe="mx")
        ops.set_fused_mlp_mx(False, backward=True)                               # backward needs the forward switch
        assert not ops.fused_mlp_mx_bwd_enabled(96)
        ops.set_fused_mlp_mx(True, backward=True)
        ops.set_math("f32")
        assert not ops.fused_mlp_mx_bwd_enabled(96)
    finally:
        ops.set_fused_mlp_mx(False)
        S.set_linear_fp8(False)
        ops.set_math("f32")
