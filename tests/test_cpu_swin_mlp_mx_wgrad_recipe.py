"""The MXFP8 weight gradients of the fused Swin MLP (swinvox_amd/csrc/swin_mlp.hip, swin_mlp_wgrad_mx_kernel) as a torch emulation, and the C ABI of
its entry points without a GPU.

The recipe is the unfused MX weight-gradient chain's, composed: ln = bf16(LN(x1)) -> MX rows -> fc1 on MX operands -> hpre = bf16(acc + b1), h =
bf16(gelu_fast(acc + b1)) (GELU at the fp32 value, as the MX forward); dbr = bf16(s dx2) -> MX rows -> . W2^T in MX rows -> * gelu_grad_fast(hpre), bf16 =
dh (GELU' at the bf16 pre-activation, as the MX data gradient); then the MX COLUMN quantiser (blocks of 32 consecutive tokens of one column) on all four
of dbr, h, dh, ln: dW2 = q_cols(dbr) . q_cols(h)^T, dW1 = q_cols(dh) . q_cols(ln)^T; db2 / db1 = column sums of the unquantised dbr / dh.
tests/test_gpu_swin_mlp_mx_wgrad.py measures the kernel with emulate_swin_mlp_wgrad_mx, so it is tested on its own here."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_linear_mxfp8_recipe import emulate_linear_mx, mx_dequant, mx_quant_rows  # noqa: E402
from test_cpu_linear_mxfp8_bwd_recipe import emulate_dgrad_mx, emulate_wgrad_mx, mx_quant_cols  # noqa: E402
from test_cpu_swin_mlp_mx_recipe import gauss_mlp_case, gelu_fast32, layernorm_bf16  # noqa: E402
from test_cpu_swin_mlp_mx_bwd_recipe import GELU_GRAD_BOUND, dgrad_seed, gelu_grad_fast32  # noqa: E402

from swinvox_amd import hip  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GELU_BOUND = 2.9e-5               # common.h / DESIGN 4a: |gelu_fast - GELU_erf| everywhere


# ---- the emulation --------------------------------------------------------------------------------------------------------------------
def _token_scale(M, row_scale, rows_per_scale):
    if row_scale is None:
        return torch.ones(M, dtype=torch.float32)
    return row_scale.float()[torch.arange(M) // rows_per_scale]


def _gelu_fast(x):
    """gelu_fast32's formula in the dtype of x (the exact mode runs it in fp64)"""
    x2 = torch.clamp(x * x, max=64.0)
    p = x2 * (x2 * 9.975397e-04 + -1.0665937e-01) + -2.3012706e+00
    return x * (1.0 / (1.0 + torch.exp2(x * p)))


def emulate_swin_mlp_wgrad_mx(x1, dx2, ln_g, ln_b, W1, b1, W2, row_scale=None, rows_per_scale=1, eps=1e-5, exact=False, **_unused):
    """(dw1 [4C, C], db1 [4C], dw2 [C, 4C], db2 [C]) in fp64.  exact=True replaces every quantiser and every bf16 rounding by the identity (fp64
    throughout): the formula without the rounding."""
    M = x1.shape[0]
    sc = _token_scale(M, row_scale, rows_per_scale)
    if exact:
        x = x1.double()
        ln = torch.nn.functional.layer_norm(x, x.shape[1:], ln_g.double(), ln_b.double(), eps)
        hpre = ln @ W1.double().T + b1.double()
        h = _gelu_fast(hpre)
        dbr = sc.double()[:, None] * dx2.double()
        dh = (dbr @ W2.double()) * gelu_grad_fast32(hpre)
        return dh.T @ ln, dh.sum(dim=0), dbr.T @ h, dbr.sum(dim=0)
    ln = layernorm_bf16(x1, ln_g, ln_b, eps)                                     # 1.
    pre, _ = emulate_linear_mx(ln, W1, bias=b1)                                  # 2.
    hpre = pre.float().to(torch.bfloat16)                                        # 3. GELU at the fp32 value, GELU' (5.) at the bf16 one
    h = gelu_fast32(pre.float()).to(torch.bfloat16)
    dbr = (sc[:, None] * dx2.float()).to(torch.bfloat16)                         # 4. sv_rowscale's value
    acc = emulate_dgrad_mx(dbr, W2)                                              # 5. fc2 data gradient
    dh = (acc.float() * gelu_grad_fast32(hpre.float())).to(torch.bfloat16)
    dw2 = emulate_wgrad_mx(dbr, h)                                               # 6. blocks of 32 tokens per column
    dw1 = emulate_wgrad_mx(dh, ln)
    return dw1, dh.double().sum(dim=0), dw2, dbr.double().sum(dim=0)             # 7. bias gradients from the unquantised bf16 values


@pytest.mark.parametrize("C", [96, 128])
def test_emulation_is_the_composition_of_the_mx_helpers(C):
    M = 37                                                                       # one full 32-token block and a partly filled one per column
    c = gauss_mlp_case(M, C, windows=5)
    dx2 = dgrad_seed(c["x1"])
    dw1, db1, dw2, db2 = emulate_swin_mlp_wgrad_mx(dx2=dx2, **c)
    assert dw1.shape == (4 * C, C) and db1.shape == (4 * C,) and dw2.shape == (C, 4 * C) and db2.shape == (C,)
    assert all(t.dtype == torch.float64 for t in (dw1, db1, dw2, db2))
    ln = layernorm_bf16(c["x1"], c["ln_g"], c["ln_b"], c["eps"])
    lq, ls = mx_quant_rows(ln)
    w1q, w1s = mx_quant_rows(c["W1"])
    acc1 = mx_dequant(lq, ls) @ mx_dequant(w1q, w1s).T + c["b1"].double()
    hpre = acc1.float().to(torch.bfloat16)
    h = gelu_fast32(acc1.float()).to(torch.bfloat16)
    assert not torch.equal(h, gelu_fast32(hpre.float()).to(torch.bfloat16))      # GELU at the fp32 value is NOT GELU at the stored pre-activation
    sc = c["row_scale"][torch.arange(M) // c["rows_per_scale"]]
    assert bool((sc == 0).any()) and bool((sc != 0).any())                       # dropped and live scale groups
    dbr = (sc[:, None] * dx2.float()).to(torch.bfloat16)
    dq, ds = mx_quant_rows(dbr)
    w2tq, w2ts = mx_quant_cols(c["W2"])
    assert w2tq.shape == (4 * C, 128) and w2ts.shape == (4 * C, 4)
    dh = ((mx_dequant(dq, ds) @ mx_dequant(w2tq, w2ts).T).float() * gelu_grad_fast32(hpre.float())).to(torch.bfloat16)
    cols = {}
    for name, t in (("dbr", dbr), ("h", h), ("dh", dh), ("ln", ln)):
        q, s = mx_quant_cols(t)
        assert q.shape == (t.shape[1], 128) and s.shape == (t.shape[1], 4)       # [columns][Mp = 128], blocks of 32 tokens counted from token 0
        assert int(q[:, M:].max()) == 0 and bool((s[:, 2:] == 127).all())        # rows past M are zero; all-zero blocks carry byte 127
        qr, sr = mx_quant_rows(t.T.contiguous())
        assert torch.equal(q, qr) and torch.equal(s, sr)                         # the row quantiser on the transposed stored tensor
        cols[name] = mx_dequant(q, s)
    # a partly filled last block takes the maximum of its valid rows: quantising the five valid rows alone gives the same bytes and scale
    qt, st = mx_quant_cols(dbr[32:])
    qf, sf = mx_quant_cols(dbr)
    assert torch.equal(qt[:, :5], qf[:, 32:37]) and torch.equal(st[:, 0], sf[:, 1])
    assert torch.equal(dw2, cols["dbr"] @ cols["h"].T) and torch.equal(dw1, cols["dh"] @ cols["ln"].T)
    assert torch.equal(db2, dbr.double().sum(dim=0)) and torch.equal(db1, dh.double().sum(dim=0))


@pytest.mark.parametrize("C", [96, 128])
def test_formula_matches_autograd_without_the_rounding(C):
    """Identity quantisers: the emulation against torch.autograd through fp64 LayerNorm -> Linear -> GELU(erf) -> Linear -> scale -> residual.  The
    differences are gelu_fast against GELU_erf on h (|.| <= 2.9e-5) and gelu_grad_fast against the erf derivative on dh / (dbr W2) (|.| <= 1.1e-4);
    each passes through one sum over the tokens, which gives the element-wise bounds asserted here.  db2 does not pass a GELU: it is exact."""
    M = 37
    c = gauss_mlp_case(M, C, windows=5)
    dx2 = dgrad_seed(c["x1"])
    dw1, db1, dw2, db2 = emulate_swin_mlp_wgrad_mx(dx2=dx2, exact=True, **c)
    x = c["x1"].double()
    W1, B1, W2, B2 = (c[k].double().requires_grad_(True) for k in ("W1", "b1", "W2", "b2"))
    sc = _token_scale(M, c["row_scale"], c["rows_per_scale"]).double()
    ln = torch.nn.functional.layer_norm(x, (C,), c["ln_g"].double(), c["ln_b"].double(), c["eps"])
    h = torch.nn.functional.gelu(ln @ W1.T + B1)
    x2 = x + sc[:, None] * (h @ W2.T + B2)
    x2.backward(dx2.double())
    dbr = sc[:, None] * dx2.double()
    e_dh = GELU_GRAD_BOUND * (dbr @ c["W2"].double()).abs()                      # [M, 4C]
    slack = 1e-9
    assert bool(((dw1 - W1.grad).abs() <= e_dh.T @ ln.abs() + slack).all())
    assert bool(((db1 - B1.grad).abs() <= e_dh.sum(dim=0) + slack).all())
    assert bool(((dw2 - W2.grad).abs() <= GELU_BOUND * dbr.abs().sum(dim=0)[:, None] + slack).all())
    assert float((db2 - B2.grad).abs().max()) <= slack
    assert float((dw1 - W1.grad).abs().max()) > 0 and float((dw2 - W2.grad).abs().max()) > 0      # and they ARE the fast forms
    for got, ref in ((dw1, W1.grad), (db1, B1.grad), (dw2, W2.grad)):
        rel = float((got - ref).abs().max() / ref.abs().max())
        assert rel < 1e-3, rel


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("sv_swin_mlp_wgrad_mx_supported", "sv_swin_mlp_wgrad_mx", "sv_swin_mlp_wgrad_mx_launches")
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
    assert lib.sv_swin_mlp_wgrad_mx_launches() >= 0
    assert lib.sv_swin_mlp_wgrad_mx_supported(96) in (0, 1) and lib.sv_swin_mlp_wgrad_mx_supported(128) in (0, 1)
    assert [lib.sv_swin_mlp_wgrad_mx_supported(c) for c in (192, 64, 0)] == [0, 0, 0]
    # the sibling's arguments with (w1q, w1s, w2tq, w2ts) in place of (w1_rows, w2t_rows)
    assert len(hip._argtypes("sv_swin_mlp_wgrad_mx")) == 19 == len(hip._argtypes("sv_swin_mlp_wgrad")) + 2


# fake, suitably aligned device addresses: every call below is refused before anything could read them
X1, DX2, LG, LB, W1Q, W1S, W2TQ, W2TS, B1, RS, DW1, DB1, DW2, DB2 = (0x10000 * (i + 1) for i in range(14))
ORDER = ("x1", "dx2", "g", "b", "w1q", "w1s", "w2tq", "w2ts", "b1", "rs", "rps", "dw1", "db1", "dw2", "db2", "M", "C")


def _served_width():
    lib = hip.load()
    served = [c for c in (96, 128) if lib.sv_swin_mlp_wgrad_mx_supported(c) == 1]
    assert served, "sv_swin_mlp_wgrad_mx_supported serves neither width"
    return served[0]


@pytest.mark.parametrize("what,over", [
    ("x1 null", dict(x1=None)),
    ("dx2 null", dict(dx2=None)),
    ("ln_g null", dict(g=None)),
    ("ln_b null", dict(b=None)),
    ("w1q null", dict(w1q=None)),
    ("w1s null", dict(w1s=None)),
    ("w2tq null", dict(w2tq=None)),
    ("w2ts null", dict(w2ts=None)),
    ("b1 null", dict(b1=None)),
    ("dw1 null", dict(dw1=None)),
    ("db1 null", dict(db1=None)),
    ("dw2 null", dict(dw2=None)),
    ("db2 null", dict(db2=None)),
    ("C = 192", dict(C=192)),
    ("C = 64", dict(C=64)),
    ("M = 0", dict(M=0)),
    ("M < 0", dict(M=-5)),
    ("M = 2^31", dict(M=1 << 31)),
    ("x1 misaligned", dict(x1=X1 + 8)),
    ("dx2 misaligned", dict(dx2=DX2 + 4)),
    ("w1q misaligned", dict(w1q=W1Q + 4)),
    ("w2tq misaligned", dict(w2tq=W2TQ + 8)),
    ("w1s misaligned", dict(w1s=W1S + 2)),
    ("w2ts misaligned", dict(w2ts=W2TS + 1)),
    ("rows_per_scale = 0", dict(rps=0)),
    ("rows_per_scale < 0", dict(rps=-150)),
    ("row_scale with rows_per_scale < 128", dict(rps=127)),
    ("rows_per_scale = 0 without row_scale", dict(rs=None, rps=0)),
])
def test_refusals_before_any_gpu_call(what, over):
    lib = hip.load()
    a = dict(x1=X1, dx2=DX2, g=LG, b=LB, w1q=W1Q, w1s=W1S, w2tq=W2TQ, w2ts=W2TS, b1=B1, rs=RS, rps=150, dw1=DW1, db1=DB1, dw2=DW2, db2=DB2, M=300,
             C=_served_width())
    a.update(over)
    n0 = lib.sv_swin_mlp_wgrad_mx_launches()
    rc = lib.sv_swin_mlp_wgrad_mx(*(a[k] for k in ORDER), 1e-5, None)
    assert rc == SV_ERR_INVALID, (what, rc)
    assert "sv_swin_mlp_wgrad_mx" in lib.sv_last_error().decode(), (what, lib.sv_last_error())
    assert lib.sv_swin_mlp_wgrad_mx_launches() == n0, what


def test_existing_entry_keeps_its_refusals():
    lib = hip.load()
    assert lib.sv_swin_mlp_wgrad(X1, DX2, LG, LB, W1Q, W2TQ, B1, RS, 127, DW1, DB1, DW2, DB2, 300, 96, 1e-5, None) == SV_ERR_INVALID
    assert "swin_mlp_wgrad" in lib.sv_last_error().decode() and "sv_swin_mlp_wgrad_mx" not in lib.sv_last_error().decode()
    assert lib.sv_swin_mlp_wgrad(X1, None, LG, LB, W1Q, W2TQ, B1, RS, 150, DW1, DB1, DW2, DB2, 300, 96, 1e-5, None) == SV_ERR_INVALID
    assert lib.sv_swin_mlp_wgrad(X1, DX2, LG, LB, W1Q, W2TQ, B1, RS, 150, DW1, DB1, DW2, DB2, 300, 64, 1e-5, None) == SV_ERR_INVALID


def test_switch_is_off_by_default_and_needs_both_mx_recipes():
    import inspect
    import swinvox_amd as S
    from swinvox_amd import ops
    served = {c: hip.load().sv_swin_mlp_wgrad_mx_supported(c) == 1 for c in (96, 128)}
    assert inspect.signature(ops.set_fused_mlp_mx).parameters["wgrad"].default is False
    assert not ops._STATE.get("fused_mlp_mx_wgrad", False)
    assert not ops.fused_mlp_mx_wgrad_enabled(96)
    assert ops.swin_mlp_mx_wgrad_launches() == hip.load().sv_swin_mlp_wgrad_mx_launches()
    try:
        ops.set_math("bf16")
        ops.set_storage("bf16")
        S.set_linear_fp8(True, backward=True, recipe="mx", backward_recipe="mx")
        ops.set_fused_mlp_mx(True)                                               # existing calls behave as before
        assert ops.fused_mlp_mx_enabled(96) and not ops.fused_mlp_mx_wgrad_enabled(96) and not ops.fused_mlp_mx_bwd_enabled(96)
        ops.set_fused_mlp_mx(True, backward=True)                                # independent of the data-gradient switch, either way
        assert ops.fused_mlp_mx_bwd_enabled(96) and not ops.fused_mlp_mx_wgrad_enabled(96)
        ops.set_fused_mlp_mx(True, wgrad=True)
        assert not ops.fused_mlp_mx_bwd_enabled(96)
        for c in (96, 128):
            assert ops.fused_mlp_mx_wgrad_enabled(c) == served[c]
        assert not ops.fused_mlp_mx_wgrad_enabled(192)
        S.set_linear_fp8(True, backward=True, recipe="mx", backward_recipe="row")
        assert not ops.fused_mlp_mx_wgrad_enabled(96)
        S.set_linear_fp8(True, backward=True, recipe="row", backward_recipe="mx")
        assert not ops.fused_mlp_mx_wgrad_enabled(96)
        S.set_linear_fp8(True, backward=False, recipe="mx", backward_recipe="mx")
        assert not ops.fused_mlp_mx_wgrad_enabled(96)
        S.set_linear_fp8(True, backward=True, recipe="mx", backward_recipe="mx")
        ops.set_fused_mlp_mx(False, wgrad=True)                                  # effective only with `on`
        assert not ops.fused_mlp_mx_wgrad_enabled(96)
        ops.set_fused_mlp_mx(True, wgrad=True)
        ops.set_fused_mlp(False)                                                 # no fused MLP, no fused weight gradient
        assert not ops.fused_mlp_mx_wgrad_enabled(96)
        ops.set_fused_mlp(True)
        ops.set_math("f32")
        assert not ops.fused_mlp_mx_wgrad_enabled(96)
    finally:
        ops.set_fused_mlp_mx(False)
        ops.set_fused_mlp(True)
        S.set_linear_fp8(False)
        ops.set_math("f32")


def test_environment_variable_sets_the_switch(monkeypatch):
    import swinvox_amd as S
    from swinvox_amd import ops
    try:
        ops.set_math("bf16")
        ops.set_storage("bf16")
        S.set_linear_fp8(True, backward=True, recipe="mx", backward_recipe="mx")
        ops.set_fused_mlp_mx(True)
        assert not ops.fused_mlp_mx_wgrad_enabled(96)
        monkeypatch.setenv("SV_FUSED_MLP_MX_WGRAD", "1")
        assert ops.fused_mlp_mx_wgrad_enabled(96) == (hip.load().sv_swin_mlp_wgrad_mx_supported(96) == 1)
        ops.set_fused_mlp_mx(False)                                              # still needs the MX forward of the block
        assert not ops.fused_mlp_mx_wgrad_enabled(96)
    finally:
        ops.set_fused_mlp_mx(False)
        S.set_linear_fp8(False)
        ops.set_math("f32")
