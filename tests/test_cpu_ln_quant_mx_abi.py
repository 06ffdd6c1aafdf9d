"""C ABI and host switch of the MX quantising LayerNorm (csrc/norm.hip, sv_layernorm_quant_mx_fwd / sv_layernorm_quant_mx_launches) without a
GPU: the header declares both entries and says which reference operator they stand for, the ctypes tables bind them, the argument refusals -
host-side checks that run before any GPU call - answer SV_ERR_INVALID with the entry's name in sv_last_error(), and ops.ln_quant_mx_enabled()
is off by default, on only under recipe "mx" with bf16 math, and leaves the row recipe's switch alone."""
import os
import re

import pytest

import swinvox_amd as S
from swinvox_amd import hip, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sv_layernorm_quant_mx_fwd", "sv_layernorm_quant_mx_launches")
SV_ERR_INVALID = -1


def test_header_declares_and_cites():
    hdr = open(os.path.join(ROOT, "include", "swinvox_hip.h")).read()
    for name in ENTRIES:
        # the prototype, and the comment attached to it: right before the prototype or on its line
        m = re.search(r"(/\*(?:(?!\*/).)*\*/\s*)?\b(?:int|long long)\s+" + name + r"\s*\([^;]*\)\s*;[ \t]*(/\*(?:(?!\*/).)*\*/)?", hdr, flags=re.S)
        assert m, f"{name} is not declared"
        comment = (m.group(1) or "") + (m.group(2) or "")
        assert "models/swin_transformer.py:78" in comment and "LayerNorm" in comment, (name, comment)


def test_exported_and_bound():
    for name in ENTRIES:
        assert name in hip.EXPORTED_SYMBOLS
    assert "sv_layernorm_quant_mx_fwd" in hip._ACT_TYPED
    lib = hip.load()                          # dlopen only: no GPU call is made
    assert lib.sv_layernorm_quant_mx_launches() >= 0                   # callable: a pure host function
    assert len(hip._argtypes("sv_layernorm_quant_mx_fwd")) == 16 and hip._argtypes("sv_layernorm_quant_mx_launches") == []


# fake, suitably aligned device addresses: every call below is refused before anything could read them
X, G, B, Y, MEAN, RSTD, Q, SC = (0x10000 * (i + 1) for i in range(8))


def _args(**over):
    a = dict(x=X, gamma=G, beta=B, y=Y, mean=MEAN, rstd=RSTD, q=Q, Kp=128, scales=SC, rows=4, C=96, eps=1e-5, mH=0, mW=0, act=hip.BF16)
    a.update(over)
    return (a["x"], a["gamma"], a["beta"], a["y"], a["mean"], a["rstd"], a["q"], a["Kp"], a["scales"], a["rows"], a["C"], a["eps"],
            a["mH"], a["mW"], a["act"], None)


@pytest.mark.parametrize("what,over", [
    ("q null", dict(q=None)),
    ("scales_u8 null", dict(scales=None)),
    ("Kp not roundup(C, 128)", dict(Kp=256)),
    ("Kp below C", dict(C=192, Kp=128)),
    ("mean without rstd", dict(rstd=None)),
    ("rstd without mean", dict(mean=None)),
    ("q not 16-byte aligned", dict(q=Q + 8)),
    ("scales_u8 not 4-byte aligned", dict(scales=SC + 2)),
    ("C = 10", dict(C=10)),
    ("C above 3072", dict(C=3200, Kp=3200)),
    ("x null", dict(x=None)),
    ("gamma null", dict(gamma=None)),
    ("gamma not 16-byte aligned", dict(gamma=G + 4)),
    ("rows = 0", dict(rows=0)),
    ("bad activation dtype", dict(act=7)),
    ("odd merge map", dict(mH=3, mW=4)),
    ("merged C not a multiple of 16", dict(C=104, mH=4, mW=4)),
])
def test_refusals_before_any_gpu_call(what, over):
    lib = hip.load()
    n0 = lib.sv_layernorm_quant_mx_launches(), lib.sv_layernorm_quant_launches()
    rc = lib.sv_layernorm_quant_mx_fwd(*_args(**over))
    assert rc == SV_ERR_INVALID, (what, rc)
    assert "sv_layernorm_quant_mx_fwd" in lib.sv_last_error().decode(), (what, lib.sv_last_error())
    assert (lib.sv_layernorm_quant_mx_launches(), lib.sv_layernorm_quant_launches()) == n0, what


@pytest.fixture
def switches():
    try:
        yield
    finally:
        ops.set_ln_quant_mx(False)
        S.set_linear_fp8(False)
        S.set_math("f32")


def test_switch_semantics(monkeypatch, switches):
    """off by default; on only with recipe "mx", bf16 math and the setter or SV_LN_QUANT_MX=1; inert under the row recipe and under f32 math;
    ln_quant_fused_enabled() (the row recipe's switch) does not see it (no GPU needed)"""
    monkeypatch.delenv("SV_LN_QUANT_MX", raising=False)
    monkeypatch.delenv("SV_LN_QUANT_FUSED", raising=False)
    S.set_math("bf16")
    S.set_linear_fp8(True, recipe="mx")
    assert not ops.ln_quant_mx_enabled()                         # ships off
    assert not ops.ln_quant_fused_enabled()
    ops.set_ln_quant_mx(True)
    assert ops.ln_quant_mx_enabled()
    assert not ops.ln_quant_fused_enabled()                      # the row form stays out of the MX recipe
    ops.set_ln_quant_mx(False)
    assert not ops.ln_quant_mx_enabled()
    monkeypatch.setenv("SV_LN_QUANT_MX", "1")
    assert ops.ln_quant_mx_enabled()
    monkeypatch.setenv("SV_LN_QUANT_MX", "0")
    assert not ops.ln_quant_mx_enabled()
    monkeypatch.delenv("SV_LN_QUANT_MX")
    ops.set_ln_quant_mx(True)
    # the row recipe: inert, and the row form's switch is what it was
    S.set_linear_fp8(True)
    assert not ops.ln_quant_mx_enabled() and ops.ln_quant_fused_enabled()
    ops.set_ln_quant_mx(False)
    assert ops.ln_quant_fused_enabled()
    ops.set_ln_quant_mx(True)
    # fp8 linears off, and f32 math
    S.set_linear_fp8(False)
    assert not ops.ln_quant_mx_enabled()
    S.set_linear_fp8(True, recipe="mx")
    assert ops.ln_quant_mx_enabled()
    S.set_math("f32")
    assert not ops.ln_quant_mx_enabled() and not ops.ln_quant_fused_enabled()
    monkeypatch.setenv("SV_LN_QUANT_MX", "1")
    assert not ops.ln_quant_mx_enabled()
