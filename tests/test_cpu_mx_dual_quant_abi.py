"""C ABI and host switch of the MX dual quantiser (csrc/linear_fp8.hip, sv_quant_rows_cols_mx_e4m3 / sv_quant_rows_cols_mx_launches) without a
GPU: the header declares both entries and says which reference operator they stand for, the ctypes tables bind them, the argument refusals -
host-side checks that run before any GPU call - answer SV_ERR_INVALID with the entry's name in sv_last_error() and move no counter, and
ops.mx_dual_quant_enabled() is off by default, on only under the MX backward recipe with bf16 math, and inert everywhere else."""
import os
import re

import pytest

import swinvox_amd as S
from swinvox_amd import hip, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sv_quant_rows_cols_mx_e4m3", "sv_quant_rows_cols_mx_launches")
SV_ERR_INVALID = -1


def test_header_declares_and_cites():
    hdr = open(os.path.join(ROOT, "include", "swinvox_hip.h")).read()
    for name in ENTRIES:
        # the prototype, and the comment attached to it: right before the prototype or on its line
        m = re.search(r"(/\*(?:(?!\*/).)*\*/\s*)?\b(?:int|long long)\s+" + name + r"\s*\([^;]*\)\s*;[ \t]*(/\*(?:(?!\*/).)*\*/)?", hdr, flags=re.S)
        assert m, f"{name} is not declared"
        comment = (m.group(1) or "") + (m.group(2) or "")
        assert "models/swin_transformer.py:78" in comment, (name, comment)


def test_exported_and_bound():
    for name in ENTRIES:
        assert name in hip.EXPORTED_SYMBOLS
    assert "sv_quant_rows_cols_mx_e4m3" not in hip._ACT_TYPED      # the source type is an argument of its own
    lib = hip.load()                          # dlopen only: no GPU call is made
    assert lib.sv_quant_rows_cols_mx_launches() >= 0               # callable: a pure host function
    assert ops.quant_rows_cols_mx_launches() == lib.sv_quant_rows_cols_mx_launches()
    assert len(hip._argtypes("sv_quant_rows_cols_mx_e4m3")) == 13 and hip._argtypes("sv_quant_rows_cols_mx_launches") == []


# fake, suitably aligned device addresses: every call below is refused before anything could read them
SRC, RQ, RS, CQ, CS, SUM = (0x10000 * (i + 1) for i in range(6))


def _args(**over):
    a = dict(src=SRC, dt=hip.BF16, M=200, N=96, ld=96, rq=RQ, Np=128, rs=RS, cq=CQ, Mp=256, cs=CS, colsum=SUM)
    a.update(over)
    return (a["src"], a["dt"], a["M"], a["N"], a["ld"], a["rq"], a["Np"], a["rs"], a["cq"], a["Mp"], a["cs"], a["colsum"], None)


def _counters(lib):
    return lib.sv_quant_rows_cols_mx_launches(), lib.sv_quant_rows_mx_launches(), lib.sv_quant_cols_mx_launches()


@pytest.mark.parametrize("what,over", [
    ("src null", dict(src=None)),
    ("col_q null", dict(cq=None)),
    ("col_s null", dict(cs=None)),
    ("row_q without row_s", dict(rs=None)),
    ("row_s without row_q", dict(rq=None)),
    ("bad source dtype", dict(dt=7)),
    ("M = 0", dict(M=0, Mp=0)),
    ("N = 0", dict(N=0, Np=0, ld=0)),
    ("ld below N", dict(ld=95)),
    ("Np not roundup(N, 128)", dict(Np=256)),
    ("Np below N", dict(N=192, ld=192, Np=128)),
    ("Np wrong without the row pair", dict(rq=None, rs=None, Np=96)),
    ("Mp not roundup(M, 128)", dict(Mp=384)),
    ("Mp below M", dict(Mp=128)),
    ("row_q not 16-byte aligned", dict(rq=RQ + 8)),
    ("col_q not 16-byte aligned", dict(cq=CQ + 4)),
    ("row_s not 4-byte aligned", dict(rs=RS + 2)),
    ("col_s not 4-byte aligned", dict(cs=CS + 1)),
    ("Mp / 128 above 65535", dict(M=65536 * 128, Mp=65536 * 128)),
])
def test_refusals_before_any_gpu_call(what, over):
    lib = hip.load()
    n0 = _counters(lib)
    rc = lib.sv_quant_rows_cols_mx_e4m3(*_args(**over))
    assert rc == SV_ERR_INVALID, (what, rc)
    assert "sv_quant_rows_cols_mx_e4m3" in lib.sv_last_error().decode(), (what, lib.sv_last_error())
    assert _counters(lib) == n0, what


@pytest.fixture
def switches():
    try:
        yield
    finally:
        ops.set_mx_dual_quant(False)
        S.set_linear_fp8(False)
        S.set_math("f32")


def test_switch_semantics(monkeypatch, switches):
    """off by default; on only with the MX backward recipe, bf16 math and the setter or SV_MX_DUAL_QUANT=1 (handled as set_ln_quant_mx handles
    SV_LN_QUANT_MX); inert under backward_recipe "row", under backward=False, with the fp8 linears off and under f32 math (no GPU needed)"""
    monkeypatch.delenv("SV_MX_DUAL_QUANT", raising=False)
    S.set_math("bf16")
    S.set_linear_fp8(True, backward=True, recipe="mx", backward_recipe="mx")
    assert ops.linear_fp8_bwd_enabled() and ops.linear_fp8_bwd_recipe() == "mx"
    assert not ops.mx_dual_quant_enabled()                       # ships off
    ops.set_mx_dual_quant(True)
    assert ops.mx_dual_quant_enabled()
    ops.set_mx_dual_quant(False)
    assert not ops.mx_dual_quant_enabled()
    monkeypatch.setenv("SV_MX_DUAL_QUANT", "1")
    assert ops.mx_dual_quant_enabled()
    monkeypatch.setenv("SV_MX_DUAL_QUANT", "0")
    assert not ops.mx_dual_quant_enabled()
    monkeypatch.delenv("SV_MX_DUAL_QUANT")
    ops.set_mx_dual_quant(True)
    # either forward recipe, with and without the MX store
    for kw in (dict(recipe="row"), dict(recipe="mx", store="mx")):
        S.set_linear_fp8(True, backward=True, backward_recipe="mx", **kw)
        assert ops.mx_dual_quant_enabled(), kw
    # the row recipe of the backward, no fp8 backward, no fp8 linears: inert
    S.set_linear_fp8(True, backward=True, recipe="mx", backward_recipe="row")
    assert not ops.mx_dual_quant_enabled()
    S.set_linear_fp8(True, backward=False, recipe="mx", backward_recipe="mx")
    assert not ops.mx_dual_quant_enabled()
    S.set_linear_fp8(False)
    assert not ops.mx_dual_quant_enabled()
    # f32 math
    S.set_linear_fp8(True, backward=True, recipe="mx", backward_recipe="mx")
    assert ops.mx_dual_quant_enabled()
    S.set_math("f32")
    assert not ops.mx_dual_quant_enabled()
    monkeypatch.setenv("SV_MX_DUAL_QUANT", "1")
    assert not ops.mx_dual_quant_enabled()
    # the switch touches none of its neighbours
    S.set_math("bf16")
    assert not ops.ln_quant_mx_enabled() and ops.mx_producer_quant_enabled() and ops.linear_fp8_store() == "bf16"
