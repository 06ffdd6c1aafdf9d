"""C ABI of the quantising LayerNorm (csrc/norm.hip, sv_layernorm_quant_fwd / sv_layernorm_quant_launches) without a GPU: the header
declares both entries and says which reference operator they stand for, the ctypes tables bind them, and the argument refusals - host-side
checks that run before any GPU call - answer SV_ERR_INVALID with the entry's name in sv_last_error()."""
import ctypes
import os
import re

import pytest

from swinvox_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sv_layernorm_quant_fwd", "sv_layernorm_quant_launches")
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
    assert "sv_layernorm_quant_fwd" in hip._ACT_TYPED
    lib = hip.load()                          # dlopen only: no GPU call is made
    assert lib.sv_layernorm_quant_launches() >= 0                      # callable: a pure host function
    assert len(hip._argtypes("sv_layernorm_quant_fwd")) == 16 and hip._argtypes("sv_layernorm_quant_launches") == []


# fake, suitably aligned device addresses: every call below is refused before anything could read them
X, G, B, Y, MEAN, RSTD, Q, SC = (0x10000 * (i + 1) for i in range(8))


def _args(**over):
    a = dict(x=X, gamma=G, beta=B, y=Y, mean=MEAN, rstd=RSTD, q=Q, Kp=128, scales=SC, rows=4, C=96, eps=1e-5, mH=0, mW=0, act=hip.BF16)
    a.update(over)
    return (a["x"], a["gamma"], a["beta"], a["y"], a["mean"], a["rstd"], a["q"], a["Kp"], a["scales"], a["rows"], a["C"], a["eps"],
            a["mH"], a["mW"], a["act"], None)


@pytest.mark.parametrize("what,over", [
    ("q null", dict(q=None)),
    ("scales null", dict(scales=None)),
    ("Kp not roundup(C, 128)", dict(Kp=256)),
    ("Kp below C", dict(C=192, Kp=128)),
    ("mean without rstd", dict(rstd=None)),
    ("rstd without mean", dict(mean=None)),
    ("C = 10", dict(C=10)),
    ("x null", dict(x=None)),
    ("rows = 0", dict(rows=0)),
    ("bad activation dtype", dict(act=7)),
    ("odd merge map", dict(mH=3, mW=4)),
])
def test_refusals_before_any_gpu_call(what, over):
    lib = hip.load()
    n0 = lib.sv_layernorm_quant_launches()
    rc = lib.sv_layernorm_quant_fwd(*_args(**over))
    assert rc == SV_ERR_INVALID, (what, rc)
    assert "sv_layernorm_quant_fwd" in lib.sv_last_error().decode(), (what, lib.sv_last_error())
    assert lib.sv_layernorm_quant_launches() == n0, what
