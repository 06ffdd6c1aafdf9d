"""Characterization of the host path of the Swin blocks: every case of tests/golden/make_swin_host_trace.py (the fp8 / MX switch grid of
block_forward + block_backward at two shapes, fp8 attention, split fusion, drop-path, a weight-pack cache, f32 math, a patch-merging stage)
issues exactly the library calls - entry points, scalars, and WHICH buffer goes to which pointer argument - that the fixture recorded (a SHA-1
per distinct trace, and a few traces in full).
CPU tensors, recorder in place of call / ptr, the library only dlopen'ed for its queries: no GPU call is made."""
import importlib.util
import json
import os

import pytest

from swinvox_amd import hip, ops
from swinvox_amd.models import swin_transformer as st

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_swin_host_trace", os.path.join(HERE, "golden", "make_swin_host_trace.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

pytestmark = pytest.mark.skipif(not os.path.exists(hip.LIB_PATH), reason="the library is not built: its *_supported queries decide the paths")


@pytest.fixture(scope="module")
def traced():
    before = (dict(ops._STATE), hip.ACT, hip.TRACE, ops.call, ops.ptr, st.call, st.ptr, ops._CTX.packs, dict(os.environ))
    traces = gen.trace_all()
    assert before == (dict(ops._STATE), hip.ACT, hip.TRACE, ops.call, ops.ptr, st.call, st.ptr, ops._CTX.packs, dict(os.environ))
    return traces


@pytest.fixture(scope="module")
def golden():
    with open(gen.FIXTURE) as f:
        return json.load(f)


def test_every_case_issues_the_recorded_calls(traced, golden):
    assert gen.sha1(list(traced)) == golden["names"] and len(traced) == len(golden["cases"])
    for (name, trace), k in zip(traced.items(), golden["cases"]):
        for i, (got, exp) in enumerate(zip(trace, golden["traces"].get(str(k), []))):     # the traces kept in full: the first call that differs
            assert got == exp, f"{name}: call {i}"
        assert gen.sha1(trace) == golden["sha1"][k], f"{name}: {len(trace)} calls, {[c[0] for c in trace]}"


def test_fixture_covers_the_grid_and_the_path(traced, golden):
    assert len(golden["cases"]) == 2 * (4 + 512) + 27 and len(set(golden["sha1"])) == len(golden["sha1"])
    assert sorted(set(golden["cases"])) == list(range(len(golden["sha1"])))
    assert all(gen.sha1(t) == golden["sha1"][int(k)] for k, t in golden["traces"].items())
    entries = {c[0] for t in golden["traces"].values() for c in t}
    assert entries == {c[0] for t in traced.values() for c in t}
    assert {"sv_rowscale", "sv_droppath_scale", "sv_mx_rows_to_cols", "sv_quant_rows_cols_mx_e4m3", "sv_layernorm_quant_fwd", "sv_layernorm_quant_mx_fwd",
            "sv_window_attention_fwd_mxq", "sv_swin_mlp_fwd_mx", "sv_swin_mlp_bwd_mx", "sv_linear_fp8_wgrad", "sv_linear_mxfp8_wgrad"} <= entries


def test_f32_math_makes_every_switch_inert(traced):
    on = " fp8=True recipe=mx bwd=True brec=mx store=mx lnmx=True dual=True"
    for tail in ("", " fused=False"):
        assert traced["c96 math=f32" + on + tail] == traced["c96 math=f32" + tail]


def test_store_mx_keeps_pairs_on_the_stage_tape():
    """what the trace cannot show: under store "mx" the merge tape and the unfused block tapes hold (bytes, scales) pairs"""
    import torch
    s = dict(gen.DEFAULTS, fp8=True, bwd=True, recipe="mx", brec="mx", store="mx")
    stage = st.SwinStage(96, 192, 7, 2, 6, [0.0, 0.0], True)
    with gen.recording():
        gen._apply(s)
        _, sctx = st.stage_forward(stage, ops.empty(196, 96, device="cpu"), 1, False, False, None, True)
    assert isinstance(sctx["merge"][1], tuple) and all(t.dtype == torch.uint8 for t in sctx["merge"][1])
    for bctx in sctx["blocks"]:
        assert len(bctx) >= 15 and all(isinstance(bctx[i], tuple) for i in (3, 5, 11, 13)) and isinstance(bctx[12], torch.Tensor)
