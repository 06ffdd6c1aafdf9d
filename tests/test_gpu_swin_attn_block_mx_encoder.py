"""The MXFP8 forward of the fused attention branch inside the Swin-T encoder (ops.set_fused_attn_block_mx under set_linear_fp8(True, recipe="mx"),
together with set_fused_mlp_mx): two launches of the new kernel per forward (the two stage-0 blocks), the MX GEMM and quantiser counts of the
default "mx" run, and a stage-0 feature map that is the all-unfused MX run's, not the default run's with its bf16 stage 0."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_linear_fp8_recipe import l1_rel  # noqa: E402
from test_gpu_mxfp8_encoder import _forward  # noqa: E402

import swinvox_amd as S  # noqa: E402
from swinvox_amd import ops  # noqa: E402


@pytest.mark.gpu
def test_swin_t_encoder_with_both_stage0_branches_on_mx(dev, monkeypatch):
    from swinvox_amd import goldens
    from swinvox_amd.models import Encoder
    enc = Encoder(S.default_cfg())
    goldens.seeded_fill_(enc, 100)
    enc.to(dev).train()
    enc.stochastic = False
    x = goldens.synth_images(1, 2, 11).to(dev)
    runs = {}
    try:
        for mode in ("f32", "mx", "mx_unfused", "mx_fused_mx"):
            S.set_math("f32" if mode == "f32" else "bf16")
            if mode != "f32":
                S.set_storage("bf16")
            S.set_linear_fp8(mode != "f32", recipe="mx")
            ops.set_fused_attn_block(mode != "mx_unfused")
            ops.set_fused_mlp(mode != "mx_unfused")
            ops.set_fused_attn_block_mx(mode == "mx_fused_mx")
            ops.set_fused_mlp_mx(mode == "mx_fused_mx")
            n0 = ops.swin_attn_block_mx_launches()
            feats, grads, cnt = _forward(enc, x, monkeypatch)
            new = ops.swin_attn_block_mx_launches() - n0
            print(f"{mode}: new-kernel launches {new}, MX GEMMs {cnt[0]}, MX activation quantisers {cnt[2]}")
            assert all(bool(torch.isfinite(t).all()) for t in feats) and all(bool(torch.isfinite(t).all()) for t in grads.values()), mode
            runs[mode] = (feats, cnt, new)
    finally:
        ops.set_fused_attn_block_mx(False)
        ops.set_fused_mlp_mx(False)
        ops.set_fused_attn_block(True)
        ops.set_fused_mlp(True)
        S.set_linear_fp8(False)
        S.set_math("f32")
    assert runs["mx_fused_mx"][2] == 2 and runs["mx"][2] == runs["mx_unfused"][2] == runs["f32"][2] == 0
    assert runs["mx"][1][:3] == (43, 0, 23) and runs["mx_fused_mx"][1][:3] == (43, 0, 23), (runs["mx"][1], runs["mx_fused_mx"][1])
    ref = runs["mx_unfused"][0][0]
    d_new, d_default = l1_rel(runs["mx_fused_mx"][0][0], ref), l1_rel(runs["mx"][0][0], ref)
    print(f"stage-0 feature map vs the all-unfused MX run: both fused MX kernels {d_new:.3e}, default mx (bf16 stage 0) {d_default:.3e} "
          f"({d_default / max(d_new, 1e-30):.1f} x)")
    assert 3.0 * d_new <= d_default, (d_new, d_default)
    d = [l1_rel(a, b) for a, b in zip(runs["mx_fused_mx"][0], runs["f32"][0])]
    print(f"mx_fused_mx: stage feature maps vs exact f32, L1-rel {[f'{v:.3e}' for v in d]}")
    assert max(d[1:]) <= 0.5, d
