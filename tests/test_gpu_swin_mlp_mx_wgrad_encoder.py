"""The MXFP8 weight gradients of the fused Swin MLP inside the Swin-T encoder (ops.set_fused_mlp_mx(True, backward=True, wgrad=True) under
set_linear_fp8(True, backward=True, recipe="mx", backward_recipe="mx")): one training step at B 1 x V 2 in bf16 math and storage with all three
fused-MLP MX switches on.  The launch counter advances by the number of stage-0 blocks, every gradient is finite, and the gradients meet the bounds
tests/test_gpu_mxfp8_bwd_encoder.py holds the unfused MX backward to: as L1-relative distance from the exact-f32 run, worst and median of the
probed weight gradients, and the input gradient, within GRAD_FACTOR of the bf16 run's."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_linear_fp8_recipe import l1_rel  # noqa: E402

import swinvox_amd as S  # noqa: E402
from swinvox_amd import hip, ops  # noqa: E402

GRAD_FACTOR = 1.25     # tests/test_gpu_mxfp8_bwd_encoder.py


def _step(enc, x):
    enc.zero_grad(set_to_none=True)
    xin = x.clone().requires_grad_(True)
    n0 = ops.swin_mlp_mx_wgrad_launches(), ops.swin_mlp_mx_bwd_launches(), ops.swin_mlp_mx_launches()
    out = enc(xin)
    out.float().square().mean().backward()
    torch.cuda.synchronize()
    n = tuple(b - a for a, b in zip(n0, (ops.swin_mlp_mx_wgrad_launches(), ops.swin_mlp_mx_bwd_launches(), ops.swin_mlp_mx_launches())))
    assert bool(torch.isfinite(out.float()).all())
    grads = {k: p.grad.detach().float().cpu() for k, p in enc.named_parameters() if p.grad is not None}
    assert len(grads) > 100 and all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert xin.grad is not None and bool(torch.isfinite(xin.grad).all())
    return grads, xin.grad.detach().float().cpu(), n


@pytest.mark.gpu
def test_swin_t_encoder_training_step(dev):
    from swinvox_amd import goldens
    from swinvox_amd.models import Encoder
    enc = Encoder(S.default_cfg())
    goldens.seeded_fill_(enc, 100)
    enc.to(dev).train()
    enc.stochastic = False
    x = goldens.synth_images(1, 2, 11).to(dev)
    stages = list(enc.swin_transformer.model.stages())
    nblk0 = len(stages[0].blocks)
    served = hip.load().sv_swin_mlp_wgrad_mx_supported(stages[0].blocks[0].dim) == 1
    names = {id(p): n for n, p in enc.named_parameters()}
    probes = [(f"stage {i} {k}", names[id(w)]) for i, st in enumerate(stages)
              for k, w in (("qkv", st.blocks[0].attn.qkv.weight), ("proj", st.blocks[0].attn.proj.weight), ("fc1", st.blocks[0].mlp.fc1.weight),
                           ("fc2", st.blocks[0].mlp.fc2.weight), ("norm2", st.blocks[0].norm2.weight))]
    runs = {}
    try:
        for mode in ("f32", "bf16", "mx_fused_bwd", "mx_fused_all"):
            S.set_math("f32" if mode == "f32" else "bf16")
            if mode != "f32":
                S.set_storage("bf16")
            on = mode.startswith("mx")
            S.set_linear_fp8(on, backward=on, recipe="mx", backward_recipe="mx")
            ops.set_fused_mlp_mx(on, backward=on, wgrad=mode == "mx_fused_all")
            runs[mode] = _step(enc, x)
    finally:
        ops.set_fused_mlp_mx(False)
        S.set_linear_fp8(False)
        S.set_math("f32")
    assert nblk0 == 2
    assert runs["f32"][2] == (0, 0, 0) and runs["bf16"][2] == (0, 0, 0)
    assert runs["mx_fused_bwd"][2][0] == 0 and runs["mx_fused_bwd"][2][2] == nblk0       # the parent's mode: weight gradients on sv_swin_mlp_wgrad
    assert runs["mx_fused_all"][2][0] == (nblk0 if served else 0), runs["mx_fused_all"][2]   # one sv_swin_mlp_wgrad_mx launch per stage-0 block
    assert runs["mx_fused_all"][2][1:] == runs["mx_fused_bwd"][2][1:]
    stats = {}
    for mode in ("bf16", "mx_fused_bwd", "mx_fused_all"):
        d = {k: l1_rel(runs[mode][0][pn], runs["f32"][0][pn]) for k, pn in probes}
        dx = l1_rel(runs[mode][1], runs["f32"][1])
        print(f"{mode}: gradients vs exact f32, L1-rel input {dx:.3e}, " + ", ".join(f"{k} {v:.3e}" for k, v in d.items()))
        v = sorted(d.values())
        stats[mode] = (v[-1], v[len(v) // 2], dx)
    print("worst / median / input: " + ", ".join(f"{k} {v[0]:.3e} / {v[1]:.3e} / {v[2]:.3e}" for k, v in stats.items()))
    for k in (0, 1, 2):
        assert stats["mx_fused_all"][k] <= GRAD_FACTOR * stats["bf16"][k], (k, stats)
    if served:
        g_on, g_off = runs["mx_fused_all"][0], runs["mx_fused_bwd"][0]
        f1 = names[id(stages[0].blocks[0].mlp.fc1.weight)]
        assert not torch.equal(g_on[f1], g_off[f1])                              # the MX weight gradients really ran
