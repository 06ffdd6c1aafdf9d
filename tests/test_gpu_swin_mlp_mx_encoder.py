"""The MXFP8 forward of the fused Swin MLP inside the Swin-T encoder (ops.set_fused_mlp_mx under set_linear_fp8(True, recipe="mx")): golden
network of tests/golden/case_B1_V2.npz (swinvox_amd.goldens.golden_case), B 1 x V 2, bf16 math and storage.  The features with the switch on
obey the project's fp8 rule (tests/test_gpu_configs.py) against the all-MX unfused chain (set_fused_mlp(False)): e_on <= 1.25 e_off + 1e-2
mean|gold|, e being the mean |feature - golden|; one training step leaves finite features and gradients."""
import json
import os

import numpy as np
import pytest
import torch

import swinvox_amd as S
from swinvox_amd import ops


@pytest.mark.gpu
def test_swin_t_encoder_features_and_one_train_step(dev):
    from swinvox_amd import goldens
    gdir = os.path.join(os.path.dirname(__file__), "golden")
    seed = json.load(open(os.path.join(gdir, "manifest.json")))["cases"]["B1_V2"]["seed"]
    gold = torch.from_numpy(np.load(os.path.join(gdir, "case_B1_V2.npz"))["features"])
    S.set_math("f32")
    nets, x, _ = goldens.golden_case(dev, 1, 2, seed)
    enc = nets[0]
    try:
        S.set_math("bf16")
        S.set_storage("bf16")
        S.set_linear_fp8(True, recipe="mx")
        with torch.no_grad():
            f_default = enc(x).float().cpu()                     # stage 0: fused bf16 MLP (the default under MX linears)
            ops.set_fused_mlp(False)
            n0 = ops.swin_mlp_mx_launches()
            f_off = enc(x).float().cpu()                         # the all-MX unfused chain
            assert ops.swin_mlp_mx_launches() == n0
            ops.set_fused_mlp(True)
            ops.set_fused_mlp_mx(True)
            f_on = enc(x).float().cpu()
            assert ops.swin_mlp_mx_launches() == n0 + 2          # the two stage-0 blocks
        enc.train()
        enc.stochastic = False
        enc.zero_grad(set_to_none=True)
        out = enc(x)
        out.float().square().mean().backward()
        torch.cuda.synchronize()
        assert ops.swin_mlp_mx_launches() == n0 + 4
        grads = [p.grad for p in enc.parameters() if p.grad is not None]
        grads_ok = len(grads) > 100 and all(bool(torch.isfinite(g).all()) for g in grads)
        train_ok = bool(torch.isfinite(out.float()).all())
    finally:
        ops.set_fused_mlp_mx(False)
        ops.set_fused_mlp(True)
        S.set_linear_fp8(False)
        S.set_math("f32")
    gm = float(gold.abs().mean())
    e_on, e_off, e_def = (float((f - gold).abs().mean()) for f in (f_on, f_off, f_default))
    print(f"Swin-T encoder vs golden: mean|d| fused MX MLP {e_on:.4e}, unfused MX chain {e_off:.4e}, fused bf16 MLP under MX linears {e_def:.4e}, "
          f"mean|gold| {gm:.4e}")
    assert bool(torch.isfinite(f_on).all()) and train_ok and grads_ok
    assert float((f_on - f_default).abs().max()) > 0.0           # the MX kernel really ran
    assert e_on <= 1.25 * e_off + 1e-2 * gm, (e_on, e_off, gm)
