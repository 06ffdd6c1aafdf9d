"""The MX backward of the fp8 Swin linears inside the encoder (ops.set_linear_fp8(True, backward=True, backward_recipe="mx")): routing proved
by the two pairs of launch counters under both forward recipes, the forward untouched by the backward switch, the weight gradients bounded
as tests/test_gpu_linear_fp8_bwd.py bounds the row recipe's, and a training smoke run."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_linear_fp8_recipe import l1_rel  # noqa: E402

import swinvox_amd as S  # noqa: E402
from swinvox_amd import ops  # noqa: E402

GRAD_FACTOR = 1.25     # the project's factors (tests/test_gpu_attn_fp8_bwd.py, tests/test_gpu_linear_fp8_bwd.py)
LOSS_FACTOR = 1.5
TAIL_FACTOR = 1.15


def _counters():
    return np.array([*ops.linear_mxfp8_bwd_launches(), *ops.linear_fp8_bwd_launches(), ops.linear_mxfp8_launches(), ops.linear_fp8_launches()])


def _step(enc, x, monkeypatch):
    """one forward + backward; returns (the Swin stage feature maps, gradients by name, the counters' increase over the backward: MX (dgrad,
    wgrad), row-recipe (dgrad, wgrad), and over the forward: MX GEMMs, row-recipe GEMMs)"""
    from swinvox_amd.models import encoder as enc_mod
    feats = []
    real = enc_mod.swin_forward

    def spy(*a, **k):
        f, tape = real(*a, **k)
        feats.extend(t.float().cpu() for t in f)
        return f, tape

    monkeypatch.setattr(enc_mod, "swin_forward", spy)
    try:
        enc.zero_grad(set_to_none=True)
        n0 = _counters()
        out = enc(x)
        n1 = _counters()
        out.float().square().mean().backward()
        torch.cuda.synchronize()
        n2 = _counters()
    finally:
        monkeypatch.setattr(enc_mod, "swin_forward", real)
    assert bool(torch.isfinite(out.float()).all()) and len(feats) == 4
    assert not (n1 - n0)[:4].any() and not (n2 - n1)[4:].any()          # backward kernels run in the backward, forward kernels in the forward
    grads = {n: p.grad.detach().float().cpu() for n, p in enc.named_parameters() if p.grad is not None}
    return feats, grads, tuple(int(v) for v in (n2 - n1)[:4]) + tuple(int(v) for v in (n1 - n0)[4:])


def _set_mode(mode):
    """f32 | bf16[...] | <forward recipe>_<nobwd | rowbwd | mxbwd>[_unfused]"""
    S.set_math("f32" if mode == "f32" else "bf16")
    if mode != "f32":
        S.set_storage("bf16")
    fp8 = mode.startswith(("row_", "mx_"))
    kw = dict(backward_recipe="mx") if "_mxbwd" in mode else {}          # "rowbwd": backward=True WITHOUT the new argument
    S.set_linear_fp8(fp8, backward=fp8 and "_nobwd" not in mode, recipe="mx" if mode.startswith("mx_") else "row", **kw)
    unfused = mode.endswith("unfused")
    ops.set_fused_attn_block(not unfused)
    ops.set_fused_attn_block_bwd(not unfused)
    ops.set_fused_mlp(not unfused)


def _reset_modes():
    S.set_linear_fp8(False)
    ops.set_fused_attn_block(True)
    ops.set_fused_attn_block_bwd(True)
    ops.set_fused_mlp(True)
    S.set_math("f32")


def _same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.gpu
def test_swin_t_encoder_mx_backward(dev, monkeypatch):
    """Swin-T, golden weights, B = 1 x V = 2, bf16 storage.  Under both forward recipes: backward_recipe="mx" gives (43, 43) MX and (0, 0)
    row-recipe backward launches with the default fusions and (51, 51) / (0, 0) with both stage-0 fusions off; backward=True without the
    argument gives MX (0, 0) and row (43, 43); a bf16 step afterwards moves neither.  Every gradient is finite.  The forward does not know
    about the backward switch: the stage feature maps are bit-identical to the same forward recipe without it.  The qkv / proj / fc1 / fc2
    weight gradients of every stage's first block, as L1-relative distance from the exact-f32 run: worst and median within GRAD_FACTOR of
    the bf16 run's (bf16 storage alone moves these gradients by about their own size - tests/test_gpu_linear_fp8_bwd.py)."""
    from swinvox_amd import goldens
    from swinvox_amd.models import Encoder
    enc = Encoder(S.default_cfg())
    goldens.seeded_fill_(enc, 100)
    enc.to(dev).train()
    enc.stochastic = False
    x = goldens.synth_images(1, 2, 11).to(dev)
    names = {id(p): n for n, p in enc.named_parameters()}
    probes = [(f"stage {i} {k}", names[id(w)]) for i, st in enumerate(enc.swin_transformer.model.stages())
              for k, w in (("qkv", st.blocks[0].attn.qkv.weight), ("proj", st.blocks[0].attn.proj.weight), ("fc1", st.blocks[0].mlp.fc1.weight),
                           ("fc2", st.blocks[0].mlp.fc2.weight))]
    modes = ["f32", "bf16"] + [f"{fwd}_{m}" for fwd in ("row", "mx") for m in ("nobwd", "rowbwd", "mxbwd", "nobwd_unfused", "mxbwd_unfused")] + ["bf16_again"]
    runs = {}
    try:
        for mode in modes:
            _set_mode(mode)
            assert ops.linear_fp8_bwd_recipe() == ("mx" if "_mxbwd" in mode else "row"), mode
            feats, grads, cnt = _step(enc, x, monkeypatch)
            print(f"{mode}: backward launches MX {cnt[:2]}, row recipe {cnt[2:4]}; forward GEMMs MX {cnt[4]}, row recipe {cnt[5]}")
            assert all(bool(torch.isfinite(t).all()) for t in grads.values()), mode
            runs[mode] = (feats, grads, cnt)
    finally:
        _reset_modes()
    for fwd in ("row", "mx"):
        gemms = (43, 0) if fwd == "mx" else (0, 43)
        gemms_u = (51, 0) if fwd == "mx" else (0, 51)
        assert runs[f"{fwd}_nobwd"][2] == (0, 0, 0, 0) + gemms, fwd
        assert runs[f"{fwd}_rowbwd"][2] == (0, 0, 43, 43) + gemms, fwd                      # without the argument: the row-recipe backward
        assert runs[f"{fwd}_mxbwd"][2] == (43, 43, 0, 0) + gemms, fwd
        assert runs[f"{fwd}_nobwd_unfused"][2] == (0, 0, 0, 0) + gemms_u, fwd
        assert runs[f"{fwd}_mxbwd_unfused"][2] == (51, 51, 0, 0) + gemms_u, fwd
        for m in ("rowbwd", "mxbwd"):
            assert _same(runs[f"{fwd}_{m}"][0], runs[f"{fwd}_nobwd"][0]), (fwd, m)          # the forward is untouched by the backward switch
        assert _same(runs[f"{fwd}_mxbwd_unfused"][0], runs[f"{fwd}_nobwd_unfused"][0]), fwd
    for mode in ("f32", "bf16", "bf16_again"):
        assert runs[mode][2] == (0,) * 6, mode
    assert _same(runs["bf16"][0], runs["bf16_again"][0])
    n = probes[4][1]       # stage 1 qkv: unfused in every mode
    for fwd in ("row", "mx"):                                                               # the three backwards differ
        g = [runs[f"{fwd}_{m}"][1][n] for m in ("nobwd", "rowbwd", "mxbwd")]
        assert not torch.equal(g[0], g[1]) and not torch.equal(g[1], g[2]) and not torch.equal(g[0], g[2]), fwd
    gstats = {}
    for mode in ["bf16"] + [f"{fwd}_{m}" for fwd in ("row", "mx") for m in ("rowbwd", "mxbwd", "mxbwd_unfused")]:
        d = {k: l1_rel(runs[mode][1][pn], runs["f32"][1][pn]) for k, pn in probes}
        print(f"{mode}: weight gradients vs exact f32, L1-rel " + ", ".join(f"{k} {v:.3e}" for k, v in d.items()))
        v = sorted(d.values())
        gstats[mode] = (v[-1], v[len(v) // 2])
    print("worst / median: " + ", ".join(f"{k} {v[0]:.3e} / {v[1]:.3e}" for k, v in gstats.items()))
    for fwd in ("row", "mx"):
        for m in ("mxbwd", "mxbwd_unfused"):
            for k in (0, 1):
                assert gstats[f"{fwd}_{m}"][k] <= GRAD_FACTOR * gstats["bf16"][k], (fwd, m, gstats)


@pytest.mark.gpu
def test_training_smoke_mxfp8_linear_backward(dev):
    """Whole pipeline, Swin-T, B = 2 x V = 2, one fixed batch, 20 flat-Adam steps in bf16 and with the fp8 linears on the MX backward (under
    the MX forward, the consistent operand format): the loss falls and stays finite, the final loss is within LOSS_FACTOR of the bf16 run's
    of the same process, the mean of the last five steps within TAIL_FACTOR."""
    import oracle as O
    from swinvox_amd import harness
    from swinvox_amd.models import Decoder, Encoder, Merger, Refiner
    cfg = S.default_cfg()
    cfg.TRAIN.ENCODER_LEARNING_RATE = cfg.TRAIN.DECODER_LEARNING_RATE = 1e-3
    cfg.TRAIN.REFINER_LEARNING_RATE = cfg.TRAIN.MERGER_LEARNING_RATE = 1e-3
    g = torch.Generator().manual_seed(3)
    x = (0.5 * torch.randn(2, 2, 3, 224, 224, generator=g)).to(dev)
    gt = (torch.rand(2, 32, 32, 32, generator=g) < 0.1).float().to(dev)
    final = {}
    for mode in ("bf16", "mx_bwd"):
        torch.manual_seed(0)
        nets = [Encoder(cfg), Decoder(cfg), Merger(cfg), Refiner(cfg)]
        for n in nets:
            O.seeded_weights_(n, seed=7)
            n.to(dev).train()
        solvers, _ = harness.make_solvers(nets, cfg)
        S.set_math("bf16")
        S.set_storage("bf16")
        on = mode != "bf16"
        S.set_linear_fp8(on, backward=on, recipe="mx", backward_recipe="mx")
        b0, r0 = ops.linear_mxfp8_bwd_launches(), ops.linear_fp8_bwd_launches()
        try:
            losses = []
            for _ in range(20):
                el, rl = harness.train_step(nets, solvers, cfg, x, gt)
                losses.append(float(el + rl))
        finally:
            S.set_linear_fp8(False)
            S.set_math("f32")
        b1 = ops.linear_mxfp8_bwd_launches()
        print(f"{mode}: losses {[round(v, 4) for v in losses]}")
        assert (b1[0] - b0[0] > 0) == (b1[1] - b0[1] > 0) == on and ops.linear_fp8_bwd_launches() == r0
        assert all(np.isfinite(losses)) and losses[-1] < losses[0], (mode, losses)
        final[mode] = (losses[-1], sum(losses[-5:]) / 5)
    assert final["mx_bwd"][0] < LOSS_FACTOR * final["bf16"][0], final
    assert final["mx_bwd"][1] < TAIL_FACTOR * final["bf16"][1], final
