"""The MX recipe of the fp8 Swin linears inside the encoder (ops.set_linear_fp8(True, recipe="mx")): routing proved by the launch counters,
producer emission (fc1 -> fc2, window attention -> proj) against the stand-alone quantiser bit for bit, nothing lingering for the row recipe
and the bf16 path, the fp8 backward on top, Swin-B with every fp8 switch, and a training smoke run."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_linear_fp8_recipe import l1_rel  # noqa: E402

import swinvox_amd as S  # noqa: E402
from swinvox_amd import hip, ops  # noqa: E402


def _counters():
    return np.array([ops.linear_mxfp8_launches(), ops.linear_fp8_launches(), ops.mx_act_quant_launches(), ops.layernorm_quant_launches(),
                     *ops.linear_fp8_bwd_launches()])


def _forward(enc, x, monkeypatch, backward=True):
    """one forward (+ backward); returns (the Swin stage feature maps, gradients or None, the counters' increase over the forward: MX GEMMs,
    row-recipe GEMMs, stand-alone MX activation quantisers, quantising LayerNorms, and over the backward: fp8 dgrad, wgrad)"""
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
        if backward:
            out = enc(x)
            n1 = _counters()
            out.float().square().mean().backward()
        else:
            with torch.no_grad():
                out = enc(x)
            n1 = _counters()
        torch.cuda.synchronize()
        n2 = _counters()
    finally:
        monkeypatch.setattr(enc_mod, "swin_forward", real)
    assert bool(torch.isfinite(out.float()).all()) and len(feats) == 4
    grads = {n: p.grad.detach().float().cpu() for n, p in enc.named_parameters() if p.grad is not None} if backward else None
    return feats, grads, tuple(int(v) for v in (n1 - n0)[:4]) + tuple(int(v) for v in (n2 - n1)[4:])


def _same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.gpu
def test_swin_t_encoder_mx_routing_and_emission(dev, monkeypatch):
    """Swin-T, B = 1 x V = 2, bf16 storage.  Launch counts per forward (MX GEMMs, row-recipe GEMMs, stand-alone activation quantisers):
    default fusions 43 / 0 / 23 with producer emission and 43 with it off; both stage-0 fusions off 51 / 0 / 27 and 51.  The stage feature maps
    are bit-identical with emission on and off, in a training forward and under no_grad (where neither h / hpre nor att is stored); a row-recipe
    run and a bf16 run after the MX runs reproduce the ones before; the distance from exact f32 is printed and bounded by 0.5."""
    from swinvox_amd import goldens
    from swinvox_amd.models import Encoder
    enc = Encoder(S.default_cfg())
    goldens.seeded_fill_(enc, 100)
    enc.to(dev).train()
    enc.stochastic = False
    x = goldens.synth_images(1, 2, 11).to(dev)
    runs = {}
    modes = ["f32", "bf16", "row", "mx", "mx_noemit", "mx_unfused", "mx_unfused_noemit", "row_again", "bf16_again"]
    try:
        for mode in modes:
            S.set_math("f32" if mode == "f32" else "bf16")
            if mode != "f32":
                S.set_storage("bf16")
            S.set_linear_fp8(mode.startswith(("row", "mx")), recipe="mx" if mode.startswith("mx") else "row")
            ops.set_mx_producer_quant("noemit" not in mode)
            ops.set_fused_attn_block("unfused" not in mode)
            ops.set_fused_mlp("unfused" not in mode)
            feats, grads, cnt = _forward(enc, x, monkeypatch)
            print(f"{mode}: MX GEMMs {cnt[0]}, row-recipe GEMMs {cnt[1]}, MX activation quantisers {cnt[2]}, quantising LayerNorms {cnt[3]}, "
                  f"fp8 backward {cnt[4:]}")
            assert all(bool(torch.isfinite(t).all()) for t in grads.values()), mode
            runs[mode] = (feats, cnt)
            if mode.startswith("mx"):
                feats_ng, _, cnt_ng = _forward(enc, x, monkeypatch, backward=False)
                assert cnt_ng[:4] == cnt[:4], (mode, cnt_ng)
                runs[mode + "/no_grad"] = (feats_ng, cnt_ng)
    finally:
        S.set_linear_fp8(False)
        ops.set_mx_producer_quant(True)
        ops.set_fused_attn_block(True)
        ops.set_fused_mlp(True)
        S.set_math("f32")
    assert runs["mx"][1] == (43, 0, 23, 0, 0, 0) and runs["mx_noemit"][1] == (43, 0, 43, 0, 0, 0)
    assert runs["mx_unfused"][1] == (51, 0, 27, 0, 0, 0) and runs["mx_unfused_noemit"][1] == (51, 0, 51, 0, 0, 0)
    assert runs["row"][1][:3] == (0, 43, 0) and runs["bf16"][1] == (0, 0, 0, 0, 0, 0) and runs["f32"][1] == (0, 0, 0, 0, 0, 0)
    for a in ("mx", "mx_unfused"):
        assert _same(runs[a][0], runs[a + "_noemit"][0]), a                                    # emission = the stand-alone quantiser
        assert _same(runs[a + "/no_grad"][0], runs[a + "_noemit/no_grad"][0]), a
        assert _same(runs[a][0], runs[a + "/no_grad"][0]), a                                   # and what is stored does not change the result
    assert _same(runs["row"][0], runs["row_again"][0]) and runs["row"][1] == runs["row_again"][1]
    assert _same(runs["bf16"][0], runs["bf16_again"][0])
    assert not _same(runs["mx"][0], runs["row"][0]) and not _same(runs["mx"][0], runs["bf16"][0])
    assert not torch.equal(runs["mx"][0][0], runs["mx_unfused"][0][0])                         # stage 0 runs on MX linears only when unfused
    for mode in ("bf16", "row", "mx", "mx_unfused"):
        d = [l1_rel(a, b) for a, b in zip(runs[mode][0], runs["f32"][0])]
        print(f"{mode}: stage feature maps vs exact f32, L1-rel {[f'{v:.3e}' for v in d]}")
        assert max(d) <= 0.5, (mode, d)


@pytest.mark.gpu
def test_swin_t_encoder_mx_with_fp8_backward(dev, monkeypatch):
    """backward=True keeps its meaning under the MX recipe: 43 MX GEMMs in the forward, (43, 43) fp8 data / weight gradient launches in the
    backward, every gradient finite."""
    from swinvox_amd import goldens
    from swinvox_amd.models import Encoder
    enc = Encoder(S.default_cfg())
    goldens.seeded_fill_(enc, 100)
    enc.to(dev).train()
    enc.stochastic = False
    x = goldens.synth_images(1, 2, 11).to(dev)
    try:
        S.set_math("bf16")
        S.set_storage("bf16")
        S.set_linear_fp8(True, backward=True, recipe="mx")
        _, grads, cnt = _forward(enc, x, monkeypatch)
    finally:
        S.set_linear_fp8(False)
        S.set_math("f32")
    print(f"MX + fp8 backward: {cnt}")
    assert cnt == (43, 0, 23, 0, 43, 43), cnt
    assert grads and all(bool(torch.isfinite(t).all()) for t in grads.values())


@pytest.mark.gpu
def test_swin_b_encoder_every_fp8_switch(dev, monkeypatch):
    """Swin-B, fp8 attention (forward and backward), MX linears and their fp8 backward, B = 1 x V = 1: K = 128 ... 4096, the fp8 attention core
    as the emitting producer.  4 per block + 3 patch merges - 2 per block on the fused MLP (C = 128) = 95 MX GEMMs; everything finite."""
    from swinvox_amd import goldens
    from swinvox_amd.models import Encoder
    enc = Encoder(S.default_cfg(), variant="base")
    goldens.seeded_fill_(enc, 100)
    enc.to(dev).train()
    enc.stochastic = False
    x = goldens.synth_images(1, 1, 12).to(dev)
    try:
        S.set_math("bf16")
        S.set_storage("bf16")
        S.set_attention_fp8(True, backward=True)
        S.set_linear_fp8(True, backward=True, recipe="mx")
        feats, grads, cnt = _forward(enc, x, monkeypatch)
    finally:
        S.set_linear_fp8(False)
        S.set_attention_fp8(False)
        S.set_math("f32")
    print(f"Swin-B: {cnt}")
    assert cnt[0] == 95 and cnt[1] == 0, cnt
    assert all(bool(torch.isfinite(t).all()) for t in feats) and all(bool(torch.isfinite(t).all()) for t in grads.values())


LOSS_FACTOR = 1.5      # the project's factors (tests/test_gpu_attn_fp8_bwd.py, tests/test_gpu_linear_fp8.py)
TAIL_FACTOR = 1.15


@pytest.mark.gpu
def test_training_smoke_mxfp8_linear(dev):
    """Whole pipeline, Swin-T, B = 2 x V = 2, one fixed batch, 20 flat-Adam steps in bf16 and with the MX linears, as
    test_training_smoke_fp8_linear does it: the loss falls and stays finite, the final loss is within LOSS_FACTOR of the bf16 run's of the
    same process, the mean of the last five steps within TAIL_FACTOR."""
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
    for mode in ("bf16", "mx"):
        torch.manual_seed(0)
        nets = [Encoder(cfg), Decoder(cfg), Merger(cfg), Refiner(cfg)]
        for n in nets:
            O.seeded_weights_(n, seed=7)
            n.to(dev).train()
        solvers, _ = harness.make_solvers(nets, cfg)
        S.set_math("bf16")
        S.set_storage("bf16")
        S.set_linear_fp8(mode == "mx", recipe="mx")
        n0 = ops.linear_mxfp8_launches(), ops.linear_fp8_launches()
        try:
            losses = []
            for _ in range(20):
                el, rl = harness.train_step(nets, solvers, cfg, x, gt)
                losses.append(float(el + rl))
        finally:
            S.set_linear_fp8(False)
            S.set_math("f32")
        print(f"{mode}: losses {[round(v, 4) for v in losses]}")
        assert (ops.linear_mxfp8_launches() - n0[0] > 0) == (mode == "mx") and ops.linear_fp8_launches() == n0[1]
        assert all(np.isfinite(losses)) and losses[-1] < losses[0], (mode, losses)
        final[mode] = (losses[-1], sum(losses[-5:]) / 5)
    assert final["mx"][0] < LOSS_FACTOR * final["bf16"][0], final
    assert final["mx"][1] < TAIL_FACTOR * final["bf16"][1], final
