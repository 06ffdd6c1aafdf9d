"""MXFP8 Swin linears with the inputs stored as MX rows (set_linear_fp8(..., store="mx")) inside the Swin-T encoder and the training step."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_linear_fp8_recipe import l1_rel  # noqa: E402
from test_gpu_mxfp8_bwd_encoder import GRAD_FACTOR, LOSS_FACTOR, TAIL_FACTOR  # noqa: E402  (the project's factors: imported, not restated)

import swinvox_amd as S  # noqa: E402
from swinvox_amd import hip, ops  # noqa: E402

STORE_SITES = 43       # Swin-T with the default fusions: 4 linears in each of the 10 unfused blocks + 3 patch-merge reductions


def _counters():
    lib = hip.load()
    return np.array([int(lib.sv_mx_rows_to_cols_launches()), int(lib.sv_quant_cols_mx_launches()), *ops.linear_mxfp8_bwd_launches(),
                     ops.linear_mxfp8_launches(), int(lib.sv_quant_rows_mx_launches())])


def _step(enc, x, monkeypatch):
    """one forward + backward -> (stage feature maps, gradients by name, the counters' increase, bytes allocated right after the forward)"""
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
        torch.cuda.synchronize()
        n0 = _counters()
        out = enc(x)
        torch.cuda.synchronize()
        mem = torch.cuda.memory_allocated()
        out.float().square().mean().backward()
        torch.cuda.synchronize()
        n1 = _counters()
    finally:
        monkeypatch.setattr(enc_mod, "swin_forward", real)
    assert bool(torch.isfinite(out.float()).all()) and len(feats) == 4
    grads = {n: p.grad.detach().float().cpu() for n, p in enc.named_parameters() if p.grad is not None}
    del out
    return feats, grads, tuple(int(v) for v in n1 - n0), mem


def _set_mode(mode):
    S.set_math("f32" if mode == "f32" else "bf16")
    if mode != "f32":
        S.set_storage("bf16")
    on = mode.startswith("mx")
    S.set_linear_fp8(on, backward=on, recipe="mx", backward_recipe="mx", store="mx" if mode == "mx_store" else "bf16")


@pytest.mark.gpu
def test_swin_t_encoder_mx_store(dev, monkeypatch):
    """Swin-T, golden weights, B = 1 x V = 2, bf16 storage; runs: exact f32, bf16, MX forward + MX backward with store "bf16" and with store
    "mx", bf16 again.  Under store "mx" the re-blocker runs once per store site, the MX column quantiser exactly that many times less, and
    nothing else moves; a plain bf16 step afterwards moves no counter.  The forward feature maps are bit-identical to store "bf16", every
    gradient is finite, the 16 probed weight gradients are within GRAD_FACTOR of bf16's distance from exact f32, and the bytes allocated
    right after the forward are strictly fewer."""
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
    runs = {}
    try:
        for mode in ("f32", "bf16", "mx_bf16store", "mx_store", "bf16_again"):
            _set_mode(mode)
            assert ops.linear_fp8_store() == ("mx" if mode == "mx_store" else "bf16"), mode
            runs[mode] = _step(enc, x, monkeypatch)
            print(f"{mode}: (re-blocker, MX column quantiser, MX dgrad, MX wgrad, MX GEMMs, MX row quantiser) = {runs[mode][2]}; "
                  f"allocated after the forward {runs[mode][3]} bytes")
            assert all(bool(torch.isfinite(t).all()) for t in runs[mode][1].values()), mode
    finally:
        S.set_linear_fp8(False)
        S.set_math("f32")
    a, b = runs["mx_bf16store"][2], runs["mx_store"][2]
    assert a[0] == 0 and b[0] == STORE_SITES and b[3] == STORE_SITES, (a, b)
    assert a[1] - b[1] == STORE_SITES, (a, b)
    assert a[2:] == b[2:], (a, b)                                              # the GEMMs and the row quantisers do not move
    for mode in ("f32", "bf16", "bf16_again"):
        assert runs[mode][2] == (0,) * 6, mode
    assert all(torch.equal(u, v) for u, v in zip(runs["mx_store"][0], runs["mx_bf16store"][0]))
    assert all(torch.equal(u, v) for u, v in zip(runs["bf16"][0], runs["bf16_again"][0]))
    gstats = {}
    for mode in ("bf16", "mx_bf16store", "mx_store"):
        d = {k: l1_rel(runs[mode][1][pn], runs["f32"][1][pn]) for k, pn in probes}
        print(f"{mode}: weight gradients vs exact f32, L1-rel " + ", ".join(f"{k} {v:.3e}" for k, v in d.items()))
        v = sorted(d.values())
        gstats[mode] = (v[-1], v[len(v) // 2])
    print("worst / median: " + ", ".join(f"{k} {v[0]:.3e} / {v[1]:.3e}" for k, v in gstats.items()))
    for k in (0, 1):
        assert gstats["mx_store"][k] <= GRAD_FACTOR * gstats["bf16"][k], gstats
    assert runs["mx_store"][3] < runs["mx_bf16store"][3], (runs["mx_store"][3], runs["mx_bf16store"][3])


@pytest.mark.gpu
def test_training_smoke_mxfp8_store(dev):
    """Whole pipeline, Swin-T, B = 2 x V = 2, one fixed batch, 20 flat-Adam steps in bf16 and with the MX forward + MX backward on stored MX
    rows: the loss falls and stays finite, the final loss is within LOSS_FACTOR of the bf16 run's of the same process, the mean of the last
    five steps within TAIL_FACTOR."""
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
    for mode in ("bf16", "mx_store"):
        torch.manual_seed(0)
        nets = [Encoder(cfg), Decoder(cfg), Merger(cfg), Refiner(cfg)]
        for n in nets:
            O.seeded_weights_(n, seed=7)
            n.to(dev).train()
        solvers, _ = harness.make_solvers(nets, cfg)
        S.set_math("bf16")
        S.set_storage("bf16")
        on = mode != "bf16"
        S.set_linear_fp8(on, backward=on, recipe="mx", backward_recipe="mx", store="mx")
        r0 = ops.mx_rows_to_cols_launches()
        try:
            losses = []
            for _ in range(20):
                el, rl = harness.train_step(nets, solvers, cfg, x, gt)
                losses.append(float(el + rl))
        finally:
            S.set_linear_fp8(False)
            S.set_math("f32")
        print(f"{mode}: losses {[round(v, 4) for v in losses]}")
        assert (ops.mx_rows_to_cols_launches() - r0 > 0) == on
        assert all(np.isfinite(losses)) and losses[-1] < losses[0], (mode, losses)
        final[mode] = (losses[-1], sum(losses[-5:]) / 5)
    assert final["mx_store"][0] < LOSS_FACTOR * final["bf16"][0], final
    assert final["mx_store"][1] < TAIL_FACTOR * final["bf16"][1], final
