"""The quantising LayerNorm inside the Swin encoder (ops.set_ln_quant_fused, models/swin_transformer.py _norm_for_linear): the launch counter
proves which sites take it, and the stage feature maps with the fused quantiser equal those of LayerNorm + stand-alone quantiser bit for
bit - in a training forward and in a torch.no_grad() forward, where the fused form stores neither the rows nor the statistics.

Fixture of tests/test_gpu_linear_fp8.py (restated: that file's helpers are bound to its own step function): Swin-T Encoder with the
golden recipe's encoder weights (goldens.seeded_fill_(enc, 100), the network behind tests/golden/case_B1_V2.npz), B 1 x V 2 synthetic
renderings, bf16 math and storage."""
import pytest
import torch

import swinvox_amd as S
from swinvox_amd import ops


@pytest.fixture
def switches():
    """every switch these tests touch is restored afterwards"""
    try:
        yield
    finally:
        S.set_linear_fp8(False)
        S.set_attention_fp8(False)
        ops.set_ln_quant_fused(True)
        ops.set_fused_attn_block(True)
        ops.set_fused_attn_block_bwd(True)
        ops.set_fused_mlp(True)
        S.set_math("f32")


def _encoder(dev, variant="tiny"):
    from swinvox_amd import goldens
    from swinvox_amd.models import Encoder
    enc = Encoder(S.default_cfg(), variant=variant)
    goldens.seeded_fill_(enc, 100)
    enc.to(dev).train()
    enc.stochastic = False
    return enc


def _forward(enc, x, monkeypatch, grad=True):
    """one forward; returns (output, the Swin stage feature maps as stored, movement of the (quantising LayerNorm, fp8 linear) counters)"""
    from swinvox_amd.models import encoder as enc_mod
    feats = []
    real = enc_mod.swin_forward

    def spy(*a, **k):
        f, tape = real(*a, **k)
        feats.extend(t.detach().clone() for t in f)
        return f, tape

    monkeypatch.setattr(enc_mod, "swin_forward", spy)
    n0, l0 = ops.layernorm_quant_launches(), ops.linear_fp8_launches()
    try:
        if grad:
            out = enc(x)
        else:
            with torch.no_grad():
                out = enc(x)
        torch.cuda.synchronize()
    finally:
        monkeypatch.setattr(enc_mod, "swin_forward", real)
    return out, [f.cpu() for f in feats], (ops.layernorm_quant_launches() - n0, ops.linear_fp8_launches() - l0)


def _same(a, b):
    return len(a) == len(b) == 4 and all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.gpu
def test_swin_t_routing_and_bit_equality(dev, monkeypatch, switches):
    from swinvox_amd import goldens
    enc = _encoder(dev)
    x = goldens.synth_images(1, 2, 11).to(dev)
    S.set_math("bf16")
    S.set_storage("bf16")
    # bf16 run before anything fp8
    _, f_bf16, n = _forward(enc, x, monkeypatch)
    assert n == (0, 0)

    S.set_linear_fp8(True)
    # default fusions: stage 0 (2 blocks) runs the fused attention branch and the fused MLP -> 10 unfused blocks x 2 + 3 patch merges
    _, f_on, n = _forward(enc, x, monkeypatch)
    assert n == (23, 43), n
    ops.set_ln_quant_fused(False)
    _, f_off, n = _forward(enc, x, monkeypatch)
    assert n == (0, 43), n
    assert _same(f_on, f_off)
    assert not _same(f_on, f_bf16)                               # the fp8 linears did run
    # torch.no_grad(): no backward follows, the fused sites store only the e4m3 rows and scales
    ops.set_ln_quant_fused(True)
    _, f_on_ng, n = _forward(enc, x, monkeypatch, grad=False)
    assert n == (23, 43), n
    ops.set_ln_quant_fused(False)
    _, f_off_ng, n = _forward(enc, x, monkeypatch, grad=False)
    assert n == (0, 43), n
    assert _same(f_on_ng, f_off_ng)

    # both stage-0 fusions off: 12 blocks x 2 + 3
    ops.set_fused_attn_block(False)
    ops.set_fused_mlp(False)
    ops.set_ln_quant_fused(True)
    _, f_on_u, n = _forward(enc, x, monkeypatch)
    assert n == (27, 51), n
    _, f_on_u_ng, n = _forward(enc, x, monkeypatch, grad=False)
    assert n == (27, 51), n
    ops.set_ln_quant_fused(False)
    _, f_off_u, n = _forward(enc, x, monkeypatch)
    assert n == (0, 51), n
    _, f_off_u_ng, n = _forward(enc, x, monkeypatch, grad=False)
    assert _same(f_on_u, f_off_u) and _same(f_on_u_ng, f_off_u_ng)
    ops.set_fused_attn_block(True)
    ops.set_fused_mlp(True)
    ops.set_ln_quant_fused(True)

    # the fused quantiser is effective only while the fp8 linears are
    S.set_linear_fp8(False)
    _, f_bf16_again, n = _forward(enc, x, monkeypatch)
    assert n == (0, 0), n
    assert _same(f_bf16, f_bf16_again)                           # a bf16 run after all of this = the bf16 run before it, bit for bit
    S.set_linear_fp8(True)
    S.set_math("f32")                                            # inert under f32 math
    _, _, n = _forward(enc, x, monkeypatch)
    assert n == (0, 0), n


def test_switch_semantics(monkeypatch, switches):
    """on by default, effective only while the fp8 linears are; SV_LN_QUANT_FUSED=0 and set_ln_quant_fused(False) switch it off (no GPU needed)"""
    S.set_math("bf16")
    S.set_linear_fp8(True)
    assert ops.ln_quant_fused_enabled()
    monkeypatch.setenv("SV_LN_QUANT_FUSED", "0")
    assert not ops.ln_quant_fused_enabled()
    monkeypatch.delenv("SV_LN_QUANT_FUSED")
    ops.set_ln_quant_fused(False)
    assert not ops.ln_quant_fused_enabled()
    ops.set_ln_quant_fused(True)
    S.set_linear_fp8(False)
    assert not ops.ln_quant_fused_enabled()


@pytest.mark.gpu
def test_swin_t_backward_with_fused_quantiser(dev, monkeypatch, switches):
    """fp8 forward and backward of the linears with the fused quantiser on: the backward reads the stored ln1 / ln2 / lnm, which the fused
    kernel writes as before.  Gradients are finite and the (dgrad, wgrad) counters move as they do today; no bit comparison (the weight
    gradients use fp32 atomics)."""
    from swinvox_amd import goldens
    enc = _encoder(dev)
    x = goldens.synth_images(1, 2, 11).to(dev)
    S.set_math("bf16")
    S.set_storage("bf16")
    S.set_linear_fp8(True, backward=True)
    enc.zero_grad(set_to_none=True)
    out, _, n = _forward(enc, x, monkeypatch)
    assert n == (23, 43), n
    b0, q0 = ops.linear_fp8_bwd_launches(), ops.layernorm_quant_launches()
    out.float().square().mean().backward()
    torch.cuda.synchronize()
    b1 = ops.linear_fp8_bwd_launches()
    assert (b1[0] - b0[0], b1[1] - b0[1]) == (43, 43)
    assert ops.layernorm_quant_launches() == q0                  # the backward launches no quantising LayerNorm
    grads = [p.grad for p in enc.parameters() if p.grad is not None]
    assert len(grads) > 100 and all(bool(torch.isfinite(g).all()) for g in grads)


@pytest.mark.gpu
def test_swin_b_all_fp8_switches(dev, monkeypatch, switches):
    """Swin-B, B 1 x V 1, fp8 attention and fp8 linears, forward and backward: every attention branch is unfused (24 norm1), the fused MLP
    takes the two C = 128 blocks of stage 0 (22 norm2), 3 patch merges."""
    from swinvox_amd import goldens
    enc = _encoder(dev, variant="base")
    x = goldens.synth_images(1, 1, 12).to(dev)
    S.set_math("bf16")
    S.set_storage("bf16")
    S.set_attention_fp8(True, backward=True)
    S.set_linear_fp8(True, backward=True)
    enc.zero_grad(set_to_none=True)
    out, feats, n = _forward(enc, x, monkeypatch)
    assert n[0] == 49, n
    out.float().square().mean().backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(f.float()).all()) for f in feats)
    assert all(bool(torch.isfinite(p.grad).all()) for p in enc.parameters() if p.grad is not None)
