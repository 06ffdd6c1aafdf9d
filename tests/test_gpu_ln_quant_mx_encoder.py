"""The MX quantising LayerNorm inside the Swin encoder (ops.set_ln_quant_mx, models/swin_transformer.py _norm_for_linear): the launch counters
prove which sites take it - with the switch on an MX forward of the unfused Swin path runs no stand-alone activation quantiser at all - and
the stage feature maps equal those of LayerNorm + stand-alone MX quantiser bit for bit, in a training forward and in a torch.no_grad() forward,
where the fused form stores neither the rows nor the statistics.

Fixture of the neighbouring encoder tests (restated: their helpers are bound to their own counters): Swin-T Encoder with the golden recipe's
encoder weights (goldens.seeded_fill_(enc, 100)), B 1 x V 2 synthetic renderings, bf16 math and storage."""
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
        ops.set_ln_quant_mx(False)
        ops.set_ln_quant_fused(True)
        ops.set_mx_producer_quant(True)
        ops.set_fused_attn_block(True)
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


def _counters():
    return (ops.linear_mxfp8_launches(), ops.mx_act_quant_launches(), ops.layernorm_quant_mx_launches(), ops.layernorm_quant_launches())


def _forward(enc, x, monkeypatch, grad=True):
    """one forward; returns (output, the Swin stage feature maps as stored, movement over the forward of the counters: MX GEMMs, stand-alone MX
    activation quantisers, MX quantising LayerNorms, row-form quantising LayerNorms)"""
    from swinvox_amd.models import encoder as enc_mod
    feats = []
    real = enc_mod.swin_forward

    def spy(*a, **k):
        f, tape = real(*a, **k)
        feats.extend(t.detach().clone() for t in f)
        return f, tape

    monkeypatch.setattr(enc_mod, "swin_forward", spy)
    n0 = _counters()
    try:
        if grad:
            out = enc(x)
        else:
            with torch.no_grad():
                out = enc(x)
        torch.cuda.synchronize()
    finally:
        monkeypatch.setattr(enc_mod, "swin_forward", real)
    return out, [f.cpu() for f in feats], tuple(b - a for a, b in zip(n0, _counters()))


def _same(a, b):
    return len(a) == len(b) == 4 and all(torch.equal(p, q) for p, q in zip(a, b))


def _backward_is_finite(enc, out):
    out.float().square().mean().backward()
    torch.cuda.synchronize()
    grads = [p.grad for p in enc.parameters() if p.grad is not None]
    return len(grads) > 100 and all(bool(torch.isfinite(g).all()) for g in grads)


@pytest.mark.gpu
def test_swin_t_routing_and_bit_equality(dev, monkeypatch, switches):
    from swinvox_amd import goldens
    enc = _encoder(dev)
    x = goldens.synth_images(1, 2, 11).to(dev)
    S.set_math("bf16")
    S.set_storage("bf16")
    S.set_linear_fp8(True, recipe="mx")
    # the default: the switch is off.  Stage 0 (2 blocks) runs the fused attention branch and the fused MLP -> 10 unfused blocks x 2 + 3
    # patch merges take the stand-alone quantiser
    assert not ops.ln_quant_mx_enabled()
    _, f_off, n = _forward(enc, x, monkeypatch)
    assert n == (43, 23, 0, 0), n
    _, f_off_ng, n = _forward(enc, x, monkeypatch, grad=False)
    assert n == (43, 23, 0, 0), n

    ops.set_ln_quant_mx(True)
    enc.zero_grad(set_to_none=True)
    out, f_on, n = _forward(enc, x, monkeypatch)
    assert n == (43, 0, 23, 0), n                                # no stand-alone activation quantiser is left; the row form's counter rests
    assert _same(f_on, f_off)
    n0 = _counters()
    assert _backward_is_finite(enc, out)                         # the backward reads the stored ln1 / ln2 / lnm, mean and rstd
    assert _counters()[1:] == n0[1:]                             # and launches no quantiser or quantising LayerNorm of the forward
    # torch.no_grad(): no backward follows, the fused sites store only the e4m3 rows and the block scales
    _, f_on_ng, n = _forward(enc, x, monkeypatch, grad=False)
    assert n == (43, 0, 23, 0), n
    assert _same(f_on_ng, f_off_ng)

    # both stage-0 fusions off: 12 blocks x 2 + 3
    ops.set_fused_attn_block(False)
    ops.set_fused_mlp(False)
    _, f_on_u, n = _forward(enc, x, monkeypatch)
    assert n == (51, 0, 27, 0), n
    _, f_on_u_ng, n = _forward(enc, x, monkeypatch, grad=False)
    assert n == (51, 0, 27, 0), n
    ops.set_ln_quant_mx(False)
    _, f_off_u, n = _forward(enc, x, monkeypatch)
    assert n == (51, 27, 0, 0), n
    _, f_off_u_ng, n = _forward(enc, x, monkeypatch, grad=False)
    assert n == (51, 27, 0, 0), n
    assert _same(f_on_u, f_off_u) and _same(f_on_u_ng, f_off_u_ng)
    assert not torch.equal(f_on_u[0], f_on[0])                   # stage 0 runs on MX linears only when unfused


@pytest.mark.gpu
def test_swin_t_switch_is_independent_and_inert_elsewhere(dev, monkeypatch, switches):
    from swinvox_amd import goldens
    enc = _encoder(dev)
    x = goldens.synth_images(1, 2, 11).to(dev)
    S.set_math("bf16")
    S.set_storage("bf16")
    _, f_bf16, n = _forward(enc, x, monkeypatch)                 # bf16 run before anything fp8
    assert n == (0, 0, 0, 0), n
    S.set_linear_fp8(True, recipe="mx")
    _, f_mx, n = _forward(enc, x, monkeypatch)
    assert n == (43, 23, 0, 0), n

    # independent of the producers' switch: with emission off only the proj / fc2 sites (10 unfused blocks x 2) take the stand-alone quantiser
    ops.set_ln_quant_mx(True)
    ops.set_mx_producer_quant(False)
    _, f_noemit, n = _forward(enc, x, monkeypatch)
    assert n == (43, 20, 23, 0), n
    assert _same(f_noemit, f_mx)
    ops.set_mx_producer_quant(True)

    # the switch on has no effect under the row recipe (its own quantising LayerNorm runs), under bf16 without fp8 and under f32 math
    S.set_linear_fp8(True)
    _, _, n = _forward(enc, x, monkeypatch)
    assert n == (0, 0, 0, 23), n
    S.set_linear_fp8(False)
    _, f_bf16_again, n = _forward(enc, x, monkeypatch)
    assert n == (0, 0, 0, 0), n
    assert _same(f_bf16, f_bf16_again)                           # a bf16 run after all of this = the bf16 run before it, bit for bit
    assert not _same(f_mx, f_bf16)                               # the MX linears did run
    S.set_linear_fp8(True, recipe="mx")
    S.set_math("f32")
    _, _, n = _forward(enc, x, monkeypatch)
    assert n == (0, 0, 0, 0), n


@pytest.mark.gpu
def test_swin_t_mx_backward_with_the_switch_on(dev, monkeypatch, switches):
    """MX forward and MX backward of the linears with the MX quantising LayerNorm on: the forward counts as above, the MX data / weight gradient
    counters move by (43, 43), every gradient is finite; no bit comparison (the bf16 weight gradients elsewhere use atomics)."""
    from swinvox_amd import goldens
    enc = _encoder(dev)
    x = goldens.synth_images(1, 2, 11).to(dev)
    S.set_math("bf16")
    S.set_storage("bf16")
    S.set_linear_fp8(True, backward=True, recipe="mx", backward_recipe="mx")
    ops.set_ln_quant_mx(True)
    enc.zero_grad(set_to_none=True)
    out, _, n = _forward(enc, x, monkeypatch)
    assert n == (43, 0, 23, 0), n
    b0, q0 = ops.linear_mxfp8_bwd_launches(), ops.layernorm_quant_mx_launches()
    assert _backward_is_finite(enc, out)
    b1 = ops.linear_mxfp8_bwd_launches()
    assert (b1[0] - b0[0], b1[1] - b0[1]) == (43, 43)
    assert ops.layernorm_quant_mx_launches() == q0               # the backward launches no quantising LayerNorm


@pytest.mark.gpu
def test_swin_b_every_fp8_switch(dev, monkeypatch, switches):
    """Swin-B, B 1 x V 1, fp8 attention, MX linears forward and backward, producer emission and the MX quantising LayerNorm: every attention
    branch is unfused (24 norm1), the fused MLP takes the two C = 128 blocks of stage 0 (22 norm2), 3 patch merges - the 49 stand-alone
    quantisers of the same model with the switch off become 49 MX quantising LayerNorms and none is left."""
    from swinvox_amd import goldens
    enc = _encoder(dev, variant="base")
    x = goldens.synth_images(1, 1, 12).to(dev)
    S.set_math("bf16")
    S.set_storage("bf16")
    S.set_attention_fp8(True, backward=True)
    S.set_linear_fp8(True, backward=True, recipe="mx", backward_recipe="mx")
    _, f_off, n_off = _forward(enc, x, monkeypatch)
    assert n_off == (95, 49, 0, 0), n_off
    ops.set_ln_quant_mx(True)
    enc.zero_grad(set_to_none=True)
    out, feats, n = _forward(enc, x, monkeypatch)
    assert n == (95, 0, n_off[1], 0), n
    assert _same(feats, f_off)
    assert _backward_is_finite(enc, out)
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(f.float()).all()) for f in feats)
