"""MX dual quantiser (ops.set_mx_dual_quant) inside the Swin-T encoder: the training step with the MX forward, the MX backward and the inputs
stored as MX rows, switch off then on."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_linear_mxfp8_bwd import COLSUM_BOUND  # noqa: E402  (the project's bound: imported, not restated)

import swinvox_amd as S  # noqa: E402
from swinvox_amd import hip, ops  # noqa: E402


def _counters():
    lib = hip.load()
    return np.array([int(lib.sv_quant_rows_cols_mx_launches()), int(lib.sv_quant_cols_mx_launches()), int(lib.sv_quant_rows_mx_launches()),
                     int(lib.sv_mx_rows_to_cols_launches()), *ops.linear_mxfp8_bwd_launches(), ops.linear_mxfp8_launches()])


def _step(enc, x, monkeypatch):
    """one forward + backward -> (stage feature maps, gradients by name, the counters' increase, MX column quantiser calls on a weight,
    the data gradient every swin_linear_dgrad wrote, keyed by the name of its weight)"""
    from swinvox_amd.models import encoder as enc_mod
    feats, on_weights, dxs = [], [0], []
    real, real_cols, real_dgrad = enc_mod.swin_forward, ops.quantize_cols_mx, ops.swin_linear_dgrad
    names = {id(p): n for n, p in enc.named_parameters()}

    def spy(*a, **k):
        f, tape = real(*a, **k)
        feats.extend(t.float().cpu() for t in f)
        return f, tape

    def spy_cols(t, *a, **k):
        on_weights[0] += isinstance(t, torch.nn.Parameter)
        return real_cols(t, *a, **k)

    def spy_dgrad(dy, rows, spec, w, dx, **epi):
        real_dgrad(dy, rows, spec, w, dx, **epi)
        dxs.append((names[id(w)], dx.clone()))

    monkeypatch.setattr(enc_mod, "swin_forward", spy)
    monkeypatch.setattr(ops, "quantize_cols_mx", spy_cols)
    monkeypatch.setattr(ops, "swin_linear_dgrad", spy_dgrad)
    try:
        enc.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        n0 = _counters()
        out = enc(x)
        out.float().square().mean().backward()
        torch.cuda.synchronize()
        n1 = _counters()
    finally:
        monkeypatch.setattr(enc_mod, "swin_forward", real)
        monkeypatch.setattr(ops, "quantize_cols_mx", real_cols)
        monkeypatch.setattr(ops, "swin_linear_dgrad", real_dgrad)
    assert bool(torch.isfinite(out.float()).all()) and len(feats) == 4
    grads = {n: p.grad.detach().float().cpu() for n, p in enc.named_parameters() if p.grad is not None}
    del out
    return feats, grads, tuple(int(v) for v in n1 - n0), on_weights[0], {n: t.cpu() for n, t in dxs}


SPREAD_FACTOR = 8     # a gradient accumulated by fp32 atomics: switch on against off may differ by this many times what two switch-off runs differ by


@pytest.mark.gpu
def test_swin_t_encoder_mx_dual_quant(dev, monkeypatch):
    """Swin-T, golden weights, B = 1 x V = 2, bf16 storage, MX forward + MX backward + store "mx"; runs: switch off, off again, on, plain bf16.
    The forward feature maps are bit-identical.  What the MX sites compute is bit-identical to the switch-off run: every weight gradient of an
    MX site (43: the kernel is deterministic) and every data gradient swin_linear_dgrad writes (43: everything the rest of the backward reads
    from an MX site).  The biases of the MX linears (their sums moved from the column quantiser's pass into the dual quantiser's) are within
    1e-6 of max|ref| of the switch-off run.  The dual quantiser runs once per MX weight gradient of the step, the row quantiser once less per
    MX data gradient, the re-blocker and the GEMMs as before, and nothing moves in the bf16 step afterwards.
    Every other parameter gradient is formed by kernels the switch does not reach, from inputs that are bit-identical (above).  Bit-identity
    cannot be asked of them: the LayerNorm gradients, the relative position bias tables, the fused stage-0 blocks and the ResNet branch
    accumulate with fp32 atomics and differ between two switch-off runs of this very test (measured: 118 of them, by up to 4.5e-7 of
    max|ref|; swin_downsamples.0.0.bias, a conv bias in front of a BatchNorm whose exact gradient is zero, by 1.4e-5 of its own maximum; some
    agree in one pair of runs and not in the next).  They must lie within the largest of: 1e-6 of max|ref| (the project's bound for a
    reordered fp32 sum); for a bias, 1e-6 of the maximum of its layer's weight gradient (the same dy terms contracted with inputs of order
    one: the size of the terms where the bias gradient itself cancels); SPREAD_FACTOR x the difference of the two switch-off runs.
    The MX column quantiser: no launch on a gradient or an activation remains.  The counter of sv_quant_cols_mx_e4m3 itself still moves by
    the W^T operands of the data gradients (quantize_weight_t_mx, once per weight and forward: the same entry point, in both runs), so the
    check is that it moves by exactly the calls that were handed a Parameter, counted at ops.quantize_cols_mx, and by that number in the
    switch-off run plus one per MX weight gradient (its dy passes)."""
    from swinvox_amd import goldens
    from swinvox_amd.models import Encoder
    enc = Encoder(S.default_cfg())
    goldens.seeded_fill_(enc, 100)
    enc.to(dev).train()
    enc.stochastic = False
    x = goldens.synth_images(1, 2, 11).to(dev)
    runs = {}
    try:
        for mode in ("off", "off2", "on", "bf16"):
            S.set_math("bf16")
            S.set_storage("bf16")
            mx = mode != "bf16"
            S.set_linear_fp8(mx, backward=mx, recipe="mx", backward_recipe="mx", store="mx")
            ops.set_mx_dual_quant(mode == "on")
            assert ops.mx_dual_quant_enabled() == (mode == "on")
            runs[mode] = _step(enc, x, monkeypatch)
            print(f"{mode}: (dual, MX column quantiser, MX row quantiser, re-blocker, MX dgrad, MX wgrad, MX GEMMs) = {runs[mode][2]}; "
                  f"column quantiser calls on a weight {runs[mode][3]}")
            assert all(bool(torch.isfinite(t).all()) for t in runs[mode][1].values()), mode
            assert ops._CTX.dyq is None, mode
    finally:
        ops.set_mx_dual_quant(False)
        S.set_linear_fp8(False)
        S.set_math("f32")
    a, b = runs["off"][2], runs["on"][2]
    dgrads, wgrads = a[4], a[5]
    assert wgrads > 0 and dgrads > 0 and a[3:] == b[3:], (a, b)                # the re-blocker and the GEMMs do not move
    assert a[0] == 0 and b[0] == wgrads, (a, b)
    assert b[1] == runs["on"][3] and a[1] == runs["off"][3] + wgrads and runs["on"][3] == runs["off"][3], (a, b, runs["off"][3], runs["on"][3])
    assert a[2] - b[2] == dgrads, (a, b)
    assert runs["bf16"][2] == (0,) * 7
    assert all(torch.equal(u, v) for u, v in zip(runs["off"][0], runs["on"][0]))
    # what the MX sites compute
    sites = set(runs["on"][4])
    assert len(sites) == dgrads == len(runs["off"][4]) and sites == set(runs["off"][4])
    for n in sorted(sites):
        assert torch.equal(runs["off"][4][n].view(torch.int16), runs["on"][4][n].view(torch.int16)), ("dx", n)
        assert torch.equal(runs["off"][1][n], runs["on"][1][n]), ("dw", n, int((runs["off"][1][n] != runs["on"][1][n]).sum()))
        assert torch.equal(runs["off"][1][n], runs["off2"][1][n]), ("dw of two switch-off runs", n)
    mx_bias = {n.replace("weight", "bias") for n in sites} & set(runs["off"][1])
    assert len(mx_bias) == 40                                                    # the patch-merge reductions have none
    # everything else
    differing, baseline = [], 0
    for n, g_off in runs["off"][1].items():
        if n in sites:
            continue
        g_on, g_off2 = runs["on"][1][n].double(), runs["off2"][1][n].double()
        scale = float(g_off.double().abs().max())
        err, spread = float((g_on - g_off.double()).abs().max()), float((g_off2 - g_off.double()).abs().max())
        baseline += spread > 0
        if n in mx_bias:
            assert err <= COLSUM_BOUND * scale, (n, err / scale)
        elif err > 0:
            terms = float(runs["off"][1].get(n.replace("bias", "weight"), g_off).double().abs().max()) if n.endswith("bias") else scale
            differing.append((n, err / scale, spread / scale, terms / scale))
            assert err <= max(COLSUM_BOUND * max(scale, terms), SPREAD_FACTOR * spread), (n, err / scale, spread / scale, terms / scale)
    print(f"{baseline} gradients differ between the two switch-off runs; switch on against off, outside the MX sites (name, difference, "
          f"difference of the two switch-off runs, size of the terms; all of max|ref|): {differing}")
