"""fp8 forward of the Swin linears (csrc/linear_fp8.hip, ops.set_linear_fp8): the kernels through the C ABI against the recipe's torch
emulation (tests/test_cpu_linear_fp8_recipe.py, which pins that emulation on the CPU), then the host switch, the routing inside the
encoder, and a training smoke run."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_linear_fp8_recipe import INT_SHAPES, RECIPE_SHAPES, emulate_linear, gauss_case, integer_case, l1_rel, nan_padded, raw_bytes  # noqa: E402

import swinvox_amd as S  # noqa: E402
from swinvox_amd import hip, ops  # noqa: E402
from swinvox_amd.ops import call, ptr  # noqa: E402

# Bounds (L1-relative over the tensor unless noted).  fp32 against fp64 accumulation of the recipe is 3e-8 ... 5e-8 and the epilogue adds a few
# fp32 roundings and erff: 1e-4 is > 100 x what fp32 arithmetic contributes and 350 x under the distance of a bf16-operand linear from the
# recipe.  bf16 storage: the output rounding alone is 1.4e-3; 3e-3 is the window-attention test's value for bf16 storage.
L1_F32, L1_BF16 = 1e-4, 3e-3
MAX_BOUND = 1e-2       # worst element, relative to max|ref|
SEPARATION = 1.5e-2    # the bf16-operand linear_fwd must be at least this far from the recipe (measured on the CPU: 3.56e-2 ... 3.75e-2)
RPS = 49               # rows per drop-path scale


def _dt(store):
    return torch.bfloat16 if store == "bf16" else torch.float32


def _code(store):
    return hip.BF16 if store == "bf16" else hip.F32


def _quant(t, rows, K, ld=None):
    Kp = (K + 127) // 128 * 128
    q = torch.full((rows, Kp), 0x7F, dtype=torch.uint8, device=t.device)      # NaN bytes: the kernel must write all Kp of every row
    s = torch.full((rows,), float("nan"), dtype=torch.float32, device=t.device)
    call("sv_quant_rows_e4m3", ptr(t), hip.BF16 if t.dtype == torch.bfloat16 else hip.F32, rows, K, ld or K, ptr(q), Kp, ptr(s))
    return q, s


def _fp8_linear(x, W, out, M, K, N, store, **epi):
    xq, sx = _quant(x, M, K)
    wq, sw = _quant(W, N, K)
    e = ops._epilogue(epi.pop("ldc", N), **epi)
    call("sv_linear_fp8", ptr(xq), ptr(sx), ptr(wq), ptr(sw), ptr(out), M, K, N, C.byref(e), act=_code(store))
    return xq, sx, wq, sw


# ---- 1. exact integers --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", INT_SHAPES + [(37, 99, 30)])     # the last: K % 4 != 0 (unaligned rows in the quantiser), N % 4 != 0, odd ldc
def test_exact_integers(dev, shape):
    """Establishes the operand lane map, the K padding, the M / N edges and the per-row scale indexing: powers-of-two scales, operands exact
    in e4m3, partial sums exact in fp32 - the result equals the fp32 matrix product bit for bit.  The asymmetric random data catch a
    row <-> column swap.  The output buffer is over-allocated and NaN-filled: nothing beyond M rows / N columns may be touched."""
    M, K, N = shape
    x, W = integer_case(M, K, N)
    ref = (x.double() @ W.double().T).float()
    ldc, rows_alloc = (N + 8 if N % 4 == 0 else N + 1), M + 3
    out = torch.full((rows_alloc, ldc), float("nan"), dtype=torch.float32, device=dev)
    xq, sx, wq, sw = _fp8_linear(x.to(dev), W.to(dev), out, M, K, N, "f32", ldc=ldc)
    torch.cuda.synchronize()
    assert float(xq[:, K:].float().abs().max() if xq.shape[1] > K else 0) == 0.0          # padding bytes are zero
    assert torch.equal(torch.exp2(torch.log2(sx).round()), sx) and torch.equal(torch.exp2(torch.log2(sw).round()), sw)
    got = out.cpu()
    assert torch.equal(got[:M, :N], ref), float((got[:M, :N] - ref).abs().max())
    assert bool(torch.isnan(got[M:]).all()) and bool(torch.isnan(got[:, N:]).all())


# ---- 2. the recipe on N(0, 1) data ----------------------------------------------------------------------------------------------------
_CASES = {}


def _case(shape, store):
    """stored inputs of one (shape, storage), computed once and left unchanged"""
    key = (shape, store)
    if key not in _CASES:
        M, K, N = shape
        x, W = gauss_case(M, K, N)
        g = torch.Generator().manual_seed(77)
        bias = 0.5 * torch.randn(N, generator=g)
        res = torch.randn(M, N, generator=g).to(_dt(store))
        rs = 0.5 + torch.rand((M + RPS - 1) // RPS, generator=g)
        _CASES[key] = dict(x=x.to(_dt(store)), W=W, bias=bias, res=res, rs=rs, refs={})
    return _CASES[key]


def _reference(c, form):
    if form not in c["refs"]:
        kw = {"none": {}, "bias": dict(bias=c["bias"]), "gelu": dict(bias=c["bias"], gelu=True),
              "residual": dict(bias=c["bias"], residual=c["res"].float(), row_scale=c["rs"], rows_per_scale=RPS)}[form]
        c["refs"][form] = emulate_linear(c["x"], c["W"], **kw)
    return c["refs"][form]


def _check(name, got, ref, store):
    got, ref = got.float().cpu().double(), ref.double()
    l1, mx = l1_rel(got, ref), float((got - ref).abs().max() / ref.abs().max())
    print(f"{name}: L1-rel {l1:.3e}  worst element {mx:.3e} of max|ref|")
    assert bool(torch.isfinite(got).all())
    assert l1 <= (L1_BF16 if store == "bf16" else L1_F32), (name, l1)
    assert mx <= MAX_BOUND, (name, mx)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["none", "bias", "gelu", "residual"])
@pytest.mark.parametrize("store", ["f32", "bf16"])
@pytest.mark.parametrize("shape", RECIPE_SHAPES)
def test_recipe(dev, shape, store, form):
    """Kernel against the CPU emulation (fp32 scales and products, torch.float8_e4m3fn casts, fp64 contraction and epilogue) reading the same
    stored inputs, for every epilogue form the Swin call sites use."""
    M, K, N = shape
    c = _case(shape, store)
    ref, ref_pre = _reference(c, form)
    out = torch.full((M, N), float("nan"), dtype=_dt(store), device=dev)
    pre = torch.full((M, N), float("nan"), dtype=_dt(store), device=dev) if form == "gelu" else None
    epi = {"none": {}, "bias": dict(bias=c["bias"].to(dev)),
           "gelu": dict(bias=c["bias"].to(dev), act=hip.ACT_GELU, pre_act=pre),
           "residual": dict(bias=c["bias"].to(dev), residual=c["res"].to(dev), ldr=N, row_scale=c["rs"].to(dev), rows_per_scale=RPS)}[form]
    n0 = ops.linear_fp8_launches()
    _fp8_linear(c["x"].to(dev), c["W"].to(dev), out, M, K, N, store, **epi)
    torch.cuda.synchronize()
    assert ops.linear_fp8_launches() == n0 + 1
    _check(f"{shape} {store} {form}", out, ref, store)
    if pre is not None:
        _check(f"{shape} {store} {form} pre_act", pre, ref_pre, store)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["gelu", "residual"])
@pytest.mark.parametrize("store", ["f32", "bf16"])
def test_store_widths_agree(dev, store, form):
    """The epilogue's three piece widths perform the same arithmetic per element: the same quantised operands with ldc = ldr = 40 (16-byte
    pieces), 44 (4-element pieces under bf16 storage) and 41 (single elements) give the same bytes, for out and for pre_act, and nothing
    outside [:M, :N] of the NaN-filled buffers is written.  No tolerance."""
    M, K, N = 37, 99, 40
    x, W = gauss_case(M, K, N, seed=11)
    g = torch.Generator().manual_seed(79)
    bias = (0.5 * torch.randn(N, generator=g)).to(dev)
    res = torch.randn(M, N, generator=g).to(_dt(store))
    rs = (0.5 + torch.rand((M + RPS - 1) // RPS, generator=g)).to(dev)
    xq, sx = _quant(x.to(_dt(store)).to(dev), M, K)
    wq, sw = _quant(W.to(dev), N, K)
    runs = []
    for ld in (40, 44, 41):
        out = torch.full((M + 3, ld), float("nan"), dtype=_dt(store), device=dev)
        pre = torch.full((M + 3, ld), float("nan"), dtype=_dt(store), device=dev) if form == "gelu" else None
        epi = dict(bias=bias, act=hip.ACT_GELU, pre_act=pre) if form == "gelu" else \
            dict(bias=bias, residual=nan_padded(res, M + 3, ld, dev), ldr=ld, row_scale=rs, rows_per_scale=RPS)
        e = ops._epilogue(ld, **epi)
        call("sv_linear_fp8", ptr(xq), ptr(sx), ptr(wq), ptr(sw), ptr(out), M, K, N, C.byref(e), act=_code(store))
        torch.cuda.synchronize()
        runs.append([t for t in (out, pre) if t is not None])
    for ld, bufs in zip((40, 44, 41), runs):
        for t, t0 in zip(bufs, runs[0]):
            assert bool(torch.isfinite(t[:M, :N].float()).all()), ld
            assert torch.equal(raw_bytes(t[:M, :N]), raw_bytes(t0[:M, :N])), (ld, int((raw_bytes(t[:M, :N]) != raw_bytes(t0[:M, :N])).sum()))
            assert bool(torch.isnan(t[M:]).all()) and bool(torch.isnan(t[:, N:]).all()), ld


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["f32", "bf16"])
@pytest.mark.parametrize("shape", RECIPE_SHAPES)
def test_bf16_linear_is_separated_from_the_recipe(dev, shape, store):
    """Without this the bounds above would not tell the two paths apart: the engine's bf16-operand linear_fwd on the same stored inputs is
    >= 1.5e-2 (L1-relative) away from the recipe."""
    M, K, N = shape
    c = _case(shape, store)
    ref, _ = _reference(c, "none")
    ops.set_math("bf16")
    ops.set_storage(store)
    try:
        out = ops.empty(M, N, device=dev)
        ops.linear_fwd(c["x"].to(dev), M, ops.ConvSpec.linear(K, N), c["W"].to(dev), out)
        torch.cuda.synchronize()
    finally:
        ops.set_math("f32")
    d = l1_rel(out.float().cpu(), ref)
    print(f"{shape} {store}: bf16 linear_fwd vs the fp8 recipe {d:.3e}")
    assert d >= SEPARATION, d


# ---- 3. edge rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("store", ["f32", "bf16"])
def test_edge_rows(dev, store):
    """All-zero activation row and all-zero weight row: scale 1, output = the bias path only.  A row whose maximum is 1e-30: 224 / amax is
    clamped to 2^60 (the scale product of the epilogue stays finite), the row quantises to zeros; everything finite."""
    M, K, N = 24, 96, 40
    x, W = gauss_case(M, K, N, seed=5)
    x[3] = 0.0
    W[7] = 0.0
    x[9] = 1e-30 * torch.sign(x[9])
    W[11] = 1e-30 * torch.sign(W[11])
    x = x.to(_dt(store))
    bias = torch.linspace(-1, 1, N)
    ref, _ = emulate_linear(x, W, bias=bias)
    out = torch.full((M, N), float("nan"), dtype=_dt(store), device=dev)
    xq, sx, wq, sw = _fp8_linear(x.to(dev), W.to(dev), out, M, K, N, store, bias=bias.to(dev))
    torch.cuda.synchronize()
    assert float(sx[3]) == 1.0 and float(sw[7]) == 1.0 and float(sx[9]) == 2.0 ** 60 and float(sw[11]) == 2.0 ** 60
    got = out.float().cpu()
    assert bool(torch.isfinite(got).all())
    stored_bias = bias.to(_dt(store)).float()
    for r in (3, 9):
        assert torch.equal(got[r], stored_bias), r
    for col in (7, 11):
        assert torch.equal(got[:, col], stored_bias[col].expand(M)), col
    _check(f"edge rows {store}", out, ref, store)


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("what", ["stats", "act_grad_src", "col_off", "lrelu"])
def test_refusals(dev, what):
    M, K, N = 16, 128, 16
    x, W = gauss_case(M, K, N)
    out = torch.zeros(M, 2 * N, dtype=torch.float32, device=dev)
    dummy = torch.zeros(M * N * 2, dtype=torch.float64, device=dev)
    epi = {"stats": dict(stats=dummy), "act_grad_src": dict(act_grad_src=dummy, act_grad_kind=hip.ACT_GELU),
           "col_off": dict(ldc=2 * N, col_off=N), "lrelu": dict(act=hip.ACT_LRELU, slope=0.2)}[what]
    e = ops._epilogue(epi.pop("ldc", N), **epi)
    lib = hip.load()
    assert lib.sv_linear_fp8_supported(K, N, C.byref(ops._epilogue(N)), hip.MATH_BF16, hip.F32) == 1
    assert lib.sv_linear_fp8_supported(K, N, C.byref(e), hip.MATH_BF16, hip.F32) == 0
    assert lib.sv_linear_fp8_supported(K, N, C.byref(ops._epilogue(N)), hip.MATH_F32, hip.F32) == 0
    xq, sx = _quant(x.to(dev), M, K)
    wq, sw = _quant(W.to(dev), N, K)
    n0 = ops.linear_fp8_launches()
    with pytest.raises(RuntimeError, match="sv_linear_fp8"):
        call("sv_linear_fp8", ptr(xq), ptr(sx), ptr(wq), ptr(sw), ptr(out), M, K, N, C.byref(e), act=hip.F32)
    assert ops.linear_fp8_launches() == n0


# ---- 5. switch semantics --------------------------------------------------------------------------------------------------------------
def test_switch_semantics():
    try:
        ops.set_math("f32")
        assert not ops.linear_fp8_enabled()                      # off by default
        ops.set_math("bf16")
        assert not ops.linear_fp8_enabled()
        S.set_linear_fp8(True)
        assert ops.linear_fp8_enabled()
        assert ops.attention_math() == hip.MATH_BF16             # independent of the attention switch ...
        S.set_attention_fp8(True, backward=True)
        assert ops.linear_fp8_enabled() and ops.attention_math() == hip.MATH_FP8 and ops.attention_bwd_math() == hip.MATH_FP8_FULL
        S.set_linear_fp8(False)                                  # ... in both directions
        assert not ops.linear_fp8_enabled() and ops.attention_math() == hip.MATH_FP8
        S.set_attention_fp8(False)
        S.set_linear_fp8(True)
        ops.set_math("f32")                                      # inert under f32 math
        assert not ops.linear_fp8_enabled()
    finally:
        S.set_linear_fp8(False)
        S.set_attention_fp8(False)
        ops.set_math("f32")


# ---- 6. / 7. encoder runs -------------------------------------------------------------------------------------------------------------
def _expected_launches(enc):
    """fp8 launches of one forward under the CURRENT settings: 4 per block, less 2 for each branch a fused stage-0 kernel takes, + 1 per
    patch merge"""
    n = 0
    for stage in enc.swin_transformer.model.stages():
        n += 0 if isinstance(stage.downsample, torch.nn.Identity) else 1
        for blk in stage.blocks:
            n += 0 if ops.fused_attn_block_enabled(blk.dim, blk.heads) else 2
            n += 0 if ops.fused_mlp_enabled(blk.dim) else 2
    return n


def _encoder_step(enc, x, monkeypatch):
    """one forward + backward; returns (output, the Swin stage feature maps, gradients, fp8 launches of the step)"""
    from swinvox_amd.models import encoder as enc_mod
    feats = []
    real = enc_mod.swin_forward

    def spy(*a, **k):
        f, tape = real(*a, **k)
        feats.extend(t.float().cpu() for t in f)
        return f, tape

    monkeypatch.setattr(enc_mod, "swin_forward", spy)
    enc.zero_grad(set_to_none=True)
    n0 = ops.linear_fp8_launches()
    out = enc(x)
    n1 = ops.linear_fp8_launches()
    out.float().square().mean().backward()
    torch.cuda.synchronize()
    monkeypatch.setattr(enc_mod, "swin_forward", real)
    grads = {n: p.grad.detach().float().cpu() for n, p in enc.named_parameters() if p.grad is not None}
    return out.detach().float().cpu(), feats, grads, n1 - n0, ops.linear_fp8_launches() - n1


@pytest.mark.gpu
def test_swin_t_encoder_modes(dev, monkeypatch):
    """Swin-T encoder, B = 1 x V = 2, bf16 storage, one forward + backward in exact f32, bf16, fp8-linear and fp8-linear with both stage-0
    fusions off.  The launch counter proves the routing; with the switch off nothing moves, bit for bit; the backward launches no fp8
    kernel.  The distance of the four stage feature maps from exact f32 is printed and only asserted < 0.5."""
    from swinvox_amd import goldens
    from swinvox_amd.models import Encoder
    enc = Encoder(S.default_cfg())
    goldens.seeded_fill_(enc, 100)
    enc.to(dev).train()
    enc.stochastic = False
    x = goldens.synth_images(1, 2, 11).to(dev)
    runs = {}
    try:
        for mode in ("f32", "bf16", "fp8", "fp8_unfused", "bf16_again"):      # the second bf16 run follows the fp8 ones: nothing may linger
            S.set_math("f32" if mode == "f32" else "bf16")
            if mode != "f32":
                S.set_storage("bf16")
            S.set_linear_fp8(mode.startswith("fp8") or mode == "f32")       # under f32 math the switch is inert
            ops.set_fused_attn_block(mode != "fp8_unfused")
            ops.set_fused_mlp(mode != "fp8_unfused")
            want = _expected_launches(enc) if mode.startswith("fp8") else 0
            out, feats, grads, fwd, bwd = _encoder_step(enc, x, monkeypatch)
            print(f"{mode}: {fwd} fp8 launches in the forward (expected {want}), {bwd} in the backward")
            assert fwd == want and bwd == 0, (mode, fwd, want, bwd)
            assert all(bool(torch.isfinite(t).all()) for t in grads.values()), mode
            assert bool(torch.isfinite(out).all()) and len(feats) == 4
            runs[mode] = (out, feats, grads, fwd)
    finally:
        S.set_linear_fp8(False)
        ops.set_fused_attn_block(True)
        ops.set_fused_mlp(True)
        S.set_math("f32")
    assert runs["fp8"][3] == 4 * 10 + 3 and runs["fp8_unfused"][3] == 4 * 12 + 3      # Swin-T: 12 blocks, stage 0 (2 blocks) fused by default
    # switch off again AFTER the fp8 forwards (quantised-weight cache filled, fusions toggled) = the first bf16 run, bit for bit, on what the
    # Swin linears feed (the encoder output also carries the ResNet branch, whose BatchNorm statistics are summed with atomics)
    assert all(torch.equal(a, b) for a, b in zip(runs["bf16"][1], runs["bf16_again"][1]))
    for mode in ("fp8", "fp8_unfused"):
        assert not torch.equal(runs[mode][0], runs["bf16"][0]), mode
    assert not torch.equal(runs["fp8"][1][0], runs["fp8_unfused"][1][0])      # stage 0 runs on fp8 linears only when unfused
    for mode in ("bf16", "fp8", "fp8_unfused"):
        d = [l1_rel(a, b) for a, b in zip(runs[mode][1], runs["f32"][1])]
        print(f"{mode}: stage feature maps vs exact f32, L1-rel {[f'{v:.3e}' for v in d]}; encoder output {l1_rel(runs[mode][0], runs['f32'][0]):.3e}")
        assert max(d) < 0.5, (mode, d)


@pytest.mark.gpu
def test_swin_b_encoder_both_fp8_switches(dev, monkeypatch):
    """BASELINE configuration 5: Swin-B, fp8 attention (forward and backward) and fp8 linears together, one forward + backward at
    B = 1 x V = 1.  Reaches K = 128 ... 4096.  Finite; 4 launches per block + 3 patch merges, less what the fused MLP takes at C = 128."""
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
        S.set_linear_fp8(True)
        want = _expected_launches(enc)
        fused_mlp = sum(1 for st in enc.swin_transformer.model.stages() for b in st.blocks if ops.fused_mlp_enabled(b.dim))
        out, feats, grads, fwd, bwd = _encoder_step(enc, x, monkeypatch)
    finally:
        S.set_linear_fp8(False)
        S.set_attention_fp8(False)
        S.set_math("f32")
    print(f"Swin-B: {fwd} fp8 linear launches, {fused_mlp} blocks on the fused MLP")
    assert fwd == want == 4 * 24 + 3 - 2 * fused_mlp and bwd == 0
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(t).all()) for t in grads.values())


# ---- 8. training smoke ----------------------------------------------------------------------------------------------------------------
LOSS_FACTOR = 1.5      # the project's factors (tests/test_gpu_attn_fp8_bwd.py)
TAIL_FACTOR = 1.15


@pytest.mark.gpu
def test_training_smoke_fp8_linear(dev):
    """Whole pipeline, Swin-T, B = 2 x V = 2, one fixed batch, 20 flat-Adam steps in bf16 and in fp8-linear mode, as
    test_training_smoke_fp8_full does it: the loss falls and stays finite, the final loss is within LOSS_FACTOR of the bf16 run's, the mean
    of the last five steps within TAIL_FACTOR."""
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
    for mode in ("bf16", "fp8_linear"):
        torch.manual_seed(0)
        nets = [Encoder(cfg), Decoder(cfg), Merger(cfg), Refiner(cfg)]
        for n in nets:
            O.seeded_weights_(n, seed=7)
            n.to(dev).train()
        solvers, _ = harness.make_solvers(nets, cfg)
        S.set_math("bf16")
        S.set_storage("bf16")
        S.set_linear_fp8(mode == "fp8_linear")
        n0 = ops.linear_fp8_launches()
        try:
            losses = []
            for _ in range(20):
                el, rl = harness.train_step(nets, solvers, cfg, x, gt)
                losses.append(float(el + rl))
        finally:
            S.set_linear_fp8(False)
            S.set_math("f32")
        print(f"{mode}: losses {[round(v, 4) for v in losses]}")
        assert (ops.linear_fp8_launches() - n0 > 0) == (mode == "fp8_linear")
        assert all(np.isfinite(losses)) and losses[-1] < losses[0], (mode, losses)
        final[mode] = (losses[-1], sum(losses[-5:]) / 5)
    assert final["fp8_linear"][0] < LOSS_FACTOR * final["bf16"][0], final
    assert final["fp8_linear"][1] < TAIL_FACTOR * final["bf16"][1], final
