"""fp8 (OCP e4m3) backward of the Swin window attention (SV_MATH_FP8_FULL, `set_attention_fp8(True, backward=True)`).

The kernel computes the gradient of exactly the function the SV_MATH_FP8 forward evaluates, every quantiser taken as the identity.  The
op test emulates that recipe on the CPU: torch.float8_e4m3fn casts for the quantisers (OCP e4m3, what gfx950 converts to) and fp64 for
the contractions, the softmax and its gradient.  The quantiser INPUTS (q' = scale q, the per-tile scales 224 / amax and the scaled
values) are formed in fp32 as the kernel forms them, so that both sides round the same fp32 numbers to e4m3; everything the kernel then
does in fp32 (MFMA accumulation, __expf, rcp) is what the bounds absorb.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import swinvox_amd as S  # noqa: E402
from swinvox_amd import hip, ops  # noqa: E402
from swinvox_amd.ops import call, ptr  # noqa: E402

E4M3 = torch.float8_e4m3fn
SCALE32 = torch.tensor(1.0 / math.sqrt(32.0), dtype=torch.float32)   # the kernel's fp32 head_dim^-0.5

# kernel vs emulation (L1-relative over the whole tensor): fp32 MFMA accumulation, __expf / rcp in the softmax and the order of the
# sums move a few values across an e4m3 rounding boundary (dS, Pq); bf16 storage adds its own output rounding (up to 2^-9 per element).
L1_BOUND = {"f32": 1e-3, "bf16": 3e-3}
MAX_BOUND = 0.1        # worst element, relative to max|ref|: one e4m3 step of a single dS or Pq value moves an element by that much
SEPARATION = 10.0      # the bf16 backward must sit at least this many bounds away from the fp8 recipe


def _partition(x, I, H, shift):
    """[I*H*H, Cx] token rows -> [I*nW, 49, Cx] windows of the cyclically shifted map"""
    Cx = x.shape[-1]
    x = x.view(I, H, H, Cx)
    if shift:
        x = torch.roll(x, (-shift, -shift), (1, 2))
    return x.view(I, H // 7, 7, H // 7, 7, Cx).permute(0, 1, 3, 2, 4, 5).reshape(-1, 49, Cx)


def _reverse(w, I, H, shift):
    Cx = w.shape[-1]
    x = w.view(I, H // 7, H // 7, 7, 7, Cx).permute(0, 1, 3, 2, 4, 5).reshape(I, H, H, Cx)
    if shift:
        x = torch.roll(x, (shift, shift), (1, 2))
    return x.reshape(-1, Cx)


def _scale(t32):
    """per-tile scale 224 / amax over the last two dims (fp32, as the kernel); 1 for an all-zero tile"""
    m = t32.abs().amax(dim=(-2, -1), keepdim=True)
    return torch.where(m > 0, torch.tensor(224.0, dtype=torch.float32) / m, torch.ones_like(m))


def _e4m3(t32):
    return t32.to(E4M3).double()


def _emulate(qkv, table, dout, I, H, C, heads, shift):
    """The fp8 backward recipe on fp32 copies of the stored values -> (dqkv [I*H*H, 3C] fp64, dtable [169, heads] fp64)"""
    from oracle.model import rel_pos_index, shift_attn_mask
    xw = _partition(qkv.float(), I, H, shift).view(-1, 49, 3, heads, 32).permute(2, 0, 3, 1, 4)       # [3, B_, heads, 49, 32]
    q, k, v = xw[0] * SCALE32, xw[1], xw[2]
    do = _partition(dout.float(), I, H, shift).view(-1, 49, heads, 32).transpose(1, 2)                 # [B_, heads, 49, 32]
    sq, sk, sv, so = _scale(q), _scale(k), _scale(v), _scale(do)
    Qq, Kq, Vq, Dq = _e4m3(q * sq), _e4m3(k * sk), _e4m3(v * sv), _e4m3(do * so)
    sq, sk, sv, so = sq.double(), sk.double(), sv.double(), so.double()
    idx = rel_pos_index(7).reshape(-1)
    bias = table.double()[idx].view(49, 49, heads).permute(2, 0, 1)[None]
    s = Qq @ Kq.transpose(-2, -1) / (sq * sk) + bias
    if shift:
        m = shift_attn_mask(H, H, 7, shift).double()
        s = (s.view(I, -1, heads, 49, 49) + m[None, :, None]).view(-1, heads, 49, 49)
    p = s.softmax(-1)
    Pq = _e4m3((p * 256.0).float())
    dv = Pq.transpose(-2, -1) @ Dq / (256.0 * so)
    dp = Dq @ Vq.transpose(-2, -1) / (so * sv)
    ds = p * (dp - (dp * p).sum(-1, keepdim=True))
    dtable = torch.zeros(169, heads, dtype=torch.float64)
    dtable.index_add_(0, idx, ds.sum(0).permute(1, 2, 0).reshape(-1, heads))
    ss = _scale(ds.float())
    dSq = _e4m3(ds.float() * ss)
    ss = ss.double()
    dq = dSq @ Kq / (ss * sk) * float(SCALE32)
    dk = dSq.transpose(-2, -1) @ Qq / (ss * sq)
    g = torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(-1, 49, 3 * C)                  # [B_, 49, (3, heads, 32)]
    return _reverse(g, I, H, shift), dtable


def _l1(a, ref):
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    return float((a - ref).abs().sum() / (ref.abs().sum() + 1e-30))


def _mx(a, ref):
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    return float((a - ref).abs().max() / (ref.abs().max() + 1e-30))


def _images_for_two_windows_per_workgroup(heads):
    """images of a 14 x 14 map such that sv_window_attention_bwd's SV_MATH_FP8_FULL launch gives every workgroup > 1 window (the grid is one
    resident wave of 3 workgroups per CU on 256 CUs: 768 / heads window chunks per head)"""
    return (768 // heads) // 4 + 2


_CASES = {}


def _case(heads, shift, store):
    key = (heads, shift, store)
    if key not in _CASES:
        _CASES.clear()                             # one case at a time: the heads-3 images are ~0.1 GB with their reference
        H = 14
        I, C = _images_for_two_windows_per_workgroup(heads), heads * 32
        g = torch.Generator().manual_seed(100 * heads + 10 * shift + (store == "bf16"))
        dt = torch.bfloat16 if store == "bf16" else torch.float32
        qkv = torch.randn(I * H * H, 3 * C, generator=g)
        dout = torch.randn(I * H * H, C, generator=g)
        table = 0.5 * torch.randn(169, heads, generator=g)
        # one (window, head) tile whose dO is zero (finite, zero gradient of the tile) and one whose v is zero (amax 0: scale 1)
        dw = _partition(dout, I, H, shift)
        dw[1, :, 0:32] = 0.0
        dout = _reverse(dw, I, H, shift).contiguous()
        qw = _partition(qkv, I, H, shift)
        qw[2, :, 2 * C + 32 * (heads - 1):2 * C + 32 * heads] = 0.0
        qkv = _reverse(qw, I, H, shift).contiguous()
        qkv, dout = qkv.to(dt), dout.to(dt)     # the emulation reads the same stored values the kernel reads
        ref = _emulate(qkv, table, dout, I, H, C, heads, shift)
        _CASES[key] = (I, H, C, qkv, table, dout, ref)
    return _CASES[key]


def _run_bwd(dev, qkv, table, dout, I, H, C, heads, shift, math_code, store, workspace):
    act = hip.BF16 if store == "bf16" else hip.F32
    qd, td, dod = qkv.to(dev), table.to(dev), dout.to(dev)
    dqkv = torch.empty(qd.shape, dtype=qd.dtype, device=dev)
    dt = torch.zeros(169, heads, device=dev)
    ws = torch.zeros(int(hip.load().sv_window_attention_bwd_workspace_floats(heads)), device=dev) if workspace else None
    call("sv_window_attention_bwd", ptr(qd), ptr(td), ptr(dod), ptr(dqkv), ptr(dt), ptr(ws) if ws is not None else None,
         I, H, H, C, heads, shift, math_code, act=act)
    torch.cuda.synchronize()
    return dqkv.cpu(), dt.cpu()


@pytest.mark.parametrize("store", ["f32", "bf16"])
@pytest.mark.parametrize("heads", [3, 4, 32])
@pytest.mark.parametrize("shift", [0, 3])
def test_fp8_backward_matches_the_recipe(dev, shift, heads, store):
    """dqkv and dtable of SV_MATH_FP8_FULL against the emulated recipe, with the workspace NULL (direct table atomics) and given (slot
    images + fold); the bf16 backward on the same inputs must be SEPARATION bounds away from the recipe."""
    I, H, C, qkv, table, dout, (rq, rt) = _case(heads, shift, store)
    dq16, dt16 = _run_bwd(dev, qkv, table, dout, I, H, C, heads, shift, hip.MATH_BF16, store, True)
    s_q, s_t = _l1(dq16, rq), _l1(dt16, rt)
    bound = L1_BOUND[store]
    for workspace in (False, True):
        dq8, dt8 = _run_bwd(dev, qkv, table, dout, I, H, C, heads, shift, hip.MATH_FP8_FULL, store, workspace)
        e_q, e_t, e_mx = _l1(dq8, rq), _l1(dt8, rt), _mx(dq8, rq)
        print(f"fp8 bwd vs recipe shift={shift} heads={heads} {store} ws={workspace}: dqkv L1 {e_q:.3e} max {e_mx:.3e} dtable L1 {e_t:.3e}; "
              f"bf16 bwd vs recipe: dqkv L1 {s_q:.3e} dtable L1 {s_t:.3e}")
        assert bool(torch.isfinite(dq8.float()).all()) and bool(torch.isfinite(dt8).all())
        assert e_q < bound and e_t < bound and e_mx < MAX_BOUND, (workspace, e_q, e_t, e_mx)
        # the zero-dO tile (window 1, head 0) has a zero gradient, and so have dq / dk of the zero-v tile (window 2, last head)
        g8 = _partition(dq8.float(), I, H, shift)
        assert float(g8[1, :, 0:32].abs().max()) == 0.0 and float(g8[1, :, C:C + 32].abs().max()) == 0.0
        assert float(g8[1, :, 2 * C:2 * C + 32].abs().max()) == 0.0
        hl = 32 * (heads - 1)
        assert float(g8[2, :, hl:hl + 32].abs().max()) == 0.0 and float(g8[2, :, C + hl:C + hl + 32].abs().max()) == 0.0
    assert s_q > SEPARATION * bound and s_t > SEPARATION * bound, (s_q, s_t)


@pytest.mark.parametrize("store", ["f32", "bf16"])
@pytest.mark.parametrize("H,heads,shift", [(14, 3, 3), (28, 8, 0), (7, 32, 0)])
def test_fp8_full_forward_is_the_fp8_forward(dev, store, H, heads, shift):
    g = torch.Generator().manual_seed(H + heads)
    I, C = 3, heads * 32
    dt = torch.bfloat16 if store == "bf16" else torch.float32
    act = hip.BF16 if store == "bf16" else hip.F32
    qkv = torch.randn(I * H * H, 3 * C, generator=g).to(dt).to(dev)
    table = (0.5 * torch.randn(169, heads, generator=g)).to(dev)
    outs = []
    for m in (hip.MATH_FP8, hip.MATH_FP8_FULL):
        out = torch.full((I * H * H, C), float("nan"), dtype=dt, device=dev)
        call("sv_window_attention_fwd", ptr(qkv), ptr(table), ptr(out), I, H, H, C, heads, shift, m, act=act)
        outs.append(out.cpu())
    assert bool(torch.isfinite(outs[0].float()).all())
    assert torch.equal(outs[0].view(torch.int16 if store == "bf16" else torch.int32), outs[1].view(torch.int16 if store == "bf16" else torch.int32))


def test_host_switch():
    ops.set_math("bf16")
    ops.set_storage("bf16")
    try:
        assert ops.attention_bwd_math() == hip.MATH_BF16 and ops.fused_attn_block_bwd_enabled(96, 3)
        S.set_attention_fp8(True)                  # forward only: exactly today's behaviour
        assert ops.attention_math() == hip.MATH_FP8
        assert ops.attention_bwd_math() == hip.MATH_BF16 and ops.fused_attn_block_bwd_enabled(96, 3)
        S.set_attention_fp8(True, backward=True)
        assert ops.attention_math() == hip.MATH_FP8 and ops.attention_bwd_math() == hip.MATH_FP8_FULL
        assert not ops.fused_attn_block_bwd_enabled(96, 3)
        S.set_attention_fp8(False)
        assert ops.attention_bwd_math() == hip.MATH_BF16 and ops.fused_attn_block_bwd_enabled(96, 3)
        S.set_attention_fp8(True, backward=True)
        ops.set_math("f32")                        # fp8 needs bf16 math: under f32 math both calls stay exact fp32
        assert ops.attention_math() == hip.MATH_F32 and ops.attention_bwd_math() == hip.MATH_F32
    finally:
        S.set_attention_fp8(False)
        ops.set_math("f32")


def _attn_param_names(enc):
    return [n for n, _ in enc.named_parameters()
            if ".attn." in n and n.split(".")[-2] in ("qkv", "proj") or n.endswith("relative_position_bias_table")]


def test_swin_b_encoder_train_step_modes(dev):
    """Swin-B encoder (goldens weights, B = 1 x V = 2, bf16 storage): one train step in bf16, fp8-forward and fp8-forward+backward mode
    against the exact-fp32 HIP gradient of the same weights and images.  Every gradient is finite; the fp8-full gradients differ from the
    fp8-forward ones (the new kernel ran); the window-attention parameter gradients (qkv, proj, relative_position_bias_table) stay within
    GRAD_FACTOR of the bf16 path's own L1-relative distance from exact fp32."""
    import json
    import os
    from swinvox_amd import goldens
    from swinvox_amd.models import Encoder
    gdir = os.path.join(os.path.dirname(__file__), "golden")
    case = json.load(open(os.path.join(gdir, "manifest.json")))["cases"]["swin_b_B1_V2"]
    enc = Encoder(S.default_cfg(), variant="base")
    goldens.seeded_fill_(enc, case["weights_seed"])
    enc.to(dev).train()
    enc.stochastic = False
    x = goldens.synth_images(1, 2, case["seed"]).to(dev)
    names = _attn_param_names(enc)
    assert len(names) >= 24 * 3
    grads = {}
    try:
        for mode in ("f32", "bf16", "fp8", "fp8_full"):
            S.set_math("f32" if mode == "f32" else "bf16")
            if mode != "f32":
                S.set_storage("bf16")
            S.set_attention_fp8(mode.startswith("fp8"), backward=mode == "fp8_full")
            enc.zero_grad(set_to_none=True)
            enc(x).float().square().mean().backward()
            torch.cuda.synchronize()
            grads[mode] = {n: p.grad.detach().float().cpu() for n, p in enc.named_parameters() if p.grad is not None}
    finally:
        S.set_attention_fp8(False)
        S.set_math("f32")
    for mode, gm in grads.items():
        assert all(bool(torch.isfinite(t).all()) for t in gm.values()), mode
    ref = grads["f32"]
    stats = {}
    for mode in ("bf16", "fp8", "fp8_full"):
        errs = sorted(((_l1(grads[mode][n], ref[n]), n) for n in names), reverse=True)
        stats[mode] = (errs[0][0], errs[len(errs) // 2][0])
        print(f"{mode}: window-attention parameter gradients vs exact fp32, L1-rel worst {errs[:3]}, median {stats[mode][1]:.3e}")
    assert any(not torch.equal(grads["fp8"][n], grads["fp8_full"][n]) for n in names)
    # The bound is stated against the bf16 path's own distance from exact fp32 on this weight set.  Measured (one run): worst / median
    # L1-relative 1.074 / 0.908 for bf16, 1.072 / 0.910 for fp8-full - 24 blocks of bf16 storage already move these gradients by about
    # their own size, and the recipe's ~6 % on the attention core disappears inside that.  GRAD_FACTOR: the fp8 backward may not add more
    # than a quarter to it, worst parameter and median alike.
    for k in (0, 1):
        assert stats["fp8_full"][k] <= GRAD_FACTOR * stats["bf16"][k], stats


GRAD_FACTOR = 1.25


def test_training_smoke_fp8_full(dev):
    """Whole pipeline, Swin-T, B = 2 x V = 2, one fixed batch, 20 flat-Adam steps in bf16 and in fp8-full mode: the fp8-full loss falls,
    stays finite and ends within LOSS_FACTOR of the bf16 run's final loss.  Float atomics make neither run bit-reproducible, and the fp8
    gradient's extra noise shows as single-step bumps under Adam: two measured runs ended at 0.6063 / 0.5998 (ratio 1.01) and
    0.7631 / 0.6062 (1.26, a bump in the last step, after 0.6244 one step before).  So the mean of the last five steps, the stable
    statistic (ratios 1.01 and 1.07 in those runs), must stay within TAIL_FACTOR, and the final loss within LOSS_FACTOR."""
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
    for mode in ("bf16", "fp8_full"):
        torch.manual_seed(0)
        nets = [Encoder(cfg), Decoder(cfg), Merger(cfg), Refiner(cfg)]
        for n in nets:
            O.seeded_weights_(n, seed=7)
            n.to(dev).train()
        solvers, _ = harness.make_solvers(nets, cfg)
        S.set_math("bf16")
        S.set_storage("bf16")
        S.set_attention_fp8(mode == "fp8_full", backward=True)
        try:
            losses = []
            for _ in range(20):
                el, rl = harness.train_step(nets, solvers, cfg, x, gt)
                losses.append(float(el + rl))
        finally:
            S.set_attention_fp8(False)
            S.set_math("f32")
        print(f"{mode}: losses {[round(v, 4) for v in losses]}")
        assert all(np.isfinite(losses)) and losses[-1] < losses[0], (mode, losses)
        final[mode] = (losses[-1], sum(losses[-5:]) / 5)
    assert final["fp8_full"][0] < LOSS_FACTOR * final["bf16"][0], final
    assert final["fp8_full"][1] < TAIL_FACTOR * final["bf16"][1], final


LOSS_FACTOR = 1.5
TAIL_FACTOR = 1.15
