"""Fused attention branch of a stage-0 Swin block (csrc/attn.hip: sv_swin_attn_block_fwd) against
 (a) a plain PyTorch fp32 reference of x1 = x + s * proj(window_attention(qkv(LayerNorm(x)))) - timm SwinTransformerBlock._attn + the
     residual / DropPath of its forward(), models/swin_transformer.py:78 - built from the oracle's index / mask helpers, and
 (b) the unfused kernel chain (sv_layernorm_fwd -> engine linear -> sv_window_attention_fwd -> engine linear with the residual epilogue),
     whose stored tensors (LayerNorm output + statistics, qkv, head outputs) the fused kernel reproduces as side outputs for the backward.
Inputs are bf16-representable; the kernel rounds to bf16 exactly where the unfused chain stores, so (b) agrees to bf16 rounding of single
elements and (a) to the bf16 tolerance of tests/test_gpu_bf16_storage.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from swinvox_amd import hip, ops  # noqa: E402
from swinvox_amd.hip import call, ptr  # noqa: E402
from swinvox_amd.ops import ConvSpec  # noqa: E402

C, HEADS = 96, 3


def _bf(t):
    return t.to(torch.bfloat16).float()


def _case(I, H, seed):
    g = torch.Generator().manual_seed(seed)
    M = I * H * H
    p = {
        "x": _bf(torch.randn(M, C, generator=g) * 1.5 + 0.2),
        "lg": 1 + 0.1 * torch.randn(C, generator=g), "lb": 0.1 * torch.randn(C, generator=g),
        "wqkv": torch.randn(3 * C, C, generator=g) / C ** 0.5, "bqkv": 0.1 * torch.randn(3 * C, generator=g),
        "table": 0.5 * torch.randn(169, HEADS, generator=g),
        "wproj": torch.randn(C, C, generator=g) / C ** 0.5, "bproj": 0.1 * torch.randn(C, generator=g),
    }
    return p


def _reference(p, I, H, shift, sc):
    from oracle.model import rel_pos_index, shift_attn_mask
    x = p["x"].double()
    ln = torch.nn.functional.layer_norm(x, (C,), p["lg"].double(), p["lb"].double(), 1e-5)
    qkv = ln @ p["wqkv"].double().T + p["bqkv"].double()
    t = qkv.view(I, H, H, 3 * C)
    if shift:
        t = torch.roll(t, (-shift, -shift), (1, 2))
    tw = t.view(I, H // 7, 7, H // 7, 7, 3 * C).permute(0, 1, 3, 2, 4, 5).reshape(-1, 49, 3, HEADS, 32).permute(2, 0, 3, 1, 4)
    q, k, v = tw[0] * 32 ** -0.5, tw[1], tw[2]
    a = q @ k.transpose(-2, -1) + p["table"].double()[rel_pos_index(7).reshape(-1)].view(49, 49, HEADS).permute(2, 0, 1)[None]
    if shift:
        m = shift_attn_mask(H, H, 7, shift).double()
        a = (a.view(I, -1, HEADS, 49, 49) + m[None, :, None]).view(-1, HEADS, 49, 49)
    o = (a.softmax(-1) @ v).transpose(1, 2).reshape(-1, 49, C)
    o = o.view(I, H // 7, H // 7, 7, 7, C).permute(0, 1, 3, 2, 4, 5).reshape(I, H, H, C)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    att = o.reshape(-1, C)
    y = att @ p["wproj"].double().T + p["bproj"].double()
    s = torch.ones(I, dtype=torch.float64) if sc is None else sc.double()
    x1 = x + s.repeat_interleave(H * H)[:, None] * y
    return {"x1": x1.float(), "ln1": ln.float(), "qkv": qkv.float(), "att": att.float()}


def _fused(d, I, H, shift, scd, side):
    dev = d["x"].device
    M = I * H * H
    b16 = dict(dtype=torch.bfloat16, device=dev)
    x1 = torch.empty(M, C, **b16)
    ln1 = qkv = att = m1 = r1 = None
    if side:
        ln1, qkv, att = torch.empty(M, C, **b16), torch.empty(M, 3 * C, **b16), torch.empty(M, C, **b16)
        m1, r1 = torch.empty(M, device=dev), torch.empty(M, device=dev)
    call("sv_swin_attn_block_fwd", ptr(d["x"]), ptr(d["lg"]), ptr(d["lb"]), ptr(d["wqkv"]), ptr(d["bqkv"]), ptr(d["table"]), ptr(d["wproj"]),
         ptr(d["bproj"]), ptr(scd), ptr(x1), ptr(ln1), ptr(m1), ptr(r1), ptr(qkv), ptr(att), I, H, H, C, HEADS, shift, 1e-5, act=hip.BF16)
    torch.cuda.synchronize()
    return {"x1": x1, "ln1": ln1, "qkv": qkv, "att": att, "mean": m1, "rstd": r1}


def _unfused(d, I, H, shift, scd):
    """the kernel chain block_forward() runs when the fused kernel is switched off"""
    M = I * H * H
    x = d["x"]
    ln1, m1, r1 = ops.layernorm_fwd(x, d["lg"], d["lb"], M, C)
    s_qkv, s_proj = ConvSpec.linear(C, 3 * C), ConvSpec.linear(C, C)
    qkv = ops.empty(M, 3 * C, like=x)
    ops.linear_fwd(ln1, M, s_qkv, d["wqkv"], qkv, bias=d["bqkv"])
    att = ops.empty(M, C, like=x)
    call("sv_window_attention_fwd", ptr(qkv), ptr(d["table"]), ptr(att), I, H, H, C, HEADS, shift, hip.MATH_BF16)
    x1 = ops.empty(M, C, like=x)
    ops.linear_fwd(att, M, s_proj, d["wproj"], x1, bias=d["bproj"], residual=x, ldr=C, row_scale=scd, rows_per_scale=H * H)
    torch.cuda.synchronize()
    return {"x1": x1, "ln1": ln1, "qkv": qkv, "att": att, "mean": m1, "rstd": r1}


# (I, H) of the cases that run the kernels at several windows per window group (sv_swin_attn_block_windows_per_group >= 2): the window loop,
# its prefetch and the sums carried across windows exist only there.  (58, 21): 522 windows - the forward's last workgroup has an empty
# second group; (9, 56): 576 windows.
SEVERAL_WINDOWS = {(9, 56), (58, 21)}


def _share(I, H, backward):
    s = hip.load().sv_swin_attn_block_windows_per_group(I, H, H, int(backward))
    assert s >= 1, (s, I, H, backward)
    return s


def _image_slices(I, H, backward):
    """consecutive image ranges (i0, n), each as long as the kernel still runs it at one window per group"""
    n = next(n for n in range(I, 0, -1) if _share(n, H, backward) == 1)
    parts = [(i0, min(n, I - i0)) for i0 in range(0, I, n)]
    assert len(parts) >= 2 and all(_share(m, H, backward) == 1 for _, m in parts), parts
    return parts


def _rows(t, H, i0, n):
    return None if t is None else t[i0 * H * H:(i0 + n) * H * H]


def _rel(a, b):
    a, b = a.detach().float().cpu().double(), b.detach().float().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


@pytest.mark.parametrize("I,H,shift,with_scale", [(2, 14, 0, False), (3, 14, 3, True), (1, 28, 3, False), (5, 7, 0, True), (40, 14, 3, True),
                                                   (9, 56, 3, True), (58, 21, 3, True)])
def test_fused_attention_branch_matches_torch_and_the_unfused_chain(dev, I, H, shift, with_scale):
    share, windows = _share(I, H, False), I * (H // 7) ** 2
    assert (share >= 2) == ((I, H) in SEVERAL_WINDOWS), (share, I, H)
    if (I, H) == (58, 21):
        assert 0 < windows % (2 * share) <= share            # the second window group of the last workgroup has nothing to do
    assert hip.load().sv_swin_attn_block_supported(C, HEADS, hip.BF16, hip.MATH_BF16) == 1
    assert hip.load().sv_swin_attn_block_supported(192, 6, hip.BF16, hip.MATH_BF16) == 0
    p = _case(I, H, 7 * I + H + shift)
    sc = torch.tensor([0.0 if i % 3 == 1 else 1.0 / 0.9 for i in range(I)]) if with_scale else None
    ref = _reference(p, I, H, shift, sc)
    d = {k: (v.to(torch.bfloat16) if k == "x" else v).to(dev).contiguous() for k, v in p.items()}
    scd = sc.to(dev) if sc is not None else None
    got = _fused(d, I, H, shift, scd, side=True)
    # (a) against fp32 torch: bf16 operands and bf16-stored intermediates
    for k, tol in (("ln1", 1e-2), ("qkv", 1.5e-2), ("att", 2e-2), ("x1", 2e-2)):
        assert _rel(got[k], ref[k]) < tol, (k, _rel(got[k], ref[k]))
    # the inference form (no side outputs) is the same arithmetic
    lean = _fused(d, I, H, shift, scd, side=False)
    assert torch.equal(lean["x1"], got["x1"])
    if share >= 2:
        # the same images at one window per group, bit for bit: a window's rows are written by one group and must not depend on the
        # iteration of the window loop that computed them
        for i0, n in _image_slices(I, H, False):
            one = _fused(dict(d, x=_rows(d["x"], H, i0, n)), n, H, shift, scd[i0:i0 + n] if scd is not None else None, side=True)
            for k in ("x1", "qkv", "att", "ln1"):
                assert torch.equal(_rows(got[k], H, i0, n), one[k]), (k, i0, n)
    # (b) against the unfused chain in bf16 math + bf16 storage: every tensor the backward reads
    ops.set_math("bf16")
    ops.set_storage("bf16")
    try:
        un = _unfused(d, I, H, shift, scd)
    finally:
        ops.set_math("f32")
    assert _rel(got["mean"], un["mean"]) < 1e-5 and _rel(got["rstd"], un["rstd"]) < 1e-5
    for k, tol in (("ln1", 8e-3), ("qkv", 8e-3), ("att", 1.2e-2), ("x1", 1.2e-2)):     # a bf16 ulp of the largest element is 2^-8 = 3.9e-3
        assert _rel(got[k], un[k]) < tol, (k, _rel(got[k], un[k]))
        frac = float((got[k].float() != un[k].float()).float().mean())
        assert frac < 0.2, (k, frac)               # differing summation order flips the rounding of a minority of the elements


def _reference_grads(p, I, H, shift, sc, dx1):
    """fp64 autograd of the branch on the same (bf16-representable) inputs: gradients wrt x, norm1 weight / bias, the bias table, and the
    gradient that reaches the qkv rows"""
    from oracle.model import rel_pos_index, shift_attn_mask
    x = p["x"].double().requires_grad_(True)
    lg, lb = p["lg"].double().requires_grad_(True), p["lb"].double().requires_grad_(True)
    table = p["table"].double().requires_grad_(True)
    ln = torch.nn.functional.layer_norm(x, (C,), lg, lb, 1e-5)
    qkv = ln @ p["wqkv"].double().T + p["bqkv"].double()
    qkv.retain_grad()
    t = qkv.view(I, H, H, 3 * C)
    if shift:
        t = torch.roll(t, (-shift, -shift), (1, 2))
    tw = t.view(I, H // 7, 7, H // 7, 7, 3 * C).permute(0, 1, 3, 2, 4, 5).reshape(-1, 49, 3, HEADS, 32).permute(2, 0, 3, 1, 4)
    q, k, v = tw[0] * 32 ** -0.5, tw[1], tw[2]
    a = q @ k.transpose(-2, -1) + table[rel_pos_index(7).reshape(-1)].view(49, 49, HEADS).permute(2, 0, 1)[None]
    if shift:
        m = shift_attn_mask(H, H, 7, shift).double()
        a = (a.view(I, -1, HEADS, 49, 49) + m[None, :, None]).view(-1, HEADS, 49, 49)
    o = (a.softmax(-1) @ v).transpose(1, 2).reshape(-1, 49, C)
    o = o.view(I, H // 7, H // 7, 7, 7, C).permute(0, 1, 3, 2, 4, 5).reshape(I, H, H, C)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    y = o.reshape(-1, C) @ p["wproj"].double().T + p["bproj"].double()
    s = torch.ones(I, dtype=torch.float64) if sc is None else sc.double()
    x1 = x + s.repeat_interleave(H * H)[:, None] * y
    x1.backward(dx1.double())
    return {"dx": x.grad.float(), "dqkv": qkv.grad.float(), "dgamma": lg.grad.float(), "dbeta": lb.grad.float(), "dtable": table.grad.float()}


def _fused_bwd(d, fw, dx1, I, H, shift, scd):
    dev = dx1.device
    M = I * H * H
    b16 = dict(dtype=torch.bfloat16, device=dev)
    dqkv, dx = torch.empty(M, 3 * C, **b16), torch.empty(M, C, **b16)
    dbr = torch.empty(M, C, **b16) if scd is not None else None
    dg, db, dt = torch.zeros(C, device=dev), torch.zeros(C, device=dev), torch.zeros(169, HEADS, device=dev)
    ws = torch.zeros(int(hip.load().sv_window_attention_bwd_workspace_floats(HEADS)), device=dev)
    call("sv_swin_attn_block_bwd", ptr(dx1), ptr(fw["qkv"]), ptr(d["x"]), ptr(fw["mean"]), ptr(fw["rstd"]), ptr(d["lg"]), ptr(d["wqkv"]), ptr(d["wproj"]),
         ptr(d["table"]), ptr(scd), ptr(dqkv), ptr(dx), ptr(dbr), ptr(dg), ptr(db), ptr(dt), ptr(ws), I, H, H, C, HEADS, shift, act=hip.BF16)
    torch.cuda.synchronize()
    return {"dx": dx, "dqkv": dqkv, "dgamma": dg, "dbeta": db, "dtable": dt, "dbr": dbr}


def _unfused_bwd(d, fw, dx1, I, H, shift, scd):
    """the four-kernel data path of _attention_backward() when the fused backward is switched off"""
    M = I * H * H
    x = d["x"]
    s_qkv, s_proj = ConvSpec.linear(C, 3 * C), ConvSpec.linear(C, C)
    dx = dx1.clone()
    dbr = dx
    if scd is not None:
        dbr = ops.empty(M, C, like=x)
        call("sv_rowscale", ptr(dx), ptr(scd), ptr(dbr), M, C, H * H)
    datt = ops.empty(M, C, like=x)
    ops.linear_dgrad(dbr, M, s_proj, s_proj.pack_dgrad(d["wproj"]), datt)
    dqkv = ops.empty(M, 3 * C, like=x)
    dt = torch.zeros(169, HEADS, device=x.device)
    ws = ops.zeros_f64(8 * 169 * HEADS, x.device)
    call("sv_window_attention_bwd", ptr(fw["qkv"]), ptr(d["table"]), ptr(datt), ptr(dqkv), ptr(dt), ptr(ws), I, H, H, C, HEADS, shift, hip.MATH_BF16)
    dln1 = ops.empty(M, C, like=x)
    ops.linear_dgrad(dqkv, M, s_qkv, s_qkv.pack_dgrad(d["wqkv"]), dln1)
    dg, db = torch.zeros(C, device=x.device), torch.zeros(C, device=x.device)
    ops.layernorm_bwd(dln1, x, d["lg"], fw["mean"], fw["rstd"], dx, dg, db, M, C, accumulate_dx=True)
    torch.cuda.synchronize()
    return {"dx": dx, "dqkv": dqkv, "dgamma": dg, "dbeta": db, "dtable": dt}


@pytest.mark.parametrize("I,H,shift,with_scale", [(2, 14, 0, False), (3, 14, 3, True), (1, 28, 3, False), (5, 7, 0, True), (40, 14, 3, True), (9, 56, 3, True),
                                                   (58, 21, 3, True)])
def test_fused_attention_branch_backward(dev, I, H, shift, with_scale):
    """sv_swin_attn_block_bwd (dx1 -> projection data gradient -> attention backward -> qkv data gradient -> LayerNorm backward + residual in
    one kernel) against (a) fp64 autograd of the branch and (b) the unfused four-kernel chain on the same stored tensors: dx, dqkv, the
    LayerNorm parameter gradients and the bias-table gradient."""
    share = _share(I, H, True)
    assert (share >= 2) == ((I, H) in SEVERAL_WINDOWS), (share, I, H)
    p = _case(I, H, 11 * I + H + shift)
    sc = torch.tensor([0.0 if i % 3 == 1 else 1.0 / 0.9 for i in range(I)]) if with_scale else None
    g = torch.Generator().manual_seed(I + H)
    dx1_f = _bf(torch.randn(I * H * H, C, generator=g))
    ref = _reference_grads(p, I, H, shift, sc, dx1_f)
    d = {k: (v.to(torch.bfloat16) if k == "x" else v).to(dev).contiguous() for k, v in p.items()}
    scd = sc.to(dev) if sc is not None else None
    dx1 = dx1_f.to(torch.bfloat16).to(dev)
    fw = _fused(d, I, H, shift, scd, side=True)
    got = _fused_bwd(d, fw, dx1, I, H, shift, scd)
    # (a) fp64 autograd: bf16 operands, bf16-stored qkv / dqkv / datt / dln1
    for k, tol in (("dx", 2.5e-2), ("dqkv", 2.5e-2), ("dgamma", 2e-2), ("dbeta", 2e-2), ("dtable", 2e-2)):
        assert _rel(got[k], ref[k]) < tol, (k, _rel(got[k], ref[k]))
    if scd is not None:
        assert torch.equal(got["dbr"].float(), (dx1.float() * scd.repeat_interleave(H * H)[:, None]).to(torch.bfloat16).float())
    if share >= 2:
        # the same images at one window per workgroup, bit for bit (dqkv and dx rows are written by one workgroup, no atomics)
        for i0, n in _image_slices(I, H, True):
            fw1 = {k: _rows(fw[k], H, i0, n) for k in ("qkv", "mean", "rstd")}
            one = _fused_bwd(dict(d, x=_rows(d["x"], H, i0, n)), fw1, _rows(dx1, H, i0, n), n, H, shift, scd[i0:i0 + n] if scd is not None else None)
            for k in ("dqkv", "dx"):
                assert torch.equal(_rows(got[k], H, i0, n), one[k]), (k, i0, n)
    # (b) the unfused chain in bf16 math + bf16 storage
    ops.set_math("bf16")
    ops.set_storage("bf16")
    try:
        un = _unfused_bwd(d, fw, dx1, I, H, shift, scd)
    finally:
        ops.set_math("f32")
    for k, tol in (("dx", 1.5e-2), ("dqkv", 1.5e-2), ("dgamma", 1e-2), ("dbeta", 1e-2), ("dtable", 1e-2)):
        assert _rel(got[k], un[k]) < tol, (k, _rel(got[k], un[k]))


def test_fused_attention_branch_rejects_bad_arguments(dev):
    z = torch.zeros(2 * 196, 96, dtype=torch.bfloat16, device=dev)
    f = torch.zeros(3 * 96 * 96, device=dev)
    args = [ptr(z), ptr(f), ptr(f), ptr(f), ptr(f), ptr(f), ptr(f), ptr(f), None, ptr(z)]
    with pytest.raises(RuntimeError, match="swin_attn_block"):
        call("sv_swin_attn_block_fwd", *args, None, None, None, None, None, 2, 14, 14, 192, 6, 0, 1e-5, act=hip.BF16)     # unsupported width
    with pytest.raises(RuntimeError, match="swin_attn_block"):
        call("sv_swin_attn_block_fwd", *args, ptr(z), None, None, None, None, 2, 14, 14, 96, 3, 0, 1e-5, act=hip.BF16)   # partial side outputs
    with pytest.raises(RuntimeError, match="swin_attn_block"):
        call("sv_swin_attn_block_fwd", *args, None, None, None, None, None, 2, 14, 14, 96, 3, 0, 1e-5, act=hip.F32)      # fp32 token rows
    with pytest.raises(RuntimeError, match="swin_attn_block"):
        call("sv_swin_attn_block_fwd", *args, None, None, None, None, None, 2, 15, 14, 96, 3, 0, 1e-5, act=hip.BF16)     # not a multiple of 7
    bargs = [ptr(z)] * 3 + [ptr(f)] * 6 + [None, ptr(z), ptr(z), None, ptr(f), ptr(f), ptr(f), ptr(f)]
    with pytest.raises(RuntimeError, match="swin_attn_block"):
        call("sv_swin_attn_block_bwd", *bargs, 2, 14, 14, 192, 6, 0, act=hip.BF16)                                         # unsupported width
    with pytest.raises(RuntimeError, match="swin_attn_block"):
        call("sv_swin_attn_block_bwd", *bargs, 2, 14, 14, 96, 3, 0, act=hip.F32)                                           # fp32 token rows


def test_encoder_step_with_and_without_the_fused_branch(dev):
    """The benchmarked mode (bf16 MFMA + bf16 storage), Encoder forward + backward on the same images and weights with the fused attention
    branch switched on and off (ops.set_fused_attn_block): features and every parameter gradient must agree to the bf16 noise of two
    summation orders - the fused forward stores the tensors the unfused backward reads, so the backward is the same launches either way -
    and the no-grad (inference) form, which skips those tensors, must give the same features as the training form."""
    import swinvox_amd as S
    from swinvox_amd.models.encoder import Encoder
    torch.manual_seed(5)
    enc = Encoder(S.default_cfg()).to(dev).train()
    enc.stochastic = False                      # no dropout / drop-path: both runs see the same function
    g = torch.Generator().manual_seed(9)
    x = (torch.rand(2, 2, 3, 224, 224, generator=g) * 2 - 1).to(dev)
    res = {}
    ops.set_math("bf16")
    ops.set_storage("bf16")
    try:
        for fused in (True, False):
            ops.set_fused_attn_block(fused)
            ops.set_fused_attn_block_bwd(fused)
            assert ops.fused_attn_block_enabled(96, 3) == fused and ops.fused_attn_block_bwd_enabled(96, 3) == fused
            for p in enc.parameters():
                p.grad = None
            f = enc(x)
            f.square().mean().backward()
            torch.cuda.synchronize()
            res[fused] = (f.detach().float().cpu(), {n: p.grad.detach().float().cpu() for n, p in enc.named_parameters() if p.grad is not None})
        ops.set_fused_attn_block(True)
        with torch.no_grad():
            f_lean = enc(x).float().cpu()
    finally:
        ops.set_fused_attn_block(True)
        ops.set_fused_attn_block_bwd(True)
        ops.set_math("f32")
    (fa, ga), (fb, gb) = res[True], res[False]
    assert torch.isfinite(fa).all() and _rel(fa, fb) < 3e-2, _rel(fa, fb)
    assert set(ga) == set(gb)
    # L1-relative per parameter of the Swin backbone (what the switch touches), as tests/test_gpu_modules.py bounds bf16 gradients.  (The
    # convolution biases in front of the train-mode BatchNorms elsewhere in the encoder have a mathematically zero gradient - what
    # arrives there is the rounding noise of either run and says nothing.)
    names = [n for n in ga if n.startswith("swin_transformer.")]
    assert len(names) > 100
    errs = sorted(((float((ga[n] - gb[n]).abs().sum() / (gb[n].abs().sum() + 1e-20)), n) for n in names), reverse=True)
    print("largest bf16 A/B gradient deviations:", errs[:5])
    # measured: 0.19 at most (LayerNorm parameters of stage 2).  The seeded default-init weights amplify bf16 rounding - the CPU oracle under
    # torch.autocast(bfloat16) is ~40 % off its own fp32 features (tests/test_gpu_modules.py::test_bf16_math, which bounds bf16 gradients by
    # 30 % L1 for the same reason) - so two bf16 runs that differ in the rounding of single stage-0 elements drift apart by this much;
    # a wrong or missing saved tensor shows as a deviation of order 1.
    assert errs[0][0] < 0.3, errs[:5]
    # train-mode BatchNorm uses batch statistics in both forms, so the inference form differs from the training form only by the skipped stores
    assert _rel(f_lean, fa) < 3e-2, _rel(f_lean, fa)
