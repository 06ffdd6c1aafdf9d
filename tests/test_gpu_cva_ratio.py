"""Cross-view attention at every ATT_SPATIAL_DOWNSAMPLE_RATIO the module runs (1, 2, 4 ... 7; reference models/cross_view_attention.py:
26-34,67-73,81-105,110-120) and over the reference's search space of CROSS_ATT_REDUCTION_RATIO x CROSS_ATT_NUM_HEADS in {2, 4, 8}^2
(head_dim 8 ... 128).  Ratios 4 ... 7 give a 1x1 token grid: the r x r / stride r depth-wise conv reads the top-left r x r positions,
the attention sees one position per view, and the bilinear 1x1 -> 7x7 up-sampling is a broadcast.

  * the four sv_cva_* entry points against torch (F.conv2d / F.interpolate + autograd), fp32 and bf16 storage
  * ratio 2 through sv_cva_* is bit-identical to the sv_dwconv2x2_* / sv_upsample3to7_* entry points (the benchmarked path)
  * cva_forward / cva_backward against oracle.CrossViewAttention (CPU fp32 autograd): output, dx and every parameter gradient
  * whole train steps at ratio 4 and 7 against the oracle, with the protocol of test_gpu_configs.py
  * refusals: ratio 3 and >= 8 at the entry points, ratio 8 in the Encoder"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402
import swinvox_amd as S  # noqa: E402
from swinvox_amd import hip, ops  # noqa: E402
from swinvox_amd.losses import bce_with_logits as bce  # noqa: E402
from swinvox_amd.models import Decoder, Encoder, Merger, Refiner  # noqa: E402
from swinvox_amd.models._base import GradStore  # noqa: E402
from swinvox_amd.models.cross_view_attention import CrossViewAttention  # noqa: E402
from swinvox_amd.ops import call, ptr  # noqa: E402

RATIOS = (2, 4, 5, 6, 7)          # the ratios the sv_cva_* entry points accept
TOL_F32 = 1e-5                    # kernels vs torch, fp32 storage: relative to max|ref|
TOL_BF16 = 1.2e-2                 # kernels vs torch on bf16-rounded inputs, bf16 storage: ~3 bf16 ulps of max|ref|
CHAIN_TOL = 1e-4                  # cva chain vs oracle, exact-fp32 math: relative to max(1, max|ref|)
CHAIN_L1_BF16 = 3e-2              # cva chain vs oracle, bf16 math + bf16 storage: sum|a - b| / sum|b|


def grid(r):
    return (7 - r) // r + 1


def rel(a, b):
    a, b = a.detach().float().cpu().double(), b.detach().float().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def l1rel(a, b):
    a, b = a.detach().float().cpu().double(), b.detach().float().cpu().double()
    return float((a - b).abs().sum() / (b.abs().sum() + 1e-30))


def rows(t):
    """[N, C, 7, 7] or [N, C, g, g] -> channels-last rows [N*h*w, C]"""
    n, c = t.shape[:2]
    return t.reshape(n, c, -1).transpose(1, 2).reshape(-1, c).contiguous()


class _Storage:
    """fp32 storage (exact-fp32 math) or bf16 storage (bf16 math) for the duration of a block"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        ops.set_math("bf16" if self.mode == "bf16" else "f32")
        ops.set_storage(self.mode)
        return torch.bfloat16 if self.mode == "bf16" else torch.float32

    def __exit__(self, *exc):
        ops.set_math("f32")


def _spatial_case(g, r, I, C, q):
    """torch reference of the spatial path: small = conv(x), up = interpolate(small) + x, with autograd"""
    x = q(torch.randn(I, C, 7, 7, generator=g)).requires_grad_(True)
    w = q(torch.randn(C, 1, r, r, generator=g) / r).requires_grad_(True)
    b = q(torch.randn(C, generator=g)).requires_grad_(True)
    small = F.conv2d(x, w, b, stride=r, groups=C)
    sm_in = q(torch.randn(small.shape, generator=g)).requires_grad_(True)      # independent input of the up-sampling
    up = F.interpolate(sm_in, size=(7, 7), mode="bilinear", align_corners=False) + x
    dsmall = q(torch.randn(small.shape, generator=g))
    dup = q(torch.randn(up.shape, generator=g))
    torch.autograd.backward([small, up], [dsmall, dup])
    return x, w, b, small, sm_in, up, dsmall, dup


def _run_spatial(dev, dt, r, I, C, x, w, b, sm_in, dsmall, dup):
    gg = grid(r) ** 2
    A = lambda t: rows(t.detach()).to(dev).to(dt)                              # noqa: E731
    xd, wd, bd = A(x), w.detach().to(dev), b.detach().to(dev)
    y = ops.empty(I * gg, C, device=dev)
    call("sv_cva_downsample_fwd", ptr(xd), ptr(wd), ptr(bd), ptr(y), I, C, r)
    up = ops.empty(I * 49, C, device=dev)
    sd = A(sm_in)
    call("sv_cva_upsample_add_fwd", ptr(sd), ptr(xd), C, ptr(up), I, C, r)
    dupd, dsd = A(dup), A(dsmall)
    dsm = ops.empty(I * gg, C, device=dev)
    call("sv_cva_upsample_bwd", ptr(dupd), ptr(dsm), I, C, r)
    dx = ops.empty(I * 49, C, device=dev)
    dw, db = ops.fzeros(C, 1, r, r, device=dev), ops.fzeros(C, device=dev)
    call("sv_cva_downsample_bwd", ptr(dsd), ptr(xd), ptr(wd), ptr(dx), ptr(dw), ptr(db), I, C, r)
    torch.cuda.synchronize()
    return y, up, dsm, dx.float() + dupd.float(), dw, db


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("r", RATIOS)
def test_spatial_kernels_match_torch(dev, r, storage):
    q = (lambda t: t.bfloat16().float()) if storage == "bf16" else (lambda t: t)
    tol = TOL_BF16 if storage == "bf16" else TOL_F32
    for I in (3, 17):
        for C in (24, 512):
            g = torch.Generator().manual_seed(1000 * r + 10 * I + C)
            x, w, b, small, sm_in, up, dsmall, dup = _spatial_case(g, r, I, C, q)
            with _Storage(storage) as dt:
                y, upo, dsm, dx, dw, db = _run_spatial(dev, dt, r, I, C, x, w, b, sm_in, dsmall, dup)
            errs = dict(y=rel(y, rows(small)), up=rel(upo, rows(up)), dsmall=rel(dsm, rows(sm_in.grad)), dx=rel(dx, rows(x.grad)),
                        dw=rel(dw, w.grad), db=rel(db, b.grad))
            assert all(e < tol for e in errs.values()), (I, C, errs)


def _ratio2_pair(dev, dt, I, C, seed):
    """every ratio-2 output through the sv_dwconv2x2_* / sv_upsample3to7_* entry points and through sv_cva_* at r = 2"""
    g = torch.Generator().manual_seed(seed)
    x, w, b = torch.randn(I * 49, C, generator=g), torch.randn(C, 1, 2, 2, generator=g), torch.randn(C, generator=g)
    dy9, small, dup = torch.randn(I * 9, C, generator=g), torch.randn(I * 9, C, generator=g), torch.randn(I * 49, C, generator=g)
    xd, dyd, sd, dupd = (t.to(dev).to(dt) for t in (x, dy9, small, dup))
    wd, bd = w.to(dev), b.to(dev)
    outs = []
    for new in (False, True):
        ra = (2,) if new else ()
        y = ops.empty(I * 9, C, device=dev)
        call("sv_cva_downsample_fwd" if new else "sv_dwconv2x2_fwd", ptr(xd), ptr(wd), ptr(bd), ptr(y), I, C, *ra)
        dx, dw, db = ops.empty(I * 49, C, device=dev), ops.fzeros(C, 1, 2, 2, device=dev), ops.fzeros(C, device=dev)
        call("sv_cva_downsample_bwd" if new else "sv_dwconv2x2_bwd", ptr(dyd), ptr(xd), ptr(wd), ptr(dx), ptr(dw), ptr(db), I, C, *ra)
        up = ops.empty(I * 49, C, device=dev)
        call("sv_cva_upsample_add_fwd" if new else "sv_upsample3to7_add_fwd", ptr(sd), ptr(xd), C, ptr(up), I, C, *ra)
        ds = ops.empty(I * 9, C, device=dev)
        call("sv_cva_upsample_bwd" if new else "sv_upsample3to7_bwd", ptr(dupd), ptr(ds), I, C, *ra)
        torch.cuda.synchronize()
        outs.append(dict(y=y.cpu(), dx=dx.cpu(), up=up.cpu(), ds=ds.cpu(), dw=dw.cpu(), db=db.cpu()))
    return outs


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_ratio2_is_bit_identical_to_the_2x2_entry_points(dev, storage):
    with _Storage(storage) as dt:
        # I = 1: one image slice, so the weight / bias gradients are one atomic onto zero and exact too
        old, new = _ratio2_pair(dev, dt, 1, 512, 7)
        for k in old:
            assert torch.equal(old[k], new[k]), (1, k)
        # I = 17: one slice per image, whose atomics land in any order: dw / db agree to fp32 summation order only
        old, new = _ratio2_pair(dev, dt, 17, 512, 8)
        for k in old:
            if k in ("dw", "db"):
                assert rel(new[k], old[k]) < 1e-6, (17, k)
            else:
                assert torch.equal(old[k], new[k]), (17, k)


# ------------------------------------------------------------------------------------------------------------------------------
# cva_forward / cva_backward against the oracle module
# ------------------------------------------------------------------------------------------------------------------------------
def _cfgs(ratio, red, heads):
    ocfg, pcfg = O.default_cfg(), S.default_cfg()
    for c in (ocfg, pcfg):
        c.NETWORK.ATT_SPATIAL_DOWNSAMPLE_RATIO = ratio
        c.NETWORK.CROSS_ATT_REDUCTION_RATIO = red
        c.NETWORK.CROSS_ATT_NUM_HEADS = heads
    return ocfg, pcfg


def _hip_cva(cva, x_rows, dout_rows, B, V):
    """one train-mode forward + backward of the kernel chain with the per-module pack cache and arenas _ModuleFn sets"""
    packs = cva.__dict__.setdefault("_packs", ops.PackCache())
    af, ab = cva.__dict__.setdefault("_arena_f", ops.ZeroArena()), cva.__dict__.setdefault("_arena_b", ops.ZeroArena())
    ops.set_pack_cache(packs)
    ops.set_arena(af)
    try:
        packs.refresh()
        af.begin(x_rows.device)
        out, ctx = cva.cva_forward(x_rows, B, V, True, False, None)
    finally:
        ops.bn_tick_flush()
        af.end()
        ops.set_arena(None)
    grads = GradStore(list(cva.parameters()))
    ops.set_arena(ab)
    try:
        ab.begin(x_rows.device)
        dx = cva.cva_backward(ctx, dout_rows, grads)
    finally:
        ab.end()
        ops.set_pack_cache(None)
        ops.set_arena(None)
    torch.cuda.synchronize()
    return out, dx, grads


def _chain_case(dev, ratio, red, heads, B, V):
    ocfg, pcfg = _cfgs(ratio, red, heads)
    o = O.CrossViewAttention(ocfg, 512)
    O.seeded_weights_(o, seed=70 + ratio)
    o.train()
    o.dropout.p = 0.0
    g = torch.Generator().manual_seed(100 * ratio + 10 * red + heads + 1000 * V)
    x = torch.randn(B, V, 512, 7, 7, generator=g)
    do = torch.randn(B, V, 512, 7, 7, generator=g)
    xo = x.clone().requires_grad_(True)
    yo = o(xo)
    yo.backward(do)
    ref = dict(out=rows(yo.detach().reshape(B * V, 512, 7, 7)), dx=rows(xo.grad.reshape(B * V, 512, 7, 7)))
    ref.update({k: p.grad for k, p in o.named_parameters()})
    p = CrossViewAttention(pcfg, 512)
    p.load_state_dict(o.state_dict())
    p.to(dev).train()
    p.dropout.p = 0.0
    res = {}
    for mode in ("f32", "bf16"):
        with _Storage(mode) as dt:
            xr = rows(x.reshape(B * V, 512, 7, 7)).to(dev).to(dt)
            dr = rows(do.reshape(B * V, 512, 7, 7)).to(dev).to(dt)
            out, dx, grads = _hip_cva(p, xr, dr, B, V)
            got = dict(out=out.float().cpu(), dx=dx.float().cpu())
            got.update({k: grads[q].cpu().clone() for k, q in p.named_parameters()})
        res[mode] = got
    return ref, res


SPACE = [(ratio, red, heads, 2, 3) for ratio in (1, 2, 4, 7) for red in (2, 4, 8) for heads in (2, 4, 8)]
SPACE += [(7, 2, 2, 2, 1), (4, 8, 8, 2, 24)]          # one view (softmax over 1 key), 24 views (V <= 32 in LDS)


@pytest.mark.parametrize("ratio,red,heads,B,V", SPACE, ids=lambda v: str(v))
def test_cva_chain_matches_the_oracle(dev, ratio, red, heads, B, V):
    ref, res = _chain_case(dev, ratio, red, heads, B, V)
    assert set(res["f32"]) == set(ref)                  # every parameter of the module has a gradient slot
    bad = {}
    for k, r in ref.items():
        e = float((res["f32"][k] - r).abs().max()) / max(1.0, float(r.abs().max()))
        # ffn.2 feeds a train-mode BatchNorm: its bias gradient is a column sum of B*V*49 terms that cancel to 0 in exact
        # arithmetic, so both sides hold summation noise that grows with the row count (2e-4 measured at 2352 rows)
        tol = max(CHAIN_TOL, 1e-6 * B * V * 49) if k == "ffn.2.bias" else CHAIN_TOL
        if not e <= tol:
            bad[k] = e
    assert not bad, ("f32", bad)
    # bf16 math + storage: output, dx and all parameter gradients together (the key bias gradient is zero in exact
    # arithmetic - the softmax over the keys ignores a per-row shift - so a per-tensor relative error means nothing there)
    b16 = res["bf16"]
    assert all(bool(torch.isfinite(t).all()) for t in b16.values())
    pk = [k for k in ref if k not in ("out", "dx")]
    errs = dict(out=l1rel(b16["out"], ref["out"]), dx=l1rel(b16["dx"], ref["dx"]),
                params=l1rel(torch.cat([b16[k].flatten() for k in pk]), torch.cat([ref[k].flatten() for k in pk])))
    assert all(e < CHAIN_L1_BF16 for e in errs.values()), ("bf16", errs)


# ------------------------------------------------------------------------------------------------------------------------------
# whole train step (protocol and bounds of test_gpu_configs.py::test_config_variant_matches_the_oracle)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [4, 7])
def test_train_step_matches_the_oracle(dev, ratio):
    B, V = 2, 3
    ocfg, pcfg = O.default_cfg(), S.default_cfg()
    for c in (ocfg, pcfg):
        c.NETWORK.ATT_SPATIAL_DOWNSAMPLE_RATIO = ratio
    torch.manual_seed(0)
    onets = [O.Encoder(ocfg), O.Decoder(ocfg), O.Merger(ocfg), O.Refiner(ocfg)]
    for i, n in enumerate(onets):
        O.seeded_weights_(n, seed=50 + i)
        n.train()
        for m in n.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
            if isinstance(m, O.model.SwinBlock):
                m.dp = 0.0
    pnets = [Encoder(pcfg), Decoder(pcfg), Merger(pcfg), Refiner(pcfg)]
    for p, o in zip(pnets, onets):
        p.load_state_dict(o.state_dict())
        p.to(dev).train()
        p.stochastic = False
    g = torch.Generator().manual_seed(1)
    x = (0.5 * torch.randn(B, V, 3, 224, 224, generator=g)).clamp(-1, 1)
    gt = (torch.rand(B, 32, 32, 32, generator=g) < 0.1).float()
    with torch.no_grad():
        total_o, _, _, _, refined_o = O.train_step_loss(onets, ocfg, x, gt)
    out = {}
    for mode in ("f32", "bf16"):
        S.set_math(mode)
        if mode == "bf16":
            S.set_storage("bf16")
        try:
            for p in pnets:
                p.zero_grad(set_to_none=True)
            raw, vol = pnets[1](pnets[0](x.to(dev)))
            merged = pnets[2](raw, vol)
            refined = pnets[3](merged)
            total = bce(merged, gt.to(dev)) + bce(refined, gt.to(dev))
            total.backward()
            finite = all(bool(torch.isfinite(p.grad).all()) for n in pnets for p in n.parameters() if p.grad is not None)
            n_grads = sum(p.grad is not None for n in pnets for p in n.parameters())
            out[mode] = (float(total.detach()), float((refined.detach().cpu() - refined_o).abs().max()), finite, n_grads)
        finally:
            S.set_math("f32")
    l32, e32, f32, n32 = out["f32"]
    l16, _, f16, _ = out["bf16"]
    ref = float(total_o)
    assert pnets[0].cross_view_attention.downsample_qkv.weight.shape[-1] == ratio
    assert n32 == sum(1 for n in pnets for _ in n.parameters())
    assert abs(l32 - ref) < 1e-3 and e32 < 2e-3 * max(1.0, float(refined_o.abs().max())) and f32
    assert f16 and abs(l16 - ref) < 3e-2 * max(1.0, abs(ref))


# ------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------
def test_ratio_8_and_unbuilt_ratios_are_refused(dev):
    cfg = S.default_cfg()
    cfg.NETWORK.ATT_SPATIAL_DOWNSAMPLE_RATIO = 8          # the 8x8 kernel exceeds the 7x7 map (the reference's Conv2d fails too)
    enc = Encoder(cfg).to(dev).eval()
    with pytest.raises(RuntimeError, match="exceeds the 7x7 map"), torch.no_grad():
        enc(torch.zeros(1, 1, 3, 224, 224, device=dev))
    hip.load()
    I, C = 2, 8
    x, dx, small = ops.zeros(I * 49, C, device=dev), ops.zeros(I * 49, C, device=dev), ops.zeros(I * 4, C, device=dev)
    w, dw, db = ops.fzeros(C * 64, device=dev), ops.fzeros(C * 64, device=dev), ops.fzeros(C, device=dev)
    for r in (3, 8, 1, 0):
        with pytest.raises(RuntimeError, match="ATT_SPATIAL_DOWNSAMPLE_RATIO"):
            call("sv_cva_downsample_fwd", ptr(x), ptr(w), ptr(db), ptr(small), I, C, r)
        with pytest.raises(RuntimeError, match="ATT_SPATIAL_DOWNSAMPLE_RATIO"):
            call("sv_cva_downsample_bwd", ptr(small), ptr(x), ptr(w), ptr(dx), ptr(dw), ptr(db), I, C, r)
        with pytest.raises(RuntimeError, match="ATT_SPATIAL_DOWNSAMPLE_RATIO"):
            call("sv_cva_upsample_add_fwd", ptr(small), ptr(x), C, ptr(dx), I, C, r)
        with pytest.raises(RuntimeError, match="ATT_SPATIAL_DOWNSAMPLE_RATIO"):
            call("sv_cva_upsample_bwd", ptr(dx), ptr(small), I, C, r)
