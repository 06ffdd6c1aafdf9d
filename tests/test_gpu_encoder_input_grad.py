"""Gradient of the Encoder wrt the input renderings (images.requires_grad): the adjoint of sv_encoder_prep, the ResNet stem's data gradient
on the space-to-depth image (gather engine, and the halo-tile kind of csrc/conv_halo.hip), the Swin patch-embedding data gradient, and the
whole chain against the fp64 CPU oracle (reference models/encoder.py: torchvision ResNet-50 stem + timm PatchEmbed, plain PyTorch autograd)."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402
import swinvox_amd as S  # noqa: E402
from swinvox_amd import hip, ops  # noqa: E402
from swinvox_amd.losses import bce_with_logits as bce  # noqa: E402
from swinvox_amd.models import Decoder, Encoder, Merger, Refiner  # noqa: E402
from swinvox_amd.ops import ConvSpec, call, ptr  # noqa: E402

from test_gpu_modules import bn_fed_biases, grad_report, no_stochastic, synth_gt, synth_images  # noqa: E402


@pytest.fixture()
def f32_mode():
    ops.set_math("f32")
    yield
    ops.set_math("f32")


@pytest.fixture()
def bf16_mode():
    ops.set_math("bf16")
    ops.set_storage("bf16")
    mode = int(hip.load().sv_conv_halo_mode())
    try:
        yield
    finally:
        ops.set_conv_halo(mode)
        ops.set_math("f32")


def _launches():
    torch.cuda.synchronize()
    return int(hip.load().sv_conv_halo_launches())


def _prep(x, I):
    x16, xp = ops.empty(I * 112 * 112, 16, like=x), ops.empty(I * 56 * 56, 48, like=x)
    call("sv_encoder_prep", ptr(x), 1 if x.dtype == torch.float32 else 0, ptr(x16), ptr(xp), I, 224)
    return x16, xp


def _prep_bwd(dx16, dxp, I, out_dtype=torch.float32):
    out = torch.empty(I, 3, 224, 224, dtype=out_dtype, device=dx16.device)
    call("sv_encoder_prep_bwd", ptr(dx16), ptr(dxp), ptr(out), 1 if out_dtype == torch.float32 else 0, I, 224)
    return out


def _prep_bwd_torch(a, b, I):
    """the adjoint restated with reshape / permute: a [I*112*112, (sy, sx, c) = 16], b [I*56*56, (ky, kx, c) = 48]"""
    ta = a.view(I, 112, 112, 2, 2, 4)[..., :3].permute(0, 5, 1, 3, 2, 4).reshape(I, 3, 224, 224)
    tb = b.view(I, 56, 56, 4, 4, 3).permute(0, 5, 1, 3, 2, 4).reshape(I, 3, 224, 224)
    return tb + ta


# ---- 1. adjoint identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["f32", "bf16"])
def test_encoder_prep_bwd_is_the_adjoint_of_encoder_prep(dev, store):
    ops.set_math("bf16" if store == "bf16" else "f32")
    ops.set_storage(store)
    try:
        I = 3
        g = torch.Generator().manual_seed(11)
        dt = torch.bfloat16 if store == "bf16" else torch.float32
        x = torch.randn(I, 3, 224, 224, generator=g).to(dt).to(dev)
        a = torch.randn(I * 112 * 112, 16, generator=g).to(dt).to(dev)
        b = torch.randn(I * 56 * 56, 48, generator=g).to(dt).to(dev)
        x16, xp = _prep(x, I)
        dimg = _prep_bwd(a, b, I)
        torch.cuda.synchronize()
        lhs = float((x16.double() * a.double()).sum() + (xp.double() * b.double()).sum())
        rhs = float((x.double() * dimg.double()).sum())
        assert abs(lhs - rhs) <= 1e-6 * max(1.0, abs(lhs)), (lhs, rhs)
        ref = _prep_bwd_torch(a.float(), b.float(), I)
        assert torch.equal(dimg, ref)                                       # element-exact (a + b in fp32 either way)
        if store == "bf16":                                                 # the storage type out: the same sums rounded once
            d16 = _prep_bwd(a, b, I, torch.bfloat16)
            assert torch.equal(d16, ref.bfloat16())
    finally:
        ops.set_math("f32")


# ---- 2. the stem's data gradient -------------------------------------------------------------------------------------------------------
def _stem_dgrad(w, dy, I):
    """dy [I*112*112, 64] (storage dtype) -> the gradient wrt the images [I, 3, 224, 224] fp32 through the 4x4 formulation and the adjoint"""
    sp = ConvSpec.conv2d(16, 64, 4, 1, 2, og_fixed=(1, 112, 112))
    w16 = torch.empty(64, 16, 4, 4, dtype=torch.float32, device=dy.device)
    call("sv_stem_native", ptr(w), ptr(w16))
    dx16 = ops.empty(I * 112 * 112, 16, like=dy)
    sp.dgrad(dy, I, (1, 112, 112), ops.pack_one(sp, w16, "d"), dx16)
    zero = ops.zeros(I * 56 * 56, 48, like=dy)
    return dx16, _prep_bwd(dx16, zero, I)


def _stem_operands(I, seed, dt):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(64, 3, 7, 7, generator=g) / 12.0).to(dt).float()
    dy = torch.randn(I, 64, 112, 112, generator=g).to(dt).float()
    ref = torch.nn.grad.conv2d_input((I, 3, 224, 224), w.double(), dy.double(), stride=2, padding=3)
    return w, dy, ref


def _err(a, ref):
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max())


def test_stem_data_gradient_f32_engine(dev, f32_mode):
    I = 2
    w, dy, ref = _stem_operands(I, 5, torch.float32)
    n0 = _launches()
    _, dimg = _stem_dgrad(w.to(dev), dy.permute(0, 2, 3, 1).reshape(-1, 64).contiguous().to(dev), I)
    assert _launches() == n0                                                # f32 math: the gather engine
    assert _err(dimg, ref) <= 1e-5


@pytest.mark.parametrize("halo", [2, 0])
def test_stem_data_gradient_bf16(dev, bf16_mode, halo):
    I = 3
    w, dy, ref = _stem_operands(I, 6, torch.bfloat16)
    ops.set_conv_halo(halo)
    n0 = _launches()
    _, dimg = _stem_dgrad(w.to(dev), dy.permute(0, 2, 3, 1).reshape(-1, 64).contiguous().to(dev).bfloat16(), I)
    took = _launches() - n0
    assert (took == 1) if halo == 2 else (took == 0)
    assert _err(dimg, ref) <= 1e-2


@pytest.mark.parametrize("n,H,W", [(3, 45, 70), (1, 5, 9), (2, 17, 33), (1, 16, 64)])
def test_stem_data_gradient_halo_on_ragged_grids(dev, bf16_mode, n, H, W):
    """the halo kind on grids whose tiles are cut by both image edges, one smaller than a tile, and exact tiles"""
    g = torch.Generator().manual_seed(n + H + W)
    w = (torch.randn(64, 16, 4, 4, generator=g) / 16.0).bfloat16().double()
    dy = torch.randn(n, 64, H, W, generator=g).bfloat16().double()
    x = torch.zeros(n, 16, H, W, dtype=torch.float64, requires_grad=True)
    (F.conv2d(F.pad(x, (2, 1, 2, 1)), w) * dy).sum().backward()         # pads (2, 1): the stem's 4x4 formulation
    sp = ConvSpec.conv2d(16, 64, 4, 1, 2, og_fixed=(1, H, W))
    dyd = dy.permute(0, 2, 3, 1).reshape(-1, 64).to(dev).bfloat16().contiguous()
    pack = ops.pack_one(sp, w.float().to(dev), "d")
    outs = {}
    for mode in (2, 0):
        ops.set_conv_halo(mode)
        n0 = _launches()
        dx = torch.full((n * H * W, 16), float("nan"), dtype=torch.bfloat16, device=dev)
        sp.dgrad(dyd, n, (1, H, W), pack, dx)
        assert _launches() - n0 == (1 if mode == 2 else 0)
        outs[mode] = dx.float().cpu().double()
    ref = x.grad.permute(0, 2, 3, 1).reshape(-1, 16)
    for mode, dx in outs.items():
        assert bool(torch.isfinite(dx).all()), mode                          # every element written
        assert float((dx - ref).abs().max() / ref.abs().max()) < 1e-2, mode


def test_stem_data_gradient_full_size(dev, bf16_mode):
    """I = 512 (bench shape): the halo kind and the engine agree to bf16 rounding"""
    I = 512
    g = torch.Generator(device=dev).manual_seed(7)
    w = (torch.randn(64, 3, 7, 7, device=dev, generator=g) / 12.0)
    dy = torch.randn(I * 112 * 112, 64, device=dev, generator=g).bfloat16()
    res = {}
    for mode in (2, 0):
        ops.set_conv_halo(mode)
        n0 = _launches()
        dx16, _ = _stem_dgrad(w, dy, I)
        assert _launches() - n0 == (1 if mode == 2 else 0)
        res[mode] = dx16.float()
    assert bool(torch.isfinite(res[2]).all())
    d = float((res[2] - res[0]).abs().max()) / float(res[0].abs().max())
    assert d < 1e-2, d


# ---- 3. - 6. the Encoder -------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def _cfgs(multi=True, cva=True):
    ocfg, pcfg = O.default_cfg(), S.default_cfg()
    for c in (ocfg, pcfg):
        c.NETWORK.USE_SWIN_T_MULTI_STAGE = multi
        c.NETWORK.USE_CROSS_VIEW_ATTENTION = cva
    return ocfg, pcfg


def _oracle_encoder(ocfg, variant, train):
    torch.manual_seed(0)
    enc = O.Encoder(ocfg, variant=variant)
    O.seeded_weights_(enc, seed=100)
    no_stochastic([enc])
    return enc.train(train)


def _weights(B, V):
    return torch.randn(B, V, 256, 7, 7, generator=torch.Generator().manual_seed(B * 10 + V))


def _oracle_grads(key, enc, x, R, autocast=False):
    """(images.grad, {name: param.grad}) of loss = <enc(x), R> on the CPU oracle; dtype = fp32 / fp64 / fp32 under bf16 autocast.  Parameters
    the loss does not reach (the unused stage heads of the single-stage Swin) get zeros, as the HIP module gives them."""
    if key in _ORACLE:
        return _ORACLE[key]
    dt = torch.float64 if key[-1] == "f64" else torch.float32
    net = copy.deepcopy(enc).to(dt)
    xi = x.detach().to(dt).clone().requires_grad_(True)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        out = net(xi)
    (out.to(dt) * R.to(dt)).sum().backward()
    _ORACLE[key] = (xi.grad.detach(), {k: p.grad.detach() if p.grad is not None else torch.zeros_like(p) for k, p in net.named_parameters()})
    return _ORACLE[key]


def _hip_encoder(pcfg, enc, variant, train):
    p = Encoder(pcfg, variant=variant)
    p.load_state_dict(enc.state_dict())
    p.to(torch.device("cuda:0")).train(train)
    p.stochastic = False
    return p


CASES = [dict(), dict(prep=False), dict(fused=False), dict(multi=False), dict(cva=False), dict(V=1), dict(train=False), dict(variant="base", B=1)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()) or "default")
def test_encoder_image_gradient_f32_matches_the_oracle(dev, f32_mode, case):
    B, V = case.get("B", 2), case.get("V", 2)
    multi, cva, train, variant = case.get("multi", True), case.get("cva", True), case.get("train", True), case.get("variant", "tiny")
    ocfg, pcfg = _cfgs(multi, cva)
    enc = _oracle_encoder(ocfg, variant, train)
    x, R = synth_images(B, V, 21), _weights(B, V)
    okey = (B, V, multi, cva, train, variant)
    gx32, gp32 = _oracle_grads(okey + ("f32",), enc, x, R)
    gx64, gp64 = _oracle_grads(okey + ("f64",), enc, x, R)
    penc = _hip_encoder(pcfg, enc, variant, train)
    prep0, fused0 = ops.input_prep_enabled(), ops.bn_pool_fused_enabled()
    ops.set_input_prep(case.get("prep", True))
    ops.set_bn_pool_fused(case.get("fused", True))      # False: the stem's dy from the separate BatchNorm / max-pool backward passes
    try:
        (penc(x.to(dev)) * R.to(dev)).sum().backward()                    # the same step without the image gradient
        g0 = {k: p.grad.clone() for k, p in penc.named_parameters()}
        penc.zero_grad(set_to_none=True)
        xd = x.to(dev).requires_grad_(True)
        (penc(xd) * R.to(dev)).sum().backward()
        torch.cuda.synchronize()
    finally:
        ops.set_input_prep(prep0)
        ops.set_bn_pool_fused(fused0)
    assert xd.grad is not None and xd.grad.dtype == torch.float32 and xd.grad.shape == x.shape
    hg = {k: p.grad for k, p in penc.named_parameters()}
    # asking for the image gradient leaves every parameter gradient as it was (same kernels; fp32 atomics may reorder a sum).  Conv biases in
    # front of a train-mode BatchNorm are analytically zero: what both steps compute for them is rounding noise (test_gpu_modules' rule below)
    zero = bn_fed_biases(enc) if train else {}
    for k, g in hg.items():
        if k not in zero:
            assert float((g - g0[k]).abs().max()) <= 1e-5 * float(g0[k].abs().max()) + 1e-6, k
    items = [("images", xd.grad, gx32, gx64)]
    if not case:
        # and in the default configuration each of them passes the oracle rule too.  The analytically-zero biases stay at rounding level, so does
        # the one whose BatchNorm sits outside its nn.Sequential (cross-view attention ffn.2: zero in the fp64 oracle).  (Train-mode BatchNorm
        # over 2-4 images leaves other configurations' weight gradients ill-conditioned beyond the rule's floors for this loss - with or without
        # the image gradient.)
        for k, kb in zero.items():
            assert float(hg[k].abs().max()) < 0.1 * float(hg[kb].abs().max()), k
        for k, g in gp64.items():
            if k not in zero and float(g.abs().max()) < 1e-9:
                assert float(hg[k].abs().max()) < 1e-4, k
                zero[k] = None
        items += [(k, g, gp32[k], gp64[k]) for k, g in hg.items() if k not in zero]
    bad = grad_report(items)
    assert not bad, bad[:10]


def test_encoder_image_gradient_bf16(dev, bf16_mode):
    ops.set_conv_halo(2)
    B, V = 2, 2
    ocfg, pcfg = _cfgs()
    enc = _oracle_encoder(ocfg, "tiny", True)
    x, R = synth_images(B, V, 21), _weights(B, V)
    okey = (B, V, True, True, True, "tiny")
    gx64, _ = _oracle_grads(okey + ("f64",), enc, x, R)
    gxbf, _ = _oracle_grads(okey + ("autocast", "f32"), enc, x, R, autocast=True)
    l1 = float(gx64.abs().sum())
    e_bf = float((gxbf.double() - gx64).abs().sum()) / l1
    penc = _hip_encoder(pcfg, enc, "tiny", True)
    n0 = _launches()
    (penc(x.to(dev)) * R.to(dev)).sum().backward()                        # the same step without the image gradient
    n1 = _launches()
    xd = x.to(dev).requires_grad_(True)
    (penc(xd) * R.to(dev)).sum().backward()
    assert _launches() - n1 == n1 - n0 + 1                                  # the stem's data gradient ran on the halo kind
    assert xd.grad.dtype == torch.float32
    e = float((xd.grad.double().cpu() - gx64).abs().sum()) / l1
    assert e <= max(3e-2, 1.5 * e_bf), (e, e_bf)
    # images in the storage type: the gradient comes back in it
    xb = x.to(dev).bfloat16().requires_grad_(True)
    (penc(xb) * R.to(dev)).sum().backward()
    assert xb.grad.dtype == torch.bfloat16
    e = float((xb.grad.double().cpu() - gx64).abs().sum()) / l1
    assert e <= max(3e-2, 1.5 * e_bf), (e, e_bf)


def test_images_in_another_dtype_than_fp32_or_the_storage_type_are_refused(dev, f32_mode):
    """fp32 storage with bf16 (or fp16) images: the module refuses them before any kernel runs (inputs are fp32 or the storage type), so no
    backward can meet an image dtype whose element size differs from what sv_encoder_prep_bwd writes"""
    ocfg, pcfg = _cfgs()
    penc = _hip_encoder(pcfg, _oracle_encoder(ocfg, "tiny", True), "tiny", True)
    prep0 = ops.input_prep_enabled()
    ops.set_input_prep(False)
    try:
        for dt in (torch.bfloat16, torch.float16):
            xd = synth_images(1, 2, 61).to(dev).to(dt).requires_grad_(True)
            with pytest.raises(RuntimeError, match="expected float32 inputs"):
                penc(xd)
            assert xd.grad is None
    finally:
        ops.set_input_prep(prep0)


def test_whole_pipeline_image_gradient(dev, f32_mode):
    B, V = 2, 2
    ocfg, pcfg = O.default_cfg(), S.default_cfg()
    torch.manual_seed(0)
    onets = [O.Encoder(ocfg), O.Decoder(ocfg), O.Merger(ocfg), O.Refiner(ocfg)]
    for i, n in enumerate(onets):
        O.seeded_weights_(n, seed=100 + i)
        n.train()
    no_stochastic(onets)
    x, gt = synth_images(B, V, 31), synth_gt(B, 31)
    ref = {}
    for dt in (torch.float32, torch.float64):
        nets = [copy.deepcopy(n).to(dt) for n in onets]
        xi = x.detach().to(dt).clone().requires_grad_(True)
        raw, vol = nets[1](nets[0](xi))
        mer = nets[2](raw, vol)
        (O.bce_logits(mer, gt.to(dt)) + O.bce_logits(nets[3](mer), gt.to(dt))).backward()
        ref[dt] = xi.grad
    pnets = [Encoder(pcfg), Decoder(pcfg), Merger(pcfg), Refiner(pcfg)]
    for p, o in zip(pnets, onets):
        p.load_state_dict(o.state_dict())
        p.to(dev).train()
        p.stochastic = False
    xd = x.to(dev).requires_grad_(True)
    raw, vol = pnets[1](pnets[0](xd))
    mer = pnets[2](raw, vol)
    (bce(mer, gt.to(dev)) + bce(pnets[3](mer), gt.to(dev))).backward()
    bad = grad_report([("images", xd.grad, ref[torch.float32], ref[torch.float64])])
    assert not bad, bad


class _Spy:
    """stands in for the ctypes library: records every entry point looked up on it"""

    def __init__(self, lib):
        self._lib, self.names = lib, set()

    def __getattr__(self, name):
        self.names.add(name)
        return getattr(self._lib, name)


def test_no_image_gradient_no_extra_work(dev, f32_mode, monkeypatch):
    ocfg, pcfg = _cfgs()
    enc = _oracle_encoder(ocfg, "tiny", True)
    penc = _hip_encoder(pcfg, enc, "tiny", True)
    x = synth_images(1, 2, 41).to(dev)
    spy = _Spy(hip.load())
    monkeypatch.setattr(hip, "_lib", spy)
    (penc(x) * _weights(1, 2).to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert x.grad is None
    assert "sv_encoder_prep" in spy.names and "sv_conv_wgrad" in spy.names       # the spy saw the step
    assert not spy.names & {"sv_encoder_prep_bwd", "sv_stem_native"}, spy.names


def test_frozen_parameters_still_give_the_image_gradient(dev, f32_mode):
    B, V = 1, 2
    ocfg, pcfg = _cfgs()
    enc = _oracle_encoder(ocfg, "tiny", True)
    penc = _hip_encoder(pcfg, enc, "tiny", True)
    x, R = synth_images(B, V, 51).to(dev), _weights(B, V).to(dev)
    grads = []
    for frozen in (False, True):
        for p in penc.parameters():
            p.requires_grad_(not frozen)
        xd = x.clone().requires_grad_(True)
        grads.append(torch.autograd.grad((penc(xd) * R).sum(), xd)[0])
    torch.cuda.synchronize()
    assert grads[1] is not None
    assert float((grads[1] - grads[0]).abs().max()) <= 1e-5 * float(grads[0].abs().max())
