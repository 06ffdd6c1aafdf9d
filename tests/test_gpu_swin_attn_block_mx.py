"""MXFP8 forward of the fused attention branch (csrc/attn.hip: sv_swin_attn_block_mx_pack, sv_swin_attn_block_fwd_mx) through the C ABI against
the recipe's torch emulation and the exact case of tests/test_cpu_swin_attn_block_mx_recipe.py (which checks both on the CPU), against the
unfused MX chain run through the C ABI on the same inputs, against the bf16 fused kernel, and the host switch ops.set_fused_attn_block_mx
inside block_forward / block_backward.

Shapes (I, H, shift, drop-path): one and several windows per image, shifted and not, one window per image, and (58, 21): several windows per
window group with the last workgroup's second group empty.  Every output carries NaN guard rows."""
import ctypes as C_
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_linear_fp8_recipe import l1_rel  # noqa: E402
from test_cpu_swin_attn_block_mx_recipe import attn_block_pack_bytes, emulate_swin_attn_block_mx, exact_case  # noqa: E402
from test_cpu_swin_mlp_mx_recipe import random_bytes  # noqa: E402
from test_gpu_swin_attn_block import _case, _image_slices, _rel, _rows, _share  # noqa: E402

import swinvox_amd as S  # noqa: E402
from swinvox_amd import hip, ops  # noqa: E402
from swinvox_amd.ops import call, ptr  # noqa: E402

pytestmark = pytest.mark.gpu

C, HEADS = 96, 3
GUARD = 2
SHAPES = [(2, 14, 0, False), (3, 14, 3, True), (5, 7, 0, True), (1, 28, 3, False), (58, 21, 3, True)]
MARGIN = 1.5                     # the issue's, as tests/test_gpu_swin_mlp_mx.py: rare e4m3 flips on fp32-ulp differences, and nothing else
SEPARATION = 3.0
WORST = {"qkv": 8e-3, "att": 1.2e-2, "x1": 1.2e-2}      # the project's fused-vs-unfused bounds (tests/test_gpu_swin_attn_block.py)


def _quant_w(w):
    """sv_quant_rows_mx_e4m3 on an fp32 weight [N, K]: the bytes the unfused sites use"""
    N, K = w.shape
    Kp = (K + 127) // 128 * 128
    q = torch.empty(N, Kp, dtype=torch.uint8, device=w.device)
    s = torch.empty(N, Kp // 32, dtype=torch.uint8, device=w.device)
    call("sv_quant_rows_mx_e4m3", ptr(w), hip.F32, N, K, K, ptr(q), Kp, ptr(s))
    return q, s


def _upload(p, dev):
    d = {k: (v.to(torch.bfloat16) if k == "x" else v.float()).to(dev).contiguous() for k, v in p.items()}
    d["wq"], d["wp"] = _quant_w(d["wqkv"]), _quant_w(d["wproj"])
    packs = torch.empty(int(hip.load().sv_swin_attn_block_mx_pack_bytes(C)), dtype=torch.uint8, device=dev)
    call("sv_swin_attn_block_mx_pack", ptr(d["wq"][0]), ptr(d["wq"][1]), ptr(d["wp"][0]), ptr(d["wp"][1]), ptr(packs), C)
    d["packs"] = packs
    return d


def _nan(rows, cols, dev, dtype=torch.bfloat16):
    return torch.full((rows + GUARD, cols) if cols else (rows + GUARD,), float("nan"), dtype=dtype, device=dev)


def _outputs(M, dev, side):
    o = {"x1": _nan(M, C, dev), "ln1": None, "qkv": None, "att": None, "mean": None, "rstd": None}
    if side:
        o.update(ln1=_nan(M, C, dev), qkv=_nan(M, 3 * C, dev), att=_nan(M, C, dev), mean=_nan(M, 0, dev, torch.float32), rstd=_nan(M, 0, dev, torch.float32))
    return o


def _finish(o, M):
    torch.cuda.synchronize()
    for k, t in o.items():
        assert t is None or bool(torch.isnan(t[M:].float()).all()), f"guard rows of {k} were written"
    return {k: (None if t is None else t[:M]) for k, t in o.items()}


def _counters():
    return ops.swin_attn_block_mx_launches(), ops.linear_mxfp8_launches(), int(hip.load().sv_quant_rows_mx_launches())


def _fused_mx(d, I, H, shift, scd, side=True):
    M = I * H * H
    o = _outputs(M, d["x"].device, side)
    n0 = _counters()
    call("sv_swin_attn_block_fwd_mx", ptr(d["x"]), ptr(d["lg"]), ptr(d["lb"]), ptr(d["packs"]), ptr(d["bqkv"]), ptr(d["table"]), ptr(d["bproj"]),
         ptr(scd), ptr(o["x1"]), ptr(o["ln1"]), ptr(o["mean"]), ptr(o["rstd"]), ptr(o["qkv"]), ptr(o["att"]), I, H, H, C, HEADS, shift, 1e-5,
         act=hip.BF16)
    out = _finish(o, M)
    n1 = _counters()
    assert n1 == (n0[0] + 1, n0[1], n0[2]), (n0, n1)         # one launch of the new kernel, no MX GEMM, no quantiser
    return out


def _fused_bf16(d, I, H, shift, scd):
    M = I * H * H
    o = _outputs(M, d["x"].device, True)
    call("sv_swin_attn_block_fwd", ptr(d["x"]), ptr(d["lg"]), ptr(d["lb"]), ptr(d["wqkv"]), ptr(d["bqkv"]), ptr(d["table"]), ptr(d["wproj"]),
         ptr(d["bproj"]), ptr(scd), ptr(o["x1"]), ptr(o["ln1"]), ptr(o["mean"]), ptr(o["rstd"]), ptr(o["qkv"]), ptr(o["att"]), I, H, H, C, HEADS,
         shift, 1e-5, act=hip.BF16)
    return _finish(o, M)


def _unfused_chain(d, I, H, shift, scd):
    """sv_layernorm_quant_mx_fwd -> sv_linear_mxfp8 (bias) -> sv_window_attention_fwd_mxq (bf16 core) -> sv_linear_mxfp8 (bias, residual, row_scale)"""
    M, dev = I * H * H, d["x"].device
    o = _outputs(M, dev, True)
    q, s = torch.empty(M, 128, dtype=torch.uint8, device=dev), torch.empty(M, 4, dtype=torch.uint8, device=dev)
    call("sv_layernorm_quant_mx_fwd", ptr(d["x"]), ptr(d["lg"]), ptr(d["lb"]), ptr(o["ln1"]), ptr(o["mean"]), ptr(o["rstd"]), ptr(q), 128, ptr(s), M, C,
         1e-5, 0, 0, act=hip.BF16)
    e1 = ops._epilogue(3 * C, bias=d["bqkv"])
    call("sv_linear_mxfp8", ptr(q), ptr(s), ptr(d["wq"][0]), ptr(d["wq"][1]), ptr(o["qkv"]), M, C, 3 * C, C_.byref(e1), None, None, act=hip.BF16)
    aq, as_ = torch.empty(M, 128, dtype=torch.uint8, device=dev), torch.empty(M, 4, dtype=torch.uint8, device=dev)
    call("sv_window_attention_fwd_mxq", ptr(o["qkv"]), ptr(d["table"]), ptr(o["att"]), I, H, H, C, HEADS, shift, hip.MATH_BF16, ptr(aq), 128, ptr(as_),
         act=hip.BF16)
    e2 = ops._epilogue(C, bias=d["bproj"], residual=d["x"], ldr=C, row_scale=scd, rows_per_scale=H * H)
    call("sv_linear_mxfp8", ptr(aq), ptr(as_), ptr(d["wp"][0]), ptr(d["wp"][1]), ptr(o["x1"]), M, C, C, C_.byref(e2), None, None, act=hip.BF16)
    return _finish(o, M)


def _scale(I, with_scale):
    return torch.tensor([0.0 if i % 3 == 1 else 1.0 / 0.9 for i in range(I)]) if with_scale else None


def _check_geometry(I, H):
    share, windows = _share(I, H, False), I * (H // 7) ** 2
    assert (share >= 2) == ((I, H) == (58, 21)), (share, I, H)
    if (I, H) == (58, 21):
        assert 0 < windows % (2 * share) <= share            # the second window group of the last workgroup has nothing to do
    return share


# ---- 0. the pack image, byte for byte ----------------------------------------------------------------------------------------------------
def test_pack_image_byte_for_byte(dev):
    ops_ = random_bytes(51, 288, 128), random_bytes(52, 288, 4), random_bytes(53, 96, 128), random_bytes(54, 96, 4)
    ref = attn_block_pack_bytes(*ops_)
    nbytes = int(hip.load().sv_swin_attn_block_mx_pack_bytes(C))
    assert ref.numel() == nbytes
    packs = torch.full((nbytes + 16,), 0xA5, dtype=torch.uint8, device=dev)    # 16 guard bytes behind the image
    on_dev = [t.to(dev) for t in ops_]
    call("sv_swin_attn_block_mx_pack", *(ptr(t) for t in on_dev), ptr(packs), C)
    torch.cuda.synchronize()
    got = packs.cpu()
    assert bool((got[nbytes:] == 0xA5).all())
    assert torch.equal(got[:nbytes], ref), int((got[:nbytes] != ref).sum())


# ---- 1. the exact case -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I,H,shift,with_scale", SHAPES)
def test_exact_case(dev, I, H, shift, with_scale):
    """Every stored value is a small integer with <= 4 significant bits (or bf16-exact) and the block scale bytes are non-unit and differ between
    blocks, so a wrong lane, k order, row permutation of the pack or scale byte changes the result; the bf16 fused kernel is exact on the same
    case, which checks the case independently of the new code."""
    _check_geometry(I, H)
    c, sc, ref = exact_case(I, H)
    d = _upload(c, dev)
    scd = sc.to(dev)
    for name, run in (("bf16 fused kernel", _fused_bf16), ("MX fused kernel", _fused_mx)):
        got = run(d, I, H, shift, scd)
        for k in ("ln1", "qkv", "att", "x1"):
            g = got[k].cpu().double()
            assert torch.equal(g, ref[k]), (name, k, int((g != ref[k]).sum()), float((g - ref[k]).abs().max()))


# ---- 2 - 6. the recipe on N(0, 1) data ------------------------------------------------------------------------------------------------------
_RUNS = {}


def _gauss_runs(dev, I, H, shift, with_scale):
    """emulation, MX fused kernel (training and inference form), unfused MX chain and bf16 fused kernel on one case: computed once, left unchanged"""
    key = (I, H, shift, with_scale)
    if key not in _RUNS:
        p = _case(I, H, 7 * I + H + shift)
        sc = _scale(I, with_scale)
        d = _upload(p, dev)
        scd = sc.to(dev) if sc is not None else None
        emu = emulate_swin_attn_block_mx(p["x"].to(torch.bfloat16), p["lg"], p["lb"], p["wqkv"], p["bqkv"], p["table"], p["wproj"], p["bproj"], I, H,
                                         shift, sc)
        cpu = lambda r: {k: (None if v is None else v.cpu()) for k, v in r.items()}   # noqa: E731
        _RUNS[key] = dict(x=p["x"].double(), emu=emu, mx=cpu(_fused_mx(d, I, H, shift, scd)), lean=cpu(_fused_mx(d, I, H, shift, scd, side=False)),
                          chain=cpu(_unfused_chain(d, I, H, shift, scd)), bf16=cpu(_fused_bf16(d, I, H, shift, scd)), d=d, scd=scd)
    return _RUNS[key]


def _dist(got, ref):
    got, ref = got.double(), ref.double()
    return l1_rel(got, ref), float((got - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("I,H,shift,with_scale", SHAPES)
def test_recipe_within_the_unfused_chain_distance(dev, I, H, shift, with_scale):
    """qkv, att and x1 stay within 1.5 x d_chain of the emulation (L1-relative; worst element within max(1.5 x the chain's, the project's
    fused-vs-unfused bound)), d_chain being the distance of the unfused MX chain from the same emulation, measured here; mean / rstd / ln1 are
    held against the chain's own outputs to the bounds of tests/test_gpu_swin_attn_block.py."""
    _check_geometry(I, H)
    r = _gauss_runs(dev, I, H, shift, with_scale)
    for k in ("qkv", "att", "x1"):
        assert bool(torch.isfinite(r["mx"][k].float()).all()), k
        (l1, mx), (l1c, mxc) = _dist(r["mx"][k], r["emu"][k]), _dist(r["chain"][k], r["emu"][k])
        diff = int((r["mx"][k] != r["chain"][k]).sum())
        print(f"I={I} H={H} shift={shift} {k}: fused MX vs emulation L1-rel {l1:.3e} worst {mx:.3e}; unfused MX chain vs emulation L1-rel {l1c:.3e} "
              f"worst {mxc:.3e}; fused MX != chain in {diff} of {r['mx'][k].numel()} elements")
        assert l1 <= MARGIN * l1c, (k, l1, l1c)
        assert mx <= max(MARGIN * mxc, WORST[k]), (k, mx, mxc)
    dm, dr, dl = _rel(r["mx"]["mean"], r["chain"]["mean"]), _rel(r["mx"]["rstd"], r["chain"]["rstd"]), _rel(r["mx"]["ln1"], r["chain"]["ln1"])
    frac = float((r["mx"]["ln1"].float() != r["chain"]["ln1"].float()).float().mean())
    print(f"I={I} H={H} shift={shift}: vs the chain's outputs: mean {dm:.3e} rstd {dr:.3e} ln1 {dl:.3e} ({100 * frac:.2f} % of ln1 differ)")
    assert dm < 1e-5 and dr < 1e-5, (dm, dr)
    assert dl < 8e-3 and frac < 0.2, (dl, frac)


@pytest.mark.parametrize("I,H,shift,with_scale", SHAPES)
def test_it_is_the_mx_result_not_the_bf16_one(dev, I, H, shift, with_scale):
    """On qkv and on the branch x1 - x the bf16 fused kernel is at least 3 x farther from the MX emulation than the MX kernel is."""
    r = _gauss_runs(dev, I, H, shift, with_scale)
    for k, base in (("qkv", 0.0), ("x1", r["x"])):
        ref = r["emu"][k].double() - base
        d_mx, d_bf16 = l1_rel(r["mx"][k].double() - base, ref), l1_rel(r["bf16"][k].double() - base, ref)
        print(f"I={I} H={H} shift={shift} {'branch x1 - x' if k == 'x1' else k}: distance from the MX emulation: fused MX {d_mx:.3e}, "
              f"fused bf16 {d_bf16:.3e} ({d_bf16 / max(d_mx, 1e-30):.1f} x)")
        assert d_bf16 >= SEPARATION * d_mx, (k, d_mx, d_bf16)


@pytest.mark.parametrize("I,H,shift,with_scale", SHAPES)
def test_inference_form_is_bit_identical(dev, I, H, shift, with_scale):
    r = _gauss_runs(dev, I, H, shift, with_scale)
    assert all(r["lean"][k] is None for k in ("ln1", "qkv", "att", "mean", "rstd"))
    assert torch.equal(r["lean"]["x1"], r["mx"]["x1"])


def test_window_loop_invariance(dev):
    """(58, 21): the image slices run at one window per group reproduce x1, qkv, att and ln1 bit for bit"""
    I, H, shift, with_scale = SHAPES[4]
    assert _check_geometry(I, H) >= 2
    r = _gauss_runs(dev, I, H, shift, with_scale)
    d, scd = r["d"], r["scd"]
    for i0, n in _image_slices(I, H, False):
        one = _fused_mx(dict(d, x=_rows(d["x"], H, i0, n)), n, H, shift, scd[i0:i0 + n])
        for k in ("x1", "qkv", "att", "ln1"):
            assert torch.equal(_rows(r["mx"][k], H, i0, n), one[k].cpu()), (k, i0, n)


def test_launch_counters(dev):
    """one launch per call (asserted inside every _fused_mx as well); neither the MX GEMM nor the activation quantiser counter moves"""
    I, H, shift, with_scale = SHAPES[0]
    r = _gauss_runs(dev, I, H, shift, with_scale)
    n0, q0 = _counters(), ops.mx_act_quant_launches()
    for _ in range(3):
        _fused_mx(r["d"], I, H, shift, r["scd"])
    n1 = _counters()
    assert n1 == (n0[0] + 3, n0[1], n0[2]) and ops.mx_act_quant_launches() == q0


# ---- 7. host switch ------------------------------------------------------------------------------------------------------------------------
IMGS, RES = 2, 56


def _block(dev):
    from swinvox_amd.models.swin_transformer import SwinBlock
    torch.manual_seed(5)
    blk = SwinBlock(C, RES, HEADS, 3, 0.0)
    g = torch.Generator().manual_seed(6 + C)
    with torch.no_grad():
        for n, p in blk.named_parameters():
            if p.dim() == 1:
                p.copy_((1.0 if "norm" in n and n.endswith("weight") else 0.0) + 0.1 * torch.randn(p.shape, generator=g))
            elif "bias_table" not in n:
                p.copy_(torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5)
    blk.to(dev)
    M = IMGS * RES * RES
    x = torch.randn(M, C, generator=g).bfloat16().to(dev)
    dy = torch.randn(M, C, generator=g).bfloat16().to(dev)
    return blk, x, dy


def test_host_switch(dev):
    from swinvox_amd.models import swin_transformer as st
    blk, x, dy = _block(dev)
    a = blk.attn

    def run(save=True):
        grads = {p: torch.zeros_like(p, dtype=torch.float32) for p in blk.parameters()}
        n0 = _counters()
        if save:
            x2, tape = st.block_forward(blk, x, IMGS, True, False, None, True)
        else:
            with torch.no_grad():
                x2, tape = st.block_forward(blk, x, IMGS, False, False, None, False)
        torch.cuda.synchronize()
        n = _counters()[0] - n0[0]
        out = {"x2": x2.float().cpu(), "n": n, "tape": tape}
        if save:
            dx = st.block_backward(blk, tape, dy.clone(), grads)
            torch.cuda.synchronize()
            assert all(bool(torch.isfinite(g).all()) for g in grads.values()) and bool(torch.isfinite(dx.float()).all())
            out.update(dx=dx.double().cpu(), dwqkv=grads[a.qkv.weight].double().cpu(), dwproj=grads[a.proj.weight].double().cpu())
        return out

    try:
        ops.set_math("bf16")
        ops.set_storage("bf16")
        S.set_linear_fp8(True, recipe="mx")
        ops.set_pack_cache(ops.PackCache())
        assert ops.fused_attn_block_enabled(C, HEADS) and not ops.fused_attn_block_mx_enabled(C, HEADS)      # off by default
        bf16 = run()
        assert bf16["n"] == 0
        ops.set_fused_attn_block_mx(True)
        assert ops.fused_attn_block_mx_enabled(C, HEADS)
        new, lean = run(), run(save=False)
        assert new["n"] == 1 and lean["n"] == 1                                  # one new-kernel launch per block_forward, with and without save
        assert torch.equal(new["x2"], lean["x2"])
        assert new["tape"]._fields == bf16["tape"]._fields
        assert [None if v is None else type(v) for v in new["tape"]] == [None if v is None else type(v) for v in bf16["tape"]]
        assert all(getattr(lean["tape"], f) is None for f in ("ln1", "qkv", "att", "m1", "r1"))
        ops.set_fused_attn_block(False)                                          # the unfused MX forward, same backward
        assert not ops.fused_attn_block_mx_enabled(C, HEADS) and ops.fused_attn_block_bwd_enabled(C, HEADS)
        chain = run()
        assert chain["n"] == 0
        ops.set_fused_attn_block(True)
        ops.set_fused_attn_block_mx(False)
        again = run()
        assert again["n"] == 0 and torch.equal(again["x2"], bf16["x2"]) and torch.equal(again["dx"], bf16["dx"])   # off again: bit for bit
    finally:
        ops.set_fused_attn_block_mx(False)
        ops.set_fused_attn_block(True)
        ops.set_pack_cache(None)
        S.set_linear_fp8(False)
        S.set_math("f32")
    for k in ("dx", "dwqkv", "dwproj"):
        d_new, d_bf16 = l1_rel(new[k], chain[k]), l1_rel(bf16[k], chain[k])
        print(f"{k}: L1-rel distance from the unfused-MX-forward tape's: fused MX forward {d_new:.3e}, fused bf16 forward {d_bf16:.3e} "
              f"({d_bf16 / max(d_new, 1e-30):.1f} x)")
        assert SEPARATION * d_new <= d_bf16, (k, d_new, d_bf16)
