"""MXFP8 forward of the fused Swin MLP (csrc/swin_mlp.hip: sv_swin_mlp_mx_pack, sv_swin_mlp_fwd_mx) through the C ABI against the recipe's torch
emulation and the exact-integer case of tests/test_cpu_swin_mlp_mx_recipe.py (which checks both on the CPU), against the unfused MX chain run
through the C ABI on the same inputs, against the bf16 fused kernel, and the host switch ops.set_fused_mlp_mx inside block_forward.

Shapes: C in {96, 128} x M in {1, 17, 147, 200} - the single token, the token tail of a 16-token fragment and of the 128-token workgroup tile,
the K padding of C = 96, 3 windows of 49 with rows_per_scale = 49, and more than one workgroup.  Every output carries NaN guard rows."""
import ctypes as C_
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_linear_fp8_recipe import l1_rel  # noqa: E402
from test_cpu_swin_mlp_mx_recipe import (channel_row_image, emulate_swin_mlp_mx, gauss_mlp_case, hidden_row_image, integer_case,  # noqa: E402
                                         random_bytes)

import swinvox_amd as S  # noqa: E402
from swinvox_amd import hip, ops  # noqa: E402
from swinvox_amd.ops import call, ptr  # noqa: E402

GUARD = 2
WIDTHS = [96, 128]
TOKENS = [1, 17, 147, 200]
RPS = {1: 1, 17: 5, 147: 49, 200: 49}
MARGIN = 1.5                     # the issue's: rare e4m3 flips of h on fp32-ulp differences of the accumulation order, and nothing else
SEPARATION = 3.0                 # the bf16 fused kernel is at least this many times farther from the MX emulation than the MX kernel


def _quant_w(w):
    """sv_quant_rows_mx_e4m3 on an fp32 weight [N, K]: the bytes the unfused sites use"""
    N, K = w.shape
    Kp = (K + 127) // 128 * 128
    q = torch.empty(N, Kp, dtype=torch.uint8, device=w.device)
    s = torch.empty(N, Kp // 32, dtype=torch.uint8, device=w.device)
    call("sv_quant_rows_mx_e4m3", ptr(w), hip.F32, N, K, K, ptr(q), Kp, ptr(s))
    return q, s


def _upload(c, dev):
    d = {k: (v.to(dev).contiguous() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    d["w1"], d["w2"] = _quant_w(d["W1"]), _quant_w(d["W2"])
    return d


def _out(M, Cd, dev):
    return torch.full((M + GUARD, Cd), float("nan"), dtype=torch.bfloat16, device=dev)


def _guards_intact(out, M):
    return bool(torch.isnan(out[M:].float()).all())


def _fused_mx(d, M, Cd, dev):
    lib = hip.load()
    packs = torch.empty(int(lib.sv_swin_mlp_mx_pack_bytes(Cd)), dtype=torch.uint8, device=dev)
    call("sv_swin_mlp_mx_pack", ptr(d["w1"][0]), ptr(d["w1"][1]), ptr(d["w2"][0]), ptr(d["w2"][1]), ptr(packs), Cd)
    x2 = _out(M, Cd, dev)
    n0 = ops.swin_mlp_mx_launches(), ops.linear_mxfp8_launches()
    call("sv_swin_mlp_fwd_mx", ptr(d["x1"]), ptr(x2), ptr(d["ln_g"]), ptr(d["ln_b"]), ptr(packs), ptr(d["b1"]), ptr(d["b2"]), ptr(d["row_scale"]),
         d["rows_per_scale"], M, Cd, d["eps"])
    torch.cuda.synchronize()
    assert (ops.swin_mlp_mx_launches(), ops.linear_mxfp8_launches()) == (n0[0] + 1, n0[1])
    assert _guards_intact(x2, M)
    return x2[:M].cpu()


def _fused_bf16(d, M, Cd, dev):
    packs = torch.empty(16 * Cd * Cd, dtype=torch.bfloat16, device=dev)
    call("sv_swin_mlp_pack", ptr(d["W1"]), ptr(d["W2"]), ptr(packs), Cd)
    x2 = _out(M, Cd, dev)
    call("sv_swin_mlp_fwd", ptr(d["x1"]), ptr(x2), ptr(d["ln_g"]), ptr(d["ln_b"]), ptr(packs), ptr(d["b1"]), ptr(d["b2"]), ptr(d["row_scale"]),
         d["rows_per_scale"], M, Cd, d["eps"])
    torch.cuda.synchronize()
    assert _guards_intact(x2, M)
    return x2[:M].cpu()


def _unfused_chain(d, M, Cd, dev):
    """sv_layernorm_quant_mx_fwd -> sv_linear_mxfp8 (GELU, q_out) -> sv_linear_mxfp8 (residual): the parent's MX chain, bf16 storage"""
    HID = 4 * Cd
    y = torch.empty(M, Cd, dtype=torch.bfloat16, device=dev)
    mean, rstd = torch.empty(M, device=dev), torch.empty(M, device=dev)
    q = torch.empty(M, 128, dtype=torch.uint8, device=dev)
    s = torch.empty(M, 4, dtype=torch.uint8, device=dev)
    call("sv_layernorm_quant_mx_fwd", ptr(d["x1"]), ptr(d["ln_g"]), ptr(d["ln_b"]), ptr(y), ptr(mean), ptr(rstd), ptr(q), 128, ptr(s), M, Cd, d["eps"], 0, 0,
         act=hip.BF16)
    hq = torch.empty(M, HID, dtype=torch.uint8, device=dev)
    hs = torch.empty(M, HID // 32, dtype=torch.uint8, device=dev)
    e1 = ops._epilogue(HID, bias=d["b1"], act=hip.ACT_GELU)
    call("sv_linear_mxfp8", ptr(q), ptr(s), ptr(d["w1"][0]), ptr(d["w1"][1]), None, M, Cd, HID, C_.byref(e1), ptr(hq), ptr(hs), act=hip.BF16)
    x2 = _out(M, Cd, dev)
    e2 = ops._epilogue(Cd, bias=d["b2"], residual=d["x1"], ldr=Cd, row_scale=d["row_scale"], rows_per_scale=d["rows_per_scale"])
    call("sv_linear_mxfp8", ptr(hq), ptr(hs), ptr(d["w2"][0]), ptr(d["w2"][1]), ptr(x2), M, HID, Cd, C_.byref(e2), None, None, act=hip.BF16)
    torch.cuda.synchronize()
    assert _guards_intact(x2, M)
    return x2[:M].cpu()


# ---- 0. the pack image, byte for byte ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("Cd", WIDTHS)
def test_pack_image_byte_for_byte(dev, Cd):
    """W1F | W2F | W1S | W2S of random bytes against the CPU gather written from the kernel's header comment"""
    HID = 4 * Cd
    w1q, w1s = random_bytes(41 + Cd, HID, 128), random_bytes(42 + Cd, HID, 4)
    w2q, w2s = random_bytes(43 + Cd, Cd, HID), random_bytes(44 + Cd, Cd, HID // 32)
    (w1f, w1sc), (w2f, w2sc) = hidden_row_image(w1q, w1s), channel_row_image(w2q, w2s)
    ref = torch.cat([t.flatten() for t in (w1f, w2f, w1sc, w2sc)])
    nbytes = int(hip.load().sv_swin_mlp_mx_pack_bytes(Cd))
    assert ref.numel() == nbytes
    packs = torch.full((nbytes + 16,), 0xA5, dtype=torch.uint8, device=dev)    # 16 guard bytes behind the image
    on_dev = [t.to(dev) for t in (w1q, w1s, w2q, w2s)]
    call("sv_swin_mlp_mx_pack", *(ptr(t) for t in on_dev), ptr(packs), Cd)
    torch.cuda.synchronize()
    got = packs.cpu()
    assert bool((got[nbytes:] == 0xA5).all())
    assert torch.equal(got[:nbytes], ref), int((got[:nbytes] != ref).sum())


# ---- 1. exact integers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M", TOKENS)
@pytest.mark.parametrize("Cd", WIDTHS)
def test_exact_integers(dev, Cd, M):
    """Every intermediate is a small integer with <= 4 significant bits and the block scale bytes are non-unit and differ between blocks, so a
    wrong lane, k order, row permutation of the packs or scale byte changes the result; the bf16 fused kernel is exact on the same case, which
    checks the case (and that the fast GELU is the identity on it) independently of the new code."""
    c, ref = integer_case(M, Cd)
    d = _upload(c, dev)
    got16 = _fused_bf16(d, M, Cd, dev).double()
    assert torch.equal(got16, ref), ("bf16 fused kernel", int((got16 != ref).sum()), float((got16 - ref).abs().max()))
    got = _fused_mx(d, M, Cd, dev).double()
    assert torch.equal(got, ref), ("MX fused kernel", int((got != ref).sum()), float((got - ref).abs().max()))


# ---- 2 and 3. the recipe on N(0, 1) data ---------------------------------------------------------------------------------------------------
_RUNS = {}


def _gauss_runs(dev, Cd, M):
    """emulation, MX fused kernel, unfused MX chain and bf16 fused kernel on one case: computed once, left unchanged"""
    key = (Cd, M)
    if key not in _RUNS:
        c = gauss_mlp_case(M, Cd, windows=RPS[M])
        d = _upload(c, dev)
        _RUNS[key] = dict(x1=c["x1"].double(), ref=emulate_swin_mlp_mx(**c), mx=_fused_mx(d, M, Cd, dev).double(),
                          chain=_unfused_chain(d, M, Cd, dev).double(), bf16=_fused_bf16(d, M, Cd, dev).double())
    return _RUNS[key]


def _dist(got, ref):
    return l1_rel(got, ref), float((got - ref).abs().max() / ref.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("M", TOKENS)
@pytest.mark.parametrize("Cd", WIDTHS)
def test_recipe_within_the_unfused_chain_distance(dev, Cd, M):
    """The fused kernel stays within 1.5 x d_chain of the emulation, L1-relative and in the worst element, d_chain being the distance of the
    unfused MX chain (the parent's kernels, which meet L1 3e-3 / worst element 1e-2) from the same emulation, measured here."""
    r = _gauss_runs(dev, Cd, M)
    assert bool(torch.isfinite(r["mx"]).all())
    (l1, mx), (l1c, mxc) = _dist(r["mx"], r["ref"]), _dist(r["chain"], r["ref"])
    print(f"C={Cd} M={M}: fused MX vs emulation L1-rel {l1:.3e} worst {mx:.3e}; unfused MX chain vs emulation L1-rel {l1c:.3e} worst {mxc:.3e}; "
          f"fused MX != unfused chain in {int((r['mx'] != r['chain']).sum())} of {M * Cd} elements")
    assert l1c <= 3e-3 and mxc <= 1e-2, (l1c, mxc)               # the chain meets the project's bounds (tests/test_gpu_linear_mxfp8.py)
    assert l1 <= MARGIN * l1c, (l1, l1c)
    assert mx <= MARGIN * mxc, (mx, mxc)


@pytest.mark.gpu
@pytest.mark.parametrize("M", TOKENS)
@pytest.mark.parametrize("Cd", WIDTHS)
def test_it_is_the_mx_result_not_the_bf16_one(dev, Cd, M):
    """On the MLP branch x2 - x1 the MX kernel is at least 3 x closer to the MX emulation than the bf16 fused kernel is."""
    r = _gauss_runs(dev, Cd, M)
    bref = r["ref"] - r["x1"]
    d_mx, d_bf16 = l1_rel(r["mx"] - r["x1"], bref), l1_rel(r["bf16"] - r["x1"], bref)
    print(f"C={Cd} M={M}: branch distance from the MX emulation: fused MX {d_mx:.3e}, fused bf16 {d_bf16:.3e} ({d_bf16 / max(d_mx, 1e-30):.1f} x)")
    assert d_mx < d_bf16, (d_mx, d_bf16)
    assert d_bf16 >= SEPARATION * d_mx, (d_mx, d_bf16)


# ---- 4. host switch ------------------------------------------------------------------------------------------------------------------------
IMGS, RES = 2, 56


def _block(dev, Cd, heads, res=RES):
    from swinvox_amd.models.swin_transformer import SwinBlock
    torch.manual_seed(5)
    blk = SwinBlock(Cd, res, heads, 3, 0.0)
    g = torch.Generator().manual_seed(6 + Cd)
    with torch.no_grad():
        for n, p in blk.named_parameters():
            if p.dim() == 1:
                p.copy_((1.0 if "norm" in n and n.endswith("weight") else 0.0) + 0.1 * torch.randn(p.shape, generator=g))
            elif "bias_table" not in n:
                p.copy_(torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5)
    blk.to(dev)
    M = IMGS * res * res
    x = torch.randn(M, Cd, generator=g).bfloat16().to(dev)
    dy = torch.randn(M, Cd, generator=g).bfloat16().to(dev)
    return blk, x, dy


def _counters():
    return ops.swin_mlp_mx_launches(), ops.linear_mxfp8_launches(), ops.mx_act_quant_launches()


def _delta(a, b):
    return tuple(y - x for x, y in zip(a, b))


@pytest.fixture
def switches():
    try:
        yield
    finally:
        ops.set_fused_mlp_mx(False)
        ops.set_fused_mlp(True)
        ops.set_pack_cache(None)
        S.set_linear_fp8(False)
        S.set_math("f32")


@pytest.mark.gpu
@pytest.mark.parametrize("Cd,heads", [(96, 3), (128, 4)])
def test_host_switch(dev, monkeypatch, switches, Cd, heads):
    from swinvox_amd.models import swin_transformer as st
    blk, x, dy = _block(dev, Cd, heads)
    M = IMGS * RES * RES
    bf16_packs = []
    real_call = st.call

    def spy(name, *a, **k):
        if name == "sv_swin_mlp_pack":
            bf16_packs.append(name)
        return real_call(name, *a, **k)

    monkeypatch.setattr(st, "call", spy)
    ops.set_math("bf16")
    ops.set_storage("bf16")
    S.set_linear_fp8(True, recipe="mx")
    ops.set_pack_cache(ops.PackCache())
    assert ops.fused_mlp_enabled(Cd) and not ops.fused_mlp_mx_enabled(Cd)       # off by default

    def run(save):
        grads = {p: torch.zeros_like(p, dtype=torch.float32) for p in blk.parameters()}
        del bf16_packs[:]
        n0 = _counters()
        if save:
            x2, ctx = st.block_forward(blk, x, IMGS, True, False, None, True)
        else:
            with torch.no_grad():
                x2, ctx = st.block_forward(blk, x, IMGS, False, False, None, False)
        torch.cuda.synchronize()
        n, npk = _delta(n0, _counters()), len(bf16_packs)
        dx = None
        if save:
            dx = st.block_backward(blk, ctx, dy.clone(), grads)
            torch.cuda.synchronize()
            assert all(bool(torch.isfinite(g).all()) for g in grads.values())
        return x2.cpu(), ctx, n, npk, (dx.cpu() if dx is not None else None)

    x2_off, ctx_off, n_off, pk_off, dx_off = run(True)
    assert n_off[0] == 0 and pk_off == 1                                        # the parent's launches
    ops.set_fused_mlp_mx(True)
    assert ops.fused_mlp_mx_enabled(Cd)
    x2_on, ctx_on, n_on, pk_on, dx_on = run(True)
    assert n_on[0] == 1 and n_on[1:] == n_off[1:], (n_on, n_off)                # one fused MX launch; no MX GEMM or quantiser for the MLP branch
    assert n_on[1:] == ((0, 0) if Cd == 96 else (2, 1)), n_on                   # C = 96: fused bf16 attention branch; C = 128: qkv + proj, one norm1 quantiser
    assert pk_on == 1 and len(ctx_on) == len(ctx_off) == 17 and ctx_on.fused_mlp and ctx_off.fused_mlp and ctx_on[12] is None
    assert ctx_on.packs is not None and ctx_on.packs.dtype == torch.bfloat16 and ctx_on.packs.numel() == 16 * Cd * Cd
    assert [type(a) for a in ctx_on] == [type(a) for a in ctx_off]              # the ctx tuple keeps its layout
    assert bool(torch.isfinite(x2_on.float()).all()) and not torch.equal(x2_on, x2_off)
    d = l1_rel(x2_on.double(), x2_off.double())
    print(f"C={Cd}: block output, fused MX vs fused bf16 MLP: L1-rel {d:.3e}")
    assert d < 5e-2
    assert torch.equal(dx_on, dx_off)                                           # the backward does not read the forward's output
    # torch.no_grad(): no bf16 packs are built
    _, ctx_ng, n_ng, pk_ng, _ = run(False)
    assert n_ng[0] == 1 and pk_ng == 0 and ctx_ng.packs is None and ctx_ng[12] is None
    ops.set_fused_mlp_mx(False)
    x2_ng_off, _, n_ng_off, pk_ng_off, _ = run(False)
    assert n_ng_off[0] == 0 and pk_ng_off == 1                                  # as on the parent
    x2_off2, _, n_off2, _, _ = run(True)
    assert torch.equal(x2_off2, x2_off) and n_off2 == n_off                     # switched off again: the parent's result, bit for bit


@pytest.mark.gpu
def test_switch_is_inert_elsewhere(dev, switches):
    from swinvox_amd.models import swin_transformer as st
    ops.set_math("bf16")
    ops.set_storage("bf16")
    ops.set_fused_mlp_mx(True)
    S.set_linear_fp8(True, recipe="mx")
    assert ops.fused_mlp_mx_enabled(96) and ops.fused_mlp_mx_enabled(128)
    assert not ops.fused_mlp_mx_enabled(192) and not ops.fused_mlp_mx_enabled(384)
    ops.set_fused_mlp(False)
    assert not ops.fused_mlp_mx_enabled(96)
    ops.set_fused_mlp(True)
    S.set_linear_fp8(True)                                                      # the row recipe
    assert not ops.fused_mlp_mx_enabled(96)
    blk, x, _ = _block(dev, 96, 3, res=14)
    n0 = _counters()
    with torch.no_grad():
        x2_row, _ = st.block_forward(blk, x, IMGS, False, False, None, False)
    torch.cuda.synchronize()
    assert _delta(n0, _counters())[0] == 0
    S.set_linear_fp8(False)
    assert not ops.fused_mlp_mx_enabled(96)
    with torch.no_grad():
        x2_bf16, _ = st.block_forward(blk, x, IMGS, False, False, None, False)
    assert torch.equal(x2_row, x2_bf16)                                         # the fused bf16 MLP under either
    S.set_linear_fp8(True, recipe="mx")
    ops.set_math("f32")
    assert not ops.fused_mlp_mx_enabled(96)
    assert _delta(n0, _counters())[0] == 0
