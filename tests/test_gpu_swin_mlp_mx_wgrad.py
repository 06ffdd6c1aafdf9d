"""MXFP8 weight gradients of the fused Swin MLP (csrc/swin_mlp.hip: sv_swin_mlp_wgrad_mx) through the C ABI against the recipe's torch emulation
(tests/test_cpu_swin_mlp_mx_wgrad_recipe.py, which checks it on the CPU), against the unfused MX weight-gradient chain run through the C ABI on the same
bytes, against the bf16 fused weight gradients (sv_swin_mlp_wgrad), and the host switch ops.set_fused_mlp_mx(True, wgrad=True) inside block_backward.

Shapes: C in {96, 128} x (M, rows_per_scale) in {(1, 128), (17, 128), (147, 128), (300, 150), (385, 128)} with row_scale, plus (300, NULL): a lone
partly filled 32-token block, a partly filled block behind full ones, a 128-token tile boundary, several token splits (tok_per_split = 128 from M = 129
on), a scale-group boundary inside a block (150), four scale groups.  gauss_mlp_case's seed is chosen so that each width has cases with a dropped (0.0)
and a live scale group.  Every output buffer is prefilled (the kernels ADD) and carries NaN guard elements."""
import ctypes as C_
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_linear_fp8_recipe import l1_rel  # noqa: E402
from test_cpu_swin_mlp_mx_recipe import gauss_mlp_case  # noqa: E402
from test_cpu_swin_mlp_mx_bwd_recipe import dgrad_seed  # noqa: E402
from test_cpu_swin_mlp_mx_wgrad_recipe import emulate_swin_mlp_wgrad_mx  # noqa: E402

import swinvox_amd as S  # noqa: E402
from swinvox_amd import hip, ops  # noqa: E402
from swinvox_amd.ops import call, ptr  # noqa: E402

GUARD = 4
SEED = 1                         # gauss_mlp_case(seed=1): dropped and live groups at C = 96 (M = 147, 385) and C = 128 (M = 300, 385); seed 0 drops none
WIDTHS = [96, 128]
SHAPES = [(1, 128), (17, 128), (147, 128), (300, 150), (385, 128)]
CASES = [(Cd, M, rps, True) for Cd in WIDTHS for M, rps in SHAPES] + [(Cd, 300, 150, False) for Cd in WIDTHS]     # (C, M, rows_per_scale, with row_scale)
NAMES = ("dw1", "db1", "dw2", "db2")
L1_BF16, MAX_BOUND = 3e-3, 1e-2  # the project's bounds on the unfused MX kernels in bf16 storage (tests/test_gpu_linear_mxfp8_bwd.py)
MARGIN = 1.5                     # the sibling tests' margin for differing fp32 orders
FLOOR = 1e-6                     # fp32-versus-fp64 accumulation level of emulate_wgrad_mx (tests/test_cpu_linear_mxfp8_bwd_recipe.py)
SEPARATION = 3.0                 # the bf16 weight gradients are at least this many times farther from the MX emulation (the sibling tests' floor)


def _supported(Cd):
    return hip.load().sv_swin_mlp_wgrad_mx_supported(Cd) == 1


def _quant_rows(w):
    N, K = w.shape
    Kp = (K + 127) // 128 * 128
    q = torch.empty(N, Kp, dtype=torch.uint8, device=w.device)
    s = torch.empty(N, Kp // 32, dtype=torch.uint8, device=w.device)
    call("sv_quant_rows_mx_e4m3", ptr(w), hip.BF16 if w.dtype == torch.bfloat16 else hip.F32, N, K, K, ptr(q), Kp, ptr(s))
    return q, s


def _quant_cols(w, colsum=None):
    """the MX rows of w^T: [K][roundup(N, 128)] bytes, a block = 32 consecutive rows n of one column k; colsum += the column sums"""
    N, K = w.shape
    Np = (N + 127) // 128 * 128
    q = torch.empty(K, Np, dtype=torch.uint8, device=w.device)
    s = torch.empty(K, Np // 32, dtype=torch.uint8, device=w.device)
    call("sv_quant_cols_mx_e4m3", ptr(w), hip.BF16 if w.dtype == torch.bfloat16 else hip.F32, N, K, K, ptr(q), Np, ptr(s), ptr(colsum))
    return q, s


def _upload(c, dx2, dev):
    d = {k: (v.to(dev).contiguous() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    d["dx2"] = dx2.to(dev).contiguous()
    d["w1"], d["w2t"] = _quant_rows(d["W1"]), _quant_cols(d["W2"])
    return d


def _sizes(Cd):
    return (4 * Cd * Cd, 4 * Cd, 4 * Cd * Cd, Cd)


def _prefill_cpu(Cd):
    """what dw1, db1, dw2, db2 hold before the launch: the kernels ADD to it"""
    g = torch.Generator().manual_seed(41 + Cd)
    return [torch.randn(n, generator=g) for n in _sizes(Cd)]


def _outs(Cd, dev):
    bufs = []
    for pre in _prefill_cpu(Cd):
        b = torch.full((pre.numel() + GUARD,), float("nan"), dtype=torch.float32)
        b[:pre.numel()] = pre
        bufs.append(b.to(dev))
    return bufs


def _harvest(bufs, Cd):
    """(values with the prefill on, guards intact)"""
    got = [b.cpu() for b in bufs]
    return [g[:n] for g, n in zip(got, _sizes(Cd))], all(bool(torch.isnan(g[n:]).all()) for g, n in zip(got, _sizes(Cd)))


def _unfused_counters():
    return (ops.linear_mxfp8_launches(), int(hip.load().sv_quant_cols_mx_launches()), int(hip.load().sv_quant_rows_mx_launches())) + ops.linear_mxfp8_bwd_launches()


def _fused_mx(d, M, Cd, dev):
    runs = []
    for _ in range(2):
        bufs = _outs(Cd, dev)
        n0, u0 = ops.swin_mlp_mx_wgrad_launches(), _unfused_counters()
        call("sv_swin_mlp_wgrad_mx", ptr(d["x1"]), ptr(d["dx2"]), ptr(d["ln_g"]), ptr(d["ln_b"]), ptr(d["w1"][0]), ptr(d["w1"][1]), ptr(d["w2t"][0]),
             ptr(d["w2t"][1]), ptr(d["b1"]), ptr(d["row_scale"]), d["rows_per_scale"], *(ptr(b) for b in bufs), M, Cd, d["eps"])
        torch.cuda.synchronize()
        assert ops.swin_mlp_mx_wgrad_launches() == n0 + 1 and _unfused_counters() == u0     # one launch, the unfused MX counters at rest
        runs.append(_harvest(bufs, Cd))
    return runs


def _fused_bf16(d, M, Cd, dev):
    bufs = _outs(Cd, dev)
    w1r, w2tr = d["W1"].bfloat16().contiguous(), d["W2"].t().contiguous().bfloat16()
    call("sv_swin_mlp_wgrad", ptr(d["x1"]), ptr(d["dx2"]), ptr(d["ln_g"]), ptr(d["ln_b"]), ptr(w1r), ptr(w2tr), ptr(d["b1"]), ptr(d["row_scale"]),
         d["rows_per_scale"], *(ptr(b) for b in bufs), M, Cd, d["eps"])
    torch.cuda.synchronize()
    vals, intact = _harvest(bufs, Cd)
    assert intact
    return vals


def _unfused_chain(d, M, Cd, dev):
    """The parent's MX chain in bf16 storage: sv_layernorm_quant_mx_fwd -> sv_linear_mxfp8 (GELU, pre_act, bf16 h) -> sv_rowscale ->
    sv_quant_rows_mx_e4m3 -> sv_linear_mxfp8_dgrad (GELU' at hpre) -> sv_quant_cols_mx_e4m3 x 4 (colsum = db2 / db1) -> sv_linear_mxfp8_wgrad x 2."""
    HID = 4 * Cd
    bf = dict(dtype=torch.bfloat16, device=dev)
    ln = torch.empty(M, Cd, **bf)
    mean, rstd = torch.empty(M, device=dev), torch.empty(M, device=dev)
    q = torch.empty(M, 128, dtype=torch.uint8, device=dev)
    s = torch.empty(M, 4, dtype=torch.uint8, device=dev)
    call("sv_layernorm_quant_mx_fwd", ptr(d["x1"]), ptr(d["ln_g"]), ptr(d["ln_b"]), ptr(ln), ptr(mean), ptr(rstd), ptr(q), 128, ptr(s), M, Cd, d["eps"], 0, 0,
         act=hip.BF16)
    h, hpre = torch.empty(M, HID, **bf), torch.empty(M, HID, **bf)
    e1 = ops._epilogue(HID, bias=d["b1"], act=hip.ACT_GELU, pre_act=hpre)
    call("sv_linear_mxfp8", ptr(q), ptr(s), ptr(d["w1"][0]), ptr(d["w1"][1]), ptr(h), M, Cd, HID, C_.byref(e1), None, None, act=hip.BF16)
    dbr = d["dx2"]
    if d["row_scale"] is not None:
        dbr = torch.empty(M, Cd, **bf)
        call("sv_rowscale", ptr(d["dx2"]), ptr(d["row_scale"]), ptr(dbr), M, Cd, d["rows_per_scale"], act=hip.BF16)
    dq, ds = _quant_rows(dbr)
    dh = torch.empty(M, HID, **bf)
    e2 = ops._epilogue(HID, act_grad_src=hpre, act_grad_kind=hip.ACT_GELU)
    call("sv_linear_mxfp8_dgrad", ptr(dq), ptr(ds), ptr(d["w2t"][0]), ptr(d["w2t"][1]), ptr(dh), M, Cd, HID, C_.byref(e2), act=hip.BF16)
    dw1, db1, dw2, db2 = bufs = _outs(Cd, dev)
    dbt, lnt = _quant_cols(dbr, colsum=db2), _quant_cols(ln)
    ht, dht = _quant_cols(h), _quant_cols(dh, colsum=db1)
    lib = hip.load()
    for (dyt, dys), (xt, xs), dw, N, K in ((dbt, ht, dw2, Cd, HID), (dht, lnt, dw1, HID, Cd)):
        nws = int(lib.sv_linear_mxfp8_wgrad_workspace_floats(M, N, K, 0))
        ws = torch.empty(max(nws, 1), dtype=torch.float32, device=dev)
        call("sv_linear_mxfp8_wgrad", ptr(dyt), ptr(dys), ptr(xt), ptr(xs), ptr(dw), M, N, K, K, 0, ptr(ws) if nws else None)
    torch.cuda.synchronize()
    vals, intact = _harvest(bufs, Cd)
    assert intact
    return vals


_RUNS = {}


def _runs(dev, Cd, M, rps, scaled):
    """emulation, MX fused kernel (twice), unfused MX chain and bf16 fused kernel on one case: computed once, left unchanged"""
    key = (Cd, M, rps, scaled)
    if key not in _RUNS:
        c = gauss_mlp_case(M, Cd, seed=SEED, windows=rps if scaled else None)
        dx2 = dgrad_seed(c["x1"])
        d = _upload(c, dx2, dev)
        ref = emulate_swin_mlp_wgrad_mx(dx2=dx2, **c)
        ref = [ref[0].flatten(), ref[1], ref[2].flatten(), ref[3]]
        pre = [p.double() for p in _prefill_cpu(Cd)]
        _RUNS[key] = dict(c=c, ref=ref, pre=pre, mx=_fused_mx(d, M, Cd, dev), chain=_unfused_chain(d, M, Cd, dev), bf16=_fused_bf16(d, M, Cd, dev))
    return _RUNS[key]


def _net(vals, r):
    """the four gradients of one run in fp64, the prefill taken off"""
    return [v.double() - p for v, p in zip(vals, r["pre"])]


def _dist(got, ref):
    return l1_rel(got, ref), float((got - ref).abs().max() / ref.abs().max())


def test_the_seed_gives_dropped_and_live_groups():
    for Cd in WIDTHS:
        hits = 0
        for M, rps in SHAPES:
            rs = gauss_mlp_case(M, Cd, seed=SEED, windows=rps)["row_scale"]
            hits += bool((rs == 0).any()) and bool((rs != 0).any())
        assert hits >= 1, Cd


@pytest.mark.gpu
@pytest.mark.parametrize("Cd,M,rps,scaled", CASES)
def test_kernel_against_the_chain_and_the_emulation(dev, Cd, M, rps, scaled):
    """dw1, db1, dw2, db2: the unfused MX chain meets the project's bounds against the emulation, and the fused kernel stays within 1.5 x
    max(d_chain, 1e-6) of the emulation, mean (L1-relative) and worst element.  The fused-versus-chain distance is printed."""
    if not _supported(Cd):
        return
    r = _runs(dev, Cd, M, rps, scaled)
    mx, chain = _net(r["mx"][0][0], r), _net(r["chain"], r)
    for name, got, ch, ref in zip(NAMES, mx, chain, r["ref"]):
        assert bool(torch.isfinite(got).all()), name
        (l1, wm), (l1c, wmc) = _dist(got, ref), _dist(ch, ref)
        fl1, fwm = (_dist(got, ch) if float(ch.abs().max()) > 0 else (0.0, 0.0))
        print(f"C={Cd} M={M} rps={rps} row_scale={scaled} {name}: fused MX vs emulation L1-rel {l1:.3e} worst {wm:.3e}; unfused MX chain vs emulation "
              f"L1-rel {l1c:.3e} worst {wmc:.3e}; fused vs chain L1-rel {fl1:.3e} worst {fwm:.3e}")
        assert l1c <= L1_BF16 and wmc <= MAX_BOUND, (name, l1c, wmc)            # the chain meets the project's bounds
        assert l1 <= MARGIN * max(l1c, FLOOR), (name, l1, l1c)
        assert wm <= MARGIN * max(wmc, FLOOR), (name, wm, wmc)


@pytest.mark.gpu
@pytest.mark.parametrize("Cd,M,rps,scaled", CASES)
def test_it_is_the_mx_gradient_not_the_bf16_one(dev, Cd, M, rps, scaled):
    """On dw1, db1 and dw2 the MX kernel is at least SEPARATION x closer to the MX emulation than sv_swin_mlp_wgrad is (db2 does not depend on the
    recipe)."""
    if not _supported(Cd):
        return
    r = _runs(dev, Cd, M, rps, scaled)
    mx, bf = _net(r["mx"][0][0], r), _net(r["bf16"], r)
    for name, got, b, ref in list(zip(NAMES, mx, bf, r["ref"]))[:3]:
        d_mx, d_bf16 = l1_rel(got, ref), l1_rel(b, ref)
        print(f"C={Cd} M={M} rps={rps} row_scale={scaled} {name}: distance from the MX emulation: fused MX {d_mx:.3e}, fused bf16 {d_bf16:.3e} "
              f"({d_bf16 / max(d_mx, 1e-30):.1f} x)")
        assert d_bf16 >= SEPARATION * d_mx, (name, d_mx, d_bf16)


@pytest.mark.gpu
@pytest.mark.parametrize("Cd,M,rps,scaled", CASES)
def test_accumulating_and_guarded(dev, Cd, M, rps, scaled):
    if not _supported(Cd):
        return
    r = _runs(dev, Cd, M, rps, scaled)
    (a, a_intact), (b, b_intact) = r["mx"]
    assert a_intact and b_intact                                                # NaN guards behind every output buffer
    assert all(bool(torch.isfinite(t).all()) for t in a + b)
    if M <= 128:                                                                # one token split: one atomic per element, bit-repeatable
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the gradients were ADDED to the prefill: taken off, they are the emulation's; left on, they are not
    # (mean distances against the mean size of the N(0, 1) prefill: the gradients themselves range from 1e-2 at M = 1 to 60 at M = 385)
    for name, got, pre, ref in zip(NAMES, _net(a, r), r["pre"], r["ref"]):
        size = float(pre.abs().mean())
        assert float((got - ref).abs().mean()) <= 0.05 * size, name
        assert float((got + pre - ref).abs().mean()) >= 0.5 * size, name
    if scaled and bool((r["c"]["row_scale"] == 0).any()):                       # dropped groups: all-zero column blocks (byte 127) beside live ones
        assert bool((r["c"]["row_scale"] != 0).any())


# ---- host switch ------------------------------------------------------------------------------------------------------------------------
IMGS, RES = 2, 7                 # M = 98: one token tile and one token split of either weight-gradient kernel, whose float atomics are then order-free


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
    return (ops.swin_mlp_mx_wgrad_launches(), ops.swin_mlp_mx_bwd_launches(), ops.swin_mlp_mx_launches(), ops.linear_mxfp8_launches(),
            ops.mx_act_quant_launches()) + ops.linear_mxfp8_bwd_launches()


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


@pytest.fixture
def traced(monkeypatch):
    """the names that go through ops.traced_call, in order: the fused MLP kernels and every Swin linear are launched through it"""
    names = []
    real = ops.traced_call

    def spy(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)

    monkeypatch.setattr(ops, "traced_call", spy)
    return names


def _step(blk, x, dy, traced):
    from swinvox_amd.models import swin_transformer as st
    grads = {p: torch.zeros_like(p, dtype=torch.float32) for p in blk.parameters()}
    ops.set_pack_cache(ops.PackCache())
    del traced[:]
    n0 = _counters()
    x2, ctx = st.block_forward(blk, x, IMGS, True, False, None, True)
    dx = st.block_backward(blk, ctx, dy.clone(), grads)
    torch.cuda.synchronize()
    n = _delta(n0, _counters())
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    mlp = blk.mlp
    wg = [grads[p].cpu() for p in (mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias)]
    ln = [grads[p].cpu() for p in (blk.norm2.weight, blk.norm2.bias)]
    rest = {k: grads[p].cpu() for k, p in blk.named_parameters() if not k.startswith(("mlp.", "norm2."))}
    return dict(x2=x2.cpu(), dx=dx.cpu(), n=n, wg=wg, ln=ln, rest=rest, names=list(traced))


ORDER_LEVEL = 1e-5               # L1-relative: two fp32 summation orders of the same addends


def _same_other_gradients(a, b, what):
    """norm2's gradients come from the same sv_swin_mlp_bwd launch on the same inputs, the attention branch's (norm1, qkv, proj, bias table) from a
    bit-identical dx1 - through kernels that add with float atomics (in LDS among the waves of a workgroup, in memory across workgroups), so the parent
    does not repeat ITSELF bit for bit there: equal up to the fp32 order of those sums.  Bit-identical where the float atomics leave one order."""
    worst = 0.0
    pairs = [(k, a["rest"][k], b["rest"][k]) for k in a["rest"]] + [(f"norm2[{i}]", x, y) for i, (x, y) in enumerate(zip(a["ln"], b["ln"]))]
    for k, x, y in pairs:
        d = l1_rel(x.double(), y.double())
        worst = max(worst, d)
        assert d <= ORDER_LEVEL, (what, k, d)
    print(f"{what}: norm and attention-branch gradients, worst L1-rel distance {worst:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("Cd,heads", [(96, 3), (128, 4)])
def test_host_switch(dev, switches, traced, Cd, heads):
    blk, x, dy = _block(dev, Cd, heads)
    ops.set_math("bf16")
    ops.set_storage("bf16")
    S.set_linear_fp8(True, backward=True, recipe="mx", backward_recipe="mx")
    ops.set_fused_mlp_mx(True)                                                  # the parent's MX training mode: MX forward, bf16 fused backward
    assert ops.fused_mlp_mx_enabled(Cd) and not ops.fused_mlp_mx_wgrad_enabled(Cd)   # off by default
    off = _step(blk, x, dy, traced)
    assert off["n"][0] == 0 and off["names"].count("sv_swin_mlp_wgrad") == 1 and "sv_swin_mlp_wgrad_mx" not in off["names"]
    ops.set_fused_mlp_mx(True, wgrad=True)
    if not _supported(Cd):
        assert not ops.fused_mlp_mx_wgrad_enabled(Cd)                           # the host keeps the bf16 weight gradients
        same = _step(blk, x, dy, traced)
        assert same["n"] == off["n"] and same["names"] == off["names"] and all(torch.equal(a, b) for a, b in zip(same["wg"], off["wg"]))
        return
    assert ops.fused_mlp_mx_wgrad_enabled(Cd) and not ops.fused_mlp_mx_bwd_enabled(Cd)
    on = _step(blk, x, dy, traced)
    assert on["n"][0] == 1, on["n"]                                             # one sv_swin_mlp_wgrad_mx launch per block backward
    assert on["n"][1:] == off["n"][1:], (on["n"], off["n"])                     # no MX GEMM or activation quantiser launch added
    assert on["names"].count("sv_swin_mlp_wgrad_mx") == 1 and "sv_swin_mlp_wgrad" not in on["names"]
    assert [n for n in on["names"] if n != "sv_swin_mlp_wgrad_mx"] == [n for n in off["names"] if n != "sv_swin_mlp_wgrad"]
    assert torch.equal(on["x2"], off["x2"]) and torch.equal(on["dx"], off["dx"])     # forward and data gradient: the same launches, bit for bit
    _same_other_gradients(on, off, f"C={Cd} on vs off")
    for name, a, b in zip(NAMES, on["wg"], off["wg"]):
        d = l1_rel(a.double(), b.double())
        print(f"C={Cd}: block {name}, fused MX vs fused bf16 weight gradients of the MLP: L1-rel {d:.3e}")
        if name != "db2":
            assert not torch.equal(a, b), name                                  # the MX weight gradients really ran
        assert d < 4 * 3.7e-2, (name, d)                                        # the same gradient under another rounding (as the sibling test bounds it)
    ops.set_fused_mlp_mx(True, backward=True, wgrad=True)                       # independent of the data-gradient switch: same weight gradients
    both = _step(blk, x, dy, traced)
    assert both["n"][0] == 1 and both["n"][1] == (1 if ops.fused_mlp_mx_bwd_enabled(Cd) else 0)
    assert all(torch.equal(a, b) for a, b in zip(both["wg"], on["wg"]))
    ops.set_fused_mlp_mx(True)                                                  # off again: the parent's launches and results, bit for bit
    off2 = _step(blk, x, dy, traced)
    assert off2["n"] == off["n"] and off2["names"] == off["names"] and torch.equal(off2["dx"], off["dx"])
    assert all(torch.equal(a, b) for a, b in zip(off2["wg"], off["wg"]))
    _same_other_gradients(off2, off, f"C={Cd} off again vs off")


@pytest.mark.gpu
def test_switch_is_inert_elsewhere(dev, switches, traced):
    blk, x, dy = _block(dev, 96, 3)
    ops.set_math("bf16")
    ops.set_storage("bf16")

    def pair(configure, **blockargs):
        """the same step with the weight-gradient switch off and on under one configuration: equal launches, equal results, counter at rest"""
        b, xx, dd = _block(dev, **blockargs) if blockargs else (blk, x, dy)
        ops.set_fused_mlp_mx(True)
        configure()
        a0 = _step(b, xx, dd, traced)
        ops.set_fused_mlp_mx(True, wgrad=True)
        configure()
        assert not ops.fused_mlp_mx_wgrad_enabled(b.dim)
        a1 = _step(b, xx, dd, traced)
        assert a1["n"][0] == 0 and a1["n"] == a0["n"] and a1["names"] == a0["names"], (a0["n"], a1["n"])
        assert torch.equal(a1["dx"], a0["dx"]) and torch.equal(a1["x2"], a0["x2"])
        assert all(torch.equal(p, q) for p, q in zip(a1["wg"], a0["wg"]))

    pair(lambda: S.set_linear_fp8(True, backward=True, recipe="mx", backward_recipe="row"))       # the row backward recipe
    pair(lambda: S.set_linear_fp8(True, backward=False, recipe="mx"))                             # no fp8 backward at all
    pair(lambda: S.set_linear_fp8(True, backward=True, recipe="row", backward_recipe="mx"))       # the row forward recipe
    pair(lambda: S.set_linear_fp8(True, backward=True, recipe="mx", backward_recipe="mx"), Cd=192, heads=6)     # C = 192
    S.set_linear_fp8(True, backward=True, recipe="mx", backward_recipe="mx")
    ops.set_fused_mlp_mx(False, wgrad=True)                                                       # the forward switch off
    assert not ops.fused_mlp_mx_wgrad_enabled(96)
    b0 = _step(blk, x, dy, traced)
    ops.set_fused_mlp_mx(False)
    b1 = _step(blk, x, dy, traced)
    assert b0["n"][0] == 0 and b0["n"] == b1["n"] and b0["names"] == b1["names"] and all(torch.equal(p, q) for p, q in zip(b0["wg"], b1["wg"]))
    ops.set_fused_mlp_mx(True, wgrad=True)
    ops.set_math("f32")                                                                           # f32 math (and with it f32 storage)
    assert not ops.fused_mlp_mx_wgrad_enabled(96) and not ops.fused_mlp_mx_enabled(96)
    c1 = _step(blk, x.float(), dy.float(), traced)
    ops.set_fused_mlp_mx(False)
    c0 = _step(blk, x.float(), dy.float(), traced)
    assert c1["n"][0] == 0 and c1["n"] == c0["n"] and c1["names"] == c0["names"] and all(torch.equal(p, q) for p, q in zip(c1["wg"], c0["wg"]))
