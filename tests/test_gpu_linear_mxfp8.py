"""MX form of the fp8 Swin linears (csrc/linear_fp8.hip: sv_quant_rows_mx_e4m3, sv_linear_mxfp8) through the C ABI against the recipe's torch
emulation (tests/test_cpu_linear_mxfp8_recipe.py, which pins that emulation on the CPU).  The exact-integer test with non-unit block scales
establishes the lane map of the MFMA's scale operands; the bounds are those of tests/test_gpu_linear_fp8.py (same accumulate structure)."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_linear_fp8_recipe import INT_SHAPES, RECIPE_SHAPES, gauss_case, l1_rel, nan_padded, raw_bytes  # noqa: E402
from test_cpu_linear_mxfp8_recipe import emulate_linear_mx, mx_dequant, mx_integer_case, mx_quant_rows  # noqa: E402

from swinvox_amd import hip, ops  # noqa: E402
from swinvox_amd.ops import call, ptr  # noqa: E402

L1_F32, L1_BF16 = 1e-4, 3e-3     # tests/test_gpu_linear_fp8.py: fp32 arithmetic of the epilogue / the bf16 rounding of the stored output
MAX_BOUND = 1e-2                 # worst element, relative to max|ref|
SEPARATION = 1.5e-2              # the row-recipe kernel and the bf16 linear must be at least this far from the MX emulation
RPS = 49
GUARD = 2                        # guard rows behind every output


def _dt(store):
    return torch.bfloat16 if store == "bf16" else torch.float32


def _code(store):
    return hip.BF16 if store == "bf16" else hip.F32


def _quant(t, rows, K, ld=None):
    """sv_quant_rows_mx_e4m3 into poisoned buffers with GUARD rows behind them -> (bytes [rows + GUARD, Kp], scale bytes [rows + GUARD, Kp / 32])"""
    Kp = (K + 127) // 128 * 128
    q = torch.full((rows + GUARD, Kp), 0x7F, dtype=torch.uint8, device=t.device)        # e4m3 NaN
    s = torch.full((rows + GUARD, Kp // 32), 0xFF, dtype=torch.uint8, device=t.device)  # E8M0 NaN: a byte the recipe never produces
    call("sv_quant_rows_mx_e4m3", ptr(t), hip.BF16 if t.dtype == torch.bfloat16 else hip.F32, rows, K, ld or K, ptr(q), Kp, ptr(s))
    return q, s


def _guards_intact(q, s, rows):
    return bool((q[rows:] == 0x7F).all()) and bool((s[rows:] == 0xFF).all())


def _mx_linear(xq, xs, wq, ws, out, M, K, N, store, q_out=None, qs_out=None, **epi):
    e = ops._epilogue(epi.pop("ldc", N), **epi)
    call("sv_linear_mxfp8", ptr(xq), ptr(xs), ptr(wq), ptr(ws), ptr(out), M, K, N, C.byref(e), ptr(q_out), ptr(qs_out), act=_code(store))


# ---- 1. the quantiser -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K", [64, 96, 100, 192, 384, 3072])
@pytest.mark.parametrize("rows", [1, 37, 130])
def test_quantiser_is_the_emulation(dev, rows, K):
    """Bytes and scale bytes equal the emulation bit for bit, for fp32 and bf16 input and row strides K and K + 8; the values span 16 binades
    per tensor (a row factor and a block factor), so the scale bytes differ from block to block.  The guard rows keep their fill."""
    g = torch.Generator().manual_seed(rows * 10007 + K)
    x = torch.randn(rows, K, generator=g)
    x *= torch.exp2(torch.randint(-4, 5, (rows, 1), generator=g).float()) * torch.exp2(torch.randint(-4, 5, (1, K), generator=g).float())
    x[0, : min(K, 40)] = 0.0                                            # an all-zero block (and a partly zero one)
    n0 = ops.mx_act_quant_launches(), int(hip.load().sv_quant_rows_mx_launches())
    for dt in (torch.float32, torch.bfloat16):
        xs_ = x.to(dt)
        ref_q, ref_s = mx_quant_rows(xs_)
        for ld in (K, K + 8):
            buf = torch.full((rows, ld), float("nan"), dtype=dt, device=dev)
            buf[:, :K] = xs_.to(dev)
            q, s = _quant(buf, rows, K, ld)
            torch.cuda.synchronize()
            assert torch.equal(s[:rows].cpu(), ref_s), (dt, ld)
            assert torch.equal(q[:rows].cpu(), ref_q), (dt, ld, int((q[:rows].cpu() != ref_q).sum()))
            assert _guards_intact(q, s, rows), (dt, ld)
    assert int(hip.load().sv_quant_rows_mx_launches()) == n0[1] + 4 and ops.mx_act_quant_launches() == n0[0]     # the C counter, not the host's


# ---- 2. exact integers with non-unit block scales ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", INT_SHAPES + [(37, 99, 30)])
def test_exact_integers_with_block_scales(dev, shape):
    """Establishes the lane map of the MFMA's scale operands (which lane's byte scales which 32 k-values), the staging of the scale dwords
    (the W rows' permutation, the k-step stride) and the M / N / K edges: operand and scale bytes are built on the host, every partial sum is
    exact in fp32, so the result equals the fp32 product of the dequantised operands bit for bit.  Nothing beyond M rows / N columns is
    touched."""
    M, K, N = shape
    (xq, xs), (wq, ws) = mx_integer_case(M, K, N)
    ref = (mx_dequant(xq, xs) @ mx_dequant(wq, ws).T).float()
    ldc, rows_alloc = (N + 8 if N % 4 == 0 else N + 1), M + 3
    out = torch.full((rows_alloc, ldc), float("nan"), dtype=torch.float32, device=dev)
    n0 = ops.linear_mxfp8_launches(), ops.linear_fp8_launches()
    _mx_linear(xq.to(dev), xs.to(dev), wq.to(dev), ws.to(dev), out, M, K, N, "f32", ldc=ldc)
    torch.cuda.synchronize()
    assert (ops.linear_mxfp8_launches(), ops.linear_fp8_launches()) == (n0[0] + 1, n0[1])
    got = out.cpu()
    assert torch.equal(got[:M, :N], ref), (float((got[:M, :N] - ref).abs().max()), int((got[:M, :N] != ref).sum()))
    assert bool(torch.isnan(got[M:]).all()) and bool(torch.isnan(got[:, N:]).all())


# ---- 3. the recipe on N(0, 1) data ------------------------------------------------------------------------------------------------------
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
        c["refs"][form] = emulate_linear_mx(c["x"], c["W"], **kw)
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
    """Quantiser + GEMM against the CPU emulation reading the same stored inputs, for every epilogue form the Swin call sites use."""
    M, K, N = shape
    c = _case(shape, store)
    ref, ref_pre = _reference(c, form)
    out = torch.full((M, N), float("nan"), dtype=_dt(store), device=dev)
    pre = torch.full((M, N), float("nan"), dtype=_dt(store), device=dev) if form == "gelu" else None
    epi = {"none": {}, "bias": dict(bias=c["bias"].to(dev)),
           "gelu": dict(bias=c["bias"].to(dev), act=hip.ACT_GELU, pre_act=pre),
           "residual": dict(bias=c["bias"].to(dev), residual=c["res"].to(dev), ldr=N, row_scale=c["rs"].to(dev), rows_per_scale=RPS)}[form]
    xq, xs = _quant(c["x"].to(dev), M, K)
    wq, ws = _quant(c["W"].to(dev), N, K)
    n0 = ops.linear_mxfp8_launches()
    _mx_linear(xq, xs, wq, ws, out, M, K, N, store, **epi)
    torch.cuda.synchronize()
    assert ops.linear_mxfp8_launches() == n0 + 1
    _check(f"{shape} {store} {form}", out, ref, store)
    if pre is not None:
        _check(f"{shape} {store} {form} pre_act", pre, ref_pre, store)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["gelu", "residual"])
@pytest.mark.parametrize("store", ["f32", "bf16"])
def test_store_widths_agree(dev, store, form):
    """tests/test_gpu_linear_fp8.py's test of the same name on the MX kernel: ldc = ldr = 40 (16-byte pieces), 44 (4-element pieces under bf16
    storage) and 41 (single elements) give the same bytes of out and pre_act, and nothing outside [:M, :N] is written.  No tolerance."""
    M, K, N = 37, 99, 40
    x, W = gauss_case(M, K, N, seed=11)
    g = torch.Generator().manual_seed(79)
    bias = (0.5 * torch.randn(N, generator=g)).to(dev)
    res = torch.randn(M, N, generator=g).to(_dt(store))
    rs = (0.5 + torch.rand((M + RPS - 1) // RPS, generator=g)).to(dev)
    xq, xs = _quant(x.to(_dt(store)).to(dev), M, K)
    wq, ws = _quant(W.to(dev), N, K)
    runs = []
    for ld in (40, 44, 41):
        out = torch.full((M + 3, ld), float("nan"), dtype=_dt(store), device=dev)
        pre = torch.full((M + 3, ld), float("nan"), dtype=_dt(store), device=dev) if form == "gelu" else None
        epi = dict(bias=bias, act=hip.ACT_GELU, pre_act=pre) if form == "gelu" else \
            dict(bias=bias, residual=nan_padded(res, M + 3, ld, dev), ldr=ld, row_scale=rs, rows_per_scale=RPS)
        _mx_linear(xq, xs, wq, ws, out, M, K, N, store, ldc=ld, **epi)
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
def test_other_paths_are_separated_from_the_mx_recipe(dev, shape, store):
    """Without this the bounds above would not tell the kernels apart: the row-recipe kernel (sv_linear_fp8) and the engine's bf16-operand
    linear_fwd on the same stored inputs are >= 1.5e-2 (L1-relative) away from the MX emulation."""
    M, K, N = shape
    c = _case(shape, store)
    ref, _ = _reference(c, "none")
    x, W = c["x"].to(dev), c["W"].to(dev)
    out = torch.full((M, N), float("nan"), dtype=_dt(store), device=dev)
    xq, sx = ops.quantize_rows_fp8(x, M, K)
    wq, sw = ops.quantize_rows_fp8(W, N, K)
    call("sv_linear_fp8", ptr(xq), ptr(sx), ptr(wq), ptr(sw), ptr(out), M, K, N, C.byref(ops._epilogue(N)), act=_code(store))
    ops.set_math("bf16")
    ops.set_storage(store)
    try:
        out16 = ops.empty(M, N, device=dev)
        ops.linear_fwd(x, M, ops.ConvSpec.linear(K, N), W, out16)
        torch.cuda.synchronize()
    finally:
        ops.set_math("f32")
    d_row, d_bf16 = l1_rel(out.float().cpu(), ref), l1_rel(out16.float().cpu(), ref)
    print(f"{shape} {store}: row-recipe kernel vs the MX recipe {d_row:.3e}, bf16 linear_fwd vs the MX recipe {d_bf16:.3e}")
    assert d_row >= SEPARATION and d_bf16 >= SEPARATION, (d_row, d_bf16)


# ---- 4. emission of the output's own MX rows ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["plain", "gelu"])
@pytest.mark.parametrize("store", ["f32", "bf16"])
@pytest.mark.parametrize("K,N", [(96, 384), (192, 768)])
def test_emission_equals_the_quantiser_on_the_stored_output(dev, K, N, store, form):
    """q_out / qs_out are sv_quant_rows_mx_e4m3 of the stored `out`, bit for bit (M = 130: a ragged last tile), `out` and pre_act are what the
    call without emission stores, and the call with out = pre_act = NULL writes the same bytes.  Guard rows intact."""
    M = 130
    c = _case((M, K, N), store)
    x, W, bias = c["x"].to(dev), c["W"].to(dev), c["bias"].to(dev)
    xq, xs = _quant(x, M, K)
    wq, ws = _quant(W, N, K)

    def run(with_out, emit):
        out = torch.full((M + GUARD, N), float("nan"), dtype=_dt(store), device=dev) if with_out else None
        pre = torch.full((M + GUARD, N), float("nan"), dtype=_dt(store), device=dev) if (with_out and form == "gelu") else None
        q = torch.full((M + GUARD, N), 0x7F, dtype=torch.uint8, device=dev) if emit else None
        s = torch.full((M + GUARD, N // 32), 0xFF, dtype=torch.uint8, device=dev) if emit else None
        epi = dict(bias=bias, act=hip.ACT_GELU, pre_act=pre) if form == "gelu" else {}
        _mx_linear(xq, xs, wq, ws, out, M, K, N, store, q_out=q, qs_out=s, **epi)
        torch.cuda.synchronize()
        return out, pre, q, s

    out0, pre0, _, _ = run(True, False)
    out1, pre1, q1, s1 = run(True, True)
    _, _, q2, s2 = run(False, True)
    assert torch.equal(out0[:M].view(torch.uint8), out1[:M].view(torch.uint8))
    if pre0 is not None:
        assert torch.equal(pre0[:M].view(torch.uint8), pre1[:M].view(torch.uint8)) and bool(torch.isnan(pre1[M:]).all())
    assert bool(torch.isnan(out1[M:]).all())
    ref_q, ref_s = _quant(out1, M, N)
    torch.cuda.synchronize()
    for q, s in ((q1, s1), (q2, s2)):
        assert torch.equal(s[:M], ref_s[:M]) and torch.equal(q[:M], ref_q[:M]), int((q[:M] != ref_q[:M]).sum())
        assert _guards_intact(q, s, M)
    cq, cs = mx_quant_rows(out1[:M].cpu())                              # and the quantiser is the emulation on this tensor too
    assert torch.equal(q1[:M].cpu(), cq) and torch.equal(s1[:M].cpu(), cs)


# ---- 5. edge rows -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("store", ["f32", "bf16"])
def test_edge_rows(dev, store):
    """An all-zero activation row and an all-zero weight row: scale bytes 127, output = the bias path only.  A 1e-20 row beside a 1e20 row:
    block scales have no clamp to run into and no product of scales to overflow - both rows come out with the relative accuracy of any other."""
    M, K, N = 24, 96, 40
    x, W = gauss_case(M, K, N, seed=5)
    x[3] = 0.0
    W[7] = 0.0
    x[9] *= 1e-20
    x[10] *= 1e20
    x = x.to(_dt(store))
    bias = torch.linspace(-1, 1, N)
    ref, _ = emulate_linear_mx(x, W)
    out = torch.full((M, N), float("nan"), dtype=_dt(store), device=dev)
    outb = torch.full((M, N), float("nan"), dtype=_dt(store), device=dev)
    xq, xs = _quant(x.to(dev), M, K)
    wq, ws = _quant(W.to(dev), N, K)
    _mx_linear(xq, xs, wq, ws, out, M, K, N, store)
    _mx_linear(xq, xs, wq, ws, outb, M, K, N, store, bias=bias.to(dev))
    torch.cuda.synchronize()
    assert bool((xs[3] == 127).all()) and bool((ws[7] == 127).all()) and int(xq[3].max()) == 0
    got, gotb = out.float().cpu(), outb.float().cpu()
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(gotb).all())
    stored_bias = bias.to(_dt(store)).float()
    assert torch.equal(gotb[3], stored_bias) and torch.equal(gotb[:, 7], stored_bias[7].expand(M))
    bound = L1_BF16 if store == "bf16" else L1_F32
    for r in (9, 10, 11):
        d = l1_rel(got[r], ref[r])
        print(f"edge rows {store}: row {r} L1-rel {d:.3e}")
        assert d <= bound, (r, d)


# ---- 6. refusals on the GPU --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("what", ["stats", "act_grad_src", "col_off", "lrelu", "emit_residual", "emit_n", "no_out"])
def test_refusals(dev, what):
    M, K, N = 16, 128, (96 if what == "emit_n" else 128)
    x, W = gauss_case(M, K, N)
    out = torch.zeros(M, 2 * N, dtype=torch.float32, device=dev)
    dummy = torch.zeros(M * N * 2, dtype=torch.float64, device=dev)
    q = torch.zeros(M, N, dtype=torch.uint8, device=dev)
    s = torch.zeros(M, 4, dtype=torch.uint8, device=dev)
    epi = {"stats": dict(stats=dummy), "act_grad_src": dict(act_grad_src=dummy, act_grad_kind=hip.ACT_GELU),
           "col_off": dict(ldc=2 * N, col_off=N), "lrelu": dict(act=hip.ACT_LRELU, slope=0.2),
           "emit_residual": dict(residual=dummy, ldr=N), "emit_n": {}, "no_out": {}}[what]
    emit = what.startswith("emit")
    xq, xs = _quant(x.to(dev), M, K)
    wq, ws = _quant(W.to(dev), N, K)
    n0 = ops.linear_mxfp8_launches()
    with pytest.raises(RuntimeError, match="sv_linear_mxfp8"):
        _mx_linear(xq, xs, wq, ws, None if what == "no_out" else out, M, K, N, "f32", q_out=q if emit else None, qs_out=s if emit else None, **epi)
    assert ops.linear_mxfp8_launches() == n0


# ---- 7. switch semantics -----------------------------------------------------------------------------------------------------------------
def test_switch_semantics():
    import swinvox_amd as S
    try:
        ops.set_math("bf16")
        assert ops.linear_fp8_recipe() == "row"                                  # the default
        S.set_linear_fp8(True)
        assert ops.linear_fp8_enabled() and ops.linear_fp8_recipe() == "row" and ops.ln_quant_fused_enabled()
        S.set_linear_fp8(True, recipe="mx")
        assert ops.linear_fp8_enabled() and ops.linear_fp8_recipe() == "mx" and not ops.linear_fp8_bwd_enabled()
        assert not ops.ln_quant_fused_enabled() and ops.mx_producer_quant_enabled()
        assert ops.attention_math() == hip.MATH_BF16                              # independent of the attention switch
        S.set_linear_fp8(True, backward=True, recipe="mx")
        assert ops.linear_fp8_bwd_enabled()                                      # backward combines with either recipe
        ops.set_mx_producer_quant(False)
        assert not ops.mx_producer_quant_enabled()
        ops.set_mx_producer_quant(True)
        ops.set_math("f32")                                                      # inert under f32 math
        assert not ops.linear_fp8_enabled() and not ops.mx_producer_quant_enabled()
        ops.set_math("bf16")
        S.set_linear_fp8(True)                                                   # the keyword defaults back to the row recipe
        assert ops.linear_fp8_recipe() == "row"
        with pytest.raises(ValueError):
            S.set_linear_fp8(True, recipe="mxfp4")
    finally:
        S.set_linear_fp8(False)
        ops.set_mx_producer_quant(True)
        ops.set_math("f32")
