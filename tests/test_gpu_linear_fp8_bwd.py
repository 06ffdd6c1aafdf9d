"""fp8 backward of the Swin linears (csrc/linear_fp8.hip, ops.set_linear_fp8(True, backward=True)): the column quantiser, the data-gradient
and the weight-gradient kernel through the C ABI against the recipe's torch emulation (tests/test_cpu_linear_fp8_bwd_recipe.py, which pins
that emulation on the CPU), then the host switch, the routing inside the encoder, and a training smoke run."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_linear_fp8_recipe import l1_rel, quantize_rows, raw_bytes  # noqa: E402
from test_cpu_linear_fp8_bwd_recipe import emulate_dgrad, emulate_wgrad, gauss_bwd_case, integer_bwd_case  # noqa: E402

import swinvox_amd as S  # noqa: E402
from swinvox_amd import hip, ops  # noqa: E402
from swinvox_amd.ops import call, ptr  # noqa: E402

# Bounds of tests/test_gpu_linear_fp8.py (L1-relative over the tensor unless noted): fp32 against fp64 accumulation of the recipe is < 1e-6 and
# the epilogue adds a few fp32 roundings, so 1e-4 is > 100 x what fp32 arithmetic contributes and 350 x under the distance of a bf16-operand
# gradient from the recipe; with bf16 storage the output rounding alone is 1.4e-3.  dw is always fp32.
L1_F32, L1_BF16 = 1e-4, 3e-3
MAX_BOUND = 1e-2       # worst element, relative to max|ref|
SEPARATION = 1.5e-2    # the engine's bf16 gradients must be at least this far from the recipe (the CPU emulation is 3.5e-2 ... 3.75e-2 from exact)
COLSUM_BOUND = 1e-6    # column sums against fp64, worst element relative to max|ref| and L1-relative

INT_SHAPES = [(49, 96, 288), (401, 192, 192), (196, 384, 1536), (130, 1536, 384), (37, 99, 30)]      # (M, K, N)
RECIPE_SHAPES = INT_SHAPES + [(64, 3072, 768)]


def _dt(store):
    return torch.bfloat16 if store == "bf16" else torch.float32


def _code(t):
    return hip.BF16 if t.dtype == torch.bfloat16 else hip.F32


def _quant_rows(t, rows, K):
    Kp = (K + 127) // 128 * 128
    q = torch.full((rows, Kp), 0x7F, dtype=torch.uint8, device=t.device)
    s = torch.full((rows,), float("nan"), dtype=torch.float32, device=t.device)
    call("sv_quant_rows_e4m3", ptr(t), _code(t), rows, K, K, ptr(q), Kp, ptr(s))
    return q, s


def _quant_cols(t, M, Cc, ld=None, colsum=None):
    """the transposed copy [Cc][Mp] over NaN bytes (the kernel must write all Mp of every row) and the column scales"""
    Mp = (M + 127) // 128 * 128
    q = torch.full((Cc, Mp), 0x7F, dtype=torch.uint8, device=t.device)
    s = torch.full((Cc,), float("nan"), dtype=torch.float32, device=t.device)
    call("sv_quant_cols_e4m3", ptr(t), _code(t), M, Cc, ld or Cc, ptr(q), Mp, ptr(s), ptr(colsum))
    return q, s


def _dgrad(dy, W, dx, M, K, N, **epi):
    """dy [M, N] and W [N, K] on the device -> dx through the row quantiser, the column quantiser and sv_linear_fp8_dgrad"""
    dq, sd = _quant_rows(dy, M, N)
    wtq, swt = _quant_cols(W, N, K)
    e = ops._epilogue(epi.pop("ldc", K), **epi)
    call("sv_linear_fp8_dgrad", ptr(dq), ptr(sd), ptr(wtq), ptr(swt), ptr(dx), M, N, K, C.byref(e), act=_code(dx))


def _wgrad(dy, x, dw, M, K, N, ldw=None, splits=0):
    dyt, sdc = _quant_cols(dy, M, N)
    xt, sxc = _quant_cols(x, M, K)
    call("sv_linear_fp8_wgrad", ptr(dyt), ptr(sdc), ptr(xt), ptr(sxc), ptr(dw), M, N, K, ldw or K, splits)


# ---- 1. column quantiser --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("store", ["f32", "bf16"])
@pytest.mark.parametrize("Cc", [30, 96, 288])
@pytest.mark.parametrize("M", [37, 128, 401])
def test_column_quantiser(dev, M, Cc, store):
    """Values and scales equal the emulation's exactly, in the transposed layout with zero bytes past M, for fp32 and bf16 input and a row
    stride above C (C = 30: an odd one); the column sums for db against fp64 sums of the stored values.  Column 2 is all zero: scale 1.
    The 1e-6 on the sums is taken relative to max|ref| (worst element) and to sum|ref| (L1), not per element: a column whose sum nearly
    cancels cannot meet a per-element relative bound in fp32, whatever the summation order."""
    ld = Cc + (3 if Cc == 30 else 8 if Cc == 288 else 0)
    g = torch.Generator().manual_seed(M * 1000 + Cc)
    full = torch.randn(M, ld, generator=g).to(_dt(store))
    full[:, 2] = 0.0
    src = full[:, :Cc].float()
    q_ref, s_ref = quantize_rows(src.T.contiguous())                 # fp32 values of the e4m3 codes [Cc, Mp], scales [Cc]
    colsum = torch.zeros(Cc, dtype=torch.float32, device=dev)
    q, s = _quant_cols(full.to(dev), M, Cc, ld=ld, colsum=colsum)
    torch.cuda.synchronize()
    assert torch.equal(s.cpu(), s_ref) and float(s_ref[2]) == 1.0
    got = q.cpu().view(torch.float8_e4m3fn).float()
    assert got.shape == q_ref.shape and torch.equal(got, q_ref)
    if q.shape[1] > M:
        assert int(q.cpu()[:, M:].max()) == 0                         # padding: zero BYTES
    ref = src.double().sum(dim=0)
    err = (colsum.cpu().double() - ref).abs()
    print(f"M={M} C={Cc} {store}: column sums, worst element {float(err.max() / ref.abs().max()):.2e} of max|ref|, L1-rel {float(err.sum() / ref.abs().sum()):.2e}")
    assert float(err.max()) <= COLSUM_BOUND * float(ref.abs().max()) and float(err.sum()) <= COLSUM_BOUND * float(ref.abs().sum())


@pytest.mark.gpu
def test_column_sums_of_many_workgroups(dev):
    """M = 20 000 rows are 79 pass-1 workgroups per column: 79 fp32 atomic adds of fp64-summed partials, in any order.  Each add rounds the
    running sum by at most 2^-24 of it, so against the same norms the error is about sqrt(79) * 2^-24 / sqrt(3) = 3e-7 and the bound stays 1e-6.
    It grows with sqrt(M / 256): at the 1.6 M rows of stage 0 the same estimate gives 3e-6 - the fp32 bias gradient of the engine's kernels
    has that order too, and nothing smaller is claimed there."""
    M, Cc = 20000, 30
    src = torch.randn(M, Cc, generator=torch.Generator().manual_seed(31))
    colsum = torch.zeros(Cc, dtype=torch.float32, device=dev)
    q, s = _quant_cols(src.to(dev), M, Cc, colsum=colsum)
    torch.cuda.synchronize()
    q_ref, s_ref = quantize_rows(src.T.contiguous())
    assert torch.equal(s.cpu(), s_ref) and torch.equal(q.cpu().view(torch.float8_e4m3fn).float(), q_ref)
    ref = src.double().sum(dim=0)
    err = (colsum.cpu().double() - ref).abs()
    print(f"M={M} C={Cc}: column sums, worst element {float(err.max() / ref.abs().max()):.2e} of max|ref|, L1-rel {float(err.sum() / ref.abs().sum()):.2e}")
    assert float(err.max()) <= COLSUM_BOUND * float(ref.abs().max()) and float(err.sum()) <= COLSUM_BOUND * float(ref.abs().sum())


# ---- 2. exact integers ----------------------------------------------------------------------------------------------------------------
def _guarded(rows, cols, dev):
    """NaN-filled over-allocation: 3 extra rows, a row stride above cols (odd when cols is); returns (buffer, ld)"""
    ld = cols + 8 if cols % 4 == 0 else cols + 1
    return torch.full((rows + 3, ld), float("nan"), dtype=torch.float32, device=dev), ld


@pytest.mark.gpu
@pytest.mark.parametrize("shape", INT_SHAPES)
def test_exact_integers_dgrad(dev, shape):
    """Establishes the operand maps, the N padding, the M / K edges and the scale indexing of the data gradient: power-of-two scales, operands
    exact in e4m3, partial sums exact in fp32 - the result equals the fp32 product bit for bit, and nothing outside [M, K] is touched."""
    M, K, N = shape
    dy, _, W = integer_bwd_case(M, K, N)
    ref = (dy.double() @ W.double()).float()
    out, ldc = _guarded(M, K, dev)
    n0 = ops.linear_fp8_bwd_launches()
    _dgrad(dy.to(dev), W.to(dev), out, M, K, N, ldc=ldc)
    torch.cuda.synchronize()
    assert ops.linear_fp8_bwd_launches() == (n0[0] + 1, n0[1])
    got = out.cpu()
    assert torch.equal(got[:M, :K], ref), float((got[:M, :K] - ref).abs().max())
    assert bool(torch.isnan(got[M:]).all()) and bool(torch.isnan(got[:, K:]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("shape,splits", [(s, 0) for s in INT_SHAPES] + [((401, 192, 192), 1), ((401, 192, 192), 3), ((49, 96, 288), 1)])
def test_exact_integers_wgrad(dev, shape, splits):
    """The same for the weight gradient, added into a pre-filled integer dw.  M = 401 is four k-steps: one workgroup takes all (splits 1,
    plain read-add-write), three share them unevenly (1 + 1 + 2), 0 lets the library choose (4: one each)."""
    M, K, N = shape
    dy, x, _ = integer_bwd_case(M, K, N)
    g = torch.Generator().manual_seed(9)
    fill = torch.randint(-3, 4, (N, K), generator=g).float()
    ref = (dy.double().T @ x.double() + fill.double()).float()
    assert torch.equal(ref.double(), dy.double().T @ x.double() + fill.double())
    dw, ldw = _guarded(N, K, dev)
    dw[:N, :K] = fill.to(dev)
    n0, f0 = ops.linear_fp8_bwd_launches(), ops.linear_fp8_launches()
    _wgrad(dy.to(dev), x.to(dev), dw, M, K, N, ldw=ldw, splits=splits)
    torch.cuda.synchronize()
    assert ops.linear_fp8_bwd_launches() == (n0[0], n0[1] + 1) and ops.linear_fp8_launches() == f0
    got = dw.cpu()
    assert torch.equal(got[:N, :K], ref), float((got[:N, :K] - ref).abs().max())
    assert bool(torch.isnan(got[N:]).all()) and bool(torch.isnan(got[:, K:]).all())


# ---- 3. the recipe on N(0, 1) data ------------------------------------------------------------------------------------------------------
_CASES = {}


def _case(shape, store):
    """stored inputs of one (shape, storage) and their references, computed once and left unchanged"""
    key = (shape, store)
    if key not in _CASES:
        M, K, N = shape
        dy, x, W = gauss_bwd_case(M, K, N)
        hpre = 1.5 * torch.randn(M, K, generator=torch.Generator().manual_seed(78))
        _CASES[key] = dict(dy=dy.to(_dt(store)), x=x.to(_dt(store)), W=W, hpre=hpre.to(_dt(store)), refs={})
    return _CASES[key]


def _reference(c, what):
    if what not in c["refs"]:
        c["refs"][what] = {"dgrad": lambda: emulate_dgrad(c["dy"], c["W"]), "dgrad_gelu": lambda: emulate_dgrad(c["dy"], c["W"], hpre=c["hpre"]),
                           "wgrad": lambda: emulate_wgrad(c["dy"], c["x"])}[what]()
    return c["refs"][what]


def _check(name, got, ref, l1_bound):
    got, ref = got.float().cpu().double(), ref.double()
    l1, mx = l1_rel(got, ref), float((got - ref).abs().max() / ref.abs().max())
    print(f"{name}: L1-rel {l1:.3e}  worst element {mx:.3e} of max|ref|")
    assert bool(torch.isfinite(got).all())
    assert l1 <= l1_bound, (name, l1)
    assert mx <= MAX_BOUND, (name, mx)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["none", "gelu"])
@pytest.mark.parametrize("store", ["f32", "bf16"])
@pytest.mark.parametrize("shape", RECIPE_SHAPES)
def test_recipe_dgrad(dev, shape, store, form):
    """Kernel against the CPU emulation (fp32 scales and products, torch.float8_e4m3fn casts, fp64 contraction and epilogue, erf GELU
    derivative) reading the same stored inputs, plain and with fc2's act_grad_src."""
    M, K, N = shape
    c = _case(shape, store)
    ref = _reference(c, "dgrad" if form == "none" else "dgrad_gelu")
    out = torch.full((M, K), float("nan"), dtype=_dt(store), device=dev)
    epi = {} if form == "none" else dict(act_grad_src=c["hpre"].to(dev), act_grad_kind=hip.ACT_GELU)
    _dgrad(c["dy"].to(dev), c["W"].to(dev), out, M, K, N, **epi)
    torch.cuda.synchronize()
    _check(f"dgrad {shape} {store} {form}", out, ref, L1_BF16 if store == "bf16" else L1_F32)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["none", "gelu"])
@pytest.mark.parametrize("store", ["f32", "bf16"])
def test_store_widths_agree(dev, store, form):
    """The data gradient's two piece widths perform the same arithmetic per element: the same quantised operands with ldc = 40 (16-byte
    pieces) and 41 (single elements) give the same bytes of dx [37, 40], and nothing else of the NaN-filled buffers is written.  No tolerance."""
    M, K, N = 37, 40, 99
    dy, _, W = gauss_bwd_case(M, K, N, seed=11)
    hpre = (1.5 * torch.randn(M, K, generator=torch.Generator().manual_seed(80))).to(_dt(store))
    dq, sd = _quant_rows(dy.to(_dt(store)).to(dev), M, N)
    wtq, swt = _quant_cols(W.to(dev), N, K)
    runs = []
    for ld in (40, 41):
        out = torch.full((M + 3, ld), float("nan"), dtype=_dt(store), device=dev)
        epi = {}
        if form == "gelu":
            src = torch.full((M + 3, ld), float("nan"), dtype=_dt(store), device=dev)     # act_grad_src has the layout of the output
            src[:M, :K] = hpre.to(dev)
            epi = dict(act_grad_src=src, act_grad_kind=hip.ACT_GELU)
        e = ops._epilogue(ld, **epi)
        call("sv_linear_fp8_dgrad", ptr(dq), ptr(sd), ptr(wtq), ptr(swt), ptr(out), M, N, K, C.byref(e), act=_code(out))
        torch.cuda.synchronize()
        runs.append(out)
    for ld, t in zip((40, 41), runs):
        got, first = raw_bytes(t[:M, :K]), raw_bytes(runs[0][:M, :K])
        assert bool(torch.isfinite(t[:M, :K].float()).all()), ld
        assert torch.equal(got, first), (ld, int((got != first).sum()))
        assert bool(torch.isnan(t[M:]).all()) and bool(torch.isnan(t[:, K:]).all()), ld


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["f32", "bf16"])
@pytest.mark.parametrize("shape", RECIPE_SHAPES)
def test_recipe_wgrad(dev, shape, store):
    """dw is fp32 whatever the storage of dy and x: 1e-4; db from the same call sequence as the host layer runs it."""
    M, K, N = shape
    c = _case(shape, store)
    ref = _reference(c, "wgrad")
    dw = torch.zeros(N, K, dtype=torch.float32, device=dev)
    _wgrad(c["dy"].to(dev), c["x"].to(dev), dw, M, K, N)
    torch.cuda.synchronize()
    _check(f"wgrad {shape} {store}", dw, ref, L1_F32)


# ---- 4. separation ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("store", ["f32", "bf16"])
@pytest.mark.parametrize("shape", RECIPE_SHAPES)
def test_bf16_gradients_are_separated_from_the_recipe(dev, shape, store):
    """Without this the bounds above would not tell the two paths apart: the engine's bf16-operand linear_dgrad and linear_wgrad on the same
    stored inputs are >= 1.5e-2 (L1-relative) away from the recipe."""
    M, K, N = shape
    c = _case(shape, store)
    ops.set_math("bf16")
    ops.set_storage(store)
    try:
        spec = ops.ConvSpec.linear(K, N)
        dx = ops.empty(M, K, device=dev)
        dw = torch.zeros(N, K, dtype=torch.float32, device=dev)
        W = c["W"].to(dev)
        ops.linear_dgrad(c["dy"].to(dev), M, spec, spec.pack_dgrad(W), dx)
        ops.linear_wgrad(c["dy"].to(dev), c["x"].to(dev), M, spec, dw)
        torch.cuda.synchronize()
    finally:
        ops.set_math("f32")
    d_dx, d_dw = l1_rel(dx.float().cpu(), _reference(c, "dgrad")), l1_rel(dw.cpu(), _reference(c, "wgrad"))
    print(f"{shape} {store}: bf16 linear_dgrad vs the fp8 recipe {d_dx:.3e}, linear_wgrad {d_dw:.3e}")
    assert d_dx >= SEPARATION and d_dw >= SEPARATION, (d_dx, d_dw)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("what", ["stats", "bias", "residual", "act_grad_kind", "col_off"])
def test_refusals(dev, what):
    M, K, N = 16, 16, 128
    dy, _, W = gauss_bwd_case(M, K, N)
    out = torch.zeros(M, 2 * K, dtype=torch.float32, device=dev)
    dummy = torch.zeros(M * K * 2, dtype=torch.float64, device=dev)
    epi = {"stats": dict(stats=dummy), "bias": dict(bias=dummy), "residual": dict(residual=dummy, ldr=K),
           "act_grad_kind": dict(act_grad_src=dummy, act_grad_kind=hip.ACT_RELU), "col_off": dict(ldc=2 * K, col_off=K)}[what]
    e = ops._epilogue(epi.pop("ldc", K), **epi)
    lib = hip.load()
    ok = ops._epilogue(K, act_grad_src=dummy, act_grad_kind=hip.ACT_GELU)
    assert lib.sv_linear_fp8_dgrad_supported(N, K, C.byref(ops._epilogue(K)), hip.MATH_BF16, hip.F32) == 1
    assert lib.sv_linear_fp8_dgrad_supported(N, K, C.byref(ok), hip.MATH_BF16, hip.BF16) == 1
    assert lib.sv_linear_fp8_dgrad_supported(N, K, C.byref(e), hip.MATH_BF16, hip.F32) == 0
    assert lib.sv_linear_fp8_dgrad_supported(N, K, C.byref(ops._epilogue(K)), hip.MATH_F32, hip.F32) == 0
    dq, sd = _quant_rows(dy.to(dev), M, N)
    wtq, swt = _quant_cols(W.to(dev), N, K)
    n0, f0 = ops.linear_fp8_bwd_launches(), ops.linear_fp8_launches()
    with pytest.raises(RuntimeError, match="sv_linear_fp8_dgrad"):
        call("sv_linear_fp8_dgrad", ptr(dq), ptr(sd), ptr(wtq), ptr(swt), ptr(out), M, N, K, C.byref(e), act=hip.F32)
    assert ops.linear_fp8_bwd_launches() == n0 and ops.linear_fp8_launches() == f0


# ---- 6. switch semantics ----------------------------------------------------------------------------------------------------------------
def test_switch_semantics():
    try:
        ops.set_math("bf16")
        assert not ops.linear_fp8_enabled() and not ops.linear_fp8_bwd_enabled()      # off by default
        S.set_linear_fp8(False, backward=True)                   # backward alone does nothing
        assert not ops.linear_fp8_enabled() and not ops.linear_fp8_bwd_enabled()
        S.set_linear_fp8(True)                                   # today's meaning: the forward only
        assert ops.linear_fp8_enabled() and not ops.linear_fp8_bwd_enabled()
        S.set_linear_fp8(True, backward=True)
        assert ops.linear_fp8_enabled() and ops.linear_fp8_bwd_enabled()
        assert ops.attention_math() == hip.MATH_BF16 and ops.attention_bwd_math() == hip.MATH_BF16     # independent of the attention switch ...
        S.set_attention_fp8(True, backward=True)
        assert ops.linear_fp8_bwd_enabled() and ops.attention_bwd_math() == hip.MATH_FP8_FULL
        S.set_linear_fp8(True)                                   # ... in both directions; and back to forward-only
        assert ops.linear_fp8_enabled() and not ops.linear_fp8_bwd_enabled() and ops.attention_bwd_math() == hip.MATH_FP8_FULL
        S.set_attention_fp8(False)
        S.set_linear_fp8(True, backward=True)
        ops.set_math("f32")                                      # inert under f32 math
        assert not ops.linear_fp8_enabled() and not ops.linear_fp8_bwd_enabled()
    finally:
        S.set_linear_fp8(False)
        S.set_attention_fp8(False)
        ops.set_math("f32")
    assert not ops.linear_fp8_bwd_enabled()


# ---- 7. / 8. encoder runs ---------------------------------------------------------------------------------------------------------------
def _expected_fwd(enc):
    """sv_linear_fp8 launches of one forward under the CURRENT settings (the rule of tests/test_gpu_linear_fp8.py)"""
    n = 0
    for stage in enc.swin_transformer.model.stages():
        n += 0 if isinstance(stage.downsample, torch.nn.Identity) else 1
        for blk in stage.blocks:
            n += 0 if ops.fused_attn_block_enabled(blk.dim, blk.heads) else 2
            n += 0 if ops.fused_mlp_enabled(blk.dim) else 2
    return n


def _expected_bwd(enc):
    """launches of one backward under the CURRENT settings, each for dgrad and for wgrad: 2 per block whose attention branch runs the
    unfused backward, + 2 per block whose MLP is unfused, + 1 per patch merge"""
    n = 0
    for stage in enc.swin_transformer.model.stages():
        n += 0 if isinstance(stage.downsample, torch.nn.Identity) else 1
        for blk in stage.blocks:
            n += 0 if ops.fused_attn_block_bwd_enabled(blk.dim, blk.heads) else 2
            n += 0 if ops.fused_mlp_enabled(blk.dim) else 2
    return n


def _encoder_step(enc, x, monkeypatch=None, feats=None):
    """one forward + backward; returns (output, gradients by name, forward fp8 launches, the same counter's movement in the backward, the
    (dgrad, wgrad) launches of the backward).  With monkeypatch and a list, the Swin stage feature maps of the forward are appended to it."""
    from swinvox_amd.models import encoder as enc_mod
    real = enc_mod.swin_forward
    if feats is not None:
        def spy(*a, **k):
            f, tape = real(*a, **k)
            feats.extend(t.float().cpu() for t in f)
            return f, tape
        monkeypatch.setattr(enc_mod, "swin_forward", spy)
    enc.zero_grad(set_to_none=True)
    n0 = ops.linear_fp8_launches()
    out = enc(x)
    n1, b0 = ops.linear_fp8_launches(), ops.linear_fp8_bwd_launches()
    out.float().square().mean().backward()
    torch.cuda.synchronize()
    b1 = ops.linear_fp8_bwd_launches()
    if feats is not None:
        monkeypatch.setattr(enc_mod, "swin_forward", real)
    grads = {n: p.grad.detach().float().cpu() for n, p in enc.named_parameters() if p.grad is not None}
    return out.detach().float().cpu(), grads, n1 - n0, ops.linear_fp8_launches() - n1, (b1[0] - b0[0], b1[1] - b0[1])


def _set_mode(mode):
    S.set_math("f32" if mode == "f32" else "bf16")
    if mode != "f32":
        S.set_storage("bf16")
    S.set_linear_fp8(mode.startswith("fp8") or mode == "f32", backward="bwd" in mode or mode == "f32")       # under f32 math the switch is inert
    unfused = mode.endswith("unfused")
    ops.set_fused_attn_block(not unfused)
    ops.set_fused_attn_block_bwd(not unfused)
    ops.set_fused_mlp(not unfused)


def _reset_modes():
    S.set_linear_fp8(False)
    S.set_attention_fp8(False)
    ops.set_fused_attn_block(True)
    ops.set_fused_attn_block_bwd(True)
    ops.set_fused_mlp(True)
    S.set_math("f32")


@pytest.mark.gpu
def test_swin_t_encoder_modes(dev, monkeypatch):
    """Swin-T encoder, B = 1 x V = 2, bf16 storage, one forward + backward in exact f32, bf16, fp8 forward-only, fp8 with backward, and fp8
    with backward and the stage-0 fusions (attention forward and backward, MLP) off.  The counters prove the routing: forward counts as
    before, sv_linear_fp8_launches still in every backward, the (dgrad, wgrad) pair by the rule in the two backward modes and (0, 0) in every
    other, a bf16 step after the fp8 ones included.  Every gradient is finite.  The distance of the qkv / proj / fc1 / fc2 weight gradients
    of the first block of every stage from exact f32 is printed per mode.  A bound of 0.5 on them is out of reach of
    every mode on this weight set, the bf16 path included (measured: bf16 0.95 ... 1.07 per probed weight, as
    tests/test_gpu_attn_fp8_bwd.py records for Swin-B): bf16 storage alone moves these gradients by about their own size.  So the
    gradients are bounded as that file bounds them: the worst and the median distance over the 16 probed weights in the two fp8-backward
    modes may not exceed GRAD_FACTOR = 1.25 times the bf16 run's, i.e. the fp8 backward may not add more than a quarter to what bf16 storage
    already does.  0.5 is asserted on the stage feature maps, as tests/test_gpu_linear_fp8.py does."""
    from swinvox_amd import goldens
    from swinvox_amd.models import Encoder
    enc = Encoder(S.default_cfg())
    goldens.seeded_fill_(enc, 100)
    enc.to(dev).train()
    enc.stochastic = False
    x = goldens.synth_images(1, 2, 11).to(dev)
    names = {id(p): n for n, p in enc.named_parameters()}
    probes = [(f"stage {i} {k}", names[id(w)]) for i, st in enumerate(enc.swin_transformer.model.stages())
              for k, w in (("qkv", st.blocks[0].attn.qkv.weight), ("proj", st.blocks[0].attn.proj.weight), ("fc1", st.blocks[0].mlp.fc1.weight),
                           ("fc2", st.blocks[0].mlp.fc2.weight))]
    runs = {}
    try:
        for mode in ("f32", "bf16", "fp8", "fp8_bwd", "fp8_bwd_unfused", "bf16_again"):
            _set_mode(mode)
            want_f = _expected_fwd(enc) if mode.startswith("fp8") else 0
            want_b = _expected_bwd(enc) if "bwd" in mode else 0
            feats = []
            out, grads, fwd, fwd_in_bwd, bwd = _encoder_step(enc, x, monkeypatch, feats)
            print(f"{mode}: {fwd} fp8 launches in the forward (expected {want_f}); backward: {fwd_in_bwd} forward-kernel, {bwd} (dgrad, wgrad) launches "
                  f"(expected {want_b} each)")
            assert fwd == want_f and fwd_in_bwd == 0 and bwd == (want_b, want_b), (mode, fwd, want_f, fwd_in_bwd, bwd, want_b)
            assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(t).all()) for t in grads.values()), mode
            assert len(feats) == 4
            runs[mode] = (grads, fwd, bwd, feats)
    finally:
        _reset_modes()
    # Swin-T: 12 blocks, 3 patch merges; stage 0 (2 blocks) is fused by default, forward and backward
    assert runs["fp8_bwd"][1] == 4 * 10 + 3 and runs["fp8_bwd"][2] == (4 * 10 + 3,) * 2
    assert runs["fp8_bwd_unfused"][1] == 4 * 12 + 3 and runs["fp8_bwd_unfused"][2] == (4 * 12 + 3,) * 2
    gstats = {}
    for mode in ("bf16", "fp8", "fp8_bwd", "fp8_bwd_unfused"):
        d = {k: l1_rel(runs[mode][0][n], runs["f32"][0][n]) for k, n in probes}
        print(f"{mode}: weight gradients vs exact f32, L1-rel " + ", ".join(f"{k} {v:.3e}" for k, v in d.items()))
        df = [l1_rel(a, b) for a, b in zip(runs[mode][3], runs["f32"][3])]
        print(f"{mode}: stage feature maps vs exact f32, L1-rel {[f'{v:.3e}' for v in df]}")
        assert max(df) < 0.5, (mode, df)
        v = sorted(d.values())
        gstats[mode] = (v[-1], v[len(v) // 2])
    for mode in ("fp8_bwd", "fp8_bwd_unfused"):
        for k in (0, 1):
            assert gstats[mode][k] <= GRAD_FACTOR * gstats["bf16"][k], (mode, gstats)
    n = probes[4][1]       # stage 1 qkv: unfused in every mode
    assert not torch.equal(runs["fp8_bwd"][0][n], runs["fp8"][0][n])      # the backward switch changes the gradient ...
    assert not torch.equal(runs["fp8"][0][n], runs["bf16"][0][n])         # ... as the forward switch did


@pytest.mark.gpu
def test_swin_b_encoder_all_fp8_switches(dev):
    """BASELINE configuration 5 in training: Swin-B, fp8 attention and fp8 linears, forward and backward, one step at B = 1 x V = 1.  Counts by
    the rule (the fp8 attention backward unfuses every attention branch), everything finite."""
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
        S.set_linear_fp8(True, backward=True)
        want_f, want_b = _expected_fwd(enc), _expected_bwd(enc)
        fused_mlp = sum(1 for st in enc.swin_transformer.model.stages() for b in st.blocks if ops.fused_mlp_enabled(b.dim))
        out, grads, fwd, fwd_in_bwd, bwd = _encoder_step(enc, x)
    finally:
        _reset_modes()
    print(f"Swin-B: {fwd} fp8 linear launches forward, {bwd} (dgrad, wgrad) backward, {fused_mlp} blocks on the fused MLP")
    assert fwd == want_f == 4 * 24 + 3 - 2 * fused_mlp and fwd_in_bwd == 0
    assert bwd == (want_b, want_b) and want_b == 4 * 24 + 3 - 2 * fused_mlp
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(t).all()) for t in grads.values())


# ---- 9. training smoke ------------------------------------------------------------------------------------------------------------------
GRAD_FACTOR = 1.25     # the project's factors (tests/test_gpu_attn_fp8_bwd.py)
LOSS_FACTOR = 1.5
TAIL_FACTOR = 1.15


@pytest.mark.gpu
def test_training_smoke_fp8_linear_backward(dev):
    """test_training_smoke_fp8_linear's protocol with backward=True: whole pipeline, Swin-T, B = 2 x V = 2, one fixed batch, 20 flat-Adam steps
    in bf16 and with the fp8 linears forward and backward: the loss falls and stays finite, the final loss is within LOSS_FACTOR of the bf16
    run's, the mean of the last five steps within TAIL_FACTOR."""
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
    for mode in ("bf16", "fp8_linear_bwd"):
        torch.manual_seed(0)
        nets = [Encoder(cfg), Decoder(cfg), Merger(cfg), Refiner(cfg)]
        for n in nets:
            O.seeded_weights_(n, seed=7)
            n.to(dev).train()
        solvers, _ = harness.make_solvers(nets, cfg)
        S.set_math("bf16")
        S.set_storage("bf16")
        S.set_linear_fp8(mode != "bf16", backward=mode != "bf16")
        b0 = ops.linear_fp8_bwd_launches()
        try:
            losses = []
            for _ in range(20):
                el, rl = harness.train_step(nets, solvers, cfg, x, gt)
                losses.append(float(el + rl))
        finally:
            S.set_linear_fp8(False)
            S.set_math("f32")
        b1 = ops.linear_fp8_bwd_launches()
        print(f"{mode}: losses {[round(v, 4) for v in losses]}")
        assert (b1[0] - b0[0] > 0) == (b1[1] - b0[1] > 0) == (mode != "bf16")
        assert all(np.isfinite(losses)) and losses[-1] < losses[0], (mode, losses)
        final[mode] = (losses[-1], sum(losses[-5:]) / 5)
    assert final["fp8_linear_bwd"][0] < LOSS_FACTOR * final["bf16"][0], final
    assert final["fp8_linear_bwd"][1] < TAIL_FACTOR * final["bf16"][1], final
