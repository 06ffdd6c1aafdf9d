"""MX backward of the fp8 Swin linears (csrc/linear_fp8.hip, ops.set_linear_fp8(True, backward=True, backward_recipe="mx")): the one-launch
column quantiser, the data-gradient kernel and the atomic-free weight-gradient kernel through the C ABI against the recipe's torch emulation
(tests/test_cpu_linear_mxfp8_bwd_recipe.py, which pins that emulation on the CPU)."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_linear_fp8_recipe import l1_rel, raw_bytes  # noqa: E402
from test_cpu_linear_fp8_bwd_recipe import gauss_bwd_case  # noqa: E402
from test_cpu_linear_mxfp8_recipe import mx_dequant, mx_integer_case, mx_quant_rows  # noqa: E402
from test_cpu_linear_mxfp8_bwd_recipe import emulate_dgrad_mx, emulate_wgrad_mx, mx_quant_cols  # noqa: E402

from swinvox_amd import hip, ops  # noqa: E402
from swinvox_amd.ops import call, ptr  # noqa: E402

# the project's bounds (tests/test_gpu_linear_fp8_bwd.py, tests/test_gpu_linear_mxfp8.py)
L1_F32, L1_BF16 = 1e-4, 3e-3
MAX_BOUND = 1e-2       # worst element, relative to max|ref|
SEPARATION = 1.5e-2    # the row-recipe kernels and the bf16 engine must be at least this far from the MX emulation
COLSUM_BOUND = 1e-6    # column sums against fp64, worst element relative to max|ref|
GUARD = 2              # guard rows behind every quantiser output

INT_SHAPES = [(49, 96, 288), (401, 192, 192), (196, 384, 1536), (130, 1536, 384), (37, 99, 30)]      # (M, K, N)
RECIPE_SHAPES = INT_SHAPES + [(64, 3072, 768)]


def _dt(store):
    return torch.bfloat16 if store == "bf16" else torch.float32


def _code(t):
    return hip.BF16 if t.dtype == torch.bfloat16 else hip.F32


def _mx_counters():
    lib = hip.load()
    return ops.linear_mxfp8_bwd_launches() + (int(lib.sv_quant_cols_mx_launches()),)


def _row_counters():
    return ops.linear_fp8_bwd_launches() + (ops.linear_fp8_launches(), ops.linear_mxfp8_launches())


def _quant_cols(t, M, Cc, ld=None, colsum=None):
    """sv_quant_cols_mx_e4m3 into poisoned buffers with GUARD rows behind them -> (bytes [Cc + GUARD, Mp], scale bytes [Cc + GUARD, Mp / 32])"""
    Mp = (M + 127) // 128 * 128
    q = torch.full((Cc + GUARD, Mp), 0x7F, dtype=torch.uint8, device=t.device)          # e4m3 NaN
    s = torch.full((Cc + GUARD, Mp // 32), 0xFF, dtype=torch.uint8, device=t.device)    # E8M0 NaN: a byte the recipe never produces
    call("sv_quant_cols_mx_e4m3", ptr(t), _code(t), M, Cc, ld or Cc, ptr(q), Mp, ptr(s), ptr(colsum))
    return q, s


def _quant_rows(t, rows, K):
    Kp = (K + 127) // 128 * 128
    q = torch.full((rows, Kp), 0x7F, dtype=torch.uint8, device=t.device)
    s = torch.full((rows, Kp // 32), 0xFF, dtype=torch.uint8, device=t.device)
    call("sv_quant_rows_mx_e4m3", ptr(t), _code(t), rows, K, K, ptr(q), Kp, ptr(s))
    return q, s


def _dgrad_q(dq, ds, wtq, wts, dx, M, K, N, **epi):
    e = ops._epilogue(epi.pop("ldc", K), **epi)
    call("sv_linear_mxfp8_dgrad", ptr(dq), ptr(ds), ptr(wtq), ptr(wts), ptr(dx), M, N, K, C.byref(e), act=_code(dx))


def _dgrad(dy, W, dx, M, K, N, **epi):
    """dy [M, N] and W [N, K] on the device -> dx through the MX row quantiser, the MX column quantiser and sv_linear_mxfp8_dgrad"""
    dq, ds = _quant_rows(dy, M, N)
    wtq, wts = _quant_cols(W, N, K)
    _dgrad_q(dq, ds, wtq, wts, dx, M, K, N, **epi)


def _workspace(M, K, N, splits, dev):
    """NaN-filled workspace of the size the library asks for (at least one 16-byte piece, so the pointer is never NULL)"""
    n = int(hip.load().sv_linear_mxfp8_wgrad_workspace_floats(M, N, K, splits))
    return torch.full((max(n, 4),), float("nan"), dtype=torch.float32, device=dev), n


def _wgrad_q(dyt, dys, xt, xs, dw, M, K, N, ldw=None, splits=0):
    ws, n = _workspace(M, K, N, splits, dw.device)
    call("sv_linear_mxfp8_wgrad", ptr(dyt), ptr(dys), ptr(xt), ptr(xs), ptr(dw), M, N, K, ldw or K, splits, ptr(ws))
    return n


def _wgrad(dy, x, dw, M, K, N, ldw=None, splits=0):
    dyt, dys = _quant_cols(dy, M, N)
    xt, xs = _quant_cols(x, M, K)
    return _wgrad_q(dyt, dys, xt, xs, dw, M, K, N, ldw, splits)


# ---- 1. column quantiser --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("Cc", [30, 96, 288])
@pytest.mark.parametrize("M", [37, 128, 401])
def test_column_quantiser_is_the_row_quantiser_on_the_transpose(dev, M, Cc):
    """Bytes and scale bytes equal mx_quant_rows(t.T) bit for bit, for fp32 and bf16 input and the row strides C, C + 3 and C + 8.  The values
    span 16 binades (a row factor and a column factor), so the scale bytes differ from block to block; column 2 is all zero and column 5 has
    an all-zero first block.  M = 37 and 401 end in a partly filled block, followed by padding blocks (byte 127) and zero bytes.  The guard
    rows keep their fill, the column sums are within 1e-6 of max|ref| of the fp64 sums of the stored values, and the launch counter moves by
    the number of calls."""
    g = torch.Generator().manual_seed(M * 1000 + Cc)
    x = torch.randn(M, Cc, generator=g)
    x *= torch.exp2(torch.randint(-4, 5, (M, 1), generator=g).float()) * torch.exp2(torch.randint(-4, 5, (1, Cc), generator=g).float())
    x[:, 2] = 0.0
    x[:32, 5] = 0.0
    n0, r0 = _mx_counters(), _row_counters()
    calls = 0
    for dt in (torch.float32, torch.bfloat16):
        xs_ = x.to(dt)
        ref_q, ref_s = mx_quant_rows(xs_.T.contiguous())
        assert int(ref_s[2].min()) == 127 and int(ref_s[2].max()) == 127 and int(ref_s[5, 0]) == 127
        ref_sum = xs_.double().sum(dim=0)
        for ld in (Cc, Cc + 3, Cc + 8):
            buf = torch.full((M, ld), float("nan"), dtype=dt, device=dev)
            buf[:, :Cc] = xs_.to(dev)
            colsum = torch.zeros(Cc, dtype=torch.float32, device=dev)
            q, s = _quant_cols(buf, M, Cc, ld, colsum)
            torch.cuda.synchronize()
            calls += 1
            assert torch.equal(s[:Cc].cpu(), ref_s), (dt, ld, int((s[:Cc].cpu() != ref_s).sum()))
            assert torch.equal(q[:Cc].cpu(), ref_q), (dt, ld, int((q[:Cc].cpu() != ref_q).sum()))
            assert bool((q[Cc:] == 0x7F).all()) and bool((s[Cc:] == 0xFF).all()), (dt, ld)
            err = (colsum.cpu().double() - ref_sum).abs()
            print(f"M={M} C={Cc} {dt} ld={ld}: column sums, worst element {float(err.max() / ref_sum.abs().max()):.2e} of max|ref|")
            assert float(err.max()) <= COLSUM_BOUND * float(ref_sum.abs().max()), (dt, ld)
    n1 = _mx_counters()
    assert n1 == (n0[0], n0[1], n0[2] + calls) and _row_counters() == r0


@pytest.mark.gpu
def test_column_quantiser_on_a_weight_gives_the_dgrad_operand(dev):
    """On the [N, K] fp32 weight the output is the [K][Np] operand of the data gradient: blocks of 32 consecutive n of one column k."""
    N, K = 288, 96
    W = torch.randn(N, K, generator=torch.Generator().manual_seed(17)) * 0.05
    q, s = _quant_cols(W.to(dev), N, K)
    torch.cuda.synchronize()
    ref_q, ref_s = mx_quant_cols(W)
    assert ref_q.shape == (K, 384) and ref_s.shape == (K, 12)
    assert torch.equal(q[:K].cpu(), ref_q) and torch.equal(s[:K].cpu(), ref_s)
    assert int(q[:K, N:].max()) == 0 and bool((s[:K, 9:] == 127).all())
    assert l1_rel(mx_dequant(q[:K].cpu(), s[:K].cpu())[:, :N], W.T.double()) < 4e-2


# ---- 2. exact integers with non-unit block scales ---------------------------------------------------------------------------------------
def _guarded(rows, cols, dev):
    """NaN-filled over-allocation: 3 extra rows, a row stride above cols (odd when cols is); returns (buffer, ld)"""
    ld = cols + 8 if cols % 4 == 0 else cols + 1
    return torch.full((rows + 3, ld), float("nan"), dtype=torch.float32, device=dev), ld


@pytest.mark.gpu
@pytest.mark.parametrize("shape", INT_SHAPES)
def test_exact_integers_dgrad(dev, shape):
    """Operand and scale bytes built on the host (mx_integer_case with the contraction along N): every partial sum is exact in fp32, so the
    result equals the fp32 product of the dequantised operands bit for bit - the scale staging and lane maps of lf_contract<true> as the
    data gradient calls it, the N padding and the M / K edges.  Nothing outside [M, K] is touched; the row recipe's counters do not move."""
    M, K, N = shape
    (dq, ds), (wtq, wts) = mx_integer_case(M, N, K)
    ref = (mx_dequant(dq, ds) @ mx_dequant(wtq, wts).T).float()
    out, ldc = _guarded(M, K, dev)
    n0, r0 = _mx_counters(), _row_counters()
    _dgrad_q(dq.to(dev), ds.to(dev), wtq.to(dev), wts.to(dev), out, M, K, N, ldc=ldc)
    torch.cuda.synchronize()
    assert _mx_counters() == (n0[0] + 1, n0[1], n0[2]) and _row_counters() == r0
    got = out.cpu()
    assert torch.equal(got[:M, :K], ref), (float((got[:M, :K] - ref).abs().max()), int((got[:M, :K] != ref).sum()))
    assert bool(torch.isnan(got[M:]).all()) and bool(torch.isnan(got[:, K:]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("splits", [1, 3, 0])
@pytest.mark.parametrize("shape", INT_SHAPES)
def test_exact_integers_wgrad(dev, shape, splits):
    """The same for the weight gradient (contraction along the tokens), added into an integer-prefilled dw with NaN guard rows and columns
    (ldw > K) and a NaN-filled workspace: with one resulting split (M <= 128, or splits = 1) the read-add-write path, with more the
    workspace and the reduce kernel - M = 401 is four k-steps, shared 1 + 1 + 2 among three splits and one each by default; M = 130 and 196
    are two.  Stale workspace contents must not leak: one NaN anywhere would show."""
    M, K, N = shape
    (dyt, dys), (xt, xs) = mx_integer_case(N, M, K, seed=1)
    fill = torch.randint(-3, 4, (N, K), generator=torch.Generator().manual_seed(9)).float()
    ref = (mx_dequant(dyt, dys) @ mx_dequant(xt, xs).T + fill.double()).float()
    dw, ldw = _guarded(N, K, dev)
    dw[:N, :K] = fill.to(dev)
    n0, r0 = _mx_counters(), _row_counters()
    nws = _wgrad_q(dyt.to(dev), dys.to(dev), xt.to(dev), xs.to(dev), dw, M, K, N, ldw=ldw, splits=splits)
    torch.cuda.synchronize()
    nk = (M + 127) // 128
    want = 1 if splits == 1 else min(nk, 3) if splits == 3 else min(nk, -(-512 // (-(-N // 128) * -(-K // 128))))
    assert nws == (want * N * K if want > 1 else 0), (nws, want)
    assert _mx_counters() == (n0[0], n0[1] + 1, n0[2]) and _row_counters() == r0
    got = dw.cpu()
    assert torch.equal(got[:N, :K], ref), (float((got[:N, :K] - ref).abs().max()), int((got[:N, :K] != ref).sum()))
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
        c["refs"][what] = {"dgrad": lambda: emulate_dgrad_mx(c["dy"], c["W"]), "dgrad_gelu": lambda: emulate_dgrad_mx(c["dy"], c["W"], hpre=c["hpre"]),
                           "wgrad": lambda: emulate_wgrad_mx(c["dy"], c["x"])}[what]()
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
    """Kernel against the CPU emulation (torch.float8_e4m3fn casts after an exact exponent add, fp64 contraction and epilogue, erf GELU
    derivative) reading the same stored inputs, plain and with fc2's act_grad_src."""
    M, K, N = shape
    c = _case(shape, store)
    ref = _reference(c, "dgrad" if form == "none" else "dgrad_gelu")
    out = torch.full((M, K), float("nan"), dtype=_dt(store), device=dev)
    epi = {} if form == "none" else dict(act_grad_src=c["hpre"].to(dev), act_grad_kind=hip.ACT_GELU)
    _dgrad(c["dy"].to(dev), c["W"].to(dev), out, M, K, N, **epi)
    torch.cuda.synchronize()
    _check(f"MX dgrad {shape} {store} {form}", out, ref, L1_BF16 if store == "bf16" else L1_F32)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["none", "gelu"])
@pytest.mark.parametrize("store", ["f32", "bf16"])
def test_store_widths_agree(dev, store, form):
    """The data gradient's two piece widths perform the same arithmetic per element: the same quantised operands with ldc = 40 (16-byte
    pieces) and 41 (single elements) give the same bytes of dx [37, 40], and nothing else of the NaN-filled buffers is written.  No tolerance."""
    M, K, N = 37, 40, 99
    dy, _, W = gauss_bwd_case(M, K, N, seed=11)
    hpre = (1.5 * torch.randn(M, K, generator=torch.Generator().manual_seed(80))).to(_dt(store))
    dq, ds = _quant_rows(dy.to(_dt(store)).to(dev), M, N)
    wtq, wts = _quant_cols(W.to(dev), N, K)
    runs = []
    for ld in (40, 41):
        out = torch.full((M + 3, ld), float("nan"), dtype=_dt(store), device=dev)
        epi = {}
        if form == "gelu":
            src = torch.full((M + 3, ld), float("nan"), dtype=_dt(store), device=dev)     # act_grad_src has the layout of the output
            src[:M, :K] = hpre.to(dev)
            epi = dict(act_grad_src=src, act_grad_kind=hip.ACT_GELU)
        _dgrad_q(dq, ds, wtq, wts, out, M, K, N, ldc=ld, **epi)
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
    """dw is fp32 whatever the storage of dy and x: 1e-4, with the default splits"""
    M, K, N = shape
    c = _case(shape, store)
    ref = _reference(c, "wgrad")
    dw = torch.zeros(N, K, dtype=torch.float32, device=dev)
    _wgrad(c["dy"].to(dev), c["x"].to(dev), dw, M, K, N)
    torch.cuda.synchronize()
    _check(f"MX wgrad {shape} {store}", dw, ref, L1_F32)


# ---- 4. separation ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("store", ["f32", "bf16"])
@pytest.mark.parametrize("shape", RECIPE_SHAPES)
def test_other_paths_are_separated_from_the_mx_recipe(dev, shape, store):
    """Without this the bounds above would not tell the paths apart: the row-recipe kernels (sv_linear_fp8_dgrad / sv_linear_fp8_wgrad) and the
    engine's bf16-operand gradients on the same stored inputs are each >= 1.5e-2 (L1-relative) away from the MX emulation.  The row-recipe
    calls move the row counters and not the MX ones."""
    M, K, N = shape
    c = _case(shape, store)
    dy, x, W = c["dy"].to(dev), c["x"].to(dev), c["W"].to(dev)
    n0, r0 = _mx_counters(), ops.linear_fp8_bwd_launches()
    ops.set_math("bf16")
    ops.set_storage(store)
    try:
        dq, sd = ops.quantize_rows_fp8(dy, M, N)
        wtq, swt = ops.quantize_cols_fp8(W, N, K)
        dx_row = ops.empty(M, K, device=dev)
        e = ops._epilogue(K)
        call("sv_linear_fp8_dgrad", ptr(dq), ptr(sd), ptr(wtq), ptr(swt), ptr(dx_row), M, N, K, C.byref(e))
        dyt, sdc = ops.quantize_cols_fp8(dy, M, N)
        xt, sxc = ops.quantize_cols_fp8(x, M, K)
        dw_row = torch.zeros(N, K, dtype=torch.float32, device=dev)
        call("sv_linear_fp8_wgrad", ptr(dyt), ptr(sdc), ptr(xt), ptr(sxc), ptr(dw_row), M, N, K, K, 0)
        spec = ops.ConvSpec.linear(K, N)
        dx = ops.empty(M, K, device=dev)
        dw = torch.zeros(N, K, dtype=torch.float32, device=dev)
        ops.linear_dgrad(dy, M, spec, spec.pack_dgrad(W), dx)
        ops.linear_wgrad(dy, x, M, spec, dw)
        torch.cuda.synchronize()
    finally:
        ops.set_math("f32")
    r1 = ops.linear_fp8_bwd_launches()
    assert _mx_counters() == n0 and r1 == (r0[0] + 1, r0[1] + 1)
    ref_dx, ref_dw = _reference(c, "dgrad"), _reference(c, "wgrad")
    d = dict(row_dx=l1_rel(dx_row.float().cpu(), ref_dx), row_dw=l1_rel(dw_row.cpu(), ref_dw),
             bf16_dx=l1_rel(dx.float().cpu(), ref_dx), bf16_dw=l1_rel(dw.cpu(), ref_dw))
    print(f"{shape} {store}: distance from the MX emulation: " + ", ".join(f"{k} {v:.3e}" for k, v in d.items()))
    assert min(d.values()) >= SEPARATION, d


# ---- 5. determinism ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("splits", [3, 0])
def test_wgrad_is_deterministic(dev, splits):
    """No atomics into dw: two runs from the same dw give the same bits (four k-steps: three splits through the workspace, and the default's
    four).  The two split counts add in different orders and may differ from one another; each is within the recipe's bound."""
    M, K, N = 401, 192, 192
    c = _case((M, K, N), "f32")
    dy, x = c["dy"].to(dev), c["x"].to(dev)
    start = torch.randn(N, K, generator=torch.Generator().manual_seed(5))
    runs = []
    for _ in range(2):
        dw = start.to(dev)
        nws = _wgrad(dy, x, dw, M, K, N, splits=splits)
        torch.cuda.synchronize()
        runs.append(dw.cpu())
    assert nws == (3 if splits == 3 else 4) * N * K
    assert torch.equal(runs[0], runs[1]), int((runs[0] != runs[1]).sum())
    _check(f"MX wgrad splits={splits} into a filled dw", runs[0] - start, _reference(c, "wgrad"), L1_F32)


# ---- 6. refusals and counters -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("what", ["bias", "residual", "stats", "act_grad_kind", "col_off"])
def test_refusals(dev, what):
    M, K, N = 16, 16, 128
    dy, _, W = gauss_bwd_case(M, K, N)
    out = torch.zeros(M, 2 * K, dtype=torch.float32, device=dev)
    dummy = torch.zeros(M * K * 2, dtype=torch.float64, device=dev)
    epi = {"stats": dict(stats=dummy), "bias": dict(bias=dummy), "residual": dict(residual=dummy, ldr=K),
           "act_grad_kind": dict(act_grad_src=dummy, act_grad_kind=hip.ACT_RELU), "col_off": dict(ldc=2 * K, col_off=K)}[what]
    e = ops._epilogue(epi.pop("ldc", K), **epi)
    lib = hip.load()
    assert lib.sv_linear_fp8_dgrad_supported(N, K, C.byref(ops._epilogue(K)), hip.MATH_BF16, hip.F32) == 1
    assert lib.sv_linear_fp8_dgrad_supported(N, K, C.byref(e), hip.MATH_BF16, hip.F32) == 0
    dq, ds = _quant_rows(dy.to(dev), M, N)
    wtq, wts = _quant_cols(W.to(dev), N, K)
    n0, r0 = _mx_counters(), _row_counters()
    with pytest.raises(RuntimeError, match="sv_linear_mxfp8_dgrad"):
        call("sv_linear_mxfp8_dgrad", ptr(dq), ptr(ds), ptr(wtq), ptr(wts), ptr(out), M, N, K, C.byref(e), act=hip.F32)
    torch.cuda.synchronize()
    assert _mx_counters() == n0 and _row_counters() == r0
    assert float(out.abs().max()) == 0.0
