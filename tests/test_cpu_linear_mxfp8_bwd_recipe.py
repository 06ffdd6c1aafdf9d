"""The MX BACKWARD recipe of the fp8 Swin linears (swinvox_amd/csrc/linear_fp8.hip, "MX backward") as a torch emulation on the helpers of
test_cpu_linear_mxfp8_recipe.py, the checks that pin it, and the C ABI of its entry points without a GPU.

The emulation is the yardstick tests/test_gpu_linear_mxfp8_bwd.py measures the kernels with, so it is tested here on its own: exact integers
with non-unit block scales along either contraction, the padding along the tokens, and the distance from the exact products and from the
row-recipe backward on N(0, 1) data.  The ABI part follows test_cpu_linear_mxfp8_recipe.py: the header declares and cites the entries, the
ctypes tables bind them, and the refusals - host-side checks that run before any GPU call - answer SV_ERR_INVALID and move no counter."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_linear_fp8_recipe import l1_rel  # noqa: E402
from test_cpu_linear_fp8_bwd_recipe import BWD_SHAPES, emulate_dgrad, emulate_wgrad, gauss_bwd_case, gelu_grad  # noqa: E402
from test_cpu_linear_mxfp8_recipe import SEPARATION, mx_block_exp, mx_dequant, mx_integer_case, mx_quant_rows  # noqa: E402

import swinvox_amd as S  # noqa: E402
from swinvox_amd import hip, ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# measured with gauss_bwd_case (seed 0) on BWD_SHAPES: both gradients 3.69e-2 ... 3.80e-2 from the exact product
EXACT_BAND = (3.4e-2, 3.9e-2)


# ---- the emulation --------------------------------------------------------------------------------------------------------------------
def mx_quant_cols(t):
    """THE DEFINITION of the MX column quantiser: the MX row quantiser on the transposed stored tensor.  t [M, C] -> (bytes [C, Mp], scale
    bytes [C, Mp / 32]), Mp = roundup(M, 128); a block = 32 consecutive rows m of one column."""
    return mx_quant_rows(t.T.contiguous())


def emulate_dgrad_mx(dy, W, hpre=None, acc_dtype=torch.float64):
    """dx [M, K] = dy [M, N] W [N, K]: dy in MX rows (blocks along n), W^T in MX rows (blocks of 32 consecutive n of one column k); val = the
    sum of the block-scaled products, no division; optional val *= gelu'(hpre).  Before the store rounding."""
    val = mx_dequant(*mx_quant_rows(dy), dtype=acc_dtype) @ mx_dequant(*mx_quant_cols(W.float()), dtype=acc_dtype).T
    if hpre is not None:
        val = val * gelu_grad(hpre.to(acc_dtype))
    return val


def emulate_wgrad_mx(dy, x, acc_dtype=torch.float64):
    """dw [N, K] = dy^T [N, M] x [M, K]: dy^T and x^T in MX rows along the tokens (blocks of 32 consecutive tokens of one column)"""
    return mx_dequant(*mx_quant_cols(dy), dtype=acc_dtype) @ mx_dequant(*mx_quant_cols(x), dtype=acc_dtype).T


# ---- exact integers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(49, 96, 288), (401, 192, 192), (196, 384, 1536), (130, 1536, 384), (37, 99, 30), (1536, 64, 40)])
def test_integer_case_is_exact_along_either_contraction(shape):
    """mx_integer_case with the contraction along N (data gradient: dy [M, Np] against W^T [K, Np]) and along the tokens (weight gradient:
    dy^T [N, Mp] against x^T [K, Mp], tokens <= 1536) is exact in fp32, the second added into an integer-prefilled dw."""
    M, K, N = shape
    assert M <= 1536 and N <= 1536
    (dq, ds), (wtq, wts) = mx_integer_case(M, N, K)                     # contraction length N
    ref64 = mx_dequant(dq, ds) @ mx_dequant(wtq, wts).T
    ref32 = mx_dequant(dq, ds, torch.float32) @ mx_dequant(wtq, wts, torch.float32).T
    assert ref64.shape == (M, K) and torch.equal(ref32.double(), ref64) and float(ref64.abs().max()) < 2.0 ** 17
    (dyt, dys), (xt, xs) = mx_integer_case(N, M, K, seed=1)             # contraction length M
    fill = torch.randint(-3, 4, (N, K), generator=torch.Generator().manual_seed(9)).float()
    ref64 = mx_dequant(dyt, dys) @ mx_dequant(xt, xs).T + fill.double()
    ref32 = mx_dequant(dyt, dys, torch.float32) @ mx_dequant(xt, xs, torch.float32).T + fill
    assert ref64.shape == (N, K) and torch.equal(ref32.double(), ref64)
    unit = mx_dequant(dyt, torch.full_like(dys, 127)) @ mx_dequant(xt, torch.full_like(xs, 127)).T + fill.double()
    assert not torch.equal(unit, ref64)                                   # the scales matter


# ---- padding along the tokens -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [37, 401])
def test_token_padding(M):
    """zero bytes past M, byte 127 in the blocks that lie wholly past M, and a partly filled block scaled by its valid rows only"""
    Cc = 20
    g = torch.Generator().manual_seed(M)
    t = torch.randn(M, Cc, generator=g) * torch.exp2(torch.randint(-6, 7, (M, 1), generator=g).float())
    q, s = mx_quant_cols(t)
    Mp = (M + 127) // 128 * 128
    assert q.shape == (Cc, Mp) and s.shape == (Cc, Mp // 32)
    assert int(q[:, M:].max()) == 0
    assert bool((s[:, (M + 31) // 32:] == 127).all())
    b = M // 32                                                           # M % 32 != 0 at both sizes: block b is partly filled
    assert M % 32 and torch.equal(s[:, b].to(torch.int32) - 127, mx_block_exp(t[32 * b:].abs().amax(dim=0)))
    # the padding changes nothing in the product
    x = torch.randn(M, 24, generator=g)
    full = emulate_wgrad_mx(t, x)
    vals_t, vals_x = mx_dequant(*mx_quant_cols(t))[:, :M], mx_dequant(*mx_quant_cols(x))[:, :M]
    assert l1_rel(full, vals_t @ vals_x.T) < 1e-14


# ---- distances --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BWD_SHAPES)
def test_distances(shape):
    """MX is a structural feature, not an accuracy feature: both gradients are as far from the exact product as the row recipe's (e4m3's
    three mantissa bits), and far enough from the row recipe's for the bounds of the GPU tests to tell the two kernels apart."""
    M, K, N = shape
    dy, x, W = gauss_bwd_case(M, K, N)
    dx, dw = emulate_dgrad_mx(dy, W), emulate_wgrad_mx(dy, x)
    ex_dx, ex_dw = dy.double() @ W.double(), dy.double().T @ x.double()
    row_dx, row_dw = emulate_dgrad(dy, W), emulate_wgrad(dy, x)
    d = dict(dx_exact=l1_rel(dx, ex_dx), dw_exact=l1_rel(dw, ex_dw), dx_row=l1_rel(dx, row_dx), dw_row=l1_rel(dw, row_dw))
    print(f"{shape}: MX vs exact dgrad {d['dx_exact']:.3e} wgrad {d['dw_exact']:.3e}; row recipe vs exact dgrad {l1_rel(row_dx, ex_dx):.3e} "
          f"wgrad {l1_rel(row_dw, ex_dw):.3e}; MX vs row recipe dgrad {d['dx_row']:.3e} wgrad {d['dw_row']:.3e}")
    assert EXACT_BAND[0] <= d["dx_exact"] <= EXACT_BAND[1], d
    assert EXACT_BAND[0] <= d["dw_exact"] <= EXACT_BAND[1], d
    assert d["dx_row"] >= SEPARATION and d["dw_row"] >= SEPARATION, d
    assert l1_rel(emulate_dgrad_mx(dy, W, acc_dtype=torch.float32), dx) < 1e-6
    assert l1_rel(emulate_wgrad_mx(dy, x, acc_dtype=torch.float32), dw) < 1e-6


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("sv_quant_cols_mx_e4m3", "sv_linear_mxfp8_dgrad", "sv_linear_mxfp8_wgrad_workspace_floats", "sv_linear_mxfp8_wgrad",
           "sv_linear_mxfp8_bwd_launches", "sv_quant_cols_mx_launches")
SV_ERR_INVALID = -1


def test_header_declares_and_cites():
    hdr = open(os.path.join(ROOT, "include", "swinvox_hip.h")).read()
    for name in ENTRIES:
        m = re.search(r"(/\*(?:(?!\*/).)*\*/\s*)?\b(?:int|long long|size_t)\s+" + name + r"\s*\([^;]*\)\s*;[ \t]*(/\*(?:(?!\*/).)*\*/)?", hdr, flags=re.S)
        assert m, f"{name} is not declared"
        comment = (m.group(1) or "") + (m.group(2) or "")
        assert "models/swin_transformer.py:78" in comment, (name, comment)


def test_exported_and_bound():
    for name in ENTRIES:
        assert name in hip.EXPORTED_SYMBOLS
    assert "sv_linear_mxfp8_dgrad" in hip._ACT_TYPED
    assert "sv_quant_cols_mx_e4m3" not in hip._ACT_TYPED and "sv_linear_mxfp8_wgrad" not in hip._ACT_TYPED
    lib = hip.load()                          # dlopen only: no GPU call is made
    assert lib.sv_linear_mxfp8_bwd_launches(0) >= 0 and lib.sv_linear_mxfp8_bwd_launches(1) >= 0 and lib.sv_quant_cols_mx_launches() >= 0
    assert lib.sv_linear_mxfp8_bwd_launches(2) == -1
    assert len(hip._argtypes("sv_quant_cols_mx_e4m3")) == 10 and len(hip._argtypes("sv_linear_mxfp8_dgrad")) == 11
    assert len(hip._argtypes("sv_linear_mxfp8_wgrad")) == 12 and len(hip._argtypes("sv_linear_mxfp8_wgrad_workspace_floats")) == 4


def test_workspace_floats():
    """resulting splits x N x K floats, 0 when one split results: at most one split per 128 tokens, 0 = two workgroups for each of 256 CUs"""
    ws = hip.load().sv_linear_mxfp8_wgrad_workspace_floats
    assert ws(401, 192, 192, 1) == 0 and ws(100, 192, 192, 0) == 0 and ws(100, 192, 192, 7) == 0      # one k-step: one split
    assert ws(401, 192, 192, 3) == 3 * 192 * 192
    assert ws(401, 192, 192, 0) == 4 * 192 * 192 and ws(401, 192, 192, 9) == 4 * 192 * 192              # capped at the 4 k-steps
    assert ws(128 * 1000, 384, 384, 0) == 57 * 384 * 384                                              # 9 tiles: ceil(512 / 9) = 57
    assert ws(401, 192, 192, -1) == 0 and ws(0, 192, 192, 0) == 0


# fake, suitably aligned device addresses: every call below is refused before anything could read them
A0, A1, A2, A3, A4, A5, A6 = (0x10000 * (i + 1) for i in range(7))


def _counters(lib):
    return (lib.sv_linear_mxfp8_bwd_launches(0), lib.sv_linear_mxfp8_bwd_launches(1), lib.sv_quant_cols_mx_launches(),
            lib.sv_linear_fp8_bwd_launches(0), lib.sv_linear_fp8_bwd_launches(1), lib.sv_quant_rows_mx_launches())


@pytest.mark.parametrize("what,over", [
    ("src null", dict(src=None)),
    ("dst_q null", dict(q=None)),
    ("scales null", dict(s=None)),
    ("bad dtype", dict(dt=7)),
    ("Mp not roundup(M, 128)", dict(Mp=256)),
    ("Mp below M", dict(M=200, Mp=128)),
    ("Mp not a multiple of 128", dict(Mp=64)),
    ("dst_q misaligned", dict(q=A1 + 8)),
    ("scales misaligned", dict(s=A2 + 2)),
    ("M = 0", dict(M=0)),
    ("ld < C", dict(ld=64)),
])
def test_quantiser_refusals_before_any_gpu_call(what, over):
    lib = hip.load()
    a = dict(src=A0, dt=hip.F32, M=40, C=96, ld=96, q=A1, Mp=128, s=A2, colsum=None)
    a.update(over)
    n0 = _counters(lib)
    rc = lib.sv_quant_cols_mx_e4m3(a["src"], a["dt"], a["M"], a["C"], a["ld"], a["q"], a["Mp"], a["s"], a["colsum"], None)
    assert rc == SV_ERR_INVALID, (what, rc)
    assert "sv_quant_cols_mx_e4m3" in lib.sv_last_error().decode(), (what, lib.sv_last_error())
    assert _counters(lib) == n0, what


def _epi(K=128, **kw):
    f = dict(bias=None, residual=None, ldr=0, row_scale=None, rows_per_scale=1, pre_act=None, stats=None, act=hip.ACT_NONE, slope=0.0,
             act_grad_src=None, act_grad_kind=hip.ACT_NONE, ldc=K, col_off=0)
    f.update(kw)
    return hip.Epilogue(f["bias"], f["residual"], f["ldr"], f["row_scale"], f["rows_per_scale"], f["pre_act"], f["stats"], f["act"], f["slope"],
                        f["act_grad_src"], f["act_grad_kind"], f["ldc"], f["col_off"])


@pytest.mark.parametrize("what,over,epi", [
    ("dq null", dict(dq=None), {}),
    ("ds null", dict(ds=None), {}),
    ("wtq null", dict(wtq=None), {}),
    ("wts null", dict(wts=None), {}),
    ("dx null", dict(dx=None), {}),
    ("dq misaligned", dict(dq=A0 + 8), {}),
    ("wts misaligned", dict(wts=A3 + 1), {}),
    ("bias", {}, dict(bias=A5)),
    ("residual", {}, dict(residual=A5, ldr=128)),
    ("stats", {}, dict(stats=A5)),
    ("pre_act", {}, dict(pre_act=A5)),
    ("an activation", {}, dict(act=hip.ACT_GELU)),
    ("a non-GELU act_grad_kind", {}, dict(act_grad_src=A5, act_grad_kind=hip.ACT_RELU)),
    ("col_off", {}, dict(ldc=256, col_off=128)),
    ("ldc < K", {}, dict(ldc=64)),
    ("bad activation dtype", dict(act=7), {}),
    ("M = 0", dict(M=0), {}),
])
def test_dgrad_refusals_before_any_gpu_call(what, over, epi):
    lib = hip.load()
    a = dict(dq=A0, ds=A1, wtq=A2, wts=A3, dx=A4, M=16, N=128, K=128, act=hip.BF16)
    a.update(over)
    e = _epi(a["K"], **epi)
    n0 = _counters(lib)
    rc = lib.sv_linear_mxfp8_dgrad(a["dq"], a["ds"], a["wtq"], a["wts"], a["dx"], a["M"], a["N"], a["K"], C.byref(e), a["act"], None)
    assert rc == SV_ERR_INVALID, (what, rc)
    assert "sv_linear_mxfp8_dgrad" in lib.sv_last_error().decode() or what == "bad activation dtype", (what, lib.sv_last_error())
    assert _counters(lib) == n0, what


def test_dgrad_supported_answers_for_both_kernels():
    lib = hip.load()
    assert lib.sv_linear_fp8_dgrad_supported(128, 128, C.byref(_epi()), hip.MATH_BF16, hip.BF16) == 1
    assert lib.sv_linear_fp8_dgrad_supported(128, 128, C.byref(_epi(act_grad_src=A5, act_grad_kind=hip.ACT_GELU)), hip.MATH_BF16, hip.F32) == 1
    assert lib.sv_linear_fp8_dgrad_supported(128, 128, C.byref(_epi(bias=A5)), hip.MATH_BF16, hip.BF16) == 0
    assert lib.sv_linear_fp8_dgrad_supported(128, 128, C.byref(_epi()), hip.MATH_F32, hip.F32) == 0


@pytest.mark.parametrize("what,over", [
    ("dyt null", dict(dyt=None)),
    ("dys null", dict(dys=None)),
    ("xt null", dict(xt=None)),
    ("xs null", dict(xs=None)),
    ("dw null", dict(dw=None)),
    ("ldw < K", dict(ldw=100)),
    ("splits < 0", dict(splits=-1)),
    ("workspace misaligned", dict(ws=A5 + 8)),
    ("dyt misaligned", dict(dyt=A0 + 8)),
    ("three splits without a workspace", dict(splits=3, ws=None)),
    ("default splits (4 result) without a workspace", dict(splits=0, ws=None)),
    ("M = 0", dict(M=0)),
])
def test_wgrad_refusals_before_any_gpu_call(what, over):
    lib = hip.load()
    a = dict(dyt=A0, dys=A1, xt=A2, xs=A3, dw=A4, M=401, N=192, K=192, ldw=192, splits=3, ws=A5)
    a.update(over)
    n0 = _counters(lib)
    rc = lib.sv_linear_mxfp8_wgrad(a["dyt"], a["dys"], a["xt"], a["xs"], a["dw"], a["M"], a["N"], a["K"], a["ldw"], a["splits"], a["ws"], None)
    assert rc == SV_ERR_INVALID, (what, rc)
    assert "sv_linear_mxfp8_wgrad" in lib.sv_last_error().decode(), (what, lib.sv_last_error())
    assert _counters(lib) == n0, what


# ---- the host switch --------------------------------------------------------------------------------------------------------------------
def test_backward_recipe_switch():
    try:
        ops.set_math("bf16")
        assert ops.linear_fp8_bwd_recipe() == "row"                              # the default
        S.set_linear_fp8(True, backward=True)
        assert ops.linear_fp8_bwd_enabled() and ops.linear_fp8_bwd_recipe() == "row"
        S.set_linear_fp8(True, backward=True, recipe="mx")                       # the forward recipe does not choose the backward's
        assert ops.linear_fp8_recipe() == "mx" and ops.linear_fp8_bwd_recipe() == "row"
        for fwd in ("row", "mx"):                                                # combines with either forward recipe
            S.set_linear_fp8(True, backward=True, recipe=fwd, backward_recipe="mx")
            assert ops.linear_fp8_recipe() == fwd and ops.linear_fp8_bwd_enabled() and ops.linear_fp8_bwd_recipe() == "mx"
        S.set_linear_fp8(True, backward_recipe="mx")                             # effective only with `backward` ...
        assert ops.linear_fp8_enabled() and not ops.linear_fp8_bwd_enabled() and ops.linear_fp8_bwd_recipe() == "row"
        S.set_linear_fp8(False, backward=True, backward_recipe="mx")             # ... and with `on`
        assert not ops.linear_fp8_bwd_enabled() and ops.linear_fp8_bwd_recipe() == "row"
        S.set_linear_fp8(True, backward=True, backward_recipe="mx")
        S.set_linear_fp8(True, backward=True)                                    # the keyword defaults back to the row recipe
        assert ops.linear_fp8_bwd_recipe() == "row"
        with pytest.raises(ValueError, match="backward_recipe"):
            S.set_linear_fp8(True, backward=True, backward_recipe="mxfp4")
        assert ops.linear_fp8_bwd_recipe() == "row"                              # a refused call changes nothing
        S.set_linear_fp8(True, backward=True, backward_recipe="mx")
        ops.set_math("f32")                                                      # inert under f32 math
        assert not ops.linear_fp8_enabled() and not ops.linear_fp8_bwd_enabled()
    finally:
        S.set_linear_fp8(False)
        ops.set_math("f32")
    assert ops.linear_fp8_bwd_recipe() == "row" and not ops.linear_fp8_bwd_enabled()


def test_pack_cache_holds_and_clears_the_transposed_mx_weight():
    cache = ops.PackCache()
    assert cache.w8mxt == {}
    cache.w8mxt[1] = cache.w8t[1] = cache.w8mx[1] = cache.w8[1] = ("q", "s")
    cache.refresh()                                                             # no registered packs: only the quantised-weight tables are dropped
    assert cache.w8mxt == {} and cache.w8t == {} and cache.w8mx == {} and cache.w8 == {}
