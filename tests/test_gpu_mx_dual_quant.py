"""MX dual quantiser (csrc/linear_fp8.hip, sv_quant_rows_cols_mx_e4m3; ops.set_mx_dual_quant) on the GPU: one read of a tensor gives the MX row
operand and the MX column operand, each equal bit for bit to the CPU definition (mx_quant_rows / mx_quant_cols) and to the stand-alone kernels;
both operands through the MX GEMMs on exact integers; one unfused Swin block with the switch off and on; the one-slot stash between
swin_linear_wgrad and swin_linear_dgrad."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_linear_mxfp8_recipe import mx_dequant, mx_integer_case, mx_quant_rows  # noqa: E402
from test_cpu_linear_mxfp8_bwd_recipe import mx_quant_cols  # noqa: E402
from test_gpu_linear_mxfp8_bwd import COLSUM_BOUND, _dgrad_q, _guarded, _quant_cols, _wgrad_q  # noqa: E402  (the bound is imported, not restated)

import swinvox_amd as S  # noqa: E402
from swinvox_amd import hip, ops  # noqa: E402
from swinvox_amd.ops import call, ptr  # noqa: E402

GUARD = 2              # poisoned guard rows behind each of the four outputs


def _code(t):
    return hip.BF16 if t.dtype == torch.bfloat16 else hip.F32


def _counters():
    """(dual quantiser, MX row quantiser, MX column quantiser, re-blocker) launches so far"""
    lib = hip.load()
    return (int(lib.sv_quant_rows_cols_mx_launches()), int(lib.sv_quant_rows_mx_launches()), int(lib.sv_quant_cols_mx_launches()),
            int(lib.sv_mx_rows_to_cols_launches()))


def _delta(a, b):
    return tuple(y - x for x, y in zip(a, b))


def _dual(t, M, N, ld=None, colsum=None, rows_out=True):
    """sv_quant_rows_cols_mx_e4m3 into poisoned buffers with GUARD rows behind each -> (row bytes [M + GUARD, Np], row scales [M + GUARD, Np / 32],
    column bytes [N + GUARD, Mp], column scales [N + GUARD, Mp / 32]); with rows_out=False the row pair is passed as NULL and stays poisoned"""
    Np, Mp = (N + 127) // 128 * 128, (M + 127) // 128 * 128
    rq = torch.full((M + GUARD, Np), 0x7F, dtype=torch.uint8, device=t.device)           # e4m3 NaN
    rs = torch.full((M + GUARD, Np // 32), 0xFF, dtype=torch.uint8, device=t.device)     # E8M0 NaN: a byte the recipe never produces
    cq = torch.full((N + GUARD, Mp), 0x7F, dtype=torch.uint8, device=t.device)
    cs = torch.full((N + GUARD, Mp // 32), 0xFF, dtype=torch.uint8, device=t.device)
    call("sv_quant_rows_cols_mx_e4m3", ptr(t), _code(t), M, N, ld or N, ptr(rq) if rows_out else None, Np, ptr(rs) if rows_out else None,
         ptr(cq), Mp, ptr(cs), ptr(colsum))
    return rq, rs, cq, cs


def _check_dual(name, xs_, dev, ld=None, prefill=None, rows_out=True):
    """One call on the stored tensor xs_ [M, N] (CPU) placed in a NaN-filled buffer of row stride ld: all four outputs against the CPU
    definition and against the two stand-alone kernels on the same device tensor, the guard rows, and colsum from a non-zero prefill.
    Returns the number of comparison calls of the old row / column quantiser."""
    M, N = xs_.shape
    ld = ld or N
    buf = torch.full((M, ld), float("nan"), dtype=xs_.dtype, device=dev)
    buf[:, :N] = xs_.to(dev)
    ref_rq, ref_rs = mx_quant_rows(xs_)
    ref_cq, ref_cs = mx_quant_cols(xs_)
    start = prefill if prefill is not None else torch.zeros(N)
    ref_sum = start.double() + xs_.double().sum(dim=0)            # colsum accumulates: the prefill is part of the reference
    colsum = start.clone().float().to(dev)
    rq, rs, cq, cs = _dual(buf, M, N, ld, colsum, rows_out)
    torch.cuda.synchronize()
    old_rows = old_cols = 0
    if rows_out:
        assert torch.equal(rs[:M].cpu(), ref_rs), (name, int((rs[:M].cpu() != ref_rs).sum()))
        assert torch.equal(rq[:M].cpu(), ref_rq), (name, int((rq[:M].cpu() != ref_rq).sum()))
        Np = rq.shape[1]
        krq, krs = torch.empty(M, Np, dtype=torch.uint8, device=dev), torch.empty(M, Np // 32, dtype=torch.uint8, device=dev)
        call("sv_quant_rows_mx_e4m3", ptr(buf), _code(buf), M, N, ld, ptr(krq), Np, ptr(krs))
        old_rows = 1
        torch.cuda.synchronize()
        assert torch.equal(rq[:M], krq[:M]) and torch.equal(rs[:M], krs[:M]), name
        assert bool((rq[M:] == 0x7F).all()) and bool((rs[M:] == 0xFF).all()), name
    else:
        assert bool((rq == 0x7F).all()) and bool((rs == 0xFF).all()), name      # no row buffer was given: nothing of that shape is written anywhere
    assert torch.equal(cs[:N].cpu(), ref_cs), (name, int((cs[:N].cpu() != ref_cs).sum()))
    assert torch.equal(cq[:N].cpu(), ref_cq), (name, int((cq[:N].cpu() != ref_cq).sum()))
    ksum = torch.zeros(N, dtype=torch.float32, device=dev)
    kcq, kcs = _quant_cols(buf, M, N, ld, ksum)
    old_cols = 1
    torch.cuda.synchronize()
    assert torch.equal(cq[:N], kcq[:N]) and torch.equal(cs[:N], kcs[:N]), name
    assert bool((cq[N:] == 0x7F).all()) and bool((cs[N:] == 0xFF).all()), name
    err = (colsum.cpu().double() - ref_sum).abs()
    print(f"{name}: column sums, worst element {float(err.max() / ref_sum.abs().max()):.2e} of max|ref|")
    assert float(err.max()) <= COLSUM_BOUND * float(ref_sum.abs().max()), name
    return old_rows, old_cols


def _spread_case(M, N):
    """values spanning 16 binades per row and per column; column 2 all zero, the first 32 rows of column 5 zero"""
    g = torch.Generator().manual_seed(M * 1000 + N)
    x = torch.randn(M, N, generator=g)
    x *= torch.exp2(torch.randint(-4, 5, (M, 1), generator=g).float()) * torch.exp2(torch.randint(-4, 5, (1, N), generator=g).float())
    x[:, 2] = 0.0
    x[:32, 5] = 0.0
    return x


# ---- 1. bit equality --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N", [30, 96, 288])
@pytest.mark.parametrize("M", [37, 128, 401])
def test_dual_quantiser_equals_both_quantisers(dev, M, N):
    """M = 37 and 401 end in a partly filled token block followed by padding blocks, N = 30 and 96 in a partly filled row block / column tile
    (N = 288 is three column tiles, the last partial), for fp32 and bf16 input and the row strides N, N + 3 (rows that are not 16-byte
    aligned) and N + 8.  All four outputs equal the CPU definitions and the outputs of the two existing kernels on the same device tensor; the
    guard rows keep their fill; colsum, started from a non-zero prefill, is within 1e-6 of max|ref| of the fp64 sums; the dual counter moves by
    the number of calls and the two old counters only by the comparison calls."""
    x = _spread_case(M, N)
    prefill = torch.linspace(-1.0, 1.0, N)
    n0 = _counters()
    calls = old_r = old_c = 0
    for dt in (torch.float32, torch.bfloat16):
        xs_ = x.to(dt)
        ref_s = mx_quant_cols(xs_)[1]
        assert int(ref_s[2].min()) == 127 and int(ref_s[2].max()) == 127 and int(ref_s[5, 0]) == 127
        for ld in (N, N + 3, N + 8):
            r, c = _check_dual(f"M={M} N={N} {dt} ld={ld}", xs_, dev, ld, prefill)
            calls, old_r, old_c = calls + 1, old_r + r, old_c + c
    assert _delta(n0, _counters()) == (calls, old_r, old_c, 0)


# ---- 2. extremes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_extremes(dev):
    """fp32 input: rows scaled by 1e-20 and 1e20 (scale bytes far from 127 in both directions, column blocks that span 40 decades), a block of
    fp32 denormals, and the smallest shape, M = 1 x N = 1.  The equalities of test 1 hold."""
    M, N = 70, 96
    g = torch.Generator().manual_seed(11)
    x = torch.randn(M, N, generator=g)
    x[3] *= 1e-20
    x[4] *= 1e20
    x[5:8] *= 1e-20
    x[65] *= 1e20
    x[32:64, 32:64] = torch.randn(32, 32, generator=g) * 2.0 ** -140         # fp32 denormals: a whole column block and a whole row block
    assert bool(((x != 0) & (x.abs() < 2.0 ** -126)).any())
    _check_dual("extremes", x, dev)
    _check_dual("extremes ld + 3", x, dev, N + 3)
    _check_dual("1 x 1", torch.tensor([[3.0]]), dev, prefill=torch.tensor([0.5]))
    _check_dual("1 x 1 bf16", torch.tensor([[-0.75]]).bfloat16(), dev)


# ---- 3. column-only form ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(37, 30), (401, 288), (128, 96)])
def test_column_only_form(dev, shape):
    """row_q = row_s = NULL: the column outputs and colsum are those of test 1 (the CPU definition, the existing kernel), for both source
    types and an unaligned row stride"""
    M, N = shape
    x = _spread_case(M, N)
    n0 = _counters()
    calls = 0
    for dt in (torch.float32, torch.bfloat16):
        for ld in (N, N + 3):
            _check_dual(f"column-only M={M} N={N} {dt} ld={ld}", x.to(dt), dev, ld, torch.linspace(-1.0, 1.0, N), rows_out=False)
            calls += 1
    assert _delta(n0, _counters()) == (calls, 0, calls, 0)


# ---- 4. through the GEMMs ---------------------------------------------------------------------------------------------------------------
INT_SHAPES = [(49, 96, 288), (401, 192, 192), (37, 99, 30)]      # (M, K, N)


@pytest.mark.gpu
@pytest.mark.parametrize("store", ["f32", "bf16"])
@pytest.mark.parametrize("shape", INT_SHAPES)
def test_exact_integers_dual_rows_then_dgrad(dev, shape, store):
    """dy = the values of an mx_integer_case operand (integers |v| <= 2 times 2^-1 .. 2^2 per block: one significant bit and four binades, so
    they are exact in bf16 and the MX rows of ANY blocking lose nothing).  sv_linear_mxfp8_dgrad on the dual quantiser's row pair and the
    case's W^T operand equals the fp32 product of the values bit for bit."""
    M, K, N = shape
    (dq, ds), (wtq, wts) = mx_integer_case(M, N, K)
    dy = mx_dequant(dq, ds, torch.float32)[:, :N].contiguous().to(torch.bfloat16 if store == "bf16" else torch.float32)
    ref = (mx_dequant(dq, ds) @ mx_dequant(wtq, wts).T).float()
    out, ldc = _guarded(M, K, dev)
    rq, rs, _, _ = _dual(dy.to(dev), M, N)
    _dgrad_q(rq, rs, wtq.to(dev), wts.to(dev), out, M, K, N, ldc=ldc)
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(got[:M, :K], ref), (float((got[:M, :K] - ref).abs().max()), int((got[:M, :K] != ref).sum()))
    assert bool(torch.isnan(got[M:]).all()) and bool(torch.isnan(got[:, K:]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("splits", [1, 3, 0])
@pytest.mark.parametrize("shape", INT_SHAPES)
def test_exact_integers_dual_cols_then_wgrad(dev, shape, splits):
    """The same along the tokens: dy [M, N] and x [M, K] are the transposed values of the case's two operands; the dual quantiser's column pair
    of dy and the column-only form on x go through sv_linear_mxfp8_wgrad into an integer-prefilled dw with NaN guards and a NaN-filled
    workspace: bit-identical to the fp32 product, for one split, three and the default."""
    M, K, N = shape
    (dyt, dys), (xt, xs) = mx_integer_case(N, M, K, seed=1)
    dy = mx_dequant(dyt, dys, torch.float32)[:, :M].T.contiguous()
    x = mx_dequant(xt, xs, torch.float32)[:, :M].T.contiguous().bfloat16()
    fill = torch.randint(-3, 4, (N, K), generator=torch.Generator().manual_seed(9)).float()
    ref = (mx_dequant(dyt, dys) @ mx_dequant(xt, xs).T + fill.double()).float()
    dw, ldw = _guarded(N, K, dev)
    dw[:N, :K] = fill.to(dev)
    _, _, cq, cs = _dual(dy.to(dev), M, N)
    _, _, xq, xsc = _dual(x.to(dev), M, K, rows_out=False)
    _wgrad_q(cq, cs, xq, xsc, dw, M, K, N, ldw=ldw, splits=splits)
    torch.cuda.synchronize()
    got = dw.cpu()
    assert torch.equal(got[:N, :K], ref), (float((got[:N, :K] - ref).abs().max()), int((got[:N, :K] != ref).sum()))
    assert bool(torch.isnan(got[N:]).all()) and bool(torch.isnan(got[:, K:]).all())


# ---- 5. host path: one Swin block ---------------------------------------------------------------------------------------------------------
CD, HEADS, RES, IMGS = 192, 6, 14, 2
_BLOCK = {}


def _block_setup(dev):
    """the block, its inputs and a weight-operand cache warmed by one switch-off step: the quantised weights (rows for the forward, W^T for the
    data gradient) are cached for as long as the weights do not change, so the counters of the measured runs see activations and gradients only"""
    if "setup" in _BLOCK:
        return _BLOCK["setup"]
    from swinvox_amd.models.swin_transformer import SwinBlock
    torch.manual_seed(5)
    blk = SwinBlock(CD, RES, HEADS, 3, 0.0)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for n, p in blk.named_parameters():
            if p.dim() == 1:
                p.copy_((1.0 if "norm" in n and n.endswith("weight") else 0.0) + 0.1 * torch.randn(p.shape, generator=g))
            elif "bias_table" not in n:
                p.copy_(torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5)
    blk.to(dev)
    M = IMGS * RES * RES
    x = torch.randn(M, CD, generator=g).bfloat16().to(dev)
    dy = torch.randn(M, CD, generator=g).bfloat16().to(dev)
    _BLOCK["setup"] = (blk, x, dy, ops.PackCache())
    _block_run(dev, "bf16", False, True, keep=False)
    return _BLOCK["setup"]


def _block_run(dev, store, dual, overlap, keep=True):
    """forward + backward of one unfused SwinBlock under the MX forward and backward -> dx, the gradients, the dy every swin_linear_wgrad got,
    the counters' increase over the backward and the stash after it.  overlap: with an AsyncWgrad (the weight-gradient stream), as a module
    backward runs it; without, everything stays on one stream."""
    key = (store, dual, overlap)
    if keep and key in _BLOCK:
        return _BLOCK[key]
    from swinvox_amd.models.swin_transformer import block_backward, block_forward
    blk, x, dy, packs = _block_setup(dev)
    grads = {p: torch.zeros_like(p, dtype=torch.float32) for p in blk.parameters()}
    seen = []
    real_wgrad = ops.swin_linear_wgrad

    def spy_wgrad(dy_, x_, rows, spec, w, dw, db=None, async_ok=True):
        seen.append((w, dy_.detach().cpu().clone()))
        return real_wgrad(dy_, x_, rows, spec, w, dw, db, async_ok=async_ok)

    aw = None
    try:
        ops.set_math("bf16")
        ops.set_storage("bf16")
        S.set_linear_fp8(True, backward=True, recipe="mx", backward_recipe="mx", store=store)
        ops.set_mx_dual_quant(dual)
        assert ops.mx_dual_quant_enabled() == dual
        ops.set_pack_cache(packs)
        ops.swin_linear_wgrad = spy_wgrad
        _, ctx = block_forward(blk, x, IMGS, True, False, None, True)
        torch.cuda.synchronize()
        n0 = _counters()
        if overlap:
            aw = ops.AsyncWgrad(dev)
        ops.set_async_wgrad(aw)
        dx = block_backward(blk, ctx, dy.clone(), grads)
        stash = ops._CTX.dyq
        ops.set_async_wgrad(None)
        if aw is not None:
            aw.join()
        torch.cuda.synchronize()
        n1 = _counters()
    finally:
        ops.swin_linear_wgrad = real_wgrad
        ops.set_async_wgrad(None)
        ops.set_pack_cache(None)
        ops.set_mx_dual_quant(False)
        S.set_linear_fp8(False)
        ops.set_math("f32")
    names = {p: n for n, p in blk.named_parameters()}
    out = dict(dx=dx.cpu(), grads={names[p]: v.cpu() for p, v in grads.items()}, dys={names[w]: d for w, d in seen}, bwd=_delta(n0, n1), stash=stash)
    if keep:
        _BLOCK[key] = out
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("store", ["bf16", "mx"])
def test_block_switch_off_and_on(dev, store, overlap):
    """One SwinBlock (C = 192, 6 heads, 14 x 14, 2 images: M = 392), from the same inputs and dy, switch off then on.  dx and the four weight
    gradients are bit-identical (the MX weight gradient is deterministic for its default splits); the bias gradients of both runs are within
    1e-6 of max|ref| of the fp64 column sums of the dy the site got.  With the switch on the backward runs four row quantisers less (the dy
    passes), no column quantiser at all, and the dual quantiser eight times under store "bf16" (dy and x of four sites) and four times under
    store "mx", where the re-blocker moves as before.  The stash is empty after the backward.  overlap=False is the path without an
    AsyncWgrad."""
    off, on = _block_run(dev, store, False, overlap), _block_run(dev, store, True, overlap)
    assert torch.equal(off["dx"].view(torch.int16), on["dx"].view(torch.int16))
    weights = [n for n in off["grads"] if n.endswith("weight") and off["grads"][n].dim() == 2]
    assert len(weights) == 4 and len(on["dys"]) == 4
    for n in weights:
        assert torch.equal(off["grads"][n], on["grads"][n]), (n, int((off["grads"][n] != on["grads"][n]).sum()))
        nb = n.replace("weight", "bias")
        ref = on["dys"][n].double().sum(dim=0)
        for tag, r in (("off", off), ("on", on)):
            err = float((r["grads"][nb].double() - ref).abs().max() / ref.abs().max())
            print(f"store={store} overlap={overlap} switch {tag} {nb}: worst element {err:.2e} of max|ref|")
            assert err <= COLSUM_BOUND, (tag, nb, err)
    print(f"store={store} overlap={overlap}: (dual, rows, columns, re-blocker) off {off['bwd']} on {on['bwd']}")
    assert off["bwd"][0] == 0
    assert on["bwd"][1] == off["bwd"][1] - 4, (off["bwd"], on["bwd"])
    assert on["bwd"][2] == 0, on["bwd"]
    assert on["bwd"][0] == (8 if store == "bf16" else 4), on["bwd"]
    assert on["bwd"][3] == off["bwd"][3] == (0 if store == "bf16" else 4), (off["bwd"], on["bwd"])
    assert on["stash"] is None and off["stash"] is None


# ---- 6. stash safety ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_stash_is_taken_once_and_only_by_its_own_tensor(dev):
    """After swin_linear_wgrad(dy) a swin_linear_dgrad on a DIFFERENT tensor of the same shape runs the ordinary row quantiser (by counter) and
    gives the switch-off result; swin_linear_dgrad(dy) takes the stashed rows (no row quantiser) and a second one on the same dy runs the
    row quantiser again - all three results equal the switch-off results bit for bit."""
    M, K, N = 392, 192, 768
    g = torch.Generator().manual_seed(21)
    w = torch.nn.Parameter((torch.randn(N, K, generator=g) / K ** 0.5).to(dev))
    spec = ops.ConvSpec.linear(K, N)
    lib = hip.load()

    def rows():
        return int(lib.sv_quant_rows_mx_launches())

    try:
        ops.set_math("bf16")
        ops.set_storage("bf16")
        S.set_linear_fp8(True, backward=True, recipe="mx", backward_recipe="mx")
        dy = torch.randn(M, N, generator=g).bfloat16().to(dev)
        other = torch.randn(M, N, generator=g).bfloat16().to(dev)
        x = torch.randn(M, K, generator=g).bfloat16().to(dev)

        def dgrad(t):
            dx = ops.empty(M, K, device=dev)
            ops.swin_linear_dgrad(t, M, spec, w, dx)
            torch.cuda.synchronize()
            return dx

        def wgrad():
            dw, db = torch.zeros(N, K, device=dev), torch.zeros(N, device=dev)
            ops.swin_linear_wgrad(dy, x, M, spec, w, dw, db)
            torch.cuda.synchronize()
            return dw

        ref_dy, ref_other, ref_dw = dgrad(dy), dgrad(other), wgrad()
        ops.set_mx_dual_quant(True)
        d0 = int(lib.sv_quant_rows_cols_mx_launches())
        dw = wgrad()
        assert int(lib.sv_quant_rows_cols_mx_launches()) == d0 + 2 and ops._CTX.dyq is not None and ops._CTX.dyq[0] is dy
        assert torch.equal(dw, ref_dw)
        r0 = rows()
        got = dgrad(other)                                     # not the stashed tensor: the ordinary row quantiser
        assert rows() == r0 + 1 and torch.equal(got.view(torch.int16), ref_other.view(torch.int16))
        assert ops._CTX.dyq is None
        wgrad()
        r0 = rows()
        got = dgrad(dy)                                        # the stashed rows
        assert rows() == r0 and ops._CTX.dyq is None and torch.equal(got.view(torch.int16), ref_dy.view(torch.int16))
        got = dgrad(dy)                                        # the slot was consumed
        assert rows() == r0 + 1 and torch.equal(got.view(torch.int16), ref_dy.view(torch.int16))
        wgrad()
        assert ops._CTX.dyq is not None
        ops.set_async_wgrad(None)                              # the module boundary clears the slot
        assert ops._CTX.dyq is None
    finally:
        ops.set_mx_dual_quant(False)
        S.set_linear_fp8(False)
        ops.set_math("f32")
