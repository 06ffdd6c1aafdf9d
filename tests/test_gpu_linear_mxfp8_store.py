"""MXFP8 Swin linears with the inputs stored as MX rows (set_linear_fp8(..., store="mx")) on the GPU: the re-blocker against its CPU
definition, the exact-integer chain re-blocker -> MX weight gradient, the producers that stop writing the tensor (sv_linear_mxfp8 with a
null `out`, sv_layernorm_quant_mx_fwd with a null `y`) and one unfused Swin block whose tape holds the MX rows."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_linear_fp8_recipe import l1_rel  # noqa: E402
from test_cpu_linear_mxfp8_recipe import mx_dequant, mx_integer_case, mx_quant_rows  # noqa: E402
from test_cpu_linear_mxfp8_store_recipe import emulate_wgrad_mx_stored, integer_rows_case, mx_reblock  # noqa: E402
from test_gpu_linear_mxfp8_bwd import COLSUM_BOUND, L1_F32, MAX_BOUND, _guarded, _wgrad_q  # noqa: E402  (the bounds are imported, not restated)

import swinvox_amd as S  # noqa: E402
from swinvox_amd import hip, ops  # noqa: E402
from swinvox_amd.ops import call, ptr  # noqa: E402

GUARD = 2              # guard rows in front of and behind both outputs of the re-blocker
STORE_VS_BF16 = 1e-4   # weight gradients, store "mx" against store "bf16": the CPU distance is <= 1e-5 (REBLOCK_BOUND); a wrong operand gives order 1


def _code(t):
    return hip.BF16 if t.dtype == torch.bfloat16 else hip.F32


def _counters():
    lib = hip.load()
    return (int(lib.sv_mx_rows_to_cols_launches()), int(lib.sv_quant_cols_mx_launches()), int(lib.sv_quant_rows_mx_launches()))


def _reblock(xq, xs, M, K):
    """sv_mx_rows_to_cols into poisoned buffers with GUARD rows on either side -> (bytes [GUARD + K + GUARD, Mp], scales [GUARD + K + GUARD, Mp / 32])"""
    Mp = (M + 127) // 128 * 128
    q = torch.full((K + 2 * GUARD, Mp), 0x7F, dtype=torch.uint8, device=xq.device)          # e4m3 NaN
    s = torch.full((K + 2 * GUARD, Mp // 32), 0xFF, dtype=torch.uint8, device=xq.device)    # E8M0 NaN: a byte the recipe never produces
    call("sv_mx_rows_to_cols", ptr(xq), xq.shape[1], ptr(xs), M, K, ptr(q[GUARD:]), Mp, ptr(s[GUARD:]))
    return q, s


def _check_reblock(name, xq, xs, M, K, dev):
    ref_q, ref_s = mx_reblock(xq, xs, K)
    q, s = _reblock(xq.to(dev), xs.to(dev), M, K)
    torch.cuda.synchronize()
    q, s = q.cpu(), s.cpu()
    assert torch.equal(s[GUARD:GUARD + K], ref_s), (name, int((s[GUARD:GUARD + K] != ref_s).sum()))
    assert torch.equal(q[GUARD:GUARD + K], ref_q), (name, int((q[GUARD:GUARD + K] != ref_q).sum()))
    for part in (q[:GUARD], q[GUARD + K:]):
        assert bool((part == 0x7F).all()), name
    for part in (s[:GUARD], s[GUARD + K:]):
        assert bool((part == 0xFF).all()), name
    return ref_q, ref_s


# ---- 1. the re-blocker ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K", [30, 96, 288])
@pytest.mark.parametrize("M", [37, 128, 401])
def test_reblocker_is_the_column_quantiser_on_the_dequantised_rows(dev, M, K):
    """Bytes and scale bytes equal mx_reblock bit for bit.  The rows come from mx_quant_rows of bf16 data spread over 16 binades per token and
    per column (a factor 2^-8 ... 2^8 for every token and one for every column), so a row block's and a column block's exponent through
    one element differ; row 3 has an all-zero first block and column 2 is all zero.  Second case: the rows scaled by 1e-20 and 1e20 in turn (scale bytes far from 127 on both sides).  M = 37 and 401 end in a
    partly filled block followed by padding (zero bytes, byte 127); K = 30 and 288 leave padding columns in the rows.  The guard rows on
    both sides of both outputs keep their fill, 0x7E in the padding columns K .. Kp - 1 of the rows changes nothing, and the launch counter
    moves by the number of calls."""
    g = torch.Generator().manual_seed(M * 1000 + K)
    x = torch.randn(M, K, generator=g)
    x *= torch.exp2(torch.randint(-8, 9, (M, 1), generator=g).float()) * torch.exp2(torch.randint(-8, 9, (1, K), generator=g).float())
    x[:, 2] = 0.0
    x[3, :min(K, 32)] = 0.0
    n0 = _counters()
    xq, xs = mx_quant_rows(x.bfloat16())
    assert int(xs[3, 0]) == 127
    ref_q, ref_s = _check_reblock("spread", xq, xs, M, K, dev)
    assert int(ref_q[2].max()) == 0 and bool((ref_s[2] == 127).all())
    assert ref_s[:, :M // 32 + 1].unique().numel() > 4                     # the block exponents do differ
    dirty = xq.clone()
    dirty[:, K:] = 0x7E
    _check_reblock("dirty padding columns", dirty, xs, M, K, dev)
    big = x * torch.where(torch.arange(M)[:, None] % 2 == 0, 1e-20, 1e20)
    xq2, xs2 = mx_quant_rows(big.bfloat16())
    assert int(xs2.min()) < 70 and int(xs2.max()) > 180
    _check_reblock("rows times 1e-20 / 1e20", xq2, xs2, M, K, dev)
    n1 = _counters()
    assert n1 == (n0[0] + 3, n0[1], n0[2])


@pytest.mark.gpu
def test_reblocker_decodes_fp32_denormals_exactly(dev):
    """The decode byte 2^(s - 127) is exact only with fp32 denormals preserved (header of linear_fp8.hip).  Rows of bf16 data around 2^-120,
    spread over 2^-8 ... 2^8 per token and per column: scale bytes down to 0, decoded values that are fp32 denormals, and column blocks whose
    maximum is one.  Bytes and scale bytes equal mx_reblock bit for bit."""
    M, K = 70, 96
    g = torch.Generator().manual_seed(7)
    x = torch.randn(M, K, generator=g) * 2.0 ** -120
    x *= torch.exp2(torch.randint(-8, 9, (M, 1), generator=g).float()) * torch.exp2(torch.randint(-8, 9, (1, K), generator=g).float())
    xq, xs = mx_quant_rows(x.bfloat16())
    vals = mx_dequant(xq, xs, torch.float32)
    assert int(xs[:, :K // 32].min()) < 8 and bool(((vals != 0) & (vals.abs() < 2.0 ** -126)).any())
    _check_reblock("denormals", xq, xs, M, K, dev)


# ---- 2. exact integers: re-blocker -> MX weight gradient ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("splits", [1, 3, 0])
@pytest.mark.parametrize("shape", [(49, 96, 288), (401, 192, 192), (37, 99, 30)])
def test_exact_integers_reblocker_then_wgrad(dev, shape, splits):
    """x = integers times 2^p per row (its MX rows lose nothing, tests/test_cpu_linear_mxfp8_store_recipe.py), dy^T from mx_integer_case:
    sv_mx_rows_to_cols followed by sv_linear_mxfp8_wgrad into an integer-prefilled dw equals the fp32 product of the dequantised pairs bit
    for bit - a transposed, shifted or wrongly scaled block of the re-blocked operand would show."""
    M, K, N = shape
    x, (xq, xs) = integer_rows_case(M, K)
    (dyt, dys), _ = mx_integer_case(N, M, K, seed=1)
    fill = torch.randint(-3, 4, (N, K), generator=torch.Generator().manual_seed(9)).float()
    ref = (mx_dequant(dyt, dys)[:, :M] @ mx_dequant(xq, xs)[:, :K] + fill.double()).float()
    dw, ldw = _guarded(N, K, dev)
    dw[:N, :K] = fill.to(dev)
    xt, xts = _reblock(xq.to(dev), xs.to(dev), M, K)
    _wgrad_q(dyt.to(dev), dys.to(dev), xt[GUARD:], xts[GUARD:], dw, M, K, N, ldw=ldw, splits=splits)
    torch.cuda.synchronize()
    got = dw.cpu()
    assert torch.equal(got[:N, :K], ref), (float((got[:N, :K] - ref).abs().max()), int((got[:N, :K] != ref).sum()))
    assert bool(torch.isnan(got[N:]).all()) and bool(torch.isnan(got[:, K:]).all())


# ---- 3. fc1 without `out` -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("store", ["bf16", "f32"])
@pytest.mark.parametrize("shape", [(130, 96, 384), (49, 192, 768)])
def test_linear_mxfp8_with_pre_act_and_null_out(dev, shape, store):
    """sv_linear_mxfp8 with q_out, pre_act and out == NULL (what fc1 runs under store "mx"): pre_act and the emitted rows are bit-identical to
    the call that also stores out."""
    M, K, N = shape
    dt = torch.bfloat16 if store == "bf16" else torch.float32
    g = torch.Generator().manual_seed(M + K)
    x = torch.randn(M, K, generator=g).to(dt).to(dev)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
    bias = (0.1 * torch.randn(N, generator=g)).to(dev)
    xq, xs = ops.quantize_rows_mx(x, M, K, activation=False)
    wq, ws = ops.quantize_rows_mx(W, N, K, activation=False)

    def run(with_out):
        out = torch.full((M, N), float("nan"), dtype=dt, device=dev) if with_out else None
        pre = torch.full((M, N), float("nan"), dtype=dt, device=dev)
        q = torch.full((M, N), 0x7F, dtype=torch.uint8, device=dev)
        qs = torch.full((M, N // 32), 0xFF, dtype=torch.uint8, device=dev)
        e = ops._epilogue(N, bias=bias, act=hip.ACT_GELU, pre_act=pre)
        call("sv_linear_mxfp8", ptr(xq), ptr(xs), ptr(wq), ptr(ws), ptr(out), M, K, N, C.byref(e), ptr(q), ptr(qs), act=_code(pre))
        torch.cuda.synchronize()
        return out, pre, q, qs

    out_a, pre_a, q_a, qs_a = run(True)
    _, pre_b, q_b, qs_b = run(False)
    assert bool(torch.isfinite(pre_a.float()).all()) and bool(torch.isfinite(out_a.float()).all())
    assert torch.equal(pre_a.view(torch.uint8), pre_b.view(torch.uint8))
    assert torch.equal(q_a, q_b) and torch.equal(qs_a, qs_b)
    ref_q, ref_s = mx_quant_rows(out_a.cpu())                                # and the rows are those of the stored output
    assert torch.equal(q_a.cpu(), ref_q) and torch.equal(qs_a.cpu(), ref_s)


# ---- 4. LayerNorm without `y` ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("Cd", [96, 100, 384])
def test_layernorm_quant_mx_with_null_y(dev, Cd):
    """sv_layernorm_quant_mx_fwd with y == NULL and the statistics given (ops.layernorm_quant_mx_fwd(store_y=False)): q, scales, mean and
    rstd are bit-identical to the storing call, in both storage types."""
    rows = 37
    g = torch.Generator().manual_seed(Cd)
    gamma, beta = (1.0 + 0.2 * torch.randn(Cd, generator=g)).to(dev), (0.1 * torch.randn(Cd, generator=g)).to(dev)
    try:
        for store in ("bf16", "f32"):
            ops.set_math("bf16")
            ops.set_storage(store)
            x = ops.to_store((torch.randn(rows, Cd, generator=g) * 3.0 + 0.5).to(dev))
            n0 = ops.layernorm_quant_mx_launches()
            y, m, r, q, s = ops.layernorm_quant_mx_fwd(x, gamma, beta, rows, Cd)
            y2, m2, r2, q2, s2 = ops.layernorm_quant_mx_fwd(x, gamma, beta, rows, Cd, store_y=False)
            torch.cuda.synchronize()
            assert ops.layernorm_quant_mx_launches() == n0 + 2
            assert y is not None and y2 is None and m2 is not None and r2 is not None
            assert torch.equal(q, q2) and torch.equal(s, s2), store
            assert torch.equal(m.view(torch.int32), m2.view(torch.int32)) and torch.equal(r.view(torch.int32), r2.view(torch.int32)), store
            ref_q, ref_s = mx_quant_rows(y.cpu())
            assert torch.equal(q.cpu(), ref_q) and torch.equal(s.cpu(), ref_s), store
    finally:
        ops.set_math("f32")


# ---- 5. one Swin block ----------------------------------------------------------------------------------------------------------------------
CD, HEADS, RES, IMGS = 192, 6, 14, 2
_BLOCK = {}


def _tensors(obj):
    if isinstance(obj, torch.Tensor):
        return [obj]
    if isinstance(obj, (tuple, list)):
        return [t for o in obj for t in _tensors(o)]
    return []


def _block_run(dev, store, emit):
    """forward (save=True) + backward of one SwinBlock under the MX forward and backward; every call of swin_linear_wgrad and layernorm_bwd
    is recorded with copies of its operands.  One run per (store, emit), kept for the tests below."""
    key = (store, emit)
    if key in _BLOCK:
        return _BLOCK[key]
    from swinvox_amd.models.swin_transformer import SwinBlock, block_backward, block_forward
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
    grads = {p: torch.zeros_like(p, dtype=torch.float32) for p in blk.parameters()}
    rec = dict(wgrad=[], ln=[])
    real_wgrad, real_ln = ops.swin_linear_wgrad, ops.layernorm_bwd

    def spy_wgrad(dy_, x_, rows, spec, w, dw, db=None, async_ok=True):
        rec["wgrad"].append((w, dy_.detach().cpu().clone(), tuple(t.cpu().clone() for t in x_) if isinstance(x_, tuple) else x_.detach().cpu().clone()))
        return real_wgrad(dy_, x_, rows, spec, w, dw, db, async_ok=async_ok)

    def spy_ln(dy_, x_, gamma, mean, rstd, *a, **k):
        rec["ln"].append((gamma, dy_.detach().float().cpu().double(), x_.detach().float().cpu().double(), mean.cpu().double(), rstd.cpu().double()))
        return real_ln(dy_, x_, gamma, mean, rstd, *a, **k)

    try:
        ops.set_math("bf16")
        ops.set_storage("bf16")
        S.set_linear_fp8(True, backward=True, recipe="mx", backward_recipe="mx", store=store)
        ops.set_ln_quant_mx(emit)
        ops.set_mx_producer_quant(emit)
        ops.swin_linear_wgrad, ops.layernorm_bwd = spy_wgrad, spy_ln
        n0, a0 = _counters(), ops.mx_act_quant_launches()
        x2, ctx = block_forward(blk, x, IMGS, True, False, None, True)
        torch.cuda.synchronize()
        n1, a1 = _counters(), ops.mx_act_quant_launches()
        tape = [(i, t) for i, o in enumerate(ctx) for t in _tensors(o)]
        tape_info = dict(kinds=[type(o) for o in ctx], entries=[(i, tuple(t.shape), t.dtype, t.numel() * t.element_size(), t.data_ptr()) for i, t in tape],
                         ptrs=dict(x=ctx[0].data_ptr(), x1=ctx[8].data_ptr(), hpre=ctx[12].data_ptr()))
        dx = block_backward(blk, ctx, dy.clone(), grads)
        torch.cuda.synchronize()
        n2 = _counters()
    finally:
        ops.swin_linear_wgrad, ops.layernorm_bwd = real_wgrad, real_ln
        ops.set_ln_quant_mx(False)
        ops.set_mx_producer_quant(True)
        S.set_linear_fp8(False)
        ops.set_math("f32")
    names = {p: n for n, p in blk.named_parameters()}
    _BLOCK[key] = dict(x2=x2.cpu(), dx=dx.cpu(), grads={names[p]: v.cpu() for p, v in grads.items()}, rec=rec, names=names, tape=tape_info,
                       fwd=tuple(b - a for a, b in zip(n0, n1)) + (a1 - a0,), bwd=tuple(b - a for a, b in zip(n1, n2)))
    return _BLOCK[key]


@pytest.mark.gpu
@pytest.mark.parametrize("emit", [True, False])
def test_block_tape_holds_the_mx_rows(dev, emit):
    """save=True under store "mx": the tape entries of ln1 / att / ln2 / h are uint8 pairs, no tensor of the storage type with shape [M, C] or
    [M, 4C] other than x, x1 and hpre is on the tape, and its size is the value the shapes give - below the bf16-store tape by exactly
    3 (2 C - Kp 33 / 32) + (8 C - 4 C 33 / 32) bytes per token.  With both emission switches on no stand-alone activation quantiser runs;
    with both off the tape is the same and the four quantisers run instead.  The backward re-blocks four times and quantises four columns
    operands less."""
    M, Kp = IMGS * RES * RES, 256
    r, b = _block_run(dev, "mx", emit), _block_run(dev, "bf16", True)
    kinds = r["tape"]["kinds"]
    for i in (3, 5, 11, 13):
        assert kinds[i] is tuple and b["tape"]["kinds"][i] is torch.Tensor, i
    pairs = {i: [e for e in r["tape"]["entries"] if e[0] == i] for i in (3, 5, 11, 13)}
    for i, K in ((3, CD), (5, CD), (11, CD), (13, 4 * CD)):
        kp = (K + 127) // 128 * 128
        assert [(e[1], e[2]) for e in pairs[i]] == [((M, kp), torch.uint8), ((M, kp // 32), torch.uint8)], (i, pairs[i])
    keep = set(r["tape"]["ptrs"].values())
    wide = [e for e in r["tape"]["entries"] if e[2] == torch.bfloat16 and e[1] in ((M, CD), (M, 4 * CD))]
    assert len(wide) == 3 and {e[4] for e in wide} == keep, wide
    size = sum(e[3] for e in r["tape"]["entries"])
    want = M * (2 * CD * 2 + 4 * 4 + 3 * CD * 2 + 4 * CD * 2 + 3 * (Kp + Kp // 32) + (4 * CD + 4 * CD // 32))   # x x1, 4 statistics, qkv, hpre, 3 + 1 pairs
    size_b = sum(e[3] for e in b["tape"]["entries"])
    print(f"tape bytes: store mx {size}, store bf16 {size_b}, per token {size / M:.1f} / {size_b / M:.1f}")
    assert size == want, (size, want)
    assert size_b - size == M * (3 * (2 * CD - Kp * 33 // 32) + (8 * CD - 4 * CD * 33 // 32)), (size_b, size)
    assert r["fwd"][0] == 0 and r["fwd"][3] == (0 if emit else 4), r["fwd"]
    assert b["fwd"][3] == 0
    assert r["bwd"][0] == 4 and b["bwd"][0] == 0 and b["bwd"][1] - r["bwd"][1] == 4, (r["bwd"], b["bwd"])


@pytest.mark.gpu
@pytest.mark.parametrize("emit", [True, False])
def test_block_results(dev, emit):
    """x2 and dx are bit-identical to store "bf16" (neither reads the tape entries that changed).  The four weight gradients are within the dw
    bound of tests/test_gpu_linear_mxfp8_bwd.py of the CPU emulation of this recipe on the operands the kernels got, and within 1e-4 of the
    store "bf16" run.  The bias gradients and the LayerNorm gradients are within that file's column-sum bound (1e-6 of max|ref|) of the fp64
    sums, formed from the operands the kernels got; the LayerNorm gradients are within the same bound of the store "bf16" run too
    (layernorm_bwd reads nothing the switch changes, dx being bit-identical: only the order of its fp32 atomics differs)."""
    r, b = _block_run(dev, "mx", emit), _block_run(dev, "bf16", True)
    assert torch.equal(r["x2"].view(torch.int16), b["x2"].view(torch.int16))
    assert torch.equal(r["dx"].view(torch.int16), b["dx"].view(torch.int16))
    assert len(r["rec"]["wgrad"]) == 4 and len(r["rec"]["ln"]) == 2
    for w, dy, xp in r["rec"]["wgrad"]:
        n = r["names"][w]
        assert isinstance(xp, tuple), n
        N, K = w.shape
        ref = emulate_wgrad_mx_stored(dy, xp[0], xp[1], K)
        got = r["grads"][n].double()
        l1, mx = l1_rel(got, ref), float((got - ref).abs().max() / ref.abs().max())
        vs = l1_rel(got, b["grads"][n])
        print(f"emit={emit} {n}: vs CPU emulation L1-rel {l1:.3e} worst {mx:.3e}; vs store bf16 L1-rel {vs:.3e}")
        assert l1 <= L1_F32 and mx <= MAX_BOUND, (n, l1, mx)
        assert vs <= STORE_VS_BF16, (n, vs)
        nb = n.replace("weight", "bias")
        ref_b = dy.double().sum(dim=0)
        err = float((r["grads"][nb].double() - ref_b).abs().max() / ref_b.abs().max())
        print(f"emit={emit} {nb}: worst element {err:.2e} of max|ref|")
        assert err <= COLSUM_BOUND, (nb, err)
    for gamma, dln, xin, mean, rstd in r["rec"]["ln"]:
        n = r["names"][gamma]
        xhat = (xin - mean[:, None]) * rstd[:, None]
        for name, terms in ((n, dln * xhat), (n.replace("weight", "bias"), dln)):
            ref = terms.sum(dim=0)
            err = float((r["grads"][name].double() - ref).abs().max() / ref.abs().max())
            vs = float((r["grads"][name].double() - b["grads"][name].double()).abs().max() / ref.abs().max())
            print(f"emit={emit} {name}: worst element {err:.2e} of max|ref| from the fp64 sums, {vs:.2e} from the store bf16 run")
            assert err <= COLSUM_BOUND, (name, err)
            assert vs <= COLSUM_BOUND, (name, vs)
