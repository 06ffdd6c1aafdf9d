"""The MXFP8 forward of the fused Swin MLP (swinvox_amd/csrc/swin_mlp.hip, swin_mlp_fwd_mx_kernel) as a torch emulation, an exact-integer case
generator whose invariants are checked here, and the C ABI of its entry points without a GPU.

The recipe is the unfused MX chain's, composed: LayerNorm in fp32 rounded to bf16 -> MX rows (blocks of 32 channels) -> fc1 on MX operands ->
+ b1, the fast GELU of common.h, rounded to bf16 -> MX rows (blocks of 32 hidden units) -> fc2 on MX operands -> + b2, drop-path scale, + x1.
tests/test_gpu_swin_mlp_mx.py measures the kernel with emulate_swin_mlp_mx and with integer_case, so both are tested on their own here."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_linear_mxfp8_recipe import emulate_linear_mx, mx_dequant, mx_quant_rows  # noqa: E402

from swinvox_amd import hip  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the emulation --------------------------------------------------------------------------------------------------------------------
def gelu_fast32(x):
    """common.h gelu_fast restated in fp32: x * 1 / (1 + exp2(x p)), p = -log2(e) (c0 + c1 x^2 + c2 x^4), x^2 clamped at 64"""
    assert x.dtype == torch.float32
    x2 = torch.clamp(x * x, max=64.0)
    p = x2 * (x2 * 9.975397e-04 + -1.0665937e-01) + -2.3012706e+00
    return x * (1.0 / (1.0 + torch.exp2(x * p)))


def layernorm_bf16(x1, ln_g, ln_b, eps):
    """LayerNorm in fp32, rounded to bf16: the value the unfused chain stores"""
    x = x1.float()
    mean = x.mean(dim=1, keepdim=True)
    d = x - mean
    rstd = torch.rsqrt((d * d).mean(dim=1, keepdim=True) + eps)
    return (d * rstd * ln_g.float() + ln_b.float()).to(torch.bfloat16)


def emulate_swin_mlp_mx(x1, ln_g, ln_b, W1, b1, W2, b2, row_scale=None, rows_per_scale=1, eps=1e-5):
    """x2 = x1 + s (fc2(GELU(fc1(LN(x1)) + b1)) + b2) under the MX recipe, in fp64 before the bf16 store rounding"""
    ln = layernorm_bf16(x1, ln_g, ln_b, eps)
    pre, _ = emulate_linear_mx(ln, W1, bias=b1)
    h = gelu_fast32(pre.float()).to(torch.bfloat16)
    out, _ = emulate_linear_mx(h, W2, bias=b2, residual=x1, row_scale=row_scale, rows_per_scale=rows_per_scale)
    return out


def gauss_mlp_case(M, C, seed=0, windows=None):
    """N(0, 1) token rows (bf16), LayerNorm parameters near (1, 0), weights of the usual 1 / sqrt(K) size; row_scale per `windows` rows"""
    g = torch.Generator().manual_seed(7000 + 13 * C + seed)
    x1 = torch.randn(M, C, generator=g).to(torch.bfloat16)
    ln_g = 1.0 + 0.1 * torch.randn(C, generator=g)
    ln_b = 0.1 * torch.randn(C, generator=g)
    W1 = torch.randn(4 * C, C, generator=g) / C ** 0.5
    b1 = 0.1 * torch.randn(4 * C, generator=g)
    W2 = torch.randn(C, 4 * C, generator=g) / (4 * C) ** 0.5
    b2 = 0.1 * torch.randn(C, generator=g)
    rps = windows or 1
    n = (M + rps - 1) // rps
    row_scale = torch.tensor([0.0, 1.0 / 0.9, 1.0 / 0.8])[torch.randint(0, 3, (n,), generator=g)] if windows else None
    if row_scale is not None:
        row_scale[min(1, n - 1)] = 1.0 / 0.9              # at least one live group
    return dict(x1=x1, ln_g=ln_g, ln_b=ln_b, W1=W1, b1=b1, W2=W2, b2=b2, row_scale=row_scale, rows_per_scale=rps, eps=1e-5)


@pytest.mark.parametrize("C", [96, 128])
def test_emulation_is_the_composition_of_the_mx_helpers(C):
    c = gauss_mlp_case(37, C, windows=5)
    out = emulate_swin_mlp_mx(**c)
    ln = layernorm_bf16(c["x1"], c["ln_g"], c["ln_b"], c["eps"])
    ref_ln = torch.nn.functional.layer_norm(c["x1"].float(), (C,), c["ln_g"], c["ln_b"], c["eps"])
    assert float((ln.float() - ref_ln).abs().max()) <= 2.0 ** -7 * float(ref_ln.abs().max())      # one bf16 rounding
    lq, ls = mx_quant_rows(ln)
    assert lq.shape == (37, 128) and ls.shape == (37, 4)
    if C == 96:
        assert int(lq[:, 96:].max()) == 0 and bool((ls[:, 3] == 127).all())                        # K padding: zero bytes, byte 127
    w1q, w1s = mx_quant_rows(c["W1"])
    pre = mx_dequant(lq, ls) @ mx_dequant(w1q, w1s).T + c["b1"].double()
    h = gelu_fast32(pre.float()).to(torch.bfloat16)
    erf = 0.5 * pre * (1.0 + torch.erf(pre / 2.0 ** 0.5))
    assert float((gelu_fast32(pre.float()).double() - erf).abs().max()) < 4e-5                     # common.h: |fast - erf| <= 2.9e-5
    hq, hs = mx_quant_rows(h)
    assert hq.shape == (37, 4 * C) and hs.shape == (37, 4 * C // 32)                               # blocks of 32 consecutive hidden units
    w2q, w2s = mx_quant_rows(c["W2"])
    val = mx_dequant(hq, hs) @ mx_dequant(w2q, w2s).T + c["b2"].double()
    sc = c["row_scale"].double()[torch.arange(37) // c["rows_per_scale"]]
    assert torch.equal(out, c["x1"].double() + sc[:, None] * val)


# ---- exact integers ---------------------------------------------------------------------------------------------------------------------
def _sig_bits_le4(v):
    """every non-zero |v| is m 2^e with m an integer below 16"""
    a = v.double().abs()
    a = a[a > 0]
    e = torch.floor(torch.log2(a))
    return bool(((a / torch.exp2(e - 3)) % 1 == 0).all())


def integer_case(M, C, seed=0):
    """A case every intermediate of which is a small integer, so that the MX recipe, bf16 products and plain integer arithmetic agree bit for
    bit and any wrong lane, block or scale changes the result.
      LayerNorm   ln_g = 0: LN(x1) = ln_b for every token.  ln_b = v 2^e[block], v integer, |v| <= 15 (<= 4 significant bits: exact in e4m3), one
                  |v| = 15 per 32-channel block, e a permutation of 0 .. 3: the block scale bytes are non-unit and all differ.
      fc1         every W1 row has one non-zero (+-1 or +-2 at a channel of its own choice); b1 makes the pre-activation t = u 2^s, u in 8 .. 15,
                  s = (hidden block) mod 3, one u = 15 per 32-unit block: an integer >= 8 with <= 4 significant bits.  gelu_fast is the identity there
                  in fp32 (1 + exp2(x p) rounds to 1 for x >= 8, p ~ -5.04 at the clamp), so h = t and the hidden blocks' scale bytes differ.
      fc2         every W2 row has a + entry (2 where s = 0, else 1) and a -1 entry in another hidden block: |acc| <= 52; b2 integers |b2| <= 4.
      epilogue    x1 integers |x1| <= 4, row_scale in {1/2, 1, 2} per token (rows_per_scale = 1): |x2| <= 4 + 2 * 56 < 256 and every x2 is a multiple
                  of 1/2 below 128 or an integer below 256 - the bf16 store is exact.
    Returns the case (emulate_swin_mlp_mx's arguments) and the integer reference x2 [M, C] in fp64."""
    g = torch.Generator().manual_seed(9000 + 7 * C + seed)
    HID, NB, NHB = 4 * C, C // 32, 4 * C // 32
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g)   # noqa: E731
    v = ri(-15, 15, C)
    v[torch.arange(NB) * 32 + ri(0, 31, NB)] = 15
    eb = torch.randperm(4, generator=g)[:NB]
    ln_b = (v * 2 ** eb.repeat_interleave(32)).double()
    col = ri(0, C - 1, HID)
    w = torch.tensor([1.0, -1.0, 2.0, -2.0], dtype=torch.float64)[ri(0, 3, HID)]
    W1 = torch.zeros(HID, C, dtype=torch.float64)
    W1[torch.arange(HID), col] = w
    u = ri(8, 15, HID)
    u[torch.arange(NHB) * 32 + ri(0, 31, NHB)] = 15
    s_h = (torch.arange(HID) // 32) % 3
    target = (u * 2 ** s_h).double()
    b1 = target - w * ln_b[col]
    a = ri(0, HID - 1, C)
    b = (a + 32 * ri(1, NHB - 1, C)) % HID                                     # another hidden block
    W2 = torch.zeros(C, HID, dtype=torch.float64)
    W2[torch.arange(C), a] = torch.where(s_h[a] == 0, 2.0, 1.0).double()
    W2[torch.arange(C), b] = -1.0
    b2 = ri(-4, 4, C).double()
    x1 = ri(-4, 4, M, C).double()
    row_scale = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[ri(0, 2, M)]
    ref = x1 + row_scale[:, None] * ((W2 @ (W1 @ ln_b + b1)) + b2)[None, :]
    case = dict(x1=x1.to(torch.bfloat16), ln_g=torch.zeros(C), ln_b=ln_b.float(), W1=W1.float(), b1=b1.float(), W2=W2.float(), b2=b2.float(),
                row_scale=row_scale.float(), rows_per_scale=1, eps=1e-5)
    return case, ref


@pytest.mark.parametrize("C", [96, 128])
@pytest.mark.parametrize("M", [1, 17, 200])
def test_integer_case_invariants(M, C):
    c, ref = integer_case(M, C)
    ln = layernorm_bf16(c["x1"], c["ln_g"], c["ln_b"], c["eps"])
    assert torch.equal(ln.double(), c["ln_b"].double()[None, :].expand(M, C))                      # LN(x1) = ln_b, exactly
    assert _sig_bits_le4(c["ln_b"])
    _, ls = mx_quant_rows(ln)
    sb = ls[0, :C // 32].tolist()
    assert 127 not in sb and len(set(sb)) == C // 32, sb                                           # non-unit scale bytes that all differ
    assert bool(((c["W1"] != 0).sum(dim=1) == 1).all())
    pre = c["W1"].double() @ c["ln_b"].double() + c["b1"].double()
    assert bool((pre >= 8).all()) and bool((pre % 1 == 0).all()) and _sig_bits_le4(pre)
    assert torch.equal(gelu_fast32(pre.float()), pre.float())                                      # the GELU identity, in fp32
    _, hs = mx_quant_rows(pre.float().to(torch.bfloat16)[None, :])
    assert len(set(hs[0].tolist())) >= 3 and 127 not in hs[0].tolist()                             # hidden blocks of differing magnitude
    assert bool(((c["W2"] != 0).sum(dim=1) == 2).all())
    assert float(ref.abs().max()) <= 256 and torch.equal(ref.to(torch.bfloat16).double(), ref)     # the bf16 store is exact
    assert set(c["row_scale"].tolist()) <= {0.5, 1.0, 2.0}
    out = emulate_swin_mlp_mx(**c)
    assert torch.equal(out, ref)                                                                   # the emulation IS integer arithmetic here
    unit = c["x1"].double() + c["row_scale"].double()[:, None] * (
        (c["W2"].double() @ pre) + c["b2"].double())[None, :]
    assert torch.equal(unit, ref)


# ---- pack images ------------------------------------------------------------------------------------------------------------------------
# The two kinds of image of the MX packs, gathered on the CPU from the layout the header comment of swin_mlp_fwd_mx_kernel documents (lane = (r, lg),
# lane index 16 lg + r; a lane's half hf is the 16 bytes k = 64 hf + 16 lg .. + 15 of the 128-wide k-step, its scale byte block lg of the k-step).
# tests/test_gpu_swin_mlp_mx.py and tests/test_gpu_swin_mlp_mx_bwd.py compare the device's images with them byte for byte.
def hidden_row_image(q, s):
    """q [4C][128], s [4C][4] (W1 or W2^T in MX rows) -> data [G][8 tiles][2 halves][64 lanes][16], scales [G][8][64]; tile j, row r of group g is
    hidden unit 128 g + 64 (j >> 2) + 16 (r >> 2) + 4 (j & 3) + (r & 3)"""
    HID = q.shape[0]
    G = HID // 128
    assert q.shape == (HID, 128) and s.shape == (HID, 4) and HID % 128 == 0
    g, j, r = torch.arange(G)[:, None, None], torch.arange(8)[None, :, None], torch.arange(16)[None, None, :]
    hid = 128 * g + 64 * (j >> 2) + 16 * (r >> 2) + 4 * (j & 3) + (r & 3)                          # [G][8][16]
    data = q.reshape(HID, 2, 4, 16)[hid]                                                           # [G][8][r][hf][lg][16]
    return data.permute(0, 1, 3, 4, 2, 5).reshape(G, 8, 2, 64, 16), s[hid].permute(0, 1, 3, 2).reshape(G, 8, 64)


def channel_row_image(q, s):
    """q [C][4C], s [C][4C / 32] (W2 or W1^T in MX rows) -> data [G][C/16][2][64][16], scales [G][C/16][64]; tile jc, row r is channel 16 jc + r,
    k-step g its hidden units 128 g .. + 127"""
    C, HID = q.shape
    G, NJ = HID // 128, C // 16
    assert HID == 4 * C and s.shape == (C, HID // 32)
    data = q.reshape(NJ, 16, G, 2, 4, 16).permute(2, 0, 3, 4, 1, 5)                                # [G][jc][hf][lg][r][16]
    return data.reshape(G, NJ, 2, 64, 16), s.reshape(NJ, 16, G, 4).permute(2, 0, 3, 1).reshape(G, NJ, 64)


def random_bytes(seed, *shape):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int32).to(torch.uint8)


@pytest.mark.parametrize("C", [96, 128])
def test_pack_images_are_permutations_in_fragment_order(C):
    HID = 4 * C
    # every byte keeps its identity: position codes instead of random bytes
    q = torch.arange(HID * 128, dtype=torch.int32).reshape(HID, 128)
    s = torch.arange(HID * 4, dtype=torch.int32).reshape(HID, 4)
    d, sc = hidden_row_image(q, s)
    assert sorted(d.flatten().tolist()) == list(range(HID * 128)) and sorted(sc.flatten().tolist()) == list(range(HID * 4))
    # lane (r = 5, lg = 2) of tile 6 of group 1, upper half: hidden unit 128 + 64 + 16 + 8 + 1, k = 64 + 32 ..; scale block 2
    assert d[1, 6, 1, 32 + 5].tolist() == q[217, 96:112].tolist() and int(sc[1, 6, 32 + 5]) == int(s[217, 2])
    # accumulator rows 4 lg .. + 3 of tiles 0-3 are the 16 consecutive hidden units 16 lg .. + 15 (registers 0-3 of the fc2 operand), tiles 4-7
    # the same 64 units on
    units = (d[0, :, 0, :16, 0] // 128).T                                                          # [r][j]: the hidden unit of row r of tile j
    for r in range(16):
        lo = 16 * (r >> 2) + (r & 3)
        assert units[r].tolist() == [lo + 4 * jj for jj in range(4)] + [64 + lo + 4 * jj for jj in range(4)]
    q = torch.arange(C * HID, dtype=torch.int32).reshape(C, HID)
    s = torch.arange(C * HID // 32, dtype=torch.int32).reshape(C, HID // 32)
    d, sc = channel_row_image(q, s)
    assert sorted(d.flatten().tolist()) == list(range(C * HID)) and sorted(sc.flatten().tolist()) == list(range(C * HID // 32))
    assert d[2, 3, 1, 48 + 7].tolist() == q[55, 256 + 64 + 48:256 + 64 + 64].tolist() and int(sc[2, 3, 48 + 7]) == int(s[55, 8 + 3])


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("sv_swin_mlp_mx_supported", "sv_swin_mlp_mx_pack_bytes", "sv_swin_mlp_mx_pack", "sv_swin_mlp_fwd_mx", "sv_swin_mlp_mx_launches")
SV_ERR_INVALID = -1


def test_header_declares_and_cites():
    hdr = open(os.path.join(ROOT, "include", "swinvox_hip.h")).read()
    for name in ENTRIES:
        m = re.search(r"(/\*(?:(?!\*/).)*\*/\s*)?\b(?:int|long long)\s+" + name + r"\s*\([^;]*\)\s*;[ \t]*(/\*(?:(?!\*/).)*\*/)?", hdr, flags=re.S)
        assert m, f"{name} is not declared"
        comment = (m.group(1) or "") + (m.group(2) or "")
        assert "models/swin_transformer.py:78" in comment, (name, comment)


def test_exported_and_bound():
    for name in ENTRIES:
        assert name in hip.EXPORTED_SYMBOLS
    lib = hip.load()                          # dlopen only: no GPU call is made
    assert lib.sv_swin_mlp_mx_launches() >= 0
    assert [lib.sv_swin_mlp_mx_supported(c) for c in (96, 128, 192, 64, 0)] == [1, 1, 0, 0, 0]
    assert lib.sv_swin_mlp_supported(192) == 1                                  # C = 192 stays on the paths it has
    # W1 rows padded to Kp = 128 + W2 rows + one E8M0 byte per 32 elements of either
    assert lib.sv_swin_mlp_mx_pack_bytes(96) == 384 * 128 + 96 * 384 + 384 * 4 + 96 * 12
    assert lib.sv_swin_mlp_mx_pack_bytes(128) == 512 * 128 + 128 * 512 + 512 * 4 + 128 * 16
    assert lib.sv_swin_mlp_mx_pack_bytes(192) == 0
    assert len(hip._argtypes("sv_swin_mlp_fwd_mx")) == 13 and len(hip._argtypes("sv_swin_mlp_mx_pack")) == 7
    assert hip._argtypes("sv_swin_mlp_fwd_mx") == hip._argtypes("sv_swin_mlp_fwd")


# fake, suitably aligned device addresses: every call below is refused before anything could read them
X1, X2, LG, LB, PK, B1, B2, RS, W1Q, W1S, W2Q, W2S = (0x10000 * (i + 1) for i in range(12))


@pytest.mark.parametrize("what,over", [
    ("x1 null", dict(x1=None)),
    ("x2 null", dict(x2=None)),
    ("ln_g null", dict(g=None)),
    ("ln_b null", dict(b=None)),
    ("packs null", dict(packs=None)),
    ("b1 null", dict(b1=None)),
    ("b2 null", dict(b2=None)),
    ("C = 192", dict(C=192)),
    ("C = 64", dict(C=64)),
    ("M = 0", dict(M=0)),
    ("M < 0", dict(M=-5)),
    ("M = 2^31", dict(M=1 << 31)),
    ("x1 misaligned", dict(x1=X1 + 8)),
    ("x2 misaligned", dict(x2=X2 + 2)),
    ("packs misaligned", dict(packs=PK + 4)),
    ("ln_g misaligned", dict(g=LG + 4)),
    ("ln_b misaligned", dict(b=LB + 8)),
    ("b2 misaligned", dict(b2=B2 + 4)),
    ("rows_per_scale = 0", dict(rps=0)),
    ("rows_per_scale < 0", dict(rps=-49)),
])
def test_forward_refusals_before_any_gpu_call(what, over):
    lib = hip.load()
    a = dict(x1=X1, x2=X2, g=LG, b=LB, packs=PK, b1=B1, b2=B2, rs=RS, rps=49, M=147, C=96)
    a.update(over)
    n0 = lib.sv_swin_mlp_mx_launches()
    rc = lib.sv_swin_mlp_fwd_mx(a["x1"], a["x2"], a["g"], a["b"], a["packs"], a["b1"], a["b2"], a["rs"], a["rps"], a["M"], a["C"], 1e-5, None)
    assert rc == SV_ERR_INVALID, (what, rc)
    assert "sv_swin_mlp_fwd_mx" in lib.sv_last_error().decode(), (what, lib.sv_last_error())
    assert lib.sv_swin_mlp_mx_launches() == n0, what


@pytest.mark.parametrize("what,over", [
    ("w1q null", dict(w1q=None)),
    ("w1s null", dict(w1s=None)),
    ("w2q null", dict(w2q=None)),
    ("w2s null", dict(w2s=None)),
    ("packs null", dict(packs=None)),
    ("C = 192", dict(C=192)),
    ("C = 0", dict(C=0)),
    ("w1q misaligned", dict(w1q=W1Q + 4)),
    ("w2q misaligned", dict(w2q=W2Q + 8)),
    ("packs misaligned", dict(packs=PK + 1)),
])
def test_pack_refusals_before_any_gpu_call(what, over):
    lib = hip.load()
    a = dict(w1q=W1Q, w1s=W1S, w2q=W2Q, w2s=W2S, packs=PK, C=128)
    a.update(over)
    rc = lib.sv_swin_mlp_mx_pack(a["w1q"], a["w1s"], a["w2q"], a["w2s"], a["packs"], a["C"], None)
    assert rc == SV_ERR_INVALID, (what, rc)
    assert "sv_swin_mlp_mx_pack" in lib.sv_last_error().decode(), (what, lib.sv_last_error())


def test_existing_entry_keeps_its_refusals():
    lib = hip.load()
    assert lib.sv_swin_mlp_fwd(X1, X2, LG, LB, PK, B1, B2, RS, 0, 147, 96, 1e-5, None) == SV_ERR_INVALID
    assert "swin_mlp" in lib.sv_last_error().decode()


def test_switch_is_off_by_default_and_needs_the_mx_recipe():
    from swinvox_amd import ops
    assert not ops._STATE.get("fused_mlp_mx", False)
    assert not ops.fused_mlp_mx_enabled(96)
