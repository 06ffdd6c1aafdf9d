"""The MXFP8 forward of the fused attention branch (swinvox_amd/csrc/attn.hip, swin_attn_block_fwd_mx_kernel) as a torch emulation, an exact case
whose invariants are checked here, the CPU gather of its pack image, the C ABI of its entry points and the host switch - all without a GPU.

The recipe is the unfused MX chain's, composed: LayerNorm in fp32 rounded to bf16 -> MX rows (blocks of 32 channels) -> qkv on MX operands, + bias,
rounded to bf16 -> window attention (bf16 core; fp64 here) with the head outputs rounded to bf16 -> MX rows (one block per head) -> proj on MX
operands -> + bias, drop-path scale per image, + x.  tests/test_gpu_swin_attn_block_mx.py measures the kernel with emulate_swin_attn_block_mx,
exact_case and attn_block_pack_image, so all three are tested on their own here."""
import contextlib
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from test_cpu_linear_mxfp8_recipe import emulate_linear_mx, mx_dequant, mx_quant_rows  # noqa: E402
from test_cpu_swin_mlp_mx_recipe import _sig_bits_le4, layernorm_bf16  # noqa: E402

from swinvox_amd import hip  # noqa: E402

C, HEADS, HD = 96, 3, 32


# ---- the emulation --------------------------------------------------------------------------------------------------------------------
def window_attention64(qkv, table, I, H, shift):
    """tests/test_gpu_swin_attn_block.py::_reference's core restated: fp64 window attention of qkv [I*H*H, 288] -> head outputs [I*H*H, 96]"""
    from oracle.model import rel_pos_index, shift_attn_mask
    t = qkv.double().view(I, H, H, 3 * C)
    if shift:
        t = torch.roll(t, (-shift, -shift), (1, 2))
    tw = t.view(I, H // 7, 7, H // 7, 7, 3 * C).permute(0, 1, 3, 2, 4, 5).reshape(-1, 49, 3, HEADS, HD).permute(2, 0, 3, 1, 4)
    q, k, v = tw[0] * HD ** -0.5, tw[1], tw[2]
    a = q @ k.transpose(-2, -1) + table.double()[rel_pos_index(7).reshape(-1)].view(49, 49, HEADS).permute(2, 0, 1)[None]
    if shift:
        m = shift_attn_mask(H, H, 7, shift).double()
        a = (a.view(I, -1, HEADS, 49, 49) + m[None, :, None]).view(-1, HEADS, 49, 49)
    o = (a.softmax(-1) @ v).transpose(1, 2).reshape(-1, 49, C)
    o = o.view(I, H // 7, H // 7, 7, 7, C).permute(0, 1, 3, 2, 4, 5).reshape(I, H, H, C)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    return o.reshape(-1, C)


def emulate_swin_attn_block_mx(x, lg, lb, wqkv, bqkv, table, wproj, bproj, I, H, shift, sc=None, eps=1e-5):
    """x1 = x + s (proj(window_attention(qkv(LN(x))))) under the MX recipe: ln1 and att as stored (bf16), qkv and x1 in fp64 before the bf16
    store rounding (att is computed from the ROUNDED qkv, as every kernel of the chain reads it back)"""
    ln = layernorm_bf16(x, lg, lb, eps)
    qkv, _ = emulate_linear_mx(ln, wqkv, bias=bqkv)
    att = window_attention64(qkv.to(torch.bfloat16), table, I, H, shift).to(torch.bfloat16)
    x1, _ = emulate_linear_mx(att, wproj, bias=bproj, residual=x, row_scale=sc, rows_per_scale=H * H)
    return {"ln1": ln, "qkv": qkv, "att": att, "x1": x1}


def gauss_case(I, H, seed):
    """_case of tests/test_gpu_swin_attn_block.py (N(0, 1) rows, weights of the usual 1 / sqrt(K) size), restated so that this file needs no GPU module"""
    g = torch.Generator().manual_seed(seed)
    M = I * H * H
    return {
        "x": (torch.randn(M, C, generator=g) * 1.5 + 0.2).to(torch.bfloat16),
        "lg": 1 + 0.1 * torch.randn(C, generator=g), "lb": 0.1 * torch.randn(C, generator=g),
        "wqkv": torch.randn(3 * C, C, generator=g) / C ** 0.5, "bqkv": 0.1 * torch.randn(3 * C, generator=g),
        "table": 0.5 * torch.randn(169, HEADS, generator=g),
        "wproj": torch.randn(C, C, generator=g) / C ** 0.5, "bproj": 0.1 * torch.randn(C, generator=g),
    }


def test_gauss_case_is_the_existing_tests_case():
    spec = re.search(r"def _case\(I, H, seed\):\n(.*?)\n    return p\n", open(os.path.join(HERE, "test_gpu_swin_attn_block.py")).read(), flags=re.S).group(1)
    for piece in ("torch.randn(M, C, generator=g) * 1.5 + 0.2", '"lg": 1 + 0.1 * torch.randn(C, generator=g), "lb": 0.1 * torch.randn(C, generator=g)',
                  '"wqkv": torch.randn(3 * C, C, generator=g) / C ** 0.5, "bqkv": 0.1 * torch.randn(3 * C, generator=g)',
                  '"table": 0.5 * torch.randn(169, HEADS, generator=g)', '"wproj": torch.randn(C, C, generator=g) / C ** 0.5, "bproj": 0.1 * torch.randn(C, generator=g)'):
        assert piece in spec, piece


@pytest.mark.parametrize("shift", [0, 3])
def test_emulation_is_the_composition_of_the_mx_helpers(shift):
    I, H = 2, 14
    c = gauss_case(I, H, 5 + shift)
    sc = torch.tensor([0.0, 1.0 / 0.9])
    out = emulate_swin_attn_block_mx(**c, I=I, H=H, shift=shift, sc=sc)
    ln = layernorm_bf16(c["x"], c["lg"], c["lb"], 1e-5)
    assert torch.equal(out["ln1"], ln)
    lq, ls = mx_quant_rows(ln)
    assert lq.shape == (I * H * H, 128) and ls.shape == (I * H * H, 4)
    assert int(lq[:, 96:].max()) == 0 and bool((ls[:, 3] == 127).all())                            # Kp = 128: zero bytes, block 3 carries byte 127
    wq, ws = mx_quant_rows(c["wqkv"])
    qkv = mx_dequant(lq, ls) @ mx_dequant(wq, ws).T + c["bqkv"].double()
    assert torch.equal(out["qkv"], qkv)
    att = window_attention64(qkv.to(torch.bfloat16), c["table"], I, H, shift).to(torch.bfloat16)
    assert torch.equal(out["att"], att)
    aq, as_ = mx_quant_rows(att)
    assert aq.shape == (I * H * H, 128) and as_.shape == (I * H * H, 4)                            # one block per head, block 3 padding
    pq, ps = mx_quant_rows(c["wproj"])
    val = mx_dequant(aq, as_) @ mx_dequant(pq, ps).T + c["bproj"].double()
    assert torch.equal(out["x1"], c["x"].double() + sc.double().repeat_interleave(H * H)[:, None] * val)
    # the window attention is the existing test's reference: on its fp64 qkv it reproduces that reference's att
    sys.path.insert(0, HERE)
    import test_gpu_swin_attn_block as ref_mod
    p = {k: (v.float() if k == "x" else v) for k, v in c.items()}
    ref = ref_mod._reference(p, I, H, shift, sc)
    assert torch.allclose(window_attention64(ref["qkv"].double(), c["table"], I, H, shift).float(), ref["att"], rtol=1e-5, atol=1e-6)


# ---- the exact case -------------------------------------------------------------------------------------------------------------------
def exact_case(I, H, seed=0):
    """A case every stored value of which is a small integer, so that the MX recipe, bf16 products and plain integer arithmetic agree bit for bit
    and any wrong lane, block, row permutation or scale byte changes the result.
      x           rows in {+-1}^96 with zero sum, differing per token: mean = 0 and variance = 1 exactly.
      LayerNorm   gamma = a 2^e[block], beta = b 2^e[block]; 1 <= |a| <= 7, |b| <= 7, |a| != |b|, e a permutation of 0, 1, 2.  rstd = 1 - 5e-6, so
                  LN(x) rounds to (+-a + b) 2^e in bf16: |n| <= 14, <= 4 significant bits.  One channel per block has (|a|, |b|) = (11, 3): |n| is 8
                  or 14 there, so the block maximum lies in [8, 14] 2^e for EVERY token and the scale byte is 127 + e - 5: non-unit, all differ.
      qkv         q / k rows: one or two entries +-1 / +-2, integer biases |b| <= 8: integers below 256, exact in bf16.  v rows of head h: ONE entry +-1
                  at a channel of LN block h, bias c 2^e[h] with |c| <= 1 and |n| + |c| <= 14; one v row per head reads the (11, 3) channel with c = 0:
                  v keeps <= 4 significant bits and the three head blocks of att have the three non-unit scale bytes.
      attention   the bias table is 0 at the self offset (index 84) and -30000 elsewhere; max |q . k| 32^-0.5 <= 10000 is asserted: P is exactly
                  one-hot in fp32 (shift mask or not) and att == v.
      proj        one or two entries, +-1 anywhere and +-2 only at channels of the head whose e = 0; integer biases |b| <= 4; row_scale in
                  {1/2, 1, 2} per image: |x1| < 256 in steps of 1/2 - asserted exact in bf16.
    Returns the case (emulate_swin_attn_block_mx's tensor arguments), sc [I] and the integer reference {ln1, qkv, att, x1} in fp64."""
    g = torch.Generator().manual_seed(4100 + 17 * I + H + seed)
    M = I * H * H
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g)   # noqa: E731
    sign = lambda *shape: (2 * ri(0, 1, *shape) - 1).double()                   # noqa: E731
    x = torch.stack([torch.cat([torch.ones(48), -torch.ones(48)])[torch.randperm(96, generator=g)] for _ in range(M)]).double()
    a = ri(1, 7, C).double() * sign(C)
    b = ri(0, 7, C).double() * sign(C)
    clash = a.abs() == b.abs()
    b[clash] = 0.0
    special = torch.arange(3) * 32 + ri(0, 31, 3)
    a[special] = 11.0 * sign(3)
    b[special] = 3.0 * sign(3)
    eb = torch.randperm(3, generator=g)                                         # block exponents
    e = (2.0 ** eb.double()).repeat_interleave(32)
    lg, lb = a * e, b * e
    ln = x * lg + lb

    def rows(n, lo_ch, hi_ch, two, weights):
        W = torch.zeros(n, C, dtype=torch.float64)
        c1 = ri(lo_ch, hi_ch, n)
        W[torch.arange(n), c1] = weights[ri(0, len(weights) - 1, n)]
        if two:
            c2 = (c1 - lo_ch + ri(1, hi_ch - lo_ch, n)) % (hi_ch - lo_ch + 1) + lo_ch
            second = ri(0, 1, n).bool()
            W[torch.arange(n)[second], c2[second]] = weights[ri(0, len(weights) - 1, int(second.sum()))]
        return W, c1

    w12 = torch.tensor([1.0, -1.0, 2.0, -2.0], dtype=torch.float64)
    w1 = torch.tensor([1.0, -1.0], dtype=torch.float64)
    Wqk, _ = rows(2 * C, 0, C - 1, True, w12)
    bqk = ri(-8, 8, 2 * C).double()
    Wv, bv = torch.zeros(C, C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for h in range(HEADS):
        Wh, ch = rows(HD, 32 * h, 32 * h + 31, False, w1)
        j = int(ri(0, HD - 1, 1))
        Wh[j] = 0.0
        Wh[j, special[h]] = float(sign(1))
        ch[j] = special[h]
        room = (a[ch].abs() + b[ch].abs()) <= 13
        Wv[32 * h:32 * h + 32] = Wh
        bv[32 * h:32 * h + 32] = torch.where(room, ri(-1, 1, HD).double(), torch.zeros(HD, dtype=torch.float64)) * e[ch]
    wqkv, bqkv = torch.cat([Wqk, Wv]), torch.cat([bqk, bv])
    qkv = ln @ wqkv.T + bqkv
    att = qkv[:, 2 * C:]
    unit_head = int(torch.argmin(eb))                                           # the head whose block exponent is 0
    wproj = torch.zeros(C, C, dtype=torch.float64)
    for r in range(C):
        for _ in range(int(ri(1, 2, 1))):
            ch = int(ri(0, C - 1, 1))
            wproj[r, ch] = float(w12[int(ri(0, 3, 1))]) if ch // 32 == unit_head else float(w1[int(ri(0, 1, 1))])
    bproj = ri(-4, 4, C).double()
    sc = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[ri(0, 2, I)]
    table = torch.full((169, HEADS), -30000.0)
    table[84] = 0.0
    x1 = x + sc.repeat_interleave(H * H)[:, None] * (att @ wproj.T + bproj)
    case = dict(x=x.to(torch.bfloat16), lg=lg.float(), lb=lb.float(), wqkv=wqkv.float(), bqkv=bqkv.float(), table=table, wproj=wproj.float(),
                bproj=bproj.float())
    return case, sc.float(), {"ln1": ln, "qkv": qkv, "att": att, "x1": x1}


def _bf16_exact(t):
    return torch.equal(t.to(torch.bfloat16).double(), t.double())


@pytest.mark.parametrize("I,H,shift", [(2, 14, 0), (3, 14, 3), (5, 7, 0), (1, 28, 3), (58, 21, 3)])
def test_exact_case_invariants(I, H, shift):
    from oracle.model import rel_pos_index
    assert bool((rel_pos_index(7).diagonal() == 84).all())                                          # the self offset
    c, sc, ref = exact_case(I, H)
    M = I * H * H
    assert bool((c["x"].double().abs() == 1).all()) and bool((c["x"].double().sum(dim=1) == 0).all())
    assert len({tuple(r) for r in c["x"].double().tolist()}) > M // 2                               # rows differ per token
    assert bool((c["lg"].abs() != c["lb"].abs()).all())
    ln = layernorm_bf16(c["x"], c["lg"], c["lb"], 1e-5)
    assert torch.equal(ln.double(), ref["ln1"])                                                     # LN(x) = +-gamma + beta after the bf16 rounding
    v = ref["att"]
    assert _sig_bits_le4(ref["ln1"]) and _sig_bits_le4(v)
    assert _bf16_exact(ref["qkv"]) and _bf16_exact(ref["x1"]) and float(ref["x1"].abs().max()) < 256
    for name, t in (("LN", ln), ("att", v.to(torch.bfloat16))):
        _, s = mx_quant_rows(t)
        triples = {tuple(r) for r in s[:, :3].tolist()}
        assert len(triples) == 1, (name, triples)                                                   # the same bytes for every token ...
        sb = next(iter(triples))
        assert 127 not in sb and len(set(sb)) == 3, (name, sb)                                      # ... non-unit and all differ
        assert bool((s[:, 3] == 127).all())
    nz = (c["wqkv"] != 0).sum(dim=1)
    assert bool(((nz >= 1) & (nz <= 2)).all()) and bool(((c["wproj"] != 0).sum(dim=1) >= 1).all()) and bool(((c["wproj"] != 0).sum(dim=1) <= 2).all())
    assert set(c["wqkv"].abs().unique().tolist()) <= {0.0, 1.0, 2.0} and set(sc.tolist()) <= {0.5, 1.0, 2.0}
    assert bool((c["table"][84] == 0).all()) and bool((c["table"][torch.arange(169) != 84] == -30000).all())
    qkv = ref["qkv"].view(I, H * H, 3, HEADS, HD)
    # the largest |q . k| over ALL token pairs of an image bounds every window, shifted or not
    worst = max(float((qkv[i, :, 0, h] @ qkv[i, :, 1, h].T).abs().max()) for i in range(I) for h in range(HEADS))
    assert worst * HD ** -0.5 <= 10000, worst
    out = emulate_swin_attn_block_mx(**c, I=I, H=H, shift=shift, sc=sc)
    for k in ("ln1", "qkv", "att", "x1"):
        assert torch.equal(out[k].double(), ref[k]), k                                              # the emulation IS integer arithmetic here
    assert torch.equal(out["att"].double(), ref["qkv"][:, 2 * C:])                                  # P is one-hot: att == v


# ---- the pack image ---------------------------------------------------------------------------------------------------------------------
def attn_block_pack_row(T, r):
    """output column (0 .. 287 of qkv.weight, 288 + 0 .. 95 of proj.weight) of MFMA row r of tile T: chunk T >> 1, half T & 1"""
    return 32 * (T >> 1) + 8 * (r >> 2) + 4 * (T & 1) + (r & 3)


def attn_block_pack_image(wqkv_q, wqkv_s, wproj_q, wproj_s):
    """The image the header comment of swin_attn_block_fwd_mx_kernel documents, gathered on the CPU: data [24 tiles][2 halves][64 lanes][16] and
    scales [24][64]; lane (r, lg) has lane index 16 lg + r, its half hf is the 16 bytes k = 64 hf + 16 lg .. + 15 of row attn_block_pack_row(T, r),
    its scale byte that row's block lg.  Tiles 0 - 17: qkv.weight, 18 - 23: proj.weight."""
    assert wqkv_q.shape == (288, 128) and wqkv_s.shape == (288, 4) and wproj_q.shape == (96, 128) and wproj_s.shape == (96, 4)
    q, s = torch.cat([wqkv_q, wproj_q]), torch.cat([wqkv_s, wproj_s])
    T, r = torch.arange(24)[:, None], torch.arange(16)[None, :]
    n = attn_block_pack_row(T, r)                                                                   # [24][16]
    data = q.reshape(384, 2, 4, 16)[n]                                                              # [T][r][hf][lg][16]
    return data.permute(0, 2, 3, 1, 4).reshape(24, 2, 64, 16), s[n].permute(0, 2, 1).reshape(24, 64)


def attn_block_pack_bytes(wqkv_q, wqkv_s, wproj_q, wproj_s):
    d, s = attn_block_pack_image(wqkv_q, wqkv_s, wproj_q, wproj_s)
    return torch.cat([d.flatten(), s.flatten()])


def test_pack_image_is_a_permutation_in_fragment_order():
    qa = torch.arange(384 * 128, dtype=torch.int32).reshape(384, 128)
    sa = torch.arange(384 * 4, dtype=torch.int32).reshape(384, 4)
    d, s = attn_block_pack_image(qa[:288], sa[:288], qa[288:], sa[288:])
    assert sorted(d.flatten().tolist()) == list(range(384 * 128)) and sorted(s.flatten().tolist()) == list(range(384 * 4))
    # lane (r = 6, lg = 2) of tile 7 (chunk 3, half 1), upper half: column 96 + 8 + 4 + 2 = 110, k = 64 + 32 ..; scale block 2
    assert d[7, 1, 32 + 6].tolist() == qa[110, 96:112].tolist() and int(s[7, 32 + 6]) == int(sa[110, 2])
    assert d[18, 0, 0].tolist() == qa[288, 0:16].tolist()                                           # the first proj tile starts at proj row 0
    # accumulator rows 4 lg .. + 3 of the two tiles of chunk ck are the 8 CONSECUTIVE columns 32 ck + 8 lg .. + 7: 16-byte stores of qkv, att, x1
    for ck in range(12):
        for lg in range(4):
            cols = [int(d[2 * ck + hf, 0, 4 * lg + j, 0]) // 128 for hf in range(2) for j in range(4)]
            assert cols == list(range(32 * ck + 8 * lg, 32 * ck + 8 * lg + 8)), (ck, lg, cols)
    # a lane's bytes: k = 16 lg .. + 15 and 64 + 16 lg .. + 15 (the B-operand lane map of DESIGN 4i / 4m)
    for lg in range(4):
        assert [int(v) % 128 for v in d[0, 0, 16 * lg]] == list(range(16 * lg, 16 * lg + 16))
        assert [int(v) % 128 for v in d[0, 1, 16 * lg]] == list(range(64 + 16 * lg, 64 + 16 * lg + 16))


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("sv_swin_attn_block_mx_supported", "sv_swin_attn_block_mx_pack_bytes", "sv_swin_attn_block_mx_pack", "sv_swin_attn_block_fwd_mx",
           "sv_swin_attn_block_mx_launches")
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
    assert lib.sv_swin_attn_block_mx_launches() >= 0
    assert [lib.sv_swin_attn_block_mx_supported(c, h) for c, h in ((96, 3), (128, 4), (192, 6), (96, 4), (96, 6), (0, 0))] == [1, 0, 0, 0, 0, 0]
    # 288 + 96 rows padded to Kp = 128, one E8M0 byte per 32 elements
    assert lib.sv_swin_attn_block_mx_pack_bytes(96) == 384 * 128 + 384 * 4
    assert lib.sv_swin_attn_block_mx_pack_bytes(128) == 0 and lib.sv_swin_attn_block_mx_pack_bytes(192) == 0
    # the arguments of sv_swin_attn_block_fwd with ONE pack pointer in place of the two weight pointers
    assert len(hip._argtypes("sv_swin_attn_block_fwd_mx")) == len(hip._argtypes("sv_swin_attn_block_fwd")) - 1 == 23
    assert hip._argtypes("sv_swin_attn_block_fwd_mx")[14:] == hip._argtypes("sv_swin_attn_block_fwd")[15:]
    assert "sv_swin_attn_block_fwd_mx" in hip._ACT_TYPED and len(hip._argtypes("sv_swin_attn_block_mx_pack")) == 7


# fake, suitably aligned device addresses: every call below is refused before anything could read them
X, LG, LB, PK, BQ, TB, BP, RS, X1, LN1, MEAN, RSTD, QKV, ATT, WQQ, WQS, WPQ, WPS, WQ, WP = (0x10000 * (i + 1) for i in range(20))
FWD = dict(x=X, g=LG, b=LB, packs=PK, bq=BQ, table=TB, bp=BP, rs=RS, x1=X1, ln1=LN1, mean=MEAN, rstd=RSTD, qkv=QKV, att=ATT,
           I=2, H=14, W=14, C=96, heads=3, shift=3, act=hip.BF16)


def _fwd_mx(lib, a):
    return lib.sv_swin_attn_block_fwd_mx(a["x"], a["g"], a["b"], a["packs"], a["bq"], a["table"], a["bp"], a["rs"], a["x1"], a["ln1"], a["mean"],
                                         a["rstd"], a["qkv"], a["att"], a["I"], a["H"], a["W"], a["C"], a["heads"], a["shift"], 1e-5, a["act"], None)


@pytest.mark.parametrize("what,over", [
    ("x null", dict(x=None)),
    ("ln_g null", dict(g=None)),
    ("ln_b null", dict(b=None)),
    ("packs null", dict(packs=None)),
    ("bqkv null", dict(bq=None)),
    ("table null", dict(table=None)),
    ("bproj null", dict(bp=None)),
    ("x1 null", dict(x1=None)),
    ("I = 0", dict(I=0)),
    ("I < 0", dict(I=-2)),
    ("C = 128, 4 heads", dict(C=128, heads=4)),
    ("C = 192, 6 heads", dict(C=192, heads=6)),
    ("C = 96, 6 heads", dict(heads=6)),
    ("fp32 token rows", dict(act=hip.F32)),
    ("H not a multiple of 7", dict(H=15)),
    ("W not a multiple of 7", dict(W=20)),
    ("H = 0", dict(H=0)),
    ("shift = 7", dict(shift=7)),
    ("shift < 0", dict(shift=-1)),
    ("only ln1", dict(mean=None, rstd=None, qkv=None, att=None)),
    ("ln1 missing", dict(ln1=None)),
    ("mean missing", dict(mean=None)),
    ("rstd missing", dict(rstd=None)),
    ("qkv missing", dict(qkv=None)),
    ("att missing", dict(att=None)),
    ("x misaligned", dict(x=X + 8)),
    ("x1 misaligned", dict(x1=X1 + 2)),
    ("packs misaligned", dict(packs=PK + 4)),
    ("ln1 misaligned", dict(ln1=LN1 + 8)),
    ("qkv misaligned", dict(qkv=QKV + 2)),
    ("att misaligned", dict(att=ATT + 4)),
])
def test_forward_refusals_before_any_gpu_call(what, over):
    lib = hip.load()
    a = dict(FWD)
    a.update(over)
    n0 = lib.sv_swin_attn_block_mx_launches()
    rc = _fwd_mx(lib, a)
    assert rc == SV_ERR_INVALID, (what, rc)
    assert "sv_swin_attn_block_fwd_mx" in lib.sv_last_error().decode(), (what, lib.sv_last_error())
    assert lib.sv_swin_attn_block_mx_launches() == n0, what


@pytest.mark.parametrize("what,over", [
    ("wqkv_q null", dict(wqq=None)),
    ("wqkv_s null", dict(wqs=None)),
    ("wproj_q null", dict(wpq=None)),
    ("wproj_s null", dict(wps=None)),
    ("packs null", dict(packs=None)),
    ("C = 128", dict(C=128)),
    ("C = 0", dict(C=0)),
    ("wqkv_q misaligned", dict(wqq=WQQ + 4)),
    ("wproj_q misaligned", dict(wpq=WPQ + 8)),
    ("packs misaligned", dict(packs=PK + 1)),
])
def test_pack_refusals_before_any_gpu_call(what, over):
    lib = hip.load()
    a = dict(wqq=WQQ, wqs=WQS, wpq=WPQ, wps=WPS, packs=PK, C=96)
    a.update(over)
    rc = lib.sv_swin_attn_block_mx_pack(a["wqq"], a["wqs"], a["wpq"], a["wps"], a["packs"], a["C"], None)
    assert rc == SV_ERR_INVALID, (what, rc)
    assert "sv_swin_attn_block_mx_pack" in lib.sv_last_error().decode(), (what, lib.sv_last_error())


@pytest.mark.parametrize("what,over", [
    ("wqkv null", dict(wq=None)),
    ("wproj null", dict(wp=None)),
    ("x null", dict(x=None)),
    ("I = 0", dict(I=0)),
    ("C = 192, 6 heads", dict(C=192, heads=6)),
    ("fp32 token rows", dict(act=hip.F32)),
    ("H not a multiple of 7", dict(H=15)),
    ("shift = 7", dict(shift=7)),
    ("partial side outputs", dict(mean=None)),
    ("wqkv misaligned", dict(wq=WQ + 4)),
    ("wproj misaligned", dict(wp=WP + 8)),
    ("x1 misaligned", dict(x1=X1 + 2)),
])
def test_existing_entry_keeps_its_refusals(what, over):
    lib = hip.load()
    a = dict(FWD, wq=WQ, wp=WP)
    a.update(over)
    rc = lib.sv_swin_attn_block_fwd(a["x"], a["g"], a["b"], a["wq"], a["bq"], a["table"], a["wp"], a["bp"], a["rs"], a["x1"], a["ln1"], a["mean"],
                                    a["rstd"], a["qkv"], a["att"], a["I"], a["H"], a["W"], a["C"], a["heads"], a["shift"], 1e-5, a["act"], None)
    assert rc == SV_ERR_INVALID, (what, rc)
    assert "swin_attn_block_fwd" in lib.sv_last_error().decode() and "_mx" not in lib.sv_last_error().decode(), (what, lib.sv_last_error())


def test_both_entries_share_one_launch_geometry():
    lib = hip.load()
    assert lib.sv_swin_attn_block_windows_per_group(58, 21, 21, 0) >= 2 and lib.sv_swin_attn_block_windows_per_group(2, 14, 14, 0) == 1


# ---- the host switch --------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _mx_mode():
    """bf16 math + storage, set_linear_fp8(True, recipe="mx"), the new switch ON; every switch and the environment restored on exit"""
    import make_swin_host_trace as gen
    from swinvox_amd import ops
    with gen.recording() as rec:
        env = os.environ.pop("SV_FUSED_ATTN_BLOCK_MX", None)
        try:
            gen._apply(dict(gen.DEFAULTS, fp8=True, recipe="mx"))
            ops.set_fused_attn_block_mx(True)
            yield rec
        finally:
            if env is not None:
                os.environ["SV_FUSED_ATTN_BLOCK_MX"] = env


def test_switch_is_off_by_default(monkeypatch):
    from swinvox_amd import ops
    monkeypatch.delenv("SV_FUSED_ATTN_BLOCK_MX", raising=False)
    assert not ops._STATE.get("fused_attn_block_mx", False)
    assert not ops.fused_attn_block_mx_enabled(96, 3)
    import make_swin_host_trace as gen
    with gen.recording():
        gen._apply(dict(gen.DEFAULTS, fp8=True, recipe="mx"))
        assert ops.fused_attn_block_enabled(96, 3) and not ops.fused_attn_block_mx_enabled(96, 3)   # everything but the switch
    assert "SV_FUSED_ATTN_BLOCK_MX" in open(os.path.join(ROOT, "README.md")).read()


def test_switch_is_inert_under_each_condition(monkeypatch):
    from swinvox_amd import ops
    monkeypatch.delenv("SV_FUSED_ATTN_BLOCK_MX", raising=False)
    with _mx_mode():
        assert ops.fused_attn_block_mx_enabled(96, 3)
        assert not ops.fused_attn_block_mx_enabled(128, 4) and not ops.fused_attn_block_mx_enabled(192, 6) and not ops.fused_attn_block_mx_enabled(96, 6)
        ops.set_fused_attn_block(False)
        assert not ops.fused_attn_block_mx_enabled(96, 3)
        ops.set_fused_attn_block(True)
        ops.set_attention_fp8(True)
        assert not ops.fused_attn_block_mx_enabled(96, 3)
        ops.set_attention_fp8(False)
        ops.set_linear_fp8(True)                                                # the row recipe
        assert not ops.fused_attn_block_mx_enabled(96, 3)
        ops.set_linear_fp8(False)
        assert not ops.fused_attn_block_mx_enabled(96, 3)
        ops.set_linear_fp8(True, recipe="mx")
        assert ops.fused_attn_block_mx_enabled(96, 3)
        ops.set_math("f32")
        assert not ops.fused_attn_block_mx_enabled(96, 3)
        ops.set_math("bf16")
        assert not ops.fused_attn_block_mx_enabled(96, 3)                       # f32 math took the storage to f32
        ops.set_storage("bf16")
        assert ops.fused_attn_block_mx_enabled(96, 3)
        ops.set_fused_attn_block_mx(False)
        assert not ops.fused_attn_block_mx_enabled(96, 3)
        monkeypatch.setenv("SV_FUSED_ATTN_BLOCK_MX", "1")                       # the environment switches it on as well
        assert ops.fused_attn_block_mx_enabled(96, 3)
        monkeypatch.delenv("SV_FUSED_ATTN_BLOCK_MX")
    assert not ops.fused_attn_block_mx_enabled(96, 3)


def _trace(shape, settings, mx_switch, backward=True):
    """the calls one block issues (forward, and backward when the case saves) under make_swin_host_trace's settings + the new switch"""
    import itertools

    import make_swin_host_trace as gen
    from swinvox_amd import ops
    from swinvox_amd.models import swin_transformer as st
    Cd, heads, res = gen.SHAPES[shape]
    torch.manual_seed(0)
    blk = st.SwinBlock(Cd, res, heads, 3, 0.0)
    s = dict(gen.DEFAULTS, **settings)
    with gen.recording() as rec:
        gen._apply(s)
        ops.set_fused_attn_block_mx(mx_switch)
        rec.reset()
        grads = {p: torch.zeros_like(p) for p in blk.parameters()}
        x = ops.empty(res * res, Cd, device="cpu")
        y, tape = st.block_forward(blk, x, 1, False, False, itertools.count(1000).__next__, s["save"])
        n_fwd = len(rec.calls)
        if s["save"] and backward:
            st.block_backward(blk, tape, ops.empty(*y.shape, device="cpu"), grads)
        return [list(c) for c in rec.calls], n_fwd, tape


@pytest.mark.parametrize("save", [True, False])
def test_host_trace_with_the_switch_on(monkeypatch, save):
    monkeypatch.delenv("SV_FUSED_ATTN_BLOCK_MX", raising=False)
    mx = dict(fp8=True, recipe="mx", save=save)
    off, n_off, tape_off = _trace("c96", mx, False)
    on, n_on, tape_on = _trace("c96", mx, True)
    names_on, names_off = [c[0] for c in on], [c[0] for c in off]
    assert names_off.count("sv_swin_attn_block_fwd") == 1 and "sv_swin_attn_block_fwd_mx" not in names_off and "sv_swin_attn_block_mx_pack" not in names_off
    assert names_on.count("sv_swin_attn_block_fwd_mx") == 1 and names_on.count("sv_swin_attn_block_mx_pack") == 1
    assert "sv_swin_attn_block_fwd" not in names_on
    # everything else is the switch-off trace, call for call (names: the pointers are numbered by first appearance)
    rest = [n for n in names_on if n not in ("sv_swin_attn_block_fwd_mx", "sv_swin_attn_block_mx_pack", "sv_quant_rows_mx_e4m3")]
    assert rest == [n for n in names_off if n not in ("sv_swin_attn_block_fwd", "sv_quant_rows_mx_e4m3")]
    i_fwd, i_pack = names_on.index("sv_swin_attn_block_fwd_mx"), names_on.index("sv_swin_attn_block_mx_pack")
    assert i_pack < i_fwd < n_on
    fwd, pack, old = on[i_fwd], on[i_pack], off[names_off.index("sv_swin_attn_block_fwd")]
    # the pack reads the MX rows of qkv.weight and proj.weight ([288, 96] and [96, 96] fp32, K = 96 -> Kp = 128), in that order
    quants = [c for c in on[:i_pack] if c[0] == "sv_quant_rows_mx_e4m3"]
    wq, wp = [c for c in quants if c[3:6] == [288, 96, 96]], [c for c in quants if c[3:6] == [96, 96, 96]]
    assert len(wq) == 1 and len(wp) == 1 and wq[0][2] == wp[0][2] == hip.F32 and wq[0][7] == wp[0][7] == 128
    assert pack[1:5] == [wq[0][6], wq[0][8], wp[0][6], wp[0][8]] and pack[6] == 96 and pack[5] not in (None, wq[0][6], wp[0][6])
    # the forward: the pack in place of the two weights, everything else wired as sv_swin_attn_block_fwd wires it
    assert fwd[4] == pack[5]
    assert len(fwd) == len(old) - 1 and fwd[15:] == old[16:]                                        # I, H, W, C, heads, shift, eps, act, booked work
    assert [v is None for v in fwd[8:15]] == [v is None for v in old[9:16]] == [True, False] + [not save] * 5
    assert len({v for v in fwd[1:15] if v is not None}) == len([v for v in fwd[1:15] if v is not None])   # distinct buffers
    mlp = next(c for c in on[i_fwd + 1:] if c[0] in ("sv_swin_mlp_fwd", "sv_swin_mlp_fwd_mx"))
    assert mlp[1] == fwd[9]                                                                          # x1 feeds the MLP branch
    # the tape fields are unchanged
    assert type(tape_on) is type(tape_off) and tape_on._fields == tape_off._fields
    assert [v is None for v in tape_on] == [v is None for v in tape_off]
    for f in ("ln1", "qkv", "att", "m1", "r1", "x1"):
        a, b = getattr(tape_on, f), getattr(tape_off, f)
        assert (a is None) == (b is None) and (a is None or (a.dtype, a.shape) == (b.dtype, b.shape)), f
    if save:
        bwd = next(c for c in on[n_on:] if c[0] == "sv_swin_attn_block_bwd")
        assert bwd[2] == fwd[13] and bwd[3] == fwd[1] and bwd[4] == fwd[11] and bwd[5] == fwd[12]    # qkv, x, mean, rstd as stored


INERT = [
    ("row recipe", "c96", dict(fp8=True, recipe="row")),
    ("fp8 linears off", "c96", dict()),
    ("f32 math", "c96", dict(math="f32", fp8=True, recipe="mx")),
    ("fp8 attention", "c96", dict(fp8=True, recipe="mx", attn8=1)),
    ("unfused", "c96", dict(fp8=True, recipe="mx", fused=False)),
    ("C = 192", "c192", dict(fp8=True, recipe="mx")),
    ("store mx keeps the bf16 tape", "c96", dict(fp8=True, recipe="mx", bwd=True, brec="mx", store="mx")),
]


@pytest.mark.parametrize("what,shape,settings", INERT[:-1])
def test_host_trace_is_the_switch_off_trace_where_inert(monkeypatch, what, shape, settings):
    monkeypatch.delenv("SV_FUSED_ATTN_BLOCK_MX", raising=False)
    off, _, _ = _trace(shape, settings, False)
    on, _, _ = _trace(shape, settings, True)
    assert on == off, what
    assert "sv_swin_attn_block_fwd_mx" not in [c[0] for c in on]


def test_tape_stays_bf16_under_store_mx(monkeypatch):
    monkeypatch.delenv("SV_FUSED_ATTN_BLOCK_MX", raising=False)
    _, _, settings = INERT[-1]
    on, _, tape = _trace("c96", settings, True)
    assert "sv_swin_attn_block_fwd_mx" in [c[0] for c in on]
    for f in ("ln1", "qkv", "att"):
        assert isinstance(getattr(tape, f), torch.Tensor) and getattr(tape, f).dtype == torch.bfloat16, f
