"""Window attention that emits the MX operand rows of the proj linear (csrc/attn.hip, sv_window_attention_fwd_mxq).

The emitting instantiations of the two workgroup kernels (bf16 and fp8 math) must store the `out` of sv_window_attention_fwd bit for bit, and
their q_out / qs_out must equal the stand-alone MX quantiser (sv_quant_rows_mx_e4m3, which tests/test_gpu_linear_mxfp8.py ties to the
emulation) on that stored `out` bit for bit - padding bytes and padding scales included, which the kernel writes itself (C = 96 -> Kp 128,
C = 192 -> Kp 256): the buffers are poisoned beforehand.  The shapes are those of tests/test_gpu_window_attention_shares.py - several
windows per workgroup with a ragged last run - plus C = 192 with 6 heads."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from swinvox_amd import hip  # noqa: E402
from swinvox_amd.hip import call, ptr  # noqa: E402

GUARD = 2
#         I, H, heads: 1377, 513 and 130 windows at 3, 8 and 32 heads; 810 windows at 6 heads (C = 192)
CASES = {"A": (153, 21, 3), "B": (57, 21, 8), "C": (130, 7, 32), "D": (90, 21, 6)}


@pytest.fixture(scope="module", params=list(CASES))
def case(request, dev):
    I, H, heads = CASES[request.param]
    g = torch.Generator().manual_seed(4000 + 10 * I + heads)
    qkv = torch.randn(I * H * H, 3 * heads * 32, generator=g).bfloat16().float()
    # head h of every token is scaled by 2^(h mod 5 - 2) times a token factor: the block scales differ from head to head and token to token
    v = qkv[:, 2 * heads * 32:].view(-1, heads, 32)
    v *= torch.exp2((torch.arange(heads) % 5 - 2).float())[None, :, None] * torch.exp2(torch.randint(-3, 4, (v.shape[0], 1, 1), generator=g).float())
    table = 0.5 * torch.randn(169, heads, generator=g)
    d = {"f32": qkv.to(dev)}
    d["bf16"] = d["f32"].bfloat16()
    yield request.param, d, table.to(dev)
    d.clear()
    torch.cuda.empty_cache()


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def test_emission_equals_the_quantiser_on_the_stored_output(case, dev):
    name, d, table = case
    I, H, heads = CASES[name]
    for shift in ((0,) if H == 7 else (0, 3)):                             # a one-window map has no shifted form
        _check_case(name, d, table, dev, shift)


def _check_case(name, d, table, dev, shift):
    I, H, heads = CASES[name]
    C, M = heads * 32, I * H * H
    Kp = (C + 127) // 128 * 128
    lib = hip.load()
    for math in (hip.MATH_BF16, hip.MATH_FP8):
        assert lib.sv_window_attention_windows_per_group(I, H, H, heads, math, 0) > 1, (name, math)      # the window loop runs
        for store in ("f32", "bf16"):
            tag = f"{name} shift={shift} math={math} {store}"
            qkv, act = d[store], (hip.BF16 if store == "bf16" else hip.F32)
            ref = torch.full((M, C), float("nan"), dtype=qkv.dtype, device=dev)
            call("sv_window_attention_fwd", ptr(qkv), ptr(table), ptr(ref), I, H, H, C, heads, shift, math, act=act)
            rq = torch.full((M, Kp), 0x7F, dtype=torch.uint8, device=dev)
            rs = torch.full((M, Kp // 32), 0xFF, dtype=torch.uint8, device=dev)
            call("sv_quant_rows_mx_e4m3", ptr(ref), act, M, C, C, ptr(rq), Kp, ptr(rs))
            for with_out in (True, False):
                out = torch.full((M, C), float("nan"), dtype=qkv.dtype, device=dev) if with_out else None
                q = torch.full((M + GUARD, Kp), 0x7F, dtype=torch.uint8, device=dev)
                s = torch.full((M + GUARD, Kp // 32), 0xFF, dtype=torch.uint8, device=dev)
                call("sv_window_attention_fwd_mxq", ptr(qkv), ptr(table), ptr(out), I, H, H, C, heads, shift, math, ptr(q), Kp, ptr(s), act=act)
                torch.cuda.synchronize()
                if with_out:
                    assert torch.equal(_bits(out), _bits(ref)), tag
                assert torch.equal(s[:M], rs), (tag, with_out, int((s[:M] != rs).sum()))
                assert torch.equal(q[:M], rq), (tag, with_out, int((q[:M] != rq).sum()))
                assert bool((q[M:] == 0x7F).all()) and bool((s[M:] == 0xFF).all()), (tag, with_out)
            if Kp > C:
                assert int(rq[:, C:].max()) == 0 and bool((rs[:, C // 32:] == 127).all()), tag
            assert len(torch.unique(rs[:, :heads])) >= 4, tag                                             # the scales are not all one byte
