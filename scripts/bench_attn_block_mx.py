#!/usr/bin/env python3
"""Micro-benchmark of the MXFP8 forward of the fused stage-0 attention branch (sv_swin_attn_block_fwd_mx) against the fused bf16 kernel
(sv_swin_attn_block_fwd) and the unfused MX chain it composes (sv_layernorm_quant_mx_fwd -> sv_linear_mxfp8 -> sv_window_attention_fwd_mxq ->
sv_linear_mxfp8 + residual), each in training form (the five side tensors stored) and inference form, at the shapes of
scripts/bench_attn_block.py: I = 512 images of 56 x 56 tokens, bf16 rows.  The three are timed in turn, three rounds, in one process."""
import ctypes, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import swinvox_amd as S
from swinvox_amd import hip, ops
from swinvox_amd.hip import call, ptr
dev = torch.device("cuda", 0); hip.load(); S.set_math("bf16"); S.set_storage("bf16")
def timeit(fn, iters=10):
    for _ in range(2): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3
I, H, C, heads = int(os.environ.get("SV_ATTN_I", "512")), 56, 96, 3
M = I * H * H
b16, u8 = dict(dtype=torch.bfloat16, device=dev), dict(dtype=torch.uint8, device=dev)
x = torch.randn(M, C, device=dev).bfloat16()
lg, lb = torch.ones(C, device=dev), torch.zeros(C, device=dev)
wq, bq = torch.randn(3 * C, C, device=dev) / C ** 0.5, torch.zeros(3 * C, device=dev)
wp, bp = torch.randn(C, C, device=dev) / C ** 0.5, torch.zeros(C, device=dev)
table = torch.randn(169, heads, device=dev) * 0.1
x1, ln1, qkv, att = torch.empty(M, C, **b16), torch.empty(M, C, **b16), torch.empty(M, 3 * C, **b16), torch.empty(M, C, **b16)
m1, r1 = torch.empty(M, device=dev), torch.empty(M, device=dev)
(wqq, wqs), (wpq, wps) = ops.quantize_rows_mx(wq, 3 * C, C, activation=False), ops.quantize_rows_mx(wp, C, C, activation=False)
packs = torch.empty(int(hip.load().sv_swin_attn_block_mx_pack_bytes(C)), **u8)
call("sv_swin_attn_block_mx_pack", ptr(wqq), ptr(wqs), ptr(wpq), ptr(wps), ptr(packs), C)
lq, ls, aq, as_ = torch.empty(M, 128, **u8), torch.empty(M, 4, **u8), torch.empty(M, 128, **u8), torch.empty(M, 4, **u8)
e_qkv = ops._epilogue(3 * C, bias=bq)
e_proj = ops._epilogue(C, bias=bp, residual=x, ldr=C, rows_per_scale=H * H)
for shift in (0, 3):
    def side(on):
        return [ptr(t) if on else None for t in (ln1, m1, r1, qkv, att)]
    def fused_bf16(on):
        call("sv_swin_attn_block_fwd", ptr(x), ptr(lg), ptr(lb), ptr(wq), ptr(bq), ptr(table), ptr(wp), ptr(bp), None, ptr(x1), *side(on),
             I, H, H, C, heads, shift, 1e-5)
    def fused_mx(on):
        call("sv_swin_attn_block_fwd_mx", ptr(x), ptr(lg), ptr(lb), ptr(packs), ptr(bq), ptr(table), ptr(bp), None, ptr(x1), *side(on),
             I, H, H, C, heads, shift, 1e-5)
    def chain_mx(on):
        call("sv_layernorm_quant_mx_fwd", ptr(x), ptr(lg), ptr(lb), ptr(ln1) if on else None, ptr(m1) if on else None, ptr(r1) if on else None,
             ptr(lq), 128, ptr(ls), M, C, 1e-5, 0, 0)
        call("sv_linear_mxfp8", ptr(lq), ptr(ls), ptr(wqq), ptr(wqs), ptr(qkv), M, C, 3 * C, ctypes.byref(e_qkv), None, None)
        call("sv_window_attention_fwd_mxq", ptr(qkv), ptr(table), ptr(att) if on else None, I, H, H, C, heads, shift, hip.MATH_BF16, ptr(aq), 128, ptr(as_))
        call("sv_linear_mxfp8", ptr(aq), ptr(as_), ptr(wpq), ptr(wps), ptr(x1), M, C, C, ctypes.byref(e_proj), None, None)
    for rnd in range(3):
        for form, on in (("training", True), ("inference", False)):
            t = [timeit(lambda f=f: f(on)) for f in (fused_bf16, fused_mx, chain_mx)]
            print(f"shift={shift} round {rnd} {form:9s}  fused bf16 {t[0]:7.1f} us   fused MX {t[1]:7.1f} us   unfused MX chain {t[2]:7.1f} us   "
                  f"MX / bf16 {t[1] / t[0]:.3f}   MX / chain {t[1] / t[2]:.3f}", flush=True)
