"""Forward of the stage-0 Swin MLP branch at the benchmark shapes (I = 512 images of 56 x 56 tokens, C = 96 and C = 128), three ways:
the fused bf16 kernel (sv_swin_mlp_fwd), the fused MXFP8 kernel (sv_swin_mlp_fwd_mx) and the unfused MX chain it replaces
(sv_layernorm_quant_mx_fwd -> sv_linear_mxfp8 with GELU and q_out -> sv_linear_mxfp8 with the residual; no hidden tensor stored, as under
torch.no_grad()).  ms per forward, algorithmic TFLOP/s."""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swinvox_amd import hip, ops  # noqa: E402
from swinvox_amd.hip import call, ptr  # noqa: E402

dev = torch.device("cuda:0")
I = int(sys.argv[1]) if len(sys.argv) > 1 else 512


def timeit(fn, n=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def quant_w(w):
    N, K = w.shape
    Kp = (K + 127) // 128 * 128
    q = torch.empty(N, Kp, dtype=torch.uint8, device=dev)
    s = torch.empty(N, Kp // 32, dtype=torch.uint8, device=dev)
    call("sv_quant_rows_mx_e4m3", ptr(w), hip.F32, N, K, K, ptr(q), Kp, ptr(s))
    return q, s


for C, res in ((96, 56), (128, 56)):
    M, HID = I * res * res, 4 * C
    x = torch.randn(M, C, device=dev).to(torch.bfloat16)
    out = torch.empty_like(x)
    w1 = torch.randn(HID, C, device=dev) / C ** 0.5
    w2 = torch.randn(C, HID, device=dev) / HID ** 0.5
    b1, b2, lg, lb = torch.zeros(HID, device=dev), torch.zeros(C, device=dev), torch.ones(C, device=dev), torch.zeros(C, device=dev)
    packs = torch.empty(16 * C * C, dtype=torch.bfloat16, device=dev)
    call("sv_swin_mlp_pack", ptr(w1), ptr(w2), ptr(packs), C)
    (w1q, w1s), (w2q, w2s) = quant_w(w1), quant_w(w2)
    packs_mx = torch.empty(int(hip.load().sv_swin_mlp_mx_pack_bytes(C)), dtype=torch.uint8, device=dev)
    call("sv_swin_mlp_mx_pack", ptr(w1q), ptr(w1s), ptr(w2q), ptr(w2s), ptr(packs_mx), C)
    q, s = torch.empty(M, 128, dtype=torch.uint8, device=dev), torch.empty(M, 4, dtype=torch.uint8, device=dev)
    hq, hs = torch.empty(M, HID, dtype=torch.uint8, device=dev), torch.empty(M, HID // 32, dtype=torch.uint8, device=dev)
    e1 = ops._epilogue(HID, bias=b1, act=hip.ACT_GELU)
    e2 = ops._epilogue(C, bias=b2, residual=x, ldr=C)

    def chain():
        call("sv_layernorm_quant_mx_fwd", ptr(x), ptr(lg), ptr(lb), None, None, None, ptr(q), 128, ptr(s), M, C, 1e-5, 0, 0, act=hip.BF16)
        call("sv_linear_mxfp8", ptr(q), ptr(s), ptr(w1q), ptr(w1s), None, M, C, HID, ctypes.byref(e1), ptr(hq), ptr(hs), act=hip.BF16)
        call("sv_linear_mxfp8", ptr(hq), ptr(hs), ptr(w2q), ptr(w2s), ptr(out), M, HID, C, ctypes.byref(e2), None, None, act=hip.BF16)

    unit = 2.0 * M * C * 4 * C
    f = timeit(lambda: call("sv_swin_mlp_fwd", ptr(x), ptr(out), ptr(lg), ptr(lb), ptr(packs), ptr(b1), ptr(b2), None, res * res, M, C, 1e-5))
    m = timeit(lambda: call("sv_swin_mlp_fwd_mx", ptr(x), ptr(out), ptr(lg), ptr(lb), ptr(packs_mx), ptr(b1), ptr(b2), None, res * res, M, C, 1e-5))
    u = timeit(chain)
    print(f"C={C:3d} M={M:7d}  fused bf16 {f:6.3f} ms {2 * unit / f / 1e9:6.0f} TF/s | fused MX {m:6.3f} ms {2 * unit / m / 1e9:6.0f} TF/s | "
          f"unfused MX chain {u:6.3f} ms {2 * unit / u / 1e9:6.0f} TF/s", flush=True)
