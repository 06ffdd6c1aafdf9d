"""Data gradient of the stage-0 Swin MLP branch at the benchmark shapes (I = 512 images of 56 x 56 tokens, C = 96 and C = 128), three ways:
(a) the fused bf16 kernel (sv_swin_mlp_bwd), (b) the fused MXFP8 kernel (sv_swin_mlp_bwd_mx) and (c) the unfused MX data path it replaces
(sv_rowscale -> sv_quant_rows_mx_e4m3 of dy -> sv_linear_mxfp8_dgrad with GELU' at the stored pre-activation -> sv_quant_rows_mx_e4m3 of dh ->
sv_linear_mxfp8_dgrad -> sv_layernorm_bwd with the residual).  ms per launch (for (c): per chain), algorithmic TFLOP/s over the three products the
fused kernels run (recompute, fc2 and fc1 data gradients; the chain runs two and reads the pre-activation instead).  C = 128 is left out of (b) where
sv_swin_mlp_bwd_mx_supported says no."""
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


def quant_rows(w, dt=hip.F32):
    N, K = w.shape
    Kp = (K + 127) // 128 * 128
    q = torch.empty(N, Kp, dtype=torch.uint8, device=dev)
    s = torch.empty(N, Kp // 32, dtype=torch.uint8, device=dev)
    call("sv_quant_rows_mx_e4m3", ptr(w), dt, N, K, K, ptr(q), Kp, ptr(s))
    return q, s


def quant_cols(w):
    N, K = w.shape
    Np = (N + 127) // 128 * 128
    q = torch.empty(K, Np, dtype=torch.uint8, device=dev)
    s = torch.empty(K, Np // 32, dtype=torch.uint8, device=dev)
    call("sv_quant_cols_mx_e4m3", ptr(w), hip.F32, N, K, K, ptr(q), Np, ptr(s), None)
    return q, s


lib = hip.load()
for C, res in ((96, 56), (128, 56)):
    M, HID = I * res * res, 4 * C
    x = torch.randn(M, C, device=dev).to(torch.bfloat16)
    dy = torch.randn(M, C, device=dev).to(torch.bfloat16)
    dx = torch.empty_like(x)
    w1 = torch.randn(HID, C, device=dev) / C ** 0.5
    w2 = torch.randn(C, HID, device=dev) / HID ** 0.5
    b1, lg, lb = torch.zeros(HID, device=dev), torch.ones(C, device=dev), torch.zeros(C, device=dev)
    dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    sc = torch.full((I,), 1.0 / 0.9, device=dev)
    packs = torch.empty(16 * C * C, dtype=torch.bfloat16, device=dev)
    call("sv_swin_mlp_pack", ptr(w1), ptr(w2), ptr(packs), C)
    (w1q, w1s), (w2tq, w2ts), (w1tq, w1ts) = quant_rows(w1), quant_cols(w2), quant_cols(w1)
    unit = 2.0 * M * C * 4 * C
    a = timeit(lambda: call("sv_swin_mlp_bwd", ptr(x), ptr(dy), ptr(dx), ptr(lg), ptr(lb), ptr(packs), ptr(b1), ptr(sc), res * res, ptr(dg), ptr(db), M, C, 1e-5))
    b = float("nan")
    if lib.sv_swin_mlp_bwd_mx_supported(C) == 1:
        packs_mx = torch.empty(int(lib.sv_swin_mlp_bwd_mx_pack_bytes(C)), dtype=torch.uint8, device=dev)
        call("sv_swin_mlp_bwd_mx_pack", ptr(w1q), ptr(w1s), ptr(w2tq), ptr(w2ts), ptr(w1tq), ptr(w1ts), ptr(packs_mx), C)
        b = timeit(lambda: call("sv_swin_mlp_bwd_mx", ptr(x), ptr(dy), ptr(dx), ptr(lg), ptr(lb), ptr(packs_mx), ptr(b1), ptr(sc), res * res, ptr(dg), ptr(db),
                                M, C, 1e-5))
    # the unfused chain reads what its forward stored: the pre-activation and the LayerNorm statistics
    hpre = torch.randn(M, HID, device=dev).to(torch.bfloat16)
    mean, rstd = torch.zeros(M, device=dev), torch.ones(M, device=dev)
    dbr, dh, dln = torch.empty_like(x), torch.empty(M, HID, dtype=torch.bfloat16, device=dev), torch.empty_like(x)
    dq, ds = torch.empty(M, 128, dtype=torch.uint8, device=dev), torch.empty(M, 4, dtype=torch.uint8, device=dev)
    hq, hs = torch.empty(M, HID, dtype=torch.uint8, device=dev), torch.empty(M, HID // 32, dtype=torch.uint8, device=dev)
    e2 = ops._epilogue(HID, act_grad_src=hpre, act_grad_kind=hip.ACT_GELU)
    e3 = ops._epilogue(C)
    ws = torch.zeros(ops.LN_BWD_SLOTS * C + 1, dtype=torch.float64, device=dev)

    def chain():
        call("sv_rowscale", ptr(dy), ptr(sc), ptr(dbr), M, C, res * res, act=hip.BF16)
        call("sv_quant_rows_mx_e4m3", ptr(dbr), hip.BF16, M, C, C, ptr(dq), 128, ptr(ds))
        call("sv_linear_mxfp8_dgrad", ptr(dq), ptr(ds), ptr(w2tq), ptr(w2ts), ptr(dh), M, C, HID, ctypes.byref(e2), act=hip.BF16)
        call("sv_quant_rows_mx_e4m3", ptr(dh), hip.BF16, M, HID, HID, ptr(hq), HID, ptr(hs))
        call("sv_linear_mxfp8_dgrad", ptr(hq), ptr(hs), ptr(w1tq), ptr(w1ts), ptr(dln), M, HID, C, ctypes.byref(e3), act=hip.BF16)
        ws.zero_()                                         # the workspace is zero on entry (the model takes it from a cleared arena): a 6-KB memset
        call("sv_layernorm_bwd", ptr(dln), ptr(x), ptr(lg), ptr(mean), ptr(rstd), ptr(dx), ptr(dg), ptr(db), ptr(ws), M, C, 0, 0, 1, act=hip.BF16)

    u = timeit(chain)                                      # dx accumulates from launch to launch: the values do not matter to the time
    print(f"C={C:3d} M={M:7d}  (a) fused bf16 {a:6.3f} ms {3 * unit / a / 1e9:6.0f} TF/s | (b) fused MX {b:6.3f} ms {3 * unit / b / 1e9:6.0f} TF/s | "
          f"(c) unfused MX chain {u:6.3f} ms", flush=True)
