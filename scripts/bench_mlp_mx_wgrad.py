"""Weight gradients of the stage-0 Swin MLP branch at the benchmark shapes (I = 512 images of 56 x 56 tokens, C = 96 and C = 128, with row_scale),
three ways: (a) the fused bf16 kernel (sv_swin_mlp_wgrad), (b) the fused MXFP8 kernel (sv_swin_mlp_wgrad_mx) and (c) the unfused MX weight-gradient path
it replaces (sv_quant_cols_mx_e4m3 of dbr, h, dh and ln2 with the two column sums, two sv_linear_mxfp8_wgrad with their reduces; the chain reads h, dh
and ln2 that its forward and data gradient stored).  ms per launch (for (c): per chain), algorithmic TFLOP/s over the four products the fused kernels
run (two recomputes, two contractions over the tokens; the chain runs the two contractions).  (b) is left out where sv_swin_mlp_wgrad_mx_supported
says no.  Every run is printed: call the script three times, or pass a repeat count as the second argument."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swinvox_amd import hip  # noqa: E402
from swinvox_amd.hip import call, ptr  # noqa: E402

dev = torch.device("cuda:0")
I = int(sys.argv[1]) if len(sys.argv) > 1 else 512
REPEAT = int(sys.argv[2]) if len(sys.argv) > 2 else 3


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


def col_buffers(rows, cols):
    Mp = (rows + 127) // 128 * 128
    return torch.empty(cols, Mp, dtype=torch.uint8, device=dev), torch.empty(cols, Mp // 32, dtype=torch.uint8, device=dev)


def quant_cols(t, q, s, colsum=None):
    rows, cols = t.shape
    call("sv_quant_cols_mx_e4m3", ptr(t), hip.BF16 if t.dtype == torch.bfloat16 else hip.F32, rows, cols, cols, ptr(q), q.shape[1], ptr(s), ptr(colsum))


lib = hip.load()
for C, res in ((96, 56), (128, 56)):
    M, HID = I * res * res, 4 * C
    x = torch.randn(M, C, device=dev).to(torch.bfloat16)
    dy = torch.randn(M, C, device=dev).to(torch.bfloat16)
    w1 = torch.randn(HID, C, device=dev) / C ** 0.5
    w2 = torch.randn(C, HID, device=dev) / HID ** 0.5
    b1, lg, lb = torch.zeros(HID, device=dev), torch.ones(C, device=dev), torch.zeros(C, device=dev)
    dw1, db1, dw2, db2 = (torch.zeros(n, device=dev) for n in (HID * C, HID, C * HID, C))
    sc = torch.full((I,), 1.0 / 0.9, device=dev)
    w1r, w2tr = w1.bfloat16().contiguous(), w2.t().contiguous().bfloat16()
    (w1q, w1s) = quant_rows(w1)
    w2tq, w2ts = col_buffers(C, HID)
    quant_cols(w2, w2tq, w2ts)
    unit = 2.0 * M * C * 4 * C
    # the unfused chain reads what its forward and data gradient stored: ln2, h, dh (and dbr from sv_rowscale)
    ln = torch.randn(M, C, device=dev).to(torch.bfloat16)
    h = torch.randn(M, HID, device=dev).to(torch.bfloat16)
    dh = torch.randn(M, HID, device=dev).to(torch.bfloat16)
    (dbt, dbs), (lnt, lns), (ht, hs), (dht, dhs) = col_buffers(M, C), col_buffers(M, C), col_buffers(M, HID), col_buffers(M, HID)
    nws = [int(lib.sv_linear_mxfp8_wgrad_workspace_floats(M, N, K, 0)) for N, K in ((C, HID), (HID, C))]
    ws = [torch.empty(max(n, 1), dtype=torch.float32, device=dev) for n in nws]

    def chain():
        quant_cols(dy, dbt, dbs, colsum=db2)
        quant_cols(h, ht, hs)
        call("sv_linear_mxfp8_wgrad", ptr(dbt), ptr(dbs), ptr(ht), ptr(hs), ptr(dw2), M, C, HID, HID, 0, ptr(ws[0]) if nws[0] else None)
        quant_cols(dh, dht, dhs, colsum=db1)
        quant_cols(ln, lnt, lns)
        call("sv_linear_mxfp8_wgrad", ptr(dht), ptr(dhs), ptr(lnt), ptr(lns), ptr(dw1), M, HID, C, C, 0, ptr(ws[1]) if nws[1] else None)

    for rep in range(REPEAT):
        a = timeit(lambda: call("sv_swin_mlp_wgrad", ptr(x), ptr(dy), ptr(lg), ptr(lb), ptr(w1r), ptr(w2tr), ptr(b1), ptr(sc), res * res, ptr(dw1), ptr(db1),
                                ptr(dw2), ptr(db2), M, C, 1e-5))
        b = float("nan")
        if lib.sv_swin_mlp_wgrad_mx_supported(C) == 1:
            b = timeit(lambda: call("sv_swin_mlp_wgrad_mx", ptr(x), ptr(dy), ptr(lg), ptr(lb), ptr(w1q), ptr(w1s), ptr(w2tq), ptr(w2ts), ptr(b1), ptr(sc),
                                    res * res, ptr(dw1), ptr(db1), ptr(dw2), ptr(db2), M, C, 1e-5))
        u = timeit(chain)                                  # the gradients accumulate from launch to launch: the values do not matter to the time
        print(f"C={C:3d} M={M:7d} run {rep}  (a) fused bf16 {a:6.3f} ms {4 * unit / a / 1e9:6.0f} TF/s | (b) fused MX {b:6.3f} ms {4 * unit / b / 1e9:6.0f} TF/s | "
              f"(c) unfused MX chain {u:6.3f} ms", flush=True)
    del x, dy, ln, h, dh, dbt, lnt, ht, dht, ws
