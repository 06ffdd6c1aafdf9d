#!/usr/bin/env python3
"""fp8 backward of the Swin linears (csrc/linear_fp8.hip) against the engine's bf16 data and weight gradient of the same layer, per shape,
at the bench's I = 512 images (B = 64 x V = 8): the ten shapes and the protocol of scripts/bench_linear_fp8.py.

Per shape, in one process: the row quantiser on dy, the column quantiser on dy (with the bias-gradient sums) and on x, sv_linear_fp8_dgrad
(fc2's call site with its GELU-derivative epilogue), sv_linear_fp8_wgrad, and sv_conv_gather / sv_conv_wgrad with bf16 operands on the same
data (the bf16 weight gradient includes its bias gradient).  The quantisation of W^T is once per layer and step and is timed apart.
Protocol: warm-up launches, one HIP event pair per launch, median over the launches; the operands rotate over up to 4 copies so that one
rotation touches >= 512 MB where memory allows (one copy where a single set is already larger).  --rows-div shrinks the working set below
that: its times are for smoke runs only.

  python scripts/bench_linear_fp8_bwd.py [--iters 9] [--rows-div 1]
"""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_linear_fp8 import SHAPES, median_us  # noqa: E402
import swinvox_amd as S  # noqa: E402
from swinvox_amd import hip, ops  # noqa: E402
from swinvox_amd.ops import ACT_GELU, ConvSpec, call, ptr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--rows-div", type=int, default=1, help="divide every M by this (quick runs)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    hip.load()
    S.set_math("bf16"); S.set_storage("bf16")
    print(f"{'layer':10s} {'M':>8s} {'K':>5s} {'N':>5s} | {'q rows dy':>9s} {'q cols dy':>9s} {'q cols x':>9s} | {'fp8 dgrad':>9s} {'bf16':>8s} {'gemm/bf16':>9s} "
          f"{'(q+g)/bf16':>10s} | {'fp8 wgrad':>9s} {'bf16':>8s} {'gemm/bf16':>9s} {'(q+g)/bf16':>10s} | quant W^T   (us)")
    tot = [0.0] * 6
    bf = torch.bfloat16
    for name, M, K, N, epi in SHAPES:
        M //= a.rows_div
        sp = ConvSpec.linear(K, N)
        R = max(1, min(4, -(-(512 << 20) // (2 * M * (K + N)))))           # rotating copies of (dy, x)
        Np, Mp = (N + 127) // 128 * 128, (M + 127) // 128 * 128
        dys = [torch.randn(M, N, device=dev).to(bf) for _ in range(R)]
        xs = [torch.randn(M, K, device=dev).to(bf) for _ in range(R)]
        dxs = [torch.empty(M, K, device=dev, dtype=bf) for _ in range(R)]
        w = torch.nn.Parameter(torch.randn(N, K, device=dev) / K ** 0.5, requires_grad=False)
        wd = sp.pack_dgrad(w)
        dw, db = torch.zeros(N, K, device=dev), torch.zeros(N, device=dev)
        kw = dict(act_grad_src=xs[0], act_grad_kind=ACT_GELU) if name.endswith("fc2") else {}   # fc2's data gradient runs through GELU'(hpre); x stands in
        e = ops._epilogue(K, **kw)
        assert hip.load().sv_linear_fp8_dgrad_supported(N, K, C.byref(e), hip.MATH_BF16, hip.BF16) == 1
        dqs = [torch.empty(M, Np, dtype=torch.uint8, device=dev) for _ in range(R)]
        sds = [torch.empty(M, dtype=torch.float32, device=dev) for _ in range(R)]
        dyts = [torch.empty(N, Mp, dtype=torch.uint8, device=dev) for _ in range(R)]
        xts = [torch.empty(K, Mp, dtype=torch.uint8, device=dev) for _ in range(R)]
        sdc, sxc = torch.empty(N, device=dev), torch.empty(K, device=dev)
        wtq, swt = ops.quantize_cols_fp8(w, N, K)

        def q_rows(k):
            call("sv_quant_rows_e4m3", ptr(dys[k % R]), hip.BF16, M, N, N, ptr(dqs[k % R]), Np, ptr(sds[k % R]))

        def q_cols_dy(k):
            call("sv_quant_cols_e4m3", ptr(dys[k % R]), hip.BF16, M, N, N, ptr(dyts[k % R]), Mp, ptr(sdc), ptr(db))

        def q_cols_x(k):
            call("sv_quant_cols_e4m3", ptr(xs[k % R]), hip.BF16, M, K, K, ptr(xts[k % R]), Mp, ptr(sxc), None)

        def dgrad8(k):
            call("sv_linear_fp8_dgrad", ptr(dqs[k % R]), ptr(sds[k % R]), ptr(wtq), ptr(swt), ptr(dxs[k % R]), M, N, K, C.byref(e))

        def wgrad8(k):
            call("sv_linear_fp8_wgrad", ptr(dyts[k % R]), ptr(sdc), ptr(xts[k % R]), ptr(sxc), ptr(dw), M, N, K, K, 0)

        def dgrad16(k):
            sp.dgrad(dys[k % R], M, (1, 1, 1), wd, dxs[k % R], **kw)

        def wgrad16(k):
            sp._wgrad(dys[k % R], xs[k % R], M, (1, 1, 1), dw, None, None, db)

        for k in range(R):
            q_rows(k); q_cols_dy(k); q_cols_x(k)
        tqr, tqd, tqx, td8, td16, tw8, tw16 = (median_us(f, a.iters) for f in (q_rows, q_cols_dy, q_cols_x, dgrad8, dgrad16, wgrad8, wgrad16))
        twt = median_us(lambda k: ops.quantize_cols_fp8(w, N, K), a.iters)
        for i, v in enumerate((td8, tqr + td8, td16, tw8, tqd + tqx + tw8, tw16)):
            tot[i] += v
        fl = 2.0 * M * K * N / 1e6
        print(f"{name:10s} {M:8d} {K:5d} {N:5d} | {tqr:9.1f} {tqd:9.1f} {tqx:9.1f} | {td8:9.1f} {td16:8.1f} {td8 / td16:9.2f} {(tqr + td8) / td16:10.2f} | "
              f"{tw8:9.1f} {tw16:8.1f} {tw8 / tw16:9.2f} {(tqd + tqx + tw8) / tw16:10.2f} | {twt:7.1f}   "
              f"(TF/s: dgrad fp8 {fl / td8:.0f} bf16 {fl / td16:.0f}, wgrad fp8 {fl / tw8:.0f} bf16 {fl / tw16:.0f})", flush=True)
        del dys, xs, dxs, dqs, sds, dyts, xts, kw, e
        torch.cuda.empty_cache()
    print(f"TOTAL dgrad: fp8 gemm {tot[0]:.1f} us, quantise + gemm {tot[1]:.1f} us, bf16 {tot[2]:.1f} us; "
          f"wgrad: fp8 gemm {tot[3]:.1f} us, quantise + gemm {tot[4]:.1f} us, bf16 {tot[5]:.1f} us")


if __name__ == "__main__":
    main()
