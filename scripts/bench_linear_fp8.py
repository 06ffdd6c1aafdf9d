#!/usr/bin/env python3
"""fp8 forward of the Swin linears (csrc/linear_fp8.hip) against the engine's bf16 forward of the same layer, per shape, at the bench's
I = 512 images (B = 64 x V = 8): ten distinct Swin-T / Swin-B linear shapes with the epilogue their call site uses.

Per shape, in one process: activation quantisation + sv_linear_fp8 (what a forward pays; the weight quantisation is once per layer and
forward and is timed apart), sv_linear_fp8 alone, and sv_conv_gather with bf16 operands.  Protocol: warm-up launches, one HIP event pair per
launch, median over the launches.  The operands (x, its quantised rows, the output) rotate over up to 4 copies; at the listed shapes the bytes one
rotation touches are 0.5 ... 1.2 GB (one copy alone where a single x + y pair is already > 512 MB), above L2 + MALL, so no launch finds its
inputs cached.  --rows-div shrinks the working set below that: its times are for smoke runs only and flatter the small shapes.

  python scripts/bench_linear_fp8.py [--iters 9] [--rows-div 1]
  python scripts/bench_linear_fp8.py --iou      # |dIoU| / |dlogit| of the whole pipeline against the golden vectors of case_B2_V8, bf16 and fp8-linear
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import swinvox_amd as S  # noqa: E402
from swinvox_amd import hip, ops  # noqa: E402
from swinvox_amd.ops import ACT_GELU, ConvSpec, call, ptr  # noqa: E402

I = 512
SHAPES = [  # name, M, K, N, epilogue
    ("T s1 fc1", I * 784, 192, 768, "gelu"), ("T s1 fc2", I * 784, 768, 192, "resscale"),
    ("T s2 qkv", I * 196, 384, 1152, "bias"), ("T s2 proj", I * 196, 384, 384, "resscale"),
    ("T s2 fc1", I * 196, 384, 1536, "gelu"), ("T s2 fc2", I * 196, 1536, 384, "resscale"),
    ("T s3 fc1", I * 49, 768, 3072, "gelu"), ("T s3 fc2", I * 49, 3072, 768, "resscale"),
    ("B s2 fc1", I * 196, 512, 2048, "gelu"), ("B s2 fc2", I * 196, 2048, 512, "resscale")]


def median_us(fn, iters, warmup=2):
    for k in range(warmup):
        fn(k)
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for k, (e0, e1) in enumerate(evs):
        e0.record(); fn(k); e1.record()
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in evs) * 1e3


def iou_report(dev):
    """Eval forward of the whole pipeline on the golden inputs of case_B2_V8 against the committed fp32 golden vectors, as bench.py's
    iou_delta_vs_oracle computes it, in bf16 mode and with the fp8 Swin linears.  Reported, not asserted."""
    import json
    import numpy as np
    from swinvox_amd.goldens import golden_case
    from swinvox_amd.harness import voxel_metrics
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gold = np.load(os.path.join(root, "tests", "golden", "case_B2_V8.npz"))
    seed = json.load(open(os.path.join(root, "tests", "golden", "manifest.json")))["cases"]["B2_V8"]["seed"]
    S.set_math("bf16"); S.set_storage("bf16")
    nets, x, gt = golden_case(dev, 2, 8, seed)
    ref = torch.from_numpy(gold["refined"]).to(dev)
    for mode in ("bf16", "fp8-linear", "fp8-linear, stage 0 unfused"):
        S.set_linear_fp8(mode != "bf16")
        ops.set_fused_attn_block(not mode.endswith("unfused")); ops.set_fused_mlp(not mode.endswith("unfused"))
        n0 = ops.linear_fp8_launches()
        with torch.no_grad():
            raw, vol = nets[1](nets[0](x))
            refined = nets[3](nets[2](raw, vol))
        iou, _ = voxel_metrics(refined, gt, S.default_cfg().TEST.VOXEL_THRESH)
        d = (refined - ref).abs()
        print(json.dumps({"mode": mode, "fp8_launches": ops.linear_fp8_launches() - n0, "max_abs_dIoU": float(np.abs(iou.cpu().numpy() - gold["iou"]).max()),
                          "max_abs_dlogit": float(d.max()), "mean_abs_dlogit": float(d.mean()), "logit_absmax": float(ref.abs().max())}), flush=True)
    S.set_linear_fp8(False); ops.set_fused_attn_block(True); ops.set_fused_mlp(True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iou", action="store_true", help="whole-pipeline |dIoU| against the golden vectors instead of the per-layer times")
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--rows-div", type=int, default=1, help="divide every M by this (quick runs)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    hip.load()
    if a.iou:
        return iou_report(dev)
    S.set_math("bf16"); S.set_storage("bf16")
    print(f"{'layer':10s} {'M':>8s} {'K':>5s} {'N':>5s} {'epi':8s} | {'quant x':>8s} {'fp8 gemm':>9s} {'q + gemm':>9s} {'bf16':>8s} | gemm/bf16  (q+gemm)/bf16 | quant W")
    tot = [0.0, 0.0, 0.0]
    for name, M, K, N, epi in SHAPES:
        M //= a.rows_div
        sp = ConvSpec.linear(K, N)
        R = max(1, min(4, -(-(512 << 20) // (2 * M * (K + N)))))           # rotating copies of (x, y): R * bytes(x + y) >= 512 MB, or 4 copies
        xs = [torch.randn(M, K, device=dev).bfloat16() for _ in range(R)]
        ys = [torch.empty(M, N, device=dev, dtype=torch.bfloat16) for _ in range(R)]
        w = torch.nn.Parameter(torch.randn(N, K, device=dev) / K ** 0.5, requires_grad=False)
        wp = sp.pack_fwd(w)
        kw = dict(bias=torch.randn(N, device=dev))
        if epi == "gelu":
            kw.update(act=ACT_GELU, pre_act=torch.empty(M, N, device=dev, dtype=torch.bfloat16))
        if epi == "resscale":
            kw.update(residual=torch.randn(M, N, device=dev).bfloat16(), ldr=N, row_scale=torch.rand(-(-M // 49), device=dev), rows_per_scale=49)
        e = ops._epilogue(N, **kw)
        assert hip.load().sv_linear_fp8_supported(K, N, C.byref(e), hip.MATH_BF16, hip.BF16) == 1
        Kp = (K + 127) // 128 * 128
        xqs = [torch.empty(M, Kp, dtype=torch.uint8, device=dev) for _ in range(R)]
        sxs = [torch.empty(M, dtype=torch.float32, device=dev) for _ in range(R)]
        wq, sw = ops.quantize_rows_fp8(w, N, K)

        def quant(k):
            call("sv_quant_rows_e4m3", ptr(xs[k % R]), hip.BF16, M, K, K, ptr(xqs[k % R]), Kp, ptr(sxs[k % R]))

        def gemm(k):
            call("sv_linear_fp8", ptr(xqs[k % R]), ptr(sxs[k % R]), ptr(wq), ptr(sw), ptr(ys[k % R]), M, K, N, C.byref(e))

        def both(k):
            quant(k); gemm(k)

        def bf16(k):
            sp.forward(xs[k % R], M, (1, 1, 1), wp, ys[k % R], **kw)

        for k in range(R):
            quant(k)
        tq, tg, tb, t16 = (median_us(f, a.iters) for f in (quant, gemm, both, bf16))
        twq = median_us(lambda k: ops.quantize_rows_fp8(w, N, K), a.iters)
        tot[0] += tg; tot[1] += tb; tot[2] += t16
        print(f"{name:10s} {M:8d} {K:5d} {N:5d} {epi:8s} | {tq:8.1f} {tg:9.1f} {tb:9.1f} {t16:8.1f} | {tg / t16:9.2f} {tb / t16:13.2f} | {twq:7.1f}   (us; "
              f"fp8 gemm {2.0 * M * K * N / tg / 1e6:.0f} TF/s, bf16 {2.0 * M * K * N / t16 / 1e6:.0f} TF/s)", flush=True)
        del xs, ys, xqs, sxs, kw, e
        torch.cuda.empty_cache()
    print(f"TOTAL fp8 gemm {tot[0]:.1f} us, quantise + gemm {tot[1]:.1f} us, bf16 {tot[2]:.1f} us")


if __name__ == "__main__":
    main()
