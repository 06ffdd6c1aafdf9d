#!/usr/bin/env python3
"""The MX quantising LayerNorm (csrc/norm.hip, sv_layernorm_quant_mx_fwd) against what it replaces, per site, at the bench's I = 512 images
(B = 64 x V = 8), bf16 storage: the token LayerNorms that feed an MXFP8 Swin linear (norm1 -> qkv, norm2 -> fc1, patch-merge norm ->
reduction).  The sites, the rotation of the buffers and the protocol are those of scripts/bench_ln_quant.py (the row recipe's form).

Per (M, C), in one process:
  (a) sv_layernorm_fwd                                  (b) sv_quant_rows_mx_e4m3 on its output
  (c) sv_layernorm_quant_mx_fwd                         (d) sv_layernorm_quant_mx_fwd with y = mean = rstd = NULL (no backward follows)
The yardstick is (a) + (b) of the same run.  2 warm-up launches, one HIP event pair per launch, median of --iters launches; the operands
rotate over up to 4 copies, >= 512 MB per rotation where 4 copies reach it (above L2 + MALL).
TB/s counts the bytes a pass must move: x once, plus what it writes ((b): y once, its second read is served from cache).

  python scripts/bench_ln_quant_mx.py [--iters 9] [--rows-div 1]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import swinvox_amd as S  # noqa: E402
from swinvox_amd import hip  # noqa: E402
from swinvox_amd.ops import call, ptr  # noqa: E402

I = 512
SITES = [  # name, M, C, merged
    ("T s1 norm", I * 784, 192, False), ("T s2 norm", I * 196, 384, False), ("T s3 norm", I * 49, 768, False),
    ("T merge 1", I * 784, 384, True), ("T merge 2", I * 196, 768, True), ("T merge 3", I * 49, 1536, True),
    ("B s2 norm", I * 196, 512, False)]


def median_us(fn, iters, warmup=2):
    for k in range(warmup):
        fn(k)
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for k, (e0, e1) in enumerate(evs):
        e0.record(); fn(k); e1.record()
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in evs) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--rows-div", type=int, default=1, help="divide the image count by this (quick runs: the working set then fits the caches)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    hip.load()
    S.set_math("bf16"); S.set_storage("bf16")
    imgs = I // a.rows_div
    print(f"{'site':10s} {'M':>7s} {'C':>5s} | {'(a) LN':>8s} {'(b) quant':>9s} {'(a)+(b)':>8s} {'(c) fused':>9s} {'(d) no y':>8s} | (c)/(a+b) (d)/(a+b) | TB/s (a) (b) (c) (d)")
    tot = [0.0, 0.0, 0.0, 0.0]
    for name, M, Cd, merged in SITES:
        M = M // I * imgs
        side = int(round((M // imgs) ** 0.5))                  # output map side; the merged form reads a [imgs, 2 side, 2 side, C / 4] map
        mh = 2 * side if merged else 0
        Kp = (Cd + 127) // 128 * 128
        R = max(1, min(4, -(-(512 << 20) // (4 * M * Cd))))    # rotating copies of (x, y): R * bytes(x + y) >= 512 MB, or 4 copies
        xs = [torch.randn(M, Cd, device=dev).bfloat16() for _ in range(R)]       # merged: the same bytes seen as the un-merged map
        ys = [torch.empty(M, Cd, device=dev, dtype=torch.bfloat16) for _ in range(R)]
        ms = [torch.empty(M, device=dev) for _ in range(R)]
        rs = [torch.empty(M, device=dev) for _ in range(R)]
        qs = [torch.empty(M, Kp, dtype=torch.uint8, device=dev) for _ in range(R)]
        ss = [torch.empty(M, Kp // 32, dtype=torch.uint8, device=dev) for _ in range(R)]
        g, b = 1.0 + 0.1 * torch.randn(Cd, device=dev), 0.1 * torch.randn(Cd, device=dev)

        def ln(k):
            j = k % R
            call("sv_layernorm_fwd", ptr(xs[j]), ptr(g), ptr(b), ptr(ys[j]), ptr(ms[j]), ptr(rs[j]), M, Cd, 1e-5, mh, mh)

        def quant(k):
            j = k % R
            call("sv_quant_rows_mx_e4m3", ptr(ys[j]), hip.BF16, M, Cd, Cd, ptr(qs[j]), Kp, ptr(ss[j]))

        def fused(k):
            j = k % R
            call("sv_layernorm_quant_mx_fwd", ptr(xs[j]), ptr(g), ptr(b), ptr(ys[j]), ptr(ms[j]), ptr(rs[j]), ptr(qs[j]), Kp, ptr(ss[j]), M, Cd, 1e-5, mh, mh)

        def fused_nostore(k):
            j = k % R
            call("sv_layernorm_quant_mx_fwd", ptr(xs[j]), ptr(g), ptr(b), None, None, None, ptr(qs[j]), Kp, ptr(ss[j]), M, Cd, 1e-5, mh, mh)

        for k in range(R):
            ln(k)                                              # (b) quantises real LayerNorm outputs
        ta, tb, tc, td = (median_us(f, a.iters) for f in (ln, quant, fused, fused_nostore))
        by = (4.0 * M * Cd + 8.0 * M, 2.0 * M * Cd + M * (Kp + Kp / 32.0), 4.0 * M * Cd + 8.0 * M + M * (Kp + Kp / 32.0), 2.0 * M * Cd + M * (Kp + Kp / 32.0))
        tbs = [n / t / 1e6 for n, t in zip(by, (ta, tb, tc, td))]
        for i, t in enumerate((ta, tb, tc, td)):
            tot[i] += t
        print(f"{name:10s} {M:7d} {Cd:5d} | {ta:8.1f} {tb:9.1f} {ta + tb:8.1f} {tc:9.1f} {td:8.1f} | {tc / (ta + tb):9.2f} {td / (ta + tb):9.2f} | "
              f"{tbs[0]:.2f} {tbs[1]:.2f} {tbs[2]:.2f} {tbs[3]:.2f}   (us; {R} cop{'y' if R == 1 else 'ies'})", flush=True)
        del xs, ys, ms, rs, qs, ss
        torch.cuda.empty_cache()
    ab = tot[0] + tot[1]
    print(f"TOTAL (a) {tot[0]:.1f} us, (b) {tot[1]:.1f} us, (a)+(b) {ab:.1f} us, (c) {tot[2]:.1f} us = {tot[2] / ab:.2f} x, (d) {tot[3]:.1f} us = {tot[3] / ab:.2f} x")


if __name__ == "__main__":
    main()
