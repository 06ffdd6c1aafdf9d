#!/usr/bin/env python3
"""MX form of the fp8 Swin linears (csrc/linear_fp8.hip, sv_linear_mxfp8) against the per-row recipe and the engine's bf16 forward, per
layer, and the producer emission against the stand-alone MX quantiser, per pair of layers.  Protocol of scripts/bench_linear_fp8.py: the
bench's I = 512 images, its ten shapes with the epilogue their call site uses, warm-up launches, one HIP event pair per measured unit, the
median of 9, operands rotating over up to 4 copies so that no launch finds its inputs cached.

Per layer: bf16 | row recipe, quantise + GEMM | MX, stand-alone quantise + GEMM (and the MX GEMM alone).
Per pair:  fc1 -> quantise h -> fc2  against  fc1 with emission -> fc2, in the training form (h and hpre stored) and the no_grad form (with
           emission neither is written); window attention -> quantise att -> proj  against  attention with emission -> proj, likewise.
The yardstick of an emitting pair is the stand-alone-quantiser pair of the same run.

  python scripts/bench_linear_mxfp8.py [--iters 9] [--rows-div 1] [--skip-layers] [--skip-pairs]"""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_linear_fp8 import SHAPES, I, median_us  # noqa: E402
import swinvox_amd as S  # noqa: E402
from swinvox_amd import hip, ops  # noqa: E402
from swinvox_amd.ops import ACT_GELU, ConvSpec, call, ptr  # noqa: E402

MLP_PAIRS = [("T s1", I * 784, 192), ("T s2", I * 196, 384), ("T s3", I * 49, 768), ("B s2", I * 196, 512)]      # name, M, C
ATT_PAIRS = [("T s1", 28, 192), ("T s2", 14, 384), ("T s3", 7, 768), ("B s1", 28, 256)]                        # name, H = W, C


def rup(k):
    return (k + 127) // 128 * 128


def copies(nbytes):
    return max(1, min(4, -(-(512 << 20) // nbytes)))


def epilogue_kw(epi, M, N, dev):
    kw = dict(bias=torch.randn(N, device=dev))
    if epi == "gelu":
        kw.update(act=ACT_GELU, pre_act=torch.empty(M, N, device=dev, dtype=torch.bfloat16))
    if epi == "resscale":
        kw.update(residual=torch.randn(M, N, device=dev).bfloat16(), ldr=N, row_scale=torch.rand(-(-M // 49), device=dev), rows_per_scale=49)
    return kw


def mx_buffers(M, K, dev, R):
    return ([torch.empty(M, rup(K), dtype=torch.uint8, device=dev) for _ in range(R)],
            [torch.empty(M, rup(K) // 32, dtype=torch.uint8, device=dev) for _ in range(R)])


def quant_mx(x, M, K, q, s):
    call("sv_quant_rows_mx_e4m3", ptr(x), hip.BF16, M, K, K, ptr(q), rup(K), ptr(s))


def gemm_mx(xq, xs, wq, ws, out, M, K, N, e, q_out=None, qs_out=None):
    call("sv_linear_mxfp8", ptr(xq), ptr(xs), ptr(wq), ptr(ws), ptr(out), M, K, N, C.byref(e), ptr(q_out), ptr(qs_out))


def layers(a, dev):
    print(f"{'layer':10s} {'M':>8s} {'K':>5s} {'N':>5s} {'epi':8s} | {'bf16':>8s} | {'row q+g':>8s} | {'mx quant':>8s} {'mx gemm':>8s} {'mx q+g':>8s} | mx/row  mx/bf16")
    tot = [0.0, 0.0, 0.0]
    for name, M, K, N, epi in SHAPES:
        M //= a.rows_div
        sp = ConvSpec.linear(K, N)
        R = copies(2 * M * (K + N))
        xs = [torch.randn(M, K, device=dev).bfloat16() for _ in range(R)]
        ys = [torch.empty(M, N, device=dev, dtype=torch.bfloat16) for _ in range(R)]
        w = torch.nn.Parameter(torch.randn(N, K, device=dev) / K ** 0.5, requires_grad=False)
        wp = sp.pack_fwd(w)
        kw = epilogue_kw(epi, M, N, dev)
        e = ops._epilogue(N, **kw)
        xq8 = [torch.empty(M, rup(K), dtype=torch.uint8, device=dev) for _ in range(R)]
        sx8 = [torch.empty(M, dtype=torch.float32, device=dev) for _ in range(R)]
        wq8, sw8 = ops.quantize_rows_fp8(w, N, K)
        xqm, xsm = mx_buffers(M, K, dev, R)
        wqm, wsm = ops.quantize_rows_mx(w, N, K, activation=False)

        def row(k):
            call("sv_quant_rows_e4m3", ptr(xs[k % R]), hip.BF16, M, K, K, ptr(xq8[k % R]), rup(K), ptr(sx8[k % R]))
            call("sv_linear_fp8", ptr(xq8[k % R]), ptr(sx8[k % R]), ptr(wq8), ptr(sw8), ptr(ys[k % R]), M, K, N, C.byref(e))

        def mxq(k):
            quant_mx(xs[k % R], M, K, xqm[k % R], xsm[k % R])

        def mxg(k):
            gemm_mx(xqm[k % R], xsm[k % R], wqm, wsm, ys[k % R], M, K, N, e)

        def mx(k):
            mxq(k); mxg(k)

        def bf16(k):
            sp.forward(xs[k % R], M, (1, 1, 1), wp, ys[k % R], **kw)

        for k in range(R):
            mxq(k)
        t16, trow, tq, tg, tmx = (median_us(f, a.iters) for f in (bf16, row, mxq, mxg, mx))
        tot[0] += t16; tot[1] += trow; tot[2] += tmx
        print(f"{name:10s} {M:8d} {K:5d} {N:5d} {epi:8s} | {t16:8.1f} | {trow:8.1f} | {tq:8.1f} {tg:8.1f} {tmx:8.1f} | {tmx / trow:6.2f} {tmx / t16:8.2f}   (us; "
              f"mx gemm {2.0 * M * K * N / tg / 1e6:.0f} TF/s)", flush=True)
        del xs, ys, xq8, sx8, xqm, xsm, kw, e
        torch.cuda.empty_cache()
    print(f"TOTAL bf16 {tot[0]:.1f} us, row recipe quantise + gemm {tot[1]:.1f} us, MX quantise + gemm {tot[2]:.1f} us")


def mlp_pairs(a, dev):
    print(f"\n{'fc1 -> fc2':10s} {'M':>8s} {'C':>5s} | training: {'stand-alone':>11s} {'emission':>9s}  ratio | no_grad: {'stand-alone':>11s} {'emission':>9s}  ratio   (us)")
    for name, M, Cd in MLP_PAIRS:
        M //= a.rows_div
        Hd = 4 * Cd
        R = copies(2 * M * (2 * Hd + 2 * Cd))
        xs = [torch.randn(M, Cd, device=dev).bfloat16() for _ in range(R)]
        h, hpre = torch.empty(M, Hd, device=dev, dtype=torch.bfloat16), torch.empty(M, Hd, device=dev, dtype=torch.bfloat16)   # written, then read at once
        ys = [torch.empty(M, Cd, device=dev, dtype=torch.bfloat16) for _ in range(R)]
        w1 = torch.randn(Hd, Cd, device=dev) / Cd ** 0.5
        w2 = torch.randn(Cd, Hd, device=dev) / Hd ** 0.5
        b1 = torch.randn(Hd, device=dev)
        kw2 = epilogue_kw("resscale", M, Cd, dev)
        e1, e1n, e2 = ops._epilogue(Hd, bias=b1, act=ACT_GELU, pre_act=hpre), ops._epilogue(Hd, bias=b1, act=ACT_GELU), ops._epilogue(Cd, **kw2)
        xq, xsc = mx_buffers(M, Cd, dev, R)
        hq, hs = mx_buffers(M, Hd, dev, 1)
        w1q, w1s = ops.quantize_rows_mx(w1, Hd, Cd, activation=False)
        w2q, w2s = ops.quantize_rows_mx(w2, Cd, Hd, activation=False)
        for k in range(R):
            quant_mx(xs[k], M, Cd, xq[k], xsc[k])

        def alone(k):          # both forms store h and hpre: without emission the quantiser has to read h
            gemm_mx(xq[k % R], xsc[k % R], w1q, w1s, h, M, Cd, Hd, e1)
            quant_mx(h, M, Hd, hq[0], hs[0])
            gemm_mx(hq[0], hs[0], w2q, w2s, ys[k % R], M, Hd, Cd, e2)

        def emit_train(k):
            gemm_mx(xq[k % R], xsc[k % R], w1q, w1s, h, M, Cd, Hd, e1, hq[0], hs[0])
            gemm_mx(hq[0], hs[0], w2q, w2s, ys[k % R], M, Hd, Cd, e2)

        def emit_nograd(k):
            gemm_mx(xq[k % R], xsc[k % R], w1q, w1s, None, M, Cd, Hd, e1n, hq[0], hs[0])
            gemm_mx(hq[0], hs[0], w2q, w2s, ys[k % R], M, Hd, Cd, e2)

        ta, tt, tn = (median_us(f, a.iters) for f in (alone, emit_train, emit_nograd))
        print(f"{name:10s} {M:8d} {Cd:5d} | {'':9s} {ta:11.1f} {tt:9.1f} {tt / ta:6.2f} | {'':8s} {ta:11.1f} {tn:9.1f} {tn / ta:6.2f}", flush=True)
        del xs, ys, h, hpre, hq, hs, xq, xsc, kw2
        torch.cuda.empty_cache()


def att_pairs(a, dev):
    print(f"\n{'att -> proj':10s} {'M':>8s} {'C':>5s} | training: {'stand-alone':>11s} {'emission':>9s}  ratio | no_grad: {'stand-alone':>11s} {'emission':>9s}  ratio   (us)")
    for name, H, Cd in ATT_PAIRS:
        Ii = max(1, I // a.rows_div)
        M, heads = Ii * H * H, Cd // 32
        R = copies(2 * M * 6 * Cd)
        qkvs = [torch.randn(M, 3 * Cd, device=dev).bfloat16() for _ in range(R)]
        table = 0.5 * torch.randn(169, heads, device=dev)
        att = torch.empty(M, Cd, device=dev, dtype=torch.bfloat16)
        ys = [torch.empty(M, Cd, device=dev, dtype=torch.bfloat16) for _ in range(R)]
        w = torch.randn(Cd, Cd, device=dev) / Cd ** 0.5
        kw = epilogue_kw("resscale", M, Cd, dev)
        e = ops._epilogue(Cd, **kw)
        aq, asc = mx_buffers(M, Cd, dev, 1)
        wq, ws = ops.quantize_rows_mx(w, Cd, Cd, activation=False)
        shift = 3 if H > 7 else 0

        def alone(k):
            call("sv_window_attention_fwd", ptr(qkvs[k % R]), ptr(table), ptr(att), Ii, H, H, Cd, heads, shift, hip.MATH_BF16)
            quant_mx(att, M, Cd, aq[0], asc[0])
            gemm_mx(aq[0], asc[0], wq, ws, ys[k % R], M, Cd, Cd, e)

        def emit(k, out=att):
            call("sv_window_attention_fwd_mxq", ptr(qkvs[k % R]), ptr(table), ptr(out), Ii, H, H, Cd, heads, shift, hip.MATH_BF16, ptr(aq[0]), rup(Cd), ptr(asc[0]))
            gemm_mx(aq[0], asc[0], wq, ws, ys[k % R], M, Cd, Cd, e)

        ta, tt, tn = (median_us(f, a.iters) for f in (alone, emit, lambda k: emit(k, None)))
        print(f"{name:10s} {M:8d} {Cd:5d} | {'':9s} {ta:11.1f} {tt:9.1f} {tt / ta:6.2f} | {'':8s} {ta:11.1f} {tn:9.1f} {tn / ta:6.2f}", flush=True)
        del qkvs, ys, att, aq, asc, kw
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--rows-div", type=int, default=1, help="divide every M by this (quick runs: the working set then fits the caches)")
    ap.add_argument("--skip-layers", action="store_true")
    ap.add_argument("--skip-pairs", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    hip.load()
    S.set_math("bf16"); S.set_storage("bf16")
    if not a.skip_layers:
        layers(a, dev)
    if not a.skip_pairs:
        mlp_pairs(a, dev)
        att_pairs(a, dev)


if __name__ == "__main__":
    main()
