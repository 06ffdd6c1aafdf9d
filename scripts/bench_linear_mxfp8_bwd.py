#!/usr/bin/env python3
"""MX backward of the Swin linears (csrc/linear_fp8.hip, backward_recipe="mx") against the row-recipe fp8 backward and the engine's bf16 data
and weight gradient of the same layer, per shape, at the bench's I = 512 images (B = 64 x V = 8): the ten shapes and the protocol of
scripts/bench_linear_fp8_bwd.py, all three measured in the same process.

Per shape: the MX row quantiser on dy, the one-launch MX column quantiser on dy (with the bias-gradient sums) and on x, sv_linear_mxfp8_dgrad
(fc2's call site with its GELU-derivative epilogue), sv_linear_mxfp8_wgrad with the default splits (the workspace is allocated once, outside
the timed region: the host layer takes it from the caching allocator); the same five for the row recipe, measured TWICE (rowA, rowB: their
spread is the yardstick a difference has to exceed); and sv_conv_gather / sv_conv_wgrad with bf16 operands.
"rb x" beside "MX qc x": the re-blocker (sv_mx_rows_to_cols) on the stored MX rows of x, what store="mx" runs in place of the column quantiser of x.
"dual dy" and "dual x": the dual quantiser (sv_quant_rows_cols_mx_e4m3) on dy - one launch for what "qr dy" + "qc dy" do in two - and its column-only
form on x, what set_mx_dual_quant(True) runs.  --sweep adds their table: qr dy + qc dy measured twice (A, B: the yardstick and its spread), the dual
quantiser against it, the column-only form against qc x, each with the achieved read + write TB/s.
--sweep: the MX weight-gradient GEMM at splits that give about 128, 256, 512, 1024 and 2048 workgroups (never more than one per 128 tokens), and
the re-blocker against its yardstick, the MX column quantiser on the bf16 tensor of the same shape, with the achieved read + write TB/s of both.
Protocol: warm-up launches, one HIP event pair per launch, median over the launches; the operands rotate over up to 4 copies so that one
rotation touches >= 512 MB where memory allows.  --rows-div shrinks the working set below that: its times are for smoke runs only.

  python scripts/bench_linear_mxfp8_bwd.py [--iters 9] [--rows-div 1] [--sweep]
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

TARGETS = (128, 256, 512, 1024, 2048)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--rows-div", type=int, default=1, help="divide every M by this (quick runs)")
    ap.add_argument("--sweep", action="store_true", help="also time the MX weight-gradient GEMM over the number of splits")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = hip.load()
    S.set_math("bf16"); S.set_storage("bf16")
    print("all times in us; q = quantisers, g = GEMM; dgrad q+g = row quantiser of dy + GEMM, wgrad q+g = both column quantisers + GEMM (+ reduce)")
    print(f"{'layer':10s} {'M':>8s} {'K':>5s} {'N':>5s} | {'MX qr dy':>8s} {'qc dy':>7s} {'qc x':>7s} {'rb x':>7s} {'dual dy':>7s} {'dual x':>7s} | {'row qr dy':>9s} {'qc dy':>7s} {'qc x':>7s} | "
          f"{'dgrad g MX':>10s} {'row':>7s} {'bf16':>7s} | {'dgrad q+g MX':>12s} {'rowA':>7s} {'rowB':>7s} {'bf16':>7s} | "
          f"{'wgrad g MX':>10s} {'splits':>6s} {'row':>7s} {'bf16':>7s} | {'wgrad q+g MX':>12s} {'rowA':>7s} {'rowB':>7s} {'bf16':>7s} | quant W^T MX / row")
    tot = {}
    sweep, rbs, duals = [], [], []
    bf = torch.bfloat16
    for name, M, K, N, epi in SHAPES:
        M //= a.rows_div
        sp = ConvSpec.linear(K, N)
        R = max(1, min(4, -(-(512 << 20) // (2 * M * (K + N)))))           # rotating copies of (dy, x)
        Np, Mp, Kp = (N + 127) // 128 * 128, (M + 127) // 128 * 128, (K + 127) // 128 * 128
        dys = [torch.randn(M, N, device=dev).to(bf) for _ in range(R)]
        xs = [torch.randn(M, K, device=dev).to(bf) for _ in range(R)]
        dxs = [torch.empty(M, K, device=dev, dtype=bf) for _ in range(R)]
        w = torch.nn.Parameter(torch.randn(N, K, device=dev) / K ** 0.5, requires_grad=False)
        wd = sp.pack_dgrad(w)
        dw, db = torch.zeros(N, K, device=dev), torch.zeros(N, device=dev)
        kw = dict(act_grad_src=xs[0], act_grad_kind=ACT_GELU) if name.endswith("fc2") else {}   # fc2's data gradient runs through GELU'(hpre); x stands in
        e = ops._epilogue(K, **kw)
        assert lib.sv_linear_fp8_dgrad_supported(N, K, C.byref(e), hip.MATH_BF16, hip.BF16) == 1
        u8 = dict(dtype=torch.uint8, device=dev)
        dqs = [torch.empty(M, Np, **u8) for _ in range(R)]
        dyts = [torch.empty(N, Mp, **u8) for _ in range(R)]
        xts = [torch.empty(K, Mp, **u8) for _ in range(R)]
        # row recipe: fp32 scales
        sds = [torch.empty(M, dtype=torch.float32, device=dev) for _ in range(R)]
        sdc, sxc = torch.empty(N, device=dev), torch.empty(K, device=dev)
        wtq, swt = ops.quantize_cols_fp8(w, N, K)
        # MX: E8M0 scale bytes
        dss = [torch.empty(M, Np // 32, **u8) for _ in range(R)]
        dyss = [torch.empty(N, Mp // 32, **u8) for _ in range(R)]
        xss = [torch.empty(K, Mp // 32, **u8) for _ in range(R)]
        wtqm, wtsm = ops.quantize_cols_mx(w, N, K)
        xrows = [ops.quantize_rows_mx(t_, M, K, activation=False) for t_ in xs]     # the MX rows of x a store="mx" tape holds
        nws = int(lib.sv_linear_mxfp8_wgrad_workspace_floats(M, N, K, 0))
        splits0 = nws // (N * K) if nws else 1
        ws = torch.empty(max(nws, 4), device=dev)

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

        def mq_rows(k):
            call("sv_quant_rows_mx_e4m3", ptr(dys[k % R]), hip.BF16, M, N, N, ptr(dqs[k % R]), Np, ptr(dss[k % R]))

        def mq_cols_dy(k):
            call("sv_quant_cols_mx_e4m3", ptr(dys[k % R]), hip.BF16, M, N, N, ptr(dyts[k % R]), Mp, ptr(dyss[k % R]), ptr(db))

        def mq_cols_x(k):
            call("sv_quant_cols_mx_e4m3", ptr(xs[k % R]), hip.BF16, M, K, K, ptr(xts[k % R]), Mp, ptr(xss[k % R]), None)

        def dual_dy(k):
            call("sv_quant_rows_cols_mx_e4m3", ptr(dys[k % R]), hip.BF16, M, N, N, ptr(dqs[k % R]), Np, ptr(dss[k % R]), ptr(dyts[k % R]), Mp, ptr(dyss[k % R]), ptr(db))

        def dual_x(k):
            call("sv_quant_rows_cols_mx_e4m3", ptr(xs[k % R]), hip.BF16, M, K, K, None, Kp, None, ptr(xts[k % R]), Mp, ptr(xss[k % R]), None)

        def rb_x(k):
            call("sv_mx_rows_to_cols", ptr(xrows[k % R][0]), Kp, ptr(xrows[k % R][1]), M, K, ptr(xts[k % R]), Mp, ptr(xss[k % R]))

        def mdgrad(k):
            call("sv_linear_mxfp8_dgrad", ptr(dqs[k % R]), ptr(dss[k % R]), ptr(wtqm), ptr(wtsm), ptr(dxs[k % R]), M, N, K, C.byref(e))

        def mwgrad(k, splits=0, wsp=None):
            call("sv_linear_mxfp8_wgrad", ptr(dyts[k % R]), ptr(dyss[k % R]), ptr(xts[k % R]), ptr(xss[k % R]), ptr(dw), M, N, K, K, splits, ptr(ws if wsp is None else wsp))

        def dgrad16(k):
            sp.dgrad(dys[k % R], M, (1, 1, 1), wd, dxs[k % R], **kw)

        def wgrad16(k):
            sp._wgrad(dys[k % R], xs[k % R], M, (1, 1, 1), dw, None, None, db)

        t = {}
        # the row recipe first (its operands are overwritten by the MX quantisers afterwards), twice: the spread between two runs of the same kernels
        for k in range(R):
            q_rows(k); q_cols_dy(k); q_cols_x(k)
        for run in ("A", "B"):
            for key, f in (("qr", q_rows), ("qd", q_cols_dy), ("qx", q_cols_x), ("dg", dgrad8), ("wg", wgrad8)):
                t[key + run] = median_us(f, a.iters)
        t["rwt"] = median_us(lambda k: ops.quantize_cols_fp8(w, N, K), a.iters)
        t["d16"], t["w16"] = median_us(dgrad16, a.iters), median_us(wgrad16, a.iters)
        for k in range(R):
            mq_rows(k); mq_cols_dy(k); mq_cols_x(k)
        for key, f in (("mqr", mq_rows), ("mqd", mq_cols_dy), ("mqx", mq_cols_x), ("mdg", mdgrad), ("mwg", mwgrad)):
            t[key] = median_us(f, a.iters)
        t["mwt"] = median_us(lambda k: ops.quantize_cols_mx(w, N, K), a.iters)
        t["ddy"], t["dx"] = median_us(dual_dy, a.iters), median_us(dual_x, a.iters)      # the same bytes as mq_rows + mq_cols_dy / mq_cols_x wrote
        if a.sweep:
            t["mqrB"], t["mqdB"] = median_us(mq_rows, a.iters), median_us(mq_cols_dy, a.iters)
            out_r, out_c = M * Np * 33 / 32, N * Mp * 33 / 32
            duals.append((name, M, N, K, t["mqr"], t["mqd"], t["mqrB"], t["mqdB"], t["ddy"], (4.0 * M * N + out_r + out_c) * 1e-6, (2.0 * M * N + out_r + out_c) * 1e-6,
                          t["mqx"], t["dx"], (2.0 * M * K + K * Mp * 33 / 32) * 1e-6))
        t["rbx"] = median_us(rb_x, a.iters)                                  # last: it overwrites the column operand of x with (nearly) the same bytes
        out_b = K * Mp * 33 / 32
        rbs.append((name, M, K, t["mqx"], (2.0 * M * K + out_b) / t["mqx"] * 1e-6, t["rbx"], (M * Kp * 33 / 32 + out_b) / t["rbx"] * 1e-6))
        dq = dict(mx=t["mqr"] + t["mdg"], rowA=t["qrA"] + t["dgA"], rowB=t["qrB"] + t["dgB"], bf16=t["d16"])
        wq = dict(mx=t["mqd"] + t["mqx"] + t["mwg"], rowA=t["qdA"] + t["qxA"] + t["wgA"], rowB=t["qdB"] + t["qxB"] + t["wgB"], bf16=t["w16"])
        for k, v in list(dq.items()) + [("w_" + k, v) for k, v in wq.items()]:
            tot[k] = tot.get(k, 0.0) + v
        print(f"{name:10s} {M:8d} {K:5d} {N:5d} | {t['mqr']:8.1f} {t['mqd']:7.1f} {t['mqx']:7.1f} {t['rbx']:7.1f} {t['ddy']:7.1f} {t['dx']:7.1f} | {t['qrA']:9.1f} {t['qdA']:7.1f} {t['qxA']:7.1f} | "
              f"{t['mdg']:10.1f} {t['dgA']:7.1f} {t['d16']:7.1f} | {dq['mx']:12.1f} {dq['rowA']:7.1f} {dq['rowB']:7.1f} {dq['bf16']:7.1f} | "
              f"{t['mwg']:10.1f} {splits0:6d} {t['wgA']:7.1f} {t['w16']:7.1f} | {wq['mx']:12.1f} {wq['rowA']:7.1f} {wq['rowB']:7.1f} {wq['bf16']:7.1f} | "
              f"{t['mwt']:.1f} / {t['rwt']:.1f}", flush=True)
        if a.sweep:
            tiles, nk = -(-N // 128) * -(-K // 128), Mp // 128
            row = []
            for target in TARGETS:
                s_ = max(1, min(nk, -(-target // tiles)))
                n = int(lib.sv_linear_mxfp8_wgrad_workspace_floats(M, N, K, s_))
                wsp = torch.empty(max(n, 4), device=dev)
                row.append((s_, median_us(lambda k: mwgrad(k, s_, wsp), a.iters), n * 4 / 2 ** 20))
                del wsp
            sweep.append((name, row))
        del dys, xs, dxs, dqs, sds, dyts, xts, dss, dyss, xss, xrows, ws, kw, e
        torch.cuda.empty_cache()
    print("TOTAL dgrad quantise + gemm: " + ", ".join(f"{k} {tot[k]:.1f}" for k in ("mx", "rowA", "rowB", "bf16")) +
          "; wgrad quantise + gemm: " + ", ".join(f"{k} {tot['w_' + k]:.1f}" for k in ("mx", "rowA", "rowB", "bf16")))
    if sweep:
        print("column operand of x: MX column quantiser on bf16 x (reads 2 bytes, writes 1 per element) against the re-blocker on the MX rows of x "
              "(reads 1, writes 1); TB/s = bytes read + written, scale bytes included")
        for name, M, K, tq, bq, tr, br in rbs:
            print(f"{name:10s} {M:8d} {K:5d} | qc x {tq:8.1f} us {bq:5.2f} TB/s | rb x {tr:8.1f} us {br:5.2f} TB/s | rb / qc {tr / tq:5.2f}", flush=True)
        print("operands of dy: MX row quantiser + MX column quantiser (two launches, dy read twice; A and B = two measurements) against the dual quantiser "
              "(one launch, dy read once); column operand of x: MX column quantiser against the dual quantiser's column-only form; TB/s = bytes read + "
              "written, scale bytes included")
        for name, M, N, K, qrA, qcA, qrB, qcB, dd, b2, b1, qx, dx_, bx in duals:
            A, B = qrA + qcA, qrB + qcB
            print(f"{name:10s} {M:8d} {N:5d} {K:5d} | qr + qc dy A {A:8.1f} ({qrA:.1f} + {qcA:.1f}) B {B:8.1f} us {b2 / min(A, B):5.2f} TB/s | dual dy {dd:8.1f} us "
                  f"{b1 / dd:5.2f} TB/s | dual / min(A, B) {dd / min(A, B):5.2f}, A/B spread {abs(A - B) / min(A, B):5.3f} | qc x {qx:8.1f} us {bx / qx:5.2f} TB/s | "
                  f"dual x {dx_:8.1f} us {bx / dx_:5.2f} TB/s | dual x / qc x {dx_ / qx:5.2f}", flush=True)
        print("TOTAL qr + qc dy: A %.1f B %.1f, dual dy %.1f; qc x %.1f, dual x %.1f" % (
            sum(d[4] + d[5] for d in duals), sum(d[6] + d[7] for d in duals), sum(d[8] for d in duals), sum(d[11] for d in duals), sum(d[12] for d in duals)))
        print("MX weight-gradient GEMM (+ reduce) over the splits: target workgroups -> splits, us, workspace MB")
        for name, row in sweep:
            print(f"{name:10s} " + " | ".join(f"{tg:4d} -> {s_:4d} {us:7.1f} us {mb:6.1f} MB" for tg, (s_, us, mb) in zip(TARGETS, row)), flush=True)


if __name__ == "__main__":
    main()
