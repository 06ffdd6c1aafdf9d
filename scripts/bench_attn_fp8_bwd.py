#!/usr/bin/env python3
"""Cost of the fp8 window-attention backward (SV_MATH_FP8_FULL) against the bf16 backward (SV_MATH_BF16), bf16 storage:
  * event-timed sv_window_attention_bwd at the Swin-B stage shapes for --images images (56^2 C = 128 / 4 heads, 28^2 C = 256 / 8,
    14^2 C = 512 / 16, 7^2 C = 1024 / 32) and at Swin-T stage 0 (56^2 C = 96 / 3 heads), median of --iters launches;
  * a Swin-B encoder train step (forward + backward of a squared-mean loss, bf16 math + storage, --step-images images) with the fp8
    forward only (set_attention_fp8(True)) against fp8 forward + backward (set_attention_fp8(True, backward=True)), median of --steps.
Prints one line per kernel shape and one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import swinvox_amd as S  # noqa: E402
from swinvox_amd import hip  # noqa: E402
from swinvox_amd.hip import call, ptr  # noqa: E402


def events(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def kernels(dev, images, iters, warmup):
    res = []
    for name, H, heads in (("swin_b_s0", 56, 4), ("swin_b_s1", 28, 8), ("swin_b_s2", 14, 16), ("swin_b_s3", 7, 32), ("swin_t_s0", 56, 3)):
        C = heads * 32
        rows = images * H * H
        g = torch.Generator(device=dev).manual_seed(H + heads)
        qkv = torch.randn(rows, 3 * C, device=dev, generator=g).bfloat16()
        dout = torch.randn(rows, C, device=dev, generator=g).bfloat16()
        table = 0.5 * torch.randn(169, heads, device=dev, generator=g)
        dqkv = torch.empty_like(qkv)
        dt = torch.zeros(169, heads, device=dev)
        ws = torch.zeros(int(hip.load().sv_window_attention_bwd_workspace_floats(heads)), device=dev)
        for shift in ((0, 3) if H > 7 else (0,)):
            t = {}
            for label, m in (("bf16", hip.MATH_BF16), ("fp8_full", hip.MATH_FP8_FULL)):
                def run():
                    ws.zero_()
                    call("sv_window_attention_bwd", ptr(qkv), ptr(table), ptr(dout), ptr(dqkv), ptr(dt), ptr(ws), images, H, H, C, heads,
                         shift, m, act=hip.BF16)
                t[label] = events(run, iters, warmup) * 1e3
            r = dict(shape=name, H=H, C=C, heads=heads, shift=shift, bf16_us=round(t["bf16"], 1), fp8_full_us=round(t["fp8_full"], 1),
                     ratio=round(t["fp8_full"] / t["bf16"], 3))
            print(f"{name} H={H} C={C} heads={heads} shift={shift}: bf16 {t['bf16']:8.1f} us  fp8-full {t['fp8_full']:8.1f} us  "
                  f"(x{r['ratio']:.3f})", flush=True)
            res.append(r)
        del qkv, dout, dqkv
        torch.cuda.empty_cache()
    return res


def encoder_step(dev, images, steps, warmup):
    from swinvox_amd import goldens
    from swinvox_amd.models import Encoder
    enc = Encoder(S.default_cfg(), variant="base")
    goldens.seeded_fill_(enc, 0)
    enc.to(dev).train()
    enc.stochastic = False
    V = 8 if images % 8 == 0 else 1
    x = goldens.synth_images(images // V, V, 1).to(dev)
    out = {}
    for label, bwd in (("fp8_fwd", False), ("fp8_full", True)):
        S.set_attention_fp8(True, backward=bwd)

        def step():
            enc.zero_grad(set_to_none=True)
            enc(x).float().square().mean().backward()
        out[label] = events(step, steps, warmup)
        print(f"Swin-B encoder train step, {images} images, {label}: {out[label]:.2f} ms", flush=True)
    S.set_attention_fp8(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-images", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    hip.load()
    S.set_math("bf16")
    S.set_storage("bf16")
    res = dict(kernels=kernels(dev, args.images, args.iters, args.warmup))
    if not args.no_step:
        res["encoder_step_ms"] = {k: round(v, 3) for k, v in encoder_step(dev, args.step_images, args.steps, args.warmup).items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
