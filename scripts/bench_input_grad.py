#!/usr/bin/env python3
"""Cost of the gradient wrt the input renderings (Encoder backward with images.requires_grad), at the bench shape (B = 64 x V = 8, bf16):
  * the whole training step (Encoder -> Decoder -> Merger -> Refiner, both BCE losses, forward + backward) without and with image gradients,
    median of --steps event-timed steps after --warmup;
  * the stem's data gradient on the space-to-depth image (512 images, 112 x 112, 64 -> 16 channels): the halo-tile kind against the gather
    engine, and the adjoint of sv_encoder_prep;
  * --profile-step: only runs a few steps with image gradients (for `rocprofv3 --kernel-trace --stats -- python scripts/bench_input_grad.py
    --profile-step`, in a run of its own).
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import swinvox_amd as S  # noqa: E402
from swinvox_amd import hip, ops  # noqa: E402
from swinvox_amd.losses import bce_with_logits as bce  # noqa: E402
from swinvox_amd.models import Decoder, Encoder, Merger, Refiner  # noqa: E402
from swinvox_amd.ops import ConvSpec, call, ptr  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-step", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    hip.load()
    S.set_math("bf16")
    S.set_storage("bf16")
    torch.manual_seed(1234)
    cfg = S.default_cfg()
    nets = [Encoder(cfg), Decoder(cfg), Merger(cfg), Refiner(cfg)]
    for n in nets:
        n.to(dev).train()
    B, V = args.batch, args.views
    g = torch.Generator().manual_seed(0)
    images = (0.5 * torch.randn(B, V, 3, 224, 224, generator=g)).clamp(-1, 1).to(dev)
    gt = (torch.rand(B, 32, 32, 32, generator=g) < 0.10).float().to(dev)

    def step(img_grad):
        for n in nets:
            for p in n.parameters():
                p.grad = None
        x = images.detach().requires_grad_(img_grad)
        raw, vol = nets[1](nets[0](x))
        merged = nets[2](raw, vol)
        (bce(merged, gt) + bce(nets[3](merged), gt)).backward()

    if args.profile_step:
        for _ in range(args.warmup + 3):
            step(True)
        torch.cuda.synchronize()
        print(json.dumps({"profile_step": "done", "steps": args.warmup + 3}))
        return
    res = {"batch": B, "views": V, "storage": "bf16", "steps": args.steps, "warmup": args.warmup, "build": hip.kernel_source_hash()}
    res["step_ms_without_image_grad"] = events(lambda: step(False), args.steps, args.warmup)
    res["step_ms_with_image_grad"] = events(lambda: step(True), args.steps, args.warmup)
    res["step_ms_without_image_grad_again"] = events(lambda: step(False), args.steps, args.warmup)   # drift check

    # ---- the stem's data gradient alone (512 images)
    I = B * V
    sp = ConvSpec.conv2d(16, 64, 4, 1, 2, og_fixed=(1, 112, 112))
    w = torch.randn(64, 3, 7, 7, device=dev) / 12.0
    w16 = torch.empty(64, 16, 4, 4, device=dev)
    call("sv_stem_native", ptr(w), ptr(w16))
    pack = ops.pack_one(sp, w16, "d")
    dy = torch.randn(I * 112 * 112, 64, device=dev).bfloat16()
    dx16 = ops.empty(I * 112 * 112, 16, device=dev)
    mode0 = int(hip.load().sv_conv_halo_mode())
    for mode, key in ((2, "stem_dgrad_us_halo"), (0, "stem_dgrad_us_engine")):
        ops.set_conv_halo(mode)
        res[key] = 1e3 * events(lambda: sp.dgrad(dy, I, (1, 112, 112), pack, dx16), args.steps, args.warmup)
    ops.set_conv_halo(mode0)
    dxp = ops.empty(I * 56 * 56, 48, device=dev)
    dimg = torch.empty(I, 3, 224, 224, device=dev)
    res["encoder_prep_bwd_us"] = 1e3 * events(lambda: call("sv_encoder_prep_bwd", ptr(dx16), ptr(dxp), ptr(dimg), 1, I, 224), args.steps, args.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
