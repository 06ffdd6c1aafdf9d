"""Whole optimisation step (harness.train_step: forward + backward + clip + solver) with the flat-buffer solvers and with
the stock torch.optim sequence, next to forward+backward alone.  python scripts/bench_train_step.py [--batch 32]
--fp8-linear: forward+backward alone with the fp8 Swin linears (set_linear_fp8) off and on, same process.
--fp8-linear-bwd: the same with a third run, set_linear_fp8(True, backward=True): data and weight gradients of the linears in e4m3 too.
--fp8-linear-mx: forward+backward alone, alternating (two rounds, one process) bf16, the row recipe, the MX recipe with producer emission and
the MX recipe with the stand-alone quantiser everywhere (set_mx_producer_quant(False)).
--fp8-linear-mx-bwd: forward+backward alone, alternating (two rounds, one process) bf16, the row-recipe forward + backward, the MX forward with
the row-recipe backward, and the MX forward with the MX backward (backward_recipe="mx").
--fp8-linear-mx-store: forward+backward alone, alternating (two rounds, one process) bf16, the MX forward + MX backward, and the same with the
inputs of the linears stored as MX rows (store="mx"); every line also reports torch.cuda.max_memory_allocated of its run.
--fp8-linear-mx-dual: forward+backward alone, alternating (two rounds, one process) bf16, the MX forward + MX backward with store="mx", and the
same with the MX dual quantiser (set_mx_dual_quant(True)); with the peak memory of every run."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import swinvox_amd as S  # noqa: E402
from swinvox_amd import harness, ops  # noqa: E402
from swinvox_amd.models import Decoder, Encoder, Merger, Refiner  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--views", type=int, default=8)
ap.add_argument("--steps", type=int, default=6)
ap.add_argument("--fp8-linear", action="store_true", help="time forward+backward only, with set_linear_fp8 off and on")
ap.add_argument("--fp8-linear-bwd", action="store_true", help="as --fp8-linear, plus a run with the fp8 backward of the linears")
ap.add_argument("--fp8-linear-mx", action="store_true", help="forward+backward only: bf16, row recipe, MX with and without producer emission, two rounds")
ap.add_argument("--fp8-linear-mx-bwd", action="store_true", help="forward+backward only: bf16, row fwd + bwd, MX fwd + row bwd, MX fwd + MX bwd, two rounds")
ap.add_argument("--fp8-linear-mx-store", action="store_true", help="forward+backward only: bf16, MX fwd + MX bwd, the same with store='mx', two rounds; with peak memory")
ap.add_argument("--fp8-linear-mx-dual", action="store_true", help="forward+backward only: bf16, MX fwd + MX bwd + store='mx', the same with the dual quantiser, two rounds; with peak memory")
a = ap.parse_args()
dev = torch.device("cuda:0")
cfg = S.default_cfg()
S.set_math("bf16")
S.set_storage("bf16")
x = (0.5 * torch.randn(a.batch, a.views, 3, 224, 224, device=dev)).clamp(-1, 1)
gt = (torch.rand(a.batch, 32, 32, 32, device=dev) < 0.1).float()


def timed(fn, n):
    fn()
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


MX_MODES = (None, "fp8", "mx", "mx-noemit")
MX_BWD_MODES = (None, "fp8+bwd", "mx+bwd", "mx+mxbwd")
MX_STORE_MODES = (None, "mx+mxbwd", "mx+mxbwd+store")
MX_DUAL_MODES = (None, "mx+mxbwd+store", "mx+mxbwd+store+dual")
for fused in (MX_DUAL_MODES * 2 if a.fp8_linear_mx_dual else MX_STORE_MODES * 2 if a.fp8_linear_mx_store else MX_BWD_MODES * 2 if a.fp8_linear_mx_bwd else MX_MODES * 2 if a.fp8_linear_mx else (None, "fp8", "fp8+bwd") if a.fp8_linear_bwd else (None, "fp8") if a.fp8_linear else (True, False, None)):
    torch.manual_seed(0)
    nets = [m(cfg).to(dev).train() for m in (Encoder, Decoder, Merger, Refiner)]
    dual = fused == "mx+mxbwd+store+dual"
    if dual:
        fused = "mx+mxbwd+store"
    fp8 = fused in ("fp8", "fp8+bwd", "mx", "mx-noemit", "mx+bwd", "mx+mxbwd", "mx+mxbwd+store")
    S.set_linear_fp8(fp8, backward=fused in ("fp8+bwd", "mx+bwd", "mx+mxbwd", "mx+mxbwd+store"),
                     recipe="mx" if fused in ("mx", "mx-noemit", "mx+bwd", "mx+mxbwd", "mx+mxbwd+store") else "row",
                     backward_recipe="mx" if fused in ("mx+mxbwd", "mx+mxbwd+store") else "row", store="mx" if fused == "mx+mxbwd+store" else "bf16")
    ops.set_mx_producer_quant(fused != "mx-noemit")
    ops.set_mx_dual_quant(dual)
    if fused is None or fp8:
        def step():
            for n in nets:
                n.zero_grad(set_to_none=True)
            harness.forward_losses(nets, cfg, x, gt)[0].backward()
        name = "forward+backward only" + {"fp8": ", fp8 Swin linears", "fp8+bwd": ", fp8 Swin linears fwd + bwd", "mx": ", MX Swin linears, emission",
                                          "mx-noemit": ", MX Swin linears, quantiser", "mx+bwd": ", MX Swin linears fwd + row-recipe bwd",
                                          "mx+mxbwd": ", MX Swin linears fwd + MX bwd",
                                          "mx+mxbwd+store": ", MX fwd + MX bwd, inputs stored as MX rows"}.get(fused, "") + (", dual quantiser" if dual else "")
    else:
        solvers, _ = harness.make_solvers(nets, cfg, fused=fused)
        def step():
            harness.train_step(nets, solvers, cfg, x, gt)
        name = "train_step, flat solvers" if fused else "train_step, torch.optim + clip_grad_norm_"
    torch.cuda.reset_peak_memory_stats()
    ms = timed(step, a.steps)
    peak = f"  peak {torch.cuda.max_memory_allocated() / 2 ** 20:9.1f} MiB" if a.fp8_linear_mx_store or a.fp8_linear_mx_dual else ""
    print(f"{name:45s} {ms:8.2f} ms/step  {a.batch * a.views / ms * 1e3:8.1f} views/s{peak}", flush=True)
    del nets
    torch.cuda.empty_cache()
