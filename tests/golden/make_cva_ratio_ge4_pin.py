#!/usr/bin/env python3
"""Pins the oracle's CrossViewAttention at cfg.NETWORK.ATT_SPATIAL_DOWNSAMPLE_RATIO 4 and 7 (depth-wise r x r / stride r conv 7x7 -> 1x1,
attention on one position per view, bilinear 1x1 -> 7x7 = broadcast: reference models/cross_view_attention.py:26-34,67-73,81-105,110-120)
against the reference module itself, imported read-only from the reference checkout: forward (eval and train) and every gradient,
for V in {1, 3} and (CROSS_ATT_REDUCTION_RATIO, CROSS_ATT_NUM_HEADS) in {(4, 4), (2, 2), (8, 8)}.  Also records that both modules
raise at ratio 8 (the kernel exceeds the 7x7 map).  Writes tests/golden/cva_ratio_ge4_pin.json; tests/test_cpu_cva_ratio_pin.py
checks every recorded difference is <= 1e-6.

  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cva_ratio_ge4_pin.py <path of the reference checkout>
"""
import importlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if len(sys.argv) != 2:
    sys.exit(__doc__)
REF = sys.argv[1]
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
import oracle as O  # noqa: E402

sys.path.insert(0, REF)
ref_mod = importlib.import_module("models.cross_view_attention")
torch.manual_seed(0)
pins = {}
for ratio in (4, 7):
    for red, heads in ((4, 4), (2, 2), (8, 8)):
        cfg = O.default_cfg()
        cfg.NETWORK.ATT_SPATIAL_DOWNSAMPLE_RATIO = ratio
        cfg.NETWORK.CROSS_ATT_REDUCTION_RATIO = red
        cfg.NETWORK.CROSS_ATT_NUM_HEADS = heads
        for V in (1, 3):
            o, r = O.CrossViewAttention(cfg, 512), ref_mod.CrossViewAttention(cfg, 512)
            O.seeded_weights_(o, seed=60 + ratio)
            r.load_state_dict(o.state_dict(), strict=True)
            g = torch.Generator().manual_seed(100 * ratio + 10 * red + V)
            x = torch.randn(2, V, 512, 7, 7, generator=g)
            for mode in ("eval", "train"):
                o.train(mode == "train"), r.train(mode == "train")
                for m in (o, r):
                    m.dropout.p = 0.0
                xo, xr = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
                yo, yr = o(xo), r(xr)
                worst = float((yo - yr).detach().abs().max())
                do = torch.randn(yo.shape, generator=g)
                o.zero_grad(), r.zero_grad()
                yo.backward(do), yr.backward(do)
                worst = max(worst, float((xo.grad - xr.grad).abs().max()))
                for (k, a), (_, b) in zip(o.named_parameters(), r.named_parameters()):
                    worst = max(worst, float((a.grad - b.grad).abs().max()))
                pins[f"cva_ds{ratio}_red{red}_h{heads}_V{V}_{mode}_fwd_bwd_maxdiff"] = worst
raises = {}
cfg = O.default_cfg()
cfg.NETWORK.ATT_SPATIAL_DOWNSAMPLE_RATIO = 8
for name, mod in (("oracle", O), ("reference", ref_mod)):
    try:
        mod.CrossViewAttention(cfg, 512)(torch.randn(1, 2, 512, 7, 7))
        raises[name] = False
    except RuntimeError:
        raises[name] = True
print(pins, raises)
with open(os.path.join(HERE, "cva_ratio_ge4_pin.json"), "w") as f:
    json.dump({"pins": pins, "ratio8_raises": raises}, f, indent=1)
    f.write("\n")
